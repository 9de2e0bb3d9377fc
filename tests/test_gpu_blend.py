"""Seamless mosaics on device tensors (papteam_opticalflow_amd/tensors.py: mosaic with gains and mode "feather",
mosaic_overlap, exposure_gains, panorama(exposure=True) -> papof_mosaic_blend_tensor, papof_mosaic_overlap_tensor).  The
blend's output must be the BYTES of the numpy restatement (tests/_blend_ref.py) under tests/test_gpu_mosaic.py's rule for NaNs
that arithmetic makes, on that module's frame and canvas pairs: every frame dtype, 1 .. 4 channels, both layouts, every
output dtype, the four modes with float32 and float64 gains, a broadcast, a NaN and an infinite gain, without gains against
mosaic's own bytes, the source counts at which the median changes instance and 255 for "feather", with and without masks and
the count, empty slots, NaN and infinite matrix entries, strided and expanded views.  The overlap statistics must be the
restatement's INTEGERS at the source counts at which the kernel changes instance, steps up to beyond the canvas, several
outputs, masks, NaN frames, values beyond the bound, into buffers that held garbage, twice the same.  Then the pipeline
against the same composition of public calls, the inputs left unchanged and the caller's stream order."""
import ctypes
import math

import numpy as np
import pytest

from _blend_ref import MODES, blend_reference, gains_reference, overlap_reference
from _interp_ref import convert
from test_gpu_batch import _video
from test_gpu_mosaic import PAIRS, _frame_masks, _mats, _nhwc, _same, _sources
from test_gpu_refine import _NP, _as_layout, _guide

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _gains(rng, n_out, N, dtype=np.float64):
    return np.exp(rng.uniform(math.log(0.6), math.log(1.5), (n_out, N))).astype(dtype)


def _blend_call(t, src, tm, size, mode, gains=None, masks=None, count=True, out_dtype=None):
    """papof_mosaic_blend_tensor itself on NHWC frames, whatever the mode and the gains (tensors.mosaic goes to
    papof_mosaic_tensor for the old modes without gains)"""
    from papteam_opticalflow_amd import tensors
    ts, descs, _, _ = tensors._check([("frames", t)], "NHWC", None, 1)
    (T, H, W, C), strides, code = descs[0]
    n_out, N = src.shape
    out, d_out = tensors._new_frames(n_out, size[0], size[1], C, "NHWC", out_dtype or t.dtype, t.device)
    cnt = torch.empty((n_out,) + tuple(size), dtype=torch.uint8, device=t.device) if count else None
    d_in = tensors._struct(ts[0], strides, code)
    d_mat = tensors._struct(tm, tuple(tm.stride()), tensors.capi.DTYPE_F64)
    d_mask = tensors._mask_struct(masks) if masks is not None else None
    d_cnt = tensors._mask_struct(cnt) if count else None
    d_gain = None if gains is None else tensors._struct(gains, (gains.stride(0), gains.stride(1), 0, 0), tensors.capi.DTYPE_F64)
    s32 = torch.from_numpy(np.asarray(src)).to(torch.int32).cuda()
    tensors._launch(t.device, "papof_mosaic_blend_tensor", T, H, W, C, ctypes.byref(d_in), tensors._ref(d_mask), n_out, N, size[0],
                    size[1], ctypes.c_void_p(s32.data_ptr()), ctypes.byref(d_mat), tensors._ref(d_gain), tensors.MOSAIC_MODES[mode],
                    ctypes.byref(d_out), tensors._ref(d_cnt))
    return out, cnt


# ---- the blend
@pytest.mark.parametrize("frame,canvas", PAIRS)
def test_every_dtype_channel_count_layout_and_output(frame, canvas):
    from papteam_opticalflow_amd.tensors import mosaic
    (H, W), (Hc, Wc) = frame, canvas
    T, n_out, N = 4, 2, 5
    rng = np.random.default_rng(H * 1000 + W + 7)
    runs, seen = 0, set()
    for dtype in (torch.uint8, torch.float32, torch.float64):
        for C in (1, 2, 3, 4):
            frames = _guide(T, H, W, C, dtype, 3 + C)
            M = _mats(rng, n_out, N, H, W, Hc, Wc)
            src = _sources(rng, n_out, N, T)
            masks = _frame_masks(rng, T, H, W) if C % 2 else None
            g = _gains(rng, n_out, N, np.float32 if C > 2 else np.float64)
            tm = torch.from_numpy(M).to(torch.float32 if C == 2 else torch.float64).cuda()
            t_masks = None if masks is None else torch.from_numpy(masks).cuda()
            tg = torch.from_numpy(g).cuda()
            for mode in MODES:
                want64, wcnt = blend_reference(frames, src, tm.cpu().numpy(), (Hc, Wc), mode, g, masks)
                seen |= set(np.unique(wcnt).tolist())
                for layout in ("NCHW", "NHWC"):
                    t = _as_layout(frames, layout)
                    for odt in (None, torch.uint8, torch.float32, torch.float64):
                        got = mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=t_masks, layout=layout, out_dtype=odt, gains=tg)
                        what = "%s frames %s C %d %s %s out %s" % (frame, dtype, C, mode, layout, odt)
                        assert got.out.shape == ((n_out, C, Hc, Wc) if layout == "NCHW" else (n_out, Hc, Wc, C)), what
                        _same(_nhwc(got.out, layout), convert(want64, _NP[odt or dtype]), what)
                        _same(got.count, wcnt, what + " count")
                        runs += 1
    assert runs == 3 * 4 * 4 * 2 * 4
    assert Hc * Wc < 100 or (0 in seen and max(seen) >= 2), seen


@pytest.mark.parametrize("mode", MODES)
def test_gains_of_both_dtypes_broadcast_nan_and_infinite(mode):
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, C, n_out, N, Hc, Wc = 5, 37, 53, 3, 2, 7, 40, 70
    rng = np.random.default_rng(31)
    frames = _guide(T, H, W, C, torch.float32, 4)
    t = torch.from_numpy(frames).cuda()
    M = _mats(rng, n_out, N, H, W, Hc, Wc)
    M[:, 1] = np.eye(2, 3)                                    # slots that are live over the frame's part of the canvas
    M[:, 5] = [[0.9, 0.0, 1.5], [0.0, 0.9, 0.5]]
    tm = torch.from_numpy(M).cuda()
    src = _sources(rng, n_out, N, T)
    src[:, 1], src[:, 5] = 2, 3
    most = 0
    for name in ("float64", "float32", "row", "column", "one", "nan", "inf", "none"):
        g = _gains(rng, n_out, N)
        if name == "float32":
            g = g.astype(np.float32)
        tg = torch.from_numpy(g).cuda()
        if name == "row":                                     # one row of gains for every output: stride 0 along o
            tg = tg[:1].expand(n_out, N)
        elif name == "column":
            tg = tg[:, :1].expand(n_out, N)
        elif name == "one":
            tg = tg[0, 0].expand(n_out, N)
        elif name == "nan":
            g[0, 1], g[1, 5] = math.nan, math.nan
            tg = torch.from_numpy(g).cuda()
        elif name == "inf":
            g[0, 1], g[1, 5] = math.inf, -math.inf
            tg = torch.from_numpy(g).cuda()
        elif name == "none":
            tg = None
        if name in ("row", "column", "one"):
            assert 0 in tg.stride()
        gn = None if tg is None else tg.cpu().numpy()
        for odt in (torch.float64, torch.uint8):
            want, wcnt = blend_reference(frames, src, M, (Hc, Wc), mode, gn, None, _NP[odt])
            if tg is None and mode != "feather":
                out, cnt = _blend_call(t, src, tm, (Hc, Wc), mode, None, out_dtype=odt)
            else:
                out, cnt = mosaic(t, src, tm, (Hc, Wc), mode=mode, layout="NHWC", out_dtype=odt, gains=tg)
            _same(out, want, "gains %s %s out %s" % (name, mode, odt))
            _same(cnt, wcnt, "gains %s count" % name)
            most = max(most, int(wcnt.max()))
        if name in ("nan", "inf") and mode in ("mean", "feather"):
            assert not np.isfinite(blend_reference(frames, src, M, (Hc, Wc), mode, gn)[0]).all()
    assert most >= 2


def test_without_gains_the_old_modes_are_mosaics_bytes():
    """papof_mosaic_blend_tensor with gains NULL, and with gains of 1.0 (through the multiplication), against
    papof_mosaic_tensor on the same inputs: float frames with NaNs and infinities among them"""
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, N, n_out, Hc, Wc = 6, 37, 53, 9, 2, 40, 70
    rng = np.random.default_rng(32)
    for dtype in (torch.uint8, torch.float64):
        frames = _guide(T, H, W, 3, dtype, 5)
        if dtype == torch.float64:
            salt = rng.random(frames.shape) < 0.05
            frames[salt] = rng.choice([math.nan, math.inf, -math.inf, -0.0, 5e-324], int(salt.sum()))
        t = torch.from_numpy(frames).cuda()
        M = _mats(rng, n_out, N, H, W, Hc, Wc)
        tm = torch.from_numpy(M).cuda()
        src = _sources(rng, n_out, N, T)
        mk = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda()
        ones = torch.ones(n_out, N, dtype=torch.float64).cuda()
        for mode in ("first", "mean", "median"):
            for masks in (None, mk):
                base = mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=masks, layout="NHWC")
                iv = torch.uint8 if dtype == torch.uint8 else torch.int64
                for g in (None, ones):
                    out, cnt = _blend_call(t, src, tm, (Hc, Wc), mode, g, masks)
                    assert torch.equal(out.view(iv), base.out.view(iv)) and torch.equal(cnt, base.count), (dtype, mode, g is None)
                got = mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=masks, layout="NHWC", gains=ones[:1, :1].expand(n_out, N))
                assert torch.equal(got.out.view(iv), base.out.view(iv)) and torch.equal(got.count, base.count)


@pytest.mark.parametrize("N", [1, 8, 9, 16, 17, 32, 33, 64, 255])
def test_source_counts_with_and_without_masks_and_count(N):
    """the median with gains at the counts at which it changes instance; "feather" and "mean" at each and at 255"""
    from papteam_opticalflow_amd import tensors
    T, H, W, n_out = 6, 37, 53, 2
    rng = np.random.default_rng(100 + N)
    most = 0
    for dtype, C, (Hc, Wc) in [(torch.uint8, 3, (40, 70)), (torch.float64, 1, (3, 130))]:
        frames = _guide(T, H, W, C, dtype, N + C)
        t = torch.from_numpy(frames).cuda()
        M = _mats(rng, n_out, N, H, W, Hc, Wc)
        src = _sources(rng, n_out, N, T)
        src[0, N // 2] = src[0, 0]
        masks = _frame_masks(rng, T, H, W)
        g = _gains(rng, n_out, N)
        tm, t_masks, tg = torch.from_numpy(M).cuda(), torch.from_numpy(masks).cuda().bool(), torch.from_numpy(g).cuda()
        for mode in ("median", "feather", "mean") if N != 255 else ("feather", "first", "median"):
            if mode == "median" and N > 64:
                with pytest.raises(ValueError):
                    tensors.mosaic(t, src, tm, (Hc, Wc), mode=mode, layout="NHWC", gains=tg)
                continue
            for mk, tmk in ((None, None), (masks, t_masks)):
                want, wcnt = blend_reference(frames, src, M, (Hc, Wc), mode, g, mk, _NP[dtype])
                got = tensors.mosaic(t, torch.from_numpy(src).cuda(), tm, (Hc, Wc), mode=mode, masks=tmk, layout="NHWC", gains=tg)
                what = "N %d %s C %d %s masks %s" % (N, dtype, C, mode, mk is not None)
                _same(got.out, want, what)
                _same(got.count, wcnt, what + " count")
                most = max(most, int(wcnt.max()))
                out, none = _blend_call(t, src, tm, (Hc, Wc), mode, tg, None if tmk is None else tmk.view(torch.uint8), count=False)
                assert none is None
                _same(out, want, what + " no count")
    assert most >= (2 if N >= 8 else 1), most


def test_strided_and_expanded_views():
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, N, n_out, Hc, Wc = 3, 29, 41, 4, 2, 33, 80
    rng = np.random.default_rng(36)
    big = torch.from_numpy(_guide(2 * T, H + 3, 2 * W, 4, torch.uint8, 8)).cuda()
    f = big[::2, 2:H + 2, ::2, 1:]
    bm = torch.from_numpy(np.repeat(_frame_masks(rng, T, H, W), 2, axis=2)).cuda()
    mk = bm[:, :, ::2]
    M = _mats(rng, n_out, N, H, W, Hc, Wc)
    tm = torch.from_numpy(np.repeat(M, 2, axis=1)).cuda()[:, ::2]
    g = _gains(rng, n_out, N, np.float32)
    tg = torch.from_numpy(np.repeat(g, 3, axis=1)).cuda()[:, ::3]
    assert not f.is_contiguous() and not mk.is_contiguous() and not tm.is_contiguous() and not tg.is_contiguous()
    src = _sources(rng, n_out, N, T)
    for mode in MODES:
        want, wcnt = blend_reference(f.cpu().numpy(), src, M, (Hc, Wc), mode, g, mk.cpu().numpy(), np.float32)
        got = mosaic(f, src, tm, (Hc, Wc), mode=mode, masks=mk, layout="NHWC", out_dtype=torch.float32, gains=tg)
        _same(got.out, want, "strided " + mode)
        _same(got.count, wcnt, "strided count " + mode)
    # one frame, one mask, one matrix and one gain seen many times (stride 0)
    one = torch.from_numpy(_guide(1, H, W, 2, torch.float32, 10)).cuda()
    m1 = torch.from_numpy(_frame_masks(rng, 1, H, W)).cuda()
    M1 = np.array([[[[0.5, 0.1, 2.0], [-0.1, 0.5, 6.0]]]])
    want, wcnt = blend_reference(np.repeat(one.cpu().numpy(), T, 0), None, np.repeat(np.repeat(M1, T, 1), n_out, 0), (Hc, Wc),
                                 "feather", np.full((n_out, T), 1.25), np.repeat(m1.cpu().numpy(), T, 0))
    got = mosaic(one.expand(T, H, W, 2), None, torch.from_numpy(M1).cuda().expand(n_out, T, 2, 3), (Hc, Wc), mode="feather",
                 masks=m1.expand(T, H, W), layout="NHWC", out_dtype=torch.float64,
                 gains=torch.tensor(1.25, dtype=torch.float64).cuda().expand(n_out, T))
    _same(got.out, want, "expanded")
    _same(got.count, wcnt, "expanded count")
    assert set(np.unique(wcnt).tolist()) == {0, T}


# ---- the overlap statistics
def _overlap_raw(t, src, tm, size, step, bound, masks=None, fill=None):
    """papof_mosaic_overlap_tensor into buffers of the test's own: fill None, or the int64 both hold before the call"""
    from papteam_opticalflow_amd import tensors
    ts, descs, _, _ = tensors._check([("frames", t)], "NHWC", None, 1)
    (T, H, W, C), strides, code = descs[0]
    n_out, N = src.shape
    sums = torch.full((n_out, N, N), fill, dtype=torch.int64).cuda()
    counts = torch.full((n_out, N, N), fill ^ 0x5555, dtype=torch.int64).cuda()
    d_in = tensors._struct(ts[0], strides, code)
    d_mat = tensors._struct(tm, tuple(tm.stride()), tensors.capi.DTYPE_F64)
    d_mask = tensors._mask_struct(masks) if masks is not None else None
    s32 = torch.from_numpy(np.asarray(src)).to(torch.int32).cuda()
    tensors._launch(t.device, "papof_mosaic_overlap_tensor", T, H, W, C, ctypes.byref(d_in), tensors._ref(d_mask), n_out, N, size[0],
                    size[1], ctypes.c_void_p(s32.data_ptr()), ctypes.byref(d_mat), step, ctypes.c_double(bound),
                    ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(counts.data_ptr()))
    return sums, counts


def _equal_ints(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == np.int64 and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    bad = g != want
    assert not bad.any(), "%s: %d of %d differ; first at %s: %d against %d" % (
        what, int(bad.sum()), bad.size, tuple(int(k[0]) for k in np.nonzero(bad)), g[bad][0], want[bad][0])


@pytest.mark.parametrize("N", [1, 2, 9, 17, 33, 64])
def test_overlap_is_the_restatement_integer_for_integer(N):
    from papteam_opticalflow_amd.tensors import mosaic_overlap
    T, H, W, n_out = 6, 37, 53, 3
    rng = np.random.default_rng(200 + N)
    pairs = 0
    for dtype, C, (Hc, Wc), bound in [(torch.uint8, 3, (40, 70), 1.0), (torch.float32, 2, (3, 130), 4.0), (torch.float64, 1, (70, 9), 0.5)]:
        frames = _guide(T, H, W, C, dtype, N + C)
        if dtype != torch.uint8:                              # NaNs, infinities, values beyond the bound and below zero
            frames = frames * 6.0 - 1.0
            salt = rng.random(frames.shape) < 0.02
            frames[salt] = rng.choice([math.nan, math.inf, -math.inf, 100.0], int(salt.sum())).astype(frames.dtype)
        t = torch.from_numpy(frames).cuda()
        M = _mats(rng, n_out, N, H, W, Hc, Wc)
        src = _sources(rng, n_out, N, T)
        masks = _frame_masks(rng, T, H, W)
        tm, t_masks = torch.from_numpy(M).cuda(), torch.from_numpy(masks).cuda()
        for step in (1, 2, 3, 7, 131):
            for mk, tmk in ((None, None), (masks, t_masks)) if step < 7 else ((None, None),):
                ws, wc = overlap_reference(frames, src, M, (Hc, Wc), step, bound, mk)
                got = mosaic_overlap(t, src, tm, (Hc, Wc), masks=tmk, step=step, bound=bound, layout="NHWC")
                what = "N %d %s canvas %s step %d masks %s" % (N, dtype, (Hc, Wc), step, mk is not None)
                assert got.bound == bound
                _equal_ints(got.sums, ws, what + " sums")
                _equal_ints(got.counts, wc, what + " counts")
                if step == 2:                                 # into buffers full of garbage, twice
                    for fill in (-1, 0x0123456789abcdef):
                        s, c = _overlap_raw(t, src, tm, (Hc, Wc), step, bound, tmk, fill)
                        _equal_ints(s, ws, what + " prefilled sums")
                        _equal_ints(c, wc, what + " prefilled counts")
                if step == 1:
                    off = wc * (1 - np.eye(N, dtype=np.int64))
                    pairs = max(pairs, int((off > 0).sum()))
                    assert (wc == wc.transpose(0, 2, 1)).all()
    assert N == 1 or pairs > 0


@pytest.mark.parametrize("frame,canvas", PAIRS)
def test_overlap_on_every_frame_and_canvas_pair(frame, canvas):
    """frames of one row, one column and 5 x 4 (W - 1 or H - 1 = 0, taps that collapse) and a canvas of one pixel: the
    kernel's culling and liveness test against the restatement, at step 1 and 2, with and without
    masks, every frame dtype, 1 .. 4 channels, both layouts"""
    from papteam_opticalflow_amd.tensors import mosaic_overlap
    (H, W), (Hc, Wc) = frame, canvas
    T, n_out = 4, 2
    rng = np.random.default_rng(H * 1000 + W + 11)
    runs, live, pairs = 0, 0, 0
    for dtype in (torch.uint8, torch.float32, torch.float64):
        for C, N in ((1, 5), (2, 9), (3, 5), (4, 17)):
            frames = _guide(T, H, W, C, dtype, 5 + C)
            M = _mats(rng, n_out, N, H, W, Hc, Wc)
            src = _sources(rng, n_out, N, T)
            masks = _frame_masks(rng, T, H, W)
            tm = torch.from_numpy(M).to(torch.float32 if C == 2 else torch.float64).cuda()
            t_masks = torch.from_numpy(masks).cuda()
            layout = "NCHW" if C % 2 else "NHWC"
            t = _as_layout(frames, layout)
            for step in (1, 2):
                for mk, tmk in ((None, None), (masks, t_masks)):
                    ws, wc = overlap_reference(frames, src, tm.cpu().numpy(), (Hc, Wc), step, 1.0, mk)
                    got = mosaic_overlap(t, src, tm, (Hc, Wc), masks=tmk, step=step, layout=layout)
                    what = "%s on %s %s C %d N %d step %d masks %s" % (frame, canvas, dtype, C, N, step, mk is not None)
                    _equal_ints(got.sums, ws, what + " sums")
                    _equal_ints(got.counts, wc, what + " counts")
                    runs += 1
                    live = max(live, int(wc.max()))
                    pairs = max(pairs, int((wc * (1 - np.eye(N, dtype=np.int64)) > 0).sum()))
    assert runs == 3 * 4 * 2 * 2 and live > 0 and pairs > 0, (runs, live, pairs)


def test_overlap_in_nchw_from_views_and_default_arguments():
    from papteam_opticalflow_amd.tensors import mosaic_overlap
    T, H, W, N, n_out, Hc, Wc = 3, 29, 41, 5, 2, 33, 80
    rng = np.random.default_rng(37)
    big = torch.from_numpy(_guide(2 * T, H + 3, 2 * W, 4, torch.uint8, 8)).cuda()
    f = big[::2, 2:H + 2, ::2, 1:]
    M = _mats(rng, n_out, N, H, W, Hc, Wc)
    tm = torch.from_numpy(np.repeat(M, 2, axis=1)).cuda()[:, ::2]
    src = _sources(rng, n_out, N, T)
    ws, wc = overlap_reference(f.cpu().numpy(), src, M, (Hc, Wc))
    got = mosaic_overlap(f.permute(0, 3, 1, 2), src, tm, (Hc, Wc))
    _equal_ints(got.sums, ws, "views sums")
    _equal_ints(got.counts, wc, "views counts")
    assert got.bound == 1.0 and got.sums.is_cuda


def test_culling_changes_no_byte(monkeypatch):
    """PAPOF_MOSAIC_CULL=0 walks every source in every tile: the blend with gains in its four modes and the overlap
    statistics are the same bytes as with the tile-level culling, at the shapes and matrices of test_gpu_mosaic's test of
    that name (tiles with no source, with all of them and cut by a frame's edge, entries that are not finite)"""
    from papteam_opticalflow_amd.tensors import mosaic_overlap
    T, H, W, N, Hc, Wc = 5, 37, 53, 32, 150, 200
    rng = np.random.default_rng(21)
    t = torch.from_numpy(_guide(T, H, W, 3, torch.float32, 22)).cuda()
    tm = torch.from_numpy(_mats(rng, 2, N, H, W, Hc, Wc)).cuda()
    src = _sources(rng, 2, N, T)
    mk = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda()
    tg = torch.from_numpy(_gains(rng, 2, N)).cuda()

    def both(call):
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        on = call()
        monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
        off = call()
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        return on, off

    for mode in MODES:
        (out, cnt), (out0, cnt0) = both(lambda: _blend_call(t, src, tm, (Hc, Wc), mode, tg, mk))
        assert torch.equal(out.view(torch.int32), out0.view(torch.int32)) and torch.equal(cnt, cnt0), mode
        assert int(cnt.min()) == 0 and int(cnt.max()) >= 2
    for step in (1, 2):
        on, off = both(lambda: mosaic_overlap(t, src, tm, (Hc, Wc), masks=mk, step=step, layout="NHWC"))
        assert torch.equal(on.sums, off.sums) and torch.equal(on.counts, off.counts), step
        assert int(on.counts.max()) > 0, step


# ---- pipelines and hygiene
def _exposed_video(n):
    """n frames of the committed 240 x 135 video, frame t under a gain of its own"""
    v = np.stack(_video("240", n)).astype(np.float64)
    g = np.exp(np.random.default_rng(3).uniform(math.log(0.75), 0.0, n))
    return torch.from_numpy(np.clip(np.rint(v * g[:, None, None, None]), 0, 255).astype(np.uint8)).cuda()


@pytest.mark.parametrize("mode,step,ref", [("feather", 1, None), ("median", 1, 0), ("mean", 2, 2), ("first", 2, 1)])
def test_panorama_with_exposure_is_its_composition(mode, step, ref):
    from papteam_opticalflow_amd import tensors
    v = _exposed_video(5)
    T, H, W, _ = v.shape
    p = tensors.panorama(v, 3, mode=mode, step=step, ref=ref, exposure=True, layout="NHWC")
    flow, _, _ = tensors.flow_video(v, 3, layout="NHWC")
    m = tensors.global_motion(flow, model="affine")
    M, size, origin = tensors.mosaic_transforms(m, (H, W), ref=ref)
    assert torch.equal(flow, p.flow) and torch.equal(M[0], p.matrices) and origin == p.origin
    picked = list(range(0, T, step))
    r = (T - 1) // 2 if ref is None else ref
    ov = tensors.mosaic_overlap(v, [picked], M[:, ::step], size, step=2, layout="NHWC")
    g = tensors.exposure_gains(ov, anchor=picked.index(r) if r in picked else None)
    assert g.dtype == torch.float64 and tuple(g.shape) == (1, len(picked)) and torch.equal(g[0], p.gains)
    got = tensors.mosaic(v, [picked], M[:, ::step], size, mode=mode, layout="NHWC", gains=g)
    assert torch.equal(got.out[0], p.image) and torch.equal(got.count[0], p.count)
    assert int(p.count.max()) >= 2 and p.image.dtype == torch.uint8
    # the gains are the restatement's solution of the restated statistics, and the anchor keeps its look
    ws, wc = overlap_reference(v.cpu().numpy(), [picked], M[:, ::step].cpu().numpy(), size, 2, 1.0)
    _equal_ints(ov.sums, ws, "pipeline sums")
    _equal_ints(ov.counts, wc, "pipeline counts")
    want = gains_reference(ws, wc, anchor=picked.index(r) if r in picked else None)
    assert np.abs(g.cpu().numpy() - want).max() < 1e-9
    if r in picked:
        assert float(g[0, picked.index(r)]) == 1.0
    # without exposure: today's call, and no gains
    q = tensors.panorama(v, 3, mode=mode, step=step, ref=ref, layout="NHWC")
    assert q.gains is None
    plain = tensors.mosaic(v, [picked], M[:, ::step], size, mode=mode, layout="NHWC")
    assert torch.equal(plain.out[0], q.image)


def test_inputs_are_unchanged():
    from papteam_opticalflow_amd.tensors import mosaic, mosaic_overlap
    T, H, W, N, Hc, Wc = 4, 37, 53, 6, 40, 70
    rng = np.random.default_rng(14)
    t = torch.from_numpy(_guide(T, H, W, 3, torch.float32, 15)).cuda()
    tm = torch.from_numpy(_mats(rng, 2, N, H, W, Hc, Wc)).cuda()
    mk = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda()
    src = torch.from_numpy(_sources(rng, 2, N, T)).cuda()
    g = torch.from_numpy(_gains(rng, 2, N)).cuda()
    keep = [x.clone() for x in (t, tm, mk, src, g)]
    for mode in MODES:
        mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=mk, layout="NHWC", gains=g)
    mosaic_overlap(t, src, tm, (Hc, Wc), masks=mk, layout="NHWC")
    torch.cuda.synchronize()
    assert torch.equal(t.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(mk, keep[2]) and torch.equal(src, keep[3])
    assert torch.equal(tm.view(torch.int64), keep[1].view(torch.int64)) and torch.equal(g, keep[4])


def test_the_calls_are_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and used under that stream with no synchronisation: both kernels
    (and the zeroing of the statistics) must run after the inputs are written, and what is queued behind them must see
    their output"""
    import time
    from papteam_opticalflow_amd.tensors import mosaic, mosaic_overlap
    T, H, W, Hc, Wc = 5, 40, 60, 50, 90
    rng = np.random.default_rng(16)
    f = _guide(T, H, W, 3, torch.uint8, 17)
    M = _mats(rng, 2, T, H, W, Hc, Wc)
    masks = _frame_masks(rng, T, H, W)
    g = _gains(rng, 2, T)
    want, wcnt = blend_reference(f, None, M, (Hc, Wc), "feather", g, masks, np.uint8)
    ws, wc = overlap_reference(f, None, M, (Hc, Wc), 2, 1.0, masks)
    src = [torch.from_numpy(f).cuda(), torch.from_numpy(M).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(g).cuda()]
    dst = [torch.zeros_like(s) for s in src]
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = mosaic(dst[0], None, dst[1], (Hc, Wc), mode="feather", masks=dst[2], layout="NHWC", gains=dst[3]).out.clone()
        warm2 = mosaic_overlap(dst[0], None, dst[1], (Hc, Wc), masks=dst[2], layout="NHWC").sums.clone()
    del warm, warm2
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        for d, s in zip(dst, src):
            d.copy_(s)
        got = mosaic(dst[0], None, dst[1], (Hc, Wc), mode="feather", masks=dst[2], layout="NHWC", gains=dst[3])
        ov = mosaic_overlap(dst[0], None, dst[1], (Hc, Wc), masks=dst[2], layout="NHWC")
        took = time.perf_counter() - t0
        copy, scopy = got.out.clone(), ov.sums.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    assert took < 0.25, "the calls waited for the stream: %.3f s" % took
    _same(got.out, want, "side stream")
    _same(copy, want, "side stream clone")
    _same(got.count, wcnt, "side stream count")
    _equal_ints(ov.sums, ws, "side stream sums")
    _equal_ints(scopy, ws, "side stream sums clone")
    _equal_ints(ov.counts, wc, "side stream counts")
