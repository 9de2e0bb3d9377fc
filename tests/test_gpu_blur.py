"""Synthetic motion blur on device tensors (papteam_opticalflow_amd/tensors.py: motion_blur, blur_video ->
papof_motion_blur_tensor).  The device's frames must be the BYTES of the numpy fp64 restatement (tests/_blur_ref.py:
blur_reference), compared as raw bytes so that a NaN's payload or a zero's sign is caught: 1, 2 and 3 channels (the two
compiled channel counts and the channel-outermost path), uint8, float32 and float64 frames, NCHW, NHWC and strided views,
float32 and float64 flows with NaNs, infinities and points far outside the image, with and without a mask, 1 to 64
samples, both shutters, every phase, both shapes, every output dtype; the shape edges; sample tables in any order through the C call; flows that reuse the held taps on
every sample and flows that never do; the composition of interpolate's frames; blur_video on the committed video and the
caller's stream order."""
import os

import numpy as np
import pytest

from _blur_ref import blur_reference
from _interp_ref import as_f64, convert
from test_gpu_batch import _video
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same_bytes(got, want, layout, what):
    """got (T, C, H, W) or (T, H, W, C) by layout against want (T, H, W, C), byte for byte"""
    g = got.permute(0, 2, 3, 1) if layout == "NCHW" else got
    g = np.ascontiguousarray(g.cpu().numpy())
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    gb, wb = g.view(np.uint8).reshape(g.shape + (-1,)), w.view(np.uint8).reshape(w.shape + (-1,))
    bad = (gb != wb).any(-1)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r against %r" % (what, int(bad.sum()), bad.size,
                                                                                          i, g[i], w[i]))


def _frames(T, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (T, H, W, C)).astype(np.uint8)
    return rng.random((T, H, W, C)).astype(_NP[dtype])


def _mask(B, H, W, seed):
    """a random mask with an all-occluded block in both channels"""
    rng = np.random.default_rng(seed)
    m = (rng.random((B, 2, H, W)) < 0.3).astype(np.uint8)
    m[:, :, H // 3:H // 3 + 6, W // 4:W // 4 + 9] = 1
    return m


def _on_device(frames, layout):
    """the frames (T, H, W, C) as a device tensor in `layout`; "strided": an NHWC view that skips frames, rows, columns and
    a channel of a larger tensor"""
    t = torch.from_numpy(frames).cuda()
    if layout == "NHWC":
        return t, "NHWC"
    if layout == "NCHW":
        return t.permute(0, 3, 1, 2).contiguous(), "NCHW"
    T, H, W, C = frames.shape
    big = torch.zeros((2 * T, H + 3, 2 * W, C + 1), dtype=t.dtype, device="cuda")
    view = big[::2, 2:H + 2, ::2, 1:]
    view.copy_(t)
    assert not view.is_contiguous()
    return view, "NHWC"


# (samples, shutter, phase, shape): every K of 1, 5, 16, 64, both shutters, the three phases, both shapes
SCHEDULES = [(1, 0.5, -0.5, "box"), (1, 1.0, -1.0, "triangle"), (5, 1.0, -1.0, "box"), (5, 0.5, 0.0, "triangle"),
             (16, 0.5, -0.5, "box"), (16, 1.0, -0.5, "triangle"), (16, 1.0, 0.0, "box"), (64, 1.0, -0.5, "box"),
             (64, 0.5, -1.0, "triangle"), (64, 1.0, 0.0, "triangle")]
T, H, W = 4, 37, 53
_refs = {}  # the float64 results of the restatement, computed once for the layouts that share them


def _case(C, dtype):
    """the frames, the flows in both dtypes (as numpy float64 holds them) and the mask of the main sweep"""
    key = ("case", C, dtype)
    if key not in _refs:
        fw, bw = _fields(T, H, W, 3)
        f32 = tuple(f.astype(np.float32) for f in (fw, bw))
        _refs[key] = (_frames(T, H, W, C, dtype, 1 + C), {torch.float64: (fw, bw), torch.float32: f32}, _mask(T - 1, H, W, 4))
    return _refs[key]


def _reference(C, dtype, i, fdt, masked):
    from papteam_opticalflow_amd.tensors import blur_schedule
    key = (C, dtype, i, fdt, masked)
    if key not in _refs:
        frames, flows, occ = _case(C, dtype)
        K, shutter, phase, shape = SCHEDULES[i]
        off, w = blur_schedule(shutter, K, phase, shape)
        _refs[key] = blur_reference(frames, flows[fdt][0], flows[fdt][1], off, w, occ if masked else None)
    return _refs[key]


@pytest.mark.parametrize("layout", ["NCHW", "NHWC", "strided"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_main_sweep(C, dtype, layout):
    """every schedule with float64 flows and float32 flows, one of the two with the mask (alternating), every out dtype"""
    from papteam_opticalflow_amd.tensors import motion_blur
    frames, flows, occ = _case(C, dtype)
    tv, lay = _on_device(frames, layout)
    tf = {fdt: tuple(torch.from_numpy(f).cuda() for f in flows[fdt]) for fdt in flows}
    tm = torch.from_numpy(occ).cuda().bool()
    seen = set()
    for i, (K, shutter, phase, shape) in enumerate(SCHEDULES):
        for fdt, masked in ((torch.float64, i % 2 == 0), (torch.float32, i % 2 == 1)):
            want = _reference(C, dtype, i, fdt, masked)
            for odt in (None, torch.uint8, torch.float32, torch.float64):
                got = motion_blur(tv, tf[fdt][0], tf[fdt][1], shutter=shutter, samples=K, phase=phase, shape=shape,
                                  occlusion=tm if masked else None, layout=lay, out_dtype=odt)
                assert got.shape == tv.shape and got.dtype == (odt or dtype)
                _same_bytes(got, convert(want, _NP[odt or dtype]), lay, "C %d %s %s schedule %s flows %s mask %s out %s" % (
                    C, dtype, layout, SCHEDULES[i], fdt, masked, odt))
                seen.add(odt or dtype)
    assert len(seen) == 3


def test_branches_are_reached():
    """the fields of the main sweep take every branch of the rule on both sides of a frame, and the schedules reach an end
    frame with no sample left"""
    from papteam_opticalflow_amd.tensors import blur_schedule
    fw, bw = _fields(T, H, W, 3)
    x, r = np.arange(W)[None, None, :], np.arange(H)[:, None][None]
    for t in (0.25, 0.75):  # a sample after the frame, one before it
        s = 1.0 - t
        with np.errstate(invalid="ignore"):
            X0, Y0 = x + (t * t * bw[:, 0] - s * t * fw[:, 0]), r + (t * t * bw[:, 1] - s * t * fw[:, 1])
            X1, Y1 = x + (s * s * fw[:, 0] - s * t * bw[:, 0]), r + (s * s * fw[:, 1] - s * t * bw[:, 1])
            in0 = (X0 >= 0) & (X0 <= W - 1) & (Y0 >= 0) & (Y0 <= H - 1)
            in1 = (X1 >= 0) & (X1 <= W - 1) & (Y1 >= 0) & (Y1 <= H - 1)
        assert (in0 & in1).any() and (in0 & ~in1).any() and (~in0 & in1).any() and (~in0 & ~in1).any()
    assert all(o > 0 for o in blur_schedule(1.0, 16, 0.0)[0]) and all(o < 0 for o in blur_schedule(1.0, 5, -1.0)[0])
    assert 0.0 in blur_schedule(0.5, 5, -0.5)[0]


@pytest.mark.parametrize("shape", [(2, 1, 1, 3), (3, 1, 130, 1), (2, 5, 65, 3), (3, 5, 65, 4), (2, 37, 53, 2)])
def test_shape_edges(shape):
    """one pixel, one row that ends in a part tile, rows beyond one block's four and a part tile, two frames (every frame
    an end frame), four channels"""
    from papteam_opticalflow_amd.tensors import blur_schedule, motion_blur
    Tn, Hn, Wn, C = shape
    fw, bw = _fields(Tn, Hn, Wn, 21, wild=Hn > 8 and Wn > 8)
    rng = np.random.default_rng(22)
    fw[0, :, 0, 0] = (np.nan, 1.0)            # and, in the small fields, a NaN, a far point and a near one
    bw[-1, :, Hn - 1, Wn - 1] = (-3.0 * Wn, 0.5)
    fw[-1, :, Hn // 2, Wn // 2] = (0.75, -0.25)
    occ = (rng.random((Tn - 1, 2, Hn, Wn)) < 0.3).astype(np.uint8)
    for dtype in (torch.uint8, torch.float64):
        frames = _frames(Tn, Hn, Wn, C, dtype, 23)
        tv = torch.from_numpy(frames).cuda()
        for K, shutter, phase, shp in ((5, 1.0, -0.5, "box"), (16, 0.5, -0.5, "triangle"), (4, 1.0, 0.0, "box")):
            off, w = blur_schedule(shutter, K, phase, shp)
            for m in (None, occ):
                got = motion_blur(tv, torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), shutter=shutter, samples=K,
                                  phase=phase, shape=shp, occlusion=None if m is None else torch.from_numpy(m).cuda(),
                                  layout="NHWC")
                _same_bytes(got, blur_reference(frames, fw, bw, off, w, m, _NP[dtype]), "NHWC",
                            "%s %s K %d mask %s" % (shape, dtype, K, m is not None))


def _blur_table(frames, fw, bw, occ, offsets, weights, layout="NHWC"):
    """papof_motion_blur_tensor with a sample table of the caller's own (motion_blur makes blur_schedule's)"""
    from papteam_opticalflow_amd import capi, tensors
    ts, descs, _, _ = tensors._check([("frames", frames)], layout, None, 1, min_frames=2)
    codes = tuple(capi.DTYPE_F32 if f.dtype == torch.float32 else capi.DTYPE_F64 for f in (fw, bw))
    return tensors._blur(ts, descs, (fw, bw), codes, occ, (list(offsets), list(weights)), layout, ts[0].dtype)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_tables_in_any_order_and_weights_of_zero(C):
    """The C call takes any table: offsets that are not sorted by sign are summed in the table's order (the kernel's
    one-loop form), a weight of 0 drops its sample (here one whose frames hold NaNs), and a sorted table may hold an
    offset more than once"""
    Tn, Hn, Wn = 4, 21, 70
    fw, bw = _fields(Tn, Hn, Wn, 61)
    occ = _mask(Tn - 1, Hn, Wn, 62)
    tf, tb, tm = (torch.from_numpy(a).cuda() for a in (fw, bw, occ))
    tables = [([0.25, -0.5, 0.0, 0.75, -0.125, 0.5, 0.0], [0.5, 2.0, 1.0, 0.25, 0.75, 1.5, 0.125]),   # no order
              ([0.5, 0.25, -0.25, -0.5], [1.0, 2.0, 3.0, 4.0]),                                        # descending
              ([-0.5, -0.5, 0.0, 0.0, 0.5, 0.5], [1.0, 0.5, 0.25, 2.0, 1.0, 0.5]),                     # sorted, repeats
              ([-0.5, 0.25, 0.0, 0.5], [1.0, 0.0, 0.0, 1.0]),                                          # sorted once the 0s go
              ([2.0 ** -20, -(1.0 - 2.0 ** -20)], [1.0, 1.0])]                                        # the bounds
    for dtype in (torch.uint8, torch.float64):
        frames = _frames(Tn, Hn, Wn, C, dtype, 63)
        tv = torch.from_numpy(frames).cuda()
        for off, w in tables:
            got = _blur_table(tv, tf, tb, tm, off, w)
            _same_bytes(got, blur_reference(frames, fw, bw, off, w, occ, _NP[dtype]), "NHWC", "C %d %s table %s" % (C, dtype, off))
    nan = _frames(2, Hn, Wn, C, torch.float64, 64)
    nan[1] = np.nan  # the pair's samples are NaN wherever frame 1 enters; frame 0's own sample is not
    got = _blur_table(torch.from_numpy(nan).cuda(), tf[:1], tb[:1], None, [0.0, 0.25], [1.0, 0.0])
    assert np.array_equal(got[0].cpu().numpy().view(np.int64), (nan[0] / 1.0).view(np.int64)) and bool(got[1].isnan().all())


def _cells_change(fw, bw, offsets):
    """over the pixels of the middle frame of three and the consecutive samples on one side of it: the fraction of steps at
    which both of the sample's bilinear cells (in the pair's two frames) stay what they were"""
    Hn, Wn = fw.shape[2:]
    x, r = np.arange(Wn)[None, :], np.arange(Hn)[:, None]
    keep, steps, prev = 0, 0, None
    for tau in offsets:
        if tau == 0.0:
            continue
        pair, t = (1, tau) if tau > 0 else (0, 1.0 + tau)
        s = 1.0 - t
        u, v, bu, bv = fw[pair, 0], fw[pair, 1], bw[pair, 0], bw[pair, 1]
        cells = [np.floor(x + (t * t * bu - s * t * u)), np.floor(r + (t * t * bv - s * t * v)),
                 np.floor(x + (s * s * u - s * t * bu)), np.floor(r + (s * s * v - s * t * bv))]
        if prev is not None and prev[0] == pair:
            same = np.all([a == b for a, b in zip(cells, prev[1])], 0)
            keep += int(same.sum())
            steps += same.size
        prev = (pair, cells)
    return keep / steps


def test_tap_reuse_on_every_sample_and_on_none(monkeypatch):
    """Smooth flows of a fraction of a pixel keep a pixel's samples in one bilinear cell, so every sample after a side's
    first reuses the held taps; flows of tens of pixels change the cell with every sample.  Both must be the restatement's
    bytes, and the bytes with the held taps switched off (PAPOF_BLUR_REUSE=0, read at every call)."""
    from papteam_opticalflow_amd.tensors import blur_schedule, motion_blur
    Tn, Hn, Wn, C = 3, 45, 140, 3
    y, x = np.mgrid[0:Hn, 0:Wn].astype(np.float64)
    slow = np.stack([np.stack([0.30 + 0.05 * np.sin(0.05 * x + p), 0.20 + 0.05 * np.cos(0.04 * y + p)]) for p in (0.0, 1.0)])
    rng = np.random.default_rng(31)
    fast = rng.uniform(-40.0, 40.0, (Tn - 1, 2, Hn, Wn))
    off, w = blur_schedule(1.0, 16, -0.5, "box")
    assert _cells_change(slow, -slow, off) > 0.9 and _cells_change(fast, -fast, off) < 0.1
    occ = _mask(Tn - 1, Hn, Wn, 32)
    for dtype in (torch.uint8, torch.float32):
        frames = _frames(Tn, Hn, Wn, C, dtype, 33)
        tv = torch.from_numpy(frames).cuda()
        for name, fw in (("slow", slow), ("fast", fast)):
            bw = -fw
            want = blur_reference(frames, fw, bw, off, w, occ, _NP[dtype])
            args = (tv, torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda())
            kw = dict(shutter=1.0, samples=16, occlusion=torch.from_numpy(occ).cuda(), layout="NHWC")
            monkeypatch.delenv("PAPOF_BLUR_REUSE", raising=False)
            _same_bytes(motion_blur(*args, **kw), want, "NHWC", "%s flows, %s, held taps" % (name, dtype))
            monkeypatch.setenv("PAPOF_BLUR_REUSE", "0")
            _same_bytes(motion_blur(*args, **kw), want, "NHWC", "%s flows, %s, every sample gathered" % (name, dtype))
    monkeypatch.delenv("PAPOF_BLUR_REUSE", raising=False)
    assert "PAPOF_BLUR_REUSE" not in os.environ


def test_composition_of_interpolated_frames():
    """float64 out is the stated accumulation of interpolate's float64 frames (the composition the kernel replaces), the
    sums made on the host in numpy"""
    from papteam_opticalflow_amd.tensors import blur_schedule, interpolate, motion_blur
    Tn, Hn, Wn, C = 4, 30, 70, 3
    frames = _frames(Tn, Hn, Wn, C, torch.uint8, 41)
    fw, bw = _fields(Tn, Hn, Wn, 42)
    occ = _mask(Tn - 1, Hn, Wn, 43)
    tv, tf, tb, tm = (torch.from_numpy(a).cuda() for a in (frames, fw, bw, occ))
    off, w = blur_schedule(0.8, 9, -0.5, "triangle")
    got = motion_blur(tv, tf, tb, shutter=0.8, samples=9, shape="triangle", occlusion=tm, layout="NHWC",
                      out_dtype=torch.float64)
    neg, pos = [1.0 + o for o in off if o < 0], [o for o in off if o > 0]
    kw = dict(occlusion=tm, layout="NHWC", out_dtype=torch.float64)
    before = interpolate(tv[:-1], tv[1:], tf, tb, neg, **kw).cpu().numpy()  # pair i at 1 + tau: samples of frame i + 1
    after = interpolate(tv[:-1], tv[1:], tf, tb, pos, **kw).cpu().numpy()   # pair i at tau: samples of frame i
    I = as_f64(frames)
    want = np.empty_like(I)
    for f in range(Tn):
        acc, ws, jn, jp = np.zeros(I.shape[1:]), 0.0, 0, 0
        for o, wk in zip(off, w):
            if o < 0:
                S = before[f - 1, jn] if f > 0 else None
                jn += 1
            elif o > 0:
                S = after[f, jp] if f < Tn - 1 else None
                jp += 1
            else:
                S = I[f]
            if S is not None:
                acc = acc + wk * S
                ws = ws + wk
        want[f] = acc / ws
    _same_bytes(got, want, "NHWC", "composition")


def test_blur_video_is_flow_video_fb_and_motion_blur(gpu):
    from papteam_opticalflow_amd.tensors import flow_video_fb, motion_blur, blur_video
    v = _dev(_video("240", 4))
    bv = blur_video(v, 3, shutter=1.0, samples=8, layout="NHWC")
    assert tuple(bv.video.shape) == (4, 135, 240, 3) and bv.video.dtype == torch.uint8
    fb = flow_video_fb(v, 3, layout="NHWC")
    assert torch.equal(bv.flow_fw, fb.flow_fw) and torch.equal(bv.flow_bw, fb.flow_bw)
    assert torch.equal(bv.occlusion, fb.occlusion)
    want = motion_blur(v, fb.flow_fw, fb.flow_bw, shutter=1.0, samples=8, occlusion=fb.occlusion, layout="NHWC")
    assert torch.equal(bv.video, want)
    assert not torch.equal(bv.video, v)
    # NCHW, float32 out, no mask, another schedule
    bv2 = blur_video(v.permute(0, 3, 1, 2), 3, shutter=0.5, samples=5, phase=0.0, shape="triangle", consistency=None,
                     out_dtype=torch.float32)
    assert bv2.occlusion is None and tuple(bv2.video.shape) == (4, 3, 135, 240)
    want = motion_blur(v.permute(0, 3, 1, 2), fb.flow_fw, fb.flow_bw, shutter=0.5, samples=5, phase=0.0, shape="triangle",
                       out_dtype=torch.float32)
    assert torch.equal(bv2.video, want)
    assert torch.equal(bv2.video[-1], (v[-1].permute(2, 0, 1).double() / 255.0).float())  # phase 0: the last frame as it is


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames written on a side stream behind a long sleep and blurred under that stream with no synchronisation: the
    kernel must read them after they are written, and what is queued behind it must see its output"""
    import time
    from papteam_opticalflow_amd.tensors import blur_schedule, motion_blur
    Tn, Hn, Wn, C = 3, 40, 60, 3
    frames = _frames(Tn, Hn, Wn, C, torch.uint8, 51)
    fw, bw = _fields(Tn, Hn, Wn, 52)
    occ = _mask(Tn - 1, Hn, Wn, 53)
    off, w = blur_schedule(0.5, 16)
    want = blur_reference(frames, fw, bw, off, w, occ, np.uint8)
    src = torch.from_numpy(frames).cuda()
    dst = torch.zeros_like(src)
    tf, tb, tm = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), torch.from_numpy(occ).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = motion_blur(dst, tf, tb, occlusion=tm, layout="NHWC").clone()
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the call
        dst.copy_(src)
        got = motion_blur(dst, tf, tb, occlusion=tm, layout="NHWC")
        took = time.perf_counter() - t0
        copy = got.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    assert took < 0.25, "motion_blur waited for the stream: %.3f s" % took
    _same_bytes(got, want, "NHWC", "side stream")
    _same_bytes(copy, want, "NHWC", "side stream clone")
