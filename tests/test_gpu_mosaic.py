"""Video mosaics on device tensors (papteam_opticalflow_amd/tensors.py: mosaic, panorama, stabilize_video_full ->
papof_mosaic_tensor).  The device's output must be the BYTES of the numpy restatement (tests/_mosaic_ref.py): every frame
dtype, 1 .. 4 channels, both layouts, every output dtype, frames and canvases down to one row, column or pixel, 1 .. 255
sources per output in the three modes, matrices that leave tiles with no source, with all of them and cut by a frame's edge,
repeated and empty sources, NaN and infinite entries, with and without masks and the count, float frames with NaNs,
infinities, signed zeros and subnormals, strided and expanded views, the pipelines against the same composition of public
calls, a 1080p canvas run twice and compared at sampled pixels, the inputs left unchanged and the caller's stream order.
The source counts are those at which the kernel changes instance (the median holds 8, 16, 32 or 64 samples per lane, in
tiles of 64 x 4, 64 x 4, 64 x 2 and 64 x 1), each on a canvas with ragged tiles.
One exception to "bytes": a NaN that arithmetic MAKES (infinity times a tap of weight 0, infinity minus infinity) has the
processor's sign -- x86 sets the sign bit, gfx950 does not -- and the rule states none, so where both sides hold a NaN its
SIGN BIT is left out of the comparison; the NaN's other bits, and every bit of every other value, are compared."""
import math

import numpy as np
import pytest

from _interp_ref import convert
from _mosaic_ref import canvas_truth, clean_plate_scene, first_order, mosaic_reference, psnr
from test_gpu_batch import _video
from test_gpu_refine import _NP, _as_layout, _guide

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAIRS = [((37, 53), (40, 70)), ((1, 9), (1, 1)), ((9, 1), (3, 130)), ((5, 4), (70, 9))]  # (frames, canvas)
MODES = ("first", "mean", "median")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same(got, want, what):
    """two arrays of one dtype, byte for byte (NaN against NaN: without the sign bit -- the module's docstring)"""
    g = np.ascontiguousarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got)
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype == np.uint8:
        bad = g != w
    else:
        iv = np.int64 if g.dtype == np.float64 else np.int32
        sign = np.where(np.isnan(g) & np.isnan(w), iv(np.iinfo(iv).min), iv(0))
        bad = (g.view(iv) | sign) != (w.view(iv) | sign)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r against %r" % (what, int(bad.sum()), bad.size, i,
                                                                                          g[i], w[i]))


def _nhwc(t, layout):
    return t if layout == "NHWC" else t.permute(0, 2, 3, 1)


def _mats(rng, n_out, N, H, W, Hc, Wc, wild=True):
    """canvas -> frame matrices, similarities (even k) and affine maps (odd k): most send a random canvas point to a random
    frame point at a scale between 0.3 and 2 -- whole tiles miss the frame, others are cut by its edge --, every fifth
    shrinks the whole canvas into the frame (live at every pixel), every third fits a frame of one row or column (a zero
    row of the matrix); with `wild` an identity, a NaN and an infinite entry"""
    M = np.empty((n_out, N, 2, 3))
    for o in range(n_out):
        for k in range(N):
            th, s = rng.uniform(-math.pi, math.pi), math.exp(rng.uniform(math.log(0.3), math.log(2.0)))
            L = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
            if k % 2:
                L = L @ (np.eye(2) + rng.normal(0, 0.15, (2, 2)))
            c = np.array([rng.uniform(-0.3, 1.3) * (Wc - 1), rng.uniform(-0.3, 1.3) * (Hc - 1)])
            p = np.array([rng.uniform(0, W - 1), rng.uniform(0, H - 1)])
            if k % 5 == 0:
                L = L / s * 0.45 * min(W - 1, H - 1) / max(1.0, math.hypot(Wc, Hc))
                c, p = np.array([(Wc - 1) / 2, (Hc - 1) / 2]), np.array([(W - 1) / 2, (H - 1) / 2])
            if k % 3 == 0 and H == 1:
                L[1], p[1] = 0.0, 0.0
            if k % 3 == 0 and W == 1:
                L[0], p[0] = 0.0, 0.0
            M[o, k, :, :2], M[o, k, :, 2] = L, p - L @ c
    if wild:
        M[0, 0] = np.eye(2, 3)
        if N > 2:
            M[0, 1, 0, 0] = math.nan
            M[-1, N // 2, 1, 2] = math.inf
    return M


def _sources(rng, n_out, N, T):
    """frames in any order with repeats, about one slot in six empty"""
    s = rng.integers(0, T, (n_out, N))
    s[rng.random((n_out, N)) < 0.15] = -1
    return s


def _frame_masks(rng, T, H, W):
    m = (rng.random((T, H, W)) < 0.1).astype(np.uint8)
    m[:, H // 4:H // 2, W // 3:W // 2] = 1
    m[m != 0] = rng.integers(1, 256, int((m != 0).sum()))  # any nonzero byte masks
    return m


@pytest.mark.parametrize("frame,canvas", PAIRS)
def test_every_dtype_channel_count_layout_and_output(frame, canvas):
    from papteam_opticalflow_amd.tensors import mosaic
    (H, W), (Hc, Wc) = frame, canvas
    T, n_out, N = 4, 2, 5
    rng = np.random.default_rng(H * 1000 + W)
    runs, seen = 0, set()
    for dtype in (torch.uint8, torch.float32, torch.float64):
        for C in (1, 2, 3, 4):
            frames = _guide(T, H, W, C, dtype, 3 + C)
            M = _mats(rng, n_out, N, H, W, Hc, Wc)
            src = _sources(rng, n_out, N, T)
            masks = _frame_masks(rng, T, H, W) if C % 2 else None
            tm = torch.from_numpy(M).to(torch.float32 if C == 2 else torch.float64).cuda()
            t_masks = None if masks is None else torch.from_numpy(masks).cuda()
            for mode in MODES:
                want64, wcnt = mosaic_reference(frames, src, tm.cpu().numpy(), (Hc, Wc), mode, masks)
                seen |= set(np.unique(wcnt).tolist())
                for layout in ("NCHW", "NHWC"):
                    t = _as_layout(frames, layout)
                    for odt in (None, torch.uint8, torch.float32, torch.float64):
                        got = mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=t_masks, layout=layout, out_dtype=odt)
                        what = "%s frames %s C %d %s %s out %s" % (frame, dtype, C, mode, layout, odt)
                        assert got.out.shape == ((n_out, C, Hc, Wc) if layout == "NCHW" else (n_out, Hc, Wc, C)), what
                        _same(_nhwc(got.out, layout), convert(want64, _NP[odt or dtype]), what)
                        _same(got.count, wcnt, what + " count")
                        runs += 1
    assert runs == 3 * 4 * 3 * 2 * 4
    assert Hc * Wc < 100 or (0 in seen and max(seen) >= 2), seen  # pixels with no source and with several


@pytest.mark.parametrize("N", [1, 2, 3, 8, 16, 17, 32, 33, 64, 255])
def test_source_counts_in_every_mode_with_and_without_masks_and_count(N):
    from papteam_opticalflow_amd import tensors
    T, H, W, n_out = 6, 37, 53, 2
    rng = np.random.default_rng(N)
    cases = [(torch.uint8, 3, (40, 70)), (torch.float64, 1, (3, 130))] + ([(torch.float32, 2, (70, 9))] if N in (3, 33) else [])
    most = 0
    for dtype, C, (Hc, Wc) in cases:
        frames = _guide(T, H, W, C, dtype, N + C)
        t = torch.from_numpy(frames).cuda()
        M = _mats(rng, n_out, N, H, W, Hc, Wc)
        src = _sources(rng, n_out, N, T)
        src[0, N // 2] = src[0, 0]  # a repeated source
        masks = _frame_masks(rng, T, H, W)
        tm, t_masks = torch.from_numpy(M).cuda(), torch.from_numpy(masks).cuda().bool()
        for mode in MODES:
            if mode == "median" and N > 64:
                with pytest.raises(ValueError):
                    tensors.mosaic(t, src, tm, (Hc, Wc), mode=mode, layout="NHWC")
                continue
            for mk, tmk in ((None, None), (masks, t_masks)):
                want, wcnt = mosaic_reference(frames, src, M, (Hc, Wc), mode, mk, _NP[dtype])
                got = tensors.mosaic(t, torch.from_numpy(src).cuda(), tm, (Hc, Wc), mode=mode, masks=tmk, layout="NHWC")
                what = "N %d %s C %d %s masks %s" % (N, dtype, C, mode, mk is not None)
                _same(got.out, want, what)
                _same(got.count, wcnt, what + " count")
                most = max(most, int(wcnt.max()))
                # without the count (mode "first" then stops at the first live source): the same image
                ts, descs, _, _ = tensors._check([("frames", t)], "NHWC", None, 1)
                out, none = tensors._mosaic(ts, descs, torch.from_numpy(src).to(torch.int32).cuda(), tm, tensors.capi.DTYPE_F64,
                                            None if tmk is None else tmk.view(torch.uint8), Hc, Wc, mode, "NHWC", t.dtype,
                                            count=False)
                assert none is None
                _same(out, want, what + " no count")
    assert most >= (2 if N >= 8 else 1), most


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nans_infinities_signed_zeros_and_subnormals(dtype):
    """Float frames salted with special values, MEDIAN, MEAN and FIRST: a NaN sample sorts last and poisons a mean, an
    infinity is a NaN sample wherever a tap of weight 0 touches it, a subnormal survives; identity and half-pixel matrices
    so that both whole values and blends are met"""
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, C = 7, 21, 30, 2
    rng = np.random.default_rng(5)
    frames = rng.normal(0, 1, (T, H, W, C)).astype(_NP[dtype])
    tiny = 1e-40 if dtype == torch.float32 else 5e-324
    specials = np.array([math.nan, math.inf, -math.inf, 0.0, -0.0, tiny, -tiny, 1e-310 if dtype == torch.float64 else 1e-44])
    salt = rng.random(frames.shape) < 0.3
    frames[salt] = rng.choice(specials, int(salt.sum())).astype(_NP[dtype])
    frames[:, 5:9, 4:12] = 0.25  # equal samples in every frame: ties
    M = np.tile(np.eye(2, 3), (3, T, 1, 1))
    M[1, :, 0, 2] = 0.5
    M[2, :, :, 2] = rng.uniform(-3, 3, (T, 2))
    t, tm = torch.from_numpy(frames).cuda(), torch.from_numpy(M).cuda()
    for mode in MODES:
        for odt in (torch.float32, torch.float64, torch.uint8):
            want, wcnt = mosaic_reference(frames, None, M, (H, W), mode, None, _NP[odt])
            got = mosaic(t, None, tm, (H, W), mode=mode, layout="NHWC", out_dtype=odt)
            _same(got.out, want, "specials %s %s out %s" % (dtype, mode, odt))
            _same(got.count, wcnt, "specials count")
    w64 = mosaic_reference(frames, None, M, (H, W), "median")[0]
    assert np.isnan(w64).any() and np.isfinite(w64).any()
    first = np.abs(mosaic_reference(frames, None, M, (H, W), "first")[0])
    assert ((first > 0) & (first < 1e-39)).any()  # a subnormal came through


def test_strided_and_expanded_views_and_3d_frames():
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, N, n_out, Hc, Wc = 3, 29, 41, 4, 2, 33, 80
    rng = np.random.default_rng(6)
    big = torch.from_numpy(_guide(2 * T, H + 3, 2 * W, 4, torch.uint8, 8)).cuda()
    f = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut: 3 channels
    bm = torch.from_numpy(np.repeat(_frame_masks(rng, T, H, W), 2, axis=2)).cuda()
    mk = bm[:, :, ::2]
    M = _mats(rng, n_out, N, H, W, Hc, Wc)
    wide = torch.from_numpy(np.repeat(M, 2, axis=1)).cuda()
    tm = wide[:, ::2]
    assert not f.is_contiguous() and not mk.is_contiguous() and not tm.is_contiguous()
    src = _sources(rng, n_out, N, T)
    for mode in MODES:
        want, wcnt = mosaic_reference(f.cpu().numpy(), src, M, (Hc, Wc), mode, mk.cpu().numpy(), np.float32)
        got = mosaic(f, src, tm, (Hc, Wc), mode=mode, masks=mk, layout="NHWC", out_dtype=torch.float32)
        _same(got.out, want, "strided " + mode)
        _same(got.count, wcnt, "strided count " + mode)
    # one frame, one mask and one matrix seen many times (stride 0)
    one = torch.from_numpy(_guide(1, H, W, 2, torch.float32, 10)).cuda()
    m1 = torch.from_numpy(_frame_masks(rng, 1, H, W)).cuda()
    M1 = _mats(rng, 1, 1, H, W, Hc, Wc, wild=False)
    M1[0, 0] = [[0.5, 0.1, 2.0], [-0.1, 0.5, 6.0]]
    want, wcnt = mosaic_reference(np.repeat(one.cpu().numpy(), T, 0), None, np.repeat(np.repeat(M1, T, 1), n_out, 0), (Hc, Wc),
                                  "median", np.repeat(m1.cpu().numpy(), T, 0))
    got = mosaic(one.expand(T, H, W, 2), None, torch.from_numpy(M1).cuda().expand(n_out, T, 2, 3), (Hc, Wc),
                 masks=m1.expand(T, H, W), layout="NHWC", out_dtype=torch.float64)
    _same(got.out, want, "expanded")
    _same(got.count, wcnt, "expanded count")
    assert set(np.unique(wcnt).tolist()) == {0, T}
    # 3-D frames: a batch of one
    want, wcnt = mosaic_reference(one.cpu().numpy(), [[0, -1, 0]], np.repeat(M1, 3, 1), (Hc, Wc), "mean")
    got = mosaic(one[0], [[0, -1, 0]], torch.from_numpy(np.repeat(M1, 3, 1)).cuda(), (Hc, Wc), mode="mean", layout="NHWC",
                 out_dtype=torch.float64)
    _same(got.out, want, "3-D frames")
    _same(got.count, wcnt, "3-D frames count")


def test_stabilize_video_full_is_stabilize_video_where_valid_and_its_composition():
    """Four frames of the committed 240 x 135 video, each rolled by a few pixels to shake it.  Measured on an MI355X: 3434
    of 129600 pixels invalid, 3377 of them filled from two neighbours either side."""
    from papteam_opticalflow_amd import tensors
    v = torch.from_numpy(np.stack(_video("240", 4))).cuda()
    T, H, W, _ = v.shape
    # a shaken copy, so that there are borders to fill: frame t rolled by a few pixels (what leaves one edge enters at the other)
    shifts = [(0, 0), (5, -3), (-4, 6), (7, 2)]
    v = torch.stack([torch.roll(v[t], shifts[t], (0, 1)) for t in range(T)])
    sv = tensors.stabilize_video(v, 3, layout="NHWC", radius=15)
    full = tensors.stabilize_video_full(v, 3, layout="NHWC", radius=15, fill_radius=2)
    assert torch.equal(full.valid, sv.valid) and torch.equal(full.transforms, sv.transforms)
    assert torch.equal(full.motion, sv.motion) and torch.equal(full.flow, sv.flow)
    assert full.video.dtype == torch.uint8 and tuple(full.video.shape) == (T, H, W, 3)
    assert torch.equal(full.video[sv.valid], sv.video[sv.valid])
    assert not bool((full.filled & full.valid).any())
    src, mats = tensors.neighbour_transforms(full.transforms, tensors.Motion(full.motion, full.ok, None), 2)
    got = tensors.mosaic(v, src, mats, (H, W), mode="first", layout="NHWC")
    assert torch.equal(got.out, full.video)
    assert torch.equal((got.count > 0) & ~full.valid, full.filled)
    want, wcnt = mosaic_reference(v.cpu().numpy(), src.cpu().numpy(), mats.cpu().numpy(), (H, W), "first", None, np.uint8)
    _same(full.video, want, "stabilize_video_full")
    invalid, filled = int((~full.valid).sum()), int(full.filled.sum())
    print("stabilize_video_full: %d of %d pixels invalid, %d of them filled" % (invalid, T * H * W, filled))
    assert invalid > 0 and filled > 0
    assert not bool(full.video[~full.valid & ~full.filled].any())  # what nobody saw stays 0


@pytest.mark.parametrize("step", [1, 2])
def test_panorama_is_its_composition(step):
    from papteam_opticalflow_amd import tensors
    frames = clean_plate_scene()[0]
    v = torch.from_numpy(frames).cuda()
    T, H, W, _ = frames.shape
    for mode in ("median", "first"):
        p = tensors.panorama(v, 6, mode=mode, step=step, margin=2, layout="NHWC")
        flow, _, _ = tensors.flow_video(v, 6, layout="NHWC")
        m = tensors.global_motion(flow, model="affine")
        M, size, origin = tensors.mosaic_transforms(m, (H, W), margin=2)
        assert torch.equal(flow, p.flow) and torch.equal(m.motion, p.motion) and torch.equal(M[0], p.matrices)
        assert origin == p.origin and tuple(p.image.shape) == size + (3,) and tuple(p.count.shape) == size
        got = tensors.mosaic(v[::step], None, M[:, ::step], size, mode=mode, layout="NHWC")
        assert torch.equal(got.out[0], p.image) and torch.equal(got.count[0], p.count)
        got = tensors.mosaic(v, [list(range(0, T, step))], M[:, ::step], size, mode=mode, layout="NHWC")
        assert torch.equal(got.out[0], p.image)
        assert int(p.count.max()) >= 2 and p.image.dtype == torch.uint8


def test_panorama_with_estimated_motions_keeps_the_median_ahead_of_the_mean():
    """tests/test_mosaic_cpu.py's clean-plate scene, the motions ESTIMATED (flow_video at 6 levels, affine fits) instead of
    exact; PSNR against the world over the pixels that at least three frames cover.  The figures are printed; MEDIAN >= MEAN
    is asserted.  Measured on an MI355X over 23049 pixels: MEDIAN 24.56 dB, MEAN 22.68 dB, FIRST 21.89 dB (with exact
    motions the restatement gives 36.57, 26.98 and 22.20 dB: the estimated chain costs the median most, and keeps the
    order)."""
    from papteam_opticalflow_amd import tensors
    frames, Ks, _, world = clean_plate_scene()
    T = len(frames)
    ref = (T - 1) // 2
    v = torch.from_numpy(frames).cuda()
    p = tensors.panorama(v, 6, mode="median", layout="NHWC", out_dtype=torch.float64)
    size = tuple(p.count.shape)
    truth = canvas_truth(world, Ks[ref], p.origin, size)
    where = (p.count.cpu().numpy() >= 3) & np.isfinite(truth).all(-1)
    res = {"median": psnr(p.image.cpu().numpy(), truth, where)}
    for mode in ("mean", "first"):
        order = first_order(T, ref) if mode == "first" else list(range(T))
        got = tensors.mosaic(v, [order], p.matrices[order][None], size, mode=mode, layout="NHWC", out_dtype=torch.float64)
        res[mode] = psnr(got.out[0].cpu().numpy(), truth, where)
    print("estimated-motion panorama over %d pixels: MEDIAN %.2f dB, MEAN %.2f dB, FIRST %.2f dB" % (
        int(where.sum()), res["median"], res["mean"], res["first"]))
    assert where.sum() > 10000
    assert res["median"] >= res["mean"], res


def test_1080p_canvas_from_sixteen_sources_twice_and_at_sampled_pixels():
    """One 1920 x 1080 canvas, the median of sixteen 480 x 270 uint8 sources, run twice: the same bytes; and 4096 random
    pixels, the four corners and 64 points on every border against the restatement evaluated at those pixels only"""
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, Hc, Wc = 16, 270, 480, 1080, 1920
    rng = np.random.default_rng(13)
    frames = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    M = np.empty((1, T, 2, 3))
    for k in range(T):
        th, s = rng.normal(0, 0.1), rng.uniform(0.28, 0.5)
        L = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        c = np.array([rng.uniform(0.2, 0.8) * Wc, rng.uniform(0.2, 0.8) * Hc])
        M[0, k, :, :2], M[0, k, :, 2] = L, np.array([(W - 1) / 2, (H - 1) / 2]) - L @ c
    t, tm = torch.from_numpy(frames).cuda(), torch.from_numpy(M).cuda()
    a = mosaic(t, None, tm, (Hc, Wc), layout="NHWC")
    b = mosaic(t, None, tm, (Hc, Wc), layout="NHWC")
    assert torch.equal(a.out, b.out) and torch.equal(a.count, b.count)
    edge_y, edge_x = rng.integers(0, Hc, 64), rng.integers(0, Wc, 64)
    ys = np.concatenate([rng.integers(0, Hc, 4096), [0, 0, Hc - 1, Hc - 1], np.zeros(64, int), np.full(64, Hc - 1), edge_y, edge_y])
    xs = np.concatenate([rng.integers(0, Wc, 4096), [0, Wc - 1, 0, Wc - 1], edge_x, edge_x, np.zeros(64, int), np.full(64, Wc - 1)])
    assert len(ys) == len(xs) == 4096 + 4 + 256
    want, wcnt = mosaic_reference(frames, None, M, (Hc, Wc), "median", None, np.uint8,
                                  pixels=np.stack([np.zeros_like(ys), ys, xs], 1))
    _same(a.out.cpu().numpy()[0][ys, xs], want, "1080p sampled")
    _same(a.count.cpu().numpy()[0][ys, xs], wcnt, "1080p sampled count")
    assert wcnt.min() == 0 and wcnt.max() >= 8, (wcnt.min(), wcnt.max())


def test_culling_changes_no_byte(monkeypatch):
    """PAPOF_MOSAIC_CULL=0 walks every source in every tile: the same bytes as with the tile-level culling, on matrices that
    leave tiles with no source, with all of them and cut by a frame's edge, and with entries that are not finite"""
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, N, Hc, Wc = 5, 37, 53, 32, 150, 200
    rng = np.random.default_rng(21)
    t = torch.from_numpy(_guide(T, H, W, 3, torch.float32, 22)).cuda()
    tm = torch.from_numpy(_mats(rng, 2, N, H, W, Hc, Wc)).cuda()
    src = _sources(rng, 2, N, T)
    mk = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda()
    for mode in MODES:
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        on = mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=mk, layout="NHWC")
        monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
        off = mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=mk, layout="NHWC")
        assert torch.equal(on.out.view(torch.int32), off.out.view(torch.int32)) and torch.equal(on.count, off.count), mode
        assert int(on.count.min()) == 0 and int(on.count.max()) >= 2
    monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
    want, wcnt = mosaic_reference(t.cpu().numpy(), src, tm.cpu().numpy(), (Hc, Wc), "median", mk.cpu().numpy(), np.float32)
    _same(off.out, want, "culling off")
    _same(off.count, wcnt, "culling off count")


def test_inputs_are_unchanged():
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, N, Hc, Wc = 4, 37, 53, 6, 40, 70
    rng = np.random.default_rng(14)
    t = torch.from_numpy(_guide(T, H, W, 3, torch.float32, 15)).cuda()
    tm = torch.from_numpy(_mats(rng, 2, N, H, W, Hc, Wc)).cuda()
    mk = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda()
    src = torch.from_numpy(_sources(rng, 2, N, T)).cuda()
    keep = [x.clone() for x in (t, tm, mk, src)]
    for mode in MODES:
        mosaic(t, src, tm, (Hc, Wc), mode=mode, masks=mk, layout="NHWC")
    torch.cuda.synchronize()
    assert torch.equal(t.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(mk, keep[2]) and torch.equal(src, keep[3])
    assert torch.equal(tm.view(torch.int64), keep[1].view(torch.int64))  # (the NaN entry included)


def test_the_call_is_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and used under that stream with no synchronisation: the kernel
    must read them after they are written, and what is queued behind it must see its output"""
    import time
    from papteam_opticalflow_amd.tensors import mosaic
    T, H, W, Hc, Wc = 5, 40, 60, 50, 90
    rng = np.random.default_rng(16)
    f = _guide(T, H, W, 3, torch.uint8, 17)
    M = _mats(rng, 2, T, H, W, Hc, Wc)
    masks = _frame_masks(rng, T, H, W)
    want, wcnt = mosaic_reference(f, None, M, (Hc, Wc), "median", masks, np.uint8)
    src = [torch.from_numpy(f).cuda(), torch.from_numpy(M).cuda(), torch.from_numpy(masks).cuda()]
    dst = [torch.zeros_like(s) for s in src]
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = mosaic(dst[0], None, dst[1], (Hc, Wc), masks=dst[2], layout="NHWC").out.clone()
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
        for d, s in zip(dst, src):
            d.copy_(s)
        got = mosaic(dst[0], None, dst[1], (Hc, Wc), masks=dst[2], layout="NHWC")
        took = time.perf_counter() - t0
        copy, ccopy = got.out.clone(), got.count.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    assert took < 0.25, "the call waited for the stream: %.3f s" % took
    _same(got.out, want, "side stream")
    _same(copy, want, "side stream clone")
    _same(ccopy, wcnt, "side stream count")
