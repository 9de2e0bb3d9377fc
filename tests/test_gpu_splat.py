"""Forward warping on device tensors (papteam_opticalflow_amd/tensors.py: splat, splat_weights, interpolate(method="splat"),
interpolate_pairs / interpolate_video(method="splat") -> papof_splat_tensor, papof_interp_splat_tensor).  The device's
output must be the BYTES of the numpy restatement (tests/_splat_ref.py), compared as raw bytes: uint8, float32 and float64
inputs, NCHW, NHWC and strided views, float32 and float64 flows and weights, no weights, one and several times (0 and 1.2
among them), every output dtype, a bound other than 1, synthetic flows with NaNs and landings outside the image, real flows
of the committed video, full collisions, a dense 1080p case run twice; the interpolation with and without mask and weights,
sequence mode against pair mode, interpolate_video, method="gather" unchanged, the caller's stream order, and the
interpolation error on the committed frame triples."""
import numpy as np
import pytest

from _interp_ref import as_f64, interp_reference
from _splat_ref import interp_splat_reference, splat_reference
from test_gpu_batch import _video
from test_gpu_interp import _frames, _mask, _same_bytes
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


def _same_coverage(got, want, what):
    g = np.ascontiguousarray(got.cpu().numpy())
    assert g.shape == want.shape and g.dtype == np.float64, (what, g.shape, want.shape, g.dtype)
    bad = g.view(np.int64) != np.ascontiguousarray(want).view(np.int64)
    assert not bad.any(), "%s: %d of %d coverages differ; first at %s" % (what, int(bad.sum()), bad.size,
                                                                         tuple(int(k[0]) for k in np.nonzero(bad)))


def _weights(B, H, W, seed):
    """weights in (0, 1.3) with zeros, negatives, NaNs and infinities"""
    rng = np.random.default_rng(seed)
    w = rng.random((B, H, W)) * 1.3
    for val in (0.0, -0.5, np.nan, np.inf):
        w[tuple(rng.integers(0, s, max(1, w.size // 300)) for s in (B, H, W))] = val
    return w


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    from papteam_opticalflow_amd.tensors import splat
    B, H, W, C = 2, 37, 53, 3
    x = _frames(B, H, W, C, dtype, 1)
    fw, _ = _fields(B + 1, H, W, 3)
    w = _weights(B, H, W, 4)
    tx = _dev(list(x)) if layout == "NHWC" else _dev(list(x)).permute(0, 3, 1, 2)
    seen = set()
    for fdt in (torch.float64, torch.float32):
        tf = torch.from_numpy(fw).to(fdt).cuda()
        nf = tf.cpu().numpy()
        for wdt in (None, torch.float64, torch.float32):
            tw = torch.from_numpy(w).to(wdt).cuda() if wdt is not None else None
            nw = tw.cpu().numpy() if tw is not None else None
            for times in ([1.0], [0.0, 0.5, 1.0, 1.2]):
                for odt in (None, torch.uint8, torch.float32, torch.float64):
                    got = splat(tx, tf, times, weight=tw, fill=0.5, layout=layout, out_dtype=odt)
                    want, cov = splat_reference(x, nf, times, nw, fill=0.5, out_dtype=_NP[odt or dtype])
                    what = "%s %s flows %s weights %s times %s out %s" % (dtype, layout, fdt, wdt, times, odt)
                    _same_bytes(got.out, want, layout, what)
                    _same_coverage(got.coverage, cov, what)
                    seen.add(odt or dtype)
    assert len(seen) == 3
    # the fields reach every branch: holes, landings outside, skipped pixels
    _, cov = splat_reference(x, fw, [1.0], w)
    assert (cov < 2.0 ** -24).any() and (cov >= 2.0 ** -24).any() and np.isnan(fw).any()


def test_strided_views_bound_and_default_time():
    from papteam_opticalflow_amd.tensors import splat
    B, H, W = 3, 29, 41
    fw, _ = _fields(B + 1, H, W, 5, wild=False)
    rng = np.random.default_rng(6)
    big = torch.from_numpy(rng.uniform(-900.0, 900.0, (2 * B, H + 3, 2 * W, 3))).cuda()
    x = big[::2, 2:H + 2, ::2, 1:]  # every other item, rows cut, every other column, channels cut: a 2-channel field
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)  # channels-last flow
    w = _weights(B, H, 2 * W, 7)
    tw = torch.from_numpy(w).cuda()[:, :, 1::2]
    assert not x.is_contiguous() and not tf.is_contiguous() and not tw.is_contiguous()
    got = splat(x, tf, weight=tw, bound=1024.0, fill=-1.0, layout="NHWC")  # times: 1.0 by default
    want, cov = splat_reference(x.cpu().numpy(), fw, [1.0], tw.cpu().numpy(), bound=1024.0, fill=-1.0)
    _same_bytes(got.out, want, "NHWC", "strided, bound 1024")
    _same_coverage(got.coverage, cov, "strided, bound 1024")
    # a flow carried to the frame it points to, float32 in, NCHW: splat(flow, flow, bound=...)
    f32 = torch.from_numpy(fw).float().cuda()
    got = splat(f32, f32, 1.0, bound=4.0, out_dtype=torch.float64)
    want, cov = splat_reference(f32.cpu().numpy().transpose(0, 2, 3, 1), f32.cpu().numpy(), [1.0], bound=4.0)
    _same_bytes(got.out, want, "NCHW", "flow along itself")
    _same_coverage(got.coverage, cov, "flow along itself")
    # a small bound, 3-D input: a batch of one
    small = torch.from_numpy(rng.uniform(-1e-3, 1e-3, (H, W, 1))).cuda()
    got = splat(small, tf[:1], [0.5], bound=2.0 ** -9, layout="NHWC")
    want, cov = splat_reference(small.cpu().numpy()[None], fw[:1], [0.5], bound=2.0 ** -9)
    _same_bytes(got.out, want, "NHWC", "bound 2^-9")


def test_more_times_than_one_round_takes():
    from papteam_opticalflow_amd.tensors import splat
    B, H, W, C = 2, 20, 70, 1
    x = _frames(B, H, W, C, torch.float64, 9)
    fw, _ = _fields(B + 1, H, W, 11)
    times = [(j - 4) / 30 for j in range(40)]
    got = splat(_dev(list(x)), torch.from_numpy(fw).cuda(), times, layout="NHWC")
    want, cov = splat_reference(x, fw, times)
    _same_bytes(got.out, want, "NHWC", "40 times")
    _same_coverage(got.coverage, cov, "40 times")


def test_real_flows_of_the_committed_video(gpu):
    from papteam_opticalflow_amd.tensors import flow_video_fb, splat, splat_weights
    v = _dev(_video("240", 4))
    fb = flow_video_fb(v, 4, layout="NHWC")
    w = splat_weights(v[:-1], fb.warpI2_fw, layout="NHWC")
    assert w.dtype == torch.float64 and tuple(w.shape) == (3, 135, 240)
    assert float(w.min()) >= np.exp(-11.0) * (1 - 1e-12) and float(w.max()) <= 1.0
    got = splat(v[:-1], fb.flow_fw, [0.5, 1.0], weight=w, layout="NHWC")
    want, cov = splat_reference(v[:-1].cpu().numpy(), fb.flow_fw.cpu().numpy(), [0.5, 1.0], w.cpu().numpy(),
                                out_dtype=np.uint8)
    _same_bytes(got.out, want, "NHWC", "real flows")
    _same_coverage(got.coverage, cov, "real flows")


def test_every_pixel_lands_on_one_of_four_targets():
    """about 32 K adds per address, in whatever order the hardware takes them: the integer sums do not depend on it"""
    from papteam_opticalflow_amd.tensors import splat
    B, H, W, C = 1, 135, 240, 3
    x = _frames(B, H, W, C, torch.float64, 20)
    rng = np.random.default_rng(21)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    tx, ty = 100.0 + rng.random((H, W)), 60.0 + rng.random((H, W))  # every landing inside one cell: four targets
    flow = np.stack([tx - xs, ty - ys])[None]
    w = rng.random((B, H, W))
    got = splat(_dev(list(x)), torch.from_numpy(flow).cuda(), 1.0, weight=torch.from_numpy(w).cuda(), layout="NHWC")
    want, cov = splat_reference(x, flow, [1.0], w)
    assert (cov >= 2.0 ** -24).sum() == 4 and cov.max() > 1000.0
    _same_bytes(got.out, want, "NHWC", "four targets")
    _same_coverage(got.coverage, cov, "four targets")


def _smooth_1080p(seed):
    B, H, W = 1, 1080, 1920
    g = torch.Generator().manual_seed(seed)
    fw = torch.nn.functional.interpolate(torch.randn(B, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 6,
                                         size=(H, W), mode="bilinear", align_corners=False)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    return fw


def test_dense_1080p_twice():
    from papteam_opticalflow_amd.tensors import splat
    B, H, W, C = 1, 1080, 1920, 3
    x = _frames(B, H, W, C, torch.uint8, 12)
    fw = _smooth_1080p(14)
    tx, tf = _dev(list(x)), fw.cuda()
    one = splat(tx, tf, [0.5], layout="NHWC", out_dtype=torch.float64)
    two = splat(tx, tf, [0.5], layout="NHWC", out_dtype=torch.float64)
    assert torch.equal(one.out.view(torch.int64), two.out.view(torch.int64))
    assert torch.equal(one.coverage.view(torch.int64), two.coverage.view(torch.int64))
    want, cov = splat_reference(x, fw.numpy(), [0.5])
    _same_bytes(one.out, want, "NHWC", "1080p")
    _same_coverage(one.coverage, cov, "1080p")


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float64])
def test_interpolate_by_splatting(dtype, layout):
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 2, 37, 53, 3
    a, b = _frames(B, H, W, C, dtype, 1), _frames(B, H, W, C, dtype, 2)
    fw, bw = _fields(B + 1, H, W, 3)
    occ = _mask(B, H, W, 4)
    w0, w1 = _weights(B, H, W, 5), _weights(B, H, W, 6)
    w0[:, 10:20, 10:30] = 0.0  # a region nothing is splatted from: holes where the gather rule and its mask decide
    w1[:, 5:25, 5:35] = 0.0
    dev = lambda x: _dev(list(x)) if layout == "NHWC" else _dev(list(x)).permute(0, 3, 1, 2)  # noqa: E731
    ta, tb = dev(a), dev(b)
    holes = 0
    for fdt in (torch.float64, torch.float32):
        tf, tbw = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tbw.cpu().numpy()
        for m in (None, occ):
            tm = torch.from_numpy(m).cuda().bool() if m is not None else None
            for ws in (None, (w0, w1), (None, w1.astype(np.float32))):
                tws = None if ws is None else tuple(None if w is None else torch.from_numpy(w).cuda() for w in ws)
                for times in ([0.5], [0.125, 0.5, 0.875]):
                    for odt in (None, torch.float32) if fdt == torch.float64 else (torch.uint8, torch.float64):
                        got = interpolate(ta, tb, tf, tbw, times, occlusion=tm, layout=layout, out_dtype=odt,
                                          method="splat", weights=tws)
                        want = interp_splat_reference(a, b, nf, nb, times, ws, m, _NP[odt or dtype])
                        _same_bytes(got, want, layout, "%s %s flows %s mask %s weights %s times %s out %s" % (
                            dtype, layout, fdt, m is not None, ws is not None, times, odt))
                if ws is not None and m is not None:
                    plain = interp_splat_reference(a, b, nf, nb, [0.5], ws, None)
                    masked = interp_splat_reference(a, b, nf, nb, [0.5], ws, m)
                    holes += int((plain != masked).sum())
    assert holes > 0  # the mask's fallback was reached


def test_gather_is_unchanged():
    """method="gather" and the default give interp_reference's bytes, as before"""
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 2, 37, 53, 3
    a, b = _frames(B, H, W, C, torch.uint8, 1), _frames(B, H, W, C, torch.uint8, 2)
    fw, bw = _fields(B + 1, H, W, 3)
    occ = _mask(B, H, W, 4)
    ta, tb, tf, tbw = _dev(list(a)), _dev(list(b)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    tm = torch.from_numpy(occ).cuda()
    want = interp_reference(a, b, fw, bw, [0.25, 0.5], occ, np.uint8)
    _same_bytes(interpolate(ta, tb, tf, tbw, [0.25, 0.5], occlusion=tm, layout="NHWC"), want, "NHWC", "default")
    _same_bytes(interpolate(ta, tb, tf, tbw, [0.25, 0.5], occlusion=tm, layout="NHWC", method="gather"), want, "NHWC",
                "gather")
    with pytest.raises(ValueError):
        interpolate(ta, tb, tf, tbw, 0.5, layout="NHWC", method="nearest")


def test_video_by_splatting_is_the_pairwise_call(gpu):
    """interpolate_video(method="splat") (sequence mode): the input frames in place, the rest equal to interpolate on the
    same pairs with the weights of the flow call's own warped frames -- and to the restatement"""
    from papteam_opticalflow_amd.tensors import flow_video_fb, interpolate, interpolate_pairs, interpolate_video, splat_weights
    v = _dev(_video("240", 4))
    factor = 4
    iv = interpolate_video(v, 3, factor=factor, layout="NHWC", method="splat")
    assert tuple(iv.video.shape) == (3 * factor + 1, 135, 240, 3) and iv.video.dtype == torch.uint8
    assert torch.equal(iv.video[::factor], v)  # the originals, byte for byte
    fb = flow_video_fb(v, 3, layout="NHWC")
    assert torch.equal(iv.flow_fw, fb.flow_fw) and torch.equal(iv.flow_bw, fb.flow_bw)
    ws = (splat_weights(v[:-1], fb.warpI2_fw, layout="NHWC"), splat_weights(v[1:], fb.warpI2_bw, layout="NHWC"))
    times = [0.25, 0.5, 0.75]
    got = interpolate(v[:-1], v[1:], fb.flow_fw, fb.flow_bw, times, occlusion=fb.occlusion, layout="NHWC", method="splat",
                      weights=ws)
    for i in range(3):
        for j in range(3):
            assert torch.equal(iv.video[factor * i + 1 + j], got[i, j]), (i, j)
    n = v.cpu().numpy()
    want = interp_splat_reference(n[:-1], n[1:], fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), times,
                                  tuple(w.cpu().numpy() for w in ws), fb.occlusion.cpu().numpy(), np.uint8)
    _same_bytes(got, want, "NHWC", "video by splatting")
    # the pairs call with another alpha
    from papteam_opticalflow_amd.tensors import flow_pairs_fb
    ip = interpolate_pairs(v[:2], v[2:], 3, [0.5], layout="NHWC", method="splat", alpha=5.0)
    fp = flow_pairs_fb(v[:2], v[2:], 3, layout="NHWC")
    assert torch.equal(ip.flow_fw, fp.flow_fw) and torch.equal(ip.occlusion, fp.occlusion)
    wp = (splat_weights(v[:2], fp.warpI2_fw, 5.0, layout="NHWC"), splat_weights(v[2:], fp.warpI2_bw, 5.0, layout="NHWC"))
    want = interpolate(v[:2], v[2:], fp.flow_fw, fp.flow_bw, [0.5], occlusion=fp.occlusion, layout="NHWC", method="splat",
                       weights=wp)
    assert torch.equal(ip.frames, want)
    # NCHW views of the same frames: the same frames
    ipc = interpolate_pairs(v[:2].permute(0, 3, 1, 2), v[2:].permute(0, 3, 1, 2), 3, [0.5], method="splat", alpha=0.0)
    ones = interpolate(v[:2], v[2:], fp.flow_fw, fp.flow_bw, [0.5], occlusion=fp.occlusion, layout="NHWC", method="splat")
    assert torch.equal(ipc.frames.permute(0, 1, 3, 4, 2), ones)  # alpha = 0: every weight is exp(-0) = 1


def test_the_calls_are_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and splatted under that stream with no synchronisation: the
    clear, the adds and the resolve must follow the writes, and what is queued behind them must see their output"""
    import time
    from papteam_opticalflow_amd.tensors import interpolate, splat
    B, H, W, C = 2, 40, 60, 3
    a, b = _frames(B, H, W, C, torch.uint8, 16), _frames(B, H, W, C, torch.uint8, 17)
    fw, bw = _fields(B + 1, H, W, 18)
    w = _weights(B, H, W, 19)
    want_s, want_c = splat_reference(a, fw, [0.25, 1.0], w, out_dtype=np.uint8)
    want_i = interp_splat_reference(a, b, fw, bw, [0.25, 0.5], (w, None), None, np.uint8)
    src = [_dev(list(a)), _dev(list(b)), torch.from_numpy(w).cuda()]
    dst = [torch.zeros_like(s) for s in src]
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = splat(dst[0], tf, [0.25, 1.0], weight=dst[2], layout="NHWC").out.clone()
        warm2 = interpolate(dst[0], dst[1], tf, tb, [0.25, 0.5], layout="NHWC", method="splat", weights=(dst[2], None)).clone()
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
        got = splat(dst[0], tf, [0.25, 1.0], weight=dst[2], layout="NHWC")
        goti = interpolate(dst[0], dst[1], tf, tb, [0.25, 0.5], layout="NHWC", method="splat", weights=(dst[2], None))
        took = time.perf_counter() - t0
        copy, copyi = got.out.clone(), goti.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    assert took < 0.25, "the calls waited for the stream: %.3f s" % took
    _same_bytes(got.out, want_s, "NHWC", "side stream")
    _same_bytes(copy, want_s, "NHWC", "side stream clone")
    _same_coverage(got.coverage, want_c, "side stream")
    _same_bytes(goti, want_i, "NHWC", "side stream, interpolate")
    _same_bytes(copyi, want_i, "NHWC", "side stream clone, interpolate")


def test_interpolation_error_on_the_committed_frames(gpu):
    """Frame 2 of the committed 240x135 and 480x270 triples from frames 1 and 3 at t = 0.5 by splatting along the device's
    flows of (1, 3) both ways (5 levels) with the default alpha: a mean absolute error below that of the plain blend
    0.5 (I1 + I3).  The error beside method="gather"'s is printed, not asserted (DESIGN.md 19 records it)."""
    import cases
    from papteam_opticalflow_amd.tensors import interpolate_pairs
    for res in ("240", "480"):
        f1, f2, f3 = (cases.load_frame_u8(res, i) for i in (1, 2, 3))
        sp = interpolate_pairs(_dev([f1]), _dev([f3]), 5, 0.5, layout="NHWC", out_dtype=torch.float64, method="splat")
        ga = interpolate_pairs(_dev([f1]), _dev([f3]), 5, 0.5, layout="NHWC", out_dtype=torch.float64)
        err = float(np.abs(sp.frames[0, 0].cpu().numpy() - as_f64(f2)).mean())
        gather = float(np.abs(ga.frames[0, 0].cpu().numpy() - as_f64(f2)).mean())
        blend = float(np.abs(0.5 * (as_f64(f1) + as_f64(f3)) - as_f64(f2)).mean())
        print("interpolation error %s: splat %.6f  gather %.6f  blend %.6f" % (res, err, gather, blend))
        assert np.isfinite(err) and err < blend, (res, err, blend)
