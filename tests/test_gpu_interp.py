"""Frame interpolation on device tensors (papteam_opticalflow_amd/tensors.py: interpolate, interpolate_pairs,
interpolate_video -> papof_interp_tensor).  The device's frames must be the BYTES of the numpy fp64 restatement
(tests/_interp_ref.py: interp_reference), compared as raw bytes so that a NaN's payload or a zero's sign is caught: uint8,
float32 and float64 frames, NCHW, NHWC and strided views, float32 and float64 flows, with and without a mask, one and
several times, every output dtype, synthetic flows with NaNs, points outside the image and occluded pixels, a dense 1080p
case; sequence mode against pair mode, interpolate_video on the committed video, the caller's stream order, and the
interpolation error on the committed frame triples."""
import math

import numpy as np
import pytest

from _interp_ref import as_f64, interp_reference
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
    """got (B, K, C, H, W) or (B, K, H, W, C) by layout against want (B, K, H, W, C), byte for byte"""
    g = got.permute(0, 1, 3, 4, 2) if layout == "NCHW" else got
    g = np.ascontiguousarray(g.cpu().numpy())
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    gb, wb = g.view(np.uint8).reshape(g.shape + (-1,)), w.view(np.uint8).reshape(w.shape + (-1,))
    bad = (gb != wb).any(-1)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r against %r" % (what, int(bad.sum()), bad.size,
                                                                                          i, g[i], w[i]))


def _frames(B, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    return rng.random((B, H, W, C)).astype(_NP[dtype])


def _mask(B, H, W, seed):
    """a random mask with an all-occluded block in both channels"""
    rng = np.random.default_rng(seed)
    m = (rng.random((B, 2, H, W)) < 0.3).astype(np.uint8)
    m[:, :, H // 3:H // 3 + 6, W // 4:W // 4 + 9] = 1
    return m


def _synthetic(B, H, W, seed):
    """flows with NaNs, infinities and large displacements (test_gpu_track._fields), as B pairs"""
    fw, bw = _fields(B + 1, H, W, seed)
    return fw, bw


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 2, 37, 53, 3
    a, b = _frames(B, H, W, C, dtype, 1), _frames(B, H, W, C, dtype, 2)
    fw, bw = _synthetic(B, H, W, 3)
    occ = _mask(B, H, W, 4)
    dev = lambda x: _dev(list(x)) if layout == "NHWC" else _dev(list(x)).permute(0, 3, 1, 2)  # noqa: E731
    ta, tb = dev(a), dev(b)
    seen = set()
    for fdt in (torch.float64, torch.float32):
        tf, tbw = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tbw.cpu().numpy()
        for m in (None, occ):
            tm = torch.from_numpy(m).cuda().bool() if m is not None else None
            for times in ([0.5], [0.125, 0.5, 0.875]):
                for odt in (None, torch.uint8, torch.float32, torch.float64):
                    got = interpolate(ta, tb, tf, tbw, times, occlusion=tm, layout=layout, out_dtype=odt)
                    want = interp_reference(a, b, nf, nb, times, m, _NP[odt or dtype])
                    _same_bytes(got, want, layout, "%s %s flows %s mask %s times %s out %s" % (
                        dtype, layout, fdt, m is not None, times, odt))
                    seen.add(odt or dtype)
    assert len(seen) == 3


def test_branches_are_reached(gpu):
    """the synthetic fields of the tests above take every branch of the rule at t = 0.5"""
    B, H, W = 2, 37, 53
    fw, bw = _synthetic(B, H, W, 3)
    t, s = 0.5, 0.5
    x, r = np.arange(W)[None, None, :], np.arange(H)[:, None][None]
    with np.errstate(invalid="ignore"):
        X0, Y0 = x + (t * t * bw[:, 0] - s * t * fw[:, 0]), r + (t * t * bw[:, 1] - s * t * fw[:, 1])
        X1, Y1 = x + (s * s * fw[:, 0] - s * t * bw[:, 0]), r + (s * s * fw[:, 1] - s * t * bw[:, 1])
        in0 = (X0 >= 0) & (X0 <= W - 1) & (Y0 >= 0) & (Y0 <= H - 1)
        in1 = (X1 >= 0) & (X1 <= W - 1) & (Y1 >= 0) & (Y1 <= H - 1)
    assert (in0 & in1).any() and (in0 & ~in1).any() and (~in0 & in1).any() and (~in0 & ~in1).any()
    m = _mask(B, H, W, 4)
    assert (in0 & in1 & (m[:, 0] == 1) & (m[:, 1] == 1)).any()  # integer points inside the all-occluded block


def test_strided_views_and_mixed_dtypes():
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 3, 29, 41, 3
    fw, bw = _synthetic(B, H, W, 5)
    big = torch.from_numpy(_frames(2 * B, H + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    a = big[::2, 2:H + 2, ::2, 1:]                        # every other frame, rows cut, every other column, channels cut
    b = torch.from_numpy(_frames(B, H, W, C, torch.float32, 7)).cuda().permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not a.is_contiguous() and not b.is_contiguous()
    # flows as (B, H, W, 2) channels-last, read as (B, 2, H, W), and a mask sliced from a wider one
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    tb = torch.from_numpy(bw).float().cuda()
    m = _mask(B, H, 2 * W, 8)
    tm = torch.from_numpy(m).cuda()[:, :, :, 1::2]
    times = [0.3, 0.7]
    want = interp_reference(a.cpu().numpy(), b.cpu().numpy(), fw, tb.cpu().numpy(), times, tm.cpu().numpy(), np.float32)
    got = interpolate(a, b, tf, tb, times, occlusion=tm, layout="NHWC")  # uint8 with float32: float32 out
    assert got.dtype == torch.float32
    _same_bytes(got, want, "NHWC", "strided views")
    # the same frames as NCHW views, a 1-D tensor of times and uint8 out
    got = interpolate(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), tf, tb, torch.tensor(times), occlusion=tm,
                      out_dtype=torch.uint8)
    want = interp_reference(a.cpu().numpy(), b.cpu().numpy(), fw, tb.cpu().numpy(), times, tm.cpu().numpy(), np.uint8)
    _same_bytes(got, want, "NCHW", "strided views, NCHW, uint8 out")


def test_more_times_than_one_launch_takes():
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 2, 20, 70, 1
    a, b = _frames(B, H, W, C, torch.float64, 9), _frames(B, H, W, C, torch.float64, 10)
    fw, bw = _synthetic(B, H, W, 11)
    times = [(j + 0.5) / 40 for j in range(40)]
    got = interpolate(_dev(list(a)), _dev(list(b)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), times,
                      layout="NHWC")
    _same_bytes(got, interp_reference(a, b, fw, bw, times), "NHWC", "40 times")


def test_sequence_mode_is_pair_mode(gpu):
    """interpolate_video's call (sequence mode, pair i = frames i, i + 1) against interpolate on the same pairs"""
    from papteam_opticalflow_amd.tensors import interpolate, interpolate_video
    v = _dev(_video("240", 4))
    iv = interpolate_video(v, 3, factor=4, layout="NHWC")
    occ = iv.occlusion
    got = interpolate(v[:-1], v[1:], iv.flow_fw, iv.flow_bw, [0.25, 0.5, 0.75], occlusion=occ, layout="NHWC")
    for i in range(3):
        for j in range(3):
            assert torch.equal(iv.video[4 * i + 1 + j], got[i, j]), (i, j)


def test_dense_1080p():
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 1, 1080, 1920, 3
    a, b = _frames(B, H, W, C, torch.uint8, 12), _frames(B, H, W, C, torch.uint8, 13)
    g = torch.Generator().manual_seed(14)
    fw = torch.nn.functional.interpolate(torch.randn(B, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 6,
                                         size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.3 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    occ = _mask(B, H, W, 15)
    got = interpolate(_dev(list(a)), _dev(list(b)), fw.cuda(), bw.cuda(), [0.5], occlusion=torch.from_numpy(occ).cuda(),
                      layout="NHWC")
    _same_bytes(got, interp_reference(a, b, fw.numpy(), bw.numpy(), [0.5], occ, np.uint8), "NHWC", "1080p")


def test_interpolate_video_on_the_committed_video(gpu):
    from papteam_opticalflow_amd.tensors import flow_video_fb, interpolate_video
    v = _dev(_video("240", 5))
    factor = 3
    iv = interpolate_video(v, 4, factor=factor, layout="NHWC")
    assert tuple(iv.video.shape) == (4 * factor + 1, 135, 240, 3) and iv.video.dtype == torch.uint8
    assert torch.equal(iv.video[::factor], v)  # the originals, byte for byte
    fb = flow_video_fb(v, 4, layout="NHWC")
    assert torch.equal(iv.flow_fw, fb.flow_fw) and torch.equal(iv.flow_bw, fb.flow_bw)
    assert torch.equal(iv.occlusion, fb.occlusion)
    n = v.cpu().numpy()
    want = interp_reference(n[:-1], n[1:], fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), [1 / 3, 2 / 3],
                            fb.occlusion.cpu().numpy(), np.uint8)
    got = torch.stack([iv.video[factor * i + 1:factor * i + factor] for i in range(4)])
    _same_bytes(got, want, "NHWC", "interpolate_video")
    # NCHW, float32 out, no mask: originals converted as the kernel converts (x / 255)
    iv2 = interpolate_video(v.permute(0, 3, 1, 2), 4, factor=2, consistency=None, out_dtype=torch.float32)
    assert iv2.occlusion is None and tuple(iv2.video.shape) == (9, 3, 135, 240)
    conv = torch.from_numpy((n.astype(np.float64) / 255.0).astype(np.float32)).permute(0, 3, 1, 2)
    assert np.array_equal(iv2.video[::2].cpu().numpy().view(np.int32), conv.numpy().view(np.int32))
    want = interp_reference(n[:-1], n[1:], fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), [0.5], None, np.float32)
    _same_bytes(iv2.video[1::2].unsqueeze(1), want, "NCHW", "interpolate_video NCHW float32")


def test_interpolate_pairs_is_flow_pairs_fb_and_interpolate(gpu):
    from papteam_opticalflow_amd.tensors import flow_pairs_fb, interpolate, interpolate_pairs
    v = _dev(_video("240", 4))
    ip = interpolate_pairs(v[:2], v[2:], 3, [0.25, 0.75], layout="NHWC", out_dtype=torch.float64)
    fb = flow_pairs_fb(v[:2], v[2:], 3, layout="NHWC")
    assert torch.equal(ip.flow_fw, fb.flow_fw) and torch.equal(ip.occlusion, fb.occlusion)
    want = interpolate(v[:2], v[2:], fb.flow_fw, fb.flow_bw, [0.25, 0.75], occlusion=fb.occlusion, layout="NHWC",
                       out_dtype=torch.float64)
    assert np.array_equal(ip.frames.cpu().numpy().view(np.int64), want.cpu().numpy().view(np.int64))


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames written on a side stream behind a long sleep and interpolated under that stream with no synchronisation: the
    kernel must read them after they are written, and what is queued behind it must see its output"""
    import time
    from papteam_opticalflow_amd.tensors import interpolate
    B, H, W, C = 2, 40, 60, 3
    a, b = _frames(B, H, W, C, torch.uint8, 16), _frames(B, H, W, C, torch.uint8, 17)
    fw, bw = _synthetic(B, H, W, 18)
    occ = _mask(B, H, W, 19)
    want = interp_reference(a, b, fw, bw, [0.25, 0.5], occ, np.uint8)
    src = [_dev(list(a)), _dev(list(b))]
    dst = [torch.zeros_like(s) for s in src]
    tf, tb, tm = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), torch.from_numpy(occ).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = interpolate(dst[0], dst[1], tf, tb, [0.25, 0.5], occlusion=tm, layout="NHWC").clone()
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
        got = interpolate(dst[0], dst[1], tf, tb, [0.25, 0.5], occlusion=tm, layout="NHWC")
        took = time.perf_counter() - t0
        copy = got.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    assert took < 0.25, "interpolate waited for the stream: %.3f s" % took
    _same_bytes(got, want, "NHWC", "side stream")
    _same_bytes(copy, want, "NHWC", "side stream clone")


def test_interpolation_error_on_the_committed_frames(gpu):
    """Frame 2 of the committed 240x135 and 480x270 triples from frames 1 and 3 at t = 0.5, with the device's flows of
    (1, 3) both ways (5 levels) and their occlusion mask: the bytes of the restatement, and a mean absolute error below
    that of the plain blend 0.5 (I1 + I3).  Measured with the oracle's flows (tests/test_interp_cpu.py): 240x135 0.009064
    against 0.009856; 480x270 0.009442 against 0.013774."""
    import cases
    from papteam_opticalflow_amd.tensors import interpolate_pairs
    for res in ("240", "480"):
        f1, f2, f3 = (cases.load_frame_u8(res, i) for i in (1, 2, 3))
        ip = interpolate_pairs(_dev([f1]), _dev([f3]), 5, 0.5, layout="NHWC", out_dtype=torch.float64)
        want = interp_reference(f1[None], f3[None], ip.flow_fw.cpu().numpy(), ip.flow_bw.cpu().numpy(), [0.5],
                                ip.occlusion.cpu().numpy())
        _same_bytes(ip.frames, want, "NHWC", "frame 2 of " + res)
        err = float(np.abs(ip.frames[0, 0].cpu().numpy() - as_f64(f2)).mean())
        blend = float(np.abs(0.5 * (as_f64(f1) + as_f64(f3)) - as_f64(f2)).mean())
        assert err < blend, (res, err, blend)
        assert math.isfinite(err)
