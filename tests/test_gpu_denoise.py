"""Motion-compensated temporal denoising on device tensors (papteam_opticalflow_amd/tensors.py: temporal_filter,
denoise_video -> papof_temporal_filter_tensor).  The device's video and support must be the BYTES of the numpy fp64
restatement (tests/_denoise_ref.py: denoise_reference), compared as raw bytes so that a NaN's payload or a zero's sign is
caught: uint8, float32 and float64 frames, NCHW, NHWC and strided views, float32 and float64 flows, radius 1, 2, 3 and
beyond the video's length, sigma and the consistency check on and off, every output dtype, synthetic flows with NaNs,
infinities and large displacements, two-frame videos, a dense 1080p case; denoise_video's flows against flow_video_fb's,
the caller's stream order, and the PSNR gain on the noisy committed frame triples."""
import math

import numpy as np
import pytest

from _denoise_ref import denoise_reference
from _interp_ref import as_f64, convert
from test_denoise_cpu import GAIN_BOUND, SIGMA, noisy_triple
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd.tensors import CONSISTENCY, denoise_video, flow_video_fb, temporal_filter  # noqa: E402

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
    """got (T, C, H, W) or (T, H, W, C) by layout -- or (T, H, W) with layout None -- against want in (T, H, W, C) / (T, H, W),
    byte for byte"""
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


def _as_layout(n, layout):
    t = _dev(list(n))
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    T, H, W, C = 5, 37, 53, 3
    n = _frames(T, H, W, C, dtype, 1)
    fw, bw = _fields(T, H, W, 2)
    v = _as_layout(n, layout)
    seen = set()
    for fdt in (torch.float64, torch.float32):
        tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
        for radius in (1, 2, 3, T + 1):
            for sigma in (SIGMA, None):
                for cons in (CONSISTENCY, None):
                    want, want_sup = denoise_reference(n, nf, nb, radius, sigma, cons)
                    for odt in (None, torch.uint8, torch.float32, torch.float64):
                        got = temporal_filter(v, tf, tb, radius=radius, sigma=sigma, consistency=cons, layout=layout,
                                              out_dtype=odt)
                        what = "%s %s flows %s R %d sigma %s check %s out %s" % (dtype, layout, fdt, radius, sigma,
                                                                                 cons is not None, odt)
                        _same_bytes(got.video, convert(want, _NP[odt or dtype]), layout, what)
                        _same_bytes(got.support, want_sup, None, what + " support")
                        seen.add(odt or dtype)
    assert len(seen) == 3


def test_branches_are_reached():
    """the synthetic fields above take every branch of the rule: hops that leave the image (NaN, infinite and large flows
    among them), hops that fail the check and hops that pass it, chains cut after a first hop that entered, neighbours
    down-weighted by sigma, and the ends of the video"""
    T, H, W, C = 5, 37, 53, 3
    fw, bw = _fields(T, H, W, 2)
    n = _frames(T, H, W, C, torch.float64, 1)
    x, r = np.arange(W)[None, :] + np.zeros((H, 1)), np.arange(H)[:, None] + np.zeros((1, W))
    from test_track_cpu import _step
    _, _, inside = _step(fw[0], bw[0], x.ravel(), r.ravel(), np.ones(H * W, bool), False, 0, 0)
    _, _, checked = _step(fw[0], bw[0], x.ravel(), r.ravel(), np.ones(H * W, bool), True, *CONSISTENCY)
    assert (~inside).any() and (inside & ~checked).any() and checked.any()
    assert (~np.isfinite(fw[0])).any(axis=0).any() and (np.abs(fw[0]) > W / 4).any()
    _, sup = denoise_reference(n, fw, bw, 3, SIGMA, CONSISTENCY)
    full = np.array([min(3, T - 1 - t) + min(3, t) for t in range(T)])[:, None, None]
    assert (sup == full).any() and (sup == 0).any() and ((sup > 0) & (sup < full)).any()
    assert len(set(full.ravel().tolist())) > 1  # the ends of the video hold fewer neighbours
    # photometric weights strictly between 0 and 1 (random frames): the sigma output differs from the unweighted one
    a, _ = denoise_reference(n, fw, bw, 3, SIGMA, CONSISTENCY)
    b, _ = denoise_reference(n, fw, bw, 3, None, CONSISTENCY)
    assert ((a != b) & (sup[..., None] > 0)).any()


@pytest.mark.parametrize("radius", [1, 3])
def test_two_frames(radius):
    T, H, W, C = 2, 30, 70, 2
    n = _frames(T, H, W, C, torch.float32, 3)
    fw, bw = _fields(T, H, W, 4)
    got = temporal_filter(_as_layout(n, "NHWC"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), radius=radius,
                          layout="NHWC")
    want, sup = denoise_reference(n, fw, bw, radius, SIGMA, CONSISTENCY, np.float32)
    _same_bytes(got.video, want, "NHWC", "T = 2")
    _same_bytes(got.support, sup, None, "T = 2 support")
    assert got.video.dtype == torch.float32 and got.support.dtype == torch.uint8


def test_strided_views_and_one_channel():
    T, H, W, C = 4, 29, 41, 3
    fw, bw = _fields(T, H, W, 5)
    big = torch.from_numpy(_frames(2 * T, H + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    # flows as (T - 1, H, W, 2) channels-last, read as (T - 1, 2, H, W), and float32 backward flows
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    tb = torch.from_numpy(bw).float().cuda()
    n = v.cpu().numpy()
    want, sup = denoise_reference(n, fw, tb.cpu().numpy(), 2, SIGMA, CONSISTENCY, np.float64)
    got = temporal_filter(v, tf, tb, layout="NHWC", out_dtype=torch.float64)
    _same_bytes(got.video, want, "NHWC", "strided NHWC")
    _same_bytes(got.support, sup, None, "strided NHWC support")
    got = temporal_filter(v.permute(0, 3, 1, 2), tf, tb)  # the same view as NCHW, uint8 out
    assert got.video.shape == (T, C, H, W)
    _same_bytes(got.video, convert(want, np.uint8), "NCHW", "strided NCHW")
    # one channel of a float64 video, picked from NCHW
    w64 = torch.from_numpy(_frames(T, H, W, 3, torch.float64, 7)).cuda().permute(0, 3, 1, 2)[:, 1:2]
    got = temporal_filter(w64, tf, tb, radius=3, sigma=None)
    want, sup = denoise_reference(w64.permute(0, 2, 3, 1).cpu().numpy(), fw, tb.cpu().numpy(), 3, None, CONSISTENCY)
    _same_bytes(got.video, want, "NCHW", "one channel")
    _same_bytes(got.support, sup, None, "one channel support")


def test_four_channels_float32_frames_float64_out():
    T, H, W, C = 3, 20, 66, 4
    n = _frames(T, H, W, C, torch.float32, 8)
    fw, bw = _fields(T, H, W, 9)
    got = temporal_filter(_as_layout(n, "NCHW"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), radius=2,
                          sigma=0.05, consistency=(0.05, 1.0), out_dtype=torch.float64)
    want, sup = denoise_reference(n, fw, bw, 2, 0.05, (0.05, 1.0))
    _same_bytes(got.video, want, "NCHW", "C = 4")
    _same_bytes(got.support, sup, None, "C = 4 support")


def test_dense_1080p():
    T, H, W, C = 3, 1080, 1920, 3
    n = _frames(T, H, W, C, torch.uint8, 10)
    g = torch.Generator().manual_seed(11)
    fw = torch.nn.functional.interpolate(torch.randn(T - 1, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 6,
                                         size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.3 * torch.randn(T - 1, 2, H, W, generator=g, dtype=torch.float64)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    got = temporal_filter(_as_layout(n, "NHWC"), fw.cuda(), bw.cuda(), radius=2, layout="NHWC")
    want, sup = denoise_reference(n, fw.numpy(), bw.numpy(), 2, SIGMA, CONSISTENCY, np.uint8)
    _same_bytes(got.video, want, "NHWC", "1080p")
    _same_bytes(got.support, sup, None, "1080p support")


def test_denoise_video_is_flow_video_fb_and_temporal_filter():
    from test_gpu_batch import _video
    v = _dev(_video("240", 5))
    dv = denoise_video(v, 4, radius=2, layout="NHWC")
    fb = flow_video_fb(v, 4, layout="NHWC", consistency=None)
    assert torch.equal(dv.flow_fw, fb.flow_fw) and torch.equal(dv.flow_bw, fb.flow_bw)
    assert dv.flow_fw.dtype == torch.float64 and sorted(dv.timing) == sorted(fb.timing)
    tf = temporal_filter(v, fb.flow_fw, fb.flow_bw, radius=2, layout="NHWC")
    assert torch.equal(dv.video, tf.video) and torch.equal(dv.support, tf.support)
    n = v.cpu().numpy()
    want, sup = denoise_reference(n, fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 2, SIGMA, CONSISTENCY, np.uint8)
    _same_bytes(dv.video, want, "NHWC", "denoise_video")
    _same_bytes(dv.support, sup, None, "denoise_video support")
    # NCHW, float32 out, no check, no photometric weight
    dv2 = denoise_video(v.permute(0, 3, 1, 2), 4, radius=1, sigma=None, consistency=None, out_dtype=torch.float32)
    assert torch.equal(dv2.flow_fw, fb.flow_fw)
    want, sup = denoise_reference(n, fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 1, None, None, np.float32)
    _same_bytes(dv2.video, want, "NCHW", "denoise_video NCHW float32")
    _same_bytes(dv2.support, sup, None, "denoise_video NCHW support")


def test_psnr_gain_on_the_noisy_committed_frames():
    """Frames 1 .. 3 of the committed 240x135 and 480x270 triples with the seeded noise of tests/test_denoise_cpu.py,
    denoise_video with radius 1 and the defaults (the device's flows, 5 levels): the bytes of the restatement on those
    flows, and a PSNR gain of the middle frame above the bound calibrated there with the oracle's flows (+4.06 dB and
    +4.04 dB measured, 3.5 dB asserted)."""
    for res in ("240", "480"):
        clean, noisy = noisy_triple(res)
        dv = denoise_video(_dev(list(noisy)), 5, radius=1, layout="NHWC", out_dtype=torch.float64)
        want, sup = denoise_reference(noisy, dv.flow_fw.cpu().numpy(), dv.flow_bw.cpu().numpy(), 1, SIGMA, CONSISTENCY)
        _same_bytes(dv.video, want, "NHWC", "noisy " + res)
        _same_bytes(dv.support, sup, None, "noisy support " + res)
        c = as_f64(clean[1])
        mse = lambda a: float(np.mean((a - c) ** 2))  # noqa: E731
        gain = 10.0 * math.log10(mse(as_f64(noisy[1])) / mse(dv.video[1].cpu().numpy()))
        assert gain > GAIN_BOUND, (res, gain)


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames written on a side stream behind a long sleep and filtered under that stream with no synchronisation: the
    kernel must read them after they are written, and what is queued behind it must see its output"""
    import time
    T, H, W, C = 4, 40, 60, 3
    n = _frames(T, H, W, C, torch.uint8, 12)
    fw, bw = _fields(T, H, W, 13)
    want, sup = denoise_reference(n, fw, bw, 2, SIGMA, CONSISTENCY, np.uint8)
    src = _dev(list(n))
    dst = torch.zeros_like(src)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = temporal_filter(dst, tf, tb, layout="NHWC").video.clone()
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the call
        dst.copy_(src)
        got = temporal_filter(dst, tf, tb, layout="NHWC")
        copy = got.video.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    _same_bytes(got.video, want, "NHWC", "side stream")
    _same_bytes(copy, want, "NHWC", "side stream clone")
    _same_bytes(got.support, sup, None, "side stream support")
