"""Multi-frame super-resolution on device tensors (papteam_opticalflow_amd/tensors.py: super_resolve, super_resolve_video ->
papof_super_resolve_tensor).  The device's video and coverage must be the BYTES of the numpy restatement
(tests/_superres_ref.py), compared as raw bytes: uint8, float32 and float64 frames, NCHW, NHWC, sliced and permuted views,
one and three channels, scales 2, 3 and 4, radii 0, 1 and 3, one frame, with and without the photometric weight and the
check, with and without back-projection, real flows of the committed video and synthetic flows with NaNs, infinities and
landings outside the image, ragged sizes; two runs of a 960x540 video give the same bytes; every grouping of the targets
gives the same bytes; super_resolve_video is flow_video_fb followed by super_resolve; the caller's stream order.
The largest allocation is test_twice_the_same_bytes_at_960x540's workspace: 6 targets x 8 x 4 x 540 x 960 x (4 + 6) bytes =
995 MB, beside 100 MB of coverage."""
import numpy as np
import pytest

from _superres_ref import superres_reference
from test_gpu_batch import _video
from test_gpu_interp import _frames, _same_bytes
from test_gpu_splat import _same_coverage
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}
CONSISTENCY = (0.01, 0.5)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same(got, want, cov, layout, what):
    """got: SuperResolved in `layout`; want (T, S H, S W, C), cov (T, S H, S W) of the restatement"""
    _same_bytes(got.video.unsqueeze(1), want[:, None], layout, what)
    _same_coverage(got.coverage, cov, what)


def _in(x, layout):
    return _dev(list(x)) if layout == "NHWC" else _dev(list(x)).permute(0, 3, 1, 2)


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    from papteam_opticalflow_amd.tensors import super_resolve
    T, H, W, C, S = 4, 37, 53, 3, 2
    x = _frames(T, H, W, C, dtype, 1)
    fw, bw = _fields(T, H, W, 3)
    assert np.isnan(fw).any() and np.isinf(bw).any()
    tx = _in(x, layout)
    outs = [None, torch.uint8, torch.float32, torch.float64]
    n = 0
    for fdt in (torch.float64, torch.float32):
        tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
        for sigma, cons in ((0.15, CONSISTENCY), (None, None), (0.05, None)):
            for iters in (0, 2):
                odt = outs[n % 4]
                n += 1
                got = super_resolve(tx, tf, tb, S, sigma=sigma, consistency=cons, iters=iters, layout=layout, out_dtype=odt)
                want, cov = superres_reference(x, nf, nb, S, sigma=sigma, consistency=cons, iters=iters,
                                               out_dtype=_NP[odt or dtype])
                _same(got, want, cov, layout, "%s %s flows %s sigma %s check %s iters %d out %s" % (dtype, layout, fdt, sigma,
                                                                                                   cons, iters, odt))
    # the check and the weight both act on these fields
    _, plain = superres_reference(x, fw, bw, S, sigma=None, consistency=None, iters=0)
    _, checked = superres_reference(x, fw, bw, S, sigma=None, consistency=CONSISTENCY, iters=0)
    assert checked.sum() < plain.sum()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("R", [0, 1, 3])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_scales_radii_and_channels(S, R, C):
    from papteam_opticalflow_amd.tensors import super_resolve
    T, H, W = 5, 23, 31
    x = _frames(T, H, W, C, torch.float64, 10 + S)
    fw, bw = _fields(T, H, W, 20 + R, wild=(R != 1))
    got = super_resolve(_in(x, "NCHW"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), S, radius=R, prior=0.2)
    want, cov = superres_reference(x, fw, bw, S, radius=R, prior=0.2)
    _same(got, want, cov, "NCHW", "scale %d radius %d channels %d" % (S, R, C))
    if R == 0 and S > 2:
        assert (cov == 0).any()  # pixels that are the prior's alone


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float64])
def test_one_frame(dtype):
    from papteam_opticalflow_amd.tensors import super_resolve
    H, W, C = 19, 27, 4
    x = _frames(1, H, W, C, dtype, 30)
    for S, iters in ((2, 0), (3, 2), (4, 1)):
        empty = torch.zeros((0, 2, H, W), dtype=torch.float64, device="cuda")
        got = super_resolve(_in(x, "NHWC"), empty, empty, S, iters=iters, layout="NHWC")
        want, cov = superres_reference(x, np.zeros((0, 2, H, W)), np.zeros((0, 2, H, W)), S, iters=iters)
        _same(got, want, cov, "NHWC", "one frame, scale %d, iters %d" % (S, iters))


def test_sliced_and_permuted_views():
    from papteam_opticalflow_amd.tensors import super_resolve
    T, H, W, S = 3, 21, 29, 2
    rng = np.random.default_rng(31)
    big = torch.from_numpy(rng.random((2 * T, H + 3, 2 * W, 4))).cuda()
    x = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    fw, bw = _fields(T, H, W, 32)
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)  # channels-last flows
    tb = torch.from_numpy(bw).cuda()
    assert not x.is_contiguous() and not tf.is_contiguous()
    got = super_resolve(x, tf, tb, S, layout="NHWC")
    want, cov = superres_reference(x.cpu().numpy(), fw, bw, S)
    _same(got, want, cov, "NHWC", "sliced views")
    # the same frames as a permuted NCHW view, one frame repeated by a zero stride
    rep = big[:1, 2:H + 2, ::2, 1:].expand(T, H, W, 3).permute(0, 3, 1, 2)
    got = super_resolve(rep, tf, tb, S, iters=1, out_dtype=torch.float32)
    want, cov = superres_reference(rep.permute(0, 2, 3, 1).cpu().numpy(), fw, bw, S, iters=1, out_dtype=np.float32)
    _same(got, want, cov, "NCHW", "expanded view")


@pytest.mark.parametrize("H,W", [(1, 9), (9, 1), (65, 5), (8, 16), (9, 17)])
def test_ragged_sizes(H, W):
    from papteam_opticalflow_amd.tensors import super_resolve
    T, C = 3, 2
    x = _frames(T, H, W, C, torch.uint8, 40)
    fw, bw = _fields(T, H, W, 41, amp=0.7, wild=False)
    for S in (2, 3, 4):
        got = super_resolve(_in(x, "NHWC"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), S, layout="NHWC",
                            out_dtype=torch.float64)
        want, cov = superres_reference(x, fw, bw, S, out_dtype=np.float64)
        _same(got, want, cov, "NHWC", "%d x %d scale %d" % (H, W, S))


def test_real_flows_and_the_video_call(gpu):
    """super_resolve on flow_video_fb's flows equals the restatement, and super_resolve_video is the two calls in a row"""
    from papteam_opticalflow_amd.tensors import flow_video_fb, super_resolve, super_resolve_video
    v = _dev(_video("240", 4))
    fb = flow_video_fb(v, 4, layout="NHWC", consistency=None)
    got = super_resolve(v, fb.flow_fw, fb.flow_bw, 2, layout="NHWC")
    assert got.video.dtype == torch.uint8 and tuple(got.video.shape) == (4, 270, 480, 3)
    want, cov = superres_reference(v.cpu().numpy(), fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 2)
    _same(got, want, cov, "NHWC", "real flows")
    sv = super_resolve_video(v, 4, 2, layout="NHWC")
    assert torch.equal(sv.flow_fw, fb.flow_fw) and torch.equal(sv.flow_bw, fb.flow_bw) and sv.timing is not None
    assert torch.equal(sv.video, got.video) and torch.equal(sv.coverage.view(torch.int64), got.coverage.view(torch.int64))
    given = super_resolve_video(v.permute(0, 3, 1, 2), 4, 3, flows=(fb.flow_fw, fb.flow_bw), iters=0, out_dtype=torch.float32)
    assert given.timing is None
    want, cov = superres_reference(v.cpu().numpy(), fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 3, iters=0,
                                   out_dtype=np.float32)
    _same(given, want, cov, "NCHW", "given flows, scale 3")


def _one_target_bytes(T, H, W, C, S, iters):
    return 8 * S * S * H * W * ((C + 1) + (2 * C if iters else 0))


@pytest.mark.parametrize("iters", [0, 2])
def test_every_grouping_of_the_targets_gives_the_same_bytes(gpu, monkeypatch, iters):
    """a workspace of one, two or three target frames against the whole workspace and the restatement: the rounds re-walk
    the chains of the frames they share and must deposit each term once"""
    from papteam_opticalflow_amd.tensors import super_resolve
    T, H, W, C, S, R = 5, 33, 47, 3, 2, 3
    x = _frames(T, H, W, C, torch.uint8, 50)
    fw, bw = _fields(T, H, W, 51)
    tx, tf, tb = _in(x, "NHWC"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    want, cov = superres_reference(x, fw, bw, S, radius=R, iters=iters)
    per = _one_target_bytes(T, H, W, C, S, iters)
    assert gpu.L.papof_sr_workspace(T, H, W, C, S, iters) == T * per
    _same(super_resolve(tx, tf, tb, S, radius=R, iters=iters, layout="NHWC"), want, cov, "NHWC", "whole workspace")
    for g in (1, 2, 3):
        monkeypatch.setattr(gpu.L, "papof_sr_workspace", lambda *a, g=g: g * per + 8)  # (a remainder that is no target's)
        got = super_resolve(tx, tf, tb, S, radius=R, iters=iters, layout="NHWC")
        monkeypatch.undo()
        _same(got, want, cov, "NHWC", "rounds of %d targets" % g)


def _smooth(T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    fw = torch.nn.functional.interpolate(torch.randn(T - 1, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 3,
                                         size=(H, W), mode="bilinear", align_corners=False)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    return fw, -fw + 0.05 * torch.randn(fw.shape, generator=g, dtype=torch.float64)


def test_twice_the_same_bytes_at_960x540(gpu, monkeypatch):
    """960x540 -> 1920x1080, six frames: about 62 million atomic adds per target in whatever order the hardware takes
    them, twice, and once more in rounds of two targets"""
    from papteam_opticalflow_amd.tensors import super_resolve
    T, H, W, C = 6, 540, 960, 3
    tx = _dev(list(_frames(T, H, W, C, torch.uint8, 60)))
    fw, bw = _smooth(T, H, W, 61)
    tf, tb = fw.cuda(), bw.cuda()
    one = super_resolve(tx, tf, tb, 2, layout="NHWC")
    two = super_resolve(tx, tf, tb, 2, layout="NHWC")
    assert torch.equal(one.video, two.video) and torch.equal(one.coverage.view(torch.int64), two.coverage.view(torch.int64))
    assert float(one.coverage.max()) > 2.0 and float(one.coverage[:, :60, :60].max()) < 1.5  # chains arrive; the corner's do not
    monkeypatch.setattr(gpu.L, "papof_sr_workspace", lambda *a: 2 * _one_target_bytes(T, H, W, C, 2, 2))
    three = super_resolve(tx, tf, tb, 2, layout="NHWC")
    monkeypatch.undo()
    assert torch.equal(one.video, three.video) and torch.equal(one.coverage.view(torch.int64), three.coverage.view(torch.int64))


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames written on a side stream behind a long sleep and super-resolved under that stream with no synchronisation:
    the clear, the adds, the resolve and the back-projection must follow the writes, and what is queued behind them must see
    their output; the call itself returns while the stream still sleeps"""
    import time
    from papteam_opticalflow_amd.tensors import super_resolve
    T, H, W, C, S = 3, 40, 60, 3, 2
    x = _frames(T, H, W, C, torch.uint8, 70)
    fw, bw = _fields(T, H, W, 71)
    want, cov = superres_reference(x, fw, bw, S)
    src = _dev(list(x))
    dst = torch.zeros_like(src)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = super_resolve(dst, tf, tb, S, layout="NHWC").video.clone()
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
        got = super_resolve(dst, tf, tb, S, layout="NHWC")
        took = time.perf_counter() - t0
        copy = got.video.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    assert took < 0.25, "the call waited for the stream: %.3f s" % took
    _same(got, want, cov, "NHWC", "side stream")
    _same_bytes(copy.unsqueeze(1), want[:, None], "NHWC", "side stream clone")
