"""Blind video temporal consistency on device tensors (papteam_opticalflow_amd/tensors.py: temporal_consistency,
consistent_video -> papof_temporal_consistency_tensor).  The device's output must be the BYTES of the numpy fp64
restatement (tests/_consistency_ref.py), compared as raw bytes: uint8, float32 and float64 frames, processed and out, NCHW,
NHWC and strided views, C_I != C_P, the check on and off, sigma 0, lambda 0, `first`, T = 2, 1 x 1, 1 x W, H x 1 and 1080p
frames, wild flows; the same bytes for every PAPOF_TC_DEPTH, chunked calls equal to one call, consistent_video equal to
flow_video_fb followed by temporal_consistency, and the caller's stream order."""
import os

import numpy as np
import pytest

from _consistency_ref import consistency_reference
from _interp_ref import convert
from test_gpu_inpaint import _NP, _as_layout, _frames, _same_bytes
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd.tensors import (CONSISTENCY, consistent_video, flow_video_fb,  # noqa: E402
                                             temporal_consistency)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _video(T, H, W, CI, CP, dt_i, dt_p, seed, wild=True):
    """frames, processed (a flickering function of the frames plus noise) and flows: numpy arrays"""
    I = _frames(T, H, W, CI, dt_i, seed)
    rng = np.random.default_rng(seed + 1)
    base = I.astype(np.float64) / (255.0 if dt_i == torch.uint8 else 1.0)
    base = base.mean(-1, keepdims=True) if CP != CI else base
    base = np.broadcast_to(base, (T, H, W, CP))
    P = rng.uniform(0.8, 1.2, (T, 1, 1, CP)) * base + rng.uniform(-0.1, 0.1, (T, 1, 1, CP))
    P = P + 0.02 * rng.random(P.shape)
    P = convert(np.clip(P, 0, 1), np.uint8) if dt_p == torch.uint8 else P.astype(_NP[dt_p])
    fw, bw = _fields(T, H, W, seed + 2, wild=wild and H > 8 and W > 8)
    return I, P, fw, bw


def _run(I, P, fw, bw, layout="NHWC", **kw):
    return temporal_consistency(_as_layout(I, layout), _as_layout(P, layout), torch.from_numpy(fw).cuda(),
                                torch.from_numpy(bw).cuda(), layout=layout, **kw)


@pytest.mark.parametrize("dt_p", [torch.uint8, torch.float32, torch.float64])
@pytest.mark.parametrize("dt_i", [torch.uint8, torch.float32, torch.float64])
def test_every_dtype_of_frames_processed_and_out(dt_i, dt_p):
    I, P, fw, bw = _video(4, 29, 71, 3, 3, dt_i, dt_p, 10)
    for odt in (None, torch.uint8, torch.float32, torch.float64):
        want = consistency_reference(I, P, fw, bw, 4.0, 0.05, 7, CONSISTENCY, out_dtype=_NP[odt or dt_p])
        got = _run(I, P, fw, bw, lam=4.0, sigma=0.05, iters=7, out_dtype=odt)
        _same_bytes(got, want, "NHWC", "frames %s processed %s out %s" % (dt_i, dt_p, odt))


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
def test_layouts_channels_check_sigma_and_first(layout):
    T, H, W = 5, 37, 90
    for CI, CP in ((1, 3), (3, 1), (4, 2), (2, 4)):
        I, P, fw, bw = _video(T, H, W, CI, CP, torch.float32, torch.float64, 20 + CI)
        first = np.random.default_rng(CI).random((H, W, CP))
        for lam, sigma, iters, cons in ((4.0, 0.05, 20, CONSISTENCY), (1.0, 0.0, 3, None), (0.5, 0.2, 0, CONSISTENCY)):
            for f in (None, first):
                want = consistency_reference(I, P, fw, bw, lam, sigma, iters, cons, first=f)
                tf = None if f is None else (torch.from_numpy(f).cuda() if layout == "NHWC"
                                             else torch.from_numpy(f).cuda().permute(2, 0, 1))
                got = _run(I, P, fw, bw, layout, lam=lam, sigma=sigma, iters=iters, consistency=cons, first=tf)
                what = "%s C %d -> %d lam %g sigma %g iters %d check %s first %s" % (layout, CI, CP, lam, sigma, iters,
                                                                                   cons is not None, f is not None)
                _same_bytes(got, want, layout, what)


@pytest.mark.parametrize("dt_p", [torch.uint8, torch.float32, torch.float64])
def test_lambda_zero_gives_processed_back(dt_p):
    I, P, fw, bw = _video(4, 33, 47, 3, 3, torch.uint8, dt_p, 30)
    for odt in (None, torch.uint8, torch.float32, torch.float64):
        got = _run(I, P, fw, bw, lam=0.0, iters=9, out_dtype=odt)
        want = convert(P.astype(np.float64) / (255.0 if dt_p == torch.uint8 else 1.0), _NP[odt or dt_p])
        _same_bytes(got, want, "NHWC", "lam 0 processed %s out %s" % (dt_p, odt))
        if odt is None:
            assert got.cpu().numpy().tobytes() == P.tobytes()


def test_strided_views():
    big_i = torch.from_numpy(_frames(8, 70, 150, 4, torch.uint8, 40)).cuda()
    big_p = torch.from_numpy(_frames(8, 70, 150, 4, torch.float32, 41)).cuda()
    vi = big_i[::2, 3:68, 1::2, :3]  # every other frame, rows cut, every other column, channels cut: (4, 65, 75, 3)
    vp = big_p[1::2, 2:67, ::2, 1:3]
    assert not vi.is_contiguous() and not vp.is_contiguous() and vi.shape[:3] == vp.shape[:3]
    T, H, W = vi.shape[:3]
    fw, bw = _fields(T, H, W, 42)
    tfw = torch.from_numpy(np.ascontiguousarray(np.swapaxes(fw, 2, 3))).cuda().transpose(2, 3)  # strided flows
    bw32 = bw.astype(np.float32)
    tbw = torch.from_numpy(bw32).cuda()
    ni, np_ = vi.cpu().numpy(), vp.cpu().numpy()
    want = consistency_reference(ni, np_, fw, bw32, 4.0, 0.05, 11, CONSISTENCY)
    got = temporal_consistency(vi, vp, tfw, tbw, layout="NHWC", iters=11)
    _same_bytes(got, want, "NHWC", "strided NHWC")
    want8 = consistency_reference(ni, np_, fw, bw32, 4.0, 0.05, 11, CONSISTENCY, out_dtype=np.uint8)
    got = temporal_consistency(vi.permute(0, 3, 1, 2), vp.permute(0, 3, 1, 2), tfw, tbw, iters=11, out_dtype=torch.uint8)
    _same_bytes(got, want8, "NCHW", "strided NCHW")


@pytest.mark.parametrize("shape", [(1, 1), (1, 90), (90, 1), (2, 3), (135, 240)])
def test_shapes_and_two_frames(shape):
    H, W = shape
    for T in (2, 4):
        I, P, fw, bw = _video(T, H, W, 3, 3, torch.uint8, torch.float64, 50 + H + T)
        for lam, sigma, iters in ((4.0, 0.05, 20), (2.0, 0.0, 33), (0.0, 0.1, 2)):
            want = consistency_reference(I, P, fw, bw, lam, sigma, iters, CONSISTENCY)
            _same_bytes(_run(I, P, fw, bw, lam=lam, sigma=sigma, iters=iters), want, "NHWC",
                        "%s T %d lam %g iters %d" % (shape, T, lam, iters))


def test_1080p():
    T, H, W = 3, 1080, 1920
    I, P, fw, bw = _video(T, H, W, 3, 3, torch.uint8, torch.uint8, 60, wild=False)
    want = consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CONSISTENCY)
    _same_bytes(_run(I, P, fw, bw), want, "NHWC", "1080p")


def test_the_depth_does_not_change_the_bits(monkeypatch):
    I, P, fw, bw = _video(4, 135, 240, 3, 3, torch.uint8, torch.float64, 70)
    want = consistency_reference(I, P, fw, bw, 4.0, 0.05, 37, CONSISTENCY)
    for depth in (None, "1", "2", "15"):
        if depth is None:
            monkeypatch.delenv("PAPOF_TC_DEPTH", raising=False)
        else:
            monkeypatch.setenv("PAPOF_TC_DEPTH", depth)
        _same_bytes(_run(I, P, fw, bw, iters=37), want, "NHWC", "PAPOF_TC_DEPTH %s" % depth)


@pytest.mark.parametrize("odt", [torch.uint8, torch.float32])
def test_chunks_overlapping_by_one_frame_equal_one_call(odt):
    T, H, W = 9, 60, 110
    I, P, fw, bw = _video(T, H, W, 3, 3, torch.uint8, torch.float32, 80)
    ti, tp = _as_layout(I, "NCHW"), _as_layout(P, "NCHW")
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    whole = temporal_consistency(ti, tp, tf, tb, out_dtype=odt)
    parts, first = [], None
    for a, b in ((0, 4), (3, 7), (6, 9)):  # frames a .. b - 1: each chunk shares its first frame with the previous one
        o = temporal_consistency(ti[a:b], tp[a:b], tf[a:b - 1], tb[a:b - 1], first=first, out_dtype=odt)
        parts.append(o if a == 0 else o[1:])
        first = o[-1]
    chunked = torch.cat(parts)
    assert chunked.shape == whole.shape and torch.equal(chunked, whole)
    _same_bytes(whole, consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CONSISTENCY, out_dtype=_NP[odt]), "NCHW",
                "one call")


def test_consistent_video_is_flow_video_fb_then_temporal_consistency():
    import cases
    img = cases.load_frame_u8("1920", 1)
    T, H, W = 5, 64, 112
    frames = np.stack([img[300 + t:300 + t + H, 800 + 2 * t:800 + 2 * t + W] for t in range(T)])
    rng = np.random.default_rng(90)
    P = rng.uniform(0.8, 1.2, (T, 1, 1, 3)) * (frames / 255.0) + rng.uniform(-0.1, 0.1, (T, 1, 1, 3))
    v, tp = _dev(list(frames)), torch.from_numpy(P).cuda()
    cv = consistent_video(v, tp, 3, layout="NHWC")
    fb = flow_video_fb(v, 3, layout="NHWC", consistency=None)
    assert torch.equal(cv.flow_fw, fb.flow_fw) and torch.equal(cv.flow_bw, fb.flow_bw)
    direct = temporal_consistency(v, tp, fb.flow_fw, fb.flow_bw, layout="NHWC")
    assert torch.equal(cv.video, direct)
    want = consistency_reference(frames, P, fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 4.0, 0.05, 20, CONSISTENCY)
    _same_bytes(cv.video, want, "NHWC", "consistent_video")
    given = consistent_video(v, tp, 3, flows=(fb.flow_fw, fb.flow_bw), layout="NHWC", out_dtype=torch.float32)
    direct32 = temporal_consistency(v, tp, fb.flow_fw, fb.flow_bw, layout="NHWC", out_dtype=torch.float32)
    assert given.timing is None and torch.equal(given.video, direct32)
    assert cv.video.dtype == torch.float64 and cv.timing is not None


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames written on a side stream behind a long sleep and used under that stream with no synchronisation: the
    kernels must read them after they are written; a reused workspace block is not overwritten early; two runs are
    bitwise equal."""
    import time
    T, H, W = 5, 70, 130
    I, P, fw, bw = _video(T, H, W, 3, 3, torch.uint8, torch.uint8, 100)
    want = consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CONSISTENCY)
    si, sp = _dev(list(I)), _dev(list(P))
    di, dp = torch.zeros_like(si), torch.zeros_like(sp)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        temporal_consistency(di, dp, tf, tb, layout="NHWC")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        di.copy_(si)
        dp.copy_(sp)
        a = temporal_consistency(di, dp, tf, tb, layout="NHWC")
        b = temporal_consistency(di, dp, tf, tb, layout="NHWC")  # the first call's workspace block, reused behind it
        copy = b.clone()
    side.synchronize()
    for got, what in ((a, "first"), (b, "second"), (copy, "clone")):
        _same_bytes(got, want, "NHWC", "side stream " + what)
    assert os.environ.get("PAPOF_TC_DEPTH") is None
