"""Flow on PyTorch device tensors (papteam_opticalflow_amd/tensors.py -> papof_flow_batch_tensor): every pair must come back
with the BITS of the single host call on the fp64 values of its frames -- for uint8, float32 and float64 frames, NCHW and
NHWC, views that are read in place, what the batched chain does not cover, the guard's re-run, sub-batches, float32 outputs
-- and the call must be ordered behind the caller's stream.  Bits are compared as integer views, so that a flipped sign of a
zero is caught.  One handle (the module's own, tensors._handle) serves the tensor calls and the reference single calls."""
import numpy as np
import pytest

from test_gpu_batch import _video

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


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    iv = np.int64 if g.dtype == np.float64 else np.int32
    if not np.array_equal(g.view(iv), w.view(iv)):
        raise AssertionError("%s: %d elements differ, max-abs %.3e" % (what, int((g.view(iv) != w.view(iv)).sum()),
                                                                        float(np.abs(g.astype(np.float64) - w).max())))


def _check_pairs(flow, warp, layout, singles, what):
    """flow (B, 2, H, W), warp in `layout` against [(vx, vy, warpI2 HWC)] of the single calls"""
    assert flow.shape[0] == len(singles)
    for i, (vx, vy, wi) in enumerate(singles):
        _same_bits(flow[i, 0], vx, "%s pair %d vx" % (what, i))
        _same_bits(flow[i, 1], vy, "%s pair %d vy" % (what, i))
        w = warp[i].permute(1, 2, 0) if layout == "NCHW" else warp[i]
        _same_bits(w, wi, "%s pair %d warpI2" % (what, i))


def _dev(frames):
    return torch.from_numpy(np.stack(frames)).cuda()


@pytest.fixture(scope="module")
def video17(gpu):
    """the 240x135 video of 17 frames (uint8 HWC) and the single calls on its 16 pairs, 5 levels"""
    v = _video("240", 17)
    return v, [gpu.coarse2fine_flow_u8(v[i], v[i + 1], 5)[:3] for i in range(16)]


def test_video_of_uint8_nhwc_frames(video17):
    from papteam_opticalflow_amd.tensors import flow_video
    v, singles = video17
    flow, warp, t = flow_video(_dev(v), 5, layout="NHWC")
    assert flow.shape == (16, 2, 135, 240) and warp.shape == (16, 135, 240, 3) and flow.dtype == torch.float64
    assert not flow.requires_grad and float(t["Total C++ Execution"]) > 0 and float(t["Phase5_SOR"]) > 0
    _check_pairs(flow, warp, "NHWC", singles, "video")


def test_independent_pairs_float32_nchw_and_float64_nhwc(gpu):
    from papteam_opticalflow_amd import default_params
    from papteam_opticalflow_amd.tensors import flow_pairs
    kw = dict(n_outer=3, n_outer_per_level=0, n_sor=30, n_sor_per_level=0)  # config-4 schedule
    P = default_params(**kw)
    v = np.stack(_video("480", 8))
    f32 = torch.from_numpy(v).float() / 255  # float32 samples: the call widens them exactly
    a, b = f32[0::2].permute(0, 3, 1, 2).contiguous().cuda(), f32[1::2].permute(0, 3, 1, 2).contiguous().cuda()
    flow, warp, _ = flow_pairs(a, b, 5, layout="NCHW", **kw)
    assert warp.shape == (4, 3, 270, 480)
    singles = [gpu.coarse2fine_flow(f32[2 * i].double().numpy(), f32[2 * i + 1].double().numpy(), 5, P)[:3] for i in range(4)]
    _check_pairs(flow, warp, "NCHW", singles, "float32 NCHW")
    f64 = np.roll(v, 5, axis=2).astype(np.float64) / 255.0
    flow, warp, _ = flow_pairs(torch.from_numpy(f64[1::2]).cuda(), torch.from_numpy(f64[0::2]).cuda(), 5, layout="NHWC", **kw)
    singles = [gpu.coarse2fine_flow(f64[2 * i + 1], f64[2 * i], 5, P)[:3] for i in range(4)]
    _check_pairs(flow, warp, "NHWC", singles, "float64 NHWC")


def _same_run(got, want, what):
    for name, g, w in zip(("flow", "warpI2"), got[:2], want[:2]):
        _same_bits(g, w, "%s %s" % (what, name))


def test_views_are_read_in_place():
    from papteam_opticalflow_amd.tensors import flow_video
    frames = _dev(_video("240", 9))  # (T, H, W, C) uint8
    sl = frames[::2]
    _same_run(flow_video(sl, 3, layout="NHWC"), flow_video(sl.contiguous(), 3, layout="NHWC"), "frame slice")
    nchw = frames[:4].permute(0, 3, 1, 2)  # NCHW view of NHWC storage
    _same_run(flow_video(nchw, 3, layout="NCHW"), flow_video(nchw.contiguous(), 3, layout="NCHW"), "permuted view")
    gray = frames[:4, 7:108, 11:184, 1:2]  # gray crop of odd size, 101 x 173
    assert gray.shape == (4, 101, 173, 1) and not gray.is_contiguous()
    _same_run(flow_video(gray, 3, layout="NHWC"), flow_video(gray.contiguous(), 3, layout="NHWC"), "gray crop")


@pytest.mark.parametrize("what,kw,C", [
    ("red-black", dict(sor_mode=1), 3),
    ("bicubic", dict(interpolation=1), 3),
    ("two channels", {}, 2),
])
def test_what_the_batched_chain_does_not_cover(gpu, what, kw, C):
    from papteam_opticalflow_amd import default_params
    from papteam_opticalflow_amd.tensors import flow_pairs
    v = np.stack(_video("240", 4))[..., :C].astype(np.float64) / 255.0
    flow, warp, _ = flow_pairs(torch.from_numpy(v[0::2]).cuda(), torch.from_numpy(v[1::2]).cuda(), 3, layout="NHWC", **kw)
    P = default_params(**kw) if kw else None
    singles = [gpu.coarse2fine_flow(np.ascontiguousarray(v[2 * i]), np.ascontiguousarray(v[2 * i + 1]), 3, P)[:3]
               for i in range(2)]
    _check_pairs(flow, warp, "NHWC", singles, what)


def test_a_1080p_pair_runs_on_its_own(gpu):
    import cases
    from papteam_opticalflow_amd.tensors import flow_pairs
    a, b = cases.load_frame_u8("1920", 1), cases.load_frame_u8("1920", 2)
    ta, tb = torch.from_numpy(a).cuda().permute(2, 0, 1), torch.from_numpy(b).cuda().permute(2, 0, 1)  # 3-D: a batch of one
    flow, warp, _ = flow_pairs(ta, tb, 5)
    assert flow.shape == (1, 2, 1080, 1920) and warp.shape == (1, 3, 1080, 1920)
    _check_pairs(flow, warp, "NCHW", [gpu.coarse2fine_flow_u8(a, b, 5)[:3]], "1080p")


def test_guard_rerun_of_a_repeated_frame(gpu):
    from papteam_opticalflow_amd.tensors import flow_video
    v = _video("240", 4)
    frames = [v[0], v[1], v[1], v[2]]
    before = gpu.lap_guard_stats()["reruns"]
    flow, warp, _ = flow_video(_dev(frames), 3, layout="NHWC")
    assert gpu.lap_guard_stats()["reruns"] > before
    assert not flow[1].any()
    _check_pairs(flow, warp, "NHWC", [gpu.coarse2fine_flow_u8(frames[i], frames[i + 1], 3)[:3] for i in range(3)],
                 "repeated frame")


def test_sub_batches_equal_the_unsplit_result(monkeypatch):
    from papteam_opticalflow_amd.tensors import flow_video
    frames = _dev(_video("240", 9))
    whole = flow_video(frames, 3, layout="NHWC")
    monkeypatch.setenv("PAPOF_BATCH_MAX", "3")
    split = flow_video(frames, 3, layout="NHWC")
    monkeypatch.delenv("PAPOF_BATCH_MAX")
    _same_run(split, whole, "8 pairs in sub-batches of at most 3")


def test_float32_outputs_are_the_rounded_float64_ones():
    from papteam_opticalflow_amd.tensors import flow_video
    frames = _dev(_video("240", 5)).permute(0, 3, 1, 2)
    f64 = flow_video(frames, 3)
    f32 = flow_video(frames, 3, out_dtype=torch.float32)
    assert f32[0].dtype == torch.float32 and f32[1].dtype == torch.float32
    _same_run(f32, (f64[0].to(torch.float32), f64[1].to(torch.float32)), "float32 outputs")


def test_the_call_is_ordered_behind_the_callers_stream(video17):
    """Frames written on a side stream behind a long sleep, the call made under that stream with no synchronisation: the
    call must read the frames after they are written (the entry wait of papof_flow_batch_tensor).  The side stream has a high
    priority, so its hardware queue is never one the handle's streams share -- only the entry wait orders the two."""
    import time
    from papteam_opticalflow_amd.tensors import flow_video
    v, singles = video17
    src = _dev(v)
    dst = torch.zeros_like(src)
    flow_video(dst, 5, layout="NHWC")  # arena, counters: the call below allocates nothing (an allocation synchronises)
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.5 / per_cycle))  # ~0.5 s: far longer than the enqueueing of the call
        dst.copy_(src)
        flow, warp, _ = flow_video(dst, 5, layout="NHWC")
        took = time.perf_counter() - t0
    _check_pairs(flow, warp, "NHWC", singles, "side stream")
    assert took > 0.3, "the sleep in front of the frames was not visible: the call took %.3f s" % took
