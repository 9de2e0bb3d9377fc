"""Forward and backward flow with occlusion masks on device tensors (papteam_opticalflow_amd/tensors.py: flow_video_fb,
flow_pairs_fb, fb_consistency -> papof_flow_batch_tensor_fb, papof_fb_check_tensor).  Each direction of every pair must come
back with the BITS of the single host call on its frames (backward: the frames exchanged) -- in the batched chain, in what
it does not cover, through the guard's re-run and in sub-batches -- and the occlusion mask must equal the numpy fp64
restatement of the check (tests/test_fb_cpu.py: fb_reference) bit for bit.  Bits are compared as integer views, so that a
flipped sign of a zero is caught."""
import math

import numpy as np
import pytest

from test_fb_cpu import fb_reference
from test_gpu_batch import _video
from test_gpu_tensors import _dev, _same_bits

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


def _check_dirs(res, layout, fw_singles, bw_singles, what):
    """both directions of a FlowFB against [(vx, vy, warpI2 HWC)] of the single calls"""
    for name, flow, warp, singles in (("fw", res.flow_fw, res.warpI2_fw, fw_singles),
                                      ("bw", res.flow_bw, res.warpI2_bw, bw_singles)):
        assert flow.shape[0] == len(singles)
        for i, (vx, vy, wi) in enumerate(singles):
            _same_bits(flow[i, 0], vx, "%s %s pair %d vx" % (what, name, i))
            _same_bits(flow[i, 1], vy, "%s %s pair %d vy" % (what, name, i))
            w = warp[i].permute(1, 2, 0) if layout == "NCHW" else warp[i]
            _same_bits(w, wi, "%s %s pair %d warpI2" % (what, name, i))


def _same_mask(got, want, what):
    g = got.detach().cpu().numpy().astype(np.uint8) if isinstance(got, torch.Tensor) else np.asarray(got, np.uint8)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not np.array_equal(g, want):
        raise AssertionError("%s: %d of %d mask elements differ" % (what, int((g != want).sum()), g.size))


@pytest.fixture(scope="module")
def video17(gpu):
    """the 240x135 video of 17 frames (uint8 HWC), its flow_video_fb result and the single calls on its 16 pairs in both
    directions, 5 levels"""
    from papteam_opticalflow_amd.tensors import flow_video_fb
    v = _video("240", 17)
    res = flow_video_fb(_dev(v), 5, layout="NHWC")
    fw = [gpu.coarse2fine_flow_u8(v[i], v[i + 1], 5)[:3] for i in range(16)]
    bw = [gpu.coarse2fine_flow_u8(v[i + 1], v[i], 5)[:3] for i in range(16)]
    return v, res, fw, bw


def test_video_both_directions_are_the_single_calls(video17):
    v, res, fw, bw = video17
    assert res.flow_fw.shape == (16, 2, 135, 240) and res.flow_bw.shape == (16, 2, 135, 240)
    assert res.warpI2_fw.shape == (16, 135, 240, 3) and res.warpI2_bw.shape == (16, 135, 240, 3)
    assert res.flow_fw.dtype == torch.float64 and res.occlusion.dtype == torch.bool
    assert res.occlusion.shape == (16, 2, 135, 240)
    assert float(res.timing["Total C++ Execution"]) > 0 and float(res.timing["Phase5_SOR"]) > 0
    _check_dirs(res, "NHWC", fw, bw, "video")


def test_occlusion_mask_is_the_definition(video17):
    from papteam_opticalflow_amd.tensors import fb_consistency, flow_video_fb
    v, res, _, _ = video17
    fw, bw = res.flow_fw.cpu().numpy(), res.flow_bw.cpu().numpy()
    want = fb_reference(fw, bw)
    assert 0 < want.sum() < want.size  # both kinds of pixels are present
    _same_mask(res.occlusion, want, "flow_video_fb occlusion")
    _same_mask(fb_consistency(res.flow_fw, res.flow_bw), want, "fb_consistency on the returned flows")
    r32 = flow_video_fb(_dev(v), 5, layout="NHWC", out_dtype=torch.float32)
    assert r32.flow_fw.dtype == torch.float32
    _same_mask(r32.occlusion, want, "occlusion with float32 outputs")
    _same_bits(r32.flow_bw, res.flow_bw.to(torch.float32), "float32 backward flow")
    other = flow_video_fb(_dev(v), 5, layout="NHWC", consistency=(0.05, 1.0))
    _same_mask(other.occlusion, fb_reference(fw, bw, 0.05, 1.0), "occlusion with other alphas")
    none = flow_video_fb(_dev(v), 5, layout="NHWC", consistency=None)
    assert none.occlusion is None
    _same_bits(none.flow_fw, res.flow_fw, "flow_fw without the check")
    _same_bits(none.flow_bw, res.flow_bw, "flow_bw without the check")


def test_pairs_float32_nchw_config4(gpu):
    from papteam_opticalflow_amd import default_params
    from papteam_opticalflow_amd.tensors import flow_pairs_fb
    kw = dict(n_outer=3, n_outer_per_level=0, n_sor=30, n_sor_per_level=0)  # config-4 schedule
    P = default_params(**kw)
    v = np.stack(_video("480", 8))
    f32 = torch.from_numpy(v).float() / 255  # float32 samples: the call widens them exactly
    a, b = f32[0::2].permute(0, 3, 1, 2).contiguous().cuda(), f32[1::2].permute(0, 3, 1, 2).contiguous().cuda()
    res = flow_pairs_fb(a, b, 5, layout="NCHW", **kw)
    assert res.warpI2_bw.shape == (4, 3, 270, 480)
    x = [f32[i].double().numpy() for i in range(8)]
    fw = [gpu.coarse2fine_flow(x[2 * i], x[2 * i + 1], 5, P)[:3] for i in range(4)]
    bw = [gpu.coarse2fine_flow(x[2 * i + 1], x[2 * i], 5, P)[:3] for i in range(4)]
    _check_dirs(res, "NCHW", fw, bw, "float32 NCHW pairs")
    _same_mask(res.occlusion, fb_reference(res.flow_fw.cpu().numpy(), res.flow_bw.cpu().numpy()), "pairs occlusion")


def _synthetic(B, H, W):
    """flows that reach every branch of the check: a constant shift that leaves the image, a flow onto the clamped border,
    pixels where e == alpha1 * m + alpha2 exactly (alphas 0.5, 0.125), NaNs, and smooth random flow elsewhere"""
    rng = np.random.default_rng(7)
    fw = rng.normal(0, 2, (B, 2, H, W))
    bw = -fw + rng.normal(0, 0.3, (B, 2, H, W))
    fw[0, 0], fw[0, 1] = 5.0, -3.0  # pair 0: a constant shift; its right columns and top rows leave the image
    bw[0, 0], bw[0, 1] = -5.0, 3.0
    fw[1, 0, :, -4:-2] = 0.75  # near the right border ...
    fw[1, 0, :, -2] = 1.0  # ... onto the last column: its right neighbour is clamped into the image
    fw[1, 0, :, -1] = 0.0
    fw[1, 1, -3, :] = 0.5
    fw[1, 1, -2, :] = 1.0  # onto the last row: the row below is clamped
    bw[1, :, -1, :] = 0.0
    fw[2], bw[2] = 0.0, 0.0  # pair 2, columns 0 .. W - 2: u = 0.5, b = 0: e = 0.25 == 0.5 * 0.25 + 0.125
    fw[2, 0, :, :-1] = 0.5
    fw[0, 0, 3, 4] = math.nan
    bw[1, 1, 5, 6] = math.nan
    fw[1, 0, 7, 7] = math.inf
    return fw, bw


def test_standalone_check_on_synthetic_flows(gpu):
    from papteam_opticalflow_amd.tensors import fb_consistency
    B, H, W = 3, 37, 53
    fw, bw = _synthetic(B, H, W)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    for a1, a2 in ((0.01, 0.5), (0.5, 0.125), (0.0, 0.0)):
        want = fb_reference(fw, bw, a1, a2)
        _same_mask(fb_consistency(tf, tb, a1, a2), want, "float64 (%g, %g)" % (a1, a2))
    at_bound = fb_reference(fw, bw, 0.5, 0.125)
    assert not at_bound[2, 0].any()  # e == bound: not occluded
    assert fb_reference(fw, bw)[0, 0, 3, 4] == 1 and fb_reference(fw, bw)[0, 0, :3, :].all()
    # float32 inputs, widened exactly
    f32, b32 = tf.float(), tb.float()
    want = fb_reference(f32.cpu().numpy(), b32.cpu().numpy())
    _same_mask(fb_consistency(f32, b32), want, "float32")
    _same_mask(fb_consistency(f32, tb), fb_reference(f32.cpu().numpy(), bw), "float32 forward, float64 backward")
    # permuted and sliced views, read in place
    big = torch.from_numpy(np.ascontiguousarray(np.concatenate([fw, fw], axis=3).transpose(0, 2, 3, 1))).cuda()  # B H 2W 2
    view = big.permute(0, 3, 1, 2)[:, :, 1:, 3::2]  # (B, 2, H - 1, W - 1) of odd strides
    assert not view.is_contiguous()
    bv = tb[:, :, 1:, 1:]
    want = fb_reference(view.cpu().numpy(), bv.cpu().numpy())
    _same_mask(fb_consistency(view, bv), want, "views")
    _same_mask(fb_consistency(view.flip(0), bv.flip(0)), want[::-1], "reversed pairs")


@pytest.mark.parametrize("what,kw,C", [
    ("red-black", dict(sor_mode=1), 3),
    ("two channels", {}, 2),
])
def test_what_the_batched_chain_does_not_cover(gpu, what, kw, C):
    from papteam_opticalflow_amd import default_params
    from papteam_opticalflow_amd.tensors import flow_pairs_fb
    v = np.stack(_video("240", 4))[..., :C].astype(np.float64) / 255.0
    res = flow_pairs_fb(torch.from_numpy(v[0::2]).cuda(), torch.from_numpy(v[1::2]).cuda(), 3, layout="NHWC", **kw)
    P = default_params(**kw) if kw else None
    x = [np.ascontiguousarray(v[i]) for i in range(4)]
    fw = [gpu.coarse2fine_flow(x[2 * i], x[2 * i + 1], 3, P)[:3] for i in range(2)]
    bw = [gpu.coarse2fine_flow(x[2 * i + 1], x[2 * i], 3, P)[:3] for i in range(2)]
    _check_dirs(res, "NHWC", fw, bw, what)
    _same_mask(res.occlusion, fb_reference(res.flow_fw.cpu().numpy(), res.flow_bw.cpu().numpy()), what + " occlusion")


def test_a_1080p_video_of_two_frames(gpu):
    import cases
    from papteam_opticalflow_amd.tensors import flow_video_fb
    a, b = cases.load_frame_u8("1920", 1), cases.load_frame_u8("1920", 2)
    res = flow_video_fb(_dev([a, b]).permute(0, 3, 1, 2), 5)
    assert res.flow_fw.shape == (1, 2, 1080, 1920) and res.warpI2_bw.shape == (1, 3, 1080, 1920)
    _check_dirs(res, "NCHW", [gpu.coarse2fine_flow_u8(a, b, 5)[:3]], [gpu.coarse2fine_flow_u8(b, a, 5)[:3]], "1080p")
    _same_mask(res.occlusion, fb_reference(res.flow_fw.cpu().numpy(), res.flow_bw.cpu().numpy()), "1080p occlusion")


def test_guard_reruns_of_a_repeated_frame(gpu):
    from papteam_opticalflow_amd.tensors import flow_video_fb
    v = _video("240", 4)
    frames = [v[0], v[1], v[1], v[2]]
    before = gpu.lap_guard_stats()["reruns"]
    res = flow_video_fb(_dev(frames), 3, layout="NHWC")
    assert gpu.lap_guard_stats()["reruns"] >= before + 2  # the repeated pair in both directions
    assert not res.flow_fw[1].any() and not res.flow_bw[1].any()
    fw = [gpu.coarse2fine_flow_u8(frames[i], frames[i + 1], 3)[:3] for i in range(3)]
    bw = [gpu.coarse2fine_flow_u8(frames[i + 1], frames[i], 3)[:3] for i in range(3)]
    _check_dirs(res, "NHWC", fw, bw, "repeated frame")
    _same_mask(res.occlusion, fb_reference(res.flow_fw.cpu().numpy(), res.flow_bw.cpu().numpy()), "repeated frame occlusion")


def _same_fb(got, want, what):
    for name in ("flow_fw", "flow_bw", "warpI2_fw", "warpI2_bw"):
        _same_bits(getattr(got, name), getattr(want, name), "%s %s" % (what, name))
    _same_mask(got.occlusion, want.occlusion.cpu().numpy().astype(np.uint8), what + " occlusion")


@pytest.mark.parametrize("bound", ["3", "5"])
def test_sub_batches_equal_the_unsplit_result(monkeypatch, bound):
    from papteam_opticalflow_amd.tensors import flow_video_fb
    frames = _dev(_video("240", 9))
    whole = flow_video_fb(frames, 3, layout="NHWC")
    monkeypatch.setenv("PAPOF_BATCH_MAX", bound)
    split = flow_video_fb(frames, 3, layout="NHWC")
    monkeypatch.delenv("PAPOF_BATCH_MAX")
    _same_fb(split, whole, "8 pairs in sub-batches of at most %s solver pairs" % bound)


def test_the_call_is_ordered_behind_the_callers_stream(video17):
    """Frames written on a side stream behind a long sleep, the call made under that stream with no synchronisation: the
    call must read the frames after they are written (the entry wait), as tests/test_gpu_tensors.py checks for flow_video."""
    import time
    from papteam_opticalflow_amd.tensors import flow_video_fb
    v, res, fw, bw = video17
    src = _dev(v)
    dst = torch.zeros_like(src)
    flow_video_fb(dst, 5, layout="NHWC")  # arena, counters: the call below allocates nothing (an allocation synchronises)
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
        got = flow_video_fb(dst, 5, layout="NHWC")
        took = time.perf_counter() - t0
    _check_dirs(got, "NHWC", fw, bw, "side stream")
    _same_mask(got.occlusion, res.occlusion.cpu().numpy().astype(np.uint8), "side stream occlusion")
    assert took > 0.3, "the sleep in front of the frames was not visible: the call took %.3f s" % took
