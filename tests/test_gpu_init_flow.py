"""The device-tensor calls started from a caller's initial flow (tensors.py: init_flow / init_flow_bw -> include/papof.h:
papof_flow_batch_tensor_init, _fb_init).  What is held to what:
  * an all-zero init gives the BYTES of no init on the default branches (the sign of a zero counts);
  * a non-zero init gives the bits of the oracle composition of tests/_init_ref.py (the rule of papof.h restated on the
    CPU oracle's stages) -- in the batched chain and in the pair-by-pair paths outside it;
  * each direction of the _fb call is flow_pairs with that direction's init;
  * an init is read in order behind the caller's stream, and a refused value leaves every output untouched;
  * and the point of it all: a translation that a 1-level call cannot see is recovered from a prior."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402
from _init_ref import BICUBIC, GMIXTURE, coarse2fine_init  # noqa: E402
from _libs import OracleLib  # noqa: E402
from test_gpu_batch import _video  # noqa: E402

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


@pytest.fixture(scope="module")
def orc():
    return OracleLib()


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same_bytes(got, want, what):
    g, w = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if g.tobytes() != w.tobytes():
        iv = np.int64 if g.dtype == np.float64 else np.int32
        raise AssertionError("%s: %d elements differ, max-abs %.3e" % (what, int((g.view(iv) != w.view(iv)).sum()),
                                                                        float(np.abs(g.astype(np.float64) - w).max())))


def _same_run(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, torch.Tensor):
            _same_bytes(g, w, "%s [%d]" % (what, i))


def _dev(frames):
    return torch.from_numpy(np.stack(frames)).cuda()


def _smooth_init(B, H, W, per_pair=True):
    """a smooth analytic flow (B, 2, H, W) of a few pixels, different for every pair, exactly representable in float32"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, 2, H, W))
    for p in range(B):
        q = p if per_pair else 0
        out[p, 0] = 2.5 * np.sin(2 * np.pi * x / W + 0.7 * q) + 0.8 * np.cos(2 * np.pi * y / H) + 0.5 * q
        out[p, 1] = -1.5 * np.cos(2 * np.pi * (x + y) / (W + H) + 0.3 * q) + 0.25 * q
    return out.astype(np.float32).astype(np.float64)


def _oracle_pairs(orc, frames_u8, init, levels, **kw):
    """[(vx, vy, warpI2 HWC)] of the composition on the consecutive pairs of uint8 HWC frames, init (B, 2, H, W)"""
    out = []
    for p in range(len(frames_u8) - 1):
        a, b = frames_u8[p].astype(np.float64) / 255.0, frames_u8[p + 1].astype(np.float64) / 255.0
        out.append(coarse2fine_init(orc, a, b, levels, np.ascontiguousarray(init[p].transpose(1, 2, 0)), **kw))
    return out


def _check_oracle(flow, warp, layout, want, what):
    assert flow.shape[0] == len(want)
    for i, (vx, vy, wi) in enumerate(want):
        _same_bytes(flow[i, 0], vx, "%s pair %d vx" % (what, i))
        _same_bytes(flow[i, 1], vy, "%s pair %d vy" % (what, i))
        w = warp[i].permute(1, 2, 0) if layout == "NCHW" else warp[i]
        _same_bytes(w, wi, "%s pair %d warpI2" % (what, i))


# ---- an all-zero init: the bytes of none
@pytest.mark.parametrize("levels", [3, 5, 15])
def test_zero_init_is_no_init(levels):
    from papteam_opticalflow_amd.tensors import flow_pairs, flow_video
    v = _dev(_video("240", 5))
    z = torch.zeros((4, 2, 135, 240), dtype=torch.float64, device="cuda")
    _same_run(flow_video(v, levels, layout="NHWC", init_flow=z), flow_video(v, levels, layout="NHWC"),
              "flow_video L%d" % levels)
    _same_run(flow_pairs(v[:-1], v[1:], levels, layout="NHWC", init_flow=z),
              flow_pairs(v[:-1], v[1:], levels, layout="NHWC"), "flow_pairs L%d" % levels)


def test_zero_init_is_no_init_fb_and_float32_outputs():
    from papteam_opticalflow_amd.tensors import flow_video, flow_video_fb
    v = _dev(_video("240", 4))
    z = torch.zeros((2, 135, 240), dtype=torch.float32, device="cuda")  # broadcast, float32
    _same_run(flow_video_fb(v, 5, layout="NHWC", init_flow=z, init_flow_bw=z), flow_video_fb(v, 5, layout="NHWC"),
              "flow_video_fb")
    _same_run(flow_video_fb(v, 5, layout="NHWC", init_flow_bw=z), flow_video_fb(v, 5, layout="NHWC"), "bw only")
    _same_run(flow_video(v, 5, layout="NHWC", out_dtype=torch.float32, init_flow=z),
              flow_video(v, 5, layout="NHWC", out_dtype=torch.float32), "float32 outputs")


# ---- a non-zero init against the oracle composition
@pytest.fixture(scope="module")
def clip():
    v = _video("240", 4)
    return v, _smooth_init(3, 135, 240)


@pytest.fixture(scope="module")
def oracle_clip(orc, clip):
    v, init = clip
    return {levels: _oracle_pairs(orc, v, init, levels) for levels in (1, 5, 8)}


@pytest.mark.parametrize("levels", [1, 5, 8])
def test_nonzero_init_is_the_oracle_composition(clip, oracle_clip, levels):
    from papteam_opticalflow_amd.tensors import flow_pairs, flow_video
    v, init = clip
    t = _dev(v)
    ti = torch.from_numpy(init).cuda()
    flow, warp, _ = flow_video(t, levels, layout="NHWC", init_flow=ti)
    _check_oracle(flow, warp, "NHWC", oracle_clip[levels], "sequence L%d" % levels)
    nchw = t.permute(0, 3, 1, 2)
    flow, warp, _ = flow_pairs(nchw[:-1], nchw[1:], levels, init_flow=ti)
    _check_oracle(flow, warp, "NCHW", oracle_clip[levels], "pairs L%d" % levels)
    # float32 of the same values: the same bits; a (B, H, W, 2) tensor permuted, read in place
    flow32, _, _ = flow_video(t, levels, layout="NHWC", init_flow=ti.to(torch.float32))
    _same_bytes(flow32, flow, "float32 init L%d" % levels)
    hw2 = ti.permute(0, 2, 3, 1).contiguous()
    flowp, _, _ = flow_video(t, levels, layout="NHWC", init_flow=hw2.permute(0, 3, 1, 2))
    _same_bytes(flowp, flow, "permuted init L%d" % levels)


def test_broadcast_init_is_the_oracle_composition(orc, clip):
    from papteam_opticalflow_amd.tensors import flow_video
    v, init = clip
    one = init[:1].repeat(3, axis=0)
    flow, warp, _ = flow_video(_dev(v), 5, layout="NHWC", init_flow=torch.from_numpy(init[0]).cuda())
    _check_oracle(flow, warp, "NHWC", _oracle_pairs(orc, v, one, 5), "broadcast L5")


# ---- outside the batched chain: the pair-by-pair paths
@pytest.mark.parametrize("case", ["bicubic", "gmixture", "c2"])
def test_init_outside_the_chain(orc, case):
    from papteam_opticalflow_amd.tensors import flow_video
    v = _video("240", 3)
    init = _smooth_init(2, 135, 240)
    kw, okw, levels = {}, {}, 3
    if case == "bicubic":
        kw, okw = dict(interpolation=1), dict(interpolation=BICUBIC)
    elif case == "gmixture":  # chaotic by nature (test_gpu_parity.py): the short schedule, and its 1e-7
        kw = dict(noise_model=1, n_outer=2, n_outer_per_level=0)
        okw = dict(noise_model=GMIXTURE, n_outer=2, n_outer_per_level=0)
    else:
        v = [np.ascontiguousarray(f[..., :2]) for f in v]
    flow, warp, _ = flow_video(_dev(v), levels, layout="NHWC", init_flow=torch.from_numpy(init).cuda(), **kw)
    want = _oracle_pairs(orc, v, init, levels, **okw)
    if case != "gmixture":
        _check_oracle(flow, warp, "NHWC", want, case)
        return
    for i, (vx, vy, wi) in enumerate(want):
        for g, w_ in ((flow[i, 0], vx), (flow[i, 1], vy), (warp[i], wi)):
            assert np.abs(_np(g) - w_).max() < 1e-7, (case, i)


# ---- the fallbacks of the batched chain
def test_guard_rerun_with_zero_init(gpu):
    from papteam_opticalflow_amd.tensors import flow_video
    v = _video("240", 4)
    frames = _dev([v[0], v[1], v[1], v[2]])
    z = torch.zeros((3, 2, 135, 240), dtype=torch.float64, device="cuda")
    before = gpu.lap_guard_stats()["reruns"]
    got = flow_video(frames, 3, layout="NHWC", init_flow=z)
    assert gpu.lap_guard_stats()["reruns"] > before
    _same_run(got, flow_video(frames, 3, layout="NHWC"), "repeated frame, zero init")


def test_sub_batches_with_per_pair_inits(monkeypatch):
    from papteam_opticalflow_amd.tensors import flow_video
    frames = _dev(_video("240", 9))
    init = torch.from_numpy(_smooth_init(8, 135, 240)).cuda()
    whole = flow_video(frames, 3, layout="NHWC", init_flow=init)
    monkeypatch.setenv("PAPOF_BATCH_MAX", "3")
    split = flow_video(frames, 3, layout="NHWC", init_flow=init)
    monkeypatch.delenv("PAPOF_BATCH_MAX")
    _same_run(split, whole, "8 pairs with inits in sub-batches of at most 3")


# ---- both directions
def test_each_direction_is_flow_pairs_with_its_init():
    from papteam_opticalflow_amd.tensors import fb_consistency, flow_pairs, flow_pairs_fb
    v = _dev(_video("240", 4))
    im1, im2 = v[:-1], v[1:]
    a = torch.from_numpy(_smooth_init(3, 135, 240)).cuda()
    b = -0.5 * a.flip(0)
    fb = flow_pairs_fb(im1, im2, 5, layout="NHWC", init_flow=a, init_flow_bw=b)
    _same_run(fb[0::2][:2], flow_pairs(im1, im2, 5, layout="NHWC", init_flow=a)[:2], "forward")
    _same_run(fb[1::2][:2], flow_pairs(im2, im1, 5, layout="NHWC", init_flow=b)[:2], "backward")
    _same_bytes(fb.occlusion, fb_consistency(fb.flow_fw, fb.flow_bw), "occlusion")


# ---- what an initial flow is for: a translation beyond a 1-level call, given as a prior
def test_a_translation_is_recovered_from_its_prior():
    """frame 1 of the 480x270 clip cropped at two offsets: im2(x + 9, y - 6) = im1(x, y).  The median endpoint error over
    the interior (16 px margin) of a cold 1-level call is several pixels (it sees ~1 px at most); with the true shift as
    the initial flow it is far below one pixel.  Measured on an MI355X: 10.54 px cold, 0.0000 px from the prior; the
    margins asserted are > 5 px and < 0.25 px."""
    from papteam_opticalflow_amd.tensors import flow_pairs
    f = cases.load_frame_u8("480", 1)
    du, dv, h, w, y0, x0 = 9, -6, 224, 400, 20, 30
    im1 = np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w])
    im2 = np.ascontiguousarray(f[y0 - dv:y0 - dv + h, x0 - du:x0 - du + w])
    assert np.array_equal(im2[16 + dv, 16 + du], im1[16, 16])
    t1, t2 = _dev([im1]), _dev([im2])
    prior = torch.zeros((2, h, w), dtype=torch.float64, device="cuda")
    prior[0], prior[1] = du, dv
    m = 16

    def epe(flow):
        f_ = _np(flow[0])[:, m:-m, m:-m]
        return float(np.median(np.hypot(f_[0] - du, f_[1] - dv)))

    cold = epe(flow_pairs(t1, t2, 1, layout="NHWC")[0])
    warm = epe(flow_pairs(t1, t2, 1, layout="NHWC", init_flow=prior)[0])
    print("translation (%d, %d): median EPE cold %.4f px, from the prior %.4f px" % (du, dv, cold, warm))
    assert cold > 5.0 and warm < 0.25, (cold, warm)


# ---- order and refusals
def test_the_init_is_read_behind_the_callers_stream(clip, oracle_clip):
    import time
    from papteam_opticalflow_amd.tensors import flow_video
    v, init = clip
    t = _dev(v)
    src = torch.from_numpy(init).cuda()
    dst = torch.zeros_like(src)
    flow_video(t, 5, layout="NHWC", init_flow=dst)  # arena, counters: the call below allocates nothing
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.5 / per_cycle))
        dst.copy_(src)
        flow, warp, _ = flow_video(t, 5, layout="NHWC", init_flow=dst)
        took = time.perf_counter() - t0
    _check_oracle(flow, warp, "NHWC", oracle_clip[5], "side stream")
    assert took > 0.3, "the sleep in front of the init was not visible: the call took %.3f s" % took


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e7])
def test_refused_values(gpu, bad):
    from papteam_opticalflow_amd import capi
    from papteam_opticalflow_amd.tensors import flow_pairs, flow_video
    v = _dev(_video("240", 3))
    init = torch.zeros((2, 2, 135, 240), dtype=torch.float64, device="cuda")
    init[1, 1, 70, 100] = bad
    with pytest.raises(ValueError):
        flow_video(v, 3, layout="NHWC", init_flow=init)
    with pytest.raises(ValueError):
        flow_pairs(v[:-1], v[1:], 3, layout="NHWC", init_flow=init.to(torch.float32))
    # the C entry: PAPOF_EINVAL after the entry wait, and not one output element written
    flow = torch.full((2, 2, 135, 240), 7.25, dtype=torch.float64, device="cuda")
    warp = torch.full((2, 135, 240, 3), -3.5, dtype=torch.float64, device="cuda")

    def desc(t, strides, code):
        d = capi.PapofTensor()
        d.data, d.dtype = t.data_ptr(), code
        for i, s in enumerate(strides):
            d.stride[i] = s
        return d

    d_fr = desc(v, (v.stride(0), v.stride(1), v.stride(2), v.stride(3)), capi.DTYPE_U8)
    d_init = desc(init, (init.stride(0), init.stride(2), init.stride(3), init.stride(1)), capi.DTYPE_F64)
    d_flow = desc(flow, (flow.stride(0), flow.stride(2), flow.stride(3), flow.stride(1)), capi.DTYPE_F64)
    d_warp = desc(warp, (warp.stride(0), warp.stride(1), warp.stride(2), warp.stride(3)), capi.DTYPE_F64)
    tm = (ctypes.c_double * capi.N_TIMERS)()
    torch.cuda.synchronize()
    rc = gpu.L.papof_flow_batch_tensor_init(gpu.h, 2, 1, ctypes.byref(d_fr), None, 135, 240, 3, 3, None,
                                            ctypes.byref(d_init), ctypes.byref(d_flow), ctypes.byref(d_warp), None, tm)
    rc_fb = gpu.L.papof_flow_batch_tensor_fb_init(gpu.h, 2, 1, ctypes.byref(d_fr), None, 135, 240, 3, 3, None, None,
                                                  ctypes.byref(d_init), ctypes.byref(d_flow), ctypes.byref(d_warp),
                                                  ctypes.byref(d_flow), ctypes.byref(d_warp), None, 0.01, 0.5, None, tm)
    torch.cuda.synchronize()
    assert rc == -1 and rc_fb == -1, (rc, rc_fb)
    assert bool((flow == 7.25).all()) and bool((warp == -3.5).all())
