"""Edge-aware flow refinement, checked on the CPU: known answers of the numpy restatement (tests/_refine_ref.py) that the
device's bytes are compared with in tests/test_gpu_refine.py -- plain medians under equal weights, the order of the key, what
occlusion and NaN do, a fixed point, and the scene with known ground truth on which one pass must halve the error at the motion
boundaries -- the library's host-made tables against numpy's, and every argument error of tensors.refine_flow /
refine_video_flows raised before a launch (CPU tensors, a stubbed handle), with the C ABI's own refusals through ctypes.
No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

from _refine_ref import epe, key, q_of, refine_reference, tables, two_layer_scene, unkey

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402

EINVAL = -1  # PAPOF_EINVAL


def _flat(radius):
    """equal weights: sigma_s = 1e6 makes every spatial weight 32768, and a constant guide every range weight R[0]"""
    S, R = tables(radius, 1e6)
    assert np.all(S == 32768)
    return S, R


def test_equal_weights_give_the_plain_median():
    rng = np.random.default_rng(1)
    H, W, r = 11, 13, 2
    flow = rng.normal(0, 3, (1, 2, H, W))
    guide = np.full((1, H, W, 1), 0.5)
    S, R = _flat(r)
    out = refine_reference(flow, guide, S, R, q_of(0.1, 1, False), r)
    for y, x in ((2, 2), (5, 6), (8, 10)):  # interior: 25 live neighbours
        for c in range(2):
            assert out[0, c, y, x] == np.median(flow[0, c, y - r:y + r + 1, x - r:x + r + 1])
    for (y, x), (ys, xs) in (((0, 0), (slice(0, 3), slice(0, 3))), ((H - 1, W - 1), (slice(H - 3, H), slice(W - 3, W)))):
        for c in range(2):  # a corner: 9 live neighbours
            assert out[0, c, y, x] == np.median(flow[0, c, ys, xs])
    # an even number of live neighbours: the LOWER median
    occ = np.zeros((1, H, W), np.uint8)
    occ[0, 5, 5] = 1
    out = refine_reference(flow, guide, S, R, q_of(0.1, 1, False), r, occlusion=occ)
    for c in range(2):
        live = np.delete(flow[0, c, 3:8, 4:9].ravel(), 2 * 5 + 1)  # (5, 5) in the window of (5, 6)
        assert len(live) == 24 and out[0, c, 5, 6] == np.sort(live)[11]


def test_the_key_is_strictly_increasing():
    v = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-300, 1.0, np.inf])
    k = key(v)
    assert np.all(np.diff(k) > 0)
    assert np.array_equal(unkey(k).view(np.int64), v.view(np.int64))  # its own inverse, signed zeros included


def test_occluded_garbage_and_nan_take_their_neighbours_motion():
    H, W, r = 24, 28, 4
    flow = np.empty((1, 2, H, W))
    flow[0, 0], flow[0, 1] = 1.25, -0.5
    clean = flow.copy()
    guide = np.full((1, H, W, 3), 100, np.uint8)
    S, R = tables(r, 7.0)
    q = q_of(7 / 255, 3, True)
    bad, occ = flow.copy(), np.zeros((1, H, W), np.uint8)
    bad[0, :, 8:14, 10:16] = np.random.default_rng(2).normal(0, 50, (2, 6, 6))
    occ[0, 8:14, 10:16] = 1
    assert np.array_equal(refine_reference(bad, guide, S, R, q, r, occlusion=occ), clean)
    # everything occluded: the input
    assert np.array_equal(refine_reference(bad, guide, S, R, q, r, occlusion=np.ones((1, H, W), np.uint8)), bad)
    # a block of NaN without any mask comes back finite
    nan = flow.copy()
    nan[0, :, 8:14, 10:16] = np.nan
    assert np.array_equal(refine_reference(nan, guide, S, R, q, r), clean)
    # where = 0: copied, NaN included
    got = refine_reference(nan, guide, S, R, q, r, where=np.zeros((1, H, W), np.uint8))
    assert np.array_equal(got.view(np.int64), nan.view(np.int64))


def test_two_layers_with_their_guide_are_a_fixed_point():
    guide, true, _, _ = two_layer_scene(0)
    flat = np.where(true[0, 0][..., None] == 4.0, np.array([200, 90, 80]), np.array([60, 130, 170])).astype(np.uint8)[None]
    S, R = tables(7, 7.0)
    out = refine_reference(true, flat, S, R, q_of(7 / 255, 3, True), 7)
    assert np.array_equal(out, true)


def test_quality_on_the_scene_with_known_ground_truth():
    """Band EPE (where the blurred layer mask is in (0.02, 0.98)) of the degraded flow against the refined one, defaults
    (r = 7, sigma_s = 7, sigma_c = 7 / 255), measured: seed 0: 0.7781 before, 0.1648 after one pass (ratio 0.212), 0.0974
    after two, 0.0759 after three; whole image 0.2050 -> 0.0463 after one pass, 0.0279 after three.  Seeds 1 and 2: 0.1639 and
    0.1638 after one pass.  Asserted: band EPE after one pass <= 0.5 x before, and no
    further pass up to three may raise it."""
    S, R = tables(7, 7.0)
    q = q_of(7 / 255, 3, True)
    for seed in (0, 1, 2):
        guide, true, degraded, band = two_layer_scene(seed)
        before = epe(degraded, true, band)
        flows, errs = degraded, []
        for _ in range(3 if seed == 0 else 1):
            flows = refine_reference(flows, guide, S, R, q, 7)
            errs.append(epe(flows, true, band))
        print("seed %d: band of %d px, band EPE %.4f -> %s; whole image %.4f -> %.4f after %d" % (
            seed, band.sum(), before, " ".join("%.4f" % e for e in errs), epe(degraded, true), epe(flows, true), len(errs)))
        assert errs[0] <= 0.5 * before
        assert all(b <= a for a, b in zip(errs, errs[1:]))
        if seed == 0:  # iters = 3 is three passes
            assert np.array_equal(refine_reference(degraded, guide, S, R, q, 7, iters=3), flows)


def test_library_tables_against_numpy():
    for radius, sigma_s in ((1, 0.5), (2, 1e6), (7, 7.0), (15, 3.3)):
        S, R = tensors.refine_tables(radius, sigma_s)
        S0, R0 = tables(radius, sigma_s)
        assert S.dtype == np.uint32 and S.shape == ((2 * radius + 1) ** 2,) and R.shape == (4096,)
        assert np.abs(S.astype(np.int64) - S0.astype(np.int64)).max() <= 1
        assert np.abs(R.astype(np.int64) - R0.astype(np.int64)).max() <= 1
        assert S[len(S) // 2] == 32768 and R[0] == 65408 and R[4095] == 0
        assert int(S.max()) * int(R.max()) < 2 ** 31
    L = capi.load()
    U = ctypes.POINTER(ctypes.c_uint)
    S, R = np.zeros(961, np.uint32), np.zeros(4096, np.uint32)
    ps, pr = S.ctypes.data_as(U), R.ctypes.data_as(U)
    for bad in ((0, 1.0, ps, pr), (16, 1.0, ps, pr), (3, 0.0, ps, pr), (3, -1.0, ps, pr), (3, math.nan, ps, pr),
                (3, math.inf, ps, pr), (3, 1.0, None, pr), (3, 1.0, ps, None)):
        assert L.papof_refine_tables(*bad) == EINVAL, bad[:2]
    assert tensors.refine_q(0.1, 3, False) == 128.0 / (0.1 * 0.1 * 3)
    assert tensors.refine_q(7 / 255, 3, True) == q_of(7 / 255, 3, True)


def test_workspace_sizes_and_refusals():
    L = capi.load()
    one = 16 * 3 * 135 * 240
    assert L.papof_refine_workspace(3, 135, 240, 1) == 0
    assert L.papof_refine_workspace(3, 135, 240, 2) == one
    assert L.papof_refine_workspace(3, 135, 240, 3) == 2 * one
    assert L.papof_refine_workspace(3, 135, 240, 65536) == 2 * one
    assert L.papof_refine_workspace(1, 32768, 32767, 2) > 0  # H W < 2^30
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 8, 65537), (1, 32768, 32768, 1), (2 ** 31 - 1, 32768, 32767, 2)):
        assert L.papof_refine_workspace(*bad) < 0, bad


def test_c_abi_refuses_bad_arguments_without_a_device():
    """PAPOF_EINVAL is decided before the handle is used: a fake non-NULL handle and fake pointers are never dereferenced"""
    L = capi.load()
    h = ctypes.c_void_p(8)

    def T(dtype=capi.DTYPE_F64, strides=(128, 8, 1, 64), data=4096):
        t = capi.PapofTensor()
        t.data, t.dtype = data, dtype
        for i, s in enumerate(strides):
            t.stride[i] = s
        return t
    m = T(dtype=capi.DTYPE_U8, strides=(64, 8, 1, 0))
    ok = dict(h=h, n=1, H=8, W=8, C=1, flow=T(), guide=T(strides=(64, 8, 1, 64)), occ=None, where=None, r=2,
              S=ctypes.c_void_p(4096), R=ctypes.c_void_p(4096), q=1.0, iters=1, out=T(), passes=None, ws=None, nbytes=0)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        ref = lambda t: ctypes.byref(t) if t is not None else None  # noqa: E731
        return L.papof_refine_flow_tensor(a["h"], a["n"], a["H"], a["W"], a["C"], ref(a["flow"]), ref(a["guide"]), ref(a["occ"]),
                                          ref(a["where"]), a["r"], a["S"], a["R"], a["q"], a["iters"], ref(a["out"]),
                                          ref(a["passes"]), a["ws"], a["nbytes"], None)
    for kw in (dict(h=None), dict(n=0), dict(H=0), dict(W=0), dict(H=32768, W=32768), dict(C=0), dict(C=5), dict(r=0),
               dict(r=16), dict(flow=None), dict(guide=None), dict(out=None), dict(flow=T(dtype=capi.DTYPE_U8)),
               dict(flow=T(data=None)), dict(guide=T(dtype=7)), dict(guide=T(strides=(64, -8, 1, 64))),
               dict(out=T(dtype=capi.DTYPE_U8)), dict(out=T(strides=(128, 8, 0, 64))), dict(occ=T()), dict(where=T()),
               dict(occ=T(dtype=capi.DTYPE_U8, strides=(64, -8, 1, 0))), dict(passes=T()), dict(S=None), dict(R=None),
               dict(q=-1.0), dict(q=math.nan), dict(q=math.inf), dict(iters=0), dict(iters=65537, ws=ctypes.c_void_p(4096), nbytes=1 << 20),
               dict(iters=2), dict(iters=2, ws=ctypes.c_void_p(4096), nbytes=16 * 64 - 8),
               dict(iters=3, ws=ctypes.c_void_p(4096), nbytes=16 * 64), dict(occ=m, where=m, iters=0)):
        assert call(**kw) == EINVAL, kw


# ---- argument errors of the Python calls, before any launch ----

@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused; CPU tensors pass for device ones"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")
    return calls


def _z(*shape, **kw):
    return torch.zeros(*shape, **kw)


@pytest.mark.parametrize("kw,exc", [
    (dict(radius=0), ValueError), (dict(radius=16), ValueError), (dict(radius=2.0), TypeError), (dict(radius=True), TypeError),
    (dict(sigma_s=0.0), ValueError), (dict(sigma_s=-1.0), ValueError), (dict(sigma_s=math.nan), ValueError),
    (dict(sigma_s=math.inf), ValueError), (dict(sigma_s="wide"), TypeError),
    (dict(sigma_c=0.0), ValueError), (dict(sigma_c=math.inf), ValueError), (dict(sigma_c=None), TypeError),
    (dict(iters=0), ValueError), (dict(iters=-3), ValueError), (dict(iters=65537), ValueError), (dict(iters=1.5), TypeError),
    (dict(layout="CHWN"), ValueError), (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.uint8), TypeError),
    (dict(flow=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow=_z(2, 3, 8, 8)), ValueError),
    (dict(flow=_z(3, 2, 8, 8)), ValueError), (dict(flow=_z(2, 2, 8, 9)), ValueError), (dict(flow=None), TypeError),
    (dict(flow=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(guide=_z(2, 5, 8, 8)), ValueError), (dict(guide=_z(2, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(guide=_z(8, 8)), ValueError), (dict(guide=None), TypeError),
    (dict(occlusion=_z(2, 8, 8)), TypeError), (dict(occlusion=_z(2, 1, 8, 8, dtype=torch.bool)), ValueError),
    (dict(occlusion=_z(2, 8, 8, dtype=torch.bool, device="meta")), ValueError), (dict(occlusion=[1]), TypeError),
    (dict(where=_z(2, 8, 8, dtype=torch.int32)), TypeError), (dict(where=_z(2, 8, 9, dtype=torch.uint8)), ValueError),
    (dict(where=_z(2, 8, 8, dtype=torch.uint8, device="meta")), ValueError),
])
def test_refine_flow_errors_before_any_launch(stub, kw, exc):
    args = dict(flow=_z(2, 2, 8, 8), guide=_z(2, 3, 8, 8))
    args.update(kw)
    with pytest.raises(exc):
        tensors.refine_flow(args.pop("flow"), args.pop("guide"), **args)
    assert stub == []


def test_refine_flow_refuses_cpu_tensors(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    with pytest.raises(ValueError):
        tensors.refine_flow(_z(2, 2, 8, 8), _z(2, 3, 8, 8))
    with pytest.raises(ValueError):
        tensors.refine_video_flows(_z(3, 3, 8, 8), _z(2, 2, 8, 8), _z(2, 2, 8, 8))
    assert calls == []


@pytest.mark.parametrize("kw,exc", [
    (dict(radius=0), ValueError), (dict(sigma_c=-1.0), ValueError), (dict(iters=0), ValueError), (dict(window=3), TypeError),
    (dict(out_dtype=torch.int32), TypeError), (dict(consistency=(1.0,)), TypeError), (dict(consistency=(-1.0, 0.5)), ValueError),
    (dict(layout="HWC"), ValueError), (dict(frames=_z(1, 3, 8, 8)), ValueError), (dict(frames=_z(3, 5, 8, 8)), ValueError),
    (dict(flow_fw=_z(3, 2, 8, 8)), ValueError), (dict(flow_bw=_z(2, 2, 8, 9)), ValueError),
    (dict(flow_bw=_z(2, 2, 8, 8, dtype=torch.int32)), TypeError),
    (dict(occlusion=_z(2, 2, 8, 8)), TypeError), (dict(occlusion=_z(2, 8, 8, dtype=torch.bool)), ValueError),
])
def test_refine_video_flows_errors_before_any_launch(stub, kw, exc):
    args = dict(frames=_z(3, 3, 8, 8), flow_fw=_z(2, 2, 8, 8), flow_bw=_z(2, 2, 8, 8))
    args.update(kw)
    with pytest.raises(exc):
        tensors.refine_video_flows(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []
