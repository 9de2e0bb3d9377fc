"""CPU-side checks of the homography model (papteam_opticalflow_amd/tensors.py: global_homography, warp_homography,
mosaic_homography, mosaic_overlap_homography, homography_transforms, panorama_homography; include/papof.h:
papof_homography_fit_tensor and the projective calls): the numpy fp64 restatement in tests/_homography_ref.py that
tests/test_gpu_homography.py compares the device with -- exact recovery and robustness of the fit, the rotating-camera chain
against the affine model's, the tile culling against brute-force liveness, the bytes of the affine restatements on matrices
whose last row is (0, 0, 1) --, homography_transforms, every Python argument error raised before a launch (CPU tensors, a
stubbed handle), refusals of the C ABI through ctypes, and the quality of a rotating camera's panorama under both models.
No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _blend_ref import blend_reference, overlap_reference  # noqa: E402
from _homography_ref import (chain, cull_keep, cull_matrices, fit_reference_h, homography_flow, homography_flows,  # noqa: E402
                             mosaic_reference_h, overlap_reference_h, projective_corner_distance, rotating_camera,
                             rotating_scene, tile_live, tiles, warp_reference_h)
from _mosaic_ref import canvas_truth, mosaic_reference, psnr  # noqa: E402
from _stab_ref import fit_reference, warp_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the fit
@pytest.mark.parametrize("H,W", [(50, 67), (70, 93)])
def test_fit_recovers_homographies_exactly_and_robustly(H, W):
    """Measured: clean fields < 1e-13 px at the corners after one iteration; with 20 % outliers of +-15 px and noise 0.2 px
    0.55 .. 1.22 px after one iteration and 0.018 .. 0.068 px after five"""
    clean, Ms = homography_flows(3, H, W, 1, outliers=0.0, noise=0.0)
    motion, ok, support = fit_reference_h(clean, iters=1)
    assert ok.all() and (motion[:, 2, 2] == 1.0).all()
    for i in range(3):
        assert projective_corner_distance(motion[i], Ms[i], H, W) < 1e-9
    noisy, Ms = homography_flows(3, H, W, 2)
    one, five = fit_reference_h(noisy, iters=1)[0], fit_reference_h(noisy, iters=5)[0]
    for i in range(3):
        e1, e5 = (projective_corner_distance(m[i], Ms[i], H, W) for m in (one, five))
        print("%d x %d pair %d: %.4f px after 1 iteration, %.4f px after 5" % (H, W, i, e1, e5))
        assert e5 < 0.25 and e5 < e1 / 4, (e1, e5)


def test_fit_failures():
    H, W = 50, 67
    f, _ = homography_flows(3, H, W, 3)
    f[1] = math.nan                      # no valid pixel
    f[2] = math.nan
    f[2, :, :, 10] = 0.0                 # one valid column: iteration 0 fails at a pivot
    motion, ok, support = fit_reference_h(f)
    assert ok.tolist() == [True, False, False]
    assert _same(motion[1], np.eye(3)) and _same(motion[2], np.eye(3))
    assert support[1] == 0.0 and support[2] == H / (H * W)
    masked = np.zeros((3, 2, H, W), np.uint8)
    masked[0, 0] = 1                     # every pixel masked
    assert fit_reference_h(f, masked)[1].tolist() == [False, False, False]


def test_fit_with_the_identity_weights_is_support_one():
    f = np.zeros((1, 2, 20, 30))
    motion, ok, support = fit_reference_h(f, iters=3)
    assert ok[0] and support[0] == 1.0 and projective_corner_distance(motion[0], np.eye(3), 20, 30) < 1e-12


def test_rotating_camera_chain():
    """focal length 200 px, 4 degrees of yaw per frame, nine 96 x 160 frames, exact flows.  Measured: the homography chain
    5e-13 px from the exact one at the corners after 8 pairs, the affine chain 82 px"""
    H, W = 96, 160
    A = rotating_camera(9, H, W)
    flows = np.stack([homography_flow(a, H, W) for a in A])
    mh, ok, _ = fit_reference_h(flows, iters=1)
    ma, oka, _ = fit_reference(flows)
    assert ok.all() and oka.all()
    eh = projective_corner_distance(chain(mh), chain(A), H, W)
    ea = projective_corner_distance(chain(ma), chain(A), H, W)
    print("rotating camera, 8 pairs: homography chain %.3g px, affine chain %.3g px" % (eh, ea))
    assert eh < 1e-9 and ea > 50


# ---- the tile culling
@pytest.mark.parametrize("ty", [4, 2, 1])
def test_culling_never_drops_a_live_slot(ty):
    H, W, Hc, Wc = 40, 56, 77, 150
    M = cull_matrices(H, W, Hc, Wc)
    M = [m for m in M] + [m.astype(np.float32) for m in M[:34]]
    dropped = live = 0
    for m in M:
        for xa, xb, ra, rb in tiles(Hc, Wc, ty):
            keep, alive = cull_keep(m, xa, xb, ra, rb, H, W), tile_live(m, xa, xb, ra, rb, H, W)
            assert keep or not alive, (m, xa, xb, ra, rb)
            dropped += not keep
            live += alive
    assert dropped > 0 and live > 0


def test_culling_keeps_fewer_than_all_slots_of_a_panorama():
    """The rotating camera's panorama (9 sources, 64 x 4 tiles).  Measured: the rule keeps 62.7 % of the (tile, slot) pairs,
    60.5 % are live somewhere in their tile"""
    H, W = 96, 160
    A = torch.from_numpy(rotating_camera(9, H, W))
    M, (Hc, Wc), _ = tensors.homography_transforms(A, (H, W))
    M = M[0].numpy()
    kept = alive = total = 0
    for m in M:
        for t in tiles(Hc, Wc, 4):
            k, a = cull_keep(m, *t, H, W), tile_live(m, *t, H, W)
            assert k or not a
            kept, alive, total = kept + k, alive + a, total + 1
    print("culling on the %d x %d panorama: %.1f %% of %d (tile, slot) pairs kept, %.1f %% live" % (
        Wc, Hc, 100.0 * kept / total, total, 100.0 * alive / total))
    assert alive <= kept < total


# ---- matrices whose last row is (0, 0, 1): the bytes of the affine restatements
def _embedded(M2):
    M3 = np.zeros(M2.shape[:-2] + (3, 3), M2.dtype)
    M3[..., :2, :] = M2
    M3[..., 2, 2] = 1.0
    return M3


def _frames(T, H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, H, W, C)).astype(np.uint8)


def _placements(n_out, N, H, W, Hc, Wc, seed):
    """affine (n_out, N, 2, 3): small rotations and scales, shifted over the canvas; one NaN, one far outside"""
    rng = np.random.default_rng(seed)
    M = np.empty((n_out, N, 2, 3))
    for o in range(n_out):
        for k in range(N):
            th, s = rng.normal(0, 0.1), 1 + rng.normal(0, 0.05)
            a, b = s * math.cos(th), s * math.sin(th)
            M[o, k] = [[a, -b, -rng.uniform(-10, Wc - W + 10)], [b, a, -rng.uniform(-10, Hc - H + 10)]]
    M[0, 1, 0, 0] = math.nan
    M[0, 2, :, 2] += 1000.0
    return M


def test_affine_embedded_matrices_give_the_affine_bytes():
    T, H, W, C, Hc, Wc = 5, 20, 28, 3, 37, 70
    f = _frames(T, H, W, C, 6)
    M2 = _placements(2, T, H, W, Hc, Wc, 7)
    masks = np.random.default_rng(8).random((T, H, W)) < 0.1
    gains = np.random.default_rng(9).uniform(0.7, 1.2, (2, T))
    for dt in (np.float64, np.float32):
        m2 = M2.astype(dt)
        m3 = _embedded(m2)
        wo, wv = warp_reference(f, m2[0])
        ho, hv = warp_reference_h(f, m3[0])
        assert _same(wo, ho) and _same(wv, hv)
        for mode in ("first", "mean", "median"):
            a, b = mosaic_reference(f, None, m2, (Hc, Wc), mode, masks), mosaic_reference_h(f, None, m3, (Hc, Wc), mode, masks=masks)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), mode
        for mode in ("first", "mean", "median", "feather"):
            a = blend_reference(f, None, m2, (Hc, Wc), mode, gains, masks, np.uint8)
            b = mosaic_reference_h(f, None, m3, (Hc, Wc), mode, gains, masks, np.uint8)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), mode
        for step in (1, 2):
            a, b = overlap_reference(f, None, m2, (Hc, Wc), step, 1.0, masks), overlap_reference_h(f, None, m3, (Hc, Wc), step, 1.0, masks)
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[1].sum() > 0


def test_projective_rule_known_answers():
    """a horizon in the frame: pixels behind it (D <= 0) are outside, whatever X and Y are; D = 2 halves the point"""
    f = np.arange(24, dtype=np.float64).reshape(1, 4, 6, 1)
    m = np.array([[[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]]])
    out, valid = warp_reference_h(f, m)
    assert valid.all() and _same(out, f)
    m = np.array([[[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]]])  # the same points, every D = -1
    out, valid = warp_reference_h(f, m)
    assert not valid.any() and not out.any()
    m = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-0.5, 0.0, 1.0]]])  # D = 1 - x / 2: 1, 0.5, 0, < 0 ...
    out, valid = warp_reference_h(f, m)
    assert valid[0, 0].tolist() == [True, True, False, False, False, False]  # x = 1 samples X = 2; x = 2 divides by 0
    assert out[0, 0, 1, 0] == f[0, 0, 2, 0] and out[0, 1, 1, 0] == f[0, 2, 2, 0]


# ---- homography_transforms
def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def test_transforms_identity_and_translations():
    M, size, origin = tensors.homography_transforms(_t(np.tile(np.eye(3), (4, 1, 1))), (20, 30))
    assert size == (20, 30) and origin == (0, 0) and tuple(M.shape) == (1, 5, 3, 3)
    assert _same(M[0].numpy(), np.tile(np.eye(3), (5, 1, 1)))
    A2 = np.tile(np.eye(2, 3), (4, 1, 1))
    A2[:, 0, 2], A2[:, 1, 2] = (3.5, -2.0, 4.25, 1.0), (1.0, 2.5, -0.75, 0.0)
    for ref, margin in ((None, 0), (0, 3), (4, 1)):
        Ma, sa, oa = tensors.mosaic_transforms(_t(A2), (20, 30), ref=ref, margin=margin)
        Mh, sh, oh = tensors.homography_transforms(_t(_embedded(A2)), (20, 30), ref=ref, margin=margin)
        assert sa == sh and oa == oh
        assert np.abs(Mh[0, :, :2].numpy() - Ma[0].numpy()).max() < 1e-12 and _same(Mh[0, :, 2].numpy(), np.tile([0.0, 0.0, 1.0], (5, 1)))


def test_transforms_of_the_rotating_chain():
    H, W = 96, 160
    A = rotating_camera(9, H, W)
    M, (Hc, Wc), (x0, y0) = tensors.homography_transforms(_t(A), (H, W))
    M = M[0].numpy()
    assert (M[:, 2, 2] == 1.0).all()
    shift = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])
    assert _same(M[4], shift)  # the reference frame keeps its integer corners
    for t in range(9):  # canvas -> frame t is (reference -> frame t) after the shift
        want = (chain(A[4:t]) if t >= 4 else np.linalg.inv(chain(A[t:4]))) @ shift
        assert projective_corner_distance(M[t], want / want[2, 2], Hc, Wc) < 1e-9
    # every frame's corners land inside the canvas, and touch its edges
    xs, ys = [], []
    for t in range(9):
        inv = np.linalg.inv(M[t])
        for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            p = inv @ np.array([cx, cy, 1.0])
            xs.append(p[0] / p[2])
            ys.append(p[1] / p[2])
    assert -1e-9 <= min(xs) < 1 and -1e-9 <= min(ys) < 1 and Wc - 2 < max(xs) <= Wc - 1 + 1e-9 and Hc - 2 < max(ys) <= Hc - 1 + 1e-9
    ok = torch.ones(8, dtype=torch.bool)
    ok[5] = False  # a failed pair enters as the identity
    Mi = tensors.homography_transforms(tensors.Homography(_t(A), ok, None), (H, W))[0][0].numpy()
    assert _same(Mi[5], Mi[6]) and not _same(Mi[4], Mi[5])


@pytest.mark.parametrize("kw,exc", [
    (dict(motion=torch.zeros(4, 2, 3)), ValueError), (dict(motion=torch.zeros(0, 3, 3)), ValueError), (dict(motion=[1]), TypeError),
    (dict(size=(8,)), TypeError), (dict(size=(0, 8)), ValueError),
    (dict(ref=5), ValueError), (dict(ref=-1), ValueError), (dict(ref=1.0), ValueError),
    (dict(margin=-1), ValueError), (dict(margin=0.5), ValueError),
    (dict(max_pixels=100), ValueError), (dict(max_pixels=0), ValueError),
    (dict(motion=torch.full((4, 3, 3), math.nan, dtype=torch.float64)), ValueError),
    (dict(motion=torch.full((4, 3, 3), 1e200, dtype=torch.float64)), ValueError),
    (dict(motion=torch.zeros(4, 3, 3, dtype=torch.float64)), ValueError),                       # singular
    (dict(motion=_t(rotating_camera(9, 20, 30, focal=40.0, yaw_deg=20.0))), ValueError),         # the horizon: 80 degrees
])
def test_transforms_errors(kw, exc):
    motion = kw.pop("motion", _t(np.tile(np.eye(3), (4, 1, 1))))
    size = kw.pop("size", (20, 30))
    with pytest.raises(exc):
        tensors.homography_transforms(motion, size, **kw)


def test_transforms_refuse_a_negative_scale():
    """a pair motion times a negative number is live nowhere under the sampling rule: dividing by its [2][2] would hide
    that, so it is refused -- as is a chain whose frames all lie behind the reference frame's horizon"""
    A = np.tile(np.eye(3), (4, 1, 1))
    A[1] = -A[1]
    with pytest.raises(ValueError, match=r"\[2\]\[2\]"):
        tensors.homography_transforms(_t(A), (20, 30))
    back = rotating_camera(3, 20, 30, focal=400.0, yaw_deg=85.0)  # frame 1 stays in front of frame 2's horizon; frame 0,
    with pytest.raises(ValueError, match=r"\[2\]\[2\]"):             # 170 degrees away, lies behind it with all four corners
        tensors.homography_transforms(_t(back), (20, 30), ref=2)


def test_transforms_name_the_horizon():
    with pytest.raises(ValueError, match="horizon"):
        tensors.homography_transforms(_t(rotating_camera(9, 20, 30, focal=40.0, yaw_deg=20.0)), (20, 30))


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")


_M = lambda n_out=1, N=3: _z(n_out, N, 3, 3, dtype=torch.float64)  # noqa: E731


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.global_homography(_z(2, 2, 8, 8)), ValueError),                                       # CPU tensors
    (lambda: tensors.warp_homography(_z(3, 3, 8, 8), _z(3, 3, 3)), ValueError),
    (lambda: tensors.mosaic_homography(_z(3, 3, 8, 8), None, _M(), (8, 8)), ValueError),
    (lambda: tensors.mosaic_overlap_homography(_z(3, 3, 8, 8), None, _M(), (8, 8)), ValueError),
    (lambda: tensors.panorama_homography(_z(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.global_homography(None), TypeError),
    (lambda: tensors.warp_homography(None, _z(3, 3, 3)), TypeError),
    (lambda: tensors.mosaic_homography(None, None, _M(), (8, 8)), TypeError),
    (lambda: tensors.mosaic_overlap_homography(None, None, _M(), (8, 8)), TypeError),
    (lambda: tensors.panorama_homography(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(flow=_z(2, 3, 8, 8)), ValueError), (dict(flow=_z(2, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow=[1]), TypeError), (dict(iters=0), ValueError), (dict(iters=1.0), ValueError), (dict(iters=True), ValueError),
    (dict(scale=0.0), ValueError), (dict(scale=math.nan), ValueError), (dict(scale="1"), TypeError),
    (dict(occlusion=_z(2, 2, 8, 8)), TypeError), (dict(occlusion=_z(2, 2, 8, 9, dtype=torch.bool)), ValueError),
    (dict(occlusion=_z(2, 2, 8, 8, dtype=torch.bool, device="meta")), ValueError),
    (dict(model="affine"), TypeError),
])
def test_global_homography_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.global_homography(kw.pop("flow", _z(2, 2, 8, 8)), **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError), (dict(frames=_z(3, 8)), ValueError), (dict(layout="HWC"), ValueError),
    (dict(out_dtype=torch.float16), TypeError),
    (dict(matrices=None), TypeError), (dict(matrices=_z(3, 3, 3, dtype=torch.float16)), TypeError),
    (dict(matrices=_z(3, 2, 3)), ValueError), (dict(matrices=_z(2, 3, 3)), ValueError), (dict(matrices=_z(3, 3, 3, 3)), ValueError),
    (dict(matrices=_z(3, 3, 3, device="meta")), ValueError),
])
def test_warp_homography_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _z(3, 3, 3))
    with pytest.raises(exc):
        tensors.warp_homography(frames, matrices, **kw)
    assert stub == []


_MOSAIC_ERRORS = [
    (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError), (dict(frames=_z(3, 3, 0, 8)), ValueError), (dict(layout="HWC"), ValueError),
    (dict(size=(8,)), TypeError), (dict(size=(0, 8)), ValueError), (dict(size=(8.0, 8)), ValueError),
    (dict(matrices=None), TypeError), (dict(matrices=_z(1, 3, 3, 3, dtype=torch.float16)), TypeError),
    (dict(matrices=_z(1, 3, 2, 3)), ValueError), (dict(matrices=_z(3, 3, 3)), ValueError), (dict(matrices=_z(1, 0, 3, 3)), ValueError),
    (dict(matrices=_z(1, 3, 3, 3, device="meta")), ValueError), (dict(matrices=_M(1, 2)), ValueError),
    (dict(sources=torch.zeros(1, 3)), TypeError), (dict(sources=torch.zeros(2, 3, dtype=torch.int64)), ValueError),
    (dict(sources=[[0, 1, 3]]), ValueError),
    (dict(masks=_z(3, 8, 8)), TypeError), (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError),
    (dict(masks=_z(3, 8, 8, dtype=torch.uint8, device="meta")), ValueError),
]


@pytest.mark.parametrize("kw,exc", _MOSAIC_ERRORS + [
    (dict(out_dtype=torch.float16), TypeError), (dict(mode="max"), ValueError), (dict(mode=2), ValueError),
    (dict(matrices=_M(1, 256), sources=torch.zeros(1, 256, dtype=torch.int32), mode="mean"), ValueError),
    (dict(matrices=_M(1, 256), sources=torch.zeros(1, 256, dtype=torch.int32), mode="feather"), ValueError),
    (dict(matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),                # the median's 64
    (dict(gains=[1.0]), TypeError), (dict(gains=_z(1, 3, dtype=torch.float16)), TypeError), (dict(gains=_z(1, 4)), ValueError),
    (dict(gains=_z(1, 3, device="meta")), ValueError),
])
def test_mosaic_homography_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _M())
    sources, size = kw.pop("sources", None), kw.pop("size", (8, 8))
    with pytest.raises(exc):
        tensors.mosaic_homography(frames, sources, matrices, size, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _MOSAIC_ERRORS + [
    (dict(matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),                # the overlap's 64
    (dict(step=0), ValueError), (dict(step=1.5), ValueError), (dict(bound=0.0), ValueError), (dict(bound="1"), TypeError),
    (dict(bound=math.inf), ValueError),
])
def test_mosaic_overlap_homography_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _M())
    sources, size = kw.pop("sources", None), kw.pop("size", (8, 8))
    with pytest.raises(exc):
        tensors.mosaic_overlap_homography(frames, sources, matrices, size, **kw)
    assert stub == []


def test_the_projective_calls_accept_the_bounds_of_their_slots(monkeypatch):
    """255 sources for the mean and the feather, 64 for the median and the overlap pass every check and reach the launch of
    the projective entry points; the affine calls still refuse 3 x 3 matrices"""
    _on_gpu_stub(monkeypatch)
    reached = []
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *args, **kw: reached.append((name, args[7])))
    f = _z(3, 3, 8, 8)
    tensors.mosaic_homography(f, torch.zeros(1, 255, dtype=torch.int64), _M(1, 255), (4, 4), mode="mean")
    tensors.mosaic_homography(f, torch.zeros(1, 255, dtype=torch.int64), _M(1, 255), (4, 4), mode="feather")
    tensors.mosaic_homography(f, np.zeros((2, 64), np.int16) - 5, _M(2, 64), (4, 4))
    out, cnt = tensors.mosaic_homography(_z(3, 8, 8), [[0]], _M(1, 1), (4, 5), mode="first", layout="NHWC", out_dtype=torch.uint8)
    tensors.mosaic_overlap_homography(f, torch.zeros(1, 64, dtype=torch.int64), _M(1, 64), (4, 4))
    assert reached == [("papof_mosaic_projective_tensor", 255), ("papof_mosaic_projective_tensor", 255),
                       ("papof_mosaic_projective_tensor", 64), ("papof_mosaic_projective_tensor", 1),
                       ("papof_mosaic_overlap_projective_tensor", 64)]
    assert tuple(out.shape) == (1, 4, 5, 8) and out.dtype == torch.uint8 and tuple(cnt.shape) == (1, 4, 5)
    for call in (lambda: tensors.mosaic(f, None, _M(), (8, 8)), lambda: tensors.mosaic_overlap(f, None, _M(), (8, 8)),
                 lambda: tensors.warp_affine(f, _z(3, 3, 3)), lambda: tensors.global_motion(_z(2, 2, 8, 8), model="homography"),
                 lambda: tensors.panorama(f, 2, model="projective")):
        with pytest.raises(ValueError):
            call()


def test_the_count_less_call_passes_a_null_count(monkeypatch):
    """_mosaic(count=False, rule=_PROJECTIVE): the projective entry point with count NULL, and None returned for it"""
    _on_gpu_stub(monkeypatch)
    reached = []
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *args, **kw: reached.append((name, args[-1])))
    f = _z(3, 8, 8, 3)
    ts, descs, _, _ = tensors._check([("frames", f)], "NHWC", None, 1)
    for mode in ("first", "mean", "median", "feather"):
        out, cnt = tensors._mosaic(ts, descs, torch.zeros(1, 3, dtype=torch.int32), _M(), capi.DTYPE_F64, None, 4, 5, mode, "NHWC",
                                   torch.float32, count=False, rule=tensors._PROJECTIVE)
        assert cnt is None and tuple(out.shape) == (1, 4, 5, 3)
    assert reached == [("papof_mosaic_projective_tensor", None)] * 4


@pytest.mark.parametrize("kw,exc", [
    (dict(mode="mode"), ValueError), (dict(ref=3), ValueError), (dict(ref=-1), ValueError), (dict(step=0), ValueError),
    (dict(step=1.0), ValueError), (dict(margin=-1), ValueError), (dict(masks=_z(3, 8, 8)), TypeError),
    (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError), (dict(iters=0), ValueError), (dict(scale=-2.0), ValueError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError), (dict(exposure=1), TypeError),
    (dict(bogus=1), TypeError), (dict(model="affine"), TypeError),
])
def test_panorama_homography_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.panorama_homography(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


def test_panorama_homography_names_step_when_too_many_frames_are_deposited(stub, monkeypatch):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama_homography(_z(65, 1, 8, 8).expand(65, 3, 8, 8), 2)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama_homography(_z(256, 1, 8, 8).expand(256, 3, 8, 8), 2, mode="feather")
    with pytest.raises(ValueError, match="step"):
        tensors.panorama_homography(_z(65, 1, 8, 8).expand(65, 3, 8, 8), 2, mode="mean", exposure=True)
    with pytest.raises(ValueError):
        tensors.panorama_homography(_z(1, 3, 8, 8), 2)
    assert stub == []


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _d(dtype=capi.DTYPE_F64, strides=(192, 24, 3, 1), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_H = ctypes.cast(_FAKE, ctypes.c_void_p)
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731


def test_c_abi_workspace():
    lib = _lib()
    assert lib.papof_homography_workspace(1, 32, 64) == 8 * (12 + 32)
    assert lib.papof_homography_workspace(3, 33, 65) == 8 * 3 * (12 + 32 * 4)
    assert lib.papof_homography_workspace(0, 8, 8) == -1 and lib.papof_homography_workspace(1, 0, 8) == -1


@pytest.mark.parametrize("kw", [
    dict(flow=None), dict(motion=None), dict(ok=None), dict(support=None), dict(flow=_d(data=0)),
    dict(flow=_d(capi.DTYPE_U8)), dict(occ=_d(capi.DTYPE_F32)), dict(motion=_d(capi.DTYPE_F32, (9, 3, 1, 0))),
    dict(ok=_d(capi.DTYPE_F64, (1, 0, 0, 0))), dict(flow=_d(strides=(128, -8, 1, 64))), dict(motion=_d(strides=(9, 3, 0, 0))),
    dict(n_iter=0), dict(scale=0.0), dict(scale=math.nan), dict(n_pairs=0), dict(size=(0, 8)), dict(ws=None), dict(ws_bytes=8),
    dict(h=None),
])
def test_c_abi_refuses_the_fit(kw):
    lib = _lib()
    a = dict(h=_H, n_pairs=2, size=(8, 8), flow=_d(strides=(128, 8, 1, 64)), occ=None, n_iter=5, scale=1.0,
             motion=_d(strides=(9, 3, 1, 0)), ok=_d(capi.DTYPE_U8, (1, 0, 0, 0)), support=_d(strides=(1, 0, 0, 0)), ws=0x5000,
             ws_bytes=1 << 20)
    a.update(kw)
    assert lib.papof_homography_fit_tensor(a["h"], a["n_pairs"], a["size"][0], a["size"][1], _ref(a["flow"]), _ref(a["occ"]),
                                           a["n_iter"], a["scale"], _ref(a["motion"]), _ref(a["ok"]), _ref(a["support"]),
                                           a["ws"], a["ws_bytes"], None) == -1


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(out=None), dict(mat=_d(capi.DTYPE_U8, (9, 3, 1, 0))), dict(out=_d(strides=(192, 24, 3, 0))),
    dict(valid=_d(capi.DTYPE_F64, (64, 8, 1, 0))), dict(n=0), dict(size=(8, 0, 3)), dict(h=None),
])
def test_c_abi_refuses_the_warp(kw):
    lib = _lib()
    a = dict(h=_H, n=2, size=(8, 8, 3), fr=_d(capi.DTYPE_U8), mat=_d(strides=(9, 3, 1, 0)), out=_d(), valid=None)
    a.update(kw)
    assert lib.papof_warp_projective_tensor(a["h"], a["n"], *a["size"], _ref(a["fr"]), _ref(a["mat"]), _ref(a["out"]),
                                            _ref(a["valid"]), None) == -1


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(out=None), dict(sources=None), dict(mat=_d(capi.DTYPE_U8, (27, 9, 3, 1))),
    dict(mat=_d(strides=(27, -9, 3, 1))), dict(gains=_d(capi.DTYPE_U8, (3, 1, 0, 0))), dict(gains=_d(data=0)),
    dict(n_src=0), dict(n_src=256, mode=capi.MOSAIC_MEAN), dict(n_src=256, mode=capi.MOSAIC_FEATHER), dict(n_src=65),
    dict(mode=4), dict(mode=-1), dict(canvas=(0, 9)), dict(h=None),
])
def test_c_abi_refuses_the_mosaic(kw):
    lib = _lib()
    a = dict(h=_H, fr=_d(capi.DTYPE_U8), mat=_d(capi.DTYPE_F32, (27, 9, 3, 1)), out=_d(), sources=0x3000, gains=None, n_src=3,
             mode=capi.MOSAIC_MEDIAN, canvas=(5, 9))
    a.update(kw)
    assert lib.papof_mosaic_projective_tensor(a["h"], 3, 8, 8, 3, _ref(a["fr"]), None, 2, a["n_src"], a["canvas"][0],
                                              a["canvas"][1], a["sources"], _ref(a["mat"]), _ref(a["gains"]), a["mode"],
                                              _ref(a["out"]), None, None) == -1


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(sources=None), dict(n_src=65), dict(n_src=0), dict(step=0), dict(bound=0.0),
    dict(bound=math.inf), dict(sums=None), dict(counts=None), dict(h=None),
])
def test_c_abi_refuses_the_overlap(kw):
    lib = _lib()
    a = dict(h=_H, fr=_d(capi.DTYPE_U8), mat=_d(capi.DTYPE_F32, (27, 9, 3, 1)), sources=0x3000, n_src=3, step=2, bound=1.0,
             sums=0x6000, counts=0x7000)
    a.update(kw)
    assert lib.papof_mosaic_overlap_projective_tensor(a["h"], 3, 8, 8, 3, _ref(a["fr"]), None, 2, a["n_src"], 5, 9, a["sources"],
                                                      _ref(a["mat"]), a["step"], a["bound"], a["sums"], a["counts"], None) == -1


def test_the_constant_is_the_headers():
    import os
    import re
    from _homography_ref import MIN_DEN
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "papof.h")).read()
    assert float(re.search(r"#define PAPOF_HOMOGRAPHY_MIN_DEN (\S+)", header).group(1)) == MIN_DEN


# ---- what the model buys: a rotating camera's panorama under both models
def test_panorama_quality_of_a_rotating_camera():
    """Nine 96 x 160 frames cut from the committed 960 x 540 frame by the exact homographies of a camera of focal length
    200 px that yaws by 4 degrees per frame; the chains are fitted to the exact flows.  PSNR of the mosaic restatement
    against the reference frame's plane, over the pixels both mosaics cover (README records the figures)"""
    frames, Ks, A, world = rotating_scene()
    T, H, W, _ = frames.shape
    flows = np.stack([homography_flow(a, H, W) for a in A])
    mh = fit_reference_h(flows)[0]
    ma = fit_reference(flows)[0]
    Mh, sh, oh = tensors.homography_transforms(_t(mh), (H, W))
    Ma, sa, oa = tensors.mosaic_transforms(_t(ma), (H, W))
    th, ta = canvas_truth(world, Ks[4], oh, sh), canvas_truth(world, Ks[4], oa, sa)
    for mode in ("first", "mean", "median", "feather"):
        ih, ch = mosaic_reference_h(frames, None, Mh.numpy(), sh, mode)
        ia, ca = blend_reference(frames, None, Ma.numpy(), sa, mode)
        ph = psnr(ih[0], th, (ch[0] > 0) & np.isfinite(th).all(-1))
        pa = psnr(ia[0], ta, (ca[0] > 0) & np.isfinite(ta).all(-1))
        print("rotating camera, %s: %.2f dB with the homography chain (%d x %d), %.2f dB with the affine chain (%d x %d)" % (
            mode, ph, sh[1], sh[0], pa, sa[1], sa[0]))
        assert ph > pa, (mode, ph, pa)
