"""CPU-side checks of video stabilization (papteam_opticalflow_amd/tensors.py: global_motion, warp_affine,
stabilizing_transforms, stabilize_video; include/papof.h: papof_motion_fit_tensor, papof_motion_workspace,
papof_warp_affine_tensor): known answers of the numpy fp64 restatement in tests/_stab_ref.py that tests/test_gpu_stab.py
compares the device's results with, the camera path on the host, every Python argument error raised before a launch (CPU
tensors, a stubbed handle), and each refusal of the C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _stab_ref import (AFFINE, SIMILARITY, corner_distance, fit_reference, path_reference, sums,  # noqa: E402
                       warp_reference)
from papteam_opticalflow_amd import capi, tensors  # noqa: E402

H, W = 45, 64


def _field(m, H=H, W=W):
    """the flow (1, 2, H, W) of an exact motion m (2, 3): flow(x, r) = m (x, r, 1) - (x, r)"""
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    X = m[0, 0] * x + m[0, 1] * r + m[0, 2]
    Y = m[1, 0] * x + m[1, 1] * r + m[1, 2]
    return np.stack([X - x, Y - r])[None]


def _similarity(scale, deg, tx, ty, H=H, W=W):
    """a similarity about the image centre followed by (tx, ty)"""
    a, b = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return np.array([[a, -b, cx - a * cx + b * cy + tx], [b, a, cy - b * cx - a * cy + ty]])


# ---- known answers of the fit
@pytest.mark.parametrize("model", [SIMILARITY, AFFINE])
def test_constant_translation(model):
    want = np.array([[1.0, 0.0, 2.5], [0.0, 1.0, -1.25]])
    m, ok, sup = fit_reference(_field(want), model=model, iters=3)
    assert ok[0] and np.abs(m[0] - want).max() < 1e-12
    assert 0.9 < sup[0] < 1.0  # the pixels whose target leaves the image are left out


@pytest.mark.parametrize("model,m", [
    (SIMILARITY, _similarity(1.02, 1.5, 1.7, -0.8)), (SIMILARITY, _similarity(0.97, -0.4, -3.0, 2.2)),
    (AFFINE, np.array([[1.01, 0.02, 1.5], [-0.015, 0.985, -0.7]])), (AFFINE, _similarity(1.03, 0.9, 0.4, 0.3)),
])
def test_exact_fields_give_their_matrix_at_the_corners(model, m):
    got, ok, _ = fit_reference(_field(m), model=model)
    assert ok[0] and corner_distance(got[0], m, H, W) < 1e-9


def test_masked_nonfinite_and_leaving_pixels_are_left_out():
    rng = np.random.default_rng(1)
    m = np.array([[1.01, 0.02, 1.5], [-0.015, 0.985, -0.7]])
    clean = _field(m) + rng.normal(0, 0.2, (1, 2, H, W))
    bad = clean.copy()
    occ = np.zeros((1, 2, H, W), np.uint8)
    bad[0, :, 5:15, 10:30] = 40.0           # a masked block of garbage that stays in the image
    occ[0, 0, 5:15, 10:30] = 1
    occ[0, 1] = 1                           # channel 1 is not read
    bad[0, 0, 20, ::3] = math.nan
    bad[0, 1, 30, ::4] = math.inf
    bad[0, 0, 40, ::5] = -math.inf
    bad[0, 0, 25:28, :] = 500.0             # targets outside the image
    drop = np.isnan(bad[0, 0]) | np.isinf(bad).any((0, 1)) | (occ[0, 0] != 0) | (bad[0, 0] == 500.0)
    rest = clean.copy()
    rest[0, :, drop] = math.nan             # the fit of the remaining pixels alone
    for model in (SIMILARITY, AFFINE):
        a = fit_reference(bad, occ, model=model)
        b = fit_reference(rest, None, model=model)
        assert (a[0] == b[0]).all() and (a[2] == b[2]).all() and a[1][0] and b[1][0]
    assert sums(bad[0], occ[0, 0], None, 1.0)[12] == sums(rest[0], None, None, 1.0)[12] < H * W - drop.sum() + 1


def test_cauchy_irls_recovers_the_field_through_outliers_and_a_moving_patch():
    """30 % gross outliers (uniform in +-20 px) and a 16 x 16 patch moving its own way; the least-squares start is far off,
    five Cauchy iterations at c = 1 px bring it back.  Measured here on this seed: corner error 0.0161 px (similarity) and
    0.0219 px (affine) at 5 iterations, against 2.03 and 2.42 px for the plain least squares (1 iteration); the bound is
    0.05 px."""
    rng = np.random.default_rng(2)
    Hb, Wb = 90, 128
    for model, m in ((SIMILARITY, _similarity(1.01, 0.8, 2.0, -1.0, Hb, Wb)),
                     (AFFINE, np.array([[1.01, 0.015, 2.0], [-0.01, 0.99, -1.0]]))):
        f = _field(m, Hb, Wb) + rng.normal(0, 0.1, (1, 2, Hb, Wb))
        out = rng.random((Hb, Wb)) < 0.3
        f[0, :, out] += rng.uniform(-20, 20, (int(out.sum()), 2))
        f[0, 0, 30:46, 60:76] = -6.0
        f[0, 1, 30:46, 60:76] = 4.0
        ls = fit_reference(f, model=model, iters=1)[0][0]
        got, ok, sup = fit_reference(f, model=model, iters=5)
        err = corner_distance(got[0], m, Hb, Wb)
        assert ok[0] and err < 0.05, err
        assert corner_distance(ls, m, Hb, Wb) > 20 * err  # the reweighting did the work
        assert 0 < sup[0] < 1


def test_an_all_invalid_pair_is_the_identity_and_not_ok():
    f = np.full((2, 2, H, W), math.nan)
    f[1] = _field(np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.5]]))[0]
    occ = np.zeros((2, 2, H, W), np.uint8)
    m, ok, sup = fit_reference(f, occ)
    assert not ok[0] and (m[0] == np.eye(2, 3)).all() and sup[0] == 0.0
    assert ok[1]
    occ[1, 0] = 1  # masked everywhere
    m, ok, _ = fit_reference(f, occ)
    assert not ok[1] and (m[1] == np.eye(2, 3)).all()
    # a degenerate pair (one valid column: no unique affine motion) fails at its pivot
    g = np.full((1, 2, H, W), math.nan)
    g[0, :, :, 7] = 0.0
    assert not fit_reference(g, model=AFFINE)[1][0]


# ---- known answers of the warp
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_integer_translation_warps_are_exact_shifts(dtype):
    rng = np.random.default_rng(3)
    Hs, Ws, C = 17, 23, 3
    f = rng.integers(0, 256, (2, Hs, Ws, C)).astype(dtype) if dtype == np.uint8 else rng.random((2, Hs, Ws, C)).astype(dtype)
    M = np.array([np.eye(2, 3), [[1.0, 0.0, 3.0], [0.0, 1.0, -2.0]]])
    out, valid = warp_reference(f, M, dtype)
    assert (out[0] == f[0]).all() and valid[0].all()  # the identity copies the bytes, uint8 to uint8 included
    assert out[0].tobytes() == f[0].tobytes()
    want = np.zeros_like(f[1])
    want[2:, :Ws - 3] = f[1][:Hs - 2, 3:]              # out(r, x) = f(r - 2, x + 3)
    assert out[1].tobytes() == want.tobytes()
    assert valid[1].sum() == (Hs - 2) * (Ws - 3)


def test_warp_outside_and_nan_give_zero():
    f = np.ones((1, 5, 6, 1))
    out, valid = warp_reference(f, np.array([[[1.0, 0.0, math.nan], [0.0, 1.0, 0.0]]]))
    assert (out == 0).all() and not valid.any()
    out, valid = warp_reference(f, np.array([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.0]]]))
    assert valid[0, :, :5].all() and not valid[0, :, 5].any() and (out[0, :, :5] == 1.0).all()


# ---- the camera path
def test_a_constant_pan_needs_no_correction_inside_the_window():
    T, R = 40, 6
    A = np.tile(np.array([[1.0, 0.0, 0.6], [0.0, 1.0, -0.3]]), (T - 1, 1, 1))
    M = path_reference(A, R)
    for t in range(R, T - R):
        assert np.abs(M[t] - np.eye(2, 3)).max() < 1e-12, t
    assert np.abs(M[0] - np.eye(2, 3)).max() > 0.1  # the clipped window at the ends does correct


def test_jitter_about_a_fixed_camera_is_cancelled_to_the_windows_residual():
    rng = np.random.default_rng(4)
    T, R = 30, 5
    j = rng.uniform(-2, 2, (T, 2))                     # frame t shows the scene shifted by j_t: K_t = T(j_t)
    A = np.array([[[1.0, 0.0, j[t, 0] - j[t + 1, 0]], [0.0, 1.0, j[t, 1] - j[t + 1, 1]]] for t in range(T - 1)])
    M = path_reference(A, R)
    for t in range(T):
        ks = [k for k in range(-R, R + 1) if 0 <= t + k < T]
        g = np.array([math.exp(-k * k / (2 * (R / 2) ** 2)) for k in ks])
        resid = (g[:, None] * j[[t + k for k in ks]]).sum(0) / g.sum()
        cam = j[t] + M[t][:, 2]                        # the stabilized camera K_t M_t is T(j_t + M_t's translation)
        assert np.abs(M[t][:, :2] - np.eye(2)).max() < 1e-12
        assert np.abs(cam - resid).max() < 1e-12, t
    d2 = lambda p: np.sqrt((np.diff(p, 2, axis=0) ** 2).sum(1).mean())  # noqa: E731
    assert d2(j + M[:, :, 2]) < 0.25 * d2(j)


def test_stabilizing_transforms_is_the_restated_path():
    rng = np.random.default_rng(5)
    T = 12
    A = np.array([_similarity(1 + rng.normal(0, 0.01), rng.normal(0, 0.3), *rng.normal(0, 1.5, 2)) for _ in range(T - 1)])
    for R, crop in ((0, 1.0), (1, 1.0), (4, 0.9), (15, 0.8)):
        got = tensors.stabilizing_transforms(torch.from_numpy(A), R, crop, size=(H, W))
        assert got.dtype == torch.float64 and tuple(got.shape) == (T, 2, 3)
        assert np.abs(got.numpy() - path_reference(A, R, crop, (H, W))).max() < 1e-12
    # a Motion: pairs with ok False enter as the identity
    ok = torch.ones(T - 1, dtype=torch.bool)
    ok[3] = False
    got = tensors.stabilizing_transforms(tensors.Motion(torch.from_numpy(A), ok, torch.ones(T - 1)), 3)
    B = A.copy()
    B[3] = np.eye(2, 3)
    assert np.abs(got.numpy() - path_reference(B, 3)).max() < 1e-12
    # radius 0: no smoothing, every frame is left as it is
    assert np.abs(tensors.stabilizing_transforms(torch.from_numpy(A), 0).numpy() - np.eye(2, 3)).max() < 1e-12


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


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.global_motion(_z(2, 2, 8, 8)), ValueError),                                         # CPU tensors
    (lambda: tensors.warp_affine(_z(2, 3, 8, 8), _z(2, 2, 3)), ValueError),
    (lambda: tensors.stabilize_video(_z(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.global_motion(None), TypeError),
    (lambda: tensors.warp_affine(None, _z(2, 2, 3)), TypeError),
    (lambda: tensors.stabilize_video(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_F = lambda: _z(2, 2, 8, 8)  # noqa: E731


@pytest.mark.parametrize("kw,exc", [
    (dict(flow=_z(2, 2, 8, 8, dtype=torch.float16)), TypeError), (dict(flow=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError),
    (dict(flow=_z(2, 3, 8, 8)), ValueError), (dict(flow=_z(2, 8, 8)), ValueError), (dict(flow=_z(0, 2, 8, 8)), ValueError),
    (dict(flow=[0]), TypeError), (dict(flow=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(occlusion=_z(2, 2, 8, 8)), TypeError), (dict(occlusion=_z(2, 1, 8, 8, dtype=torch.bool)), ValueError),
    (dict(occlusion=[1]), TypeError), (dict(occlusion=_z(2, 2, 8, 8, dtype=torch.bool, device="meta")), ValueError),
    (dict(model="homography"), ValueError), (dict(model=None), ValueError),
    (dict(iters=0), ValueError), (dict(iters=2.0), ValueError), (dict(iters=True), ValueError),
    (dict(scale=0.0), ValueError), (dict(scale=-1.0), ValueError), (dict(scale=math.nan), ValueError),
    (dict(scale=math.inf), ValueError), (dict(scale="1"), TypeError), (dict(scale=None), TypeError),
])
def test_global_motion_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    flow = kw.pop("flow", _F())
    with pytest.raises(exc):
        tensors.global_motion(flow, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(matrices=_z(2, 2, 3, dtype=torch.float16)), TypeError), (dict(matrices=_z(2, 3, 3)), ValueError),
    (dict(matrices=_z(3, 2, 3)), ValueError), (dict(matrices=None), TypeError),
    (dict(matrices=_z(2, 2, 3, device="meta")), ValueError),
    (dict(frames=_z(2, 3, 8, 8, dtype=torch.int16)), TypeError), (dict(frames=_z(3, 8)), ValueError),
    (dict(layout="HWC"), ValueError), (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.bool), TypeError),
])
def test_warp_affine_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    frames, matrices = kw.pop("frames", _z(2, 3, 8, 8)), kw.pop("matrices", _z(2, 2, 3))
    with pytest.raises(exc):
        tensors.warp_affine(frames, matrices, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(model="projective"), ValueError), (dict(radius=-1), ValueError), (dict(radius=1.5), ValueError),
    (dict(crop=0.0), ValueError), (dict(crop=1.1), ValueError), (dict(crop=math.nan), ValueError),
    (dict(crop="all"), TypeError), (dict(iters=0), ValueError), (dict(scale=-2.0), ValueError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError), (dict(bogus=1), TypeError),
])
def test_stabilize_video_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.stabilize_video(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


def test_stabilize_video_needs_two_frames_and_levels(stub, monkeypatch):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(ValueError):
        tensors.stabilize_video(_z(1, 3, 8, 8), 2)
    with pytest.raises(ValueError):
        tensors.stabilize_video(_z(3, 3, 8, 8), 0)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(motion=_z(4, 3, 3)), ValueError), (dict(motion=_z(0, 2, 3)), ValueError), (dict(motion=[1]), TypeError),
    (dict(radius=-2), ValueError), (dict(crop=0.8), ValueError), (dict(crop=0.8, size=(8,)), TypeError),
    (dict(crop=0.8, size=(0, 8)), ValueError),
])
def test_stabilizing_transforms_errors(kw, exc):
    motion = kw.pop("motion", _z(4, 2, 3, dtype=torch.float64))
    with pytest.raises(exc):
        tensors.stabilizing_transforms(motion, **kw)


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_F64, strides=(128, 8, 1, 64), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_OK = "ok"


def _fit(lib, h, n=2, size=(8, 8), flow=_OK, occ=None, model=capi.MOTION_AFFINE, iters=3, scale=1.0, motion=_OK, ok=_OK,
         support=_OK, ws=0x2000, ws_bytes=None):
    make = {"flow": lambda: _t(capi.DTYPE_F32), "motion": lambda: _t(strides=(6, 3, 1, 0)),
            "ok": lambda: _t(capi.DTYPE_U8, (1, 0, 0, 0)), "support": lambda: _t(strides=(1, 0, 0, 0))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(flow=flow, motion=motion, ok=ok, support=support).items()}
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    if ws_bytes is None:
        ws_bytes = max(0, lib.papof_motion_workspace(n, size[0], size[1]))
    return lib.papof_motion_fit_tensor(h, n, size[0], size[1], ref(d["flow"]), ref(occ), model, iters, scale, ref(d["motion"]),
                                       ref(d["ok"]), ref(d["support"]), ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(flow=None), dict(motion=None), dict(ok=None), dict(support=None),                            # NULL descriptors
    dict(flow=_t(data=0)), dict(motion=_t(data=0)), dict(ok=_t(capi.DTYPE_U8, data=0)), dict(support=_t(data=0)),
    dict(occ=_t(capi.DTYPE_U8, data=0)),
    dict(flow=_t(capi.DTYPE_U8)), dict(flow=_t(dtype=3)),                                             # dtypes
    dict(occ=_t(capi.DTYPE_F32)), dict(motion=_t(capi.DTYPE_F32, (6, 3, 1, 0))), dict(ok=_t(capi.DTYPE_F64, (1, 0, 0, 0))),
    dict(support=_t(capi.DTYPE_F32, (1, 0, 0, 0))),
    dict(flow=_t(strides=(128, -8, 1, 64))), dict(flow=_t(strides=(128, 8, 1, -64))),                 # strides
    dict(occ=_t(capi.DTYPE_U8, (128, 8, -1, 64))),
    dict(motion=_t(strides=(0, 3, 1, 0))), dict(motion=_t(strides=(6, 0, 1, 0))), dict(motion=_t(strides=(6, 3, -1, 0))),
    dict(ok=_t(capi.DTYPE_U8, (0, 0, 0, 0))), dict(support=_t(strides=(-1, 0, 0, 0))),
    dict(model=2), dict(model=-1), dict(iters=0), dict(iters=-3),                                      # model, iterations
    dict(scale=0.0), dict(scale=-1.0), dict(scale=math.nan), dict(scale=math.inf),                     # scale
    dict(n=0), dict(size=(0, 8)), dict(size=(8, -1)),                                                  # sizes
    dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=-1),                                                # workspace
])
def test_c_abi_fit_refuses(kw):
    lib = _lib()
    assert _fit(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_fit_refuses_a_workspace_one_byte_short():
    lib = _lib()
    need = lib.papof_motion_workspace(2, 8, 8)
    assert _fit(lib, ctypes.cast(_FAKE, ctypes.c_void_p), ws_bytes=need - 1) == -1
    assert _fit(lib, None) == -1


def _warp(lib, h, n=2, size=(8, 8, 3), fr=_OK, mat=_OK, out=_OK, valid=None):
    make = {"fr": lambda: _t(capi.DTYPE_U8, (192, 24, 3, 1)), "mat": lambda: _t(capi.DTYPE_F32, (6, 3, 1, 0)),
            "out": lambda: _t(capi.DTYPE_F64, (192, 24, 3, 1))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mat=mat, out=out).items()}
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return lib.papof_warp_affine_tensor(h, n, size[0], size[1], size[2], ref(d["fr"]), ref(d["mat"]), ref(d["out"]),
                                        ref(valid), None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(out=None),
    dict(fr=_t(data=0)), dict(mat=_t(data=0)), dict(out=_t(data=0)), dict(valid=_t(capi.DTYPE_U8, data=0)),
    dict(fr=_t(dtype=3)), dict(mat=_t(capi.DTYPE_U8, (6, 3, 1, 0))), dict(out=_t(dtype=-1)),
    dict(valid=_t(capi.DTYPE_F32, (64, 8, 1, 0))),
    dict(fr=_t(strides=(192, 24, 3, -1))), dict(mat=_t(strides=(6, -3, 1, 0))),
    dict(out=_t(strides=(192, 24, 3, 0))), dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(192, 24, -3, 1))),
    dict(valid=_t(capi.DTYPE_U8, (64, 8, 0, 0))), dict(valid=_t(capi.DTYPE_U8, (0, 8, 1, 0))),
    dict(n=0), dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)),
])
def test_c_abi_warp_refuses(kw):
    lib = _lib()
    assert _warp(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_warp_without_a_handle():
    assert _warp(_lib(), None) == -1


def test_workspace_sizes():
    lib = _lib()
    ws = lib.papof_motion_workspace
    assert ws(1, 1, 1) == 8 * (8 + 16)
    assert ws(1, 1080, 1920) == 8 * (8 + 16 * 30 * 34)
    assert ws(100, 135, 240) == 8 * 100 * (8 + 16 * 4 * 5)
    assert ws(3, 32, 64) == 8 * 3 * (8 + 16) and ws(3, 33, 65) == 8 * 3 * (8 + 16 * 4)
    assert ws(0, 8, 8) == -1 and ws(1, 0, 8) == -1 and ws(1, 8, -1) == -1
    assert ws(70000, 135, 240) == 8 * 70000 * (8 + 16 * 20)  # 64-bit sizes, more pairs than one launch takes


def test_version():
    assert _lib().papof_version() >= 113
