"""CPU-side checks of wide panoramas (papteam_opticalflow_amd/tensors.py: mosaic_rays, mosaic_overlap_rays, estimate_focal,
wide_transforms, panorama_wide; include/papof.h: papof_mosaic_ray_tensor, papof_mosaic_overlap_ray_tensor): the numpy fp64
restatement in tests/_wide_ref.py that tests/test_gpu_wide.py compares the device with -- the bytes of the projective
restatement on the plane's tables, the tile culling against brute-force liveness --, the determinant-normalised chain of
wide_transforms on a 160 degree pan that homography_transforms refuses, its refusals, estimate_focal, the quality of the
cylinder panorama, every Python argument error raised before a launch (CPU tensors, a stubbed handle) and the refusals of the
C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _homography_ref import cull_matrices, mosaic_reference_h, overlap_reference_h, rotating_camera  # noqa: E402
from _mosaic_ref import psnr  # noqa: E402
from _wide_ref import (MODES, cull_keep_rays, cull_tables_and_matrices, cylinder_truth, intrinsics,  # noqa: E402
                       mosaic_reference_rays, overlap_reference_rays, pair_homographies, pan, pitch, plane_tables,
                       project_rays, ray_box, roll, tile_live_rays, tiles, wide_scene, yaw)
from papteam_opticalflow_amd import capi, tensors  # noqa: E402


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


@pytest.fixture(scope="module")
def scene():
    """the wide scene, rendered once: (frames, exact matrices K R_t, exact pair homographies, the texture)"""
    return wide_scene()


# ---- the chain
def test_the_chain_keeps_its_sign_through_a_wide_pan(scene):
    """41 frames at 4 degrees, ref = 20: the canvas-to-frame matrices against the exact K R_t at each frame's four corners.
    Measured: 3.8e-12 px; the [2][2] of frame 0's exact matrix is cos 80 degrees > 0, and past 90 degrees it is negative"""
    _, Ks, A, _ = scene
    H, W = 96, 160
    M, cols, rows, (Hc, Wc), origin = tensors.wide_transforms(_t(A), (H, W), 240.0, ref=20)
    M = M[0].numpy()
    assert M.shape == (41, 3, 3) and tuple(cols.shape) == (Wc, 2) and tuple(rows.shape) == (Hc, 2)
    corners = np.array([[0.0, W - 1.0, 0.0, W - 1.0], [0.0, 0.0, H - 1.0, H - 1.0], [1.0, 1.0, 1.0, 1.0]])
    worst = 0.0
    for t in range(41):
        d = np.linalg.inv(Ks[t]) @ corners  # the rays of frame t's corners
        worst = max(worst, float(np.abs(project_rays(M[t], d) - corners[:2]).max()))
        assert abs(np.linalg.det(M[t]) - 1.0) < 1e-9
    print("wide chain, 40 pairs: %.3g px from the exact matrices at the corners" % worst)
    assert worst < 1e-9
    # one canvas pixel is 1 / f radian, the reference frame's centre looks along theta = 0, and every frame fits
    assert abs(origin[0] * 240.0 - round(origin[0] * 240.0)) < 1e-9
    assert np.abs(cols.numpy()[:, 0] - np.sin(origin[0] + np.arange(Wc) / 240.0)).max() < 1e-12
    assert _same(rows.numpy()[:, 1], np.ones(Hc)) and abs(rows.numpy()[1, 0] - rows.numpy()[0, 0] - 1 / 240.0) < 1e-15
    span = math.degrees((Wc - 1) / 240.0)
    assert 196.6 < span < 197.2, span  # 160 degrees of pan and the field of view, 2 atan(79.5 / 240), rounded out to pixels


def test_a_chain_past_ninety_degrees():
    """61 frames at 4 degrees from ref = 0: 240 degrees of pan; the [2][2] that homography_transforms divides by goes through 0"""
    H, W = 96, 160
    K, Rs = intrinsics(200.0, H, W), pan(61, 0, 4.0)
    A = pair_homographies(K, Rs)
    M = tensors.wide_transforms(_t(A), (H, W), 200.0, ref=0)[0][0].numpy()
    centre = np.array([[(W - 1) / 2.0], [(H - 1) / 2.0], [1.0]])
    for t in range(61):
        d = Rs[t].T @ np.linalg.inv(K) @ centre
        assert float((M[t] @ d)[2, 0]) > 0  # the frame's own centre is in front of it
        assert np.abs(project_rays(M[t], d) - centre[:2]).max() < 1e-9
    assert M[45, 2, 2] < 0 < M[10, 2, 2]


def test_the_planar_call_refuses_the_wide_scene(scene):
    with pytest.raises(ValueError, match="horizon"):
        tensors.homography_transforms(_t(scene[2]), (96, 160), ref=20)


def test_wide_transforms_refusals():
    H, W = 20, 30
    A = np.tile(np.eye(3), (4, 1, 1))
    A[1] = np.diag([1.0, -1.0, 1.0])  # a mirror: determinant -1
    with pytest.raises(ValueError, match="determinant"):
        tensors.wide_transforms(_t(A), (H, W), 40.0)
    A[1] = np.diag([1.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="determinant"):
        tensors.wide_transforms(_t(A), (H, W), 40.0)
    full = pair_homographies(intrinsics(40.0, H, W), pan(91, 45, 4.0))  # 360 degrees between the outer centres
    with pytest.raises(ValueError, match="360"):
        tensors.wide_transforms(_t(full), (H, W), 40.0)
    ok = pair_homographies(intrinsics(40.0, H, W), pan(80, 40, 4.0))    # 316 degrees and the field of view: fits
    _, cols, rows, (Hc, Wc), _ = tensors.wide_transforms(_t(ok), (H, W), 40.0)
    assert (Wc - 1) / 40.0 < 2 * math.pi
    with pytest.raises(ValueError, match="max_pixels"):
        tensors.wide_transforms(_t(ok), (H, W), 40.0, max_pixels=Hc * Wc - 1)
    assert tensors.wide_transforms(_t(ok), (H, W), 40.0, max_pixels=Hc * Wc)[3] == (Hc, Wc)
    up = pair_homographies(intrinsics(40.0, H, W), [pitch(math.radians(45.0 * t)) for t in range(4)])
    with pytest.raises(ValueError):  # frame 3 looks along the cylinder's axis: its heights are not finite, or beyond any canvas
        tensors.wide_transforms(_t(up), (H, W), 40.0, surface="cylinder")
    Hs, Ws = tensors.wide_transforms(_t(up[:2]), (H, W), 40.0, surface="sphere")[3]  # 90 degrees of pitch on a sphere
    assert 90.0 / 180.0 * math.pi * 40.0 < Hs < 125.0 / 180.0 * math.pi * 40.0


def test_margin_ref_and_failed_pairs():
    H, W = 20, 30
    A = pair_homographies(intrinsics(40.0, H, W), pan(9, 4, 20.0))
    M0, c0, r0, (Hc, Wc), o0 = tensors.wide_transforms(_t(A), (H, W), 40.0)
    M3, c3, r3, size3, o3 = tensors.wide_transforms(_t(A), (H, W), 40.0, margin=3)
    assert size3 == (Hc + 6, Wc + 6) and _same(M0.numpy(), M3.numpy()) and _same(c3.numpy()[3:-3], c0.numpy())
    assert abs(o3[0] - (o0[0] - 3 / 40.0)) < 1e-12
    Mr = tensors.wide_transforms(_t(A), (H, W), 40.0, ref=0)[0][0].numpy()
    assert np.abs(Mr[0] - intrinsics(40.0, H, W) / np.cbrt(1600.0)).max() < 1e-12  # the reference frame: K over cbrt(det K)
    okay = torch.ones(8, dtype=torch.bool)
    okay[5] = False
    Mi = tensors.wide_transforms(tensors.Homography(_t(A), okay, None), (H, W), 40.0)[0][0].numpy()
    assert _same(Mi[5], Mi[6]) and not _same(Mi[4], Mi[5])


# ---- the focal length
def test_estimate_focal():
    """exact pairs: a pure yaw (two of the four conditions are 0 / 0 and are skipped), and a camera that yaws, pitches and
    rolls.  Measured: within 1e-13 relative on the yaws, 4e-16 on the other"""
    H, W = 96, 160
    for f in (200.0, 240.0, 777.5):
        got = tensors.estimate_focal(_t(rotating_camera(9, H, W, f, 4.0)), (H, W))
        assert abs(got / f - 1) < 1e-9, (f, got)
    rng = np.random.default_rng(3)
    Rs = [np.eye(3)]
    for _ in range(8):
        Rs.append(yaw(rng.normal(0, 0.08)) @ pitch(0.3 + rng.normal(0, 0.05)) @ roll(rng.normal(0, 0.1)))
    A = pair_homographies(intrinsics(333.0, H, W), Rs)
    got = tensors.estimate_focal(_t(A), (H, W))
    print("estimate_focal, pitched and rolled: %.3g relative" % abs(got / 333.0 - 1))
    assert abs(got / 333.0 - 1) < 1e-9
    okay = torch.zeros(8, dtype=torch.bool)
    okay[2] = True
    assert abs(tensors.estimate_focal(tensors.Homography(_t(A), okay, None), (H, W)) / 333.0 - 1) < 1e-9
    with pytest.raises(ValueError, match="focal="):
        tensors.estimate_focal(_t(np.tile(np.eye(3), (4, 1, 1))), (H, W))
    shift = np.tile(np.eye(3), (4, 1, 1))
    shift[:, 0, 2] = 5.0  # a camera that translates: no rotation to measure
    with pytest.raises(ValueError, match="focal="):
        tensors.estimate_focal(_t(shift), (H, W))
    with pytest.raises(ValueError, match="focal="):
        tensors.estimate_focal(tensors.Homography(_t(A), torch.zeros(8, dtype=torch.bool), None), (H, W))


# ---- the plane's tables: the bytes of the projective restatement
def test_plane_tables_give_the_projective_bytes():
    T, H, W, C, Hc, Wc = 5, 20, 28, 3, 37, 70
    rng = np.random.default_rng(6)
    f = rng.integers(0, 256, (T, H, W, C)).astype(np.uint8)
    M = cull_matrices(H, W, Hc, Wc)[:30].reshape(2, 15, 3, 3)
    src = rng.integers(-1, T, (2, 15))
    masks = rng.random((T, H, W)) < 0.1
    gains = rng.uniform(0.7, 1.2, (2, 15))
    for dt in (np.float64, np.float32):
        m = M.astype(dt)
        cols, rows = plane_tables(Hc, Wc, dt)
        for mode in MODES:
            a = mosaic_reference_h(f, src, m, (Hc, Wc), mode, gains, masks, np.float32)
            b = mosaic_reference_rays(f, src, m, cols, rows, mode, gains, masks, np.float32)
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and int(a[1].max()) >= 2, mode
        for step in (1, 2):
            a = overlap_reference_h(f, src, m, (Hc, Wc), step, 1.0, masks)
            b = overlap_reference_rays(f, src, m, cols, rows, step, 1.0, masks)
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[1].sum() > 0


def test_ray_rule_known_answers():
    """a source in front of the camera and the same matrix negated; a ray along the camera's own axis lands on the principal
    point"""
    f = np.arange(24, dtype=np.float64).reshape(1, 4, 6, 1) / 24.0
    K = np.array([[2.0, 0.0, 2.0], [0.0, 2.0, 1.0], [0.0, 0.0, 1.0]])
    cols = np.array([[math.sin(t), math.cos(t)] for t in (-0.5, 0.0, 0.5, math.pi)])
    rows = np.array([[0.0, 1.0]])
    out, cnt = mosaic_reference_rays(f, None, K[None, None], cols, rows, "first")
    assert cnt[0, 0].tolist() == [1, 1, 1, 0]           # theta = pi looks backwards: D = cos pi < 0
    assert out[0, 0, 1, 0] == f[0, 1, 2, 0]            # theta = 0: the principal point (2, 1)
    assert abs(out[0, 0, 2, 0] - (f[0, 1, 3, 0] + (2 * math.tan(0.5) - 1) / 24.0)) < 1e-12
    out, cnt = mosaic_reference_rays(f, None, -K[None, None], cols, rows, "first")
    assert cnt[0, 0].tolist() == [0, 0, 0, 1]           # the negated matrix sees what lies behind: theta = pi is its axis
    assert abs(out[0, 0, 3, 0] - f[0, 1, 2, 0]) < 1e-12 and not out[0, 0, :3].any()


# ---- the tile culling
@pytest.mark.parametrize("ty", [4, 2, 1])
def test_culling_never_drops_a_live_slot(ty):
    dropped = live = 0
    for what, cols, rows, M in cull_tables_and_matrices():
        for step in (1, 2) if ty == 2 else (1,):  # (the overlap kernel's tiles are 64 x 2 sampled pixels)
            for xs, rs in tiles(len(rows), len(cols), ty, step):
                lo, hi = ray_box(cols, rows, xs, rs)
                for m in M:
                    keep, alive = cull_keep_rays(m, lo, hi, 20, 30), tile_live_rays(m, cols, rows, xs, rs, 20, 30)
                    assert keep or not alive, (what, m, xs[0], rs[0])
                    dropped += not keep
                    live += alive
    assert dropped > 0 and live > 0


def test_culling_keeps_fewer_than_all_slots_of_the_wide_scene(scene):
    """the wide scene's cylinder (41 sources, 64 x 1 tiles -- the median's instance for 41 sources -- and 64 x 4).  Measured:
    64 x 1: 35.4 % of the (tile, slot) pairs kept, 25.1 % live; 64 x 4: 35.5 % kept, 24.9 % live"""
    H, W = 96, 160
    M, cols, rows, (Hc, Wc), _ = tensors.wide_transforms(_t(scene[2]), (H, W), 240.0, ref=20)
    M, cols, rows = M[0].numpy(), cols.numpy(), rows.numpy()
    for ty in (1, 4):
        kept = alive = total = 0
        for xs, rs in tiles(Hc, Wc, ty):
            lo, hi = ray_box(cols, rows, xs, rs)
            for m in M:
                k, a = cull_keep_rays(m, lo, hi, H, W), tile_live_rays(m, cols, rows, xs, rs, H, W)
                assert k or not a
                kept, alive, total = kept + k, alive + a, total + 1
        print("culling on the %d x %d cylinder, 64 x %d tiles: %.1f %% of %d (tile, slot) pairs kept, %.1f %% live" % (
            Wc, Hc, ty, 100.0 * kept / total, total, 100.0 * alive / total))
        assert alive <= kept < total


# ---- the quality of the cylinder panorama
QUALITY = {"first": 42.39, "mean": 45.30, "median": 44.58, "feather": 45.29}  # dB, measured with the restatement (README)


def test_panorama_quality_of_the_wide_scene(scene):
    """exact matrices, every second frame deposited (21 sources): PSNR of the cylinder panorama against the texture resampled
    on the canvas grid, over the covered pixels; each mode is held to its measured figure less 0.5 dB (the computation is
    deterministic; the margin covers the platform's sine and cosine in the tables)"""
    frames, _, A, world = scene
    H, W = 96, 160
    M, cols, rows, size, origin = tensors.wide_transforms(_t(A), (H, W), 240.0, ref=20)
    truth = cylinder_truth(world, origin, size, 240.0)
    src = np.arange(0, 41, 2)[None]
    for mode in MODES:
        img, cnt = mosaic_reference_rays(frames, src, M.numpy()[:, ::2], cols.numpy(), rows.numpy(), mode)
        where = (cnt[0] > 0) & np.isfinite(truth).all(-1)
        p = psnr(img[0], truth, where)
        print("wide scene, %s: %.2f dB over %d pixels of the %d x %d cylinder" % (mode, p, int(where.sum()), size[1], size[0]))
        assert where.sum() > 0.9 * where.size and p > QUALITY[mode] - 0.5, (mode, p)


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
_C = lambda n=8: _z(n, 2, dtype=torch.float64)  # noqa: E731


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.mosaic_rays(_z(3, 3, 8, 8), None, _M(), _C(), _C()), ValueError),                       # CPU tensors
    (lambda: tensors.mosaic_overlap_rays(_z(3, 3, 8, 8), None, _M(), _C(), _C()), ValueError),
    (lambda: tensors.panorama_wide(_z(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.mosaic_rays(None, None, _M(), _C(), _C()), TypeError),
    (lambda: tensors.mosaic_overlap_rays(None, None, _M(), _C(), _C()), TypeError),
    (lambda: tensors.panorama_wide(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_RAY_ERRORS = [
    (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError), (dict(frames=_z(3, 3, 0, 8)), ValueError), (dict(layout="HWC"), ValueError),
    (dict(cols=None), TypeError), (dict(rows=[[0.0, 1.0]]), TypeError), (dict(cols=_z(8, 2, dtype=torch.float16)), TypeError),
    (dict(rows=_z(8, 2, dtype=torch.int32)), TypeError), (dict(cols=_z(8, 3)), ValueError), (dict(rows=_z(8)), ValueError),
    (dict(cols=_z(0, 2)), ValueError), (dict(rows=_z(2, 8, 2)), ValueError), (dict(cols=_z(8, 2, device="meta")), ValueError),
    (dict(rows=_z(8, 2, device="meta")), ValueError),
    (dict(matrices=None), TypeError), (dict(matrices=_z(1, 3, 3, 3, dtype=torch.float16)), TypeError),
    (dict(matrices=_z(1, 3, 2, 3)), ValueError), (dict(matrices=_z(3, 3, 3)), ValueError), (dict(matrices=_z(1, 0, 3, 3)), ValueError),
    (dict(matrices=_z(1, 3, 3, 3, device="meta")), ValueError), (dict(matrices=_M(1, 2)), ValueError),
    (dict(sources=torch.zeros(1, 3)), TypeError), (dict(sources=torch.zeros(2, 3, dtype=torch.int64)), ValueError),
    (dict(sources=[[0, 1, 3]]), ValueError),
    (dict(masks=_z(3, 8, 8)), TypeError), (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError),
    (dict(masks=_z(3, 8, 8, dtype=torch.uint8, device="meta")), ValueError),
]


@pytest.mark.parametrize("kw,exc", _RAY_ERRORS + [
    (dict(out_dtype=torch.float16), TypeError), (dict(mode="max"), ValueError), (dict(mode=2), ValueError),
    (dict(matrices=_M(1, 256), sources=torch.zeros(1, 256, dtype=torch.int32), mode="mean"), ValueError),
    (dict(matrices=_M(1, 256), sources=torch.zeros(1, 256, dtype=torch.int32), mode="feather"), ValueError),
    (dict(matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),                # the median's 64
    (dict(gains=[1.0]), TypeError), (dict(gains=_z(1, 3, dtype=torch.float16)), TypeError), (dict(gains=_z(1, 4)), ValueError),
    (dict(gains=_z(1, 3, device="meta")), ValueError),
])
def test_mosaic_rays_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _M())
    sources, cols, rows = kw.pop("sources", None), kw.pop("cols", _C()), kw.pop("rows", _C(5))
    with pytest.raises(exc):
        tensors.mosaic_rays(frames, sources, matrices, cols, rows, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _RAY_ERRORS + [
    (dict(matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),                # the overlap's 64
    (dict(step=0), ValueError), (dict(step=1.5), ValueError), (dict(bound=0.0), ValueError), (dict(bound="1"), TypeError),
    (dict(bound=math.inf), ValueError),
])
def test_mosaic_overlap_rays_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _M())
    sources, cols, rows = kw.pop("sources", None), kw.pop("cols", _C()), kw.pop("rows", _C(5))
    with pytest.raises(exc):
        tensors.mosaic_overlap_rays(frames, sources, matrices, cols, rows, **kw)
    assert stub == []


def test_the_ray_calls_reach_their_entry_points_with_the_tables_lengths(monkeypatch):
    """255 sources for the mean and the feather, 64 for the median and the overlap pass every check; the canvas is the
    tables' lengths; float32 tables and strided views are handed on as they are"""
    _on_gpu_stub(monkeypatch)
    reached = []
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *args, **kw: reached.append((name, args[7], args[8], args[9])))
    f = _z(3, 3, 8, 8)
    cols, rows = _z(7, 2), _z(10, 4, dtype=torch.float64)[::2, 1:3]
    tensors.mosaic_rays(f, torch.zeros(1, 255, dtype=torch.int64), _M(1, 255), cols, rows, mode="mean")
    tensors.mosaic_rays(f, torch.zeros(1, 255, dtype=torch.int64), _M(1, 255), cols, rows, mode="feather")
    tensors.mosaic_rays(f, np.zeros((2, 64), np.int16) - 5, _M(2, 64), cols, rows)
    out, cnt = tensors.mosaic_rays(_z(3, 8, 8), [[0]], _M(1, 1), cols, rows, mode="first", layout="NHWC", out_dtype=torch.uint8)
    tensors.mosaic_overlap_rays(f, torch.zeros(1, 64, dtype=torch.int64), _M(1, 64), cols, rows)
    assert reached == [("papof_mosaic_ray_tensor", 255, 5, 7)] * 2 + [("papof_mosaic_ray_tensor", 64, 5, 7),
                                                                      ("papof_mosaic_ray_tensor", 1, 5, 7),
                                                                      ("papof_mosaic_overlap_ray_tensor", 64, 5, 7)]
    assert tuple(out.shape) == (1, 5, 7, 8) and out.dtype == torch.uint8 and tuple(cnt.shape) == (1, 5, 7)
    d = tensors._table_struct(rows)
    assert (d.stride[0], d.stride[1], d.dtype) == (8, 1, capi.DTYPE_F64) and tensors._table_struct(cols).dtype == capi.DTYPE_F32


def test_every_rule_reaches_its_entry_point_with_its_argument_list(monkeypatch):
    """the three rules' mosaics and overlaps, with and without gains, under "first" and "feather": which C symbol is reached,
    how many arguments it gets behind the handle, and the two tables behind the matrices (positions 12 and 13) for the ray rule
    alone -- the descriptor of a (Wc, 2) and an (Hc, 2) table there, the gains or the step otherwise"""
    _on_gpu_stub(monkeypatch)
    reached = []
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *args, **kw: reached.append((name, args)))
    f, g = _z(3, 3, 8, 8), torch.ones(1, 3, dtype=torch.float64)
    cols, rows = _z(7, 2, dtype=torch.float64) + 2.0, _z(5, 2, dtype=torch.float64) + 3.0
    for blend, overlap, stem, mats, canvas in (
            (tensors.mosaic, tensors.mosaic_overlap, "", _z(1, 3, 2, 3, dtype=torch.float64), ((5, 7),)),
            (tensors.mosaic_homography, tensors.mosaic_overlap_homography, "_projective", _M(), ((5, 7),)),
            (tensors.mosaic_rays, tensors.mosaic_overlap_rays, "_ray", _M(), (cols, rows))):
        ray = stem == "_ray"
        for gains, mode in ((None, "first"), (None, "feather"), (g, "first"), (g, "feather")):
            del reached[:]
            blend(f, None, mats, *canvas, mode=mode, gains=gains)
            overlap(f, None, mats, *canvas)
            (name, args), (oname, oargs) = reached
            want = "papof_mosaic%s_tensor" % (stem or "_blend")
            if not stem and gains is None and mode == "first":  # the one special case: the call without gains or weights
                want = "papof_mosaic_tensor"
            what = (blend.__name__, gains is not None, mode)
            assert name == want and oname == "papof_mosaic_overlap%s_tensor" % stem, what
            assert len(args) == (15 if name == "papof_mosaic_tensor" else 16) + 2 * ray and len(oargs) == 16 + 2 * ray, what
            assert args[:4] == oargs[:4] == (3, 8, 8, 3) and args[6:10] == oargs[6:10] == (1, 3, 5, 7), what
            for a in (args, oargs):
                assert a[11]._obj.data == mats.data_ptr(), what
                if ray:
                    assert (a[12]._obj.data, a[13]._obj.data) == (cols.data_ptr(), rows.data_ptr()), what
            behind = 12 + 2 * ray
            assert oargs[behind] == 2 and oargs[behind + 1].value == 1.0, what                     # step, bound
            if name == "papof_mosaic_tensor":
                assert args[behind] == tensors.MOSAIC_MODES[mode], what
            else:
                assert (args[behind] is None) == (gains is None) and args[behind + 1] == tensors.MOSAIC_MODES[mode], what
                assert gains is None or args[behind]._obj.data == g.data_ptr(), what


@pytest.mark.parametrize("kw,exc", [
    (dict(motion=torch.zeros(4, 2, 3)), ValueError), (dict(motion=torch.zeros(0, 3, 3)), ValueError), (dict(motion=[1]), TypeError),
    (dict(size=(8,)), TypeError), (dict(size=(0, 8)), ValueError),
    (dict(focal=0.0), ValueError), (dict(focal=-40.0), ValueError), (dict(focal=math.nan), ValueError), (dict(focal="40"), TypeError),
    (dict(focal=True), TypeError), (dict(surface="plane"), ValueError), (dict(surface=None), ValueError),
    (dict(ref=5), ValueError), (dict(ref=-1), ValueError), (dict(ref=1.0), ValueError),
    (dict(margin=-1), ValueError), (dict(margin=0.5), ValueError),
    (dict(max_pixels=100), ValueError), (dict(max_pixels=0), ValueError),
    (dict(motion=torch.full((4, 3, 3), math.nan, dtype=torch.float64)), ValueError),
    (dict(motion=torch.full((4, 3, 3), 1e200, dtype=torch.float64)), ValueError),
    (dict(motion=torch.zeros(4, 3, 3, dtype=torch.float64)), ValueError),                       # singular
])
def test_wide_transforms_errors(kw, exc):
    kw = dict(kw)
    motion = kw.pop("motion", _t(np.tile(np.eye(3), (4, 1, 1))))
    size, focal = kw.pop("size", (20, 30)), kw.pop("focal", 40.0)
    with pytest.raises(exc):
        tensors.wide_transforms(motion, size, focal, **kw)


@pytest.mark.parametrize("kw,exc", [
    (dict(motion=torch.zeros(4, 2, 3)), ValueError), (dict(motion=[1]), TypeError), (dict(size=(8,)), TypeError),
    (dict(size=(0, 8)), ValueError),
])
def test_estimate_focal_errors(kw, exc):
    kw = dict(kw)
    with pytest.raises(exc):
        tensors.estimate_focal(kw.pop("motion", _t(rotating_camera(5, 20, 30))), kw.pop("size", (20, 30)))


@pytest.mark.parametrize("kw,exc", [
    (dict(mode="mode"), ValueError), (dict(ref=3), ValueError), (dict(ref=-1), ValueError), (dict(step=0), ValueError),
    (dict(step=1.0), ValueError), (dict(margin=-1), ValueError), (dict(masks=_z(3, 8, 8)), TypeError),
    (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError), (dict(iters=0), ValueError), (dict(scale=-2.0), ValueError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError), (dict(exposure=1), TypeError),
    (dict(bogus=1), TypeError), (dict(model="affine"), TypeError),
    (dict(focal=0.0), ValueError), (dict(focal="240"), TypeError), (dict(focal=math.inf), ValueError),
    (dict(surface="plane"), ValueError), (dict(surface=1), ValueError),
])
def test_panorama_wide_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.panorama_wide(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


def test_panorama_wide_names_step_when_too_many_frames_are_deposited(stub, monkeypatch):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama_wide(_z(65, 1, 8, 8).expand(65, 3, 8, 8), 2)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama_wide(_z(256, 1, 8, 8).expand(256, 3, 8, 8), 2, mode="feather")
    with pytest.raises(ValueError, match="step"):
        tensors.panorama_wide(_z(65, 1, 8, 8).expand(65, 3, 8, 8), 2, mode="mean", exposure=True)
    with pytest.raises(ValueError):
        tensors.panorama_wide(_z(1, 3, 8, 8), 2)
    assert stub == []


def test_the_named_tuple_extends_panoramas():
    assert tensors.WidePanorama._fields == tensors.Panorama._fields + ("focal", "cols", "rows")
    assert tensors.Panorama._fields == ("image", "count", "matrices", "origin", "motion", "ok", "flow", "timing", "gains")


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
_TABLE = lambda **kw: _d(strides=(2, 1, 0, 0), **kw)  # noqa: E731


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(out=None), dict(sources=None), dict(mat=_d(capi.DTYPE_U8, (27, 9, 3, 1))),
    dict(mat=_d(strides=(27, -9, 3, 1))), dict(gains=_d(capi.DTYPE_U8, (3, 1, 0, 0))), dict(gains=_d(data=0)),
    dict(n_src=0), dict(n_src=256, mode=capi.MOSAIC_MEAN), dict(n_src=256, mode=capi.MOSAIC_FEATHER), dict(n_src=65),
    dict(mode=4), dict(mode=-1), dict(canvas=(0, 9)), dict(h=None),
    dict(cols=None), dict(rows=None), dict(cols=_TABLE(data=0)), dict(rows=_TABLE(data=0)), dict(cols=_TABLE(dtype=capi.DTYPE_U8)),
    dict(rows=_TABLE(dtype=capi.DTYPE_U8)), dict(cols=_d(strides=(-2, 1, 0, 0))), dict(rows=_d(strides=(2, -1, 0, 0))),
])
def test_c_abi_refuses_the_mosaic(kw):
    lib = _lib()
    a = dict(h=_H, fr=_d(capi.DTYPE_U8), mat=_d(capi.DTYPE_F32, (27, 9, 3, 1)), out=_d(), sources=0x3000, gains=None, n_src=3,
             mode=capi.MOSAIC_MEDIAN, canvas=(5, 9), cols=_TABLE(), rows=_TABLE(dtype=capi.DTYPE_F32))
    a.update(kw)
    assert lib.papof_mosaic_ray_tensor(a["h"], 3, 8, 8, 3, _ref(a["fr"]), None, 2, a["n_src"], a["canvas"][0], a["canvas"][1],
                                       a["sources"], _ref(a["mat"]), _ref(a["cols"]), _ref(a["rows"]), _ref(a["gains"]),
                                       a["mode"], _ref(a["out"]), None, None) == -1


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(sources=None), dict(n_src=65), dict(n_src=0), dict(step=0), dict(bound=0.0),
    dict(bound=math.inf), dict(sums=None), dict(counts=None), dict(h=None),
    dict(cols=None), dict(rows=None), dict(cols=_TABLE(data=0)), dict(rows=_TABLE(dtype=capi.DTYPE_U8)),
    dict(cols=_d(strides=(2, -1, 0, 0))),
])
def test_c_abi_refuses_the_overlap(kw):
    lib = _lib()
    a = dict(h=_H, fr=_d(capi.DTYPE_U8), mat=_d(capi.DTYPE_F32, (27, 9, 3, 1)), sources=0x3000, n_src=3, step=2, bound=1.0,
             sums=0x6000, counts=0x7000, cols=_TABLE(), rows=_TABLE())
    a.update(kw)
    assert lib.papof_mosaic_overlap_ray_tensor(a["h"], 3, 8, 8, 3, _ref(a["fr"]), None, 2, a["n_src"], 5, 9, a["sources"],
                                               _ref(a["mat"]), _ref(a["cols"]), _ref(a["rows"]), a["step"], a["bound"],
                                               a["sums"], a["counts"], None) == -1
