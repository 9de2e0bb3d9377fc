"""CPU-side checks of the spatially varying stabilization (papteam_opticalflow_amd/tensors.py: mesh_motion, mesh_transforms,
mesh_profiles, warp_mesh, stabilize_video_mesh; include/papof.h: papof_mesh_motion_tensor, papof_mesh_workspace,
papof_warp_mesh_tensor): known answers of the numpy fp64 restatement in tests/_mesh_ref.py that tests/test_gpu_mesh.py
compares the device's results with, the profiles on the host, the quality of the rule on a synthetic scene whose shake varies
across the image, every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of
the C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _interp_ref import _sample, _taps, as_f64  # noqa: E402
from _mesh_ref import (lattice_step, lower_median, mesh_displacement, mesh_motion_reference, vertex_positions,  # noqa: E402
                       warp_mesh_reference)
from _stab_ref import SIMILARITY, fit_reference, path_reference, warp_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402


# ---- the selection rule
def test_lower_median_is_the_bits_of_one_sample():
    assert lower_median(np.array([3.0, 1.0, 2.0])) == 2.0
    assert lower_median(np.array([4.0, 1.0, 2.0, 3.0])) == 2.0           # rank (n - 1) // 2: the lower of the two
    assert lower_median(np.array([-1.0, -3.0, -2.0, -4.0])) == -3.0
    assert math.copysign(1.0, lower_median(np.array([0.0, -0.0]))) == -1.0  # -0 before +0
    assert lower_median(np.array([math.inf, -math.inf, 5.0])) == 5.0
    assert lower_median(np.array([7.25])) == 7.25


def test_lattice_step_keeps_a_window_within_1024_samples():
    assert lattice_step(33, 47, 4, 5) == 1 and lattice_step(9, 9, 8, 8) == 1
    assert lattice_step(33, 47, 3, 2) == 2        # step 1: (46 + 1) * (21 + 1) = 1034 > 1024
    assert lattice_step(135, 240, 8, 8) == 2      # (59 // 2 + 1) * (33 // 2 + 1) = 30 * 17
    assert lattice_step(135, 240, 2, 2) == 6      # (239 // 6 + 1) * (134 // 6 + 1) = 40 * 23 = 920; step 5: 48 * 27 > 1024
    assert lattice_step(1080, 1920, 16, 16) == 6
    for H, W, g in ((135, 240, (2, 2)), (1080, 1920, (16, 16)), (1080, 1920, (1, 1)), (64, 4000, (1, 3))):
        s = lattice_step(H, W, *g)
        Lx, Ly = 2 * (W - 1) // g[1], 2 * (H - 1) // g[0]
        assert (Lx // s + 1) * (Ly // s + 1) <= 1024
        assert s == 1 or (Lx // (s - 1) + 1) * (Ly // (s - 1) + 1) > 1024


# ---- exactness
def _similarity(scale, deg, tx, ty, H, W):
    a, b = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return np.array([[a, -b, cx - a * cx + b * cy + tx], [b, a, cy - b * cx - a * cy + ty]])


def _field(m, H, W):
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([(m[0, 0] * x + m[0, 1] * r + m[0, 2]) - x, (m[1, 0] * x + m[1, 1] * r + m[1, 2]) - r])[None]


@pytest.mark.parametrize("spatial", [True, False])
def test_an_exactly_affine_flow_has_zero_residuals(spatial):
    H, W, grid = 67, 91, (5, 7)
    A = _similarity(1.02, 3.0, 1.5, -0.75, H, W)
    vert, sup, res = mesh_motion_reference(_field(A, H, W), A[None], None, grid, 16, spatial)
    assert sup.min() >= 16
    assert np.abs(res).max() <= 1e-12
    px, py = vertex_positions(H, W, *grid)
    PX, PY = np.meshgrid(px, py)
    want = np.stack([A[0, 0] * PX + A[0, 1] * PY + A[0, 2] - PX, A[1, 0] * PX + A[1, 1] * PY + A[1, 2] - PY], -1)
    assert np.abs(vert[0] - want).max() <= 1e-12
    # without the global motion the same flow's medians are the flow near the vertices, not zero
    _, _, plain = mesh_motion_reference(_field(A, H, W), None, None, grid, 16, spatial)
    assert np.abs(plain).max() > 1.0


def test_radius_zero_gives_zero_tables_exactly():
    rng = np.random.default_rng(3)
    r = rng.normal(0, 1, (7, 4, 5, 2))
    D = tensors.mesh_profiles(r, 0)
    assert D.shape == (8, 4, 5, 2) and not D.any() and not np.signbit(D).any()
    got = tensors.mesh_transforms(torch.from_numpy(r), 0)
    assert got.dtype == torch.float64 and tuple(got.shape) == (8, 4, 5, 2) and not got.numpy().any()


def test_profiles_are_the_cumulated_residuals_minus_their_gaussian_average():
    rng = np.random.default_rng(4)
    r = rng.normal(0, 1, (9, 2, 3, 2))
    radius = 3
    D = tensors.mesh_profiles(r, radius)
    C = np.concatenate([np.zeros((1, 2, 3, 2)), np.cumsum(r, 0)])
    for t in range(10):
        ks = [k for k in range(-radius, radius + 1) if 0 <= t + k < 10]
        g = np.array([math.exp(-k * k / (2 * (radius / 2) ** 2)) for k in ks])
        S = sum(gk * C[t + k] for gk, k in zip(g, ks)) / g.sum()
        assert np.abs(D[t] - (C[t] - S)).max() < 1e-12
    # a constant residual is a linear profile: the symmetric average leaves the interior frames alone
    lin = tensors.mesh_profiles(np.full((9, 2, 3, 2), 0.5), radius)
    assert np.abs(lin[radius:10 - radius]).max() < 1e-12 and np.abs(lin[0]).max() > 0.1
    # a MeshMotion goes in as its residuals
    mm = tensors.MeshMotion(None, None, torch.from_numpy(r))
    assert np.array_equal(tensors.mesh_transforms(mm, radius).numpy(), D)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_a_zero_mesh_gives_the_bytes_of_the_affine_warp(dtype):
    rng = np.random.default_rng(5)
    B, H, W, C = 3, 19, 26, 2
    f = rng.integers(0, 256, (B, H, W, C)).astype(dtype) if dtype == np.uint8 else rng.random((B, H, W, C)).astype(dtype)
    M = np.array([_similarity(1.1, 7.0, 2.0, -1.0, H, W), np.eye(2, 3), [[1.0, 0.0, -3.5], [0.0, 1.0, 40.0]]])
    for grid in ((1, 1), (3, 4)):
        out, valid = warp_mesh_reference(f, M, np.zeros((B, grid[0] + 1, grid[1] + 1, 2)), dtype)
        want, wvalid = warp_reference(f, M, dtype)
        assert out.tobytes() == want.tobytes() and np.array_equal(valid, wvalid)
    assert not valid[2].any() and valid[1].all() and 0 < valid[0].sum() < H * W


def test_mesh_displacement_is_bilinear_in_the_cell_and_clamped_outside():
    H, W = 21, 31
    D = np.zeros((3, 4, 2))
    D[1, 2] = (2.0, -1.0)
    px, py = vertex_positions(H, W, 2, 3)
    dx, dy = mesh_displacement(np.array([px[2]]), np.array([py[1]]), D, H, W)
    assert dx[0] == 2.0 and dy[0] == -1.0                                  # at the vertex: its own entry
    dx, _ = mesh_displacement(np.array([(px[2] + px[3]) / 2]), np.array([py[1]]), D, H, W)
    assert abs(dx[0] - 1.0) < 1e-12                                        # half way along an edge
    E = np.zeros((3, 4, 2))
    E[:, 0, 0], E[:, 3, 0] = 5.0, 7.0
    dx, _ = mesh_displacement(np.array([-40.0, 1e9, math.inf]), np.array([3.0, 3.0, 3.0]), E, H, W)
    assert dx.tolist() == [5.0, 7.0, 7.0]                                  # outside the mesh: the border's value
    dx, _ = mesh_displacement(np.array([math.nan]), np.array([3.0]), E, H, W)
    assert math.isnan(dx[0])
    N = np.zeros((3, 4, 2))
    N[0, 0, 0] = math.nan
    out, valid = warp_mesh_reference(np.ones((1, H, W, 1)), np.eye(2, 3)[None], N[None])
    assert not valid[0, :int(py[1]), :int(px[1])].any()  # the NaN's cell, x < px[1] = 10 and y < py[1] = 10: weight 0 * NaN too
    assert valid[0, int(py[1]):, :].all() and valid[0, :, int(px[1]):].all()


# ---- robustness
H0, W0, G0 = 135, 240, (8, 8)
T0 = (1.5, -0.75)


def _translation_with_a_region():
    f = np.empty((1, 2, H0, W0))
    f[0, 0], f[0, 1] = T0
    f[0, 0, 50:74, 100:124], f[0, 1, 50:74, 100:124] = 9.0, -6.0
    return f


@pytest.mark.parametrize("spatial", [True, False])
def test_a_moving_region_under_half_of_every_window_leaves_no_trace(spatial):
    f = _translation_with_a_region()
    vert, sup, res = mesh_motion_reference(f, None, None, G0, 16, spatial)
    assert (vert[..., 0] == T0[0]).all() and (vert[..., 1] == T0[1]).all()
    assert vert.tobytes() == res.tobytes()  # no global motion: A v - v = +0
    occ = np.zeros((1, H0, W0), np.uint8)
    occ[0, 50:74, 100:124] = 1
    vert2, sup2, _ = mesh_motion_reference(f, None, occ, G0, 16, spatial)
    assert vert2.tobytes() == vert.tobytes()
    assert (sup2 <= sup).all() and (sup2 < sup).sum() >= 4 and sup2.min() >= 16
    # the window sizes: interior windows hold (59 // 2 + 1) * (33 // 2 + 1) lattice points at most
    assert sup.max() <= 30 * 17 and 144 < sup.max() // 2


def test_a_fully_occluded_window_takes_its_neighbours_median_or_zero():
    rng = np.random.default_rng(6)
    f = np.empty((1, 2, H0, W0))
    f[0, 0], f[0, 1] = T0
    f[0] += rng.normal(0, 0.05, (2, H0, W0))
    px, py = vertex_positions(H0, W0, *G0)
    i, j = 3, 4
    occ = np.zeros((1, H0, W0), np.uint8)
    occ[0, int(py[i - 1]):int(py[i + 1]) + 2, int(px[j - 1]):int(px[j + 1]) + 2] = 1
    vs, sup, rs = mesh_motion_reference(f, None, occ, G0, 16, True)
    vn, _, rn = mesh_motion_reference(f, None, occ, G0, 16, False)
    assert sup[0, i, j] == 0
    assert (rn[0, i, j] == 0).all() and (vn[0, i, j] == 0).all()
    raw = rn[0]  # spatial=False: the valid vertices' own window medians
    ok = sup[0] >= 16
    for c in range(2):
        want = lower_median(np.array([raw[a, b, c] for a in (i - 1, i, i + 1) for b in (j - 1, j, j + 1) if ok[a, b]]))
        assert rs[0, i, j, c] == want and abs(want - T0[c]) < 0.05
    # no valid vertex at all: everything follows the global motion
    A = _similarity(1.01, 1.0, 0.5, 0.25, H0, W0)
    v0, s0, r0 = mesh_motion_reference(f, A[None], np.ones((1, H0, W0), np.uint8), G0, 16, True)
    assert not s0.any() and not r0.any()
    PX, PY = np.meshgrid(px, py)
    assert np.abs(v0[0, ..., 0] - (A[0, 0] * PX + A[0, 1] * PY + A[0, 2] - PX)).max() < 1e-12


def test_nonfinite_and_leaving_samples_do_not_count():
    H, W, grid = 33, 47, (3, 2)
    rng = np.random.default_rng(7)
    f = rng.normal(0, 1, (1, 2, H, W))
    clean = f.copy()
    f[0, 0, 5, ::2] = math.nan
    f[0, 1, 9, ::3] = math.inf
    f[0, 0, 20:23] = 500.0
    drop = ~np.isfinite(f).all(1)[0] | (f[0, 0] == 500.0)
    a = mesh_motion_reference(f, None, None, grid, 16, False)
    b = mesh_motion_reference(clean, None, drop[None].astype(np.uint8), grid, 16, False)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# ---- quality: a scene whose shake varies across the image (parallax-like quadratic terms), exact flows
SCENE_T, SCENE_RADIUS, SCENE_SEED = 24, 6, 20


class _Scene:
    """Camera displacement d_t(x, y) = (a_x + b ((x / W)^2 - 1/3) + c ((y / H)^2 - 1/3), a_y + e ((x / W)(y / H) - 1/4)):
    pixel q of frame t shows the world point q + d_t(q).  a_t is a random walk with steps N(0, 1.5 px); b_t, c_t, e_t are
    N(0, 2 px) per frame."""

    def __init__(self, T=SCENE_T, H=H0, W=W0, seed=SCENE_SEED):
        rng = np.random.default_rng(seed)
        self.T, self.H, self.W = T, H, W
        self.a = np.cumsum(rng.normal(0, 1.5, (T, 2)), 0)
        self.bce = rng.normal(0, 2.0, (T, 3))

    def d(self, t, x, y):
        b, c, e = self.bce[t]
        xn, yn = x / self.W, y / self.H
        return (self.a[t, 0] + b * (xn * xn - 1 / 3) + c * (yn * yn - 1 / 3), self.a[t, 1] + e * (xn * yn - 1 / 4))

    def flows(self):
        """the exact forward flows (T - 1, 2, H, W): q' + d_{t+1}(q') = q + d_t(q), solved to convergence"""
        r, x = np.mgrid[0:self.H, 0:self.W].astype(np.float64)
        out = np.empty((self.T - 1, 2, self.H, self.W))
        for t in range(self.T - 1):
            dx, dy = self.d(t, x, r)
            wx, wy = x + dx, r + dy
            qx, qy = x.copy(), r.copy()
            for _ in range(60):
                ex, ey = self.d(t + 1, qx, qy)
                qx, qy = wx - ex, wy - ey
            ex, ey = self.d(t + 1, qx, qy)
            assert max(np.abs(qx + ex - wx).max(), np.abs(qy + ey - wy).max()) < 1e-10
            out[t] = qx - x, qy - r
        return out

    def shown(self, t, X, Y):
        """the world point that frame t shows at the sampling position (X, Y)"""
        dx, dy = self.d(t, X, Y)
        return X + dx, Y + dy


def _jitter(world):
    """RMS over pixels and interior frames of the second time difference of the world positions (T, 2, H, W)"""
    d2 = world[2:] - 2 * world[1:-1] + world[:-2]
    return float(np.sqrt((d2 ** 2).sum(1).mean()))


def _sampling_points(M, D, H, W):
    """where output pixel q of every frame samples its frame: M_t q, plus the table's displacement when D is given"""
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for t in range(len(M)):
        X0 = (M[t, 0, 0] * x + M[t, 0, 1] * r) + M[t, 0, 2]
        Y0 = (M[t, 1, 0] * x + M[t, 1, 1] * r) + M[t, 1, 2]
        if D is not None:
            dx, dy = mesh_displacement(X0, Y0, D[t], H, W)
            X0, Y0 = X0 + dx, Y0 + dy
        out.append((X0, Y0))
    return out


@pytest.fixture(scope="module")
def scene():
    sc = _Scene()
    flows = sc.flows()
    A, ok, _ = fit_reference(flows, None, SIMILARITY, 5, 1.0)
    assert ok.all()
    M = path_reference(A, SCENE_RADIUS)
    tables = {}
    for spatial in (True, False):
        _, sup, res = mesh_motion_reference(flows, A, None, G0, 16, spatial)
        assert sup.min() >= 16
        tables[spatial] = tensors.mesh_profiles(res, SCENE_RADIUS)
    return sc, flows, A, M, tables


def test_mesh_jitter_is_at_most_half_the_affine_jitter(scene):
    """The issue's prototype measured 3.85 px unstabilized, 0.737 affine, 0.149 mesh without and 0.215 with the spatial
    pass (ratios 0.20 and 0.29); the bar is one half.  This restatement, with the robust similarity fit and the sampling
    lattice, seed 20: printed below and recorded in the README."""
    sc, _, _, M, tables = scene
    H, W, T = sc.H, sc.W, sc.T
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def world(points):
        return np.array([np.stack(sc.shown(t, *points[t])) for t in range(T)])

    plain = _jitter(world([(x, r)] * T))
    affine = _jitter(world(_sampling_points(M, None, H, W)))
    mesh = {s: _jitter(world(_sampling_points(M, tables[s], H, W))) for s in (True, False)}
    print("jitter (px): unstabilized %.3f, affine %.3f, mesh %.3f (no spatial pass), mesh %.3f (3 x 3 pass)"
          % (plain, affine, mesh[False], mesh[True]))
    assert affine < plain
    assert mesh[False] <= 0.5 * affine, (mesh[False], affine)
    assert mesh[True] <= 0.5 * affine, (mesh[True], affine)


def test_mesh_psnr_is_above_the_affine_psnr(scene):
    """Frames of 135 x 240 cut from the committed 960 x 540 frame through d_t, stabilized by the restatements of both rules,
    against the world sampled along the smoothed path (the Gaussian average over time of the positions the unstabilized
    pixels show, where a perfect stabilizer with this kernel would sample).  No bar set in advance: the mesh is higher.
    Printed below and recorded in the README."""
    import cases
    sc, _, _, M, tables = scene
    H, W, T = sc.H, sc.W, sc.T
    world_img = as_f64(cases.load_frame_u8("960", 1))[:, :, 1]
    FH, FW = world_img.shape
    ox, oy = (FW - W) / 2.0, (FH - H) / 2.0
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def sample_world(wx, wy):
        X, Y = wx + ox, wy + oy
        assert X.min() >= 0 and X.max() <= FW - 1 and Y.min() >= 0 and Y.max() <= FH - 1
        return _sample(world_img[None], np.zeros((1, 1, 1), np.int64), _taps(X[None], Y[None], FH, FW))[0]

    frames = np.stack([sample_world(*sc.shown(t, x, r)) for t in range(T)])[..., None]
    seen = np.array([np.stack(sc.shown(t, x, r)) for t in range(T)])
    target = np.empty((T, H, W))
    for t in range(T):
        ks = [k for k in range(-SCENE_RADIUS, SCENE_RADIUS + 1) if 0 <= t + k < T]
        g = np.array([math.exp(-k * k / (2 * (SCENE_RADIUS / 2) ** 2)) for k in ks])
        S = sum(gk * seen[t + k] for gk, k in zip(g, ks)) / g.sum()
        target[t] = sample_world(S[0], S[1])
    aff, va = warp_reference(frames, M)
    psnr = {}
    for name, (out, valid) in (("affine", (aff, va)), ("mesh", warp_mesh_reference(frames, M, tables[True])),
                               ("mesh, no spatial pass", warp_mesh_reference(frames, M, tables[False]))):
        both = valid & va
        mse = ((out[..., 0] - target) ** 2)[both].mean()
        psnr[name] = 10 * math.log10(1.0 / mse)
    print("PSNR against the smoothed path (dB): " + ", ".join("%s %.2f" % kv for kv in psnr.items()))
    assert psnr["mesh"] > psnr["affine"]
    assert psnr["mesh, no spatial pass"] > psnr["affine"]


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _z64(*shape, device="cpu"):
    return _z(*shape, dtype=torch.float64, device=device)


def test_cpu_tensors_are_refused(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    for call in (lambda: tensors.mesh_motion(_z(2, 2, 20, 20)),
                 lambda: tensors.warp_mesh(_z(2, 3, 20, 20), _z(2, 2, 3), _z64(2, 3, 3, 2)),
                 lambda: tensors.stabilize_video_mesh(_z(3, 3, 20, 20), 2)):
        with pytest.raises(ValueError):
            call()
    assert calls == []


@pytest.mark.parametrize("kw,exc", [
    (dict(grid=(0, 4)), ValueError), (dict(grid=(4, 0)), ValueError), (dict(grid=(20, 4)), ValueError),      # H - 1 = 19
    (dict(grid=(4, 30)), ValueError), (dict(grid=(4, -1)), ValueError), (dict(grid=4), TypeError),            # W - 1 = 29
    (dict(grid=(4, 4, 4)), TypeError), (dict(grid=(4.0, 4)), TypeError), (dict(grid=(True, 4)), TypeError),
    (dict(flow=_z(2, 2, 100, 100), grid=(65, 4)), ValueError), (dict(flow=_z(2, 2, 100, 100), grid=(4, 65)), ValueError),
    (dict(flow=_z(2, 2, 20, 30, dtype=torch.float16)), TypeError), (dict(flow=_z(2, 3, 20, 30)), ValueError),
    (dict(flow=_z(2, 20, 30)), ValueError), (dict(flow=[0]), TypeError), (dict(flow=_z(2, 2, 20, 30, device="meta")), ValueError),
    (dict(flow=_z(2, 2, 1, 30)), ValueError),                                                                  # no cell fits
    (dict(min_support=0), ValueError), (dict(min_support=-3), ValueError), (dict(min_support=2.0), ValueError),
    (dict(min_support=True), ValueError), (dict(spatial=1), TypeError), (dict(spatial=None), TypeError),
    (dict(motion=_z(2, 2, 3)), TypeError), (dict(motion=_z64(2, 3, 3)), ValueError), (dict(motion=_z64(3, 2, 3)), ValueError),
    (dict(motion=[1]), TypeError), (dict(motion=_z64(2, 2, 3, device="meta")), ValueError),
    (dict(motion=tensors.Motion(_z64(2, 2, 3), _z(3, dtype=torch.bool), None)), ValueError),
    (dict(occlusion=_z(2, 20, 30)), TypeError), (dict(occlusion=_z(2, 1, 20, 30, dtype=torch.bool)), ValueError),
    (dict(occlusion=_z(3, 20, 30, dtype=torch.uint8)), ValueError), (dict(occlusion=[1]), TypeError),
    (dict(occlusion=_z(2, 20, 30, dtype=torch.bool, device="meta")), ValueError),
])
def test_mesh_motion_errors(stub, kw, exc):
    flow = kw.pop("flow", _z(2, 2, 20, 30))
    kw.setdefault("grid", (4, 4))
    with pytest.raises(exc):
        tensors.mesh_motion(flow, **kw)
    assert stub == []


def test_mesh_motion_accepts_the_largest_grid_of_its_frames(stub, monkeypatch):
    """the bounds are inclusive: the checks pass and the call reaches the launch (recorded here, not made)"""
    launched = []
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *a, **k: launched.append((name, a[1:3], a[6:10])))
    for flow, grid in ((_z(1, 2, 20, 30), (19, 29)), (_z(1, 2, 100, 100), (64, 64)), (_z(1, 2, 2, 2), (1, 1))):
        mm = tensors.mesh_motion(flow, grid=grid, min_support=3, spatial=False)
        assert tuple(mm.vertices.shape) == (1, grid[0] + 1, grid[1] + 1, 2) and mm.support.dtype == torch.int32
        assert launched.pop() == ("papof_mesh_motion_tensor", tuple(flow.shape[2:]), grid + (3, 0))
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(mesh=_z(2, 3, 3, 2)), TypeError), (dict(mesh=None), TypeError), (dict(mesh=_z64(3, 3, 3, 2)), ValueError),
    (dict(mesh=_z64(2, 3, 3)), ValueError), (dict(mesh=_z64(2, 3, 3, 3)), ValueError), (dict(mesh=_z64(2, 1, 3, 2)), ValueError),
    (dict(mesh=_z64(2, 3, 1, 2)), ValueError), (dict(mesh=_z64(2, 21, 3, 2)), ValueError),     # 20 cells on 20 rows
    (dict(mesh=_z64(2, 3, 31, 2)), ValueError), (dict(mesh=_z64(2, 3, 3, 2, device="meta")), ValueError),
    (dict(frames=_z(2, 3, 100, 100), mesh=_z64(2, 66, 3, 2)), ValueError),                       # beyond 64 cells
    (dict(matrices=_z(2, 3, 3)), ValueError), (dict(matrices=_z(3, 2, 3)), ValueError), (dict(matrices=None), TypeError),
    (dict(matrices=_z(2, 2, 3, dtype=torch.float16)), TypeError),
    (dict(frames=_z(2, 3, 20, 30, dtype=torch.int16)), TypeError), (dict(frames=_z(3, 8)), ValueError),
    (dict(layout="HWC"), ValueError), (dict(out_dtype=torch.float16), TypeError),
])
def test_warp_mesh_errors(stub, kw, exc):
    frames, matrices, mesh = kw.pop("frames", _z(2, 3, 20, 30)), kw.pop("matrices", _z(2, 2, 3)), kw.pop("mesh", _z64(2, 3, 3, 2))
    with pytest.raises(exc):
        tensors.warp_mesh(frames, matrices, mesh, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(grid=(0, 2)), ValueError), (dict(grid=(2, 30)), ValueError), (dict(grid=(20, 2)), ValueError), (dict(grid=3), TypeError),
    (dict(min_support=0), ValueError), (dict(spatial="yes"), TypeError),
    (dict(model="projective"), ValueError), (dict(radius=-1), ValueError), (dict(radius=1.5), ValueError),
    (dict(crop=0.0), ValueError), (dict(crop="all"), TypeError), (dict(iters=0), ValueError), (dict(scale=-2.0), ValueError),
    (dict(consistency=(1.0,)), TypeError), (dict(consistency=(-1.0, 0.5)), ValueError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError), (dict(bogus=1), TypeError),
])
def test_stabilize_video_mesh_errors(stub, kw, exc):
    kw.setdefault("grid", (4, 4))
    with pytest.raises(exc):
        tensors.stabilize_video_mesh(_z(3, 3, 20, 30), 2, **kw)
    assert stub == []


def test_stabilize_video_mesh_needs_two_frames_levels_and_a_grid_that_fits(stub):
    with pytest.raises(ValueError):
        tensors.stabilize_video_mesh(_z(1, 3, 20, 30), 2, grid=(4, 4))
    with pytest.raises(ValueError):
        tensors.stabilize_video_mesh(_z(3, 3, 20, 30), 0, grid=(4, 4))
    with pytest.raises(ValueError):
        tensors.stabilize_video_mesh(_z(3, 3, 8, 8), 2)  # the default 16 x 16 grid does not fit 8 x 8 frames
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(mesh_motion=_z64(4, 3, 3)), ValueError), (dict(mesh_motion=_z64(0, 3, 3, 2)), ValueError),
    (dict(mesh_motion=_z64(4, 3, 3, 3)), ValueError), (dict(mesh_motion=_z64(4, 1, 3, 2)), ValueError),
    (dict(mesh_motion=[1]), TypeError), (dict(radius=-2), ValueError), (dict(radius=1.5), ValueError),
    (dict(radius=True), ValueError),
])
def test_mesh_transforms_errors(kw, exc):
    mm = kw.pop("mesh_motion", _z64(4, 3, 3, 2))
    with pytest.raises(exc):
        tensors.mesh_transforms(mm, **kw)


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
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731


def _motion(lib, h, n=2, size=(20, 30), flow=_OK, occ=None, motion=None, grid=(4, 5), min_support=16, spatial=1, vert=_OK,
            res=_OK, support=0x3000, ws=0x2000, ws_bytes=None):
    make = {"flow": lambda: _t(capi.DTYPE_F32, (1200, 30, 1, 600)), "vert": lambda: _t(strides=(60, 12, 2, 1)),
            "res": lambda: _t(strides=(60, 12, 2, 1))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(flow=flow, vert=vert, res=res).items()}
    if ws_bytes is None:
        ws_bytes = max(0, lib.papof_mesh_workspace(n, grid[0], grid[1]))
    return lib.papof_mesh_motion_tensor(h, n, size[0], size[1], _ref(d["flow"]), _ref(occ), _ref(motion), grid[0], grid[1],
                                        min_support, spatial, _ref(d["vert"]), _ref(d["res"]), support, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(flow=None), dict(vert=None), dict(res=None), dict(support=None),                              # NULL
    dict(flow=_t(data=0)), dict(vert=_t(data=0)), dict(res=_t(data=0)), dict(occ=_t(capi.DTYPE_U8, data=0)),
    dict(motion=_t(data=0)),
    dict(flow=_t(capi.DTYPE_U8)), dict(flow=_t(dtype=3)), dict(occ=_t(capi.DTYPE_F32)),                 # dtypes
    dict(motion=_t(capi.DTYPE_F32, (6, 3, 1, 0))), dict(vert=_t(capi.DTYPE_F32, (60, 12, 2, 1))),
    dict(res=_t(capi.DTYPE_U8, (60, 12, 2, 1))),
    dict(flow=_t(strides=(128, -8, 1, 64))), dict(occ=_t(capi.DTYPE_U8, (128, 8, -1, 0))),              # strides
    dict(motion=_t(strides=(6, -3, 1, 0))), dict(vert=_t(strides=(60, 12, 2, 0))), dict(vert=_t(strides=(0, 12, 2, 1))),
    dict(res=_t(strides=(60, 0, 2, 1))), dict(res=_t(strides=(60, 12, -2, 1))),
    dict(grid=(0, 5)), dict(grid=(4, 0)), dict(grid=(20, 5)), dict(grid=(4, 30)), dict(grid=(-1, 5)),   # the grid
    dict(size=(100, 100), grid=(65, 4)), dict(size=(100, 100), grid=(4, 65)),
    dict(min_support=0), dict(min_support=-1),
    dict(n=0), dict(size=(0, 30)), dict(size=(20, -1)), dict(size=(1, 30), grid=(1, 5)),                # sizes
    dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=-1),                                                 # workspace
])
def test_c_abi_mesh_motion_refuses(kw):
    assert _motion(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_mesh_motion_workspace():
    lib = _lib()
    ws = lib.papof_mesh_workspace
    assert ws(1, 1, 1) == 16 * 4 and ws(3, 16, 16) == 16 * 3 * 289 and ws(100, 64, 64) == 16 * 100 * 65 * 65
    assert ws(70000, 64, 64) == 16 * 70000 * 65 * 65  # 64-bit sizes
    assert ws(0, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 4, 65) == -1 and ws(1, 65, 4) == -1
    assert _motion(lib, ctypes.cast(_FAKE, ctypes.c_void_p), ws_bytes=ws(2, 4, 5) - 1) == -1
    assert _motion(lib, None) == -1


def _warp(lib, h, n=2, size=(20, 30, 3), fr=_OK, mat=_OK, mesh=_OK, grid=(4, 5), out=_OK, valid=None):
    make = {"fr": lambda: _t(capi.DTYPE_U8, (1800, 90, 3, 1)), "mat": lambda: _t(capi.DTYPE_F32, (6, 3, 1, 0)),
            "mesh": lambda: _t(strides=(60, 12, 2, 1)), "out": lambda: _t(capi.DTYPE_F64, (1800, 90, 3, 1))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mat=mat, mesh=mesh, out=out).items()}
    return lib.papof_warp_mesh_tensor(h, n, size[0], size[1], size[2], _ref(d["fr"]), _ref(d["mat"]), _ref(d["mesh"]), grid[0],
                                      grid[1], _ref(d["out"]), _ref(valid), None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(mesh=None), dict(out=None),
    dict(fr=_t(data=0)), dict(mat=_t(data=0)), dict(mesh=_t(data=0)), dict(out=_t(data=0)), dict(valid=_t(capi.DTYPE_U8, data=0)),
    dict(fr=_t(dtype=3)), dict(mat=_t(capi.DTYPE_U8, (6, 3, 1, 0))), dict(mesh=_t(capi.DTYPE_F32, (60, 12, 2, 1))),
    dict(out=_t(dtype=-1)), dict(valid=_t(capi.DTYPE_F32, (600, 30, 1, 0))),
    dict(fr=_t(strides=(1800, 90, 3, -1))), dict(mat=_t(strides=(6, -3, 1, 0))), dict(mesh=_t(strides=(60, 12, 2, -1))),
    dict(mesh=_t(strides=(-60, 12, 2, 1))), dict(out=_t(strides=(1800, 90, 3, 0))), dict(out=_t(strides=(0, 90, 3, 1))),
    dict(valid=_t(capi.DTYPE_U8, (600, 30, 0, 0))),
    dict(grid=(0, 5)), dict(grid=(4, 0)), dict(grid=(20, 5)), dict(grid=(4, 30)), dict(size=(100, 100, 3), grid=(65, 5)),
    dict(size=(100, 100, 3), grid=(4, 65)),
    dict(n=0), dict(size=(0, 30, 3)), dict(size=(20, 0, 3)), dict(size=(20, 30, 0)), dict(size=(20, 1, 3), grid=(4, 1)),
])
def test_c_abi_warp_mesh_refuses(kw):
    assert _warp(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_warp_mesh_without_a_handle():
    assert _warp(_lib(), None) == -1
