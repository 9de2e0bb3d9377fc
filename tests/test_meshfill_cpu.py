"""CPU-side checks of the full-frame mesh stabilization (papteam_opticalflow_amd/tensors.py: mosaic_mesh, neighbour_mesh,
stabilize_video_mesh_full; include/papof.h: papof_mosaic_mesh_tensor, papof_mosaic_mesh_workspace): the two invariants of the
numpy fp64 restatement in tests/_meshfill_ref.py that tests/test_gpu_meshfill.py compares the device's results with, the
tables on the host, how well a filling neighbour registers on test_mesh_cpu's scene, every Python argument error raised before
a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _blend_ref import blend_reference  # noqa: E402
from _interp_ref import _sample, _taps, as_f64  # noqa: E402
from _mesh_ref import mesh_motion_reference, warp_mesh_reference  # noqa: E402
from _meshfill_ref import gather_mesh, mosaic_mesh_reference, neighbour_mesh_reference  # noqa: E402
from _mosaic_ref import mosaic_reference, neighbour_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from test_mesh_cpu import G0, SCENE_RADIUS, _FAKE, _lib, _ref, _similarity, _t, _z, _z64, scene, stub  # noqa: E402, F401

FILL = 2


# ---- the two invariants of the rule
def _case(dtype, seed=11, T=4, H=19, W=26, C=2, n_out=2, N=3, size=(23, 31)):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (T, H, W, C)).astype(dtype) if dtype == np.uint8 else rng.random((T, H, W, C)).astype(dtype)
    M = np.empty((n_out, N, 2, 3))
    for o in range(n_out):
        for k in range(N):
            M[o, k] = _similarity(1.0 + 0.05 * k, 4.0 * k - 3.0 * o, 2.0 * k - 3.0, 1.5 * o - 2.0, H, W)
    src = rng.integers(-1, T, (n_out, N))
    src[0, 0] = 0
    masks = (rng.random((T, H, W)) < 0.05).astype(np.uint8)
    gains = rng.uniform(0.5, 1.5, (n_out, N))
    return f, src, M, masks, gains, size


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("mode", ["first", "mean", "median", "feather"])
def test_invariant_a_zero_tables_give_the_bytes_of_the_blend_call(dtype, mode):
    f, src, M, masks, gains, size = _case(dtype)
    for grid in ((1, 1), (3, 4)):
        Z = np.zeros((2, 3, grid[0] + 1, grid[1] + 1, 2))
        for g, mk in ((None, None), (gains, None), (None, masks), (gains, masks)):
            out, cnt = mosaic_mesh_reference(f, src, M, Z, size, mode, g, mk, dtype)
            want, wcnt = blend_reference(f, src, M, size, mode, g, mk, dtype)
            assert out.tobytes() == want.tobytes() and np.array_equal(cnt, wcnt)
            assert 0 < (cnt > 0).sum() < cnt.size
    if mode != "feather":  # and without gains those are papof_mosaic_tensor's
        want, wcnt = mosaic_reference(f, src, M, size, mode, None, dtype)
        out, cnt = mosaic_mesh_reference(f, src, M, Z, size, mode, None, None, dtype)
        assert out.tobytes() == want.tobytes() and np.array_equal(cnt, wcnt)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_invariant_b_one_slot_per_frame_is_the_mesh_warp(dtype):
    rng = np.random.default_rng(12)
    B, H, W, C = 3, 19, 26, 2
    f = rng.integers(0, 256, (B, H, W, C)).astype(dtype) if dtype == np.uint8 else rng.random((B, H, W, C)).astype(dtype)
    M = np.array([_similarity(1.1, 7.0, 2.0, -1.0, H, W), np.eye(2, 3), [[1.0, 0.0, -3.5], [0.0, 1.0, 40.0]]])
    D = rng.normal(0, 2.0, (B, 4, 5, 2))
    D[1, 0, 0, 0] = math.nan
    out, cnt = mosaic_mesh_reference(f, np.arange(B)[:, None], M[:, None], D[:, None], (H, W), "first", None, None, dtype)
    want, valid = warp_mesh_reference(f, M, D, dtype)
    assert out.tobytes() == want.tobytes() and np.array_equal(cnt, valid.astype(np.uint8))
    assert not valid[2].any() and 0 < valid[0].sum() < H * W and 0 < valid[1].sum() < H * W


def test_a_table_moves_a_source_into_and_out_of_the_frame():
    H, W = 9, 12
    f = np.ones((1, H, W, 1))
    M = np.array([[[[1.0, 0.0, -20.0], [0.0, 1.0, 0.0]]]])  # every pixel 8 or more to the left of the frame
    _, cnt = mosaic_mesh_reference(f, [[0]], M, np.zeros((1, 1, 2, 2, 2)), (H, W), "first")
    assert not cnt.any()
    D = np.zeros((1, 1, 2, 2, 2))
    D[..., 0] = 20.0
    out, cnt = mosaic_mesh_reference(f, [[0]], M, D, (H, W), "first")
    assert cnt.all() and (out == 1.0).all()
    D[..., 0] = -math.inf
    assert not mosaic_mesh_reference(f, [[0]], np.tile(np.eye(2, 3), (1, 1, 1, 1)), D, (H, W), "first")[1].any()


# ---- the tables on the host
def test_neighbour_mesh_is_its_restatement_and_slot_0_is_mesh_profiles():
    rng = np.random.default_rng(13)
    r = rng.normal(0, 1, (8, 3, 4, 2))
    for radius, fill in ((3, 2), (0, 1), (5, 0), (2, 9)):
        D = tensors.mesh_profiles(r, radius)
        E = tensors.neighbour_mesh(torch.from_numpy(r), radius, fill)
        assert E.dtype == torch.float64 and tuple(E.shape) == (9, 2 * fill + 1, 3, 4, 2)
        E = E.numpy()
        assert E.tobytes() == neighbour_mesh_reference(r, D, fill).tobytes()
        assert E[:, 0].tobytes() == D.tobytes()
        assert np.array_equal(tensors.neighbour_mesh(tensors.MeshMotion(None, None, torch.from_numpy(r)), radius, fill).numpy(), E)
        # the shape of neighbour_transforms's slots: the same sources, and +0.0 where there is none
        src, _ = tensors.neighbour_transforms(torch.from_numpy(np.tile(np.eye(2, 3), (9, 1, 1))),
                                              torch.from_numpy(np.tile(np.eye(2, 3), (8, 1, 1))), fill)
        assert tuple(src.shape) == E.shape[:2]
        dead = src.numpy() < 0
        assert not E[dead].any() and not np.signbit(E[dead]).any()
        if fill:
            assert dead.any() and E[~dead].any()
    # E[t, slot of s] - E[t, 0] is what the vertices moved between t and s beyond the global motion
    C = np.concatenate([np.zeros((1, 3, 4, 2)), np.cumsum(r, 0)])
    E = tensors.neighbour_mesh(torch.from_numpy(r), 3, 2).numpy()
    assert np.abs((E[4, 3] - E[4, 0]) - (C[2] - C[4])).max() < 1e-12 and np.abs((E[4, 4] - E[4, 0]) - (C[6] - C[4])).max() < 1e-12


def test_zero_residuals_give_zero_tables_exactly():
    E = tensors.neighbour_mesh(torch.zeros(6, 3, 3, 2, dtype=torch.float64), 4, 3).numpy()
    assert E.shape == (7, 7, 3, 3, 2) and not E.any() and not np.signbit(E).any()


def test_mesh_profiles_are_unchanged_by_the_shared_accumulation():
    """the parent's mesh_profiles, restated: the same bits"""
    rng = np.random.default_rng(14)
    r = rng.normal(0, 1, (9, 2, 3, 2))
    for radius in (0, 1, 4):
        n = 10
        C = np.zeros((n, 2, 3, 2))
        for t in range(n - 1):
            C[t + 1] = C[t] + r[t]
        D = np.zeros_like(C)
        if radius:
            for t in range(n):
                ks = range(max(-radius, -t), min(radius, n - 1 - t) + 1)
                g = [math.exp(-k * k / (2.0 * (radius / 2.0) ** 2)) for k in ks]
                D[t] = C[t] - sum(gk * C[t + k] for gk, k in zip(g, ks)) / sum(g)
        assert tensors.mesh_profiles(r, radius).tobytes() == D.tobytes()


# ---- quality: how well a filling neighbour registers on test_mesh_cpu's scene (24 frames of 135 x 240, exact flows)
def _fill_points(sc, A, M, E):
    """per frame t the points of the walk under the tables E (T, N, GH + 1, GW + 1, 2): (X, Y (N, H * W) the moved points, live (N,
    H * W))"""
    src, mats = neighbour_reference(M, A, FILL)
    one = np.zeros((sc.T, sc.H, sc.W, 1))
    _, live, X, Y, o = gather_mesh(one, src, mats, E, (sc.H, sc.W))
    return src, live, X, Y, o


def _registration(sc, A, M, E_own, E_fill):
    """(RMS distance in px between the world point the filling neighbour shows -- under the tables E_fill -- and the world point
    the mesh-stabilized frame (tables E_own, slot 0) would show there, the share of its invalid pixels that are filled)"""
    src, live_own, X_own, Y_own, o = _fill_points(sc, A, M, E_own)
    _, live, X, Y, _ = _fill_points(sc, A, M, E_fill)
    invalid = ~live_own[0]
    first = np.argmax(live[1:], 0) + 1
    filled = invalid & live[1:].any(0)
    p = np.nonzero(filled)[0]
    k = first[p]
    t, s = o[p], src[o[p], k]
    err2 = np.empty(p.size)
    for frame in range(sc.T):  # the scene's d is per frame
        for source in range(sc.T):
            sel = (t == frame) & (s == source)
            if sel.any():
                wx, wy = sc.shown(frame, X_own[0, p[sel]], Y_own[0, p[sel]])
                nx, ny = sc.shown(source, X[k[sel], p[sel]], Y[k[sel], p[sel]])
                err2[sel] = (nx - wx) ** 2 + (ny - wy) ** 2
    return float(np.sqrt(err2.mean())), filled.sum() / invalid.sum()


@pytest.fixture(scope="module")
def fill_tables(scene):  # noqa: F811
    sc, flows, A, M, _ = scene
    tables = {}
    for spatial in (True, False):
        _, _, res = mesh_motion_reference(flows, A, None, G0, 16, spatial)
        tables[spatial] = tensors.neighbour_mesh(torch.from_numpy(res), SCENE_RADIUS, FILL).numpy()
    return tables


@pytest.mark.parametrize("spatial", [True, False])
def test_a_filling_neighbour_registers_twice_as_well_with_its_table(scene, fill_tables, spatial):  # noqa: F811
    """The issue's prototype, fill radius 2: 1.305 px with neighbour_transforms's matrix alone and 0.458 px with E under the
    3 x 3 spatial pass (0.35 of it, 96.8 % of the invalid pixels filled), 1.292 and 0.312 px without the pass (0.24, 96.5 %);
    the bars are one half and 90 %.  This restatement (robust similarity fit, sampling lattice, seed 20): 1.334 and 0.458 px
    (0.34, 96.8 %) with the pass, 1.306 and 0.312 px (0.24, 96.5 %) without; frame t's own table on every slot: 2.060 and
    2.046 px, worse than none.  Printed below and recorded in the README."""
    sc, _, A, M, _ = scene
    E = fill_tables[spatial]
    alone = E.copy()
    alone[:, 1:] = 0.0      # the neighbours by their matrices alone; slot 0, the frame itself, keeps its table
    own = np.repeat(E[:, :1], E.shape[1], 1)  # frame t's table on every slot
    rms_alone, _ = _registration(sc, A, M, E, alone)
    rms_own, _ = _registration(sc, A, M, E, own)
    rms_e, share = _registration(sc, A, M, E, E)
    print("registration of the fill (px RMS), spatial pass %s: matrix alone %.3f, frame t's table on every slot %.3f, "
          "with E %.3f (%.2f of the matrix alone), %.1f %% of the invalid pixels filled"
          % (spatial, rms_alone, rms_own, rms_e, rms_e / rms_alone, 100 * share))
    assert rms_e <= 0.5 * rms_alone, (rms_e, rms_alone)
    assert share >= 0.9, share


def test_mesh_fill_psnr_is_above_the_affine_registered_fill(scene, fill_tables):  # noqa: F811
    """Frames of 135 x 240 cut from the committed 960 x 540 frame through d_t, as test_mesh_psnr_is_above_the_affine_psnr cuts
    them; over the FILLED pixels, against the world at the mesh-stabilized frame's own sampling points (the analytic d_t
    reaches beyond the frame).  No bar set in advance: the fill registered by E is above the fill registered by the matrices
    alone: 30.30 dB against 23.00 dB over 15008 pixels.  Printed below and recorded in the README."""
    import cases
    sc, _, A, M, _ = scene
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
    E = fill_tables[True]
    alone = E.copy()
    alone[:, 1:] = 0.0
    src, mats = neighbour_reference(M, A, FILL)
    _, live, X, Y, _ = gather_mesh(frames, src, mats, E, (H, W))
    target = np.stack([sample_world(*sc.shown(t, X[0].reshape(T, H, W)[t], Y[0].reshape(T, H, W)[t])) for t in range(T)])
    valid = live[0].reshape(T, H, W)
    psnr = {}
    filled = {}
    for name, tables in (("mesh", E), ("affine", alone)):
        out, cnt = mosaic_mesh_reference(frames, src, mats, tables, (H, W), "first")
        filled[name] = (cnt > 0) & ~valid
        psnr[name] = out[..., 0]
    both = filled["mesh"] & filled["affine"]
    assert both.sum() > 1000
    psnr = {k: 10 * math.log10(1.0 / ((v - target) ** 2)[both].mean()) for k, v in psnr.items()}
    print("PSNR over the filled pixels (dB): registered by E %.2f, by the matrices alone %.2f (%d pixels)"
          % (psnr["mesh"], psnr["affine"], both.sum()))
    assert psnr["mesh"] > psnr["affine"]


# ---- Python argument errors, before any launch
def test_cpu_tensors_are_refused(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    for call in (lambda: tensors.mosaic_mesh(_z(2, 3, 20, 30), None, _z(1, 2, 2, 3), _z64(1, 2, 3, 3, 2), (20, 30)),
                 lambda: tensors.stabilize_video_mesh_full(_z(3, 3, 20, 30), 2, grid=(4, 4))):
        with pytest.raises(ValueError):
            call()
    assert calls == []


@pytest.mark.parametrize("kw,exc", [
    (dict(mesh=_z(1, 2, 3, 3, 2)), TypeError), (dict(mesh=None), TypeError), (dict(mesh=_z64(2, 3, 3, 2)), ValueError),
    (dict(mesh=_z64(2, 2, 3, 3, 2)), ValueError), (dict(mesh=_z64(1, 3, 3, 3, 2)), ValueError),
    (dict(mesh=_z64(1, 2, 3, 3, 3)), ValueError), (dict(mesh=_z64(1, 2, 1, 3, 2)), ValueError),
    (dict(mesh=_z64(1, 2, 3, 1, 2)), ValueError), (dict(mesh=_z64(1, 2, 21, 3, 2)), ValueError),   # 20 cells on 20 rows
    (dict(mesh=_z64(1, 2, 3, 31, 2)), ValueError), (dict(mesh=_z64(1, 2, 3, 3, 2, device="meta")), ValueError),
    (dict(frames=_z(2, 3, 100, 100), mesh=_z64(1, 2, 66, 3, 2)), ValueError),                        # beyond 64 cells
    (dict(size=(0, 30)), ValueError), (dict(size=30), TypeError), (dict(size=(20.0, 30)), ValueError),
    (dict(matrices=_z(1, 2, 3, 3)), ValueError), (dict(matrices=_z(2, 2, 3)), ValueError), (dict(matrices=None), TypeError),
    (dict(matrices=_z(1, 2, 2, 3, dtype=torch.float16)), TypeError),
    (dict(sources=[[0, 2]]), ValueError), (dict(sources=[[0.0, 1.0]]), TypeError), (dict(sources=[[0, 1, 1]]), ValueError),
    (dict(sources=None, matrices=_z(1, 3, 2, 3), mesh=_z64(1, 3, 3, 3, 2)), ValueError),
    (dict(mode="max"), ValueError), (dict(masks=_z(2, 20, 30)), TypeError), (dict(masks=_z(3, 20, 30, dtype=torch.uint8)), ValueError),
    (dict(gains=_z(2, 2)), ValueError), (dict(gains=_z(1, 2, dtype=torch.float16)), TypeError), (dict(gains=[1.0]), TypeError),
    (dict(matrices=_z(1, 65, 2, 3), mesh=_z64(1, 65, 3, 3, 2), sources=[[0] * 65], mode="median"), ValueError),
    (dict(matrices=_z(1, 256, 2, 3), mesh=_z64(1, 256, 3, 3, 2), sources=[[0] * 256], mode="first"), ValueError),
    (dict(frames=_z(2, 3, 20, 30, dtype=torch.int16)), TypeError), (dict(layout="HWC"), ValueError),
    (dict(out_dtype=torch.float16), TypeError),
])
def test_mosaic_mesh_errors(stub, kw, exc):  # noqa: F811
    frames, matrices = kw.pop("frames", _z(2, 3, 20, 30)), kw.pop("matrices", _z(1, 2, 2, 3))
    mesh, size, sources = kw.pop("mesh", _z64(1, 2, 3, 3, 2)), kw.pop("size", (20, 30)), kw.pop("sources", [[0, 1]])
    with pytest.raises(exc):
        tensors.mosaic_mesh(frames, sources, matrices, mesh, size, **kw)
    assert stub == []


def test_mosaic_mesh_passes_a_view_of_the_tables_where_their_strides_allow(stub, monkeypatch):  # noqa: F811
    """(n_out, N, ...) goes down as (n_out * N, ...): contiguous, sliced and expanded tables without a copy; the checks pass and
    the call reaches the launch (recorded here, not made)"""
    seen = []

    def launch(dev, name, *a, workspace=None, **k):
        d = ctypes.cast(a[12], ctypes.POINTER(capi.PapofTensor)).contents
        seen.append((name, d.data, tuple(d.stride), a[13:15], workspace[:2]))
    monkeypatch.setattr(tensors, "_launch", launch)
    monkeypatch.setattr(tensors, "_device_sources", lambda src, T, n_out, dev: src)
    f, m = _z(4, 3, 20, 30), _z(2, 3, 2, 3)
    src = [[0, 1, 2], [1, 2, 3]]
    whole = _z64(2, 3, 5, 6, 2)
    wide = _z64(2, 3, 5, 9, 2)
    for mesh, strides in ((whole, (60, 12, 2, 1)), (wide[:, :, :, :6], (90, 18, 2, 1)), (whole[0, 0].expand(2, 3, 5, 6, 2), (0, 12, 2, 1))):
        got = tensors.mosaic_mesh(f, src, m, mesh, (7, 9), mode="first")
        assert tuple(got.out.shape) == (2, 3, 7, 9) and tuple(got.count.shape) == (2, 7, 9)
        name, data, st, grid, ws = seen.pop()
        assert name == "papof_mosaic_mesh_tensor" and data == mesh.data_ptr() and st == strides and grid == (4, 5)
        assert ws == ("papof_mosaic_mesh_workspace", (2, 3))
    # a slice of the slot axis that cannot be one axis: a copy
    tall = _z64(2, 5, 5, 6, 2)
    tensors.mosaic_mesh(f, src, m, tall[:, :3], (7, 9), mode="first")
    name, data, st, grid, ws = seen.pop()
    assert data != tall.data_ptr() and st == (60, 12, 2, 1)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(mesh_motion=_z64(4, 3, 3)), ValueError), (dict(mesh_motion=_z64(0, 3, 3, 2)), ValueError),
    (dict(mesh_motion=_z64(4, 3, 3, 3)), ValueError), (dict(mesh_motion=_z64(4, 1, 3, 2)), ValueError),
    (dict(mesh_motion=[1]), TypeError), (dict(radius=-2), ValueError), (dict(radius=1.5), ValueError),
    (dict(radius=True), ValueError), (dict(fill_radius=-1), ValueError), (dict(fill_radius=128), ValueError),
    (dict(fill_radius=2.0), ValueError), (dict(fill_radius=True), ValueError),
])
def test_neighbour_mesh_errors(kw, exc):
    mm = kw.pop("mesh_motion", _z64(4, 3, 3, 2))
    kw.setdefault("radius", 3)
    kw.setdefault("fill_radius", 2)
    with pytest.raises(exc):
        tensors.neighbour_mesh(mm, **kw)


@pytest.mark.parametrize("kw,exc", [
    (dict(fill_radius=-1), ValueError), (dict(fill_radius=128), ValueError), (dict(fill_radius=1.0), ValueError),
    (dict(fill_radius=False), ValueError),
    (dict(grid=(0, 2)), ValueError), (dict(grid=(2, 30)), ValueError), (dict(grid=(20, 2)), ValueError), (dict(grid=3), TypeError),
    (dict(min_support=0), ValueError), (dict(spatial="yes"), TypeError),
    (dict(model="projective"), ValueError), (dict(radius=-1), ValueError), (dict(radius=1.5), ValueError),
    (dict(crop=0.0), ValueError), (dict(crop="all"), TypeError), (dict(iters=0), ValueError), (dict(scale=-2.0), ValueError),
    (dict(consistency=(1.0,)), TypeError), (dict(consistency=(-1.0, 0.5)), ValueError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError), (dict(bogus=1), TypeError),
])
def test_stabilize_video_mesh_full_errors(stub, kw, exc):  # noqa: F811
    kw.setdefault("grid", (4, 4))
    with pytest.raises(exc):
        tensors.stabilize_video_mesh_full(_z(3, 3, 20, 30), 2, **kw)
    assert stub == []


def test_stabilize_video_mesh_full_needs_two_frames_levels_and_a_grid_that_fits(stub):  # noqa: F811
    with pytest.raises(ValueError):
        tensors.stabilize_video_mesh_full(_z(1, 3, 20, 30), 2, grid=(4, 4))
    with pytest.raises(ValueError):
        tensors.stabilize_video_mesh_full(_z(3, 3, 20, 30), 0, grid=(4, 4))
    with pytest.raises(ValueError):
        tensors.stabilize_video_mesh_full(_z(3, 3, 8, 8), 2)  # the default 16 x 16 grid does not fit 8 x 8 frames
    assert stub == []


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
_OK = "ok"


def _mesh(lib, h, n_frames=3, size=(20, 30, 3), fr=_OK, masks=None, n_out=2, n_src=3, canvas=(25, 35), sources=0x4000, mat=_OK,
          mesh=_OK, grid=(4, 5), gains=None, mode=capi.MOSAIC_FIRST, out=_OK, count=None, ws=0x2000, ws_bytes=None):
    make = {"fr": lambda: _t(capi.DTYPE_U8, (1800, 90, 3, 1)), "mat": lambda: _t(capi.DTYPE_F32, (18, 6, 3, 1)),
            "mesh": lambda: _t(strides=(60, 12, 2, 1)), "out": lambda: _t(capi.DTYPE_F64, (2625, 105, 3, 1))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mat=mat, mesh=mesh, out=out).items()}
    if ws_bytes is None:
        ws_bytes = max(0, lib.papof_mosaic_mesh_workspace(n_out, n_src))
    return lib.papof_mosaic_mesh_tensor(h, n_frames, size[0], size[1], size[2], _ref(d["fr"]), _ref(masks), n_out, n_src,
                                        canvas[0], canvas[1], sources, _ref(d["mat"]), _ref(d["mesh"]), grid[0], grid[1],
                                        _ref(gains), mode, _ref(d["out"]), _ref(count), ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(mesh=None), dict(out=None), dict(sources=None),                      # NULL
    dict(fr=_t(data=0)), dict(mat=_t(data=0)), dict(mesh=_t(data=0)), dict(out=_t(data=0)),
    dict(masks=_t(capi.DTYPE_U8, data=0)), dict(count=_t(capi.DTYPE_U8, data=0)), dict(gains=_t(data=0)),
    dict(fr=_t(dtype=3)), dict(mat=_t(capi.DTYPE_U8, (18, 6, 3, 1))), dict(mesh=_t(capi.DTYPE_F32, (60, 12, 2, 1))),   # dtypes
    dict(mesh=_t(capi.DTYPE_U8, (60, 12, 2, 1))), dict(out=_t(dtype=-1)), dict(masks=_t(capi.DTYPE_F32, (600, 30, 1, 0))),
    dict(count=_t(capi.DTYPE_F64, (875, 35, 1, 0))), dict(gains=_t(capi.DTYPE_U8, (3, 1, 0, 0))),
    dict(fr=_t(strides=(1800, 90, 3, -1))), dict(mat=_t(strides=(18, -6, 3, 1))), dict(mesh=_t(strides=(60, 12, 2, -1))),  # strides
    dict(mesh=_t(strides=(-60, 12, 2, 1))), dict(mesh=_t(strides=(60, -12, 2, 1))), dict(out=_t(strides=(2625, 105, 3, 0))),
    dict(out=_t(strides=(0, 105, 3, 1))), dict(count=_t(capi.DTYPE_U8, (875, 35, 0, 0))), dict(masks=_t(capi.DTYPE_U8, (600, -30, 1, 0))),
    dict(gains=_t(strides=(3, -1, 0, 0))),
    dict(grid=(0, 5)), dict(grid=(4, 0)), dict(grid=(20, 5)), dict(grid=(4, 30)), dict(grid=(-1, 5)),         # the grid, on the FRAMES
    dict(size=(100, 100, 3), grid=(65, 5)), dict(size=(100, 100, 3), grid=(4, 65)), dict(size=(20, 1, 3), grid=(4, 1)),
    dict(n_frames=0), dict(size=(0, 30, 3)), dict(size=(20, 0, 3)), dict(size=(20, 30, 0)), dict(n_out=0),     # sizes
    dict(canvas=(0, 35)), dict(canvas=(25, 0)), dict(n_src=0), dict(n_src=256),
    dict(mode=-1), dict(mode=4), dict(n_src=65, mode=capi.MOSAIC_MEDIAN),
    dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=-1),                                                       # workspace
])
def test_c_abi_mosaic_mesh_refuses(kw):
    assert _mesh(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_mosaic_mesh_workspace():
    lib = _lib()
    ws = lib.papof_mosaic_mesh_workspace
    assert ws(1, 1) == 32 and ws(8, 31) == 32 * 8 * 31 and ws(3, 255) == 32 * 3 * 255
    assert ws(100000000, 255) == 32 * 100000000 * 255  # 64-bit sizes
    assert ws(0, 3) == -1 and ws(-1, 3) == -1 and ws(2, 0) == -1 and ws(2, 256) == -1
    assert _mesh(lib, ctypes.cast(_FAKE, ctypes.c_void_p), ws_bytes=ws(2, 3) - 1) == -1
    assert _mesh(lib, None) == -1
