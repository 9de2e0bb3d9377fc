"""CPU-side checks of point tracking (papteam_opticalflow_amd/tensors.py: track_points, track_video; include/papof.h:
papof_track_tensor): the numpy fp64 restatement of the tracker that tests/test_gpu_track.py compares the device's tracks
with, its known answers, every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each
refusal of the C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from test_fb_cpu import fb_reference  # noqa: E402

QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]  # a lost point's coordinates, bit for bit


def _bilinear(fl, X, Y):
    """(u, v) of one flow (2, H, W) sampled at the points (X, Y), all inside the image, by the reference's rule -- the
    sampling of fb_reference: truncation toward zero, fraction clamped to [0, 1], neighbours clamped into the image, taps
    accumulated from 0 in (m, n) order"""
    H, W = fl.shape[1:]
    xx, yy = X.astype(np.int64), Y.astype(np.int64)
    dx, dy = X - xx, Y - yy
    dx = np.where(dx > 1, 1.0, dx)
    dx = np.where(dx < 0, 0.0, dx)
    dy = np.where(dy > 1, 1.0, dy)
    dy = np.where(dy < 0, 0.0, dy)
    u, v = np.zeros_like(X), np.zeros_like(X)
    for m in (0, 1):
        for n in (0, 1):
            cu, cv = np.clip(xx + m, 0, W - 1), np.clip(yy + n, 0, H - 1)
            s = np.abs(float(1 - m) - dx) * np.abs(float(1 - n) - dy)
            with np.errstate(invalid="ignore"):  # (an infinite tap of weight 0: NaN, as on the device)
                u = u + fl[0, cv, cu] * s
                v = v + fl[1, cv, cu] * s
    return u, v


def _step(f, b, x, y, alive, check, alpha1, alpha2):
    """one step of the points (x, y) that are `alive` through the flow f, checked against b: (X, Y, still visible)"""
    H, W = f.shape[1:]
    xs, ys = np.where(alive, x, 0.0), np.where(alive, y, 0.0)
    u, v = _bilinear(f, xs, ys)
    X, Y = xs + u, ys + v
    with np.errstate(invalid="ignore"):
        ok = alive & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        if check:
            bu, bv = _bilinear(b, np.where(ok, X, 0.0), np.where(ok, Y, 0.0))
            du, dv = u + bu, v + bv
            e = du * du + dv * dv
            mag = (u * u + v * v) + (bu * bu + bv * bv)
            ok = ok & (e <= alpha1 * mag + alpha2)
    return np.where(ok, X, QNAN), np.where(ok, Y, QNAN), ok


def track_reference(fw, bw, queries=None, alpha1=0.01, alpha2=0.5, check=True):
    """The tracker of include/papof.h (papof_track_tensor) restated in numpy fp64, vectorised over the points: fw, bw
    (T - 1, 2, H, W) flows, queries (N, 3) rows (t0, x, y) or None (every pixel of frame 0, row-major) -> tracks (T, N, 2)
    float64, visible (T, N) bool.  numpy does not contract a * b + c: the bits are the kernel's."""
    fw, bw = np.asarray(fw, dtype=np.float64), np.asarray(bw, dtype=np.float64)
    T, (H, W) = fw.shape[0] + 1, fw.shape[2:]
    if queries is None:
        n = np.arange(H * W)
        t0, x, y = np.zeros(H * W), (n % W).astype(np.float64), (n // W).astype(np.float64)
    else:
        q = np.asarray(queries, dtype=np.float64)
        t0, x, y = q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()
    N = len(t0)
    with np.errstate(invalid="ignore"):
        valid = ((t0 >= 0) & (t0 <= T - 1) & (t0 == np.trunc(t0)) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1))
    s = np.where(valid, t0, 0).astype(np.int64)
    tracks = np.full((T, N, 2), QNAN)
    vis = np.zeros((T, N), bool)
    tracks[s[valid], valid.nonzero()[0]] = np.stack([x[valid], y[valid]], 1)
    vis[s[valid], valid.nonzero()[0]] = True
    for direction in (1, -1):
        px, py, alive = x.copy(), y.copy(), valid.copy()
        for t in (range(T - 1) if direction == 1 else range(T - 1, 0, -1)):
            if direction == 1:  # t -> t + 1 for the points with t0 <= t (an invalid query: every frame)
                f, b, mine = fw[t], bw[t], s <= t
            else:               # t -> t - 1 for the points with t0 >= t
                f, b, mine = bw[t - 1], fw[t - 1], valid & (s >= t)
            nx, ny, ok = _step(f, b, px, py, alive & mine, check, alpha1, alpha2)
            px, py, alive = np.where(mine, nx, px), np.where(mine, ny, py), np.where(mine, ok, alive)
            tracks[t + direction, mine, 0] = nx[mine]
            tracks[t + direction, mine, 1] = ny[mine]
            vis[t + direction, mine] = ok[mine]
    return tracks, vis


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _const(T, H, W, u, v):
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0], fw[:, 1] = u, v
    return fw, -fw


# ---- known answers of the restatement
@pytest.mark.parametrize("u,v", [(1.0, 2.0), (0.25, -0.5), (-0.75, 0.125)])
def test_constant_translation_sums_exactly_until_the_point_leaves(u, v):
    T, H, W = 12, 9, 11
    fw, bw = _const(T, H, W, u, v)
    q = [[0, 2.0, 4.0], [5, 6.5, 3.25], [T - 1, 5.0, 4.0]]
    tr, vis = track_reference(fw, bw, q)
    for i, (t0, x, y) in enumerate(q):
        at = lambda k: (x + (k - t0) * u, y + (k - t0) * v)  # noqa: E731  (dyadic: exact)
        for t in range(T):
            # visible while every position from frame t0 to frame t (either way) lies in the image
            inside = all(0 <= at(k)[0] <= W - 1 and 0 <= at(k)[1] <= H - 1 for k in range(min(t, t0), max(t, t0) + 1))
            assert vis[t, i] == inside, (i, t)
            want = at(t) if inside else (QNAN, QNAN)
            assert (_bits(tr[t, i]) == _bits(want)).all(), (i, t, tr[t, i], want)
    assert vis.sum(0).min() >= 2  # every query moves at least once


def test_inconsistent_backward_flow_loses_the_point_at_t0_plus_and_minus_one():
    T, H, W = 6, 8, 8
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0] = 1.0
    bw = np.zeros_like(fw)  # 1 + 0 against 0.01 * 1 + 0.5: inconsistent both ways
    tr, vis = track_reference(fw, bw, [[2, 3.0, 3.0]])
    assert vis[:, 0].tolist() == [False, False, True, False, False, False]
    assert (_bits(tr[2, 0]) == _bits([3.0, 3.0])).all()
    assert (_bits(np.delete(tr[:, 0], 2, 0)) == _bits(QNAN)).all()


def test_consistency_at_the_bound_is_not_lost():
    T, H, W = 3, 4, 6
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0] = 0.5
    bw = np.zeros_like(fw)
    # e = 0.25, m = 0.25: e == 0.5 * m + 0.125 exactly
    tr, vis = track_reference(fw, bw, [[0, 1.0, 1.0]], 0.5, 0.125)
    assert vis[:, 0].all() and tr[2, 0].tolist() == [2.0, 1.0]
    _, vis = track_reference(fw, bw, [[0, 1.0, 1.0]], 0.5, 0.124)
    assert vis[:, 0].tolist() == [True, False, False]


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("where", ["tap", "neighbour", "backward"])
def test_a_non_finite_flow_loses_the_point(bad, where):
    T, H, W = 4, 6, 7
    fw, bw = _const(T, H, W, 1.0, 0.0)
    if where == "tap":
        fw[1, 0, 2, 3] = bad  # the point is at (3, 2) in frame 1
    elif where == "neighbour":
        fw[1, 1, 2, 4] = bad  # a tap of weight 0: bad * 0 is NaN
    else:
        bw[1, 0, 2, 4] = bad  # where it lands
    tr, vis = track_reference(fw, bw, [[0, 2.0, 2.0]])
    if where == "backward" and math.isinf(bad):  # an infinite bu: e = m = inf, and inf <= alpha1 * inf + alpha2 holds
        assert vis[:, 0].all()
        return
    assert vis[:, 0].tolist() == [True, True, False, False]
    assert (_bits(tr[2:, 0]) == _bits(QNAN)).all()
    # without the check, only the forward flow matters
    _, vis = track_reference(fw, bw, [[0, 2.0, 2.0]], check=False)
    assert vis[:, 0].tolist() == ([True, True, True, True] if where == "backward" else [True, True, False, False])


def test_invalid_queries_are_lost_at_every_frame():
    T, H, W = 4, 5, 6
    fw, bw = _const(T, H, W, 0.0, 0.0)
    bad = [[-1, 1, 1], [T, 1, 1], [1.5, 1, 1], [math.nan, 1, 1], [math.inf, 1, 1], [-0.5, 1, 1],
           [0, math.nan, 1], [0, 1, math.inf], [0, -math.inf, 1],
           [0, -0.5, 1], [0, W - 1 + 1e-9, 1], [0, 1, -1e-300], [0, 1, H - 0.5]]
    good = [[T - 1, W - 1, H - 1], [0, 0, 0], [2.0, 0.0, 3.5]]  # the edges are inside
    tr, vis = track_reference(fw, bw, bad + good)
    nb = len(bad)
    assert not vis[:, :nb].any() and (_bits(tr[:, :nb]) == _bits(QNAN)).all()
    assert vis[:, nb:].all()
    assert (_bits(tr[:, nb:]) == _bits(np.broadcast_to(np.array(good)[:, 1:], (T, 3, 2)))).all()  # zero flow: they stay
    tr, vis = track_reference(fw, bw, [[1, -0.0, 2.0]])  # -0 is inside; frame t0 keeps it, a step adds +0
    assert vis[:, 0].all() and _bits(tr[1, 0, 0]) == _bits(-0.0) and (_bits(tr[[0, 2, 3], 0, 0]) == _bits(0.0)).all()


def test_without_the_check_inconsistent_flows_keep_the_point():
    T, H, W = 5, 6, 6
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 1] = 1.0
    bw = np.full_like(fw, math.nan)  # never read forward without the check
    tr, vis = track_reference(fw, bw, [[0, 2.0, 1.0]], check=False)
    assert vis[:, 0].all() and tr[:, 0, 1].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    _, vis = track_reference(fw, bw, [[0, 2.0, 1.0]])
    assert vis[:, 0].tolist() == [True, False, False, False, False]


def test_dense_first_step_is_the_forward_occlusion_mask():
    rng = np.random.default_rng(3)
    T, H, W = 3, 13, 17
    fw = rng.normal(0, 2, (T - 1, 2, H, W))
    bw = -fw + rng.normal(0, 0.4, (T - 1, 2, H, W))
    tr, vis = track_reference(fw, bw)
    occ = fb_reference(fw, bw)[0, 0].astype(bool)
    assert 0 < occ.sum() < occ.size
    assert (vis[1] == ~occ.reshape(-1)).all()
    n = np.arange(H * W)
    assert (_bits(tr[0]) == _bits(np.stack([n % W, n // W], 1).astype(np.float64))).all() and vis[0].all()


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8)), ValueError),                     # CPU flows
    (lambda: tensors.track_points(_z(2, 2, 8, 8), None), TypeError),                                 # not a tensor
    (lambda: tensors.track_points([0], _z(2, 2, 8, 8)), TypeError),
    (lambda: tensors.track_points(_z(2, 3, 8, 8), _z(2, 3, 8, 8)), ValueError),                     # not (T - 1, 2, H, W)
    (lambda: tensors.track_points(_z(2, 8, 8), _z(2, 8, 8)), ValueError),
    (lambda: tensors.track_points(_z(0, 2, 8, 8), _z(0, 2, 8, 8)), ValueError),
    (lambda: tensors.track_points(_z(2, 2, 0, 8), _z(2, 2, 0, 8)), ValueError),
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(3, 2, 8, 8)), ValueError),                     # mismatched shapes
    (lambda: tensors.track_points(_z(2, 2, 8, 8, dtype=torch.uint8), _z(2, 2, 8, 8)), TypeError),   # dtypes
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8, dtype=torch.float16)), TypeError),
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8, device="meta")), ValueError),      # mixed devices
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8), consistency=(0.01,)), TypeError),  # consistency
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8), consistency=0.5), TypeError),
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8), consistency=(-1, 0.5)), ValueError),
    (lambda: tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8), consistency=(0.01, math.nan)), ValueError),
    (lambda: tensors.track_video(_z(3, 3, 8, 8), 2), ValueError),                                   # CPU frames
    (lambda: tensors.track_video(None, 2), TypeError),
    (lambda: tensors.track_video(_z(1, 3, 8, 8), 2), ValueError),                                   # fewer than 2 frames
    (lambda: tensors.track_video(_z(3, 3, 8, 8), 0), ValueError),                                   # pyramid levels
    (lambda: tensors.track_video(_z(3, 3, 8, 8), 2, layout="CHWN"), ValueError),                    # layout
    (lambda: tensors.track_video(_z(3, 3, 8, 8, dtype=torch.int32), 2), TypeError),                 # frame dtype
    (lambda: tensors.track_video(_z(3, 3, 8, 8), 2, consistency=(0.01, -0.5)), ValueError),
    (lambda: tensors.track_video(_z(3, 3, 8, 8), 2, consistency="yes"), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


@pytest.mark.parametrize("queries,exc", [
    ([[0, 1, 1]], TypeError),                                            # not a tensor
    (_z(4, 2), ValueError), (_z(4, 3, 1), ValueError), (_z(3), ValueError), (_z(0, 3), ValueError),  # not (N, 3), N >= 1
    (_z(4, 3, dtype=torch.int64), TypeError), (_z(4, 3, dtype=torch.float16), TypeError),           # dtypes
    (_z(4, 3, device="meta"), ValueError),                               # not on the flows' device
])
def test_query_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, queries, exc):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: True)  # the CPU tensors pass for device ones up to the handle
    with pytest.raises(exc):
        tensors.track_points(_z(2, 2, 8, 8), _z(2, 2, 8, 8), queries)
    with pytest.raises(exc):
        tensors.track_video(_z(3, 3, 8, 8), 2, queries)
    assert stub == []


def test_track_video_solver_errors_before_any_launch(stub, monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: True)
    with pytest.raises(TypeError):
        tensors.track_video(_z(3, 3, 8, 8), 2, bogus=1)
    with pytest.raises(TypeError):
        tensors.track_video(_z(3, 3, 8, 8), 2, None, "NHWC")  # layout and consistency are keywords
    assert stub == []


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


def _call(lib, h, T=3, hw=(8, 8), fw=_OK, bw=_OK, n=4, q=_OK, check=1, alphas=(0.01, 0.5), tr=_OK, vis=_OK):
    make = {"fw": lambda: _t(capi.DTYPE_F32), "bw": lambda: _t(), "q": lambda: _t(strides=(3, 0, 0, 1)),
            "tr": lambda: _t(strides=(8, 2, 0, 1)), "vis": lambda: _t(capi.DTYPE_U8, (4, 1, 0, 0))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fw=fw, bw=bw, q=q, tr=tr, vis=vis).items()}
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return lib.papof_track_tensor(h, T, hw[0], hw[1], ref(d["fw"]), ref(d["bw"]), n, ref(d["q"]), check, alphas[0],
                                  alphas[1], ref(d["tr"]), ref(d["vis"]), None)


@pytest.mark.parametrize("kw", [
    dict(fw=None), dict(bw=None), dict(tr=None), dict(vis=None),                                      # NULL descriptors
    dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(q=_t(strides=(3, 0, 0, 1), data=0)),              # NULL data
    dict(tr=_t(strides=(8, 2, 0, 1), data=0)), dict(vis=_t(capi.DTYPE_U8, (4, 1, 0, 0), data=0)),
    dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=3)), dict(fw=_t(dtype=-1)),                          # flow dtypes
    dict(q=_t(capi.DTYPE_U8, (3, 0, 0, 1))), dict(q=_t(dtype=7, strides=(3, 0, 0, 1))),              # query dtypes
    dict(tr=_t(capi.DTYPE_F32, (8, 2, 0, 1))), dict(tr=_t(capi.DTYPE_U8, (8, 2, 0, 1))),             # tracks: F64 only
    dict(vis=_t(capi.DTYPE_F64, (4, 1, 0, 0))), dict(vis=_t(capi.DTYPE_F32, (4, 1, 0, 0))),          # visible: U8 only
    dict(fw=_t(strides=(-128, 8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))),                     # negative strides
    dict(q=_t(strides=(-3, 0, 0, 1))), dict(q=_t(strides=(3, 0, 0, -1))),
    dict(tr=_t(strides=(8, -2, 0, 1))), dict(vis=_t(capi.DTYPE_U8, (-4, 1, 0, 0))),
    dict(tr=_t(strides=(0, 2, 0, 1))), dict(tr=_t(strides=(8, 0, 0, 1))), dict(tr=_t(strides=(8, 2, 0, 0))),  # zero out
    dict(vis=_t(capi.DTYPE_U8, (0, 1, 0, 0))), dict(vis=_t(capi.DTYPE_U8, (4, 0, 0, 0))),
    dict(T=1), dict(T=0), dict(T=-3), dict(hw=(0, 8)), dict(hw=(8, 0)), dict(hw=(-1, 8)),              # sizes
    dict(n=0), dict(n=-1),                                                                              # queries given
    dict(alphas=(-0.01, 0.5)), dict(alphas=(0.01, -1e-300)), dict(alphas=(math.nan, 0.5)),              # alphas
    dict(alphas=(0.01, math.inf)), dict(alphas=(-math.inf, 0.5)), dict(check=0, alphas=(0.01, math.nan)),
    dict(q=None, fw=_t(capi.DTYPE_U8)), dict(q=None, tr=_t(strides=(8, 2, 0, 0))), dict(q=None, T=1),  # dense
])
def test_c_abi_track_refuses(kw):
    assert _call(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_track_without_a_handle():
    lib = _lib()
    assert _call(lib, None) == -1
    assert _call(lib, None, q=None) == -1
