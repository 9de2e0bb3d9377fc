"""The mesh rules of include/papof.h (papof_mesh_motion_tensor, papof_warp_mesh_tensor) restated in numpy fp64 from the
header's text -- what tests/test_mesh_cpu.py checks with known answers and tests/test_gpu_mesh.py compares the device's
results with, byte for byte.  numpy does not contract a * b + c: the bits are the kernels'.  The sampler is
tests/_interp_ref.py's."""
import numpy as np

from _interp_ref import _sample, _taps, as_f64, convert

MAX_SAMPLES = 1024


def vertex_positions(H, W, GH, GW):
    """(px (GW + 1,), py (GH + 1,)): the product of two exact integers, then one division"""
    px = (np.arange(GW + 1, dtype=np.float64) * float(W - 1)) / float(GW)
    py = (np.arange(GH + 1, dtype=np.float64) * float(H - 1)) / float(GH)
    return px, py


def lattice_step(H, W, GH, GW):
    Lx, Ly = (2 * (W - 1)) // GW, (2 * (H - 1)) // GH
    s = 1
    while (Lx // s + 1) * (Ly // s + 1) > MAX_SAMPLES:
        s += 1
    return s


def _axis(v, G, N, step):
    """the lattice coordinates of the window of vertex index v along an axis of N pixels and G cells"""
    lo = max(0, -((-(v - 1) * (N - 1)) // G))   # ceil((v - 1) (N - 1) / G)
    hi = min(N - 1, ((v + 1) * (N - 1)) // G)
    first = -((-lo) // step) * step
    return np.arange(first, hi + 1, step)


def _keys(v):
    """float64 values as signed integers that order numerically, -0 before +0"""
    b = np.ascontiguousarray(v, np.float64).view(np.int64)
    return b ^ ((b >> 63) & np.int64(0x7fffffffffffffff))


def lower_median(v):
    """the element of rank (n - 1) // 2 of the 1-D float64 array v (n >= 1) in the order of _keys: its bits"""
    k = np.sort(_keys(v), kind="stable")[(len(v) - 1) // 2]
    return (k ^ ((k >> 63) & np.int64(0x7fffffffffffffff))).view(np.float64)


def _global(m, x, y):
    """(A q - q) at points, grouped as the header writes it"""
    return ((m[0, 0] * x + m[0, 1] * y) + m[0, 2]) - x, ((m[1, 0] * x + m[1, 1] * y) + m[1, 2]) - y


def mesh_motion_reference(flow, motion=None, occlusion=None, grid=(16, 16), min_support=16, spatial=True):
    """flow (B, 2, H, W) float32 / float64; motion None or (B, 2, 3); occlusion None or (B, H, W) (nonzero: left out) ->
    (vertices (B, GH + 1, GW + 1, 2), support (B, GH + 1, GW + 1) int32, residuals as vertices)"""
    flow = np.asarray(flow)
    B, _, H, W = flow.shape
    GH, GW = grid
    step = lattice_step(H, W, GH, GW)
    px, py = vertex_positions(H, W, GH, GW)
    raw = np.zeros((B, GH + 1, GW + 1, 2))
    support = np.zeros((B, GH + 1, GW + 1), np.int32)
    for b in range(B):
        m = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) if motion is None else np.asarray(motion, np.float64)[b]
        u_all, v_all = flow[b, 0].astype(np.float64), flow[b, 1].astype(np.float64)
        for i in range(GH + 1):
            ys = _axis(i, GH, H, step)
            for j in range(GW + 1):
                xs = _axis(j, GW, W, step)
                assert len(xs) * len(ys) <= MAX_SAMPLES
                if len(xs) == 0 or len(ys) == 0:
                    continue
                yy, xx = np.meshgrid(ys, xs, indexing="ij")  # row-major: r outer, x inner
                yy, xx = yy.ravel(), xx.ravel()
                u, v = u_all[yy, xx], v_all[yy, xx]
                x, r = xx.astype(np.float64), yy.astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    X, Y = x + u, r + v
                    valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
                    if occlusion is not None:
                        valid &= np.asarray(occlusion)[b][yy, xx] == 0
                    gx, gy = _global(m, x, r)
                    rx, ry = u - gx, v - gy
                    valid &= ~np.isnan(rx) & ~np.isnan(ry)
                n = int(valid.sum())
                support[b, i, j] = n
                if n:
                    raw[b, i, j] = lower_median(rx[valid]), lower_median(ry[valid])
    ok = support >= min_support
    res = np.zeros_like(raw)
    for b in range(B):
        for i in range(GH + 1):
            for j in range(GW + 1):
                if spatial:
                    xs, ys = [], []
                    for di in (-1, 0, 1):
                        for dj in (-1, 0, 1):
                            a, c = i + di, j + dj
                            if 0 <= a <= GH and 0 <= c <= GW and ok[b, a, c]:
                                xs.append(raw[b, a, c, 0])
                                ys.append(raw[b, a, c, 1])
                    if xs:
                        res[b, i, j] = lower_median(np.array(xs)), lower_median(np.array(ys))
                elif ok[b, i, j]:
                    res[b, i, j] = raw[b, i, j]
    vert = np.empty_like(res)
    PX, PY = np.meshgrid(px, py)
    for b in range(B):
        m = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) if motion is None else np.asarray(motion, np.float64)[b]
        with np.errstate(invalid="ignore", over="ignore"):
            gx, gy = _global(m, PX, PY)
            vert[b, ..., 0] = res[b, ..., 0] + gx
            vert[b, ..., 1] = res[b, ..., 1] + gy
    return vert, support, res


def mesh_displacement(X0, Y0, D, H, W):
    """(dx, dy) of the table D (GH + 1, GW + 1, 2) at the points (X0, Y0)"""
    GH, GW = D.shape[0] - 1, D.shape[1] - 1
    with np.errstate(invalid="ignore", over="ignore"):
        gx, gy = (X0 * float(GW)) / float(W - 1), (Y0 * float(GH)) / float(H - 1)
        gx = np.where(gx < 0, 0.0, np.where(gx > GW, float(GW), gx))
        gy = np.where(gy < 0, 0.0, np.where(gy > GH, float(GH), gy))
        j = np.where(gx >= 0, np.minimum(np.where(gx >= 0, gx, 0.0).astype(np.int64), GW - 1), 0)
        i = np.where(gy >= 0, np.minimum(np.where(gy >= 0, gy, 0.0).astype(np.int64), GH - 1), 0)
        fx, fy = gx - j, gy - i
        dx, dy = np.zeros(X0.shape), np.zeros(X0.shape)
        for m in (0, 1):
            for n in (0, 1):
                w = np.abs(float(1 - m) - fx) * np.abs(float(1 - n) - fy)
                dx = dx + D[i + n, j + m, 0] * w
                dy = dy + D[i + n, j + m, 1] * w
    return dx, dy


def warp_mesh_reference(frames, matrices, mesh, out_dtype=np.float64):
    """frames (B, H, W, C) uint8 / float32 / float64, matrices (B, 2, 3), mesh (B, GH + 1, GW + 1, 2) ->
    (out (B, H, W, C) of out_dtype, valid (B, H, W))"""
    I = as_f64(frames)
    M = np.asarray(matrices, np.float64)
    D = np.asarray(mesh, np.float64)
    B, H, W, C = I.shape
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, H, W, C))
    valid = np.zeros((B, H, W), bool)
    for i in range(B):
        m = M[i]
        with np.errstate(invalid="ignore", over="ignore"):
            X0 = (m[0, 0] * x + m[0, 1] * r) + m[0, 2]
            Y0 = (m[1, 0] * x + m[1, 1] * r) + m[1, 2]
            dx, dy = mesh_displacement(X0, Y0, D[i], H, W)
            X, Y = X0 + dx, Y0 + dy
            inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        k = _taps(np.where(inside, X, 0.0)[None], np.where(inside, Y, 0.0)[None], H, W)
        for ch in range(C):
            out[i, :, :, ch] = np.where(inside, _sample(I[i:i + 1, :, :, ch], np.zeros((1, 1, 1), np.int64), k)[0], 0.0)
        valid[i] = inside
    return convert(out, out_dtype), valid
