"""Video stabilization of include/papof.h (papof_motion_fit_tensor, papof_warp_affine_tensor) and of
papteam_opticalflow_amd/tensors.py (stabilizing_transforms) restated in numpy fp64 -- the rules that tests/test_stab_cpu.py
checks with known answers and tests/test_gpu_stab.py compares the device's results with.  The fit's sums are added in numpy's
order, not the kernel's, so fitted matrices agree to rounding, not bit for bit; the warp is the bits of the kernel (the
sampler is tests/_interp_ref.py's)."""
import math

import numpy as np

from _interp_ref import _sample, _taps, as_f64, convert

SIMILARITY, AFFINE = 0, 1


def _eliminate(g, n, tol):
    """Gaussian elimination in natural order without row exchanges on the n x n part of the rows of g (lists, right-hand
    sides after column n): the solutions, one list per right-hand side, or None where a pivot is not > tol"""
    g = [list(row) for row in g]
    R = len(g[0]) - n
    for k in range(n):
        piv = g[k][k]
        if not piv > tol:
            return None
        for i in range(k + 1, n):
            f = g[i][k] / piv
            for j in range(k, n + R):
                g[i][j] = g[i][j] - f * g[k][j]
    xs = []
    for r in range(R):
        x = [0.0] * n
        for i in range(n - 1, -1, -1):
            v = g[i][n + r]
            for j in range(i + 1, n):
                v = v - g[i][j] * x[j]
            x[i] = v / g[i][i]
        xs.append(x)
    return xs


def solve(S, model, H, W):
    """the pixel-coordinate matrix (2, 3) of the fourteen sums S, or None where the iteration fails"""
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(W, H) / 2.0
    sw = S[5]
    if not sw > 0:
        return None
    tol = 1e-12 * sw
    if model == AFFINE:
        p = _eliminate([[S[0], S[1], S[3], S[6], S[9]], [S[1], S[2], S[4], S[7], S[10]], [S[3], S[4], S[5], S[8], S[11]]],
                       3, tol)
        if p is None:
            return None
        L0, L1, tx, L2, L3, ty = p[0][0], p[0][1], p[0][2], p[1][0], p[1][1], p[1][2]
    else:
        q = S[0] + S[2]
        p = _eliminate([[q, 0.0, S[3], S[4], S[6] + S[10]], [0.0, q, -S[4], S[3], S[9] - S[7]], [S[3], -S[4], sw, 0.0, S[8]],
                        [S[4], S[3], 0.0, sw, S[11]]], 4, tol)
        if p is None:
            return None
        a, b, tx, ty = p[0]
        L0, L1, L2, L3 = a, -b, b, a
    m = np.array([[L0, L1, (cx + s * tx) - (L0 * cx + L1 * cy)], [L2, L3, (cy + s * ty) - (L2 * cx + L3 * cy)]])
    return m if np.isfinite(m).all() else None


def sums(flow, mask, m, scale):
    """the fourteen sums of one pair: flow (2, H, W), mask None or (H, W) (nonzero: left out), m the previous iteration's
    matrix or None (iteration 0)"""
    _, H, W = flow.shape
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(W, H) / 2.0
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = flow[0].astype(np.float64), flow[1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y = x + u, r + v
        valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    if mask is not None:
        valid &= np.asarray(mask) == 0
    x, r, X, Y = x[valid], r[valid], X[valid], Y[valid]
    if m is None:
        w, e2 = np.ones(x.shape), np.zeros(x.shape)
    else:
        ex = X - ((m[0, 0] * x + m[0, 1] * r) + m[0, 2])
        ey = Y - ((m[1, 0] * x + m[1, 1] * r) + m[1, 2])
        e2 = ex * ex + ey * ey
        w = 1.0 / (1.0 + e2 / (scale * scale))
    xh, yh, Xh, Yh = (x - cx) / s, (r - cy) / s, (X - cx) / s, (Y - cy) / s
    terms = [xh * xh, xh * yh, yh * yh, xh, yh, np.ones(x.shape), xh * Xh, yh * Xh, Xh, xh * Yh, yh * Yh, Yh]
    return [float(np.sum(w * t)) for t in terms] + [float(valid.sum()), float(np.sum(w * e2))]


def fit_reference(flow, occlusion=None, model=AFFINE, iters=5, scale=1.0):
    """flow (B, 2, H, W); occlusion None or (B, 2, H, W) (channel 0 read) -> (motion (B, 2, 3), ok (B,) bool, support (B,))"""
    flow = np.asarray(flow)
    B, _, H, W = flow.shape
    motion, ok, support = np.empty((B, 2, 3)), np.zeros(B, bool), np.empty(B)
    for i in range(B):
        mask = None if occlusion is None else np.asarray(occlusion)[i, 0]
        m = None
        for it in range(iters):
            S = sums(flow[i], mask, m, scale)
            support[i] = S[5] / (H * W)
            got = solve(S, model, H, W)
            if got is not None:
                m = got
            elif it == 0:
                break
        ok[i] = m is not None
        motion[i] = m if m is not None else np.eye(2, 3)
    return motion, ok, support


def warp_reference(frames, matrices, out_dtype=np.float64):
    """frames (B, H, W, C) uint8 / float32 / float64, matrices (B, 2, 3) -> (out (B, H, W, C) of out_dtype, valid (B, H, W))"""
    I = as_f64(frames)
    M = np.asarray(matrices, np.float64)
    B, H, W, C = I.shape
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, H, W, C))
    valid = np.zeros((B, H, W), bool)
    for i in range(B):
        m = M[i]
        with np.errstate(invalid="ignore", over="ignore"):
            X = (m[0, 0] * x + m[0, 1] * r) + m[0, 2]
            Y = (m[1, 0] * x + m[1, 1] * r) + m[1, 2]
            inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        k = _taps(np.where(inside, X, 0.0)[None], np.where(inside, Y, 0.0)[None], H, W)
        for ch in range(C):
            out[i, :, :, ch] = np.where(inside, _sample(I[i:i + 1, :, :, ch], np.zeros((1, 1, 1), np.int64), k)[0], 0.0)
        valid[i] = inside
    return convert(out, out_dtype), valid


def path_reference(A, radius, crop=1.0, size=None):
    """the sampling matrices (T, 2, 3) of tensors.stabilizing_transforms for pair motions A (T - 1, 2, 3)"""
    A = np.asarray(A, np.float64)
    T = A.shape[0] + 1
    h = lambda m: np.vstack([m, [0.0, 0.0, 1.0]])  # noqa: E731
    P = [np.eye(3)]
    for t in range(T - 1):
        P.append(h(A[t]) @ P[-1])
    cx, cy = ((size[1] - 1) / 2.0, (size[0] - 1) / 2.0) if size is not None else (0.0, 0.0)
    Z = np.array([[crop, 0.0, cx * (1 - crop)], [0.0, crop, cy * (1 - crop)], [0.0, 0.0, 1.0]])
    out = []
    for t in range(T):
        S, G = np.zeros((3, 3)), 0.0
        for k in range(-radius, radius + 1):
            if 0 <= t + k < T:
                g = math.exp(-k * k / (2 * (radius / 2) ** 2)) if radius else 1.0
                S, G = S + g * P[t + k], G + g
        out.append((P[t] @ np.linalg.inv(S / G) @ Z)[:2])
    return np.array(out)


def apply(m, x, y):
    """a (2, 3) matrix applied to points"""
    return m[0, 0] * x + m[0, 1] * y + m[0, 2], m[1, 0] * x + m[1, 1] * y + m[1, 2]


def corner_distance(m1, m2, H, W):
    """the largest distance in pixels between where two (2, 3) matrices send the four image corners"""
    x, y = np.array([0.0, W - 1, 0.0, W - 1]), np.array([0.0, 0.0, H - 1, H - 1])
    a, b = apply(m1, x, y), apply(m2, x, y)
    return float(np.max(np.hypot(a[0] - b[0], a[1] - b[1])))
