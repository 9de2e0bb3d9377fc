"""The fill and the propagation of flow-guided video completion (include/papof.h: papof_fill_holes_tensor,
papof_propagate_tensor) restated in numpy fp64 -- the rules that tests/test_inpaint_cpu.py checks with known answers and
tests/test_gpu_inpaint.py compares the device's outputs with, byte for byte.  The hop is test_track_cpu's (_step: k_track's
step), the bilinear taps _interp_ref's (_taps).  numpy does not contract a * b + c and divides with correct rounding: the
bits are the kernels'."""
import numpy as np

from _interp_ref import _taps, as_f64, convert, sample_plane
from test_track_cpu import _step


def level_sizes(H, W):
    """[(h_l, w_l)] of the fill's levels: ceil-halved down to 1 x 1"""
    s = [(H, W)]
    while s[-1] != (1, 1):
        s.append(((s[-1][0] + 1) // 2, (s[-1][1] + 1) // 2))
    return s


def _pull(V, K):
    """level l + 1 of (V (n, h, w, C) values, K (n, h, w) known): the mean of the known children, (a, b) in order"""
    n, h, w, C = V.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    Vp, Kp = np.zeros((n, 2 * h2, 2 * w2, C)), np.zeros((n, 2 * h2, 2 * w2), bool)  # children beyond level l: not known
    Vp[:, :h, :w], Kp[:, :h, :w] = V, K
    S, N = np.zeros((n, h2, w2, C)), np.zeros((n, h2, w2), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in (0, 1):
            for b in (0, 1):
                k = Kp[:, a::2, b::2]
                S = S + np.where(k[..., None], Vp[:, a::2, b::2], 0.0)  # (S is never -0.0: adding +0.0 is exact)
                N = N + k
    known = N > 0
    with np.errstate(invalid="ignore", over="ignore"):
        V2 = np.where(known[..., None], S / np.maximum(N, 1)[..., None].astype(np.float64), 0.0)
    return V2, known


def _push(V, K, V2, K2, it2):
    """level l's unknown pixels from the filled level l + 1 (its unknown pixels' values in it2): bilinear at
    (0.5 x - 0.25, 0.5 y - 0.25) clamped into level l + 1"""
    n, h, w, C = V.shape
    h2, w2 = V2.shape[1:3]
    X = np.clip(0.5 * np.arange(w, dtype=np.float64) - 0.25, 0.0, float(w2 - 1))[None, :] + np.zeros((h, 1))
    Y = np.clip(0.5 * np.arange(h, dtype=np.float64) - 0.25, 0.0, float(h2 - 1))[:, None] + np.zeros((1, w))
    U = np.where(K2[..., None], V2, it2)
    g = np.zeros((n, h, w, C))
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, cols, wt in _taps(X, Y, h2, w2):
            g = g + U[:, rows, cols, :] * wt[None, :, :, None]
    return np.where(K[..., None], V, g)


def _sweep(V, K, it):
    """one Jacobi sweep over the unknown pixels: ((N + S) + (W + E)) * 0.25, neighbours clamped"""
    h, w = V.shape[1:3]
    U = np.where(K[..., None], V, it)
    r, c = np.arange(h), np.arange(w)
    rn, rs = np.maximum(r - 1, 0), np.minimum(r + 1, h - 1)
    cw, ce = np.maximum(c - 1, 0), np.minimum(c + 1, w - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        new = ((U[:, rn] + U[:, rs]) + (U[:, :, cw] + U[:, :, ce])) * 0.25
    return np.where(K[..., None], V, new)


def fill_reference(x, mask, relax, out_dtype=np.float64):
    """x (n, H, W, C) uint8 / float32 / float64, mask (n, H, W) (nonzero: a hole), relax sweeps per level -> out (n, H, W, C)
    of out_dtype"""
    V0 = as_f64(x)
    K0 = np.asarray(mask) == 0
    V0 = np.where(K0[..., None], V0, 0.0)
    levels = [(V0, K0)]
    while levels[-1][0].shape[1:3] != (1, 1):
        levels.append(_pull(*levels[-1]))
    # the filled values of the coarsest level: its own
    it = levels[-1][0]
    for l in range(len(levels) - 2, -1, -1):
        V, K = levels[l]
        V2, K2 = levels[l + 1]
        it = _push(V, K, V2, K2, it)
        for _ in range(relax):
            it = _sweep(V, K, it)
    V, K = levels[0]
    return convert(np.where(K[..., None], V, it), out_dtype)


def propagate_reference(frames, masks, flow_fw, flow_bw, radius, consistency=(0.01, 0.5), out_dtype=np.float64):
    """frames (T, H, W, C) uint8 / float32 / float64, masks (T, H, W) (nonzero: a hole), flow_fw, flow_bw (T - 1, 2, H, W)
    (vx, vy), radius 1 .. T - 1, consistency (alpha1, alpha2) or None: no check -> (out (T, H, W, C) of out_dtype, status
    (T, H, W) uint8: 0 not a hole, 1 filled, 2 still a hole)"""
    F = as_f64(frames)
    M = np.asarray(masks) != 0
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    T, H, W, C = F.shape
    check = consistency is not None
    a1, a2 = (float(consistency[0]), float(consistency[1])) if check else (0.0, 0.0)
    n = np.arange(H * W)
    x0, y0 = (n % W).astype(np.float64), (n // W).astype(np.float64)
    out = np.empty((T, H * W, C))
    status = np.zeros((T, H * W), np.uint8)
    for t in range(T):
        c = F[t].reshape(-1, C)
        hole = M[t].reshape(-1)
        cand = []
        for d in (1, -1):
            X, Y, active = x0.copy(), y0.copy(), hole.copy()
            g, dist = np.zeros((H * W, C)), np.zeros(H * W, np.int64)
            steps = min(radius, T - 1 - t) if d > 0 else min(radius, t)
            for j in range(1, steps + 1):
                pair = t + j - 1 if d > 0 else t - j
                f, b = (fw[pair], bw[pair]) if d > 0 else (bw[pair], fw[pair])
                X, Y, active = _step(f, b, X, Y, active, check, a1, a2)
                taps = _taps(np.where(active, X, 0.0), np.where(active, Y, 0.0), H, W)
                clear = active.copy()
                for rows, cols, _ in taps:
                    clear &= ~M[t + d * j][rows, cols]
                for k in range(C):
                    g[:, k] = np.where(clear, sample_plane(F[t + d * j][..., k], taps), g[:, k])
                dist = np.where(clear, j, dist)
                active = active & ~clear  # the chain stops where it found its candidate
            cand.append((g, dist))
        (gf, df), (gb, db) = cand
        both, only_f, only_b = (df > 0) & (db > 0), (df > 0) & (db == 0), (df == 0) & (db > 0)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            wf, wb = (1.0 / np.maximum(df, 1))[:, None], (1.0 / np.maximum(db, 1))[:, None]
            mix = (wf * gf + wb * gb) / (wf + wb)
        o = np.where(both[:, None], mix, np.where(only_f[:, None], gf, np.where(only_b[:, None], gb, c)))
        out[t] = o
        status[t] = np.where(~hole, 0, np.where((df > 0) | (db > 0), 1, 2))
    return convert(out.reshape(T, H, W, C), out_dtype), status.reshape(T, H, W)
