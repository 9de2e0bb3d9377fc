"""Blind video temporal consistency (include/papof.h: papof_temporal_consistency_tensor) restated in numpy fp64 -- the rule
that tests/test_consistency_cpu.py checks with known answers and calibrates, and tests/test_gpu_consistency.py compares the
device's output with, byte for byte.  The hop is test_track_cpu's (_step: k_track's step, k_temporal_filter's backward
hop), the bilinear taps _interp_ref's (_taps), the levels and the push point _inpaint_ref's.  numpy does not contract
a * b + c and divides with correct rounding: the bits are the kernels'."""
import numpy as np

from _interp_ref import _taps, as_f64, convert
from test_track_cpu import _step


def _sample(img, taps):
    """img (H, W, C) sampled at the taps, accumulated from 0 in (m, n) order -> (N, C)"""
    g = np.zeros(taps[0][0].shape + img.shape[-1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, cols, w in taps:
            g = g + img[rows, cols] * w[:, None]
    return g


def _pull(V, A):
    """level l + 1 of (V (h, w, C) values, A (h, w) confidences): over the children (a, b) in order, from 0,
    A' = sum a, S = sum a v; v = S / A' where A' > 0, else 0; a = min(A', 1)"""
    h, w, C = V.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    Vp, Ap = np.zeros((2 * h2, 2 * w2, C)), np.zeros((2 * h2, 2 * w2))  # children beyond level l: absent (confidence 0)
    Vp[:h, :w], Ap[:h, :w] = V, A
    S, N = np.zeros((h2, w2, C)), np.zeros((h2, w2))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in (0, 1):
            for b in (0, 1):
                k = Ap[a::2, b::2]
                # an absent child adds +0.0 to A (exact) and +0.0 * v = +0.0 to S (S is never -0.0: S starts at +0.0)
                N = N + k
                S = S + k[..., None] * Vp[a::2, b::2]
        V2 = np.where((N > 0)[..., None], S / np.where(N > 0, N, 1.0)[..., None], 0.0)
    return V2, np.minimum(N, 1.0)


def _push(V, A, V2):
    """level l from the pushed level l + 1: a v + (1 - a) g, g bilinear at (0.5 x - 0.25, 0.5 y - 0.25) clamped"""
    h, w, C = V.shape
    h2, w2 = V2.shape[:2]
    X = (np.clip(0.5 * np.arange(w, dtype=np.float64) - 0.25, 0.0, float(w2 - 1))[None, :] + np.zeros((h, 1))).ravel()
    Y = (np.clip(0.5 * np.arange(h, dtype=np.float64) - 0.25, 0.0, float(h2 - 1))[:, None] + np.zeros((1, w))).ravel()
    g = _sample(V2, _taps(X, Y, h2, w2)).reshape(h, w, C)
    with np.errstate(invalid="ignore", over="ignore"):
        return A[..., None] * V + (1.0 - A)[..., None] * g


def start_value(r, a):
    """delta0 (H, W, C): the pull-push of r (H, W, C) with confidences a (H, W)"""
    levels = [(r, a)]
    while levels[-1][0].shape[:2] != (1, 1):
        levels.append(_pull(*levels[-1]))
    v = levels[-1][0]
    for l in range(len(levels) - 2, -1, -1):
        v = _push(levels[l][0], levels[l][1], v)
    return v


def _neighbours(H, W):
    r, c = np.mgrid[0:H, 0:W]
    return ((r > 0).astype(np.float64) + (r < H - 1)) + ((c > 0).astype(np.float64) + (c < W - 1))


def jacobi(delta, w, r, iters):
    """`iters` sweeps of delta <- (S + w r) / (n + w) (0 where n + w = 0), S = ((N + S) + (W + E)) with a neighbour outside
    the image entering as +0.0"""
    H, W, C = delta.shape
    den = _neighbours(H, W) + w
    wr = w[..., None] * r
    for _ in range(iters):
        p = np.zeros((H + 2, W + 2, C))
        p[1:-1, 1:-1] = delta
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            S = (p[:-2, 1:-1] + p[2:, 1:-1]) + (p[1:-1, :-2] + p[1:-1, 2:])
            delta = np.where((den != 0)[..., None], (S + wr) / np.where(den != 0, den, 1.0)[..., None], 0.0)
    return delta


def frame_terms(I_t, I_prev, O_prev, P_t, fw, bw, lam, sigma, consistency):
    """(w (H, W), a (H, W), r (H, W, C_P)) of one frame: I_t, I_prev (H, W, C_I) fp64, O_prev (H, W, C_P) fp64 (the stored
    previous output read back), P_t (H, W, C_P) fp64, fw = flow_fw[t - 1], bw = flow_bw[t - 1] (2, H, W) fp64"""
    H, W, CI = I_t.shape
    n = np.arange(H * W)
    x0, y0 = (n % W).astype(np.float64), (n // W).astype(np.float64)
    check = consistency is not None
    a1, a2 = (float(consistency[0]), float(consistency[1])) if check else (0.0, 0.0)
    X, Y, valid = _step(bw, fw, x0, y0, np.ones(H * W, bool), check, a1, a2)
    taps = _taps(np.where(valid, X, 0.0), np.where(valid, Y, 0.0), H, W)
    Ih = _sample(I_prev, taps)
    Oh = _sample(O_prev, taps)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        D = np.zeros(H * W)
        for k in range(CI):
            d = I_t.reshape(-1, CI)[:, k] - Ih[:, k]
            D = D + d * d
        D = D / CI
        w = lam / (1.0 + D / (sigma * sigma)) if sigma > 0 else np.full(H * W, float(lam))
        on = valid & (w > 0)
        w = np.where(on, w, 0.0)
        a = np.where(on, w / (lam if lam > 0 else 1.0), 0.0)
        r = np.where(on[:, None], Oh - P_t.reshape(H * W, -1), 0.0)
    return w.reshape(H, W), a.reshape(H, W), r.reshape(H, W, -1)


def consistency_reference(frames, processed, flow_fw, flow_bw, lam, sigma, iters, consistency=(0.01, 0.5), first=None,
                          out_dtype=None):
    """frames (T, H, W, C_I), processed (T, H, W, C_P) uint8 / float32 / float64; flow_fw, flow_bw (T - 1, 2, H, W) (vx, vy);
    consistency (alpha1, alpha2) or None: no check; first None or (H, W, C_P) -> out (T, H, W, C_P) of out_dtype (None:
    processed's dtype)"""
    out_dtype = np.dtype(processed.dtype if out_dtype is None else out_dtype)
    I = as_f64(frames)
    P = as_f64(processed)
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    T = P.shape[0]
    out = np.empty(P.shape, out_dtype)
    out[0] = convert(as_f64(first) if first is not None else P[0], out_dtype)
    for t in range(1, T):
        O_prev = as_f64(out[t - 1])
        w, a, r = frame_terms(I[t], I[t - 1], O_prev, P[t], fw[t - 1], bw[t - 1], lam, sigma, consistency)
        d = jacobi(start_value(r, a), w, r, iters)
        with np.errstate(invalid="ignore", over="ignore"):
            out[t] = convert(P[t] + d, out_dtype)
    return out
