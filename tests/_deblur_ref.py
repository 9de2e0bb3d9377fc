"""The deblurring rule of include/papof.h (papof_deblur_tensor) restated in numpy fp64, in the header's order of operations
-- the rule that tests/test_deblur_cpu.py checks with known answers and quality bars and tests/test_gpu_deblur.py compares
the device's output with, byte for byte.  The taps are _interp_ref's (_taps), the frame sampler _interp_ref's (sample_plane),
the flow sampler and the hop test_track_cpu's (_bilinear, _step: k_track's step).  numpy does not contract a * b + c and
divides with correct rounding: the bits are the kernel's."""
import numpy as np

from _interp_ref import _taps, as_f64, convert, sample_plane
from test_track_cpu import _bilinear, _step

EPS = 2.0 ** -10
# what the census of tests/test_gpu_deblur.py counts (lanes, summed over iterations): chains that died and velocities that
# were not finite in either pass, estimates under the floor, sample points that were clamped, slots outside the video,
# pixels whose update had no slot left
BRANCHES = ("dead_a", "nonfinite_a", "floor", "clamped_a", "dead_b", "nonfinite_b", "clamped_b", "absent", "unchanged")


def slots(t, T, R):
    """[(slot index j, frame s)] of target t in the rule's order, t, t + 1, t - 1, t + 2, ..., without the absent ones"""
    order = [t]
    for d in range(1, R + 1):
        order += [t + d, t - d]
    return [(j, s) for j, s in enumerate(order) if 0 <= s < T]


def _chain(fw, bw, a, b, X, Y, check, a1, a2):
    """the chain of the points (X, Y) from frame a to frame b: (X, Y, alive)"""
    alive = np.ones(X.shape, bool)
    for f in range(a, b):
        X, Y, alive = _step(fw[f], bw[f], X, Y, alive, check, a1, a2)
    for f in range(a, b, -1):
        X, Y, alive = _step(bw[f - 1], fw[f - 1], X, Y, alive, check, a1, a2)
    return X, Y, alive


def _velocity(s, T, f, b):
    """the velocity of frame s from (fu, fv) of flow_fw[s] and (bu, bv) of flow_bw[s - 1] (None on the side an end frame lacks)"""
    with np.errstate(invalid="ignore", over="ignore"):
        if s == 0:
            return f[0], f[1]
        if s == T - 1:
            return 0.0 - b[0], 0.0 - b[1]
        return 0.5 * (f[0] - b[0]), 0.5 * (f[1] - b[1])


def _velocity_at_pixels(fw, bw, s, T):
    f = (fw[s, 0].ravel(), fw[s, 1].ravel()) if s < T - 1 else None
    b = (bw[s - 1, 0].ravel(), bw[s - 1, 1].ravel()) if s > 0 else None
    return _velocity(s, T, f, b)


def _velocity_at_points(fw, bw, s, T, X, Y):
    f = _bilinear(fw[s], X, Y) if s < T - 1 else None
    b = _bilinear(bw[s - 1], X, Y) if s > 0 else None
    return _velocity(s, T, f, b)


def _line(img, X, Y, vx, vy, table, sign, use):
    """(sum over the table, k ascending, of w_k * (img (H, W, C) sampled at the clamped points (X, Y) +- tau_k (vx, vy))
    (N, C), how many sample points of the lanes `use` were clamped)"""
    H, W, C = img.shape
    acc = np.zeros((X.size, C))
    clamped = 0
    for tau, w in table:
        xs, ys = (X + tau * vx, Y + tau * vy) if sign > 0 else (X - tau * vx, Y - tau * vy)
        Xs, Ys = np.fmin(np.fmax(xs, 0.0), float(W - 1)), np.fmin(np.fmax(ys, 0.0), float(H - 1))
        clamped += int((use & ((Xs != xs) | (Ys != ys))).sum())
        taps = _taps(Xs, Ys, H, W)
        with np.errstate(invalid="ignore", over="ignore"):
            for ch in range(C):
                acc[:, ch] = acc[:, ch] + w * sample_plane(img[..., ch], taps)
    return acc, clamped


def deblur_reference(frames, flow_fw, flow_bw, offsets, weights, radius=1, iters=6, consistency=(0.01, 0.5),
                     out_dtype=np.float64, targets=None, parts=False, each=None):
    """frames (T, H, W, C) uint8 / float32 / float64; flow_fw, flow_bw (T - 1, 2, H, W) (vx, vy); offsets, weights: the sample
    table; consistency (alpha1, alpha2) or None: no check; targets: the frames to compute, in the order given (None: all;
    the others come back as zeros); each(t, iteration, L (H, W, C)): called after every update -> (out (T, H, W, C) of
    out_dtype, support (T, H, W) uint8), with parts=True also the census {branch: count}"""
    F = as_f64(frames)
    with np.errstate(invalid="ignore"):
        B = np.fmax(F, 0.0)
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    T, H, W, C = F.shape
    check = consistency is not None
    a1, a2 = (float(consistency[0]), float(consistency[1])) if check else (0.0, 0.0)
    table = [(float(tau), float(w)) for tau, w in zip(offsets, weights) if w != 0]
    wsum = 0.0
    for _, w in table:
        wsum = wsum + w
    n_pix = np.arange(H * W)
    x0, y0 = (n_pix % W).astype(np.float64), (n_pix // W).astype(np.float64)
    zero = np.zeros(H * W)
    out = np.zeros((T, H, W, C))
    support = np.zeros((T, H, W), np.uint8)
    seen = dict.fromkeys(BRANCHES, 0)
    for t in (range(T) if targets is None else targets):
        L = B[t].copy()
        seen["absent"] += (2 * radius + 1 - len(slots(t, T, radius))) * H * W
        for it in range(iters):
            ratios = {}
            for j, s in slots(t, T, radius):  # pass A
                X, Y, alive = _chain(fw, bw, s, t, x0.copy(), y0.copy(), check, a1, a2)
                vx, vy = _velocity_at_pixels(fw, bw, s, T)
                finite = np.isfinite(vx) & np.isfinite(vy)
                use = alive & finite
                seen["dead_a"] += int((~alive).sum())
                seen["nonfinite_a"] += int((alive & ~finite).sum())
                est, clamped = _line(L, np.where(use, X, zero), np.where(use, Y, zero), np.where(use, vx, zero),
                                     np.where(use, vy, zero), table, +1, use)
                seen["clamped_a"] += clamped
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    est = est / wsum
                    seen["floor"] += int((use[:, None] & ~(est >= EPS)).sum())
                    ratio = B[s].reshape(-1, C) / np.fmax(est, EPS)
                ratios[j] = np.where(use[:, None], ratio, 1.0).reshape(H, W, C)
            corr, n = np.zeros((H * W, C)), np.zeros(H * W, np.int64)  # pass B
            for j, s in slots(t, T, radius):
                X, Y, alive = _chain(fw, bw, t, s, x0.copy(), y0.copy(), check, a1, a2)
                Xa, Ya = np.where(alive, X, zero), np.where(alive, Y, zero)
                vx, vy = _velocity_at_points(fw, bw, s, T, Xa, Ya)
                finite = np.isfinite(vx) & np.isfinite(vy)
                use = alive & finite
                seen["dead_b"] += int((~alive).sum())
                seen["nonfinite_b"] += int((alive & ~finite).sum())
                cs, clamped = _line(ratios[j], np.where(use, X, zero), np.where(use, Y, zero), np.where(use, vx, zero),
                                    np.where(use, vy, zero), table, -1, use)
                seen["clamped_b"] += clamped
                with np.errstate(invalid="ignore", over="ignore"):
                    corr = np.where(use[:, None], corr + cs / wsum, corr)
                n = n + use
            seen["unchanged"] += int((n == 0).sum())
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                new = L.reshape(-1, C) * (corr / np.maximum(n, 1).astype(np.float64)[:, None])
            L = np.where((n > 0)[:, None], new, L.reshape(-1, C)).reshape(H, W, C)
            if each is not None:
                each(t, it, L)
        out[t] = L
        support[t] = n.reshape(H, W)
    res = (convert(out, out_dtype), support)
    return res + (seen,) if parts else res
