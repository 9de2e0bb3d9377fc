"""papof_warp_rows_tensor of include/papof.h restated in numpy fp64, bytes included (numpy does not contract a * b + c and
divides with correct rounding; the sampler is tests/_homography_ref.py's, which is tests/_interp_ref.py's) -- the rule that
tests/test_rows_cpu.py checks with known answers and tests/test_gpu_rows.py compares the device's bytes with.  Also the
rotating rolling-shutter camera of both test files: a continuous R(tau), the rays an output pixel shows, and the picture scene
rendered from the committed frame."""
import math

import numpy as np

from _homography_ref import _point
from _interp_ref import _sample, _taps, as_f64, convert

BRANCHES = ("one_knot", "no_clamp", "clamp_low", "clamp_high", "last_interval", "dead_d", "dead_xy", "nan_iterate")
MAX_ITERS = 8


def rows_points(table, H, W, iters, seen=None):
    """the rule's (X, Y, inside) (H, W) each for one frame's table (Kn, 3, 3) float64; `seen` counts the branches taken"""
    seen = dict.fromkeys(BRANCHES, 0) if seen is None else seen
    Kn = table.shape[0]
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if Kn == 1:
        X, Y, front = _point(table[0], x, r)
        seen["one_knot"] += x.size
    else:
        assert H >= 2 and 1 <= iters <= MAX_ITERS
        g = float(Kn - 1) / float(H - 1)
        Y = r
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in range(iters):
                low, high = ~(Y >= 0), Y > H - 1
                seen["clamp_low"] += int(low.sum())
                seen["clamp_high"] += int(high.sum())
                seen["no_clamp"] += int((~low & ~high).sum())
                seen["nan_iterate"] += int(np.isnan(Y).sum())
                Yc = np.where(low, 0.0, np.where(high, float(H - 1), Y))
                s = Yc * g
                k = s.astype(np.int64)
                seen["last_interval"] += int((k > Kn - 2).sum())
                k = np.minimum(k, Kn - 2)
                f = s - k.astype(np.float64)
                A, B = table[k], table[k + 1]  # (H, W, 3, 3)
                m = A + f[..., None, None] * (B - A)
                X, Y, front = _point(m, x, r)
    with np.errstate(invalid="ignore"):
        inside = front & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    seen["dead_d"] += int((~front).sum())
    seen["dead_xy"] += int((front & ~inside).sum())
    return X, Y, inside


def warp_rows_reference(frames, tables, iters=3, out_dtype=None, parts=False):
    """frames (B, H, W, C) uint8 / float32 / float64, tables (B, Kn, 3, 3) float32 / float64 -> (out (B, H, W, C) of out_dtype
    -- by default the frames' --, valid (B, H, W) bool); parts=True: also the points (B, H, W, 2) (x, y) and the counts of
    the branches taken (BRANCHES)"""
    I = as_f64(frames)
    M = np.asarray(tables)
    assert M.dtype in (np.float32, np.float64) and M.ndim == 4 and M.shape[2:] == (3, 3) and M.shape[0] == I.shape[0]
    M = M.astype(np.float64)
    B, H, W, C = I.shape
    out = np.zeros((B, H, W, C))
    valid = np.zeros((B, H, W), bool)
    P = np.empty((B, H, W, 2))
    seen = dict.fromkeys(BRANCHES, 0)
    for i in range(B):
        X, Y, inside = rows_points(M[i], H, W, iters, seen)
        k = _taps(np.where(inside, X, 0.0)[None], np.where(inside, Y, 0.0)[None], H, W)
        for ch in range(C):
            out[i, :, :, ch] = np.where(inside, _sample(I[i:i + 1, :, :, ch], np.zeros((1, 1, 1), np.int64), k)[0], 0.0)
        valid[i] = inside
        P[i, ..., 0], P[i, ..., 1] = X, Y
    res = convert(out, np.asarray(frames).dtype if out_dtype is None else out_dtype), valid
    return res + (P, seen) if parts else res


# ---- the camera of the tests: a rotation R(tau), tau in frame intervals, read by a rolling shutter
def rodrigues(w):
    """exp([w]x) of the rotation vectors w (..., 3): (..., 3, 3)"""
    w = np.asarray(w, np.float64)
    t = np.sqrt((w * w).sum(-1))[..., None, None]
    Kx = np.zeros(w.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    small = t < 1e-8
    ts = np.where(small, 1.0, t)
    a = np.where(small, 1.0, np.sin(ts) / ts)
    b = np.where(small, 0.5, (1.0 - np.cos(ts)) / (ts * ts))
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def shaken_path(periods, amp=0.02, drift=0.004):
    """R(tau): a drift about the vertical axis plus two sinusoids of `periods` frames about the two image axes and a smaller
    roll, as one rotation vector -- tau an array -> (..., 3, 3)"""
    p1, p2 = periods

    def R(tau):
        tau = np.asarray(tau, np.float64)
        w = np.stack([amp * np.sin(2 * math.pi * tau / p1 + 0.3),
                      drift * tau + amp * np.sin(2 * math.pi * tau / p2 + 1.1),
                      0.3 * amp * np.sin(2 * math.pi * tau / p1 + 2.0)], -1)
        return rodrigues(w)
    return R


def camera(f, H, W):
    return np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def row_times(H, readout, anchor=0.5):
    """tau of each source row: readout * (y - a) / H, a = anchor * (H - 1)"""
    return readout * (np.arange(H, dtype=np.float64) - anchor * (H - 1)) / H


def ray_error(P, inside, R, t, S, f, H, W, readout, anchor=0.5, Z=None):
    """the distance in pixels between the world ray that output pixel q of frame t shows -- it shows source point P (H, W, 2)
    of a camera R(t + tau(row of P)) -- and the ray S^T K^-1 Z q it should show, both seen through K S: (the sum of its
    squares over `inside`, their number), for rms()"""
    K = camera(f, H, W)
    Ki = np.linalg.inv(K)
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    q = np.stack([x, r, np.ones_like(x)], -1)
    if Z is not None:
        q = q @ Z.T
    p = np.stack([P[..., 0], P[..., 1], np.ones_like(x)], -1)
    tau = readout * (P[..., 1] - anchor * (H - 1)) / H
    with np.errstate(invalid="ignore"):
        Rp = R(t + np.where(inside, tau, 0.0))                             # (H, W, 3, 3)
        d = np.einsum("hwji,hwj->hwi", Rp, p @ Ki.T)                       # R^T K^-1 p: the ray shown
        back = np.einsum("ij,hwj->hwi", K @ S, d)                          # seen through the stabilized camera
        e = back[..., :2] / back[..., 2:] - q[..., :2] / q[..., 2:]
    e2 = (e * e).sum(-1)[inside]
    return float(e2.sum()), int(e2.size)


def rms(parts):
    """the RMS of ray_error's (sum of squares, count) pairs"""
    parts = list(parts)
    return math.sqrt(sum(p[0] for p in parts) / sum(p[1] for p in parts))


def render(texture, rot, f, H, W, ft):
    """a frame (H, W, C) uint8 of the distant picture `texture` (Ht, Wt, C) float64 in 0 .. 255, which a camera of focal length
    ft at the identity sees pixel for pixel: pixel (x, y) shows the ray R_y^T K^-1 (x, y, 1), rot (3, 3) or one rotation per row
    (H, 3, 3) -- the camera while row y is read --, sampled bilinearly; every ray must fall inside the picture"""
    Ht, Wt, _ = texture.shape
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    p = np.stack([x, r, np.ones_like(x)], -1) @ np.linalg.inv(camera(f, H, W)).T
    rot = np.broadcast_to(rot, (H, 3, 3))
    u = np.einsum("hji,hwj->hwi", rot, p) @ camera(ft, Ht, Wt).T
    X, Y = u[..., 0] / u[..., 2], u[..., 1] / u[..., 2]
    assert X.min() >= 0 and X.max() < Wt - 1 and Y.min() >= 0 and Y.max() < Ht - 1
    x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int)
    fx, fy = (X - x0)[..., None], (Y - y0)[..., None]
    v = (texture[y0, x0] * (1 - fx) + texture[y0, x0 + 1] * fx) * (1 - fy) + \
        (texture[y0 + 1, x0] * (1 - fx) + texture[y0 + 1, x0 + 1] * fx) * fy
    return np.rint(v).astype(np.uint8)
