"""Multi-frame super-resolution (include/papof.h: papof_super_resolve_tensor) restated in numpy -- the rule that
tests/test_superres_cpu.py checks with known answers and tests/test_gpu_superres.py compares the device's output with, byte
for byte.  The hop is test_track_cpu's (_step), the frame sampler _interp_ref's (_taps), the deposit _splat_ref's tap rule on
the fine grid: every term is one product of doubles (numpy does not contract a * b + c) and one rint, and the sums are
int64 (np.add.at), so the bits are the kernel's whatever order its atomic adds arrive in."""
import numpy as np

from _interp_ref import _taps, as_f64, convert, sample_plane
from test_track_cpu import _step

FIX = 4294967296.0  # 2^32


def deposit(num, den, S, PX, PY, w, val, keep):
    """the points (PX, PY) (N,) of the low-resolution grid with weights w (N,) and clamped values val (N, C), where `keep`,
    into num (S H, S W, C) / den (S H, S W) int64"""
    FH, FW = den.shape
    PX, PY, w = np.where(keep, PX, 0.0), np.where(keep, PY, 0.0), np.where(keep, w, 0.0)
    QX, QY = float(S) * (PX + 0.5) - 0.5, float(S) * (PY + 0.5) - 0.5
    x0, y0 = np.floor(QX), np.floor(QY)
    fx, fy = QX - x0, QY - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    for m in (0, 1):
        for n in (0, 1):
            tx, ty = x0 + n, y0 + m
            wb = w * ((fy if m else 1.0 - fy) * (fx if n else 1.0 - fx))
            k = keep & (tx >= 0) & (tx < FW) & (ty >= 0) & (ty < FH) & (wb != 0)
            np.add.at(den, (ty[k], tx[k]), np.rint(wb[k] * FIX).astype(np.int64))
            np.add.at(num, (ty[k], tx[k]), np.rint((wb[k][:, None] * val[k]) * FIX).astype(np.int64))


def accumulate(F, fw, bw, S, radius, sigma=None, consistency=None):
    """F (T, H, W, C) float64; fw, bw (T - 1, 2, H, W) -> num (T, S H, S W, C), den (T, S H, S W) int64"""
    T, H, W, C = F.shape
    check = consistency is not None
    a1, a2 = (float(consistency[0]), float(consistency[1])) if check else (0.0, 0.0)
    weighted = sigma is not None and sigma > 0
    s2 = float(sigma) * float(sigma) if weighted else 0.0
    num, den = np.zeros((T, S * H, S * W, C), np.int64), np.zeros((T, S * H, S * W), np.int64)
    n = np.arange(H * W)
    x0, y0 = (n % W).astype(np.float64), (n // W).astype(np.float64)
    everything = np.ones(H * W, bool)
    for k in range(T):
        v = F[k].reshape(-1, C)
        with np.errstate(invalid="ignore"):
            val = np.fmin(np.fmax(v, -1.0), 1.0)
        deposit(num[k], den[k], S, x0, y0, np.ones(H * W), val, everything)
        for d in (1, -1):
            X, Y, alive = x0.copy(), y0.copy(), everything.copy()
            steps = min(radius, T - 1 - k) if d > 0 else min(radius, k)
            for j in range(1, steps + 1):
                pair = k + j - 1 if d > 0 else k - j
                f, b = (fw[pair], bw[pair]) if d > 0 else (bw[pair], fw[pair])
                X, Y, alive = _step(np.asarray(f, np.float64), np.asarray(b, np.float64), X, Y, alive, check, a1, a2)
                taps = _taps(np.where(alive, X, 0.0), np.where(alive, Y, 0.0), H, W)
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    D = np.zeros(H * W)
                    for c in range(C):
                        dc = v[:, c] - sample_plane(F[k + d * j][..., c], taps)
                        D = D + dc * dc
                    D = D / C
                    w = 1.0 / (1.0 + D / s2) if weighted else np.ones(H * W)
                    enter = alive & (w > 0)
                deposit(num[k + d * j], den[k + d * j], S, X, Y, w, val, enter)
    return num, den


def cubic_weights(f):
    """the cubic convolution weights (Keys, a = -0.5) of the taps at -1, 0, 1, 2 for the fraction f"""
    return [((-0.5 * f + 1.0) * f - 0.5) * f, (1.5 * f - 2.5) * f * f + 1.0, ((-1.5 * f + 2.0) * f + 0.5) * f,
            (0.5 * f - 0.5) * f * f]


def _low(n, S):
    """(floor, fraction) of the low-resolution coordinates of the n * S fine pixels of an axis"""
    p = (np.arange(n * S, dtype=np.float64) + 0.5) / float(S) - 0.5
    p0 = np.floor(p)
    return p0.astype(np.int64), p - p0


def cubic_base(Y, S):
    """Y (H, W, C) float64 -> (S H, S W, C): the frame upsampled with the cubic convolution kernel, indices clamped"""
    H, W, C = Y.shape
    (x0, tx), (y0, ty) = _low(W, S), _low(H, S)
    wx, wy = cubic_weights(tx), cubic_weights(ty)
    base = np.zeros((S * H, S * W, C))
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(4):
            rows = np.clip(y0 - 1 + m, 0, H - 1)
            row = np.zeros((S * H, S * W, C))
            for n in range(4):
                cols = np.clip(x0 - 1 + n, 0, W - 1)
                row = row + wx[n][None, :, None] * Y[rows][:, cols]
            base = base + wy[m][:, None, None] * row
    return base


def resolve(num, den, Y, S, prior):
    """one target: num (S H, S W, C), den (S H, S W) int64, Y (H, W, C) -> (X (S H, S W, C), coverage (S H, S W))"""
    coverage = den.astype(np.float64) * (1.0 / FIX)
    with np.errstate(invalid="ignore", over="ignore"):
        X = (num.astype(np.float64) * (1.0 / FIX) + prior * cubic_base(Y, S)) / (coverage + prior)[..., None]
    return X, coverage


def backproject(X, Y, S):
    """one Jacobi step of one target: X (S H, S W, C), Y (H, W, C) -> X'"""
    H, W, C = Y.shape
    with np.errstate(invalid="ignore", over="ignore"):
        B = X.reshape(H, S, W, S, C)
        s = np.zeros((H, W, C))
        for m in range(S):
            for n in range(S):
                s = s + B[:, m, :, n]
        r = Y - s / float(S * S)
        (x0, tx), (y0, ty) = _low(W, S), _low(H, S)
        xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
        ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
        tx, ty = tx[None, :, None], ty[:, None, None]
        top = (1.0 - tx) * r[ya][:, xa] + tx * r[ya][:, xb]
        bot = (1.0 - tx) * r[yb][:, xa] + tx * r[yb][:, xb]
        return X + ((1.0 - ty) * top + ty * bot)


def superres_reference(frames, flow_fw, flow_bw, scale, radius=2, sigma=0.15, consistency=(0.01, 0.5), prior=0.05, iters=2,
                       out_dtype=None):
    """frames (T, H, W, C) uint8 / float32 / float64; flow_fw, flow_bw (T - 1, 2, H, W); sigma None or 0: no photometric
    weight; consistency (alpha1, alpha2) or None -> (video (T, S H, S W, C) of out_dtype (None: the frames'), coverage
    (T, S H, S W) float64)"""
    F = as_f64(frames)
    T, H, W, C = F.shape
    num, den = accumulate(F, flow_fw, flow_bw, scale, radius, sigma, consistency)
    video, coverage = np.empty((T, scale * H, scale * W, C)), np.empty((T, scale * H, scale * W))
    for t in range(T):
        X, coverage[t] = resolve(num[t], den[t], F[t], scale, float(prior))
        for _ in range(iters):
            X = backproject(X, F[t], scale)
        video[t] = X
    return convert(video, np.asarray(frames).dtype if out_dtype is None else out_dtype), coverage
