"""Forward warping (include/papof.h: papof_splat_tensor, papof_interp_splat_tensor) restated in numpy -- the rule that
tests/test_splat_cpu.py checks with known answers and tests/test_gpu_splat.py compares the device's output with, byte for
byte.  Every term is one product of doubles (numpy does not contract a * b + c) and one rint, and the sums are int64
(np.add.at): integer addition is associative, so the bits are the kernel's whatever order its atomic adds arrive in."""
import numpy as np

from _interp_ref import as_f64, convert, interp_reference

FIX = 4294967296.0  # 2^32
MIN_DEN = 256  # a coverage of 2^-24


def accumulate(x, flow, weight, t, inv_bound=1.0):
    """x (B, H, W, C) float64, flow (B, 2, H, W), weight None or (B, H, W), one time t -> (num (B, H, W, C) int64,
    den (B, H, W) int64, kept: the sum of the quantised wb of the taps that were kept, a Python int)"""
    B, H, W, C = x.shape
    u, v = np.asarray(flow[:, 0], np.float64), np.asarray(flow[:, 1], np.float64)
    w = np.ones((B, H, W)) if weight is None else np.asarray(weight, np.float64)
    num, den = np.zeros((B, H, W, C), np.int64), np.zeros((B, H, W), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(w) & (w > 0)
        w = np.where(ok, np.minimum(w, 1.0), 0.0)
        X = np.arange(W, dtype=np.float64)[None, None, :] + float(t) * np.where(ok, u, 0.0)
        Y = np.arange(H, dtype=np.float64)[None, :, None] + float(t) * np.where(ok, v, 0.0)
        ok &= (X > -1.0) & (X < W) & (Y > -1.0) & (Y < H)
    X, Y = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
    x0, y0 = np.floor(X), np.floor(Y)
    fx, fy = X - x0, Y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    val = np.fmin(np.fmax(x * inv_bound, -1.0), 1.0)
    b = np.broadcast_to(np.arange(B)[:, None, None], (B, H, W))
    kept = 0
    for m in (0, 1):
        for n in (0, 1):
            tx, ty = x0 + n, y0 + m
            wb = w * ((fy if m else 1.0 - fy) * (fx if n else 1.0 - fx))
            keep = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & (wb != 0)
            q = np.rint(wb[keep] * FIX).astype(np.int64)
            kept += int(q.sum())
            np.add.at(den, (b[keep], ty[keep], tx[keep]), q)
            np.add.at(num, (b[keep], ty[keep], tx[keep]), np.rint((wb[keep][:, None] * val[keep]) * FIX).astype(np.int64))
    return num, den, kept


def splat_reference(x, flow, times, weight=None, bound=1.0, fill=0.0, out_dtype=np.float64):
    """x (B, H, W, C) uint8 / float32 / float64; flow (B, 2, H, W); weight None or (B, H, W); times: finite values ->
    (out (B, K, H, W, C) of out_dtype, coverage (B, K, H, W) float64)"""
    x = as_f64(x)
    B, H, W, C = x.shape
    out, cov = np.empty((B, len(times), H, W, C)), np.empty((B, len(times), H, W))
    for j, t in enumerate(times):
        num, den, _ = accumulate(x, flow, weight, t, 1.0 / bound)
        cov[:, j] = den.astype(np.float64) * (1.0 / FIX)
        d = np.where(den >= MIN_DEN, den, 1).astype(np.float64)[..., None]
        out[:, j] = np.where((den >= MIN_DEN)[..., None], (num.astype(np.float64) / d) * bound, fill)
    return convert(out, out_dtype), cov


def interp_splat_reference(im1, im2, flow_fw, flow_bw, times, weights=None, occlusion=None, out_dtype=np.float64):
    """im1, im2 (B, H, W, C); flow_fw, flow_bw (B, 2, H, W); weights None or (w_fw, w_bw), each None or (B, H, W);
    occlusion as interp_reference's; times inside (0, 1) -> (B, K, H, W, C) of out_dtype"""
    I0, I1 = as_f64(im1), as_f64(im2)
    w_fw, w_bw = (None, None) if weights is None else weights
    out = interp_reference(im1, im2, flow_fw, flow_bw, times, occlusion)  # the holes' values
    for j, t in enumerate(times):
        t = float(t)
        s = 1.0 - t
        n0, d0, _ = accumulate(I0, flow_fw, w_fw, t)
        n1, d1, _ = accumulate(I1, flow_bw, w_bw, 1.0 - t)
        den = s * d0.astype(np.float64) + t * d1.astype(np.float64)
        num = s * n0.astype(np.float64) + t * n1.astype(np.float64)
        hit = den >= float(MIN_DEN)
        out[:, j] = np.where(hit[..., None], num / np.where(hit, den, 1.0)[..., None], out[:, j])
    return convert(out, out_dtype)


def photometric_weights(im, warped, alpha=20.0):
    """tensors.splat_weights' formula on (B, H, W, C) arrays"""
    return np.exp(np.maximum(-alpha * np.abs(as_f64(im) - as_f64(warped)).mean(-1), -11.0))
