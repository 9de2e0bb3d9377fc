"""The frame interpolation of include/papof.h (papof_interp_tensor) restated in numpy fp64 -- the rule that
tests/test_interp_cpu.py checks with known answers and tests/test_gpu_interp.py compares the device's output with, byte for
byte.  numpy does not contract a * b + c and divides with correct rounding: the bits are the kernel's."""
import numpy as np


def as_f64(frames):
    """frames of uint8 (x / 255.0, as the flow's ingest), float32 (widened exactly) or float64 as float64"""
    a = np.asarray(frames)
    if a.dtype == np.uint8:
        return a.astype(np.float64) / 255.0
    return a.astype(np.float64)


def convert(out, dtype):
    """float64 results stored as `dtype`: float64 as is, float32 with one round-to-nearest, uint8 as
    clamp(rint(255 out), 0, 255) with rint half to even and NaN -> 0"""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return out
    if dtype == np.float32:
        return out.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(np.rint(255.0 * out), 0.0), 255.0).astype(np.uint8)


def _taps(X, Y, H, W):
    """the four taps of the reference's bilinear rule at (X, Y) (points of the image) in (m, n) order: [(rows, cols,
    weights)] -- truncation toward zero, fraction clamped to [0, 1], neighbours clamped into the image"""
    xx, yy = X.astype(np.int64), Y.astype(np.int64)
    dx, dy = X - xx, Y - yy
    dx = np.where(dx > 1, 1.0, dx)
    dx = np.where(dx < 0, 0.0, dx)
    dy = np.where(dy > 1, 1.0, dy)
    dy = np.where(dy < 0, 0.0, dy)
    out = []
    for m in (0, 1):
        for n in (0, 1):
            out.append((np.clip(yy + n, 0, H - 1), np.clip(xx + m, 0, W - 1),
                        np.abs(float(1 - m) - dx) * np.abs(float(1 - n) - dy)))
    return out


def sample_plane(img, taps):
    """one plane img (H, W) sampled at the taps, accumulated from 0 in (m, n) order (the video references' sampler)"""
    g = np.zeros(taps[0][0].shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, cols, w in taps:
            g = g + img[rows, cols] * w
    return g


def _sample(img, pb, taps):
    """img (B, H, W) sampled at the taps, accumulated from 0 in (m, n) order"""
    g = np.zeros(taps[0][0].shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, cols, w in taps:
            g = g + img[pb, rows, cols] * w
    return g


def interp_reference(im1, im2, flow_fw, flow_bw, times, occlusion=None, out_dtype=np.float64):
    """im1, im2 (B, H, W, C) uint8 / float32 / float64; flow_fw, flow_bw (B, 2, H, W) (vx, vy); occlusion None or
    (B, 2, H, W) (nonzero = occluded; channel 0 pixels of im1, 1 of im2); times: sequence of t in (0, 1) ->
    (B, K, H, W, C) of out_dtype"""
    I0, I1 = as_f64(im1), as_f64(im2)
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    B, H, W, C = I0.shape
    occ = None if occlusion is None else (np.asarray(occlusion) != 0).astype(np.float64)
    pb = np.arange(B)[:, None, None]
    x = np.arange(W, dtype=np.float64)[None, None, :]
    r = np.arange(H, dtype=np.float64)[None, :, None]
    u, v, bu, bv = fw[:, 0], fw[:, 1], bw[:, 0], bw[:, 1]
    out = np.empty((B, len(times), H, W, C))
    for j, t in enumerate(times):
        t = float(t)
        s = 1.0 - t
        tt, st, ss = t * t, s * t, s * s
        with np.errstate(invalid="ignore", over="ignore"):
            a0, b0 = tt * bu - st * u, tt * bv - st * v
            a1, b1 = ss * u - st * bu, ss * v - st * bv
            X0, Y0, X1, Y1 = x + a0, r + b0, x + a1, r + b1
            in0 = (X0 >= 0) & (X0 <= W - 1) & (Y0 >= 0) & (Y0 <= H - 1)
            in1 = (X1 >= 0) & (X1 <= W - 1) & (Y1 >= 0) & (Y1 <= H - 1)
        k0 = _taps(np.where(in0, X0, 0.0), np.where(in0, Y0, 0.0), H, W)
        k1 = _taps(np.where(in1, X1, 0.0), np.where(in1, Y1, 0.0), H, W)
        both = in0 & in1
        o0 = np.zeros((B, H, W))
        o1 = np.zeros((B, H, W))
        if occ is not None:
            o0 = np.where(both, _sample(occ[:, 0], pb, k0), 0.0)
            o1 = np.where(both, _sample(occ[:, 1], pb, k1), 0.0)
        w0 = np.where(in0, s * (1.0 - o1), 0.0)
        w1 = np.where(in1, t * (1.0 - o0), 0.0)
        weighted = w0 + w1 > 0
        c0, c1 = np.where(weighted, w0, s), np.where(weighted, w1, t)
        den = np.where(weighted, w0 + w1, np.where(in0, s, 0.0) + np.where(in1, t, 0.0))
        for ch in range(C):
            g0 = _sample(I0[..., ch], pb, k0)
            g1 = _sample(I1[..., ch], pb, k1)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                num = np.where(both, c0 * g0 + c1 * g1, np.where(in0, c0 * g0, c1 * g1))
                val = np.where(in0 | in1, num / np.where(in0 | in1, den, 1.0), s * I0[..., ch] + t * I1[..., ch])
            out[:, j, :, :, ch] = val
    return convert(out, out_dtype)
