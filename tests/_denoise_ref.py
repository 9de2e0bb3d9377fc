"""The temporal filter of include/papof.h (papof_temporal_filter_tensor) restated in numpy fp64 -- the rule that
tests/test_denoise_cpu.py checks with known answers and tests/test_gpu_denoise.py compares the device's output with, byte
for byte.  The hop is test_track_cpu's (_step: k_track's step), the frame sampler _interp_ref's (_taps).  numpy does not
contract a * b + c and divides with correct rounding: the bits are the kernel's."""
import numpy as np

from _interp_ref import _taps, as_f64, convert, sample_plane
from test_track_cpu import _step


def denoise_reference(frames, flow_fw, flow_bw, radius, sigma=None, consistency=(0.01, 0.5), out_dtype=np.float64):
    """frames (T, H, W, C) uint8 / float32 / float64; flow_fw, flow_bw (T - 1, 2, H, W) (vx, vy); sigma None or 0: no
    photometric weight; consistency (alpha1, alpha2) or None: no check -> (out (T, H, W, C) of out_dtype, support (T, H, W)
    uint8)"""
    F = as_f64(frames)
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    T, H, W, C = F.shape
    check = consistency is not None
    a1, a2 = (float(consistency[0]), float(consistency[1])) if check else (0.0, 0.0)
    weighted = sigma is not None and sigma > 0
    s2 = float(sigma) * float(sigma) if weighted else 0.0
    n = np.arange(H * W)
    x0, y0 = (n % W).astype(np.float64), (n // W).astype(np.float64)
    out = np.empty((T, H * W, C))
    support = np.zeros((T, H * W), np.uint8)
    for t in range(T):
        c = F[t].reshape(-1, C)
        num, den, sup = c.copy(), np.ones(H * W), np.zeros(H * W, np.int64)
        for d in (1, -1):
            X, Y, alive = x0.copy(), y0.copy(), np.ones(H * W, bool)
            steps = min(radius, T - 1 - t) if d > 0 else min(radius, t)
            for j in range(1, steps + 1):
                pair = t + j - 1 if d > 0 else t - j
                f, b = (fw[pair], bw[pair]) if d > 0 else (bw[pair], fw[pair])
                X, Y, alive = _step(f, b, X, Y, alive, check, a1, a2)
                taps = _taps(np.where(alive, X, 0.0), np.where(alive, Y, 0.0), H, W)
                g = [sample_plane(F[t + d * j][..., k], taps) for k in range(C)]
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    D = np.zeros(H * W)
                    for k in range(C):
                        dk = g[k] - c[:, k]
                        D = D + dk * dk
                    D = D / C
                    w = 1.0 / (1.0 + D / s2) if weighted else np.ones(H * W)
                    enter = alive & (w > 0)
                    for k in range(C):
                        num[:, k] = np.where(enter, num[:, k] + w * g[k], num[:, k])
                    den = np.where(enter, den + w, den)
                sup = sup + enter
        with np.errstate(invalid="ignore", over="ignore"):
            out[t] = num / den[:, None]
        support[t] = sup
    return convert(out.reshape(T, H, W, C), out_dtype), support.reshape(T, H, W)
