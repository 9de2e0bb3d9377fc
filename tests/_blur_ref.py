"""The motion blur of include/papof.h (papof_motion_blur_tensor) restated in numpy fp64 -- the rule that
tests/test_blur_cpu.py checks with known answers and tests/test_gpu_blur.py compares the device's output with, byte for
byte.  Every sample is interp_reference's frame (tests/_interp_ref.py) of the pair that holds its time; the sums are
accumulated sample by sample in the table's order, as the kernel rounds them."""
import numpy as np

from _interp_ref import as_f64, convert, interp_reference


def blur_reference(frames, flow_fw, flow_bw, offsets, weights, occlusion=None, out_dtype=np.float64):
    """frames (T, H, W, C) uint8 / float32 / float64, T >= 2; flow_fw, flow_bw (T - 1, 2, H, W): pair i = frames (i, i + 1);
    occlusion None or (T - 1, 2, H, W); offsets, weights: the sample table -> (T, H, W, C) of out_dtype"""
    frames = np.asarray(frames)
    I = as_f64(frames)
    T = I.shape[0]
    acc = np.zeros(I.shape)
    wsum = np.zeros(T)           # the same for every pixel of a frame
    kept = np.zeros(T, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for tau, w in zip(offsets, weights):
            tau, w = float(tau), float(w)
            if w == 0.0:
                continue
            if tau == 0.0:
                fs, S = slice(0, T), I
            else:
                # one call for every pair: pair i at t -- the sample of frame i (tau > 0) or of frame i + 1 (tau < 0)
                t = tau if tau > 0 else 1.0 + tau
                S = interp_reference(frames[:-1], frames[1:], flow_fw, flow_bw, [t], occlusion)[:, 0]
                fs = slice(0, T - 1) if tau > 0 else slice(1, T)
            acc[fs] = acc[fs] + w * S
            wsum[fs] = wsum[fs] + w
            kept[fs] = True
        out = np.where(kept[:, None, None, None], acc / np.where(kept, wsum, 1.0)[:, None, None, None], I)
    return convert(out, out_dtype)
