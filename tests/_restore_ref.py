"""The defect detector and the mask dilation of include/papof.h (papof_defect_detect_tensor, papof_mask_dilate_tensor) and
the passes that tensors.repair_defects and tensors.restore_video make of them, restated in numpy fp64 -- the rules that
tests/test_restore_cpu.py checks with known answers and tests/test_gpu_restore.py compares the device's outputs with, byte
for byte.  The hop is test_track_cpu's (_step: k_track's step), the bilinear taps _interp_ref's (_taps), the fill and the
propagation _inpaint_ref's.  numpy does not contract a * b + c: the bits are the kernel's."""
import numpy as np

from _inpaint_ref import fill_reference, propagate_reference
from _interp_ref import _taps, as_f64, sample_plane
from test_track_cpu import _step


def offsets(t, T):
    """(o1, o2): the references of frame t are the frames t + o1 and t + o2"""
    return (1, 2) if t == 0 else ((-1, -2) if t == T - 1 else (-1, 1))


def detect_reference(frames, flow_fw, flow_bw, threshold, consistency=None, score_dtype=np.float64):
    """frames (T, H, W, C) uint8 / float32 / float64, T >= 3; flow_fw, flow_bw (T - 1, 2, H, W) (vx, vy); consistency
    (alpha1, alpha2) or None: no check -> (mask (T, H, W) uint8 of 0 / 1, score (T, H, W) of score_dtype, support (T, H, W)
    uint8)"""
    F = as_f64(frames)
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    T, H, W, C = F.shape
    check = consistency is not None
    a1, a2 = (float(consistency[0]), float(consistency[1])) if check else (0.0, 0.0)
    n = np.arange(H * W)
    x0, y0 = (n % W).astype(np.float64), (n // W).astype(np.float64)

    def hop(frm, d, X, Y, alive):
        """frame frm -> frm + d: forward through flow_fw[frm] checked with flow_bw[frm], backward the other way round"""
        f, b = (fw[frm], bw[frm]) if d > 0 else (bw[frm - 1], fw[frm - 1])
        return _step(f, b, X, Y, alive, check, a1, a2)

    mask = np.zeros((T, H * W), np.uint8)
    score = np.zeros((T, H * W))
    support = np.zeros((T, H * W), np.uint8)
    everyone = np.ones(H * W, bool)
    for t in range(T):
        o1, o2 = offsets(t, T)
        X1, Y1, alive1 = hop(t, o1, x0, y0, everyone)
        if o1 * o2 < 0:
            X2, Y2, alive2 = hop(t, o2, x0, y0, everyone)
        else:  # one chain of two hops: dead after the first, it stays dead
            X2, Y2, alive2 = hop(t + o1, o1, X1, Y1, alive1)
        both = alive1 & alive2
        t1 = _taps(np.where(both, X1, 0.0), np.where(both, Y1, 0.0), H, W)
        t2 = _taps(np.where(both, X2, 0.0), np.where(both, Y2, 0.0), H, W)
        c = F[t].reshape(-1, C)
        s = np.zeros(H * W)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(C):
                g1, g2 = sample_plane(F[t + o1][..., k], t1), sample_plane(F[t + o2][..., k], t2)
                lo, hi = np.where(g2 < g1, g2, g1), np.where(g2 > g1, g2, g1)
                a, b = c[:, k] - hi, lo - c[:, k]
                d = np.where(b > a, b, a)
                s = np.where(d > s, d, s)
            s = np.where(both, s, 0.0)
            mask[t] = both & (s > threshold)
        score[t] = s
        support[t] = alive1.astype(np.uint8) + alive2
    return mask.reshape(T, H, W), score.reshape(T, H, W).astype(score_dtype), support.reshape(T, H, W)


def dilate_reference(mask, radius):
    """mask (T, H, W), nonzero set -> uint8 (T, H, W) of 0 / 1: set where any element of the (2 radius + 1)^2 window,
    clipped to the image, is set"""
    m = np.asarray(mask) != 0
    T, H, W = m.shape
    p = np.zeros((T, H + 2 * radius, W + 2 * radius), bool)
    p[:, radius:radius + H, radius:radius + W] = m
    rows = np.zeros((T, H + 2 * radius, W), bool)
    for k in range(2 * radius + 1):
        rows |= p[:, :, k:k + W]
    out = np.zeros((T, H, W), bool)
    for k in range(2 * radius + 1):
        out |= rows[:, k:k + H]
    return out.astype(np.uint8)


def _complete(fw, bw, masks, relax):
    """complete_flows: flow_fw[t] filled under masks[t], flow_bw[t] under masks[t + 1]"""
    cfw = np.moveaxis(fill_reference(np.moveaxis(fw, 1, -1), masks[:-1], relax), -1, 1)
    cbw = np.moveaxis(fill_reference(np.moveaxis(bw, 1, -1), masks[1:], relax), -1, 1)
    return cfw, cbw


def repair_reference(frames, flow_fw, flow_bw, masks=None, threshold=0.08, dilate=2, radius=None, relax=0, consistency=None,
                     out_dtype=None):
    """tensors.repair_defects in numpy: (video (T, H, W, C) of out_dtype -- None: the frames' --, masks (T, H, W) bool: the
    repaired set, detected (T, H, W) bool, status (T, H, W) uint8)"""
    frames = np.asarray(frames)
    fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
    T = len(frames)
    given = np.zeros(frames.shape[:3], bool) if masks is None else np.asarray(masks) != 0
    first = detect_reference(frames, fw, bw, threshold, consistency)[0] != 0
    grown = dilate_reference(first | given, dilate)
    second = detect_reference(frames, *_complete(fw, bw, grown, relax), threshold, consistency)[0] != 0
    detected = first | second
    m = dilate_reference(detected | given, dilate)
    p, st = propagate_reference(frames, m, *_complete(fw, bw, m, relax), T - 1 if radius is None else radius, consistency)
    video = fill_reference(p, st == 2, relax, frames.dtype if out_dtype is None else out_dtype)
    return video, m != 0, detected, st


def restore_reference(frames, flows_of, passes=2, masks=None, **kw):
    """tensors.restore_video in numpy: flows_of(video) -> (flow_fw, flow_bw) stands for flow_video_fb; the passes before the
    last make the frames' dtype.  -> (video, masks, detected of all passes, status, the flows of the last pass)"""
    frames = np.asarray(frames)
    out_dtype = kw.pop("out_dtype", None)
    given = None if masks is None else np.asarray(masks) != 0
    video, detected = frames, None
    for k in range(passes):
        flows = flows_of(video)
        known = given if detected is None else (detected if given is None else detected | given)
        video, m, det, st = repair_reference(frames, *flows, masks=known, out_dtype=out_dtype if k == passes - 1 else None, **kw)
        detected = det if detected is None else detected | det
    return video, m, detected, st, flows
