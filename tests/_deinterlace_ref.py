"""The deinterlacer of include/papof.h (papof_deinterlace_tensor) restated in numpy fp64, written from the header's text, for
both modes and both outputs -- the rule that tests/test_deinterlace_cpu.py checks with known answers and
tests/test_gpu_deinterlace.py compares the device's video and confidence with, byte for byte.  The bilinear taps and the
stores are _interp_ref's.  numpy does not contract a * b + c and divides with correct rounding: the bits are the kernel's."""
import numpy as np

from _interp_ref import _taps, as_f64, convert, sample_plane


def split_reference(frames, top_first=True):
    """woven frames (N, H, W, C), H even -> (fields (2 N, H / 2, W, C), first): frame n gives fields 2 n and 2 n + 1, the
    top field (even rows) before the bottom one when top_first"""
    frames = np.asarray(frames)
    N, H, W, C = frames.shape
    assert H % 2 == 0
    first = 0 if top_first else 1
    out = np.empty((2 * N, H // 2, W, C), frames.dtype)
    out[0::2] = frames[:, first::2]
    out[1::2] = frames[:, 1 - first::2]
    return out, first


def fields_of(video, first=0):
    """field k of a progressive video (T, H, W, C): the rows of parity (k + first) & 1 of frame k"""
    video = np.asarray(video)
    return np.stack([video[k, (k + first) & 1::2] for k in range(len(video))])


def _phase(inside, Y):
    with np.errstate(invalid="ignore"):
        return np.where(inside, 1.0 - 2.0 * np.abs(Y - np.rint(Y)), 0.0)


def _inside(X, Y, Hf, W):
    with np.errstate(invalid="ignore"):
        return (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= Hf - 1)


def deinterlace_reference(fields, flow_fw=None, flow_bw=None, first=0, mode=1, sigma=0.05, out_dtype=None,
                          conf_dtype=np.float64, parts=False):
    """fields (T, Hf, W, C) uint8 / float32 / float64, T >= 4; flow_fw, flow_bw (T - 2, 2, Hf, W) (vx, vy) in field
    coordinates (mode 0: unused) -> (video (T, 2 Hf, W, C) of out_dtype -- None: the fields' --, confidence (T, Hf, W) of
    conf_dtype); parts: also (c0, c1 (T, Hf, W))"""
    fields = np.asarray(fields)
    F = as_f64(fields)
    T, Hf, W, C = F.shape
    assert T >= 4 and first in (0, 1) and mode in (0, 1)
    s2 = float(sigma) * float(sigma)
    x = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (Hf, W))
    jj = np.broadcast_to(np.arange(Hf, dtype=np.float64)[:, None], (Hf, W))
    rows = np.arange(Hf)
    video = np.empty((T, 2 * Hf, W, C))
    conf = np.zeros((T, Hf, W))
    C0, C1 = np.zeros((T, Hf, W)), np.zeros((T, Hf, W))
    if mode:
        fw, bw = np.asarray(flow_fw, np.float64), np.asarray(flow_bw, np.float64)
        assert fw.shape == bw.shape == (T - 2, 2, Hf, W)
    for t in range(T):
        p = (t + first) & 1
        pm = 1 - p
        cl = lambda r: np.clip(r, 0, Hf - 1)  # noqa: E731
        a1, b1 = F[t][cl(rows - 1 + pm)], F[t][cl(rows + pm)]
        a3, b3 = F[t][cl(rows - 2 + pm)], F[t][cl(rows + 1 + pm)]
        with np.errstate(invalid="ignore", over="ignore"):
            s = (9.0 * (a1 + b1) - (a3 + b3)) * 0.0625
        out = s
        if mode:
            in0 = in1 = np.zeros((Hf, W), bool)
            X0 = Y0 = X1 = Y1 = np.zeros((Hf, W))
            with np.errstate(invalid="ignore", over="ignore"):
                if 1 <= t <= T - 2:
                    u, v, bu, bv = fw[t - 1, 0], fw[t - 1, 1], bw[t - 1, 0], bw[t - 1, 1]
                    X0, Y0 = x + (0.25 * bu - 0.25 * u), jj + (0.25 * bv - 0.25 * v)
                    X1, Y1 = x + (0.25 * u - 0.25 * bu), jj + (0.25 * v - 0.25 * bv)
                    in0, in1 = _inside(X0, Y0, Hf, W), _inside(X1, Y1, Hf, W)
                elif t == 0:
                    X1, Y1 = x + 0.5 * fw[1, 0], jj + 0.5 * fw[1, 1]
                    in1 = _inside(X1, Y1, Hf, W)
                else:
                    X0, Y0 = x + 0.5 * bw[T - 4, 0], jj + 0.5 * bw[T - 4, 1]
                    in0 = _inside(X0, Y0, Hf, W)
            c0, c1 = _phase(in0, Y0), _phase(in1, Y1)
            use0, use1 = c0 > 0, c1 > 0
            both = use0 & use1
            k0 = _taps(np.where(in0, X0, 0.0), np.where(in0, Y0, 0.0), Hf, W)
            k1 = _taps(np.where(in1, X1, 0.0), np.where(in1, Y1, 0.0), Hf, W)
            g0 = np.zeros((Hf, W, C))
            g1 = np.zeros((Hf, W, C))
            if t >= 1:
                g0 = np.stack([np.where(use0, sample_plane(F[t - 1][..., k], k0), 0.0) for k in range(C)], -1)
            if t <= T - 2:
                g1 = np.stack([np.where(use1, sample_plane(F[t + 1][..., k], k1), 0.0) for k in range(C)], -1)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                D = np.zeros((Hf, W))
                for k in range(C):
                    d = g0[..., k] - g1[..., k]
                    D = D + d * d
                q2 = np.where(c1 > c0, c1, c0) / (1.0 + (D / float(C)) / s2)
                q = np.where(both, q2, np.where(use0, 0.5 * c0, np.where(use1, 0.5 * c1, 0.0)))
                den = np.where(both, c0 + c1, 1.0)
                m = np.where(both[..., None], (c0[..., None] * g0 + c1[..., None] * g1) / den[..., None],
                             np.where(use0[..., None], g0, g1))
                blend = (1.0 - q[..., None]) * s + q[..., None] * m
            out = np.where((q != 0)[..., None], blend, s)
            conf[t], C0[t], C1[t] = q, c0, c1
        video[t, p::2] = F[t]
        video[t, pm::2] = out
    res = (convert(video, fields.dtype if out_dtype is None else out_dtype), conf.astype(conf_dtype))
    return res + (C0, C1) if parts else res
