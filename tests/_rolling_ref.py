"""Rolling-shutter rectification of include/papof.h (papof_rs_rectify_tensor, papof_rs_flow_tensor) restated in numpy fp64,
written from the header's text -- the rules that tests/test_rolling_cpu.py checks with known answers and
tests/test_gpu_rolling.py compares the device's output with, byte for byte.  The bilinear taps and the stores are
_interp_ref's.  numpy does not contract a * b + c and divides with correct rounding: the bits are the kernel's."""
import numpy as np

from _interp_ref import _taps, as_f64, convert, sample_plane

BRANCHES = ("s_zero", "tf_fails", "tb_fails", "left", "first", "last", "interior")


def _inside(X, Y, H, W):
    with np.errstate(invalid="ignore"):
        return (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)


class _Rule:
    """the flows as float64 and r, a of the header; `seen` counts the lanes that took each branch"""

    def __init__(self, flow_fw, flow_bw, readout, anchor, iters):
        self.fw, self.bw = np.asarray(flow_fw).astype(np.float64), np.asarray(flow_bw).astype(np.float64)
        assert self.fw.shape == self.bw.shape and self.fw.ndim == 4 and self.fw.shape[1] == 2
        self.T, (self.H, self.W) = self.fw.shape[0] + 1, self.fw.shape[2:]
        assert np.isfinite(readout) and abs(readout) <= 1 and 0 <= anchor <= 1 and 1 <= iters <= 8
        self.r, self.a, self.iters = float(readout) / float(self.H), float(anchor) * float(self.H - 1), int(iters)
        self.seen = dict.fromkeys(BRANCHES, 0)

    def displacement(self, t, X, Y, live):
        """L_t at the points (X, Y), evaluated where `live` (points of the image): (Lx, Ly, alive)"""
        H, W, r = self.H, self.W, self.r
        X, Y = np.where(live, X, 0.0), np.where(live, Y, 0.0)
        s = (self.a - Y) * r
        zero = s == 0
        k = _taps(X, Y, H, W)
        z = np.zeros(X.shape)
        Fu, Fv = (sample_plane(self.fw[t, 0], k), sample_plane(self.fw[t, 1], k)) if t < self.T - 1 else (z, z)
        Bu, Bv = (sample_plane(self.bw[t - 1, 0], k), sample_plane(self.bw[t - 1, 1], k)) if t > 0 else (z, z)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            tf, tb = 1.0 + r * Fv, r * Bv - 1.0
            okf, okb = tf >= 0.5, tb <= -0.5
            if t == 0:
                ok = okf
                cF = s / tf
                Lx, Ly = cF * Fu, cF * Fv
            elif t == self.T - 1:
                ok = okb
                cB = s / tb
                Lx, Ly = cB * Bu, cB * Bv
            else:
                ok = okf & okb
                cF = (s * (s - tb)) / (tf * (tf - tb))
                cB = (s * (s - tf)) / (tb * (tb - tf))
                Lx, Ly = cF * Fu + cB * Bu, cF * Fv + cB * Bv
        run = live & ~zero
        self.seen["s_zero"] += int((live & zero).sum())
        self.seen["first" if t == 0 else "last" if t == self.T - 1 else "interior"] += int((run & ok).sum())
        if t < self.T - 1:
            self.seen["tf_fails"] += int((run & ~okf).sum())
        if t > 0:
            self.seen["tb_fails"] += int((run & ~okb).sum())
        return np.where(zero, 0.0, Lx), np.where(zero, 0.0, Ly), live & (zero | ok)

    def solve(self, t, Qx, Qy):
        """(Px, Py, alive) of the solve for the points Q in frame t; P is meaningless where not alive"""
        alive = _inside(Qx, Qy, self.H, self.W)
        Px, Py = Qx, Qy
        for _ in range(self.iters):
            Lx, Ly, alive = self.displacement(t, Px, Py, alive)
            with np.errstate(invalid="ignore", over="ignore"):
                Px, Py = Qx - Lx, Qy - Ly
            inside = _inside(Px, Py, self.H, self.W)
            self.seen["left"] += int((alive & ~inside).sum())
            alive = alive & inside
        return Px, Py, alive


def rectify_reference(frames, flow_fw, flow_bw, readout, anchor=0.5, iters=3, matrices=None, out_dtype=None, parts=False):
    """frames (T, H, W, C) uint8 / float32 / float64, T >= 2; flow_fw, flow_bw (T - 1, 2, H, W) (vx, vy); matrices None or
    (T, 2, 3) -> (video (T, H, W, C) of out_dtype -- None: the frames' --, valid (T, H, W) bool); parts: also P_iters
    (T, H, W, 2) (x, y), NaN where not valid, and the counts of the branches taken (BRANCHES)"""
    frames = np.asarray(frames)
    I = as_f64(frames)
    T, H, W, C = I.shape
    g = _Rule(flow_fw, flow_bw, readout, anchor, iters)
    assert (g.T, g.H, g.W) == (T, H, W) and T >= 2
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((T, H, W, C))
    valid = np.zeros((T, H, W), bool)
    P = np.full((T, H, W, 2), np.nan)
    for t in range(T):
        Qx, Qy = x, r
        if matrices is not None:
            m = np.asarray(matrices[t]).astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                Qx = (m[0, 0] * x + m[0, 1] * r) + m[0, 2]
                Qy = (m[1, 0] * x + m[1, 1] * r) + m[1, 2]
        Px, Py, alive = g.solve(t, Qx, Qy)
        k = _taps(np.where(alive, Px, 0.0), np.where(alive, Py, 0.0), H, W)
        for ch in range(C):
            out[t, :, :, ch] = np.where(alive, sample_plane(I[t, :, :, ch], k), 0.0)
        valid[t] = alive
        P[t, ..., 0], P[t, ..., 1] = np.where(alive, Px, np.nan), np.where(alive, Py, np.nan)
    res = (convert(out, frames.dtype if out_dtype is None else out_dtype), valid)
    return res + (P, g.seen) if parts else res


def flows_reference(flow_fw, flow_bw, readout, anchor=0.5, iters=3, out_dtype=np.float64, parts=False):
    """flow_fw, flow_bw (T - 1, 2, H, W) -> the rectified video's (flow_fw, flow_bw) of out_dtype, NaN where dead; parts: also
    the counts of the branches taken"""
    g = _Rule(flow_fw, flow_bw, readout, anchor, iters)
    H, W = g.H, g.W
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    outs = []
    for f, back in ((g.fw, False), (g.bw, True)):
        o = np.full(f.shape, np.nan)
        for i in range(g.T - 1):
            t, t2 = (i + 1, i) if back else (i, i + 1)
            Px, Py, alive = g.solve(t, x, r)
            k = _taps(np.where(alive, Px, 0.0), np.where(alive, Py, 0.0), H, W)
            Fu, Fv = sample_plane(f[i, 0], k), sample_plane(f[i, 1], k)
            with np.errstate(invalid="ignore", over="ignore"):
                X2, Y2 = Px + Fu, Py + Fv
            alive = alive & _inside(X2, Y2, H, W)
            Lx, Ly, alive = g.displacement(t2, X2, Y2, alive)
            with np.errstate(invalid="ignore", over="ignore"):
                u, v = ((Px - x) + Fu) + Lx, ((Py - r) + Fv) + Ly
            dead = ~alive
            o[i, 0], o[i, 1] = np.where(dead | np.isnan(u), np.nan, u), np.where(dead | np.isnan(v), np.nan, v)
        outs.append(o.astype(out_dtype))
    return tuple(outs) + (g.seen,) if parts else tuple(outs)
