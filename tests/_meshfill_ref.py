"""The mosaic under the mesh rule of include/papof.h (papof_mosaic_mesh_tensor) and neighbour_mesh of
papteam_opticalflow_amd/tensors.py restated in numpy fp64 -- what tests/test_meshfill_cpu.py checks with known answers and
tests/test_gpu_meshfill.py compares the device's output with, byte for byte.  The walk is tests/_mosaic_ref.py's
(mosaic_reference) with tests/_mesh_ref.py's mesh_displacement added to the point; the gains and the four modes behind it are
tests/_blend_ref.py's rules.  numpy does not contract a * b + c: the bits are the kernel's."""
import numpy as np

from _interp_ref import _sample, _taps, as_f64, convert
from _mesh_ref import mesh_displacement
from _mosaic_ref import lower_median

MODES = ("first", "mean", "median", "feather")


def gather_mesh(frames, sources, matrices, mesh, size, masks=None):
    """the walk at every canvas pixel: (S (N, C, P) samples, live (N, P), X, Y (N, P) the moved points -- as they are, also
    where the slot is dead --, o (P,) the output of each pixel), pixels in (o, r, x) order.  mesh (n_out, N, GH + 1, GW + 1, 2)"""
    I = as_f64(frames)
    M = np.asarray(matrices)
    assert M.dtype in (np.float32, np.float64)
    M = M.astype(np.float64)
    D = np.asarray(mesh)
    assert D.dtype == np.float64
    T, H, W, C = I.shape
    n_out, N = M.shape[:2]
    assert D.shape[:2] == (n_out, N) and D.shape[4] == 2
    Hc, Wc = size
    src = np.tile(np.arange(T), (n_out, 1)) if sources is None else np.asarray(sources).astype(np.int64)
    assert src.shape == (n_out, N) and src.max() < T
    o, r, x = (a.reshape(-1) for a in np.mgrid[0:n_out, 0:Hc, 0:Wc])
    P = o.size
    xd, rd = x.astype(np.float64), r.astype(np.float64)
    mk = None if masks is None else np.asarray(masks) != 0
    S = np.zeros((N, C, P))
    live = np.zeros((N, P), bool)
    Xs, Ys = np.zeros((N, P)), np.zeros((N, P))
    for k in range(N):
        s = src[o, k]
        m = M[o, k]
        with np.errstate(invalid="ignore", over="ignore"):
            X0 = (m[:, 0, 0] * xd + m[:, 0, 1] * rd) + m[:, 0, 2]
            Y0 = (m[:, 1, 0] * xd + m[:, 1, 1] * rd) + m[:, 1, 2]
            dx, dy = np.zeros(P), np.zeros(P)
            for out in range(n_out):  # the table of slot (out, k)
                sel = slice(out * Hc * Wc, (out + 1) * Hc * Wc)
                dx[sel], dy[sel] = mesh_displacement(X0[sel], Y0[sel], D[out, k], H, W)
            X, Y = X0 + dx, Y0 + dy
            ok = (s >= 0) & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        Xs[k], Ys[k] = X, Y
        sc = np.maximum(s, 0)
        taps = _taps(np.where(ok, X, 0.0), np.where(ok, Y, 0.0), H, W)
        if mk is not None:
            for rows, cols, w in taps:
                ok &= ~((w > 0) & mk[sc, rows, cols])
        live[k] = ok
        for ch in range(C):
            S[k, ch] = _sample(I[..., ch], sc, taps)
    return S, live, Xs, Ys, o


def mosaic_mesh_reference(frames, sources, matrices, mesh, size, mode, gains=None, masks=None, out_dtype=np.float64):
    """papof_mosaic_mesh_tensor: frames (T, H, W, C); gains None or (n_out, N) float32 / float64 -> (out (n_out, Hc, Wc, C) of
    out_dtype, count (n_out, Hc, Wc) uint8)"""
    assert mode in MODES
    S, live, X, Y, o = gather_mesh(frames, sources, matrices, mesh, size, masks)
    N, C, P = S.shape
    H, W = np.asarray(frames).shape[1:3]
    n_out = np.asarray(matrices).shape[0]
    Hc, Wc = size
    with np.errstate(invalid="ignore", over="ignore"):
        if gains is not None:
            g = np.asarray(gains)
            assert g.dtype in (np.float32, np.float64) and g.shape == (n_out, N)
            V = g.astype(np.float64).T[:, o][:, None, :] * S
        else:
            V = 1.0 * S
        n = live.sum(0)
        if mode == "first":
            k0 = np.argmax(live, 0)
            out = np.where((n > 0)[:, None], V[k0, :, np.arange(P)], 0.0)
        elif mode == "mean":
            acc = np.zeros((C, P))
            for k in range(N):
                acc = np.where(live[k], acc + V[k], acc)
            out = np.where(n > 0, acc / np.maximum(n, 1).astype(np.float64), 0.0).T
        elif mode == "median":
            out = lower_median(V, live).T
        else:
            W1, H1 = float(W - 1), float(H - 1)
            num, den = np.zeros((C, P)), np.zeros(P)
            for k in range(N):
                w = np.minimum(np.minimum(X[k], W1 - X[k]), np.minimum(Y[k], H1 - Y[k])) + 1.0
                num = np.where(live[k], num + w * V[k], num)
                den = np.where(live[k], den + w, den)
            out = np.where(n > 0, num / np.where(n > 0, den, 1.0), 0.0).T
    out = convert(np.ascontiguousarray(out), out_dtype)
    return out.reshape(n_out, Hc, Wc, C), n.astype(np.uint8).reshape(n_out, Hc, Wc)


def neighbour_mesh_reference(residuals, D, fill_radius):
    """tensors.neighbour_mesh from the residuals (T - 1, GH + 1, GW + 1, 2) and mesh_profiles's tables D of them: (T,
    2 fill_radius + 1, GH + 1, GW + 1, 2), slot 0 = D[t], slot 2 d - 1 + e of s = t + (2 e - 1) d: D[t] + (C[s] - C[t])"""
    r = np.asarray(residuals, np.float64)
    C = np.concatenate([np.zeros((1,) + r.shape[1:]), np.cumsum(r, 0)])
    T = C.shape[0]
    E = np.zeros((T, 2 * fill_radius + 1) + C.shape[1:])
    for t in range(T):
        E[t, 0] = D[t]
        for d in range(1, fill_radius + 1):
            for e in (0, 1):
                s = t + (2 * e - 1) * d
                if 0 <= s < T:
                    E[t, 2 * d - 1 + e] = D[t] + (C[s] - C[t])
    return E
