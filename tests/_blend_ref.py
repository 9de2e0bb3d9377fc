"""Seamless mosaics of include/papof.h (papof_mosaic_blend_tensor, papof_mosaic_overlap_tensor) and exposure_gains of
papteam_opticalflow_amd/tensors.py restated in numpy fp64 -- the rules that tests/test_blend_cpu.py checks with known answers
and tests/test_gpu_blend.py compares the device's output with, byte for byte (the overlap statistics: integer for integer).
Liveness and the sampler are tests/_mosaic_ref.py's and tests/_interp_ref.py's rules, restated here only as far as the points
(X, Y) are needed too.  Also the exposure scene of both test files: tests/_mosaic_ref.py's pan over the committed 960 x 540
frame, every frame under a gain of its own."""
import numpy as np

from _interp_ref import _sample, _taps, as_f64, convert
from _mosaic_ref import _camera, _pairs, _world, lower_median, sample_world

MODES = ("first", "mean", "median", "feather")
ONE = 16777216.0  # 2^24: the fixed point of the overlap statistics


def gather(frames, sources, matrices, size, masks=None, step=1):
    """papof_mosaic_tensor's walk at the canvas pixels with x % step == 0 and r % step == 0: (S (N, C, P) samples, live (N, P),
    X, Y (N, P) the sampled points, o (P,) the output of each pixel), pixels in (o, r, x) order"""
    I = as_f64(frames)
    M = np.asarray(matrices)
    assert M.dtype in (np.float32, np.float64)
    M = M.astype(np.float64)
    T, H, W, C = I.shape
    n_out, N = M.shape[:2]
    Hc, Wc = size
    src = np.tile(np.arange(T), (n_out, 1)) if sources is None else np.asarray(sources).astype(np.int64)
    assert src.shape == (n_out, N) and src.max() < T
    o, r, x = (a.reshape(-1) for a in np.mgrid[0:n_out, 0:Hc:step, 0:Wc:step])
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
            X = (m[:, 0, 0] * xd + m[:, 0, 1] * rd) + m[:, 0, 2]
            Y = (m[:, 1, 0] * xd + m[:, 1, 1] * rd) + m[:, 1, 2]
            ok = (s >= 0) & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        sc = np.maximum(s, 0)
        X, Y = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
        taps = _taps(X, Y, H, W)
        if mk is not None:
            for rows, cols, w in taps:
                ok &= ~((w > 0) & mk[sc, rows, cols])
        live[k], Xs[k], Ys[k] = ok, X, Y
        for ch in range(C):
            S[k, ch] = _sample(I[..., ch], sc, taps)
    return S, live, Xs, Ys, o


def blend_reference(frames, sources, matrices, size, mode, gains=None, masks=None, out_dtype=np.float64):
    """papof_mosaic_blend_tensor: frames (T, H, W, C); gains None or (n_out, N) float32 / float64 -> (out (n_out, Hc, Wc, C)
    of out_dtype, count (n_out, Hc, Wc) uint8)"""
    assert mode in MODES
    S, live, X, Y, o = gather(frames, sources, matrices, size, masks)
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


def overlap_reference(frames, sources, matrices, size, step=2, bound=1.0, masks=None):
    """papof_mosaic_overlap_tensor: (sums, counts) int64 (n_out, N, N)"""
    S, live, _, _, o = gather(frames, sources, matrices, size, masks, step)
    N, C, P = S.shape
    n_out = np.asarray(matrices).shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.zeros((N, P))
        for ch in range(C):
            y = y + S[:, ch]
        y = y / float(C)
        alive = live & ~np.isnan(y)
        t = np.clip(np.where(alive, y, 0.0) / float(bound), 0.0, 1.0)
    q = np.rint(t * ONE).astype(np.int64)
    sums, counts = np.zeros((n_out, N, N), np.int64), np.zeros((n_out, N, N), np.int64)
    for out in range(n_out):
        L = alive[:, o == out].astype(np.int64)
        counts[out] = L @ L.T
        sums[out] = (L * q[:, o == out]) @ L.T
    return sums, counts


def gains_reference(sums, counts, bound=1.0, sigma_n=10.0 / 255.0, sigma_g=0.1, anchor=None):
    """tensors.exposure_gains, the normal equations written out entry by entry: (n_out, N) float64"""
    sums, counts = np.asarray(sums), np.asarray(counts)
    n_out, N = sums.shape[:2]
    g = np.ones((n_out, N))
    for o in range(n_out):
        I = np.zeros((N, N))
        for i in range(N):
            for j in range(N):
                if counts[o, i, j] > 0:
                    I[i, j] = sums[o, i, j] / counts[o, i, j] / ONE * bound
        A, b = np.zeros((N, N)), np.zeros(N)
        for i in range(N):
            n_i = sum(float(counts[o, i, j]) for j in range(N) if j != i)
            if n_i == 0:
                A[i, i], b[i] = 1.0, 1.0
                continue
            for j in range(N):
                if j != i:
                    A[i, i] += 2.0 * counts[o, i, j] * I[i, j] ** 2 / sigma_n ** 2
                    A[i, j] = -2.0 * counts[o, i, j] * I[i, j] * I[j, i] / sigma_n ** 2
            A[i, i] += n_i / sigma_g ** 2
            b[i] = n_i / sigma_g ** 2
        g[o] = np.linalg.solve(A, b)
        if anchor is not None:
            g[o] = g[o] / g[o, anchor]
    return g


def energy(g, sums, counts, bound=1.0, sigma_n=10.0 / 255.0, sigma_g=0.1):
    """what exposure_gains minimises, for one output"""
    N = len(g)
    e = 0.0
    for i in range(N):
        for j in range(N):
            if i != j and counts[i, j] > 0:
                Iij, Iji = sums[i, j] / counts[i, j] / ONE * bound, sums[j, i] / counts[j, i] / ONE * bound
                e += counts[i, j] * ((g[i] * Iij - g[j] * Iji) ** 2 / sigma_n ** 2 + (1 - g[i]) ** 2 / sigma_g ** 2)
    return e


# ---- the scene
def scene_gains(T=9, seed=3):
    """one gain per frame, log-uniform in [0.75, 1]: an auto-exposure that moves by up to a third"""
    return np.exp(np.random.default_rng(seed).uniform(np.log(0.75), 0.0, T))


def exposure_scene(square, true_gains, T=9, H=96, W=160):
    """tests/_mosaic_ref.py: clean_plate_scene -- the pan over the committed 960 x 540 frame, with or without its moving
    square --, frame t multiplied by true_gains[t] before it is quantised: (frames (T, H, W, 3) uint8, cameras, exact pair
    motions, the world)"""
    world = _world()
    Ks = np.array([_camera(300.0 + 17.5 * t, 180.0 + 6.25 * t, 0.01 * t, 1.004 ** t, H, W) for t in range(T)])
    frames = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        f = sample_world(world, Ks[t], H, W)
        if square:
            x, y = 104 - 9 * t, 16 + 5 * t
            f[y:y + 24, x:x + 24] = (1.0, 0.0, 1.0)
        frames[t] = np.clip(np.rint(255 * (true_gains[t] * f)), 0, 255).astype(np.uint8)
    return frames, Ks, _pairs(Ks), world


def scaled_psnr(out, truth, where):
    """PSNR of (..., C) images over the pixels `where` after the one least-squares scale of `out`: gains fix ratios, not the
    level -> (dB, the scale)"""
    a, b = np.asarray(out, np.float64)[where], np.asarray(truth, np.float64)[where]
    s = float((a * b).sum() / (a * a).sum())
    d = s * a - b
    return float(10 * np.log10(1.0 / np.mean(d * d))), s


def seam_step(out, truth, live, where):
    """the mean absolute horizontal difference of the error image (out scaled as scaled_psnr scales it) between neighbours
    x, x + 1 that are both in `where`: (at pairs whose sets of live sources differ, at the others).  out, truth (Hc, Wc, C);
    live (N, Hc, Wc)"""
    _, s = scaled_psnr(out, truth, where)
    e = np.where(where[..., None], s * np.asarray(out, np.float64) - truth, 0.0)
    d = np.abs(e[:, 1:] - e[:, :-1]).mean(-1)
    both = where[:, 1:] & where[:, :-1]
    border = (live[:, :, 1:] != live[:, :, :-1]).any(0)
    return float(d[both & border].mean()), float(d[both & ~border].mean())
