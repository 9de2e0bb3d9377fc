"""Video mosaics of include/papof.h (papof_mosaic_tensor) and of papteam_opticalflow_amd/tensors.py (mosaic_transforms,
neighbour_transforms) restated in numpy fp64 -- the rules that tests/test_mosaic_cpu.py checks with known answers and
tests/test_gpu_mosaic.py compares the device's output with, byte for byte.  numpy does not contract a * b + c, divides with
correct rounding, and its stable sorts order floats as the rule does (a < b, or b NaN and a not): the bits are the kernel's.
The sampler is tests/_interp_ref.py's.  Also the two scenes both test files use, cut from the committed 960 x 540 frame."""
import math

import numpy as np

from _interp_ref import _sample, _taps, as_f64, convert

MODES = ("first", "mean", "median")


def mosaic_reference(frames, sources, matrices, size, mode, masks=None, out_dtype=np.float64, pixels=None):
    """frames (T, H, W, C) uint8 / float32 / float64; sources None (source k is frame k) or integers (n_out, N); matrices
    (n_out, N, 2, 3); size (Hc, Wc); mode "first" / "mean" / "median"; masks None or (T, H, W) (nonzero: left out) ->
    (out (n_out, Hc, Wc, C) of out_dtype, count (n_out, Hc, Wc) uint8).  pixels: None, or integers (P, 3) of rows (o, r, x):
    only those pixels, -> (out (P, C), count (P,))"""
    assert mode in MODES
    I = as_f64(frames)
    M = np.asarray(matrices)
    assert M.dtype in (np.float32, np.float64)
    M = M.astype(np.float64)
    T, H, W, C = I.shape
    n_out, N = M.shape[:2]
    Hc, Wc = size
    src = np.tile(np.arange(T), (n_out, 1)) if sources is None else np.asarray(sources).astype(np.int64)
    assert src.shape == (n_out, N) and src.max() < T
    if pixels is None:
        o, r, x = (a.reshape(-1) for a in np.mgrid[0:n_out, 0:Hc, 0:Wc])
    else:
        o, r, x = (np.asarray(pixels)[:, i].astype(np.int64) for i in range(3))
    P = o.size
    xd, rd = x.astype(np.float64), r.astype(np.float64)
    mk = None if masks is None else np.asarray(masks) != 0
    S = np.zeros((N, C, P))
    live = np.zeros((N, P), bool)
    for k in range(N):
        s = src[o, k]
        m = M[o, k]
        with np.errstate(invalid="ignore", over="ignore"):
            X = (m[:, 0, 0] * xd + m[:, 0, 1] * rd) + m[:, 0, 2]
            Y = (m[:, 1, 0] * xd + m[:, 1, 1] * rd) + m[:, 1, 2]
            ok = (s >= 0) & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        sc = np.maximum(s, 0)
        taps = _taps(np.where(ok, X, 0.0), np.where(ok, Y, 0.0), H, W)
        if mk is not None:
            for rows, cols, w in taps:
                ok &= ~((w > 0) & mk[sc, rows, cols])
        live[k] = ok
        for ch in range(C):
            S[k, ch] = _sample(I[..., ch], sc, taps)
    n = live.sum(0)
    out = np.zeros((P, C))
    if mode == "first":
        k0 = np.argmax(live, 0)
        out = np.where((n > 0)[:, None], S[k0, :, np.arange(P)], 0.0)
    elif mode == "mean":
        acc = np.zeros((C, P))
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(N):
                acc = np.where(live[k], acc + S[k], acc)
            out = np.where(n > 0, acc / np.maximum(n, 1).astype(np.float64), 0.0).T
    else:
        out = lower_median(S, live).T
    out, cnt = convert(np.ascontiguousarray(out), out_dtype), n.astype(np.uint8)
    if pixels is None:
        return out.reshape(n_out, Hc, Wc, C), cnt.reshape(n_out, Hc, Wc)
    return out, cnt


def lower_median(S, live):
    """S (N, C, P) samples in k order, live (N, P): per channel and pixel the element at index (n - 1) // 2 of the live
    samples ordered by (value, k) -- a before b when a < b, or a is a number and b NaN; equal samples (-0.0 and +0.0
    included) and NaNs among themselves by k --, its bits as they are; 0.0 where n = 0 -> (C, P)"""
    N, C, P = S.shape
    n = live.sum(0)
    dead = np.broadcast_to(~live[:, None, :], S.shape)
    order = np.lexsort((S, dead), axis=0)  # stable: by liveness, then value (NaN last), then k
    pick = np.take_along_axis(order, np.broadcast_to(((np.maximum(n, 1) - 1) // 2)[None, None, :], (1, C, P)), 0)
    return np.where(n > 0, np.take_along_axis(S, pick, 0)[0], 0.0)


def _h(m):
    return np.vstack([np.asarray(m, np.float64), [0.0, 0.0, 1.0]])


def _between(A, s, t):
    """frame s's coordinates to frame t's along the pair motions A (T - 1, 2, 3): the product of the pairs in between, or
    the inverse of the way back"""
    if s <= t:
        m = np.eye(3)
        for i in range(s, t):
            m = _h(A[i]) @ m
        return m
    return np.linalg.inv(_between(A, t, s))


def canvas_reference(A, size, ref=None, margin=0):
    """tensors.mosaic_transforms for pair motions A (T - 1, 2, 3) and frames of size (H, W): (matrices (T, 2, 3), (Hc, Wc),
    (x0, y0))"""
    A = np.asarray(A, np.float64)
    T = A.shape[0] + 1
    H, W = size
    ref = (T - 1) // 2 if ref is None else ref
    xs, ys = [], []
    for t in range(T):
        m = _between(A, t, ref)
        for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            p = m @ np.array([cx, cy, 1.0])
            xs.append(p[0])
            ys.append(p[1])
    x0, y0 = math.floor(min(xs)) - margin, math.floor(min(ys)) - margin
    Wc, Hc = math.ceil(max(xs)) + margin - x0 + 1, math.ceil(max(ys)) + margin - y0 + 1
    sh = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])
    return np.array([(_between(A, ref, t) @ sh)[:2] for t in range(T)]), (Hc, Wc), (x0, y0)


def neighbour_reference(M, A, radius):
    """tensors.neighbour_transforms: (sources (T, 2 radius + 1), matrices (T, 2 radius + 1, 2, 3))"""
    M, A = np.asarray(M, np.float64), np.asarray(A, np.float64)
    T = A.shape[0] + 1
    N = 2 * radius + 1
    src = np.full((T, N), -1, np.int64)
    mats = np.tile(np.eye(2, 3), (T, N, 1, 1))
    for t in range(T):
        slots = [(0, t)] + [(2 * d - 1 + e, t + (2 * e - 1) * d) for d in range(1, radius + 1) for e in (0, 1)]
        for slot, s in slots:
            if 0 <= s < T:
                src[t, slot] = s
                mats[t, slot] = (_between(A, t, s) @ _h(M[t]))[:2]
    return src, mats


# ---- the scenes
def _camera(tx, ty, angle, zoom, H, W):
    """frame pixel -> world: a similarity about the frame's centre, then the shift (tx, ty)"""
    a, b = zoom * math.cos(angle), zoom * math.sin(angle)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([[a, -b, cx - a * cx + b * cy + tx], [b, a, cy - b * cx - a * cy + ty], [0.0, 0.0, 1.0]])


def sample_world(world, K, H, W):
    """the world (h, w, C) float64 read bilinearly at K (x, y, 1) for the H x W pixels of a frame: (H, W, C); every point
    must lie in the world"""
    h, w, C = world.shape
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y = K[0, 0] * x + K[0, 1] * r + K[0, 2], K[1, 0] * x + K[1, 1] * r + K[1, 2]
    assert X.min() >= 0 and X.max() <= w - 1 and Y.min() >= 0 and Y.max() <= h - 1
    k = _taps(X[None], Y[None], h, w)
    pb = np.zeros((1, 1, 1), np.int64)
    return np.stack([_sample(world[None, :, :, ch], pb, k)[0] for ch in range(C)], -1)


def _world():
    import cases
    return as_f64(cases.load_frame_u8("960", 1))


def _pairs(Ks):
    """the exact pair motions of cameras Ks: frame t's coordinates to frame t + 1's"""
    return np.array([(np.linalg.inv(Ks[t + 1]) @ Ks[t])[:2] for t in range(len(Ks) - 1)])


def clean_plate_scene(T=9, H=96, W=160):
    """T frames of H x W panning over the committed 960 x 540 frame by (17.5, 6.25) pixels per frame with 0.01 rad and
    0.4 % zoom steps, a 24 x 24 saturated square moving by (-9, 5) per frame in frame coordinates on top: (frames (T, H, W,
    3) uint8, cameras (T, 3, 3), exact pair motions (T - 1, 2, 3), the world (540, 960, 3) float64)"""
    world = _world()
    Ks = np.array([_camera(300.0 + 17.5 * t, 180.0 + 6.25 * t, 0.01 * t, 1.004 ** t, H, W) for t in range(T)])
    frames = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        f = sample_world(world, Ks[t], H, W)
        x, y = 104 - 9 * t, 16 + 5 * t
        f[y:y + 24, x:x + 24] = (1.0, 0.0, 1.0)
        frames[t] = np.clip(np.rint(255 * f), 0, 255).astype(np.uint8)
    return frames, Ks, _pairs(Ks), world


def shaky_scene(T=9, H=96, W=160, seed=31):
    """T frames under a pan of (3, 1) pixels per frame plus Gaussian shake of 5 px and 0.02 rad: (frames uint8, cameras,
    exact pair motions, world)"""
    world = _world()
    rng = np.random.default_rng(seed)
    Ks = np.array([_camera(400.0 + 3.0 * t + rng.normal(0, 5), 220.0 + 1.0 * t + rng.normal(0, 5), rng.normal(0, 0.02), 1.0,
                           H, W) for t in range(T)])
    frames = np.stack([np.clip(np.rint(255 * sample_world(world, K, H, W)), 0, 255).astype(np.uint8) for K in Ks])
    return frames, Ks, _pairs(Ks), world


def psnr(a, b, where):
    """of two (..., C) images in [0, 1] over the pixels `where`"""
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[where]
    return float(10 * np.log10(1.0 / np.mean(d * d)))


def canvas_truth(world, K_ref, origin, size):
    """the world seen from the canvas of a panorama whose reference camera is K_ref (pixels outside the world: NaN)"""
    Hc, Wc = size
    h, w, C = world.shape
    r, x = np.mgrid[0:Hc, 0:Wc].astype(np.float64)
    xr, yr = x + origin[0], r + origin[1]
    X, Y = K_ref[0, 0] * xr + K_ref[0, 1] * yr + K_ref[0, 2], K_ref[1, 0] * xr + K_ref[1, 1] * yr + K_ref[1, 2]
    ok = (X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)
    k = _taps(np.where(ok, X, 0.0)[None], np.where(ok, Y, 0.0)[None], h, w)
    pb = np.zeros((1, 1, 1), np.int64)
    out = np.stack([_sample(world[None, :, :, ch], pb, k)[0] for ch in range(C)], -1)
    out[~ok] = np.nan
    return out


def first_order(T, ref):
    """the sources of mode "first" that prefer the reference frame, then its neighbours: ref, ref - 1, ref + 1, ..."""
    order = [ref]
    for d in range(1, T):
        order += [s for s in (ref - d, ref + d) if 0 <= s < T]
    return order
