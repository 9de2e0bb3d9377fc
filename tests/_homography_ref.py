"""The homography model of include/papof.h (papof_homography_fit_tensor, papof_warp_projective_tensor,
papof_mosaic_projective_tensor, papof_mosaic_overlap_projective_tensor) restated in numpy fp64 -- the rules that
tests/test_homography_cpu.py checks with known answers and tests/test_gpu_homography.py compares the device's results with.
The fit's sums are added in numpy's order, not the kernel's, so fitted matrices agree to rounding, not bit for bit; the warp,
the mosaic and the overlap statistics are the bits of the kernels (numpy does not contract a * b + c and divides with correct
rounding; the sampler is tests/_interp_ref.py's, the modes are tests/_mosaic_ref.py's and tests/_blend_ref.py's).  Also the
tile culling of mosaic.hip restated, so that the CPU can check it against brute-force liveness, and the rotating-camera
scene of both test files."""
import math

import numpy as np

from _blend_ref import ONE
from _interp_ref import _sample, _taps, as_f64, convert
from _mosaic_ref import _world, lower_median
from _stab_ref import _eliminate

MIN_DEN = 0.0625  # PAPOF_HOMOGRAPHY_MIN_DEN
MODES = ("first", "mean", "median", "feather")


# ---- the fit
def sums_h(flow, mask, m, scale):
    """the twenty-five sums of one pair: flow (2, H, W), mask None or (H, W) (nonzero: left out), m the previous iteration's
    (3, 3) matrix or None (iteration 0)"""
    _, H, W = flow.shape
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(W, H) / 2.0
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = flow[0].astype(np.float64), flow[1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y = x + u, r + v
        valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    if mask is not None:
        valid &= np.asarray(mask) == 0
    n_valid = float(valid.sum())
    x, r, X, Y = x[valid], r[valid], X[valid], Y[valid]
    if m is None:
        w, c = np.ones(x.shape), np.ones(x.shape)
    else:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            d = (m[2, 0] * x + m[2, 1] * r) + m[2, 2]
            dn = d / ((m[2, 0] * cx + m[2, 1] * cy) + m[2, 2])
            keep = dn > MIN_DEN
        x, r, X, Y, d, dn = x[keep], r[keep], X[keep], Y[keep], d[keep], dn[keep]
        ex = X - ((m[0, 0] * x + m[0, 1] * r) + m[0, 2]) / d
        ey = Y - ((m[1, 0] * x + m[1, 1] * r) + m[1, 2]) / d
        e2 = ex * ex + ey * ey
        c = 1.0 / (1.0 + e2 / (scale * scale))
        w = c / (dn * dn)
    xh, yh, Xh, Yh = (x - cx) / s, (r - cy) / s, (X - cx) / s, (Y - cy) / s
    xx, xy, yy, q = xh * xh, xh * yh, yh * yh, Xh * Xh + Yh * Yh
    terms = [xx, xy, yy, xh, yh, np.ones(x.shape), xx * Xh, xy * Xh, yy * Xh, xh * Xh, yh * Xh, Xh, xx * Yh, xy * Yh, yy * Yh,
             xh * Yh, yh * Yh, Yh, xx * q, xy * q, yy * q, xh * q, yh * q]
    return [float(np.sum(w * t)) for t in terms] + [n_valid, float(np.sum(c))]


def solve_h(S, H, W):
    """the pixel-coordinate homography (3, 3) of the twenty-five sums S, or None where the iteration fails"""
    cx, cy, s = (W - 1) / 2.0, (H - 1) / 2.0, max(W, H) / 2.0
    sw = S[5]
    if not sw > 0:
        return None
    g = [[S[0], S[1], S[3], 0.0, 0.0, 0.0, -S[6], -S[7], S[9]],
         [S[1], S[2], S[4], 0.0, 0.0, 0.0, -S[7], -S[8], S[10]],
         [S[3], S[4], S[5], 0.0, 0.0, 0.0, -S[9], -S[10], S[11]],
         [0.0, 0.0, 0.0, S[0], S[1], S[3], -S[12], -S[13], S[15]],
         [0.0, 0.0, 0.0, S[1], S[2], S[4], -S[13], -S[14], S[16]],
         [0.0, 0.0, 0.0, S[3], S[4], S[5], -S[15], -S[16], S[17]],
         [-S[6], -S[7], -S[9], -S[12], -S[13], -S[15], S[18], S[19], -S[21]],
         [-S[7], -S[8], -S[10], -S[13], -S[14], -S[16], S[19], S[20], -S[22]]]
    p = _eliminate(g, 8, 1e-12 * sw)
    if p is None:
        return None
    hn = [p[0][0:3], p[0][3:6], [p[0][6], p[0][7], 1.0]]
    with np.errstate(all="ignore"):
        A = [[hn[i][0], hn[i][1], s * hn[i][2] - (hn[i][0] * cx + hn[i][1] * cy)] for i in range(3)]
        z = A[2][2]
        if not z > 0:
            return None
        m = np.array([[(s * A[0][j] + cx * A[2][j]) / z for j in range(3)],
                      [(s * A[1][j] + cy * A[2][j]) / z for j in range(3)],
                      [A[2][j] / z for j in range(3)]], np.float64)
    if not np.isfinite(m).all():
        return None
    W1, H1 = float(W - 1), float(H - 1)
    front = m[2, 2] > 0 and m[2, 0] * W1 + m[2, 2] > 0 and m[2, 1] * H1 + m[2, 2] > 0 and \
        (m[2, 0] * W1 + m[2, 1] * H1) + m[2, 2] > 0
    return m if front else None


def fit_reference_h(flow, occlusion=None, iters=5, scale=1.0):
    """flow (B, 2, H, W); occlusion None or (B, 2, H, W) (channel 0 read) -> (motion (B, 3, 3), ok (B,) bool, support (B,))"""
    flow = np.asarray(flow)
    B, _, H, W = flow.shape
    motion, ok, support = np.empty((B, 3, 3)), np.zeros(B, bool), np.empty(B)
    for i in range(B):
        mask = None if occlusion is None else np.asarray(occlusion)[i, 0]
        m = None
        for it in range(iters):
            S = sums_h(flow[i], mask, m, scale)
            support[i] = S[24] / (H * W)
            got = solve_h(S, H, W)
            if got is not None:
                m = got
            elif it == 0:
                break
        ok[i] = m is not None
        motion[i] = m if m is not None else np.eye(3)
    return motion, ok, support


def project(m, x, y):
    """a (3, 3) matrix applied to points: (X, Y)"""
    d = m[2, 0] * x + m[2, 1] * y + m[2, 2]
    return (m[0, 0] * x + m[0, 1] * y + m[0, 2]) / d, (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / d


def projective_corner_distance(m1, m2, H, W):
    """the largest distance in pixels between where two matrices, (3, 3) or (2, 3), send the four image corners"""
    full = lambda m: np.vstack([m, [0.0, 0.0, 1.0]]) if np.shape(m) == (2, 3) else np.asarray(m, np.float64)  # noqa: E731
    x, y = np.array([0.0, W - 1, 0.0, W - 1]), np.array([0.0, 0.0, H - 1, H - 1])
    a, b = project(full(m1), x, y), project(full(m2), x, y)
    return float(np.max(np.hypot(a[0] - b[0], a[1] - b[1])))


def homography_flow(m, H, W):
    """the exact flow (2, H, W) of the (3, 3) matrix m: where it sends each pixel, less the pixel"""
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y = project(np.asarray(m, np.float64), x, r)
    return np.stack([X - x, Y - r])


# ---- projective sampling
def _point(m, xd, rd):
    """(X, Y, D > 0) of the projective rule for matrices m (..., 3, 3) broadcast against the pixels"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        D = (m[..., 2, 0] * xd + m[..., 2, 1] * rd) + m[..., 2, 2]
        X = ((m[..., 0, 0] * xd + m[..., 0, 1] * rd) + m[..., 0, 2]) / D
        Y = ((m[..., 1, 0] * xd + m[..., 1, 1] * rd) + m[..., 1, 2]) / D
        return X, Y, D > 0


def warp_reference_h(frames, matrices, out_dtype=np.float64):
    """frames (B, H, W, C) uint8 / float32 / float64, matrices (B, 3, 3) -> (out (B, H, W, C) of out_dtype, valid (B, H, W))"""
    I = as_f64(frames)
    M = np.asarray(matrices).astype(np.float64)
    B, H, W, C = I.shape
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, H, W, C))
    valid = np.zeros((B, H, W), bool)
    for i in range(B):
        X, Y, front = _point(M[i], x, r)
        with np.errstate(invalid="ignore"):
            inside = front & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        k = _taps(np.where(inside, X, 0.0)[None], np.where(inside, Y, 0.0)[None], H, W)
        for ch in range(C):
            out[i, :, :, ch] = np.where(inside, _sample(I[i:i + 1, :, :, ch], np.zeros((1, 1, 1), np.int64), k)[0], 0.0)
        valid[i] = inside
    return convert(out, out_dtype), valid


def gather_h(frames, sources, matrices, size, masks=None, step=1):
    """tests/_blend_ref.py's gather under the projective rule, matrices (n_out, N, 3, 3): (S (N, C, P) samples, live (N, P),
    X, Y (N, P) the sampled points, o (P,) the output of each pixel), pixels in (o, r, x) order"""
    I = as_f64(frames)
    M = np.asarray(matrices)
    assert M.dtype in (np.float32, np.float64) and M.shape[2:] == (3, 3)
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
        X, Y, front = _point(M[o, k], xd, rd)
        with np.errstate(invalid="ignore"):
            ok = (s >= 0) & front & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
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


def mosaic_reference_h(frames, sources, matrices, size, mode, gains=None, masks=None, out_dtype=np.float64):
    """papof_mosaic_projective_tensor: tests/_blend_ref.py's blend_reference over gather_h -> (out (n_out, Hc, Wc, C) of
    out_dtype, count (n_out, Hc, Wc) uint8)"""
    assert mode in MODES
    S, live, X, Y, o = gather_h(frames, sources, matrices, size, masks)
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


def overlap_reference_h(frames, sources, matrices, size, step=2, bound=1.0, masks=None):
    """papof_mosaic_overlap_projective_tensor: (sums, counts) int64 (n_out, N, N)"""
    S, live, _, _, o = gather_h(frames, sources, matrices, size, masks, step)
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


# ---- the tile culling of mosaic.hip (projective_keep)
def cull_keep(m, xa, xb, ra, rb, H, W):
    """False where the rule drops the slot of matrix m (3, 3) from the tile of canvas pixels [xa, xb] x [ra, rb]; frames H x W"""
    m = np.asarray(m).astype(np.float64)
    if not np.isfinite(m[:2]).all():
        return False
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xs, rs = np.array([xa, xb, xa, xb], np.float64), np.array([ra, ra, rb, rb], np.float64)
        D = (m[2, 0] * xs + m[2, 1] * rs) + m[2, 2]
        Nx = (m[0, 0] * xs + m[0, 1] * rs) + m[0, 2]
        Ny = (m[1, 0] * xs + m[1, 1] * rs) + m[1, 2]
        if np.isnan(D).any() or np.isnan(Nx).any() or np.isnan(Ny).any():
            return True
        if not D.max() > 0:
            return False
        if not D.min() > 0:
            return True
        W1, H1 = float(W - 1), float(H - 1)
        missx = (Nx.max() / D.min() < -1.0 and Nx.max() / D.max() < -1.0) or \
            (Nx.min() / D.min() > W1 + 1.0 and Nx.min() / D.max() > W1 + 1.0)
        missy = (Ny.max() / D.min() < -1.0 and Ny.max() / D.max() < -1.0) or \
            (Ny.min() / D.min() > H1 + 1.0 and Ny.min() / D.max() > H1 + 1.0)
    return not missx and not missy


def tile_live(m, xa, xb, ra, rb, H, W):
    """brute force: True where the projective rule makes the slot live (masks aside) at some pixel of the tile"""
    r, x = np.mgrid[int(ra):int(rb) + 1, int(xa):int(xb) + 1].astype(np.float64)
    X, Y, front = _point(np.asarray(m).astype(np.float64), x, r)
    with np.errstate(invalid="ignore"):
        return bool((front & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)).any())


def tiles(Hc, Wc, ty):
    """the 64 x ty tiles of an Hc x Wc canvas as (xa, xb, ra, rb)"""
    return [(x0, min(x0 + 63, Wc - 1), r0, min(r0 + ty - 1, Hc - 1)) for r0 in range(0, Hc, ty) for x0 in range(0, Wc, 64)]


# ---- the rotating camera
def rotating_camera(T=9, H=96, W=160, focal=200.0, yaw_deg=4.0):
    """the exact pair homographies (T - 1, 3, 3) of a camera of focal length `focal` px that yaws by yaw_deg per frame about
    its centre of projection, principal point at the image centre: frame t's pixels to frame t + 1's"""
    K = np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    a = math.radians(yaw_deg)
    R = np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
    G = K @ R @ np.linalg.inv(K)
    return np.array([G / G[2, 2]] * (T - 1))


def chain(A):
    """the product of pair motions, (n, 3, 3) or (n, 2, 3): frame 0's coordinates to frame n's, [2][2] = 1"""
    P = np.eye(3)
    for a in A:
        a = np.vstack([a, [0.0, 0.0, 1.0]]) if np.shape(a) == (2, 3) else np.asarray(a, np.float64)
        P = a @ P
        P = P / P[2, 2]
    return P


def rotating_scene(T=9, H=96, W=160, focal=200.0, yaw_deg=4.0):
    """T frames of H x W cut from the committed 960 x 540 frame by the exact homographies of rotating_camera, the middle
    frame a plain crop about the world's centre: (frames (T, H, W, 3) uint8, frame-to-world matrices (T, 3, 3), exact pair
    homographies, the world (540, 960, 3) float64)"""
    world = _world()
    h, w, _ = world.shape
    A = rotating_camera(T, H, W, focal, yaw_deg)
    ref = (T - 1) // 2
    crop = np.array([[1.0, 0.0, (w - W) // 2], [0.0, 1.0, (h - H) // 2], [0.0, 0.0, 1.0]])
    Ks = [None] * T
    for t in range(T):  # frame t -> the reference frame -> the world
        to_ref = chain(A[t:ref]) if t <= ref else np.linalg.inv(chain(A[ref:t]))
        Ks[t] = crop @ to_ref
        Ks[t] = Ks[t] / Ks[t][2, 2]
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = np.empty((T, H, W, 3), np.uint8)
    pb = np.zeros((1, 1, 1), np.int64)
    for t in range(T):
        X, Y = project(Ks[t], x, r)
        assert X.min() >= 0 and X.max() <= w - 1 and Y.min() >= 0 and Y.max() <= h - 1
        k = _taps(X[None], Y[None], h, w)
        f = np.stack([_sample(world[None, :, :, ch], pb, k)[0] for ch in range(3)], -1)
        frames[t] = np.clip(np.rint(255 * f), 0, 255).astype(np.uint8)
    return frames, np.array(Ks), A, world


# ---- what both test files feed the fit and the culling
def homography_flows(B, H, W, seed, outliers=0.2, noise=0.2):
    """(flows (B, 2, H, W) of random homographies -- last-row terms N(0, 2e-4 * 240 / W) -- plus Gaussian noise and gross
    outliers of +-15 px in vx, the homographies (B, 3, 3))"""
    rng = np.random.default_rng(seed)
    f, Ms = np.empty((B, 2, H, W)), np.empty((B, 3, 3))
    for i in range(B):
        m = np.eye(3)
        m[:2, :2] += rng.normal(0, 0.01, (2, 2))
        m[:2, 2] = rng.normal(0, 2, 2)
        m[2, :2] = rng.normal(0, 2e-4 * 240 / W, 2)
        f[i], Ms[i] = homography_flow(m, H, W), m
    if noise:
        f += rng.normal(0, noise, f.shape)
    bad = rng.random((B, H, W)) < outliers
    f[:, 0][bad] += rng.uniform(-15, 15, int(bad.sum()))
    return f, Ms


def cull_matrices(H, W, Hc, Wc, seed=5):
    """float64 (n, 3, 3) matrices that try the tile culling, for frames H x W on a canvas Hc x Wc: random ones, mild
    perspective, a horizon that crosses the canvas (and so a tile) along x and along r, D <= 0 everywhere, tiny D, and NaN
    and infinite entries in every position"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(12):  # random: shears, shifts of the canvas' size, strong perspective
        m = np.eye(3)
        m[:2, :2] = np.diag([H / Hc, H / Hc]) + rng.normal(0, 0.3, (2, 2))
        m[:2, 2] = rng.normal(0, 40, 2)
        m[2, :2] = rng.normal(0, 4e-3, 2)
        out.append(m)
    for _ in range(12):  # mild perspective around a placement that covers part of the canvas
        m = np.eye(3)
        m[:2, :2] += rng.normal(0, 0.05, (2, 2))
        m[:2, 2] = -rng.uniform(0, [Wc - W, Hc - H])
        m[2, :2] = rng.normal(0, 3e-4, 2)
        out.append(m)
    base = np.array([[1.0, 0.0, -10.0], [0.0, 1.0, -5.0], [0.0, 0.0, 1.0]])
    for row in ([-1.0 / 75.0, 0.0, 1.0], [0.0, -1.0 / 38.5, 1.0], [1.0 / 75.0, 0.0, -1.0], [-1.0 / 90.0, -1.0 / 60.0, 1.0],
                [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [-1e-3, -1e-3, -1e-9], [0.0, 0.0, 1e-300], [0.0, 0.0, 5e-324],
                [1e-310, 0.0, 0.0]):
        m = base.copy()
        m[2] = row
        out.append(m)
    out += [-base, base * 1e-300, base * 1e300, base * 1e-160]
    for bad in (math.nan, math.inf, -math.inf):
        for i in range(3):
            for j in range(3):
                m = base.copy()
                m[2, :2] = (1e-4, -2e-4)
                m[i, j] = bad
                out.append(m)
    huge = base.copy()
    huge[2] = (1e308, -1e308, 1.0)  # inf - inf at the far corner
    out.append(huge)
    return np.array(out)
