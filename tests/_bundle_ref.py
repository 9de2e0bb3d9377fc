"""Bundle adjustment of include/papof.h (papof_bundle_sums_tensor) and papteam_opticalflow_amd/tensors.py (bundle_adjust,
bundle_links) restated in numpy fp64 -- what tests/test_bundle_cpu.py checks with known answers and tests/test_gpu_bundle.py
compares the device with.  The per-pixel terms are the header's operations in the header's order (numpy fuses nothing), so a
sum of the device differs from this file's only by the order of its additions: sums_reference returns, next to each sum, the
sum of its terms' absolute values and the number of terms, which bound that difference.  Also a Levenberg-Marquardt driver
written on its own (dense Jacobian blocks, not tensors.bundle_solve's code), bundle_links' overlap rule as two loops, and the
scenes: synthetic chains and rings with exact or noisy flows, and ring_scene, the committed 960 x 540 frame read as a PERIODIC
cylinder texture under a camera that turns a full circle."""
import math

import numpy as np

from _mosaic_ref import _world
from _wide_ref import intrinsics, pitch, roll, yaw  # noqa: F401  (the cameras of both test files)

MIN_DEN = 0.0625
N_SUMS = 20
MIN_VALID = 16
TRI = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]


# ---- the per-pixel rule
def predicted(R, f, x, r, H, W):
    """(Px, Py, qz) of the header's rule at the pixels (x, r) (float arrays) under the link rotation R (3, 3)"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    with np.errstate(all="ignore"):
        px, py = (x - cx) / f, (r - cy) / f
        qx = (R[0, 0] * px + R[0, 1] * py) + R[0, 2]
        qy = (R[1, 0] * px + R[1, 1] * py) + R[1, 2]
        qz = (R[2, 0] * px + R[2, 1] * py) + R[2, 2]
        gx, gy = qx / qz, qy / qz
        return f * gx + cx, f * gy + cy, qz


def jacobian(R, f, x, r, H, W):
    """(Jx (4, n), Jy (4, n)) of the header's rule: the predicted point in (a_x, a_y, a_z, f)"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    with np.errstate(all="ignore"):
        px, py = (x - cx) / f, (r - cy) / f
        qx = (R[0, 0] * px + R[0, 1] * py) + R[0, 2]
        qy = (R[1, 0] * px + R[1, 1] * py) + R[1, 2]
        qz = (R[2, 0] * px + R[2, 1] * py) + R[2, 2]
        gx, gy = qx / qz, qy / qz
        fgx, fgy = f * gx, f * gy
        Jx = np.stack([-(fgx * gy), f + fgx * gx, -fgy, gx + (R[0, 2] - gx * R[2, 2]) / qz])
        Jy = np.stack([-(f + fgy * gy), fgx * gy, fgx, gy + (R[1, 2] - gy * R[2, 2]) / qz])
    return Jx, Jy


def link_terms(flow, R, f, occ=None, step=1, scale=1.0):
    """the terms of one link: flow (2, H, W) float32 / float64, R (3, 3), occ None or (H, W) uint8 -> (n_valid, 20) float64,
    one row per valid sampled pixel in row-major order, its columns the twenty terms in the header's order"""
    _, H, W = flow.shape
    r, x = np.mgrid[0:H:step, 0:W:step]
    u, v = flow[0, r, x].astype(np.float64), flow[1, r, x].astype(np.float64)
    xd, rd = x.astype(np.float64), r.astype(np.float64)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    with np.errstate(all="ignore"):
        X, Y = xd + u, rd + v
        valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        if occ is not None:
            valid &= occ[r, x] == 0
        px, py = (xd - cx) / f, (rd - cy) / f
        qx = (R[0, 0] * px + R[0, 1] * py) + R[0, 2]
        qy = (R[1, 0] * px + R[1, 1] * py) + R[1, 2]
        qz = (R[2, 0] * px + R[2, 1] * py) + R[2, 2]
        valid &= qz > MIN_DEN
        gx, gy = qx / qz, qy / qz
        fgx, fgy = f * gx, f * gy
        ex, ey = X - (fgx + cx), Y - (fgy + cy)
        e2 = ex * ex + ey * ey
        w = 1.0 / (1.0 + e2 / (scale * scale))
        Jx = [-(fgx * gy), f + fgx * gx, -fgy, gx + (R[0, 2] - gx * R[2, 2]) / qz]
        Jy = [-(f + fgy * gy), fgx * gy, fgx, gy + (R[1, 2] - gy * R[2, 2]) / qz]
        cols = [w * (Jx[a] * Jx[b] + Jy[a] * Jy[b]) for a, b in TRI]
        cols += [w * (Jx[a] * ex + Jy[a] * ey) for a in range(4)]
        cols += [w * e2, w, np.ones_like(w), e2, np.zeros_like(w), np.zeros_like(w)]
    return np.stack([c[valid] for c in cols], 1)


def sums_reference(flow, Rij, f, occ=None, step=1, scale=1.0):
    """papof_bundle_sums_tensor: flow (L, 2, H, W), Rij (L, 3, 3), occ None or (L, 2, H, W) uint8 / bool (channel 0 read) ->
    (sums (L, 20), the sums of the terms' absolute values (L, 20), the number of valid samples (L,))"""
    L = flow.shape[0]
    S, A, n = np.zeros((L, N_SUMS)), np.zeros((L, N_SUMS)), np.zeros(L, np.int64)
    for l in range(L):
        t = link_terms(flow[l], Rij[l], f, None if occ is None else np.asarray(occ[l, 0]).astype(np.uint8), step, scale)
        S[l], A[l], n[l] = t.sum(0), np.abs(t).sum(0), t.shape[0]
    return S, A, n


# ---- the driver, written on its own
def rodrigues(w):
    t = float(np.linalg.norm(w))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-8:
        return np.eye(3) + Kx + 0.5 * (Kx @ Kx)
    return np.eye(3) + (math.sin(t) / t) * Kx + ((1.0 - math.cos(t)) / (t * t)) * (Kx @ Kx)


def expand(S, links, R, T):
    """the (3 T + 1) normal equations of the links' sums: every link's 4 x 4 block B and right-hand side c are those of (a, df),
    a = omega_j - R_ij omega_i, so with the 4 x (3 T + 1) matrix D of d(a, df) / d(omega_0 .. omega_T-1, df) they add D^T B D
    and D^T c"""
    n = 3 * T + 1
    N, g = np.zeros((n, n)), np.zeros(n)
    for l, (i, j) in enumerate(links):
        B = np.zeros((4, 4))
        for k, (a, b) in enumerate(TRI):
            B[a, b] = B[b, a] = S[l, k]
        D = np.zeros((4, n))
        D[:3, 3 * i:3 * i + 3] = -(R[j] @ R[i].T)
        D[:3, 3 * j:3 * j + 3] = np.eye(3)
        D[3, 3 * T] = 1.0
        N += D.T @ B @ D
        g += D.T @ S[l, 10:14]
    return N, g


def adjust_reference(evaluate, links, R, f, iters=10, ref=0, fix_focal=False, damping=1e-4):
    """Levenberg-Marquardt as tensors.bundle_solve states it, over evaluate(Rij, f) -> (L, 20): (R, f, cost (iters + 1,),
    accepted (iters,))"""
    R, f, T = np.array(R, np.float64), float(f), len(R)
    links = [(int(i), int(j)) for i, j in links]

    def at(R, f):
        S = np.array(evaluate(np.stack([R[j] @ R[i].T for i, j in links]), f))
        S[S[:, 16] < MIN_VALID] = 0.0
        seen = {t for l, (i, j) in enumerate(links) if S[l, 16] > 0 for t in (i, j)}
        return S, len(seen) == T

    S, whole = at(R, f)
    assert whole
    cost, accepted, kept = [S[:, 14].sum()], [], S[:, 14].sum()
    free = [k for k in range(3 * T + 1) if k // 3 != ref and not (fix_focal and k == 3 * T)]
    for _ in range(iters):
        N, g = expand(S, links, R, T)
        N, g = N[np.ix_(free, free)], g[free]
        d = np.zeros(3 * T + 1)
        try:
            d[free] = np.linalg.solve(N + damping * np.diag(np.diag(N)), g)
            good = np.isfinite(d).all() and f + d[3 * T] > 0
        except np.linalg.LinAlgError:
            good = False
        c1 = math.inf
        if good:
            R1 = np.stack([rodrigues(d[3 * t:3 * t + 3]) @ R[t] for t in range(T)])
            S1, whole = at(R1, f + d[3 * T])
            c1 = S1[:, 14].sum() if whole else math.inf
        cost.append(c1)
        accepted.append(bool(c1 <= kept))
        if accepted[-1]:
            R, f, S, kept, damping = R1, f + d[3 * T], S1, c1, damping / 10.0
        else:
            damping *= 10.0
    return R, f, np.array(cost), np.array(accepted)


# ---- bundle_links' rule
def overlap_share(Rij, H, W, f, n=16):
    """the share of an n x n grid of a frame's pixels (corners included) that Rij sends inside the other frame, qz > MIN_DEN"""
    hit = 0
    for y in np.linspace(0.0, H - 1.0, n):
        for x in np.linspace(0.0, W - 1.0, n):
            X, Y, qz = predicted(Rij, f, np.float64(x), np.float64(y), H, W)
            hit += bool(qz > MIN_DEN and 0 <= X <= W - 1 and 0 <= Y <= H - 1)
    return hit / float(n * n)


def links_reference(R, H, W, f, min_overlap=0.3):
    return np.array([(i, j) for i in range(len(R)) for j in range(i + 1, len(R))
                     if j == i + 1 or overlap_share(R[j] @ R[i].T, H, W, f) >= min_overlap], np.int64)


# ---- synthetic chains and rings
def exact_flows(Rs, links, H, W, f):
    """the flows (L, 2, H, W) of the rotations Rs (frame t sees the ray d at K Rs[t] d) along `links`; NaN behind the horizon"""
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((len(links), 2, H, W))
    for l, (i, j) in enumerate(links):
        X, Y, qz = predicted(Rs[j] @ Rs[i].T, f, x, r, H, W)
        out[l, 0], out[l, 1] = np.where(qz > 0, X - x, math.nan), np.where(qz > 0, Y - r, math.nan)
    return out


def wobble(T, yaw_deg, seed=5, amount=2.0):
    """a hand-held pan: frame t yaws by t * yaw_deg and pitches and rolls by up to `amount` degrees; frame 0 is the identity"""
    rng = np.random.default_rng(seed)
    a = np.radians(amount) * rng.uniform(-1, 1, (T, 2))
    a[0] = 0.0
    return np.stack([roll(a[t, 1]) @ pitch(a[t, 0]) @ yaw(math.radians(yaw_deg) * t) for t in range(T)])


def perturbed(Rs, deg, seed=9, ref=0):
    """Rs with every rotation but `ref`'s turned by about `deg` degrees about a random axis"""
    rng = np.random.default_rng(seed)
    out = np.array(Rs)
    for t in range(len(Rs)):
        if t != ref:
            w = rng.normal(size=3)
            out[t] = rodrigues(math.radians(deg) * w / np.linalg.norm(w)) @ Rs[t]
    return out


def open_chain(T=12, H=48, W=80, f=120.0, yaw_deg=6.0):
    """(Rs, links, exact flows): an open chain with the links (i, i + 1) and (i, i + 2)"""
    Rs = wobble(T, yaw_deg)
    links = np.array(sorted([(i, i + 1) for i in range(T - 1)] + [(i, i + 2) for i in range(T - 2)]), np.int64)
    return Rs, links, exact_flows(Rs, links, H, W, f)


def ring(T=18, H=48, W=80, f=120.0):
    """(Rs, links, exact flows): a closed ring of T frames, 360 / T degrees apart, with the consecutive links and the closing
    link (0, T - 1)"""
    Rs = wobble(T, 360.0 / T)
    links = np.array(sorted([(i, i + 1) for i in range(T - 1)] + [(0, T - 1)]), np.int64)
    return Rs, links, exact_flows(Rs, links, H, W, f)


def noisy(flows, sigma=0.2, outliers=0.2, size=15.0, seed=3):
    """flows with Gaussian noise of `sigma` px on every component and a share `outliers` of the pixels moved by up to +- size"""
    rng = np.random.default_rng(seed)
    out = flows + sigma * rng.normal(size=flows.shape)
    hit = rng.uniform(size=flows.shape[:1] + flows.shape[2:]) < outliers
    out += hit[:, None] * rng.uniform(-size, size, flows.shape)
    return out


def corner_error(R, Rs, f, H, W, ref=0):
    """the largest distance in px, over the frames' four corners, between where K R_t sends the rays of the true corners K Rs_t
    and the corners themselves, both chains taken relative to frame `ref`"""
    K = intrinsics(f, H, W)
    c = np.array([[0.0, W - 1.0, 0.0, W - 1.0], [0.0, 0.0, H - 1.0, H - 1.0], [1.0, 1.0, 1.0, 1.0]])
    worst = 0.0
    for t in range(len(R)):
        d = (Rs[t] @ Rs[ref].T).T @ (np.linalg.inv(K) @ c)
        p = K @ (R[t] @ R[ref].T) @ d
        worst = max(worst, float(np.hypot(*(p[:2] / p[2] - c[:2])).max()))
    return worst


# ---- the ring scene
def ring_texture(d=1):
    """the committed 960 x 540 frame box-decimated by d -> (540 / d, 960 / d, 3) float64: a cylinder's texture whose columns
    wrap, 960 / (2 pi d) px per radian and per unit of height"""
    w = _world()
    return w.reshape(w.shape[0] // d, d, w.shape[1] // d, d, 3).mean((1, 3))


def ring_texture_at(tex, theta, h):
    """the periodic texture at the directions (theta, h): column theta * Wt / 2 pi modulo Wt, row (Ht - 1) / 2 + h * Wt / 2 pi,
    bilinear; NaN above and below the texture"""
    Ht, Wt, _ = tex.shape
    s = Wt / (2.0 * math.pi)
    X, Y = np.mod(theta * s, Wt), (Ht - 1) / 2.0 + h * s
    inside = (Y >= 0) & (Y <= Ht - 1)
    Yc = np.clip(np.where(inside, Y, 0.0), 0, Ht - 1)
    x0 = np.floor(X).astype(np.int64) % Wt
    y0 = np.minimum(np.floor(Yc).astype(np.int64), Ht - 2)
    ax, ay = (X - np.floor(X))[..., None], (Yc - y0)[..., None]
    x1 = (x0 + 1) % Wt
    out = (1 - ay) * ((1 - ax) * tex[y0, x0] + ax * tex[y0, x1]) + ay * ((1 - ax) * tex[y0 + 1, x0] + ax * tex[y0 + 1, x1])
    return np.where(inside[..., None], out, math.nan)


def ring_scene(T=48, H=48, W=80, decimation=2):
    """T frames of H x W over a full circle, 360 / T degrees apart, seen by a camera whose focal length is the texture's
    960 / (2 pi decimation) px per radian (76.39 at 2): (frames (T, H, W, 3) uint8, rotations (T, 3, 3), focal, the texture).
    Frame 0 looks along the direction of texture column 0.5: the full-circle canvas of bundle_transforms about frame 0 then
    has its columns half way between the texture's, as its rows are and as both are on the open pan of tests/_wide_ref.py, whose
    PSNR figures the ring is compared with (a canvas that hits the texels exactly is compared with an unsmoothed truth and
    scores 10 dB less on this texture).  The defaults move by 10 px per frame on frames 80 px wide"""
    tex = ring_texture(decimation)
    f = tex.shape[1] / (2.0 * math.pi)
    Rs = np.stack([yaw(2.0 * math.pi * t / T + 0.5 / f) for t in range(T)])
    Ki = np.linalg.inv(intrinsics(f, H, W))
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    pix = np.stack([x.reshape(-1), r.reshape(-1), np.ones(H * W)])
    frames = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        d = Rs[t].T @ (Ki @ pix)
        c = ring_texture_at(tex, np.arctan2(d[0], d[2]), d[1] / np.hypot(d[0], d[2]))
        assert np.isfinite(c).all()
        frames[t] = np.clip(np.rint(255 * c), 0, 255).astype(np.uint8).reshape(H, W, 3)
    return frames, Rs, f, tex


def ring_truth(tex, cols, rows):
    """the periodic texture on a cylinder canvas given by its tables (cols = (sin, cos) of theta, rows = (h, 1))"""
    theta = np.arctan2(cols[:, 0], cols[:, 1])
    return ring_texture_at(tex, theta[None, :] + 0 * rows[:, :1], rows[:, :1] + 0 * theta[None, :])
