"""Wide panoramas of include/papof.h (papof_mosaic_ray_tensor, papof_mosaic_overlap_ray_tensor) restated in numpy fp64 -- the
rule that tests/test_wide_cpu.py checks with known answers and tests/test_gpu_wide.py compares the device's bytes with.  Only
the pixel's ray and the point (X, Y, D > 0) are restated here: from there on the gather, the modes and the overlap statistics
are tests/_homography_ref.py's own code, run with this file's point in place of the projective one.  Also the tile culling of
mosaic.hip under the ray rule (ray_box, ray_keep) restated, so that the CPU can check it against brute-force liveness, and the
wide scene of both test files: a 160 degree pan over the committed 960 x 540 frame read as a cylinder's texture."""
import math

import numpy as np

import _homography_ref as _h
from _interp_ref import _sample, _taps
from _mosaic_ref import _world

MODES = _h.MODES


# ---- the tables
def plane_tables(Hc, Wc, dtype=np.float64):
    """cols = (x, 1), rows = (y, 1): the ray of pixel (x, y) is (x, y, 1) exactly"""
    cols = np.stack([np.arange(Wc, dtype=np.float64), np.ones(Wc)], 1).astype(dtype)
    rows = np.stack([np.arange(Hc, dtype=np.float64), np.ones(Hc)], 1).astype(dtype)
    return cols, rows


def rays(cols, rows, x, r):
    """the rays (dx, dy, dz) of the canvas pixels (x, r) (integer arrays) under the tables, widened exactly to fp64"""
    c64, r64 = np.asarray(cols).astype(np.float64), np.asarray(rows).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return c64[x, 0] * r64[r, 1], r64[r, 0], c64[x, 1] * r64[r, 1]


def _ray_point(m, d):
    """(X, Y, D > 0) of the ray rule for matrices m (..., 3, 3) broadcast against the rays d = (dx, dy, dz)"""
    dx, dy, dz = d
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        D = (m[..., 2, 0] * dx + m[..., 2, 1] * dy) + m[..., 2, 2] * dz
        X = ((m[..., 0, 0] * dx + m[..., 0, 1] * dy) + m[..., 0, 2] * dz) / D
        Y = ((m[..., 1, 0] * dx + m[..., 1, 1] * dy) + m[..., 1, 2] * dz) / D
        return X, Y, D > 0


def _under_the_ray_rule(call, cols, rows, *args, **kw):
    """a restatement of tests/_homography_ref.py run with the ray rule's point: its gather hands _point the canvas pixel as
    (xd, rd), floats that hold integers; here they index the tables.  Everything behind the point -- liveness inside the
    frame, masks, taps, gains, modes, count, the overlap's fixed point -- is that file's code, unchanged."""
    assert np.asarray(cols).dtype in (np.float32, np.float64) and np.asarray(rows).dtype in (np.float32, np.float64)
    saved = _h._point
    _h._point = lambda m, xd, rd: _ray_point(m, rays(cols, rows, xd.astype(np.int64), rd.astype(np.int64)))
    try:
        return call(*args, **kw)
    finally:
        _h._point = saved


def mosaic_reference_rays(frames, sources, matrices, cols, rows, mode, gains=None, masks=None, out_dtype=np.float64):
    """papof_mosaic_ray_tensor: frames (T, H, W, C), matrices (n_out, N, 3, 3), cols (Wc, 2), rows (Hc, 2) -> (out (n_out, Hc,
    Wc, C) of out_dtype, count (n_out, Hc, Wc) uint8)"""
    size = (len(rows), len(cols))
    return _under_the_ray_rule(_h.mosaic_reference_h, cols, rows, frames, sources, matrices, size, mode, gains, masks, out_dtype)


def overlap_reference_rays(frames, sources, matrices, cols, rows, step=2, bound=1.0, masks=None):
    """papof_mosaic_overlap_ray_tensor: (sums, counts) int64 (n_out, N, N)"""
    size = (len(rows), len(cols))
    return _under_the_ray_rule(_h.overlap_reference_h, cols, rows, frames, sources, matrices, size, step, bound, masks)


# ---- the tile culling of mosaic.hip (ray_box, ray_keep)
def ray_box(cols, rows, xs, rs):
    """(lo (3,), hi (3,)): the bounds of (dx, dy, dz) over the pixels xs x rs (integer arrays), from the tables alone.
    np.min, np.max and np.minimum hand a NaN on, as the kernel's reduction does"""
    c64, r64 = np.asarray(cols).astype(np.float64)[xs], np.asarray(rows).astype(np.float64)[rs]
    with np.errstate(invalid="ignore", over="ignore"):
        ulo, uhi, wlo, whi = c64[:, 0].min(), c64[:, 0].max(), c64[:, 1].min(), c64[:, 1].max()
        slo, shi, clo, chi = r64[:, 0].min(), r64[:, 0].max(), r64[:, 1].min(), r64[:, 1].max()
        px = np.array([ulo * clo, ulo * chi, uhi * clo, uhi * chi])
        pz = np.array([wlo * clo, wlo * chi, whi * clo, whi * chi])
        return np.array([px.min(), slo, pz.min()]), np.array([px.max(), shi, pz.max()])


def cull_keep_rays(m, lo, hi, H, W):
    """False where the rule drops the slot of matrix m (3, 3) from a tile whose rays lie in [lo, hi]; frames H x W"""
    m = np.asarray(m).astype(np.float64)
    if not np.isfinite(m[:2]).all():
        return False
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        blo, bhi = [], []
        for row in (2, 0, 1):  # D, Nx, Ny
            p0, p1 = m[row] * lo, m[row] * hi
            l, h = np.minimum(p0, p1), np.maximum(p0, p1)
            blo.append((l[0] + l[1]) + l[2])
            bhi.append((h[0] + h[1]) + h[2])
        if np.isnan(blo).any() or np.isnan(bhi).any():
            return True
        if not bhi[0] > 0:
            return False
        if not blo[0] > 0:
            return True
        W1, H1 = float(W - 1), float(H - 1)
        missx = (bhi[1] / blo[0] < -1.0 and bhi[1] / bhi[0] < -1.0) or (blo[1] / blo[0] > W1 + 1.0 and blo[1] / bhi[0] > W1 + 1.0)
        missy = (bhi[2] / blo[0] < -1.0 and bhi[2] / bhi[0] < -1.0) or (blo[2] / blo[0] > H1 + 1.0 and blo[2] / bhi[0] > H1 + 1.0)
    return not missx and not missy


def tile_live_rays(m, cols, rows, xs, rs, H, W):
    """brute force: True where the ray rule makes the slot live (masks aside) at some pixel of xs x rs"""
    r, x = np.meshgrid(rs, xs, indexing="ij")
    X, Y, front = _ray_point(np.asarray(m).astype(np.float64), rays(cols, rows, x, r))
    with np.errstate(invalid="ignore"):
        return bool((front & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)).any())


def tiles(Hc, Wc, ty, step=1):
    """the 64 x ty tiles of the pixels sampled at every step-th column and row of an Hc x Wc canvas, as (xs, rs)"""
    sx, sr = np.arange(0, Wc, step), np.arange(0, Hc, step)
    return [(sx[i:i + 64], sr[j:j + ty]) for j in range(0, len(sr), ty) for i in range(0, len(sx), 64)]


# ---- the cameras
def yaw(a):
    return np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])


def pitch(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]])


def roll(a):
    return np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])


def intrinsics(focal, H, W):
    return np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def pair_homographies(K, Rs):
    """the exact pair homographies (T - 1, 3, 3), [2][2] = 1, of a camera K whose frame t sees the ray d at K Rs[t] d"""
    Ki = np.linalg.inv(K)
    G = [K @ Rs[t + 1] @ Rs[t].T @ Ki for t in range(len(Rs) - 1)]
    return np.array([g / g[2, 2] for g in G])


def pan(T, ref, yaw_deg):
    """the rotations of a camera that yaws by yaw_deg per frame, frame `ref` looking along the reference axis"""
    return [yaw(math.radians(yaw_deg) * (t - ref)) for t in range(T)]


def project_rays(m, d):
    """where the 3 x 3 matrix m sends the rays d (3, n): pixels (2, n)"""
    p = np.asarray(m, np.float64) @ d
    return p[:2] / p[2]


# ---- the wide scene
TEXTURE_SCALE = 240.0  # pixels of the committed frame per radian (and per unit of height)


def texture_at(world, theta, h):
    """the committed frame read as a cylinder's texture at the directions (theta, h): column 479.5 + 240 theta, row 269.5 +
    240 h, bilinearly; NaN outside the frame -> (..., 3)"""
    hh, ww, C = world.shape
    X, Y = (ww - 1) / 2.0 + TEXTURE_SCALE * theta, (hh - 1) / 2.0 + TEXTURE_SCALE * h
    inside = (X >= 0) & (X <= ww - 1) & (Y >= 0) & (Y <= hh - 1)
    shape = X.shape
    k = _taps(np.where(inside, X, 0.0).reshape(1, -1), np.where(inside, Y, 0.0).reshape(1, -1), hh, ww)
    pb = np.zeros((1, 1), np.int64)
    out = np.stack([_sample(world[None, :, :, ch], pb, k)[0] for ch in range(C)], -1).reshape(shape + (C,))
    return np.where(inside[..., None], out, math.nan)


def wide_scene(T=41, H=96, W=160, focal=240.0, yaw_deg=4.0):
    """T frames of H x W seen by a camera of focal length `focal` that yaws by yaw_deg per frame about the axis of the
    cylinder that carries the committed 960 x 540 frame, rendered with the exact matrices K R_t: (frames (T, H, W, 3) uint8,
    matrices (T, 3, 3) -- a ray of the reference camera (frame (T - 1) // 2) to frame t --, the exact pair homographies
    (T - 1, 3, 3), the texture (540, 960, 3) float64).  The defaults pan by 160 degrees, 197 with the field of view, inside
    the texture's 229"""
    world = _world()
    K = intrinsics(focal, H, W)
    Rs = pan(T, (T - 1) // 2, yaw_deg)
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    pix = np.stack([x.reshape(-1), r.reshape(-1), np.ones(H * W)])
    frames = np.empty((T, H, W, 3), np.uint8)
    Ki = np.linalg.inv(K)
    for t in range(T):
        d = Rs[t].T @ (Ki @ pix)
        f = texture_at(world, np.arctan2(d[0], d[2]), d[1] / np.hypot(d[0], d[2]))
        assert np.isfinite(f).all()
        frames[t] = np.clip(np.rint(255 * f), 0, 255).astype(np.uint8).reshape(H, W, 3)
    return frames, np.array([K @ R for R in Rs]), pair_homographies(K, Rs), world


def cylinder_truth(world, origin, size, focal):
    """the texture on the grid of a cylinder canvas (wide_transforms' origin and size): pixel (x, y) looks along theta_0 + x /
    focal at height v_0 + y / focal -> (Hc, Wc, 3), NaN outside the texture"""
    Hc, Wc = size
    y, x = np.mgrid[0:Hc, 0:Wc].astype(np.float64)
    return texture_at(world, origin[0] + x / focal, origin[1] + y / focal)


# ---- what both test files feed the culling
def small_pan(surface, T=9, H=20, W=30, focal=40.0, yaw_deg=20.0):
    """the pan that the planar call is pinned to refuse -- nine 20 x 30 frames, focal length 40, 20 degrees per frame -- on a
    canvas of tensors.wide_transforms: (matrices (T, 3, 3), cols, rows, the exact pair homographies)"""
    import torch
    from papteam_opticalflow_amd import tensors
    A = pair_homographies(intrinsics(focal, H, W), pan(T, (T - 1) // 2, yaw_deg))
    M, cols, rows, _, _ = tensors.wide_transforms(torch.from_numpy(A), (H, W), focal, surface=surface)
    return M[0].numpy(), cols.numpy(), rows.numpy(), A


def cull_tables_and_matrices(H=20, W=30):
    """[(what, cols, rows, matrices (n, 3, 3))] that try the tile culling under the ray rule, for frames H x W: the small pan
    on its cylinder and its sphere (its outer frames lie behind the reference: their [2][2] is negative), the same in
    float32, that pan's matrices with NaN and infinite entries in every position, scaled to tiny and huge D and negated, a
    table with a NaN and one with an infinite entry, and the plane's tables under tests/_homography_ref.py's cull_matrices"""
    out = []
    for surface in ("cylinder", "sphere"):
        M, cols, rows, _ = small_pan(surface, H=H, W=W)
        out.append((surface, cols, rows, M))
        out.append((surface + " float32", cols.astype(np.float32), rows.astype(np.float32), M.astype(np.float32)))
        bad = []
        for v in (math.nan, math.inf, -math.inf):
            for i in range(3):
                for j in range(3):
                    m = M[(3 * i + j) % len(M)].copy()
                    m[i, j] = v
                    bad.append(m)
        bad += [M[2] * 1e-300, M[6] * 1e300, M[4] * 1e-160, -M[4], M[1] * 5e-324, np.zeros((3, 3))]
        huge = M[4].copy()
        huge[2] = (1e308, -1e308, 1e308)  # inf - inf in D
        bad.append(huge)
        out.append((surface + " wild matrices", cols, rows, np.array(bad)))
        for v, at in ((math.nan, 70), (math.inf, 3), (-math.inf, 100)):
            c = cols.copy()
            c[at, at % 2] = v
            r = rows.copy()
            r[7, 1 - at % 2] = v
            out.append((surface + " table entry %r" % v, c, rows, M))
            out.append((surface + " row table entry %r" % v, cols, r, M))
    Hc, Wc = 77, 150
    cols, rows = plane_tables(Hc, Wc)
    out.append(("plane", cols, rows, _h.cull_matrices(H, W, Hc, Wc)))
    return out
