"""The rule of papof_refine_flow_tensor (include/papof.h) restated in numpy: the image-guided weighted median of a flow field
with integer weights -- what tests/test_gpu_refine.py compares the device's bytes with, and what tests/test_refine_cpu.py
checks against known answers.  Windows are gathered per pixel (fancy indexing into padded arrays, in chunks), the weights are
int64 products of the two tables, the values are ordered by argsort on the monotone integer key of their float64 bits and the
median is read off the cumulative sum.  `pixels` evaluates chosen pixels only (the 1080p comparison).

Layouts here: flow (B, 2, H, W), guide (B, H, W, C), occlusion / where (B, H, W)."""
import numpy as np

BINS = 4096
KEY_MASK = np.int64(0x7fffffffffffffff)


def key(v):
    """the monotone integer key of float64 values (its own inverse on the bits)"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
    return b ^ ((b >> np.int64(63)) & KEY_MASK)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.int64)
    return (k ^ ((k >> np.int64(63)) & KEY_MASK)).view(np.float64)


def tables(radius, sigma_s):
    """the tables by numpy's exp (the library's are libm's: equal to within one unit)"""
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    d2 = d[:, None] ** 2 + d[None, :] ** 2
    S = np.rint(32768.0 * np.exp(-d2 / (2.0 * sigma_s * sigma_s))).astype(np.uint32).ravel()
    R = np.rint(65536.0 * np.exp(-(np.arange(BINS) + 0.5) / 256.0)).astype(np.uint32)
    return S, R


def q_of(sigma_c, channels, uint8):
    q = 128.0 / (sigma_c * sigma_c * channels)
    return q / 65025.0 if uint8 else q


def _pass_at(flow, guide, dead, S, R, q, r, ys, xs):
    """one pass for one item at the pixels (ys, xs): flow (2, H, W) float64, guide (H, W, C) raw values as float64, dead (H, W)
    bool.  Returns (P, 2) float64."""
    _, H, W = flow.shape
    side = 2 * r + 1
    fp = np.zeros((2, H + 2 * r, W + 2 * r))
    fp[:, r:r + H, r:r + W] = flow
    gp = np.zeros((H + 2 * r, W + 2 * r, guide.shape[2]))
    gp[r:r + H, r:r + W] = guide
    dp = np.ones((H + 2 * r, W + 2 * r), bool)
    dp[r:r + H, r:r + W] = dead | ~np.isfinite(flow[0]) | ~np.isfinite(flow[1])
    dy, dx = np.divmod(np.arange(side * side), side)  # the offsets + r, row-major in (dy, dx) as S
    out = np.empty((len(ys), 2))
    for a in range(0, len(ys), 8192):
        y, x = ys[a:a + 8192], xs[a:a + 8192]
        Y, X = y[:, None] + dy[None, :], x[:, None] + dx[None, :]  # padded coordinates of the neighbours
        with np.errstate(invalid="ignore", over="ignore"):
            D = None
            for c in range(guide.shape[2]):
                d = gp[y + r, x + r, c][:, None] - gp[Y, X, c]
                D = d * d if D is None else D + d * d
            live = ~dp[Y, X] & np.isfinite(D)
            k = np.minimum(np.where(live, D, 0.0) * q, float(BINS - 1)).astype(np.int64)
        w = np.where(live, S.astype(np.int64)[None, :] * R.astype(np.int64)[k], 0)
        T = w.sum(axis=1)
        for comp in range(2):
            keys = key(fp[comp][Y, X])
            order = np.argsort(keys, axis=1, kind="stable")
            cum = np.cumsum(np.take_along_axis(w, order, axis=1), axis=1)
            first = np.argmax(2 * cum >= T[:, None], axis=1)
            med = unkey(np.take_along_axis(keys, np.take_along_axis(order, first[:, None], axis=1), axis=1)[:, 0])
            out[a:a + 8192, comp] = np.where(T > 0, med, flow[comp][y, x])
    return out


def refine_reference(flow, guide, S, R, q, radius, occlusion=None, where=None, iters=1, out_dtype=None, pixels=None):
    """flow (B, 2, H, W) float32 / float64; guide (B, H, W, C) uint8 / float32 / float64 (raw values); S, R, q as the C call
    takes them.  Returns the refined flow (B, 2, H, W) of out_dtype (default: the flow's) -- or, with pixels = (ys, xs) and
    iters = 1, the (B, P, 2) values at those pixels only."""
    flow = np.asarray(flow)
    out_dtype = flow.dtype if out_dtype is None else out_dtype
    B, _, H, W = flow.shape
    cur = flow.astype(np.float64)
    g = np.asarray(guide).astype(np.float64)
    occ = np.zeros((B, H, W), bool) if occlusion is None else np.asarray(occlusion) != 0
    if pixels is not None:
        assert iters == 1 and where is None
        ys, xs = (np.asarray(p, dtype=np.int64) for p in pixels)
        return np.stack([_pass_at(cur[b], g[b], occ[b], S, R, q, radius, ys, xs) for b in range(B)]).astype(out_dtype)
    sel = np.ones((B, H, W), bool) if where is None else np.asarray(where) != 0
    for _ in range(iters):
        nxt = cur.copy()
        for b in range(B):
            ys, xs = np.nonzero(sel[b])
            if len(ys):
                got = _pass_at(cur[b], g[b], occ[b], S, R, q, radius, ys, xs)
                nxt[b, 0][ys, xs], nxt[b, 1][ys, xs] = got[:, 0], got[:, 1]
        cur = nxt
    return cur.astype(out_dtype)


def two_layer_scene(seed=0, H=96, W=128):
    """The scene with known ground truth: a rectangle and a disc moving (4, -2) over a background moving (0.5, 0).  Returns
    (guide uint8 (1, H, W, 3): two distinct colours plus smooth texture of amplitude about 0.04; the true flow (1, 2, H, W);
    the degraded flow: the true one blurred by a Gaussian of sigma 2 px plus noise of std 0.05; the band (H, W) where the
    blurred layer mask is in (0.02, 0.98))."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    layer = ((ys >= 20) & (ys < 56) & (xs >= 16) & (xs < 64)) | ((ys - 60) ** 2 + (xs - 92) ** 2 <= 22 ** 2)

    def blur(a, sigma):
        t = np.arange(-int(4 * sigma), int(4 * sigma) + 1)
        k = np.exp(-t * t / (2.0 * sigma * sigma))
        k /= k.sum()
        p = np.pad(a, len(t) // 2, mode="edge")
        p = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, p)
        return np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, p)

    tex = np.stack([blur(rng.standard_normal((H, W)), 3.0) for _ in range(3)], axis=-1)
    tex *= 0.04 / np.abs(tex).max()
    colour = np.where(layer[..., None], np.array([0.75, 0.35, 0.3]), np.array([0.25, 0.5, 0.65]))
    guide = np.rint(255.0 * np.clip(colour + tex, 0, 1)).astype(np.uint8)[None]
    true = np.zeros((1, 2, H, W))
    true[0, 0] = np.where(layer, 4.0, 0.5)
    true[0, 1] = np.where(layer, -2.0, 0.0)
    soft = blur(layer.astype(np.float64), 2.0)
    degraded = np.stack([blur(true[0, 0], 2.0), blur(true[0, 1], 2.0)])[None] + rng.normal(0, 0.05, (1, 2, H, W))
    return guide, true, degraded, (soft > 0.02) & (soft < 0.98)


def epe(flow, true, mask=None):
    e = np.sqrt(((np.asarray(flow, dtype=np.float64) - true) ** 2).sum(axis=1))[0]
    return float(e[mask].mean() if mask is not None else e.mean())


def two_layer_frames(seed=0, H=96, W=128):
    """The layers of two_layer_scene rendered as two uint8 frames (1, H, W, 3) whose true forward flow is the scene's: each
    layer carries its own texture (amplitude 0.15 around its colour), the foreground moved by (4, -2) pixels and the
    background by (0.5, 0) (the mean of two neighbouring columns).  Returns (frame1, frame2, true flow, band) -- what
    tools/refine_probe.py estimates flows on."""
    guide, true, _, band = two_layer_scene(seed, H, W)
    rng = np.random.default_rng(seed + 1000)
    layer = true[0, 0] == 4.0

    def texture(colour):
        t = rng.standard_normal((H, W, 3))
        for _ in range(2):
            t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5
        return np.array(colour) + 0.15 * t / np.abs(t).max()
    fg, bg = texture([0.75, 0.35, 0.3]), texture([0.25, 0.5, 0.65])
    f1 = np.where(layer[..., None], fg, bg)
    moved = np.roll(layer, (-2, 4), (0, 1))
    f2 = np.where(moved[..., None], np.roll(fg, (-2, 4), (0, 1)), 0.5 * (bg + np.roll(bg, 1, 1)))
    q = lambda f: np.rint(255.0 * np.clip(f, 0, 1)).astype(np.uint8)[None]  # noqa: E731
    return q(f1), q(f2), true, band
