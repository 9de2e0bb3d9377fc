"""Numpy restatements of include/papof.h's papof_decimate_tensor and papof_upsample_flow_tensor, written from the header's
text: fp64, every sum in the stated order, no fused multiply-add (numpy has none).  The tables are arguments, so the tests
pass the library's own (papof_upsample_tables) and compare raw bytes.  Not part of the product."""
import numpy as np

BINS = 1024


def _samples(frames):
    """(N, H, W, C) uint8 / float32 / float64 -> the float64 samples as the library reads them"""
    f = np.asarray(frames)
    return f.astype(np.float64) / 255.0 if f.dtype == np.uint8 else f.astype(np.float64)


def decimate_reference(frames, factor, out_dtype=np.float64):
    """frames (N, H, W, C) -> (N, ceil(H / factor), ceil(W / factor), C): the mean of the block's pixels that exist, summed
    from 0 in row-major order"""
    x = _samples(frames)
    N, H, W, C = x.shape
    h, w = -(-H // factor), -(-W // factor)
    ys, xs = np.arange(h)[:, None] * factor, np.arange(w)[None, :] * factor
    total, count = np.zeros((N, h, w, C)), np.zeros((h, w))
    for j in range(factor):
        for i in range(factor):
            yy, xx = ys + j, xs + i
            ok = (yy < H) & (xx < W)
            s = x[:, np.minimum(yy, H - 1), np.minimum(xx, W - 1)]
            total = np.where(ok[None, :, :, None], total + s, total)
            count = count + ok
    return (total / count[None, :, :, None]).astype(out_dtype)


def upsample_reference(flow_lr, guide, guide_lr, S, R, q, factor, radius, occlusion=None, out_dtype=np.float64, pixels=None):
    """flow_lr (B, 2, h, w) float32 / float64, guide (B, H, W, C) uint8 / float32 / float64, guide_lr (B, h, w, C) float32 /
    float64, S (factor^2 (2 radius + 1)^2,) and R (1024,) as papof_upsample_tables fills them, occlusion None or (B, h, w).
    Returns (B, 2, H, W) -- or, with pixels = (ys, xs), (B, 2, len(ys)): the rule at those output pixels only."""
    v = np.asarray(flow_lr).astype(np.float64)
    g, gl = _samples(guide), np.asarray(guide_lr).astype(np.float64)
    B, H, W, C = g.shape
    h, w = v.shape[2:]
    assert (h, w) == (-(-H // factor), -(-W // factor)) and gl.shape == (B, h, w, C)
    side = 2 * radius + 1
    S = np.asarray(S).astype(np.int64).reshape(factor, factor, side, side)
    R = np.asarray(R).astype(np.int64)
    if pixels is None:
        Y, X = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
    else:
        Y, X = (np.asarray(a, dtype=np.int64) for a in pixels)
    cy, cx, py, px = Y // factor, X // factor, Y % factor, X % factor
    dead = ~(np.isfinite(v[:, 0]) & np.isfinite(v[:, 1]))
    if occlusion is not None:
        dead |= np.asarray(occlusion) != 0
    gp = g[:, Y, X]  # (B, P, C)
    su, sv, sw = np.zeros((B, len(Y))), np.zeros((B, len(Y))), np.zeros((B, len(Y)), np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                ty, tx = cy + dy, cx + dx
                ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                ty, tx = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                live = ok[None] & ~dead[:, ty, tx]
                D = np.zeros((B, len(Y)))
                for ch in range(C):
                    d = gp[..., ch] - gl[:, ty, tx, ch]
                    D = D + d * d
                Dq = D * q
                k = np.where(Dq < BINS - 1.0, Dq, BINS - 1.0).astype(np.int64)  # (a NaN: the last bin)
                wk = (S[py, px, dy + radius, dx + radius][None] * R[k]).astype(np.float64)
                su = np.where(live, su + wk * v[:, 0, ty, tx], su)
                sv = np.where(live, sv + wk * v[:, 1, ty, tx], sv)
                sw = sw + np.where(live, wk, 0.0).astype(np.int64)
        none = sw == 0
        den = np.where(none, 1, sw).astype(np.float64)
        u = np.where(none, factor * v[:, 0, cy, cx], su / den * factor)
        vv = np.where(none, factor * v[:, 1, cy, cx], sv / den * factor)
    out = np.stack([u, vv], 1)
    if pixels is None:
        out = out.reshape(B, 2, H, W)
    return out.astype(out_dtype)


def bilinear_reference(flow_lr, factor, H, W):
    """plain bilinear up-sampling of (B, 2, h, w) to (B, 2, H, W), times factor: the baseline of the quality tests.  Output
    pixel Y samples the low-resolution position (Y - (factor - 1) / 2) / factor, clamped into the grid."""
    v = np.asarray(flow_lr, dtype=np.float64)
    h, w = v.shape[2:]
    Y = np.clip((np.arange(H) - (factor - 1) / 2) / factor, 0, h - 1)
    X = np.clip((np.arange(W) - (factor - 1) / 2) / factor, 0, w - 1)
    y0, x0 = np.minimum(Y.astype(int), max(h - 2, 0)), np.minimum(X.astype(int), max(w - 2, 0))
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (Y - y0)[:, None], (X - x0)[None, :]
    rows = lambda r: ((1 - fx) * v[:, :, r][:, :, :, x0] + fx * v[:, :, r][:, :, :, x1])  # noqa: E731
    return factor * ((1 - fy) * rows(y0) + fy * rows(y1))


MOTION = ((6.0, -3.0), (0.5, 0.2))  # (vx, vy) of the layer and of the background
TEXTURE = (0.3, 0.25, 0.06)  # the analytic texture's (kx, ky, amplitude): periods of 21 and 25 pixels, well above the motion


def _layer(y, x, H):
    s = H / 1080.0
    return (np.hypot(y - 500 * s, x - 900 * s) < 300 * s) | ((x > 1400 * s) & (y > 700 * s))


def _colours(y, x, layer, H, texture):
    """the scene's colours at (possibly fractional) coordinates of its first frame, (..., 3) in 0 .. 1: two flat colours and
    a slow wave; with `texture`, a finer analytic pattern too, which gives a solver something to hold on to"""
    s = H / 1080.0
    base = np.where(layer[..., None], [0.7, 0.4, 0.3], [0.3, 0.5, 0.6])
    wave = 0.04 * np.sin(0.05 * x / s + 0.03 * y / s)
    if texture:
        kx, ky, amp = TEXTURE
        wave = wave + amp * np.sin(kx * x + 0.4 * np.cos(0.8 * ky * y)) * np.cos(ky * y)
    return base + wave[..., None] * np.array([1.0, 0.8, 1.2] if texture else [1.0, 1.0, 1.0])


def two_layer_scene(H=135, W=240, second=False):
    """The two-layer scene of tests/test_gpu_refine.py's 1080p case at H x W: a disc and a corner moving by (6, -3) over a
    background moving by (0.5, 0.2).  Returns (guide uint8 (1, H, W, 3): that case's colours, wave and noise of std 0.01;
    the exact flow (1, 2, H, W); the layer mask (H, W)).  With second=True the guide carries an analytic texture instead of
    the noise and the second frame uint8 (1, H, W, 3) is returned too: each layer's colours carried along its motion, the
    layer in front."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    layer = _layer(y, x, H)
    first = _colours(y, x, layer, H, second)
    if not second:
        first = first + np.random.default_rng(13).normal(0, 0.01, (H, W, 3))
    guide = np.rint(255 * np.clip(first, 0, 1)).astype(np.uint8)[None]
    flow = np.stack([np.where(layer, MOTION[0][0], MOTION[1][0]), np.where(layer, MOTION[0][1], MOTION[1][1])])[None]
    if not second:
        return guide, flow, layer
    (lu, lv), (bu, bv) = MOTION
    moved = _layer(y - lv, x - lu, H)  # a pixel of frame 2 shows the layer if it came from inside it
    true, false = np.ones_like(moved), np.zeros_like(moved)
    frame2 = np.where(moved[..., None], _colours(y - lv, x - lu, true, H, True), _colours(y - bv, x - bu, false, H, True))
    return guide, flow, layer, np.rint(255 * np.clip(frame2, 0, 1)).astype(np.uint8)[None]


def band_of(layer, factor):
    """the pixels within `factor` of a layer change: both layers occur in their (2 factor + 1)^2 neighbourhood"""
    H, W = layer.shape
    p = np.pad(layer, factor, mode="edge")
    any_, all_ = np.zeros_like(layer), np.ones_like(layer)
    for j in range(2 * factor + 1):
        for i in range(2 * factor + 1):
            any_ |= p[j:j + H, i:i + W]
            all_ &= p[j:j + H, i:i + W]
    return any_ & ~all_


def epe(flow, true, mask):
    return float(np.sqrt(((np.asarray(flow, dtype=np.float64) - true) ** 2).sum(axis=1))[0][mask].mean())
