"""Hierarchical block matching (include/papof.h: papof_match_hier_tensor) restated in numpy integers -- the rule that
tests/test_hmatch_cpu.py checks against a plain loop and tests/test_gpu_hmatch.py compares the device's outputs with, byte
for byte -- and the pan scene of the motions beyond the flat search's reach.

    disp, cost = hmatch_reference(A, B, stride=2, levels=3, patch=3, search=20, refine=1)   # as _match_ref.match_reference

Only the test suite and tools/hmatch_probe.py import this module."""
import numpy as np

from _match_ref import decimate, match_coarse, quantise, texture

MAX_LEVELS, MAX_REFINE, MAX_TOP_STRIDE = 4, 3, 32


def hkey(cost, dx, dy):
    """the lexicographic key (cost, dx^2 + dy^2, dy, dx) as one unsigned integer of 26 + 18 + 10 + 10 = 64 bits (Python
    integers, or arrays: then uint64)"""
    if isinstance(cost, np.ndarray):
        cost, dx, dy = cost.astype(np.int64), np.asarray(dx, np.int64), np.asarray(dy, np.int64)
        u = lambda v, shift: v.astype(np.uint64) << np.uint64(shift)  # noqa: E731
        return u(cost, 38) | u(dx * dx + dy * dy, 20) | u(dy + 512, 10) | u(dx + 512, 0)
    return (cost << 38) | ((dx * dx + dy * dy) << 20) | ((dy + 512) << 10) | (dx + 512)


def predictors(d1, h, w):
    """d1 (2, h1, w1) of the level above -> the five predictors (5, 2, h, w) of the h x w grid: twice the parent's vector,
    the side neighbours' in x, in y and in both, and zero"""
    _, h1, w1 = d1.shape
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = np.minimum(xx >> 1, w1 - 1), np.minimum(yy >> 1, h1 - 1)
    nx = np.clip(px + np.where(xx & 1, 1, -1), 0, w1 - 1)
    ny = np.clip(py + np.where(yy & 1, 1, -1), 0, h1 - 1)
    out = [2 * d1[:, Y, X] for Y, X in ((py, px), (py, nx), (ny, px), (ny, nx))]
    return np.stack(out + [np.zeros((2, h, w), np.int64)])


def refine_level(a, b, d1, patch, refine, penalty=0):
    """a, b (h, w, C) int64 frames of one level, d1 (2, h1, w1) the level above's field in its cells -> (d (2, h, w), cost (h, w))"""
    h, w, _ = a.shape
    P = patch
    yy, xx = np.mgrid[0:h, 0:w]
    off = np.arange(-P, P + 1)
    wy, wx = yy[:, :, None, None] + off[None, None, :, None], xx[:, :, None, None] + off[None, None, None, :]
    aw = a[np.clip(wy, 0, h - 1), np.clip(wx, 0, w - 1)]  # (h, w, n, n, C)
    best = np.full((h, w), np.iinfo(np.uint64).max)
    for pred in predictors(d1, h, w):
        for ey in range(-refine, refine + 1):
            for ex in range(-refine, refine + 1):
                dx, dy = pred[0] + ex, pred[1] + ey
                ok = (xx + dx >= 0) & (xx + dx < w) & (yy + dy >= 0) & (yy + dy < h)
                if not ok.any():
                    continue
                bw = b[np.clip(wy + dy[:, :, None, None], 0, h - 1), np.clip(wx + dx[:, :, None, None], 0, w - 1)]
                cost = np.abs(aw - bw).sum(axis=(2, 3, 4)) + penalty * (np.abs(dx) + np.abs(dy))
                best = np.where(ok, np.minimum(best, hkey(cost, dx, dy)), best)
    lo = np.uint64(1023)
    return (np.stack([(best & lo).astype(np.int64) - 512, ((best >> np.uint64(10)) & lo).astype(np.int64) - 512]),
            (best >> np.uint64(38)).astype(np.int64))


def hmatch_levels(qa, qb, stride, levels, patch, search, refine, penalty=0):
    """qa, qb (H, W, C) uint8 -> [(d_l, cost_l)] for l = 0 .. levels - 1, d_l in the cells of level l"""
    H, W, _ = qa.shape
    top = stride << (levels - 1)
    assert 1 <= levels <= MAX_LEVELS and 1 <= refine <= MAX_REFINE and top <= MAX_TOP_STRIDE and H >= top and W >= top
    out = [None] * levels
    for l in range(levels - 1, -1, -1):
        a, b = decimate(qa[None], stride << l)[0], decimate(qb[None], stride << l)[0]
        if l == levels - 1:
            out[l] = match_coarse(a, b, patch, search, penalty)
        else:
            out[l] = refine_level(a, b, out[l + 1][0], patch, refine, penalty)
    return out


def hmatch_reference(A, B, stride=2, levels=1, patch=3, search=20, refine=1, penalty=0, out_dtype=np.float64):
    """A, B (n, H, W, C) uint8 / float32 / float64 -> (disp (n, 2, h, w) = stride * d_0, cost (n, h, w)) of out_dtype"""
    qa, qb = quantise(A), quantise(B)
    got = [hmatch_levels(qa[i], qb[i], stride, levels, patch, search, refine, penalty)[0] for i in range(qa.shape[0])]
    return (np.stack([stride * d for d, _ in got]).astype(out_dtype), np.stack([c for _, c in got]).astype(out_dtype))


def wide_pan_scene(seed, motion, H=135, W=240, pad=160):
    """_match_ref.pan_scene with a pad that holds motions of up to `pad` pixels: (im1, im2, truth, interior)"""
    mx, my = motion
    assert max(abs(mx), abs(my)) <= pad
    rng = np.random.default_rng(seed)
    bg = texture(rng, H + 2 * pad, W + 2 * pad)
    im1 = bg[pad:pad + H, pad:pad + W].copy()
    im2 = bg[pad - my:pad - my + H, pad - mx:pad - mx + W].copy()
    truth = np.zeros((H, W, 2))
    truth[..., 0], truth[..., 1] = mx, my
    yy, xx = np.mgrid[0:H, 0:W]
    interior = (xx + mx >= 3) & (xx + mx < W - 3) & (yy + my >= 3) & (yy + my < H - 3)
    return im1, im2, truth, interior


def exact_share(disp, motion, stride, size, margin=8):
    """the share of cells that hold `motion` exactly -- a component that is no multiple of the stride: either of the two
    whole cells next to it -- among the cells whose target stays `margin` pixels inside the frame"""
    H, W = size
    _, h, w = disp.shape
    yy, xx = np.mgrid[0:h, 0:w]
    X, Y = xx * stride + motion[0], yy * stride + motion[1]
    inside = (X >= margin) & (X < W - margin) & (Y >= margin) & (Y < H - margin)
    hit = (np.abs(disp[0] - motion[0]) < stride) & (np.abs(disp[1] - motion[1]) < stride)
    return float(hit[inside].mean())
