"""Re-centred block search (include/papof.h: papof_match_recentre_tensor) restated in numpy integers -- the rule that
tests/test_recentre_cpu.py checks with known answers and tests/test_gpu_recentre.py compares the device's outputs with, byte
for byte -- and the scene of a small object that moves against a large pan.

    disp, cost = recentre_reference(A, B, stride=2, levels=3, patch=3, search=20, refine=1, window=20)   # as hmatch_reference

Only the test suite and tools/recentre_probe.py import this module."""
import numpy as np

from _hmatch_ref import hkey, hmatch_levels
from _match_ref import decimate, quantise, texture

TILE_W, TILE_H = 32, 8  # the rule's tiles of level-0 cells, from (0, 0); the last ones clipped to the grid
MAX_WINDOW = 32


def tile_origins(d):
    """d (2, h, w) in cells -> (2, ceil(h / 8), ceil(w / 32)): per tile and component the lower median of its in-grid
    cells, the value of rank (n - 1) // 2 in ascending order"""
    _, h, w = d.shape
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    out = np.zeros((2, ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            t = d[:, j * TILE_H:(j + 1) * TILE_H, i * TILE_W:(i + 1) * TILE_W].reshape(2, -1)
            out[:, j, i] = np.sort(t, axis=1)[:, (t.shape[1] - 1) // 2]
    return out


def _window_keys(a, b, y0, y1, x0, x1, o, window, patch, penalty):
    """the smallest key over the admissible o + e, |ex|, |ey| <= window, for the cells [y0, y1) x [x0, x1): (th, tw) uint64,
    all ones where no candidate is admissible"""
    h, w, _ = a.shape
    P, n = patch, 2 * patch + 1
    ys, xs = np.arange(y0 - P, y1 + P), np.arange(x0 - P, x1 + P)
    ap = a[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
    yy, xx = np.mgrid[y0:y1, x0:x1]
    best = np.full((y1 - y0, x1 - x0), np.iinfo(np.uint64).max)
    dxs = o[0] + np.arange(-window, window + 1)
    dxs = dxs[(x1 - 1 + dxs >= 0) & (x0 + dxs < w)]  # the others are inadmissible for every cell
    if dxs.size == 0:
        return best
    cols = np.clip(xs[None, :] + dxs[:, None], 0, w - 1)  # (ndx, tw + 2 P)
    col_ok = (xx[None] + dxs[:, None, None] >= 0) & (xx[None] + dxs[:, None, None] < w)
    for dy in range(o[1] - window, o[1] + window + 1):
        row_ok = (yy + dy >= 0) & (yy + dy < h)
        if not row_ok.any():
            continue
        D = np.abs(ap[:, None] - b[np.clip(ys + dy, 0, h - 1)][:, cols]).sum(axis=3)  # (th + 2 P, ndx, tw + 2 P)
        S = np.zeros((D.shape[0] + 1, D.shape[1], D.shape[2] + 1), np.int64)
        S[1:, :, 1:] = D.cumsum(0).cumsum(2)
        sad = (S[n:, :, n:] - S[:-n, :, n:] - S[n:, :, :-n] + S[:-n, :, :-n]).transpose(1, 0, 2)  # (ndx, th, tw)
        dx = dxs[:, None, None]
        key = hkey(sad + penalty * (np.abs(dx) + abs(dy)), np.broadcast_to(dx, sad.shape), np.full(sad.shape, dy))
        key = np.where(col_ok & row_ok[None], key, np.iinfo(np.uint64).max)
        best = np.minimum(best, key.min(axis=0))
    return best


def _own_keys(a, b, dh, patch, penalty):
    """the key of every cell's own candidate d_h(p): (h, w) uint64"""
    h, w, _ = a.shape
    yy, xx = np.mgrid[0:h, 0:w]
    off = np.arange(-patch, patch + 1)
    wy, wx = yy[:, :, None, None] + off[None, None, :, None], xx[:, :, None, None] + off[None, None, None, :]
    aw = a[np.clip(wy, 0, h - 1), np.clip(wx, 0, w - 1)]
    bw = b[np.clip(wy + dh[1][:, :, None, None], 0, h - 1), np.clip(wx + dh[0][:, :, None, None], 0, w - 1)]
    cost = np.abs(aw - bw).sum(axis=(2, 3, 4)) + penalty * (np.abs(dh[0]) + np.abs(dh[1]))
    return hkey(cost, dh[0], dh[1])


def recentre_level(a, b, dh, window, patch, penalty=0):
    """a, b (h, w, C) int64 frames of level 0, dh (2, h, w) the hierarchy's field in cells -> (d (2, h, w), cost (h, w),
    origins (2, ty, tx)): per cell the smallest key among o(tile) + e, |e| <= window, admissible, and d_h(p)"""
    assert 1 <= window <= MAX_WINDOW
    h, w, _ = a.shape
    org = tile_origins(dh)
    best = _own_keys(a, b, dh, patch, penalty)  # (d_h is admissible by the hierarchy's rule; a twin in the window has its key)
    # tiles that share an origin are searched together, over their bounding box: the cells of other tiles in it are dropped
    tiles = {}
    for j in range(org.shape[1]):
        for i in range(org.shape[2]):
            tiles.setdefault((int(org[0, j, i]), int(org[1, j, i])), []).append((j, i))
    for o, members in tiles.items():
        js, is_ = [j for j, _ in members], [i for _, i in members]
        y0, y1 = min(js) * TILE_H, min((max(js) + 1) * TILE_H, h)
        x0, x1 = min(is_) * TILE_W, min((max(is_) + 1) * TILE_W, w)
        keys = _window_keys(a, b, y0, y1, x0, x1, o, window, patch, penalty)
        for j, i in members:
            ya, yb, xa, xb = j * TILE_H, min((j + 1) * TILE_H, h), i * TILE_W, min((i + 1) * TILE_W, w)
            best[ya:yb, xa:xb] = np.minimum(best[ya:yb, xa:xb], keys[ya - y0:yb - y0, xa - x0:xb - x0])
    lo = np.uint64(1023)
    return (np.stack([(best & lo).astype(np.int64) - 512, ((best >> np.uint64(10)) & lo).astype(np.int64) - 512]),
            (best >> np.uint64(38)).astype(np.int64), org)


def recentre_fields(qa, qb, stride, levels, patch, search, refine, window, penalty=0):
    """qa, qb (H, W, C) uint8 -> ((d, cost) re-centred, (d_h, cost_h) of the hierarchy, origins), all in level-0 cells"""
    assert levels >= 2
    dh, ch = hmatch_levels(qa, qb, stride, levels, patch, search, refine, penalty)[0]
    a, b = decimate(qa[None], stride)[0], decimate(qb[None], stride)[0]
    d, cost, org = recentre_level(a, b, dh, window, patch, penalty)
    return (d, cost), (dh, ch), org


def recentre_reference(A, B, stride=2, levels=3, patch=3, search=20, refine=1, window=20, penalty=0, out_dtype=np.float64):
    """A, B (n, H, W, C) uint8 / float32 / float64 -> (disp (n, 2, h, w) = stride * d, cost (n, h, w)) of out_dtype"""
    qa, qb = quantise(A), quantise(B)
    got = [recentre_fields(qa[i], qb[i], stride, levels, patch, search, refine, window, penalty)[0] for i in range(qa.shape[0])]
    return (np.stack([stride * d for d, _ in got]).astype(out_dtype), np.stack([c for _, c in got]).astype(out_dtype))


def key_of(disp, cost, stride):
    """the keys of fields as the calls return them (disp = stride * d): (..., h, w) uint64"""
    d = np.asarray(disp, np.int64) // stride
    return hkey(np.asarray(cost, np.int64), d[..., 0, :, :], d[..., 1, :, :])


# ---- a small object that moves against a large pan
def pan_object_scene(seed, pan, rel, origin, H=135, W=240, size=24, pad=160):
    """_match_ref.object_scene with a pad of `pad` pixels: the background, one texture, moves by `pan`; the size x size
    object, a texture of its own with its top left corner at `origin` (x, y) in im1, moves by pan + rel.
    -> (im1, im2 (H, W, 3) uint8, background (H, W) bool, inside (H, W) bool) -- the pixels a share is counted on:
    background pixels whose target stays 8 px inside im2 and that lie 10 px away from the object in im1, from where the object
    covers their target (origin + rel) and from where it lands (origin + pan + rel); object pixels 4 px inside it."""
    px, py = pan
    assert max(abs(px), abs(py)) <= pad
    rng = np.random.default_rng(seed)
    bg = texture(rng, H + 2 * pad, W + 2 * pad)
    obj = texture(rng, size, size)
    im1 = bg[pad:pad + H, pad:pad + W].copy()
    im2 = bg[pad - py:pad - py + H, pad - px:pad - px + W].copy()
    ox, oy = origin
    mx, my = px + rel[0], py + rel[1]
    assert 0 <= ox and ox + size <= W and 0 <= oy and oy + size <= H
    assert 0 <= ox + mx and ox + mx + size <= W and 0 <= oy + my and oy + my + size <= H
    im1[oy:oy + size, ox:ox + size] = obj
    im2[oy + my:oy + my + size, ox + mx:ox + mx + size] = obj
    yy, xx = np.mgrid[0:H, 0:W]
    background = (xx + px >= 8) & (xx + px < W - 8) & (yy + py >= 8) & (yy + py < H - 8)
    for cx, cy in ((ox, oy), (ox + rel[0], oy + rel[1]), (ox + mx, oy + my)):
        background &= ~((xx >= cx - 10) & (xx < cx + size + 10) & (yy >= cy - 10) & (yy < cy + size + 10))
    inside = (xx >= ox + 4) & (xx < ox + size - 4) & (yy >= oy + 4) & (yy < oy + size - 4)
    return im1, im2, background, inside


def cells_of(pixels, stride, h, w):
    """the cells of the h x w grid all of whose stride x stride pixels are set"""
    p = pixels[:h * stride, :w * stride].reshape(h, stride, w, stride)
    return p.all(axis=(1, 3))


def shares(disp, motion_bg, motion_obj, background, inside, stride):
    """(share of the background cells, share of the object cells) that hold the true vector exactly; disp (2, h, w) pixels"""
    _, h, w = disp.shape
    out = []
    for where, m in ((background, motion_bg), (inside, motion_obj)):
        c = cells_of(where, stride, h, w)
        out.append(float(((disp[0] == m[0]) & (disp[1] == m[1]))[c].mean()))
    return tuple(out)


SCENES = [  # (pan, rel, origin) of the issue's table, texture seed 4
    ((70, 26), (34, -14), (100, 60)),
    ((-60, 20), (-30, 16), (150, 40)),
]
