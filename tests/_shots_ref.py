"""Shot boundaries restated in numpy, written from the text of include/papof.h (papof_cell_hist_tensor) and of the docstrings
of shot_distances and detect_cuts (papteam_opticalflow_amd/tensors.py): the histograms that tests/test_gpu_shots.py compares
the device's output with, byte for byte, and the host's rule that tests/test_shots_cpu.py checks on scenes with known cuts.
Everything behind the quantisation is integer, so the counts are exact; the rule is written pair by pair and region by region,
in loops, not as the package writes it."""
import numpy as np

CELL_COLUMNS = 64
BINS = (4, 8, 16, 32, 64)


def quantise(a):
    """q of the header: 257 b of a byte; of a float 0 for a NaN, else clamp(rint(65535.0 v), 0, 65535) in fp64 -> int64"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.int64) * 257
    v = a.astype(np.float64)
    out = np.zeros(v.shape, np.int64)
    ok = ~np.isnan(v)
    with np.errstate(over="ignore"):
        out[ok] = np.clip(np.rint(65535.0 * v[ok]), 0.0, 65535.0).astype(np.int64)
    return out


def luma_reference(frames):
    """frames (T, H, W, C) uint8 / float32 / float64, 1 <= C <= 4 -> L (T, H, W) int64 in 0 .. 65535"""
    Q = quantise(frames)
    C = Q.shape[3]
    assert 1 <= C <= 4
    if C <= 2:
        return Q[..., 0]
    return (77 * Q[..., 0] + 150 * Q[..., 1] + 29 * Q[..., 2]) >> 8


def hist_reference(frames, cell_rows=16, bins=16):
    """frames (T, H, W, C) -> hist (T, ceil(H / cell_rows), ceil(W / 64), bins) int32"""
    assert 1 <= cell_rows <= 64 and bins in BINS
    L = luma_reference(frames)
    T, H, W = L.shape
    b = (L * bins) >> 16
    assert b.min() >= 0 and b.max() < bins
    Gy, Gx = -(-H // cell_rows), -(-W // CELL_COLUMNS)
    out = np.zeros((T, Gy, Gx, bins), np.int32)
    cy = np.broadcast_to((np.arange(H) // cell_rows)[None, :, None], b.shape)
    cx = np.broadcast_to((np.arange(W) // CELL_COLUMNS)[None, None, :], b.shape)
    t = np.broadcast_to(np.arange(T)[:, None, None], b.shape)
    np.add.at(out, (t, cy, cx, b), 1)
    return out


def cell_pixels(H, W, cell_rows=16):
    """the pixel count of every cell (Gy, Gx)"""
    rows = np.bincount(np.arange(H) // cell_rows)
    cols = np.bincount(np.arange(W) // CELL_COLUMNS)
    return rows[:, None] * cols[None, :]


def distances_reference(hist, pool=(4, 2), step=1):
    """hist (T, Gy, Gx, bins) -> (T - step,) float64: per region of pool[0] x pool[1] cells sum |a - b| / (2 sum a), the
    numpy.median over the regions"""
    hist = np.asarray(hist).astype(np.int64)
    T, Gy, Gx, _ = hist.shape
    out = []
    for t in range(T - step):
        ds = []
        for y in range(0, Gy, pool[0]):
            for x in range(0, Gx, pool[1]):
                a = hist[t, y:y + pool[0], x:x + pool[1]].sum((0, 1))
                b = hist[t + step, y:y + pool[0], x:x + pool[1]].sum((0, 1))
                ds.append(float(np.abs(a - b).sum()) / float(2 * a.sum()))
        out.append(np.median(ds))
    return np.array(out, np.float64)


def cuts_reference(hist, floor=0.2, ratio=3.0, window=4, pool=(4, 2)):
    """the host's rule on hist -> (cuts, flashes, gradual, distances, ranges)"""
    hist = np.asarray(hist)
    T = hist.shape[0]
    d = distances_reference(hist, pool)
    cand = []
    for t in range(len(d)):
        others = [d[k] for k in range(t - window, t + window + 1) if k != t and 0 <= k < len(d)]
        base = np.median(others) if others else 0.0
        cand.append(bool(d[t] >= floor and d[t] >= ratio * base))
    runs, t = [], 0
    while t < len(cand):
        if cand[t]:
            e = t
            while e + 1 < len(cand) and cand[e + 1]:
                e += 1
            runs.append((t, e))
            t = e + 1
        else:
            t += 1
    cuts, flashes, gradual = [], [], []
    for s, e in runs:
        if e - s == 1 and distances_reference(hist, pool, 2)[s] < floor:
            flashes.append(s + 1)
            continue
        cuts += list(range(s, e + 1))
        if e - s >= 2:
            gradual.append((s, e))
    edges = [0] + [c + 1 for c in cuts] + [T]
    return cuts, flashes, gradual, d, list(zip(edges[:-1], edges[1:]))
