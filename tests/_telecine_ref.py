"""Inverse telecine restated in numpy, written from the text of include/papof.h (papof_field_metrics_tensor,
papof_weave_fields_tensor) and of match_fields' docstring (papteam_opticalflow_amd/tensors.py): the counts, the weave and the
host's rule that tests/test_telecine_cpu.py checks on scenes with known cadences and tests/test_gpu_telecine.py compares the
device's output with, byte for byte.  Everything behind the quantisation is integer, so the counts are exact."""
import numpy as np

from _interp_ref import as_f64, convert

FREE, PREV, NEXT, VIDEO = 0, 1, 2, 3
CELL_COLUMNS = 64


def quantise(a):
    """q of the header: 257 b of a byte; of a float 0 for a NaN, else clamp(rint(65535.0 v), 0, 65535) in fp64 -> int64"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.int64) * 257
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(65535.0 * a.astype(np.float64))
    return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 65535.0)).astype(np.int64)


def threshold_q(v):
    """a threshold in [0, 1] units as the integer the kernel takes"""
    return int(np.rint(65535.0 * float(v)))


def _m(b, a, c):
    outside = ((a > b) & (c > b)) | ((a < b) & (c < b))
    return np.where(outside, np.minimum(np.abs(a - b), np.abs(c - b)), 0)


def metrics_reference(fields, first=0, cell_rows=16, comb_q=threshold_q(10 / 255), diff_q=threshold_q(8 / 255)):
    """fields (T, Hf, W, C) uint8 / float32 / float64, T >= 3 -> counts (T, 3, ceil(Hf / cell_rows), ceil(W / 64)) int32"""
    Q = quantise(fields)
    T, Hf, W, C = Q.shape
    assert T >= 3 and first in (0, 1) and 1 <= cell_rows <= 64 and 1 <= C <= 4
    Gy, Gx = -(-Hf // cell_rows), -(-W // CELL_COLUMNS)
    out = np.zeros((T, 3, Gy, Gx), np.int32)
    cx = np.arange(W) // CELL_COLUMNS
    for t in range(1, T - 1):
        p = (t + first) & 1
        js = np.arange(1, Hf) if p == 0 else np.arange(0, Hf - 1)
        if len(js) == 0:
            continue
        ja, jc = (js - 1, js) if p == 0 else (js, js + 1)
        b = Q[t][js]
        am, cm, ap, cp = Q[t - 1][ja], Q[t - 1][jc], Q[t + 1][ja], Q[t + 1][jc]
        Mm, Mp = _m(b, am, cm).max(-1), _m(b, ap, cp).max(-1)
        nd = np.maximum(np.abs(ap - am), np.abs(cp - cm)).max(-1)
        for plane, hit in enumerate((Mp > Mm + comb_q, Mm > Mp + comb_q, nd > diff_q)):
            np.add.at(out[t, plane], ((js // cell_rows)[:, None], cx[None, :]), hit.astype(np.int32))
    return out


def weave_reference(fields, table, out_dtype=None):
    """fields (T, Hf, W, C), table (N, 2) -> (N, 2 Hf, W, C) of out_dtype (None: the fields'): row 2 j + r of frame n is row j
    of field table[n, r], loaded and stored as papof_deinterlace_tensor's kept lines"""
    fields, table = np.asarray(fields), np.asarray(table)
    T, Hf, W, C = fields.shape
    assert table.ndim == 2 and table.shape[1] == 2 and table.min() >= 0 and table.max() < T
    F = as_f64(fields)
    video = np.empty((len(table), 2 * Hf, W, C))
    video[:, 0::2] = F[table[:, 0]]
    video[:, 1::2] = F[table[:, 1]]
    return convert(video, fields.dtype if out_dtype is None else out_dtype)


def _ev(A, B, margin, dominance):
    best = 0
    for a, b in zip(A.ravel().tolist(), B.ravel().tolist()):
        if a > margin and dominance * b <= a:
            best = max(best, a - b)
    return best


def match_reference(counts, cell_rows=16, margin=None, dominance=3):
    """the host's rule on counts (T, 3, Gy, Gx) -> (votes (T,) uint8, links (T - 1,) bool, groups (N, 2) int64 [start,
    length], cadence, share)"""
    counts = np.asarray(counts).astype(np.int64)
    T = counts.shape[0]
    margin = cell_rows * 64 // 64 if margin is None else margin
    votes = np.zeros(T, np.uint8)
    for t in range(1, T - 1):
        A, B = counts[t, 0], counts[t, 1]
        ep, en, hi = _ev(A, B, margin, dominance), _ev(B, A, margin, dominance), max(A.max(), B.max())
        if ep > en:
            votes[t] = PREV
        elif en > ep:
            votes[t] = NEXT
        elif hi > margin:
            votes[t] = VIDEO
    links = np.array([votes[t] in (NEXT, FREE) and votes[t + 1] in (PREV, FREE) for t in range(T - 1)], bool)
    runs, start = [], 0
    for t in range(T - 1):
        if not links[t]:
            runs.append((start, t + 1 - start))
            start = t + 1
    runs.append((start, T - start))
    groups = []
    for s, L in runs:
        if L <= 3:
            groups.append((s, L))
            continue
        while L > 3:
            groups.append((s, 2))
            s, L = s + 2, L - 2
        groups.append((s, L))  # 2, or 3 when the run is odd
    groups = np.array(groups, np.int64).reshape(-1, 2)
    return (votes, links, groups) + cadence_reference(votes, groups)


def cadence_reference(votes, groups):
    T, L = len(votes), groups[:, 1].tolist()
    if (votes == FREE).all():
        return "static", 1.0
    if len(L) >= 2 and set(L) <= {2, 3} and all(a + b == 5 for a, b in zip(L, L[1:])):
        return "3:2", 1.0
    if set(L) == {2}:
        return "2:2", 1.0
    if set(L) == {1}:
        return "video", 1.0
    near = lambda i: [L[k] for k in (i - 1, i + 1) if 0 <= k < len(L)]  # noqa: E731
    film = sum(n for i, n in enumerate(L) if n in (2, 3) and 5 - n in near(i))
    return "mixed", max(film, sum(n for n in L if n == 2), sum(n for n in L if n == 1)) / T


def plan_reference(groups, first=0, orphans="bob"):
    """(table (M, 2), kept rows of groups, times (M,) float64, kinds (M,) uint8) of inverse_telecine: a group of 2 or 3 is
    woven from its first two fields -- the one of even parity gives the even rows --, a group of 1 is an orphan (its field
    twice in the table; its frame comes from the deinterlacer), left out by "drop" """
    table, keep, times, kinds = [], [], [], []
    for i, (s, n) in enumerate(np.asarray(groups).tolist()):
        if n == 1 and orphans == "drop":
            continue
        keep.append(i)
        if n == 1:
            table.append((s, s))
            times.append(float(s))
            kinds.append(1)
        else:
            pair = (s, s + 1) if (s + first) % 2 == 0 else (s + 1, s)
            table.append(pair)
            times.append((s + s + 1) / 2.0)
            kinds.append(0)
    return (np.array(table, np.int64).reshape(-1, 2), np.array(keep, np.int64), np.array(times, np.float64),
            np.array(kinds, np.uint8))
