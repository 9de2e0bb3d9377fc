"""The batched launch chain (csrc/batch.hip: flow_batch_device) at the shapes where its plan changes: a short table of named
cases, each with the decision of the code it sits on, and the chain's decisions restated in plain Python so that the table's
claims are checked on the CPU (tests/test_batch_shapes_cpu.py) before the GPU is asked (tests/test_gpu_batch_shapes.py).  The
chain falls back to single calls silently; a case that claims the chain must be one the restatement sends through it."""
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402

# ---- the chain's decisions, restated (csrc/api.hip: check_params, pyramid_plan; csrc/batch.hip: batch_applies, the sub-batch
# loops of flow_batch_host / flow_batch_tensor; csrc/sor.hip: tiny_shape; csrc/common.h: skew_dims)
DEFAULTS = dict(alpha=0.012, ratio=0.75, n_outer=7, n_outer_per_level=1, n_inner=1, n_sor=30, n_sor_per_level=3, omega=1.8,
                sor_mode=0, interpolation=0, noise_model=0)
BAND_ROWS, MAX_BANDS, MAX_SLOTS, NZ_LEVELS, TINY_MAX_CELLS, EXHAUSTIVE_PIXELS = 62, 16, 1024, 32, 8192, 4096
TINY_SHAPES = ((1, 16), (2, 16), (3, 12), (5, 8), (6, 8))  # (cells per tile, most waves) of k_sor_tiny's instances


def params_of(c):
    return {**DEFAULTS, **c.params}


def params_ok(P, levels):
    return (levels >= 1 and P["n_inner"] >= 1 and P["n_outer"] >= 1 and P["n_sor"] >= 1 and P["n_outer_per_level"] >= 0 and
            P["n_sor_per_level"] >= 0 and P["sor_mode"] in (0, 1, 2) and P["alpha"] > 0 and P["omega"] > 0 and
            P["interpolation"] in (0, 1) and P["noise_model"] in (0, 1))


def n_sor_max(c):
    P = params_of(c)
    return P["n_sor"] + (c.levels - 1) * P["n_sor_per_level"]


def bands(c):
    return -(-(c.H + n_sor_max(c) - 1) // BAND_ROWS)


def slots(c):
    P = params_of(c)
    return sum(P["n_outer"] + k * P["n_outer_per_level"] for k in range(c.levels))


def level_sizes(H, W, ratio, levels):
    """[(h, w)] of the pyramid: int(size * ratio^k) while every level is derived from level 0; deeper ones (ratio^k < 1/4)
    from level k - n at the WIDTH's rate (pyramid_plan)"""
    r = 0.75 if ratio > 0.98 or ratio < 0.4 else ratio
    n = int(math.log(0.25) / math.log(r))
    out = [(H, W)]
    for k in range(1, levels):
        sh, sw = out[0] if k <= n else out[k - n]
        rate = math.pow(r, k) if k <= n else math.pow(r, k) * W / sw
        out.append((int(sh * rate), int(sw * rate)))
    return out


def tiny_shape(H, W):
    """(cells per tile, waves) of the k_sor_tiny instance that solves an H x W plane, (0, 0) when none does"""
    if H < 1 or W < 1 or H * W > TINY_MAX_CELLS:
        return 0, 0
    for c, nw in TINY_SHAPES:
        qp = (-(-W // c) + 1) // 2
        if H * qp <= nw * 64 and (H + 2) * 2 * c * (qp + 2) * 16 <= 150 * 1024:
            return c, (H * qp + 63) // 64
    return 0, 0


def default_branches(P):
    return P["sor_mode"] == 0 and P["n_inner"] == 1 and P["interpolation"] == 0 and P["noise_model"] == 0


def expects_chain(c, B=None):
    B = c.B if B is None else B
    return bands(c) < MAX_BANDS and slots(c) <= MAX_SLOTS and c.C in (1, 3) and B >= 2 and default_branches(params_of(c))


def split(n_pairs, batch_max, fb):
    """the frame pairs per sub-batch: at most batch_max solver pairs each (forward-backward: two per frame pair), two pairs
    left for the last one rather than one where the bound allows"""
    max_b = (1 << 30) if batch_max is None else max(2, batch_max)
    if fb:
        max_b = max(1, max_b // 2)
    out, p0 = [], 0
    while p0 < n_pairs:
        nb = min(max_b, n_pairs - p0)
        if n_pairs - (p0 + nb) == 1 and nb > 2:
            nb -= 1
        out.append(nb)
        p0 += nb
    return out


def repeated_pair_is_rerun(c):
    """Does the chain run a pair of two identical frames again?  |Im1 - warpIm2| is 0 everywhere, no sample is valid, and
    the reference's estimate is then the constant 0.001: the guard is open.  On a level of at most 4096 pixels the chain looks
    at every pixel behind every update and proves just that; on a larger level it samples, finds no witness and cannot tell.
    The estimate behind the call's last update is never consulted."""
    P = params_of(c)
    sizes = level_sizes(c.H, c.W, P["ratio"], c.levels)
    consulted = [k for k in range(c.levels - 1, -1, -1) for _ in range(P["n_outer"] + k * P["n_outer_per_level"])][:-1]
    return any(sizes[k][0] * sizes[k][1] > EXHAUSTIVE_PIXELS for k in consulted)


def expected_stats(c, fb=False):
    """what papof_batch_stats must add over one call on the case: dict(chains, chain_pairs, singles, reruns).  A sub-batch of
    one forward-only pair is a single call; a repeated frame inside a chain is run again, once per frame pair, unless every
    consulted level is small enough for the exhaustive check."""
    if not expects_chain(c):
        return dict(chains=0, chain_pairs=0, singles=c.B, reruns=0)
    st, p0 = dict(chains=0, chain_pairs=0, singles=0, reruns=0), 0
    dup = c.dup if repeated_pair_is_rerun(c) else ()
    for nb in split(c.B, c.batch_max, fb):
        if nb == 1 and not fb:
            st["singles"] += 1
        else:
            st["chains"] += 1
            st["chain_pairs"] += 2 * nb if fb else nb
            st["reruns"] += sum(1 for p in dup if p0 <= p < p0 + nb)
        p0 += nb
    return st


# ---- the table
Case = namedtuple("Case", "name cls H W C levels params B sequence dtype chain nb batch_max fb init dup view out32 origin")
SMALL = dict(n_outer=2, n_outer_per_level=0, n_sor=5, n_sor_per_level=2)
CLASSES = ("few pixels", "one band / two bands", "last batched / first single", "level 0 tiny / just not", "tile borders",
           "deep pyramid", "slot limit", "remainders", "duplicates", "init flows", "dtypes and views", "seeded small draw")
MAY_RUN_SINGLY = ("first single", "slot limit, 1040")  # the only cases that may expect single calls: their `name` ends so

CASES = []


def _case(name, cls, H, W, C, levels, params, B, sequence=True, dtype="u8", chain=True, nb=None, batch_max=None, fb=False,
          init=None, dup=(), view=None, out32=False, origin=(40, 60)):
    assert cls in CLASSES, cls
    CASES.append(Case(name, cls, H, W, C, levels, dict(params), B, sequence, dtype, chain, nb, batch_max, fb, init, tuple(dup),
                      view, out32, origin))


# few pixels: tiny_cells = H * W, the guard's exhaustive check on every level, one-block kernels over the pairs
_case("1x9", "few pixels", 1, 9, 3, 1, SMALL, 2)
# (9 x 1 at a column where the clip moves: in its static background the golden pair's two frames agree in all but one of nine
# pixels, and neither the chain nor the single call can prove the guard open on such a pair)
_case("9x1", "few pixels", 9, 1, 1, 1, SMALL, 3, dtype="f64", origin=(132, 261))
_case("2x2", "few pixels", 2, 2, 1, 2, SMALL, 3, sequence=False)
_case("3x4", "few pixels", 3, 4, 3, 3, SMALL, 2, dtype="f64", fb=True)
# one band / two bands (n_sor = 30, one level): 70 columns are k_sor_tiny's, 260 columns the band kernel's first hand-off
_ONE = dict(n_outer=2, n_outer_per_level=0, n_sor=30, n_sor_per_level=0)
_case("33x70", "one band / two bands", 33, 70, 3, 1, _ONE, 3, nb=1)
_case("34x70", "one band / two bands", 34, 70, 3, 1, _ONE, 3, nb=2)
_case("33x260", "one band / two bands", 33, 260, 1, 1, _ONE, 3, nb=1)
_case("34x260", "one band / two bands", 34, 260, 1, 1, _ONE, 3, nb=2, fb=True)
# batch_applies' band limit: 15 bands run in the chain, 16 as single calls
_TALL = dict(n_outer=1, n_outer_per_level=0, n_sor=30, n_sor_per_level=0)
_case("901x24, last batched", "last batched / first single", 901, 24, 3, 2, _TALL, 2, nb=15)
_case("902x24, first single", "last batched / first single", 902, 24, 3, 2, _TALL, 2, nb=16, chain=False)
# level 0 solved by k_sor_tiny or just not (64 x 96 is the widest 64-row plane an instance holds): ST against SP strides; and
# H * W at kTinyMaxCells and just above it (neither level 0 is k_sor_tiny's, the coarser levels are): tiny_cells capped or not
for _h, _w, _lv in ((64, 96, 1), (64, 96, 3), (64, 97, 1), (64, 97, 3), (64, 128, 3), (64, 129, 3)):
    _case("%dx%d L%d" % (_h, _w, _lv), "level 0 tiny / just not", _h, _w, 3 if _lv == 3 else 1, _lv, SMALL, 2 + _lv // 3,
          sequence=_w % 2 == 0)
# border tiles of k_flow_system, k_im2feature_tiled, k_filter_hv_staged with blockIdx.y carrying the pair
for _i, (_h, _w) in enumerate(((31, 63), (32, 64), (33, 65), (33, 127), (31, 128), (32, 129))):
    _case("%dx%d" % (_h, _w), "tile borders", _h, _w, (3, 1)[_i % 2], 2, SMALL, 3, dtype=("u8", "f64")[_i // 3],
          fb=_i in (2, 3))
# deep pyramid (ratio 0.95): the non-zero flags are known up to 32 levels; levels beyond 27 chain through finer ones
_DEEP = dict(ratio=0.95, n_outer=1, n_outer_per_level=0, n_sor=3, n_sor_per_level=0)
for _lv in (32, 33, 40):
    _case("48x64 L%d" % _lv, "deep pyramid", 48, 64, 3, _lv, _DEEP, 2, fb=_lv == 33)
# kLapMaxSlots: 32 levels x 32 outer iterations = 1024 slots (no n_outer gives 1024 at 40 levels); 40 x 26 = 1040
_case("slot limit, 1024", "slot limit", 48, 64, 1, 32, dict(ratio=0.95, n_outer=32, n_outer_per_level=0, n_sor=1, n_sor_per_level=0), 2)
_case("slot limit, 1040", "slot limit", 48, 64, 1, 40, dict(ratio=0.95, n_outer=26, n_outer_per_level=0, n_sor=1, n_sor_per_level=0), 2,
      chain=False)
# sub-batches and their remainders: one video of 37 x 53 frames, forward-only and forward-backward
for _bm in (2, 3, 5):
    for _n in (3, 4, 5, 7):
        _case("37x53 max %d pairs %d" % (_bm, _n), "remainders", 37, 53, 3, 3, SMALL, _n, batch_max=_bm, fb=True)
# a repeated frame as the first, a middle and the last pair, and as the one-pair remainder of a bound of two
for _h, _w, _c in ((101, 173, 3), (37, 53, 1)):
    for _what, _dup, _bm in (("first", 0, None), ("middle", 1, None), ("last", 2, None), ("remainder", 2, 2)):
        _case("%dx%d repeated %s" % (_h, _w, _what), "duplicates", _h, _w, _c, 3, SMALL, 3, dup=(_dup,), batch_max=_bm, fb=True)
# the caller's initial flows at odd sizes
for _h, _w, _lv in ((37, 53, 7), (34, 70, 2)):
    for _init in ("per pair", "broadcast"):
        _case("%dx%d init %s" % (_h, _w, _init), "init flows", _h, _w, 3, _lv, SMALL, 3, init=_init, fb=True)
# frame dtypes, views read in place, float32 outputs
for _dt, _view, _o32 in (("u8", None, False), ("f32", None, False), ("f64", None, False), ("u8", "nchw", False),
                         ("f32", "gray", False), ("u8", None, True)):
    _case("45x67 %s%s%s" % (_dt, " " + _view if _view else "", " out32" if _o32 else ""), "dtypes and views", 45, 67,
          1 if _view == "gray" else 3, 3, SMALL, 3, dtype=_dt, view=_view, out32=_o32, sequence=_view != "nchw")


def _draw(seed=20261, n=12):
    """the generator of tests/test_gpu_fuzz_small.py (sizes, depth, schedule, gray, uint8) on the default branches, with a
    batch of 2..5 sequence or independent pairs"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 130))
        y0, x0 = int(rng.integers(0, 270 - h)), int(rng.integers(0, 480 - w))
        gray = rng.integers(0, 3) == 0
        levels = int(rng.integers(1, 6))
        while min(min(s) for s in level_sizes(h, w, 0.75, levels)) < 1:
            levels -= 1
        kw = dict(n_outer=int(rng.integers(1, 4)), n_outer_per_level=int(rng.integers(0, 2)), n_sor=int(rng.integers(1, 41)),
                  n_sor_per_level=int(rng.integers(0, 4)))
        u8 = rng.integers(0, 2) == 0
        _case("draw %d: %dx%dx%d L%d" % (i, h, w, 1 if gray else 3, levels), "seeded small draw", h, w, 1 if gray else 3, levels,
              kw, int(rng.integers(2, 6)), sequence=bool(rng.integers(0, 2)), dtype="u8" if u8 else "f64", origin=(y0, x0))


_draw()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- frames: crops of the committed 480 x 270 golden pair, made into a short video by rolls (test_gpu_batch.py: _video);
# the tall cases tile the crop vertically
_source = {}


def frame_u8(c, i, channels=None):
    """distinct frame i of the case's video, uint8 H x W x C (channels: of the storage a view is taken from)"""
    if not _source:
        _source[0], _source[1] = cases.load_frame_u8("480", 1), cases.load_frame_u8("480", 2)
    f = np.roll(_source[i % 2], (i // 2) * 3, axis=1)
    y0, x0 = c.origin
    f = np.tile(f, (-(-(y0 + c.H) // f.shape[0]), 1, 1))[y0:y0 + c.H, x0:x0 + c.W]
    return np.ascontiguousarray(f if (channels or c.C) == 3 else f[..., 1:2])


def frame_ids(c):
    """the distinct-frame number of every frame of the case's batch: a repeated pair (c.dup) has one frame twice"""
    ids, nxt = [], 0
    for p in range(c.B):
        if not c.sequence or p == 0:  # the pair's first frame (a video's: its predecessor's second)
            ids.append(nxt)
            nxt += 1
        ids.append(ids[-1] if p in c.dup else nxt)
        nxt += p not in c.dup
    return ids


def pair_ids(c):
    ids = frame_ids(c)
    return [(ids[p], ids[p + 1]) if c.sequence else (ids[2 * p], ids[2 * p + 1]) for p in range(c.B)]


def as_dtype(f, dtype):
    """a uint8 frame as the case's dtype: float32 = uint8 / 255 rounded to float32, float64 = uint8 / 255"""
    if dtype == "u8":
        return f
    return (f.astype(np.float32) / np.float32(255)) if dtype == "f32" else f.astype(np.float64) / 255.0


def smooth_init(B, H, W, per_pair=True):
    """a smooth flow (B, 2, H, W) of a pixel or two, different for every pair, exactly representable in float32"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, 2, H, W))
    for p in range(B):
        q = p if per_pair else 0
        out[p, 0] = 1.5 * np.sin(2 * np.pi * x / W + 0.7 * q) + 0.5 * np.cos(2 * np.pi * y / H) + 0.25 * q
        out[p, 1] = -1.0 * np.cos(2 * np.pi * (x + y) / (W + H) + 0.3 * q) + 0.125 * q
    return out.astype(np.float32)
