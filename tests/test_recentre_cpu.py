"""The re-centred block search without a GPU: the rule of include/papof.h (papof_match_recentre_tensor) as
tests/_recentre_ref.py restates it -- known answers on tiny grids and a candidate-by-candidate loop; the two properties that
follow from the rule; the key's width; the two scenes of a small object against a large pan, which neither the flat nor the
hierarchical search starts; every Python argument error raised before a launch; and the C ABI's refusals and workspace
sizes through ctypes."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _recentre_ref  # noqa: E402
from _hmatch_ref import hkey  # noqa: E402
from _match_ref import decimate, match_coarse, match_reference, object_scene  # noqa: E402
from _recentre_ref import (SCENES, cells_of, key_of, pan_object_scene, recentre_fields, recentre_level,  # noqa: E402
                           recentre_reference, shares, tile_origins)
from papteam_opticalflow_amd import capi, tensors  # noqa: E402


# ---- the rule
def _cl(v, n):
    return min(max(v, 0), n - 1)


def _loop_cost(a, b, x, y, dx, dy, patch, penalty):
    h, w, _ = a.shape
    c = penalty * (abs(dx) + abs(dy))
    for oy in range(-patch, patch + 1):
        for ox in range(-patch, patch + 1):
            c += int(np.abs(a[_cl(y + oy, h), _cl(x + ox, w)] - b[_cl(y + oy + dy, h), _cl(x + ox + dx, w)]).sum())
    return c


def _loop_recentre(a, b, dh, window, patch, penalty):
    """the rule tile by tile, cell by cell and candidate by candidate, in plain Python: (d (2, h, w), cost (h, w))"""
    h, w, _ = a.shape
    d, cost = np.zeros((2, h, w), np.int64), np.zeros((h, w), np.int64)
    for y0 in range(0, h, 8):
        for x0 in range(0, w, 32):
            cells = [(x, y) for y in range(y0, min(y0 + 8, h)) for x in range(x0, min(x0 + 32, w))]
            o = [sorted(int(dh[k, y, x]) for x, y in cells)[(len(cells) - 1) // 2] for k in (0, 1)]
            for x, y in cells:
                own = (int(dh[0, y, x]), int(dh[1, y, x]))
                cands = {(o[0] + ex, o[1] + ey) for ey in range(-window, window + 1) for ex in range(-window, window + 1)
                         if 0 <= x + o[0] + ex < w and 0 <= y + o[1] + ey < h} | {own}  # a set: a twin counts once
                best = min((_loop_cost(a, b, x, y, dx, dy, patch, penalty), dx * dx + dy * dy, dy, dx) for dx, dy in cands)
                d[0, y, x], d[1, y, x], cost[y, x] = best[3], best[2], best[0]
    return d, cost


def test_the_origin_is_the_lower_median_per_component():
    d = np.zeros((2, 1, 4), np.int64)
    d[0, 0], d[1, 0] = [3, 1, 2, 0], [-5, 7, 7, -6]   # n = 4: rank 1 of (0, 1, 2, 3) and of (-6, -5, 7, 7)
    assert tile_origins(d)[:, 0, 0].tolist() == [1, -5]
    d = np.zeros((2, 1, 5), np.int64)
    d[0, 0], d[1, 0] = [9, -2, 4, 4, 30], [0, 1, 0, 1, 1]   # n = 5: rank 2
    assert tile_origins(d)[:, 0, 0].tolist() == [4, 1]
    d = np.zeros((2, 8, 32), np.int64)
    d[0].flat[:128], d[1].flat[:127] = 6, -3   # a full tile of 256: rank 127 -- 128 sixes leave it at 0, 127 times -3 at 0 too
    assert tile_origins(d)[:, 0, 0].tolist() == [0, 0]
    d[0].flat[128], d[1].flat[127] = 6, -3     # 129 sixes: rank 127 is a 6; 128 times -3: rank 127 is the last -3
    assert tile_origins(d)[:, 0, 0].tolist() == [6, -3]


def test_the_last_tiles_are_clipped_to_the_grid():
    """9 x 33 cells: tiles of 8 x 32, 8 x 1, 1 x 32 and 1 x 1 cells, each with the median of its own cells alone"""
    d = np.zeros((2, 9, 33), np.int64)
    d[0, :8, :32], d[0, :8, 32], d[0, 8, :32], d[0, 8, 32] = 1, 2, 3, 4
    d[1, :8, 32] = [5, 1, 4, 2, 3, 9, 8, 7]    # n = 8: rank 3 of (1, 2, 3, 4, 5, 7, 8, 9)
    org = tile_origins(d)
    assert org.shape == (2, 2, 2) and org[0].tolist() == [[1, 2], [3, 4]] and org[1].tolist() == [[0, 4], [0, 0]]


@pytest.mark.parametrize("h,w,C,window,patch,penalty", [
    (8, 20, 3, 1, 1, 0), (9, 33, 1, 2, 2, 0), (5, 40, 2, 3, 1, 3), (17, 7, 3, 2, 1, 0),
])
def test_restatement_against_the_plain_loop(h, w, C, window, patch, penalty):
    """hand-made fields d_h (admissible, a few distinct vectors so that origins differ and twins occur), few grey levels: ties"""
    rng = np.random.default_rng(100 * h + w)
    a, b = (rng.integers(0, 4, (h, w, C)) * 60 for _ in range(2))
    yy, xx = np.mgrid[0:h, 0:w]
    dh = np.stack([np.clip(xx + rng.integers(-4, 5, (h, w)), 0, w - 1) - xx, np.clip(yy + rng.integers(-2, 3, (h, w)), 0, h - 1) - yy])
    d, cost, _ = recentre_level(a, b, dh, window, patch, penalty)
    ld, lcost = _loop_recentre(a, b, dh, window, patch, penalty)
    assert np.array_equal(d, ld) and np.array_equal(cost, lcost)


def test_a_twin_counts_once_and_an_inadmissible_window_keeps_d_h():
    """8 x 20 cells, one clipped tile of 160: d_h = (8, 0) on the 96 cells of x <= 11 and (0, 0) on the 64 others, so the
    origin is (8, 0) (rank 79 of 64 zeros and 96 eights); window 1: the candidates are dx = 7 .. 9, dy = -1 .. 1.
    Cells of x >= 13 reach no cell of the grid through the window (x + 7 >= 20) and keep d_h = (0, 0) with its cost; on the
    cells of x <= 11, d_h = (8, 0) is the window's own centre: a twin, which changes nothing."""
    rng = np.random.default_rng(12)
    a, b = (rng.integers(0, 256, (8, 20, 3)) for _ in range(2))
    dh = np.zeros((2, 8, 20), np.int64)
    dh[0, :, :12] = 8
    d, cost, org = recentre_level(a, b, dh, 1, 1)
    assert org[:, 0, 0].tolist() == [8, 0]
    assert (d[:, :, 13:] == 0).all()
    for x, y in ((13, 0), (19, 7), (16, 3)):
        assert cost[y, x] == _loop_cost(a, b, x, y, 0, 0, 1, 0)
    ld, lcost = _loop_recentre(a, b, dh, 1, 1, 0)
    assert np.array_equal(d, ld) and np.array_equal(cost, lcost)
    # the twin: with the d_h of one cell moved to another member of its window (the origin stays) nothing changes there
    only_window = np.zeros((2, 8, 20), np.int64)
    only_window[0, :, :12] = 8
    only_window[0, 0, 0] = 7
    d2, cost2, org2 = recentre_level(a, b, only_window, 1, 1)
    assert org2[:, 0, 0].tolist() == [8, 0]
    assert np.array_equal(d2[:, :, :12], d[:, :, :12]) and np.array_equal(cost2[:, :12], cost[:, :12])


def test_property_a_on_random_frames():
    """every cell's key is <= the key of the hierarchical result: the candidates hold d_h(p)"""
    rng = np.random.default_rng(21)
    for (H, W, C, stride, levels, patch, search, refine, window, penalty) in [
            (24, 70, 3, 1, 2, 1, 3, 1, 2, 0), (40, 90, 1, 2, 3, 2, 2, 2, 3, 2), (33, 35, 4, 1, 3, 1, 2, 3, 1, 0)]:
        qa, qb = (rng.integers(0, 256, (H, W, C)).astype(np.uint8) for _ in range(2))
        (d, cost), (dh, ch), _ = recentre_fields(qa, qb, stride, levels, patch, search, refine, window, penalty)
        k, kh = hkey(cost, d[0], d[1]), hkey(ch, dh[0], dh[1])
        assert (k <= kh).all() and (k < kh).any()
        disp, c = recentre_reference(qa[None], qb[None], stride, levels, patch, search, refine, window, penalty)
        assert np.array_equal(disp[0], stride * d) and np.array_equal(c[0], cost) and disp.dtype == np.float64
        assert np.array_equal(key_of(disp, c, stride)[0], k)


def test_property_b_a_zero_origin_gives_the_flat_search():
    """a static background and a 16 x 16 object that moves by (14, -8), within the flat reach of stride 2 * search 10: on the
    tiles whose origin is (0, 0), with window == search, the cells whose d_h lies within the window hold the flat result"""
    im1, im2, _, interior = object_scene(2, (14, -8), H=72, W=136, size=16, origin=(50, 30), background=(0, 0))
    kw = dict(stride=2, patch=2, search=10, penalty=0)
    (d, cost), (dh, _), org = recentre_fields(im1, im2, levels=2, refine=1, window=10, **kw)
    a, b = decimate(im1[None], 2)[0], decimate(im2[None], 2)[0]
    fd, fcost = match_coarse(a, b, 2, 10, 0)
    zero = np.repeat(np.repeat((org == 0).all(axis=0), 8, axis=0), 32, axis=1)[:36, :68]
    within = zero & (np.abs(dh) <= 10).all(axis=0)
    assert zero.mean() > 0.5 and within.sum() > 0.5 * zero.sum()
    assert np.array_equal(d[:, within], fd[:, within]) and np.array_equal(cost[within], fcost[within])
    obj = cells_of(interior, 2, 36, 68)
    assert obj.sum() >= 16 and (within & obj).any()
    assert ((d[0] == 7) & (d[1] == -4))[obj].all()


def test_the_key_holds_the_largest_accepted_parameters():
    """|d| <= 277 + 32 = 309 cells per component; dx^2 + dy^2 < 2^18; a cost below 2^26: 26 + 18 + 10 + 10 bits still"""
    assert tensors.MAX_WINDOW == _recentre_ref.MAX_WINDOW == 32 and (_recentre_ref.TILE_W, _recentre_ref.TILE_H) == (32, 8)
    d = tensors.MAX_SEARCH
    for _ in range(tensors.MAX_MATCH_LEVELS - 1):
        d = 2 * d + tensors.MAX_REFINE
    d += tensors.MAX_WINDOW
    assert d == 309
    worst = (2 * tensors.MAX_PATCH + 1) ** 2 * 4 * 255 + tensors.MAX_PENALTY * 2 * d
    assert worst == 40730130 < 1 << 26
    assert 2 * d * d == 190962 < 1 << 18 and d + 512 < 1 << 10 and -d + 512 >= 0
    assert hkey(worst, d, d) < (1 << 64) - 1
    for dx, dy in ((d, -d), (-d, d), (0, 0)):
        k = hkey(worst, dx, dy)
        assert (k >> 38, (k >> 20) & ((1 << 18) - 1), ((k >> 10) & 1023) - 512, (k & 1023) - 512) == (worst, dx * dx + dy * dy, dy, dx)


# ---- what it finds
@pytest.mark.parametrize("pan,rel,origin", SCENES)
def test_a_small_object_against_a_large_pan(pan, rel, origin):
    """135 x 240 frames of texture (seed 4), stride 2, patch 3, search 20, 3 levels, refine 1, window 20; a 24 x 24 object
    moves by pan + rel on a background that moves by pan.  The share of cells that hold the true vector exactly, background
    / object (the cells that _recentre_ref.pan_object_scene counts).  Measured:
        pan (70, 26), rel (34, -14):    flat 0.0000 / 0.0000   3 levels 0.9966 / 0.0000   re-centred 1.0000 / 1.0000
        pan (-60, 20), rel (-30, 16):   flat 0.0000 / 0.0000   3 levels 0.9877 / 0.0000   re-centred 0.9997 / 1.0000"""
    im1, im2, background, inside = pan_object_scene(4, pan, rel, origin)
    moved = (pan[0] + rel[0], pan[1] + rel[1])
    flat = match_reference(im1[None], im2[None], stride=2, patch=3, search=20)[0][0]
    (d, _), (dh, _), _ = recentre_fields(im1, im2, 2, 3, 3, 20, 1, 20)
    got = {name: shares(f, pan, moved, background, inside, 2) for name, f in (("flat", flat), ("3 levels", 2 * dh), ("re-centred", 2 * d))}
    print("pan %r, rel %r: %s" % (pan, rel, "   ".join("%s %.4f / %.4f" % (k, *v) for k, v in got.items())))
    assert cells_of(inside, 2, 67, 120).sum() == 64 and cells_of(background, 2, 67, 120).sum() > 1000
    assert got["3 levels"][1] <= 0.1
    assert got["re-centred"][0] >= 0.95 and got["re-centred"][1] >= 0.9


# ---- Python argument errors, before anything is launched (CPU tensors pass for device ones up to the handle)
torch = pytest.importorskip("torch")


@pytest.fixture
def stub(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")
    return calls


def _frames(B=3, H=64, W=96, C=3, dtype=torch.uint8):
    return torch.zeros((B, C, H, W), dtype=dtype)


_PREFIX = {"match_pairs": "", "match_video": "", "flow_pairs_ld": "match_", "flow_video_ld": "match_"}


@pytest.mark.parametrize("kw,exc", [
    (dict(levels=3, recentre=0), ValueError), (dict(levels=3, recentre=33), ValueError), (dict(levels=3, recentre=-1), ValueError),
    (dict(levels=3, recentre=20.0), ValueError), (dict(levels=3, recentre=True), ValueError), (dict(levels=3, recentre="20"), ValueError),
    (dict(recentre=20), ValueError), (dict(levels=1, recentre=1), ValueError),          # no hierarchy to centre on
    (dict(levels=5, recentre=20), ValueError), (dict(levels=3, refine=4, recentre=20), ValueError),
    (dict(levels=4, stride=8, recentre=20), ValueError),                                 # what the hierarchical call refuses
    (dict(levels=3, stride=2, recentre=20, frames=_frames(W=7)), ValueError),
    (dict(levels=2, recentre=20, frames=_frames(C=5)), ValueError),
    (dict(levels=2, recentre=20, frames=_frames(dtype=torch.int32)), TypeError),
    (dict(levels=2, recentre=20, frames=torch.zeros((3, 3, 64, 96), dtype=torch.uint8, device="meta")), ValueError),
])
@pytest.mark.parametrize("fn", ["match_pairs", "match_video", "flow_pairs_ld", "flow_video_ld"])
def test_argument_errors_before_any_launch(stub, kw, exc, fn):
    kw = dict(kw)
    fr = kw.pop("frames", _frames())
    for name in ("levels", "refine", "recentre"):
        if name in kw:
            kw[_PREFIX[fn] + name] = kw.pop(name)
    with pytest.raises(exc):
        if fn.endswith("video_ld") or fn == "match_video":
            getattr(tensors, fn)(fr, **kw)
        else:
            getattr(tensors, fn)(fr, fr, **kw)
    assert stub == []


def test_signatures():
    for fn in (tensors.match_pairs, tensors.match_video):
        p = inspect.signature(fn).parameters["recentre"]
        assert p.default is None and p.kind == inspect.Parameter.KEYWORD_ONLY
    for fn in (tensors.flow_pairs_ld, tensors.flow_video_ld):
        p = inspect.signature(fn).parameters["match_recentre"]
        assert p.default is None and p.kind == inspect.Parameter.KEYWORD_ONLY


@pytest.fixture
def launches(monkeypatch):
    """tensors._launch recorded instead of run: [(name, args, workspace)]"""
    calls = []
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: True)
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *args, workspace=None, timers=None: calls.append((name, args, workspace)))
    return calls


def test_none_makes_the_calls_of_before(launches):
    fr = _frames(B=2, H=33, W=49)
    tensors.match_pairs(fr, fr, stride=2, patch=3, search=20, recentre=None)
    tensors.match_pairs(fr, fr, stride=2, patch=3, search=20, levels=3, refine=2, recentre=None)
    assert [c[0] for c in launches] == ["papof_match_tensor", "papof_match_hier_tensor"]
    assert [a for a in launches[0][1] if isinstance(a, int)] == [2, 0, 33, 49, 3, 2, 3, 20, 0, 1]
    assert [a for a in launches[1][1] if isinstance(a, int)] == [2, 0, 33, 49, 3, 2, 3, 3, 20, 2, 0, 1]
    assert launches[1][2][:2] == ("papof_match_hier_workspace", (2, 0, 33, 49, 2, 3))


def test_a_window_makes_the_recentred_call(launches):
    fr = _frames(B=2, H=33, W=49)
    got = tensors.match_pairs(fr, fr, stride=2, patch=3, search=20, levels=3, refine=2, penalty=7, recentre=9, out_dtype=torch.float32)
    assert [c[0] for c in launches] == ["papof_match_recentre_tensor"]
    _, args, ws = launches[0]
    assert ws[:2] == ("papof_match_recentre_workspace", (2, 0, 33, 49, 2, 3))
    # n_pairs, sequence, height, width, c, stride, levels, patch, search, refine, window, penalty, both
    assert [a for a in args if isinstance(a, int)] == [2, 0, 33, 49, 3, 2, 3, 3, 20, 2, 9, 7, 1]
    assert tuple(got.disp_fw.shape) == (2, 2, 16, 24) and got.disp_fw.dtype == torch.float32
    del launches[:]
    got = tensors.match_video(fr, stride=4, levels=2, recentre=32, both=False)
    assert launches[0][0] == "papof_match_recentre_tensor" and launches[0][2][1] == (1, 1, 33, 49, 4, 2)
    assert tuple(got.disp_fw.shape) == (1, 2, 8, 12) and got.disp_bw is None


def test_the_bounds_themselves_reach_the_handle(stub, monkeypatch):
    monkeypatch.setattr(tensors, "_index", lambda dev: 0)
    fr = _frames(dtype=torch.float32, H=32, W=32)
    with pytest.raises(TypeError):  # the stubbed handle returns None: the call fails after the checks
        tensors.match_pairs(fr, fr, stride=4, levels=4, refine=3, patch=7, search=32, penalty=65535, recentre=32)
    with pytest.raises(TypeError):
        tensors.match_video(fr, stride=8, levels=2, recentre=1)
    with pytest.raises(TypeError):
        tensors.flow_video_ld(fr, 1, stride=1, match_levels=2, match_recentre=20)
    assert stub == [0, 0, 0]


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_F64, strides=(4096, 64, 1, 2048), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_H = ctypes.cast(_FAKE, ctypes.c_void_p)
_WS = ctypes.c_void_p(0x2000)


def _ref(d):
    return ctypes.byref(d) if d is not None else None


def _rec(lib, h=_H, n_pairs=2, sequence=1, frames="ok", frames2=None, height=32, width=48, c=3, stride=2, levels=3, patch=3,
         search=20, refine=1, window=20, penalty=0, both=1, disp="ok", cost="ok", ws=_WS, ws_bytes=1 << 30):
    fr = _t(capi.DTYPE_U8) if frames == "ok" else frames
    return lib.papof_match_recentre_tensor(h, n_pairs, sequence, _ref(fr), _ref(frames2), height, width, c, stride, levels, patch,
                                           search, refine, window, penalty, both, _ref(_t() if disp == "ok" else disp),
                                           _ref(_t(capi.DTYPE_F32) if cost == "ok" else cost), ws, ws_bytes, None)


_HIER = 4 * (3 * (16 * 24 + 8 * 12 + 4 * 6) + 4 * (8 * 12 + 4 * 6))   # 32 x 48, stride 2, 3 levels, 2 pairs in sequence
_NEED = _HIER + 4 * 4 * (16 * 24 + 2 * 1)                              # + d_h and 2 x 1 tile origins for 4 items


@pytest.mark.parametrize("kw", [
    dict(h=None), dict(n_pairs=0), dict(frames=None), dict(frames=_t(data=0)), dict(frames=_t(dtype=3)),
    dict(frames=_t(capi.DTYPE_U8, (-1, 64, 1, 2048))), dict(sequence=0), dict(sequence=0, frames2=_t(dtype=7)),
    dict(height=7), dict(width=7), dict(height=0), dict(height=1 << 16, width=1 << 15), dict(c=0), dict(c=5),
    dict(stride=0), dict(stride=3), dict(stride=16), dict(stride=-2),
    dict(levels=5), dict(levels=4, stride=8), dict(levels=3, stride=16), dict(levels=4, stride=4, height=31),
    dict(refine=0), dict(refine=4), dict(patch=0), dict(patch=8), dict(search=0), dict(search=33), dict(penalty=-1),
    dict(penalty=65536), dict(disp=None), dict(disp=_t(capi.DTYPE_U8)), dict(disp=_t(strides=(4096, 64, 1, 0))), dict(cost=None),
    dict(cost=_t(capi.DTYPE_U8)), dict(cost=_t(strides=(0, 64, 1, 0))),
    dict(ws=None), dict(ws=ctypes.c_void_p(0x2002)),
    dict(levels=1), dict(levels=0), dict(levels=-1),                    # the call's own: no hierarchy
    dict(window=0), dict(window=33), dict(window=-1),
    dict(ws_bytes=_NEED - 1), dict(ws_bytes=_HIER),                     # the hierarchical call's workspace is not enough
])
def test_c_abi_refusals(kw):
    assert _rec(_lib(), **kw) == -1


def test_c_abi_workspace():
    """the hierarchical call's bytes + one dword per level-0 cell and per 32 x 8 tile, for 2 n_pairs items"""
    lib = _lib()
    assert lib.papof_match_hier_workspace(2, 1, 32, 48, 2, 3) == _HIER
    assert lib.papof_match_recentre_workspace(2, 1, 32, 48, 2, 3) == _NEED
    for args, cells, tiles in (((2, 0, 33, 49, 2, 2), 16 * 24, 2), ((1, 1, 135, 240, 2, 3), 67 * 120, 9 * 4),
                               ((1, 1, 33, 70, 1, 2), 33 * 70, 5 * 3), ((3, 0, 32, 32, 4, 4), 64, 1)):
        assert lib.papof_match_recentre_workspace(*args) == lib.papof_match_hier_workspace(*args) + 4 * 2 * args[0] * (cells + tiles)
    for args in ((2, 1, 32, 48, 2, 1), (2, 1, 32, 48, 2, 0), (0, 1, 32, 48, 2, 2), (1, 1, 32, 48, 3, 2), (1, 1, 32, 48, 2, 5),
                 (1, 1, 32, 48, 8, 4), (1, 1, 31, 48, 4, 4), (1, 1, 1 << 15, 1 << 15, 1, 2)):
        assert lib.papof_match_recentre_workspace(*args) == -1, args


def test_the_symbols_are_listed_and_the_version_stays():
    lib = _lib()
    assert lib.papof_version() == 115
    assert {"papof_match_recentre_tensor", "papof_match_recentre_workspace"} <= set(capi.SYMBOLS)
    assert lib.papof_match_recentre_tensor.restype is ctypes.c_int and len(lib.papof_match_recentre_tensor.argtypes) == 21
    assert lib.papof_match_recentre_workspace.restype is ctypes.c_longlong
