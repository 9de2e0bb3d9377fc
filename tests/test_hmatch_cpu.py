"""Hierarchical block matching without a GPU: the rule of include/papof.h (papof_match_hier_tensor) as tests/_hmatch_ref.py
restates it, against a candidate-by-candidate loop; the key's width; the pans that the flat search cannot reach; the
composition matcher -> densify -> hole fill -> the oracle's coarse-to-fine call; the known loss on a small object; every
Python argument error raised before a launch; and the C ABI's refusals and workspace sizes through ctypes."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _hmatch_ref  # noqa: E402
from _hmatch_ref import exact_share, hkey, hmatch_levels, hmatch_reference, wide_pan_scene  # noqa: E402
from _init_ref import coarse2fine_init  # noqa: E402
from _inpaint_ref import fill_reference  # noqa: E402
from _libs import OracleLib  # noqa: E402
from _match_ref import decimate, densify_reference, epe, match_reference, object_scene  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import MAX_MATCH_LEVELS, MAX_REFINE, MAX_TOP_STRIDE  # noqa: E402  (the feature under test)


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


def _loop_hier(qa, qb, stride, levels, patch, search, refine, penalty):
    """the rule level by level, cell by cell and candidate by candidate, in plain Python: (d_0 (2, h, w), cost_0 (h, w))"""
    d1 = None
    for l in range(levels - 1, -1, -1):
        a, b = decimate(qa[None], stride << l)[0], decimate(qb[None], stride << l)[0]
        h, w, _ = a.shape
        d, cost = np.zeros((2, h, w), np.int64), np.zeros((h, w), np.int64)
        for y in range(h):
            for x in range(w):
                if d1 is None:
                    cands = [(dx, dy) for dy in range(-search, search + 1) for dx in range(-search, search + 1)]
                else:
                    h1, w1 = d1.shape[1:]
                    px, py = min(x >> 1, w1 - 1), min(y >> 1, h1 - 1)
                    nx, ny = _cl(px + (1 if x & 1 else -1), w1), _cl(py + (1 if y & 1 else -1), h1)
                    preds = [(2 * int(d1[0, Y, X]), 2 * int(d1[1, Y, X])) for Y, X in ((py, px), (py, nx), (ny, px), (ny, nx))]
                    cands = [(qx + ex, qy + ey) for qx, qy in preds + [(0, 0)]
                             for ey in range(-refine, refine + 1) for ex in range(-refine, refine + 1)]
                best = None
                for dx, dy in cands:
                    if not (0 <= x + dx < w and 0 <= y + dy < h):
                        continue
                    key = (_loop_cost(a, b, x, y, dx, dy, patch, penalty), dx * dx + dy * dy, dy, dx)
                    if best is None or key < best:
                        best = key
                d[0, y, x], d[1, y, x], cost[y, x] = best[3], best[2], best[0]
        d1 = d
    return d1, cost


@pytest.mark.parametrize("H,W,C,stride,levels,patch,search,refine,penalty", [
    (7, 9, 3, 1, 3, 1, 2, 1, 0),      # grids 7 x 9, 3 x 4, 1 x 2: odd at every level
    (4, 5, 1, 1, 3, 2, 3, 2, 0),      # 4 x 5, 2 x 2, 1 x 1: a top level of one cell
    (11, 13, 2, 1, 4, 1, 1, 1, 0),    # 11 x 13, 5 x 6, 2 x 3, 1 x 1
    (10, 15, 4, 2, 2, 1, 2, 3, 4),    # 5 x 7, 2 x 3 at stride 2, the widest refinement, a penalty
    (9, 10, 3, 1, 2, 3, 2, 1, 0),     # a window larger than the top grid
])
def test_restatement_against_the_plain_loop(H, W, C, stride, levels, patch, search, refine, penalty):
    """clamped parents and windows, admissibility and the key on grids of a few cells, few grey levels: many ties"""
    rng = np.random.default_rng(H * 10 + W)
    qa, qb = ((rng.integers(0, 4, (H, W, C)) * 60).astype(np.uint8) for _ in range(2))
    d, cost = hmatch_levels(qa, qb, stride, levels, patch, search, refine, penalty)[0]
    ld, lcost = _loop_hier(qa, qb, stride, levels, patch, search, refine, penalty)
    assert np.array_equal(d, ld) and np.array_equal(cost, lcost)
    disp, c = hmatch_reference(qa[None], qb[None], stride, levels, patch, search, refine, penalty)
    assert np.array_equal(disp[0], stride * ld) and np.array_equal(c[0], lcost) and disp.dtype == np.float64


def test_levels_1_is_the_flat_rule():
    rng = np.random.default_rng(5)
    a, b = (rng.integers(0, 256, (2, 21, 30, 3)).astype(np.uint8) for _ in range(2))
    flat = match_reference(a, b, stride=2, patch=2, search=4, penalty=1)
    hier = hmatch_reference(a, b, stride=2, levels=1, patch=2, search=4, refine=3, penalty=1)
    assert np.array_equal(flat[0], hier[0]) and np.array_equal(flat[1], hier[1])


def test_the_key_holds_the_largest_accepted_parameters():
    """|d| <= 32 * 8 + 3 * 7 = 277 cells per component at level 0 of 4 levels; a cost below 2^26; 26 + 18 + 10 + 10 bits"""
    assert (_hmatch_ref.MAX_LEVELS, _hmatch_ref.MAX_REFINE, _hmatch_ref.MAX_TOP_STRIDE) == \
        (MAX_MATCH_LEVELS, MAX_REFINE, MAX_TOP_STRIDE) == (4, 3, 32)
    d = tensors.MAX_SEARCH
    for _ in range(MAX_MATCH_LEVELS - 1):
        d = 2 * d + MAX_REFINE
    assert d == 277 == 32 * 8 + 3 * 7
    worst = (2 * tensors.MAX_PATCH + 1) ** 2 * 4 * 255 + tensors.MAX_PENALTY * 2 * d
    assert worst == 15 * 15 * 4 * 255 + 65535 * 554 and worst < 1 << 26
    assert 2 * d * d < 1 << 18 and d + 512 < 1 << 10 and -d + 512 >= 0
    assert hkey(worst, d, d) < 1 << 64  # an unsigned 64-bit key, and below the all-ones start of the search
    k = hkey(np.array([worst, 0]), np.array([d, -d]), np.array([-d, d]))  # the arrays' key is the integers', unsigned
    assert k.dtype == np.uint64 and [int(v) for v in k] == [hkey(worst, d, -d), hkey(0, -d, d)] and k[1] < k[0]
    for dx, dy in ((d, -d), (-d, d), (0, 0), (-1, 1)):  # the fields do not overlap
        k = hkey(worst, dx, dy)
        assert (k >> 38, (k >> 20) & ((1 << 18) - 1), ((k >> 10) & 1023) - 512, (k & 1023) - 512) == (worst, dx * dx + dy * dy, dy, dx)
    assert hkey(3, 0, 0) < hkey(3, 0, -1) < hkey(3, -1, 0) < hkey(3, 1, 0) < hkey(3, 0, 1) < hkey(3, -1, -1) < hkey(4, 0, 0)


# ---- what it finds
_PANS = [(90, 30), (-70, 26), (120, -40), (28, 9)]


@pytest.fixture(scope="module")
def pans():
    """the four pans at the defaults (stride 2, patch 3, search 20, refine 1): {motion: (scene, {levels: forward (disp, cost)})}"""
    out = {}
    for motion in _PANS:
        scene = wide_pan_scene(3, motion)
        out[motion] = (scene, {levels: hmatch_reference(scene[0][None], scene[1][None], levels=levels) for levels in (1, 3)})
    return out


@pytest.mark.parametrize("motion", _PANS)
def test_the_pans_beyond_the_flat_reach(pans, motion):
    """135 x 240 frames of texture (seed 3), stride 2, patch 3, search 20, refine 1: the share of cells with the exact
    displacement (a component that is no whole number of cells: either cell next to it) among the cells whose target stays 8 px
    inside the frame.  Measured, flat / levels 3: (90, 30) 0.0000 / 0.9991, (-70, 26) 0.0000 / 0.9978, (120, -40) 0.0000 /
    1.0000, (28, 9) 0.9997 / 0.9973."""
    scene, fields = pans[motion]
    share = {levels: exact_share(fields[levels][0][0], motion, 2, scene[0].shape[:2]) for levels in (1, 3)}
    print("pan %r: flat %.4f, levels 3 %.4f" % (motion, share[1], share[3]))
    assert share[3] >= 0.99
    if max(abs(motion[0]), abs(motion[1])) > 40:
        assert share[1] <= 0.01


@pytest.fixture(scope="module")
def orc():
    return OracleLib()


def test_the_oracle_started_from_the_hierarchical_fields(orc, pans):
    """The (90, 30) pan through match_init's rule (densify, hole fill) and the oracle's coarse-to-fine call with 2 levels.
    Measured on the pixels that stay in view: cold 5 levels 94.41 px; with the prior of levels 3 0.0486 px (reliable
    share of the forward field 0.515: the rest of the frame leaves the view)."""
    (im1, im2, truth, interior), fields = pans[(90, 30)]
    a, b = im1 / 255.0, im2 / 255.0
    vx, vy, _ = coarse2fine_init(orc, a, b, 5)
    cold = epe(vx, vy, truth, interior)
    print("pan (90, 30): cold 5 levels %.3f px" % cold)
    assert cold > 10.0
    fw, cf = fields[3]
    bw, _ = hmatch_reference(im2[None], im1[None], levels=3)
    flow, hole = densify_reference(fw, bw, cf, im1.shape[:2], 2)
    init_fw = fill_reference(flow.transpose(0, 2, 3, 1), hole, tensors.RELAX)[0]
    vx, vy, _ = coarse2fine_init(orc, a, b, 2, init_fw)
    e = epe(vx, vy, truth, interior)
    print("pan (90, 30): prior of levels 3 + 2 levels %.4f px; reliable %.3f" % (e, 1.0 - float(hole.mean())))
    assert e < 0.5


def test_the_known_loss_on_a_small_object():
    """object_scene(1, (34, -14)): a 24 x 24 object on a background that moves by (1, 0).  The top level's window (56 px at
    stride 8) sees the background, and the lower levels only refine what it found.  Measured, the share of the object's
    interior cells with the exact displacement: flat 1.0000, levels 3 0.0000 (of 64 cells) -- the loss that keeps levels=1 the
    default; recorded, not a merit."""
    im1, im2, _, interior = object_scene(1, (34, -14))
    cells = interior[::2, ::2][:67, :120] & interior[1::2, 1::2][:67, :120]
    share = {}
    for levels in (1, 3):
        d = hmatch_reference(im1[None], im2[None], levels=levels)[0][0]
        share[levels] = float(((d[0] == 34) & (d[1] == -14))[cells].mean())
    print("object (34, -14): flat %.4f, levels 3 %.4f of %d interior cells" % (share[1], share[3], int(cells.sum())))
    assert share[1] > 0.9  # the premise: the flat search has it


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
    (dict(levels=0), ValueError), (dict(levels=5), ValueError), (dict(levels=2.0), ValueError), (dict(levels=True), ValueError),
    (dict(levels=None), ValueError), (dict(levels="2"), ValueError),
    (dict(refine=0), ValueError), (dict(refine=4), ValueError), (dict(refine=1.0), ValueError), (dict(refine=False), ValueError),
    (dict(levels=1, refine=0), ValueError),                                     # checked although not used
    (dict(levels=4, stride=8), ValueError), (dict(levels=3, stride=16), ValueError),   # a top stride of 64; no stride at all
    (dict(levels=4, stride=4, frames=_frames(H=31)), ValueError),            # smaller than one cell of the top level (32)
    (dict(levels=3, stride=2, frames=_frames(W=7)), ValueError),
    (dict(levels=2, patch=8), ValueError), (dict(levels=2, search=33), ValueError), (dict(levels=2, penalty=-1), ValueError),
    (dict(levels=2, frames=_frames(C=5)), ValueError), (dict(levels=2, frames=_frames(dtype=torch.int32)), TypeError),
    (dict(levels=2, out_dtype=torch.uint8), TypeError),
    (dict(levels=2, frames=torch.zeros((3, 3, 64, 96), dtype=torch.uint8, device="meta")), ValueError),
])
@pytest.mark.parametrize("fn", ["match_pairs", "match_video", "flow_pairs_ld", "flow_video_ld"])
def test_argument_errors_before_any_launch(stub, kw, exc, fn):
    kw = dict(kw)
    fr = kw.pop("frames", _frames())
    for name in ("levels", "refine"):
        if name in kw:
            kw[_PREFIX[fn] + name] = kw.pop(name)
    with pytest.raises(exc):
        if fn.endswith("video") or fn == "flow_video_ld":
            getattr(tensors, fn)(fr, **kw)
        else:
            getattr(tensors, fn)(fr, fr, **kw)
    assert stub == []


def test_signatures():
    for fn in (tensors.match_pairs, tensors.match_video):
        ps = inspect.signature(fn).parameters
        assert (ps["levels"].default, ps["refine"].default) == (1, 1)
        assert ps["levels"].kind == ps["refine"].kind == inspect.Parameter.KEYWORD_ONLY
    for fn in (tensors.flow_pairs_ld, tensors.flow_video_ld):
        ps = inspect.signature(fn).parameters
        assert (ps["match_levels"].default, ps["match_refine"].default) == (1, 1)
        assert ps["match_levels"].kind == inspect.Parameter.KEYWORD_ONLY
    assert tensors.STRIDES == (1, 2, 4, 8)


@pytest.fixture
def launches(monkeypatch):
    """tensors._launch recorded instead of run: [(name, args, workspace)]"""
    calls = []
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: True)
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *args, workspace=None, timers=None: calls.append((name, args, workspace)))
    return calls


def test_levels_1_makes_the_call_of_before(launches):
    fr = _frames(B=2, H=33, W=49)
    for kw in (dict(), dict(levels=1), dict(levels=1, refine=3)):
        del launches[:]
        got = tensors.match_pairs(fr, fr, stride=2, patch=3, search=20, **kw)
        assert [c[0] for c in launches] == ["papof_match_tensor"]
        name, args, ws = launches[0]
        assert ws[:2] == ("papof_match_workspace", (2, 0, 33, 49, 2))
        assert [a for a in args if isinstance(a, int)] == [2, 0, 33, 49, 3, 2, 3, 20, 0, 1]
        assert tuple(got.disp_fw.shape) == (2, 2, 16, 24) and tuple(got.cost_bw.shape) == (2, 16, 24)
    del launches[:]
    tensors.match_video(fr, stride=1, both=False)
    assert [c[0] for c in launches] == ["papof_match_tensor"] and launches[0][2][1] == (1, 1, 33, 49, 1)


def test_levels_above_1_make_the_hierarchical_call(launches):
    fr = _frames(B=2, H=33, W=49)
    got = tensors.match_pairs(fr, fr, stride=2, patch=3, search=20, levels=3, refine=2, penalty=7, out_dtype=torch.float32)
    assert [c[0] for c in launches] == ["papof_match_hier_tensor"]
    name, args, ws = launches[0]
    assert ws[:2] == ("papof_match_hier_workspace", (2, 0, 33, 49, 2, 3))
    # n_pairs, sequence, height, width, c, stride, levels, patch, search, refine, penalty, both
    assert [a for a in args if isinstance(a, int)] == [2, 0, 33, 49, 3, 2, 3, 3, 20, 2, 7, 1]
    assert tuple(got.disp_fw.shape) == (2, 2, 16, 24) and got.disp_fw.dtype == torch.float32
    del launches[:]
    got = tensors.match_video(fr, stride=8, levels=3, both=False)
    assert launches[0][0] == "papof_match_hier_tensor" and launches[0][2][1] == (1, 1, 33, 49, 8, 3)
    assert tuple(got.disp_fw.shape) == (1, 2, 4, 6) and got.disp_bw is None


def test_the_bounds_themselves_reach_the_handle(stub, monkeypatch):
    monkeypatch.setattr(tensors, "_index", lambda dev: 0)
    fr = _frames(dtype=torch.float32, H=32, W=32)
    with pytest.raises(TypeError):  # the stubbed handle returns None: the call fails after the checks
        tensors.match_pairs(fr, fr, stride=4, levels=4, refine=3, patch=7, search=32, penalty=65535)
    with pytest.raises(TypeError):
        tensors.match_video(fr, stride=8, levels=3, refine=1)
    with pytest.raises(TypeError):
        tensors.flow_video_ld(fr, 1, stride=1, match_levels=4, match_refine=2)
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


def _hier(lib, h=_H, n_pairs=2, sequence=1, frames="ok", frames2=None, height=32, width=48, c=3, stride=2, levels=3, patch=3,
          search=20, refine=1, penalty=0, both=1, disp="ok", cost="ok", ws=_WS, ws_bytes=1 << 30):
    fr = _t(capi.DTYPE_U8) if frames == "ok" else frames
    return lib.papof_match_hier_tensor(h, n_pairs, sequence, _ref(fr), _ref(frames2), height, width, c, stride, levels, patch,
                                       search, refine, penalty, both, _ref(_t() if disp == "ok" else disp),
                                       _ref(_t(capi.DTYPE_F32) if cost == "ok" else cost), ws, ws_bytes, None)


_NEED = 4 * (3 * (16 * 24 + 8 * 12 + 4 * 6) + 4 * (8 * 12 + 4 * 6))


@pytest.mark.parametrize("kw", [
    dict(h=None), dict(n_pairs=0), dict(frames=None), dict(frames=_t(data=0)), dict(frames=_t(dtype=3)),
    dict(frames=_t(capi.DTYPE_U8, (-1, 64, 1, 2048))), dict(sequence=0), dict(sequence=0, frames2=_t(dtype=7)),
    dict(height=7), dict(width=7), dict(height=0), dict(height=1 << 16, width=1 << 15), dict(c=0), dict(c=5),
    dict(stride=0), dict(stride=3), dict(stride=16), dict(stride=-2),
    dict(levels=0), dict(levels=5), dict(levels=-1), dict(levels=4, stride=8), dict(levels=3, stride=16),
    dict(levels=4, stride=4, height=31), dict(levels=4, stride=4, width=31),
    dict(refine=0), dict(refine=4), dict(refine=-1), dict(levels=1, refine=0), dict(levels=1, refine=4),
    dict(patch=0), dict(patch=8), dict(search=0), dict(search=33), dict(penalty=-1), dict(penalty=65536),
    dict(disp=None), dict(disp=_t(capi.DTYPE_U8)), dict(disp=_t(strides=(4096, 64, 1, 0))), dict(cost=None),
    dict(cost=_t(capi.DTYPE_U8)), dict(cost=_t(strides=(0, 64, 1, 0))),
    dict(ws=None), dict(ws=ctypes.c_void_p(0x2002)), dict(ws_bytes=_NEED - 1),
    dict(levels=1, ws_bytes=3 * 16 * 24 * 4 - 1), dict(levels=1, patch=8), dict(levels=1, disp=None),
])
def test_c_abi_hier_refusals(kw):
    assert _hier(_lib(), **kw) == -1


def test_c_abi_hier_workspace():
    """the packed frames of every level, and one dword per cell and item (2 n_pairs) of every level above 0"""
    lib = _lib()
    assert lib.papof_match_hier_workspace(2, 1, 32, 48, 2, 3) == _NEED
    assert lib.papof_match_hier_workspace(2, 0, 33, 49, 2, 2) == 4 * (4 * (16 * 24 + 8 * 12) + 4 * 8 * 12)
    assert lib.papof_match_hier_workspace(1, 1, 135, 240, 8, 3) == 4 * (2 * (16 * 30 + 8 * 15 + 4 * 7) + 2 * (8 * 15 + 4 * 7))
    assert lib.papof_match_hier_workspace(1, 1, 39, 79, 2, 3) == 4 * (2 * (19 * 39 + 9 * 19 + 4 * 9) + 2 * (9 * 19 + 4 * 9))
    assert lib.papof_match_hier_workspace(3, 0, 32, 32, 4, 4) == 4 * (6 * (64 + 16 + 4 + 1) + 6 * (16 + 4 + 1))
    for args in ((2, 1, 32, 48, 2), (2, 0, 33, 49, 2), (1, 1, 135, 240, 8), (5, 1, 8, 8, 8)):  # levels 1: the flat call's
        assert lib.papof_match_hier_workspace(*args, 1) == lib.papof_match_workspace(*args) > 0
    for args in ((0, 1, 32, 48, 2, 2), (1, 1, 0, 48, 2, 2), (1, 1, 32, 48, 3, 2), (1, 1, 32, 48, 2, 0), (1, 1, 32, 48, 2, 5),
                 (1, 1, 32, 48, 8, 4), (1, 1, 32, 48, 16, 2), (1, 1, 31, 48, 4, 4), (1, 1, 32, 15, 4, 3), (1, 1, 1 << 15, 1 << 15, 1, 2)):
        assert lib.papof_match_hier_workspace(*args) == -1, args


def test_the_flat_symbols_and_the_version_stay():
    lib = _lib()
    assert lib.papof_version() == 115
    assert {"papof_match_tensor", "papof_match_workspace", "papof_match_hier_tensor", "papof_match_hier_workspace"} <= set(capi.SYMBOLS)
    assert lib.papof_match_workspace(2, 1, 32, 48, 2) == 3 * 16 * 24 * 4
