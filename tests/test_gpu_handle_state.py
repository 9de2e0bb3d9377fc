"""A call's result must not depend on what the handle's memory held.

Every flow call carves its buffers out of one reused arena, and two more blocks (the host path's staging block, the tensor
path's one-pair scratch) live between calls.  The solver relies on zeros it finds in that memory (csrc/sor.hip: padding of the
skewed planes, the (du, dv) tails, the grouped kernel's halo rows; csrc/api.hip: the coarsest level's flow), and every clear
that is too short shows only when the bytes underneath are not zero.  So here ONE handle lives long, is filled with NaN by the
test aid papof_test_poison between calls (0x7FF8DEAD7FF8DEAD: a quiet NaN as fp64, two NaNs as fp32, no zero byte) or is left
with the leftovers of other calls, and every result must have the BYTES (`.tobytes()`: the sign of a zero counts) of the same
call on a fresh handle -- and of the oracle wherever the oracle is the bit-for-bit truth (the exact-order solve, whole calls of
the default Laplacian-noise path; the tripping pair of the guard and the Gaussian-mixture branch are not: test_gpu_parity.py).

Order: a. the stages (a NaN that is read lands in the returned array and feeds no address), b. whole calls on every route,
c. order walks of whole calls on one handle, d. the aid itself.  Nothing is larger than 70 x 120 x 3 (the stage cases of
tests/golden/cases.py that are used whole are 68 x 120 x 5 feature planes)."""
import ctypes
import functools

import numpy as np
import pytest

import cases
from _sor_shapes import TINY_SHAPES
from test_gpu_call_routes import C, H, LEVELS, W, _device_call, _f64, _pair
from test_gpu_parity import TOL_GM_PARA, TOL_GM_SOLVE, _tiny_scale_pair
from test_gpu_sor_kernels import HYPERPLANE, KNOBS, SMALL, TINY, _case, _handle

pytestmark = pytest.mark.gpu

try:  # ahead of the library, as in test_gpu_call_routes.py; only the tensor routes need it
    import torch
except ImportError:
    torch = None

PATTERN = 0x7FF8DEAD7FF8DEAD
NAMES = ("vx", "vy", "warpI2")
BIG = (70, 120)  # level 0 (8400 cells) is above k_sor_tiny's limit, the coarser levels are below it


def _fresh_handle():
    from papteam_opticalflow_amd import Papof
    return Papof(0)


def _poison(g):
    return g.test_poison(PATTERN)


def _arrays(r):
    """a result as a tuple of arrays: tuples / lists as they are, the dicts of tests/golden/cases.py in key order"""
    if isinstance(r, dict):
        return tuple(np.asarray(r[k]) for k in sorted(r))
    return tuple(np.asarray(x) for x in r)


def _same(got, want, what):
    got, want = _arrays(got), _arrays(want)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, "%s: output %d has shape %r, not %r" % (what, i, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
            bad = g.view(np.uint64) != w.view(np.uint64) if g.dtype == np.float64 and w.dtype == np.float64 else g != w
            raise AssertionError("%s: output %d differs in %d of %d values (%d of them not finite)"
                                 % (what, i, int(bad.sum()), g.size, int((~np.isfinite(g)).sum())))


def _frozen(r):
    r = tuple(np.array(x) for x in _arrays(r))  # copies: result arrays may be recycled page-locked blocks
    for x in r:
        x.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _crop8(h, w):
    """the top-left h x w crop of the committed 240 pair, uint8"""
    a, b = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    return np.ascontiguousarray(a[:h, :w]), np.ascontiguousarray(b[:h, :w])


def _big_call(g):
    """a larger call of another kind than any stage: the whole call on the 70 x 120 x 3 crop, 3 levels"""
    a, b = _crop8(*BIG)
    g.coarse2fine_flow_u8(a, b, 3)


@pytest.fixture(scope="module")
def long_handle():
    """the long-lived default handle: every test of this module that takes it finds what the ones before left behind"""
    g = _fresh_handle()
    yield g
    g.close()


def _three_ways(long, run, what, make_fresh=_fresh_handle):
    """run(handle) on a fresh handle, on the long-lived one after poison, and there again after a larger call of another
    kind and poison: the same bytes.  Returns the fresh handle's result."""
    fresh = make_fresh()
    try:
        r0 = _frozen(run(fresh))
    finally:
        fresh.close()
    _poison(long)
    _same(run(long), r0, what + ", after poison")
    _big_call(long)
    _poison(long)
    _same(run(long), r0, what + ", after a larger call and poison")
    return r0


# ======================================================================================================================
# a. stages after poison
# ======================================================================================================================
POISON_SOR = [(63, 64, 1), (124, 3, 2), (42, 75, 5), (42, 75, 36), (1, 300, 3)]
assert set(POISON_SOR) <= set(SMALL)


@pytest.fixture(scope="module", params=KNOBS, ids=lambda k: "+".join("%s=%s" % (n[10:], v) for n, v in k.items()) or "TINY=0")
def off(request):
    """a long-lived handle with k_sor_tiny switched off, alone and with each knob that forces a hyperplane kernel"""
    env = dict(request.param, PAPOF_SOR_TINY="0")
    g = _handle(env)
    yield g, request.param, env
    g.close()


def _last_kind(g, h, w, n_sor):
    e = g.last_sor_solves()[-1]
    assert (e["h"], e["w"], e["n_sor"]) == (h, w, n_sor), e  # the log's last entry is this solve
    return e["kind"]


def _check_hyperplane_kind(kind, knobs, n_sor):
    assert kind in HYPERPLANE, kind
    if knobs.get("PAPOF_SOR_FUSE") == "2" and n_sor >= 2:
        assert kind == 1
    if knobs.get("PAPOF_SOR_FUSE") == "1":
        assert kind != 1
    if "PAPOF_SOR_GROUP" in knobs and n_sor >= 2:
        assert kind == 2
    if "PAPOF_SOR_XLANE" in knobs:
        assert kind == 0
    if n_sor < 2:
        assert kind == 0


@pytest.mark.parametrize("h,w,n_sor", POISON_SOR)
def test_sor_hyperplane_kernels_after_poison(off, oracle, h, w, n_sor):
    g, knobs, env = off
    planes, want = _case(oracle, h, w, n_sor)
    kinds = []

    def run(x):
        r = x.sor(*planes, n_sor, mode=0)
        kinds.append(_last_kind(x, h, w, n_sor))
        return r

    r0 = _three_ways(g, run, "gpu.sor %dx%d x %d sweeps" % (h, w, n_sor), lambda: _handle(env))
    _same(r0, want, "gpu.sor %dx%d x %d sweeps on a fresh handle vs the oracle" % (h, w, n_sor))
    assert len(set(kinds)) == 1, kinds  # the same kernel all three times
    _check_hyperplane_kind(kinds[0], knobs, n_sor)
    print("knobs %r %dx%d x %d: kind %d" % (knobs, h, w, n_sor, kinds[0]))


TINY_EDGES = [t for t in TINY_SHAPES if t[1] in ((22, 131), (32, 63), (798, 3))]  # ragged last tile, odd number of tiles
assert len(TINY_EDGES) == 3                                                        # per row, LDS at the cap


@pytest.mark.parametrize("c,hw,waves,what", TINY_EDGES)
def test_sor_tiny_kernel_after_poison(long_handle, oracle, c, hw, waves, what):
    from papteam_opticalflow_amd import capi
    assert capi.sor_tiny_shape(*hw) == (c, waves), what
    h, w, n_sor = hw[0], hw[1], 7
    planes, want = _case(oracle, h, w, n_sor)
    kinds = []

    def run(x):
        r = x.sor(*planes, n_sor, mode=0)
        kinds.append(_last_kind(x, h, w, n_sor))
        return r

    r0 = _three_ways(long_handle, run, "gpu.sor %dx%d (k_sor_tiny<%d>, %s)" % (h, w, c, what))
    _same(r0, want, "gpu.sor %dx%d on a fresh handle vs the oracle" % (h, w))
    assert kinds == [TINY] * 3, kinds


_mode_cache = {}


def _mode_case(oracle, h, w, n_sor, mode, omega):
    key = (h, w, n_sor, mode, omega)
    if key not in _mode_cache:
        rng = np.random.default_rng(3 * h + w)
        planes = (rng.uniform(0.5, 50.0, (h, w)), rng.uniform(-0.02, 0.02, (h, w)), rng.uniform(0, 0.05, (h, w)),
                  rng.uniform(0, 0.05, (h, w)), rng.uniform(-0.01, 0.01, (h, w)), rng.uniform(-0.01, 0.01, (h, w)))
        want = oracle.sor(*planes, n_sor, omega=omega, mode=mode)
        for a in planes + want:
            a.setflags(write=False)
        _mode_cache[key] = (planes, want)
    return _mode_cache[key]


@pytest.mark.parametrize("mode,omega", [(1, 1.8), (2, 1.0)])
@pytest.mark.parametrize("h,w,n_sor", [(70, 51, 5), (6, 1, 4)])
def test_sor_red_black_and_jacobi_after_poison(long_handle, oracle, mode, omega, h, w, n_sor):
    """the row-major planes of the blocked kernels alternate between two pairs of unknowns"""
    planes, want = _mode_case(oracle, h, w, n_sor, mode, omega)
    kinds = []

    def run(x):
        r = x.sor(*planes, n_sor, omega=omega, mode=mode)
        kinds.append(_last_kind(x, h, w, n_sor))
        return r

    r0 = _three_ways(long_handle, run, "gpu.sor mode %d %dx%d" % (mode, h, w))
    print("mode %d %dx%d: max-abs to the oracle in the same mode %.3e"
          % (mode, h, w, max(np.abs(r0[0] - want[0]).max(), np.abs(r0[1] - want[1]).max())))
    _same(r0, want, "gpu.sor mode %d %dx%d on a fresh handle vs the oracle in the same mode" % (mode, h, w))
    assert kinds == [3 if mode == 1 else 4] * 3, kinds


SOLVE_SEQUENCE = [(42, 75, 36), (42, 75, 2), (20, 75, 5)]  # qt, rt, hp, nb all change: old real cells lie where new padding is


@pytest.mark.parametrize("poison", [False, True], ids=["leftovers", "poison"])
def test_sor_solve_sequence_on_one_handle(off, oracle, poison):
    g, knobs, _ = off
    for h, w, n_sor in SOLVE_SEQUENCE:
        if poison:
            _poison(g)
        planes, want = _case(oracle, h, w, n_sor)
        got = g.sor(*planes, n_sor, mode=0)
        _check_hyperplane_kind(_last_kind(g, h, w, n_sor), knobs, n_sor)
        _same(got, want, "%dx%d x %d sweeps in a sequence of solves, knobs %r" % (h, w, n_sor, knobs))


@pytest.mark.parametrize("poison", [False, True], ids=["leftovers", "poison"])
def test_sor_solve_sequence_on_the_default_handle(long_handle, oracle, poison):
    for h, w, n_sor in SOLVE_SEQUENCE:
        if poison:
            _poison(long_handle)
        planes, want = _case(oracle, h, w, n_sor)
        got = long_handle.sor(*planes, n_sor, mode=0)
        assert _last_kind(long_handle, h, w, n_sor) == TINY
        _same(got, want, "%dx%d x %d sweeps in a sequence of solves" % (h, w, n_sor))


@functools.lru_cache(maxsize=None)
def _features(h=BIG[0], w=BIG[1]):
    """5-channel feature planes of the 240 pair, cropped (the inputs of tests/golden/cases.py's stage cases, smaller)"""
    a, b = cases.load_pair("240")
    return np.ascontiguousarray(cases.features5(a)[:h, :w]), np.ascontiguousarray(cases.features5(b)[:h, :w])


@pytest.mark.parametrize("shape", [(3, 4), (1, 9), (68, 120)])
def test_linear_system_after_poison(long_handle, shape):
    h, w = shape
    f1, f2 = _features(h, w)
    rng = np.random.default_rng(5)
    u = cases.smooth_field(rng, 135, 240, 1.5)[:h, :w].copy()
    v = cases.smooth_field(rng, 135, 240, 1.5)[:h, :w].copy()
    _three_ways(long_handle, lambda g: g.linear_system(f1, f2, u, v), "linear_system %dx%d" % shape)


def _stage_pyramid(g):
    a = _f64(_crop8(*BIG)[0])
    return g.pyramid(a, 0.75, 5) + g.pyramid(np.ascontiguousarray(a[:40, :50]), 0.5, 3)


def _stage_warps(g):
    f1, f2 = _features()
    a, b = (_f64(x) for x in _crop8(*BIG))
    vx, vy = cases._flow(11, BIG[0], BIG[1], 2.5)
    return (g.warpFL(f1, f2, vx, vy), g.warpFL(a, b, vx * 3, vy * 3), g.bicubic_warp(a, b, vx, vy),
            g.bicubic_warp(a, b, vx * 4, vy * 4))


def _stage_getdxs(g):
    f1, f2 = _features()
    return g.getDxs(f1, f2) + g.getDxs(np.ascontiguousarray(f1[:3, :4]), np.ascontiguousarray(f2[:3, :4]))


STAGES = {
    "laplacian": cases.CASES["stage_laplacian"],
    "smoothflow_sor": cases.CASES["stage_smoothflow"],  # includes n_inner = 2
    "smoothflow_lapguard": cases.CASES["stage_lapguard"],  # the exact pass's LapPara decides the result
    "pyramid": _stage_pyramid,
    "warpFL_and_bicubic_warp": _stage_warps,
    "getDxs": _stage_getdxs,
}


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_stage_after_poison(long_handle, stage):
    _three_ways(long_handle, STAGES[stage], stage)


GM_TOL = {"gm_est": TOL_GM_PARA, "gm_para": TOL_GM_PARA, "gm_warp": TOL_GM_SOLVE, "gm_u": TOL_GM_SOLVE, "gm_v": TOL_GM_SOLVE}


def test_branch_stages_after_poison(long_handle):
    """smoothflow_sor_opts: the in-loop bicubic warp (bytes) and the Gaussian-mixture model.  The mixture model is not
    bit-compatible with the oracle; whether the library is with ITSELF is found out first, from two fresh handles: if they
    agree in every byte, so must the poisoned handle; else the tolerances of test_gpu_parity.py hold (parameters: relative)."""
    run = cases.CASES["stage_branches"]
    other = _fresh_handle()
    try:
        r_other = {k: np.array(v) for k, v in run(other).items()}
    finally:
        other.close()
    keys = sorted(r_other)
    results = []

    def run_logged(g):
        results.append({k: np.array(v) for k, v in run(g).items()})
        return {k: v for k, v in results[-1].items() if k not in GM_TOL}

    _three_ways(long_handle, run_logged, "stage_branches, bicubic part")
    fresh = results[0]
    reproducible = all(fresh[k].tobytes() == r_other[k].tobytes() for k in keys)
    print("Gaussian-mixture stage: two fresh handles give %s" % ("the same bytes" if reproducible else "different bytes"))
    for r, what in zip(results[1:], ("after poison", "after a larger call and poison")):
        for k in GM_TOL:
            assert np.all(np.isfinite(r[k])), (k, what)
            if reproducible:
                _same((r[k],), (fresh[k],), "stage_branches/%s %s" % (k, what))
            elif k in ("gm_est", "gm_para"):
                assert float(np.abs(r[k] / fresh[k] - 1).max()) <= GM_TOL[k], (k, what)
            else:
                assert float(np.abs(r[k] - fresh[k]).max()) <= GM_TOL[k], (k, what)


# ======================================================================================================================
# whole-call cases: the oracle's bytes and a fresh handle's, computed once per case
# ======================================================================================================================
class Case:
    """one whole call: a frame pair (uint8 or float64), a level count, solver parameters"""

    def __init__(self, name, a, b, levels, oracle_bits=True, **solver):
        self.name, self.a, self.b, self.levels, self.oracle_bits, self.solver = name, a, b, levels, oracle_bits, solver

    def params(self):
        from papteam_opticalflow_amd import default_params
        return default_params(**self.solver) if self.solver else None

    def run(self, g):
        if self.a.dtype == np.uint8:
            return g.coarse2fine_flow_u8(self.a, self.b, self.levels, self.params())[:3]
        return g.coarse2fine_flow(self.a, self.b, self.levels, self.params())[:3]

    def oracle(self, orc):
        p = orc.default_params()
        for k, v in self.solver.items():
            setattr(p, k, v)
        a, b = (_f64(x) if x.dtype == np.uint8 else x for x in (self.a, self.b))
        return orc.coarse2fine_flow(a, b, self.levels, p)[:3]


@functools.lru_cache(maxsize=None)
def _cases():
    small, big = _pair(), _crop8(*BIG)
    gray = tuple(np.ascontiguousarray(x[..., 1:2]) for x in big)
    tiny = tuple(np.ascontiguousarray(x[:BIG[0], :BIG[1]]) for x in _tiny_scale_pair())
    out = [Case("small_L3", small[0], small[1], 3), Case("small_L7", small[0], small[1], 7),
           Case("small_L3_sor5", small[0], small[1], 3, n_sor=5, n_sor_per_level=0),
           Case("small_L3_bicubic", small[0], small[1], 3, interpolation=1),
           # the mixture model: not the oracle's bits (test_gpu_parity.py: TOL_GM_*)
           Case("small_L3_gmixture", small[0], small[1], 3, oracle_bits=False, noise_model=1),
           Case("big_L3", big[0], big[1], 3), Case("gray_big_L3", gray[0], gray[1], 3),
           Case("big_f64_L3", _f64(big[0]), _f64(big[1]), 3),
           # trips the guard; within 1e-9 of the oracle, not its bits (test_gpu_parity.py)
           Case("tiny_scale_L3", tiny[0], tiny[1], 3, oracle_bits=False),
           Case("duplicate_L3", big[0], big[0], 3)]
    return {c.name: c for c in out}


_fresh_cache = {}


def _fresh(name, oracle):
    """the result of case `name` on a fresh handle (checked against the oracle's bytes where they are the truth): once"""
    if name not in _fresh_cache:
        case = _cases()[name]
        g = _fresh_handle()
        try:
            r = _frozen(case.run(g))
            kinds = [e["kind"] for e in g.last_sor_solves()]
        finally:
            g.close()
        if case.oracle_bits:
            _same(r, case.oracle(oracle), "%s on a fresh handle vs the oracle" % name)
        print("%s: solver kinds %s" % (name, sorted(set(kinds))))
        _fresh_cache[name] = r
    return _fresh_cache[name]


# ======================================================================================================================
# b. whole calls after poison, every route
# ======================================================================================================================
def _route_host_u8(g, a, b, levels):
    return g.coarse2fine_flow_u8(a, b, levels)[:3]


def _route_host_f64(g, a, b, levels):
    return g.coarse2fine_flow(_f64(a), _f64(b), levels)[:3]


def _route_device_u8(g, a, b, levels):
    return _device_call(g, a, b, levels, True)


def _route_device_f64(g, a, b, levels):
    return _device_call(g, _f64(a), _f64(b), levels, False)


def _route_batch(g, a, b, levels):
    out, _ = g.flow_batch([a, b, a, b, a, b], levels, None, sequence=False)
    assert len(out) == 3
    _same(out[1], out[0], "flow_batch: pair 1 vs pair 0")
    _same(out[2], out[0], "flow_batch: pair 2 vs pair 0")
    return out[0]


ROUTES = {"host_u8": _route_host_u8, "host_f64": _route_host_f64, "device_u8": _route_device_u8,
          "device_f64": _route_device_f64, "flow_batch_3_pairs": _route_batch}


# every route with the streams overlapped; the host routes on one stream as well
ROUTE_PARAMS = [(r, True) for r in sorted(ROUTES)] + [("host_f64", False), ("host_u8", False)]


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("route,overlap", ROUTE_PARAMS, ids=["%s-%s" % (r, "overlap" if o else "one_stream") for r, o in ROUTE_PARAMS])
def test_whole_call_after_poison(long_handle, oracle, route, overlap, levels):
    want = _fresh("small_L%d" % levels, oracle)
    a, b = _pair()
    long_handle.set_stream_overlap(overlap)
    try:
        _poison(long_handle)
        _same(ROUTES[route](long_handle, a, b, levels), want, "%s, %d levels, after poison" % (route, levels))
        _same(ROUTES[route](long_handle, a, b, levels), want, "%s, %d levels, again" % (route, levels))
    finally:
        long_handle.set_stream_overlap(True)


@pytest.mark.parametrize("case", ["small_L3_bicubic", "small_L3_gmixture"])
def test_whole_call_other_branches_after_poison(long_handle, oracle, case):
    want = _fresh(case, oracle)
    run = _cases()[case].run
    if case.endswith("gmixture"):
        other = _fresh_handle()
        try:
            reproducible = all(x.tobytes() == y.tobytes() for x, y in zip(run(other), want))
        finally:
            other.close()
        print("Gaussian-mixture whole call: two fresh handles give %s" % ("the same bytes" if reproducible else "different bytes"))
    for what in ("after poison", "after a larger call and poison"):
        if what != "after poison":
            _big_call(long_handle)
        _poison(long_handle)
        got = run(long_handle)
        if case.endswith("gmixture") and not reproducible:
            for name, x, y in zip(NAMES, got, want):
                assert np.all(np.isfinite(x)) and float(np.abs(x - y).max()) <= TOL_GM_SOLVE, (name, what)
        else:
            _same(got, want, "%s %s" % (case, what))


@pytest.mark.parametrize("levels", LEVELS)
def test_sequences_after_poison(long_handle, oracle, levels):
    """after the aid the next push primes again: the kept pyramid lived in the arena"""
    want = _fresh("small_L%d" % levels, oracle)
    g, (a, b) = long_handle, _pair()
    g.seq_reset()
    _poison(g)
    assert g.seq_push(a, levels) is None
    _same(g.seq_push(b, levels)[:3], want, "sequence, host frames, after poison")
    _poison(g)
    assert g.seq_push(a, levels) is None, "a push after the aid must prime again"
    _same(g.seq_push(b, levels)[:3], want, "sequence, host frames, primed again")
    g.seq_reset()
    n = H * W
    d = [g.dev_alloc(a.nbytes), g.dev_alloc(8 * n), g.dev_alloc(8 * n), g.dev_alloc(8 * n * C)]
    try:
        def push(frame):
            g.dev_upload(d[0], frame)
            return g.seq_push_device(d[0], True, H, W, C, levels, None, d[1], d[2], d[3])

        def result():
            out = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, C))
            for arr, p in zip(out, d[1:]):
                g.dev_download(arr, p)
            return out

        _poison(g)
        assert push(a) is None
        assert push(b) is not None
        _same(result(), want, "sequence, device frames, after poison")
        _poison(g)
        assert push(a) is None, "a push after the aid must prime again"
        assert push(b) is not None
        _same(result(), want, "sequence, device frames, primed again")
    finally:
        g.seq_reset()
        for p in d:
            g.dev_free(p)


@pytest.mark.parametrize("levels", LEVELS)
def test_page_locked_outputs_after_poison(long_handle, oracle, levels):
    from papteam_opticalflow_amd import capi
    want = _fresh("small_L%d" % levels, oracle)
    g, (a, b) = long_handle, _pair()
    shapes = ((H, W), (H, W), (H, W, C))
    addrs = [capi._pinned_alloc(8 * int(np.prod(s))) for s in shapes]
    assert all(addrs)
    try:
        out = tuple(np.frombuffer((ctypes.c_char * (8 * int(np.prod(s)))).from_address(p), dtype=np.float64).reshape(s)
                    for s, p in zip(shapes, addrs))
        for x in out:
            x[...] = np.nan
        g.seq_reset()
        _poison(g)
        assert g.seq_push(a, levels, None, out) is None
        assert g.seq_push(b, levels, None, out) is not None
        _same(out, want, "sequence into page-locked arrays after poison")
        for x in out:
            x[...] = np.nan
        _poison(g)
        D = ctypes.POINTER(ctypes.c_double)
        fa, fb, t = _f64(a), _f64(b), np.zeros(10)
        rc = g.L.papof_flow(g.h, fa.ctypes.data_as(D), fb.ctypes.data_as(D), H, W, C, levels, None,
                            out[0].ctypes.data_as(D), out[1].ctypes.data_as(D), out[2].ctypes.data_as(D), t.ctypes.data_as(D))
        assert rc == 0
        _same(out, want, "host call into page-locked arrays after poison")
        del out, x
    finally:
        g.seq_reset()
        for p in addrs:
            capi._pinned_free(p)


def _tensor_pairs(flow, warp):
    flow, warp = flow.cpu().numpy(), warp.cpu().numpy()
    return [(np.ascontiguousarray(flow[p, 0]), np.ascontiguousarray(flow[p, 1]), np.ascontiguousarray(warp[p]))
            for p in range(flow.shape[0])]


def _poison_tensor_handle():
    from papteam_opticalflow_amd import tensors
    g, lock = tensors._handle(0)
    torch.cuda.synchronize()
    with lock:
        return _poison(g)


@pytest.fixture(scope="module")
def want_swapped(oracle):
    """the oracle's result per level count for the pair with its frames exchanged (the backward pairs, a video's (b, a))"""
    a, b = _pair()
    out = {}
    for levels in LEVELS:
        out[levels] = _frozen(oracle.coarse2fine_flow(_f64(b), _f64(a), levels)[:3])
    return out


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("n_pairs", [1, 3], ids=["one_pair_scratch", "three_pairs_chain"])
@pytest.mark.skipif(torch is None, reason="the tensor calls take torch tensors")
def test_tensor_routes_after_poison(oracle, want_swapped, levels, n_pairs):
    """flow_video, flow_video_fb and flow_video(init_flow=0) on the process-wide handle of the tensor calls: one pair runs
    through the handle's one-pair scratch, three through the batched chain.  Each route once over what the calls before
    left, once after poison."""
    from papteam_opticalflow_amd import tensors
    fw, bw = _fresh("small_L%d" % levels, oracle), want_swapped[levels]
    a, b = _pair()
    frames = torch.from_numpy(np.stack([a, b, a, b][:n_pairs + 1])).cuda()
    wants = [fw, bw, fw][:n_pairs]
    swapped = [bw, fw, bw][:n_pairs]
    kw = dict(layout="NHWC", out_dtype=torch.float64)
    zero = torch.zeros((n_pairs, 2, H, W), dtype=torch.float64, device=frames.device)
    for state in ("leftovers", "poison"):
        if state == "poison":
            assert _poison_tensor_handle() > 0
        flow, warp, _ = tensors.flow_video(frames, levels, **kw)
        for p, r in enumerate(_tensor_pairs(flow, warp)):
            _same(r, wants[p], "flow_video pair %d (%s)" % (p, state))
        if state == "poison":
            _poison_tensor_handle()
        r = tensors.flow_video_fb(frames, levels, **kw)
        for p, x in enumerate(_tensor_pairs(r.flow_fw, r.warpI2_fw)):
            _same(x, wants[p], "flow_video_fb forward pair %d (%s)" % (p, state))
        for p, x in enumerate(_tensor_pairs(r.flow_bw, r.warpI2_bw)):
            _same(x, swapped[p], "flow_video_fb backward pair %d (%s)" % (p, state))
        if state == "poison":
            _poison_tensor_handle()
        flow, warp, _ = tensors.flow_video(frames, levels, init_flow=zero, **kw)
        for p, r in enumerate(_tensor_pairs(flow, warp)):
            _same(r, wants[p], "flow_video(init_flow=0) pair %d (%s)" % (p, state))
    torch.cuda.synchronize()


def test_crop_that_runs_the_tiny_and_a_hyperplane_kernel_after_poison(long_handle, oracle):
    from papteam_opticalflow_amd import capi
    assert capi.sor_tiny_shape(*BIG)[0] == 0  # level 0: a hyperplane kernel
    assert capi.sor_tiny_shape(int(BIG[0] * 0.75), int(BIG[1] * 0.75))[0] > 0  # level 1: k_sor_tiny
    want = _fresh("big_L3", oracle)
    run = _cases()["big_L3"].run
    _poison(long_handle)
    _same(run(long_handle), want, "70 x 120 crop, 3 levels, after poison")
    kinds = {e["kind"] for e in long_handle.last_sor_solves()}
    assert TINY in kinds and kinds & set(HYPERPLANE), kinds
    print("70 x 120 crop: solver kinds %s" % sorted(kinds))
    _same(run(long_handle), want, "70 x 120 crop, 3 levels, again")


@pytest.fixture(scope="module", params=KNOBS, ids=lambda k: "+".join("%s=%s" % (n[10:], v) for n, v in k.items()) or "TINY=0")
def off_whole(request):
    """as `off`, for the whole calls (handles of their own: the stage tests of section a all run before any whole call)"""
    g = _handle(dict(request.param, PAPOF_SOR_TINY="0"))
    yield g, request.param
    g.close()


def test_crop_on_every_hyperplane_kernel_after_poison(off_whole, oracle):
    """the whole call with k_sor_tiny off and each hyperplane kernel forced: every level's skewed planes lie over poison, and
    over the larger level's planes at another pitch"""
    g, knobs = off_whole
    want = _fresh("big_L3", oracle)
    run = _cases()["big_L3"].run
    for what in ("on a new handle", "after poison", "after poison, again"):
        if what != "on a new handle":
            _poison(g)
        _same(run(g), want, "70 x 120 crop, 3 levels, knobs %r, %s" % (knobs, what))
        kinds = {e["kind"] for e in g.last_sor_solves()}
        assert kinds and kinds <= set(HYPERPLANE), kinds
        if knobs.get("PAPOF_SOR_FUSE") == "2":
            assert kinds == {1}, kinds
        if "PAPOF_SOR_GROUP" in knobs:
            assert kinds == {2}, kinds
        if "PAPOF_SOR_XLANE" in knobs:
            assert kinds == {0}, kinds
    print("70 x 120 crop, knobs %r: solver kinds %s" % (knobs, sorted(kinds)))


# ======================================================================================================================
# c. order walks on one handle
# ======================================================================================================================
def _walk(g, oracle, poison):
    """the fixed list of calls; before every call the handle is poisoned, or left as the call before left it"""
    c = _cases()
    grown = {}

    def before(tag=None):
        if poison:
            n = _poison(g)
            if tag:
                grown[tag] = n

    def pair(name):
        before()
        _same(c[name].run(g), _fresh(name, oracle), "walk (%s): %s" % ("poison" if poison else "leftovers", name))

    pair("big_L3")         # big, then small, then the same big again
    pair("small_L3")
    pair("big_L3")
    pair("gray_big_L3")    # C = 3, then C = 1 at the same size
    pair("small_L7")       # 7 levels, then 3 at the same size
    pair("small_L3")
    pair("small_L3_sor5")  # default sweeps, then n_sor = 5 on every level, then default again
    pair("small_L3")
    # a call that makes the arena grow (three pairs' arrays in one arena), directly followed by a small one
    before("before_growth")
    big = c["big_L3"]
    out, _ = g.flow_batch([big.a, big.b] * 3, 3, None, sequence=False)
    for p in range(3):
        _same(out[p], _fresh("big_L3", oracle), "walk: batch of three 70 x 120 pairs, pair %d" % p)
    del out
    before("after_growth")
    _same(c["small_L3"].run(g), _fresh("small_L3", oracle), "walk: the small pair behind the arena's growth")
    if poison:
        assert grown["after_growth"] > grown["before_growth"], grown
    # a stage call between two whole calls
    before()
    planes, want = _case(oracle, 42, 75, 5)
    _same(g.sor(*planes, 5, mode=0), want, "walk: gpu.sor between two whole calls")
    pair("gray_big_L3")
    # a sequence push, then a pair call, then a push: it must prime again
    small = c["small_L3"]
    g.seq_reset()
    before()
    assert g.seq_push(small.a, 3) is None
    pair("big_L3")
    if not poison:
        assert g.seq_push(small.a, 3) is None, "a push behind a pair call must prime again"
    else:
        before()
        assert g.seq_push(small.a, 3) is None
    r = g.seq_push(small.b, 3)
    assert r is not None
    _same(r[:3], _fresh("small_L3", oracle), "walk: the sequence's pair")
    g.seq_reset()
    # the guard: the tripping pair (optimistic pass, then the exact pass over used memory), the sticky exact start of an
    # ordinary pair, the duplicate pair through the single call and through the batch (test_gpu_parity.py, test_gpu_batch.py)
    st0 = g.lap_guard_stats()
    assert st0["exact_next"] is False and st0["guard_on"] is True, st0
    pair("tiny_scale_L3")
    st = g.lap_guard_stats()
    assert st["reruns"] == st0["reruns"] + 1 and st["exact_next"] is True, st
    pair("big_f64_L3")
    st = g.lap_guard_stats()
    assert (st["reruns"] == st0["reruns"] + 1 and st["exact_calls"] == st0["exact_calls"] + 1
            and st["exact_next"] is False), st
    pair("duplicate_L3")
    st = g.lap_guard_stats()
    assert st["reruns"] == st0["reruns"] + 2 and st["exact_next"] is True, st
    dup = _fresh("duplicate_L3", oracle)
    assert not dup[0].any() and not dup[1].any()
    before()
    out, _ = g.flow_batch([big.a] * 4, 3, None, sequence=False)
    assert g.lap_guard_stats()["reruns"] > st["reruns"]
    for p in range(2):
        _same(out[p], dup, "walk: batch of two duplicate pairs, pair %d" % p)
    del out
    pair("big_L3")


@pytest.mark.parametrize("poison", [True, False], ids=["poison", "leftovers"])
def test_order_walk_on_one_handle(oracle, poison):
    g = _fresh_handle()
    try:
        _walk(g, oracle, poison)
    finally:
        g.close()


# ======================================================================================================================
# d. the aid itself
# ======================================================================================================================
def test_the_aid_itself(oracle):
    from papteam_opticalflow_amd import capi
    assert capi.load().papof_test_poison(None, PATTERN, None) == -1  # PAPOF_EINVAL: a null handle
    small, big = _cases()["small_L3"], _cases()["big_L3"]
    g = _fresh_handle()
    try:
        n0 = _poison(g)
        # a handle that ran nothing has no arena and no staging block: at most LapPara (8 doubles) and the scratch of the
        # exact pass's reduction (csrc/kernels.hip: lap_scratch_doubles() = 256 blocks x 8 channels x 2)
        assert n0 in (0, 8 * (8 + 256 * 8 * 2)), n0
        assert _poison(g) == n0
        _same(small.run(g), _fresh("small_L3", oracle), "the first call of a poisoned new handle")
        n1 = _poison(g)
        assert n1 >= n0 + 2 * small.a.nbytes + 8 * (H * W * C + 2 * H * W)  # at least the call's inputs and outputs
        _same(big.run(g), _fresh("big_L3", oracle), "a larger call")
        n2 = _poison(g)
        assert n2 > n1
        assert _poison(g) == n2  # twice in a row: harmless
        _same(small.run(g), _fresh("small_L3", oracle), "a call behind two poisonings")
        assert g.L.papof_test_poison(g.h, PATTERN, None) == 0  # the byte count is optional
        _same(small.run(g), _fresh("small_L3", oracle), "a call behind a poisoning without a byte count")
    finally:
        g.close()
