"""Every exact-order solver kernel of csrc/sor.hip on planes that SELECT it, bit for bit against the oracle's in-place
lexicographic sweeps (src/OpticalFlow.cpp:458-505) -- and every case proves which kernel it ran on: the instance of the
one-workgroup solver from the library's own host-side query (papof_sor_tiny_shape), the kernel from the handle's log of solves
(papof_last_sor_solves: kind 0 k_sor_exact, 1 k_sor_fused, 2 k_sor_group, 6 k_sor_tiny).

a. k_sor_tiny: each of its instances at the edges of the shape heuristic (tests/_sor_shapes.py): a full workgroup, dynamic LDS
   exactly at the cap, a ragged last tile, an odd number of tiles per row (the last lane owns one tile instead of two).
b. the hyperplane kernels on the small planes k_sor_tiny takes from them by default -- planes of one and two bands, a band
   boundary at rows 62 / 63, single rows and columns -- on handles created with PAPOF_SOR_TINY=0 alone and with each knob that
   forces one of the kernels.
c. whole calls with the switch off give the default handle's bits, single and batched.

No tolerance anywhere: np.array_equal."""
import numpy as np
import pytest

import cases
from _sor_shapes import TINY_SHAPES

pytestmark = pytest.mark.gpu

TINY, HYPERPLANE = 6, (0, 1, 2)


@pytest.fixture(scope="module")
def gpu():
    from papteam_opticalflow_amd import Papof
    g = Papof(0)
    yield g
    g.close()


def _handle(env):
    """a handle created under `env`: the solver knobs are read when a handle is created"""
    from papteam_opticalflow_amd import Papof
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return Papof(0)


def _sor_planes(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 50.0, (h, w)), rng.uniform(-0.02, 0.02, (h, w)), rng.uniform(0, 0.05, (h, w)),
            rng.uniform(0, 0.05, (h, w)), rng.uniform(-0.01, 0.01, (h, w)), rng.uniform(-0.01, 0.01, (h, w)))


_cache = {}


def _case(oracle, h, w, n_sor, alpha=0.012, omega=1.8):
    """(operand planes, the oracle's (du, dv)) of a case: computed once, shared by every handle, read-only"""
    key = (h, w, n_sor, alpha, omega)
    if key not in _cache:
        planes = _sor_planes(h, w, h * 7 + w)
        want = oracle.sor(*planes, n_sor, alpha=alpha, omega=omega, mode=0)
        for a in planes + want:
            a.setflags(write=False)
        _cache[key] = (planes, want)
    return _cache[key]


def _solve(g, oracle, h, w, n_sor, alpha=0.012, omega=1.8):
    """one solve on handle g checked against the oracle's bits; returns the kind of kernel that ran it"""
    planes, (eu, ev) = _case(oracle, h, w, n_sor, alpha, omega)
    du, dv = g.sor(*planes, n_sor, alpha=alpha, omega=omega, mode=0)
    e = g.last_sor_solves()[-1]
    assert (e["h"], e["w"], e["n_sor"]) == (h, w, n_sor), e  # the log's last entry is this solve
    bad = int((du != eu).sum() + (dv != ev).sum())
    assert np.array_equal(du, eu) and np.array_equal(dv, ev), \
        "%dx%d x %d sweeps on kind %d: %d cells differ, max-abs %.3e" % (h, w, n_sor, e["kind"], bad,
                                                                         max(np.abs(du - eu).max(), np.abs(dv - ev).max()))
    return e["kind"]


# ---- a. every instance of k_sor_tiny at its edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n_sor", [1, 2, 7])
@pytest.mark.parametrize("c,hw,waves,what", TINY_SHAPES)
def test_tiny_instance_at_its_edges(gpu, oracle, c, hw, waves, what, n_sor):
    from papteam_opticalflow_amd import capi
    assert capi.sor_tiny_shape(*hw) == (c, waves), what
    assert _solve(gpu, oracle, hw[0], hw[1], n_sor) == TINY


@pytest.mark.parametrize("c,hw", [(1, (32, 63)), (2, (798, 3)), (3, (48, 85)), (5, (238, 19)), (6, (198, 23))])
def test_tiny_instance_other_alpha_and_omega(gpu, oracle, c, hw):
    from papteam_opticalflow_amd import capi
    assert capi.sor_tiny_shape(*hw)[0] == c
    assert _solve(gpu, oracle, hw[0], hw[1], 7, alpha=0.05, omega=1.3) == TINY


# ---- b. the hyperplane kernels on the small planes -------------------------------------------------------------------
KNOBS = [{}, {"PAPOF_SOR_FUSE": "1"}, {"PAPOF_SOR_FUSE": "2"}, {"PAPOF_SOR_GROUP": "2"}, {"PAPOF_SOR_GROUP": "4"},
         {"PAPOF_SOR_XLANE": "shfl"}, {"PAPOF_SOR_DEPTH": "4"}]
SMALL = [(1, 1, 1), (1, 1, 3), (1, 5, 3), (5, 1, 3), (2, 2, 2),          # fewer cells than a wave has lanes
         (62, 1, 3), (63, 1, 3),                                          # one column across the band boundary
         (61, 40, 2), (62, 40, 1), (63, 64, 1),                           # the last row of band 0 / the first of band 1
         (124, 3, 2), (60, 33, 5), (64, 20, 3), (70, 50, 4),
         (7, 100, 4), (1, 300, 3),                                        # wider than a wave, one band
         (42, 75, 5), (42, 75, 36)]                                       # 36 sweeps on 2 bands: the default picks k_sor_group


@pytest.fixture(scope="module", params=KNOBS, ids=lambda k: "+".join("%s=%s" % (n[10:], v) for n, v in k.items()) or "TINY=0")
def off(request):
    g = _handle(dict(request.param, PAPOF_SOR_TINY="0"))
    yield g, request.param
    g.close()


@pytest.mark.parametrize("h,w,n_sor", SMALL)
def test_hyperplane_kernels_on_small_planes(off, oracle, h, w, n_sor):
    from papteam_opticalflow_amd import capi
    g, knobs = off
    assert capi.sor_tiny_shape(h, w)[0] > 0  # a plane the default handle gives to k_sor_tiny
    kind = _solve(g, oracle, h, w, n_sor)
    assert kind in HYPERPLANE, kind
    if knobs.get("PAPOF_SOR_FUSE") == "2" and n_sor >= 2:
        assert kind == 1  # odd sweep counts included: the identity second sweep of the last pair
    if knobs.get("PAPOF_SOR_FUSE") == "1":
        assert kind != 1
    if "PAPOF_SOR_GROUP" in knobs and n_sor >= 2:
        assert kind == 2
    if "PAPOF_SOR_XLANE" in knobs:
        assert kind == 0  # the fused and grouped kernels need the DPP lane shifts
    if n_sor < 2:
        assert kind == 0


def test_default_handle_takes_the_same_planes_to_the_tiny_solver(gpu, oracle):
    """... and picks the grouped kernel where it is left the choice: what section b's handles must NOT do by accident"""
    for h, w, n_sor in SMALL:
        assert _solve(gpu, oracle, h, w, n_sor) == TINY
    g = _handle({"PAPOF_SOR_TINY": "0"})
    try:
        assert _solve(g, oracle, 42, 75, 36) == 2
        assert _solve(g, oracle, 42, 75, 5) == 0
    finally:
        g.close()
    g = _handle({"PAPOF_SOR_TINY": "1"})  # any other value leaves the switch on
    try:
        assert _solve(g, oracle, 42, 75, 5) == TINY
    finally:
        g.close()


# ---- c. whole calls with the switch off ------------------------------------------------------------------------------
def _kinds(g):
    return [e["kind"] for e in g.last_sor_solves()]


def _shapes(g):
    return [(e["h"], e["w"], e["n_sor"]) for e in g.last_sor_solves()]


@pytest.fixture(scope="module")
def plain_off():
    g = _handle({"PAPOF_SOR_TINY": "0"})
    yield g
    g.close()


@pytest.mark.parametrize("crop,levels", [(None, 15), ((37, 53), 3)])
def test_whole_call_with_the_switch_off_gives_the_default_bits(gpu, plain_off, crop, levels):
    a, b = cases.load_pair("240")
    if crop:
        a, b = np.ascontiguousarray(a[:crop[0], :crop[1]]), np.ascontiguousarray(b[:crop[0], :crop[1]])
    want = [x.copy() for x in gpu.coarse2fine_flow(a, b, levels)[:3]]
    on_kinds, on_shapes = _kinds(gpu), _shapes(gpu)
    got = plain_off.coarse2fine_flow(a, b, levels)[:3]
    off_kinds, off_shapes = _kinds(plain_off), _shapes(plain_off)
    assert TINY in on_kinds
    assert off_kinds and TINY not in off_kinds and set(off_kinds) <= set(HYPERPLANE), off_kinds
    assert off_shapes == on_shapes  # the same solves, in the same order
    for name, x, y in zip(("vx", "vy", "warpI2"), got, want):
        assert np.array_equal(x, y), "%s: max-abs %.3e" % (name, np.abs(x - y).max())


def test_batch_with_the_switch_off_gives_the_default_bits(gpu, plain_off):
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    frames = [np.ascontiguousarray(np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1)) for i in range(4)]
    want, _ = gpu.flow_batch(frames, 8, None, sequence=True)
    want = [[x.copy() for x in pair] for pair in want]
    on_kinds, on_shapes = _kinds(gpu), _shapes(gpu)
    got, _ = plain_off.flow_batch(frames, 8, None, sequence=True)
    off_kinds, off_shapes = _kinds(plain_off), _shapes(plain_off)
    assert len(got) == len(want) == 3
    assert TINY in on_kinds
    assert off_kinds and TINY not in off_kinds and set(off_kinds) <= set(HYPERPLANE), off_kinds
    assert off_shapes == on_shapes
    for i in range(3):
        for name, x, y in zip(("vx", "vy", "warpI2"), got[i], want[i]):
            assert np.array_equal(x, y), "pair %d %s: max-abs %.3e" % (i, name, np.abs(x - y).max())
