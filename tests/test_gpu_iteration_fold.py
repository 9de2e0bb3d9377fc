"""k_flow_system carries the update of the outer iteration before it (u + du, v + dv taken from the solver's increment planes and
written to the other pair of flow planes), so no update kernel runs between two outer iterations of a level: whole calls at
the shapes where that can go wrong, held byte for byte (-0.0 != +0.0) to
  * the same call under PAPOF_FUSED_SYSTEM=0 -- the pair of kernels, with an update kernel behind every solve --
  * and the oracle (OracleLib.coarse2fine_flow_sched).
Two levels (one entered from zero, one from the up-sampled flow), three outer iterations (two carried updates and one kept
per level), five sweeps unless stated, exact order.  The one-column frames are one-level calls: a second level of a frame
one pixel wide has no pixel (the plan refuses it: (int)(1 * 0.75) columns), so these enter from zero only.
One column on SKEWED planes is a frame of 130 rows on a handle made with PAPOF_SOR_TINY=0: the default handle gives a column
of up to 8192 cells to k_sor_tiny, and the skewed layout of a taller one ((H + W) x H cells of 16 bytes) is beyond the solver's
32-bit offsets (8300 x 1: 1.1 GB, refused).  k_sor_group is selected by 36 sweeps on at most two bands (88 + 35 rows).
What ran is asserted, not assumed: the solver kernel of level 0 from last_sor_solves(), the launches from last_chain_stats()
-- every outer iteration but a level's first carries an increment, one update kernel per level, a (du, dv) fill in front of a
solve only where k_sor_group solves.  Where the guard runs a call again in its exact pass (the pair of kernels),
k_flow_system's result is taken from a handle without the guard, as tests/test_gpu_flow_system_taps.py does.

The poison tests run two of the calls on a fresh handle, on a long-lived one after papof_test_poison, and there again after
a larger call of another shape and a second poison: the same bytes."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402
from _libs import OracleLib  # noqa: E402

pytestmark = pytest.mark.gpu

N_OUTER = 3
EXACT, FUSED, GROUP, TINY = 0, 1, 2, 6  # include/papof.h: papof_last_sor_solves
PATTERN = 0x7FF8DEAD7FF8DEAD
# (H, W, sweeps, the solver kernel of level 0, the handle's environment)
SHAPES = [
    (83, 99, 5, EXACT, {}),    # two bands, ragged tiles on both borders, just above the one-workgroup limit
    (130, 67, 5, EXACT, {}),   # three bands, tiles straddling two boundaries
    (24, 3, 5, TINY, {}),      # row-major increments of k_sor_tiny, the narrowest widths
    (24, 1, 5, TINY, {}),
    (130, 1, 5, EXACT, {"PAPOF_SOR_TINY": "0"}),  # the one-column instantiation on skewed planes, three bands
    (1000, 24, 5, FUSED, {}),  # at least 16 bands: k_sor_fused and its dpar
    (88, 95, 36, GROUP, {}),   # k_sor_group, which reads the zeros of its (du, dv) fill
]
IDS = ["%dx%d-sor%d" % s[:3] for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _frames(h, w, gray):
    """uint8 HWC frames cut from the committed 240 fixture (rows and columns beyond it: the fixture mirrored back and forth)"""
    a, b = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)

    def mirror(n, size, first):
        i = (first + np.arange(n)) % (2 * size - 2)
        return np.where(i < size, i, 2 * size - 2 - i)

    rows, cols = mirror(h, a.shape[0], 40), mirror(w, a.shape[1], 60)
    ch = slice(0, 1) if gray else slice(None)
    out = tuple(np.ascontiguousarray(x[rows][:, cols][:, :, ch]) for x in (a, b))
    for x in out:
        x.setflags(write=False)
    return out


def _params(n_sor):
    from papteam_opticalflow_amd import default_params
    return default_params(n_outer=N_OUTER, n_outer_per_level=0, n_sor=n_sor, n_sor_per_level=0)


def _levels(w):
    return 2 if w > 1 else 1


def _run(g, h, w, n_sor, gray):
    a, b = _frames(h, w, gray)
    return tuple(np.array(x) for x in g.coarse2fine_flow_u8(a, b, _levels(w), _params(n_sor))[:3])


@functools.lru_cache(maxsize=None)
def _oracle(h, w, n_sor, gray):
    a, b = _frames(h, w, gray)
    return OracleLib().coarse2fine_flow_sched(a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0, _levels(w), 0.012, 0.75,
                                              N_OUTER, 0, 1, n_sor, 0)


def _same(got, want, what):
    for name, g, w_ in zip(("vx", "vy", "warpI2"), got, want):
        g, w_ = np.ascontiguousarray(g), np.ascontiguousarray(w_)
        assert g.shape == w_.shape and g.dtype == w_.dtype, (what, name, g.shape, w_.shape)
        if g.tobytes() != w_.tobytes():
            raise AssertionError("%s, %s: %d elements differ, max-abs %.3e"
                                 % (what, name, int((g.view(np.int64) != w_.view(np.int64)).sum()), float(np.abs(g - w_).max())))


def _handle(guard=True, env={}):
    """a handle made under `env` (the solver knobs are read when a handle is made)"""
    from papteam_opticalflow_amd import Papof
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        if not guard:
            mp.setenv("PAPOF_LAP_GUARD", "0")  # read when a handle is made
        g = Papof(0)
    assert g.lap_guard_stats()["guard_on"] == guard
    return g


def _check_chain(g, h, w, kind, carried):
    """the launches of the last call on g: every level ran k_flow_system (carried) or the pair of kernels (not carried)"""
    solves = g.last_sor_solves()
    LEVELS = _levels(w)
    assert len(solves) == LEVELS * N_OUTER, solves
    kinds0 = {s["kind"] for s in solves if (s["h"], s["w"]) == (h, w)}
    assert kinds0 == {kind}, (kinds0, kind)
    st = g.last_chain_stats()
    fills = sum(1 for s in solves if s["kind"] == GROUP)  # (k_sor_exact / k_sor_fused: one clear when the level is entered)
    if carried:
        want = dict(flow_systems=LEVELS * N_OUTER, carried=LEVELS * (N_OUTER - 1), updates=LEVELS, clears=fills)
    else:
        want = dict(flow_systems=0, carried=0, updates=LEVELS * N_OUTER, clears=fills)
    assert st == want, (st, want)


@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
@pytest.mark.parametrize("h,w,n_sor,kind,env", SHAPES, ids=IDS)
def test_carried_updates_give_the_bytes_of_the_update_kernel_and_the_oracle(monkeypatch, h, w, n_sor, kind, env, gray):
    what = "%dx%d %s, %d sweeps" % (h, w, "gray" if gray else "rgb", n_sor)
    want = _oracle(h, w, n_sor, gray)
    g = _handle(env=env)
    try:
        got = _run(g, h, w, n_sor, gray)
        st = g.lap_guard_stats()
        rerun = (st["reruns"], st["exact_calls"]) != (0, 0)
        if not rerun:
            _check_chain(g, h, w, kind, True)
    finally:
        g.close()
    _same(got, want, what + ": the default call vs the oracle")
    if rerun:
        print(what + ": the guard ran the call again in its exact pass; k_flow_system's result from a handle without the guard")
    g = _handle(guard=not rerun, env=env)
    try:
        one = _run(g, h, w, n_sor, gray)
        _check_chain(g, h, w, kind, True)
        monkeypatch.setenv("PAPOF_FUSED_SYSTEM", "0")
        two = _run(g, h, w, n_sor, gray)
        _check_chain(g, h, w, kind, False)
        monkeypatch.delenv("PAPOF_FUSED_SYSTEM")
    finally:
        g.close()
    _same(one, two, what + ": carried updates vs the update kernel")
    if rerun and any(x.tobytes() != y.tobytes() for x, y in zip(one, got)):
        assert w == 1, what + ": without the guard k_flow_system's call is not the oracle's, with it (pair of kernels) it is"
        pytest.skip(what + ": the reference's guard trips here (a channel's warp is frame 1 in every pixel), so the call is "
                    "assembled by the pair of kernels in the exact pass; k_flow_system agrees with them without the guard")
    _same(one, want, what + ": carried updates vs the oracle")


@pytest.fixture(scope="module")
def long_handle():
    g = _handle()
    yield g
    g.close()


@pytest.mark.parametrize("h,w,n_sor,kind,env", [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_carried_updates_do_not_depend_on_what_the_handle_held(long_handle, h, w, n_sor, kind, env):
    what = "%dx%d rgb" % (h, w)
    g = _handle()
    try:
        fresh = _run(g, h, w, n_sor, False)
        _check_chain(g, h, w, kind, True)
    finally:
        g.close()
    _same(fresh, _oracle(h, w, n_sor, False), what + ": a fresh handle vs the oracle")
    long_handle.test_poison(PATTERN)
    _same(_run(long_handle, h, w, n_sor, False), fresh, what + ": after poison")
    _check_chain(long_handle, h, w, kind, True)
    big = _frames(150, 200, False)  # a larger call of another shape: three levels, the default schedule's sweeps
    long_handle.coarse2fine_flow_u8(big[0], big[1], 3)
    long_handle.test_poison(PATTERN)
    _same(_run(long_handle, h, w, n_sor, False), fresh, what + ": after a larger call and a second poison")
