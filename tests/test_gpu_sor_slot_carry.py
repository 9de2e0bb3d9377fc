"""The operand slots of the exact-order solver steps (csrc/sor.hip: step(), f_step(), g_step()) carry the left weight and the
next centre: (phi, xy) and (du, dv) are requested R - 1 steps early into the slot of the PREVIOUS step, after the last use of
what it held, and nothing is copied out of a slot.  The bits may not change.  Every kernel that carries the order, bit for bit
against the oracle's in-place lexicographic sweeps, with the kernel and the pipeline depth proven from the handle's log of
solves (kind 0 k_sor_exact, 1 k_sor_fused, 2 k_sor_group):

  k_sor_exact at every depth it is instantiated for (4 / 6 / 8 / 10 / 12), the shuffle path (depth 8), k_sor_fused (depth 8),
  k_sor_group with 2 and 4 sweeps per workgroup (depth 8).

Planes of two bands (63 <= H <= 125; 62 .. 123 for the fused kernel's 61-row bands), 3 - 5 sweeps and an odd count for the
fused kernel.  WIDTHS per depth R such that a task's step count -- W + 63 for every wave kernel (csrc/common.h: SkewDims::ns)
-- leaves the remainders 0, 1 and R - 1 modulo R: the last iteration is empty, one step long, or full but one, and the slot
R - 1, which is carried from an iteration's last step into the next one's first, is refilled for a step that exists, for the
last step, or for none.  Operands: random planes and the `special` planes of tests/test_gpu_sor_step_products.py (exact
zeros of both signs, the subnormal rows).  A case is a plane of a few hundred cells.

No tolerance: np.array_equal, and on the special planes the sign bits too (array_equal takes -0.0 for 0.0)."""
import numpy as np
import pytest

from test_gpu_sor_step_products import _random_planes, _special_planes

pytestmark = pytest.mark.gpu

EXACT, FUSED, GROUP = 0, 1, 2
STEPS_BEYOND_WIDTH = 63  # a task runs W + 63 steps: 64 lanes, the lane above one column ahead


def _widths(r, least=3):
    """the smallest widths >= least whose step count leaves 0, 1 and R - 1 modulo R"""
    return [next(w for w in range(least, least + r) if (w + STEPS_BEYOND_WIDTH) % r == m) for m in (0, 1, r - 1)]


# (knobs, kind, the depth the log must show, its instance's R, [(H, sweeps)])
PLAN = [
    ({"PAPOF_SOR_DEPTH": "4"}, EXACT, 4, 4, [(63, 3)]),
    ({"PAPOF_SOR_DEPTH": "6"}, EXACT, 6, 6, [(125, 5)]),
    ({"PAPOF_SOR_DEPTH": "8"}, EXACT, 8, 8, [(100, 4)]),
    ({"PAPOF_SOR_DEPTH": "10"}, EXACT, 10, 10, [(63, 5)]),
    ({"PAPOF_SOR_DEPTH": "12"}, EXACT, 12, 12, [(125, 3)]),
    ({"PAPOF_SOR_XLANE": "shfl"}, EXACT, None, 8, [(63, 3)]),
    ({"PAPOF_SOR_FUSE": "2"}, FUSED, 8, 8, [(62, 3), (123, 5), (90, 4)]),
    ({"PAPOF_SOR_GROUP": "2"}, GROUP, 8, 8, [(70, 4)]),
    ({"PAPOF_SOR_GROUP": "4"}, GROUP, 8, 8, [(125, 5)]),
]


def _knob_id(knobs):
    return "+".join("%s=%s" % (n[10:], v) for n, v in knobs.items())


CASES = [pytest.param(i, h, w, n, kind, id="%s-%dx%dx%d-%s" % (_knob_id(PLAN[i][0]), h, w, n, kind))
         for i in range(len(PLAN)) for h, n in PLAN[i][4] for w in _widths(PLAN[i][3]) for kind in ("random", "special")]

_cache = {}


def _case(oracle, h, w, n_sor, kind):
    """(operand planes, the oracle's (du, dv)) of a case: computed once, read-only"""
    key = (h, w, n_sor, kind)
    if key not in _cache:
        planes = _random_planes(h, w, h * 13 + w) if kind == "random" else _special_planes(h, w, h * 17 + w)
        want = oracle.sor(*planes, n_sor, alpha=0.012, omega=1.8, mode=0)
        for a in list(planes) + list(want):
            a.setflags(write=False)
        _cache[key] = (planes, want)
    return _cache[key]


@pytest.fixture(scope="module")
def handle_for():
    """the handle created under PLAN[i]'s knobs (read when a handle is created) and PAPOF_SOR_TINY=0; the cases come grouped by
    knob, so one handle is open at a time"""
    from papteam_opticalflow_amd import Papof
    open_ = {}

    def get(i):
        if i not in open_:
            for g in open_.values():
                g.close()
            open_.clear()
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("PAPOF_SOR_TINY", "0")
                for k, v in PLAN[i][0].items():
                    mp.setenv(k, v)
                open_[i] = Papof(0)
        return open_[i]

    yield get
    for g in open_.values():
        g.close()


def test_widths_leave_the_remainders():
    for _, _, _, r, _ in PLAN:
        assert [(w + STEPS_BEYOND_WIDTH) % r for w in _widths(r)] == [0, 1, r - 1]


@pytest.mark.parametrize("i,h,w,n_sor,kind", CASES)
def test_slot_carry_bit_for_bit(handle_for, oracle, i, h, w, n_sor, kind):
    knobs, want_kind, want_depth, _, _ = PLAN[i]
    planes, (eu, ev) = _case(oracle, h, w, n_sor, kind)
    g = handle_for(i)
    du, dv = g.sor(*planes, n_sor, alpha=0.012, omega=1.8, mode=0)
    e = g.last_sor_solves()[-1]
    assert (e["h"], e["w"], e["n_sor"]) == (h, w, n_sor), e  # the log's last entry is this solve
    assert e["kind"] == want_kind, e
    if want_depth is not None:
        assert e["depth"] == want_depth, e
    bad = int((du != eu).sum() + (dv != ev).sum())
    print("%s %dx%d x %d %s: kind %d depth %d, %d cells differ" % (_knob_id(knobs), h, w, n_sor, kind, e["kind"], e["depth"], bad))
    assert np.array_equal(du, eu) and np.array_equal(dv, ev), \
        "%d cells differ, max-abs %.3e" % (bad, max(np.abs(du - eu).max(), np.abs(dv - ev).max()))
    if kind == "special":
        su, sv = int((np.signbit(du) != np.signbit(eu)).sum()), int((np.signbit(dv) != np.signbit(ev)).sum())
        assert su == 0 and sv == 0, "sign bits differ in %d / %d cells of du / dv" % (su, sv)
