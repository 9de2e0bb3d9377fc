"""The up-neighbour products of the exact-order solver step (csrc/sor.hip: step(), f_step(), g_step()) are formed ONCE -- lane
l - 1's left products phi * du, phi * dv -- and handed to lane l across the wave, instead of handing over their three factors and
multiplying again.  The bits may not change: every kernel that carries the hand-over, on the smallest planes on which a product
crosses every kind of lane, bit for bit against the oracle's in-place lexicographic sweeps, and the kernel (and the pipeline
depth where a knob sets it) proven from the handle's log of solves (kind 0 k_sor_exact, 1 k_sor_fused, 2 k_sor_group).

  k_sor_exact, depth 6 / 4 / 8   63x5x3, 125x7x5    band 1's ghost lane 0 carries band 0's last row; the top band's dead lanes
                                                    at sweeps >= 1
  shuffle path                   63x5x3             the wave-edge lane receives its own value
  k_sor_fused                    62x9x4, 62x9x3,    61-row bands, carrier / ghost lanes 0, 1, 62; an odd sweep count runs the
                                 123x6x5            identity second sweep
  k_sor_group, 2 / 4 sweeps      70x11x4, 130x6x8   the LDS ring between the sweeps of a workgroup, the halo row

Two sets of operand planes per shape: the random ones of tests/test_gpu_sor_kernels.py, and `special` ones -- a checkerboard of
exact 0.0 in phi, b1 = b2 = 0 on alternate rows (exact zeros of either sign travel as up-products), row 20 of every operand
scaled by 1e-300 and row 61 (band 0's last row, the one a ghost lane carries) by 1e-158.  Under the checkerboard a cell with
phi != 0 has only zero weights around it, so on a scaled row its du and dv scale with the row: at 1e-300 the up-products
phi * du underflow to exact zeros of either sign, at 1e-158 they land near 1e-313 -- subnormal.  The last test checks on the
oracle's result that both really occur.

No tolerance: np.array_equal, and on the special planes the sign bits too (array_equal takes -0.0 for 0.0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT, FUSED, GROUP = 0, 1, 2

# (knobs, kind, depth the log must show or None, [(H, W, sweeps)])
PLAN = [
    ({}, EXACT, 6, [(63, 5, 3), (125, 7, 5)]),
    ({"PAPOF_SOR_DEPTH": "4"}, EXACT, 4, [(63, 5, 3), (125, 7, 5)]),
    ({"PAPOF_SOR_DEPTH": "8"}, EXACT, 8, [(63, 5, 3), (125, 7, 5)]),
    ({"PAPOF_SOR_XLANE": "shfl"}, EXACT, None, [(63, 5, 3)]),
    ({"PAPOF_SOR_FUSE": "2"}, FUSED, None, [(62, 9, 4), (62, 9, 3), (123, 6, 5)]),
    ({"PAPOF_SOR_GROUP": "2"}, GROUP, None, [(70, 11, 4), (130, 6, 8)]),
    ({"PAPOF_SOR_GROUP": "4"}, GROUP, None, [(70, 11, 4), (130, 6, 8)]),
]
TINY_ROW_1, TINY_ROW_2 = 20, 61  # rows scaled by 1e-300 / 1e-158 (every plane here has at least 62 rows)


def _knob_id(knobs):
    return "+".join("%s=%s" % (n[10:], v) for n, v in knobs.items()) or "TINY=0"


CASES = [pytest.param(i, h, w, n, kind, id="%s-%dx%dx%d-%s" % (_knob_id(PLAN[i][0]), h, w, n, kind))
         for i in range(len(PLAN)) for h, w, n in PLAN[i][3] for kind in ("random", "special")]


def _random_planes(h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 50.0, (h, w)), rng.uniform(-0.02, 0.02, (h, w)), rng.uniform(0, 0.05, (h, w)),
            rng.uniform(0, 0.05, (h, w)), rng.uniform(-0.01, 0.01, (h, w)), rng.uniform(-0.01, 0.01, (h, w))]


def _special_planes(h, w, seed):
    phi, xy, x2, y2, b1, b2 = planes = _random_planes(h, w, seed)
    i, j = np.indices((h, w))
    phi[(i + j) % 2 == 0] = 0.0
    b1[0::2] = 0.0
    b2[0::2] = 0.0
    for p in planes:
        p[TINY_ROW_1] *= 1e-300
        p[TINY_ROW_2] *= 1e-158
    return planes


_cache = {}


def _case(oracle, h, w, n_sor, kind):
    """(operand planes, the oracle's (du, dv)) of a case: computed once, shared by every handle, read-only"""
    key = (h, w, n_sor, kind)
    if key not in _cache:
        planes = _random_planes(h, w, h * 7 + w) if kind == "random" else _special_planes(h, w, h * 11 + w)
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


@pytest.mark.parametrize("i,h,w,n_sor,kind", CASES)
def test_step_products_bit_for_bit(handle_for, oracle, i, h, w, n_sor, kind):
    knobs, want_kind, want_depth, _ = PLAN[i]
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


@pytest.mark.parametrize("h,w,n_sor", sorted({s for p in PLAN for s in p[3]}))
def test_special_planes_carry_what_they_claim(oracle, h, w, n_sor):
    """the special planes' up-products (phi * du, phi * dv of the row above, on the oracle's result) include exact zeros of
    both signs and subnormals -- a property of the test's inputs, checked on the CPU side of the comparison"""
    (phi, _, _, _, b1, b2), (eu, ev) = _case(oracle, h, w, n_sor, "special")
    with np.errstate(under="ignore"):
        up = np.concatenate([(phi * eu).ravel(), (phi * ev).ravel()])
    tiny = np.finfo(np.float64).tiny
    assert ((up == 0) & ~np.signbit(up)).any() and ((up == 0) & np.signbit(up)).any()
    assert ((up != 0) & (np.abs(up) < tiny)).any()
    assert not b1[0::2].any() and not b2[0::2].any() and np.isfinite(eu).all() and np.isfinite(ev).all()
