"""Host-logic test of the issue order in which the operand slots of the exact-order SOR steps carry the left weight and the
next centre (tests/sim_sor_carry.py: unknowns and phi requested R - 1 steps early into the previous step's slot, planes that
start out as NaN, stores visible only once a publication covers them, publications lagging, a random one-step scheduler):
bit for bit the oracle's in-place lexicographic sweeps -- and NOT so once the coverage bound is one step weaker, which is
what makes the model a check of that bound.

Widths leave a task's step count (W + 63) with the remainders 0, 1 and R - 1 modulo R: the last iteration is empty, one step
long, or full but one, and the carried slot R - 1 crosses an iteration in each of them."""
import numpy as np
import pytest

import sim_sor_carry as carry
import sim_sor_wave as sim


def _planes(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 50.0, (h, w)), rng.uniform(-0.02, 0.02, (h, w)), rng.uniform(0, 0.05, (h, w)),
            rng.uniform(0, 0.05, (h, w)), rng.uniform(-0.01, 0.01, (h, w)), rng.uniform(-0.01, 0.01, (h, w)))


def _widths(r, least=3):
    """the smallest widths >= least whose step count W + 63 leaves 0, 1 and R - 1 modulo R"""
    return [next(w for w in range(least, least + r) if (w + sim.LANES - 1) % r == m) for m in (0, 1, r - 1)]


_cache = {}


def _case(oracle, h, w, n_sor):
    key = (h, w, n_sor)
    if key not in _cache:
        phi, xy, x2, y2, r1, r2 = _planes(h, w, h * 1000 + w * 10 + n_sor)
        a1, a2 = sim.sor_coefficients(phi, x2, y2, 0.012, 1.8)
        want = oracle.sor(phi, xy, x2, y2, r1, r2, n_sor, alpha=0.012, omega=1.8, mode=0)
        _cache[key] = ((phi, xy, a1, a2, r1, r2), want)
    return _cache[key]


EXACT = [(h, w, n, r) for r in (4, 6, 8, 10) for h, n in ((70, 4),) for w in _widths(r)] + \
        [(130, 5, 3, 8), (1, 5, 3, 6), (5, 1, 3, 8), (125, 9, 5, 6)]
FUSED = [(h, w, n, r) for r in (6, 8, 10) for h, n in ((70, 5),) for w in _widths(r)] + \
        [(123, 6, 4, 8), (1, 5, 3, 6), (62, 9, 1, 6), (130, 5, 6, 8)]


@pytest.mark.parametrize("h,w,n_sor,r", EXACT)
def test_slot_carry_order_is_bit_exact(oracle, h, w, n_sor, r):
    ops, (eu, ev) = _case(oracle, h, w, n_sor)
    du, dv = carry.simulate(*ops, n_sor, 0.012, 1.8, r=r, seed=h + w)
    assert np.array_equal(du, eu) and np.array_equal(dv, ev)


@pytest.mark.parametrize("h,w,n_sor,r", FUSED)
def test_fused_slot_carry_order_is_bit_exact(oracle, h, w, n_sor, r):
    ops, (eu, ev) = _case(oracle, h, w, n_sor)
    du, dv = carry.simulate_fused(*ops, n_sor, 0.012, 1.8, r=r, seed=h + w)
    assert np.array_equal(du, eu) and np.array_equal(dv, ev)


@pytest.mark.parametrize("which", ["exact", "fused"])
def test_a_bound_one_step_weaker_reads_before_the_write(oracle, which):
    """the model is sensitive to the bound: with the unknowns' loads allowed one step further than the producers cover, some
    schedule reads a cell that is not there yet (two bands, so that both the own-band and the band-above edge exist)"""
    h, w, n_sor, r = 70, 9, 4, 8
    ops, (eu, ev) = _case(oracle, h, w, n_sor)
    f = carry.simulate if which == "exact" else carry.simulate_fused
    wrong = 0
    for seed in range(4):
        du, dv = f(*ops, n_sor, 0.012, 1.8, r=r, seed=seed, weaken=1)
        wrong += not (np.array_equal(du, eu) and np.array_equal(dv, ev))
    assert wrong > 0
