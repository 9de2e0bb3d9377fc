"""The older forms of the kernels between two solves, held to the oracle's BYTES (-0.0 != +0.0).

k_flow_system is what a default call runs, and tests/test_gpu_flow_system_taps.py holds it to bytes.  The forms it grew out
of still run for n_inner > 1, the guard's exact pass, one-block levels, pass-through channel counts, the red-black and Jacobi
modes and the stage entry points; DESIGN.md 2 records them as bit-exact, and elsewhere they are compared under a tolerance
only.  They share their expressions with k_flow_system, so they are pinned here:

  * Papof.smoothflow_sor against the oracle's -- the materialised-warp chain: k_warp, k_smooth_hv_blend, k_phi, k_assemble_skew
    / k_assemble (not FAST), k_update_warp_phi with phi_out and the re-warp, the guard's exact pass -- from a start flow that
    takes pixels out of the image on the small shapes, in all three solver modes, with one and two inner iterations (the
    second reads the increment where the solver left it), for 3 and 2 feature channels;
  * a whole call on 2-channel frames (passed through by im2feature: k_warp_smooth_blend + k_assemble_skew<0, false>).

Shapes: one row, one column, no interior cell; smaller than the 5-tap reach; ragged 16-row and 16-column tiles; across the
64-column block and the 16-row tile of the blend kernels; and 9215 cells, just above kTinyMaxCells = 8192 (skewed operands,
dudv_cell through the increment when n_inner = 2)."""
import numpy as np
import pytest

import cases
from test_gpu_flow_system_taps import _same_bytes

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9), (9, 1), (2, 2), (5, 7), (17, 33), (21, 67), (95, 97)]
MODES = [(0, 1.8), (1, 1.8), (2, 1.0)]
N_OUTER, N_SOR, ALPHA = 2, 3, 0.012


@pytest.fixture(scope="module")
def gpu():
    from papteam_opticalflow_amd import Papof
    g = Papof(0)
    yield g
    g.close()


_inputs = {}


def _level(oracle, h, w, c):
    """(f1, f2, warp, u, v): features cut from the committed 240 fixture, a start flow seeded from the shape, the oracle's warp"""
    key = (h, w, c)
    if key not in _inputs:
        a, b = cases.load_pair("240")
        f1 = np.ascontiguousarray(cases.features5(a)[40:40 + h, 60:60 + w, :c])
        f2 = np.ascontiguousarray(cases.features5(b)[40:40 + h, 60:60 + w, :c])
        rng = np.random.default_rng(1000 * h + w)
        u, v = rng.uniform(-1.5, 1.5, (h, w)), rng.uniform(-1.5, 1.5, (h, w))
        _inputs[key] = (f1, f2, oracle.warpFL(f1, f2, u, v), u, v)
    return _inputs[key]


_wants = {}


def _want(oracle, h, w, c, mode, omega, n_inner):
    key = (h, w, c, mode, n_inner)
    if key not in _wants:
        f1, f2, warp, u, v = _level(oracle, h, w, c)
        _wants[key] = oracle.smoothflow_sor(f1, f2, warp, u, v, ALPHA, N_OUTER, n_inner, N_SOR, omega=omega, mode=mode)
    return _wants[key]


@pytest.mark.parametrize("c", [3, 2])
@pytest.mark.parametrize("n_inner", [1, 2])
@pytest.mark.parametrize("mode,omega", MODES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_level_chain_has_the_oracles_bytes(gpu, oracle, h, w, mode, omega, n_inner, c):
    f1, f2, warp, u, v = _level(oracle, h, w, c)
    if h * w <= 10:  # (the start flow does what the shapes are here for)
        i, j = np.mgrid[0:h, 0:w]
        assert ((j + u < 0) | (j + u > w - 1) | (i + v < 0) | (i + v > h - 1)).any()
    want = _want(oracle, h, w, c, mode, omega, n_inner)
    got = gpu.smoothflow_sor(f1, f2, warp, u, v, ALPHA, N_OUTER, n_inner, N_SOR, omega=omega, mode=mode)
    what = "%dx%d C=%d mode %d n_inner %d: " % (h, w, c, mode, n_inner)
    for name, g, w_ in zip(("warp", "u", "v"), got, want):
        print("%s%-4s max-abs %.3e" % (what, name, float(np.abs(g - w_).max())))
    for name, g, w_ in zip(("warp", "u", "v"), got, want):
        _same_bytes(g, w_, what + name)


def test_two_channel_call_has_the_oracles_bytes(gpu, oracle):
    a, b = cases.load_pair("240")
    a = np.ascontiguousarray(a[40:77, 60:113, :2])
    b = np.ascontiguousarray(b[40:77, 60:113, :2])
    got = gpu.coarse2fine_flow(a, b, 2)[:3]
    want = oracle.coarse2fine_flow(a, b, 2)[:3]
    for name, g, w_ in zip(("vx", "vy", "warpI2"), got, want):
        print("37x53 C=2 L2 %-6s max-abs %.3e" % (name, float(np.abs(g - w_).max())))
    for name, g, w_ in zip(("vx", "vy", "warpI2"), got, want):
        _same_bytes(g, w_, "37x53 C=2 L2 " + name)
