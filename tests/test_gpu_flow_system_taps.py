"""k_flow_system's bilinear taps at the places where its paired 16-byte loads, its hoisted offsets and its passes by
wave could go wrong: flows that land on the last column and the last row, a hair inside them, one ulp outside the image on
each side, on frames with ragged tiles on both borders and on the narrowest widths.  A one-level call hands the caller's flow
to level 0 unchanged (tests/_init_ref.py: coarsest_init), so the flows below ARE what the kernel warps with.

Held to, for every case:
  * the default build's bytes are those of PAPOF_FUSED_SYSTEM=0 (k_warp_smooth_blend + k_assemble*), -0.0 != +0.0;
  * and those of the oracle composition (_init_ref.coarse2fine_init), as tests/test_gpu_init_flow.py compares;
  * a batch of three pairs (the batched instantiations) gives each pair the bytes of its single call.
That the fused kernel and the intended solver are what ran is asserted, not assumed: the rule of api.hip restated (a level
of at most 16 rows and 64 columns keeps the pair of kernels for the guard; none of the shapes is one) plus the guard's
counters (no exact pass, no rerun), and the solver kind from last_sor_solves().  Where the guard does run a call again in
its exact pass -- the pair of kernels -- comparing that call would be vacuous: k_flow_system's result is then taken from a
handle without the guard (see the test), and a case is skipped, with its reason, only where the reference's guard really
trips -- allowed at one column, a failure anywhere else."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402
from _init_ref import coarse2fine_init  # noqa: E402
from _libs import OracleLib  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KIND_TINY = 6  # include/papof.h: papof_last_sor_solves
TINY_MAX_CELLS = 8192  # csrc/common.h: kTinyMaxCells
# ragged tiles on both borders and more than one block: two shapes of k_sor_tiny (row-major operands), one just above its
# limit (skewed operands); the narrowest widths with more than 16 rows
SHAPES = [(17, 33), (37, 53), (83, 99), (24, 1), (24, 2), (24, 3)]
FLOWS = ["last_col_row", "near_last_col", "ulp_outside", "zero", "random3"]


def _close_handles():
    from papteam_opticalflow_amd import tensors
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


@pytest.fixture(scope="module", autouse=True)
def handles():
    yield
    _close_handles()


def _gpu():
    """the handle of device 0 the tensor calls use -- a fresh one when the last call left it in the guard's exact pass
    (sticky: the pair of kernels would assemble the next call as well)"""
    from papteam_opticalflow_amd import tensors
    if tensors._handle(0)[0].lap_guard_stats()["exact_next"]:
        _close_handles()
    return tensors._handle(0)[0]


@pytest.fixture(scope="module")
def orc():
    return OracleLib()


def _frames(h, w, gray):
    """uint8 HWC frames cut from the committed 240 fixture"""
    a, b = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    sl = (slice(40, 40 + h), slice(60, 60 + w), slice(0, 1) if gray else slice(None))
    return np.ascontiguousarray(a[sl]), np.ascontiguousarray(b[sl])


def _flow(name, h, w):
    """(2, H, W) float64: u, v"""
    i, j = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = np.zeros((h, w)), np.zeros((h, w))
    if name == "last_col_row":  # integers: even rows land on column W - 1, every third column on row H - 1, both in the corner
        u = np.where(i % 2 == 0, w - 1 - j, 0.0)
        v = np.where(j % 3 == 0, h - 1 - i, 0.0)
    elif name == "near_last_col":  # even columns land at W - 1 - 2^-52 W, odd ones at W - 2
        u = np.where(j % 2 == 0, (w - 1 - 2.0 ** -52 * w) - j, (w - 2) - j)
        v = np.where(i % 4 == 0, (h - 1 - 2.0 ** -52 * h) - i, 0.0)
    elif name == "ulp_outside":  # the smallest step beyond each side (exactly one ulp of the border where j + u is exact)
        cls = (i * 7 + j * 3) % 5
        u = np.where(cls == 0, np.nextafter(w - 1 - j, np.inf), u)
        u = np.where(cls == 1, np.nextafter(-j, -np.inf), u)
        v = np.where(cls == 2, np.nextafter(h - 1 - i, np.inf), v)
        v = np.where(cls == 3, np.nextafter(-i, -np.inf), v)
    elif name == "random3":
        rng = np.random.default_rng(1000 * h + w)
        u, v = rng.uniform(-3, 3, (h, w)), rng.uniform(-3, 3, (h, w))
    else:
        assert name == "zero"
    return np.ascontiguousarray(np.stack([u, v]))


def test_the_flows_land_where_they_say():
    """(no GPU work: the constructions above, in the kernel's own arithmetic x = j + u)"""
    h, w = 37, 53
    i, j = np.mgrid[0:h, 0:w].astype(np.float64)
    f = _flow("last_col_row", h, w)
    assert ((j + f[0])[0::2] == w - 1).all() and ((i + f[1])[:, 0::3] == h - 1).all()
    f = _flow("near_last_col", h, w)
    x = j + f[0]
    assert (x[:, 1::2] == w - 2).all() and (x[:, 0::2] < w - 1).all() and (x[:, 0::2] > w - 1 - 1e-9).all()
    f = _flow("ulp_outside", h, w)
    x, y, cls = j + f[0], i + f[1], (i * 7 + j * 3) % 5
    assert (x[cls == 1] < 0).all() and (x[cls == 1] > -1e-9).all() and (y[cls == 3] < 0).all()
    assert (x[(cls == 0) & (j == 0)] == np.nextafter(w - 1.0, np.inf)).all() and (x[cls == 0] >= w - 1).all()
    assert (y[(cls == 2) & (i == 0)] == np.nextafter(h - 1.0, np.inf)).all() and (y[cls == 2] >= h - 1).all()


def _same_bytes(got, want, what):
    g = np.ascontiguousarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got)
    w_ = np.ascontiguousarray(want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want)
    assert g.shape == w_.shape and g.dtype == w_.dtype, (what, g.shape, w_.shape, g.dtype, w_.dtype)
    if g.tobytes() != w_.tobytes():
        raise AssertionError("%s: %d elements differ, max-abs %.3e" % (what, int((g.view(np.int64) != w_.view(np.int64)).sum()),
                                                                        float(np.abs(g - w_).max())))


_singles = {}


def _single(h, w, gray, name):
    """(flow (2, H, W), warp (H, W, C), fused) of the default build's single call; fused: k_flow_system assembled the call's
    result (False: the guard ran the call again in its exact pass, that is through the pair of kernels)"""
    key = (h, w, gray, name)
    if key not in _singles:
        from papteam_opticalflow_amd.tensors import flow_pairs
        a, b = _frames(h, w, gray)
        ta, tb = torch.from_numpy(a[None]).cuda(), torch.from_numpy(b[None]).cuda()
        init = torch.from_numpy(_flow(name, h, w)).cuda()
        gpu = _gpu()
        before = gpu.lap_guard_stats()
        assert not before["exact_next"], before
        flow, warp, _ = flow_pairs(ta, tb, 1, layout="NHWC", init_flow=init)
        after = gpu.lap_guard_stats()
        # api.hip: the one-kernel form unless the level is one block of the guard's (<= 16 rows and <= 64 columns) or the
        # guard's exact pass runs
        assert h > 16, "a one-block level: the pair of kernels, not k_flow_system"
        fused = (after["reruns"], after["exact_calls"]) == (before["reruns"], before["exact_calls"])
        kinds = {s["kind"] for s in gpu.last_sor_solves() if (s["h"], s["w"]) == (h, w)}
        assert kinds, gpu.last_sor_solves()
        if h * w <= TINY_MAX_CELLS:
            assert kinds == {KIND_TINY}, kinds  # row-major operands
        else:
            assert KIND_TINY not in kinds, kinds  # skewed operands
        _singles[key] = (flow[0].clone(), warp[0].clone(), fused)
    return _singles[key]


class _guard_off:
    """handles made inside have no Laplacian-noise guard (PAPOF_LAP_GUARD=0 is read when a handle is made): a call keeps
    what k_flow_system assembled whatever the witnesses say"""

    def __enter__(self):
        _close_handles()
        os.environ["PAPOF_LAP_GUARD"] = "0"
        from papteam_opticalflow_amd import tensors
        assert not tensors._handle(0)[0].lap_guard_stats()["guard_on"]

    def __exit__(self, *exc):
        _close_handles()
        del os.environ["PAPOF_LAP_GUARD"]


def _equal(a, b):
    return all(np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes() ==
               np.ascontiguousarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y).tobytes()
               for x, y in zip(a, b))


@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
@pytest.mark.parametrize("name", FLOWS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_taps_against_the_pair_of_kernels_and_the_oracle(orc, monkeypatch, h, w, name, gray):
    """Where the guard kept the call's first pass (fused), that pass is compared.  Where it ran the call again -- a frame
    of two or three columns has a handful of sampled pixels, and flows pinned to a border push those out of the image with
    the first update, so a channel is left without a witness -- the guarded result must still be the oracle's, and
    k_flow_system's own result is taken from a handle WITHOUT the guard: against the pair of kernels on such a handle, and
    against the oracle, whose guard does not trip unless a channel's warp equals frame 1 in every pixel.  Only then (the
    unguarded result is not the oracle's, the guarded one is) is there nothing of k_flow_system to hold to the oracle: that
    is a skip with its reason, allowed at one column only."""
    from papteam_opticalflow_amd.tensors import flow_pairs
    flow, warp, fused = _single(h, w, gray, name)
    a, b = _frames(h, w, gray)
    ta, tb = torch.from_numpy(a[None]).cuda(), torch.from_numpy(b[None]).cuda()
    f0 = _flow(name, h, w)
    what = "%dx%d %s %s" % (h, w, name, "gray" if gray else "rgb")
    vx, vy, wi = coarse2fine_init(orc, a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0, 1,
                                  np.ascontiguousarray(f0.transpose(1, 2, 0)))
    _same_bytes(flow[0], vx, what + ": vx vs oracle")
    _same_bytes(flow[1], vy, what + ": vy vs oracle")
    _same_bytes(warp, wi, what + ": warpI2 vs oracle")

    def both_forms():
        one = flow_pairs(ta, tb, 1, layout="NHWC", init_flow=torch.from_numpy(f0).cuda())[:2]
        monkeypatch.setenv("PAPOF_FUSED_SYSTEM", "0")
        two = flow_pairs(ta, tb, 1, layout="NHWC", init_flow=torch.from_numpy(f0).cuda())[:2]
        monkeypatch.delenv("PAPOF_FUSED_SYSTEM")
        return (one[0][0].clone(), one[1][0].clone()), (two[0][0].clone(), two[1][0].clone())

    if fused:
        _gpu()
        one, two = both_forms()
        _same_bytes(one[0], flow, what + ": flow, the same call twice")
    else:
        print(what + ": the guard ran the call again in its exact pass; k_flow_system's result from a handle without the guard")
        with _guard_off():
            one, two = both_forms()
    _same_bytes(one[0], two[0], what + ": flow, one kernel vs two")
    _same_bytes(one[1], two[1], what + ": warpI2, one kernel vs two")
    if not fused and not _equal(one, (flow, warp)):
        assert w == 1, what + ": without the guard k_flow_system's call is not the oracle's, with it (pair of kernels) it is"
        pytest.skip(what + ": the reference's guard trips here (a channel's warp is frame 1 in every pixel), so the call is "
                    "assembled by the pair of kernels in the exact pass; k_flow_system agrees with them without the guard")
    _same_bytes(one[0][0], vx, what + ": vx vs oracle")
    _same_bytes(one[0][1], vy, what + ": vy vs oracle")
    _same_bytes(one[1], wi, what + ": warpI2 vs oracle")


@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
@pytest.mark.parametrize("names", [FLOWS[0:3], FLOWS[2:5]], ids=["borders", "outside-zero-random"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_a_batch_of_three_gives_each_pair_its_single_call(h, w, names, gray):
    """(the batched chain assembles with k_flow_system<.., BATCH> whatever the guard decides later: a pair it cannot prove runs
    again through the single call, and so has that call's bytes either way)"""
    from papteam_opticalflow_amd.tensors import flow_pairs
    singles = [_single(h, w, gray, n) for n in names]
    a, b = _frames(h, w, gray)
    ta = torch.from_numpy(np.stack([a] * 3)).cuda()
    tb = torch.from_numpy(np.stack([b] * 3)).cuda()
    init = torch.from_numpy(np.stack([_flow(n, h, w) for n in names])).cuda()
    assert tuple(init.shape) == (3, 2, h, w)
    flow, warp, _ = flow_pairs(ta, tb, 1, layout="NHWC", init_flow=init)
    for p, n in enumerate(names):
        f1, w1, _ = singles[p]
        _same_bytes(flow[p], f1, "%dx%d %s pair %d (%s): flow, batch vs single" % (h, w, "gray" if gray else "rgb", p, n))
        _same_bytes(warp[p], w1, "%dx%d %s pair %d (%s): warpI2, batch vs single" % (h, w, "gray" if gray else "rgb", p, n))
