"""CPU-side checks of the video mosaics (papteam_opticalflow_amd/tensors.py: mosaic, mosaic_transforms, neighbour_transforms,
panorama, stabilize_video_full; include/papof.h: papof_mosaic_tensor): known answers of every clause of the numpy fp64
restatement in tests/_mosaic_ref.py that tests/test_gpu_mosaic.py compares the device's bytes with, the two matrix helpers
against their restatements, a clean-plate scene and a border-fill scene cut from the committed 960 x 540 frame, every Python
argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through ctypes.  No
device is touched here."""
import ctypes
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _inpaint_ref import fill_reference  # noqa: E402
from _mosaic_ref import (canvas_reference, canvas_truth, clean_plate_scene, first_order, lower_median,  # noqa: E402
                         mosaic_reference, neighbour_reference, psnr, sample_world, shaky_scene)
from _stab_ref import corner_distance, path_reference, warp_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402

ID = np.eye(2, 3)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _stack(values, **kw):
    """one output pixel over len(values) 1 x 1 one-channel float64 frames under identity matrices"""
    f = np.array(values, np.float64).reshape(-1, 1, 1, 1)
    M = np.tile(ID, (1, len(values), 1, 1))
    out, cnt = mosaic_reference(f, None, M, (1, 1), kw.pop("mode", "median"), **kw)
    return out[0, 0, 0, 0], int(cnt[0, 0, 0])


def _before(a, b):
    return a < b or (not math.isnan(a) and math.isnan(b))


def _lower_median(values):
    """the rule, literally: order by (value, k), take index (n - 1) // 2"""
    def cmp(p, q):
        if _before(p[1], q[1]):
            return -1
        if _before(q[1], p[1]):
            return 1
        return p[0] - q[0]
    s = sorted(enumerate(values), key=functools.cmp_to_key(cmp))
    return s[(len(values) - 1) // 2][1]


# ---- every clause, by hand
def test_the_median_index_for_one_to_six_samples():
    vals = [5.0, 1.0, 4.0, 2.0, 6.0, 3.0]
    want = {1: 5.0, 2: 1.0, 3: 4.0, 4: 2.0, 5: 4.0, 6: 3.0}  # sorted[(n - 1) // 2]: the lower of the two middle ones
    for n in range(1, 7):
        got, cnt = _stack(vals[:n])
        assert got == want[n] == sorted(vals[:n])[(n - 1) // 2] and cnt == n


def _select(values):
    """lower_median of one pixel's samples, all live"""
    return lower_median(np.array(values, np.float64).reshape(-1, 1, 1), np.ones((len(values), 1), bool))[0, 0]


def test_ties_are_broken_by_k_shown_by_the_sign_of_zero():
    """Among SAMPLES: the bilinear rule adds its taps to +0.0, so a frame's -0.0 is sampled as +0.0 and two samples that
    compare equal have the same bits (NaNs aside) -- the order by k shows in the selection alone, not through frames."""
    for vals in ([-0.0, 0.0], [0.0, -0.0], [0.0, -0.0, -0.0, 0.0], [-0.0, 0.0, 0.0, -0.0], [1.0, -0.0, 0.0, -1.0],
                 [0.0, 0.0, -0.0], [-0.0, -0.0, 0.0, 0.0, 5.0, -5.0]):
        got, want = _select(vals), _lower_median(vals)
        assert _bits(got) == _bits(want), (vals, got, want)
    assert math.copysign(1.0, _select([-0.0, 0.0])) == -1.0 and math.copysign(1.0, _select([0.0, -0.0])) == 1.0
    assert math.copysign(1.0, _select([0.0, -0.0, -0.0, 0.0])) == -1.0   # index 1 of (0, -0, -0, 0) in k order
    rng = np.random.default_rng(1)
    pool = np.array([math.nan, math.inf, -math.inf, 0.0, -0.0, 1.0, 1.0, 5e-324, -5e-324, 2.5])
    for _ in range(300):
        vals = list(rng.choice(pool, rng.integers(1, 9)))
        assert _bits(_select(vals)) == _bits(_lower_median(vals)), vals
    # through frames under identity matrices the sign is gone before the samples are ordered
    assert math.copysign(1.0, _stack([-0.0, 0.0])[0]) == 1.0 and math.copysign(1.0, _stack([-0.0], mode="first")[0]) == 1.0
    # dead samples take no part, whatever their value
    S = np.array([7.0, -0.0, 9.0, 0.0]).reshape(4, 1, 1)
    assert math.copysign(1.0, lower_median(S, np.array([[False], [True], [False], [True]]))[0, 0]) == -1.0
    assert lower_median(S, np.zeros((4, 1), bool))[0, 0] == 0.0


def test_nan_sorts_last_and_infinities_in_their_place():
    nan, inf = math.nan, math.inf
    assert _stack([nan, 1.0, 2.0])[0] == 2.0          # 1, 2, NaN -> index 1
    assert _stack([nan, 1.0])[0] == 1.0               # 1, NaN -> index 0
    assert math.isnan(_stack([nan, nan, 1.0])[0])     # 1, NaN, NaN -> index 1
    assert _select([inf, nan, -inf, 0.0]) == 0.0      # -inf, 0, inf, NaN -> index 1
    assert _select([inf, nan, 3.0]) == inf
    assert _stack([inf, 3.0, 4.0])[0] == 4.0          # through a frame an infinity meets taps of weight 0: a NaN sample
    rng = np.random.default_rng(1)
    pool = np.array([nan, 0.0, 1.0, 1.0, 5e-324, -5e-324, 2.5, -3.0])
    for _ in range(200):
        vals = list(rng.choice(pool, rng.integers(1, 9)))
        assert _bits(_stack(vals)[0]) == _bits(_lower_median(vals)), vals


def test_first_and_mean_follow_k_order():
    assert _stack([3.0, 1.0, 2.0], mode="first") == (3.0, 3)
    assert _stack([3.0, 1.0, 2.0], mode="mean") == (((3.0 + 1.0) + 2.0) / 3.0, 3)
    a, b, c = 1e16, 1.0, -1e16                        # the order of the additions shows
    assert _stack([a, b, c], mode="mean")[0] == ((0.0 + a) + b + c) / 3.0 == 0.0
    assert _stack([a, c, b], mode="mean")[0] == 1.0 / 3.0
    assert math.copysign(1.0, _stack([-0.0], mode="mean")[0]) == 1.0   # added from +0.0


def test_dead_sources_and_an_empty_pixel():
    f = np.arange(1.0, 5.0).reshape(4, 1, 1, 1)
    M = np.tile(ID, (1, 4, 1, 1))
    for mode, want in (("first", 2.0), ("mean", 3.0), ("median", 2.0)):
        out, cnt = mosaic_reference(f, [[-1, 1, -1, 3]], M, (1, 1), mode)
        assert out[0, 0, 0, 0] == want and cnt[0, 0, 0] == 2
    # repeated sources count each time
    out, cnt = mosaic_reference(f, [[2, 2, 0, 2]], M, (1, 1), "median")
    assert out[0, 0, 0, 0] == 3.0 and cnt[0, 0, 0] == 4
    for bad in (math.nan, math.inf, -math.inf):
        for i in range(6):
            B = M.copy()
            B[0, 0].flat[i] = bad                      # any entry: X or Y is NaN or infinite at every pixel
            out, cnt = mosaic_reference(f[:2], None, B[:, :2], (2, 3), "first")
            assert (cnt == 0).all() or (out[cnt > 0] == 2.0).all()
            out, cnt = mosaic_reference(f[:1], None, B[:, :1], (2, 3), "mean")
            assert (cnt == 0).all() and (out == 0).all()
    # a singular matrix sends every pixel to one point: live everywhere
    Z = np.array([[[[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]]])
    out, cnt = mosaic_reference(f[:1], None, Z, (3, 2), "median")
    assert (out == 1.0).all() and (cnt == 1).all()
    out, cnt = mosaic_reference(f, [[-1, -1, -1, -1]], M, (1, 1), "median", out_dtype=np.uint8)
    assert out[0, 0, 0, 0] == 0 and cnt[0, 0, 0] == 0 and out.dtype == np.uint8


def test_a_mask_under_a_zero_weight_tap_does_not_kill_a_source():
    f = np.array([[[[1.0], [2.0], [3.0]]]])            # one 1 x 3 frame
    mask = np.zeros((1, 1, 3), np.uint8)
    mask[0, 0, 1] = 1
    at = lambda tx: np.array([[[[1.0, 0.0, tx], [0.0, 1.0, 0.0]]]])  # noqa: E731
    # x = 0 exactly: the taps at column 1 have weight 0
    out, cnt = mosaic_reference(f, None, at(0.0), (1, 1), "first", masks=mask)
    assert out[0, 0, 0, 0] == 1.0 and cnt[0, 0, 0] == 1
    out, cnt = mosaic_reference(f, None, at(0.25), (1, 1), "first", masks=mask)
    assert out[0, 0, 0, 0] == 0.0 and cnt[0, 0, 0] == 0
    out, cnt = mosaic_reference(f, None, at(2.0), (1, 1), "first", masks=mask)  # the clamped neighbour is column 2 itself
    assert out[0, 0, 0, 0] == 3.0 and cnt[0, 0, 0] == 1
    out, cnt = mosaic_reference(f, None, at(1.0), (1, 1), "first", masks=mask)
    assert cnt[0, 0, 0] == 0


def test_one_source_is_warp_affine():
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, (3, 17, 23, 3)).astype(np.uint8)
    M = np.array([[[1.01, 0.02, 1.5], [-0.015, 0.985, -0.7]], [[1.0, 0.0, 30.0], [0.0, 1.0, 0.0]],
                  [[0.9, 0.1, 2.0], [-0.1, 0.9, 3.0]]])
    want, valid = warp_reference(f, M, np.uint8)
    for mode in ("first", "mean", "median"):
        out, cnt = mosaic_reference(f, np.arange(3)[:, None], M[:, None], (17, 23), mode, out_dtype=np.uint8)
        assert out.tobytes() == want.tobytes() and ((cnt > 0) == valid).all(), mode
    px = np.array([[2, 5, 7], [0, 16, 22], [1, 0, 0]])
    out, cnt = mosaic_reference(f, np.arange(3)[:, None], M[:, None], (17, 23), "median", out_dtype=np.uint8, pixels=px)
    assert (out == want[px[:, 0], px[:, 1], px[:, 2]]).all() and (cnt == valid[px[:, 0], px[:, 1], px[:, 2]]).all()


# ---- the matrix helpers
def _motions(T, seed, H=45, W=64):
    rng = np.random.default_rng(seed)
    A = []
    for _ in range(T - 1):
        th, s = rng.normal(0, 0.01), 1 + rng.normal(0, 0.005)
        a, b = s * math.cos(th), s * math.sin(th)
        A.append([[a, -b, rng.normal(4, 2)], [b, a, rng.normal(1, 1)]])
    return np.array(A)


def test_mosaic_transforms_is_the_restated_canvas():
    H, W = 45, 64
    for T, ref, margin in ((2, None, 0), (7, None, 3), (8, 0, 0), (8, 7, 1), (12, 5, 0)):
        A = _motions(T, T)
        M, size, origin = tensors.mosaic_transforms(torch.from_numpy(A), (H, W), ref=ref, margin=margin)
        wm, wsize, worigin = canvas_reference(A, (H, W), ref, margin)
        assert M.dtype == torch.float64 and tuple(M.shape) == (1, T, 2, 3) and size == wsize and origin == worigin
        assert max(corner_distance(M[0, t].numpy(), wm[t], *size) for t in range(T)) < 1e-9
        # every frame's corners land on the canvas, and the reference frame is the canvas shifted
        r = (T - 1) // 2 if ref is None else ref
        assert np.abs(M[0, r].numpy() - np.array([[1.0, 0.0, origin[0]], [0.0, 1.0, origin[1]]])).max() < 1e-12
        for t in range(T):
            inv = np.linalg.inv(np.vstack([M[0, t].numpy(), [0, 0, 1]]))
            for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
                p = inv @ np.array([cx, cy, 1.0])
                assert margin - 1e-9 <= p[0] <= size[1] - 1 - margin + 1e-9 and margin - 1e-9 <= p[1] <= size[0] - 1 - margin + 1e-9
    # a Motion: pairs with ok False enter as the identity
    A = _motions(6, 9)
    ok = torch.ones(5, dtype=torch.bool)
    ok[2] = False
    got = tensors.mosaic_transforms(tensors.Motion(torch.from_numpy(A), ok, torch.ones(5)), (H, W))
    B = A.copy()
    B[2] = ID
    want = canvas_reference(B, (H, W))
    assert got[1:] == want[1:] and np.abs(got[0][0].numpy() - want[0]).max() < 1e-9


def test_neighbour_transforms_is_the_restatement():
    H, W = 45, 64
    for T, radius in ((2, 0), (5, 1), (6, 4), (4, 9)):
        A = _motions(T, 20 + T)
        M = path_reference(A, 3)
        src, mats = tensors.neighbour_transforms(torch.from_numpy(M), torch.from_numpy(A), radius)
        ws, wm = neighbour_reference(M, A, radius)
        assert src.dtype == torch.int32 and tuple(src.shape) == (T, 2 * radius + 1) and (src.numpy() == ws).all()
        assert mats.dtype == torch.float64 and tuple(mats.shape) == (T, 2 * radius + 1, 2, 3)
        live = ws >= 0
        d = max(corner_distance(mats[t, k].numpy(), wm[t, k], H, W) for t in range(T) for k in range(2 * radius + 1)
                if live[t, k])
        assert d < 1e-9
        assert (src[:, 0].numpy() == np.arange(T)).all() and np.abs(mats[:, 0].numpy() - M).max() == 0
        for t in range(T):
            for dd in range(1, radius + 1):
                assert ws[t, 2 * dd - 1] == (t - dd if t - dd >= 0 else -1) and ws[t, 2 * dd] == (t + dd if t + dd < T else -1)


# ---- the scenes
@pytest.fixture(scope="module")
def plate():
    frames, Ks, A, world = clean_plate_scene()
    M, size, origin = canvas_reference(A, frames.shape[1:3])
    return frames, Ks, A, world, M, size, origin


def test_clean_plate_median_beats_mean_beats_first(plate):
    """Nine 96 x 160 frames panning over the committed 960 x 540 frame with a 24 x 24 saturated square moving across them,
    exact matrices; PSNR against the world over the canvas pixels that at least three frames cover.  Measured with this
    restatement over 22748 pixels: MEDIAN 36.57 dB, MEAN 26.98 dB, FIRST 22.20 dB.  Only the order is asserted."""
    frames, Ks, A, world, M, size, origin = plate
    T = len(frames)
    ref = (T - 1) // 2
    truth = canvas_truth(world, Ks[ref], origin, size)
    res = {}
    for mode in ("median", "mean", "first"):
        order = first_order(T, ref) if mode == "first" else list(range(T))
        out, cnt = mosaic_reference(frames, [order], M[order][None], size, mode)
        where = (cnt[0] >= 3) & np.isfinite(truth).all(-1)
        res[mode] = psnr(out[0], truth, where)
    print("clean plate over %d pixels: MEDIAN %.2f dB, MEAN %.2f dB, FIRST %.2f dB" % (
        int(where.sum()), res["median"], res["mean"], res["first"]))
    assert where.sum() > 10000
    assert res["median"] > res["mean"] > res["first"], res


def test_border_fill_covers_what_a_neighbour_saw_and_beats_a_spatial_fill():
    """Nine frames under a pan of (3, 1) plus Gaussian shake of 5 px and 0.02 rad, exact motions, path radius 15, no crop,
    fill radius 4.  Measured with this restatement: 7.8 % of the pixels invalid, 99.8 % of those filled, 37.19 dB over the
    filled pixels against 17.76 dB for fill_reference (pull-push, relax 0) on the same holes."""
    frames, Ks, A, world = shaky_scene()
    T, H, W, _ = frames.shape
    M = path_reference(A, 15)
    src, mats = neighbour_reference(M, A, 4)
    out, cnt = mosaic_reference(frames, src, mats, (H, W), "first")
    warped, valid = warp_reference(frames, M)
    assert (out[valid] == warped[valid]).all()           # where the frame itself covers, it is the stabilized frame
    filled = (cnt > 0) & ~valid
    # every pixel filled has some neighbour covering it, and the reverse
    covered = np.zeros((T, H, W), bool)
    for t in range(T):
        for k in range(1, src.shape[1]):
            if src[t, k] >= 0:
                covered[t] |= warp_reference(frames[src[t, k]][None], mats[t, k][None])[1][0]
    assert (filled == (covered & ~valid)).all()
    truth = np.stack([sample_world(world, Ks[t] @ np.vstack([M[t], [0, 0, 1]]), H, W) for t in range(T)])
    spatial = fill_reference(warped, ~valid, 0)
    ours, theirs = psnr(out, truth, filled), psnr(spatial, truth, filled)
    print("border fill: %.1f %% invalid, %.1f %% of those filled, %.2f dB against %.2f dB for the spatial fill" % (
        100 * (~valid).mean(), 100 * filled.sum() / max(1, (~valid).sum()), ours, theirs))
    assert filled.sum() > 1000 and ours > theirs, (ours, theirs)


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")


_M = lambda n_out=1, N=3: _z(n_out, N, 2, 3, dtype=torch.float64)  # noqa: E731


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.mosaic(_z(3, 3, 8, 8), None, _M(), (8, 8)), ValueError),                        # CPU tensors
    (lambda: tensors.panorama(_z(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.stabilize_video_full(_z(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.mosaic(None, None, _M(), (8, 8)), TypeError),
    (lambda: tensors.panorama(None, 2), TypeError),
    (lambda: tensors.stabilize_video_full(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError), (dict(frames=_z(3, 8)), ValueError),
    (dict(frames=_z(3, 3, 0, 8)), ValueError), (dict(layout="HWC"), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.bool), TypeError),
    (dict(mode="max"), ValueError), (dict(mode=None), ValueError), (dict(mode=2), ValueError),
    (dict(size=(8,)), TypeError), (dict(size=8), TypeError), (dict(size=(0, 8)), ValueError), (dict(size=(8.0, 8)), ValueError),
    (dict(size=(True, 8)), ValueError),
    (dict(matrices=None), TypeError), (dict(matrices=_z(1, 3, 2, 3, dtype=torch.float16)), TypeError),
    (dict(matrices=_z(3, 2, 3)), ValueError), (dict(matrices=_z(1, 3, 3, 3)), ValueError), (dict(matrices=_z(1, 0, 2, 3)), ValueError),
    (dict(matrices=_z(1, 3, 2, 3, device="meta")), ValueError),
    (dict(matrices=_M(1, 2)), ValueError),                                                               # None needs N = T
    (dict(sources=torch.zeros(1, 3)), TypeError), (dict(sources=np.zeros((1, 3))), TypeError), (dict(sources="abc"), TypeError),
    (dict(sources=torch.zeros(1, 3, dtype=torch.bool)), TypeError),
    (dict(sources=torch.zeros(2, 3, dtype=torch.int64)), ValueError), (dict(sources=[[0, 1]]), ValueError),
    (dict(sources=[[0, 1, 3]]), ValueError),                                                              # frame 3 of 3
    (dict(masks=_z(3, 8, 8)), TypeError), (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError), (dict(masks=[1]), TypeError),
    (dict(masks=_z(3, 8, 8, dtype=torch.uint8, device="meta")), ValueError),
    (dict(matrices=_M(1, 256), sources=torch.zeros(1, 256, dtype=torch.int32), mode="mean"), ValueError),
    (dict(matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),                # the median's 64
])
def test_mosaic_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _M())
    sources, size = kw.pop("sources", None), kw.pop("size", (8, 8))
    with pytest.raises(exc):
        tensors.mosaic(frames, sources, matrices, size, **kw)
    assert stub == []


def test_mosaic_accepts_the_bounds_of_its_slots(monkeypatch):
    """255 sources for the mean and 64 for the median pass every check and reach the launch"""
    _on_gpu_stub(monkeypatch)
    reached = []

    def launch(dev, name, *args, **kw):
        reached.append((name, args[7]))

    monkeypatch.setattr(tensors, "_launch", launch)
    tensors.mosaic(_z(3, 3, 8, 8), torch.zeros(1, 255, dtype=torch.int64), _M(1, 255), (4, 4), mode="mean")
    tensors.mosaic(_z(3, 3, 8, 8), np.zeros((2, 64), np.int16) - 5, _M(2, 64), (4, 4))
    out, cnt = tensors.mosaic(_z(3, 8, 8), [[0]], _M(1, 1), (4, 5), mode="first", layout="NHWC", out_dtype=torch.uint8)
    assert reached == [("papof_mosaic_tensor", 255), ("papof_mosaic_tensor", 64), ("papof_mosaic_tensor", 1)]
    assert tuple(out.shape) == (1, 4, 5, 8) and out.dtype == torch.uint8 and tuple(cnt.shape) == (1, 4, 5)


@pytest.mark.parametrize("kw,exc", [
    (dict(motion=_z(4, 3, 3)), ValueError), (dict(motion=_z(0, 2, 3)), ValueError), (dict(motion=[1]), TypeError),
    (dict(size=(8,)), TypeError), (dict(size=(0, 8)), ValueError),
    (dict(ref=5), ValueError), (dict(ref=-1), ValueError), (dict(ref=1.0), ValueError),
    (dict(margin=-1), ValueError), (dict(margin=0.5), ValueError),
    (dict(max_pixels=100), ValueError), (dict(max_pixels=0), ValueError),
    (dict(motion=torch.full((4, 2, 3), math.nan, dtype=torch.float64)), ValueError),
    (dict(motion=torch.full((4, 2, 3), 1e200, dtype=torch.float64)), ValueError),
])
def test_mosaic_transforms_errors(kw, exc):
    motion = kw.pop("motion", torch.from_numpy(np.tile(ID, (4, 1, 1))))
    size = kw.pop("size", (20, 30))
    with pytest.raises(exc):
        tensors.mosaic_transforms(motion, size, **kw)


@pytest.mark.parametrize("kw,exc", [
    (dict(transforms=None), TypeError), (dict(transforms=_z(4, 2, 3)), ValueError), (dict(transforms=_z(5, 3, 3)), ValueError),
    (dict(motion=[1]), TypeError), (dict(motion=_z(4, 3, 3)), ValueError),
    (dict(radius=-1), ValueError), (dict(radius=128), ValueError), (dict(radius=1.0), ValueError), (dict(radius=True), ValueError),
    (dict(motion=torch.zeros(4, 2, 3, dtype=torch.float64)), ValueError),
])
def test_neighbour_transforms_errors(kw, exc):
    """(a singular pair motion makes the camera path singular: a ValueError, as mosaic_transforms gives)"""
    transforms = kw.pop("transforms", _z(5, 2, 3, dtype=torch.float64))
    motion = kw.pop("motion", torch.from_numpy(np.tile(ID, (4, 1, 1))))
    with pytest.raises(exc):
        tensors.neighbour_transforms(transforms, motion, kw.pop("radius", 2))


@pytest.mark.parametrize("kw,exc", [
    (dict(mode="mode"), ValueError), (dict(ref=3), ValueError), (dict(ref=-1), ValueError), (dict(step=0), ValueError),
    (dict(step=1.0), ValueError), (dict(margin=-1), ValueError), (dict(masks=_z(3, 8, 8)), TypeError),
    (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError), (dict(model="projective"), ValueError), (dict(iters=0), ValueError),
    (dict(scale=-2.0), ValueError), (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError),
    (dict(bogus=1), TypeError),
])
def test_panorama_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.panorama(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


def test_panorama_names_step_when_too_many_frames_are_deposited(stub, monkeypatch):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama(_z(65, 1, 8, 8).expand(65, 3, 8, 8), 2)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama(_z(256, 1, 8, 8).expand(256, 3, 8, 8), 2, mode="mean")
    with pytest.raises(ValueError, match="step"):
        tensors.panorama(_z(130, 1, 8, 8).expand(130, 3, 8, 8), 2, step=2)
    with pytest.raises(ValueError):
        tensors.panorama(_z(1, 3, 8, 8), 2)
    with pytest.raises(ValueError):
        tensors.panorama(_z(3, 3, 8, 8), 0)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(fill_radius=-1), ValueError), (dict(fill_radius=128), ValueError), (dict(fill_radius=1.5), ValueError),
    (dict(fill_radius=True), ValueError), (dict(model="projective"), ValueError), (dict(radius=-1), ValueError),
    (dict(crop=0.0), ValueError), (dict(crop="all"), TypeError), (dict(iters=0), ValueError), (dict(scale=-2.0), ValueError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="CHW"), ValueError), (dict(bogus=1), TypeError),
])
def test_stabilize_video_full_errors(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.stabilize_video_full(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_F64, strides=(192, 24, 3, 1), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_OK = "ok"


def _call(lib, h, n_frames=3, size=(8, 8, 3), fr=_OK, masks=None, n_out=2, n_src=3, canvas=(5, 9), sources=0x3000, mat=_OK,
          mode=capi.MOSAIC_MEDIAN, out=_OK, count=None):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "mat": lambda: _t(capi.DTYPE_F32, (18, 6, 3, 1)), "out": lambda: _t(capi.DTYPE_F64)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mat=mat, out=out).items()}
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return lib.papof_mosaic_tensor(h, n_frames, size[0], size[1], size[2], ref(d["fr"]), ref(masks), n_out, n_src, canvas[0],
                                   canvas[1], sources, ref(d["mat"]), mode, ref(d["out"]), ref(count), None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mat=None), dict(out=None), dict(sources=None),                                  # NULL
    dict(fr=_t(data=0)), dict(mat=_t(data=0)), dict(out=_t(data=0)), dict(masks=_t(capi.DTYPE_U8, data=0)),
    dict(count=_t(capi.DTYPE_U8, data=0)),
    dict(fr=_t(dtype=3)), dict(mat=_t(capi.DTYPE_U8, (18, 6, 3, 1))), dict(out=_t(dtype=-1)),             # dtypes
    dict(masks=_t(capi.DTYPE_F32, (64, 8, 1, 0))), dict(count=_t(capi.DTYPE_F64, (64, 8, 1, 0))),
    dict(fr=_t(strides=(192, 24, 3, -1))), dict(fr=_t(strides=(-192, 24, 3, 1))),                       # strides
    dict(mat=_t(strides=(18, -6, 3, 1))), dict(mat=_t(strides=(18, 6, 3, -1))),
    dict(masks=_t(capi.DTYPE_U8, (64, -8, 1, 0))),
    dict(out=_t(strides=(192, 24, 3, 0))), dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(192, 24, -3, 1))),
    dict(count=_t(capi.DTYPE_U8, (64, 8, 0, 0))), dict(count=_t(capi.DTYPE_U8, (0, 8, 1, 0))),
    dict(n_src=0), dict(n_src=-1), dict(n_src=256), dict(n_src=256, mode=capi.MOSAIC_MEAN),               # slots
    dict(n_src=65), dict(n_src=255),                                                                     # the median's 64
    dict(mode=3), dict(mode=-1),
    dict(n_frames=0), dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)), dict(n_out=0),   # sizes
    dict(canvas=(0, 9)), dict(canvas=(5, 0)), dict(canvas=(-5, 9)),
])
def test_c_abi_refuses(kw):
    lib = _lib()
    assert _call(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_without_a_handle():
    assert _call(_lib(), None) == -1


def test_the_constants_are_the_headers():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "papof.h")).read()
    for name, value in (("FIRST", capi.MOSAIC_FIRST), ("MEAN", capi.MOSAIC_MEAN), ("MEDIAN", capi.MOSAIC_MEDIAN),
                        ("MAX_SOURCES", capi.MOSAIC_MAX_SOURCES), ("MAX_MEDIAN", capi.MOSAIC_MAX_MEDIAN)):
        assert int(re.search(r"PAPOF_MOSAIC_%s = (\d+)" % name, header).group(1)) == value
    assert tensors.MAX_SOURCES == 255 and tensors.MAX_MEDIAN == 64
