"""CPU-side checks of the seamless mosaics (papteam_opticalflow_amd/tensors.py: mosaic with gains and mode "feather",
mosaic_overlap, exposure_gains, panorama(exposure=True); include/papof.h: papof_mosaic_blend_tensor,
papof_mosaic_overlap_tensor): known answers of every clause of the numpy fp64 restatement in tests/_blend_ref.py that
tests/test_gpu_blend.py compares the device's output with, exposure_gains against its closed form and its restatement, the
exposure scene (tests/_mosaic_ref.py's pan, every frame under a gain of its own) whose figures the README quotes, every
Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through ctypes.
No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _blend_ref import (MODES, ONE, blend_reference, energy, exposure_scene, gains_reference, gather,  # noqa: E402
                        overlap_reference, scaled_psnr, scene_gains, seam_step)
from _mosaic_ref import canvas_reference, canvas_truth, mosaic_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402

ID = np.eye(2, 3)


def _shift(tx, ty=0.0):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty]])


# ---- every clause, by hand
def test_feather_weights_by_hand():
    """Two 5 x 5 constant frames, the second shifted by two columns.  At canvas pixel (2, 2) frame 0 is read at its centre
    (w = 2 + 1) and frame 1 at (4, 2), on its border (w = 0 + 1); at (1, 0) frame 0 is on its border and frame 1 at (3, 0)."""
    f = np.stack([np.full((5, 5, 1), 0.25), np.full((5, 5, 1), 0.75)])
    M = np.stack([ID, _shift(2.0)])[None]
    out, cnt = blend_reference(f, None, M, (5, 5), "feather")
    assert out[0, 2, 2, 0] == (3.0 * 0.25 + 1.0 * 0.75) / 4.0 and cnt[0, 2, 2] == 2
    assert out[0, 0, 1, 0] == (1.0 * 0.25 + 1.0 * 0.75) / 2.0
    assert out[0, 2, 1, 0] == (2.0 * 0.25 + 2.0 * 0.75) / 4.0   # (1, 2) and (3, 2): both one pixel from a border
    assert out[0, 2, 3, 0] == 0.25 and cnt[0, 2, 3] == 1          # frame 1 would be read at column 5: outside
    # with gains: v = g * sample enters the weighted sum
    out, _ = blend_reference(f, None, M, (5, 5), "feather", np.array([[2.0, 0.5]]))
    assert out[0, 2, 2, 0] == (3.0 * (2.0 * 0.25) + 1.0 * (0.5 * 0.75)) / 4.0
    # a half-pixel shift: the weight follows the sampled point, not the pixel
    out, _ = blend_reference(f, None, np.stack([ID, _shift(0.5)])[None], (5, 5), "feather")
    assert out[0, 2, 1, 0] == (2.0 * 0.25 + 2.5 * 0.75) / 4.5


def test_one_row_frames_weigh_every_sample_one():
    """H = 1: min(Y, H1 - Y) = 0 everywhere, so w = 1 and FEATHER adds what MEAN adds"""
    rng = np.random.default_rng(0)
    f = rng.random((3, 1, 9, 2))
    M = np.stack([ID, _shift(1.5), _shift(-2.25)])[None]
    a, ca = blend_reference(f, None, M, (1, 9), "feather")
    b, cb = blend_reference(f, None, M, (1, 9), "mean")
    assert (ca == cb).all() and ca.max() == 3 and np.abs(a - b).max() < 1e-15
    assert (a[cb == 1] == b[cb == 1]).all()


def test_a_lone_live_source_returns_its_sample_whatever_its_weight():
    """(w v) / w: exact for the dyadic samples here at every weight met, within an ulp for any other"""
    f = np.zeros((2, 9, 9, 1))
    f[0] = 0.375
    rng = np.random.default_rng(1)
    g = rng.random((9, 9))
    f[1, :, :, 0] = g
    M = np.stack([ID, ID])[None]
    out, cnt = blend_reference(f, [[0, -1]], M, (9, 9), "feather")
    assert (out == 0.375).all() and (cnt == 1).all()
    out, cnt = blend_reference(f, [[-1, 1]], M, (9, 9), "feather")
    assert np.abs(out[0, :, :, 0] / g - 1).max() <= 2.0 ** -52 and (out[0, 0, :, 0] == g[0]).all()   # (w = 1 on the border)
    out, cnt = blend_reference(f, [[-1, -1]], M, (9, 9), "feather", out_dtype=np.uint8)
    assert (out == 0).all() and (cnt == 0).all() and out.dtype == np.uint8


def test_without_gains_the_old_modes_are_the_mosaic_byte_for_byte():
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, (5, 17, 23, 3)).astype(np.uint8)
    M = np.stack([_shift(rng.uniform(-6, 6), rng.uniform(-6, 6)) for _ in range(7)])[None]
    M[0, 2, 0, 0] = 0.9
    src = [[0, 1, -1, 2, 3, 3, 4]]
    mask = (rng.random((5, 17, 23)) < 0.1).astype(np.uint8)
    for mode in ("first", "mean", "median"):
        for dt in (np.float64, np.float32, np.uint8):
            want, wcnt = mosaic_reference(f, src, M, (20, 30), mode, mask, dt)
            got, cnt = blend_reference(f, src, M, (20, 30), mode, None, mask, dt)
            assert got.tobytes() == want.tobytes() and (cnt == wcnt).all(), (mode, dt)
            ones, _ = blend_reference(f, src, M, (20, 30), mode, np.ones((1, 7), np.float32), mask, dt)
            assert ones.tobytes() == want.tobytes()


def _stack(values, gains, mode):
    f = np.array(values, np.float64).reshape(-1, 1, 1, 1)
    M = np.tile(ID, (1, len(values), 1, 1))
    out, cnt = blend_reference(f, None, M, (1, 1), mode, np.array([gains], np.float64))
    return out[0, 0, 0, 0], int(cnt[0, 0, 0])


def test_gains_enter_before_the_mode():
    assert _stack([1.0, 2.0, 3.0], [5.0, 1.0, 1.0], "median") == (3.0, 3)     # 5, 2, 3 -> the middle one is 3
    assert _stack([1.0, 2.0, 3.0], [1.0, 1.0, 1.0], "median") == (2.0, 3)
    assert _stack([1.0, 2.0, 3.0], [2.5, 1.0, 0.5], "median") == (2.0, 3)     # 2.5, 2, 1.5
    assert _stack([1.0, 2.0, 4.0], [4.0, 2.0, 1.0], "median") == (4.0, 3)     # three equal values: ties by k, the bits of g v
    assert _stack([1.0, 2.0, 3.0], [5.0, 1.0, 1.0], "first") == (5.0, 3)
    assert _stack([1.0, 2.0, 3.0], [5.0, 1.0, 2.0], "mean") == (((5.0 + 2.0) + 6.0) / 3.0, 3)
    assert _stack([1.0, 2.0, 3.0], [5.0, 1.0, 2.0], "feather") == (((5.0 + 2.0) + 6.0) / 3.0, 3)   # 1 x 1 frames: w = 1
    # a NaN gain is a NaN value: last in the median, poison in the sums; an infinite gain is an infinite value
    assert _stack([1.0, 2.0, 3.0], [math.nan, 1.0, 1.0], "median") == (3.0, 3)
    assert math.isnan(_stack([1.0, 2.0, 3.0], [math.nan, 1.0, 1.0], "mean")[0])
    assert math.isnan(_stack([1.0, 2.0, 3.0], [1.0, math.nan, 1.0], "feather")[0])
    assert _stack([1.0, 2.0, 3.0], [math.inf, 1.0, 1.0], "median") == (3.0, 3)
    assert _stack([1.0, 2.0, 3.0], [math.inf, 1.0, 1.0], "first") == (math.inf, 3)
    # float32 gains are widened exactly
    f = np.full((1, 1, 1, 1), 3.0)
    out, _ = blend_reference(f, None, ID[None, None], (1, 1), "first", np.array([[0.1]], np.float32))
    assert out[0, 0, 0, 0] == float(np.float32(0.1)) * 3.0


def _q(v, bound=1.0):
    return int(np.rint(min(max(v / bound, 0.0), 1.0) * ONE))


def test_overlap_of_shifted_constant_frames_is_area_times_q():
    """Three constant 6 x 8 frames on a 6 x 12 canvas, canvas pixel x reading frame k at x - 2 k: frame k covers the columns
    2 k .. 2 k + 7.  The counts are the sampled overlap areas and the sums count x q of the row's frame, the diagonal too."""
    vals = [0.2, 0.5, 0.9]
    f = np.stack([np.full((6, 8, 2), v) for v in vals])
    f[1, :, :, 1] = 0.7                                     # luminance of frame 1: (0.5 + 0.7) / 2
    lum = [0.2, (0.5 + 0.7) / 2.0, 0.9]
    M = np.stack([_shift(-2.0 * k) for k in range(3)])[None]
    for step in (1, 2, 3, 5, 20):
        cols = [set(x for x in range(0, 12, step) if 2 * k <= x <= 2 * k + 7) for k in range(3)]
        rows = len(range(0, 6, step))
        sums, counts = overlap_reference(f, None, M, (6, 12), step, 1.0)
        for i in range(3):
            for j in range(3):
                area = rows * len(cols[i] & cols[j])
                assert counts[0, i, j] == area and sums[0, i, j] == area * _q(lum[i]), (step, i, j)
    # beyond the bound and below zero: clamped; the bound scales
    g = np.stack([np.full((2, 2, 1), v) for v in (3.0, -1.0, 1.0)])
    sums, counts = overlap_reference(g, None, np.tile(ID, (1, 3, 1, 1)), (2, 2), 1, 4.0)
    assert (counts == 4).all()
    assert sums[0, 0, 0] == 4 * _q(0.75) and sums[0, 1, 2] == 0 and sums[0, 2, 1] == 4 * _q(0.25)
    sums, _ = overlap_reference(g, None, np.tile(ID, (1, 3, 1, 1)), (2, 2), 1, 1.0)
    assert sums[0, 0, 1] == 4 * int(ONE) and sums[0, 2, 0] == 4 * int(ONE)
    # half to even at the fixed point's last place
    h = np.array([0.5 / ONE, 1.5 / ONE, 2.5 / ONE]).reshape(3, 1, 1, 1)
    sums, _ = overlap_reference(h, None, np.tile(ID, (1, 3, 1, 1)), (1, 1), 1, 1.0)
    assert [int(sums[0, i, i]) for i in range(3)] == [0, 2, 2]


def test_masks_nan_samples_dead_slots_and_nan_matrices_take_their_pairs_out():
    f = np.stack([np.full((4, 4, 1), v) for v in (0.25, 0.5, 0.75)])
    M = np.tile(ID, (1, 3, 1, 1))
    sums, counts = overlap_reference(f, None, M, (4, 4), 1, 1.0)
    assert (counts == 16).all()
    mask = np.zeros((3, 4, 4), np.uint8)
    mask[1, 0, :] = 9                                        # a row of frame 1
    sums, counts = overlap_reference(f, None, M, (4, 4), 1, 1.0, mask)
    assert counts[0].tolist() == [[16, 12, 16], [12, 12, 12], [16, 12, 16]]
    assert sums[0, 0, 1] == 12 * _q(0.25) and sums[0, 1, 0] == 12 * _q(0.5) and sums[0, 0, 2] == 16 * _q(0.25)
    g = f.copy()
    g[2, 1, 1, 0] = math.nan   # a NaN in frame 2: a NaN sample at the four pixels one of whose taps (weight 0 included) is it
    sums, counts = overlap_reference(g, None, M, (4, 4), 1, 1.0)
    assert counts[0].tolist() == [[16, 16, 12], [16, 16, 12], [12, 12, 12]]
    assert sums[0, 2, 2] == 12 * _q(0.75) and sums[0, 0, 2] == 12 * _q(0.25) and sums[0, 0, 1] == 16 * _q(0.25)
    sums, counts = overlap_reference(f, [[0, -1, 2]], M, (4, 4), 1, 1.0)   # a dead slot
    assert counts[0].tolist() == [[16, 0, 16], [0, 0, 0], [16, 0, 16]] and (sums[0, 1] == 0).all() and (sums[0, :, 1] == 0).all()
    B = M.copy()
    B[0, 0, 1, 1] = math.nan                                 # a NaN matrix
    sums, counts = overlap_reference(f, None, B, (4, 4), 1, 1.0)
    assert counts[0].tolist() == [[0, 0, 0], [0, 16, 16], [0, 16, 16]]
    # n_out outputs are kept apart
    M2 = np.concatenate([M, np.stack([ID, _shift(2.0), _shift(9.0)])[None]])
    sums, counts = overlap_reference(f, None, M2, (4, 4), 1, 1.0)
    assert counts[1].tolist() == [[16, 8, 0], [8, 8, 0], [0, 0, 0]] and (counts[0] == 16).all()


# ---- exposure_gains
def _ov(sums, counts, bound=1.0):
    return tensors.Overlap(torch.from_numpy(np.asarray(sums, np.int64)), torch.from_numpy(np.asarray(counts, np.int64)), bound)


def test_two_sources_in_closed_form():
    """N = 2 with mean luminances a, b over n shared pixels: with p = 2 / sigma_n^2 and r = 1 / sigma_g^2,
    g_0 = (p b^2 + p a b + r) / (p a^2 + p b^2 + r) and g_1 = (p a^2 + p a b + r) / (p a^2 + p b^2 + r), whatever n"""
    for a, b, n, sn, sg, bound in ((0.5, 0.25, 100, 10 / 255, 0.1, 1.0), (0.3, 0.6, 7, 0.05, 0.2, 1.0), (0.5, 0.5, 3, 0.1, 0.1, 1.0),
                                   (2.0, 1.0, 50, 0.2, 0.1, 4.0)):
        qa, qb = _q(a, bound), _q(b, bound)
        a, b = qa / ONE * bound, qb / ONE * bound
        sums = [[[n * qa + 11 * qa, n * qa], [n * qb, n * qb]]]
        counts = [[[n + 11, n], [n, n]]]                     # (the diagonal takes no part)
        g = tensors.exposure_gains(_ov(sums, counts, bound), sigma_n=sn, sigma_g=sg)
        p, r = 2.0 / sn ** 2, 1.0 / sg ** 2
        den = p * a * a + p * b * b + r
        want = [(p * b * b + p * a * b + r) / den, (p * a * a + p * a * b + r) / den]
        assert g.dtype == torch.float64 and tuple(g.shape) == (1, 2)
        assert np.abs(g.numpy()[0] - want).max() < 1e-12, (g, want)
        assert np.abs(g.numpy() - gains_reference(sums, counts, bound, sn, sg)).max() < 1e-12
    g = tensors.exposure_gains(_ov([[[5, 5], [5, 5]]], [[[9, 9], [9, 9]]]))
    assert np.abs(g.numpy() - 1).max() < 1e-12               # equal luminances: nothing to compensate


def _random_stats(rng, n_out, N):
    lum = rng.uniform(0.2, 0.8, (n_out, N))
    counts = np.zeros((n_out, N, N), np.int64)
    sums = np.zeros((n_out, N, N), np.int64)
    for o in range(n_out):
        c = rng.integers(0, 500, (N, N)) * (rng.random((N, N)) < 0.6)
        c = np.triu(c, 1)
        counts[o] = c + c.T + np.diag(rng.integers(500, 900, N))
        sums[o] = np.rint(counts[o] * (lum[o][:, None] * rng.uniform(0.95, 1.05, (N, N))) * ONE).astype(np.int64)
    return sums, counts


def test_gains_are_the_restatement_and_minimise_the_energy():
    rng = np.random.default_rng(4)
    for n_out, N in ((1, 3), (2, 9), (1, 64)):
        sums, counts = _random_stats(rng, n_out, N)
        g = tensors.exposure_gains(_ov(sums, counts)).numpy()
        assert np.abs(g - gains_reference(sums, counts)).max() < 1e-9
        if N <= 9:
            e0 = energy(g[0], sums[0], counts[0])
            for _ in range(20):
                assert energy(g[0] + rng.normal(0, 1e-3, N), sums[0], counts[0]) > e0


def test_a_source_without_overlap_has_gain_one():
    rng = np.random.default_rng(5)
    sums, counts = _random_stats(rng, 1, 5)
    for t in (sums, counts):
        t[0, 3, :3] = t[0, 3, 4:] = 0
        t[0, :3, 3] = t[0, 4:, 3] = 0
    g = tensors.exposure_gains(_ov(sums, counts)).numpy()
    assert g[0, 3] == 1.0 and np.abs(g[0] - 1).max() > 1e-3
    # nothing overlaps anything
    g = tensors.exposure_gains(_ov(np.diag([5, 6, 7])[None], np.diag([9, 9, 9])[None])).numpy()
    assert (g == 1.0).all()


def test_anchor_divides_by_the_anchors_gain_and_permuting_sources_permutes_gains():
    rng = np.random.default_rng(6)
    sums, counts = _random_stats(rng, 2, 6)
    g = tensors.exposure_gains(_ov(sums, counts)).numpy()
    for k in (0, 4):
        a = tensors.exposure_gains(_ov(sums, counts), anchor=k).numpy()
        assert (a[:, k] == 1.0).all() and np.abs(a - g / g[:, k:k + 1]).max() < 1e-14
    perm = rng.permutation(6)
    gp = tensors.exposure_gains(_ov(sums[:, perm][:, :, perm], counts[:, perm][:, :, perm])).numpy()
    assert np.abs(gp - g[:, perm]).max() < 1e-12


@pytest.mark.parametrize("kw,exc", [
    (dict(overlap=(1, 2, 3)), TypeError), (dict(overlap=None), TypeError),
    (dict(overlap=tensors.Overlap(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64), 1.0)), TypeError),
    (dict(overlap=tensors.Overlap(torch.zeros(1, 2, 2, dtype=torch.int64), None, 1.0)), TypeError),
    (dict(overlap=tensors.Overlap(torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64), 1.0)), ValueError),
    (dict(overlap=tensors.Overlap(torch.zeros(1, 2, 3, dtype=torch.int64), torch.zeros(1, 2, 3, dtype=torch.int64), 1.0)), ValueError),
    (dict(overlap=tensors.Overlap(torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 3, 3, dtype=torch.int64), 1.0)), ValueError),
    (dict(overlap=tensors.Overlap(torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64), 0.0)), ValueError),
    (dict(overlap=tensors.Overlap(torch.zeros(1, 2, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64), "1")), TypeError),
    (dict(sigma_n=0.0), ValueError), (dict(sigma_n=math.nan), ValueError), (dict(sigma_n="a"), TypeError),
    (dict(sigma_g=-1.0), ValueError), (dict(sigma_g=math.inf), ValueError), (dict(sigma_g=None), TypeError),
    (dict(anchor=2), ValueError), (dict(anchor=-1), ValueError), (dict(anchor=0.0), ValueError), (dict(anchor=True), ValueError),
    (dict(bogus=1), TypeError),
])
def test_exposure_gains_errors(kw, exc):
    ov = kw.pop("overlap", _ov(np.ones((1, 2, 2)), np.ones((1, 2, 2))))
    with pytest.raises(exc):
        tensors.exposure_gains(ov, **kw)


# ---- the scene
@pytest.fixture(scope="module")
def scenes():
    """static and with the square: frames under the gains of default_rng(3), exact matrices, the restated statistics at
    step 2 and the gains solved from them, every mode with and without the gains"""
    true = scene_gains()
    res = {}
    for square in (False, True):
        frames, Ks, A, world = exposure_scene(square, true)
        T = len(frames)
        M, size, origin = canvas_reference(A, frames.shape[1:3])
        truth = canvas_truth(world, Ks[(T - 1) // 2], origin, size)
        sums, counts = overlap_reference(frames, None, M[None], size, 2, 1.0)
        g = tensors.exposure_gains(_ov(sums, counts)).numpy()
        assert np.abs(g - gains_reference(sums, counts)).max() < 1e-9
        live = gather(frames, None, M[None], size)[1].reshape((T,) + size)
        where = live.any(0) & np.isfinite(truth).all(-1)
        out = {}
        for mode in MODES:
            for key, gg in (("plain", None), ("gains", g)):
                img = blend_reference(frames, None, M[None], size, mode, gg)[0][0]
                out[mode, key] = (scaled_psnr(img, truth, where)[0], seam_step(img, truth, live, where))
        res[square] = dict(true=true, g=g[0], out=out, pixels=int(where.sum()))
    return res


def test_gains_undo_the_exposure(scenes):
    """Measured with this restatement: the true gains spread by max / min - 1 = 0.229; g x true spreads by 0.040 on the
    static scene and 0.046 with the moving square (normalised by its mean it lies in [0.981, 1.020] and [0.977, 1.022]).
    Asserted: less than a quarter of the true gains' spread."""
    for square in (False, True):
        true, g = scenes[square]["true"], scenes[square]["g"]
        left = g * true
        spread, before = left.max() / left.min() - 1, true.max() / true.min() - 1
        print("square %s: spread %.4f of %.4f, g x true / mean in [%.3f, %.3f]" % (
            square, spread, before, (left / left.mean()).min(), (left / left.mean()).max()))
        assert spread < before / 4, (spread, before)


def test_unit_exposure_gives_unit_gains():
    """the static scene with every true gain 1: the largest |g - 1| measured is 3.0e-4"""
    frames, Ks, A, world = exposure_scene(False, np.ones(9))
    M, size, _ = canvas_reference(A, frames.shape[1:3])
    sums, counts = overlap_reference(frames, None, M[None], size, 2, 1.0)
    g = tensors.exposure_gains(_ov(sums, counts)).numpy()
    print("unit exposure: max |g - 1| = %.2e" % np.abs(g - 1).max())
    assert np.abs(g - 1).max() < 1e-3


def test_psnr_rises_with_gains_in_every_mode(scenes):
    """PSNR against the world after one least-squares global scale, over the covered canvas pixels (34572 of them).
    Measured with this restatement, without -> with gains: FIRST 26.11 -> 36.65 dB, MEAN 30.12 -> 37.10 dB, MEDIAN 28.57 ->
    36.23 dB, FEATHER 29.31 -> 36.98 dB; with the moving square FIRST 22.07 -> 23.60, MEAN 26.64 -> 28.52, MEDIAN 28.27 ->
    36.01, FEATHER 23.98 -> 25.11 dB."""
    for square in (False, True):
        out = scenes[square]["out"]
        print("square %s over %d pixels: %s" % (square, scenes[square]["pixels"], ", ".join(
            "%s %.2f -> %.2f dB" % (m.upper(), out[m, "plain"][0], out[m, "gains"][0]) for m in MODES)))
        assert scenes[square]["pixels"] > 10000
        for m in MODES:
            assert out[m, "gains"][0] > out[m, "plain"][0], (square, m)


def test_the_clean_plate_needs_the_gains(scenes):
    """with the square, the median of the compensated frames beats the plain median and every other mode with gains: under
    unequal exposure the median selects by brightness rank, and the square comes back"""
    out = scenes[True]["out"]
    assert out["median", "gains"][0] > out["median", "plain"][0] + 3
    for m in ("first", "mean", "feather"):
        assert out["median", "gains"][0] > out[m, "gains"][0] + 3, m


def test_feathering_removes_the_step_at_frame_borders(scenes):
    """The mean absolute horizontal difference of the error image between neighbours whose sets of live frames differ
    (elsewhere).  Measured on the static scene, without gains: FIRST 0.0318 (0.0051), MEAN 0.0174 (0.0062), FEATHER 0.0078
    (0.0064); with gains: FIRST 0.0092 (0.0044), MEAN 0.0078 (0.0059), FEATHER 0.0060 (0.0058)."""
    out = scenes[False]["out"]
    for key in ("plain", "gains"):
        at = {m: out[m, key][1] for m in ("first", "mean", "feather")}
        print("%s: %s" % (key, ", ".join("%s %.4f (%.4f)" % (m.upper(), at[m][0], at[m][1]) for m in at)))
        assert at["feather"][0] < at["mean"][0] < at["first"][0], (key, at)
    assert out["feather", "gains"][1][0] < 1.25 * out["feather", "gains"][1][1]   # no step left: the border is as elsewhere


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_M = lambda n_out=1, N=3: _z(n_out, N, 2, 3, dtype=torch.float64)  # noqa: E731


@pytest.mark.parametrize("kw,exc", [
    (dict(gains=[[1.0, 1.0, 1.0]]), TypeError), (dict(gains=np.ones((1, 3))), TypeError),
    (dict(gains=_z(1, 3, dtype=torch.float16)), TypeError), (dict(gains=_z(1, 3, dtype=torch.int64)), TypeError),
    (dict(gains=_z(3)), ValueError), (dict(gains=_z(1, 2)), ValueError), (dict(gains=_z(2, 3)), ValueError),
    (dict(gains=_z(1, 3, 1)), ValueError), (dict(gains=_z(1, 3, device="meta")), ValueError),
    (dict(mode="feathered"), ValueError), (dict(mode=3), ValueError),
    (dict(mode="feather", matrices=_M(1, 256), sources=torch.zeros(1, 256, dtype=torch.int32)), ValueError),
    (dict(mode="median", gains=_z(1, 65), matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),
    (dict(mode="feather", masks=_z(3, 8, 8)), TypeError), (dict(mode="feather", size=(0, 8)), ValueError),
    (dict(mode="feather", out_dtype=torch.float16), TypeError),
])
def test_mosaic_errors_of_the_new_keywords(stub, kw, exc):
    matrices, sources = kw.pop("matrices", _M()), kw.pop("sources", None)
    with pytest.raises(exc):
        tensors.mosaic(_z(3, 3, 8, 8), sources, matrices, kw.pop("size", (8, 8)), **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(step=0), ValueError), (dict(step=-2), ValueError), (dict(step=1.0), ValueError), (dict(step=True), ValueError),
    (dict(step=None), ValueError),
    (dict(bound=0.0), ValueError), (dict(bound=-1.0), ValueError), (dict(bound=math.inf), ValueError), (dict(bound=math.nan), ValueError),
    (dict(bound="1"), TypeError), (dict(bound=None), TypeError), (dict(bound=True), TypeError),
    (dict(matrices=_M(1, 65), sources=torch.zeros(1, 65, dtype=torch.int32)), ValueError),
    (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError), (dict(frames=None), TypeError), (dict(layout="HWC"), ValueError),
    (dict(size=(8,)), TypeError), (dict(size=(0, 8)), ValueError), (dict(matrices=None), TypeError),
    (dict(matrices=_z(1, 3, 3, 3)), ValueError), (dict(matrices=_M(1, 2)), ValueError),
    (dict(sources=[[0, 1, 3]]), ValueError), (dict(sources=torch.zeros(1, 3)), TypeError),
    (dict(masks=_z(3, 8, 8)), TypeError), (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError),
    (dict(mode="mean"), TypeError), (dict(out_dtype=torch.float32), TypeError),
])
def test_mosaic_overlap_errors(stub, kw, exc):
    frames, matrices = kw.pop("frames", _z(3, 3, 8, 8)), kw.pop("matrices", _M())
    sources, size = kw.pop("sources", None), kw.pop("size", (8, 8))
    with pytest.raises(exc):
        tensors.mosaic_overlap(frames, sources, matrices, size, **kw)
    assert stub == []


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    with pytest.raises(ValueError):
        tensors.mosaic(_z(3, 3, 8, 8), None, _M(), (8, 8), mode="feather")
    with pytest.raises(ValueError):
        tensors.mosaic(_z(3, 3, 8, 8), None, _M(), (8, 8), gains=_z(1, 3))
    with pytest.raises(ValueError):
        tensors.mosaic_overlap(_z(3, 3, 8, 8), None, _M(), (8, 8))
    with pytest.raises(ValueError):
        tensors.panorama(_z(3, 3, 8, 8), 2, mode="feather", exposure=True)
    assert calls == []


def test_which_c_symbol_is_reached(stub, monkeypatch):
    """without gains the three old modes go through papof_mosaic_tensor as before; gains or "feather" through
    papof_mosaic_blend_tensor; 255 sources for "feather" and 64 for the statistics pass every check"""
    reached = []

    def launch(dev, name, *args, **kw):
        reached.append((name, args[7]))
        reached.append(args[12] if name == "papof_mosaic_blend_tensor" else "-")

    monkeypatch.setattr(tensors, "_launch", launch)
    f = _z(3, 3, 8, 8)
    for mode in ("first", "mean", "median"):
        tensors.mosaic(f, None, _M(), (4, 4), mode=mode)
        tensors.mosaic(f, None, _M(), (4, 4), mode=mode, gains=None)
    assert reached == [("papof_mosaic_tensor", 3), "-"] * 6
    del reached[:]
    out, cnt = tensors.mosaic(f, torch.zeros(1, 255, dtype=torch.int64), _M(1, 255), (4, 5), mode="feather", layout="NHWC",
                              out_dtype=torch.uint8)
    assert reached == [("papof_mosaic_blend_tensor", 255), None]          # gains NULL
    assert tuple(out.shape) == (1, 4, 5, 8) and out.dtype == torch.uint8 and tuple(cnt.shape) == (1, 4, 5)
    del reached[:]
    for mode in MODES:
        tensors.mosaic(f, None, _M(2, 3), (4, 4), mode=mode, gains=torch.ones(2, 1).expand(2, 3))
    assert [r for r in reached if isinstance(r, tuple)] == [("papof_mosaic_blend_tensor", 3)] * 4
    assert all(r is not None for r in reached)
    del reached[:]
    ov = tensors.mosaic_overlap(f, np.zeros((2, 64), np.int16) - 5, _M(2, 64), (4, 4), step=7, bound=2)
    assert reached == [("papof_mosaic_overlap_tensor", 64), "-"]
    assert isinstance(ov, tensors.Overlap) and ov.bound == 2.0 and ov.sums.dtype == ov.counts.dtype == torch.int64
    assert tuple(ov.sums.shape) == tuple(ov.counts.shape) == (2, 64, 64)


@pytest.mark.parametrize("kw,exc", [
    (dict(exposure=1), TypeError), (dict(exposure="yes"), TypeError), (dict(exposure=None), TypeError),
    (dict(mode="feathered"), ValueError), (dict(mode="feather", step=0), ValueError),
    (dict(mode="feather", exposure=True, ref=3), ValueError), (dict(mode="feather", exposure=True, bogus=1), TypeError),
])
def test_panorama_errors_of_the_new_keywords(stub, kw, exc):
    with pytest.raises(exc):
        tensors.panorama(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


def test_panorama_with_exposure_names_step_beyond_64_frames(stub):
    for mode in ("feather", "mean", "first", "median"):
        with pytest.raises(ValueError, match="a larger step"):
            tensors.panorama(_z(65, 1, 8, 8).expand(65, 3, 8, 8), 2, mode=mode, exposure=True)
    with pytest.raises(ValueError, match="a larger step"):
        tensors.panorama(_z(130, 1, 8, 8).expand(130, 3, 8, 8), 2, mode="feather", step=2, exposure=True)
    with pytest.raises(ValueError, match="step"):
        tensors.panorama(_z(256, 1, 8, 8).expand(256, 3, 8, 8), 2, mode="feather")
    assert stub == []


def test_panorama_keeps_its_fields_and_gains_default_to_none():
    assert tensors.Panorama._fields == ("image", "count", "matrices", "origin", "motion", "ok", "flow", "timing", "gains")
    assert tensors.Panorama(1, 2, 3, 4, 5, 6, 7, 8).gains is None


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
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
_make = {"fr": lambda: _t(capi.DTYPE_U8), "mat": lambda: _t(capi.DTYPE_F32, (18, 6, 3, 1)), "out": lambda: _t(capi.DTYPE_F64)}


def _blend(lib, h, n_frames=3, size=(8, 8, 3), fr=_OK, masks=None, n_out=2, n_src=3, canvas=(5, 9), sources=0x3000, mat=_OK,
           gains=None, mode=capi.MOSAIC_FEATHER, out=_OK, count=None):
    d = {k: _make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mat=mat, out=out).items()}
    return lib.papof_mosaic_blend_tensor(h, n_frames, size[0], size[1], size[2], _ref(d["fr"]), _ref(masks), n_out, n_src,
                                         canvas[0], canvas[1], sources, _ref(d["mat"]), _ref(gains), mode, _ref(d["out"]),
                                         _ref(count), None)


def _overlap(lib, h, n_frames=3, size=(8, 8, 3), fr=_OK, masks=None, n_out=2, n_src=3, canvas=(5, 9), sources=0x3000, mat=_OK,
             step=2, bound=1.0, sums=0x4000, counts=0x5000):
    d = {k: _make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mat=mat).items()}
    return lib.papof_mosaic_overlap_tensor(h, n_frames, size[0], size[1], size[2], _ref(d["fr"]), _ref(masks), n_out, n_src,
                                           canvas[0], canvas[1], sources, _ref(d["mat"]), step, bound, sums, counts, None)


_COMMON = [
    dict(fr=None), dict(mat=None), dict(sources=None),                                                    # NULL
    dict(fr=_t(data=0)), dict(mat=_t(data=0)), dict(masks=_t(capi.DTYPE_U8, data=0)),
    dict(fr=_t(dtype=3)), dict(mat=_t(capi.DTYPE_U8, (18, 6, 3, 1))), dict(masks=_t(capi.DTYPE_F32, (64, 8, 1, 0))),  # dtypes
    dict(fr=_t(strides=(192, 24, 3, -1))), dict(fr=_t(strides=(-192, 24, 3, 1))),                       # strides
    dict(mat=_t(strides=(18, -6, 3, 1))), dict(mat=_t(strides=(18, 6, 3, -1))), dict(masks=_t(capi.DTYPE_U8, (64, -8, 1, 0))),
    dict(n_src=0), dict(n_src=-1), dict(n_src=256),                                                      # slots
    dict(n_frames=0), dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)), dict(n_out=0),   # sizes
    dict(canvas=(0, 9)), dict(canvas=(5, 0)), dict(canvas=(-5, 9)),
]


@pytest.mark.parametrize("kw", _COMMON + [
    dict(out=None), dict(out=_t(data=0)), dict(out=_t(dtype=-1)), dict(count=_t(capi.DTYPE_U8, data=0)),
    dict(count=_t(capi.DTYPE_F64, (64, 8, 1, 0))),
    dict(out=_t(strides=(192, 24, 3, 0))), dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(192, 24, -3, 1))),
    dict(count=_t(capi.DTYPE_U8, (64, 8, 0, 0))), dict(count=_t(capi.DTYPE_U8, (0, 8, 1, 0))),
    dict(n_src=256, mode=capi.MOSAIC_MEAN), dict(n_src=65, mode=capi.MOSAIC_MEDIAN), dict(n_src=255, mode=capi.MOSAIC_MEDIAN),
    dict(mode=4), dict(mode=-1),
    dict(gains=_t(capi.DTYPE_U8, (3, 1, 0, 0))), dict(gains=_t(dtype=7, strides=(3, 1, 0, 0))),           # the gains
    dict(gains=_t(capi.DTYPE_F32, (3, 1, 0, 0), data=0)),
    dict(gains=_t(capi.DTYPE_F64, (-3, 1, 0, 0))), dict(gains=_t(capi.DTYPE_F32, (3, -1, 0, 0))),
])
def test_blend_c_abi_refuses(kw):
    assert _blend(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


@pytest.mark.parametrize("kw", _COMMON + [
    dict(n_src=65), dict(n_src=255),
    dict(step=0), dict(step=-1),
    dict(bound=0.0), dict(bound=-1.0), dict(bound=math.inf), dict(bound=-math.inf), dict(bound=math.nan),
    dict(sums=None), dict(counts=None),
])
def test_overlap_c_abi_refuses(kw):
    assert _overlap(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_without_a_handle_and_the_symbols_are_bound():
    lib = _lib()
    assert _blend(lib, None) == -1 and _overlap(lib, None) == -1
    for name in ("papof_mosaic_blend_tensor", "papof_mosaic_overlap_tensor"):
        assert name in capi.SYMBOLS and getattr(lib, name).restype is ctypes.c_int and len(getattr(lib, name).argtypes) == 18


def test_the_constants_are_the_headers():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "papof.h")).read()
    for name, value in (("FEATHER", capi.MOSAIC_FEATHER), ("MAX_OVERLAP", capi.MOSAIC_MAX_OVERLAP)):
        assert int(re.search(r"PAPOF_MOSAIC_%s = (\d+)" % name, header).group(1)) == value
    assert tensors.MAX_OVERLAP == 64 and tensors.OVERLAP_ONE == int(ONE) and tensors.MOSAIC_MODES["feather"] == 3
