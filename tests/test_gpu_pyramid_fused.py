"""The pyramid, whose levels of Gaussian half-width 1 .. 4 are one launch each (csrc/kernels.hip: k_smooth_resize), returns the
oracle's bytes.

Frames from 1 x 9 to 135 x 240 at the ratios 0.5, 0.75 and 0.9, at EVERY level count from 2 up to the deepest pyramid whose
levels all keep a pixel: the half-widths 1, 2, 3 and 4 (ratio 0.9 reaches all of them; its coarsest source levels are the
widest footprints, a rate of 0.254), the single-tap level that is a resize alone, the half-width 6 of ratio 0.5 (two kernels
through the temporaries) and the levels beyond "derived from level 0", which are built from finer levels of the same pyramid.
Level i of a pyramid does not depend on the level count, so the oracle runs once per frame and ratio, at the deepest count.
A frame with a side of one pixel has no second level: the product refuses the count (its rule since the first commit).
`.tobytes()` equality: the sign of a zero counts.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = [(1, 9, 1), (9, 1, 3), (2, 2, 3), (3, 4, 1), (17, 33, 3), (64, 80, 3), (135, 240, 3)]  # H, W, C
RATIOS = [0.5, 0.75, 0.9]


def _frame(h, w, c):
    return np.random.default_rng(1000 * h + 10 * w + c).random((h, w, c))


def _deepest(oracle, im, ratio):
    """the oracle's pyramid at the largest level count whose levels all have a pixel (the oracle itself sizes them)"""
    h, w, c = im.shape
    n = 1
    while True:
        dims = np.zeros(2 * (n + 1), dtype=np.int32)
        oracle.L.orc_pyramid(im.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), h, w, c, ratio, n + 1,
                             dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None)
        if dims.min() < 1:
            break
        n += 1
    return oracle.pyramid(im, ratio, n)


@pytest.fixture(scope="module")
def gpu():
    from papteam_opticalflow_amd import Papof
    g = Papof(0)
    yield g
    g.close()


def _same(got, want, what):
    assert len(got) <= len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: level %d differs from the oracle" % (what, i)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%dx%d" % f)
def test_every_level_count(gpu, oracle, frame, ratio):
    from papteam_opticalflow_amd.capi import PapofError
    im = _frame(*frame)
    want = _deepest(oracle, im, ratio)
    print("%s ratio %.2f: %d levels, coarsest %s" % (frame, ratio, len(want), want[-1].shape))
    if min(frame[:2]) == 1:
        assert len(want) == 1
        _same(gpu.pyramid(im, ratio, 1), want, "one level")
    else:
        assert len(want) >= 2
        for levels in range(2, len(want) + 1):
            _same(gpu.pyramid(im, ratio, levels), want, "%d levels" % levels)
    with pytest.raises(PapofError):  # one level more: a level without a pixel
        gpu.pyramid(im, ratio, len(want) + 1)


def test_half_widths_of_the_three_ratios():
    """what the cases above reach, from the rule of src/GaussianPyramid.cpp:89-106 (fsize = (int)(sigma * 3))"""
    def halves(ratio, levels):
        base, n = 1 / ratio - 1, int(np.log(0.25) / np.log(ratio))
        return {int(base * min(i, n) * 3) for i in range(1, levels)}
    assert halves(0.9, 20) == {0, 1, 2, 3, 4}
    assert halves(0.75, 8) >= {2, 3} and max(halves(0.75, 8)) <= 4
    assert halves(0.5, 4) == {3, 6}  # 6: beyond the fused kernel's half-widths


def test_min_width_pyramid(gpu, oracle):
    im = _frame(135, 240, 3)
    want = oracle.pyramid_minwidth(im, 0.75, 20)  # log(20 / 240) / log(.75) = 8.6 -> 8 levels, three of them chained
    assert len(want) == 8
    _same(gpu.pyramid_minwidth(im, 0.75, 20), want, "min_width 20")
    assert len(gpu.pyramid_minwidth(im, 0.75, 20)) == 8


def test_half_width_beyond_the_fused_kernel_takes_two_kernels(gpu, oracle):
    im = _frame(64, 80, 3)
    want = oracle.pyramid(im, 0.5, 4)  # half-widths 3, 6, 6: level 1 fused, levels 2 and 3 through the temporaries
    _same(gpu.pyramid(im, 0.5, 4), want, "ratio 0.5, 4 levels")
    assert len(want) == 4


def test_five_level_flow_on_device_frames(gpu, oracle):
    h, w, c, levels = 135, 240, 3, 5
    rng = np.random.default_rng(135 * 240)
    a = rng.random((h, w, c))
    b = np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))
    want = oracle.coarse2fine_flow(a, b, levels)[:3]
    n = h * w
    d = [gpu.dev_alloc(a.nbytes), gpu.dev_alloc(b.nbytes), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n * c)]
    try:
        gpu.dev_upload(d[0], a)
        gpu.dev_upload(d[1], b)
        gpu.flow_device(d[0], d[1], h, w, c, levels, None, d[2], d[3], d[4])
        got = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, c))
        for arr, p in zip(got, d[2:]):
            gpu.dev_download(arr, p)
    finally:
        for p in d:
            gpu.dev_free(p)
    for name, g, x in zip(("vx", "vy", "warpI2"), got, want):
        assert g.tobytes() == x.tobytes(), "papof_flow_device, 5 levels: %s differs from the oracle" % name
