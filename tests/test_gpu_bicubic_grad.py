"""The bicubic warp that takes frame 2's derivatives from frame 2 itself (csrc/kernels.hip: k_bicubic_grad, and k_bicubic_grad3
for three channels) returns the oracle's bytes, clamped (the final warp of a call) and unclamped.

Sizes 1 x 7, 7 x 1, 2 x 2, 5 x 6 and 33 x 47 (more than one block each way, no multiple of the 64 x 4 tile) with one and three
channels.  Flows: zero; a constant 0.5; flows that land exactly on column W - 1, on row H - 1 and on column / row 0 -- where
the corners x1 == x0 or y1 == y0 coincide and the lower corner's upper neighbour is not the upper corner; one pixel outside on
each of the four sides (frame 1's value); a seeded random +-3 px.  Frame values reach beyond [0, 1] so that the clamp acts.
The final warp of a host call into page-locked result arrays runs in four row chunks: its warpI2 must be the one launch's.
`.tobytes()` equality: the sign of a zero counts.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(1, 7), (7, 1), (2, 2), (5, 6), (33, 47)]  # H, W


@pytest.fixture(scope="module")
def gpu():
    from papteam_opticalflow_amd import Papof
    g = Papof(0)
    yield g
    g.close()


def _frames(h, w, c):
    rng = np.random.default_rng(100 * h + w + 7 * c)
    return rng.random((h, w, c)) * 1.5 - 0.25, rng.random((h, w, c)) * 1.5 - 0.25


def _flows(h, w):
    """{name: (vx, vy)}; x = column + vx, y = row + vy"""
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = np.zeros((h, w))
    rng = np.random.default_rng(h * 1000 + w)
    return {
        "zero": (z, z),
        "half": (z + 0.5, z + 0.5),
        "onto the last column": (w - 1 - jj, z),
        "onto the last row": (z, h - 1 - ii),
        "onto column 0 and row 0": (-jj, -ii),
        "one pixel left of the image": (-jj - 1, z),
        "one pixel right of the image": (w - jj, z),
        "one pixel above the image": (z, -ii - 1),
        "one pixel below the image": (z, h - ii),
        "random": (rng.uniform(-3, 3, (h, w)), rng.uniform(-3, 3, (h, w))),
    }


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_clamped_and_unclamped_against_the_oracle(gpu, oracle, size, c):
    h, w = size
    im1, im2 = _frames(h, w, c)
    for name, (vx, vy) in _flows(h, w).items():
        want = oracle.bicubic_warp(im1, im2, vx, vy)
        got = gpu.bicubic_warp(im1, im2, vx, vy)
        assert got.tobytes() == want.tobytes(), "clamped, flow %s: differs from the oracle" % name
        want = oracle.bicubic_warp_noclamp(im1, im2, vx, vy)
        got = gpu.bicubic_warp_noclamp(im1, im2, vx, vy)
        assert got.tobytes() == want.tobytes(), "unclamped, flow %s: differs from the oracle" % name
        if name.startswith("one pixel"):
            assert want.tobytes() == im1.tobytes()  # every position left the image


def test_final_warp_in_row_chunks_equals_the_one_launch(gpu, oracle):
    from papteam_opticalflow_amd import capi
    h, w, c, levels = 33, 47, 3, 2
    rng = np.random.default_rng(33 * 47)
    a = rng.random((h, w, c))
    b = np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))
    want = oracle.coarse2fine_flow(a, b, levels)[:3]
    # one launch: the device-resident call
    n = h * w
    d = [gpu.dev_alloc(a.nbytes), gpu.dev_alloc(b.nbytes), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n * c)]
    try:
        gpu.dev_upload(d[0], a)
        gpu.dev_upload(d[1], b)
        gpu.flow_device(d[0], d[1], h, w, c, levels, None, d[2], d[3], d[4])
        one = np.zeros((h, w, c))
        gpu.dev_download(one, d[4])
    finally:
        for p in d:
            gpu.dev_free(p)
    # four row chunks: the host call into page-locked result arrays
    shapes = ((h, w), (h, w), (h, w, c))
    addrs = [capi._pinned_alloc(8 * int(np.prod(s))) for s in shapes]
    assert all(addrs)
    try:
        out = tuple(np.frombuffer((ctypes.c_char * (8 * int(np.prod(s)))).from_address(p), dtype=np.float64).reshape(s)
                    for s, p in zip(shapes, addrs))
        for x in out:
            x[...] = np.nan
        D = ctypes.POINTER(ctypes.c_double)
        t = np.zeros(10)
        rc = gpu.L.papof_flow(gpu.h, a.ctypes.data_as(D), b.ctypes.data_as(D), h, w, c, levels, None,
                              out[0].ctypes.data_as(D), out[1].ctypes.data_as(D), out[2].ctypes.data_as(D), t.ctypes.data_as(D))
        assert rc == 0
        chunks = out[2].copy()
        vx, vy = out[0].copy(), out[1].copy()
        del out, x
    finally:
        for p in addrs:
            capi._pinned_free(p)
    assert chunks.tobytes() == one.tobytes(), "warpI2 in row chunks differs from the one launch"
    assert one.tobytes() == want[2].tobytes() and vx.tobytes() == want[0].tobytes() and vy.tobytes() == want[1].tobytes()
