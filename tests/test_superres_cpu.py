"""Multi-frame super-resolution, checked on the CPU: known answers of the numpy restatement (tests/_superres_ref.py) that the
device's bytes are compared with in tests/test_gpu_superres.py, computed here by hand-written loops; its quality on the
committed 480x270 frame with exact and with estimated flows, and its known weak case, the static video; every argument
error of tensors.super_resolve / super_resolve_video raised before a launch (CPU tensors, a stubbed handle), and the C ABI's
own refusals through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

import cases
from _superres_ref import FIX, accumulate, backproject, cubic_base, cubic_weights, resolve, superres_reference

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402

EINVAL = -1  # PAPOF_EINVAL
QUARTER = 1 << 30  # a tap of weight 0.25 in the fixed point


def _frames(T, H, W, C, seed):
    return np.random.default_rng(seed).random((T, H, W, C))


def _flows(T, H, W, dx=0.0, dy=0.0):
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0], fw[:, 1] = dx, dy
    return fw, -fw


def _q(w, v):
    """one term of num: the tap weight w times the value v, quantised"""
    return int(np.rint((w * v) * FIX))


# ---- known answers of the accumulation ----

@pytest.mark.parametrize("S", [2, 3, 4])
def test_zero_flows_split_every_pixel_over_the_fine_pixels_around_its_centre(S):
    """q = S (p + 0.5) - 0.5: for even S the centre of a source pixel lies between four fine pixels and splits evenly over
    them, for S = 3 it is the centre of one fine pixel; with zero flows every frame within the radius lands there too"""
    T, H, W, C, R = 4, 5, 7, 2, 1
    F = _frames(1, H, W, C, 1).repeat(T, 0)
    num, den = accumulate(F, *_flows(T, H, W), S, R)
    for t in range(T):
        n = 1 + min(R, t) + min(R, T - 1 - t)  # the frame itself and the chains that reach it
        want_den, want_num = np.zeros((S * H, S * W), np.int64), np.zeros((S * H, S * W, C), np.int64)
        for j in range(H):
            for i in range(W):
                if S == 3:
                    taps = [(3 * j + 1, 3 * i + 1, 1.0)]
                else:
                    y, x = S * j + S // 2 - 1, S * i + S // 2 - 1
                    taps = [(y, x, 0.25), (y, x + 1, 0.25), (y + 1, x, 0.25), (y + 1, x + 1, 0.25)]
                for y, x, w in taps:
                    want_den[y, x] += n * int(w * FIX)
                    for c in range(C):
                        want_num[y, x, c] += n * _q(w, F[t, j, i, c])
        assert np.array_equal(den[t], want_den) and np.array_equal(num[t], want_num)


def test_integer_translations_put_all_frames_on_one_lattice():
    """flows of whole low-resolution pixels: every frame lands on the half-phase lattice of the target, and num / den there
    is the mean of the aligned samples of the frames whose pixel lies inside the image"""
    T, H, W, C, R, S, dx, dy = 4, 6, 8, 1, 2, 2, 2, -1
    F = _frames(T, H, W, C, 2)
    num, den = accumulate(F, *_flows(T, H, W, dx, dy), S, R)
    for t in range(T):
        for j in range(H):
            for i in range(W):
                vals = []
                for k in range(max(0, t - R), min(T, t + R + 1)):
                    sj, si = j - (t - k) * dy, i - (t - k) * dx  # the pixel of frame k that lands on (i, j) of frame t
                    # every hop of its chain must stay inside the image
                    steps = range(0, t - k + 1) if k <= t else range(t - k, 1)
                    if all(0 <= sj + s * dy < H and 0 <= si + s * dx < W for s in steps):
                        vals.append(F[k, sj, si, 0])
                for y, x in ((2 * j, 2 * i), (2 * j + 1, 2 * i), (2 * j, 2 * i + 1), (2 * j + 1, 2 * i + 1)):
                    assert den[t, y, x] == len(vals) * QUARTER
                    assert num[t, y, x, 0] == sum(_q(0.25, v) for v in vals)
                mean = num[t, 2 * j, 2 * i, 0] / den[t, 2 * j, 2 * i]
                assert abs(mean - np.mean(vals)) <= 2.0 ** -30


@pytest.mark.parametrize("dx,dy", [(0.25, 0.25), (-0.25, 0.75), (0.75, -0.25), (-0.75, -0.75)])
def test_quarter_pixel_flows_put_the_whole_weight_on_one_fine_pixel(dx, dy):
    """scale 2: P = (i + dx, j + dy) with dx, dy in {+-0.25, +-0.75} gives Q = 2 (P + 0.5) - 0.5, a pixel centre"""
    T, H, W, S = 2, 5, 6, 2
    F = _frames(T, H, W, 1, 3)
    fw, bw = _flows(T, H, W, dx, dy)
    num, den = accumulate(F, fw, bw, S, 1)
    want_den = np.zeros((S * H, S * W), np.int64)
    want_num = np.zeros((S * H, S * W), np.int64)
    for j in range(H):
        for i in range(W):
            for y, x in ((2 * j, 2 * i), (2 * j + 1, 2 * i), (2 * j, 2 * i + 1), (2 * j + 1, 2 * i + 1)):  # frame 1 itself
                want_den[y, x] += QUARTER
                want_num[y, x] += _q(0.25, F[1, j, i, 0])
            PX, PY = i + dx, j + dy  # frame 0's pixel in frame 1
            if 0 <= PX <= W - 1 and 0 <= PY <= H - 1:
                x, y = int(2 * (PX + 0.5) - 0.5), int(2 * (PY + 0.5) - 0.5)
                assert (x, y) == (2 * (PX + 0.5) - 0.5, 2 * (PY + 0.5) - 0.5)
                want_den[y, x] += 1 << 32
                want_num[y, x] += _q(1.0, F[0, j, i, 0])
    assert np.array_equal(den[1], want_den) and np.array_equal(num[1, ..., 0], want_num)


def test_a_chain_that_leaves_the_image_or_fails_the_check_deposits_nothing_from_there_on():
    T, H, W, S, R = 3, 6, 9, 2, 2
    F = _frames(T, H, W, 1, 4)
    fw, bw = np.zeros((T - 1, 2, H, W)), np.zeros((T - 1, 2, H, W))
    fw[0, 0], bw[0, 0] = 1.0, -1.0       # pair 0: one pixel to the right and back; pair 1: nothing moves
    bw[0, 0, 2:4, 3:6] = 50.0            # ... but not back from these pixels of frame 1
    total = lambda den, t: int(den[t].sum())  # noqa: E731  (whole-pixel flows: every deposit is four taps of 2^30)
    # frames 0 -> 1 -> 2: the last column leaves the image at the first hop and is dead at the second as well
    for consistency, dead in ((None, 0), ((0.01, 0.5), 2 * 3)):
        num, den = accumulate(F, fw, bw, S, R, None, consistency)
        alive01 = H * (W - 1) - dead          # sources of frame 0 that reach frame 1: those pixels of frame 1 fail the check
        assert total(den, 1) == (H * W + alive01 + H * W) << 32           # itself, frame 0's chains, frame 2's chains
        assert total(den, 2) == (H * W + H * W + alive01) << 32           # itself, frame 1's chains, frame 0's second hop
        # backward: frame 1's pixels move one to the left; column 0 leaves, and so do the block's pixels, check or none
        back10 = H * (W - 1) - 2 * 3
        assert total(den, 0) == (H * W + back10 + back10) << 32           # itself, frame 1's chains, frame 2's second hop
    # a NaN flow kills its chain, the others are untouched
    fw[0, 0, 0, 0] = np.nan
    num, den = accumulate(F, fw, bw, S, R)
    assert total(den, 1) == (H * W + H * (W - 1) - 1 + H * W) << 32


def test_the_photometric_weight_lowers_a_sample_that_looks_different():
    T, H, W, S = 2, 4, 4, 2
    F = np.full((T, H, W, 1), 0.5)
    F[1] = 0.8
    num, den = accumulate(F, *_flows(T, H, W), S, 1, sigma=0.1)
    w = 1.0 / (1.0 + ((0.5 - 0.8) * (0.5 - 0.8) / 1) / (0.1 * 0.1))
    assert den[1, 0, 0] == QUARTER + int(np.rint((w * 0.25) * FIX))
    assert num[1, 0, 0, 0] == _q(0.25, 0.8) + int(np.rint(((w * 0.25) * 0.5) * FIX))


# ---- the cubic base, the prior, the back-projection, the stores ----

def test_cubic_base_by_hand_and_on_polynomials():
    H, W, S = 7, 9, 3
    Y = _frames(1, H, W, 1, 5)[0]
    base = cubic_base(Y, S)
    for y, x in ((0, 0), (4, 7), (10, 13), (S * H - 1, S * W - 1), (8, 26)):
        py, px = (y + 0.5) / S - 0.5, (x + 0.5) / S - 0.5
        y0, x0 = math.floor(py), math.floor(px)
        wy, wx = cubic_weights(py - y0), cubic_weights(px - x0)
        b = 0.0
        for m in range(4):
            row = 0.0
            for n in range(4):
                row += wx[n] * Y[min(max(y0 - 1 + m, 0), H - 1), min(max(x0 - 1 + n, 0), W - 1), 0]
            b += wy[m] * row
        assert base[y, x, 0] == b
    assert np.abs(cubic_base(np.full((H, W, 1), 0.375), S) - 0.375).max() <= 1e-15  # the weights sum to 1
    ramp = (np.arange(W, dtype=np.float64)[None, :, None] * 0.0625).repeat(H, 0)
    want = ((np.arange(S * W) + 0.5) / S - 0.5) * 0.0625
    assert np.abs(cubic_base(ramp, S)[:, 2 * S:-2 * S, 0] - want[None, 2 * S:-2 * S]).max() <= 1e-15  # exact on a line


def test_where_nothing_lands_the_prior_alone_answers_with_the_cubic_base():
    """scale 3, one frame: only the centre fine pixel of every source pixel is reached; the other eight are the prior's"""
    H, W, S, prior = 5, 6, 3, 0.05
    F = _frames(1, H, W, 2, 6)
    video, cov = superres_reference(F, np.zeros((0, 2, H, W)), np.zeros((0, 2, H, W)), S, prior=prior, iters=0)
    base = cubic_base(F[0], S)
    centre = np.zeros((S * H, S * W), bool)
    centre[1::3, 1::3] = True
    assert np.all(cov[0][centre] == 1.0) and np.all(cov[0][~centre] == 0.0)
    assert np.array_equal(video[0][~centre], ((prior * base) / prior)[~centre])
    assert np.abs(video[0][~centre] - base[~centre]).max() <= 1e-15
    rows, cols = np.nonzero(centre)
    want = (np.rint(F[0][rows // 3, cols // 3] * FIX) * (1.0 / FIX) + prior * base[centre]) / (1.0 + prior)
    assert np.array_equal(video[0][centre], want)


@pytest.mark.parametrize("S", [2, 3, 4])
def test_back_projection_fixed_point_and_one_step(S):
    H, W = 5, 7
    rng = np.random.default_rng(7)
    Y = rng.integers(0, 9, (H, W, 2)) / 8.0
    X = Y.repeat(S, 0).repeat(S, 1)
    pattern = np.zeros((S, S))
    pattern[0, 0], pattern[-1, -1] = 0.125, -0.125  # zero mean over the block, dyadic: every sum is exact
    X = X + np.tile(pattern, (H, W))[..., None]
    assert np.array_equal(backproject(X, Y, S), X)  # block means equal Y: nothing changes
    # from zero, a constant frame is reached in one step (r = the constant everywhere, dyadic weights at S = 2 and 4)
    Z = backproject(np.zeros((S * H, S * W, 1)), np.full((H, W, 1), 0.5), S)
    assert np.abs(Z - 0.5).max() <= (0 if S != 3 else 4e-16)  # (thirds are not dyadic: two roundings of 0.5)
    # one step by hand at a pixel in the interior
    X = rng.random((S * H, S * W, 1))
    r = np.empty((H, W))
    for j in range(H):
        for i in range(W):
            s = 0.0
            for m in range(S):
                for n in range(S):
                    s += X[S * j + m, S * i + n, 0]
            r[j, i] = Y[j, i, 0] - s / (S * S)
    for y, x in ((0, 0), (S * 2 + 1, S * 3), (S * H - 1, S * W - 1), (S, S * W - 2)):
        py, px = (y + 0.5) / S - 0.5, (x + 0.5) / S - 0.5
        y0, x0 = math.floor(py), math.floor(px)
        ty, tx = py - y0, px - x0
        cl = lambda v, n: min(max(v, 0), n - 1)  # noqa: E731
        top = (1.0 - tx) * r[cl(y0, H), cl(x0, W)] + tx * r[cl(y0, H), cl(x0 + 1, W)]
        bot = (1.0 - tx) * r[cl(y0 + 1, H), cl(x0, W)] + tx * r[cl(y0 + 1, H), cl(x0 + 1, W)]
        assert backproject(X, Y[..., :1], S)[y, x, 0] == X[y, x, 0] + ((1.0 - ty) * top + ty * bot)


def test_uint8_in_and_out():
    T, H, W, S = 3, 6, 8, 2
    u8 = np.random.default_rng(8).integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    fw, bw = _flows(T, H, W, 0.5, 0.0)
    video, cov = superres_reference(u8, fw, bw, S)
    assert video.dtype == np.uint8 and video.shape == (T, S * H, S * W, 3) and cov.dtype == np.float64
    f64, cov64 = superres_reference(u8.astype(np.float64) / 255.0, fw, bw, S)
    assert np.array_equal(cov, cov64)
    assert np.array_equal(video, np.clip(np.rint(255.0 * f64), 0, 255).astype(np.uint8))
    f32, _ = superres_reference(u8, fw, bw, S, out_dtype=np.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32))


# ---- quality on the committed frame ----

def _shift(img, dx, dy):
    """img (H, W, C) moved by (dx, dy) pixels -- what is at x lands at x + d -- by cubic convolution, edges clamped"""
    out = img
    for axis, d in ((1, dx), (0, dy)):
        n = img.shape[axis]
        p = np.arange(n) - d
        p0 = np.floor(p)
        w = cubic_weights(p - p0)
        acc = 0.0
        for k in range(4):
            wk = w[k][None, :, None] if axis == 1 else w[k][:, None, None]
            acc = acc + wk * np.take(out, np.clip(p0.astype(int) - 1 + k, 0, n - 1), axis=axis)
        out = acc
    return out


def _box(x, S):
    h, w, c = x.shape
    return x.reshape(h // S, S, w // S, S, c).mean((1, 3))


def _psnr(a, b, m=8):
    return 10.0 * math.log10(1.0 / np.mean((a[m:-m, m:-m] - b[m:-m, m:-m]) ** 2))


def _up(a, S, mode):
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))[None]
    return torch.nn.functional.interpolate(t, scale_factor=S, mode=mode, align_corners=False)[0].numpy().transpose(1, 2, 0)


def _image(colour):
    rgb = cases.load_frame_u8("480", 1).astype(np.float64) / 255.0
    return rgb if colour else rgb.mean(-1, keepdims=True)


def _video(img, pan, S, T=5):
    """the protocol: frame k shows the committed frame moved by k * pan * S fine pixels, cropped by 8 and decimated by the
    S x S box -> (the full-resolution frames, the low-resolution video, its exact flows)"""
    H0, W0, _ = img.shape
    crop = (slice(8, H0 - 8 - (H0 - 16) % (2 * S)), slice(8, W0 - 8 - (W0 - 16) % (2 * S)))
    hr = [_shift(img, k * pan[0] * S, k * pan[1] * S)[crop] for k in range(T)]
    lr = np.stack([_box(h, S) for h in hr])
    fw, bw = _flows(T, lr.shape[1], lr.shape[2], pan[0], pan[1])
    return hr, lr, fw, bw


PANS = [(0.5, 0.25), (0.3, 0.2), (1.37, -0.61)]  # low-resolution pixels per frame


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("S,pan,floor", [(2, PANS[0], 1.0), (2, PANS[1], 1.0), (2, PANS[2], 1.0), (3, PANS[0], 0.7)])
def test_quality_exact_flows(S, pan, floor, colour):
    """Five frames, exact flows, the defaults, PSNR of the centre frame against the full-resolution frame (border of 8 fine
    pixels left out) over bicubic upsampling of the centre frame.  Measured (grey / colour, iters 0 -> 2):
        scale 2, pan (0.5, 0.25):    +1.27 -> +2.09 / +1.27 -> +2.10 dB   (bicubic 23.89 / 23.85 dB)
        scale 2, pan (0.3, 0.2):     +1.58 -> +2.74 / +1.59 -> +2.75 dB   (24.93 / 24.88)
        scale 2, pan (1.37, -0.61):  +2.22 -> +4.09 / +2.21 -> +4.10 dB   (26.99 / 26.94)
        scale 3, pan (0.5, 0.25):    +1.26 -> +1.82 / +1.25 -> +1.83 dB   (22.48 / 22.41; 1.2 % of the fine pixels unreached)
    Asserted: at least 1.0 dB (scale 2) and 0.7 dB (scale 3) without back-projection, and two steps do not lower it."""
    hr, lr, fw, bw = _video(_image(colour), pan, S)
    c = len(hr) // 2
    bicubic = _psnr(_up(lr[c], S, "bicubic"), hr[c])
    g0 = _psnr(superres_reference(lr, fw, bw, S, iters=0)[0][c], hr[c]) - bicubic
    g2 = _psnr(superres_reference(lr, fw, bw, S, iters=2)[0][c], hr[c]) - bicubic
    print("scale %d pan %s colour %s: bicubic %.2f dB, gain %+.2f dB, with two steps %+.2f dB" % (S, pan, colour, bicubic, g0, g2))
    assert g0 >= floor
    assert g2 >= g0


def _oracle_flows(lr, levels=4):
    from _libs import OracleLib
    L = OracleLib()
    T = lr.shape[0]
    fw, bw = np.empty((T - 1, 2) + lr.shape[1:3]), np.empty((T - 1, 2) + lr.shape[1:3])
    for k in range(T - 1):
        fw[k, 0], fw[k, 1] = L.coarse2fine_flow(lr[k], lr[k + 1], levels)[:2]
        bw[k, 0], bw[k, 1] = L.coarse2fine_flow(lr[k + 1], lr[k], levels)[:2]
    return fw, bw


# measured gains over bicubic with the oracle's flows at the defaults: (iters = 0 over BILINEAR, iters = 2 over bicubic,
# iters = 2 over two back-projection steps of the bicubic frame)
ESTIMATED = {
    (PANS[0], False): (0.87, 0.77, 0.51), (PANS[1], False): (1.24, 1.15, 0.82), (PANS[2], False): (1.40, 1.35, 0.82),
    (PANS[0], True): (1.46, 1.45, 1.19), (PANS[1], True): (1.97, 2.00, 1.67), (PANS[2], True): (2.41, 2.60, 2.07),
}


@pytest.mark.parametrize("pan,colour", list(ESTIMATED))
def test_quality_estimated_flows(pan, colour):
    """The same low-resolution videos at scale 2 with the oracle's flows (both directions of every consecutive pair, 4
    levels; mean error against the exact flows 0.15 .. 0.17 px on the grey videos, 0.08 .. 0.09 px in colour) through the
    restatement at the defaults.  Measured gains of the centre frame over bicubic upsampling, dB:
                               iters 0    iters 2    bicubic + the same 2 steps    iters 0 over bilinear
        grey   pan (0.5, 0.25)    -0.05      +0.77      +0.26                         +0.87
        grey   pan (0.3, 0.2)     +0.11      +1.15      +0.33                         +1.24
        grey   pan (1.37, -0.61)  -0.26      +1.35      +0.53                         +1.40
        colour pan (0.5, 0.25)    +0.53      +1.45      +0.26                         +1.46
        colour pan (0.3, 0.2)     +0.82      +2.00      +0.33                         +1.97
        colour pan (1.37, -0.61)  +0.72      +2.60      +0.53                         +2.41
    WITHOUT back-projection the gain over bicubic is NOT reliably positive with estimated flows (-0.26 .. +0.11 dB on the grey
    videos): a flow error of a sixth of a pixel is a third of a fine pixel.  What does hold, and is asserted (each measured
    value minus 0.2 dB): the shift-and-add result alone beats bilinear upsampling, with the default two steps it beats
    bicubic, and it beats the same two steps applied to the bicubic frame -- the neighbours' samples are what helps.
    The defaults, from the grid sigma in (None, 0.05, 0.15, 0.3) x prior in (0.02, 0.05, 0.2) x iters in (0, 1, 2, 4) on the
    three grey videos (gain over bicubic at iters 2, the three pans in the order above):
        sigma None: +0.87 +1.25 +1.48    0.05: +0.45 +0.76 +0.81    0.15: +0.77 +1.15 +1.35    0.3: +0.84 +1.23 +1.45   (prior 0.05)
        prior 0.02: +0.76 +1.14 +1.31    0.05: +0.77 +1.15 +1.35    0.2:  +0.79 +1.14 +1.44                              (sigma 0.15)
        iters 0: -0.05 +0.11 -0.26       1: +0.62 +0.95 +1.01       2: +0.77 +1.15 +1.35       4: +0.82 +1.22 +1.50     (0.15, 0.05)
    prior moves the result by less than 0.1 dB; the first two steps bring nearly all of the back-projection's gain;
    sigma = 0.05 is too sharp (it rejects aliased detail, which is the signal), and on these occlusion-free pans no weight at
    all is 0.1 dB better than temporal_filter's 0.15, which is kept for the wrong flows of real videos that this protocol
    does not contain."""
    S = 2
    hr, lr, fw, bw = _video(_image(colour), pan, S)
    c = len(hr) // 2
    efw, ebw = _oracle_flows(lr)
    err = float(np.sqrt(((efw - fw) ** 2).sum(1))[:, 8:-8, 8:-8].mean())
    bicubic, bilinear = _psnr(_up(lr[c], S, "bicubic"), hr[c]), _psnr(_up(lr[c], S, "bilinear"), hr[c])
    y = _up(lr[c], S, "bicubic")
    for _ in range(2):
        y = backproject(y, lr[c], S)
    alone = _psnr(y, hr[c])
    p0 = _psnr(superres_reference(lr, efw, ebw, S, iters=0)[0][c], hr[c])
    p2 = _psnr(superres_reference(lr, efw, ebw, S, iters=2)[0][c], hr[c])
    got = (p0 - bilinear, p2 - bicubic, p2 - alone)
    print("pan %s colour %s: mean flow error %.3f px, bicubic %.2f bilinear %.2f bicubic + 2 steps %.2f dB | iters 0: %+.2f over "
          "bicubic, %+.2f over bilinear | iters 2: %+.2f over bicubic, %+.2f over bicubic + 2 steps"
          % (pan, colour, err, bicubic, bilinear, alone, p0 - bicubic, got[0], got[1], got[2]))
    for g, measured in zip(got, ESTIMATED[(pan, colour)]):
        assert g >= measured - 0.2


@pytest.mark.parametrize("colour", [False, True])
def test_static_video_is_the_weak_case(colour):
    """No sub-pixel motion, nothing to add.  At scale 2 every frame lands on the same half-phase and the result is close to
    bilinear upsampling; at scale 3 every sample lands on the centre of one fine pixel in nine and the rest is the prior's
    cubic base.  Measured against the full-resolution frame (grey / colour, iters 0; in brackets iters 2):
        scale 2: 22.97 / 22.90 dB (22.98 / 22.91), bilinear 22.97 / 22.92, bicubic 23.88 / 23.84: 0.9 dB BELOW bicubic
        scale 3: 21.44 / 21.37 dB (21.70 / 21.64), bilinear 21.07 / 20.99, bicubic 21.50 / 21.44
    Asserted: no worse than bilinear upsampling minus 0.1 dB."""
    for S in (2, 3):
        hr, lr, fw, bw = _video(_image(colour), (0.0, 0.0), S)
        c = len(hr) // 2
        bilinear, bicubic = _psnr(_up(lr[c], S, "bilinear"), hr[c]), _psnr(_up(lr[c], S, "bicubic"), hr[c])
        for iters in (0, 2):
            p = _psnr(superres_reference(lr, fw, bw, S, iters=iters)[0][c], hr[c])
            print("static, scale %d, colour %s, iters %d: %.2f dB, bilinear %.2f, bicubic %.2f" % (S, colour, iters, p, bilinear, bicubic))
            assert p >= bilinear - 0.1


# ---- argument errors, before any launch ----

@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused; CPU tensors pass for device ones"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")
    return calls


def _z(*shape, **kw):
    return torch.zeros(*shape, **kw)


@pytest.mark.parametrize("kw,exc", [
    (dict(scale=1), ValueError), (dict(scale=5), ValueError), (dict(scale=2.0), TypeError), (dict(scale=True), TypeError),
    (dict(radius=-1), ValueError), (dict(radius=1.5), TypeError), (dict(radius=2 ** 28), ValueError),
    (dict(sigma=-0.1), ValueError), (dict(sigma=math.nan), ValueError), (dict(sigma="soft"), TypeError),
    (dict(prior=0.0), ValueError), (dict(prior=2.0 ** -25), ValueError), (dict(prior=math.inf), ValueError),
    (dict(prior=None), TypeError), (dict(iters=-1), ValueError), (dict(iters=1.0), TypeError), (dict(iters=65537), ValueError),
    (dict(consistency=(0.1,)), TypeError), (dict(consistency=(-1.0, 0.5)), ValueError), (dict(consistency=(math.nan, 0.5)), ValueError),
    (dict(layout="CHWN"), ValueError), (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError),
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow_fw=_z(3, 2, 8, 8)), ValueError),
    (dict(flow_bw=_z(2, 2, 8, 9)), ValueError), (dict(flow_bw=None), TypeError), (dict(flow_fw=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(frames=_z(3, 5, 8, 8)), ValueError), (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(frames=_z(8, 8)), ValueError), (dict(frames=None), TypeError), (dict(frames=_z(3, 3, 0, 8)), ValueError),
])
def test_super_resolve_errors_before_any_launch(stub, kw, exc):
    args = dict(frames=_z(3, 3, 8, 8), flow_fw=_z(2, 2, 8, 8), flow_bw=_z(2, 2, 8, 8), scale=2)
    args.update(kw)
    with pytest.raises(exc):
        tensors.super_resolve(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), args.pop("scale"), **args)
    assert stub == []


def test_one_frame_takes_empty_flows_and_nothing_else(stub):
    for fw, bw, exc in ((_z(1, 2, 8, 8), _z(0, 2, 8, 8), ValueError), (_z(0, 2, 8, 8), _z(0, 2, 8, 9), ValueError),
                        (_z(0, 2, 8, 8), None, TypeError), (_z(0, 2, 8, 8, dtype=torch.int32), _z(0, 2, 8, 8), TypeError)):
        with pytest.raises(exc):
            tensors.super_resolve(_z(1, 3, 8, 8), fw, bw)
    assert stub == []
    assert tensors._check_sr_flows(_z(0, 2, 8, 8), _z(0, 2, 8, 8, dtype=torch.float64), 1, 8, 8, torch.device("cpu")) is None


def test_super_resolve_refuses_cpu_tensors(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    with pytest.raises(ValueError):
        tensors.super_resolve(_z(3, 3, 8, 8), _z(2, 2, 8, 8), _z(2, 2, 8, 8))
    with pytest.raises(ValueError):
        tensors.super_resolve_video(_z(3, 3, 8, 8), 2)
    assert calls == []


@pytest.mark.parametrize("kw,exc", [
    (dict(scale=6), ValueError), (dict(prior=0.0), ValueError), (dict(iters=-2), ValueError), (dict(radius=-1), ValueError),
    (dict(sigma=-1.0), ValueError), (dict(consistency=3), TypeError), (dict(pyramidLevels=0), ValueError),
    (dict(flows=_z(2, 2, 8, 8)), TypeError), (dict(flows=(_z(2, 2, 8, 8), _z(2, 2, 8, 9))), ValueError),
    (dict(flows=(_z(2, 2, 8, 8),)), TypeError), (dict(no_such_keyword=1), TypeError),
    (dict(frames=_z(1, 3, 8, 8)), ValueError), (dict(out_dtype=torch.float16), TypeError),
])
def test_super_resolve_video_errors_before_any_launch(stub, kw, exc):
    args = dict(frames=_z(3, 3, 8, 8), pyramidLevels=2)
    args.update(kw)
    with pytest.raises(exc):
        tensors.super_resolve_video(args.pop("frames"), args.pop("pyramidLevels"), **args)
    assert stub == []


# ---- the C ABI's own refusals (no device is needed: every one is decided before anything is enqueued) ----

def test_new_symbols_are_declared():
    assert "papof_super_resolve_tensor" in capi.SYMBOLS and "papof_sr_workspace" in capi.SYMBOLS
    L = capi.load()
    assert L.papof_sr_workspace.restype is ctypes.c_longlong and len(L.papof_super_resolve_tensor.argtypes) == 22


def test_sr_workspace_sizes_and_refusals():
    L = capi.load()
    fine = 8 * 4 * 135 * 240
    assert L.papof_sr_workspace(1, 135, 240, 3, 2, 0) == fine * 4                   # the accumulator alone
    assert L.papof_sr_workspace(1, 135, 240, 3, 2, 2) == fine * (4 + 6)            # ... and two buffers of X
    assert L.papof_sr_workspace(1, 135, 240, 3, 2, 1) == fine * (4 + 6)
    assert L.papof_sr_workspace(7, 135, 240, 1, 2, 2) == 7 * fine * (2 + 2)
    assert L.papof_sr_workspace(5, 135, 240, 3, 3, 0) == 5 * 8 * 9 * 135 * 240 * 4
    per = 8 * 4 * 1080 * 1920 * (4 + 6)                                            # 1080p -> 2160p, C = 3: 265 MB + 398 MB
    assert per == 663552000
    assert L.papof_sr_workspace(2, 1080, 1920, 3, 2, 2) == 2 * per
    assert L.papof_sr_workspace(100, 1080, 1920, 3, 2, 2) == 3 * per               # as many targets as fit 2 GiB
    assert L.papof_sr_workspace(100, 1080, 1920, 3, 2, 0) == 8 * (8 * 4 * 1080 * 1920 * 4)
    assert L.papof_sr_workspace(9, 2160, 3840, 3, 4, 2) == 8 * 16 * 2160 * 3840 * 10  # never less than one target
    assert L.papof_sr_workspace(1, 32768, 32767, 1, 2, 0) > 0                      # H W < 2^30
    for bad in ((0, 8, 8, 1, 2, 0), (1, 0, 8, 1, 2, 0), (1, 8, 0, 1, 2, 0), (1, 8, 8, 0, 2, 0), (1, 8, 8, 5, 2, 0),
                (1, 8, 8, 1, 1, 0), (1, 8, 8, 1, 5, 0), (1, 8, 8, 1, 2, -1), (1, 8, 8, 1, 2, 65537), (1, 32768, 32768, 1, 2, 0),
                (1, 2 ** 31 - 1, 2 ** 31 - 1, 1, 2, 0)):
        assert L.papof_sr_workspace(*bad) == -1, bad


def test_c_abi_refuses_bad_arguments_without_a_device():
    """PAPOF_EINVAL is decided before the handle is used: a fake non-NULL handle and fake pointers are never dereferenced"""
    L = capi.load()

    def T(dtype=capi.DTYPE_F64, strides=(64, 8, 1, 64), data=4096):
        t = capi.PapofTensor()
        t.data, t.dtype = data, dtype
        for i, s in enumerate(strides):
            t.stride[i] = s
        return t
    fr, flow, out, cov = T(), T(strides=(128, 8, 1, 64)), T(strides=(256, 16, 1, 256)), T(strides=(256, 16, 1, 0))
    nbytes = 8 * 4 * 8 * 8 * (2 + 2)
    ok = dict(h=ctypes.c_void_p(8), T=3, H=8, W=8, C=1, S=2, fr=fr, fw=flow, bw=flow, R=2, us=1, sigma=0.15, uc=1, a1=0.01, a2=0.5,
              prior=0.05, iters=2, out=out, cov=cov, ws=ctypes.c_void_p(4096), nbytes=nbytes)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        ref = lambda t: ctypes.byref(t) if t is not None else None  # noqa: E731
        return L.papof_super_resolve_tensor(a["h"], a["T"], a["H"], a["W"], a["C"], a["S"], ref(a["fr"]), ref(a["fw"]),
                                            ref(a["bw"]), a["R"], a["us"], a["sigma"], a["uc"], a["a1"], a["a2"], a["prior"],
                                            a["iters"], ref(a["out"]), ref(a["cov"]), a["ws"], a["nbytes"], None)
    for kw in (dict(h=None), dict(T=0), dict(H=0), dict(W=0), dict(C=0), dict(C=5), dict(S=1), dict(S=5), dict(R=-1),
               dict(sigma=-1.0), dict(sigma=math.nan), dict(sigma=math.inf), dict(a1=-0.1), dict(a2=math.nan),
               dict(prior=0.0), dict(prior=2.0 ** -25), dict(prior=math.nan), dict(prior=math.inf), dict(iters=-1),
               dict(H=16384, W=16384, R=2),                    # 5 H W >= 2^30
               dict(H=32768, W=32768, R=0),                    # H W >= 2^30
               dict(fr=None), dict(fr=T(data=None)), dict(fr=T(dtype=7)), dict(fr=T(strides=(64, -8, 1, 64))),
               dict(fw=None), dict(bw=None), dict(fw=T(dtype=capi.DTYPE_U8)), dict(bw=T(strides=(128, 8, -1, 64))),
               dict(out=None), dict(out=T(strides=(256, 16, 0, 256))), dict(out=T(dtype=9)),
               dict(cov=T(dtype=capi.DTYPE_F32, strides=(256, 16, 1, 0))), dict(cov=T(strides=(256, 0, 1, 0))),
               dict(ws=None), dict(nbytes=nbytes - 8), dict(nbytes=0)):
        assert call(**kw) == EINVAL, kw
