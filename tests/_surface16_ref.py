"""High-bit-depth decoder surfaces restated in numpy, written from the text of include/papof.h (papof_ycc16_to_rgb_tensor,
papof_rgb_to_ycc16_tensor): both integer rules, the tables of a matrix, a range and a depth, and the real-valued rules in
float64 that the integer ones approximate.  Nothing here calls the package.  The header takes its taps from the 8-bit calls
"word for word": they are _surface_ref's (upsample32, reduce16), and so is q (quantise).

Planes are numpy arrays of uint16 WORDS: y (T, H, W), cb and cr (T, Hc, Wc); the sample of a word is (word >> shift) & P with
P = 2^depth - 1.  RGB frames are (T, H, W, 3).  The rules are written for any depth d >= 8, so that d = 8 can be held against
_surface_ref; the device takes 9 .. 16."""
from fractions import Fraction

import numpy as np

from _surface_ref import MATRICES, RANGES, SITINGS, chroma_size, quantise, reduce16, upsample32, _float_reduce  # noqa: F401

KR_KB = {"bt601": ("0.299", "0.114"), "bt709": ("0.2126", "0.0722"), "bt2020": ("0.2627", "0.0593")}
DEPTHS = (9, 10, 12, 16)
E = 65535 << 14  # one level of q at the reverse coefficients' scale
FORWARD_BOUND = 2.0 ** -6          # LSB of d bits (float results), and beyond 0.5 LSB of 8 bits (uint8): the header's derivation
REVERSE_BOUND = 0.5 + 2.0 ** -13   # LSB of d bits


def _k(matrix):
    kr, kb = (Fraction(s) for s in KR_KB[matrix])
    return kr, kb, 1 - kr - kb


def _ranges(rng, d):
    """(y_off, Sy, Sc): the luma offset and the excursions of luma and chroma in levels of d bits"""
    m, P = 1 << (d - 8), (1 << d) - 1
    return (16 * m, 219 * m, 224 * m) if rng == "limited" else (0, P, P)


def shift_of(d, aligned):
    return 16 - d if aligned == "msb" else 0


def tables(matrix, rng, d, peak=None):
    """[y_off, cy, crv, cgu, cgv, cbu, peak] of the forward rule: coefficients at 2^(d+6) for the output level `peak` = 1.0"""
    kr, kb, kg = _k(matrix)
    y_off, sy, sc = _ranges(rng, d)
    Q = (1 << d) - 1 if peak is None else peak
    one = Q << (d + 6)
    return [y_off, round(Fraction(one, sy))] + [round(one * f / sc) for f in (
        2 * (1 - kr), 2 * kb * (1 - kb) / kg, 2 * kr * (1 - kr) / kg, 2 * (1 - kb))] + [Q]


def reverse_tables(matrix, rng, d):
    """[y_off, yr, yg, yb, ur, ug, vg, vb] of the reverse rule: yg is what is left of 2^14 Sy, so a grey maps exactly"""
    kr, kb, kg = _k(matrix)
    y_off, sy, sc = _ranges(rng, d)
    one_y, half_c = sy << 14, sc << 13
    yr, yb = round(one_y * kr), round(one_y * kb)
    return [y_off, yr, one_y - yr - yb, yb, round(half_c * kr / (1 - kb)), round(half_c * kg / (1 - kb)),
            round(half_c * kg / (1 - kr)), round(half_c * kb / (1 - kr))]


def samples(words, d, shift):
    return (words.astype(np.int64) >> shift) & ((1 << d) - 1)


def words(levels, shift):
    return (levels.astype(np.int64) << shift).astype(np.uint16)


# ---- forward: surfaces -> RGB
def numerators(y, cb, cr, tab, d, shift, siting, interlaced, sub_v):
    """N (T, H, W, 3) int64 of planes of words"""
    T, H, W = y.shape
    assert cb.shape == cr.shape == (T,) + chroma_size(H, W, sub_v)
    y_off, cy, crv, cgu, cgv, cbu = tab[:6]
    L = 32 * cy * (samples(y, d, shift) - y_off)
    u = upsample32(samples(cb, d, shift), H, W, siting, interlaced, sub_v) - (1 << (d + 4))
    v = upsample32(samples(cr, d, shift), H, W, siting, interlaced, sub_v) - (1 << (d + 4))
    N = np.stack([L + crv * v, L - cgu * u - cgv * v, L + cbu * u], -1)
    assert np.abs(N).max() < 1 << (2 * d + 14)  # the header's bound, 2^46 at 16 bits
    return N


def ycc16_to_rgb_reference(y, cb, cr, tab, d, shift, siting=("left", "center"), interlaced=False, sub_v=2, dtype=np.float32):
    """(T, H, W, 3) of dtype: the integer rule"""
    N = numerators(y, cb, cr, tab, d, shift, siting, interlaced, sub_v)
    if dtype == np.uint8:
        assert tab[6] == 255
        return np.clip((N + (1 << (d + 10))) >> (d + 11), 0, 255).astype(np.uint8)
    one = tab[6] << (d + 11)
    assert one < 1 << 53
    return (np.clip(N, 0, one).astype(np.float64) / float(one)).astype(dtype)


def ycc16_to_rgb_real(y, cb, cr, matrix, rng, d, shift, peak, siting=("left", "center"), interlaced=False, sub_v=2):
    """(T, H, W, 3) float64 levels 0 .. peak: the rule the integers approximate -- the same bilinear chroma (its weights are
    exact), the matrix of the standard in float64, clamped and not rounded"""
    T, H, W = y.shape
    kr, kb, kg = (float(k) for k in _k(matrix))
    y_off, sy, sc = _ranges(rng, d)
    L = (samples(y, d, shift).astype(np.float64) - y_off) / sy
    u = (upsample32(samples(cb, d, shift), H, W, siting, interlaced, sub_v) / 32.0 - float(1 << (d - 1))) / sc
    v = (upsample32(samples(cr, d, shift), H, W, siting, interlaced, sub_v) / 32.0 - float(1 << (d - 1))) / sc
    r, b = L + 2.0 * (1.0 - kr) * v, L + 2.0 * (1.0 - kb) * u
    g = L - 2.0 * kb * (1.0 - kb) / kg * u - 2.0 * kr * (1.0 - kr) / kg * v
    return np.clip(peak * np.stack([r, g, b], -1), 0.0, float(peak))


# ---- reverse: RGB -> surfaces
def chroma_numerators(frames, tab):
    q = quantise(frames)
    R, G, B = q[..., 0], q[..., 1], q[..., 2]
    ur, ug, vg, vb = tab[4:]
    return (ur + ug) * B - ur * R - ug * G, (vg + vb) * R - vg * G - vb * B


def rgb_to_ycc16_reference(frames, tab, d, shift, siting=("left", "center"), interlaced=False, sub_v=2):
    """(y, cb, cr) uint16 words of frames (T, H, W, 3) uint8 / float32 / float64: the integer rule"""
    q = quantise(frames)
    P = (1 << d) - 1
    y_off, yr, yg, yb = tab[:4]
    R, G, B = q[..., 0], q[..., 1], q[..., 2]
    planes = [np.clip((yr * R + yg * G + yb * B + y_off * E + E // 2) // E, 0, P)]
    for N in chroma_numerators(frames, tab):
        S = reduce16(N, siting, interlaced, sub_v)
        assert np.abs(S).max() < 1 << 51
        planes.append(np.clip((S + (1 << (d - 1)) * 16 * E + 8 * E) // (16 * E), 0, P))
    return tuple(words(p, shift) for p in planes)


def rgb_to_ycc16_real(frames, matrix, rng, d, siting=("left", "center"), interlaced=False, sub_v=2):
    """(y, cb, cr) float64 levels of d bits: the standard's matrix on q / 65535 in float64, the same taps, clamped, not rounded"""
    v = quantise(frames).astype(np.float64) / 65535.0
    kr, kb, kg = (float(k) for k in _k(matrix))
    y_off, sy, sc = _ranges(rng, d)
    P = float((1 << d) - 1)
    Y = kr * v[..., 0] + kg * v[..., 1] + kb * v[..., 2]
    u, w = sc * 0.5 * (v[..., 2] - Y) / (1.0 - kb), sc * 0.5 * (v[..., 0] - Y) / (1.0 - kr)
    c = [float(1 << (d - 1)) + _float_reduce(p, siting, interlaced, sub_v) for p in (u, w)]
    return np.clip(y_off + sy * Y, 0, P), np.clip(c[0], 0, P), np.clip(c[1], 0, P)


def psnr(a, b, peak):
    e = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if e == 0 else 10.0 * np.log10(float(peak) ** 2 / e)
