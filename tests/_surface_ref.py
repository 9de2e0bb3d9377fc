"""Decoder surfaces restated in numpy, written from the text of include/papof.h (papof_ycc_to_rgb_tensor,
papof_rgb_to_ycc_tensor): both integer rules, the tables of a matrix and a range, and the real-valued rules in float64 that
the integer ones approximate.  Nothing here calls the package.

Planes are numpy arrays: y (T, H, W), cb and cr (T, Hc, Wc) uint8 with Wc = ceil(W / 2), Hc = ceil(H / sub_v); RGB frames are
(T, H, W, 3).  siting = (horizontal, vertical), horizontal "left" | "center", vertical "center" | "top"."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
MATRICES, RANGES = tuple(KR_KB), ("limited", "full")
SITINGS = [(h, v) for h in ("left", "center") for v in ("center", "top")]
SCALE = 1 << 14
D = 257 * SCALE  # one level of a byte in the reverse rule's numerators: q = 257 b, coefficients at 2^14
FORWARD_BOUND = 0.5 + 511.0 / 32768.0      # LSB: the header's derivation
REVERSE_BOUND = 0.5 + 2.5 * 255.0 / 16384.0


def _rint(v):
    return int(np.rint(v))


def _ranges(rng):
    """(y_off, luma excursion / 255, chroma excursion / 255)"""
    return (16, 219.0 / 255.0, 224.0 / 255.0) if rng == "limited" else (0, 1.0, 1.0)


def tables(matrix, rng):
    """[y_off, cy, crv, cgu, cgv, cbu] of the forward rule"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y_off, sy, sc = _ranges(rng)
    return [y_off, _rint(SCALE / sy), _rint(SCALE * 2.0 * (1.0 - kr) / sc), _rint(SCALE * 2.0 * kb * (1.0 - kb) / kg / sc),
            _rint(SCALE * 2.0 * kr * (1.0 - kr) / kg / sc), _rint(SCALE * 2.0 * (1.0 - kb) / sc)]


def reverse_tables(matrix, rng):
    """[y_off, yr, yg, yb, ur, ug, vg, vb] of the reverse rule: yg is what is left of rint(2^14 sy), so a grey maps exactly"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y_off, sy, sc = _ranges(rng)
    yr, yb = _rint(SCALE * sy * kr), _rint(SCALE * sy * kb)
    return [y_off, yr, _rint(SCALE * sy) - yr - yb, yb,
            _rint(SCALE * sc * 0.5 * kr / (1.0 - kb)), _rint(SCALE * sc * 0.5 * kg / (1.0 - kb)),
            _rint(SCALE * sc * 0.5 * kg / (1.0 - kr)), _rint(SCALE * sc * 0.5 * kb / (1.0 - kr))]


def chroma_size(H, W, sub_v):
    return -(-H // sub_v), -(-W // 2)


# ---- forward: surfaces -> RGB
def h_taps(W, siting):
    """(a, b, wa, wb) per luma column: chroma columns (clamped) and weights that add to 4"""
    x = np.arange(W)
    k, odd = x >> 1, (x & 1) == 1
    if siting == "left":
        a, b, wa, wb = k, k + odd, np.where(odd, 2, 4), np.where(odd, 2, 0)
    else:
        a, b, wa, wb = np.where(odd, k, k - 1), np.where(odd, k + 1, k), np.where(odd, 3, 1), np.where(odd, 1, 3)
    Wc = -(-W // 2)
    return np.clip(a, 0, Wc - 1), np.clip(b, 0, Wc - 1), wa, wb


def v_taps(H, siting, interlaced, sub_v):
    """(a, b, wa, wb) per luma row: chroma ROWS OF THE FRAME (clamped) and weights that add to 8"""
    y = np.arange(H)
    if sub_v == 1:
        return y, y, np.full(H, 8), np.full(H, 0)
    Hc = -(-H // 2)
    if interlaced:
        assert H % 2 == 0 and H >= 4
        p, m, r = y & 1, y >> 2, y & 3
        a, b = np.where(r < 2, m - 1, m), np.where(r < 2, m, m + 1)
        wa = np.array([1, 3, 5, 7])[r]
        n = (Hc - p + 1) // 2  # the field's own chroma rows
        return 2 * np.clip(a, 0, n - 1) + p, 2 * np.clip(b, 0, n - 1) + p, wa, 8 - wa
    j, odd = y >> 1, (y & 1) == 1
    if siting == "center":
        a, b, wa = np.where(odd, j, j - 1), np.where(odd, j + 1, j), np.where(odd, 6, 2)
    else:
        a, b, wa = j, j + odd, np.where(odd, 4, 8)
    return np.clip(a, 0, Hc - 1), np.clip(b, 0, Hc - 1), wa, 8 - wa


def upsample32(c, H, W, siting, interlaced, sub_v):
    """C32 (T, H, W) int64 of a chroma plane c (T, Hc, Wc): 32 times the bilinear value, unrounded"""
    c = c.astype(np.int64)
    xa, xb, wxa, wxb = h_taps(W, siting[0])
    ra, rb, wya, wyb = v_taps(H, siting[1], interlaced, sub_v)
    rows = lambda r: wxa * c[:, r][:, :, xa] + wxb * c[:, r][:, :, xb]  # noqa: E731
    return wya[:, None] * rows(ra) + wyb[:, None] * rows(rb)


def _numerators(y, cb, cr, tab, siting, interlaced, sub_v):
    T, H, W = y.shape
    assert cb.shape == cr.shape == (T,) + chroma_size(H, W, sub_v)
    y_off, cy, crv, cgu, cgv, cbu = tab
    L = 32 * cy * (y.astype(np.int64) - y_off)
    u = upsample32(cb, H, W, siting, interlaced, sub_v) - 4096
    v = upsample32(cr, H, W, siting, interlaced, sub_v) - 4096
    N = np.stack([L + crv * v, L - cgu * u - cgv * v, L + cbu * u], -1)
    assert np.abs(N).max() < 2 ** 31 - 2 ** 18
    return N


def ycc_to_rgb_reference(y, cb, cr, tab, siting=("left", "center"), interlaced=False, sub_v=2, dtype=np.uint8):
    """(T, H, W, 3) of dtype: the integer rule"""
    N = _numerators(y, cb, cr, tab, siting, interlaced, sub_v)
    if dtype == np.uint8:
        return np.clip((N + (1 << 18)) >> 19, 0, 255).astype(np.uint8)
    return (np.clip(N, 0, 255 << 19).astype(np.float64) / float(255 << 19)).astype(dtype)


def ycc_to_rgb_real(y, cb, cr, matrix, rng, siting=("left", "center"), interlaced=False, sub_v=2):
    """(T, H, W, 3) float64 levels 0 .. 255: the rule the integers approximate -- the same bilinear chroma (its weights are
    exact), the matrix of the standard in float64, clamped and not rounded"""
    T, H, W = y.shape
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y_off, sy, sc = _ranges(rng)
    L = (y.astype(np.float64) - y_off) / sy
    u = (upsample32(cb, H, W, siting, interlaced, sub_v) / 32.0 - 128.0) / sc
    v = (upsample32(cr, H, W, siting, interlaced, sub_v) / 32.0 - 128.0) / sc
    r, b = L + 2.0 * (1.0 - kr) * v, L + 2.0 * (1.0 - kb) * u
    g = L - 2.0 * kb * (1.0 - kb) / kg * u - 2.0 * kr * (1.0 - kr) / kg * v
    return np.clip(np.stack([r, g, b], -1), 0.0, 255.0)


# ---- reverse: RGB -> surfaces
def quantise(frames):
    """q of include/papof.h: 257 b of a byte; of a float 0 for a NaN, else clamp(rint(65535.0 v), 0, 65535) in float64"""
    if frames.dtype == np.uint8:
        return 257 * frames.astype(np.int64)
    with np.errstate(invalid="ignore"):
        v = np.rint(65535.0 * frames.astype(np.float64))
    return np.clip(np.where(np.isnan(v), 0.0, v), 0.0, 65535.0).astype(np.int64)


def _reduce(N, axis, positions, weights, hi):
    """sum over the taps of weights[i] * N at positions[i] (arrays of indices along `axis`, clamped to 0 .. hi)"""
    return sum(w * np.take(N, np.clip(p, 0, hi), axis=axis) for p, w in zip(positions, weights))


def reduce16(N, siting, interlaced, sub_v):
    """(T, Hc, Wc) int64: the taps' sum of a per-pixel plane N (T, H, W); the weights add to 16"""
    T, H, W = N.shape
    Hc, Wc = chroma_size(H, W, sub_v)
    k = 2 * np.arange(Wc)
    if siting[0] == "left":
        N = _reduce(N, 2, (k - 1, k, k + 1), (1, 2, 1), W - 1)
    else:
        N = _reduce(N, 2, (k, k + 1), (2, 2), W - 1)
    if sub_v == 1:
        return 4 * N
    if interlaced:
        assert H % 2 == 0 and H >= 4
        j = np.arange(Hc)
        p, m = j & 1, j >> 1
        first, second = 4 * m + p, np.minimum(4 * m + p + 2, H - 2 + p)  # clamped within the field's rows
        return np.where(p == 0, 3, 1)[:, None] * N[:, first] + np.where(p == 0, 1, 3)[:, None] * N[:, second]
    j = 2 * np.arange(Hc)
    if siting[1] == "center":
        return _reduce(N, 1, (j, j + 1), (2, 2), H - 1)
    return _reduce(N, 1, (j - 1, j, j + 1), (1, 2, 1), H - 1)


def rgb_to_ycc_reference(frames, tab, siting=("left", "center"), interlaced=False, sub_v=2):
    """(y, cb, cr) uint8 of frames (T, H, W, 3) uint8 / float32 / float64: the integer rule"""
    q = quantise(frames)
    y_off, yr, yg, yb, ur, ug, vg, vb = tab
    R, G, B = q[..., 0], q[..., 1], q[..., 2]
    y = np.clip((yr * R + yg * G + yb * B + y_off * D + D // 2) // D, 0, 255).astype(np.uint8)
    planes = []
    for N in ((ur + ug) * B - ur * R - ug * G, (vg + vb) * R - vg * G - vb * B):
        S = reduce16(N, siting, interlaced, sub_v)
        planes.append(np.clip((S + 128 * 16 * D + 8 * D) // (16 * D), 0, 255).astype(np.uint8))
    return y, planes[0], planes[1]


def rgb_to_ycc_real(frames, matrix, rng, siting=("left", "center"), interlaced=False, sub_v=2):
    """(y, cb, cr) float64 levels: the standard's matrix on q / 257 in float64, the same taps, clamped and not rounded"""
    v = quantise(frames).astype(np.float64) / 257.0
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y_off, sy, sc = _ranges(rng)
    Y = kr * v[..., 0] + kg * v[..., 1] + kb * v[..., 2]
    u, w = sc * 0.5 * (v[..., 2] - Y) / (1.0 - kb), sc * 0.5 * (v[..., 0] - Y) / (1.0 - kr)
    c = [128.0 + _float_reduce(p, siting, interlaced, sub_v) for p in (u, w)]
    return np.clip(y_off + sy * Y, 0, 255), np.clip(c[0], 0, 255), np.clip(c[1], 0, 255)


def _float_reduce(N, siting, interlaced, sub_v):
    T, H, W = N.shape
    Hc, Wc = chroma_size(H, W, sub_v)
    k = 2 * np.arange(Wc)
    N = _reduce(N, 2, (k - 1, k, k + 1), (0.25, 0.5, 0.25), W - 1) if siting[0] == "left" else _reduce(N, 2, (k, k + 1), (0.5, 0.5), W - 1)
    if sub_v == 1:
        return N
    if interlaced:
        j = np.arange(Hc)
        p, m = j & 1, j >> 1
        first, second = 4 * m + p, np.minimum(4 * m + p + 2, H - 2 + p)
        return np.where(p == 0, 0.75, 0.25)[:, None] * N[:, first] + np.where(p == 0, 0.25, 0.75)[:, None] * N[:, second]
    j = 2 * np.arange(Hc)
    if siting[1] == "center":
        return _reduce(N, 1, (j, j + 1), (0.5, 0.5), H - 1)
    return _reduce(N, 1, (j - 1, j, j + 1), (0.25, 0.5, 0.25), H - 1)


def psnr(a, b):
    e = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if e == 0 else 10.0 * np.log10(255.0 ** 2 / e)
