"""CPU-side checks of the high-bit-depth decoder surfaces (papteam_opticalflow_amd/tensors.py: ycc16_to_rgb, rgb_to_ycc16,
ycc_tables16, p010_planes, i010_planes, y210_planes, new_p010; include/papof.h: papof_ycc16_to_rgb_tensor,
papof_rgb_to_ycc16_tensor): the numpy restatement in tests/_surface16_ref.py -- at depth 8 it is the 8-bit restatement to the
byte; at 9, 10, 12 and 16 bits the integer rules against the real-valued ones within the header's bounds for every matrix,
range and siting, greys, the numerators' bounds; the round trip on the committed crop beside the 8-bit one --, the package's
tables against the restatement's, the view helpers on CPU tensors, every Python argument error raised before a launch, and
each refusal of the C ABI through ctypes.  No device is touched here."""
import ctypes
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _surface16_ref as R16  # noqa: E402
import _surface_ref as R  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (Surfaces, i010_planes, new_p010, p010_planes, rgb_to_ycc16, y210_planes,  # noqa: E402
                                             ycc16_to_rgb, ycc_tables16)
from test_surface_cpu import _lib, _on_gpu_stub, _ref, _t, _with, crop, stub  # noqa: E402,F401

RULES = [(s, i) for s in R.SITINGS for i in (False, True)]  # (siting, interlaced)


def random_words(rng, T, H, W, sub_v, d, shift):
    """planes of words whose samples take all codes of d bits, the extremes planted, every other bit 0"""
    Hc, Wc = R.chroma_size(H, W, sub_v)
    P = (1 << d) - 1
    ps = []
    for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc)):
        lv = rng.integers(0, P + 1, s)
        lv.reshape(-1)[:2] = (0, P)[:lv.size]
        ps.append((lv << shift).astype(np.uint16))
    return ps


def dirtied(ps, d, shift, seed):
    """(the planes, the same samples with random bits in the rest of every word)"""
    rng = np.random.default_rng(seed)
    keep = ((1 << d) - 1) << shift
    dirty = [(p | (rng.integers(0, 1 << 16, p.shape) & ~keep & 0xffff)).astype(np.uint16) for p in ps]
    assert all((a != b).any() and ((a & keep) == (b & keep)).all() for a, b in zip(ps, dirty))
    return ps, dirty


# ---- depth 8 is the 8-bit restatement
@pytest.mark.parametrize("matrix,rng", list(itertools.product(R.MATRICES, R.RANGES)))
def test_at_depth_8_the_tables_and_the_bytes_are_the_8_bit_rules(matrix, rng):
    tab = R16.tables(matrix, rng, 8, peak=255)
    assert tab[:6] == R.tables(matrix, rng) and tab[6] == 255
    g = np.random.default_rng(3)
    for (siting, inter), sub_v in itertools.product(RULES, (1, 2)):
        csize = (2,) + R.chroma_size(10, 13, sub_v)
        ps = [g.integers(0, 256, s).astype(np.uint8) for s in ((2, 10, 13), csize, csize)]
        for dtype in (np.uint8, np.float64):
            want = R.ycc_to_rgb_reference(*ps, R.tables(matrix, rng), siting, inter, sub_v, dtype=dtype)
            got = R16.ycc16_to_rgb_reference(*(p.astype(np.uint16) for p in ps), tab, 8, 0, siting, inter, sub_v, dtype=dtype)
            assert got.tobytes() == want.tobytes(), (siting, inter, sub_v, dtype)


# ---- the tables
@pytest.mark.parametrize("d", range(9, 17))
def test_the_packages_tables_are_the_restatements(d):
    P = (1 << d) - 1
    for matrix, rng in itertools.product(R.MATRICES, R.RANGES):
        fw, u8, rv = ycc_tables16(matrix, rng, d), ycc_tables16(matrix, rng, d, peak=255), ycc_tables16(matrix, rng, d, reverse=True)
        assert fw == R16.tables(matrix, rng, d) and u8 == R16.tables(matrix, rng, d, 255) and rv == R16.reverse_tables(matrix, rng, d)
        assert len(fw) == 7 and len(rv) == 8 and all(isinstance(v, int) for v in fw + u8 + rv)
        assert fw[6] == P and u8[6] == 255 and 0 <= fw[0] <= P and fw[0] == rv[0] == (16 << (d - 8) if rng == "limited" else 0)
        assert all(0 <= v < 1 << (d + 8) for v in fw[1:6] + u8[1:6]) and all(0 <= v <= 1 << 30 for v in rv[1:])
        sy = 219 << (d - 8) if rng == "limited" else P
        assert rv[1] + rv[2] + rv[3] == sy << 14
        if rng == "full":
            assert fw[1] == 1 << (d + 6)  # Q = P over Sy = P
    assert ycc_tables16(depth=d) == ycc_tables16("bt709", "limited", d)


def test_ycc_tables16_errors():
    for kw in (dict(matrix="bt470"), dict(range="tv"), dict(depth=8), dict(depth=17), dict(depth=10.0), dict(depth=True),
               dict(peak=0), dict(peak=65536), dict(peak=255.0), dict(depth=9, peak=65535), dict(reverse=True, peak=255)):
        with pytest.raises(ValueError):
            ycc_tables16(**kw)


# ---- the integer rules against the real-valued ones, greys, bounds
def test_the_bounds_are_the_headers():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "papof.h")).read()
    header = " ".join(header.replace("\n *", "\n").split())  # the comment's lines joined
    assert "within 2^-6 LSB of d bits" in header and "0.5 + 2^-6 = 0.5156 LSB of 8 bits" in header and R16.FORWARD_BOUND == 2.0 ** -6
    assert "within 0.5 + 2^-13 LSB of d bits" in header and R16.REVERSE_BOUND == 0.5 + 2.0 ** -13
    assert "|N| < 2^(2d+14) <= 2^46" in header and "|S| < 2^51" in header


@pytest.mark.parametrize("d", R16.DEPTHS)
def test_the_integer_rules_are_within_their_bounds_of_the_real_valued_ones(d):
    """forward: 2^-6 LSB of d bits for a float result, 0.5 + 2^-6 LSB of 8 bits for a uint8 one; reverse: 0.5 + 2^-13 LSB of d
    bits; for every matrix x range x siting x interlaced x sub_v.  The worst measured over all rules is printed."""
    worst = [0.0, 0.0, 0.0]
    P = (1 << d) - 1
    g = np.random.default_rng(5 + d)
    T, H, W = 1, 22, 37
    for matrix, rng, (siting, inter), sub_v in itertools.product(R.MATRICES, R.RANGES, RULES, (1, 2)):
        shift = (16 - d) * (sub_v - 1)  # both alignments
        ps = random_words(g, T, H, W, sub_v, d, shift)
        f = R16.ycc16_to_rgb_reference(*ps, R16.tables(matrix, rng, d), d, shift, siting, inter, sub_v, dtype=np.float64)
        real = R16.ycc16_to_rgb_real(*ps, matrix, rng, d, shift, P, siting, inter, sub_v)
        worst[0] = max(worst[0], np.abs(P * f - real).max())
        f32 = R16.ycc16_to_rgb_reference(*ps, R16.tables(matrix, rng, d), d, shift, siting, inter, sub_v, dtype=np.float32)
        assert f32.dtype == np.float32 and np.abs(f32.astype(np.float64) - f).max() <= 2.0 ** -24  # one more rounding
        b = R16.ycc16_to_rgb_reference(*ps, R16.tables(matrix, rng, d, 255), d, shift, siting, inter, sub_v, dtype=np.uint8)
        real8 = R16.ycc16_to_rgb_real(*ps, matrix, rng, d, shift, 255, siting, inter, sub_v)
        worst[1] = max(worst[1], np.abs(b.astype(np.float64) - real8).max())
        frames = g.uniform(-0.1, 1.1, (T, H, W, 3))
        frames.reshape(-1)[:2] = (0.0, 1.0)
        back = R16.rgb_to_ycc16_reference(frames, R16.reverse_tables(matrix, rng, d), d, shift, siting, inter, sub_v)
        want = R16.rgb_to_ycc16_real(frames, matrix, rng, d, siting, inter, sub_v)
        for a, w in zip(back, want):
            assert not (a & ~np.uint16(P << shift)).any()  # the word's other bits are 0
            worst[2] = max(worst[2], np.abs(R16.samples(a, d, shift).astype(np.float64) - w).max())
    print("depth %d: forward float %.4f LSB of %d bits, uint8 %.4f LSB of 8 bits; reverse %.6f LSB" % (d, worst[0], d, worst[1], worst[2]))
    assert worst[0] <= R16.FORWARD_BOUND and worst[1] <= 0.5 + R16.FORWARD_BOUND and worst[2] <= R16.REVERSE_BOUND


@pytest.mark.parametrize("d", R16.DEPTHS)
def test_greys_have_neutral_chroma_and_full_range_luma_is_the_level(d):
    P, mid = (1 << d) - 1, 1 << (d - 1)
    g = np.random.default_rng(d)
    q = g.integers(0, 65536, (2, 10, 13, 1))
    q.reshape(-1)[:2] = (0, 65535)
    grey = np.repeat(q / 65535.0, 3, axis=-1)
    assert (R.quantise(grey)[..., 0] == q[..., 0]).all()
    for matrix, rng, (siting, inter), sub_v in itertools.product(R.MATRICES, R.RANGES, RULES, (1, 2)):
        y, cb, cr = R16.rgb_to_ycc16_reference(grey, R16.reverse_tables(matrix, rng, d), d, 0, siting, inter, sub_v)
        assert (cb == mid).all() and (cr == mid).all(), (matrix, rng, siting, inter, sub_v)
        if rng == "full":
            want = q[..., 0] if d == 16 else np.rint(P * q[..., 0] / 65535.0)
            assert (y == want).all(), matrix
    grey8 = np.repeat(g.integers(0, 256, (1, 6, 8, 1)).astype(np.uint8), 3, axis=-1)
    _, cb, cr = R16.rgb_to_ycc16_reference(grey8, R16.reverse_tables("bt709", "limited", d), d, 16 - d)
    assert (cb == mid << (16 - d)).all() and (cr == mid << (16 - d)).all()


@pytest.mark.parametrize("d", R16.DEPTHS)
def test_the_numerators_stay_below_the_headers_bounds(d):
    """the extremes of every sample against the largest coefficients the C ABI admits, and against every standard's"""
    P = (1 << d) - 1
    big = [0, (1 << (d + 8)) - 1] + [(1 << (d + 8)) - 1] * 4 + [P]
    worst = 0
    for yv, u, v in itertools.product((0, P), repeat=3):
        ps = [np.full((1, 2, 2), yv, np.uint16), np.full((1, 1, 1), u, np.uint16), np.full((1, 1, 1), v, np.uint16)]
        for tab in [big, [P] + big[1:]] + [R16.tables(m, r, d) for m, r in itertools.product(R.MATRICES, R.RANGES)]:
            N = R16.numerators(*ps, tab, d, 0, ("left", "center"), False, 2)
            worst = max(worst, int(np.abs(N).max()))
    assert worst < 1 << (2 * d + 14) <= 1 << 46
    rv = [P] + [1 << 30] * 7
    for rgb in itertools.product((0.0, 1.0), repeat=3):
        f = np.empty((1, 4, 4, 3))
        f[...] = rgb
        for N in R16.chroma_numerators(f, rv):
            assert np.abs(N).max() < 1 << 47 and np.abs(R.reduce16(N, ("left", "center"), False, 2)).max() < 1 << 51
        R16.rgb_to_ycc16_reference(f, rv, d, 0)  # asserts |S| < 2^51 itself


def test_garbage_in_the_unused_bits_is_not_looked_at():
    for d, shift in ((10, 6), (10, 0), (12, 4)):
        clean, dirty = dirtied(random_words(np.random.default_rng(1), 1, 6, 8, 2, d, shift), d, shift, 9)
        tab = R16.tables("bt709", "limited", d)
        assert (R16.ycc16_to_rgb_reference(*clean, tab, d, shift) == R16.ycc16_to_rgb_reference(*dirty, tab, d, shift)).all()


def test_the_round_trip_at_10_bits_is_not_below_the_8_bit_one():
    """RGB -> 4:2:0 -> RGB on the 128 x 192 crop at (300, 600) of the committed 1080p frame, BT.709 limited: the decode of the
    encode against the frame, as bytes, through 10-bit planes and through 8-bit ones"""
    f = crop()[None]
    y, cb, cr = R.rgb_to_ycc_reference(f, R.reverse_tables("bt709", "limited"))
    db8 = R.psnr(R.ycc_to_rgb_reference(y, cb, cr, R.tables("bt709", "limited")), f)
    ps = R16.rgb_to_ycc16_reference(f, R16.reverse_tables("bt709", "limited", 10), 10, 6)
    db10 = R.psnr(R16.ycc16_to_rgb_reference(*ps, R16.tables("bt709", "limited", 10, 255), 10, 6, dtype=np.uint8), f)
    print("round trip of the crop: %.2f dB through 10-bit planes, %.2f dB through 8-bit planes" % (db10, db8))
    assert db10 >= db8


# ---- the view helpers: shapes, strides, shared storage
def _words(*shape, dtype=torch.uint16):
    return torch.from_numpy((np.arange(int(np.prod(shape)), dtype=np.int64) % 65521).astype(np.uint16).reshape(shape)).view(dtype)


def _offsets(p, s):
    return [(t.data_ptr() - s.data_ptr()) // 2 for t in p]


def test_p010_planes_are_views():
    T, H, W, pitch = 2, 6, 10, 16  # words
    for dtype in (torch.uint16, torch.int16):
        s = _words(T, H + 3, pitch, dtype=dtype)
        p = p010_planes(s, H, width=W)
        assert isinstance(p, Surfaces) and all(t.dtype == dtype for t in p)
        assert tuple(p.y.shape) == (T, H, W) and tuple(p.cb.shape) == tuple(p.cr.shape) == (T, 3, 5)
        assert p.y.stride() == (9 * pitch, pitch, 1) and p.cb.stride() == p.cr.stride() == (9 * pitch, pitch, 2)
        assert _offsets(p, s) == [0, H * pitch, H * pitch + 1]  # Cr one word beside Cb
        q = p010_planes(s, H, "vu", width=W)
        assert q.cr.data_ptr() == p.cb.data_ptr() and q.cb.data_ptr() == p.cr.data_ptr()
    p.cb[0, 0, 0] = 250
    assert int(s[0, H, 0]) == 250  # shared storage
    whole = p010_planes(s[0], H)  # a 2-D surface, the whole pitch
    assert tuple(whole.y.shape) == (1, H, pitch) and tuple(whole.cb.shape) == (1, 3, 8)
    assert tuple(p010_planes(_words(1, 5 + 3, 8), 5, width=7).cb.shape) == (1, 3, 4)  # odd sizes: chroma rounds up
    p210 = p010_planes(_words(1, 8, 8), 4, sub_v=1)
    assert tuple(p210.cb.shape) == (1, 4, 4) and _offsets(p210, p210.y) == [0, 32, 33]
    for bad in (dict(height=7), dict(height=0), dict(height=6, width=17), dict(height=6, order="uvw"), dict(height=6, sub_v=3),
                dict(height=6.0)):
        with pytest.raises(ValueError):
            p010_planes(s, **bad)
    for bad in (s.float(), s.to(torch.int32), None):
        with pytest.raises(TypeError):
            p010_planes(bad, H)
    with pytest.raises(ValueError):
        p010_planes(s[0, 0], H)


def test_a_surface_of_bytes_is_reinterpreted():
    T, H, W, pitch = 2, 6, 10, 32  # bytes
    raw = torch.arange(3 + T * 9 * pitch, dtype=torch.int64).remainder(251).to(torch.uint8)
    s = raw[2:2 + T * 9 * pitch].view(T, 9, pitch)  # 2 bytes into its storage
    p = p010_planes(s, H, width=W)
    assert all(t.dtype == torch.uint16 for t in p) and tuple(p.y.shape) == (T, H, W)
    assert p.y.stride() == (9 * 16, 16, 1) and p.cb.stride() == (9 * 16, 16, 2)
    assert [t.data_ptr() - s.data_ptr() for t in p] == [0, H * pitch, H * pitch + 2]
    assert int(p.y[1, 2, 3]) == int(s[1, 2, 6]) + 256 * int(s[1, 2, 7])  # little-endian words
    assert tuple(i010_planes(s, H, width=W).cb.shape) == (T, 3, 5) and tuple(y210_planes(s).y.shape) == (T, 9, 8)
    for bad in (raw[1:1 + T * 9 * pitch].view(T, 9, pitch),       # an odd storage offset
                raw[:T * 9 * 31].view(T, 9, 31),                  # an odd pitch
                s[:, :, ::2],                                     # bytes that are not adjacent
                raw[:2 * 9 * 32 + 1].as_strided((2, 9, 30), (9 * 32 + 1, 32, 1))):   # an odd frame stride
        with pytest.raises(ValueError):
            p010_planes(bad, H, width=W)


def test_i010_planes_are_views():
    T, H, W, pitch = 2, 6, 10, 12
    s = _words(T, 9, pitch)
    p = i010_planes(s, H, width=W)
    assert tuple(p.y.shape) == (T, H, W) and tuple(p.cb.shape) == tuple(p.cr.shape) == (T, 3, 5)
    assert p.cb.stride() == (9 * pitch, pitch // 2, 1)
    assert _offsets(p, s) == [0, H * pitch, H * pitch + 3 * (pitch // 2)]
    flat = s.reshape(T, -1)
    assert torch.equal(p.cb[1].view(torch.int16), flat[1, H * pitch:H * pitch + 3 * 6].reshape(3, 6)[:, :5].view(torch.int16))
    q = i010_planes(s, H, "vu", width=W)
    assert q.cr.data_ptr() == p.cb.data_ptr() and q.cb.data_ptr() == p.cr.data_ptr()
    sliced = i010_planes(_words(3, 9, pitch)[1:], H)  # a storage offset is kept
    assert _offsets(sliced, sliced.y)[1] == H * pitch
    p422 = i010_planes(_words(1, 12, pitch), H, sub_v=1)  # yuv422p10le: 6 + 2 * 6 / 2 rows
    assert tuple(p422.cb.shape) == (1, 6, 6) and _offsets(p422, p422.y) == [0, 6 * pitch, 9 * pitch]
    for bad in (dict(surface=_words(1, 9, 11), height=6), dict(surface=_words(1, 8, 12), height=6),
                dict(surface=_words(1, 9, 24)[:, :, ::2], height=6), dict(surface=s, height=6, order="yuv"),
                dict(surface=_words(1, 11, 12), height=6, sub_v=1), dict(surface=s, height=6, sub_v=0)):
        with pytest.raises(ValueError):
            i010_planes(**bad)
    with pytest.raises(TypeError):
        i010_planes(s.double(), H)


def test_y210_planes_are_views():
    T, H, W = 2, 3, 8
    s = _words(T, H, 2 * W)
    for order, offs in (("yuyv", (0, 1, 3)), ("uyvy", (1, 0, 2)), ("yvyu", (0, 3, 1)), ("vyuy", (1, 2, 0))):
        p = y210_planes(s, order)
        assert tuple(p.y.shape) == (T, H, W) and tuple(p.cb.shape) == tuple(p.cr.shape) == (T, H, W // 2)
        assert p.y.stride() == (H * 2 * W, 2 * W, 2) and p.cb.stride() == p.cr.stride() == (H * 2 * W, 2 * W, 4)
        assert _offsets(p, s) == list(offs)
    assert _offsets(y210_planes(s), s) == [0, 1, 3]
    for bad in (dict(surface=_words(1, 3, 10)), dict(surface=s, order="y210")):
        with pytest.raises(ValueError):
            y210_planes(**bad)
    with pytest.raises(TypeError):
        y210_planes(s.float())


def test_new_p010():
    s, p = new_p010(2, 5, 7, "cpu")
    assert tuple(s.shape) == (2, 8, 128) and s.dtype == torch.uint16 and not bool(s.view(torch.int16).any())  # 256 bytes a row
    assert tuple(p.y.shape) == (2, 5, 7) and tuple(p.cb.shape) == (2, 3, 4) and p.cr.data_ptr() == p.cb.data_ptr() + 2
    assert tuple(new_p010(1, 4, 129, "cpu")[0].shape) == (1, 6, 256)  # 258 bytes round up to 512
    s, p = new_p010(1, 4, 300, "cpu", pitch=608)
    assert tuple(s.shape) == (1, 6, 304) and p.y.stride() == (6 * 304, 304, 1)
    for bad in (dict(T=0), dict(H=0), dict(W=2.0), dict(pitch=14), dict(pitch=17), dict(pitch=True)):
        with pytest.raises(ValueError):
            new_p010(**{**dict(T=1, H=4, W=7, device="cpu"), **bad})


# ---- every Python argument error, before a launch
def _p(*shape, dtype=torch.uint16, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_Y, _C = lambda: _p(2, 8, 12), lambda: _p(2, 4, 6)  # noqa: E731
_RULE_ERRORS = [
    (dict(depth=8), ValueError), (dict(depth=17), ValueError), (dict(depth=10.0), ValueError), (dict(depth=None), ValueError),
    (dict(depth=True), ValueError), (dict(aligned="left"), ValueError), (dict(aligned=6), ValueError), (dict(aligned=None), ValueError),
    (dict(matrix="bt470"), ValueError), (dict(range="video"), ValueError),
    (dict(siting="left"), TypeError), (dict(siting=("center", "left")), ValueError), (dict(interlaced=2), ValueError),
    (dict(sub_v=0), ValueError), (dict(sub_v=True), ValueError), (dict(layout="CHWN"), ValueError),
]


def test_cpu_tensors_are_refused(stub):  # noqa: F811
    with pytest.raises(ValueError):
        ycc16_to_rgb(_Y(), _C(), _C())
    with pytest.raises(ValueError):
        rgb_to_ycc16(torch.zeros(2, 8, 12, 3))
    assert stub == []


_FORWARD_ERRORS = _RULE_ERRORS + [
    (dict(y=None), TypeError), (dict(cb=np.zeros((2, 4, 6), np.uint16)), TypeError),
    (dict(y=_p(2, 8, 12, dtype=torch.uint8)), TypeError), (dict(cr=_p(2, 4, 6, dtype=torch.int32)), TypeError),
    (dict(cb=_p(2, 4, 6, dtype=torch.float16)), TypeError),
    (dict(y=_p(2, 1, 8, 12)), ValueError), (dict(y=_p(12)), ValueError),
    (dict(y=_p(0, 8, 12), cb=_p(0, 4, 6), cr=_p(0, 4, 6)), ValueError),
    (dict(cb=_p(2, 4, 5)), ValueError), (dict(cr=_p(2, 3, 6)), ValueError), (dict(cb=_p(1, 4, 6)), ValueError),
    (dict(cb=_p(2, 8, 6)), ValueError), (dict(sub_v=1), ValueError),
    (dict(y=_p(2, 7, 12), interlaced=True), ValueError),
    (dict(cr=_p(2, 4, 6, device="meta")), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.uint16), TypeError), (dict(bogus=1), TypeError),
]


def test_ycc16_to_rgb_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch):  # noqa: F811
    _on_gpu_stub(monkeypatch)
    for kw, exc in _FORWARD_ERRORS:
        args = dict(kw)
        planes = [args.pop("y", _Y()), args.pop("cb", _C()), args.pop("cr", _C())]
        with pytest.raises(exc):
            ycc16_to_rgb(*planes, **args)
            pytest.fail("not refused: %r" % (kw,))
        assert stub == [], kw


_OUT = lambda **kw: tuple({**dict(y=_Y(), cb=_C(), cr=_C()), **kw}.values())  # noqa: E731
_REVERSE_ERRORS = _RULE_ERRORS + [
    (dict(frames=None), TypeError), (dict(frames=_p(2, 8, 12, 3)), TypeError),                # uint16 frames
    (dict(frames=torch.zeros(2, 8, 12, 4)), ValueError), (dict(frames=torch.zeros(2, 3, 8, 12)), ValueError),
    (dict(frames=torch.zeros(2, 7, 12, 3), interlaced=True), ValueError),
    (dict(out=_Y()), TypeError), (dict(out=(_Y(), _C())), TypeError),
    (dict(out=_OUT(cb=_p(2, 4, 6, dtype=torch.uint8))), TypeError), (dict(out=_OUT(y=None)), TypeError),
    (dict(out=_OUT(y=_p(2, 8, 10))), ValueError), (dict(out=_OUT(cr=_p(2, 8, 6))), ValueError),
    (dict(out=_OUT(cb=_p(2, 4, 1).expand(2, 4, 6))), ValueError),
    (dict(out=_OUT(cr=_p(2, 4, 6, device="meta"))), ValueError),
    (dict(out_dtype=torch.uint8), TypeError),
]


def test_rgb_to_ycc16_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch):  # noqa: F811
    _on_gpu_stub(monkeypatch)
    for kw, exc in _REVERSE_ERRORS:
        args = dict(kw)
        frames = args.pop("frames", torch.zeros(2, 8, 12, 3))
        with pytest.raises(exc):
            rgb_to_ycc16(frames, **args)
            pytest.fail("not refused: %r" % (kw,))
        assert stub == [], kw


def test_what_reaches_the_launch(monkeypatch):
    """with nothing wrong the calls hand the C ABI the sizes, depth, shift, codes and tables of their keywords, and return
    tensors of the documented shapes and dtypes (the launch itself is recorded, not made)"""
    _on_gpu_stub(monkeypatch)
    calls = []
    monkeypatch.setattr(tensors, "_launch", lambda dev, name, *a: calls.append((name,) + tuple(
        list(v) if isinstance(v, ctypes.Array) else v for v in a if isinstance(v, (int, ctypes.Array)))))
    rgb = ycc16_to_rgb(_Y(), _C(), _C())
    assert tuple(rgb.shape) == (2, 8, 12, 3) and rgb.dtype == torch.float32
    assert calls.pop() == ("papof_ycc16_to_rgb_tensor", 2, 8, 12, 10, 6, 2, 0, 0, 0, R16.tables("bt709", "limited", 10))
    rgb = ycc16_to_rgb(_Y()[0].view(torch.int16), _p(8, 6), _p(8, 6), depth=12, aligned="lsb", interlaced=True, sub_v=1,
                       siting=("center", "top"), matrix="bt2020", range="full", layout="NCHW", out_dtype=torch.uint8)
    assert tuple(rgb.shape) == (1, 3, 8, 12) and rgb.dtype == torch.uint8
    assert calls.pop() == ("papof_ycc16_to_rgb_tensor", 1, 8, 12, 12, 0, 1, 1, 1, 1, R16.tables("bt2020", "full", 12, 255))
    assert ycc16_to_rgb(_Y(), _C(), _C(), depth=16, out_dtype=torch.float64).dtype == torch.float64
    assert calls.pop()[4:6] == (16, 0)
    s = rgb_to_ycc16(torch.zeros(2, 9, 13, 3, dtype=torch.float64), matrix="bt2020", depth=12)
    assert isinstance(s, Surfaces) and [tuple(p.shape) for p in s] == [(2, 9, 13), (2, 5, 7), (2, 5, 7)]
    assert all(p.dtype == torch.uint16 and p.is_contiguous() for p in s)
    assert calls.pop() == ("papof_rgb_to_ycc16_tensor", 2, 9, 13, 12, 4, 2, 0, 0, 0, R16.reverse_tables("bt2020", "limited", 12))
    out = (_Y(), _C().view(torch.int16), _C())
    s = rgb_to_ycc16(torch.zeros(2, 3, 8, 12, dtype=torch.uint8), layout="NCHW", interlaced=True, aligned="lsb", out=out)
    assert all(a is b for a, b in zip(s, out))
    assert calls.pop() == ("papof_rgb_to_ycc16_tensor", 2, 8, 12, 10, 0, 2, 0, 0, 1, R16.reverse_tables("bt709", "limited", 10)) and not calls


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
_FAKE = ctypes.create_string_buffer(1 << 20)
_OK = "ok"
U16 = capi.DTYPE_U16
_CS, _RS = (24, 6, 1, 0), (288, 36, 3, 1)  # the chroma planes and the NHWC frames of 8 x 12
FORWARD_TABLES, REVERSE_TABLES = R16.tables("bt709", "limited", 10, 255), R16.reverse_tables("bt709", "limited", 10)


def _ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def c_abi_forward16(lib, h, n=2, size=(8, 12), y=_OK, cb=_OK, cr=_OK, depth=10, shift=6, sub_v=2, sh=0, sv=0, interlaced=0,
                    tables=_OK, rgb=_OK):
    y, cb, cr = (_t(U16) if isinstance(y, str) else y, _t(U16, strides=_CS, data=0x2000) if isinstance(cb, str) else cb,
                 _t(U16, strides=_CS, data=0x3000) if isinstance(cr, str) else cr)
    rgb = _t(strides=_RS, data=0x9000) if isinstance(rgb, str) else rgb
    tables = _ints(FORWARD_TABLES if isinstance(tables, str) else tables)
    return lib.papof_ycc16_to_rgb_tensor(h, n, size[0], size[1], _ref(y), _ref(cb), _ref(cr), depth, shift, sub_v, sh, sv, interlaced,
                                         tables, _ref(rgb), None)


def c_abi_reverse16(lib, h, n=2, size=(8, 12), y=_OK, cb=_OK, cr=_OK, depth=10, shift=6, sub_v=2, sh=0, sv=0, interlaced=0,
                    tables=_OK, rgb=_OK):
    y, cb, cr = (_t(U16, data=0x9000) if isinstance(y, str) else y, _t(U16, strides=_CS, data=0xa000) if isinstance(cb, str) else cb,
                 _t(U16, strides=_CS, data=0xb000) if isinstance(cr, str) else cr)
    rgb = _t(strides=_RS) if isinstance(rgb, str) else rgb
    tables = _ints(REVERSE_TABLES if isinstance(tables, str) else tables)
    return lib.papof_rgb_to_ycc16_tensor(h, n, size[0], size[1], _ref(rgb), depth, shift, sub_v, sh, sv, interlaced, tables, _ref(y),
                                         _ref(cb), _ref(cr), None)


_SHARED_REFUSALS = [
    dict(depth=8), dict(depth=17), dict(depth=0), dict(depth=-20), dict(depth=40),                     # the depth
    dict(shift=7), dict(shift=-1), dict(shift=16), dict(depth=16, shift=1), dict(depth=12, shift=5),   # the shift: 0 .. 16 - depth
    dict(y=_t(capi.DTYPE_U8)), dict(cb=_t(capi.DTYPE_U8, strides=_CS)), dict(cr=_t(capi.DTYPE_F32, strides=_CS)),   # planes not U16
    dict(y=_t(4)), dict(rgb=_t(U16, strides=_RS)), dict(rgb=_t(-1, strides=_RS)),
    dict(y=None), dict(cb=None), dict(cr=None), dict(rgb=None), dict(tables=None),
    dict(y=_t(U16, data=0)), dict(rgb=_t(strides=_RS, data=0)),
    dict(y=_t(U16, strides=(96, -12, 1, 0))), dict(cr=_t(U16, strides=(24, 6, -1, 0))), dict(rgb=_t(strides=(288, 36, 3, -1))),
    dict(n=0), dict(size=(0, 12)), dict(size=(8, -12)), dict(sub_v=0), dict(sub_v=3), dict(sh=2), dict(sv=-1),
    dict(interlaced=1, size=(7, 12)), dict(interlaced=1, size=(2, 12)),
]
FORWARD_REFUSALS = _SHARED_REFUSALS + [
    dict(rgb=_t(strides=(0, 36, 3, 1))), dict(rgb=_t(strides=(288, 36, 3, 0))),                         # a written tensor
    dict(tables=_with(FORWARD_TABLES, 0, -1)), dict(tables=_with(FORWARD_TABLES, 0, 1024)),             # y_off: 0 .. P
    dict(tables=_with(FORWARD_TABLES, 6, 1023)),                                                         # a uint8 rgb needs peak 255
    dict(tables=_with(FORWARD_TABLES, 6, 0), rgb=_t(capi.DTYPE_F32, strides=_RS)),
    dict(tables=_with(FORWARD_TABLES, 6, 65536), rgb=_t(capi.DTYPE_F32, strides=_RS)),
] + [dict(tables=_with(FORWARD_TABLES, i, v)) for i in range(1, 6) for v in (-1, 1 << 18)]             # a coefficient: < 2^(d+8)
REVERSE_REFUSALS = _SHARED_REFUSALS + [
    dict(y=_t(U16, strides=(0, 12, 1, 0))), dict(cb=_t(U16, strides=(24, 0, 1, 0))), dict(cr=_t(U16, strides=(24, 6, 0, 0))),
    dict(tables=_with(REVERSE_TABLES, 0, -1)), dict(tables=_with(REVERSE_TABLES, 0, 1024)),
] + [dict(tables=_with(REVERSE_TABLES, i, v)) for i in range(1, 8) for v in (-1, (1 << 30) + 1)]


def test_c_abi_ycc16_to_rgb_refuses():
    h = ctypes.cast(_FAKE, ctypes.c_void_p)
    for kw in FORWARD_REFUSALS:
        assert c_abi_forward16(_lib(), h, **kw) == -1, kw
    assert c_abi_forward16(_lib(), None) == -1


def test_c_abi_rgb_to_ycc16_refuses():
    h = ctypes.cast(_FAKE, ctypes.c_void_p)
    for kw in REVERSE_REFUSALS:
        assert c_abi_reverse16(_lib(), h, **kw) == -1, kw
    assert c_abi_reverse16(_lib(), None) == -1


def test_the_8_bit_call_refuses_planes_of_words():
    from test_surface_cpu import c_abi_forward, c_abi_reverse
    h = ctypes.cast(_FAKE, ctypes.c_void_p)
    for kw in (dict(y=_t(U16)), dict(cb=_t(U16, strides=_CS)), dict(cr=_t(U16, strides=_CS)), dict(rgb=_t(U16, strides=_RS))):
        assert c_abi_forward(_lib(), h, **kw) == -1 and c_abi_reverse(_lib(), h, **kw) == -1, kw
    assert capi.DTYPE_U16 == 3 and "papof_ycc16_to_rgb_tensor" in capi.SYMBOLS and "papof_rgb_to_ycc16_tensor" in capi.SYMBOLS
    assert "papof_ycc16_to_rgb_fast" in capi.SYMBOLS


def test_c_abi_which_instance():
    """papof_ycc16_to_rgb_fast on descriptors alone: an aligned P010 surface of a width that is a multiple of 4 takes the 8-byte
    instance, and each condition that fails sends the call to the generic one.  Strides are in words, addresses in bytes."""
    lib = _lib()
    y = lambda **kw: _t(U16, **{**dict(strides=(3072, 256, 1, 0), data=0x10000), **kw})  # noqa: E731
    c = lambda off=0, **kw: _t(U16, **{**dict(strides=(3072, 256, 2, 0), data=0x10000 + 2 * 8 * 256 + off), **kw})  # noqa: E731
    nhwc, nchw = _t(strides=(8 * 36, 36, 3, 1), data=0x40000), _t(strides=(3 * 96, 12, 1, 96), data=0x40000)
    fast = lambda w=12, yy=None, cb=None, cr=None, rgb=nhwc: lib.papof_ycc16_to_rgb_fast(  # noqa: E731
        w, _ref(yy or y()), _ref(cb or c()), _ref(cr or c(2)), _ref(rgb))
    assert fast() == 1 and fast(rgb=nchw) == 1 and fast(cb=c(2), cr=c()) == 1  # P010 to NHWC and NCHW, Cr first
    f32 = lambda strides, data=0x40000: _t(capi.DTYPE_F32, strides=strides, data=data)  # noqa: E731
    assert fast(rgb=f32((288, 36, 3, 1))) == 1 and fast(rgb=f32((288, 12, 1, 96))) == 1
    assert fast(rgb=f32((288, 36, 3, 1), 0x40004)) == 0 and fast(rgb=_t(capi.DTYPE_F64, strides=(288, 36, 3, 1), data=0x40000)) == 0
    assert fast(w=10) == 0 and fast(w=11) == 0                                            # the width
    for off in (2, 4, 6):                                                                 # luma off its 8 bytes
        assert fast(yy=y(data=0x10000 + off)) == 0
    assert fast(yy=y(strides=(3072, 254, 1, 0))) == 0 and fast(yy=y(strides=(3074, 256, 1, 0))) == 0   # pitch, frame stride
    assert fast(yy=y(strides=(3072, 256, 2, 0))) == 0
    assert fast(cb=c(4), cr=c(6)) == 0 and fast(cb=c(2), cr=c(4)) == 0                    # the chroma pair off its 8 bytes
    assert fast(cb=c(), cr=c(4)) == 0 and fast(cb=c(), cr=c(0x1000)) == 0                 # not adjacent: planar
    assert fast(cb=c(), cr=c(1)) == 0                                                     # a byte beside, not a word
    assert fast(cb=c(strides=(3072, 256, 1, 0)), cr=c(2, strides=(3072, 256, 1, 0))) == 0
    assert fast(cr=c(2, strides=(3072, 512, 2, 0))) == 0 and fast(cb=c(strides=(3072, 258, 2, 0)), cr=c(2, strides=(3072, 258, 2, 0))) == 0
    assert fast(rgb=_t(strides=(8 * 36, 36, 3, 1), data=0x40001)) == 0 and fast(rgb=_t(strides=(3 * 98, 12, 1, 98), data=0x40000)) == 0
    assert lib.papof_ycc16_to_rgb_fast(12, None, _ref(c()), _ref(c(2)), _ref(nhwc)) == -1 and fast(w=0) == -1
    assert fast(yy=_t(capi.DTYPE_U8, strides=(3072, 256, 1, 0), data=0x10000)) == -1 and fast(rgb=_t(strides=(0, 36, 3, 1), data=0x40000)) == -1
