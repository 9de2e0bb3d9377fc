"""High-bit-depth decoder surfaces on device tensors (papteam_opticalflow_amd/tensors.py: ycc16_to_rgb, rgb_to_ycc16 ->
papof_ycc16_to_rgb_tensor, papof_rgb_to_ycc16_tensor).  The device's bytes must be the BYTES of the numpy restatement
(tests/_surface16_ref.py) for both calls: depth 10 in the high and in the low bits of its words, depth 12, depth 16; uint8,
float32 and float64 frames, NCHW and NHWC, every siting, interlaced, 4:2:0 and 4:2:2, 1, 2 and 5 frames; the edge shapes of
tests/test_gpu_surface.py; P010, P210, I010 and Y210 surfaces as views; a surface off its 8 bytes, where the 8-byte instance
must not be chosen, an aligned one where it must, and both instances on the same data; garbage in the bits around a sample;
outputs whose memory held two different patterns; rgb_to_ycc16(out=) into a P010 surface whose padding stays; the second
launch of the split grid; the caller's stream order; the C ABI's refusals on a live handle.

torch implements few operations for uint16 on the device: words are gathered, copied and compared as int16 views."""
import ctypes
import itertools

import numpy as np
import pytest

import _surface16_ref as R16
import _surface_ref as R
from test_gpu_surface import RULES, SHAPES
from test_surface16_cpu import (FORWARD_REFUSALS, FORWARD_TABLES, REVERSE_REFUSALS, REVERSE_TABLES, dirtied, random_words)
from test_surface_cpu import _image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (Surfaces, i010_planes, new_p010, p010_planes, rgb_to_ycc16, y210_planes,  # noqa: E402
                                             ycc16_to_rgb)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}
CFGS = [(10, "msb"), (10, "lsb"), (12, "msb"), (16, "msb")]  # (depth, aligned): shifts 6, 0, 4, 0
B709 = dict(matrix="bt709", range="limited")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()
    torch.cuda.empty_cache()


def _cfg(k):
    """the k-th case's (depth, aligned): every rule of RULES (8 of them, the fastest index) meets every one over six cases"""
    return CFGS[(k + k // len(RULES)) % len(CFGS)]


def _shift(d, aligned):
    return R16.shift_of(d, aligned)


def _words(T, H, W, sub_v, d, aligned, seed):
    return random_words(np.random.default_rng(seed), T, H, W, sub_v, d, _shift(d, aligned))


def _rgb(T, H, W, dtype, seed):
    """frames of all codes; floats reach beyond 0 .. 1 and hold NaNs and infinities"""
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    f = rng.uniform(-0.2, 1.2, (T, H, W, 3)).astype(_NP[dtype])
    flat = f.reshape(-1)
    idx = rng.integers(0, flat.size, max(3, flat.size // 50))
    flat[idx[0::3]], flat[idx[1::3]], flat[idx[2::3]] = np.nan, np.inf, -np.inf
    return f


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    """a device tensor of words (uint16 or int16) as a numpy array of uint16"""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _put(dst, src):
    dst.view(torch.int16).copy_(_cuda(src).view(torch.int16))


def _as_layout(a, layout):
    t = _cuda(a)
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t, layout):
    return (t if layout == "NHWC" else t.permute(0, 2, 3, 1)).cpu().numpy()


def _p010(ps, sub_v=2, order="uv", pitch=None, offset=0):
    """the planes on the device as views of one semi-planar surface of `pitch` WORDS per row that starts `offset` words into its
    buffer; the surface's other words are 0x5a5a"""
    T, H, W = ps[0].shape
    Hc = R.chroma_size(H, W, sub_v)[0]
    pitch = pitch or -(-W // 128) * 128
    buf = torch.full((T * (H + Hc) * pitch + offset,), 0x5a5a, dtype=torch.int16, device="cuda").view(torch.uint16)
    surface = buf[offset:].view(T, H + Hc, pitch)
    v = p010_planes(surface, H, order, width=W, sub_v=sub_v)
    for dst, src in zip(v, ps):
        _put(dst, src)
    return surface, v


def _fast(planes, out):
    """papof_ycc16_to_rgb_fast of the planes and an output tensor (NHWC, or NCHW when its second axis is 3 and its last is not)"""
    layout = "NHWC" if out.shape[-1] == 3 else "NCHW"
    d = [tensors._plane_struct16(p) for p in planes] + [tensors._struct(out, *tensors.descriptor(out, layout)[1:])]
    return capi.load().papof_ycc16_to_rgb_fast(int(planes[0].shape[2]), *(ctypes.byref(x) for x in d))


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = got != want
        at = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r for %r" % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


def _want(ps, d, aligned, rule, dtype, **kw):
    siting, inter, sub_v = rule
    tab = R16.tables(kw.get("matrix", "bt709"), kw.get("range", "limited"), d, 255 if dtype == torch.uint8 else None)
    return R16.ycc16_to_rgb_reference(*ps, tab, d, _shift(d, aligned), siting, inter, sub_v, dtype=_NP[dtype])


def _forward_case(ps, planes, cfg, rule, layout, dtype, what, want=None, **kw):
    siting, inter, sub_v = rule
    d, aligned = cfg
    want = _want(ps, d, aligned, rule, dtype, **kw) if want is None else want
    got = ycc16_to_rgb(*planes, depth=d, aligned=aligned, siting=siting, interlaced=inter, sub_v=sub_v, layout=layout, out_dtype=dtype,
                       **(kw or B709))
    assert got.dtype == dtype and got.is_contiguous()
    _same(_nhwc(got, layout), want, "%s %s %s %s %s" % (what, cfg, rule, layout, dtype))
    return got


# ---- both calls, every depth, dtype, layout, rule and frame count; planar tensors and P010 / P210 surfaces, a width that the
# 8-byte instance takes (72) and one that it does not (70)
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_ycc16_to_rgb_every_rule(dtype, layout):
    seen, met = set(), set()
    for k, ((H, W), T, rule) in enumerate(itertools.product(((38, 70), (38, 72)), (1, 2, 5), RULES)):
        cfg = _cfg(k)
        met.add((cfg, rule))
        ps = _words(T, H, W, rule[2], *cfg, T + W)
        want = _want(ps, *cfg, rule, dtype)
        planar = [_cuda(p) for p in ps]
        got = _forward_case(ps, planar, cfg, rule, layout, dtype, "planar %d x %d T %d" % (H, W, T), want)
        assert _fast(planar, got) == 0
        _, nv = _p010(ps, rule[2])
        again = _forward_case(ps, nv, cfg, rule, layout, dtype, "P010 %d x %d T %d" % (H, W, T), want)
        seen.add((W, _fast(nv, again)))
    assert seen == {(70, 0), (72, 0 if dtype == torch.float64 else 1)}
    assert met == set(itertools.product(CFGS, RULES))  # every rule at every depth and alignment
    for k, (matrix, rng) in enumerate(itertools.product(R.MATRICES, R.RANGES)):  # the tables reach the device
        cfg = CFGS[k % 4]
        ps = _words(2, 6, 8, 2, *cfg, 3)
        for planes in ([_cuda(p).view(torch.int16) for p in ps], _p010(ps)[1]):  # (int16 planes: the same bits)
            _forward_case(ps, planes, cfg, RULES[0], layout, dtype, "%s %s" % (matrix, rng), matrix=matrix, range=rng)


def _reverse_case(n, frames, cfg, rule, layout, what, **kw):
    siting, inter, sub_v = rule
    d, aligned = cfg
    s = _shift(d, aligned)
    want = R16.rgb_to_ycc16_reference(n, R16.reverse_tables(kw.get("matrix", "bt709"), kw.get("range", "limited"), d), d, s, siting, inter,
                                      sub_v)
    got = rgb_to_ycc16(frames, depth=d, aligned=aligned, siting=siting, interlaced=inter, sub_v=sub_v, layout=layout, **kw)
    assert isinstance(got, Surfaces)
    for name, g, w in zip(("y", "cb", "cr"), got, want):
        assert g.dtype == torch.uint16
        host = _host(g)
        _same(host, w, "%s %s %s %s %s" % (what, cfg, rule, layout, name))
        assert not (host & ~np.uint16(((1 << d) - 1) << s)).any()  # the bits around the level are 0
    return got


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_rgb_to_ycc16_every_rule(dtype, layout):
    for k, ((H, W), T, rule) in enumerate(itertools.product(((38, 70), (38, 72)), (1, 2, 5), RULES)):
        n = _rgb(T, H, W, dtype, T + W)
        _reverse_case(n, _as_layout(n, layout), _cfg(k), rule, layout, "%s %d x %d T %d" % (dtype, H, W, T))
    for k, (matrix, rng) in enumerate(itertools.product(R.MATRICES, R.RANGES)):
        n = _rgb(2, 6, 8, dtype, 4)
        _reverse_case(n, _as_layout(n, layout), CFGS[k % 4], RULES[0], layout, "%s %s" % (matrix, rng), matrix=matrix, range=rng)


# ---- the shapes that can go wrong
@pytest.mark.parametrize("H,W", SHAPES)
def test_edge_shapes(H, W):
    """tests/test_gpu_surface.py's shapes: 2 x 2 and its neighbours, odd sizes whose chroma is clamped, 6 x 6 interlaced, the
    seams of 64 lanes and of 64 lanes x 4 columns with widths that either forward instance takes; planar and P010 views"""
    rules = [r for r in RULES if not r[1] or (H % 2 == 0 and H >= 4)]
    for k, rule in enumerate(rules):
        T = (1, 2, 5)[(k + H + W) % 3]
        cfg = CFGS[(k + H + W) % 4]
        ps = _words(T, H, W, rule[2], *cfg, H + W + T)
        for layout, dtype in (("NHWC", torch.uint8), ("NCHW", torch.uint8), ("NCHW", torch.float32), ("NHWC", torch.float32),
                              ("NHWC", torch.float64)):
            want = _want(ps, *cfg, rule, dtype)
            _forward_case(ps, [_cuda(p) for p in ps], cfg, rule, layout, dtype, "planar %d x %d T %d" % (H, W, T), want)
            _forward_case(ps, _p010(ps, rule[2])[1], cfg, rule, layout, dtype, "P010 %d x %d T %d" % (H, W, T), want)
        for layout, dtype in (("NHWC", torch.uint8), ("NCHW", torch.float32), ("NCHW", torch.float64)):
            n = _rgb(T, H, W, dtype, H + W + T)
            got = _reverse_case(n, _as_layout(n, layout), cfg, rule, layout, "%d x %d T %d %s" % (H, W, T, dtype))
            surface, planes = _p010([np.zeros(tuple(p.shape), np.uint16) for p in got], rule[2])  # and written into a P010 view
            rgb_to_ycc16(_as_layout(n, layout), depth=cfg[0], aligned=cfg[1], siting=rule[0], interlaced=rule[1], sub_v=rule[2],
                         layout=layout, out=planes, **B709)
            for g, w in zip(planes, got):
                assert torch.equal(g.view(torch.int16), w.view(torch.int16)), (H, W, rule)
            assert bool((surface[:, :, W + W % 2:].view(torch.int16) == 0x5a5a).all())


def test_dense_1080p():
    """one frame of 1080 x 1920 through both calls and both forward instances: the committed frame coded to P010 by the
    restatement, decoded by the device from planar tensors and from a P010 surface; then coded by the device"""
    img = _image()[None]
    assert img.shape == (1, 1080, 1920, 3)
    cfg = (10, "msb")
    for rule in (RULES[0], RULES[4]):
        siting, inter, sub_v = rule
        ps = R16.rgb_to_ycc16_reference(img, R16.reverse_tables("bt709", "limited", 10), 10, 6, siting, inter, sub_v)
        want = _want(ps, *cfg, rule, torch.uint8)
        assert R.psnr(want, img) > 40.0
        nv = _p010(ps)[1]
        for planes, fast in (([_cuda(p) for p in ps], 0), (nv, 1)):
            got = _forward_case(ps, planes, cfg, rule, "NHWC", torch.uint8, "1080 x 1920 fast %d" % fast, want)
            assert _fast(planes, got) == fast
        got = _forward_case(ps, nv, cfg, rule, "NCHW", torch.float32, "1080 x 1920 float32")
        assert _fast(nv, got) == 1
        _reverse_case(img, _cuda(img), cfg, rule, "NHWC", "1080 x 1920")


# ---- surfaces as views
def test_surfaces_as_views():
    T, H, W = 2, 10, 24
    cfg, rule = (10, "msb"), RULES[0]
    ps = _words(T, H, W, 2, *cfg, 11)
    want = _want(ps, *cfg, rule, torch.float32)
    kw = dict(depth=10, **B709)
    surface, p010 = _p010(ps, pitch=W + 128)  # P010, a pitch of 256 bytes beyond the width
    assert p010.y.stride(1) == W + 128 and p010.cb.stride() == (15 * (W + 128), W + 128, 2)
    got = ycc16_to_rgb(*p010, **kw)
    assert _fast(p010, got) == 1
    _same(got.cpu().numpy(), want, "P010 with a pitch")
    _, vu = _p010(ps, order="vu")
    assert vu.cb.data_ptr() == vu.cr.data_ptr() + 2
    got = ycc16_to_rgb(*vu, **kw)
    assert _fast(vu, got) == 1
    _same(got.cpu().numpy(), want, "Cr first")
    # the same words read as "uv" swap the chroma planes
    _same(ycc16_to_rgb(*p010_planes(_p010(ps, order="vu")[0], H, width=W), **kw).cpu().numpy(),
          _want([ps[0], ps[2], ps[1]], *cfg, rule, torch.float32), "Cr first read as Cb first")
    lsb = _words(T, H, W, 2, 10, "lsb", 12)  # I010 / yuv420p10le: a planar surface of 15 rows of 24 words, as bytes
    flat = np.concatenate([p.reshape(T, -1) for p in lsb], 1)
    for surf in (_cuda(flat).view(T, H + H // 2, W), _cuda(flat.view(np.uint8)).view(T, H + H // 2, 2 * W)):
        planes = i010_planes(surf, H)
        assert planes.cb.stride(2) == 1 and planes.cb.stride(1) == W // 2
        got = ycc16_to_rgb(*planes, aligned="lsb", **kw)
        assert _fast(planes, got) == 0
        _same(got.cpu().numpy(), _want(lsb, 10, "lsb", rule, torch.float32), "I010")
    rule2 = (rule[0], False, 1)
    ps2 = _words(T, H, W, 1, *cfg, 13)  # 4:2:2: P210 and Y210
    want2 = _want(ps2, *cfg, rule2, torch.float32)
    p210 = _p010(ps2, sub_v=1)[1]
    got = ycc16_to_rgb(*p210, sub_v=1, **kw)
    assert _fast(p210, got) == 1
    _same(got.cpu().numpy(), want2, "P210")
    packed = np.empty((T, H, 2 * W), np.uint16)
    packed[:, :, 0::2], packed[:, :, 1::4], packed[:, :, 3::4] = ps2
    planes = y210_planes(_cuda(packed))
    got = ycc16_to_rgb(*planes, sub_v=1, **kw)
    assert _fast(planes, got) == 0
    _same(got.cpu().numpy(), want2, "Y210")
    back = torch.full((T, H, 2 * W), 0x5a5a, dtype=torch.int16, device="cuda")  # and written in place, every word of it
    n = _rgb(T, H, W, torch.float32, 14)
    rgb_to_ycc16(_cuda(n), sub_v=1, out=y210_planes(back), **kw)
    y, cb, cr = R16.rgb_to_ycc16_reference(n, REVERSE_TABLES, 10, 6, sub_v=1)
    host = _host(back)
    assert (host[:, :, 0::2] == y).all() and (host[:, :, 1::4] == cb).all() and (host[:, :, 3::4] == cr).all()


@pytest.mark.parametrize("layout,dtype", [("NHWC", torch.uint8), ("NCHW", torch.uint8), ("NHWC", torch.float32), ("NCHW", torch.float32)])
def test_both_instances_on_the_same_data(layout, dtype):
    """an aligned P010 surface takes the 8-byte instance; the same words 2 bytes further into their buffer, a luma view that
    starts at column 1 and a width that is no multiple of 4 must not; all return the restatement's bytes"""
    T, H, W = 3, 12, 520
    for k, rule in enumerate(RULES[:6]):
        siting, inter, sub_v = rule
        d, al = cfg = CFGS[k % 4]
        ps = _words(T, H, W, 2, *cfg, 21 + k)
        kw = dict(depth=d, aligned=al, siting=siting, interlaced=inter, layout=layout, out_dtype=dtype, **B709)
        want = _want(ps, *cfg, rule, dtype)
        aligned, off = _p010(ps)[1], _p010(ps, offset=1)[1]
        assert off.y.data_ptr() % 8 == 2 and aligned.y.data_ptr() % 8 == 0
        a, b = ycc16_to_rgb(*aligned, **kw), ycc16_to_rgb(*off, **kw)
        assert (_fast(aligned, a), _fast(off, b)) == (1, 0)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), rule
        _same(_nhwc(a, layout), want, "aligned %s" % (rule,))
        cut = Surfaces(aligned.y[:, :, 1:517], aligned.cb[:, :, :258], aligned.cr[:, :, :258])  # luma off its 8 bytes: columns 1 .. 516
        cps = (ps[0][:, :, 1:517], ps[1][:, :, :258], ps[2][:, :, :258])
        c = ycc16_to_rgb(*cut, **kw)
        assert _fast(cut, c) == 0
        _same(_nhwc(c, layout), _want(cps, *cfg, rule, dtype), "cut %s" % (rule,))
        narrow = Surfaces(aligned.y[:, :, :518], aligned.cb[:, :, :259], aligned.cr[:, :, :259])
        nps = (ps[0][:, :, :518], ps[1][:, :, :259], ps[2][:, :, :259])
        e = ycc16_to_rgb(*narrow, **kw)
        assert _fast(narrow, e) == 0
        _same(_nhwc(e, layout), _want(nps, *cfg, rule, dtype), "narrow %s" % (rule,))


def test_garbage_in_the_unused_bits_changes_nothing():
    """the low bits under shift 6 and the high bits under shift 0 at depth 10 (and the low four at depth 12): both instances"""
    T, H, W = 2, 10, 24
    for (d, al), dtype in itertools.product(CFGS[:3], (torch.uint8, torch.float32)):
        clean, dirty = dirtied(_words(T, H, W, 2, d, al, 25), d, _shift(d, al), 26)
        want = _want(clean, d, al, RULES[0], dtype)
        for planes, fast in (([_cuda(p) for p in dirty], 0), (_p010(dirty)[1], 1)):
            got = ycc16_to_rgb(*planes, depth=d, aligned=al, out_dtype=dtype, **B709)
            assert _fast(planes, got) == fast
            _same(got.cpu().numpy(), want, "garbage %d %s fast %d" % (d, al, fast))


# ---- outputs whose memory held two different patterns
def test_the_results_do_not_depend_on_what_the_outputs_held():
    T, H, W, guard = 2, 10, 24, 64
    ps = _words(T, H, W, 2, 10, "msb", 31)
    want = _want(ps, 10, "msb", RULES[0], torch.uint8)
    tables = (ctypes.c_int * 7)(*FORWARD_TABLES)
    for planes, fast in (([_cuda(p) for p in ps], 0), (_p010(ps)[1], 1)):
        d = [tensors._plane_struct16(p) for p in planes]
        buf = torch.empty(want.size + 2 * guard, dtype=torch.uint8, device="cuda")
        out = buf[guard:guard + want.size].view(T, H, W, 3)
        assert _fast(planes, out) == fast
        d_out = tensors._struct(out, *tensors.descriptor(out, "NHWC")[1:])
        for pattern in (0x5a, 0xff):
            buf.fill_(pattern)
            tensors._launch(out.device, "papof_ycc16_to_rgb_tensor", T, H, W, ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]),
                            10, 6, 2, 0, 0, 0, tables, ctypes.byref(d_out))
            got = buf.cpu().numpy()
            assert got[guard:-guard].tobytes() == want.tobytes(), (fast, hex(pattern))
            assert (got[:guard] == pattern).all() and (got[-guard:] == pattern).all()  # nothing beyond the frames
    n = _rgb(T, H, W, torch.uint8, 32)
    planes = R16.rgb_to_ycc16_reference(n, REVERSE_TABLES, 10, 6)
    for pattern in (0x5a5a, -1):
        out = [torch.full(p.shape, pattern, dtype=torch.int16, device="cuda") for p in planes]
        rgb_to_ycc16(_cuda(n), out=out, **B709)
        for g, w in zip(out, planes):
            _same(_host(g), w, hex(pattern & 0xffff))


def test_rgb_to_ycc16_into_a_p010_surface_leaves_the_padding():
    T, H, W = 2, 9, 70  # odd height: 5 chroma rows; 70 of 128 words per row in use
    surface, planes = new_p010(T, H, W, "cuda")
    assert tuple(surface.shape) == (T, 14, 128)
    surface.view(torch.int16).fill_(0x5a5a)
    n = _rgb(T, H, W, torch.float32, 41)
    got = rgb_to_ycc16(_cuda(n), out=planes, **B709)
    assert all(a is b for a, b in zip(got, planes))
    y, cb, cr = R16.rgb_to_ycc16_reference(n, REVERSE_TABLES, 10, 6)
    host = _host(surface)
    assert (host[:, :H, :W] == y).all() and (host[:, H:, 0:W:2] == cb).all() and (host[:, H:, 1:W:2] == cr).all()
    assert (host[:, :, W:] == 0x5a5a).all()
    # and back through the same views
    _same(ycc16_to_rgb(*planes, **B709).cpu().numpy(), _want((y, cb, cr), 10, "msb", RULES[0], torch.float32), "the surface read back")


# ---- the second launch of the split grid: launch_tiles cuts the frames at 65535 (gridDim.y)
def test_every_frame_of_both_launches():
    """65535 + 2 frames of 2 x 4, periodic with period 7 (65535 mod 7 = 1: the first frame of the second launch is not frame
    0), every frame with memory of its own (an index gather, not a stride-0 view); both forward instances and the reverse"""
    P, cut = 7, 65535
    N = cut + 2
    assert cut % P != 0
    ps = _words(P, 2, 4, 2, 10, "msb", 51)
    want = _want(ps, 10, "msb", RULES[0], torch.uint8)
    assert all((want[i] != want[0]).any() for i in range(1, P))  # no base frame passes for frame 0
    idx = torch.from_numpy(np.arange(N, dtype=np.int64) % P).cuda()
    expect = _cuda(want).index_select(0, idx)

    def check(got, expect, what):
        assert got.shape == expect.shape and got.dtype == expect.dtype
        if not torch.equal(got, expect):
            bad = (got != expect).reshape(N, -1).any(1).nonzero().reshape(-1)
            raise AssertionError("%s: %d of %d frames differ, the first is frame %d; %d of them before the cut at %d" % (
                what, bad.numel(), N, int(bad[0]), int((bad < cut).sum()), cut))

    planar = [_cuda(p).view(torch.int16).index_select(0, idx) for p in ps]
    kw = dict(depth=10, out_dtype=torch.uint8, **B709)
    got = ycc16_to_rgb(*planar, **kw)
    assert _fast(planar, got) == 0
    check(got, expect, "generic")
    surface = torch.cat([planar[0], torch.stack(planar[1:], -1).reshape(N, 1, 4)], 1)  # P010 at a pitch of 4 words: (N, 3, 4)
    nv = p010_planes(surface, 2)
    got = ycc16_to_rgb(*nv, **kw)
    assert _fast(nv, got) == 1
    check(got, expect, "8 bytes")
    n = _rgb(P, 2, 4, torch.uint8, 52)
    back = rgb_to_ycc16(_cuda(n).index_select(0, idx), **B709)
    for g, w in zip(back, R16.rgb_to_ycc16_reference(n, REVERSE_TABLES, 10, 6)):
        check(g.view(torch.int16), _cuda(w).view(torch.int16).index_select(0, idx), "reverse")


# ---- the caller's stream
def test_the_calls_are_ordered_on_the_callers_stream():
    """Planes written on a side stream behind a long sleep, converted and converted back under that stream with no
    synchronisation: the kernels must read them after they are written, and what is queued behind them must see their output"""
    import time
    T, H, W = 2, 40, 136
    ps = _words(T, H, W, 2, 10, "msb", 61)
    want = _want(ps, 10, "msb", RULES[0], torch.float32)
    want_back = R16.rgb_to_ycc16_reference(want, REVERSE_TABLES, 10, 6)
    src = _p010(ps)[0].view(torch.int16)
    dst = torch.zeros_like(src)
    planes = p010_planes(dst, H, width=W)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = ycc16_to_rgb(*planes, **B709)
        rgb_to_ycc16(warm, **B709)
    torch.cuda.synchronize()
    assert warm.cpu().numpy().tobytes() != want.tobytes()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock: the shortest of three windows
        windows = []
        for _ in range(3):
            t0 = time.perf_counter()
            torch.cuda._sleep(50_000_000)
            side.synchronize()
            windows.append(time.perf_counter() - t0)
        per_cycle = min(windows) / 50_000_000
    before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        before.record()
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        after.record()
        dst.copy_(src)
        got = ycc16_to_rgb(*planes, **B709)
        back = rgb_to_ycc16(got, **B709)
        copy = [p.view(torch.int16).clone() for p in back]  # queued behind the kernels on the same stream
    side.synchronize()
    assert before.elapsed_time(after) > 150.0, "the sleep in front of the planes took %.1f ms" % before.elapsed_time(after)
    _same(got.cpu().numpy(), want, "side stream")
    for g, w in zip(copy, want_back):
        _same(_host(g), w, "side stream, back")


# ---- the C ABI's refusals on a live handle: nothing is enqueued and the outputs are untouched
def _live(desc, t):
    """the CPU test's descriptor with the live tensor behind its stand-in address"""
    if desc is None:
        return None
    d = tensors._struct(t, tuple(desc.stride), desc.dtype)
    d.data = t.data_ptr() if desc.data else None
    return d


def test_c_abi_refusals_leave_the_outputs_untouched(gpu):
    T, H, W = 2, 8, 12
    words = _words(T, H, W, 2, 10, "msb", 71)
    ps = [_cuda(p) for p in words]
    rgb = torch.full((T, H, W, 3), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = [tensors._plane_struct16(p) for p in ps] + [tensors._struct(rgb, *tensors.descriptor(rgb, "NHWC")[1:])]
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

    def call(reverse, n=T, size=(H, W), y="ok", cb="ok", cr="ok", depth=10, shift=6, sub_v=2, sh=0, sv=0, interlaced=0, tables="ok",
             rgb_="ok", h="ok"):
        d = [ok[i] if isinstance(v, str) else _live(v, t) for i, (v, t) in enumerate(zip((y, cb, cr, rgb_), ps + [rgb]))]
        default = REVERSE_TABLES if reverse else FORWARD_TABLES
        tab = None if tables is None else (ctypes.c_int * len(default))(*(default if isinstance(tables, str) else tables))
        hh = gpu.h if h == "ok" else h
        if reverse:
            return gpu.L.papof_rgb_to_ycc16_tensor(hh, n, size[0], size[1], ref(d[3]), depth, shift, sub_v, sh, sv, interlaced, tab,
                                                   ref(d[0]), ref(d[1]), ref(d[2]), None)
        return gpu.L.papof_ycc16_to_rgb_tensor(hh, n, size[0], size[1], ref(d[0]), ref(d[1]), ref(d[2]), depth, shift, sub_v, sh, sv,
                                               interlaced, tab, ref(d[3]), None)

    before = [p.view(torch.int16).clone() for p in ps]
    with_ = lambda tab, i, v: tab[:i] + [v] + tab[i + 1:]  # noqa: E731
    named = [dict(depth=8), dict(depth=17), dict(shift=7), dict(tables=with_(FORWARD_TABLES, 1, 1 << 18)),   # a coefficient of 2^(d+8)
             dict(tables=with_(FORWARD_TABLES, 6, 1023))]                                                     # peak 1023 with a uint8 rgb
    u8 = [torch.zeros(tuple(p.shape), dtype=torch.uint8, device="cuda") for p in ps]
    for kw in named:
        assert call(False, **kw) == -1, kw
    for i in range(3):  # uint8 planes
        d = list(ok)
        d[i] = tensors._plane_struct(u8[i])
        tab = (ctypes.c_int * 7)(*FORWARD_TABLES)
        assert gpu.L.papof_ycc16_to_rgb_tensor(gpu.h, T, H, W, ref(d[0]), ref(d[1]), ref(d[2]), 10, 6, 2, 0, 0, 0, tab, ref(d[3]), None) == -1
    for reverse, refusals in ((False, FORWARD_REFUSALS), (True, REVERSE_REFUSALS)):
        for kw in refusals:
            kw = {("rgb_" if k == "rgb" else k): v for k, v in kw.items()}
            assert call(reverse, **kw) == -1, (reverse, kw)
        assert call(reverse, h=None) == -1
    # a descriptor of words handed to the 8-bit call and to a video call is refused
    tab8 = (ctypes.c_int * 6)(*R.tables("bt709", "limited"))
    assert gpu.L.papof_ycc_to_rgb_tensor(gpu.h, T, H, W, ref(ok[0]), ref(ok[1]), ref(ok[2]), 2, 0, 0, 0, tab8, ref(ok[3]), None) == -1
    frames = torch.zeros((T, H, W, 3), dtype=torch.int16, device="cuda")
    d_in = tensors._struct(frames, tuple(frames.stride()), capi.DTYPE_U16)
    mats = torch.eye(3, dtype=torch.float64, device="cuda")[:2].expand(T, 2, 3).contiguous()
    d_mat = tensors._struct(mats, (6, 3, 1, 0), capi.DTYPE_F64)
    valid = torch.full((T, H, W), 0x5a, dtype=torch.uint8, device="cuda")
    d_valid = tensors._struct(valid, (H * W, W, 1, 1), capi.DTYPE_U8)
    assert gpu.L.papof_warp_affine_tensor(gpu.h, T, H, W, 3, ref(d_in), ref(d_mat), ref(ok[3]), ref(d_valid), None) == -1
    d_ok_in = tensors._struct(rgb, *tensors.descriptor(rgb, "NHWC")[1:])
    d_out16 = tensors._struct(frames, tuple(frames.stride()), capi.DTYPE_U16)
    assert gpu.L.papof_warp_affine_tensor(gpu.h, T, H, W, 3, ref(d_ok_in), ref(d_mat), ref(d_out16), ref(d_valid), None) == -1
    torch.cuda.synchronize()
    assert bool((rgb == 0x5a).all()) and bool((valid == 0x5a).all()) and not bool(frames.any())
    assert all(torch.equal(a.view(torch.int16), b) for a, b in zip(ps, before))
    assert call(False) == 0  # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    assert rgb.cpu().numpy().tobytes() == _want(words, 10, "msb", RULES[0], torch.uint8).tobytes()
    host = rgb.cpu().numpy()
    assert call(True) == 0
    torch.cuda.synchronize()
    for g, w in zip(ps, R16.rgb_to_ycc16_reference(host, REVERSE_TABLES, 10, 6)):
        assert _host(g).tobytes() == w.tobytes()
