"""Decoder surfaces on device tensors (papteam_opticalflow_amd/tensors.py: ycc_to_rgb, rgb_to_ycc -> papof_ycc_to_rgb_tensor,
papof_rgb_to_ycc_tensor).  The device's bytes must be the BYTES of the numpy restatement (tests/_surface_ref.py) for both calls:
uint8, float32 and float64 frames, NCHW and NHWC, every siting, interlaced, 4:2:0 and 4:2:2, 1, 2 and 5 frames; the shapes at
which the code can go wrong (2 x 2 up to one dense 1080p frame, odd sizes whose chroma is clamped, a bottom field with one
chroma row, the seams of a wave of 64 lanes and of 64 lanes x 4 columns); surfaces as views (NV12 with a pitch, NV21, NV16,
I420, YV12, YUY2, UYVY), a surface at an odd byte offset, where the dword instance must not be chosen, an aligned one where
it must, and both instances on the same data; outputs whose memory held two different patterns; rgb_to_ycc(out=) into an NV12
surface whose padding stays; the second launch of the split grid; the caller's stream order; the C ABI's refusals on a
live handle."""
import ctypes
import itertools

import numpy as np
import pytest

import _surface_ref as R
from test_surface_cpu import FORWARD_REFUSALS, FORWARD_TABLES, REVERSE_REFUSALS, REVERSE_TABLES, _image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (Surfaces, i420_planes, new_nv12, nv12_planes, packed422_planes, rgb_to_ycc,  # noqa: E402
                                             ycc_to_rgb)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}
# (siting, interlaced, sub_v): every vertical rule with both horizontal ones
RULES = [(s, False, 2) for s in R.SITINGS] + [(("left", "center"), True, 2), (("center", "top"), True, 2),
                                               (("left", "center"), False, 1), (("center", "center"), True, 1)]
B709 = dict(matrix="bt709", range="limited")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()
    torch.cuda.empty_cache()


def _planes(T, H, W, sub_v, seed):
    """random bytes of all codes with the extremes planted, different from frame to frame"""
    rng = np.random.default_rng(seed)
    Hc, Wc = R.chroma_size(H, W, sub_v)
    ps = [rng.integers(0, 256, s).astype(np.uint8) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc))]
    for p in ps:
        p.reshape(-1)[:2] = (0, 255)[:p.size]
    return ps


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


def _as_layout(a, layout):
    t = _cuda(a)
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t, layout):
    return (t if layout == "NHWC" else t.permute(0, 2, 3, 1)).cpu().numpy()


def _nv(ps, sub_v=2, order="uv", pitch=None, offset=0):
    """the planes on the device as views of one semi-planar surface of `pitch` bytes per row that starts `offset` bytes into its
    buffer; the surface's other bytes are 0x5a"""
    T, H, W = ps[0].shape
    Hc = R.chroma_size(H, W, sub_v)[0]
    pitch = pitch or -(-W // 256) * 256
    buf = torch.full((T * (H + Hc) * pitch + offset,), 0x5a, dtype=torch.uint8, device="cuda")
    surface = buf[offset:].view(T, H + Hc, pitch)
    v = nv12_planes(surface, H, order, width=W, sub_v=sub_v)
    for dst, src in zip(v, ps):
        dst.copy_(_cuda(src))
    return surface, v


def _fast(planes, out):
    """papof_ycc_to_rgb_fast of the planes and an output tensor (NHWC, or NCHW when its second axis is 3 and its last is not)"""
    layout = "NHWC" if out.shape[-1] == 3 else "NCHW"
    d = [tensors._plane_struct(p) for p in planes] + [tensors._struct(out, *tensors.descriptor(out, layout)[1:])]
    return capi.load().papof_ycc_to_rgb_fast(int(planes[0].shape[2]), *(ctypes.byref(x) for x in d))


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    if got.tobytes() != want.tobytes():
        bad = got != want
        at = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r for %r" % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


def _forward_case(ps, planes, rule, layout, dtype, what):
    siting, inter, sub_v = rule
    want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES, siting, inter, sub_v, dtype=_NP[dtype])
    got = ycc_to_rgb(*planes, siting=siting, interlaced=inter, sub_v=sub_v, layout=layout, out_dtype=dtype, **B709)
    assert got.dtype == dtype and got.is_contiguous()
    _same(_nhwc(got, layout), want, "%s %s %s %s" % (what, rule, layout, dtype))
    return got


# ---- both calls, every dtype, layout, rule and frame count; planar tensors and NV12 / NV16 surfaces, a width that the dword
# instance takes (72) and one that it does not (70)
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_ycc_to_rgb_every_rule(dtype, layout):
    seen = set()
    for (H, W), T, rule in itertools.product(((38, 70), (38, 72)), (1, 2, 5), RULES):
        ps = _planes(T, H, W, rule[2], T + W)
        planar = [_cuda(p) for p in ps]
        got = _forward_case(ps, planar, rule, layout, dtype, "planar %d x %d T %d" % (H, W, T))
        assert _fast(planar, got) == 0
        _, nv = _nv(ps, rule[2])
        again = _forward_case(ps, nv, rule, layout, dtype, "NV %d x %d T %d" % (H, W, T))
        seen.add((W, _fast(nv, again)))
    assert seen == {(70, 0), (72, 0 if dtype == torch.float64 else 1)}
    for matrix, rng in itertools.product(R.MATRICES, R.RANGES):  # the tables reach the device
        ps = _planes(2, 6, 8, 2, 3)
        for planes in ([_cuda(p) for p in ps], _nv(ps)[1]):
            got = ycc_to_rgb(*planes, matrix=matrix, range=rng, layout=layout, out_dtype=dtype)
            _same(_nhwc(got, layout), R.ycc_to_rgb_reference(*ps, R.tables(matrix, rng), dtype=_NP[dtype]), "%s %s" % (matrix, rng))


def _reverse_case(n, frames, rule, layout, what, **kw):
    siting, inter, sub_v = rule
    want = R.rgb_to_ycc_reference(n, R.reverse_tables(kw.get("matrix", "bt709"), kw.get("range", "limited")), siting, inter, sub_v)
    got = rgb_to_ycc(frames, siting=siting, interlaced=inter, sub_v=sub_v, layout=layout, **kw)
    assert isinstance(got, Surfaces)
    for name, g, w in zip(("y", "cb", "cr"), got, want):
        assert g.dtype == torch.uint8
        _same(g.cpu().numpy(), w, "%s %s %s %s" % (what, rule, layout, name))
    return got


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_rgb_to_ycc_every_rule(dtype, layout):
    for (H, W), T, rule in itertools.product(((38, 70), (38, 72)), (1, 2, 5), RULES):
        n = _rgb(T, H, W, dtype, T + W)
        _reverse_case(n, _as_layout(n, layout), rule, layout, "%s %d x %d T %d" % (dtype, H, W, T))
    for matrix, rng in itertools.product(R.MATRICES, R.RANGES):
        n = _rgb(2, 6, 8, dtype, 4)
        _reverse_case(n, _as_layout(n, layout), RULES[0], layout, "%s %s" % (matrix, rng), matrix=matrix, range=rng)


# ---- the shapes that can go wrong
SHAPES = [(2, 2), (4, 2), (2, 4), (3, 5), (5, 3), (6, 6), (1, 1), (4, 254), (4, 256), (4, 258), (4, 260), (8, 514), (8, 516), (38, 70)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_edge_shapes(H, W):
    """2 x 2 and its neighbours, odd sizes whose chroma is clamped, 6 x 6 interlaced (the bottom field has one chroma row), the
    seams of 64 lanes and of 64 lanes x 4 columns with widths that either forward instance takes"""
    rules = [r for r in RULES if not r[1] or (H % 2 == 0 and H >= 4)]
    assert (H, W) != (6, 6) or any(r[1] and r[2] == 2 for r in rules)
    for k, rule in enumerate(rules):
        T = (1, 2, 5)[(k + H + W) % 3]  # (every rule at every T: test_ycc_to_rgb_every_rule, test_rgb_to_ycc_every_rule)
        ps = _planes(T, H, W, rule[2], H + W + T)
        for layout, dtype in (("NHWC", torch.uint8), ("NCHW", torch.uint8), ("NCHW", torch.float32), ("NHWC", torch.float64)):
            _forward_case(ps, [_cuda(p) for p in ps], rule, layout, dtype, "planar %d x %d T %d" % (H, W, T))
            _forward_case(ps, _nv(ps, rule[2])[1], rule, layout, dtype, "NV %d x %d T %d" % (H, W, T))
        for layout, dtype in (("NHWC", torch.uint8), ("NCHW", torch.float32), ("NCHW", torch.float64)):
            n = _rgb(T, H, W, dtype, H + W + T)
            _reverse_case(n, _as_layout(n, layout), rule, layout, "%d x %d T %d %s" % (H, W, T, dtype))


def test_dense_1080p():
    """one frame of 1080 x 1920 through both calls and both forward instances: the committed frame coded by the restatement,
    decoded by the device from planar tensors and from an NV12 surface; then coded by the device"""
    img = _image()[None]
    assert img.shape == (1, 1080, 1920, 3)
    for rule in (RULES[0], RULES[4]):
        siting, inter, sub_v = rule
        ps = R.rgb_to_ycc_reference(img, REVERSE_TABLES, siting, inter, sub_v)
        want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES, siting, inter, sub_v)
        assert R.psnr(want, img) > 40.0
        nv = _nv(ps)[1]
        for planes, fast in (([_cuda(p) for p in ps], 0), (nv, 1)):
            got = ycc_to_rgb(*planes, siting=siting, interlaced=inter, **B709)
            assert _fast(planes, got) == fast
            _same(got.cpu().numpy(), want, "1080 x 1920 %s fast %d" % (rule, fast))
        _reverse_case(img, _cuda(img), rule, "NHWC", "1080 x 1920")


# ---- surfaces as views
def test_surfaces_as_views():
    T, H, W = 2, 10, 24
    ps = _planes(T, H, W, 2, 11)
    want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES)
    surface, nv12 = _nv(ps, pitch=W + 256)  # NV12, a pitch of 256 beyond the width
    assert nv12.y.stride(1) == W + 256 and nv12.cb.stride() == (15 * (W + 256), W + 256, 2)
    got = ycc_to_rgb(*nv12, **B709)
    assert _fast(nv12, got) == 1
    _same(got.cpu().numpy(), want, "NV12 with a pitch")
    _, nv21 = _nv(ps, order="vu")
    assert nv21.cb.data_ptr() == nv21.cr.data_ptr() + 1
    got = ycc_to_rgb(*nv21, **B709)
    assert _fast(nv21, got) == 1
    _same(got.cpu().numpy(), want, "NV21")
    # the same bytes read as NV12 swap the chroma planes
    _same(ycc_to_rgb(*nv12_planes(_nv(ps, order="vu")[0], H, width=W), **B709).cpu().numpy(),
          R.ycc_to_rgb_reference(ps[0], ps[2], ps[1], FORWARD_TABLES), "NV21 read as NV12")
    for order in ("uv", "vu"):  # I420 and YV12: a planar surface of 16 rows of 24 bytes
        flat = np.concatenate([ps[0].reshape(T, -1)] + [p.reshape(T, -1) for p in (ps[1:] if order == "uv" else ps[:0:-1])], 1)
        planes = i420_planes(_cuda(flat).view(T, H + H // 2, W), H, order)
        assert planes.cb.stride(2) == 1 and planes.cb.stride(1) == W // 2
        got = ycc_to_rgb(*planes, **B709)
        assert _fast(planes, got) == 0
        _same(got.cpu().numpy(), want, "I420" if order == "uv" else "YV12")
    ps2 = _planes(T, H, W, 1, 12)  # 4:2:2: NV16, YUY2 and UYVY
    want2 = R.ycc_to_rgb_reference(*ps2, FORWARD_TABLES, sub_v=1)
    nv16 = _nv(ps2, sub_v=1)[1]
    got = ycc_to_rgb(*nv16, sub_v=1, **B709)
    assert _fast(nv16, got) == 1
    _same(got.cpu().numpy(), want2, "NV16")
    for order, (oy, ou, ov) in (("yuyv", (0, 1, 3)), ("uyvy", (1, 0, 2))):
        packed = np.empty((T, H, 2 * W), np.uint8)
        packed[:, :, oy::2], packed[:, :, ou::4], packed[:, :, ov::4] = ps2
        planes = packed422_planes(_cuda(packed), order)
        got = ycc_to_rgb(*planes, sub_v=1, **B709)
        assert _fast(planes, got) == 0
        _same(got.cpu().numpy(), want2, order)
        back = torch.full((T, H, 2 * W), 0x5a, dtype=torch.uint8, device="cuda")  # and written in place, every byte of it
        n = _rgb(T, H, W, torch.uint8, 13)
        rgb_to_ycc(_cuda(n), sub_v=1, out=packed422_planes(back, order), **B709)
        y, cb, cr = R.rgb_to_ycc_reference(n, REVERSE_TABLES, sub_v=1)
        host = back.cpu().numpy()
        assert (host[:, :, oy::2] == y).all() and (host[:, :, ou::4] == cb).all() and (host[:, :, ov::4] == cr).all(), order


@pytest.mark.parametrize("layout,dtype", [("NHWC", torch.uint8), ("NCHW", torch.uint8), ("NHWC", torch.float32), ("NCHW", torch.float32)])
def test_both_instances_on_the_same_data(layout, dtype):
    """an aligned NV12 surface takes the dword instance; the same bytes one byte further into their buffer, a luma view that
    starts at column 1 and a width that is no multiple of 4 must not; all return the restatement's bytes"""
    T, H, W = 3, 12, 520
    ps = _planes(T, H, W, 2, 21)
    for rule in RULES[:6]:
        siting, inter, sub_v = rule
        kw = dict(siting=siting, interlaced=inter, layout=layout, out_dtype=dtype, **B709)
        want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES, siting, inter, dtype=_NP[dtype])
        aligned, odd = _nv(ps)[1], _nv(ps, offset=1)[1]
        assert odd.y.data_ptr() % 2 == 1 and aligned.y.data_ptr() % 4 == 0
        a, b = ycc_to_rgb(*aligned, **kw), ycc_to_rgb(*odd, **kw)
        assert (_fast(aligned, a), _fast(odd, b)) == (1, 0)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), rule
        _same(_nhwc(a, layout), want, "aligned %s" % (rule,))
        cut = Surfaces(aligned.y[:, :, 1:517], aligned.cb[:, :, :258], aligned.cr[:, :, :258])  # luma off a dword: columns 1 .. 516
        cps = (ps[0][:, :, 1:517], ps[1][:, :, :258], ps[2][:, :, :258])
        c = ycc_to_rgb(*cut, **kw)
        assert _fast(cut, c) == 0
        _same(_nhwc(c, layout), R.ycc_to_rgb_reference(*cps, FORWARD_TABLES, siting, inter, dtype=_NP[dtype]), "cut %s" % (rule,))
        narrow = Surfaces(aligned.y[:, :, :518], aligned.cb[:, :, :259], aligned.cr[:, :, :259])
        assert _fast(narrow, ycc_to_rgb(*narrow, **kw)) == 0


# ---- outputs whose memory held two different patterns
def test_the_results_do_not_depend_on_what_the_outputs_held():
    T, H, W, guard = 2, 10, 24, 64
    ps = _planes(T, H, W, 2, 31)
    want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES)
    tables = (ctypes.c_int * 6)(*FORWARD_TABLES)
    for planes, fast in (([_cuda(p) for p in ps], 0), (_nv(ps)[1], 1)):
        d = [tensors._plane_struct(p) for p in planes]
        buf = torch.empty(want.size + 2 * guard, dtype=torch.uint8, device="cuda")
        out = buf[guard:guard + want.size].view(T, H, W, 3)
        assert _fast(planes, out) == fast
        d_out = tensors._struct(out, *tensors.descriptor(out, "NHWC")[1:])
        for pattern in (0x5a, 0xff):
            buf.fill_(pattern)
            tensors._launch(out.device, "papof_ycc_to_rgb_tensor", T, H, W, ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]),
                            2, 0, 0, 0, tables, ctypes.byref(d_out))
            got = buf.cpu().numpy()
            assert got[guard:-guard].tobytes() == want.tobytes(), (fast, hex(pattern))
            assert (got[:guard] == pattern).all() and (got[-guard:] == pattern).all()  # nothing beyond the frames
    n = _rgb(T, H, W, torch.uint8, 32)
    y, cb, cr = R.rgb_to_ycc_reference(n, REVERSE_TABLES)
    for pattern in (0x5a, 0xff):
        out = [torch.full(p.shape, pattern, dtype=torch.uint8, device="cuda") for p in (y, cb, cr)]
        rgb_to_ycc(_cuda(n), out=out, **B709)
        for g, w in zip(out, (y, cb, cr)):
            _same(g.cpu().numpy(), w, hex(pattern))


def test_rgb_to_ycc_into_an_nv12_surface_leaves_the_padding():
    T, H, W = 2, 9, 70  # odd height: 5 chroma rows; 70 of 256 bytes per row in use
    surface, planes = new_nv12(T, H, W, "cuda")
    assert tuple(surface.shape) == (T, 14, 256)
    surface.fill_(0x5a)
    n = _rgb(T, H, W, torch.float32, 41)
    got = rgb_to_ycc(_cuda(n), out=planes, **B709)
    assert all(a is b for a, b in zip(got, planes))
    y, cb, cr = R.rgb_to_ycc_reference(n, REVERSE_TABLES)
    host = surface.cpu().numpy()
    assert (host[:, :H, :W] == y).all() and (host[:, H:, 0:W:2] == cb).all() and (host[:, H:, 1:W:2] == cr).all()
    assert (host[:, :, W:] == 0x5a).all()
    # and back through the same views
    _same(ycc_to_rgb(*planes, **B709).cpu().numpy(), R.ycc_to_rgb_reference(y, cb, cr, FORWARD_TABLES), "the surface read back")


# ---- the second launch of the split grid: launch_tiles cuts the frames at 65535 (gridDim.y)
def test_every_frame_of_both_launches():
    """65535 + 2 frames of 2 x 4, periodic with period 7 (65535 mod 7 = 1: the first frame of the second launch is not frame
    0), every frame with memory of its own (an index gather, not a stride-0 view); both forward instances and the reverse"""
    P, cut = 7, 65535
    N = cut + 2
    assert cut % P != 0
    ps = _planes(P, 2, 4, 2, 51)
    want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES)
    assert all((want[i] != want[0]).any() for i in range(1, P))  # no base frame passes for frame 0
    idx = torch.from_numpy(np.arange(N, dtype=np.int64) % P).cuda()
    expect = _cuda(want).index_select(0, idx)

    def check(got, expect, what):
        assert got.shape == expect.shape and got.dtype == expect.dtype
        if not torch.equal(got, expect):
            bad = (got != expect).reshape(N, -1).any(1).nonzero().reshape(-1)
            raise AssertionError("%s: %d of %d frames differ, the first is frame %d; %d of them before the cut at %d" % (
                what, bad.numel(), N, int(bad[0]), int((bad < cut).sum()), cut))

    planar = [_cuda(p).index_select(0, idx) for p in ps]
    got = ycc_to_rgb(*planar, **B709)
    assert _fast(planar, got) == 0
    check(got, expect, "generic")
    surface = torch.cat([planar[0], torch.stack(planar[1:], -1).reshape(N, 1, 4)], 1)  # NV12 at a pitch of 4: (N, 3, 4)
    nv = nv12_planes(surface, 2)
    got = ycc_to_rgb(*nv, **B709)
    assert _fast(nv, got) == 1
    check(got, expect, "dwords")
    n = _rgb(P, 2, 4, torch.uint8, 52)
    back = rgb_to_ycc(_cuda(n).index_select(0, idx), **B709)
    for g, w in zip(back, R.rgb_to_ycc_reference(n, REVERSE_TABLES)):
        check(g, _cuda(w).index_select(0, idx), "reverse")


# ---- the caller's stream
def test_the_calls_are_ordered_on_the_callers_stream():
    """Planes written on a side stream behind a long sleep, converted and converted back under that stream with no
    synchronisation: the kernels must read them after they are written, and what is queued behind them must see their output"""
    import time
    T, H, W = 2, 40, 136
    ps = _planes(T, H, W, 2, 61)
    want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES)
    want_back = R.rgb_to_ycc_reference(want, REVERSE_TABLES)
    src = _nv(ps)[0]
    dst = torch.zeros_like(src)
    planes = nv12_planes(dst, H, width=W)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = ycc_to_rgb(*planes, **B709)
        rgb_to_ycc(warm, **B709)
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
        got = ycc_to_rgb(*planes, **B709)
        back = rgb_to_ycc(got, **B709)
        copy = [p.clone() for p in back]  # queued behind the kernels on the same stream
    side.synchronize()
    assert before.elapsed_time(after) > 150.0, "the sleep in front of the planes took %.1f ms" % before.elapsed_time(after)
    _same(got.cpu().numpy(), want, "side stream")
    for g, w in zip(copy, want_back):
        _same(g.cpu().numpy(), w, "side stream, back")


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
    ps = [_cuda(p) for p in _planes(T, H, W, 2, 71)]
    rgb = torch.full((T, H, W, 3), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = [tensors._plane_struct(p) for p in ps] + [tensors._struct(rgb, *tensors.descriptor(rgb, "NHWC")[1:])]
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

    def call(reverse, n=T, size=(H, W), y="ok", cb="ok", cr="ok", sub_v=2, sh=0, sv=0, interlaced=0, tables="ok", rgb_="ok", h="ok"):
        d = [ok[i] if isinstance(v, str) else _live(v, t) for i, (v, t) in enumerate(zip((y, cb, cr, rgb_), ps + [rgb]))]
        default = REVERSE_TABLES if reverse else FORWARD_TABLES
        tab = None if tables is None else (ctypes.c_int * len(default))(*(default if isinstance(tables, str) else tables))
        hh = gpu.h if h == "ok" else h
        if reverse:
            return gpu.L.papof_rgb_to_ycc_tensor(hh, n, size[0], size[1], ref(d[3]), sub_v, sh, sv, interlaced, tab, ref(d[0]),
                                                 ref(d[1]), ref(d[2]), None)
        return gpu.L.papof_ycc_to_rgb_tensor(hh, n, size[0], size[1], ref(d[0]), ref(d[1]), ref(d[2]), sub_v, sh, sv, interlaced,
                                             tab, ref(d[3]), None)

    before = [p.clone() for p in ps]
    for reverse, refusals in ((False, FORWARD_REFUSALS), (True, REVERSE_REFUSALS)):
        for kw in refusals:
            kw = {("rgb_" if k == "rgb" else k): v for k, v in kw.items()}
            assert call(reverse, **kw) == -1, (reverse, kw)
        assert call(reverse, h=None) == -1
    torch.cuda.synchronize()
    assert bool((rgb == 0x5a).all()) and all(torch.equal(a, b) for a, b in zip(ps, before))
    assert call(False) == 0  # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    host = [p.cpu().numpy() for p in ps]
    assert rgb.cpu().numpy().tobytes() == R.ycc_to_rgb_reference(*host, FORWARD_TABLES).tobytes()
    frames = rgb.cpu().numpy()
    assert call(True) == 0
    torch.cuda.synchronize()
    for g, w in zip(ps, R.rgb_to_ycc_reference(frames, REVERSE_TABLES)):
        assert g.cpu().numpy().tobytes() == w.tobytes()
