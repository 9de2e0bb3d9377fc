"""Flow-guided video completion on device tensors (papteam_opticalflow_amd/tensors.py: fill_holes, complete_flows, propagate,
inpaint_video -> papof_fill_holes_tensor, papof_propagate_tensor).  The device's outputs must be the BYTES of the numpy
fp64 restatement (tests/_inpaint_ref.py), compared as raw bytes: uint8, float32 and float64 inputs, NCHW, NHWC and strided
views, 1 to 4 channels, random, all-known, all-hole and single-pixel masks, 1 x N, N x 1, 1 x 1, 135 x 240 and 1080p frames,
wild flows, radius 1 and T - 1 with and without the check; inpaint_video on the panning video of tests/test_inpaint_cpu.py
(pixels outside the masks byte-identical, the calibrated quality margin with the device's own flows); the caller's stream
order, a reused workspace and bitwise determinism."""
import numpy as np
import pytest

from _inpaint_ref import fill_reference, propagate_reference
from _interp_ref import convert
from test_gpu_tensors import _dev
from test_gpu_track import _fields
from test_inpaint_cpu import PIPELINE_MARGIN, _psnr_masked, pipeline_reference, synthetic_video

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd.tensors import (CONSISTENCY, complete_flows, fill_holes, flow_video_fb,  # noqa: E402
                                             inpaint_video, propagate)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same_bytes(got, want, layout, what):
    """got (N, C, H, W) or (N, H, W, C) by layout -- or (N, H, W) with layout None -- against want in (N, H, W, C) /
    (N, H, W), byte for byte"""
    g = got.permute(0, 2, 3, 1) if layout == "NCHW" else got
    g = np.ascontiguousarray(g.cpu().numpy())
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    gb, wb = g.view(np.uint8).reshape(g.shape + (-1,)), w.view(np.uint8).reshape(w.shape + (-1,))
    bad = (gb != wb).any(-1)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r against %r" % (what, int(bad.sum()), bad.size,
                                                                                          i, g[i], w[i]))


def _frames(n, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (n, H, W, C)).astype(np.uint8)
    return rng.random((n, H, W, C)).astype(_NP[dtype])


def _as_layout(a, layout):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2)


def _masks(kind, n, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        m = rng.random((n, H, W)) < 0.3
    elif kind == "known":
        m = np.zeros((n, H, W), bool)
    elif kind == "hole":
        m = np.ones((n, H, W), bool)
        m[0] = rng.random((H, W)) < 0.5  # frame 0 a random mask, the others all holes
    else:
        m = np.zeros((n, H, W), bool)
        m[:, rng.integers(0, H), rng.integers(0, W)] = True
    return m


# ---- fill_holes
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_fill_every_dtype_layout_and_channel_count(dtype, layout):
    for C, (H, W) in zip((1, 2, 3, 4), ((37, 53), (1, 70), (70, 1), (1, 1))):
        x = _frames(3, H, W, C, dtype, C)
        for kind in ("random", "known", "hole", "single"):
            m = _masks(kind, 3, H, W, 10 + C)
            tm = torch.from_numpy(m).cuda()
            for relax in (0, 3):
                want64 = fill_reference(x, m, relax)
                for odt in (None, torch.uint8, torch.float32, torch.float64):
                    got = fill_holes(_as_layout(x, layout), tm if odt is None else tm.to(torch.uint8), layout=layout,
                                     relax=relax, out_dtype=odt)
                    what = "%s %s C %d %dx%d %s relax %d out %s" % (dtype, layout, C, H, W, kind, relax, odt)
                    _same_bytes(got, convert(want64, _NP[odt or dtype]), layout, what)


def test_fill_strided_views_and_135x240():
    big = torch.from_numpy(_frames(6, 140, 490, 4, torch.uint8, 20)).cuda()
    v = big[::2, 2:137, ::2, 1:]  # every other frame, rows cut, every other column, channels cut: (3, 135, 245, 3)
    v = v[:, :, :240]
    assert not v.is_contiguous() and tuple(v.shape) == (3, 135, 240, 3)
    m = _masks("random", 3, 135, 240, 21)
    mt = torch.from_numpy(np.repeat(m, 2, axis=2)).cuda()[:, :, ::2]  # a strided mask
    want = fill_reference(v.cpu().numpy(), m, 5)
    _same_bytes(fill_holes(v, mt, layout="NHWC", relax=5, out_dtype=torch.float64), want, "NHWC", "strided NHWC")
    _same_bytes(fill_holes(v.permute(0, 3, 1, 2), mt, relax=5), convert(want, np.uint8), "NCHW", "strided NCHW")


def test_fill_1080p():
    x = _frames(1, 1080, 1920, 3, torch.uint8, 30)
    m = np.zeros((1, 1080, 1920), bool)
    m[0, 200:700, 300:1400] = True
    m[0] |= np.random.default_rng(31).random((1080, 1920)) < 0.05
    want = fill_reference(x, m, 2, np.uint8)
    _same_bytes(fill_holes(_as_layout(x, "NHWC"), torch.from_numpy(m).cuda(), layout="NHWC", relax=2), want, "NHWC", "1080p")


def test_complete_flows():
    T, H, W = 5, 41, 67
    fw, bw = _fields(T, H, W, 40, wild=False)  # (a filled infinity gives a NaN whose sign bit is the platform's)
    m = _masks("random", T, H, W, 41)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).float().cuda()
    for relax in (0, 4):
        cf = complete_flows(tf, tb, torch.from_numpy(m).cuda(), relax=relax)
        assert cf.flow_fw.dtype == torch.float64 and cf.flow_bw.dtype == torch.float32
        want_f = np.moveaxis(fill_reference(np.moveaxis(fw, 1, -1), m[:-1], relax), -1, 1)
        want_b = np.moveaxis(fill_reference(np.moveaxis(tb.cpu().numpy(), 1, -1), m[1:], relax, np.float32), -1, 1)
        _same_bytes(cf.flow_fw, np.moveaxis(want_f, 1, -1), "NCHW", "flow_fw relax %d" % relax)
        _same_bytes(cf.flow_bw, np.moveaxis(want_b, 1, -1), "NCHW", "flow_bw relax %d" % relax)


# ---- propagate
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_propagate_wild_flows(dtype, layout):
    T, H, W, C = 5, 37, 53, 3
    x = _frames(T, H, W, C, dtype, 50)
    fw, bw = _fields(T, H, W, 51)
    m = _masks("random", T, H, W, 52) | (np.random.default_rng(53).random((T, H, W)) < 0.2)
    tm = torch.from_numpy(m).cuda()
    v = _as_layout(x, layout)
    for fdt in (torch.float64, torch.float32):
        tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
        for R in (1, 2, T - 1):
            for cons in (CONSISTENCY, None):
                want, st = propagate_reference(x, m, nf, nb, R, cons)
                for odt in (None, torch.uint8, torch.float64):
                    got = propagate(v, tm, tf, tb, radius=R, consistency=cons, layout=layout, out_dtype=odt)
                    what = "%s %s flows %s R %d check %s out %s" % (dtype, layout, fdt, R, cons is not None, odt)
                    _same_bytes(got.video, convert(want, _NP[odt or dtype]), layout, what)
                    _same_bytes(got.status, st, None, what + " status")
    assert (st == 1).any() and (st == 2).any() and (st == 0).any()


@pytest.mark.parametrize("C,shape", [(1, (1, 90)), (2, (90, 1)), (4, (1, 1)), (3, (135, 240))])
def test_propagate_shapes_and_channels(C, shape):
    H, W = shape
    T = 4
    x = _frames(T, H, W, C, torch.float32, 60 + C)
    fw, bw = _fields(T, H, W, 61, wild=H > 8 and W > 8)
    for kind in ("random", "known", "hole", "single"):
        m = _masks(kind, T, H, W, 62)
        for R, cons in ((1, None), (T - 1, CONSISTENCY)):
            want, st = propagate_reference(x, m, fw, bw, R, cons, np.float32)
            got = propagate(_as_layout(x, "NCHW"), torch.from_numpy(m).cuda(), torch.from_numpy(fw).cuda(),
                            torch.from_numpy(bw).cuda(), radius=R, consistency=cons)
            _same_bytes(got.video, want, "NCHW", "%s %s R %d" % (kind, shape, R))
            _same_bytes(got.status, st, None, "%s %s R %d status" % (kind, shape, R))


def test_propagate_1080p():
    T, H, W, C = 3, 1080, 1920, 3
    x = _frames(T, H, W, C, torch.uint8, 70)
    g = torch.Generator().manual_seed(71)
    fw = torch.nn.functional.interpolate(torch.randn(T - 1, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 6,
                                         size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.3 * torch.randn(T - 1, 2, H, W, generator=g, dtype=torch.float64)
    m = np.zeros((T, H, W), bool)
    for t in range(T):
        m[t, 300 + 40 * t:600 + 40 * t, 500 + 90 * t:900 + 90 * t] = True
    want, st = propagate_reference(x, m, fw.numpy(), bw.numpy(), 2, CONSISTENCY, np.uint8)
    got = propagate(_as_layout(x, "NHWC"), torch.from_numpy(m).cuda(), fw.cuda(), bw.cuda(), radius=2,
                    consistency=CONSISTENCY, layout="NHWC")
    _same_bytes(got.video, want, "NHWC", "1080p")
    _same_bytes(got.status, st, None, "1080p status")


# ---- end to end
def test_inpaint_video_on_the_panning_video():
    """the device's flows (4 levels), the composition of the restatement on them byte for byte, the pixels outside the masks
    untouched, and the calibrated margin of the pipeline over spatial fill alone (tests/test_inpaint_cpu.py)"""
    clean, frames, masks, _, _ = synthetic_video()
    v = _dev(list(frames))
    tm = torch.from_numpy(masks).cuda()
    iv = inpaint_video(v, tm, 4, layout="NHWC")
    fb = flow_video_fb(v, 4, layout="NHWC", consistency=None)
    want, st = pipeline_reference(frames, masks, fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 0, None)
    _same_bytes(iv.video, want, "NHWC", "inpaint_video")
    _same_bytes(iv.status, st, None, "inpaint_video status")
    out = iv.video.cpu().numpy()
    assert (out[~masks] == frames[~masks]).all()
    spatial = fill_holes(v, tm, layout="NHWC").cpu().numpy()
    ps, pf = _psnr_masked(spatial, clean, masks), _psnr_masked(out, clean, masks)
    assert pf > ps + PIPELINE_MARGIN, (ps, pf)
    # the given flows, NCHW, float32 out
    iv2 = inpaint_video(v.permute(0, 3, 1, 2), tm, 4, flows=(fb.flow_fw, fb.flow_bw), out_dtype=torch.float32)
    want32, _ = pipeline_reference(frames, masks, fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 0, None,
                                   out_dtype=np.float32)
    _same_bytes(iv2.video, want32, "NCHW", "inpaint_video float32")
    assert torch.equal(iv2.status, iv.status)


# ---- stream order, workspace reuse, determinism
def test_stream_order_workspace_reuse_and_determinism():
    """Inputs written on a side stream behind a long sleep and used under that stream with no synchronisation: the kernels
    must read them after they are written.  Calls in a row reuse the allocator's workspace blocks; two runs are bitwise
    equal."""
    import time
    T, H, W, C = 4, 60, 90, 3
    x = _frames(T, H, W, C, torch.uint8, 80)
    m = _masks("random", T, H, W, 81)
    fw, bw = _fields(T, H, W, 82, wild=False)
    want_f = fill_reference(x, m, 3, np.uint8)
    want_p, want_s = propagate_reference(x, m, fw, bw, T - 1, None, np.uint8)
    src, msrc = _dev(list(x)), torch.from_numpy(m).cuda()
    dst, mdst = torch.zeros_like(src), torch.zeros_like(msrc)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        fill_holes(dst, mdst, layout="NHWC", relax=3)
        propagate(dst, mdst, tf, tb, layout="NHWC")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        dst.copy_(src)
        mdst.copy_(msrc)
        f1 = fill_holes(dst, mdst, layout="NHWC", relax=3)
        f2 = fill_holes(dst, mdst, layout="NHWC", relax=3)  # the first call's workspace block, reused behind it
        p1 = propagate(dst, mdst, tf, tb, layout="NHWC")
        p2 = propagate(dst, mdst, tf, tb, layout="NHWC")
    side.synchronize()
    for got, what in ((f1, "fill 1"), (f2, "fill 2")):
        _same_bytes(got, want_f, "NHWC", what)
    for got, what in ((p1, "propagate 1"), (p2, "propagate 2")):
        _same_bytes(got.video, want_p, "NHWC", what)
        _same_bytes(got.status, want_s, None, what + " status")
    clean, frames, masks, _, _ = synthetic_video(T=5, H=64, W=120, box0=(20, 20))
    a = inpaint_video(_dev(list(frames)), torch.from_numpy(masks).cuda(), 3, layout="NHWC")
    b = inpaint_video(_dev(list(frames)), torch.from_numpy(masks).cuda(), 3, layout="NHWC")
    assert torch.equal(a.video, b.video) and torch.equal(a.status, b.status)
