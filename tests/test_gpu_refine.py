"""Edge-aware flow refinement on device tensors (papteam_opticalflow_amd/tensors.py: refine_flow, refine_video_flows ->
papof_refine_flow_tensor).  The device's output must be the BYTES of the numpy restatement (tests/_refine_ref.py) given the
library's own tables, compared as raw bytes: uint8, float32 and float64 guides of 1 .. 4 channels, NCHW, NHWC and strided
views, float32 and float64 flows, every output dtype, radius 1, 2, 7 and 15, one and three passes, with and without the
occlusion and `where` masks, ragged sizes down to frames smaller than the window, fields with NaNs, infinities, signed zeros,
ties and duplicates, the real flows of the committed video through refine_video_flows, a 1080p case run twice and compared at
sampled pixels, `where` all zero, the caller's stream order and the inputs left unchanged."""
import numpy as np
import pytest

from _refine_ref import refine_reference
from test_gpu_batch import _video
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same_flow(got, want, what):
    """two flows (B, 2, H, W), byte for byte"""
    g, w = np.ascontiguousarray(got.cpu().numpy()), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    iv = np.int64 if g.dtype == np.float64 else np.int32
    bad = g.view(iv) != w.view(iv)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r against %r" % (what, int(bad.sum()), bad.size, i,
                                                                                          g[i], w[i]))


def _guide(B, H, W, C, dtype, seed):
    """two flat regions split by a slanted edge, a smooth wave and a little noise, (B, H, W, C) in the dtype's range"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.empty((B, H, W, C))
    for b in range(B):
        for c in range(C):
            side = (x * rng.uniform(0.5, 1.5) + y * rng.uniform(-1, 1) > rng.uniform(0.3, 0.7) * W)
            g[b, ..., c] = 0.3 + 0.4 * side + 0.05 * np.sin(0.3 * x + c + b) * np.cos(0.2 * y) + rng.normal(0, 0.01, (H, W))
    g = np.clip(g, 0, 1)
    return np.rint(255 * g).astype(np.uint8) if dtype == torch.uint8 else g.astype(_NP[dtype])


def _masks(B, H, W, seed):
    rng = np.random.default_rng(seed)
    occ = (rng.random((B, H, W)) < 0.2).astype(np.uint8)
    occ[:, H // 3:H // 3 + 9, W // 4:W // 4 + 12] = 1  # a block larger than a small window: pixels with no live neighbour
    where = rng.random((B, H, W)) < 0.6
    where[:, :, W // 2:W // 2 + 40] = False  # whole tiles without a pixel to filter
    return occ, where


def _as_layout(a, layout):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2)


def _want(flow, guide, radius, sigma_s, sigma_c, **kw):
    """the restatement with the library's own tables and q"""
    from papteam_opticalflow_amd import tensors
    S, R = tensors.refine_tables(radius, sigma_s)
    g = np.asarray(guide)
    return refine_reference(flow, g, S, R, tensors.refine_q(sigma_c, g.shape[3], g.dtype == np.uint8), radius, **kw)


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    from papteam_opticalflow_amd.tensors import refine_flow
    B, H, W, C = 2, 37, 53, 3
    guide = _guide(B, H, W, C, dtype, 1)
    tg = _as_layout(guide, layout)
    fw, _ = _fields(B + 1, H, W, 3)
    assert np.isnan(fw).any() and np.isinf(fw).any()
    occ, where = _masks(B, H, W, 4)
    t_occ, t_where = torch.from_numpy(occ).cuda(), torch.from_numpy(where).cuda()
    runs = 0
    for fdt in (torch.float64, torch.float32):
        tf = torch.from_numpy(fw).to(fdt).cuda()
        nf = tf.cpu().numpy()
        for radius, sigma_s, sigma_c in ((1, 0.8, 0.05), (2, 1e6, 0.5), (7, 7.0, 7 / 255), (15, 9.0, 0.1)):
            for use_occ, use_where in ((False, False), (True, False), (False, True), (True, True)):
                for iters in (1, 3):
                    for odt in (None, torch.float32, torch.float64) if iters == 1 and radius in (2, 7) else (None,):
                        got = refine_flow(tf, tg, occlusion=t_occ if use_occ else None, where=t_where if use_where else None,
                                          radius=radius, sigma_s=sigma_s, sigma_c=sigma_c, iters=iters, layout=layout,
                                          out_dtype=odt)
                        want = _want(nf, guide, radius, sigma_s, sigma_c, occlusion=occ if use_occ else None,
                                     where=where if use_where else None, iters=iters, out_dtype=_NP[odt or fdt])
                        _same_flow(got, want, "%s %s flows %s r %d occ %d where %d iters %d out %s" % (
                            dtype, layout, fdt, radius, use_occ, use_where, iters, odt))
                        runs += 1
    assert runs == 2 * 4 * 4 * 2 + 2 * 2 * 4 * 2
    # the fields reach the branches: the filter changes pixels and replaces NaNs
    want = _want(fw, guide, 2, 1e6, 0.5, occlusion=occ)
    assert (want != fw).any() and np.isnan(want).sum() < np.isnan(fw).sum()


@pytest.mark.parametrize("H,W", [(37, 53), (1, 9), (9, 1), (5, 4), (8, 32), (9, 33)])
def test_ragged_sizes_and_channel_counts(H, W):
    """frames that are one row, one column, smaller than the window, exactly one tile and one pixel more than a tile, with
    1, 2 and 4 channels of every dtype"""
    from papteam_opticalflow_amd.tensors import refine_flow
    B = 2
    rng = np.random.default_rng(H * 100 + W)
    flow = rng.normal(0, 2, (B, 2, H, W))
    flow[rng.random(flow.shape) < 0.05] = np.nan
    occ = (rng.random((B, H, W)) < 0.15)
    tf = torch.from_numpy(flow).cuda()
    for C, dtype in ((1, torch.uint8), (1, torch.float64), (2, torch.float32), (4, torch.uint8), (4, torch.float64)):
        guide = _guide(B, H, W, C, dtype, 7 + C)
        for layout in ("NCHW", "NHWC"):
            for radius in (1, 2, 7, 15):
                got = refine_flow(tf, _as_layout(guide, layout), occlusion=torch.from_numpy(occ).cuda(), radius=radius,
                                  sigma_s=radius / 1.5, sigma_c=0.08, layout=layout, iters=2)
                want = _want(flow, guide, radius, radius / 1.5, 0.08, occlusion=occ, iters=2)
                _same_flow(got, want, "%d x %d C %d %s %s r %d" % (H, W, C, dtype, layout, radius))


def test_strided_views_and_a_batch_of_one():
    from papteam_opticalflow_amd.tensors import refine_flow
    B, H, W = 3, 29, 41
    fw, _ = _fields(B + 1, H, W, 5)
    rng = np.random.default_rng(6)
    big = torch.from_numpy(_guide(2 * B, H + 3, 2 * W, 4, torch.uint8, 8)).cuda()
    g = big[::2, 2:H + 2, ::2, 1:]  # every other item, rows cut, every other column, channels cut: 3 channels
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)  # channels-last flow
    occ, where = _masks(B, H, 2 * W, 9)
    t_occ, t_where = torch.from_numpy(occ).cuda()[:, :, 1::2], torch.from_numpy(where).cuda()[:, :, ::2]
    assert not g.is_contiguous() and not tf.is_contiguous() and not t_occ.is_contiguous() and not t_where.is_contiguous()
    got = refine_flow(tf, g, occlusion=t_occ, where=t_where, radius=3, sigma_s=2.0, sigma_c=0.1, layout="NHWC", iters=2)
    want = _want(fw, g.cpu().numpy(), 3, 2.0, 0.1, occlusion=occ[:, :, 1::2], where=where[:, :, ::2], iters=2)
    _same_flow(got, want, "strided views")
    # an expanded guide (stride 0 along the items) and a 3-D guide: a batch of one
    one = torch.from_numpy(_guide(1, H, W, 1, torch.float32, 10)).cuda()
    got = refine_flow(tf, one.expand(B, H, W, 1), radius=4, sigma_c=0.2, layout="NHWC")
    want = _want(fw, np.repeat(one.cpu().numpy(), B, 0), 4, 7.0, 0.2)
    _same_flow(got, want, "expanded guide")
    got = refine_flow(tf[:1], one[0], radius=4, sigma_c=0.2, layout="NHWC")
    _same_flow(got, want[:1], "3-D guide")


def test_signed_zeros_ties_and_duplicates():
    from papteam_opticalflow_amd.tensors import refine_flow
    H, W = 20, 45
    rng = np.random.default_rng(11)
    flow = np.zeros((4, 2, H, W))
    flow[0] = np.where(rng.random((2, H, W)) < 0.5, -0.0, 0.0)                 # -0.0 next to +0.0
    flow[1, 0], flow[1, 1] = 1.75, -3.5                                         # all equal: ties everywhere
    flow[2] = rng.integers(-2, 3, (2, H, W)) * 0.25                             # five values, many duplicates, different weights
    flow[3] = np.where(rng.random((2, H, W)) < 0.3, np.inf, rng.integers(0, 2, (2, H, W)) * 1e-310)  # subnormals, infinities
    flow[3][rng.random((2, H, W)) < 0.1] = -np.inf
    guide = _guide(4, H, W, 3, torch.uint8, 12)
    for radius, sigma_c in ((1, 0.1), (3, 7 / 255), (7, 0.3)):
        for fdt in (torch.float64, torch.float32):
            tf = torch.from_numpy(flow).to(fdt).cuda()
            got = refine_flow(tf, torch.from_numpy(guide).cuda(), radius=radius, sigma_c=sigma_c, layout="NHWC")
            want = _want(tf.cpu().numpy(), guide, radius, 7.0, sigma_c)
            _same_flow(got, want, "special values r %d %s" % (radius, fdt))
    z = _want(flow[:1], guide[:1], 3, 7.0, 0.3)
    assert np.signbit(z).any() and not np.signbit(z).all()  # both zeros are chosen somewhere


@pytest.mark.parametrize("res,n", [("240", 4), ("480", 2)])
def test_real_flows_of_the_committed_video(res, n):
    """flow_video_fb -> refine_video_flows against the restatement composed the same way: forward flows guided by frames[:-1]
    with channel 0 of the mask, backward flows by frames[1:] with channel 1, the mask recomputed by fb_consistency"""
    from papteam_opticalflow_amd.tensors import fb_consistency, flow_video_fb, refine_video_flows
    v = _dev(_video(res, n))
    fb = flow_video_fb(v, 4, layout="NHWC")
    got = refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion, layout="NHWC")
    frames, occ = v.cpu().numpy(), fb.occlusion.cpu().numpy()
    fw = _want(fb.flow_fw.cpu().numpy(), frames[:-1], 7, 7.0, 7 / 255, occlusion=occ[:, 0])
    bw = _want(fb.flow_bw.cpu().numpy(), frames[1:], 7, 7.0, 7 / 255, occlusion=occ[:, 1])
    _same_flow(got.flow_fw, fw, "%s forward" % res)
    _same_flow(got.flow_bw, bw, "%s backward" % res)
    assert got.occlusion.dtype == torch.bool
    assert torch.equal(got.occlusion, fb_consistency(torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()))
    changed = float((got.flow_fw != fb.flow_fw).double().mean())
    print("%s: %.1f %% of the forward components changed, occluded %.2f %% -> %.2f %%" % (
        res, 100 * changed, 100 * float(fb.occlusion.double().mean()), 100 * float(got.occlusion.double().mean())))
    assert changed > 0.1
    # without a mask, NCHW frames, two passes, float32 out; consistency=None gives no mask
    got = refine_video_flows(v.permute(0, 3, 1, 2), fb.flow_fw, fb.flow_bw, consistency=None, radius=3, iters=2,
                             out_dtype=torch.float32)
    assert got.occlusion is None
    _same_flow(got.flow_fw, _want(fb.flow_fw.cpu().numpy(), frames[:-1], 3, 7.0, 7 / 255, iters=2, out_dtype=np.float32),
               "%s forward, r 3" % res)
    _same_flow(got.flow_bw, _want(fb.flow_bw.cpu().numpy(), frames[1:], 3, 7.0, 7 / 255, iters=2, out_dtype=np.float32),
               "%s backward, r 3" % res)


def test_1080p_twice_and_at_sampled_pixels():
    """One 1920 x 1080 flow at the defaults, run twice: the same bytes; and 4096 random pixels, the four corners and 64 points
    on every border against the restatement evaluated at those pixels only"""
    from papteam_opticalflow_amd import tensors
    H, W = 1080, 1920
    rng = np.random.default_rng(13)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    layer = (np.hypot(y - 500, x - 900) < 300) | ((x > 1400) & (y > 700))
    guide = np.rint(255 * np.clip(np.where(layer[..., None], [0.7, 0.4, 0.3], [0.3, 0.5, 0.6]) + 0.04 * np.sin(0.05 * x + 0.03 * y)[..., None]
                                  + rng.normal(0, 0.01, (H, W, 3)), 0, 1)).astype(np.uint8)[None]
    flow = np.stack([np.where(layer, 6.0, 0.5) + np.sin(0.01 * x), np.where(layer, -3.0, 0.2) + np.cos(0.013 * y)])[None]
    flow += rng.normal(0, 0.05, flow.shape)
    flow[0, :, rng.integers(0, H, 500), rng.integers(0, W, 500)] = np.nan
    occ = rng.random((1, H, W)) < 0.05
    tf, tg, to = torch.from_numpy(flow).cuda(), torch.from_numpy(guide).cuda(), torch.from_numpy(occ).cuda()
    a = tensors.refine_flow(tf, tg, occlusion=to, layout="NHWC")
    b = tensors.refine_flow(tf, tg, occlusion=to, layout="NHWC")
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    edge_y, edge_x = rng.integers(0, H, 64), rng.integers(0, W, 64)
    ys = np.concatenate([rng.integers(0, H, 4096), [0, 0, H - 1, H - 1], np.zeros(64, int), np.full(64, H - 1), edge_y, edge_y])
    xs = np.concatenate([rng.integers(0, W, 4096), [0, W - 1, 0, W - 1], edge_x, edge_x, np.zeros(64, int), np.full(64, W - 1)])
    assert len(ys) == len(xs) == 4096 + 4 + 256
    S, R = tensors.refine_tables(tensors.RADIUS, tensors.SIGMA_S)
    want = refine_reference(flow, guide, S, R, tensors.refine_q(tensors.SIGMA_C, 3, True), tensors.RADIUS, occlusion=occ,
                            pixels=(ys, xs))
    got = a.cpu().numpy()[0][:, ys, xs].T
    bad = got.view(np.int64) != np.ascontiguousarray(want[0]).view(np.int64)
    assert not bad.any(), "%d of %d sampled components differ; first at pixel (%d, %d)" % (
        int(bad.sum()), bad.size, ys[np.nonzero(bad)[0][0]], xs[np.nonzero(bad)[0][0]])
    assert (got != flow[0][:, ys, xs].T).mean() > 0.5  # the filter did something there


def test_where_all_zero_copies_and_inputs_are_unchanged():
    from papteam_opticalflow_amd.tensors import refine_flow
    B, H, W = 2, 37, 53
    fw, _ = _fields(B + 1, H, W, 14)
    guide = _guide(B, H, W, 3, torch.uint8, 15)
    occ, where = _masks(B, H, W, 16)
    for fdt in (torch.float64, torch.float32):
        tf, tg = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(guide).cuda()
        t_occ, t_where = torch.from_numpy(occ).cuda(), torch.from_numpy(where).cuda()
        keep = [t.clone() for t in (tf, tg, t_occ, t_where)]
        got = refine_flow(tf, tg, occlusion=t_occ, where=torch.zeros((B, H, W), dtype=torch.bool, device="cuda"), layout="NHWC")
        _same_flow(got, tf.cpu().numpy(), "where all zero")  # NaNs and infinities included, bit for bit
        refine_flow(tf, tg, occlusion=t_occ, where=t_where, layout="NHWC", iters=3)
        iv = torch.int64 if fdt == torch.float64 else torch.int32
        assert torch.equal(tf.view(iv), keep[0].view(iv)) and torch.equal(tg, keep[1])
        assert torch.equal(t_occ, keep[2]) and torch.equal(t_where, keep[3])


def test_the_call_is_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and refined under that stream with no synchronisation: every pass
    must follow the writes, and what is queued behind them must see their output"""
    import time
    from papteam_opticalflow_amd.tensors import refine_flow
    B, H, W = 2, 40, 60
    fw, _ = _fields(B + 1, H, W, 18)
    guide = _guide(B, H, W, 3, torch.uint8, 17)
    occ, _ = _masks(B, H, W, 19)
    want = _want(fw, guide, 7, 7.0, 7 / 255, occlusion=occ, iters=3)
    src = [torch.from_numpy(fw).cuda(), torch.from_numpy(guide).cuda(), torch.from_numpy(occ).cuda()]
    dst = [torch.zeros_like(s) for s in src]
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks and the tables exist
        warm = refine_flow(dst[0], dst[1], occlusion=dst[2], layout="NHWC", iters=3).clone()
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the call
        for d, s in zip(dst, src):
            d.copy_(s)
        got = refine_flow(dst[0], dst[1], occlusion=dst[2], layout="NHWC", iters=3)
        took = time.perf_counter() - t0
        copy = got.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    assert took < 0.25, "the call waited for the stream: %.3f s" % took
    _same_flow(got, want, "side stream")
    _same_flow(copy, want, "side stream clone")
