"""Dense block matching on device tensors (papteam_opticalflow_amd/tensors.py: match_pairs, match_video, match_init,
flow_pairs_ld, flow_video_ld -> papof_match_tensor, papof_match_densify_tensor).  The device's displacements, costs, dense
flows and hole masks must be the BYTES of the numpy restatement (tests/_match_ref.py): uint8, float32 and float64 frames of
1, 3 and 4 channels, NCHW, NHWC, permuted and sliced views, every stride, patch 1, 3 and 7, search 1, 8 and 32, sizes that
are multiples of neither the tile nor the stride, pairs and sequences with and without the backward fields, a penalty; two
runs give the same bytes, a call on a side stream behind a pending producer is correct, and on the synthetic scenes of the
CPU test the cold flow_pairs_fb loses the motion that flow_pairs_ld finds."""
import numpy as np
import pytest

from _inpaint_ref import fill_reference
from _match_ref import densify_reference, epe, match_reference, object_scene, pan_scene, texture

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


def _same(got, want, what):
    """a device tensor and an array, byte for byte"""
    g, w = np.ascontiguousarray(got.cpu().numpy()), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = g.view(np.uint8) != w.view(np.uint8)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(g != w)) if (g != w).any() else None
        raise AssertionError("%s: %d of %d bytes differ; first element at %s: %r against %r" % (
            what, int(bad.sum()), bad.size, i, g[i] if i else None, w[i] if i else None))


def _frames(n, H, W, C, dtype, seed, shift=(3, -2)):
    """(a, b): n textured frames (n, H, W, C) of `dtype` and the same texture moved by `shift` with a little noise; floats
    reach beyond 0 .. 1 and hold a NaN"""
    rng = np.random.default_rng(seed)
    pad = 16
    a, b = [], []
    for _ in range(n):
        t = texture(rng, H + 2 * pad, W + 2 * pad, C)
        a.append(t[pad:pad + H, pad:pad + W])
        b.append(t[pad - shift[1]:pad - shift[1] + H, pad - shift[0]:pad - shift[0] + W])
    a, b = np.stack(a), np.stack(b)
    b = np.clip(b.astype(np.int64) + rng.integers(-2, 3, b.shape), 0, 255).astype(np.uint8)
    if dtype == torch.uint8:
        return a, b
    a, b = (a / 255.0 * 1.2 - 0.1).astype(_NP[dtype]), (b / 255.0 * 1.2 - 0.1).astype(_NP[dtype])
    a[0, H // 2, W // 2, 0] = np.nan
    return a, b


def _as_layout(a, layout):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2).contiguous()


def _check_pairs(a, b, layout, what, both=True, out_dtype=None, **kw):
    from papteam_opticalflow_amd.tensors import match_pairs
    ta, tb = (a, b) if isinstance(a, torch.Tensor) else (_as_layout(a, layout), _as_layout(b, layout))
    na, nb = (t.cpu().numpy() if layout == "NHWC" else t.permute(0, 2, 3, 1).cpu().numpy() for t in (ta, tb))
    got = match_pairs(ta, tb, both=both, layout=layout, out_dtype=out_dtype, **kw)
    np_dtype = _NP[out_dtype or torch.float64]
    fw = match_reference(na, nb, out_dtype=np_dtype, **kw)
    _same(got.disp_fw, fw[0], what + ": disp_fw")
    _same(got.cost_fw, fw[1], what + ": cost_fw")
    if both:
        bw = match_reference(nb, na, out_dtype=np_dtype, **kw)
        _same(got.disp_bw, bw[0], what + ": disp_bw")
        _same(got.cost_bw, bw[1], what + ": cost_bw")
    else:
        assert got.disp_bw is None and got.cost_bw is None
    return got


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_dtypes_layouts_channels(C, dtype, layout):
    a, b = _frames(2, 45, 77, C, dtype, 10 + C)
    got = _check_pairs(a, b, layout, "%s %s C %d" % (dtype, layout, C), stride=2, patch=3, search=8)
    assert (got.disp_fw != 0).any()
    _check_pairs(a, b, layout, "%s %s C %d float32" % (dtype, layout, C), out_dtype=torch.float32, stride=1, patch=1,
                 search=8, both=False)


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
@pytest.mark.parametrize("patch", [1, 3, 7])
@pytest.mark.parametrize("search", [1, 8, 32])
def test_strides_patches_searches(stride, patch, search):
    """(H, W) multiples of neither the 32 x 8 tile nor the stride; a grid smaller than the window and the search"""
    for H, W in ((9 * stride + stride // 2, 37 * stride + (stride - 1)), (8 * stride, 32 * stride), (stride, 3 * stride + 1)):
        a, b = _frames(1, H, W, 3, torch.uint8, stride * 100 + patch * 10 + search, shift=(2 * stride, -stride))
        _check_pairs(a, b, "NHWC", "stride %d patch %d search %d %d x %d" % (stride, patch, search, H, W), stride=stride,
                     patch=patch, search=search)


def test_penalty_and_ties():
    a, b = _frames(2, 40, 70, 3, torch.uint8, 5)
    free = _check_pairs(a, b, "NHWC", "no penalty", stride=2, patch=2, search=6)
    for penalty in (1, 40, 65535):
        got = _check_pairs(a, b, "NHWC", "penalty %d" % penalty, stride=2, patch=2, search=6, penalty=penalty)
    assert (free.disp_fw != 0).any() and not (got.disp_fw != 0).any()  # the largest penalty pins every cell
    # constant frames: every candidate ties at cost 0, the shortest wins
    z = torch.full((1, 30, 50, 3), 7, dtype=torch.uint8, device="cuda")
    got = _check_pairs(z, z, "NHWC", "constant frames", stride=1, patch=3, search=5)
    assert not got.disp_fw.any() and not got.cost_fw.any()
    # a periodic pattern: ties between displacements of one length go to the smallest dy, then dx
    y, x = np.mgrid[0:32, 0:48]
    p = (((x % 4 == 0) | (y % 4 == 0)) * 200).astype(np.uint8)[None, ..., None]
    _check_pairs(p, np.roll(p, (2, 2), (1, 2)), "NHWC", "periodic", stride=1, patch=2, search=7)


def test_views_are_read_in_place():
    rng = np.random.default_rng(8)
    big = torch.from_numpy(texture(rng, 2 * 50 + 3, 2 * 90, 4)).cuda()[None].repeat(4, 1, 1, 1)
    big[1::2] = torch.roll(big[1::2], (3, -4), (1, 2))
    a = big[::2, 2:102:2, ::2, 1:]   # every other item, rows and columns, channels cut: (2, 50, 90, 3)
    b = big[1::2, 2:102:2, ::2, 1:]
    assert not a.is_contiguous()
    _check_pairs(a, b, "NHWC", "sliced NHWC", stride=2, patch=3, search=8)
    ap, bp = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)  # NCHW views of channels-last memory
    assert not ap.is_contiguous()
    _check_pairs(ap, bp, "NCHW", "permuted NCHW", stride=2, patch=3, search=8)
    one = a[:1].expand(2, 50, 90, 3)  # stride 0 along the items
    _check_pairs(one, b, "NHWC", "expanded", stride=4, patch=1, search=4)


@pytest.mark.parametrize("both", [True, False])
def test_sequence(both):
    from papteam_opticalflow_amd.tensors import match_pairs, match_video
    rng = np.random.default_rng(9)
    t = texture(rng, 80, 120, 3)
    v = np.stack([t[8 + 2 * k:8 + 2 * k + 57, 10 + 3 * k:10 + 3 * k + 91] for k in range(4)])
    tv = torch.from_numpy(v).cuda()
    got = match_video(tv, stride=2, patch=3, search=6, both=both, layout="NHWC")
    fw = match_reference(v[:-1], v[1:], stride=2, patch=3, search=6)
    _same(got.disp_fw, fw[0], "sequence: disp_fw")
    _same(got.cost_fw, fw[1], "sequence: cost_fw")
    assert tuple(got.disp_fw.shape) == (3, 2, 28, 45)
    if both:
        bw = match_reference(v[1:], v[:-1], stride=2, patch=3, search=6)
        _same(got.disp_bw, bw[0], "sequence: disp_bw")
        _same(got.cost_bw, bw[1], "sequence: cost_bw")
    else:
        assert got.disp_bw is None
    pairs = match_pairs(tv[:-1], tv[1:], stride=2, patch=3, search=6, both=both, layout="NHWC")
    assert torch.equal(pairs.disp_fw, got.disp_fw) and torch.equal(pairs.cost_fw, got.cost_fw)
    # the interior of the texture moved by (-3, -2) pixels per frame: the nearest cells
    mid = got.disp_fw[:, :, 8:-8, 8:-8]
    assert set(mid[:, 0].unique().tolist()) <= {-2.0, -4.0} and set(mid[:, 1].unique().tolist()) == {-2.0}


@pytest.mark.parametrize("stride,H,W", [(2, 45, 77), (1, 20, 33), (4, 45, 77), (8, 70, 100)])
def test_densify_and_init(stride, H, W):
    from papteam_opticalflow_amd import capi, tensors
    from papteam_opticalflow_amd.tensors import fill_holes, match_init, match_pairs
    a, b = _frames(2, H, W, 3, torch.uint8, 20 + stride, shift=(2 * stride, -stride))
    b[:, H // 3:H // 3 + 12, W // 3:W // 3 + 12] = 255 - b[:, H // 3:H // 3 + 12, W // 3:W // 3 + 12]  # something unmatched
    m = match_pairs(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), stride=stride, patch=2, search=6, layout="NHWC")
    n = [t.cpu().numpy() for t in m]
    for tol, max_cost in ((1, None), (0, None), (1, float(np.median(n[2]))), (3, 0)):
        got = match_init(*m, (H, W), tol=tol, max_cost=max_cost)
        fw, hole_fw = densify_reference(n[0], n[1], n[2], (H, W), stride, tol, max_cost)
        bw, hole_bw = densify_reference(n[1], n[0], n[3], (H, W), stride, tol, max_cost)
        what = "stride %d tol %d max_cost %r" % (stride, tol, max_cost)
        # the kernel's own outputs, before the fill: the flow (zeros where unreliable) and the hole mask of both directions
        f64 = (capi.DTYPE_F64, capi.DTYPE_F64)
        raw_flow, raw_mask = tensors._densify((m.disp_fw, m.disp_bw), f64, (m.cost_fw, m.cost_bw), f64, H, W, stride,
                                              *tensors._check_densify(tol, max_cost))
        _same(raw_flow, np.concatenate([fw, bw]), what + ": k_match_densify's flow")
        _same(raw_mask, np.concatenate([hole_fw, hole_bw]), what + ": k_match_densify's mask")
        _same(got.reliable, np.stack([hole_fw == 0, hole_bw == 0], 1), what + ": reliable")
        _same(got.init_fw, fill_reference(fw.transpose(0, 2, 3, 1), hole_fw, 0).transpose(0, 3, 1, 2), what + ": init_fw")
        _same(got.init_bw, fill_reference(bw.transpose(0, 2, 3, 1), hole_bw, 0).transpose(0, 3, 1, 2), what + ": init_bw")
        # the mask is what fill_holes takes: the composition by hand gives the same bytes
        by_hand = fill_holes(torch.from_numpy(fw).cuda(), torch.from_numpy(hole_fw).cuda())
        assert torch.equal(by_hand.view(torch.int64), got.init_fw.view(torch.int64))
    assert 0 < hole_fw.mean() < 1 or max_cost == 0
    # fields that are not whole cells, leave the grid or are not finite are unreliable, not read out of bounds
    bad = m.disp_fw.clone()
    bad[0, 0, 0, 0], bad[0, 1, 1, 1], bad[0, 0, 2, 2], bad[1, 0, 0, 0] = float("nan"), 1e300, stride * 0.5, float("inf")
    got = match_init(bad, m.disp_bw, None, None, (H, W))
    fw, hole_fw = densify_reference(bad.cpu().numpy(), n[1], None, (H, W), stride)
    _same(got.reliable[:, 0], hole_fw == 0, "bad fields")
    assert not got.reliable[0, 0, 0, 0] and torch.isfinite(got.init_fw).all()


def test_two_runs_and_a_side_stream():
    """the same bytes twice; inputs written on a side stream behind a long sleep and matched under that stream with no
    synchronisation: every kernel must follow the writes"""
    import time
    from papteam_opticalflow_amd.tensors import match_init, match_pairs
    a, b = _frames(2, 135, 240, 3, torch.uint8, 30, shift=(9, -5))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    first = match_pairs(ta, tb, layout="NHWC")
    again = match_pairs(ta, tb, layout="NHWC")
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    want = [t.cpu().numpy() for t in first]
    want_init = [t.cpu().numpy() for t in match_init(*first, (135, 240))]
    da, db = torch.zeros_like(ta), torch.zeros_like(tb)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = match_init(*match_pairs(da, db, layout="NHWC"), (135, 240))
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        da.copy_(ta)
        db.copy_(tb)
        got = match_pairs(da, db, layout="NHWC")
        init = match_init(*got, (135, 240))
        took = time.perf_counter() - t0
    side.synchronize()
    assert took < 0.25, "the calls waited for the stream: %.3f s" % took
    for g, w, name in zip(got, want, got._fields):
        _same(g, w, "side stream: " + name)
    for g, w, name in zip(init, want_init, init._fields):
        _same(g, w, "side stream: " + name)


def _epe(flow, truth, where):
    f = flow.cpu().numpy()
    return epe(f[0], f[1], truth, where)


@pytest.mark.parametrize("scene,kind", [((1, (34, -14)), "object"), ((2, (20, 10)), "object"), ((3, (28, 9)), "pan")])
def test_flow_pairs_ld_finds_what_the_cold_call_loses(scene, kind):
    """The premise and the thresholds of tests/test_match_cpu.py against the device's own cold flow_pairs_fb, and each
    direction byte-equal to flow_pairs_fb started from match_init's flows"""
    from papteam_opticalflow_amd.tensors import flow_pairs_fb, flow_pairs_ld, match_init, match_pairs
    im1, im2, truth, interior = (object_scene if kind == "object" else pan_scene)(*scene)
    t1, t2 = torch.from_numpy(im1[None]).cuda(), torch.from_numpy(im2[None]).cuda()
    cold = flow_pairs_fb(t1, t2, 5, layout="NHWC")
    e_cold = _epe(cold.flow_fw[0], truth, interior)
    print("%s %r: cold 5 levels, interior EPE %.3f" % (kind, scene[1], e_cold))
    assert e_cold > (0.5 * float(np.hypot(*scene[1])) if kind == "object" else 10.0)
    init = match_init(*match_pairs(t1, t2, layout="NHWC"), im1.shape[:2])
    for levels in (1, 2):
        ld = flow_pairs_ld(t1, t2, levels, layout="NHWC")
        e = _epe(ld.flow_fw[0], truth, interior)
        print("%s %r: flow_pairs_ld %d level(s), interior EPE %.4f" % (kind, scene[1], levels, e))
        assert e < 0.5
        ref = flow_pairs_fb(t1, t2, levels, layout="NHWC", init_flow=init.init_fw, init_flow_bw=init.init_bw)
        for name in ("flow_fw", "flow_bw", "warpI2_fw", "warpI2_bw"):
            assert torch.equal(getattr(ld, name).view(torch.int64), getattr(ref, name).view(torch.int64)), name
        assert torch.equal(ld.occlusion, ref.occlusion)
    assert flow_pairs_ld(t1, t2, layout="NHWC").flow_fw.shape == (1, 2, 135, 240)


def test_flow_video_ld_is_flow_video_fb_from_the_matches():
    from papteam_opticalflow_amd.tensors import flow_video_fb, flow_video_ld, match_init, match_video
    rng = np.random.default_rng(12)
    t = texture(rng, 200, 300, 3)
    v = torch.from_numpy(np.stack([t[20 + 11 * k:20 + 11 * k + 90, 30 + 17 * k:30 + 17 * k + 150] for k in range(3)])).cuda()
    ld = flow_video_ld(v, layout="NHWC", out_dtype=torch.float32)
    init = match_init(*match_video(v, layout="NHWC"), (90, 150))
    ref = flow_video_fb(v, 2, layout="NHWC", out_dtype=torch.float32, init_flow=init.init_fw, init_flow_bw=init.init_bw)
    assert torch.equal(ld.flow_fw.view(torch.int32), ref.flow_fw.view(torch.int32))
    assert torch.equal(ld.flow_bw.view(torch.int32), ref.flow_bw.view(torch.int32))
    mid = ld.flow_fw[:, :, 20:-20, 30:-30]
    assert float((mid[:, 0] + 17).abs().mean()) < 0.5 and float((mid[:, 1] + 11).abs().mean()) < 0.5
