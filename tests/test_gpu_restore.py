"""Dirt and dropout removal on device tensors (papteam_opticalflow_amd/tensors.py: detect_defects, dilate_masks,
repair_defects, restore_video -> papof_defect_detect_tensor, papof_mask_dilate_tensor).  The device's mask, score and
support must be the BYTES of the numpy fp64 restatement (tests/_restore_ref.py), compared as raw bytes: uint8, float32 and
float64 frames of 1 .. 4 channels, NCHW, NHWC and strided views, float32 and float64 flows with NaNs, infinities and large
displacements, 3, 4 and 5 frames, one-row and one-column frames, the consistency check on and off, a threshold of 0, a
float32 score and absent outputs through the C ABI, a dense 1080p case; the dilation's bytes for radius 0 .. 32 on bool,
uint8 and strided masks; repair_defects and restore_video against their parts chained by hand, the caller's stream order,
and the calibration scene of tests/test_restore_cpu.py with the device's flows."""
import ctypes

import numpy as np
import pytest

from _restore_ref import detect_reference, dilate_reference, restore_reference
from test_gpu_denoise import _as_layout, _frames, _same_bytes
from test_gpu_tensors import _dev
from test_gpu_track import _fields
from test_restore_cpu import ESTIMATED, THR, UNJUDGED, defect_scene, figures, meets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (CONSISTENCY, complete_flows, detect_defects, dilate_masks, fill_holes,  # noqa: E402
                                             flow_video_fb, propagate, repair_defects, restore_video)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _check(got, want, what):
    mask, score, support = want
    assert got.mask.dtype == torch.bool and got.score.dtype == torch.float64 and got.support.dtype == torch.uint8
    _same_bytes(got.mask.view(torch.uint8), mask, None, what + " mask")
    _same_bytes(got.score, score, None, what + " score")
    _same_bytes(got.support, support, None, what + " support")


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    H, W = 37, 53
    for T, C in ((3, 3), (4, 1), (5, 4), (5, 2)):
        n = _frames(T, H, W, C, dtype, T + C)
        fw, bw = _fields(T, H, W, 2 + T)
        v = _as_layout(n, layout)
        for fdt in (torch.float64, torch.float32):
            tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
            nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
            for thr, cons in ((0.3, None), (0.3, CONSISTENCY), (0.0, CONSISTENCY)):
                got = detect_defects(v, tf, tb, threshold=thr, consistency=cons, layout=layout)
                _check(got, detect_reference(n, nf, nb, thr, cons), "%s %s T %d C %d flows %s thr %s check %s"
                       % (dtype, layout, T, C, fdt, thr, cons is not None))


def test_branches_are_reached():
    """the synthetic cases above take every branch of the rule: pixels flagged and not, judged and not (support 0, 1 and
    2) in the middle of the video and at both ends, hops that fail only the check, NaN and infinite flows"""
    T, H, W = 5, 37, 53
    n = _frames(T, H, W, 4, torch.uint8, T + 4)
    fw, bw = _fields(T, H, W, 2 + T)
    mask, score, sup = detect_reference(n, fw, bw, 0.3, CONSISTENCY)
    _, _, sup_nc = detect_reference(n, fw, bw, 0.3, None)
    for t in (0, 2, T - 1):
        assert set(np.unique(sup[t]).tolist()) == {0, 1, 2}, t
        assert mask[t].any() and (mask[t] == 0)[sup[t] == 2].any(), t
    assert (sup_nc > sup).any() and (score[sup == 2] > 0).any() and (score[sup < 2] == 0).all()
    assert (~np.isfinite(fw)).any() and (~np.isfinite(bw)).any()
    m0 = detect_reference(n, fw, bw, 0.0, CONSISTENCY)[0]
    assert (m0 > mask).any() and (m0 == 0)[sup == 2].any()  # a threshold of 0 flags every positive score, not a score of 0


@pytest.mark.parametrize("H,W", [(1, 70), (30, 1)])
def test_one_row_and_one_column(H, W):
    T, C = 4, 3
    n = _frames(T, H, W, C, torch.float32, 3)
    fw, bw = _fields(T, H, W, 4, wild=False)
    for f in (fw, bw):  # no motion across the single row or column, but for a few pixels that leave; NaN and infinite flows
        flat = f.reshape(T - 1, 2, -1)  # (a view: _fields returns contiguous arrays)
        flat[:, 1 if H == 1 else 0, 2:] = 0.0
        flat[:, :, 7] = np.nan
        flat[:, :, 11] = (np.inf, -np.inf)
    got = detect_defects(_as_layout(n, "NHWC"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), threshold=0.2,
                         consistency=CONSISTENCY, layout="NHWC")
    want = detect_reference(n, fw, bw, 0.2, CONSISTENCY)
    assert (want[2] == 2).any()
    _check(got, want, "%d x %d" % (H, W))


def test_strided_views():
    T, H, W, C = 4, 29, 41, 3
    fw, bw = _fields(T, H, W, 5)
    big = torch.from_numpy(_frames(2 * T, H + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    # flows as (T - 1, H, W, 2) channels-last, read as (T - 1, 2, H, W), and float32 backward flows
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    tb = torch.from_numpy(bw).float().cuda()
    want = detect_reference(v.cpu().numpy(), fw, tb.cpu().numpy(), 0.25, CONSISTENCY)
    _check(detect_defects(v, tf, tb, threshold=0.25, consistency=CONSISTENCY, layout="NHWC"), want, "strided NHWC")
    _check(detect_defects(v.permute(0, 3, 1, 2), tf, tb, threshold=0.25, consistency=CONSISTENCY), want, "strided NCHW")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(T, 2, H, W)  # one channel read twice: a zero stride
    want = detect_reference(v.cpu().numpy()[..., [1, 1]], fw, tb.cpu().numpy(), 0.25, None)
    _check(detect_defects(one, tf, tb, threshold=0.25), want, "expanded channel")


def test_float32_score_and_absent_outputs_through_the_c_abi():
    T, H, W, C = 3, 20, 66, 2
    n = _frames(T, H, W, C, torch.float64, 8)
    fw, bw = _fields(T, H, W, 9)
    want = detect_reference(n, fw, bw, 0.2, CONSISTENCY, np.float32)
    v, tf, tb = _dev(list(n)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    d_f = [tensors._flow_struct(f, capi.DTYPE_F64) for f in (tf, tb)]
    strided = torch.zeros((T, H, 2 * W), dtype=torch.uint8, device="cuda")  # the mask into every other column
    score = torch.zeros((T, H, W), dtype=torch.float32, device="cuda")
    for with_rest in (True, False):
        strided.zero_()
        d_m = tensors._mask_struct(strided[:, :, ::2])
        d_sc = tensors._struct(score, (H * W, W, 1, 0), capi.DTYPE_F32)
        rest = (ctypes.byref(d_sc), None) if with_rest else (None, None)
        tensors._launch(v.device, "papof_defect_detect_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_f[0]),
                        ctypes.byref(d_f[1]), 0.2, 1, *CONSISTENCY, ctypes.byref(d_m), *rest)
        _same_bytes(strided[:, :, ::2], want[0], None, "strided mask")
        assert not strided[:, :, 1::2].any()
    _same_bytes(score, want[1], None, "float32 score")


def test_dense_1080p():
    T, H, W, C = 3, 1080, 1920, 3
    n = _frames(T, H, W, C, torch.uint8, 10)
    g = torch.Generator().manual_seed(11)
    fw = torch.nn.functional.interpolate(torch.randn(T - 1, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 6,
                                         size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.3 * torch.randn(T - 1, 2, H, W, generator=g, dtype=torch.float64)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    got = detect_defects(_as_layout(n, "NHWC"), fw.cuda(), bw.cuda(), threshold=0.3, consistency=CONSISTENCY, layout="NHWC")
    _check(got, detect_reference(n, fw.numpy(), bw.numpy(), 0.3, CONSISTENCY), "1080p")


@pytest.mark.parametrize("radius", [0, 1, 2, 5, 16, 32])
def test_dilation(radius):
    rng = np.random.default_rng(20 + radius)
    for H, W in ((33, 70), (1, 5)):
        m = (rng.random((3, H, W)) < 0.01) * rng.integers(1, 256, (3, H, W))
        m[1] = 0
        m[2, H - 1, W - 1] = 255  # a corner; frame 1 stays empty
        m = m.astype(np.uint8)
        want = dilate_reference(m, radius)
        got = dilate_masks(torch.from_numpy(m).cuda(), radius)
        assert got.dtype == torch.bool and not got[1].any()
        _same_bytes(got.view(torch.uint8), want, None, "uint8 %d x %d" % (H, W))
        _same_bytes(dilate_masks(torch.from_numpy(m != 0).cuda(), radius).view(torch.uint8), want, None, "bool")
        big = torch.zeros((6, H + 2, 2 * W + 1), dtype=torch.uint8, device="cuda")
        view = big[::2, 1:H + 1, 1::2]
        view.copy_(torch.from_numpy(m))
        assert not view.is_contiguous()
        _same_bytes(dilate_masks(view, radius).view(torch.uint8), want, None, "strided")
        _same_bytes(dilate_masks(torch.from_numpy(m[0] != 0).cuda(), radius).view(torch.uint8), want[:1], None, "2-D")


def test_dilation_across_tiles():
    """masks wider than one 64-column word and taller than one 16-row tile: set pixels at the tiles' seams"""
    H, W = 40, 200
    m = np.zeros((2, H, W), np.uint8)
    for r, x in ((0, 63), (15, 64), (16, 127), (31, 128), (39, 199), (17, 0), (20, 96)):
        m[0, r, x] = 1
    m[1, ::7, ::31] = 3
    for radius in (1, 31, 32):
        _same_bytes(dilate_masks(torch.from_numpy(m).cuda(), radius).view(torch.uint8), dilate_reference(m, radius), None,
                    "radius %d" % radius)


def _by_hand(v, fw, bw, masks, dilate, layout, out_dtype=None):
    """repair_defects from the public calls"""
    given = torch.zeros(fw.shape[0] + 1, *fw.shape[2:], dtype=torch.bool, device=fw.device) if masks is None else masks != 0
    first = detect_defects(v, fw, bw, layout=layout).mask
    cf = complete_flows(fw, bw, dilate_masks(first | given, dilate))
    detected = first | detect_defects(v, cf.flow_fw, cf.flow_bw, layout=layout).mask
    m = dilate_masks(detected | given, dilate)
    cf = complete_flows(fw, bw, m)
    p = propagate(v, m, cf.flow_fw, cf.flow_bw, layout=layout, out_dtype=torch.float64)
    return fill_holes(p.video, p.status == 2, layout=layout, out_dtype=out_dtype or v.dtype), m, detected, p.status


@pytest.fixture(scope="module")
def scene():
    clean, damaged, truth, _, _ = defect_scene()
    return clean, damaged, truth, _dev(list(damaged))


def test_repair_defects_and_restore_video_are_their_parts(scene):
    _, damaged, _, v = scene
    fb = flow_video_fb(v, 4, layout="NHWC", consistency=None)
    given = torch.zeros(damaged.shape[:3], dtype=torch.uint8, device="cuda")
    given[3, 50:60, 90:100] = 7
    for masks, kw in ((None, {}), (given, dict(out_dtype=torch.float32))):
        r = repair_defects(v, fb.flow_fw, fb.flow_bw, masks=masks, layout="NHWC", **kw)
        video, m, detected, status = _by_hand(v, fb.flow_fw, fb.flow_bw, masks, tensors.DEFECT_DILATE, "NHWC", kw.get("out_dtype"))
        assert torch.equal(r.video, video) and torch.equal(r.masks, m) and torch.equal(r.detected, detected)
        assert torch.equal(r.status, status) and r.masks.dtype == torch.bool and r.detected.dtype == torch.bool
        assert r.video.dtype == kw.get("out_dtype", torch.uint8) and (masks is None or r.masks[3, 50:60, 90:100].all())
    r1 = repair_defects(v, fb.flow_fw, fb.flow_bw, layout="NHWC")
    assert torch.equal(r1.video[~r1.masks], v[~r1.masks])  # outside the repaired set: the input's bytes
    rv = restore_video(v, 4, layout="NHWC")
    assert torch.equal(rv.detected, r1.detected | rv.detected) and rv.video.dtype == torch.uint8
    fb2 = flow_video_fb(r1.video, 4, layout="NHWC", consistency=None)
    r2 = repair_defects(v, fb2.flow_fw, fb2.flow_bw, masks=r1.detected, layout="NHWC")
    assert torch.equal(rv.video, r2.video) and torch.equal(rv.masks, r2.masks) and torch.equal(rv.status, r2.status)
    assert torch.equal(rv.detected, r1.detected | r2.detected)
    assert torch.equal(rv.flow_fw, fb2.flow_fw) and torch.equal(rv.flow_bw, fb2.flow_bw) and sorted(rv.timing) == sorted(fb2.timing)
    one = restore_video(v.permute(0, 3, 1, 2), 4, passes=1)  # NCHW, one pass
    assert torch.equal(one.video.permute(0, 2, 3, 1), r1.video) and torch.equal(one.flow_fw, fb.flow_fw)


def test_the_scene_with_the_devices_flows(scene):
    """The calibration scene of tests/test_restore_cpu.py, restore_video at the defaults: the bytes of the restatement on
    the device's flows of each pass, and the bars calibrated there with the oracle's flows"""
    clean, damaged, truth, v = scene
    rv = restore_video(v, 4, layout="NHWC")
    r1 = restore_video(v, 4, layout="NHWC", passes=1)
    flows = iter([(r1.flow_fw.cpu().numpy(), r1.flow_bw.cpu().numpy()), (rv.flow_fw.cpu().numpy(), rv.flow_bw.cpu().numpy())])
    video, m, detected, status, _ = restore_reference(damaged, lambda _: next(flows), 2, threshold=THR, dilate=tensors.DEFECT_DILATE)
    _same_bytes(rv.video, video, "NHWC", "restore_video")
    _same_bytes(rv.masks.view(torch.uint8), m.astype(np.uint8), None, "restore_video masks")
    _same_bytes(rv.detected.view(torch.uint8), detected.astype(np.uint8), None, "restore_video detected")
    _same_bytes(rv.status, status, None, "restore_video status")
    for k, r in ((1, r1), (2, rv)):
        got = figures(r.video.cpu().numpy(), r.detected.cpu().numpy(), clean, damaged, truth)
        print("the device's flows, %d pass(es): recall %.4f, significant %.4f, false alarms %.5f, PSNR %.2f dB over the "
              "defects, %.2f dB whole" % ((k,) + got))
        meets(got, ESTIMATED[k])
    sup = detect_defects(v, rv.flow_fw, rv.flow_bw, layout="NHWC").support
    assert float((sup < 2).float().mean()) < UNJUDGED


def test_the_calls_are_ordered_on_the_callers_stream():
    """Frames and masks written on a side stream behind a long sleep, detected and dilated under that stream with no
    synchronisation: the kernels must read them after they are written, and what is queued behind them must see their
    outputs"""
    import time
    T, H, W, C = 4, 40, 60, 3
    n = _frames(T, H, W, C, torch.uint8, 12)
    fw, bw = _fields(T, H, W, 13)
    want = detect_reference(n, fw, bw, 0.3, CONSISTENCY)
    grown = dilate_reference(want[0], 3)
    src = _dev(list(n))
    dst = torch.zeros_like(src)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = dilate_masks(detect_defects(dst, tf, tb, layout="NHWC").mask, 3).clone()
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        dst.copy_(src)
        got = detect_defects(dst, tf, tb, threshold=0.3, consistency=CONSISTENCY, layout="NHWC")
        big = dilate_masks(got.mask, 3)  # queued behind the detector on the same stream
        copy = big.clone()
    side.synchronize()
    _check(got, want, "side stream")
    _same_bytes(big.view(torch.uint8), grown, None, "side stream dilation")
    _same_bytes(copy.view(torch.uint8), grown, None, "side stream clone")
