"""Rotation-path stabilization on device tensors (papteam_opticalflow_amd/tensors.py: warp_rows, camera_rotations,
stabilize_video_rotation -> papof_warp_rows_tensor).  The device's video and valid mask must be the BYTES of the numpy fp64
restatement (tests/_rows_ref.py), compared as raw bytes: 1 .. 4 channels, uint8, float32 and float64, NCHW, NHWC, strided
views, float32 and float64 tables, contiguous or not, 1, 2, 3, 17 and H knots, 1, 3 and 8 iterations, every output dtype, an
absent valid and a strided out through the C ABI, one-pixel, one-row, two-row, tiny and tile-crossing frames, a 1080p frame;
hostile tables -- a NaN knot, a horizon across the frame, iterates far outside, the last interval hit exactly -- that
together take every branch of the rule; Kn = 1 and equal knots against warp_homography; the public chain against its parts
chained by hand; the picture scene of tests/test_rows_cpu.py with the device's flows; the second launch of the split grid;
every refusal of the C ABI on a live handle; the caller's stream order."""
import ctypes
import itertools

import numpy as np
import pytest

from _rows_ref import BRANCHES, warp_rows_reference
from test_gpu_denoise import _as_layout, _frames, _same_bytes
from test_gpu_tensors import _dev
from test_rows_cpu import (CHAIN_MEASURED, F_SCENE, H_SCENE, RADIUS_PIC, READOUT_PIC, ROWS_REFUSALS, W_SCENE, hostile_tables,
                           picture_scene, psnr, rows_call, some_tables)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (camera_rotations, flow_video, flow_video_fb, rotation_rows,  # noqa: E402
                                             smooth_rotations, stabilize_video_rotation, warp_homography, warp_rows)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, None: None}
ITERS = (1, 3, 8)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _check_frames(got, want, layout, what):
    video, valid = got
    assert valid.dtype == torch.bool
    _same_bytes(video, want[0], layout, what + " video")
    _same_bytes(valid, want[1], None, what + " valid")


def _knots(H):
    return (1, 2, 3, 17, H)


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_every_dtype_channel_count_knot_count_and_iteration_count(dtype, layout):
    B, H, W = 3, 19, 53
    odts = (None, torch.uint8, torch.float32, torch.float64)
    seen = {k: set() for k in ("mdt", "odt")}
    for j, (C, Kn, iters) in enumerate(itertools.product((1, 2, 3, 4), _knots(H), ITERS)):
        mdt, odt = (torch.float64, torch.float32)[(j // 2) % 2], odts[(j + C) % 4]
        n = _frames(B, H, W, C, dtype, C + Kn)
        tab = torch.from_numpy(some_tables(B, Kn, H, W, 3 + Kn + iters)).to(mdt).cuda()
        what = "%s %s C %d Kn %d iters %d table %s out %s" % (dtype, layout, C, Kn, iters, mdt, odt)
        got = warp_rows(_as_layout(n, layout), tab, iters=iters, layout=layout, out_dtype=odt)
        want = warp_rows_reference(n, tab.cpu().numpy(), iters, _NP[odt])
        assert want[1].any() and not want[1].all(), what
        _check_frames(got, want, layout, what)
        assert got[0].dtype == (odt or dtype)
        seen["mdt"].add(mdt)
        seen["odt"].add(odt)
    assert seen == dict(mdt={torch.float32, torch.float64}, odt=set(odts))


@pytest.mark.parametrize("H,W,knots", [(1, 1, (1,)), (1, 9, (1,)), (2, 1, (1, 2)), (5, 7, (1, 2, 3, 5)), (9, 130, (1, 2, 3, 9)),
                                       (6, 65, (1, 2, 6))])
def test_edge_shapes(H, W, knots):
    """one pixel and one row (Kn = 1 only), two rows of one pixel (Kn = 2 at its smallest), a frame smaller than a tile, and two
    that cross the 64-column and 4-row tile seams"""
    B, C = 2, 3
    n = _frames(B, H, W, C, torch.float32, 3)
    for Kn in knots:
        for iters in ITERS if Kn > 1 else (3,):
            M = some_tables(B, Kn, H, W, 5 + Kn, shift=0.4 if min(H, W) <= 2 else 1.5)
            if min(H, W) <= 2:  # whole-pixel shifts along the long axis: anything else leaves a one-pixel-wide frame everywhere
                M[:] = np.eye(3)
                M[:, :, 0, 2], M[:, :, 1, 2] = (W > 2) * 1.0, 0.0
            if Kn > 1:
                M[1, -1, 1, 2] += 0.5  # the last knot differs
            got = warp_rows(_as_layout(n, "NHWC"), torch.from_numpy(M).cuda(), iters=iters, layout="NHWC")
            want = warp_rows_reference(n, M, iters)
            assert want[1].any(), (H, W, Kn)
            _check_frames(got, want, "NHWC", "%d x %d Kn %d iters %d" % (H, W, Kn, iters))


def test_a_1080p_frame():
    H, W, C, Kn = 1080, 1920, 3, 17
    n = _frames(1, H, W, C, torch.uint8, 10)
    M = some_tables(1, Kn, H, W, 11, shift=6.0)
    got = warp_rows(_as_layout(n, "NHWC"), torch.from_numpy(M).cuda(), layout="NHWC")
    want = warp_rows_reference(n, M)
    assert 0.8 < want[1].mean() < 1
    _check_frames(got, want, "NHWC", "1080p")
    again = warp_rows(_as_layout(n, "NHWC"), torch.from_numpy(M).cuda(), layout="NHWC")  # two runs, the same bytes
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float64])
def test_hostile_tables_and_every_branch(dtype):
    H, W, C = 19, 53, 2
    n = _frames(1, H, W, C, dtype, 12)
    total = dict.fromkeys(BRANCHES, 0)
    for name, tab in hostile_tables(H, W).items():
        for iters in ITERS:
            got = warp_rows(_as_layout(n, "NCHW"), torch.from_numpy(tab).cuda(), iters=iters)
            out, valid, _, seen = warp_rows_reference(n, tab, iters, parts=True)
            _check_frames(got, (out, valid), "NCHW", "hostile table %s, %d iterations" % (name, iters))
            for k in BRANCHES:
                total[k] += seen[k]
    assert sorted(total) == sorted(BRANCHES) and all(total.values()), total


def test_strided_views_and_a_table_that_is_not_contiguous():
    B, H, W, C, Kn = 4, 29, 41, 3, 5
    big = torch.from_numpy(_frames(2 * B, H + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    M = some_tables(B + 2, Kn, H, W, 7)
    tab = torch.from_numpy(np.ascontiguousarray(M.transpose(0, 3, 2, 1))).cuda().permute(0, 3, 2, 1)[1:-1]  # knots innermost
    assert not tab.is_contiguous() and tuple(tab.shape) == (B, Kn, 3, 3)
    want = warp_rows_reference(v.cpu().numpy(), M[1:-1])
    _check_frames(warp_rows(v, tab, layout="NHWC"), want, "NHWC", "strided NHWC")
    _check_frames(warp_rows(v.permute(0, 3, 1, 2), tab), want, "NCHW", "strided NCHW")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(B, 2, H, W)  # one channel read twice: a zero stride
    same = tab[:1].expand(B, Kn, 3, 3)                      # one frame's table for every frame
    want = warp_rows_reference(v.cpu().numpy()[..., [1, 1]], np.repeat(M[1:2], B, 0), 8)
    _check_frames(warp_rows(one, same, iters=8), want, "NCHW", "expanded channel and table")


def test_valid_absent_and_a_strided_out_through_the_c_abi():
    B, H, W, C, Kn = 3, 20, 66, 2, 3
    n = _frames(B, H, W, C, torch.float64, 8)
    M = some_tables(B, Kn, H, W, 9)
    v, tab = _dev(list(n)), torch.from_numpy(M).float().cuda()
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    d_tab = tensors._struct(tab, tuple(tab.stride()), capi.DTYPE_F32)
    strided = torch.zeros((B, H, 2 * W, C), dtype=torch.float32, device="cuda")  # the video into every other column
    view = strided[:, :, ::2]
    d_out = tensors._struct(view, *tensors.descriptor(view, "NHWC")[1:])
    valid = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    d_valid = tensors._struct(valid, (H * W, W, 1, 0), capi.DTYPE_U8)
    want = warp_rows_reference(n, tab.cpu().numpy(), 3, np.float32)
    for with_valid in (True, False):
        strided.zero_()
        valid.fill_(7)
        tensors._launch(v.device, "papof_warp_rows_tensor", B, H, W, C, ctypes.byref(d_in), ctypes.byref(d_tab), Kn, 3,
                        ctypes.byref(d_out), ctypes.byref(d_valid) if with_valid else None)
        _same_bytes(view, want[0], "NHWC", "strided video")
        assert not strided[:, :, 1::2].any()
        if with_valid:
            _same_bytes(valid.view(torch.bool), want[1], None, "valid")
        else:
            assert (valid == 7).all()


def test_one_knot_is_warp_homography_and_equal_knots_are_one_knot():
    B, H, W, C = 4, 37, 70, 3
    M = some_tables(B, 1, H, W, 13)
    M[1, 0, 2, 0] = -2.0 / W  # a horizon across a frame
    M[2, 0, 0, 0] = np.nan
    assert not np.signbit(M).any() or (M[np.signbit(M)] != 0).all()  # no negative zeros
    for dtype in (torch.uint8, torch.float32, torch.float64):
        n = _frames(B, H, W, C, dtype, 14)
        if dtype == torch.uint8:
            n.reshape(-1)[:256] = np.arange(256)  # every byte value occurs
        v = _as_layout(n, "NHWC")
        for mdt in (torch.float64, torch.float32):
            tab = torch.from_numpy(M).to(mdt).cuda()
            for odt in (None, torch.uint8, torch.float64):
                want = warp_homography(v, tab[:, 0], layout="NHWC", out_dtype=odt)
                assert bool(want[1].any()) and not bool(want[1].all()) and not bool(want[1][2].any())
                got = warp_rows(v, tab, iters=1, layout="NHWC", out_dtype=odt)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                for Kn, iters in ((2, 1), (5, 3), (H, 8)):
                    same = warp_rows(v, tab.expand(B, Kn, 3, 3), iters=iters, layout="NHWC", out_dtype=odt)
                    assert torch.equal(same[0], want[0]) and torch.equal(same[1], want[1]), (dtype, mdt, odt, Kn)


def _small_video(T=6, H=48, W=64, f=80.0):
    """frames rendered from the committed frame through a rotating camera with a rolling shutter (test_rows_cpu's renderer)"""
    import cases
    import _rows_ref as RR
    img = cases.load_frame_u8("960", 1).astype(np.float64)
    Rf = RR.shaken_path((12.0, 7.0), amp=0.04)
    tau = RR.row_times(H, 0.8)
    return np.stack([RR.render(img, Rf(t + tau), f, H, W, 2 * f) for t in range(T)])


def test_the_public_chain_is_its_parts():
    n = _small_video()
    T, H, W, _ = n.shape
    v = _dev(list(n))
    # readout 0: flow_video, the plain chain, and warp_homography of rotation_rows' single matrix
    for kw in (dict(focal=80.0), dict(focal=75.0, radius=2, crop=0.9, knots=5, iters=1, fit_iters=3, scale=2.0, bundle_iters=4,
                                      out_dtype=torch.float64)):
        sv = stabilize_video_rotation(v, 2, layout="NHWC", **kw)
        flow, _, timing = flow_video(v, 2, layout="NHWC", out_dtype=torch.float64)
        cam = camera_rotations(flow, (H, W), focal=kw["focal"], iters=kw.get("fit_iters", 5), scale=kw.get("scale", 1.0),
                               bundle_iters=kw.get("bundle_iters", 10))
        S = smooth_rotations(cam.rotations, kw.get("radius", 15))
        tab = rotation_rows(cam.rotations, S, cam.focal, (H, W), 0.0, knots=kw.get("knots", 17), crop=kw.get("crop", 1.0))
        assert tuple(tab.shape) == (T, 1, 3, 3) and torch.equal(sv.tables, tab) and sv.focal == kw["focal"]
        video, valid = warp_homography(v, tab[:, 0], layout="NHWC", out_dtype=kw.get("out_dtype"))
        assert torch.equal(sv.video, video) and torch.equal(sv.valid, valid) and sv.video.dtype == kw.get("out_dtype", torch.uint8)
        assert torch.equal(sv.rotations, cam.rotations) and torch.equal(sv.smoothed, S)
        assert torch.equal(sv.motion, cam.motion) and torch.equal(sv.ok, cam.ok) and bool(sv.ok.all())
        assert sv.flow.cpu().numpy().tobytes() == flow.cpu().numpy().tobytes() and sorted(sv.timing) == sorted(timing)
        assert bool(valid.any())
    # readout 0.8: flow_video_fb, the rectified flows under their mask, one warp_rows
    for kw in (dict(focal=80.0), dict(focal=80.0, anchor=0.0, rs_iters=2, radius=3, knots=9, iters=2, out_dtype=torch.float32)):
        sv = stabilize_video_rotation(v.permute(0, 3, 1, 2), 2, readout=0.8, **kw)
        fb = flow_video_fb(v, 2, layout="NHWC", consistency=None, out_dtype=torch.float64)
        cam = camera_rotations(fb.flow_fw, (H, W), flow_bw=fb.flow_bw, readout=0.8, anchor=kw.get("anchor", 0.5),
                               rs_iters=kw.get("rs_iters", 3), focal=80.0)
        S = smooth_rotations(cam.rotations, kw.get("radius", 15))
        tab = rotation_rows(cam.rotations, S, cam.focal, (H, W), 0.8, anchor=kw.get("anchor", 0.5), knots=kw.get("knots", 17))
        assert tuple(tab.shape) == (T, kw.get("knots", 17), 3, 3) and torch.equal(sv.tables, tab)
        video, valid = warp_rows(v.permute(0, 3, 1, 2), tab, iters=kw.get("iters", 3), out_dtype=kw.get("out_dtype"))
        assert torch.equal(sv.video, video) and torch.equal(sv.valid, valid) and sv.video.dtype == kw.get("out_dtype", torch.uint8)
        assert torch.equal(sv.rotations, cam.rotations) and torch.equal(sv.smoothed, S) and torch.equal(sv.motion, cam.motion)
        assert sv.flow.cpu().numpy().tobytes() == fb.flow_fw.cpu().numpy().tobytes() and sorted(sv.timing) == sorted(fb.timing)
        want = warp_rows_reference(n, tab.cpu().numpy(), kw.get("iters", 3), _NP[kw.get("out_dtype")])
        _check_frames((sv.video, sv.valid), want, "NCHW", "stabilize_video_rotation")
    again = stabilize_video_rotation(v.permute(0, 3, 1, 2), 2, readout=0.8, **kw)  # two runs, the same bytes
    assert torch.equal(again.video, sv.video) and torch.equal(again.valid, sv.valid) and torch.equal(again.tables, sv.tables)


def pictures_bar():
    """the least PSNR with the device's flows: halfway between the unstabilized video's and the one measured with the oracle's
    flows in tests/test_rows_cpu.py -- the slack is for the device's flows differing from the oracle's"""
    return 0.5 * (CHAIN_MEASURED[0] + CHAIN_MEASURED[2])


def test_the_pictures_with_the_devices_flows():
    """The picture scene of tests/test_rows_cpu.py, stabilize_video_rotation with nothing given but readout and the radius: the
    bytes of the restatement on the device's tables, and the bar set there with the oracle's flows (33.91 dB, 18.40 dB
    unstabilized: the bar is 26.15 dB; 33.89 dB came out here, with the oracle's focal length of 646.7 px)"""
    _, rolling, _, _, truth = picture_scene()
    sv = stabilize_video_rotation(_dev(list(rolling)), 4, readout=READOUT_PIC, radius=RADIUS_PIC, layout="NHWC")
    want = warp_rows_reference(rolling, sv.tables.cpu().numpy())
    _check_frames((sv.video, sv.valid), want, "NHWC", "stabilize_video_rotation on the pictures")
    valid = sv.valid.cpu().numpy()
    got, before = psnr(sv.video.cpu().numpy(), truth, valid), psnr(rolling, truth, valid)
    print("pictures with the device's flows: %.2f dB (unstabilized %.2f dB, bar %.2f dB) over %.3f of the interior pixels; focal "
          "%.1f px of %.1f" % (got, before, pictures_bar(), valid[1:-1].mean(), sv.focal, F_SCENE))
    assert tuple(sv.tables.shape) == (len(rolling), 17, 3, 3) and (H_SCENE, W_SCENE) == rolling.shape[1:3]
    assert valid[1:-1].mean() > 0.9 and got >= pictures_bar()


def test_the_second_launch_of_the_split_grid():
    """65535 + 2 frames of 2 x 3 with two knots: the frames and tables are periodic with every item in memory of its own, and
    every item of both launches has the bytes of its base item's restatement"""
    from _seam import N_TILES, P, TILES_CUT, expand, frames, gather, index, same_bytes
    H, W, C = 2, 3, 2
    f = frames(P, H, W, C, 57)
    M = some_tables(P, 2, H, W, 58, shift=0.3)
    assert TILES_CUT % P != 0  # the first item of the second launch is not item 0
    idx = index(N_TILES, P)
    out, valid = warp_rows_reference(f, M, 3)
    assert valid.any()
    got = warp_rows(gather(f, idx), gather(M, idx), layout="NHWC")
    same_bytes(got[0], expand(out, idx), "warp_rows video", TILES_CUT)
    same_bytes(got[1].view(torch.uint8), expand(valid.astype(np.uint8), idx), "warp_rows valid", TILES_CUT)


@pytest.mark.parametrize("kw", ROWS_REFUSALS)
def test_the_c_abi_refuses_on_a_live_handle(gpu, kw):
    """PAPOF_EINVAL before anything is enqueued: the descriptors point at no memory"""
    assert rows_call(gpu.L, gpu.h, **kw) == -1


def test_python_argument_errors_launch_nothing():
    v = torch.zeros((2, 3, 8, 8), device="cuda")
    tab = torch.eye(3, dtype=torch.float64, device="cuda").expand(2, 3, 3, 3)
    for call, exc in ((lambda: warp_rows(v, tab.cpu()), ValueError), (lambda: warp_rows(v.cpu(), tab), ValueError),
                      (lambda: warp_rows(v, tab[:1]), ValueError), (lambda: warp_rows(v, tab, iters=0), ValueError),
                      (lambda: warp_rows(v, tab.half()), TypeError), (lambda: warp_rows(v[:, :, :1], tab), ValueError),
                      (lambda: stabilize_video_rotation(v, 2, readout=0.5, knots=9), ValueError),
                      (lambda: stabilize_video_rotation(v, 2, focal=0.0), ValueError),
                      (lambda: camera_rotations(torch.zeros((1, 2, 8, 8), device="cuda"), (8, 8), readout=0.5), ValueError)):
        with pytest.raises(exc):
            call()


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames and tables written on a side stream behind a long sleep, warped under that stream with no synchronisation: the
    kernel must read them after they are written, and what is queued behind it must see its outputs"""
    import time
    B, H, W, C, Kn = 4, 40, 60, 3, 5
    n = _frames(B, H, W, C, torch.uint8, 12)
    M = some_tables(B, Kn, H, W, 13)
    want = warp_rows_reference(n, M)
    src, sm = _dev(list(n)), torch.from_numpy(M).cuda()
    dst, tm = torch.zeros_like(src), torch.zeros_like(sm)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = warp_rows(dst, tm, layout="NHWC")[0].clone()
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the call
        dst.copy_(src)
        tm.copy_(sm)
        got = warp_rows(dst, tm, layout="NHWC")
        copy = got[0].clone()  # queued behind the kernel on the same stream
    side.synchronize()
    _check_frames(got, want, "NHWC", "side stream")
    _same_bytes(copy, want[0], "NHWC", "side stream clone")
