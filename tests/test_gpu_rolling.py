"""Rolling-shutter rectification on device tensors (papteam_opticalflow_amd/tensors.py: rectify_frames, rectify_flows,
rectify_video, stabilize_video_rs -> papof_rs_rectify_tensor, papof_rs_flow_tensor).  The device's video, valid mask and
flows must be the BYTES of the numpy fp64 restatement (tests/_rolling_ref.py), compared as raw bytes: 2, 3 and 5 frames of
1 .. 4 channels, uint8, float32 and float64, NCHW, NHWC, strided and expanded views, float32 and float64 flows with NaNs,
infinities and 900-pixel entries, readout 0.8, -0.6 and 0, anchor 0, 0.5 and 1, 1, 3 and 8 iterations, with and without
matrices, every output dtype, an absent valid and a strided out through the C ABI, one-row, one-column, tiny and
tile-crossing frames, a dense 1080p case; that those cases reach every branch of the rule; readout = 0 against warp_affine;
the public chains against their parts chained by hand; the picture scene of tests/test_rolling_cpu.py with the device's
flows; the caller's stream order."""
import ctypes
import itertools

import numpy as np
import pytest

from _rolling_ref import BRANCHES, flows_reference, rectify_reference
from test_gpu_denoise import _as_layout, _frames, _same_bytes
from test_gpu_tensors import _dev
from test_gpu_track import _fields
from test_rolling_cpu import READOUT_PIC, picture_scene, pictures_bar, psnr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (CONSISTENCY, fb_consistency, flow_video_fb, global_motion,  # noqa: E402
                                             rectify_flows, rectify_frames, rectify_video, stabilize_video_rs,
                                             stabilizing_transforms, warp_affine)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, None: None}
READOUTS, ANCHORS, ITERS = (0.8, -0.6, 0.0), (0.0, 0.5, 1.0), (1, 3, 8)
SHAPES = ((2, 3), (3, 1), (5, 4), (3, 2))  # (T, C): T = 2 is two end frames


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _rs_fields(T, H, W, seed, wild=True):
    """test_gpu_track's flow pairs (NaNs, infinities, a patch of large displacements) with 900-pixel entries of both signs
    in both flows: vertical ones fail the rule's guards on tf and tb for a readout of either sign"""
    fw, bw = _fields(T, H, W, seed, amp=3.0, wild=wild)
    n = H * W
    for k, f in enumerate((fw, bw)):
        flat = f.reshape(T - 1, 2, n)  # (a view: _fields returns contiguous arrays)
        for j, val in enumerate((900.0, -900.0)):
            flat[:, 1, (5 + 17 * j + 3 * k) % n] = val
            flat[:, 0, (11 + 23 * j + 3 * k) % n] = val
    return fw, bw


def _matrices(T, H, W, seed):
    """small rotations, scales and shifts about the centre, (T, 2, 3)"""
    rng = np.random.default_rng(seed)
    M = np.empty((T, 2, 3))
    cx, cy = (W - 1) / 2, (H - 1) / 2
    for i in range(T):
        th, s = rng.normal(0, 0.05), 1 + rng.normal(0, 0.05)
        a, b = s * np.cos(th), s * np.sin(th)
        t = rng.normal(0, 1.5, 2)
        M[i] = [[a, -b, cx - a * cx + b * cy + t[0]], [b, a, cy - b * cx - a * cy + t[1]]]
    return M


def _check_frames(got, want, layout, what):
    video, valid = got
    assert valid.dtype == torch.bool
    _same_bytes(video, want[0], layout, what + " video")
    _same_bytes(valid, want[1], None, what + " valid")


def _check_flows(got, want, what):
    _same_bytes(got.flow_fw, want[0], None, what + " flow_fw")
    _same_bytes(got.flow_bw, want[1], None, what + " flow_bw")


def _sweep(dtype):
    """the cases of test_synthetic_flows_every_dtype for one frame dtype: every (T, C) with every (readout, anchor, iters),
    the flows' dtype, the matrices and the output dtype rotating through their values"""
    odts = (None, torch.uint8, torch.float32, torch.float64)
    for (T, C), (k, (readout, anchor, iters)) in itertools.product(SHAPES, enumerate(itertools.product(READOUTS, ANCHORS, ITERS))):
        j = k + T + C
        yield T, C, readout, anchor, iters, (torch.float64, torch.float32)[(j // 3) % 2], bool((j // 2) % 2), odts[j % 4]


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    H, W = 19, 53
    seen = {k: set() for k in ("iters", "fdt", "mats", "odt")}
    for T, C, readout, anchor, iters, fdt, mats, odt in _sweep(dtype):
        n = _frames(T, H, W, C, dtype, T + C)
        fw, bw = _rs_fields(T, H, W, 2 + T)
        tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
        mdt = torch.float32 if iters == 3 else torch.float64
        tm = torch.from_numpy(_matrices(T, H, W, 3 + T)).to(mdt).cuda() if mats else None
        what = "%s %s T %d C %d readout %s anchor %s iters %d flows %s matrices %s out %s" % (
            dtype, layout, T, C, readout, anchor, iters, fdt, mats and mdt, odt)
        got = rectify_frames(_as_layout(n, layout), tf, tb, readout, anchor=anchor, iters=iters, matrices=tm, layout=layout,
                             out_dtype=odt)
        want = rectify_reference(n, nf, nb, readout, anchor, iters, None if tm is None else tm.cpu().numpy(), _NP[odt])
        _check_frames(got, want, layout, what)
        assert got[0].dtype == (odt or dtype)
        for k, v in (("iters", iters), ("fdt", fdt), ("mats", mats), ("odt", odt)):
            seen[k].add(v)
    assert seen == dict(iters=set(ITERS), fdt={torch.float32, torch.float64}, mats={False, True},
                        odt={None, torch.uint8, torch.float32, torch.float64})


@pytest.mark.parametrize("fdt", [torch.float64, torch.float32])
def test_rectified_flows(fdt):
    H, W = 19, 53
    for T in (2, 3, 5):
        fw, bw = _rs_fields(T, H, W, 2 + T)
        tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
        nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
        for k, (readout, anchor) in enumerate(itertools.product(READOUTS, ANCHORS)):
            iters = ITERS[(k + T) % 3]
            odt = (None, torch.float32, torch.float64)[(k + T) % 3]
            got = rectify_flows(tf, tb, readout, anchor=anchor, iters=iters, out_dtype=odt)
            assert got.flow_fw.dtype == got.flow_bw.dtype == (odt or fdt)
            want = flows_reference(nf, nb, readout, anchor, iters, _NP[odt or fdt])
            assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()
            _check_flows(got, want, "flows %s T %d readout %s anchor %s iters %d out %s" % (fdt, T, readout, anchor, iters, odt))


def test_branches_are_reached():
    """the synthetic cases above take every branch of the rule: the anchor row and readout = 0 (s == 0), each of the two
    guards failing, an iterate that leaves the image, both end-frame forms and the interior one -- in frames and in flows"""
    H, W = 19, 53
    total = dict.fromkeys(BRANCHES, 0)
    for T in (2, 3, 5):
        fw, bw = _rs_fields(T, H, W, 2 + T)
        assert (~np.isfinite(fw)).any() and (~np.isfinite(bw)).any() and (np.abs(fw) == 900).any() and (np.abs(bw) == 900).any()
        n = _frames(T, H, W, 1, torch.float64, T + 1)
        for readout in (0.8, -0.6):
            _, valid, P, seen = rectify_reference(n, fw, bw, readout, 0.5, 3, parts=True)
            assert valid.any() and (~valid).any()
            *_, fseen = flows_reference(fw, bw, readout, 0.5, 3, parts=True)
            for s in (seen, fseen):
                assert s["s_zero"] and s["left"] and s["first"] and s["last"] and (T == 2 or s["interior"]), (T, readout, s)
                for k in BRANCHES:
                    total[k] += s[k]
    assert all(total.values()), total
    _, valid, _, seen = rectify_reference(n, fw, bw, 0.0, 0.5, 3, parts=True)
    assert valid.all() and seen["s_zero"] == 3 * n[..., 0].size and sum(seen.values()) == seen["s_zero"]


def _edge_fields(T, H, W):
    """_rs_fields with little motion across a single row or column -- whole pixels, mostly none --, so that points stay in
    the image, and a NaN and infinities"""
    fw, bw = _rs_fields(T, H, W, 4, wild=False)
    for f in (fw, bw):
        flat = f.reshape(T - 1, 2, -1)
        if H <= 2:
            flat[:, 1] = np.round(flat[:, 1] / 8.0)
        if W <= 3:
            flat[:, 0] = np.round(flat[:, 0] / 8.0)
        if flat.shape[2] > 29:
            flat[:, :, 21] = np.nan
            flat[:, :, 29] = (np.inf, -np.inf)
    return fw, bw


@pytest.mark.parametrize("H,W", [(1, 70), (30, 1), (2, 3), (9, 130)])
def test_edge_shapes(H, W):
    """one row (the identity: a = 0 and every s is 0), one column, a frame smaller than a tile, and one that crosses the
    64-column and 4-row tile seams"""
    T, C = 3, 3
    n = _frames(T, H, W, C, torch.float32, 3)
    fw, bw = _edge_fields(T, H, W)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    M = _matrices(T, H, W, 5)
    if min(H, W) <= 3:  # whole-pixel shifts along the long axes: a rotation would leave a one-pixel-wide image everywhere
        M[:] = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
        M[:, 0, 2], M[:, 1, 2] = (np.arange(T) - 1) * (W > 3), (1 - np.arange(T)) * (H > 3)
    tm = torch.from_numpy(M).cuda()
    for readout in (0.8, -0.6):
        for mats in (None, tm):
            got = rectify_frames(_as_layout(n, "NHWC"), tf, tb, readout, matrices=mats, layout="NHWC")
            want = rectify_reference(n, fw, bw, readout, matrices=None if mats is None else mats.cpu().numpy())
            _check_frames(got, want, "NHWC", "%d x %d readout %s matrices %s" % (H, W, readout, mats is not None))
            if H == 1 and mats is None:
                assert want[0].tobytes() == n.tobytes() and want[1].all()
        _check_flows(rectify_flows(tf, tb, readout, anchor=0.25), flows_reference(fw, bw, readout, 0.25), "%d x %d flows" % (H, W))


def test_strided_views():
    T, H, W, C = 5, 29, 41, 3
    fw, bw = _rs_fields(T, H, W, 5)
    big = torch.from_numpy(_frames(2 * T, H + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    # flows as (T - 1, H, W, 2) channels-last, read as (T - 1, 2, H, W), and float32 backward flows
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    tb = torch.from_numpy(bw).float().cuda()
    nb = tb.cpu().numpy()
    M = _matrices(T + 2, H, W, 7)
    tm = torch.from_numpy(M).cuda()[1:-1].transpose(1, 2).contiguous().transpose(1, 2)  # a slice, columns before rows
    want = rectify_reference(v.cpu().numpy(), fw, nb, 0.8, 0.5, 3, M[1:-1])
    _check_frames(rectify_frames(v, tf, tb, 0.8, matrices=tm, layout="NHWC"), want, "NHWC", "strided NHWC")
    _check_frames(rectify_frames(v.permute(0, 3, 1, 2), tf, tb, 0.8, matrices=tm), want, "NCHW", "strided NCHW")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(T, 2, H, W)  # one channel read twice: a zero stride
    want = rectify_reference(v.cpu().numpy()[..., [1, 1]], fw, nb, -0.6, 1.0, 8)
    _check_frames(rectify_frames(one, tf, tb, -0.6, anchor=1.0, iters=8), want, "NCHW", "expanded channel")
    same = tf[:1].expand(T - 1, 2, H, W)  # one pair's flow for every pair
    _check_flows(rectify_flows(same, tb, 0.8), flows_reference(np.repeat(fw[:1], T - 1, 0), nb, 0.8), "expanded flows")
    _check_flows(rectify_flows(tf, tb, -0.6, out_dtype=torch.float32), flows_reference(fw, nb, -0.6, out_dtype=np.float32),
                 "strided flows")


def test_valid_absent_and_strided_outputs_through_the_c_abi():
    T, H, W, C = 3, 20, 66, 2
    n = _frames(T, H, W, C, torch.float64, 8)
    fw, bw = _rs_fields(T, H, W, 9)
    v, tf, tb = _dev(list(n)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    d_f = [tensors._flow_struct(f, capi.DTYPE_F64) for f in (tf, tb)]
    strided = torch.zeros((T, H, 2 * W, C), dtype=torch.float32, device="cuda")  # the video into every other column
    view = strided[:, :, ::2]
    d_out = tensors._struct(view, *tensors.descriptor(view, "NHWC")[1:])
    valid = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
    d_valid = tensors._struct(valid, (H * W, W, 1, 0), capi.DTYPE_U8)
    want = rectify_reference(n, fw, bw, 0.8, 0.5, 3, out_dtype=np.float32)
    for with_valid in (True, False):
        strided.zero_()
        valid.fill_(7)
        tensors._launch(v.device, "papof_rs_rectify_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_f[0]),
                        ctypes.byref(d_f[1]), 0.8, 0.5, 3, None, ctypes.byref(d_out), ctypes.byref(d_valid) if with_valid else None)
        _same_bytes(view, want[0], "NHWC", "strided video")
        assert not strided[:, :, 1::2].any()
        if with_valid:
            _same_bytes(valid.view(torch.bool), want[1], None, "valid")
        else:
            assert (valid == 7).all()
    # the flows into the even columns of wider tensors, forward float32 and backward float64
    wide = [torch.zeros((T - 1, 2, H, 2 * W), dtype=dt, device="cuda") for dt in (torch.float32, torch.float64)]
    d_o = [tensors._flow_struct(w[..., ::2], c) for w, c in zip(wide, (capi.DTYPE_F32, capi.DTYPE_F64))]
    tensors._launch(v.device, "papof_rs_flow_tensor", T, H, W, ctypes.byref(d_f[0]), ctypes.byref(d_f[1]), -0.6, 1.0, 8,
                    ctypes.byref(d_o[0]), ctypes.byref(d_o[1]))
    _same_bytes(wide[0][..., ::2], flows_reference(fw, bw, -0.6, 1.0, 8, np.float32)[0], None, "strided flow_fw")
    _same_bytes(wide[1][..., ::2], flows_reference(fw, bw, -0.6, 1.0, 8)[1], None, "strided flow_bw")
    assert not wide[0][..., 1::2].any() and not wide[1][..., 1::2].any()


def test_dense_1080p():
    T, H, W, C = 3, 1080, 1920, 3
    n = _frames(T, H, W, C, torch.uint8, 10)
    g = torch.Generator().manual_seed(11)
    fw = torch.nn.functional.interpolate(torch.randn(T - 1, 2, H // 32, W // 32, generator=g, dtype=torch.float64) * 6,
                                         size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.3 * torch.randn(T - 1, 2, H, W, generator=g, dtype=torch.float64)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    got = rectify_frames(_as_layout(n, "NHWC"), fw.cuda(), bw.cuda(), 0.8, layout="NHWC")
    want = rectify_reference(n, fw.numpy(), bw.numpy(), 0.8)
    assert 0.9 < want[1].mean() < 1
    _check_frames(got, want, "NHWC", "1080p")


def test_readout_zero_is_the_input_and_with_matrices_warp_affine():
    T, H, W, C = 4, 37, 70, 3
    fw, bw = _rs_fields(T, H, W, 12)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    tm = torch.from_numpy(_matrices(T, H, W, 13)).cuda()
    for dtype in (torch.uint8, torch.float32, torch.float64):
        n = _frames(T, H, W, C, dtype, 14)
        if dtype == torch.uint8:
            n.reshape(-1)[:256] = np.arange(256)  # every byte value occurs
        v = _as_layout(n, "NHWC")
        video, valid = rectify_frames(v, tf, tb, 0.0, layout="NHWC")
        assert torch.equal(video, v) and bool(valid.all())
        for odt in (None, torch.uint8, torch.float64):
            got = rectify_frames(v, tf, tb, 0.0, matrices=tm, layout="NHWC", out_dtype=odt)
            want = warp_affine(v, tm, layout="NHWC", out_dtype=odt)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not bool(want[1].all())
    fw, bw = _rs_fields(T, H, W, 15, wild=False)  # finite flows: a NaN neighbour enters a sample through its zero weight
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    got = rectify_flows(tf, tb, 0.0)
    for g, f in ((got.flow_fw, tf), (got.flow_bw, tb)):
        x, y = torch.arange(W, device="cuda") + f[:, 0], torch.arange(H, device="cuda")[:, None] + f[:, 1]
        inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        assert inside.any() and (~inside).any()
        assert torch.equal(g[:, 0][inside], f[:, 0][inside]) and torch.equal(g[:, 1][inside], f[:, 1][inside])
        assert bool(torch.isnan(g[:, 0][~inside]).all()) and bool(torch.isnan(g[:, 1][~inside]).all())


def test_the_public_calls_are_their_parts():
    from test_gpu_batch import _video
    v = _dev(_video("240", 5))
    T, H, W = v.shape[0], v.shape[1], v.shape[2]
    fb = flow_video_fb(v, 4, layout="NHWC", consistency=None, out_dtype=torch.float64)
    for kw in (dict(), dict(anchor=0.0, iters=2, out_dtype=torch.float32, consistency=(0.05, 1.0)), dict(consistency=None)):
        rv = rectify_video(v, 4, 0.8, layout="NHWC", **kw)
        shutter = dict(anchor=kw.get("anchor", 0.5), iters=kw.get("iters", 3))
        video, valid = rectify_frames(v, fb.flow_fw, fb.flow_bw, 0.8, layout="NHWC", out_dtype=kw.get("out_dtype"), **shutter)
        flows = rectify_flows(fb.flow_fw, fb.flow_bw, 0.8, **shutter)
        assert torch.equal(rv.video, video) and torch.equal(rv.valid, valid) and rv.video.dtype == kw.get("out_dtype", torch.uint8)
        for a, b in ((rv.flow_fw, flows.flow_fw), (rv.flow_bw, flows.flow_bw)):
            assert a.dtype == torch.float64 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        if kw.get("consistency", CONSISTENCY) is None:
            assert rv.occlusion is None
        else:
            occ = fb_consistency(flows.flow_fw, flows.flow_bw, *kw.get("consistency", CONSISTENCY))
            assert torch.equal(rv.occlusion, occ) and bool(occ[:, 0][torch.isnan(flows.flow_fw[:, 0])].all())
        assert sorted(rv.timing) == sorted(fb.timing)
    want = rectify_reference(v.cpu().numpy(), fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), 0.8)
    rv = rectify_video(v.permute(0, 3, 1, 2), 4, 0.8)
    _check_frames((rv.video, rv.valid), want, "NCHW", "rectify_video")
    # stabilize_video_rs: the fit on the rectified forward flows under their mask, one resampling through the matrices
    for kw in (dict(), dict(model="affine", radius=2, crop=0.9, iters=3, scale=2.0, anchor=1.0, rs_iters=2, consistency=None,
                            out_dtype=torch.float64)):
        sv = stabilize_video_rs(v, 4, -0.6, layout="NHWC", **kw)
        shutter = dict(anchor=kw.get("anchor", 0.5), iters=kw.get("rs_iters", 3))
        flows = rectify_flows(fb.flow_fw, fb.flow_bw, -0.6, **shutter)
        occ = fb_consistency(flows.flow_fw, flows.flow_bw) if "consistency" not in kw else None
        m = global_motion(flows.flow_fw, occlusion=occ, model=kw.get("model", "similarity"), iters=kw.get("iters", 5),
                          scale=kw.get("scale", 1.0))
        M = stabilizing_transforms(m, kw.get("radius", 15), kw.get("crop", 1.0), size=(H, W))
        video, valid = rectify_frames(v, fb.flow_fw, fb.flow_bw, -0.6, matrices=M, layout="NHWC", out_dtype=kw.get("out_dtype"),
                                      **shutter)
        assert torch.equal(sv.video, video) and torch.equal(sv.valid, valid) and torch.equal(sv.transforms, M)
        assert torch.equal(sv.motion, m.motion) and torch.equal(sv.ok, m.ok)
        assert sv.flow_fw.cpu().numpy().tobytes() == flows.flow_fw.cpu().numpy().tobytes()
        assert sv.flow_bw.cpu().numpy().tobytes() == flows.flow_bw.cpu().numpy().tobytes()
        assert (sv.occlusion is None) if occ is None else torch.equal(sv.occlusion, occ)
        assert sv.transforms.shape == (T, 2, 3) and sv.video.dtype == kw.get("out_dtype", torch.uint8)


def test_the_pictures_with_the_devices_flows():
    """The picture scene of tests/test_rolling_cpu.py, rectify_video at the defaults: the bytes of the restatement on the
    device's flows, and the bar calibrated there with the oracle's flows (27.54 dB came out here, 17.95 dB unrectified over
    the same pixels, against the oracle's 27.58 dB and the bar of 22.78 dB)"""
    _, rolling, glob, _, _ = picture_scene()
    rv = rectify_video(_dev(list(rolling)), 4, READOUT_PIC, layout="NHWC")
    fb = flow_video_fb(_dev(list(rolling)), 4, layout="NHWC", consistency=None)
    want = rectify_reference(rolling, fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), READOUT_PIC)
    _check_frames((rv.video, rv.valid), want, "NHWC", "rectify_video on the pictures")
    _check_flows(rv, flows_reference(fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy(), READOUT_PIC), "rectify_video on the pictures")
    valid = rv.valid.cpu().numpy()
    got, before = psnr(rv.video.cpu().numpy(), glob, valid), psnr(rolling, glob, valid)
    print("pictures with the device's flows: %.2f dB (unrectified %.2f dB, bar %.2f dB) over %.3f of the interior pixels"
          % (got, before, pictures_bar(), valid[1:-1].mean()))
    assert valid[1:-1].mean() > 0.9 and got >= pictures_bar()


def test_the_calls_are_ordered_on_the_callers_stream():
    """Frames and flows written on a side stream behind a long sleep, rectified under that stream with no synchronisation:
    the kernels must read them after they are written, and what is queued behind them must see their outputs"""
    import time
    T, H, W, C = 4, 40, 60, 3
    n = _frames(T, H, W, C, torch.uint8, 12)
    fw, bw = _rs_fields(T, H, W, 13)
    want = rectify_reference(n, fw, bw, 0.8)
    want_flows = flows_reference(fw, bw, 0.8)
    src, sf, sb = _dev(list(n)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    dst, tf, tb = torch.zeros_like(src), torch.zeros_like(sf), torch.zeros_like(sb)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = (rectify_frames(dst, tf, tb, 0.8, layout="NHWC")[0].clone(), rectify_flows(tf, tb, 0.8).flow_fw.clone())
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
        tf.copy_(sf)
        tb.copy_(sb)
        got = rectify_frames(dst, tf, tb, 0.8, layout="NHWC")
        flows = rectify_flows(tf, tb, 0.8)
        copy, fcopy = got[0].clone(), flows.flow_bw.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    _check_frames(got, want, "NHWC", "side stream")
    _check_flows(flows, want_flows, "side stream")
    _same_bytes(copy, want[0], "NHWC", "side stream clone")
    _same_bytes(fcopy, want_flows[1], None, "side stream flow clone")
