"""Motion-compensated deinterlacing on device tensors (papteam_opticalflow_amd/tensors.py: split_fields, bob_fields,
field_flows, deinterlace_fields, deinterlace_video -> papof_deinterlace_tensor).  The device's video and confidence must be
the BYTES of the numpy fp64 restatement (tests/_deinterlace_ref.py), compared as raw bytes: uint8, float32 and float64 fields
of 1 .. 4 channels, NCHW, NHWC and strided views, float32 and float64 flows with NaNs, infinities and large displacements,
4, 5 and 7 fields, both parities, both modes, two sigmas, every output dtype, one-row, one-column and tile-crossing fields,
a float32 confidence, an absent one and a strided video through the C ABI, a dense 540 x 1920 case; the public calls against
their parts chained by hand, the caller's stream order, and the calibration scenes of tests/test_deinterlace_cpu.py with
the device's flows."""
import ctypes

import numpy as np
import pytest

from _deinterlace_ref import deinterlace_reference, split_reference
from test_deinterlace_cpu import CRITICAL, SCENES, SIGMA, bar, deint_scene, made_psnr
from test_gpu_denoise import _as_layout, _frames, _same_bytes
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (bob_fields, deinterlace_fields, deinterlace_video, field_flows,  # noqa: E402
                                             flow_pairs_fb, split_fields)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, None: None}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _pair_fields(T, Hf, W, seed, **kw):
    """flows of the T - 2 pairs of T fields, as test_gpu_track makes them for T - 1 frames"""
    return _fields(T - 1, Hf, W, seed, **kw)


def _check(got, want, layout, what):
    video, conf = want
    assert got.confidence.dtype == torch.float64
    _same_bytes(got.video, video, layout, what + " video")
    _same_bytes(got.confidence, conf, None, what + " confidence")


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    Hf, W = 19, 53
    for T, C in ((4, 3), (5, 1), (7, 4), (5, 2)):
        n = _frames(T, Hf, W, C, dtype, T + C)
        fw, bw = _pair_fields(T, Hf, W, 2 + T)
        v = _as_layout(n, layout)
        for first in (0, 1):
            what = "%s %s T %d C %d first %d" % (dtype, layout, T, C, first)
            _same_bytes(bob_fields(v, first, layout=layout), deinterlace_reference(n, first=first, mode=0)[0], layout,
                        what + " bob")
            for fdt in (torch.float64, torch.float32):
                tf, tb = torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()
                nf, nb = tf.cpu().numpy(), tb.cpu().numpy()
                for sigma in (SIGMA, 1e-3):
                    for odt in (None,) if sigma != SIGMA or fdt != torch.float64 else (None, torch.uint8, torch.float32,
                                                                                      torch.float64):
                        got = deinterlace_fields(v, tf, tb, first, sigma=sigma, layout=layout, out_dtype=odt)
                        want = deinterlace_reference(n, nf, nb, first=first, sigma=sigma, out_dtype=_NP[odt])
                        _check(got, want, layout, "%s flows %s sigma %s out %s" % (what, fdt, sigma, odt))


def test_branches_are_reached():
    """the synthetic cases above take every branch of the rule: q = 0, one sample and two, on interior frames; q = 0 and
    one sample on both end frames; NaN and infinite flows; a two-sided q lowered by the samples' disagreement"""
    Hf, W = 19, 53
    for T in (4, 5, 7):
        n = _frames(T, Hf, W, 3, torch.uint8, T + 3)
        fw, bw = _pair_fields(T, Hf, W, 2 + T)
        assert (~np.isfinite(fw)).any() and (~np.isfinite(bw)).any()
        for first in (0, 1):
            _, q, c0, c1 = deinterlace_reference(n, fw, bw, first=first, sigma=SIGMA, parts=True)
            for t in range(1, T - 1):
                both, one, none = (c0[t] > 0) & (c1[t] > 0), (c0[t] > 0) ^ (c1[t] > 0), (c0[t] <= 0) & (c1[t] <= 0)
                assert both.any() and one.any() and none.any(), (T, t)
                assert (q[t][none] == 0).all() and (q[t][one] > 0).all()
                assert (q[t][both] < np.maximum(c0[t], c1[t])[both]).any()
            assert (c0[0] == 0).all() and (c1[0] > 0).any() and (c1[0] == 0).any() and (q[0] == 0.5 * c1[0]).all()
            assert (c1[T - 1] == 0).all() and (c0[T - 1] > 0).any() and (c0[T - 1] == 0).any()
            assert (q[T - 1] == 0.5 * c0[T - 1]).all()


@pytest.mark.parametrize("Hf,W", [(1, 70), (30, 1), (2, 3), (9, 130)])
def test_edge_shapes(Hf, W):
    """one row, one column, a field smaller than the cubic's reach, and one that crosses the 64-column and 4-row tile seams"""
    T, C = 5, 3
    n = _frames(T, Hf, W, C, torch.float32, 3)
    fw, bw = _pair_fields(T, Hf, W, 4, wild=False)
    for f in (fw, bw):  # little motion across a single row or column, but for a few pixels that leave; NaN and infinite flows
        flat = f.reshape(T - 2, 2, -1)  # (a view: _fields returns contiguous arrays)
        if Hf <= 2:
            flat[:, 1, 2:] = np.round(flat[:, 1, 2:] / 4.0)
        if W <= 3:
            flat[:, 0, 2:] = np.round(flat[:, 0, 2:] / 4.0)
        if flat.shape[2] > 11:
            flat[:, :, 7] = np.nan
            flat[:, :, 11] = (np.inf, -np.inf)
    for first in (0, 1):
        want = deinterlace_reference(n, fw, bw, first=first, sigma=SIGMA)
        assert (want[1] > 0).any()
        got = deinterlace_fields(_as_layout(n, "NHWC"), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), first,
                                 layout="NHWC")
        _check(got, want, "NHWC", "%d x %d first %d" % (Hf, W, first))
        _same_bytes(bob_fields(_as_layout(n, "NCHW"), first), deinterlace_reference(n, first=first, mode=0)[0], "NCHW", "bob")


def test_strided_views():
    T, Hf, W, C = 5, 29, 41, 3
    fw, bw = _pair_fields(T, Hf, W, 5)
    big = torch.from_numpy(_frames(2 * T, Hf + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:Hf + 2, ::2, 1:]  # every other field, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    # flows as (T - 2, Hf, W, 2) channels-last, read as (T - 2, 2, Hf, W), and float32 backward flows
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    tb = torch.from_numpy(bw).float().cuda()
    want = deinterlace_reference(v.cpu().numpy(), fw, tb.cpu().numpy(), first=1, sigma=SIGMA)
    _check(deinterlace_fields(v, tf, tb, 1, layout="NHWC"), want, "NHWC", "strided NHWC")
    _check(deinterlace_fields(v.permute(0, 3, 1, 2), tf, tb, 1), want, "NCHW", "strided NCHW")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(T, 2, Hf, W)  # one channel read twice: a zero stride
    want = deinterlace_reference(v.cpu().numpy()[..., [1, 1]], fw, tb.cpu().numpy(), sigma=SIGMA)
    _check(deinterlace_fields(one, tf, tb), want, "NCHW", "expanded channel")
    _same_bytes(bob_fields(one), deinterlace_reference(v.cpu().numpy()[..., [1, 1]], mode=0)[0], "NCHW", "expanded bob")


def test_float32_confidence_absent_one_and_a_strided_video_through_the_c_abi():
    T, Hf, W, C = 4, 20, 66, 2
    n = _frames(T, Hf, W, C, torch.float64, 8)
    fw, bw = _pair_fields(T, Hf, W, 9)
    v, tf, tb = _dev(list(n)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    d_f = [tensors._flow_struct(f, capi.DTYPE_F64) for f in (tf, tb)]
    strided = torch.zeros((T, 2 * Hf, 2 * W, C), dtype=torch.float32, device="cuda")  # the video into every other column
    view = strided[:, :, ::2]
    d_out = tensors._struct(view, *tensors.descriptor(view, "NHWC")[1:])
    conf = torch.zeros((T, Hf, W), dtype=torch.float32, device="cuda")
    d_conf = tensors._struct(conf, (Hf * W, W, 1, 0), capi.DTYPE_F32)
    for mode in (1, 0):
        want = deinterlace_reference(n, fw, bw, first=1, mode=mode, sigma=0.1, out_dtype=np.float32, conf_dtype=np.float32)
        for with_conf in (True, False):
            strided.zero_()
            conf.fill_(-1.0)
            flows = (ctypes.byref(d_f[0]), ctypes.byref(d_f[1])) if mode else (None, None)  # mode 0: no flows are read
            tensors._launch(v.device, "papof_deinterlace_tensor", T, Hf, W, C, ctypes.byref(d_in), 1, mode, *flows, 0.1,
                            ctypes.byref(d_out), ctypes.byref(d_conf) if with_conf else None)
            _same_bytes(view, want[0], "NHWC", "strided video, mode %d" % mode)
            assert not strided[:, :, 1::2].any()
            if with_conf:
                _same_bytes(conf, want[1], None, "float32 confidence, mode %d" % mode)
            else:
                assert (conf == -1.0).all()


def test_uint8_kept_lines_are_the_inputs_bytes():
    rng = np.random.default_rng(14)
    V = rng.integers(0, 256, (3, 24, 37, 3)).astype(np.uint8)
    V.reshape(-1)[:256] = np.arange(256)  # every byte value occurs
    for top_first, first in ((True, 0), (False, 1)):
        F = split_fields(torch.from_numpy(V).cuda(), top_first, layout="NHWC")
        assert torch.equal(F.cpu(), torch.from_numpy(split_reference(V, top_first)[0]))
        fw, bw = _pair_fields(6, 12, 37, 15)
        d = deinterlace_fields(F, torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), first, layout="NHWC")
        b = bob_fields(F, first, layout="NHWC")
        assert d.video.dtype == torch.uint8 and b.dtype == torch.uint8 and d.video.shape == (6, 24, 37, 3)
        for k in range(6):
            p = (k + first) & 1
            assert torch.equal(d.video[k, p::2], F[k]) and torch.equal(b[k, p::2], F[k])
            assert torch.equal(d.video[k, p::2].cpu(), torch.from_numpy(V[k // 2, p::2]))  # the woven frame's own lines


def test_dense_540x1920():
    T, Hf, W, C = 4, 540, 1920, 3
    n = _frames(T, Hf, W, C, torch.uint8, 10)
    g = torch.Generator().manual_seed(11)
    fw = torch.nn.functional.interpolate(torch.randn(T - 2, 2, Hf // 30, W // 32, generator=g, dtype=torch.float64) * 3,
                                         size=(Hf, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.3 * torch.randn(T - 2, 2, Hf, W, generator=g, dtype=torch.float64)
    fw[:, :, :40, :40] = 900.0  # a corner that leaves the image
    got = deinterlace_fields(_as_layout(n, "NHWC"), fw.cuda(), bw.cuda(), layout="NHWC")
    _check(got, deinterlace_reference(n, fw.numpy(), bw.numpy(), sigma=SIGMA), "NHWC", "540 x 1920")


@pytest.fixture(scope="module")
def scenes():
    return {s: deint_scene(*s) for s in SCENES}


def test_the_public_calls_are_their_parts(scenes):
    _, F, _, _ = scenes[(2.5, 0.25)]
    v = _dev(list(F))
    ff = field_flows(v, 4, layout="NHWC")
    fb = flow_pairs_fb(v[:-2], v[2:], 4, layout="NHWC", consistency=None, out_dtype=torch.float64)
    assert torch.equal(ff.flow_fw, fb.flow_fw) and torch.equal(ff.flow_bw, fb.flow_bw) and ff.occlusion is None
    assert ff.flow_fw.shape == (F.shape[0] - 2, 2) + F.shape[1:3] and ff.flow_fw.dtype == torch.float64
    for kw in ({}, dict(sigma=0.1, out_dtype=torch.float32)):
        dv = deinterlace_video(v, 4, 0, layout="NHWC", **kw)
        d = deinterlace_fields(v, ff.flow_fw, ff.flow_bw, 0, layout="NHWC", **kw)
        assert torch.equal(dv.video, d.video) and torch.equal(dv.confidence, d.confidence)
        assert torch.equal(dv.flow_fw, ff.flow_fw) and torch.equal(dv.flow_bw, ff.flow_bw) and sorted(dv.timing) == sorted(ff.timing)
        assert dv.video.dtype == kw.get("out_dtype", torch.uint8)
    nchw = deinterlace_video(v.permute(0, 3, 1, 2), 4, 1)
    d1 = deinterlace_fields(v, ff.flow_fw, ff.flow_bw, 1, layout="NHWC")
    assert torch.equal(nchw.video.permute(0, 2, 3, 1), d1.video) and torch.equal(nchw.confidence, d1.confidence)
    # bob_fields is mode 0 of the same kernel: the restatement's bytes, and deinterlace_fields' wherever q is 0
    b = bob_fields(v, 0, layout="NHWC")
    _same_bytes(b, deinterlace_reference(F, mode=0)[0], "NHWC", "bob_fields")
    d0 = deinterlace_fields(v, ff.flow_fw, ff.flow_bw, 0, layout="NHWC")
    made = torch.stack([d0.video[t, 1 - (t & 1)::2] for t in range(len(F))])
    bobs = torch.stack([b[t, 1 - (t & 1)::2] for t in range(len(F))])
    assert (d0.confidence == 0).any() and torch.equal(made[d0.confidence == 0], bobs[d0.confidence == 0])


@pytest.mark.parametrize("scene", SCENES)
def test_the_scenes_with_the_devices_flows(scenes, scene):
    """The calibration scenes of tests/test_deinterlace_cpu.py, deinterlace_video at the defaults: the bytes of the restatement on
    the device's flows, and the bars calibrated there with the oracle's flows"""
    truth, F, _, _ = scenes[scene]
    dv = deinterlace_video(_dev(list(F)), 4, 0, layout="NHWC")
    want = deinterlace_reference(F, dv.flow_fw.cpu().numpy(), dv.flow_bw.cpu().numpy(), sigma=SIGMA)
    _check(dv, want, "NHWC", "deinterlace_video %s" % (scene,))
    got, bob = made_psnr(dv.video.cpu().numpy(), truth), made_psnr(deinterlace_reference(F, mode=0)[0], truth)
    print("pan %s with the device's flows: %.2f dB (bob %.2f dB, bar %.2f dB)" % (scene, got, bob, bar(scene)))
    assert got >= bar(scene), (scene, got, bar(scene))
    if scene == (0.0, 0.0):
        assert dv.video[1:-1].cpu().numpy().tobytes() == truth[1:-1].tobytes()
    if scene == CRITICAL:
        assert abs(got - bob) <= 0.1


def test_the_calls_are_ordered_on_the_callers_stream():
    """Fields written on a side stream behind a long sleep, deinterlaced under that stream with no synchronisation: the
    kernel must read them after they are written, and what is queued behind it must see its outputs"""
    import time
    T, Hf, W, C = 5, 40, 60, 3
    n = _frames(T, Hf, W, C, torch.uint8, 12)
    fw, bw = _pair_fields(T, Hf, W, 13)
    want = deinterlace_reference(n, fw, bw, first=1, sigma=SIGMA)
    want_bob = deinterlace_reference(n, first=1, mode=0)[0]
    src = _dev(list(n))
    dst = torch.zeros_like(src)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = (deinterlace_fields(dst, tf, tb, 1, layout="NHWC").video.clone(), bob_fields(dst, 1, layout="NHWC").clone())
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
        got = deinterlace_fields(dst, tf, tb, 1, layout="NHWC")
        bob = bob_fields(dst, 1, layout="NHWC")
        copy = got.video.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    _check(got, want, "NHWC", "side stream")
    _same_bytes(bob, want_bob, "NHWC", "side stream bob")
    _same_bytes(copy, want[0], "NHWC", "side stream clone")
