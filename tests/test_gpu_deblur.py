"""Video deblurring on device tensors (papteam_opticalflow_amd/tensors.py: deblur, deblur_video -> papof_deblur_tensor).  The
device's video and support must be the BYTES of the numpy fp64 restatement (tests/_deblur_ref.py), compared as raw bytes: 4
frames of 3 channels on 9 x 130 (three tiles across with a ragged edge), uint8, float32 and float64, NCHW, NHWC and strided
views, float32 and float64 flows with NaNs, infinities and displacements that leave the image, radius 0, 1 and 2, 1 and 3
iterations, box and triangle tables and one with an offset of 0 and a zero weight, every output dtype; one-row, one-column
and tiny frames of 1 and 4 channels; that those inputs reach every branch of the rule; any workspace size, an absent support
and a strided out through the C ABI; more frames than one launch's grid holds; deblur_video against its parts chained by
hand; the shake scene of tests/test_deblur_cpu.py with the device's flows; the caller's stream order."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from _deblur_ref import BRANCHES, deblur_reference
from test_deblur_cpu import BAR_ESTIMATED, MID, psnr, scene
from test_gpu_denoise import _as_layout, _same_bytes
from test_gpu_tensors import _dev
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import CONSISTENCY, blur_schedule, deblur, deblur_video, flow_video_fb  # noqa: E402

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, None: None}
T, H, W, C = 4, 9, 130, 3
TABLES = {"box": blur_schedule(0.5, 5), "triangle": blur_schedule(1.0, 6, -0.5, "triangle"),
          "mixed": ([0.3, 0.0, -0.7, 0.5, -0.2], [0.5, 2.0, 0.0, 1.0, 1.5])}  # unsorted, an offset of 0, a zero weight


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _frames(T, H, W, C, dtype, seed):
    """random frames with a dark band (estimates under the floor) and, for the float dtypes, a NaN, an infinity-free
    negative patch and values above 1"""
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        n = rng.integers(0, 256, (T, H, W, C)).astype(np.uint8)
    else:
        n = (rng.random((T, H, W, C)) * 1.2).astype(_NP[dtype])
        n.reshape(-1)[7::97] = -0.25
        n.reshape(-1)[11::389] = math.nan
    n[:, :, : max(1, W // 16)] = 0
    return n


def _flows(T, H, W, seed, wild=True):
    """test_gpu_track's flow pairs: smooth, the backward flow roughly undoing the forward one, with NaNs, infinities and a
    patch of displacements that leave the image; wild=False: small and finite but for one NaN and one infinity"""
    fw, bw = _fields(T, H, W, seed, amp=3.0 if wild else 0.8, wild=wild and min(H, W) >= 4)
    if not wild:
        for f in (fw, bw):
            if H == 1:
                f[:, 1] = 0.0  # (no motion across a single row or column: the chains stay in the image)
            if W == 1:
                f[:, 0] = 0.0
        if H * W > 5:
            fw.reshape(T - 1, 2, -1)[:, :, 2] = math.nan
            bw.reshape(T - 1, 2, -1)[:, :, 5] = math.inf
    return fw, bw


def _run(v, tf, tb, table, radius, iters, cons, layout, odt):
    """deblur's checks and launch with any sample table (the public call takes blur_schedule's only)"""
    ts, descs, out_dtype, _ = tensors._check_video(v, layout, 1, odt)
    codes = tensors._check_flows(tf, tb, (v.shape[0] - 1, 2) + tuple(tf.shape[2:]), v.device)
    return tensors._deblur(ts, descs, (tf, tb), codes, table, radius, iters, tensors._alphas(cons), layout, out_dtype)


def _check(got, want, layout, what):
    _same_bytes(got.video, want[0], layout, what + " video")
    _same_bytes(got.support, want[1], None, what + " support")


def _sweep():
    """(radius, iters, table, flow dtype, consistency, output dtype): every (radius, iters, table), the rest rotating"""
    odts = (None, torch.uint8, torch.float32, torch.float64)
    for k, (radius, iters, table) in enumerate(itertools.product((0, 1, 2), (1, 3), sorted(TABLES))):
        yield radius, iters, table, (torch.float64, torch.float32)[(k // 2) % 2], (CONSISTENCY, None)[(k // 3) % 2], odts[k % 4]


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_synthetic_flows_every_dtype(dtype, layout):
    n = _frames(T, H, W, C, dtype, 1)
    fw, bw = _flows(T, H, W, 2)
    v = _as_layout(n, layout)
    dev = {fdt: (torch.from_numpy(fw).to(fdt).cuda(), torch.from_numpy(bw).to(fdt).cuda()) for fdt in (torch.float64, torch.float32)}
    seen = {k: set() for k in ("fdt", "cons", "odt")}
    for radius, iters, table, fdt, cons, odt in _sweep():
        tf, tb = dev[fdt]
        want = deblur_reference(n, tf.cpu().numpy(), tb.cpu().numpy(), *TABLES[table], radius=radius, iters=iters,
                                consistency=cons, out_dtype=_NP[odt or dtype])
        got = _run(v, tf, tb, TABLES[table], radius, iters, cons, layout, odt)
        assert got.video.dtype == (odt or dtype) and got.support.dtype == torch.uint8
        _check(got, want, layout, "%s %s R %d iters %d %s flows %s check %s out %s" % (dtype, layout, radius, iters, table, fdt,
                                                                                       cons is not None, odt))
        for k, val in (("fdt", fdt), ("cons", cons), ("odt", odt)):
            seen[k].add(val)
    assert seen == dict(fdt={torch.float32, torch.float64}, cons={CONSISTENCY, None},
                        odt={None, torch.uint8, torch.float32, torch.float64})


def test_the_public_call_uses_the_schedule():
    n = _frames(T, H, W, C, torch.uint8, 3)
    fw, bw = _flows(T, H, W, 4)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    v = _as_layout(n, "NHWC")
    _check(deblur(v, tf, tb, layout="NHWC"), deblur_reference(n, fw, bw, *blur_schedule(), out_dtype=np.uint8), "NHWC", "defaults")
    kw = dict(shutter=0.9, samples=7, phase=-0.3, shape="triangle", radius=2, iters=2, consistency=(0.05, 1.0))
    want = deblur_reference(n, fw, bw, *blur_schedule(0.9, 7, -0.3, "triangle"), radius=2, iters=2, consistency=(0.05, 1.0),
                            out_dtype=np.float32)
    _check(deblur(v, tf, tb, layout="NHWC", out_dtype=torch.float32, **kw), want, "NHWC", "keywords")


def test_branches_are_reached():
    """the inputs of test_synthetic_flows_every_dtype take every branch of the rule: chains that die and velocities that are
    not finite in both passes, estimates under the floor, clamped sample points, absent slots, pixels left unchanged"""
    fw, bw = _flows(T, H, W, 2)
    assert (~np.isfinite(fw)).any() and (~np.isfinite(bw)).any()
    for dtype in (torch.uint8, torch.float64):
        n = _frames(T, H, W, C, dtype, 1)
        for radius, cons in ((1, CONSISTENCY), (2, None)):
            *_, seen = deblur_reference(n, fw, bw, *TABLES["triangle"], radius=radius, iters=1, consistency=cons, parts=True)
            assert sorted(seen) == sorted(BRANCHES) and all(seen.values()), (dtype, radius, seen)


@pytest.mark.parametrize("Te,Ce", [(2, 1), (3, 4)])
@pytest.mark.parametrize("He,We", [(1, 70), (30, 1), (2, 3)])
def test_edge_shapes(He, We, Te, Ce):
    """one row, one column and a frame smaller than a tile, with two frames (both are end frames) and three"""
    n = _frames(Te, He, We, Ce, torch.float32, 5)
    fw, bw = _flows(Te, He, We, 6, wild=False)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    for radius, cons in ((0, None), (2, CONSISTENCY)):
        want = deblur_reference(n, fw, bw, *TABLES["mixed"], radius=radius, iters=2, consistency=cons, out_dtype=np.float32)
        got = _run(_as_layout(n, "NHWC"), tf, tb, TABLES["mixed"], radius, 2, cons, "NHWC", None)
        _check(got, want, "NHWC", "%d x %d T %d C %d R %d" % (He, We, Te, Ce, radius))
        assert want[1].any()


def test_strided_views():
    Ts, Hs, Ws, Cs = 5, 13, 41, 3
    fw, bw = _flows(Ts, Hs, Ws, 7)
    big = torch.from_numpy(_frames(2 * Ts, Hs + 3, 2 * Ws, Cs + 1, torch.uint8, 8)).cuda()
    v = big[::2, 2:Hs + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    # flows as (T - 1, H, W, 2) channels-last, read as (T - 1, 2, H, W), and float32 backward flows
    tf = torch.from_numpy(np.ascontiguousarray(fw.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    tb = torch.from_numpy(bw).float().cuda()
    nb = tb.cpu().numpy()
    want = deblur_reference(v.cpu().numpy(), fw, nb, *blur_schedule(0.5, 4), radius=1, iters=2, out_dtype=np.uint8)
    _check(deblur(v, tf, tb, samples=4, iters=2, layout="NHWC"), want, "NHWC", "strided NHWC")
    _check(deblur(v.permute(0, 3, 1, 2), tf, tb, samples=4, iters=2), want, "NCHW", "strided NCHW")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(Ts, 2, Hs, Ws)  # one channel read twice: a zero stride
    want = deblur_reference(v.cpu().numpy()[..., [1, 1]], fw, nb, *blur_schedule(0.5, 4), radius=2, iters=1, out_dtype=np.float64)
    _check(deblur(one, tf, tb, samples=4, radius=2, iters=1, out_dtype=torch.float64), want, "NCHW", "expanded channel")
    same = tf[:1].expand(Ts - 1, 2, Hs, Ws)  # one pair's flow for every pair
    want = deblur_reference(v.cpu().numpy(), np.repeat(fw[:1], Ts - 1, 0), nb, *blur_schedule(0.5, 4), iters=1, out_dtype=np.uint8)
    _check(deblur(v, same, tb, samples=4, iters=1, layout="NHWC"), want, "NHWC", "expanded flows")


def test_workspace_sizes_absent_support_and_strided_outputs_through_the_c_abi():
    Ts, Hs, Ws, Cs, R = 5, 10, 66, 2, 1
    n = _frames(Ts, Hs, Ws, Cs, torch.float64, 9)
    fw, bw = _flows(Ts, Hs, Ws, 10)
    v, tf, tb = _dev(list(n)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    d_f = [tensors._flow_struct(f, capi.DTYPE_F64) for f in (tf, tb)]
    strided = torch.zeros((Ts, Hs, 2 * Ws, Cs), dtype=torch.float32, device="cuda")  # the video into every other column
    view = strided[:, :, ::2]
    d_out = tensors._struct(view, *tensors.descriptor(view, "NHWC")[1:])
    wide = torch.zeros((Ts, 2 * Hs, Ws), dtype=torch.uint8, device="cuda")  # the support into every other row
    sup = wide[:, ::2]
    d_sup = tensors._struct(sup, (sup.stride(0), sup.stride(1), sup.stride(2), 0), capi.DTYPE_U8)
    off, w = TABLES["mixed"]
    k = len(off)
    want = deblur_reference(n, fw, bw, off, w, radius=R, iters=2, out_dtype=np.float32)
    P = 8 * Cs * Hs * Ws * (2 * R + 2)
    gpu = tensors._handle(0)[0]
    assert gpu.L.papof_deblur_workspace(Ts, Hs, Ws, Cs, R) == Ts * P
    for nbytes, with_sup in ((P, True), (Ts * P, True), (2 * P + 17, False), (3 * P, True), (9 * P, True)):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        strided.zero_()
        wide.fill_(7)
        tensors._launch(v.device, "papof_deblur_tensor", Ts, Hs, Ws, Cs, ctypes.byref(d_in), ctypes.byref(d_f[0]),
                        ctypes.byref(d_f[1]), k, (ctypes.c_double * k)(*off), (ctypes.c_double * k)(*w), R, 2, 1, *CONSISTENCY,
                        ctypes.byref(d_out), ctypes.byref(d_sup) if with_sup else None, ctypes.c_void_p(ws.data_ptr()),
                        ctypes.c_longlong(nbytes))
        _same_bytes(view, want[0], "NHWC", "workspace of %d bytes" % nbytes)
        assert not strided[:, :, 1::2].any() and bool((wide[:, 1::2] == 7).all())
        if with_sup:
            _same_bytes(sup, want[1], None, "support, workspace of %d bytes" % nbytes)
        else:
            assert bool((wide == 7).all())
        torch.cuda.synchronize()
        del ws


def test_more_frames_than_one_launch_holds():
    """65535 + 2 frames of 2 x 3: the grid axis that counts the targets (and, three times as long, the one that counts
    (target, slot) pairs) is cut by launch_tiles.  The video repeats every 4 frames, so every frame away from the ends
    equals one of 4 frames of the restatement on 13 frames; compared on the device."""
    Tl, Hl, Wl, period, Tr = 65535 + 2, 2, 3, 4, 13
    assert (Tl - Tr) % period == 0
    base = _frames(period, Hl, Wl, 1, torch.float64, 11) + 0.1
    fb, bb = _flows(period + 1, Hl, Wl, 12, wild=False)
    at = lambda a, count: a[np.arange(count) % period]  # noqa: E731
    want, want_sup = deblur_reference(at(base, Tr), at(fb, Tr - 1), at(bb, Tr - 1), *blur_schedule(0.5, 3), radius=1, iters=1)
    assert want_sup.any() and len({want[t].tobytes() for t in range(Tr)}) > period
    idx = torch.arange(Tl, device="cuda")
    frames = torch.from_numpy(base).cuda()[idx % period]
    tf, tb = (torch.from_numpy(f[:period]).cuda()[idx[:-1] % period] for f in (fb, bb))
    got = deblur(frames, tf, tb, samples=3, iters=1, layout="NHWC")
    ref = torch.where(idx < 6, idx, torch.where(idx >= Tl - 6, idx - (Tl - Tr), 4 + idx % period))
    assert got.video.dtype == torch.float64
    assert torch.equal(got.video.view(torch.int64), torch.from_numpy(want).cuda()[ref].view(torch.int64))
    assert torch.equal(got.support, torch.from_numpy(want_sup).cuda()[ref])


def test_deblur_video_is_its_parts():
    from test_gpu_batch import _video
    v = _dev(_video("240", 4))
    for kw in (dict(), dict(shutter=0.8, samples=5, radius=2, iters=2, consistency=None, out_dtype=torch.float32)):
        cons = kw.get("consistency", CONSISTENCY)
        fb = flow_video_fb(v, 3, layout="NHWC", consistency=cons, out_dtype=torch.float64)
        dk = {k: kw[k] for k in kw if k != "out_dtype"}
        dv = deblur_video(v, 3, layout="NHWC", **kw)
        d = deblur(v, fb.flow_fw, fb.flow_bw, layout="NHWC", out_dtype=kw.get("out_dtype"), **dk)
        assert torch.equal(dv.video, d.video) and torch.equal(dv.support, d.support) and dv.video.dtype == kw.get("out_dtype", torch.uint8)
        for a, b in ((dv.flow_fw, fb.flow_fw), (dv.flow_bw, fb.flow_bw)):
            assert a.dtype == torch.float64 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert (dv.occlusion is None) if cons is None else torch.equal(dv.occlusion, fb.occlusion)
        assert sorted(dv.timing) == sorted(fb.timing)
    # passes=2: the flows of the first pass's video (in the frames' dtype), the ORIGINAL frames deblurred with them
    dv = deblur_video(v, 3, passes=2, layout="NHWC", iters=2, out_dtype=torch.float64)
    first = deblur_video(v, 3, layout="NHWC", iters=2)
    fb = flow_video_fb(first.video, 3, layout="NHWC", out_dtype=torch.float64)
    d = deblur(v, fb.flow_fw, fb.flow_bw, layout="NHWC", iters=2, out_dtype=torch.float64)
    assert first.video.dtype == torch.uint8 and torch.equal(dv.video.view(torch.int64), d.video.view(torch.int64))
    assert torch.equal(dv.support, d.support) and dv.flow_fw.cpu().numpy().tobytes() == fb.flow_fw.cpu().numpy().tobytes()
    assert torch.equal(dv.occlusion, fb.occlusion)


def test_the_shake_scene_with_the_devices_flows():
    """The shake scene of tests/test_deblur_cpu.py, deblur_video at the defaults with 4 pyramid levels: the middle frame is
    the bytes of the restatement on the device's flows and meets the bar set there for estimated flows (+2.5 dB).  Measured
    on an MI355X: blurred 25.58 dB, deblurred 30.70 dB (+5.12; the oracle's flows give 30.71 dB)."""
    frames, sharp, _, _ = scene("shake", 0.5)
    dv = deblur_video(_dev(list(frames)), 4, layout="NHWC")
    want = deblur_reference(frames, dv.flow_fw.cpu().numpy(), dv.flow_bw.cpu().numpy(), *blur_schedule(), targets=[MID],
                            out_dtype=np.uint8)
    got = dv.video.cpu().numpy()
    assert got[MID].tobytes() == want[0][MID].tobytes() and dv.support[MID].cpu().numpy().tobytes() == want[1][MID].tobytes()
    before, after = psnr(frames[MID], sharp[MID]), psnr(got[MID], sharp[MID])
    print("shake scene with the device's flows: blurred %.2f dB, deblurred %.2f dB (bar +%.1f dB)" % (before, after, BAR_ESTIMATED))
    assert after - before >= BAR_ESTIMATED


def test_the_calls_are_ordered_on_the_callers_stream():
    """Frames and flows written on a side stream behind a long sleep, deblurred under that stream with no synchronisation:
    the kernels must read them after they are written, and what is queued behind them must see their outputs"""
    import time
    Ts, Hs, Ws, Cs = 4, 40, 60, 3
    n = _frames(Ts, Hs, Ws, Cs, torch.uint8, 12)
    fw, bw = _flows(Ts, Hs, Ws, 13)
    want = deblur_reference(n, fw, bw, *blur_schedule(0.5, 4), iters=2, out_dtype=np.uint8)
    src, sf, sb = _dev(list(n)), torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    dst, tf, tb = torch.zeros_like(src), torch.zeros_like(sf), torch.zeros_like(sb)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = deblur(dst, tf, tb, samples=4, iters=2, layout="NHWC").video.clone()
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
        got = deblur(dst, tf, tb, samples=4, iters=2, layout="NHWC")
        copy = got.video.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    _check(got, want, "NHWC", "side stream")
    _same_bytes(copy, want[0], "NHWC", "side stream clone")
