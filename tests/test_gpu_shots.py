"""Shot boundaries on device tensors (papteam_opticalflow_amd/tensors.py: shot_histograms, detect_shots, cut_flows,
flow_video_shots -> papof_cell_hist_tensor).  The device's histograms must be the BYTES of the numpy restatement
(tests/_shots_ref.py): uint8, float32 and float64 frames (floats with NaNs, infinities and values beyond 0 .. 1) of 1 .. 4
channels, NCHW, NHWC, 1, 2 and 5 frames, cells of 1, 16 and 64 rows, 4, 16 and 64 bins, frames across the 64-column and
cell-row seams, with partial cells and with fewer rows than are loaded ahead, strided, channel-expanded and misaligned packed
views, a dense 1080p case, a `hist` buffer that held two different patterns, the second launch of the split grid, the C ABI's
refusals on a live handle; then the public calls: the scenes of tests/test_shots_cpu.py, flow_video_shots against flow_video_fb
shot by shot, what temporal_filter and track_points make of a cut pair, and the caller's stream order."""
import ctypes

import numpy as np
import pytest

from _shots_ref import cell_pixels, hist_reference
from test_shots_cpu import A, C_ABI_REFUSALS, FAR, SCENES, T_SCENE, _image, scene_frames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (cut_flows, detect_cuts, detect_shots, flow_video_fb, flow_video_shots,  # noqa: E402
                                             shot_histograms, split_shots, temporal_filter, track_points)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()
    torch.cuda.empty_cache()


def _frames(T, H, W, C, dtype, seed):
    """frames whose luma covers every bin: a ramp across the frame plus noise, different from frame to frame and from channel
    to channel; floats reach beyond 0 .. 1 and hold NaNs and infinities"""
    rng = np.random.default_rng(seed)
    y, x = np.arange(H)[:, None, None], np.arange(W)[None, :, None]
    base = 128.0 + 110.0 * np.sin(y * 0.37 + x * 0.11 + np.arange(C) * 1.3)
    f = np.stack([base * (0.6 + 0.1 * k) + rng.normal(0, 20, base.shape) for k in range(T)])
    if dtype == torch.uint8:
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    f = ((f - 128.0) / 180.0 + 0.5).astype(_NP[dtype])  # about -0.3 .. 1.3
    flat = f.reshape(-1)
    idx = rng.integers(0, flat.size, max(3, flat.size // 50))
    flat[idx[0::3]], flat[idx[1::3]], flat[idx[2::3]] = np.nan, np.inf, -np.inf
    return f


def _as_layout(a, layout):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2).contiguous()


def _same_hist(got, want, what, cell_rows=16, bins=16):
    assert (got.cell_rows, got.bins) == (cell_rows, bins) and got.hist.dtype == torch.int32 and got.hist.is_contiguous(), what
    assert tuple(got.hist.shape) == want.shape, (what, tuple(got.hist.shape), want.shape)
    g = got.hist.cpu().numpy()
    if g.tobytes() != want.tobytes():
        bad = g != want
        raise AssertionError("%s: %d of %d counts differ; first at %s: %d for %d" % (
            what, int(bad.sum()), bad.size, tuple(int(k[0]) for k in np.nonzero(bad)), g[bad][0], want[bad][0]))


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_hist_every_dtype(dtype, layout):
    H, W = 37, 150
    for T, C in ((1, 3), (2, 1), (5, 4), (2, 2)):
        n = _frames(T, H, W, C, dtype, T + C)
        v = _as_layout(n, layout)
        for cell_rows in (1, 16, 64):
            for bins in (4, 16, 64):
                want = hist_reference(n, cell_rows, bins)
                assert (want.sum(-1) == cell_pixels(H, W, cell_rows)).all() and (want.sum((0, 1, 2)) > 0).sum() >= bins // 2
                got = shot_histograms(v, cell_rows=cell_rows, bins=bins, layout=layout)
                assert got.size == (H, W)
                _same_hist(got, want, "%s %s T %d C %d cell_rows %d bins %d" % (dtype, layout, T, C, cell_rows, bins),
                           cell_rows, bins)


@pytest.mark.parametrize("H,W", [(1, 70), (2, 3), (30, 1), (17, 63), (16, 64), (33, 65), (9, 130), (37, 150)])
def test_hist_edge_shapes(H, W):
    """the 64-column and cell-row seams, partial cells, and cells with fewer rows than are loaded ahead"""
    for dtype, C, layout in ((torch.uint8, 3, "NHWC"), (torch.uint8, 1, "NCHW"), (torch.float32, 2, "NHWC"),
                             (torch.float64, 4, "NCHW")):
        for T in (1, 2, 5):
            n = _frames(T, H, W, C, dtype, 3 + T)
            for cell_rows, bins in ((1, 4), (16, 16), (64, 64), (16, 64)):
                _same_hist(shot_histograms(_as_layout(n, layout), cell_rows=cell_rows, bins=bins, layout=layout),
                           hist_reference(n, cell_rows, bins), "%d x %d %s C %d T %d cell_rows %d bins %d" % (
                               H, W, dtype, C, T, cell_rows, bins), cell_rows, bins)


def test_hist_of_strided_and_expanded_views():
    T, H, W, C = 3, 29, 75, 3
    big = torch.from_numpy(_frames(2 * T, H + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:H + 2, ::2, 1:]  # every other frame, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    want = hist_reference(v.cpu().numpy())
    _same_hist(shot_histograms(v, layout="NHWC"), want, "strided NHWC")
    _same_hist(shot_histograms(v.permute(0, 3, 1, 2)), want, "strided NCHW")
    rows = big[:, ::3]  # a row stride of three rows, packed within the row
    _same_hist(shot_histograms(rows, layout="NHWC"), hist_reference(rows.cpu().numpy()), "row-strided")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(T, 3, H, W)  # one channel read three times: a zero stride
    _same_hist(shot_histograms(one), hist_reference(v.cpu().numpy()[..., [1] * 3]), "expanded channel")
    same = v[2:3].expand(4, H, W, C)  # one frame four times, a zero frame stride
    h = shot_histograms(same, layout="NHWC").hist
    assert torch.equal(h, h[:1].expand_as(h)) and torch.equal(h[0], torch.from_numpy(want[2]).cuda())
    f = torch.from_numpy(_frames(T, H, W, 4, torch.float32, 8)).cuda()[:, 1::2, :, ::2]  # floats: every other row and channel
    _same_hist(shot_histograms(f, layout="NHWC"), hist_reference(f.cpu().numpy()), "strided float32")


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_hist_of_packed_rows_at_every_alignment(C):
    """packed uint8 rows are loaded as aligned dwords: column slices of one NHWC tensor whose rows are no multiple of 4 bytes
    long, so that the rows of a cell start at every byte offset 0 .. 3 -- with four channels and a misaligned buffer a full cell
    spans 65 dwords"""
    T, H, W = 2, 19, 131
    rng = np.random.default_rng(20 + C)
    buf = torch.from_numpy(rng.integers(0, 256, T * H * (W + 5) * C + 8).astype(np.uint8)).cuda()
    seen = set()
    for base in range(4):
        big = buf[base:base + T * H * (W + 5) * C].view(T, H, W + 5, C)
        for off in range(4):
            v = big[:, :, off:off + W]
            assert v.stride(2) == C and v.stride(3) == 1 and not v.is_contiguous()
            seen.update((v.data_ptr() + r * v.stride(1)) % 4 for r in range(H))
            _same_hist(shot_histograms(v, layout="NHWC"), hist_reference(v.cpu().numpy()), "C %d base %d offset %d" % (C, base, off))
    assert seen == {0, 1, 2, 3}


def test_dense_1080p():
    img = _image()
    n = np.stack([img, np.ascontiguousarray(img[::-1, ::-1])])
    assert n.shape == (2, 1080, 1920, 3)
    _same_hist(shot_histograms(_as_layout(n, "NHWC"), layout="NHWC"), hist_reference(n), "1080 x 1920")


def test_the_hist_does_not_depend_on_what_the_buffer_held():
    T, H, W, C = 3, 21, 140, 3
    n = _frames(T, H, W, C, torch.uint8, 7)
    v = _as_layout(n, "NHWC")
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    want = hist_reference(n)
    guard = 64
    buf = torch.empty(want.size + 2 * guard, dtype=torch.int32, device="cuda")
    for pattern in (0x5a5a5a5a, -1):
        buf.fill_(pattern)
        tensors._launch(v.device, "papof_cell_hist_tensor", T, H, W, C, ctypes.byref(d_in), 16, 16,
                        ctypes.c_void_p(buf[guard:].data_ptr()))
        got = buf.cpu().numpy()
        assert got[guard:-guard].tobytes() == want.tobytes(), hex(pattern & 0xffffffff)
        assert (got[:guard] == pattern).all() and (got[-guard:] == pattern).all()  # nothing beyond the table


# ---- the second launch of the split grid: launch_tiles cuts the frames at 65535 (gridDim.y)
def test_every_frame_of_both_launches():
    """65535 + 2 frames of 2 x 3 x 1, periodic with period 7 (65535 mod 7 = 1: the first frame of the second launch is not
    frame 0), every frame with memory of its own (an index gather, not a stride-0 view, which would hide a missing start
    index); every frame's histogram is compared on the device with the restatement's of its base frame"""
    P, cut = 7, 65535
    N = cut + 2
    assert cut % P != 0
    base = np.random.default_rng(30).integers(0, 256, (P, 2, 3, 1)).astype(np.uint8)
    want = hist_reference(base, 16, 16)
    assert all((want[i] != want[0]).any() for i in range(1, P))  # no base frame passes for frame 0
    idx = torch.from_numpy(np.arange(N, dtype=np.int64) % P).cuda()
    frames = torch.from_numpy(base).cuda().index_select(0, idx)
    assert frames.is_contiguous() and frames.stride(0) > 0
    got = shot_histograms(frames, layout="NHWC").hist
    expect = torch.from_numpy(want).cuda().index_select(0, idx)
    assert got.shape == expect.shape and got.dtype == expect.dtype
    if not torch.equal(got, expect):
        bad = (got != expect).reshape(N, -1).any(1).nonzero().reshape(-1)
        raise AssertionError("%d of %d frames differ, the first is frame %d; %d of them before the cut at %d" % (
            bad.numel(), N, int(bad[0]), int((bad < cut).sum()), cut))


# ---- the C ABI's refusals on a live handle: nothing is enqueued and `hist` is untouched
def test_c_abi_refusals_leave_hist_untouched(gpu):
    T, H, W, C = 4, 8, 8, 3
    v = _as_layout(_frames(T, H, W, C, torch.uint8, 9), "NHWC")
    hist = torch.full((T * 16,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(n=T, size=(H, W, C), fr="ok", cell_rows=16, bins=16, out="ok", h="ok"):
        if isinstance(fr, str):
            fr = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
        elif fr is not None:  # the CPU test's descriptor of 8 x 8 x 3 frames: the live tensor behind its stand-in address
            null = not fr.data
            fr = tensors._struct(v, tuple(fr.stride), fr.dtype)
            fr.data = None if null else v.data_ptr()
        out = hist.data_ptr() if out == "ok" or out == 0x9000 else out
        return gpu.L.papof_cell_hist_tensor(gpu.h if h == "ok" else h, n, size[0], size[1], size[2],
                                            ctypes.byref(fr) if fr is not None else None, cell_rows, bins, out, None)

    for kw in C_ABI_REFUSALS:
        assert call(**kw) == -1, kw
    assert call(h=None) == -1
    torch.cuda.synchronize()
    assert bool((hist == 0x5a5a5a5a).all())
    assert call() == 0  # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert hist.cpu().numpy().tobytes() == hist_reference(v.cpu().numpy()).tobytes()


# ---- the public calls
@pytest.mark.parametrize("name", ["cut at 7", "near cut", "flash at 4", "pan (4, 25) noise 5"])
def test_the_scenes_on_the_device(name):
    _, cuts, flashes = SCENES[name]
    F = scene_frames(name)
    want = hist_reference(F)
    v = _as_layout(F, "NHWC")
    _same_hist(shot_histograms(v, layout="NHWC"), want, name)
    for t, layout in ((v, "NHWC"), (v.permute(0, 3, 1, 2), "NCHW")):
        s = detect_shots(t, layout=layout)
        assert (s.cuts, s.flashes, s.gradual) == (cuts, flashes, []) and s.ranges == split_shots(T_SCENE, cuts), (name, layout)
        host = detect_cuts(tensors.ShotHist(torch.from_numpy(want), 16, 16, F.shape[1:3]))
        assert s.distances.tobytes() == host.distances.tobytes()


def _two_shots():
    """6 + 5 frames of 48 x 64 x 3 uint8 cut from the committed 1080p frame: a slow pan, a cut to a far region at pair 5"""
    img = _image()
    k = np.arange(11)
    rows = np.where(k < 6, A[0] + k, FAR[0] + k)
    cols = np.where(k < 6, A[1] + 2 * k, FAR[1] + 2 * k)
    return np.stack([img[r:r + 48, c:c + 64] for r, c in zip(rows, cols)])


@pytest.fixture(scope="module")
def two_shots(gpu):
    """the video, flow_video_shots on it (the cut detected) and flow_video_fb on each shot alone, 2 levels; the timings that
    _run_fb returned inside flow_video_shots"""
    v = _as_layout(_two_shots(), "NHWC")
    timings, run_fb = [], tensors._run_fb

    def recorder(*a, **kw):
        fb = run_fb(*a, **kw)
        timings.append(fb.timing)
        return fb
    tensors._run_fb = recorder
    try:
        fb, shots = flow_video_shots(v, 2, layout="NHWC")
    finally:
        tensors._run_fb = run_fb
    return v, fb, shots, [flow_video_fb(v[:6], 2, layout="NHWC"), flow_video_fb(v[6:], 2, layout="NHWC")], timings


def test_flow_video_shots_is_flow_video_fb_shot_by_shot(two_shots):
    v, fb, shots, alone, timings = two_shots
    assert shots.cuts == [5] and shots.ranges == [(0, 6), (6, 11)] and shots.flashes == [] and shots.gradual == []
    assert shots.distances.shape == (10,)
    for name in ("flow_fw", "flow_bw", "warpI2_fw", "warpI2_bw", "occlusion"):
        got, a, b = getattr(fb, name), getattr(alone[0], name), getattr(alone[1], name)
        assert got.shape[0] == 10 and got.dtype == a.dtype and got.is_contiguous(), name
        raw = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
        assert torch.equal(raw(got[:5]), raw(a)) and torch.equal(raw(got[6:]), raw(b)), name  # byte for byte
    for f in (fb.flow_fw, fb.flow_bw):
        assert f.dtype == torch.float64 and bool((f[5].view(torch.int64) == 0x7ff8000000000000).all())  # the quiet NaN
    assert bool(fb.occlusion[5].all()) and not bool(fb.warpI2_fw[5].any()) and not bool(fb.warpI2_bw[5].any())
    assert not bool(torch.isnan(fb.flow_fw[[4, 6]]).any())
    # the timers add: two shots, two calls
    assert len(timings) == 2 and sorted(fb.timing) == sorted(timings[0])
    for k in fb.timing:
        assert abs(float(fb.timing[k]) - (float(timings[0][k]) + float(timings[1][k]))) <= 1.5e-6, k
    # given cuts give the same flows without the detection; a FlowFB marked by cut_flows is the same again
    given, s2 = flow_video_shots(v, 2, cuts=[5], layout="NHWC")
    assert (s2.cuts, s2.ranges, s2.distances) == ([5], [(0, 6), (6, 11)], None)
    marked = cut_flows(given, [5])
    for g, w, m in zip(given[:5], fb[:5], marked[:5]):
        assert torch.equal(g.view(torch.uint8), w.view(torch.uint8)) and torch.equal(m.view(torch.uint8), w.view(torch.uint8))
    # every pair a cut: no solve at all; float32 and no mask
    none, s3 = flow_video_shots(v[:3], 2, cuts=[0, 1], layout="NHWC", out_dtype=torch.float32, consistency=None)
    assert none.occlusion is None and bool(torch.isnan(none.flow_fw).all()) and not bool(none.warpI2_bw.any())
    assert none.flow_fw.dtype == torch.float32 and s3.ranges == [(0, 1), (1, 2), (2, 3)] and float(none.timing["Phase5_SOR"]) == 0.0
    with pytest.raises(TypeError):
        flow_video_shots(v, 2, layout="NHWC", init_flow=torch.zeros((10, 2, 48, 64), device="cuda"))


def test_temporal_filter_does_not_cross_a_cut(two_shots):
    """include/papof.h (papof_temporal_filter_tensor): a chain dies at its first NaN hop and the sums keep their order, so the
    filter on the whole video with the cut pair marked is the filter on each shot alone, byte for byte"""
    v, fb, shots, alone, _ = two_shots
    whole = cut_flows(flow_video_fb(v, 2, layout="NHWC"), shots.cuts)
    assert torch.equal(whole.flow_fw[:5], alone[0].flow_fw) and torch.equal(whole.flow_bw[6:], alone[1].flow_bw)
    got = temporal_filter(v, *whole[:2], radius=2, layout="NHWC")
    a = temporal_filter(v[:6], alone[0].flow_fw, alone[0].flow_bw, radius=2, layout="NHWC")
    b = temporal_filter(v[6:], alone[1].flow_fw, alone[1].flow_bw, radius=2, layout="NHWC")
    assert torch.equal(got.video, torch.cat([a.video, b.video])) and torch.equal(got.support, torch.cat([a.support, b.support]))
    assert bool(got.support.any())


def test_no_track_is_visible_on_the_far_side_of_a_cut(two_shots):
    v, fb, shots, alone, _ = two_shots
    dense = track_points(fb.flow_fw, fb.flow_bw)
    assert bool(dense.visible[0].all()) and bool(dense.visible[:6].any(1).all()) and not bool(dense.visible[6:].any())
    q = torch.tensor([[8.0, 30.0, 20.0], [6.0, 10.0, 40.0], [5.0, 31.0, 24.0]], dtype=torch.float64, device="cuda")
    tr = track_points(fb.flow_fw, fb.flow_bw, q)
    assert bool(tr.visible[8, 0]) and bool(tr.visible[6, 1]) and bool(tr.visible[5, 2])
    assert not bool(tr.visible[:6, :2].any()) and not bool(tr.visible[6:, 2].any())
    assert bool(torch.isnan(tr.tracks[:6, :2]).all())


def test_the_call_is_ordered_on_the_callers_stream():
    """Frames written on a side stream behind a long sleep, reduced under that stream with no synchronisation: the kernel must
    read them after they are written, and what is queued behind it must see its output"""
    import time
    n = _frames(4, 40, 130, 3, torch.uint8, 12)
    want = hist_reference(n)
    src = _as_layout(n, "NHWC")
    dst = torch.zeros_like(src)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = shot_histograms(dst, layout="NHWC").hist.clone()
    assert not torch.equal(warm.cpu(), torch.from_numpy(want))
    torch.cuda.synchronize()
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
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the call
        after.record()
        dst.copy_(src)
        got = shot_histograms(dst, layout="NHWC")
        copy = got.hist.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    assert before.elapsed_time(after) > 150.0, "the sleep in front of the frames took %.1f ms" % before.elapsed_time(after)
    _same_hist(got, want, "side stream")
    assert copy.cpu().numpy().tobytes() == want.tobytes()
