"""Inverse telecine on device tensors (papteam_opticalflow_amd/tensors.py: field_metrics, match_fields, weave_fields,
inverse_telecine, inverse_telecine_video -> papof_field_metrics_tensor, papof_weave_fields_tensor).  The device's counts and
videos must be the BYTES of the numpy restatement (tests/_telecine_ref.py), compared as raw bytes: uint8, float32 and float64
fields (floats with NaNs and values beyond 0 .. 1) of 1 .. 4 channels, NCHW, NHWC, strided and channel-expanded views, both
parities, 3, 4 and 7 fields, cells of 1, 16 and 64 rows, fields without a centre row, with partial cells and across the
64-column and cell-row seams, the thresholds' ends, a dense 540 x 1920 case, a `metrics` buffer that held two different
patterns; the weave for every dtype pair, repeated and out-of-order fields, a strided video through the C ABI; the public calls
against their parts chained by hand, the scenes of tests/test_telecine_cpu.py, and the caller's stream order."""
import ctypes

import numpy as np
import pytest

from _deinterlace_ref import deinterlace_reference
from _telecine_ref import match_reference, metrics_reference, plan_reference, threshold_q, weave_reference
from test_gpu_denoise import _as_layout, _same_bytes
from test_gpu_tensors import _dev
from test_telecine_cpu import SCENES, scene_fields, scene_match, truth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (bob_fields, deinterlace_fields, field_flows, field_metrics,  # noqa: E402
                                             inverse_telecine, inverse_telecine_video, match_fields, weave_fields)

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, None: None}
COMB, DIFF = threshold_q(10 / 255), threshold_q(8 / 255)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _fields(T, Hf, W, C, dtype, seed):
    """fields that comb against one neighbour more than against the other at many pixels: a smooth ramp plus noise whose
    size differs from field to field; floats reach beyond 0 .. 1 and hold NaNs and infinities"""
    rng = np.random.default_rng(seed)
    base = 128.0 + 60.0 * np.sin(np.arange(Hf)[:, None, None] * 0.7 + np.arange(W)[None, :, None] * 0.11 + np.arange(C))
    f = np.stack([base + rng.normal(0, (3, 25, 8)[(k + seed) % 3], base.shape) for k in range(T)])
    if dtype == torch.uint8:
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    f = ((f - 128.0) / 100.0 + 0.5).astype(_NP[dtype])  # about -0.4 .. 1.4
    flat = f.reshape(-1)
    idx = rng.integers(0, flat.size, max(3, flat.size // 50))
    flat[idx[0::3]], flat[idx[1::3]], flat[idx[2::3]] = np.nan, np.inf, -np.inf
    return f


def _same_counts(got, want, what):
    assert got.counts.dtype == torch.int32 and tuple(got.counts.shape) == want.shape, (what, got.counts.shape, want.shape)
    g = got.counts.cpu().numpy()
    bad = g != want
    assert not bad.any(), "%s: %d of %d counts differ; first at %s: %d for %d" % (
        what, int(bad.sum()), bad.size, tuple(int(k[0]) for k in np.nonzero(bad)), g[bad][0], want[bad][0])


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_counts_every_dtype(dtype, layout):
    Hf, W = 37, 150
    for T, C in ((3, 3), (4, 1), (7, 4), (4, 2)):
        n = _fields(T, Hf, W, C, dtype, T + C)
        v = _as_layout(n, layout)
        for first in (0, 1):
            for cell_rows in (1, 16, 64):
                want = metrics_reference(n, first, cell_rows, COMB, DIFF)
                assert want[1:-1, 0].any() and want[1:-1, 1].any() and want[1:-1, 2].any() and not want[[0, -1]].any()
                got = field_metrics(v, first, cell_rows=cell_rows, layout=layout)
                assert (got.cell_rows, got.first) == (cell_rows, first)
                _same_counts(got, want, "%s %s T %d C %d first %d cell_rows %d" % (dtype, layout, T, C, first, cell_rows))


@pytest.mark.parametrize("Hf,W", [(1, 70), (2, 3), (30, 1), (17, 63), (16, 64), (33, 65), (9, 130)])
def test_counts_edge_shapes(Hf, W):
    """no centre row at all (one row), partial cells, and the 64-column and cell-row seams"""
    for dtype, C in ((torch.uint8, 3), (torch.float32, 2)):
        n = _fields(5, Hf, W, C, dtype, 3)
        for first in (0, 1):
            for cell_rows in (1, 16):
                want = metrics_reference(n, first, cell_rows, COMB, DIFF)
                assert not want.any() if Hf == 1 else want.any() or Hf * W < 30
                _same_counts(field_metrics(_as_layout(n, "NHWC"), first, cell_rows=cell_rows, layout="NHWC"), want,
                             "%d x %d %s first %d cell_rows %d" % (Hf, W, dtype, first, cell_rows))


def test_counts_at_the_thresholds_ends():
    n = _fields(4, 20, 70, 3, torch.uint8, 5)
    n[1, 3, 5], n[0, 2:4, 5], n[2, 2:4, 5] = 0, 0, 255  # a comb and a difference of the full range
    v = _as_layout(n, "NHWC")
    for comb, diff in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)):
        want = metrics_reference(n, 1, 16, threshold_q(comb), threshold_q(diff))
        _same_counts(field_metrics(v, 1, comb_threshold=comb, diff_threshold=diff, layout="NHWC"), want, "thresholds %s %s" % (comb, diff))
        if comb == 1.0:
            assert not want[:, :2].any()  # nothing exceeds 65535
        if diff == 0.0:
            assert want[1:-1, 2].any()


def test_counts_of_strided_and_expanded_views():
    T, Hf, W, C = 5, 29, 75, 3
    big = torch.from_numpy(_fields(2 * T, Hf + 3, 2 * W, C + 1, torch.uint8, 6)).cuda()
    v = big[::2, 2:Hf + 2, ::2, 1:]  # every other field, rows cut, every other column, channels cut
    assert not v.is_contiguous()
    want = metrics_reference(v.cpu().numpy(), 1, 16, COMB, DIFF)
    _same_counts(field_metrics(v, 1, layout="NHWC"), want, "strided NHWC")
    _same_counts(field_metrics(v.permute(0, 3, 1, 2), 1), want, "strided NCHW")
    one = v.permute(0, 3, 1, 2)[:, 1:2].expand(T, 4, Hf, W)  # one channel read four times: a zero stride
    _same_counts(field_metrics(one), metrics_reference(v.cpu().numpy()[..., [1] * 4], 0, 16, COMB, DIFF), "expanded channel")
    same = v[2:3].expand(3, Hf, W, C)  # one field three times, a zero field stride: no pixel can differ
    assert not field_metrics(same, layout="NHWC").counts.any()


@pytest.mark.parametrize("C", [1, 3, 4])
def test_counts_of_packed_rows_at_every_alignment(C):
    """packed uint8 rows are loaded as aligned dwords: the same fields at byte offsets 0 .. 3 of one buffer, in rows whose
    length is no multiple of 4 -- with four channels and a misaligned start a full cell spans 65 dwords"""
    T, Hf, W = 4, 19, 131
    n = _fields(T, Hf, W, C, torch.uint8, 20 + C)
    want = metrics_reference(n, 0, 16, COMB, DIFF)
    flat = torch.from_numpy(n).reshape(-1)
    for off in range(4):
        buf = torch.full((flat.numel() + 8,), 255, dtype=torch.uint8, device="cuda")
        buf[off:off + flat.numel()] = flat.cuda()
        v = buf[off:off + flat.numel()].view(T, Hf, W, C)
        assert v.data_ptr() % 4 == off and v.is_contiguous()
        _same_counts(field_metrics(v, layout="NHWC"), want, "C %d offset %d" % (C, off))


def test_dense_540x1920():
    n = _fields(4, 540, 1920, 3, torch.uint8, 10)
    _same_counts(field_metrics(_as_layout(n, "NHWC"), layout="NHWC"), metrics_reference(n, 0, 16, COMB, DIFF), "540 x 1920")


def test_the_counts_do_not_depend_on_what_the_buffer_held():
    T, Hf, W, C = 5, 21, 140, 3
    n = _fields(T, Hf, W, C, torch.uint8, 7)
    v = _dev(list(n))
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    want = metrics_reference(n, 0, 16, COMB, DIFF)
    guard = 64
    buf = torch.empty(want.size + 2 * guard, dtype=torch.int32, device="cuda")
    for pattern in (0x5a5a5a5a, -1):
        buf.fill_(pattern if pattern < 2 ** 31 else pattern - 2 ** 32)
        tensors._launch(v.device, "papof_field_metrics_tensor", T, Hf, W, C, ctypes.byref(d_in), 0, 16, COMB, DIFF,
                        ctypes.c_void_p(buf[guard:].data_ptr()))
        got = buf.cpu().numpy()
        assert (got[guard:-guard].reshape(want.shape) == want).all(), hex(pattern & 0xffffffff)
        assert (got[:guard] == got[0]).all() and (got[-guard:] == got[0]).all() and got[0] != 0  # nothing beyond the table


# ---- the weave
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_weave_every_dtype_pair(dtype, layout):
    T, Hf, W = 6, 19, 70
    table = np.array([[0, 1], [3, 2], [5, 5], [1, 0], [4, 2], [0, 1]])  # repeated, out of order, one field twice
    for C in (1, 2, 3, 4):
        n = _fields(T, Hf, W, C, dtype, 11 + C)
        v = _as_layout(n, layout)
        for odt in (None, torch.uint8, torch.float32, torch.float64):
            tab = torch.from_numpy(table).to(torch.int16).cuda() if C == 2 else table if C == 3 else torch.from_numpy(table)
            got = weave_fields(v, tab, layout=layout, out_dtype=odt)
            _same_bytes(got, weave_reference(n, table, _NP[odt]), layout, "%s -> %s %s C %d" % (dtype, odt, layout, C))


def test_weave_uint8_rows_are_the_inputs_bytes_and_edge_shapes():
    rng = np.random.default_rng(14)
    for Hf, W in ((12, 37), (1, 70), (30, 1), (9, 130)):
        n = rng.integers(0, 256, (4, Hf, W, 3)).astype(np.uint8)
        n.reshape(-1)[:min(256, n.size)] = np.arange(min(256, n.size))  # every byte value occurs
        v = _dev(list(n))
        got = weave_fields(v, [[2, 1], [0, 3]], layout="NHWC")
        assert got.dtype == torch.uint8 and got.shape == (2, 2 * Hf, W, 3)
        assert torch.equal(got[0, 0::2], v[2]) and torch.equal(got[0, 1::2], v[1])
        assert torch.equal(got[1, 0::2], v[0]) and torch.equal(got[1, 1::2], v[3])


def test_weave_into_a_strided_video_through_the_c_abi():
    T, Hf, W, C = 4, 20, 66, 2
    n = _fields(T, Hf, W, C, torch.float64, 8)
    v = _dev(list(n))
    d_in = tensors._struct(v, *tensors.descriptor(v, "NHWC")[1:])
    strided = torch.zeros((3, 2 * Hf, 2 * W, C), dtype=torch.float32, device="cuda")  # the video into every other column
    view = strided[:, :, ::2]
    d_out = tensors._struct(view, *tensors.descriptor(view, "NHWC")[1:])
    table = np.array([[0, 1], [3, 2], [2, 2]])
    tab = torch.from_numpy(table).to(torch.int32).cuda()
    tensors._launch(v.device, "papof_weave_fields_tensor", T, Hf, W, C, ctypes.byref(d_in), 3, ctypes.c_void_p(tab.data_ptr()),
                    ctypes.byref(d_out))
    _same_bytes(view, weave_reference(n, table, np.float32), "NHWC", "strided video")
    assert not strided[:, :, 1::2].any()


# ---- the public calls and the scenes
def _expected(F, first, orphans, frames_of_orphans, **rule):
    """the restatement's Detelecined of uint8 fields F: (video, groups, times, kinds, match)"""
    counts = metrics_reference(F, first, **rule)
    match = match_reference(counts)
    table, keep, times, kinds = plan_reference(match[2], first, orphans)
    video = weave_reference(F, table)
    if kinds.any():
        video[kinds != 0] = frames_of_orphans()[table[kinds != 0][:, 0]]
    return video, match[2][keep], times, kinds, match


def _check_detelecined(got, want, what):
    video, groups, times, kinds, match = want
    _same_bytes(got.video, video, "NHWC", what + " video")
    assert got.groups.tolist() == groups.tolist() and got.times.tolist() == times.tolist(), what
    assert got.kinds.tolist() == kinds.tolist() and got.times.dtype == torch.float64 and got.kinds.dtype == torch.uint8, what
    assert got.match.votes.tolist() == match[0].tolist() and got.match.links.tolist() == match[1].tolist(), what
    assert got.match.groups.tolist() == match[2].tolist() and (got.match.cadence, got.match.share) == match[3:], what


@pytest.mark.parametrize("name", [s[0] for s in SCENES])
def test_the_scenes_on_the_device(name):
    """the scenes of tests/test_telecine_cpu.py: the device's counts, links, groups and video are the restatement's, and the
    links are the truth"""
    _, seq, _, _, _, comb = next(s for s in SCENES if s[0] == name)
    F = scene_fields(name)
    counts = scene_match(name)[0]
    kw = {} if comb is None else dict(comb_threshold=comb)
    v = _dev(list(F))
    _same_counts(field_metrics(v, layout="NHWC", **kw), counts, name)
    rule = {} if comb is None else dict(comb_q=threshold_q(comb))
    got = inverse_telecine(v, layout="NHWC", **kw)
    _check_detelecined(got, _expected(F, 0, "bob", lambda: deinterlace_reference(F, mode=0)[0], **rule), name)
    assert got.match.links.tolist() == truth(seq).tolist()


def test_the_cut_scene_with_every_orphan_rule():
    name = "3:2 with a cut"
    F = scene_fields(name)
    v = _dev(list(F))
    drop = inverse_telecine(v, orphans="drop", layout="NHWC")
    _check_detelecined(drop, _expected(F, 0, "drop", None), "drop")
    assert drop.video.shape[0] == 7 and not drop.kinds.any()
    iv = inverse_telecine_video(v, 3, layout="NHWC")
    assert iv.kinds.tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and iv.flow_fw.shape == (len(F) - 2, 2, 60, 200) and iv.timing
    fw, bw = iv.flow_fw.cpu().numpy(), iv.flow_bw.cpu().numpy()
    want = _expected(F, 0, "mc", lambda: deinterlace_reference(F, fw, bw, sigma=tensors.DEINT_SIGMA)[0])
    _check_detelecined(iv, want, "inverse_telecine_video")
    mc = inverse_telecine(v, orphans="mc", flow_fw=iv.flow_fw, flow_bw=iv.flow_bw, layout="NHWC")
    _check_detelecined(mc, want, "mc")
    bob = inverse_telecine(v, layout="NHWC")
    assert torch.equal(bob.video[bob.kinds == 0], mc.video[mc.kinds == 0]) and torch.equal(bob.video[bob.kinds == 0], drop.video)
    assert not torch.equal(bob.video[4], mc.video[4])


def test_the_public_calls_are_their_parts():
    name = "3:2 with a cut"
    F = scene_fields(name)
    v = _dev(list(F))
    for layout, first, odt in (("NHWC", 0, None), ("NCHW", 1, torch.float32)):
        t = v if layout == "NHWC" else v.permute(0, 3, 1, 2)
        m = match_fields(field_metrics(t, first, cell_rows=8, comb_threshold=0.05, layout=layout), margin=6, dominance=2)
        table, keep, times, kinds = tensors.telecine_plan(m.groups.numpy(), first, "bob")
        assert kinds.any() and not kinds.all()
        video = weave_fields(t, table, layout=layout, out_dtype=odt)
        orphan = torch.from_numpy(kinds != 0)
        video[orphan.cuda()] = bob_fields(t, first, layout=layout, out_dtype=odt)[torch.from_numpy(table[:, 0])[orphan].cuda()]
        kw = dict(cell_rows=8, comb_threshold=0.05, margin=6, dominance=2, layout=layout, out_dtype=odt)
        got = inverse_telecine(t, first, **kw)
        assert torch.equal(got.video, video) and got.video.dtype == (odt or torch.uint8)
        assert got.groups.tolist() == m.groups.tolist() and got.times.tolist() == times.tolist() and got.kinds.tolist() == kinds.tolist()
        assert torch.equal(got.match.votes, m.votes) and (got.match.cadence, got.match.share) == (m.cadence, m.share)
        ff = field_flows(t, 3, layout=layout)
        video[orphan.cuda()] = deinterlace_fields(t, ff.flow_fw, ff.flow_bw, first, sigma=0.1, layout=layout,
                                                  out_dtype=odt).video[torch.from_numpy(table[:, 0])[orphan].cuda()]
        iv = inverse_telecine_video(t, 3, first, sigma=0.1, **kw)
        assert torch.equal(iv.video, video) and torch.equal(iv.flow_fw, ff.flow_fw) and torch.equal(iv.flow_bw, ff.flow_bw)
        assert sorted(iv.timing) == sorted(ff.timing) and iv.kinds.tolist() == kinds.tolist()
    # no orphan: no flows are computed
    iv = inverse_telecine_video(_dev(list(scene_fields("3:2 pan (3, 1)"))), 3, layout="NHWC")
    assert iv.flow_fw is None and iv.flow_bw is None and iv.timing is None and not iv.kinds.any() and iv.match.cadence == "3:2"
    # three fields: an orphan can only be dropped
    three = v[3:6]  # B B C
    assert inverse_telecine(three, 1, orphans="drop", layout="NHWC").groups.tolist() == [[0, 2]]
    with pytest.raises(ValueError):
        inverse_telecine(three, 1, layout="NHWC")


def test_the_calls_are_ordered_on_the_callers_stream():
    """Fields written on a side stream behind a long sleep, measured and woven under that stream with no synchronisation: the
    kernels must read them after they are written, and what is queued behind them must see their outputs"""
    import time
    T, Hf, W, C = 6, 40, 130, 3
    n = _fields(T, Hf, W, C, torch.uint8, 12)
    table = np.array([[0, 1], [3, 2], [4, 5]])
    want, want_video = metrics_reference(n, 1, 16, COMB, DIFF), weave_reference(n, table)
    src = _dev(list(n))
    dst = torch.zeros_like(src)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = (field_metrics(dst, 1, layout="NHWC").counts.clone(), weave_fields(dst, table, layout="NHWC").clone())
    del warm
    torch.cuda.synchronize()
    # The rate of the sleep kernel's clock: 50 M cycles are some 20 ms, so the first use of the kernel or a stall of the
    # host inside one timed window would make the clock look several times slower and the sleep below as much shorter.  A
    # stall can only lengthen a window: the shortest of three is taken, and the sleep's own length is checked below.
    with torch.cuda.stream(side):
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
        got = field_metrics(dst, 1, layout="NHWC")
        video = weave_fields(dst, table, layout="NHWC")
        copies = (got.counts.clone(), video.clone())  # queued behind the kernels on the same stream
    side.synchronize()
    assert before.elapsed_time(after) > 150.0, "the sleep in front of the fields took %.1f ms" % before.elapsed_time(after)
    _same_counts(got, want, "side stream")
    assert (copies[0].cpu().numpy() == want).all()
    _same_bytes(video, want_video, "NHWC", "side stream weave")
    _same_bytes(copies[1], want_video, "NHWC", "side stream clone")
