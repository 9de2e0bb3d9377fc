"""Point tracking on device tensors (papteam_opticalflow_amd/tensors.py: track_points, track_video -> papof_track_tensor).
The tracks must be the BITS of the numpy fp64 restatement (tests/test_track_cpu.py: track_reference), compared as integer
views so that a NaN's payload or a zero's sign is caught, and visible must equal it exactly: on synthetic fields with NaNs,
infinities and large displacements, float32 and float64 flows, strided views, queries in the middle of the clip, invalid
queries, without the check, from T = 2 to a clip of 300 frames, densely at 1080p, and on the committed video through
track_video."""
import math

import numpy as np
import pytest

from test_fb_cpu import fb_reference
from test_gpu_batch import _video
from test_gpu_tensors import _dev, _same_bits
from test_track_cpu import track_reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same_tracks(got, want, what):
    tracks, vis = want
    assert tuple(got.tracks.shape) == tracks.shape and got.tracks.dtype == torch.float64, (what, tuple(got.tracks.shape))
    assert tuple(got.visible.shape) == vis.shape and got.visible.dtype == torch.bool, (what, tuple(got.visible.shape))
    g = got.visible.cpu().numpy()
    if not np.array_equal(g, vis):
        raise AssertionError("%s: visible differs at %d of %d entries" % (what, int((g != vis).sum()), g.size))
    _same_bits(got.tracks, tracks, what + " tracks")


def _fields(T, H, W, seed, amp=2.0, noise=0.05, wild=True):
    """T - 1 smooth random flow pairs (T - 1, 2, H, W) whose backward flow roughly undoes the forward one -- plus, when
    `wild`, NaNs, infinities and a patch of large displacements in both directions"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fw = np.empty((T - 1, 2, H, W))
    for t in range(T - 1):
        for c in range(2):
            k, ph = rng.uniform(0.02, 0.2, 2), rng.uniform(0, 2 * math.pi, 2)
            fw[t, c] = amp * np.sin(k[0] * x + ph[0]) * np.cos(k[1] * y + ph[1])
    bw = -fw + rng.normal(0, noise, fw.shape)
    if wild:
        for f in (fw, bw):
            n = max(1, f[:, 0].size // 400)
            for val in (math.nan, math.inf, -math.inf):
                idx = tuple(rng.integers(0, s, n) for s in (T - 1, 2, H, W))
                f[idx] = val
            r0, c0 = rng.integers(0, H // 2), rng.integers(0, W // 2)
            f[:, 0, r0:r0 + H // 4, c0:c0 + W // 4] = rng.uniform(-W, W)  # large displacements
            f[:, 1, r0:r0 + H // 4, c0:c0 + W // 4] = rng.uniform(-H / 3, H / 3)
    return fw, bw


def _queries(T, H, W, n, seed, invalid=True):
    """n queries (t0, x, y) spread over the clip, integer and fractional positions, edges included -- and each kind of
    invalid one"""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.integers(0, T, n).astype(np.float64), rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], 1)
    q[::5, 1:] = np.round(q[::5, 1:])
    q[1, :] = (T - 1, W - 1, H - 1)
    q[2, :] = (0, 0, 0)
    if invalid:
        bad = [[-1, 1, 1], [T, 1, 1], [0.5, 1, 1], [math.nan, 1, 1], [0, math.nan, 1], [0, 1, math.inf],
               [0, -0.25, 1], [0, W - 0.5, 1], [0, 1, -1e-300], [0, 1, H - 1 + 1e-9]]
        q = np.concatenate([q, bad])
    return q


def test_queries_on_synthetic_fields_float64_and_float32(gpu):
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 9, 37, 53
    fw, bw = _fields(T, H, W, 1)
    q = _queries(T, H, W, 700, 2)
    tf, tb, tq = (torch.from_numpy(a).cuda() for a in (fw, bw, q))
    want = track_reference(fw, bw, q)
    assert 0.2 < want[1].mean() < 0.95  # points are kept and lost
    assert want[1][:, :-10].any(1).all() and want[1][0].any() and want[1][-1].any()  # both directions reach the ends
    _same_tracks(track_points(tf, tb, tq), want, "float64")
    f32, b32, q32 = tf.float(), tb.float(), tq.float()
    w32 = track_reference(f32.cpu().numpy(), b32.cpu().numpy(), q32.cpu().numpy())
    _same_tracks(track_points(f32, b32, q32), w32, "float32")
    _same_tracks(track_points(f32, tb, tq), track_reference(f32.cpu().numpy(), bw, q), "float32 forward, float64 backward")
    for a1, a2 in ((0.05, 1.0), (0.0, 0.0)):
        _same_tracks(track_points(tf, tb, tq, consistency=(a1, a2)), track_reference(fw, bw, q, a1, a2),
                     "alphas %g %g" % (a1, a2))
    none = track_points(tf, tb, tq, consistency=None)
    _same_tracks(none, track_reference(fw, bw, q, check=False), "consistency=None")
    assert none.visible.sum() > track_points(tf, tb, tq).visible.sum()


def test_dense_on_synthetic_fields(gpu):
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 7, 45, 131  # tiles cut at both edges
    fw, bw = _fields(T, H, W, 3)
    want = track_reference(fw, bw)
    assert 0.2 < want[1].mean() < 0.95
    _same_tracks(track_points(torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()), want, "dense")
    _same_tracks(track_points(torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), consistency=None),
                 track_reference(fw, bw, check=False), "dense, consistency=None")


def test_strided_views_of_flows_and_queries(gpu):
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 6, 29, 41
    fw, bw = _fields(T, H, W, 4)
    # (T - 1, H, 2W, 2) laid out channels-last, read as (T - 1, 2, H, W) of odd strides
    big = torch.from_numpy(np.ascontiguousarray(np.concatenate([fw, fw], axis=3).transpose(0, 2, 3, 1))).cuda()
    view = big.permute(0, 3, 1, 2)[:, :, 1:, 3::2]
    assert not view.is_contiguous()
    bv = torch.from_numpy(bw).cuda()[:, :, 1:, 1:]
    q = _queries(T, H - 1, W - 1, 300, 5)
    qt = torch.from_numpy(np.ascontiguousarray(q.T)).cuda().t()  # column-major rows: stride (1, N)
    qs = torch.from_numpy(np.repeat(q, 2, axis=0)).cuda()[::2]  # every other row
    want = track_reference(view.cpu().numpy(), bv.cpu().numpy(), q)
    _same_tracks(track_points(view, bv, qt), want, "permuted flows, transposed queries")
    _same_tracks(track_points(view, bv, qs), want, "sliced queries")
    rev = track_points(view.flip(0), bv.flip(0), qs)
    _same_tracks(rev, track_reference(view.flip(0).cpu().numpy(), bv.flip(0).cpu().numpy(), q), "reversed pairs")
    _same_tracks(track_points(view, bv), track_reference(view.cpu().numpy(), bv.cpu().numpy()), "dense on views")


def test_two_frames(gpu):
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 2, 19, 23
    fw, bw = _fields(T, H, W, 6)
    q = _queries(T, H, W, 100, 7)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    _same_tracks(track_points(tf, tb, torch.from_numpy(q).cuda()), track_reference(fw, bw, q), "T = 2 queries")
    _same_tracks(track_points(tf, tb), track_reference(fw, bw), "T = 2 dense")


def test_a_long_clip(gpu):
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 300, 48, 64
    fw, bw = _fields(T, H, W, 8, amp=0.6, noise=0.02, wild=False)
    tf, tb = torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()
    want = track_reference(fw, bw)
    assert want[1][-1].any()  # some points survive the clip
    _same_tracks(track_points(tf, tb), want, "300 frames dense")
    q = _queries(T, H, W, 500, 9)
    _same_tracks(track_points(tf, tb, torch.from_numpy(q).cuda()), track_reference(fw, bw, q), "300 frames queries")


def test_dense_1080p(gpu):
    """N = 1920 * 1080 points: a 30 x 270 grid of tiles, 64-bit offsets into (T, N, 2)"""
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 3, 1080, 1920
    fw, bw = _fields(T, H, W, 10, wild=True)
    got = track_points(torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda())
    _same_tracks(got, track_reference(fw, bw), "1080p dense")


def test_dense_grid_split_of_a_tall_clip(gpu):
    """1 x 262148 pixels: 65537 rows of tiles, more than gridDim.y takes -- the dense launch is split in two"""
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 3, 4 * 65535 + 8, 1
    fw, bw = _fields(T, H, W, 11, amp=0.0, noise=0.0, wild=False)
    fw[:, 1], bw[:, 1] = 0.5, -0.5
    fw[:, 1, -6:], bw[:, 1, -6:] = 3.0, 7.0  # the last rows: lost (leave, or fail the check) in the second launch's tiles
    want = track_reference(fw, bw)
    assert not want[1][2, -6:].any() and want[1][2, :-8].all()
    _same_tracks(track_points(torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda()), want, "tall dense")


@pytest.fixture(scope="module")
def video9(gpu):
    """the 240x135 video of 9 frames (uint8 HWC) on the device, and flow_video_fb's result with its check"""
    from papteam_opticalflow_amd.tensors import flow_video_fb
    v = _dev(_video("240", 9))
    return v, flow_video_fb(v, 4, layout="NHWC")


def test_track_video_is_flow_video_fb_and_the_definition(video9):
    from papteam_opticalflow_amd.tensors import track_video
    v, fb = video9
    fw, bw = fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy()
    q = _queries(9, 135, 240, 400, 12)
    tv = track_video(v, 4, torch.from_numpy(q).cuda(), layout="NHWC")
    _same_bits(tv.flow_fw, fb.flow_fw, "track_video flow_fw")
    _same_bits(tv.flow_bw, fb.flow_bw, "track_video flow_bw")
    assert float(tv.timing["Total C++ Execution"]) > 0
    want = track_reference(fw, bw, q)
    assert want[1].sum() > len(q)  # points move visibly
    _same_tracks(tv, want, "track_video queries")
    dense = track_video(v.permute(0, 3, 1, 2), 4, consistency=(0.05, 1.0))
    _same_tracks(dense, track_reference(fw, bw, None, 0.05, 1.0), "track_video dense NCHW")


def test_dense_first_step_is_the_occlusion_mask(video9):
    from papteam_opticalflow_amd.tensors import track_points
    _, fb = video9
    assert torch.isfinite(fb.flow_fw).all() and torch.isfinite(fb.flow_bw).all()
    tr = track_points(fb.flow_fw, fb.flow_bw)
    occ = fb.occlusion[0, 0].reshape(-1)
    assert torch.equal(tr.visible[1], ~occ)
    assert np.array_equal(~fb_reference(fb.flow_fw.cpu().numpy(), fb.flow_bw.cpu().numpy())[0, 0].astype(bool).reshape(-1),
                          tr.visible[1].cpu().numpy())


def test_the_call_is_ordered_on_the_callers_stream(gpu):
    """Flows written on a side stream behind a long sleep and tracked under that stream with no synchronisation: the kernel
    must read them after they are written, and what is queued behind it must see its tracks"""
    import time
    from papteam_opticalflow_amd.tensors import track_points
    T, H, W = 12, 40, 60
    fw, bw = _fields(T, H, W, 13)
    q = _queries(T, H, W, 256, 14)
    want = track_reference(fw, bw, q)
    src = [torch.from_numpy(a).cuda() for a in (fw, bw)]
    dst = [torch.zeros_like(s) for s in src]
    tq = torch.from_numpy(q).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist: nothing below allocates from the device
        warm = track_points(dst[0], dst[1], tq)
        warm = warm.tracks.clone(), warm.visible.clone()
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
        got = track_points(dst[0], dst[1], tq)
        took = time.perf_counter() - t0
        copy = got.tracks.clone(), got.visible.clone()  # queued behind the kernel on the same stream
    side.synchronize()
    assert took < 0.25, "track_points waited for the stream: %.3f s" % took
    _same_tracks(got, want, "side stream")
    _same_bits(copy[0], want[0], "side stream clone of the tracks")
    assert np.array_equal(copy[1].cpu().numpy(), want[1])
