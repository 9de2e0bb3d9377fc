"""Video stabilization on device tensors (papteam_opticalflow_amd/tensors.py: global_motion, warp_affine, stabilize_video ->
papof_motion_fit_tensor, papof_warp_affine_tensor).  The device's fit must agree with the numpy fp64 restatement
(tests/_stab_ref.py: fit_reference) within 1e-8 px at the image corners -- the sums are added in another order, so not bit
for bit -- and be bitwise the same from run to run; the warp must be the BYTES of warp_reference.  Float32 and float64
flows, strided views, with and without a mask, synthetic flows with NaNs, a 1080p pair and 100 pairs of 240x135; uint8,
float32 and float64 frames in and out, NCHW, NHWC and strided views, matrices that leave the image; the caller's stream
order; and stabilize_video end to end on a jittered video cut from the committed 480x270 frame."""
import math

import numpy as np
import pytest

from _interp_ref import _sample, _taps, as_f64
from _stab_ref import AFFINE, SIMILARITY, corner_distance, fit_reference, warp_reference
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}
_MODELS = {SIMILARITY: "similarity", AFFINE: "affine"}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _affine_flows(B, H, W, seed, outliers=0.2):
    """B flows of random affine motions plus noise, gross outliers and the NaNs, infinities and large displacements of
    test_gpu_track._fields"""
    rng = np.random.default_rng(seed)
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    wild, _ = _fields(B + 1, H, W, seed)
    f = np.empty((B, 2, H, W))
    for i in range(B):
        L = np.eye(2) + rng.normal(0, 0.01, (2, 2))
        t = rng.normal(0, 2, 2)
        f[i, 0] = L[0, 0] * x + L[0, 1] * r + t[0] - x
        f[i, 1] = L[1, 0] * x + L[1, 1] * r + t[1] - r
    f += rng.normal(0, 0.2, f.shape)
    bad = rng.random((B, H, W)) < outliers
    f[:, 0][bad] += rng.uniform(-15, 15, int(bad.sum()))
    with np.errstate(invalid="ignore"):
        keep = ~np.isfinite(wild) | (np.abs(wild) > 3)  # _fields' NaNs, infinities and large-displacement patch
    f[keep] = wild[keep]
    return f


def _mask(B, H, W, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((B, 2, H, W)) < 0.1).astype(np.uint8)
    m[:, 0, H // 4:H // 2, W // 3:W // 2] = 1
    return m


def _check_fit(got, flow, occ, model, iters, what, scale=1.0):
    """the device's Motion against fit_reference: corners within 1e-8 px, ok equal, support within 1e-12"""
    motion, ok, sup = fit_reference(flow, occ, model, iters, scale)
    H, W = flow.shape[2:]
    gm, gok, gs = got.motion.cpu().numpy(), got.ok.cpu().numpy(), got.support.cpu().numpy()
    assert (gok == ok).all(), (what, gok, ok)
    d = max(corner_distance(gm[i], motion[i], H, W) for i in range(len(ok)))
    assert d < 1e-8, (what, d)
    assert np.abs(gs - sup).max() < 1e-12, what
    return d


@pytest.mark.parametrize("model", [SIMILARITY, AFFINE])
def test_fit_matches_the_restatement(model):
    from papteam_opticalflow_amd.tensors import global_motion
    B, H, W = 3, 70, 93
    f = _affine_flows(B, H, W, 1)
    occ = _mask(B, H, W, 2)
    for fdt in (torch.float64, torch.float32):
        tf = torch.from_numpy(f).to(fdt).cuda()
        nf = tf.cpu().numpy()
        for m in (None, occ):
            tm = torch.from_numpy(m).cuda().bool() if m is not None else None
            for iters in (1, 5):
                got = global_motion(tf, occlusion=tm, model=_MODELS[model], iters=iters, scale=1.5)
                _check_fit(got, nf, m, model, iters, "%s %s mask %s iters %d" % (model, fdt, m is not None, iters), 1.5)


def test_fit_strided_views_and_failed_pairs():
    from papteam_opticalflow_amd.tensors import global_motion
    B, H, W = 4, 50, 67
    f = _affine_flows(B, H, W, 3)
    f[2] = math.nan                                   # no valid pixel: the identity, not ok
    f[3, :, :, :] = math.nan
    f[3, :, :, 10] = 0.0                              # one valid column: iteration 0 fails at a pivot
    big = torch.from_numpy(np.ascontiguousarray(f.transpose(0, 2, 3, 1))).cuda()  # (B, H, W, 2) read as (B, 2, H, W)
    tf = big.permute(0, 3, 1, 2)
    wide = torch.from_numpy(np.repeat(_mask(B, H, W, 4), 2, axis=3)).cuda()[:, :, :, ::2]
    assert not tf.is_contiguous() and not wide.is_contiguous()
    for model in (SIMILARITY, AFFINE):
        got = global_motion(tf, occlusion=wide, model=_MODELS[model])
        _check_fit(got, f, wide.cpu().numpy(), model, 5, "strided %d" % model)
        assert got.ok.cpu().tolist() == [True, True, False, model == SIMILARITY]  # one column still fixes a similarity
        assert torch.equal(got.motion[2].cpu(), torch.eye(2, 3, dtype=torch.float64))


def test_fit_on_the_synthetic_fields_of_the_tracking_tests():
    from papteam_opticalflow_amd.tensors import global_motion
    fw, _ = _fields(3, 37, 53, 5)
    for model in (SIMILARITY, AFFINE):
        got = global_motion(torch.from_numpy(fw).cuda(), model=_MODELS[model], scale=2.0)
        _check_fit(got, fw, None, model, 5, "fields %d" % model, 2.0)


def test_fit_1080p_and_a_hundred_small_pairs_are_reproducible():
    from papteam_opticalflow_amd.tensors import global_motion
    for B, H, W, seed in ((1, 1080, 1920, 6), (100, 135, 240, 7)):
        f = _affine_flows(B, H, W, seed)
        tf = torch.from_numpy(f).cuda()
        for model in (SIMILARITY, AFFINE):
            a = global_motion(tf, model=_MODELS[model])
            b = global_motion(tf, model=_MODELS[model])
            torch.cuda.synchronize()
            assert a.motion.cpu().numpy().tobytes() == b.motion.cpu().numpy().tobytes()
            assert torch.equal(a.support, b.support) and torch.equal(a.ok, b.ok)
            _check_fit(a, f, None, model, 5, "%dx%d x %d, %d" % (W, H, B, model))


def _frames(B, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    return rng.random((B, H, W, C)).astype(_NP[dtype])


def _matrices(B, H, W, seed):
    """small rotations, scales and shifts about the centre, one far outside the image, one with a NaN"""
    rng = np.random.default_rng(seed)
    M = np.empty((B, 2, 3))
    for i in range(B):
        th, s = rng.normal(0, 0.05), 1 + rng.normal(0, 0.05)
        a, b = s * math.cos(th), s * math.sin(th)
        cx, cy = (W - 1) / 2, (H - 1) / 2
        t = rng.normal(0, 3, 2)
        M[i] = [[a, -b, cx - a * cx + b * cy + t[0]], [b, a, cy - b * cx - a * cy + t[1]]]
    if B > 1:
        M[1, :, 2] += (2 * W, -H)
    if B > 2:
        M[2, 1, 1] = math.nan
    return M


def _same_bytes(got, want, layout, what):
    g = got.permute(0, 2, 3, 1) if layout == "NCHW" else got
    g = np.ascontiguousarray(g.cpu().numpy())
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = (g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,))).any(-1)
    assert not bad.any(), "%s: %d of %d elements differ; first at %s" % (what, int(bad.sum()), bad.size,
                                                                         tuple(int(k[0]) for k in np.nonzero(bad)))


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
def test_warp_every_dtype(dtype, layout):
    from papteam_opticalflow_amd.tensors import warp_affine
    B, H, W, C = 4, 37, 53, 3
    f = _frames(B, H, W, C, dtype, 8)
    M = _matrices(B, H, W, 9)
    t = torch.from_numpy(f).cuda()
    t = t.permute(0, 3, 1, 2) if layout == "NCHW" else t
    for mdt in (torch.float64, torch.float32):
        tm = torch.from_numpy(M).to(mdt).cuda()
        for odt in (None, torch.uint8, torch.float32, torch.float64):
            out, valid = warp_affine(t, tm, layout=layout, out_dtype=odt)
            want, wv = warp_reference(f, tm.cpu().numpy(), _NP[odt or dtype])
            _same_bytes(out, want, layout, "%s %s matrices %s out %s" % (dtype, layout, mdt, odt))
            assert np.array_equal(valid.cpu().numpy(), wv)
    assert not wv[1].any() and not wv[2].any() and wv[0].any()


def test_warp_strided_views_and_1080p():
    from papteam_opticalflow_amd.tensors import warp_affine
    B, H, W, C = 3, 29, 41, 3
    big = torch.from_numpy(_frames(2 * B, H + 3, 2 * W, C + 1, torch.uint8, 10)).cuda()
    a = big[::2, 2:H + 2, ::2, 1:]
    assert not a.is_contiguous()
    M = torch.from_numpy(np.repeat(_matrices(B, H, W, 11), 2, axis=0)).cuda()[::2]
    out, valid = warp_affine(a, M, layout="NHWC", out_dtype=torch.float32)
    want, wv = warp_reference(a.cpu().numpy(), M.cpu().numpy(), np.float32)
    _same_bytes(out, want, "NHWC", "strided")
    assert np.array_equal(valid.cpu().numpy(), wv)
    f = _frames(2, 1080, 1920, 3, torch.uint8, 12)
    M = _matrices(2, 1080, 1920, 13)
    out, valid = warp_affine(torch.from_numpy(f).cuda(), torch.from_numpy(M).cuda(), layout="NHWC")
    want, wv = warp_reference(f, M, np.uint8)
    _same_bytes(out, want, "NHWC", "1080p")
    assert np.array_equal(valid.cpu().numpy(), wv)


def test_the_calls_are_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and used under that stream with no synchronisation: the kernels
    must read them after they are written, and what is queued behind them must see their outputs"""
    import time
    from papteam_opticalflow_amd.tensors import global_motion, warp_affine
    B, H, W, C = 2, 40, 60, 3
    f = _frames(B, H, W, C, torch.uint8, 14)
    M = _matrices(B, H, W, 15)
    fl = _affine_flows(B, H, W, 16)
    want, _ = warp_reference(f, M, np.uint8)
    src = [torch.from_numpy(f).cuda(), torch.from_numpy(fl).cuda()]
    dst = [torch.zeros_like(s) for s in src]
    tm = torch.from_numpy(M).cuda()
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = (warp_affine(dst[0], tm, layout="NHWC")[0].clone(), global_motion(dst[1]).motion.clone())
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
        for d, s in zip(dst, src):
            d.copy_(s)
        got, _ = warp_affine(dst[0], tm, layout="NHWC")
        mo = global_motion(dst[1])
        took = time.perf_counter() - t0
        copy, mcopy = got.clone(), mo.motion.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    assert took < 0.25, "the calls waited for the stream: %.3f s" % took
    _same_bytes(got, want, "NHWC", "side stream")
    _same_bytes(copy, want, "NHWC", "side stream clone")
    ref = fit_reference(fl)[0]
    assert max(corner_distance(mcopy[i].cpu().numpy(), ref[i], H, W) for i in range(B)) < 1e-8


def _jittered(T=16, Hc=220, Wc=400, seed=17):
    """T crops of Hc x Wc from the committed 480x270 frame, crop t sampled (the bilinear rule, uint8 out) at the similarity
    K_t: a pan of 0.6 px per frame, jitter within +-2 px, rotation within +-0.4 degrees about the crop's centre"""
    import cases
    F = cases.load_frame_u8("480", 1)
    FH, FW, C = F.shape
    rng = np.random.default_rng(seed)
    c = np.array([(Wc - 1) / 2, (Hc - 1) / 2])
    I = as_f64(F)
    r, x = np.mgrid[0:Hc, 0:Wc].astype(np.float64)
    Ks, frames = [], []
    for t in range(T):
        th = math.radians(rng.uniform(-0.4, 0.4))
        o = np.array([40.0 + 0.6 * t, 25.0]) + rng.uniform(-2, 2, 2)
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        K = np.eye(3)
        K[:2, :2] = R
        K[:2, 2] = c + o - R @ c
        X, Y = K[0, 0] * x + K[0, 1] * r + K[0, 2], K[1, 0] * x + K[1, 1] * r + K[1, 2]
        assert X.min() >= 0 and X.max() <= FW - 1 and Y.min() >= 0 and Y.max() <= FH - 1  # every sample inside
        k = _taps(X[None], Y[None], FH, FW)
        out = np.stack([_sample(I[None, :, :, ch], np.zeros((1, 1, 1), np.int64), k)[0] for ch in range(C)], -1)
        frames.append(np.clip(np.rint(255 * out), 0, 255).astype(np.uint8))
        Ks.append(K)
    return np.stack(frames), np.stack(Ks)


def test_stabilize_video_end_to_end():
    """The fitted pair motions against the true K_{t+1}^-1 K_t at the corners, and the stabilized camera K_t M_t's
    translational second-difference RMS against K_t's.  Measured on an MI355X (4 levels): worst corner error 0.0656 px
    (similarity; mean 0.0361) and 0.0636 px (affine), jitter ratio 0.0121; bounds 0.25 px (3.8 x) and 0.25."""
    from papteam_opticalflow_amd.tensors import global_motion, stabilize_video, stabilizing_transforms, warp_affine
    frames, Ks = _jittered()
    T, Hc, Wc, _ = frames.shape
    v = torch.from_numpy(frames).cuda()
    sv = stabilize_video(v, 4, layout="NHWC", model="similarity")
    assert tuple(sv.video.shape) == (T, Hc, Wc, 3) and sv.video.dtype == torch.uint8 and bool(sv.ok.all())
    # the composite is its parts
    m = global_motion(sv.flow, model="similarity")
    assert torch.equal(m.motion, sv.motion)
    M = stabilizing_transforms(m, 15)
    assert torch.equal(M, sv.transforms)
    w, valid = warp_affine(v, M, layout="NHWC")
    assert torch.equal(w, sv.video) and torch.equal(valid, sv.valid)
    motion = sv.motion.cpu().numpy()
    errs = [corner_distance(motion[t], (np.linalg.inv(Ks[t + 1]) @ Ks[t])[:2], Hc, Wc) for t in range(T - 1)]
    h = lambda a: np.vstack([a, [0.0, 0.0, 1.0]])  # noqa: E731
    Mn = sv.transforms.cpu().numpy()
    cam = np.array([(Ks[t] @ h(Mn[t]))[:2, 2] for t in range(T)])
    d2 = lambda p: np.sqrt((np.diff(p, 2, axis=0) ** 2).sum(1).mean())  # noqa: E731
    ratio = d2(cam) / d2(Ks[:, :2, 2])
    print("stabilize_video end to end: worst corner error %.4f px (mean %.4f), jitter ratio %.4f" % (
        max(errs), float(np.mean(errs)), ratio))
    assert max(errs) < 0.25, errs
    assert ratio <= 0.25, ratio
    # the affine model on the same flows
    ma = global_motion(sv.flow, model="affine").motion.cpu().numpy()
    erra = max(corner_distance(ma[t], (np.linalg.inv(Ks[t + 1]) @ Ks[t])[:2], Hc, Wc) for t in range(T - 1))
    print("affine model: worst corner error %.4f px" % erra)
    assert erra < 0.25
