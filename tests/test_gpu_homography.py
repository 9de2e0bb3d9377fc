"""The homography model on device tensors (papteam_opticalflow_amd/tensors.py: global_homography, warp_homography,
mosaic_homography, mosaic_overlap_homography, panorama_homography -> papof_homography_fit_tensor,
papof_warp_projective_tensor, papof_mosaic_projective_tensor, papof_mosaic_overlap_projective_tensor).  The device's fit must
agree with the numpy fp64 restatement (tests/_homography_ref.py: fit_reference_h) within 1e-8 px at the image corners -- the
sums are added in another order, so not bit for bit -- and be bitwise the same from run to run; the warp, the mosaic and the
overlap statistics must be the BYTES of their restatements, and on matrices whose last row is (0, 0, 1) the bytes of the
affine calls; tile culling must change no byte on matrices that try it; panorama_homography must be its composition and
register a rotating camera that the affine model loses."""
import math

import numpy as np
import pytest

from _homography_ref import (chain, cull_matrices, fit_reference_h, homography_flow, homography_flows, mosaic_reference_h,
                             overlap_reference_h, projective_corner_distance, rotating_camera, rotating_scene, warp_reference_h)
from test_gpu_track import _fields

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}
MODES = ("first", "mean", "median", "feather")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _wild_flows(B, H, W, seed):
    """homography_flows with the NaNs, infinities and large displacements of test_gpu_track._fields"""
    f, _ = homography_flows(B, H, W, seed)
    wild, _ = _fields(B + 1, H, W, seed)
    with np.errstate(invalid="ignore"):
        keep = ~np.isfinite(wild) | (np.abs(wild) > 3)
    f[keep[:B]] = wild[:B][keep[:B]]
    return f


def _mask(B, H, W, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((B, 2, H, W)) < 0.1).astype(np.uint8)
    m[:, 0, H // 4:H // 2, W // 3:W // 2] = 1
    return m


def _check_fit(got, flow, occ, iters, what, scale=1.0):
    """the device's Homography against fit_reference_h: corners within 1e-8 px, ok equal, support within 1e-12"""
    motion, ok, sup = fit_reference_h(flow, occ, iters, scale)
    H, W = flow.shape[2:]
    gm, gok, gs = got.motion.cpu().numpy(), got.ok.cpu().numpy(), got.support.cpu().numpy()
    assert (gok == ok).all(), (what, gok, ok)
    assert (gm[:, 2, 2] == 1.0).all(), what
    d = max(projective_corner_distance(gm[i], motion[i], H, W) for i in range(len(ok)))
    print("%s: %.3g px from the restatement at the corners, support within %.3g" % (what, d, np.abs(gs - sup).max()))
    assert d < 1e-8, (what, d)
    assert np.abs(gs - sup).max() < 1e-12, what


def test_fit_matches_the_restatement():
    from papteam_opticalflow_amd.tensors import global_homography
    B, H, W = 3, 70, 93
    f = _wild_flows(B, H, W, 1)
    occ = _mask(B, H, W, 2)
    for fdt in (torch.float64, torch.float32):
        tf = torch.from_numpy(f).to(fdt).cuda()
        nf = tf.cpu().numpy()
        for m in (None, occ):
            tm = torch.from_numpy(m).cuda().bool() if m is not None else None
            for iters in (1, 5):
                got = global_homography(tf, occlusion=tm, iters=iters, scale=1.5)
                _check_fit(got, nf, m, iters, "%s mask %s iters %d" % (fdt, m is not None, iters), 1.5)


def test_fit_strided_views_and_failed_pairs():
    from papteam_opticalflow_amd.tensors import global_homography
    B, H, W = 4, 50, 67
    f = _wild_flows(B, H, W, 3)
    f[2] = math.nan                                   # no valid pixel: the identity, not ok
    f[3, :, :, :] = math.nan
    f[3, :, :, 10] = 0.0                              # one valid column: iteration 0 fails at a pivot
    big = torch.from_numpy(np.ascontiguousarray(f.transpose(0, 2, 3, 1))).cuda()  # (B, H, W, 2) read as (B, 2, H, W)
    tf = big.permute(0, 3, 1, 2)
    wide = torch.from_numpy(np.repeat(_mask(B, H, W, 4), 2, axis=3)).cuda()[:, :, :, ::2]
    assert not tf.is_contiguous() and not wide.is_contiguous()
    before = big.clone()
    got = global_homography(tf, occlusion=wide)
    _check_fit(got, f, wide.cpu().numpy(), 5, "strided")
    assert got.ok.cpu().tolist() == [True, True, False, False]
    assert torch.equal(got.motion[2].cpu(), torch.eye(3, dtype=torch.float64))
    assert torch.equal(got.motion[3].cpu(), torch.eye(3, dtype=torch.float64))
    assert torch.equal(big.view(torch.int64), before.view(torch.int64))  # inputs unchanged


def test_fit_is_reproducible_over_many_blocks_and_many_pairs():
    """270 x 480: 72 blocks, more than the 64 lanes of the solve's row loop; 100 pairs of 37 x 53, smaller than a tile"""
    from papteam_opticalflow_amd.tensors import global_homography
    for B, H, W, seed in ((1, 270, 480, 6), (100, 37, 53, 7)):
        f = _wild_flows(B, H, W, seed)
        tf = torch.from_numpy(f).cuda()
        a = global_homography(tf)
        b = global_homography(tf)
        torch.cuda.synchronize()
        assert a.motion.cpu().numpy().tobytes() == b.motion.cpu().numpy().tobytes()
        assert torch.equal(a.support, b.support) and torch.equal(a.ok, b.ok)
        _check_fit(a, f, None, 5, "%dx%d x %d" % (W, H, B))


# ---- the warp
def _frames(B, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    return rng.random((B, H, W, C)).astype(_NP[dtype])


def _affine(B, H, W, seed):
    """small rotations, scales and shifts about the centre, (B, 2, 3)"""
    rng = np.random.default_rng(seed)
    M = np.empty((B, 2, 3))
    for i in range(B):
        th, s = rng.normal(0, 0.05), 1 + rng.normal(0, 0.05)
        a, b = s * math.cos(th), s * math.sin(th)
        cx, cy = (W - 1) / 2, (H - 1) / 2
        t = rng.normal(0, 3, 2)
        M[i] = [[a, -b, cx - a * cx + b * cy + t[0]], [b, a, cy - b * cx - a * cy + t[1]]]
    return M


def _embedded(M2):
    M3 = np.zeros(M2.shape[:-2] + (3, 3), M2.dtype)
    M3[..., :2, :] = M2
    M3[..., 2, 2] = 1.0
    return M3


def _homographies(B, H, W, seed):
    """_affine with last rows: mild perspective, a horizon that crosses the frame (1), a NaN entry (2), far outside (3)"""
    M = _embedded(_affine(B, H, W, seed))
    M[:, 2, :2] = np.random.default_rng(seed + 100).normal(0, 1e-3, (B, 2))
    if B > 1:
        M[1, 2] = (-1.0 / (0.6 * W), 0.0, 1.0)
    if B > 2:
        M[2, 2, 1] = math.nan
    if B > 3:
        M[3, :2, 2] += (2 * W, -H)
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
    from papteam_opticalflow_amd.tensors import warp_affine, warp_homography
    B, H, W, C = 5, 45, 70, 3
    f = _frames(B, H, W, C, dtype, 8)
    M = _homographies(B, H, W, 9)
    t = torch.from_numpy(f).cuda()
    t = t.permute(0, 3, 1, 2) if layout == "NCHW" else t
    for mdt in (torch.float64, torch.float32):
        tm = torch.from_numpy(M).to(mdt).cuda()
        for odt in (None, torch.uint8, torch.float32, torch.float64):
            out, valid = warp_homography(t, tm, layout=layout, out_dtype=odt)
            want, wv = warp_reference_h(f, tm.cpu().numpy(), _NP[odt or dtype])
            _same_bytes(out, want, layout, "%s %s matrices %s out %s" % (dtype, layout, mdt, odt))
            assert np.array_equal(valid.cpu().numpy(), wv)
        ta = torch.from_numpy(_affine(B, H, W, 10)).to(mdt).cuda()
        a, av = warp_affine(t, ta, layout=layout)
        h, hv = warp_homography(t, torch.from_numpy(_embedded(ta.cpu().numpy())).cuda(), layout=layout)
        assert torch.equal(a, h) and torch.equal(av, hv) and bool(av.any())
    assert wv[0].any() and wv[1].any() and not wv[1].all() and not wv[2].any() and not wv[3].any()


def test_warp_strided_views():
    from papteam_opticalflow_amd.tensors import warp_homography
    B, H, W, C = 3, 45, 70, 3
    big = torch.from_numpy(_frames(2 * B, H + 3, 2 * W, C + 1, torch.uint8, 10)).cuda()
    a = big[::2, 2:H + 2, ::2, 1:]
    assert not a.is_contiguous()
    before = big.clone()
    M = torch.from_numpy(np.repeat(_homographies(B, H, W, 11), 2, axis=0)).cuda()[::2]
    out, valid = warp_homography(a, M, layout="NHWC", out_dtype=torch.float32)
    want, wv = warp_reference_h(a.cpu().numpy(), M.cpu().numpy(), np.float32)
    _same_bytes(out, want, "NHWC", "strided")
    assert np.array_equal(valid.cpu().numpy(), wv) and torch.equal(big, before)


# ---- the mosaic
H_, W_, HC, WC = 40, 56, 77, 150


def _placed(rng, n_out, N):
    """(n_out, N, 3, 3): frames placed over the canvas with small rotations and mild perspective; slot 1 NaN, slot 2 behind
    its horizon everywhere"""
    M = np.empty((n_out, N, 3, 3))
    for o in range(n_out):
        for k in range(N):
            th, s = rng.normal(0, 0.1), 1 + rng.normal(0, 0.05)
            a, b = s * math.cos(th), s * math.sin(th)
            M[o, k] = [[a, -b, -rng.uniform(-10, WC - W_ + 10)], [b, a, -rng.uniform(-10, HC - H_ + 10)],
                       [rng.normal(0, 5e-4), rng.normal(0, 5e-4), 1.0]]
    M[0, 1, 0, 1] = math.nan
    M[0, 2] = -M[0, 2]
    return M


def _sources(rng, n_out, N, T):
    s = rng.integers(0, T, (n_out, N))
    s[rng.random((n_out, N)) < 0.15] = -1
    return s


@pytest.mark.parametrize("N", [3, 9, 17, 33])
def test_mosaic_is_the_restatements_bytes(N):
    """every median instance (8, 16, 32, 64 samples per lane), the four modes, with and without masks, gains and count,
    empty slots; the second run of each call gives the same bytes"""
    from papteam_opticalflow_amd import tensors
    from papteam_opticalflow_amd.tensors import mosaic_homography
    T = 5
    rng = np.random.default_rng(20 + N)
    f = _frames(T, H_, W_, 3, torch.uint8, 21)
    t = torch.from_numpy(f).cuda()
    M = _placed(rng, 2, N)
    src = _sources(rng, 2, N, T)
    mk = rng.random((T, H_, W_)) < 0.1
    g = rng.uniform(0.7, 1.2, (2, N))
    tm, tmk, tg = torch.from_numpy(M).cuda(), torch.from_numpy(mk).cuda(), torch.from_numpy(g).cuda()
    before = (t.clone(), tm.clone())
    for mode in MODES:
        for masks, gains in ((None, None), (mk, g)):
            kw = dict(mode=mode, masks=None if masks is None else tmk, gains=None if gains is None else tg, layout="NHWC")
            got = mosaic_homography(t, src, tm, (HC, WC), out_dtype=torch.float32, **kw)
            again = mosaic_homography(t, src, tm, (HC, WC), out_dtype=torch.float32, **kw)
            want, wcnt = mosaic_reference_h(f, src, M, (HC, WC), mode, gains, masks, np.float32)
            what = "N %d %s masks %s gains %s" % (N, mode, masks is not None, gains is not None)
            _same_bytes(got.out, want, "NHWC", what)
            assert np.array_equal(got.count.cpu().numpy(), wcnt), what
            assert torch.equal(got.out.view(torch.int32), again.out.view(torch.int32)) and torch.equal(got.count, again.count)
            assert int(wcnt.max()) >= 2 and int(wcnt.min()) == 0
            # without the count (mode "first" then stops at the first live source): the same image
            ts, descs, _, _ = tensors._check([("frames", t)], "NHWC", None, 1)
            out, none = tensors._mosaic(ts, descs, torch.from_numpy(src).to(torch.int32).cuda(), tm, tensors.capi.DTYPE_F64,
                                        None if masks is None else tmk.view(torch.uint8), HC, WC, mode, "NHWC", torch.float32,
                                        count=False, gains=kw["gains"], rule=tensors._PROJECTIVE)
            assert none is None
            _same_bytes(out, want, "NHWC", what + " no count")
    assert torch.equal(t, before[0]) and torch.equal(tm.view(torch.int64), before[1].view(torch.int64))


def test_mosaic_dtypes_layouts_and_float32_matrices():
    from papteam_opticalflow_amd.tensors import mosaic_homography
    T, N = 4, 4
    rng = np.random.default_rng(30)
    M = _placed(rng, 1, N).astype(np.float32)
    for dtype in (torch.float32, torch.float64):
        f = _frames(T, H_, W_, 2, dtype, 31)
        t = torch.from_numpy(f).cuda().permute(0, 3, 1, 2)
        for mode in ("median", "feather"):
            got = mosaic_homography(t, None, torch.from_numpy(M).cuda(), (HC, WC), mode=mode, out_dtype=torch.uint8)
            want, wcnt = mosaic_reference_h(f, None, M, (HC, WC), mode, out_dtype=np.uint8)
            _same_bytes(got.out, want, "NCHW", "%s %s" % (dtype, mode))
            assert np.array_equal(got.count.cpu().numpy(), wcnt)


def test_affine_embedded_matrices_give_the_affine_calls_bytes():
    from papteam_opticalflow_amd.tensors import mosaic, mosaic_homography, mosaic_overlap, mosaic_overlap_homography
    T, N = 5, 9
    rng = np.random.default_rng(40)
    t = torch.from_numpy(_frames(T, H_, W_, 3, torch.uint8, 41)).cuda()
    M3 = _placed(rng, 2, N)
    M3[..., 2, :] = (0.0, 0.0, 1.0)
    src = _sources(rng, 2, N, T)
    mk = torch.from_numpy(rng.random((T, H_, W_)) < 0.1).cuda()
    g = torch.from_numpy(rng.uniform(0.7, 1.2, (2, N))).cuda()
    for mdt in (torch.float64, torch.float32):
        m3 = torch.from_numpy(M3).to(mdt).cuda()
        m2 = m3[:, :, :2].contiguous()
        for mode in MODES:
            for gains in (None, g):
                a = mosaic(t, src, m2, (HC, WC), mode=mode, masks=mk, gains=gains, layout="NHWC")
                h = mosaic_homography(t, src, m3, (HC, WC), mode=mode, masks=mk, gains=gains, layout="NHWC")
                assert torch.equal(a.out, h.out) and torch.equal(a.count, h.count), (mode, gains is not None)
                assert int(a.count.max()) >= 2
        for step in (1, 2):
            a = mosaic_overlap(t, src, m2, (HC, WC), masks=mk, step=step, layout="NHWC")
            h = mosaic_overlap_homography(t, src, m3, (HC, WC), masks=mk, step=step, layout="NHWC")
            assert torch.equal(a.sums, h.sums) and torch.equal(a.counts, h.counts) and int(a.counts.sum()) > 0


def test_culling_changes_no_byte(monkeypatch):
    """PAPOF_MOSAIC_CULL=0 walks every source in every tile: the same bytes as with the tile culling on the matrices of the
    CPU culling test -- horizons that cross tiles, D <= 0 everywhere, tiny D, NaN and infinite entries, float32"""
    from papteam_opticalflow_amd.tensors import mosaic_homography, mosaic_overlap_homography
    T = 4
    f = _frames(T, H_, W_, 3, torch.float32, 50)
    t = torch.from_numpy(f).cuda()
    all_M = cull_matrices(H_, W_, HC, WC)
    n_out = -(-len(all_M) // 64)
    M = np.tile(np.eye(3), (n_out, 64, 1, 1))
    M.reshape(-1, 3, 3)[:len(all_M)] = all_M
    src = np.random.default_rng(51).integers(0, T, (n_out, 64))
    for mdt in (torch.float64, torch.float32):
        tm = torch.from_numpy(M).to(mdt).cuda()
        for mode in MODES:
            monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
            on = mosaic_homography(t, src, tm, (HC, WC), mode=mode, layout="NHWC")
            monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
            off = mosaic_homography(t, src, tm, (HC, WC), mode=mode, layout="NHWC")
            assert torch.equal(on.out.view(torch.int32), off.out.view(torch.int32)) and torch.equal(on.count, off.count), mode
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        on = mosaic_overlap_homography(t, src, tm, (HC, WC), step=1, layout="NHWC")
        monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
        off2 = mosaic_overlap_homography(t, src, tm, (HC, WC), step=1, layout="NHWC")
        assert torch.equal(on.sums, off2.sums) and torch.equal(on.counts, off2.counts)
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        want, wcnt = mosaic_reference_h(f, src, tm.cpu().numpy(), (HC, WC), "feather", out_dtype=np.float32)
        _same_bytes(off.out, want, "NHWC", "culling off %s" % mdt)
        assert np.array_equal(off.count.cpu().numpy(), wcnt) and int(wcnt.max()) >= 2


@pytest.mark.parametrize("N", [5, 33])
def test_overlap_is_the_restatements_integers(N):
    from papteam_opticalflow_amd.tensors import mosaic_overlap_homography
    T = 5
    rng = np.random.default_rng(60 + N)
    f = _frames(T, H_, W_, 3, torch.uint8, 61)
    t = torch.from_numpy(f).cuda()
    M = _placed(rng, 2, N)
    src = _sources(rng, 2, N, T)
    mk = rng.random((T, H_, W_)) < 0.1
    for step in (1, 2):
        for masks in (None, mk):
            got = mosaic_overlap_homography(t, src, torch.from_numpy(M).cuda(), (HC, WC), step=step, layout="NHWC",
                                            masks=None if masks is None else torch.from_numpy(masks).cuda())
            sums, counts = overlap_reference_h(f, src, M, (HC, WC), step, 1.0, masks)
            assert np.array_equal(got.sums.cpu().numpy(), sums) and np.array_equal(got.counts.cpu().numpy(), counts)
            assert counts.sum() > 0


# ---- the chain
def test_panorama_homography_is_its_composition():
    from papteam_opticalflow_amd.tensors import (exposure_gains, global_homography, homography_transforms, mosaic_homography,
                                                 mosaic_overlap_homography, panorama_homography)
    frames, _, _, _ = rotating_scene(T=5, H=64, W=96, focal=150.0, yaw_deg=3.0)
    v = torch.from_numpy(frames).cuda()
    for exposure, mode in ((False, "median"), (True, "feather")):
        p = panorama_homography(v, 3, mode=mode, layout="NHWC", exposure=exposure)
        m = global_homography(p.flow)
        assert torch.equal(m.motion, p.motion) and torch.equal(m.ok, p.ok) and tuple(p.motion.shape) == (4, 3, 3)
        M, size, origin = homography_transforms(m, (64, 96))
        assert torch.equal(M[0], p.matrices) and origin == p.origin and tuple(p.image.shape) == size + (3,)
        gains = None
        if exposure:
            gains = exposure_gains(mosaic_overlap_homography(v, None, M, size, step=2, layout="NHWC"), anchor=2)
            assert torch.equal(gains[0], p.gains)
        mo = mosaic_homography(v, None, M, size, mode=mode, layout="NHWC", gains=gains)
        assert torch.equal(mo.out[0], p.image) and torch.equal(mo.count[0], p.count) and int(p.count.max()) >= 2


def test_rotating_camera_chain_on_the_device():
    """exact flows of the rotating camera (focal length 200 px, 4 degrees per frame, nine 96 x 160 frames) uploaded as
    tensors: global_homography's chain stays on the exact one, the affine model's drifts by tens of pixels"""
    from papteam_opticalflow_amd.tensors import global_homography, global_motion
    H, W = 96, 160
    A = rotating_camera(9, H, W)
    tf = torch.from_numpy(np.stack([homography_flow(a, H, W) for a in A])).cuda()
    h = global_homography(tf)
    a = global_motion(tf, model="affine")
    assert bool(h.ok.all()) and bool(a.ok.all())
    eh = projective_corner_distance(chain(h.motion.cpu().numpy()), chain(A), H, W)
    ea = projective_corner_distance(chain(a.motion.cpu().numpy()), chain(A), H, W)
    print("rotating camera on the device, 8 pairs: homography chain %.3g px, affine chain %.3g px" % (eh, ea))
    assert eh < 1e-6 and ea > 50


def test_the_calls_are_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and used under that stream with no synchronisation: the kernels
    must read them after they are written, and what is queued behind them must see their outputs"""
    import time
    from papteam_opticalflow_amd.tensors import (global_homography, mosaic_homography, mosaic_overlap_homography,
                                                 warp_homography)
    B, H, W, C = 3, 40, 56, 3
    f = _frames(B, H, W, C, torch.uint8, 70)
    M = _homographies(B, H, W, 71)
    P = _placed(np.random.default_rng(72), 1, B)
    fl, _ = homography_flows(B, H, W, 73)
    want, _ = warp_reference_h(f, M, np.uint8)
    wmos, _ = mosaic_reference_h(f, None, P, (HC, WC), "mean", out_dtype=np.uint8)
    wsum, wcnt = overlap_reference_h(f, None, P, (HC, WC), 2)
    src = [torch.from_numpy(f).cuda(), torch.from_numpy(fl).cuda()]
    dst = [torch.zeros_like(s) for s in src]
    tm, tp = torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda()
    side = torch.cuda.Stream(priority=-1)

    def calls():
        return (warp_homography(dst[0], tm, layout="NHWC")[0], global_homography(dst[1]).motion,
                mosaic_homography(dst[0], None, tp, (HC, WC), mode="mean", layout="NHWC").out,
                mosaic_overlap_homography(dst[0], None, tp, (HC, WC), layout="NHWC"))

    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = calls()
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
        got, mo, mos, ov = calls()
        took = time.perf_counter() - t0
        copies = (got.clone(), mo.clone(), mos.clone(), ov.sums.clone(), ov.counts.clone())  # queued behind the kernels
    side.synchronize()
    assert took < 0.25, "the calls waited for the stream: %.3f s" % took
    _same_bytes(got, want, "NHWC", "side stream")
    _same_bytes(copies[0], want, "NHWC", "side stream clone")
    ref = fit_reference_h(fl)[0]
    assert max(projective_corner_distance(copies[1][i].cpu().numpy(), ref[i], H, W) for i in range(B)) < 1e-8
    _same_bytes(copies[2], wmos, "NHWC", "side stream mosaic")
    assert np.array_equal(copies[3].cpu().numpy(), wsum) and np.array_equal(copies[4].cpu().numpy(), wcnt)
