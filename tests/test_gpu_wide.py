"""Wide panoramas on device tensors (papteam_opticalflow_amd/tensors.py: mosaic_rays, mosaic_overlap_rays, panorama_wide ->
papof_mosaic_ray_tensor, papof_mosaic_overlap_ray_tensor).  The mosaic and the overlap statistics must be the BYTES of the
numpy restatement (tests/_wide_ref.py) on cylinder and sphere canvases of the pan that the planar call refuses, in every
instance; on the plane's tables the bytes of the projective calls; tile culling must change no byte on tables and matrices
that try it; panorama_wide must be its composition, find the focal length and register a 160 degree pan."""
import numpy as np
import pytest

from _homography_ref import cull_matrices
from _mosaic_ref import psnr
from _wide_ref import (MODES, cull_tables_and_matrices, cylinder_truth, mosaic_reference_rays, overlap_reference_rays,
                       plane_tables, small_pan, wide_scene)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}
H_, W_, T_ = 20, 30, 9  # nine 20 x 30 frames, focal length 40, 20 degrees per frame: a 141 x 21 canvas, three tiles wide


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


@pytest.fixture(scope="module")
def canvases():
    """{surface: (matrices (9, 3, 3), cols, rows)} of the small pan, made once"""
    return {s: small_pan(s)[:3] for s in ("cylinder", "sphere")}


def _frames(T, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return rng.integers(0, 256, (T, H, W, C)).astype(np.uint8)
    return rng.random((T, H, W, C)).astype(_NP[dtype])


def _slots(rng, M, n_out, N, poses=None):
    """N slots per output that repeat the pan's nine frames (slot k is frame k mod 9, under its matrix -- or that of frame
    poses[k] -- nudged by a small rotation of its own so that repeated slots differ), about one in seven empty:
    (sources (n_out, N), matrices (n_out, N, 3, 3))"""
    src = np.tile(np.arange(N) % T_, (n_out, 1))
    mats = M[src if poses is None else np.tile(poses, (n_out, 1))].copy()
    for o in range(n_out):
        for k in range(N):
            a = rng.normal(0, 0.02)
            mats[o, k] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ mats[o, k]
    src[rng.random((n_out, N)) < 0.15] = -1
    return src, mats


def _same_bytes(got, want, layout, what):
    g = got.permute(0, 2, 3, 1) if layout == "NCHW" else got
    g = np.ascontiguousarray(g.cpu().numpy())
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = (g.view(np.uint8).reshape(g.shape + (-1,)) != w.view(np.uint8).reshape(w.shape + (-1,))).any(-1)
    assert not bad.any(), "%s: %d of %d elements differ; first at %s" % (what, int(bad.sum()), bad.size,
                                                                         tuple(int(k[0]) for k in np.nonzero(bad)))


@pytest.mark.parametrize("N", [7, 9, 20, 40])
@pytest.mark.parametrize("surface", ["cylinder", "sphere"])
def test_mosaic_is_the_restatements_bytes(canvases, surface, N):
    """every median instance (8, 16, 32, 64 samples per lane; tiles of 64 x 4, 64 x 4, 64 x 2, 64 x 1), the four modes, with
    and without masks and gains, empty slots, frames behind the reference"""
    from papteam_opticalflow_amd.tensors import mosaic_rays
    M, cols, rows = canvases[surface]
    rng = np.random.default_rng(100 + N)
    f = _frames(T_, H_, W_, 3, torch.uint8, 21)
    src, mats = _slots(rng, M, 2, N)
    mk = rng.random((T_, H_, W_)) < 0.1
    g = rng.uniform(0.7, 1.2, (2, N))
    t, tm, tc, tr = (torch.from_numpy(a).cuda() for a in (f, mats, cols, rows))
    tmk, tg = torch.from_numpy(mk).cuda(), torch.from_numpy(g).cuda()
    before = (t.clone(), tm.clone(), tc.clone(), tr.clone())
    for mode in MODES:
        for masks, gains in ((None, None), (mk, g)):
            got = mosaic_rays(t, src, tm, tc, tr, mode=mode, masks=None if masks is None else tmk,
                              gains=None if gains is None else tg, layout="NHWC", out_dtype=torch.float32)
            want, wcnt = mosaic_reference_rays(f, src, mats, cols, rows, mode, gains, masks, np.float32)
            what = "%s N %d %s masks %s gains %s" % (surface, N, mode, masks is not None, gains is not None)
            _same_bytes(got.out, want, "NHWC", what)
            assert np.array_equal(got.count.cpu().numpy(), wcnt), what
            assert int(wcnt.max()) >= 2 and int(wcnt.min()) == 0
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip((t, tm, tc, tr), before))  # inputs unchanged


@pytest.mark.parametrize("surface", ["cylinder", "sphere"])
def test_mosaic_dtypes_layouts_float32_matrices_and_tables(canvases, surface):
    """float32 and float64 frames in NCHW, float32 matrices and tables (widened exactly), uint8 output, strided tables"""
    from papteam_opticalflow_amd.tensors import mosaic_rays
    M, cols, rows = canvases[surface]
    M32, c32, r32 = M.astype(np.float32)[None], cols.astype(np.float32), rows.astype(np.float32)
    wide = torch.from_numpy(np.repeat(c32, 2, axis=0)).cuda()[::2]  # a view with a row stride of 4
    assert not wide.is_contiguous()
    for dtype in (torch.float32, torch.float64):
        f = _frames(T_, H_, W_, 2, dtype, 31)
        t = torch.from_numpy(f).cuda().permute(0, 3, 1, 2)
        for mode in MODES:
            got = mosaic_rays(t, None, torch.from_numpy(M32).cuda(), wide, torch.from_numpy(r32).cuda(), mode=mode,
                              out_dtype=torch.uint8)
            want, wcnt = mosaic_reference_rays(f, None, M32, c32, r32, mode, out_dtype=np.uint8)
            _same_bytes(got.out, want, "NCHW", "%s %s %s" % (surface, dtype, mode))
            assert np.array_equal(got.count.cpu().numpy(), wcnt) and int(wcnt.max()) >= 2
        got = mosaic_rays(t, None, torch.from_numpy(M32).double().cuda(), wide, torch.from_numpy(rows).cuda(), mode="mean")
        want, wcnt = mosaic_reference_rays(f, None, M32.astype(np.float64), c32, rows, "mean", out_dtype=_NP[dtype])
        _same_bytes(got.out, want, "NCHW", "%s %s mixed" % (surface, dtype))


def test_255_sources(canvases):
    """the most slots the kernel takes, in the modes that take them.  Spread over the pan, 255 slots put about 50 on a pixel
    (each pixel lies in two of the nine frames, one slot in seven is empty); so only the first 90 slots follow the pan and
    the other 165 share the poses of frames 3, 4 and 5, which puts more than the median's 64 on the canvas's middle"""
    from papteam_opticalflow_amd.tensors import mosaic_rays
    M, cols, rows = canvases["cylinder"]
    rng = np.random.default_rng(40)
    f = _frames(T_, H_, W_, 3, torch.uint8, 41)
    k = np.arange(255)
    src, mats = _slots(rng, M, 1, 255, np.where(k < 90, k % T_, 3 + k % 3))
    t, tm, tc, tr = (torch.from_numpy(a).cuda() for a in (f, mats, cols, rows))
    for mode in ("mean", "first", "feather"):
        got = mosaic_rays(t, src, tm, tc, tr, mode=mode, layout="NHWC", out_dtype=torch.float64)
        want, wcnt = mosaic_reference_rays(f, src, mats, cols, rows, mode)
        _same_bytes(got.out, want, "NHWC", "255 sources, %s" % mode)
        assert np.array_equal(got.count.cpu().numpy(), wcnt) and int(wcnt.max()) > 64


@pytest.mark.parametrize("N", [5, 9, 20, 40])
def test_overlap_is_the_restatements_integers(canvases, N):
    """every overlap instance (8, 16, 32, 64 slots), steps 1 and 2, masks; the second run adds the same integers"""
    from papteam_opticalflow_amd.tensors import mosaic_overlap_rays
    rng = np.random.default_rng(60 + N)
    f = _frames(T_, H_, W_, 3, torch.uint8, 61)
    t = torch.from_numpy(f).cuda()
    mk = rng.random((T_, H_, W_)) < 0.1
    for surface in ("cylinder", "sphere"):
        M, cols, rows = canvases[surface]
        src, mats = _slots(rng, M, 2, N)
        tm, tc, tr = (torch.from_numpy(a).cuda() for a in (mats, cols, rows))
        for step in (1, 2):
            for masks in (None, mk):
                kw = dict(step=step, layout="NHWC", masks=None if masks is None else torch.from_numpy(masks).cuda())
                got = mosaic_overlap_rays(t, src, tm, tc, tr, **kw)
                again = mosaic_overlap_rays(t, src, tm, tc, tr, **kw)
                sums, counts = overlap_reference_rays(f, src, mats, cols, rows, step, 1.0, masks)
                assert np.array_equal(got.sums.cpu().numpy(), sums) and np.array_equal(got.counts.cpu().numpy(), counts)
                assert torch.equal(got.sums, again.sums) and torch.equal(got.counts, again.counts)
                assert counts.sum() > 0 and (counts * (1 - np.eye(N, dtype=np.int64))).sum() > 0


def test_plane_tables_give_the_projective_calls_bytes():
    """cols = (x, 1), rows = (y, 1): the bytes, the count, the sums and the counts of mosaic_homography and
    mosaic_overlap_homography on the matrices of the projective culling test"""
    from papteam_opticalflow_amd.tensors import mosaic_homography, mosaic_overlap_homography, mosaic_overlap_rays, mosaic_rays
    H, W, Hc, Wc, T = 40, 56, 77, 150, 4
    t = torch.from_numpy(_frames(T, H, W, 3, torch.uint8, 50)).cuda()
    all_M = cull_matrices(H, W, Hc, Wc)
    n_out = -(-len(all_M) // 64)
    M = np.tile(np.eye(3), (n_out, 64, 1, 1))
    M.reshape(-1, 3, 3)[:len(all_M)] = all_M
    rng = np.random.default_rng(51)
    src = rng.integers(0, T, (n_out, 64))
    mk = torch.from_numpy(rng.random((T, H, W)) < 0.1).cuda()
    g = torch.from_numpy(rng.uniform(0.7, 1.2, (n_out, 64))).cuda()
    for dt in (torch.float64, torch.float32):
        tm = torch.from_numpy(M).to(dt).cuda()
        tc, tr = (torch.from_numpy(a).cuda() for a in plane_tables(Hc, Wc, _NP[dt]))
        for mode in MODES:
            for gains in (None, g):
                a = mosaic_homography(t, src, tm, (Hc, Wc), mode=mode, masks=mk, gains=gains, layout="NHWC")
                b = mosaic_rays(t, src, tm, tc, tr, mode=mode, masks=mk, gains=gains, layout="NHWC")
                assert torch.equal(a.out, b.out) and torch.equal(a.count, b.count), (dt, mode, gains is not None)
                assert int(a.count.max()) >= 2
        for step in (1, 2):
            a = mosaic_overlap_homography(t, src, tm, (Hc, Wc), masks=mk, step=step, layout="NHWC")
            b = mosaic_overlap_rays(t, src, tm, tc, tr, masks=mk, step=step, layout="NHWC")
            assert torch.equal(a.sums, b.sums) and torch.equal(a.counts, b.counts) and int(a.counts.sum()) > 0


def test_culling_changes_no_byte(monkeypatch):
    """PAPOF_MOSAIC_CULL=0 walks every source in every tile: the same bytes as with the tile culling, for both calls, on the
    tables and matrices of the CPU culling test -- frames behind the reference, NaN and infinite matrix and table entries,
    tiny and huge D, float32"""
    from papteam_opticalflow_amd.tensors import mosaic_overlap_rays, mosaic_rays
    T = 4
    f = _frames(T, H_, W_, 3, torch.float32, 70)
    t = torch.from_numpy(f).cuda()
    rng = np.random.default_rng(71)
    live = 0
    for what, cols, rows, all_M in cull_tables_and_matrices():
        n_out = -(-len(all_M) // 64)
        N = min(len(all_M), 64)
        M = np.tile(np.eye(3), (n_out, N, 1, 1)).astype(all_M.dtype)
        M.reshape(-1, 3, 3)[:len(all_M)] = all_M
        src = rng.integers(0, T, (n_out, N))
        tm, tc, tr = (torch.from_numpy(a).cuda() for a in (M, cols, rows))
        for mode in MODES:
            monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
            on = mosaic_rays(t, src, tm, tc, tr, mode=mode, layout="NHWC")
            monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
            off = mosaic_rays(t, src, tm, tc, tr, mode=mode, layout="NHWC")
            assert torch.equal(on.out.view(torch.int32), off.out.view(torch.int32)) and torch.equal(on.count, off.count), (what, mode)
        for step in (1, 2):
            monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
            on2 = mosaic_overlap_rays(t, src, tm, tc, tr, step=step, layout="NHWC")
            monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
            off2 = mosaic_overlap_rays(t, src, tm, tc, tr, step=step, layout="NHWC")
            assert torch.equal(on2.sums, off2.sums) and torch.equal(on2.counts, off2.counts), (what, step)
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        live += int(on.count.max())
        if what in ("cylinder float32", "sphere wild matrices", "cylinder table entry nan"):  # and they are the rule's bytes
            want, wcnt = mosaic_reference_rays(f, src, M, cols, rows, "feather", out_dtype=np.float32)
            _same_bytes(off.out, want, "NHWC", "culling off, " + what)
            assert np.array_equal(off.count.cpu().numpy(), wcnt)
    assert live > 0


# ---- the chain
# levels: (|focal / 240 - 1|, the median panorama's PSNR against the texture in dB) of panorama_wide on the wide scene with
# estimated flows (README; the figures are the fp64 CPU oracle's flows through the numpy restatements, which the device's
# flows match to 1e-9 px).  The scene moves by 17 to 19 px per frame on frames 160 px wide: 4 pyramid levels (the
# coarsest 67 px wide) do not follow that -- the flows come out at 7 px, the homographies 16 px off at the corners, the focal
# length at 39 px -- and 8 levels do (0.7 px at the corners per pair).  Against the texture even that chain scores little:
# the focal length is 5 % long, so the 160 degrees of the pan come out as 152 and the ends of the panorama lie 17 px from
# the texture's; there is no bundle adjustment and nothing ties the chain to the truth.
WIDE = {4: (0.83813, 10.63), 8: (0.05082, 12.28)}


@pytest.fixture(scope="module")
def wide():
    frames, _, _, world = wide_scene()
    return torch.from_numpy(frames).cuda(), world


@pytest.mark.parametrize("levels,exposure,mode,step", [(4, False, "median", 1), (4, True, "feather", 2), (8, False, "median", 1)])
def test_panorama_wide_is_its_composition_on_the_wide_scene(wide, levels, exposure, mode, step):
    """the wide scene (41 frames of 96 x 160, 160 degrees of pan) with estimated flows: panorama_wide returns the bytes of the
    public calls chained by hand, with and without exposure compensation; its focal length is held to twice the measured
    error and its median panorama to the measured PSNR against the texture less 0.5 dB (WIDE above has the figures and what
    they say)"""
    from papteam_opticalflow_amd.tensors import (estimate_focal, exposure_gains, global_homography, mosaic_overlap_rays,
                                                 mosaic_rays, panorama_wide, wide_transforms)
    v, world = wide
    p = panorama_wide(v, levels, mode=mode, step=step, layout="NHWC", exposure=exposure)
    m = global_homography(p.flow)
    assert torch.equal(m.motion, p.motion) and torch.equal(m.ok, p.ok) and tuple(p.motion.shape) == (40, 3, 3)
    focal = estimate_focal(m, (96, 160))
    assert focal == p.focal
    M, cols, rows, size, origin = wide_transforms(m, (96, 160), focal)
    assert torch.equal(M[0], p.matrices) and torch.equal(cols, p.cols) and torch.equal(rows, p.rows) and origin == p.origin
    assert tuple(p.image.shape) == size + (3,) and cols.device == v.device
    src = torch.arange(0, 41, step)[None]
    gains = None
    if exposure:
        gains = exposure_gains(mosaic_overlap_rays(v, src, M[:, ::step], cols, rows, step=2, layout="NHWC"), anchor=10)
        assert torch.equal(gains[0], p.gains)
    mo = mosaic_rays(v, src, M[:, ::step], cols, rows, mode=mode, layout="NHWC", gains=gains)
    assert torch.equal(mo.out[0], p.image) and torch.equal(mo.count[0], p.count) and int(p.count.max()) >= 2
    if not exposure:
        truth = cylinder_truth(world, origin, size, focal)
        where = (p.count.cpu().numpy() > 0) & np.isfinite(truth).all(-1)
        got = psnr(p.image.cpu().numpy() / 255.0, truth, where)
        err = abs(focal / 240.0 - 1)
        print("panorama_wide on the wide scene, %d levels: focal %.4f (%.5f relative), ok %d of 40, median %.3f dB over %d "
              "pixels of %d x %d" % (levels, focal, err, int(p.ok.sum()), got, int(where.sum()), size[1], size[0]))
        assert err <= 2 * WIDE[levels][0], (focal, err)
        assert got > WIDE[levels][1] - 0.5, got
