"""Spatially varying stabilization on device tensors (papteam_opticalflow_amd/tensors.py: mesh_motion, warp_mesh,
stabilize_video_mesh -> papof_mesh_motion_tensor, papof_warp_mesh_tensor).  Both kernels must return the BYTES of the numpy
fp64 restatement (tests/_mesh_ref.py): k_mesh_median's vertices, residuals and support on clipped border windows, a lattice
step above 1, cells of one pixel, float32 and float64 flows, with and without global motion and mask, NaNs, infinities,
flows that leave the image, a fully occluded window, the spatial pass on and off and strided views -- and the same bytes
from run to run and alone or in a batch; k_warp_mesh's frames and valid on uint8, float32 and float64 frames in and out,
NCHW, NHWC and a permuted view, tables staged in LDS and read from global memory, matrices that leave the mesh,
displacements that leave the frame, a NaN in the table, and warp_affine's bytes on a zero table; stabilize_video_mesh is its
parts chained by hand, and stabilize_video at radius 0."""
import math

import numpy as np
import pytest

from _mesh_ref import lattice_step, mesh_motion_reference, warp_mesh_reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _motions(B, H, W, rng):
    A = np.empty((B, 2, 3))
    for i in range(B):
        A[i, :, :2] = np.eye(2) + rng.normal(0, 0.01, (2, 2))
        A[i, :, 2] = rng.normal(0, 1.5, 2)
    return A


def _flows(B, H, W, seed):
    """B flows: an affine motion plus noise, with NaNs, infinities, a band that leaves the image and a block of outliers;
    (flows, the motions, a mask (B, H, W) that covers one whole vertex window of the grids used here and scattered pixels)"""
    rng = np.random.default_rng(seed)
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    A = _motions(B, H, W, rng)
    f = np.empty((B, 2, H, W))
    for i in range(B):
        f[i, 0] = A[i, 0, 0] * x + A[i, 0, 1] * r + A[i, 0, 2] - x
        f[i, 1] = A[i, 1, 0] * x + A[i, 1, 1] * r + A[i, 1, 2] - r
    f += rng.normal(0, 0.3, f.shape)
    f[:, 0, H // 5, ::3] = math.nan
    f[:, 1, H // 3, ::4] = math.inf
    f[:, 0, H // 2, 1::5] = -math.inf
    f[:, 0, 2 * H // 3:2 * H // 3 + 2, :] = 3.0 * W          # leaves the image
    f[0, :, :H // 4, W // 2:W // 2 + W // 6] = -4.0          # a block moving its own way
    f[B - 1, 1, :, :W // 8] = -2.0 * H                        # a border strip of the last pair leaves it
    occ = (rng.random((B, H, W)) < 0.08).astype(np.uint8)
    occ[0, :H // 2 + 1, :W // 2 + 1] = 1                      # every window of the top-left vertices of pair 0
    return f, A, occ


def _check_motion(got, ref, what):
    vert, sup, res = ref
    gs = got.support.cpu().numpy()
    assert gs.dtype == np.int32 and np.array_equal(gs, sup), (what, gs, sup)
    assert got.residuals.cpu().numpy().tobytes() == res.tobytes(), what
    assert got.vertices.cpu().numpy().tobytes() == vert.tobytes(), what


_SMALL = {}


def _small():
    if not _SMALL:
        _SMALL["data"] = _flows(3, 33, 47, 11)
    return _SMALL["data"]


@pytest.mark.parametrize("grid", [(3, 2), (4, 5), (1, 1)])
def test_median_matches_the_restatement_on_clipped_windows(grid):
    """33 x 47 is a multiple of no grid here: the border windows are clipped; the lattice steps are 2, 1 and 3"""
    from papteam_opticalflow_amd.tensors import mesh_motion
    f, A, occ = _small()
    assert lattice_step(33, 47, *grid) == {(3, 2): 2, (4, 5): 1, (1, 1): 3}[grid]  # (1, 1): 47 * 33 > 1024 >= 31 * 22
    tA, tocc = torch.from_numpy(A).cuda(), torch.from_numpy(occ).cuda()
    seen_invalid = False
    for fdt in (torch.float64, torch.float32):
        tf = torch.from_numpy(f).to(fdt).cuda()
        nf = tf.cpu().numpy()
        for use_motion in (False, True):
            for use_occ in (False, True):
                for spatial in (True, False):
                    what = "%s %s motion %s mask %s spatial %s" % (grid, fdt, use_motion, use_occ, spatial)
                    got = mesh_motion(tf, motion=tA if use_motion else None, occlusion=tocc if use_occ else None, grid=grid,
                                      min_support=16, spatial=spatial)
                    ref = mesh_motion_reference(nf, A if use_motion else None, occ if use_occ else None, grid, 16, spatial)
                    _check_motion(got, ref, what)
                    seen_invalid |= bool((ref[1] < 16).any())
    assert seen_invalid or grid == (1, 1)  # the fully occluded window was among the cases


def test_median_with_a_lattice_step_above_one():
    """135 x 240 with 2 x 2 cells: an unclipped window is 240 x 135 pixels, sampled every 6th"""
    from papteam_opticalflow_amd.tensors import mesh_motion
    H, W, grid = 135, 240, (2, 2)
    assert lattice_step(H, W, *grid) == 6
    f, A, occ = _flows(2, H, W, 12)
    tf = torch.from_numpy(f).cuda()
    for spatial in (True, False):
        got = mesh_motion(tf, motion=torch.from_numpy(A).cuda(), occlusion=torch.from_numpy(occ).cuda().bool(), grid=grid,
                          spatial=spatial)
        ref = mesh_motion_reference(f, A, occ, grid, 16, spatial)
        _check_motion(got, ref, "step 6 spatial %s" % spatial)
        assert ref[1].max() > 512  # more samples than two rounds of the block's lanes
    got = mesh_motion(tf, grid=(8, 8))
    _check_motion(got, mesh_motion_reference(f, None, None, (8, 8), 16, True), "8 x 8, step 2")


def test_cells_of_one_pixel_are_all_below_min_support():
    from papteam_opticalflow_amd.tensors import Motion, mesh_motion
    rng = np.random.default_rng(13)
    f = rng.normal(0, 0.5, (2, 2, 9, 9))
    A = _motions(2, 9, 9, rng)
    tf = torch.from_numpy(f).cuda()
    for spatial in (True, False):
        got = mesh_motion(tf, motion=torch.from_numpy(A).cuda(), grid=(8, 8), spatial=spatial)
        ref = mesh_motion_reference(f, A, None, (8, 8), 16, spatial)
        _check_motion(got, ref, "9 x 9 spatial %s" % spatial)
        assert ref[1].max() <= 9 and not ref[2].any()
    got = mesh_motion(tf, motion=torch.from_numpy(A).cuda(), grid=(8, 8), min_support=4)  # now the interior is valid
    _check_motion(got, mesh_motion_reference(f, A, None, (8, 8), 4, True), "9 x 9 min_support 4")
    # a Motion whose pair is not ok enters as the identity
    ok = torch.tensor([True, False]).cuda()
    got = mesh_motion(tf, motion=Motion(torch.from_numpy(A).cuda(), ok, None), grid=(2, 2), min_support=4)
    A2 = A.copy()
    A2[1] = np.eye(2, 3)
    _check_motion(got, mesh_motion_reference(f, A2, None, (2, 2), 4, True), "Motion with ok False")


def test_median_reads_strided_views_in_place():
    from papteam_opticalflow_amd.tensors import mesh_motion
    f, A, occ = _small()
    B, _, H, W = f.shape
    big = torch.from_numpy(np.ascontiguousarray(f.transpose(0, 2, 3, 1))).cuda()  # (B, H, W, 2) read as (B, 2, H, W)
    tf = big.permute(0, 3, 1, 2)
    wide = torch.from_numpy(np.repeat(f, 2, axis=3)).cuda()[:, :, :, ::2]           # every other column of a wider tensor
    mask4 = torch.from_numpy(np.stack([occ, 1 - occ], 1)).cuda()                    # (B, 2, H, W): channel 0 is read
    tA = torch.from_numpy(np.repeat(A, 2, axis=0)).cuda()[::2]
    assert not tf.is_contiguous() and not wide.is_contiguous() and not tA.is_contiguous()
    ref = mesh_motion_reference(f, A, occ, (4, 5), 16, True)
    for t in (tf, wide):
        _check_motion(mesh_motion(t, motion=tA, occlusion=mask4, grid=(4, 5)), ref, "strided")


def test_median_is_reproducible_and_independent_of_the_batch():
    from papteam_opticalflow_amd.tensors import mesh_motion
    f, A, occ = _small()
    tf, tA, tocc = torch.from_numpy(f).cuda(), torch.from_numpy(A).cuda(), torch.from_numpy(occ).cuda()
    a = mesh_motion(tf, motion=tA, occlusion=tocc, grid=(4, 5))
    b = mesh_motion(tf, motion=tA, occlusion=tocc, grid=(4, 5))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for i in range(f.shape[0]):
        one = mesh_motion(tf[i:i + 1], motion=tA[i:i + 1], occlusion=tocc[i:i + 1], grid=(4, 5))
        for x, y in zip(one, a):
            assert torch.equal(x[0].view(torch.uint8), y[i].view(torch.uint8)), i


# ---- k_warp_mesh
def _frames(B, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (B, H, W, C)).astype(np.uint8)
    return rng.random((B, H, W, C)).astype(dtype)


def _warp_matrices(H, W):
    """a rotation with zoom about the centre (its corners leave the frame and the mesh: the clamp), a small shift, and a
    zoom out by 1.6 (most of the output samples outside)"""
    cx, cy = (W - 1) / 2, (H - 1) / 2
    out = []
    for s, deg, tx, ty in ((1.05, 8.0, 1.25, -0.5), (1.0, 0.0, 0.375, 0.625), (1.6, -3.0, 0.0, 0.0)):
        a, b = s * math.cos(math.radians(deg)), s * math.sin(math.radians(deg))
        out.append([[a, -b, cx - a * cx + b * cy + tx], [b, a, cy - b * cx - a * cy + ty]])
    return np.array(out)


def _tables(B, grid, seed, amp):
    rng = np.random.default_rng(seed)
    D = rng.normal(0, amp, (B, grid[0] + 1, grid[1] + 1, 2))
    D[0, 0, :, 1] -= 6.0                   # the top row of frame 0 pushes samples out of the frame
    D[1, -1, -1] = math.nan                # one NaN entry: its cell is not valid
    return D


def _same_bytes(got, want, layout, what):
    g = got.cpu().numpy()
    if layout == "NCHW":
        g = g.transpose(0, 2, 3, 1)
    assert g.dtype == want.dtype and np.ascontiguousarray(g).tobytes() == want.tobytes(), what


@pytest.mark.parametrize("shape,grids", [((33, 47, 3), [(1, 1), (3, 2), (16, 16), (32, 40)]),
                                          ((5, 64, 1), [(1, 1), (3, 2), (4, 16), (4, 63)])])
@pytest.mark.parametrize("fdt", [torch.uint8, torch.float32, torch.float64])
def test_warp_matches_the_restatement(shape, grids, fdt):
    """grids of at most 33 x 33 vertices are staged in LDS, (32, 40) is read from global memory; 5 rows take at most 4 cells,
    so the 5 x 64 frames replace (16, 16) by (4, 16) and end at their largest grid"""
    from papteam_opticalflow_amd.tensors import warp_mesh
    H, W, C = shape
    B = 3
    f = _frames(B, H, W, C, _NP[fdt], 21)
    M = _warp_matrices(H, W)
    tM = torch.from_numpy(M).cuda()
    nhwc = torch.from_numpy(f).cuda()
    nchw = nhwc.permute(0, 3, 1, 2).contiguous()
    for grid in grids:
        D = _tables(B, grid, 22, 1.5)
        tD = torch.from_numpy(D).cuda()
        for odt in (torch.uint8, torch.float32, torch.float64):
            want, wvalid = warp_mesh_reference(f, M, D, _NP[odt])
            what = "%s %s -> %s grid %s" % (shape, fdt, odt, grid)
            got, valid = warp_mesh(nhwc, tM, tD, layout="NHWC", out_dtype=odt)
            _same_bytes(got, want, "NHWC", what)
            assert np.array_equal(valid.cpu().numpy(), wvalid), what
            assert 0 < wvalid.sum() < wvalid.size
        plain = warp_mesh_reference(f, M, np.zeros_like(D), _NP[fdt])[1]
        assert (plain[0] & ~wvalid[0]).any() and (plain[1] & ~wvalid[1]).any()  # pushed out by the table; the NaN's cell
        got, valid = warp_mesh(nchw, tM, tD, layout="NCHW")
        want, wvalid = warp_mesh_reference(f, M, D, _NP[fdt])
        _same_bytes(got, want, "NCHW", "NCHW %s" % (grid,))
        got, valid = warp_mesh(nhwc.permute(0, 3, 1, 2), tM.float(), tD, layout="NCHW")  # a permuted view, float32 matrices
        want, wvalid = warp_mesh_reference(f, M.astype(np.float32), D, _NP[fdt])
        _same_bytes(got, want, "NCHW", "permuted view %s" % (grid,))
        assert np.array_equal(valid.cpu().numpy(), wvalid)


def test_warp_reads_a_strided_table():
    from papteam_opticalflow_amd.tensors import warp_mesh
    B, H, W, C, grid = 3, 33, 47, 3, (3, 2)
    f = _frames(B, H, W, C, np.float32, 23)
    M, D = _warp_matrices(H, W), _tables(B, grid, 24, 1.0)
    tD = torch.from_numpy(np.ascontiguousarray(np.repeat(D, 2, axis=2).transpose(0, 3, 1, 2))).cuda().permute(0, 2, 3, 1)[:, :, ::2]
    assert not tD.is_contiguous() and tuple(tD.shape) == D.shape
    got, valid = warp_mesh(torch.from_numpy(f).cuda(), torch.from_numpy(M).cuda(), tD, layout="NHWC")
    want, wvalid = warp_mesh_reference(f, M, D, np.float32)
    _same_bytes(got, want, "NHWC", "strided table")
    assert np.array_equal(valid.cpu().numpy(), wvalid)


@pytest.mark.parametrize("grid", [(1, 1), (16, 16), (32, 40)])
def test_a_zero_table_gives_the_bytes_of_warp_affine(grid):
    from papteam_opticalflow_amd.tensors import warp_affine, warp_mesh
    B, H, W, C = 3, 33, 47, 3
    M = torch.from_numpy(_warp_matrices(H, W)).cuda()
    Z = torch.zeros((B, grid[0] + 1, grid[1] + 1, 2), dtype=torch.float64).cuda()
    for fdt in (torch.uint8, torch.float32, torch.float64):
        v = torch.from_numpy(_frames(B, H, W, C, _NP[fdt], 25)).cuda()
        for odt in (None, torch.float64):
            a, va = warp_affine(v, M, layout="NHWC", out_dtype=odt)
            m, vm = warp_mesh(v, M, Z, layout="NHWC", out_dtype=odt)
            assert torch.equal(a.view(torch.uint8), m.view(torch.uint8)) and torch.equal(va, vm), (grid, fdt, odt)


# ---- stabilize_video_mesh
@pytest.fixture(scope="module")
def video():
    from test_gpu_stab import _jittered
    frames, _ = _jittered(T=6, Hc=68, Wc=120, seed=31)
    return torch.from_numpy(frames).cuda()


def test_stabilize_video_mesh_is_its_parts(video):
    from papteam_opticalflow_amd.tensors import (flow_video_fb, global_motion, mesh_motion, mesh_transforms,
                                                 stabilize_video_mesh, stabilizing_transforms, warp_mesh)
    T, H, W, C = video.shape
    sv = stabilize_video_mesh(video, 2, layout="NHWC", radius=3, crop=0.95)
    assert tuple(sv.video.shape) == (T, H, W, C) and sv.video.dtype == torch.uint8
    assert tuple(sv.mesh.shape) == (T, 17, 17, 2) and tuple(sv.vertex_motion.shape) == (T - 1, 17, 17, 2)
    assert tuple(sv.support.shape) == (T - 1, 17, 17) and sv.support.dtype == torch.int32
    fb = flow_video_fb(video, 2, layout="NHWC")
    assert torch.equal(fb.flow_fw, sv.flow)
    m = global_motion(fb.flow_fw, model="similarity")
    assert torch.equal(m.motion, sv.motion) and torch.equal(m.ok, sv.ok)
    mm = mesh_motion(fb.flow_fw, motion=m, occlusion=fb.occlusion)
    assert torch.equal(mm.vertices, sv.vertex_motion) and torch.equal(mm.support, sv.support)
    M = stabilizing_transforms(m, 3, 0.95, size=(H, W))
    D = mesh_transforms(mm, 3)
    assert torch.equal(M, sv.transforms) and torch.equal(D, sv.mesh) and bool(D.abs().max() > 0)
    w, valid = warp_mesh(video, M, D, layout="NHWC")
    assert torch.equal(w, sv.video) and torch.equal(valid, sv.valid)
    # consistency=None: flow_video and no mask
    sn = stabilize_video_mesh(video, 2, layout="NHWC", radius=3, consistency=None, grid=(4, 6), spatial=False, min_support=8)
    mn = mesh_motion(sn.flow, motion=global_motion(sn.flow, model="similarity"), grid=(4, 6), spatial=False, min_support=8)
    assert torch.equal(sn.flow, sv.flow) and torch.equal(mn.vertices, sn.vertex_motion)
    # the device's medians on real flows are the restatement's
    ref = mesh_motion_reference(fb.flow_fw.cpu().numpy(), m.motion.cpu().numpy(), fb.occlusion[:, 0].cpu().numpy(), (16, 16))
    _check_motion(mm, ref, "real flows")


def test_stabilize_video_mesh_at_radius_zero_is_stabilize_video(video):
    from papteam_opticalflow_amd.tensors import stabilize_video, stabilize_video_mesh
    a = stabilize_video(video, 2, layout="NHWC", radius=0, crop=0.9)
    b = stabilize_video_mesh(video, 2, layout="NHWC", radius=0, crop=0.9)
    assert not bool(b.mesh.any())
    assert torch.equal(a.video, b.video) and torch.equal(a.valid, b.valid) and torch.equal(a.transforms, b.transforms)
    a = stabilize_video(video, 2, layout="NHWC", radius=0, out_dtype=torch.float64, model="affine")
    b = stabilize_video_mesh(video, 2, layout="NHWC", radius=0, out_dtype=torch.float64, model="affine", grid=(3, 5))
    assert torch.equal(a.video, b.video) and torch.equal(a.valid, b.valid)
