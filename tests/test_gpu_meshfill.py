"""The mosaic under the mesh rule on device tensors (papteam_opticalflow_amd/tensors.py: mosaic_mesh, neighbour_mesh,
stabilize_video_mesh_full -> papof_mosaic_mesh_tensor).  The device's output must be the BYTES of the numpy restatement
(tests/_meshfill_ref.py): frames and canvases down to 2 x 2 pixels and one tile row, the grids from one cell to 32 x 40, every
source count at which the kernel changes instance in all four modes, every frame and output dtype, both layouts and a permuted
view, a strided table, masks, gains, with and without the count, empty slots, tables with a NaN and an infinity and tables that
push samples out of the frame and pull them in; the two invariants of include/papof.h against mosaic and warp_mesh on the
device; the tile culling and the per-pixel early-out against PAPOF_MOSAIC_CULL=0 on tables that carry sources into tiles that
their matrices miss; reproducibility; the pipeline against its parts; the inputs left unchanged and the caller's stream order.
NaNs that arithmetic makes are compared without their sign bit (tests/test_gpu_mosaic.py's docstring)."""
import math

import numpy as np
import pytest

from _interp_ref import convert
from _meshfill_ref import gather_mesh, mosaic_mesh_reference
from test_gpu_mosaic import _frame_masks, _mats, _same, _sources
from test_gpu_refine import _NP, _as_layout, _guide

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ("first", "mean", "median", "feather")
SHAPES = [((37, 53), (40, 70), [(1, 1), (3, 2), (16, 16), (32, 40)]),   # (frames, canvas, the grids the frames admit)
          ((5, 64), (3, 130), [(1, 1), (3, 2)]),
          ((2, 2), (70, 9), [(1, 1)])]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _nhwc(t, layout):
    return t if layout == "NHWC" else t.permute(0, 2, 3, 1)


def _slot_tables(rng, n_out, N, grid, H, W, wild=True):
    """a table per slot: most of a few pixels' amplitude, every fourth slot zero, every fifth up to +-30 px (whole regions pushed
    out of the frame and pulled into it); with `wild` a NaN entry and an infinite one"""
    D = rng.normal(0, 1.5, (n_out, N, grid[0] + 1, grid[1] + 1, 2))
    for k in range(N):
        if k % 4 == 3:
            D[:, k] = 0.0
        if k % 5 == 1:
            D[:, k] = rng.uniform(-30, 30, D[:, k].shape)
    D[0, 0, 0, :, 1] -= float(H)          # the top row of slot (0, 0) pushes samples out of the frame
    if wild:
        D[-1, N // 2, -1, -1, 0] = math.nan
        D[0, N - 1, 0, 0, 1] = math.inf
    return D


def _gains(rng, n_out, N):
    return rng.uniform(0.5, 1.5, (n_out, N))


@pytest.mark.parametrize("frame,canvas,grids", SHAPES)
def test_every_shape_grid_dtype_layout_and_output(frame, canvas, grids):
    from papteam_opticalflow_amd.tensors import mosaic_mesh
    (H, W), (Hc, Wc) = frame, canvas
    T, n_out, N, C = 4, 2, 5, 3
    rng = np.random.default_rng(H * 1000 + W)
    runs, seen = 0, set()
    for gi, grid in enumerate(grids):
        for di, dtype in enumerate((torch.uint8, torch.float32, torch.float64)):
            frames = _guide(T, H, W, C, dtype, 3 + gi)
            M = _mats(rng, n_out, N, H, W, Hc, Wc)
            D = _slot_tables(rng, n_out, N, grid, H, W)
            src = _sources(rng, n_out, N, T)
            masks = _frame_masks(rng, T, H, W) if di != 1 else None
            gains = _gains(rng, n_out, N) if di != 0 else None
            tm = torch.from_numpy(M).to(torch.float32 if di == 1 else torch.float64).cuda()
            tD = torch.from_numpy(D).cuda()
            t_masks = None if masks is None else torch.from_numpy(masks).cuda()
            t_gains = None if gains is None else torch.from_numpy(gains).cuda()
            for mode in MODES:
                want64, wcnt = mosaic_mesh_reference(frames, src, tm.cpu().numpy(), D, (Hc, Wc), mode, gains, masks)
                seen |= set(np.unique(wcnt).tolist())
                for layout, odt in (("NHWC", None), ("NCHW", torch.uint8), ("NHWC", torch.float32), ("NCHW", torch.float64)):
                    t = _as_layout(frames, layout)
                    got = mosaic_mesh(t, src, tm, tD, (Hc, Wc), mode=mode, masks=t_masks, layout=layout, out_dtype=odt, gains=t_gains)
                    what = "%s grid %s frames %s %s %s out %s" % (frame, grid, dtype, mode, layout, odt)
                    assert got.out.shape == ((n_out, C, Hc, Wc) if layout == "NCHW" else (n_out, Hc, Wc, C)), what
                    _same(_nhwc(got.out, layout), convert(want64, _NP[odt or dtype]), what)
                    _same(got.count, wcnt, what + " count")
                    runs += 1
                # a permuted view of NHWC storage read as NCHW
                got = mosaic_mesh(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), src, tm, tD, (Hc, Wc), mode=mode,
                                  masks=t_masks, layout="NCHW", out_dtype=torch.float64, gains=t_gains)
                _same(_nhwc(got.out, "NCHW"), want64, "permuted view " + mode)
    assert runs == len(grids) * 3 * 4 * 4
    assert 0 in seen and max(seen) >= (2 if min(frame) > 2 else 1), seen  # pixels with no source and with several (2 x 2 frames: with one)


@pytest.mark.parametrize("N", [1, 3, 9, 17, 33, 64, 255])
def test_source_counts_in_every_mode_with_and_without_masks_gains_and_count(N):
    """every median instance (8, 16, 32 and 64 samples per lane) and the largest list, on a canvas with ragged tiles"""
    from papteam_opticalflow_amd import tensors
    T, H, W, n_out = 6, 37, 53, 2
    rng = np.random.default_rng(N)
    dtype, C, (Hc, Wc), grid = {1: (torch.uint8, 3, (40, 70), (16, 16)), 3: (torch.float32, 2, (70, 9), (3, 2)),
                                9: (torch.float64, 1, (3, 130), (1, 1)), 17: (torch.uint8, 3, (40, 70), (32, 40)),
                                33: (torch.float32, 2, (40, 70), (3, 2)), 64: (torch.uint8, 1, (40, 70), (16, 16)),
                                255: (torch.uint8, 3, (40, 70), (3, 2))}[N]
    frames = _guide(T, H, W, C, dtype, N + C)
    t = torch.from_numpy(frames).cuda()
    M = _mats(rng, n_out, N, H, W, Hc, Wc)
    D = _slot_tables(rng, n_out, N, grid, H, W)
    src = _sources(rng, n_out, N, T)
    src[0, N // 2] = src[0, 0]  # a repeated source
    masks, gains = _frame_masks(rng, T, H, W), _gains(rng, n_out, N)
    tm, tD, t_masks, t_gains = (torch.from_numpy(a).cuda() for a in (M, D, masks, gains))
    t_src = torch.from_numpy(src).to(torch.int32).cuda()
    most = 0
    for mode in MODES if N < 255 else ("first",):
        for mk, tmk, g, tg in ((None, None, None, None), (masks, t_masks.bool(), gains, t_gains)):
            want, wcnt = mosaic_mesh_reference(frames, src, M, D, (Hc, Wc), mode, g, mk, _NP[dtype])
            got = tensors.mosaic_mesh(t, t_src, tm, tD, (Hc, Wc), mode=mode, masks=tmk, layout="NHWC", gains=tg)
            what = "N %d %s C %d %s masks and gains %s" % (N, dtype, C, mode, mk is not None)
            _same(got.out, want, what)
            _same(got.count, wcnt, what + " count")
            most = max(most, int(wcnt.max()))
            # without the count (mode "first" then stops at the first live source): the same image
            ts, descs, _, _ = tensors._check([("frames", t)], "NHWC", None, 1)
            out, none = tensors._mosaic(ts, descs, t_src, tm, tensors.capi.DTYPE_F64, None if tmk is None else tmk.view(torch.uint8),
                                        Hc, Wc, mode, "NHWC", t.dtype, count=False, gains=tg, rule=tensors._MESH,
                                        tables=(tD, grid[0], grid[1]))
            assert none is None
            _same(out, want, what + " no count")
    if N == 255:
        with pytest.raises(ValueError):
            tensors.mosaic_mesh(t, t_src, tm, tD, (Hc, Wc), mode="median", layout="NHWC")
    assert most >= (2 if N >= 9 else 1), most


def test_a_strided_table_is_read_in_place():
    from papteam_opticalflow_amd.tensors import mosaic_mesh
    T, H, W, C, n_out, N, grid, (Hc, Wc) = 3, 37, 53, 3, 2, 4, (3, 2), (40, 70)
    rng = np.random.default_rng(31)
    f = _guide(T, H, W, C, torch.float32, 32)
    M, D, src = _mats(rng, n_out, N, H, W, Hc, Wc), _slot_tables(rng, n_out, N, grid, H, W), _sources(rng, n_out, N, T)
    # (n_out, N, 2, GH + 1, 2 (GW + 1)) storage: the components outermost, every other vertex column
    tD = torch.from_numpy(np.ascontiguousarray(np.repeat(D, 2, axis=3).transpose(0, 1, 4, 2, 3))).cuda().permute(0, 1, 3, 4, 2)[:, :, :, ::2]
    assert not tD.is_contiguous() and tuple(tD.shape) == D.shape
    assert tD.reshape((-1,) + tuple(tD.shape[2:])).data_ptr() == tD.data_ptr()  # a view: (out, k) is one axis
    got = mosaic_mesh(torch.from_numpy(f).cuda(), src, torch.from_numpy(M).cuda(), tD, (Hc, Wc), mode="mean", layout="NHWC")
    want, wcnt = mosaic_mesh_reference(f, src, M, D, (Hc, Wc), "mean", None, None, np.float32)
    _same(got.out, want, "strided table")
    _same(got.count, wcnt, "strided table count")
    # one table for every slot (stride 0), and a slice of the slot axis that has to be copied
    one = torch.from_numpy(D[:1, :1]).cuda()
    got = mosaic_mesh(torch.from_numpy(f).cuda(), src, torch.from_numpy(M).cuda(), one.expand(n_out, N, -1, -1, -1), (Hc, Wc),
                      mode="first", layout="NHWC")
    want, wcnt = mosaic_mesh_reference(f, src, M, np.broadcast_to(D[:1, :1], D.shape), (Hc, Wc), "first", None, None, np.float32)
    _same(got.out, want, "expanded table")
    tall = torch.from_numpy(np.concatenate([D, D[:, ::-1]], 1)).cuda()
    got = mosaic_mesh(torch.from_numpy(f).cuda(), src, torch.from_numpy(M).cuda(), tall[:, :N], (Hc, Wc), mode="median", layout="NHWC")
    want, wcnt = mosaic_mesh_reference(f, src, M, D, (Hc, Wc), "median", None, None, np.float32)
    _same(got.out, want, "copied table")
    _same(got.count, wcnt, "copied table count")


@pytest.mark.parametrize("grid", [(1, 1), (16, 16), (32, 40)])
def test_invariant_a_zero_tables_give_the_bytes_of_mosaic(grid):
    from papteam_opticalflow_amd.tensors import mosaic, mosaic_mesh
    T, H, W, n_out, N, (Hc, Wc) = 5, 37, 53, 2, 9, (40, 70)
    rng = np.random.default_rng(41)
    M = torch.from_numpy(_mats(rng, n_out, N, H, W, Hc, Wc)).cuda()
    src = _sources(rng, n_out, N, T)
    Z = torch.zeros((n_out, N, grid[0] + 1, grid[1] + 1, 2), dtype=torch.float64).cuda()
    mk, g = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda(), torch.from_numpy(_gains(rng, n_out, N)).cuda()
    live = 0
    for fdt in (torch.uint8, torch.float32, torch.float64):
        v = torch.from_numpy(_guide(T, H, W, 3, fdt, 42)).cuda()
        for mode in MODES:
            for masks, gains in ((None, None), (mk, None), (None, g), (mk, g)):
                a = mosaic(v, src, M, (Hc, Wc), mode=mode, masks=masks, layout="NHWC", gains=gains, out_dtype=torch.float64)
                m = mosaic_mesh(v, src, M, Z, (Hc, Wc), mode=mode, masks=masks, layout="NHWC", gains=gains, out_dtype=torch.float64)
                what = (grid, fdt, mode, masks is not None, gains is not None)
                assert torch.equal(a.out.view(torch.int64), m.out.view(torch.int64)) and torch.equal(a.count, m.count), what
                live = max(live, int(a.count.max()))
    assert live >= 2


@pytest.mark.parametrize("grid", [(1, 1), (16, 16), (32, 40)])
def test_invariant_b_one_slot_per_frame_is_warp_mesh(grid):
    from papteam_opticalflow_amd.tensors import mosaic_mesh, warp_mesh
    from test_gpu_mesh import _frames, _tables, _warp_matrices
    B, H, W, C = 3, 33, 47, 3
    M = torch.from_numpy(_warp_matrices(H, W)).cuda()
    D = torch.from_numpy(_tables(B, grid, 43, 1.5)).cuda()
    for fdt in (torch.uint8, torch.float32, torch.float64):
        v = torch.from_numpy(_frames(B, H, W, C, _NP[fdt], 44)).cuda()
        for odt in (None, torch.float64):
            w, valid = warp_mesh(v, M, D, layout="NHWC", out_dtype=odt)
            m = mosaic_mesh(v, np.arange(B)[:, None], M[:, None], D[:, None], (H, W), mode="first", layout="NHWC", out_dtype=odt)
            assert torch.equal(w.view(torch.uint8), m.out.view(torch.uint8)), (grid, fdt, odt)
            assert torch.equal(valid, m.count > 0) and int(m.count.max()) == 1
            assert 0 < int(valid.sum()) < valid.numel()


def _corner_box_drops(M, n_out, N, H, W, Hc, Wc, TY):
    """(n_out, N, Hc, Wc) bool: the pixel lies in a tile of 64 x TY whose UNWIDENED affine corner box (papof_mosaic_tensor's
    phase 1) drops the slot"""
    drop = np.zeros((n_out, N, Hc, Wc), bool)
    for r0 in range(0, Hc, TY):
        for x0 in range(0, Wc, 64):
            xa, xb, ra, rb = float(x0), float(min(x0 + 63, Wc - 1)), float(r0), float(min(r0 + TY - 1, Hc - 1))
            with np.errstate(invalid="ignore", over="ignore"):
                X = np.stack([(M[..., 0, 0] * x + M[..., 0, 1] * r) + M[..., 0, 2] for x in (xa, xb) for r in (ra, rb)])
                Y = np.stack([(M[..., 1, 0] * x + M[..., 1, 1] * r) + M[..., 1, 2] for x in (xa, xb) for r in (ra, rb)])
                miss = (X < -1).all(0) | (X > W).all(0) | (Y < -1).all(0) | (Y > H).all(0) | ~np.isfinite(M).all((-1, -2))
            drop[:, :, r0:r0 + TY, x0:x0 + 64] = miss[:, :, None, None]
    return drop


def test_culling_changes_no_byte(monkeypatch):
    """PAPOF_MOSAIC_CULL=0 walks every source in every tile and reads every table: the same bytes as with the widened corner
    box and the per-pixel early-out, on tables of up to +-30 px in some slots and zero in others, one table with a NaN (its
    bound proves nothing: kept), one matrix that is not finite (dropped), and a slot whose matrix misses every tile of the
    canvas' left edge while its table carries it back into the frame -- a kernel that forgot the widening loses those pixels."""
    from papteam_opticalflow_amd.tensors import mosaic_mesh
    T, H, W, N, n_out, Hc, Wc, grid = 5, 37, 53, 32, 2, 150, 200, (3, 2)
    rng = np.random.default_rng(51)
    f = _guide(T, H, W, 3, torch.float32, 52)
    M = _mats(rng, n_out, N, H, W, Hc, Wc)          # (wild: a NaN and an infinite entry)
    D = _slot_tables(rng, n_out, N, grid, H, W, wild=False)
    src = _sources(rng, n_out, N, T)
    M[:, 2] = [[0.25, 0.0, -20.0], [0.0, 0.2, 1.0]]  # X0 = x / 4 - 20: left of the frame for x < 76
    D[:, 2] = 0.0
    D[:, 2, ..., 0] = 25.0                           # and carried back by the table
    src[:, 2] = 1
    D[0, 5, 1, 1, 1] = math.nan                      # a NaN bound
    D[1, 7] = rng.uniform(-30, 30, D[1, 7].shape)
    masks = _frame_masks(rng, T, H, W)
    S, live, _, _, _ = gather_mesh(f, src, M, D, (Hc, Wc), masks)
    live = live.reshape(N, n_out, Hc, Wc).transpose(1, 0, 2, 3)
    for TY in (4, 2):
        saved = live & _corner_box_drops(M, n_out, N, H, W, Hc, Wc, TY)
        assert saved[:, 2].any() and saved.sum() > 1000, (TY, int(saved.sum()))
    t, tm, tD, mk = (torch.from_numpy(a).cuda() for a in (f, M, D, masks))
    for mode in MODES:
        monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)
        on = mosaic_mesh(t, src, tm, tD, (Hc, Wc), mode=mode, masks=mk, layout="NHWC")
        monkeypatch.setenv("PAPOF_MOSAIC_CULL", "0")
        off = mosaic_mesh(t, src, tm, tD, (Hc, Wc), mode=mode, masks=mk, layout="NHWC")
        assert torch.equal(on.out.view(torch.int32), off.out.view(torch.int32)) and torch.equal(on.count, off.count), mode
        assert int(on.count.min()) == 0 and int(on.count.max()) >= 2
        if mode in ("first", "median"):
            want, wcnt = mosaic_mesh_reference(f, src, M, D, (Hc, Wc), mode, None, masks, np.float32)
            _same(off.out, want, "culling off " + mode)
            _same(on.count, wcnt, "culling on count " + mode)
    monkeypatch.delenv("PAPOF_MOSAIC_CULL", raising=False)


def test_runs_are_reproducible_and_an_output_is_the_same_alone_and_in_a_batch():
    from papteam_opticalflow_amd.tensors import mosaic_mesh
    T, H, W, N, n_out, (Hc, Wc), grid = 5, 37, 53, 17, 3, (40, 70), (16, 16)
    rng = np.random.default_rng(61)
    t = torch.from_numpy(_guide(T, H, W, 3, torch.float32, 62)).cuda()
    tm = torch.from_numpy(_mats(rng, n_out, N, H, W, Hc, Wc)).cuda()
    tD = torch.from_numpy(_slot_tables(rng, n_out, N, grid, H, W)).cuda()
    src = _sources(rng, n_out, N, T)
    for mode in MODES:
        a = mosaic_mesh(t, src, tm, tD, (Hc, Wc), mode=mode, layout="NHWC")
        b = mosaic_mesh(t, src, tm, tD, (Hc, Wc), mode=mode, layout="NHWC")
        assert torch.equal(a.out.view(torch.int32), b.out.view(torch.int32)) and torch.equal(a.count, b.count), mode
        for o in range(n_out):
            one = mosaic_mesh(t, src[o:o + 1], tm[o:o + 1], tD[o:o + 1], (Hc, Wc), mode=mode, layout="NHWC")
            assert torch.equal(one.out[0].view(torch.int32), a.out[o].view(torch.int32)), (mode, o)
            assert torch.equal(one.count[0], a.count[o]), (mode, o)


def test_stabilize_video_mesh_full_is_its_parts_and_stabilize_video_mesh_where_valid():
    """test_gpu_mesh's six frames of 68 x 120 at radius 3, filled from two neighbours either side.  Measured on an MI355X:
    the figures are printed."""
    from papteam_opticalflow_amd import tensors
    from test_gpu_stab import _jittered
    frames, _ = _jittered(T=6, Hc=68, Wc=120, seed=31)
    v = torch.from_numpy(frames).cuda()
    T, H, W, C = v.shape
    sv = tensors.stabilize_video_mesh(v, 2, layout="NHWC", radius=3)
    full = tensors.stabilize_video_mesh_full(v, 2, layout="NHWC", radius=3, fill_radius=2)
    assert isinstance(full, tensors.MeshStabilizedFull) and full._fields == tensors.MeshStabilized._fields + ("filled",)
    for name in ("valid", "transforms", "motion", "ok", "flow", "mesh", "vertex_motion", "support"):
        assert torch.equal(getattr(full, name), getattr(sv, name)), name
    assert full.video.dtype == torch.uint8 and tuple(full.video.shape) == (T, H, W, C)
    assert torch.equal(full.video[sv.valid], sv.video[sv.valid])
    assert not bool((full.filled & full.valid).any())
    # its parts chained by hand
    m = tensors.Motion(full.motion, full.ok, None)
    fb = tensors.flow_video_fb(v, 2, layout="NHWC")
    mm = tensors.mesh_motion(fb.flow_fw, motion=m, occlusion=fb.occlusion)
    src, mats = tensors.neighbour_transforms(full.transforms, m, 2)
    E = tensors.neighbour_mesh(mm, 3, 2)
    assert tuple(E.shape) == (T, 5, 17, 17, 2) and torch.equal(E[:, 0], sv.mesh)
    got = tensors.mosaic_mesh(v, src, mats, E, (H, W), mode="first", layout="NHWC")
    assert torch.equal(got.out, full.video)
    assert torch.equal((got.count > 0) & ~full.valid, full.filled)
    want, wcnt = mosaic_mesh_reference(v.cpu().numpy(), src.cpu().numpy(), mats.cpu().numpy(), E.cpu().numpy(), (H, W), "first",
                                       None, None, np.uint8)
    _same(full.video, want, "stabilize_video_mesh_full")
    invalid, filled = int((~full.valid).sum()), int(full.filled.sum())
    print("stabilize_video_mesh_full: %d of %d pixels invalid, %d of them filled" % (invalid, T * H * W, filled))
    assert invalid > 0 and filled > 0
    assert not bool(full.video[~full.valid & ~full.filled].any())  # what nobody saw stays 0
    # fill_radius=0: stabilize_video_mesh everywhere
    none = tensors.stabilize_video_mesh_full(v, 2, layout="NHWC", radius=3, fill_radius=0, out_dtype=torch.float32)
    sv32 = tensors.stabilize_video_mesh(v, 2, layout="NHWC", radius=3, out_dtype=torch.float32)
    assert torch.equal(none.video.view(torch.int32), sv32.video.view(torch.int32)) and torch.equal(none.valid, sv32.valid)
    assert not bool(none.filled.any())


def test_inputs_are_unchanged():
    from papteam_opticalflow_amd.tensors import mosaic_mesh
    T, H, W, N, Hc, Wc, grid = 4, 37, 53, 6, 40, 70, (3, 2)
    rng = np.random.default_rng(71)
    t = torch.from_numpy(_guide(T, H, W, 3, torch.float32, 72)).cuda()
    tm = torch.from_numpy(_mats(rng, 2, N, H, W, Hc, Wc)).cuda()
    tD = torch.from_numpy(_slot_tables(rng, 2, N, grid, H, W)).cuda()
    mk = torch.from_numpy(_frame_masks(rng, T, H, W)).cuda()
    g = torch.from_numpy(_gains(rng, 2, N)).cuda()
    src = torch.from_numpy(_sources(rng, 2, N, T)).cuda()
    keep = [x.clone() for x in (t, tm, mk, src, tD, g)]
    for mode in MODES:
        mosaic_mesh(t, src, tm, tD, (Hc, Wc), mode=mode, masks=mk, layout="NHWC", gains=g)
    torch.cuda.synchronize()
    assert torch.equal(t.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(mk, keep[2]) and torch.equal(src, keep[3])
    assert torch.equal(tm.view(torch.int64), keep[1].view(torch.int64))  # (the NaN entries included)
    assert torch.equal(tD.view(torch.int64), keep[4].view(torch.int64)) and torch.equal(g, keep[5])


def test_the_call_is_ordered_on_the_callers_stream():
    """Inputs written on a side stream behind a long sleep and used under that stream with no synchronisation: both kernels
    (the tables' bounds, then the mosaic) must read them after they are written, and what is queued behind must see the output"""
    import time
    from papteam_opticalflow_amd.tensors import mosaic_mesh
    T, H, W, Hc, Wc, grid = 5, 40, 60, 50, 90, (3, 2)
    rng = np.random.default_rng(81)
    f = _guide(T, H, W, 3, torch.uint8, 82)
    M = _mats(rng, 2, T, H, W, Hc, Wc)
    D = _slot_tables(rng, 2, T, grid, H, W)
    masks = _frame_masks(rng, T, H, W)
    want, wcnt = mosaic_mesh_reference(f, None, M, D, (Hc, Wc), "median", None, masks, np.uint8)
    src = [torch.from_numpy(a).cuda() for a in (f, M, masks, D)]
    dst = [torch.zeros_like(s) for s in src]
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = mosaic_mesh(dst[0], None, dst[1], dst[3], (Hc, Wc), masks=dst[2], layout="NHWC").out.clone()
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
        got = mosaic_mesh(dst[0], None, dst[1], dst[3], (Hc, Wc), masks=dst[2], layout="NHWC")
        took = time.perf_counter() - t0
        copy, ccopy = got.out.clone(), got.count.clone()  # queued behind the kernels on the same stream
    side.synchronize()
    assert took < 0.25, "the call waited for the stream: %.3f s" % took
    _same(got.out, want, "side stream")
    _same(copy, want, "side stream clone")
    _same(ccopy, wcnt, "side stream count")
