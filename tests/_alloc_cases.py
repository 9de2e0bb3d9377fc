"""The table of tests/test_gpu_alloc_guard.py: one row per public device-tensor call of papteam_opticalflow_amd/tensors.py, at
the smallest shapes at which its kernel can still go wrong (tests/_alloc.py has the why).

A row names the tensors.py function, the C entry points it must launch, and a builder that gives
  inputs   {name: numpy array}: placed on the device with Guarded.put (guard bands around each, checked unchanged afterwards)
  run      ({name: device tensor}) -> [output tensors]
  want     [numpy arrays]: the expected outputs, BYTES -- from the numpy restatements (tests/_*_ref.py), never from the library
  check    for the calls that the project pins within a bound (the fits, the bundle sums: their own tests' checks, imported;
           the flow calls: the oracle within _libs.ORACLE_BOUND, which tests/test_gpu_fuzz_small.py and
           tests/test_gpu_batch_shapes.py hold them to), a function (outputs, what) that asserts that bound; `want` then
           holds the restatement's outputs, which pass it.  Whatever the bound, the outputs under the two patterns must
           have the same bytes.
  derived  the outputs that the wrapper computes with torch from what a kernel wrote (match_init's `reliable` is
           mask == 0): every other output must lie in memory that tensors._torch().empty served

The builders of tests/_seam.py give inputs, a reference and a call for 31 rows; they are used at count = P (or the 2 reach + 3
frames of a temporal call) with no periodic expansion.  The other rows are written here with the inputs of each call's own
GPU test, so that the branches that skip a store are taken: `dead` says which output elements of the row come from a branch
that computes nothing (a dead pixel, an absent slot, a refused query), which is where a kernel may forget its store, and
the builder asserts on the expected outputs that such elements are there.

Shapes: one ragged tile on the right and one on the bottom border of the kernel's own tile, at most four tiles; three items
(a first, a middle and a last) or _seam's seven; 2 reach + 3 frames for the temporal calls."""
import collections
import functools

import numpy as np

import _seam
from _libs import ORACLE_BOUND
from _seam import CONSISTENCY, P, flows, frames, index

Row = collections.namedtuple("Row", "name fn entries dead build")
Built = collections.namedtuple("Built", "inputs run want check derived", defaults=(None, None, ()))


def _torch():
    import torch
    return torch


# ---- rows from the builders of tests/_seam.py

def _seam_row(name, entries, dead, reach=None, derived=()):
    """reach: a predicate on the expected outputs that holds when the row has the elements that `dead` names"""
    case = {c.name: c for c in _seam.CASES}[name]

    def build():
        b = case.build()
        assert b.tol is None
        if case.oracle == "temporal":
            n = max(P, 2 * b.reach + 3)
            inputs = {k: a if kind == "full" else a[index(n - (b.gap if kind == "pair" else 0), a.shape[0])]
                      for k, (a, kind) in b.inputs.items()}
            want = b.ref(0, n)
        else:
            inputs = {k: a for k, (a, kind) in b.inputs.items()}
            want = b.ref()
        want = [np.ascontiguousarray(w) for w in want]
        assert reach is None or reach(want), "%s: no output element from the branch that the row names" % name
        return Built({k: np.ascontiguousarray(a) for k, a in inputs.items()}, b.run, want, derived=derived)
    return Row(name, case.fn, tuple(entries), dead, build)


# ---- the fits and the bundle sums: _seam's inputs with a fully masked item and one whose flow is NaN everywhere, so that
# the branch that writes the identity and ok = False (sums of zero) runs; held to the restatement by the check of the call's
# own GPU test (corners within 1e-8 px, ok equal, support within 1e-12; the sums within (n - 1) 2^-53 of their magnitudes)

NAN_ITEM, MASKED_ITEM = 2, 4


def _seam_inputs(name):
    b = {c.name: c for c in _seam.CASES}[name].build()
    inputs = {k: np.array(a) for k, (a, kind) in b.inputs.items()}  # copies: the items below are overwritten
    return b, inputs


def _fit(kind):
    def build():
        import collections as c
        Got = c.namedtuple("Got", "motion ok support")
        b, inputs = _seam_inputs("global_motion" if kind == "affine" else "global_homography")
        f, occ = inputs["f"], inputs["occ"]
        f[NAN_ITEM] = np.nan
        occ[MASKED_ITEM] = 1
        if kind == "affine":
            import test_gpu_stab as t
            want = t.fit_reference(f, occ, t.AFFINE, 3, 1.5)
        else:
            import test_gpu_homography as t
            from _homography_ref import fit_reference_h
            want = fit_reference_h(f, occ, 3, 1.5)
        motion, ok, support = (np.ascontiguousarray(w) for w in want)
        assert not ok[NAN_ITEM] and not ok[MASKED_ITEM] and ok.sum() >= 3, ok

        def check(got, what):
            g = Got(got[0], got[1].bool(), got[2])
            if kind == "affine":
                t._check_fit(g, f, occ, t.AFFINE, 3, what, 1.5)
            else:
                t._check_fit(g, f, occ, 3, what, 1.5)
        return Built(inputs, b.run, [motion.astype(np.float64), ok.astype(np.uint8), support.astype(np.float64)], check)
    return build


def _bundle_sums():
    import _bundle_ref as B
    import test_gpu_bundle as t
    b, inputs = _seam_inputs("bundle_sums")
    fl, Rij, occ = inputs["fl"], inputs["R"], inputs["occ"]
    fl[NAN_ITEM] = np.nan
    occ[MASKED_ITEM] = 1
    focal = 60.0  # _seam._bundle_sums
    want, _, n = B.sums_reference(fl, Rij, focal, occ, 1, 1.5)
    assert n[NAN_ITEM] == 0 and n[MASKED_ITEM] == 0 and (n > 0).sum() >= 3, n

    def check(got, what):
        t._check(got[0], fl, Rij, focal, occ, 1, 1.5, what)
    return Built(inputs, b.run, [np.ascontiguousarray(want, dtype=np.float64)], check)


# ---- rolling shutter, rows, deblur

def _rectify_frames(mats):
    def build():
        from _rolling_ref import rectify_reference
        from test_gpu_rolling import _matrices, _rs_fields
        from papteam_opticalflow_amd import tensors
        T, H, W, C = 3, 5, 66, 2
        f = frames(T, H, W, C, 80)
        fw, bw = _rs_fields(T, H, W, 81)
        inputs = {"f": f, "fw": fw, "bw": bw}
        M = None
        if mats:
            M = inputs["M"] = _matrices(T, H, W, 82)
        video, valid = rectify_reference(f, fw, bw, 0.8, 0.5, 3, M, np.uint8)[:2]
        assert valid.any() and not valid.all()

        def run(d):
            out, ok = tensors.rectify_frames(d["f"], d["fw"], d["bw"], 0.8, anchor=0.5, iters=3, matrices=d.get("M"),
                                             layout="NHWC")
            return [out, ok]
        return Built(inputs, run, [video, valid.astype(np.uint8)])
    return build


def _rectify_flows():
    from _rolling_ref import flows_reference
    from test_gpu_rolling import _rs_fields
    from papteam_opticalflow_amd import tensors
    T, H, W = 4, 5, 66
    fw, bw = _rs_fields(T, H, W, 83)
    want = flows_reference(fw, bw, 0.8, 0.5, 3, np.float64)[:2]
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()

    def run(d):
        got = tensors.rectify_flows(d["fw"], d["bw"], 0.8, anchor=0.5, iters=3)
        return [got.flow_fw, got.flow_bw]
    return Built({"fw": fw, "bw": bw}, run, list(want))


def _warp_rows():
    from _rows_ref import warp_rows_reference
    from test_rows_cpu import some_tables
    from papteam_opticalflow_amd import tensors
    B, H, W, C, Kn = 3, 5, 66, 2, 3
    f = frames(B, H, W, C, 84)
    tab = some_tables(B, Kn, H, W, 85)
    tab[1, 1, 2, 2] = np.nan  # a knot that no row can use
    out, valid = warp_rows_reference(f, tab, 3, np.uint8)[:2]
    assert valid.any() and not valid.all()

    def run(d):
        got, ok = tensors.warp_rows(d["f"], d["tab"], iters=3, layout="NHWC")
        return [got, ok]
    return Built({"f": f, "tab": tab}, run, [out, valid.astype(np.uint8)])


def _deblur():
    from _deblur_ref import deblur_reference
    from test_gpu_deblur import _flows
    from papteam_opticalflow_amd import tensors
    T, H, W, C = 5, 5, 66, 3  # radius 1: 2 reach + 3 frames; frames 0 and 4 are end frames with absent slots
    f = frames(T, H, W, C, 86)
    f[:, :, :4] = 0  # a dark band: estimates under the floor
    fw, bw = _flows(T, H, W, 87)
    kw = dict(shutter=0.5, samples=5, phase=-0.5, shape="box")
    video, support = deblur_reference(f, fw, bw, *tensors.blur_schedule(0.5, 5, -0.5, "box"), radius=1, iters=2,
                                      consistency=CONSISTENCY, out_dtype=np.uint8)[:2]

    def run(d):
        got = tensors.deblur(d["f"], d["fw"], d["bw"], radius=1, iters=2, consistency=CONSISTENCY, layout="NHWC", **kw)
        return [got.video, got.support]
    return Built({"f": f, "fw": fw, "bw": bw}, run, [video, support])


# ---- fields and shots

def _field_metrics():
    from _telecine_ref import metrics_reference
    from test_gpu_telecine import COMB, DIFF, _fields
    from papteam_opticalflow_amd import tensors
    T, Hf, W, C = 3, 17, 65, 3  # cell_rows + 1 rows, 65 columns: a partial cell on both borders
    f = _fields(T, Hf, W, C, _torch().uint8, 88)
    want = metrics_reference(f, 1, 16, COMB, DIFF)
    assert want[1].any() and not want[[0, -1]].any()

    def run(d):
        return [tensors.field_metrics(d["f"], 1, cell_rows=16, layout="NHWC").counts]
    return Built({"f": f}, run, [np.ascontiguousarray(want, dtype=np.int32)])


def _weave_fields():
    from _telecine_ref import weave_reference
    from test_gpu_telecine import _fields
    from papteam_opticalflow_amd import tensors
    T, Hf, W, C = 4, 5, 66, 2
    f = _fields(T, Hf, W, C, _torch().uint8, 89)
    table = np.array([[2, 1], [0, 3], [1, 1]])  # out of order, one field twice
    want = weave_reference(f, table, np.uint8)

    def run(d):
        return [tensors.weave_fields(d["f"], table, layout="NHWC")]
    return Built({"f": f}, run, [want])


def _shot_histograms():
    from _shots_ref import hist_reference
    from test_gpu_shots import _frames
    from papteam_opticalflow_amd import tensors
    T, H, W, C = 3, 17, 65, 3
    f = _frames(T, H, W, C, _torch().float32, 90)  # NaNs and infinities, values beyond 0 .. 1
    want = hist_reference(f, 16, 16)

    def run(d):
        return [tensors.shot_histograms(d["f"], cell_rows=16, bins=16, layout="NHWC").hist]
    return Built({"f": f}, run, [np.ascontiguousarray(want, dtype=np.int32)])


# ---- decoder surfaces: an aligned semi-planar surface with a pitch beyond the row (the dword / 8-byte instance when W is a
# multiple of 4, lane by lane when not), odd H: the last chroma row serves one luma row

def _semi_planar(ps, pitch, fill):
    """the planes (y, cb, cr), 4:2:0, as one surface (T, H + Hc, pitch) whose other elements are `fill`"""
    T, H, W = ps[0].shape
    Hc, Wc = ps[1].shape[1:]
    s = np.full((T, H + Hc, pitch), fill, ps[0].dtype)
    s[:, :H, :W] = ps[0]
    s[:, H:, 0:2 * Wc:2], s[:, H:, 1:2 * Wc:2] = ps[1], ps[2]
    return s


def _ycc_to_rgb(W, fast, out):
    def build():
        import _surface_ref as R
        from test_surface_cpu import FORWARD_TABLES
        from papteam_opticalflow_amd import tensors
        T, H = 3, 5
        rng = np.random.default_rng(91 + W)
        Hc, Wc = R.chroma_size(H, W, 2)
        ps = [rng.integers(0, 256, s).astype(np.uint8) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc))]
        for p in ps:
            p.reshape(-1)[:2] = (0, 255)
        want = R.ycc_to_rgb_reference(*ps, FORWARD_TABLES, dtype=out)

        def run(d):
            from test_gpu_surface import _fast
            torch = _torch()
            planes = tensors.nv12_planes(d["surface"], H, "uv", width=W, sub_v=2)
            got = tensors.ycc_to_rgb(*planes, matrix="bt709", range="limited", layout="NHWC",
                                     out_dtype=torch.uint8 if out == np.uint8 else torch.float32)
            assert _fast(planes, got) == fast, "papof_ycc_to_rgb_fast says %d for W = %d" % (1 - fast, W)  # the witness
            return [got]
        return Built({"surface": _semi_planar(ps, 512, 0x5a)}, run, [want])
    return build


def _rgb_to_ycc():
    import _surface_ref as R
    from test_gpu_surface import _rgb
    from test_surface_cpu import REVERSE_TABLES
    from papteam_opticalflow_amd import tensors
    T, H, W = 3, 5, 66
    f = _rgb(T, H, W, _torch().float32, 92)  # NaNs, infinities, values beyond 0 .. 1
    want = R.rgb_to_ycc_reference(f, REVERSE_TABLES)

    def run(d):
        return list(tensors.rgb_to_ycc(d["f"], matrix="bt709", range="limited", layout="NHWC"))
    return Built({"f": f}, run, list(want))


def _ycc16_to_rgb(W, fast, out):
    def build():
        import _surface16_ref as R16
        from test_surface16_cpu import FORWARD_TABLES, random_words
        from papteam_opticalflow_amd import tensors
        T, H = 3, 5
        ps = random_words(np.random.default_rng(93 + W), T, H, W, 2, 10, 6)
        tab = FORWARD_TABLES if out == np.uint8 else R16.tables("bt709", "limited", 10, None)
        want = R16.ycc16_to_rgb_reference(*ps, tab, 10, 6, dtype=out)

        def run(d):
            from test_gpu_surface16 import _fast
            torch = _torch()
            planes = tensors.p010_planes(d["surface"], H, "uv", width=W, sub_v=2)
            got = tensors.ycc16_to_rgb(*planes, depth=10, aligned="msb", matrix="bt709", range="limited", layout="NHWC",
                                       out_dtype=torch.uint8 if out == np.uint8 else torch.float32)
            assert _fast(planes, got) == fast, "papof_ycc16_to_rgb_fast says %d for W = %d" % (1 - fast, W)  # the witness
            return [got]
        return Built({"surface": _semi_planar(ps, 384, 0x5a5a)}, run, [want])
    return build


def _rgb_to_ycc16():
    import _surface16_ref as R16
    from test_gpu_surface import _rgb
    from papteam_opticalflow_amd import tensors
    T, H, W = 3, 5, 66
    f = _rgb(T, H, W, _torch().float32, 94)
    want = R16.rgb_to_ycc16_reference(f, R16.reverse_tables("bt709", "limited", 10), 10, 6)

    def run(d):
        return list(tensors.rgb_to_ycc16(d["f"], depth=10, aligned="msb", matrix="bt709", range="limited", layout="NHWC"))
    return Built({"f": f}, run, [np.ascontiguousarray(w, dtype=np.uint16) for w in want])


# ---- temporal consistency

def _temporal_consistency():
    from _consistency_ref import consistency_reference
    from test_gpu_consistency import _video
    from papteam_opticalflow_amd import tensors
    T, H, W = 5, 5, 66
    torch = _torch()
    I, Pr, _, _ = _video(T, H, W, 3, 3, torch.uint8, torch.uint8, 95)
    fw, bw = flows(T - 1, H, W, 96)  # NaNs, infinities and displacements that leave the image
    want = consistency_reference(I, Pr, fw, bw, 4.0, 0.05, 7, CONSISTENCY, out_dtype=np.uint8)

    def run(d):
        return [tensors.temporal_consistency(d["I"], d["P"], d["fw"], d["bw"], lam=4.0, sigma=0.05, iters=7, layout="NHWC")]
    return Built({"I": I, "P": Pr, "fw": fw, "bw": bw}, run, [want])


# ---- the mosaics that _seam lacks: mesh tables, the ray canvas, the projective overlap

def _mosaic_mesh():
    from _interp_ref import convert
    from _meshfill_ref import mosaic_mesh_reference
    from test_gpu_meshfill import _slot_tables
    from test_gpu_mosaic import _frame_masks, _mats, _sources
    from papteam_opticalflow_amd import tensors
    T, H, W, C, Hc, Wc, n_out, N, grid = 4, 9, 13, 2, 5, 66, 3, 5, (2, 3)
    rng = np.random.default_rng(97)
    f = frames(T, H, W, C, 98)
    M = _mats(rng, n_out, N, H, W, Hc, Wc)
    D = _slot_tables(rng, n_out, N, grid, H, W)  # a NaN and an infinite entry, a top row pushed out of the frame
    src = _sources(rng, n_out, N, T)
    masks = _frame_masks(rng, T, H, W)
    want64, count = mosaic_mesh_reference(f, src, M, D, (Hc, Wc), "median", None, masks)
    assert 0 in count and count.max() >= 2

    def run(d):
        got = tensors.mosaic_mesh(d["f"], src, d["M"], d["D"], (Hc, Wc), mode="median", masks=d["masks"], layout="NHWC")
        return [got.out, got.count]
    return Built({"f": f, "M": M, "D": D, "masks": masks}, run, [convert(want64, np.uint8), np.asarray(count, np.uint8)])


def _mosaic3(what):
    def build():
        from _homography_ref import overlap_reference_h
        from _wide_ref import mosaic_reference_rays, overlap_reference_rays, plane_tables
        from test_gpu_mosaic import _frame_masks, _mats
        from papteam_opticalflow_amd import tensors
        T, H, W, C, Hc, Wc, n_out, N = 4, 9, 13, 2, 5, 66, 3, 2
        rng = np.random.default_rng(99)
        f = frames(T, H, W, C, 100)
        M3 = np.zeros((n_out, N, 3, 3))
        M3[..., :2, :], M3[..., 2, 2] = _mats(rng, n_out, N, H, W, Hc, Wc), 1.0
        M3[..., 2, :2] = rng.normal(0, 1e-3, (n_out, N, 2))
        src = np.array([[0, 1], [2, 3], [3, -1]])
        masks = _frame_masks(rng, T, H, W)
        cols, rows = plane_tables(Hc, Wc)
        cols[60:, 1] = -1.0   # the rays of the last columns point behind the camera
        cols[7, 0] = np.nan   # and one column has no ray at all
        inputs = {"f": f, "M": M3, "masks": masks}
        if what != "overlap-homography":
            inputs.update(cols=cols, rows=rows)
        if what == "rays":
            out, count = mosaic_reference_rays(f, src, M3, cols, rows, "mean", None, masks, np.uint8)
            assert 0 in count and count.max() >= 1
            want = [out, np.asarray(count, np.uint8)]
        elif what == "overlap-rays":
            want = [np.asarray(a, np.int64) for a in overlap_reference_rays(f, src, M3, cols, rows, 2, 1.0, masks)]
        else:
            want = [np.asarray(a, np.int64) for a in overlap_reference_h(f, src, M3, (Hc, Wc), 2, 1.0, masks)]

        def run(d):
            if what == "rays":
                got = tensors.mosaic_rays(d["f"], src, d["M"], d["cols"], d["rows"], mode="mean", masks=d["masks"], layout="NHWC")
                return [got.out, got.count]
            if what == "overlap-rays":
                got = tensors.mosaic_overlap_rays(d["f"], src, d["M"], d["cols"], d["rows"], masks=d["masks"], step=2,
                                                  layout="NHWC")
            else:
                got = tensors.mosaic_overlap_homography(d["f"], src, d["M"], (Hc, Wc), masks=d["masks"], step=2, layout="NHWC")
            return [got.sums, got.counts]
        return Built(inputs, run, want)
    return build


# ---- the densify pass alone, sparse and dense tracks

def _match_densify():
    """k_match_densify's own outputs before the fill: the flow (+0.0 where unreliable) and the hole mask of both directions"""
    from _match_ref import densify_reference, match_reference
    from papteam_opticalflow_amd import capi, tensors
    H, W, stride = 8, 8, 2
    a, b = _seam._textures(H, W, 1, 70, _seam._SHIFTS[:3])
    kw = dict(stride=stride, patch=1, search=2)
    dfw, cfw = match_reference(a, b, out_dtype=np.float32, **kw)
    dbw, cbw = match_reference(b, a, out_dtype=np.float32, **kw)
    max_cost = float(np.median(cfw))
    fw, hole_fw = densify_reference(dfw, dbw, cfw, (H, W), stride, 1, max_cost)
    bw, hole_bw = densify_reference(dbw, dfw, cbw, (H, W), stride, 1, max_cost)
    assert hole_fw.any() and not hole_fw.all()

    def run(d):
        f32 = (capi.DTYPE_F32, capi.DTYPE_F32)
        flow, mask = tensors._densify((d["dfw"], d["dbw"]), f32, (d["cfw"], d["cbw"]), f32, H, W, stride,
                                      *tensors._check_densify(1, max_cost))
        return [flow, mask]
    return Built({"dfw": dfw, "dbw": dbw, "cfw": cfw, "cbw": cbw}, run,
                 [np.concatenate([fw, bw]), np.concatenate([hole_fw, hole_bw]).astype(np.uint8)])


def _track_points(sparse):
    def build():
        from test_gpu_track import _fields, _queries
        from test_track_cpu import track_reference
        from papteam_opticalflow_amd import tensors
        T, H, W = 4, 5, 66
        fw, bw = _fields(T, H, W, 101)
        inputs = {"fw": fw, "bw": bw}
        if sparse:
            inputs["q"] = _queries(T, H, W, 30, 102)  # with every kind of invalid query
        tracks, vis = track_reference(fw, bw, inputs.get("q"))
        assert vis.any() and not vis.all() and np.isnan(tracks).any()

        def run(d):
            got = tensors.track_points(d["fw"], d["bw"], d.get("q"))
            return [got.tracks, got.visible]
        return Built(inputs, run, [tracks, vis.astype(np.uint8)])
    return build


# ---- the flow calls: the device's flows and warps within ORACLE_BOUND of the oracle, the mask the check's rule on the flows
# that the call returned (tests/test_gpu_fb.py: test_occlusion_mask_is_the_definition)

@functools.lru_cache(maxsize=None)
def _oracle():
    from _libs import OracleLib
    return OracleLib()


def _flow(B, fb, init):
    def build():
        import _batch_shapes as bs
        from _init_ref import coarse2fine_init
        from test_fb_cpu import fb_reference
        from papteam_opticalflow_amd import tensors
        H, W, C, levels = 37, 53, 3, 2
        c = bs.BY_NAME["37x53 init per pair"]
        assert (c.H, c.W, c.C) == (H, W, C) and c.params == bs.SMALL
        video = np.stack([bs.frame_u8(c, i) for i in range(B + 1)])
        inputs = {"video": video}
        ini = ini_bw = None
        if init:
            ini = inputs["init"] = bs.smooth_init(B, H, W)
            if fb:
                ini_bw = inputs["init_bw"] = np.ascontiguousarray(-0.5 * ini[..., ::-1])
        orc = _oracle()

        def direction(a, b, start):
            out = []
            for p in range(B):
                i0 = None if start is None else np.ascontiguousarray(start[p].transpose(1, 2, 0).astype(np.float64))
                out.append(coarse2fine_init(orc, video[p + a] / 255.0, video[p + b] / 255.0, levels, i0, **bs.SMALL))
            return (np.stack([np.stack([vx, vy]) for vx, vy, _ in out]), np.stack([w for _, _, w in out]))
        want = list(direction(0, 1, ini))
        if fb:  # and the mask: the check's rule on the oracle's flows (on the device: on the flows that the call returned)
            want += list(direction(1, 0, ini_bw))
            want.append(fb_reference(want[0], want[2]))
            assert 0 < want[4].sum() < want[4].size

        def run(d):
            kw = dict(layout="NHWC", **bs.SMALL)
            before = tensors._handle(0)[0].batch_stats()
            if fb:
                r = tensors.flow_video_fb(d["video"], levels, init_flow=d.get("init"), init_flow_bw=d.get("init_bw"), **kw)
                out = [r.flow_fw, r.warpI2_fw, r.flow_bw, r.warpI2_bw, r.occlusion]
            else:
                out = list(tensors.flow_video(d["video"], levels, init_flow=d.get("init"), **kw)[:2])
            after = tensors._handle(0)[0].batch_stats()
            added = {k: after[k] - before[k] for k in after}
            # the route: B = 3 takes the chain, one frame pair the single calls and their one-pair scratch (both directions too)
            assert (added["chains"], added["singles"]) == ((1, 0) if B >= 2 else (0, 1)), "B = %d: papof_batch_stats added %s" % (
                B, added)
            return out

        def check(got, what):
            names = ("flow_fw", "warpI2_fw", "flow_bw", "warpI2_bw")
            for name, g, w in zip(names, got, want):
                g = g.cpu().numpy()
                assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype)
                worst = float(np.abs(g - w).max())
                print("%s %s: max-abs %.3e against the oracle" % (what, name, worst))
                assert worst <= ORACLE_BOUND, "%s %s against the oracle: max-abs %.3e" % (what, name, worst)
            if fb:
                mask = fb_reference(got[0].cpu().numpy(), got[2].cpu().numpy())
                assert 0 < mask.sum() < mask.size
                assert np.array_equal(got[4].cpu().numpy().astype(np.uint8), mask), what + " occlusion"
        return Built(inputs, run, want, check)
    return build


def _flow_rows():
    names = {(False, False): "papof_flow_batch_tensor", (False, True): "papof_flow_batch_tensor_init",
             (True, False): "papof_flow_batch_tensor_fb", (True, True): "papof_flow_batch_tensor_fb_init"}
    rows = []
    for (fb, init), entry in names.items():
        for B in (3, 1):
            fn = "flow_video_fb" if fb else "flow_video"
            rows.append(Row("%s%s B=%d" % (fn, " init" if init else "", B), fn, (entry,),
                            "none: every pixel of every pair is solved; the warp clamps at the border", _flow(B, fb, init)))
    return rows


S = _seam_row
ROWS = [
    S("interpolate-gather", ["papof_interp_tensor"], "pixels whose both sources are occluded or leave the image"),
    S("interpolate-splat", ["papof_interp_splat_tensor"], "pixels nothing is splatted to (weights 0): the gather rule's fill"),
    S("splat", ["papof_splat_tensor"], "pixels without coverage take the fill; NaN and negative weights deposit nothing",
      lambda w: (w[1] == 0).any()),
    S("fb_consistency", ["papof_fb_check_tensor"], "pixels whose flow is not finite or leaves the image: occluded",
      lambda w: 0 < w[0].sum() < w[0].size),
    S("warp_affine", ["papof_warp_affine_tensor"], "a matrix with a NaN and one far outside: whole frames invalid",
      lambda w: (w[1].reshape(len(w[1]), -1).max(1) == 0).sum() == 2),
    S("fill_holes", ["papof_fill_holes_tensor"], "pixels outside the mask are copied"),
    S("dilate_masks", ["papof_mask_dilate_tensor"], "tiles without a masked pixel"),
    S("temporal_filter", ["papof_temporal_filter_tensor"], "the end frames' absent neighbours; chains that die: support 0",
      lambda w: (w[1] == 0).any()),
    S("motion_blur", ["papof_motion_blur_tensor"], "samples beyond the video's ends and occluded ones"),
    S("propagate", ["papof_propagate_tensor"], "hole pixels that no chain reaches: status 2; pixels outside the holes are "
      "copied: status 0", lambda w: all((w[1] == k).any() for k in (0, 1, 2))),
    S("detect_defects", ["papof_defect_detect_tensor"], "pixels without support on a side: score 0, no defect",
      lambda w: (w[2] == 0).any() and (w[1] == 0).any()),
    S("deinterlace-bob", ["papof_deinterlace_tensor"], "the first and last rows, which have one neighbour"),
    S("deinterlace-flows", ["papof_deinterlace_tensor"], "the end fields (no pair) and pixels whose flows are not finite: "
      "confidence 0", lambda w: (w[1] == 0).any()),
    S("super_resolve", ["papof_super_resolve_tensor"], "none in the outputs (every high-resolution pixel of a 2 x 65 frame is "
      "covered, by 0.25 at the least); samples whose flows are not finite or leave the frame deposit nothing in the workspace"),
    S("warp_homography", ["papof_warp_projective_tensor"], "points behind the camera and outside the frame: invalid",
      lambda w: (w[1] == 0).any()),
    S("mesh_motion", ["papof_mesh_motion_tensor"], "a vertex with too little support", lambda w: (w[1] < 4).any()),
    S("warp_mesh", ["papof_warp_mesh_tensor"], "a NaN mesh entry (its cell invalid), a row pushed out of the frame",
      lambda w: (w[1] == 0).any()),
    S("refine_flow", ["papof_refine_flow_tensor"], "pixels outside `where` are copied; windows that are all occluded"),
    S("decimate", ["papof_decimate_tensor"], "the ragged last row and column of blocks"),
    S("upsample_flow", ["papof_upsample_flow_tensor", "papof_decimate_tensor"], "windows whose taps are all NaN or occluded"),
    S("match_pairs-flat", ["papof_match_tensor"], "cells whose window leaves the frame"),
    S("match_pairs-hierarchical", ["papof_match_hier_tensor"], "cells whose window leaves the frame, on both levels"),
    S("match_pairs-recentred", ["papof_match_recentre_tensor"], "cells whose re-centred window leaves the frame"),
    S("match_init", ["papof_match_densify_tensor", "papof_fill_holes_tensor"], "unreliable cells: holes, filled",
      lambda w: (w[2] == 0).any(), derived=(2,)),
    S("mosaic", ["papof_mosaic_tensor"], "canvas pixels without a live source: 0 and count 0; empty slots",
      lambda w: (w[1] == 0).any()),
    S("mosaic-feather-gains", ["papof_mosaic_blend_tensor"], "canvas pixels without a live source; empty slots",
      lambda w: (w[1] == 0).any()),
    S("mosaic_homography", ["papof_mosaic_projective_tensor"], "canvas pixels without a live source; empty slots",
      lambda w: (w[1] == 0).any()),
    S("mosaic_overlap", ["papof_mosaic_overlap_tensor"], "pairs of slots that never overlap: sums and counts 0",
      lambda w: (w[1] == 0).any()),
    Row("global_motion", "global_motion", ("papof_motion_fit_tensor",), "a fully masked item and one whose flow is NaN "
        "everywhere: the identity, ok False, support 0", _fit("affine")),
    Row("global_homography", "global_homography", ("papof_homography_fit_tensor",), "a fully masked item and one whose flow is "
        "NaN everywhere: the identity, ok False, support 0", _fit("homography")),
    Row("bundle_sums", "bundle_sums", ("papof_bundle_sums_tensor",), "a fully masked link and one whose flow is NaN "
        "everywhere: no valid sample, sums of zero", _bundle_sums),
    Row("rectify_frames", "rectify_frames", ("papof_rs_rectify_tensor",), "rows whose guards fail, iterates that leave the image",
        _rectify_frames(False)),
    Row("rectify_frames-matrices", "rectify_frames", ("papof_rs_rectify_tensor",), "as rectify_frames, and points the matrices "
        "send outside", _rectify_frames(True)),
    Row("rectify_flows", "rectify_flows", ("papof_rs_flow_tensor",), "flows that are not finite or fail a guard: NaN",
        _rectify_flows),
    Row("warp_rows", "warp_rows", ("papof_warp_rows_tensor",), "a NaN knot and rows whose points leave the frame: invalid",
        _warp_rows),
    Row("deblur", "deblur", ("papof_deblur_tensor",), "the end frames' absent slots, chains that die, pixels left unchanged",
        _deblur),
    Row("field_metrics", "field_metrics", ("papof_field_metrics_tensor",), "the end fields have no neighbours: zero counts",
        _field_metrics),
    Row("weave_fields", "weave_fields", ("papof_weave_fields_tensor",), "none: every row is a copy of a field's row",
        _weave_fields),
    Row("shot_histograms", "shot_histograms", ("papof_cell_hist_tensor",), "bins that no pixel of a cell falls into",
        _shot_histograms),
    Row("ycc_to_rgb-fast", "ycc_to_rgb", ("papof_ycc_to_rgb_tensor",), "none: every pixel is converted; the ragged last group "
        "of four columns", _ycc_to_rgb(260, 1, np.uint8)),
    Row("ycc_to_rgb-lanes", "ycc_to_rgb", ("papof_ycc_to_rgb_tensor",), "none: every pixel is converted", _ycc_to_rgb(262, 0,
                                                                                                                 np.float32)),
    Row("rgb_to_ycc", "rgb_to_ycc", ("papof_rgb_to_ycc_tensor",), "NaN and infinite samples; the clamped last chroma row",
        _rgb_to_ycc),
    Row("ycc16_to_rgb-fast", "ycc16_to_rgb", ("papof_ycc16_to_rgb_tensor",), "none: every pixel is converted",
        _ycc16_to_rgb(260, 1, np.uint8)),
    Row("ycc16_to_rgb-lanes", "ycc16_to_rgb", ("papof_ycc16_to_rgb_tensor",), "none: every pixel is converted",
        _ycc16_to_rgb(262, 0, np.float32)),
    Row("rgb_to_ycc16", "rgb_to_ycc16", ("papof_rgb_to_ycc16_tensor",), "NaN and infinite samples; the clamped last chroma row",
        _rgb_to_ycc16),
    Row("temporal_consistency", "temporal_consistency", ("papof_temporal_consistency_tensor",), "pixels whose warp from the "
        "previous frame is occluded or leaves the image: the processed frame kept", _temporal_consistency),
    Row("mosaic_mesh", "mosaic_mesh", ("papof_mosaic_mesh_tensor",), "canvas pixels without a live source; a NaN table",
        _mosaic_mesh),
    Row("mosaic_rays", "mosaic_rays", ("papof_mosaic_ray_tensor",), "columns whose rays point behind the camera or are NaN",
        _mosaic3("rays")),
    Row("mosaic_overlap_rays", "mosaic_overlap_rays", ("papof_mosaic_overlap_ray_tensor",), "an empty slot: its row and column "
        "of sums and counts stay 0", _mosaic3("overlap-rays")),
    Row("mosaic_overlap_homography", "mosaic_overlap_homography", ("papof_mosaic_overlap_projective_tensor",), "an empty slot: "
        "its row and column of sums and counts stay 0", _mosaic3("overlap-homography")),
    Row("match_densify", "_densify", ("papof_match_densify_tensor",), "unreliable cells: +0.0 flow and a hole", _match_densify),
    Row("track_points-sparse", "track_points", ("papof_track_tensor",), "refused queries: NaN tracks, never visible",
        _track_points(True)),
    Row("track_points-dense", "track_points", ("papof_track_tensor",), "points whose flow is not finite: lost from there on",
        _track_points(False)),
] + _flow_rows()
del S

BY_NAME = {r.name: r for r in ROWS}


@functools.lru_cache(maxsize=None)
def built(name):
    """the row's inputs, call and expected outputs, computed once per process and left unchanged"""
    return BY_NAME[name].build()
