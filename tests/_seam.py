"""Inputs that make the seams of the split launches visible, and the oracle for them (tests/test_gpu_split_launches.py,
tests/test_seam_cpu.py).

The device-tensor kernels are launched through splitters that cut the work at the grid's bounds and hand each launch the index
at which it starts: launch_tiles (csrc/grid.h) at 65535 items along gridDim.y, fb_check (csrc/kernels.hip) at 32767 pairs
with shifted data pointers, launch_track (csrc/track.hip) at 65535 rows of tiles.  A second launch that forgets its start index
in one operand computes item 0's result for the first item beyond the cut.  To see that, the first item of a second launch
must differ from item 0 in every operand, and every one of the N items must be checked.

The numpy restatements loop over the items in Python, so N = 65537 items are laid out periodically: item i is item i mod P of
P distinct items, materialised on the device by an index gather (a stride-0 view would hide a missing start index: every item
would be the same memory).  65535 mod 7 = 1 and 32767 mod 5 = 2, so P = 7 for launch_tiles and P = 5 for fb_check.

- Kernels whose items are independent: the output of item i is the restatement's output of item i mod P.
- Temporal kernels read the frames t - r .. t + r of a video: on a periodic video the output is periodic away from the ends,
  so frame t is frame `period + t mod period` of the restatement run on 3 periods; the first and last r + 1 frames are those
  of the restatement run on the first and last 2 r + 2 frames (temporal_bank).  tests/test_seam_cpu.py checks both claims
  against the full restatement for every temporal case.
- The dense tracker's restatement is vectorised over the points and is run in full.
- The fits and the bundle sums add in another order than their restatements: the project pins them within a bound, not to
  the bytes, and states them bitwise reproducible and the same alone and in a batch.  Their first P items are held to that
  bound, and every item to the BYTES of its base item in the same call (periodic_in_call).

CASES is the table: one row per entry point with the tensors.py function, the split it crosses, the count that crosses it,
the frame size, whether the public wrapper or the C entry is called, and the builder of its inputs, reference and call."""
import collections

import numpy as np

P = 7                    # the period of the items of a launch_tiles case
P_FB = 5                 # ... of an fb_check case
TILES_CUT = 65535        # launch_tiles: kMaxFrames (gridDim.y)
FB_CUT = 32767           # fb_check: pairs per launch
TRACK_CUT = 4 * 65535    # launch_track, dense: rows of pixels per launch (65535 rows of 64 x 4 tiles)
N_TILES = TILES_CUT + 2  # the second launch has blockIdx.y 0 and 1
N_FB = FB_CUT + 2
H_TRACK = TRACK_CUT + 5

CONSISTENCY = (0.01, 0.5)

Case = collections.namedtuple("Case", "name fn split count cut frame via oracle build")
# oracle: "periodic" (independent items), "temporal" (interior periodic, ends windowed), "full" (the whole restatement)
Built = collections.namedtuple("Built", "inputs ref run reach period gap tol", defaults=(0, P, 0, None))
# inputs: {name: (array with the items first, "item" | "pair")}; a "pair" input of a temporal case has `gap` items fewer
# ref: independent: () -> [outputs of the P items]; temporal: (start, count) -> [outputs of the frames start .. start + count)
# run: ({name: device tensor of the N items}) -> [device outputs, items first, laid out as ref's]
# tol: None (bytes), or for the entry points that the project pins to their restatement within a bound and not to the bytes a
#      function (got outputs, expected outputs, what, cut) that asserts that bound and periodic_in_call


def index(n, period=P, start=0):
    """the base item of each of the n items start, start + 1, ...: (start + i) mod period"""
    return (start + np.arange(n, dtype=np.int64)) % period


def _torch():
    import torch
    return torch


def gather(items, idx):
    """items[idx] materialised on the device: every item has memory of its own"""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(items)).cuda()
    out = t.index_select(0, torch.from_numpy(np.asarray(idx, np.int64)).cuda())
    assert out.is_contiguous() and (out.dim() == 1 or out.stride(0) > 0)
    return out


def expand(want, idx):
    """the expected output of every item: the restatement's outputs `want` of the base items, gathered by idx"""
    return gather(want, idx)


def _bytes(t):
    torch = _torch()
    t = t.contiguous()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.view(torch.uint8).reshape(t.shape[0], -1)


def same_bytes(got, want, what, cut=None):
    """two device tensors with the items first, byte for byte over every item; names the first item that differs and says
    on which side of the cut the differing items lie"""
    torch = _torch()
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape),
                                                                              got.dtype, want.dtype)
    g, w = _bytes(got), _bytes(want)
    if torch.equal(g, w):
        return
    bad = (g != w).any(1).nonzero().reshape(-1)
    first, n = int(bad[0]), int(bad.numel())
    side = "" if cut is None else "; %d of them before the cut at %d" % (int((bad < cut).sum()), cut)
    raise AssertionError("%s: %d of %d items differ, the first is item %d%s" % (what, n, g.shape[0], first, side))


def periodic_in_call(got, period, what, cut=None):
    """every item of every output has the BYTES of its base item in the same call -- for the outputs that the project pins
    to their restatement within a bound (sums added in another order) and states to be bitwise reproducible and the same
    alone and in a batch: with the first `period` items within the bound, every item is"""
    for k, g in enumerate(got):
        idx = _torch().from_numpy(index(g.shape[0], period)).cuda()
        same_bytes(g, g[:period].index_select(0, idx), "%s output %d, item i against item i mod %d" % (what, k, period), cut)


def temporal_bank(ref, n, reach, period=P):
    """The expected outputs of a temporal kernel on a periodic video of n frames, as (bank, idx): frame t is row idx[t] of
    every array of bank.  The first and last reach + 1 frames come from the restatement run on the first and last
    2 reach + 2 frames, the others from the restatement run on 3 periods, read in the middle one."""
    r = reach
    assert n >= 2 * r + 2 and period > r
    head = ref(0, 2 * r + 2)
    mid = ref(0, 3 * period)
    tail = ref(n - 2 * r - 2, 2 * r + 2)
    bank = [np.concatenate([h[:r + 1], m[period:2 * period], t[-(r + 1):]]) for h, m, t in zip(head, mid, tail)]
    t = np.arange(n, dtype=np.int64)
    idx = np.where(t <= r, t, np.where(t >= n - r - 1, (r + 1) + period + (t - (n - r - 1)), (r + 1) + t % period))
    return bank, idx


# ---- generators: those of the GPU tests of each entry point

def frames(n, H, W, C, seed, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, H, W, C)).astype(np.uint8)
    return rng.random((n, H, W, C)).astype(dtype)


def flows(n, H, W, seed, dtype=np.float32):
    """n flow pairs with NaNs, infinities and displacements that leave the image (test_gpu_track._fields)"""
    from test_gpu_track import _fields
    fw, bw = _fields(n + 1, H, W, seed)
    return fw.astype(dtype), bw.astype(dtype)


def occlusion(n, H, W, seed):
    """a random (n, 2, H, W) mask with an all-occluded block in both channels"""
    rng = np.random.default_rng(seed)
    m = (rng.random((n, 2, H, W)) < 0.3).astype(np.uint8)
    m[:, :, H // 3:H // 3 + 2, W // 4:W // 4 + 9] = 1
    return m


def holes(n, H, W, seed):
    return np.random.default_rng(seed).random((n, H, W)) < 0.35


def matrices(n, H, W, seed):
    """small rotations, scales and shifts about the centre, one far outside the image, one with a NaN
    (test_gpu_stab._matrices)"""
    from test_gpu_stab import _matrices
    return _matrices(n, H, W, seed)


# ---- independent items

def _interpolate(method):
    def build():
        from _interp_ref import interp_reference
        from _splat_ref import interp_splat_reference
        from papteam_opticalflow_amd import tensors
        H, W, C = 5, 66, 2
        a, b = frames(P, H, W, C, 1), frames(P, H, W, C, 2)
        fw, bw = flows(P, H, W, 3)
        occ = occlusion(P, H, W, 4)
        times = [0.25, 0.5]
        rng = np.random.default_rng(5)
        w0, w1 = (rng.random((P, H, W)) * 1.3 for _ in range(2))
        w0[:, 1:3, 10:30] = 0.0  # a region nothing is splatted from: the gather rule and its mask decide there
        w1[:, 2:4, 5:35] = 0.0
        inputs = {"a": (a, "item"), "b": (b, "item"), "fw": (fw, "item"), "bw": (bw, "item"), "occ": (occ, "item")}
        if method == "splat":
            inputs.update(w0=(w0, "item"), w1=(w1, "item"))

        def ref():
            if method == "gather":
                return [interp_reference(a, b, fw, bw, times, occ, np.uint8)]
            return [interp_splat_reference(a, b, fw, bw, times, (w0, w1), occ, np.uint8)]

        def run(d):
            weights = (d["w0"], d["w1"]) if method == "splat" else None
            return [tensors.interpolate(d["a"], d["b"], d["fw"], d["bw"], times, occlusion=d["occ"], layout="NHWC",
                                        method=method, weights=weights)]
        return Built(inputs, ref, run)
    return build


def _splat():
    from _splat_ref import splat_reference
    from papteam_opticalflow_amd import tensors
    H, W, C = 5, 66, 1
    x = frames(P, H, W, C, 6)
    fw, _ = flows(P, H, W, 8)
    rng = np.random.default_rng(7)
    w = rng.random((P, H, W)) * 1.3  # weights in (0, 1.3) with zeros, negatives, NaNs and infinities (test_gpu_splat._weights)
    for val in (0.0, -0.5, np.nan, np.inf):
        w[tuple(rng.integers(0, s, max(1, w.size // 300)) for s in (P, H, W))] = val
    inputs = {"x": (x, "item"), "fw": (fw, "item"), "w": (w, "item")}

    def ref():
        return list(splat_reference(x, fw, [0.5], w, fill=0.5, out_dtype=np.uint8))

    def run(d):
        s = tensors.splat(d["x"], d["fw"], [0.5], weight=d["w"], fill=0.5, layout="NHWC")
        return [s.out, s.coverage]
    return Built(inputs, ref, run)


def _splat_weights():
    """torch operations, no kernel of the project's and no split: only the wrapper's handling of N.  The device's exp is not
    numpy's to the bit: the argument -alpha * err <= 11 in magnitude carries a relative rounding error of a few 2^-53 from
    the mean over the channels, so exp's relative error is below 11 * 4 * 2^-53 + 2 ulp < 1e-14; 1e-13 is asserted, and
    every item must have the BYTES of its base item in the same call."""
    from _splat_ref import photometric_weights
    from papteam_opticalflow_amd import tensors
    H, W, C = 5, 66, 2
    x, other = frames(P, H, W, C, 16), frames(P, H, W, C, 17)
    inputs = {"x": (x, "item"), "other": (other, "item")}

    def ref():
        return [photometric_weights(x, other, tensors.ALPHA)]

    def run(d):
        return [tensors.splat_weights(d["x"], d["other"], layout="NHWC")]

    def tol(got, want, what, cut):
        assert _torch().allclose(got[0], want[0], rtol=1e-13, atol=0.0), what
        periodic_in_call(got, P, what, cut)
    return Built(inputs, ref, run, tol=tol)


def _fb_consistency():
    from test_fb_cpu import fb_reference
    from papteam_opticalflow_amd import tensors
    H, W = 5, 66
    fw, bw = flows(P_FB, H, W, 9)
    inputs = {"fw": (fw, "item"), "bw": (bw, "item")}

    def ref():
        return [fb_reference(fw, bw)]

    def run(d):
        return [tensors.fb_consistency(d["fw"], d["bw"]).view(_torch().uint8)]
    return Built(inputs, ref, run, period=P_FB)


def _warp_affine():
    from _stab_ref import warp_reference
    from papteam_opticalflow_amd import tensors
    H, W, C = 5, 66, 2
    f = frames(P, H, W, C, 10)
    M = matrices(P, H, W, 11)
    M[[1, 3]] = M[[3, 1]]  # item 1, the first of the second launch, lands in the image
    inputs = {"f": (f, "item"), "M": (M, "item")}

    def ref():
        out, valid = warp_reference(f, M, np.uint8)
        return [out, valid.astype(np.uint8)]

    def run(d):
        out, valid = tensors.warp_affine(d["f"], d["M"], layout="NHWC")
        return [out, valid.view(_torch().uint8)]
    return Built(inputs, ref, run)


def _fill_holes():
    from _inpaint_ref import fill_reference
    from papteam_opticalflow_amd import tensors
    H, W, C = 5, 66, 1
    x = frames(P, H, W, C, 12)
    m = holes(P, H, W, 13)
    inputs = {"x": (x, "item"), "m": (m, "item")}

    def ref():
        return [fill_reference(x, m, 1, np.uint8)]

    def run(d):
        return [tensors.fill_holes(d["x"], d["m"], layout="NHWC", relax=1)]
    return Built(inputs, ref, run)


def _dilate_masks():
    from _restore_ref import dilate_reference
    from papteam_opticalflow_amd import tensors
    H, W = 17, 66  # 64 x 16 tiles
    m = np.random.default_rng(14).random((P, H, W)) < 0.03
    inputs = {"m": (m, "item")}

    def ref():
        return [np.asarray(dilate_reference(m, 2), np.uint8)]

    def run(d):
        return [tensors.dilate_masks(d["m"], 2).view(_torch().uint8)]
    return Built(inputs, ref, run)


# ---- temporal kernels

def _video_case(H, W, C, seed, n_pairs=P):
    f = frames(P, H, W, C, seed)
    fw, bw = flows(n_pairs, H, W, seed + 1)
    return f, fw, bw


def _temporal_filter():
    from _denoise_ref import denoise_reference
    from papteam_opticalflow_amd import tensors
    f, fw, bw = _video_case(5, 66, 2, 20)
    inputs = {"f": (f, "item"), "fw": (fw, "pair"), "bw": (bw, "pair")}

    def ref(start, count):
        fr, pr = index(count, P, start), index(count - 1, P, start)
        return list(denoise_reference(f[fr], fw[pr], bw[pr], 2, 0.15, CONSISTENCY, np.uint8))

    def run(d):
        got = tensors.temporal_filter(d["f"], d["fw"], d["bw"], radius=2, layout="NHWC")
        return [got.video, got.support]
    return Built(inputs, ref, run, reach=2, gap=1)


def _motion_blur():
    from _blur_ref import blur_reference
    from papteam_opticalflow_amd import tensors
    f, fw, bw = _video_case(5, 66, 2, 22)
    occ = occlusion(P, 5, 66, 24)
    schedule = tensors.blur_schedule(1.0, 4, -0.5, "triangle")  # samples before and after the frame
    inputs = {"f": (f, "item"), "fw": (fw, "pair"), "bw": (bw, "pair"), "occ": (occ, "pair")}

    def ref(start, count):
        fr, pr = index(count, P, start), index(count - 1, P, start)
        return [blur_reference(f[fr], fw[pr], bw[pr], *schedule, occ[pr], np.uint8)]

    def run(d):
        return [tensors.motion_blur(d["f"], d["fw"], d["bw"], shutter=1.0, samples=4, phase=-0.5, shape="triangle",
                                    occlusion=d["occ"], layout="NHWC")]
    return Built(inputs, ref, run, reach=1, gap=1)


def _propagate():
    from _inpaint_ref import propagate_reference
    from papteam_opticalflow_amd import tensors
    f, fw, bw = _video_case(5, 66, 2, 25)
    m = holes(P, 5, 66, 27)
    inputs = {"f": (f, "item"), "m": (m, "item"), "fw": (fw, "pair"), "bw": (bw, "pair")}

    def ref(start, count):
        fr, pr = index(count, P, start), index(count - 1, P, start)
        return list(propagate_reference(f[fr], m[fr], fw[pr], bw[pr], 2, CONSISTENCY, np.uint8))

    def run(d):
        got = tensors.propagate(d["f"], d["m"], d["fw"], d["bw"], radius=2, consistency=CONSISTENCY, layout="NHWC")
        return [got.video, got.status]
    return Built(inputs, ref, run, reach=2, gap=1)


def _detect_defects():
    from _restore_ref import detect_reference
    from papteam_opticalflow_amd import tensors
    f, fw, bw = _video_case(5, 66, 2, 28)
    inputs = {"f": (f, "item"), "fw": (fw, "pair"), "bw": (bw, "pair")}

    def ref(start, count):
        fr, pr = index(count, P, start), index(count - 1, P, start)
        return list(detect_reference(f[fr], fw[pr], bw[pr], 0.3, CONSISTENCY))

    def run(d):
        got = tensors.detect_defects(d["f"], d["fw"], d["bw"], threshold=0.3, consistency=CONSISTENCY, layout="NHWC")
        return [got.mask.view(_torch().uint8), got.score, got.support]
    # an interior frame reads t - 1 and t + 1, the end frames two frames on one side
    return Built(inputs, ref, run, reach=2, gap=1)


def _deinterlace(mode):
    def build():
        from _deinterlace_ref import deinterlace_reference
        from papteam_opticalflow_amd import tensors
        f, fw, bw = _video_case(5, 66, 2, 30 + mode)
        inputs = {"f": (f, "item")}
        if mode:
            inputs.update(fw=(fw, "pair"), bw=(bw, "pair"))

        def ref(start, count):
            fr, pr = index(count, P, start), index(count - 2, P, start)
            # field k holds the rows of parity (k + first) & 1: a window that starts at an odd field starts on the other parity
            got = deinterlace_reference(f[fr], fw[pr], bw[pr], first=start & 1, mode=mode, sigma=0.05)
            return list(got) if mode else [got[0]]

        def run(d):
            if not mode:
                return [tensors.bob_fields(d["f"], 0, layout="NHWC")]
            got = tensors.deinterlace_fields(d["f"], d["fw"], d["bw"], 0, sigma=0.05, layout="NHWC")
            return [got.video, got.confidence]
        # field t reads the fields t - 1 and t + 1 through pair t - 1, the end fields pair 1 and pair T - 4; the parity of a
        # field's rows alternates, so the output's period is 2 P
        return Built(inputs, ref, run, reach=3, period=2 * P, gap=2)
    return build


# ---- the dense tracker: the restatement in full

def _track_dense():
    from test_gpu_track import _fields
    from test_track_cpu import track_reference
    from papteam_opticalflow_amd import tensors
    T, H, W = 3, H_TRACK, 2
    fw, bw = _fields(T, H, W, 40)
    rng = np.random.default_rng(41)
    for f in (fw, bw):  # the vertical flows of rows apart differ: no row of the second launch has the first launch's values
        f[:, 1] += rng.normal(0, 0.3, f[:, 1].shape)
    inputs = {"fw": (fw, "full"), "bw": (bw, "full")}

    def ref():
        tracks, vis = track_reference(fw, bw)
        # points first: (N, T, 2) and (N, T)
        return [np.ascontiguousarray(tracks.transpose(1, 0, 2)), np.ascontiguousarray(vis.T.astype(np.uint8))]

    def run(d):
        got = tensors.track_points(d["fw"], d["bw"])
        return [got.tracks.permute(1, 0, 2), got.visible.view(_torch().uint8).t()]
    return Built(inputs, ref, run)


# ---- fits: within the project's bound of the restatement, and every item the bytes of its base item

def _fit(kind):
    def build():
        import collections as c
        from papteam_opticalflow_amd import tensors
        H, W = 9, 66  # two blocks across; 64 x 32 pixels per block: a second row of blocks would take over 1 GB of flows
        if kind == "affine":
            import test_gpu_stab as t
            f = t._affine_flows(P, H, W, 50).astype(np.float32)
        else:
            import test_gpu_homography as t
            f = t._wild_flows(P, H, W, 51).astype(np.float32)
        occ = t._mask(P, H, W, 52)
        inputs = {"f": (f, "item"), "occ": (occ, "item")}
        Got = c.namedtuple("Got", "motion ok support")

        def ref():  # the bound is asserted by tol, on the first P items
            return []

        def run(d):
            if kind == "affine":
                got = tensors.global_motion(d["f"], occlusion=d["occ"], model="affine", iters=3, scale=1.5)
            else:
                got = tensors.global_homography(d["f"], occlusion=d["occ"], iters=3, scale=1.5)
            return [got.motion, got.ok.view(_torch().uint8), got.support]

        def tol(got, want, what, cut):
            first = Got(got[0][:P], got[1][:P].bool(), got[2][:P])
            if kind == "affine":
                t._check_fit(first, f, occ, t.AFFINE, 3, what, 1.5)  # corners within 1e-8 px, ok equal, support within 1e-12
            else:
                t._check_fit(first, f, occ, 3, what, 1.5)
            periodic_in_call(got, P, what, cut)
        return Built(inputs, ref, run, tol=tol)
    return build


def _bundle_sums():
    import test_gpu_bundle as t
    from papteam_opticalflow_amd import tensors
    H, W, f = 9, 66, 60.0  # two blocks across; 64 x 32 samples per block: a second row of blocks would take over 1 GB
    fl, Rij = t._links(P, H, W, f, seed=53)
    fl = fl.astype(np.float32)
    occ = (np.random.default_rng(54).uniform(size=(P, 2, H, W)) < 0.2).astype(np.uint8)
    inputs = {"fl": (fl, "item"), "R": (Rij, "item"), "occ": (occ, "item")}

    def ref():
        return []

    def run(d):
        return [tensors.bundle_sums(d["fl"], d["R"], f, occlusion=d["occ"], scale=1.5)]

    def tol(got, want, what, cut):
        t._check(got[0][:P], fl, Rij, f, occ, 1, 1.5, what)  # within (n - 1) 2^-53 of the sums of the terms' magnitudes
        periodic_in_call(got, P, what, cut)
    return Built(inputs, ref, run, tol=tol)


# ---- more independent items

def _warp_homography():
    from _homography_ref import warp_reference_h
    from test_gpu_homography import _homographies
    from papteam_opticalflow_amd import tensors
    H, W, C = 5, 66, 2
    f = frames(P, H, W, C, 55)
    M = _homographies(P, H, W, 56)
    M[[1, 4]] = M[[4, 1]]  # item 1, the first of the second launch, is a mild perspective that stays in the image
    inputs = {"f": (f, "item"), "M": (M, "item")}

    def ref():
        out, valid = warp_reference_h(f, M, np.uint8)
        return [out, valid.astype(np.uint8)]

    def run(d):
        out, valid = tensors.warp_homography(d["f"], d["M"], layout="NHWC")
        return [out, valid.view(_torch().uint8)]
    return Built(inputs, ref, run)


def _mesh_motion():
    from _mesh_ref import mesh_motion_reference
    from test_gpu_mesh import _flows
    from papteam_opticalflow_amd import tensors
    H, W, grid = 9, 34, (2, 3)
    f, A, occ = _flows(P, H, W, 57)
    f = f.astype(np.float32)
    inputs = {"f": (f, "item"), "A": (A, "item"), "occ": (occ, "item")}

    def ref():
        vert, sup, res = mesh_motion_reference(f, A, occ, grid, 4, True)
        return [vert, np.asarray(sup, np.int32), res]

    def run(d):
        got = tensors.mesh_motion(d["f"], motion=d["A"], occlusion=d["occ"], grid=grid, min_support=4, spatial=True)
        return [got.vertices, got.support, got.residuals]
    return Built(inputs, ref, run)


def _warp_mesh():
    from _mesh_ref import warp_mesh_reference
    from papteam_opticalflow_amd import tensors
    H, W, C, grid = 5, 66, 2, (2, 3)
    f = frames(P, H, W, C, 58)
    M = matrices(P, H, W, 59)
    M[[1, 3]] = M[[3, 1]]
    rng = np.random.default_rng(60)
    D = rng.normal(0, 1.5, (P, grid[0] + 1, grid[1] + 1, 2))
    D[0, 0, :, 1] -= 6.0    # the top row of item 0 pushes samples out of the frame
    D[2, -1, -1] = np.nan   # one NaN entry: its cell is not valid
    inputs = {"f": (f, "item"), "M": (M, "item"), "D": (D, "item")}

    def ref():
        out, valid = warp_mesh_reference(f, M, D, np.uint8)
        return [out, valid.astype(np.uint8)]

    def run(d):
        out, valid = tensors.warp_mesh(d["f"], d["M"], d["D"], layout="NHWC")
        return [out, valid.view(_torch().uint8)]
    return Built(inputs, ref, run)


def _guides(H, W, C, seed):
    """two flat regions split by a slanted edge, a wave and a little noise, uint8 (test_gpu_refine._guide)"""
    from test_gpu_refine import _guide
    return _guide(P, H, W, C, _torch().uint8, seed)


def _refine_flow():
    from _refine_ref import refine_reference
    from papteam_opticalflow_amd import tensors
    H, W, radius, sigma_s, sigma_c = 9, 34, 2, 1.5, 0.1  # 32 x 8 tiles
    g = _guides(H, W, 1, 61)
    fw, _ = flows(P, H, W, 62)
    rng = np.random.default_rng(63)
    occ, where = (rng.random((P, H, W)) < 0.2).astype(np.uint8), rng.random((P, H, W)) < 0.7
    inputs = {"fw": (fw, "item"), "g": (g, "item"), "occ": (occ, "item"), "where": (where, "item")}

    def ref():
        S, R = tensors.refine_tables(radius, sigma_s)
        return [refine_reference(fw, g, S, R, tensors.refine_q(sigma_c, 1, True), radius, occlusion=occ, where=where)]

    def run(d):
        return [tensors.refine_flow(d["fw"], d["g"], occlusion=d["occ"], where=d["where"], radius=radius, sigma_s=sigma_s,
                                    sigma_c=sigma_c, layout="NHWC")]
    return Built(inputs, ref, run)


def _decimate():
    from _upsample_ref import decimate_reference
    from papteam_opticalflow_amd import tensors
    g = _guides(9, 34, 2, 64)
    inputs = {"g": (g, "item")}

    def ref():
        return [decimate_reference(g, 2, np.float32)]

    def run(d):
        return [tensors.decimate(d["g"], 2, layout="NHWC", out_dtype=_torch().float32)]
    return Built(inputs, ref, run)


def _upsample_flow():
    from _upsample_ref import decimate_reference, upsample_reference
    from papteam_opticalflow_amd import tensors
    H, W, f, r = 9, 34, 2, 1  # 32 x 8 tiles of output pixels
    h, w = -(-H // f), -(-W // f)
    g = _guides(H, W, 1, 65)
    rng = np.random.default_rng(66)
    fl = rng.normal(0, 2, (P, 2, h, w)).astype(np.float32)
    fl[rng.random(fl.shape) < 0.08] = np.nan
    occ = rng.random((P, h, w)) < 0.2
    inputs = {"fl": (fl, "item"), "g": (g, "item"), "occ": (occ, "item")}

    def ref():
        S, R = tensors.upsample_tables(f, r, 0.7)
        return [upsample_reference(fl, g, decimate_reference(g, f), S, R, tensors.upsample_q(0.1, 1), f, r, occlusion=occ,
                                   out_dtype=np.float32)]

    def run(d):  # the low-resolution guide is the call's own decimate: both kernels cross the cut
        return [tensors.upsample_flow(d["fl"], d["g"], f, occlusion=d["occ"], radius=r, sigma_s=0.7, sigma_c=0.1,
                                      layout="NHWC")]
    return Built(inputs, ref, run)


def _textures(H, W, C, seed, shifts, pad=8):
    """a pair per shift: a texture and the same texture moved by the item's own shift, with a little noise
    (test_gpu_match._frames)"""
    from _match_ref import texture
    rng = np.random.default_rng(seed)
    a, b = [], []
    for sx, sy in shifts:
        t = texture(rng, H + 2 * pad, W + 2 * pad, C)
        a.append(t[pad:pad + H, pad:pad + W])
        b.append(t[pad - sy:pad - sy + H, pad - sx:pad - sx + W])
    a, b = np.stack(a), np.stack(b)
    return a, np.clip(b.astype(np.int64) + rng.integers(-2, 3, b.shape), 0, 255).astype(np.uint8)


_SHIFTS = [(1, 0), (-2, 1), (0, 2), (3, -1), (-1, -2), (2, 2), (-3, 0)]


def _match(kind):
    def build():
        from _hmatch_ref import hmatch_reference
        from _match_ref import match_reference
        from _recentre_ref import recentre_reference
        from papteam_opticalflow_amd import tensors
        f32 = _torch().float32
        if kind == "flat":      # 9 x 34 cells: 32 x 8 tiles cut both ways; forward only
            a, b = _textures(9, 34, 1, 67, _SHIFTS)
            kw, both = dict(stride=1, patch=1, search=3), False
            reference = match_reference
        elif kind == "hier":    # two levels: 10 x 36 and 5 x 18 cells; forward only
            a, b = _textures(10, 36, 1, 68, _SHIFTS)
            kw, both = dict(stride=1, levels=2, patch=1, search=2, refine=1), False
            reference = hmatch_reference
        else:                   # re-centred, both directions: 2 N items in three launches; levels of stride 4, 8 and 16: the
            a, b = _textures(16, 16, 1, 69, [(4 * x, 4 * y) for x, y in _SHIFTS], pad=16)  # two wide decimations cross too
            kw, both = dict(stride=4, levels=3, patch=1, search=2, refine=1), True
            reference = lambda A, B, **k: recentre_reference(A, B, window=2, **k)  # noqa: E731
        inputs = {"a": (a, "item"), "b": (b, "item")}

        def ref():
            out = list(reference(a, b, out_dtype=np.float32, **kw))
            return out + list(reference(b, a, out_dtype=np.float32, **kw)) if both else out

        def run(d):
            extra = dict(recentre=2) if kind == "recentre" else {}
            m = tensors.match_pairs(d["a"], d["b"], both=both, layout="NHWC", out_dtype=f32, **kw, **extra)
            return [m.disp_fw, m.cost_fw, m.disp_bw, m.cost_bw] if both else [m.disp_fw, m.cost_fw]
        return Built(inputs, ref, run)
    return build


def _match_init():
    """k_match_densify (the pass that papof_match_densify_tensor launches) of both directions of N pairs, and the one
    fill_holes chain over their 2 N fields"""
    from _inpaint_ref import fill_reference
    from _match_ref import densify_reference, match_reference
    from papteam_opticalflow_amd import tensors
    H, W, stride = 8, 8, 2
    a, b = _textures(H, W, 1, 70, _SHIFTS)
    kw = dict(stride=stride, patch=1, search=2)
    dfw, cfw = match_reference(a, b, out_dtype=np.float32, **kw)
    dbw, cbw = match_reference(b, a, out_dtype=np.float32, **kw)
    inputs = {"dfw": (dfw, "item"), "dbw": (dbw, "item"), "cfw": (cfw, "item"), "cbw": (cbw, "item")}
    max_cost = float(np.median(cfw))

    def ref():
        fw, hole_fw = densify_reference(dfw, dbw, cfw, (H, W), stride, 1, max_cost)
        bw, hole_bw = densify_reference(dbw, dfw, cbw, (H, W), stride, 1, max_cost)
        fill = lambda f, m: np.moveaxis(fill_reference(np.moveaxis(f, 1, -1), m, tensors.RELAX), -1, 1)  # noqa: E731
        reliable = np.stack([hole_fw == 0, hole_bw == 0], 1).astype(np.uint8)
        return [np.ascontiguousarray(fill(fw, hole_fw)), np.ascontiguousarray(fill(bw, hole_bw)), reliable]

    def run(d):
        got = tensors.match_init(d["dfw"], d["dbw"], d["cfw"], d["cbw"], (H, W), tol=1, max_cost=max_cost)
        return [got.init_fw, got.init_bw, got.reliable.contiguous().view(_torch().uint8)]
    return Built(inputs, ref, run)


def _mosaic(what):
    def build():
        from _blend_ref import blend_reference, overlap_reference
        from _homography_ref import mosaic_reference_h
        from _mosaic_ref import mosaic_reference
        from test_gpu_mosaic import _frame_masks, _mats
        from papteam_opticalflow_amd import tensors
        T, H, W, C, Hc, Wc, N = 4, 9, 13, 2, 5, 66, 2  # n_out mosaics of two sources each on a 5 x 66 canvas
        rng = np.random.default_rng(71)
        f = frames(T, H, W, C, 72)
        M = _mats(rng, P, N, H, W, Hc, Wc)  # source 0 of every item is live at every pixel of the canvas
        src = np.array([[0, 1], [2, 3], [1, 1], [3, -1], [2, 0], [1, 2], [3, 0]])
        masks = _frame_masks(rng, T, H, W)
        inputs = {"f": (f, "full"), "masks": (masks, "full"), "M": (M, "item"), "src": (src, "item")}

        if what == "feather":    # papof_mosaic_blend_tensor: a gain per source
            gains = rng.uniform(0.5, 1.5, (P, N))
            inputs["gains"] = (gains, "item")
        if what == "homography":  # papof_mosaic_projective_tensor: the affine maps with a mild perspective
            M3 = np.zeros((P, N, 3, 3))
            M3[..., :2, :], M3[..., 2, 2] = M, 1.0
            M3[..., 2, :2] = rng.normal(0, 1e-3, (P, N, 2))
            inputs["M"] = (M3, "item")

        def ref():
            if what == "mosaic":
                return list(mosaic_reference(f, src, M, (Hc, Wc), "median", masks, np.uint8))
            if what == "feather":
                return list(blend_reference(f, src, M, (Hc, Wc), "feather", gains, masks, np.uint8))
            if what == "homography":
                return list(mosaic_reference_h(f, src, M3, (Hc, Wc), "mean", None, masks, np.uint8))
            return list(overlap_reference(f, src, M, (Hc, Wc), 2, 1.0, masks))

        def run(d):
            if what == "overlap":
                got = tensors.mosaic_overlap(d["f"], d["src"], d["M"], (Hc, Wc), masks=d["masks"], step=2, layout="NHWC")
                return [got.sums, got.counts]
            if what == "mosaic":
                got = tensors.mosaic(d["f"], d["src"], d["M"], (Hc, Wc), mode="median", masks=d["masks"], layout="NHWC")
            elif what == "feather":
                got = tensors.mosaic(d["f"], d["src"], d["M"], (Hc, Wc), mode="feather", masks=d["masks"], layout="NHWC",
                                     gains=d["gains"])
            else:
                got = tensors.mosaic_homography(d["f"], d["src"], d["M"], (Hc, Wc), mode="mean", masks=d["masks"],
                                                layout="NHWC")
            return [got.out, got.count]
        return Built(inputs, ref, run)
    return build


def _super_resolve():
    """N frames in one round of targets: the sources' launch, the resolve and the back-projection all cross the cut.  The
    fixed-point sums take 16.6 KB per frame of 2 x 65 at scale 2 (1.1 GB in all): the smallest frame with two tiles across"""
    from _superres_ref import superres_reference
    from papteam_opticalflow_amd import tensors
    H, W, C = 2, 65, 1
    f = frames(P, H, W, C, 73)
    fw, bw = flows(P, H, W, 74)
    inputs = {"f": (f, "item"), "fw": (fw, "pair"), "bw": (bw, "pair")}

    def ref(start, count):
        fr, pr = index(count, P, start), index(count - 1, P, start)
        return list(superres_reference(f[fr], fw[pr], bw[pr], 2, radius=1, sigma=0.15, consistency=CONSISTENCY, prior=0.05,
                                       iters=1, out_dtype=np.uint8))

    def run(d):
        got = tensors.super_resolve(d["f"], d["fw"], d["bw"], 2, radius=1, sigma=0.15, consistency=CONSISTENCY, prior=0.05,
                                    iters=1, layout="NHWC")
        return [got.video, got.coverage]
    return Built(inputs, ref, run, reach=1, gap=1)


TILES, FB, TRACK = "launch_tiles", "fb_check", "launch_track"

CASES = [
    Case("interpolate-gather", "interpolate", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _interpolate("gather")),
    Case("interpolate-splat", "interpolate", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _interpolate("splat")),
    Case("splat", "splat", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _splat),
    Case("splat_weights", "splat_weights", "none (torch operations)", N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic",
         _splat_weights),
    Case("fb_consistency", "fb_consistency", FB, N_FB, FB_CUT, (5, 66), "wrapper", "periodic", _fb_consistency),
    Case("warp_affine", "warp_affine", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _warp_affine),
    Case("fill_holes", "fill_holes", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _fill_holes),
    Case("dilate_masks", "dilate_masks", TILES, N_TILES, TILES_CUT, (17, 66), "wrapper", "periodic", _dilate_masks),
    Case("temporal_filter", "temporal_filter", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "temporal", _temporal_filter),
    Case("motion_blur", "motion_blur", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "temporal", _motion_blur),
    Case("propagate", "propagate", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "temporal", _propagate),
    Case("detect_defects", "detect_defects", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "temporal", _detect_defects),
    Case("deinterlace-bob", "bob_fields", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "temporal", _deinterlace(0)),
    Case("deinterlace-flows", "deinterlace_fields", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "temporal",
         _deinterlace(1)),
    Case("super_resolve", "super_resolve", TILES, N_TILES, TILES_CUT, (2, 65), "wrapper", "temporal", _super_resolve),
    Case("track_points-dense", "track_points", TRACK, H_TRACK, TRACK_CUT, (H_TRACK, 2), "wrapper", "full", _track_dense),
    Case("warp_homography", "warp_homography", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _warp_homography),
    Case("mesh_motion", "mesh_motion", TILES, N_TILES, TILES_CUT, (9, 34), "wrapper", "periodic", _mesh_motion),
    Case("warp_mesh", "warp_mesh", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _warp_mesh),
    Case("refine_flow", "refine_flow", TILES, N_TILES, TILES_CUT, (9, 34), "wrapper", "periodic", _refine_flow),
    Case("decimate", "decimate", TILES, N_TILES, TILES_CUT, (9, 34), "wrapper", "periodic", _decimate),
    Case("upsample_flow", "upsample_flow", TILES, N_TILES, TILES_CUT, (9, 34), "wrapper", "periodic", _upsample_flow),
    Case("match_pairs-flat", "match_pairs", TILES, N_TILES, TILES_CUT, (9, 34), "wrapper", "periodic", _match("flat")),
    Case("match_pairs-hierarchical", "match_pairs", TILES, N_TILES, TILES_CUT, (10, 36), "wrapper", "periodic",
         _match("hier")),
    Case("match_pairs-recentred", "match_pairs", TILES, N_TILES, TILES_CUT, (16, 16), "wrapper", "periodic",
         _match("recentre")),
    Case("match_init", "match_init", TILES, N_TILES, TILES_CUT, (8, 8), "wrapper", "periodic", _match_init),
    Case("mosaic", "mosaic", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _mosaic("mosaic")),
    Case("mosaic-feather-gains", "mosaic", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic", _mosaic("feather")),
    Case("mosaic_homography", "mosaic_homography", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic",
         _mosaic("homography")),
    Case("mosaic_overlap", "mosaic_overlap", TILES, N_TILES, TILES_CUT, (5, 66), "wrapper", "periodic",
         _mosaic("overlap")),
    Case("global_motion", "global_motion", TILES, N_TILES, TILES_CUT, (9, 66), "wrapper", "periodic", _fit("affine")),
    Case("global_homography", "global_homography", TILES, N_TILES, TILES_CUT, (9, 66), "wrapper", "periodic",
         _fit("homography")),
    Case("bundle_sums", "bundle_sums", TILES, N_TILES, TILES_CUT, (9, 66), "wrapper", "periodic", _bundle_sums),
]
