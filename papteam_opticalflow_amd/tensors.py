"""Flow on PyTorch device tensors (include/papof.h: papof_flow_batch_tensor): batches of frames that are already on the GPU go
in, flow tensors come out, and nothing crosses PCIe.

    from papteam_opticalflow_amd.tensors import flow_pairs, flow_video
    flow, warpI2, timing = flow_video(frames, 5, layout="NHWC")   # frames: (T, H, W, C) uint8 on cuda:0

Inputs are 4-D tensors on one HIP device (a 3-D tensor is a batch of one) of uint8, float32 or float64, with any non-negative
strides: slices, `permute`d and expanded views are read in place.  `layout` names the axes ("NCHW", PyTorch's convention, or
"NHWC", what video decoders return); it is not inferred, because C == W is ambiguous.  `flow` is (B, 2, H, W) (vx, vy),
`warpI2` has the input's layout; both are new tensors of `out_dtype` (float64, the reference's arithmetic, or float32) on the
input's device, with no autograd graph.  Every pair is bit-identical to the single call on the fp64 values of its frames
(uint8: x / 255.).

Stream contract: the call is ordered behind the work queued so far on `torch.cuda.current_stream(device)` and returns once the
outputs are written -- stream-ordered on entry, complete on return, not asynchronous.

Forward and backward: `flow_video_fb` / `flow_pairs_fb` (include/papof.h: papof_flow_batch_tensor_fb) return both directions of
every pair from one launch chain, and the occlusion mask of the forward-backward consistency check (Sundaram, Brox, Keutzer
2010) computed from the float64 flows; `fb_consistency` is the same check on any two flow tensors.

    fb = flow_video_fb(frames, 5, layout="NHWC")    # fb.flow_fw, fb.flow_bw, fb.warpI2_fw, fb.warpI2_bw, fb.occlusion, fb.timing

Point tracks: `track_points` (include/papof.h: papof_track_tensor) follows points through a video's forward and backward flows
in one HIP kernel, dropping a point where the forward-backward check fails; `track_video` is flow_video_fb followed by it.

    tv = track_video(frames, 5, queries, layout="NHWC")   # queries (N, 3) rows (t0, x, y); tv.tracks (T, N, 2), tv.visible (T, N)

Frame interpolation: `interpolate` (include/papof.h: papof_interp_tensor) makes the frames at times t in (0, 1) between the
two frames of each pair from its forward and backward flows and, optionally, its occlusion mask, in one HIP kernel;
`interpolate_pairs` and `interpolate_video` compute the flows first (flow_pairs_fb / flow_video_fb).

    iv = interpolate_video(frames, 5, factor=3, layout="NHWC")   # iv.video: (3 (T - 1) + 1, H, W, C), frames at 3x the rate

Forward warping: `splat` (include/papof.h: papof_splat_tensor) moves every pixel of a tensor along its own flow and deposits
it where it lands, with optional per-pixel weights (`splat_weights`: exp(-alpha * photometric error)); the sums are 64-bit
fixed-point integers, so the result is bitwise reproducible.  `interpolate(..., method="splat")`
(papof_interp_splat_tensor) splats both frames to the time in between, which stays right at motion boundaries.

    out, coverage = splat(frames[:-1], fb.flow_fw, 0.5, layout="NHWC")   # out (B, 1, H, W, C), coverage (B, 1, H, W)

Stabilization: `global_motion` (include/papof.h: papof_motion_fit_tensor) fits one similarity or affine motion per pair to
its forward flow (robust IRLS in float64, two HIP kernels per iteration), `stabilizing_transforms` smooths the camera path
on the host and `warp_affine` (papof_warp_affine_tensor) resamples the frames; `stabilize_video` chains flow_video and them.

    sv = stabilize_video(frames, 5, layout="NHWC", crop=0.9)   # sv.video: the stabilized frames, sv.valid (T, H, W)

Denoising: `temporal_filter` (include/papof.h: papof_temporal_filter_tensor) averages each pixel with the points it maps to
in the frames t +- 1 .. t +- radius along the forward and backward flows, dropping neighbours whose motion fails the
forward-backward check and down-weighting those that look different, in one HIP kernel; `denoise_video` computes the flows
first (flow_video_fb).

    dv = denoise_video(frames, 5, radius=2, layout="NHWC")   # dv.video: the denoised frames, dv.support (T, H, W) uint8

Video completion: `fill_holes` (include/papof.h: papof_fill_holes_tensor) fills a field inside a mask by pull-push and
Jacobi relaxation; `complete_flows` fills the flows under the masks with it; `propagate` (papof_propagate_tensor) fills
each hole from the nearest frames along the flows where the point is visible; `inpaint_video` chains flow_video_fb, them
and a spatial fill of what no frame shows.

    iv = inpaint_video(frames, masks, 5, layout="NHWC")   # iv.video: the completed frames, iv.status (T, H, W) uint8

Temporal consistency: `temporal_consistency` (include/papof.h: papof_temporal_consistency_tensor) removes the flicker of a
video that a per-frame process made from `frames` (Bonneel et al. 2015): each output frame keeps the processed frame's
gradients and follows the previous output frame warped along the flows, one screened-Poisson solve per frame on the
device; `consistent_video` computes the flows first (flow_video_fb).

    cv = consistent_video(frames, stylized, 5, layout="NHWC")   # cv.video: the consistent processed video

Flow refinement: `refine_flow` (include/papof.h: papof_refine_flow_tensor) is the image-guided weighted median filter of a
flow field (the non-local term of Sun, Roth and Black 2010): it sharpens the motion boundaries that the solver rounds off,
along the edges of a guide image, and gives occluded or NaN pixels their neighbours' motion; integer weights and sums, so the
result is bitwise reproducible.  `refine_video_flows` filters both directions of a video's flows and recomputes the mask.

    fw, bw, occ = refine_video_flows(frames, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion, layout="NHWC")

Super-resolution: `super_resolve` (include/papof.h: papof_super_resolve_tensor) carries every pixel of every frame along the
chains of flows to the frames around it and deposits it on a grid 2, 3 or 4 times finer (shift and add), resolves the sums
against a cubic upsampling and back-projects against the frame; fixed-point integer sums, so the result is bitwise
reproducible.  `super_resolve_video` computes the flows first (flow_video_fb).

    sv = super_resolve_video(frames, 5, scale=2, layout="NHWC")   # sv.video: (T, 2 H, 2 W, C), sv.coverage (T, 2 H, 2 W)

Large displacements: `match_pairs` / `match_video` (include/papof.h: papof_match_tensor) find, for every cell of a
decimated frame, the integer displacement that minimises a sum of absolute differences over a patch (brute force over one
window, integer arithmetic, bitwise reproducible); `match_init` (papof_match_densify_tensor) keeps the cells that pass a
forward-backward test and fills the rest (fill_holes); `flow_pairs_ld` / `flow_video_ld` start flow_pairs_fb from the result,
which brings motion larger than the objects that carry it within the solver's reach.  With `levels` = 2 .. 4
(`match_levels` of the _ld calls; include/papof.h: papof_match_hier_tensor) the search is hierarchical: the flat search on
the grid of stride * 2^(levels - 1), then per level twice the parents' vectors +- `refine` cells -- pans and large
structures beyond stride * search pixels (160 px at the defaults with 3 levels), not objects smaller than the top
level's window, which keep levels=1.  With `recentre` = 1 .. 32 besides (`match_recentre`; papof_match_recentre_tensor) the
flat search runs once more on the finest grid, its window centred tile by tile on the hierarchy's dominant vector: a small
object that moves fast against a large pan.

    fb = flow_video_ld(frames, layout="NHWC")   # a FlowFB, as flow_video_fb's
    fb = flow_video_ld(frames, layout="NHWC", match_levels=3)   # a fast pan: up to 160 px per frame
    fb = flow_video_ld(frames, layout="NHWC", match_levels=3, match_recentre=20)   # and a ball that crosses it

Motion blur: `motion_blur` (include/papof.h: papof_motion_blur_tensor) gives a video a longer shutter: every frame becomes
the weighted mean of the scene at the times of `blur_schedule` around it, each of them what `interpolate` states, summed in
one HIP kernel; `blur_video` computes the flows first (flow_video_fb).

    bv = blur_video(frames, 5, shutter=0.5, samples=16, layout="NHWC")   # bv.video: the frames' shape

Reduced resolution: `decimate` (include/papof.h: papof_decimate_tensor) is the box decimation of frames by 2, 3 or 4 and
`upsample_flow` (papof_upsample_flow_tensor) brings a flow estimated on the decimated frames up again, guided by the
full-resolution frame (joint bilateral upsampling, Kopf et al. 2007), so that motion boundaries land on the image's edges
instead of being spread over `factor` pixels; integer weights, sums in a stated order, bitwise reproducible.
`flow_pairs_lr` / `flow_video_lr` chain them around flow_pairs_fb / flow_video_fb: a quarter of the solver's pixels at
factor 2.

    fb = flow_video_lr(frames, 4, factor=2, layout="NHWC")   # a FlowFB, as flow_video_fb's (warpI2_* None unless refined)

Video mosaics: `mosaic` (include/papof.h: papof_mosaic_tensor) gathers many frames, each through its own affine matrix, into
one output pixel and keeps the first that covers it, their mean or their median -- one HIP kernel, the samples held on
chip; `mosaic_transforms` and `neighbour_transforms` make its matrices from global motions on the host; `panorama` chains
flow_video, global_motion and them (mode "median": the clean plate, what moved is gone); `stabilize_video_full` is
stabilize_video with the empty borders filled from the neighbouring frames.  Seamless mosaics: `mosaic_overlap`
(papof_mosaic_overlap_tensor) gathers the pairwise luminance statistics of the overlaps, `exposure_gains` solves one gain
per source from them on the host, and `mosaic(..., gains=, mode="feather")` (papof_mosaic_blend_tensor) applies the gains
and fades every frame out towards its border; `panorama(..., exposure=True)` chains them.

    pano = panorama(frames, 5, mode="median", layout="NHWC")       # pano.image (Hc, Wc, C), pano.count (Hc, Wc)
    sv = stabilize_video_full(frames, 5, layout="NHWC")            # sv.video, sv.valid, sv.filled
    pano = panorama(frames, 5, mode="feather", exposure=True, layout="NHWC")   # no steps at frame borders; pano.gains

The homography model: a parallel family of calls over 3 x 3 matrices for a camera that rotates -- `global_homography`
(include/papof.h: papof_homography_fit_tensor) fits one homography per pair, `warp_homography`, `mosaic_homography` and
`mosaic_overlap_homography` are the warp, the mosaic (all four modes, gains) and the overlap statistics under the projective
rule, `homography_transforms` makes the canvas and `panorama_homography` chains them.  On matrices whose last row is
(0, 0, 1) they return the bytes of the affine calls.

    pano = panorama_homography(frames, 5, mode="median", layout="NHWC")   # a Panorama with (T, 3, 3) matrices and motion

Wide panoramas: the plane of the homography model ends 90 degrees from the reference frame.  `mosaic_rays` and
`mosaic_overlap_rays` (include/papof.h: papof_mosaic_ray_tensor, papof_mosaic_overlap_ray_tensor) are the mosaic and the
overlap statistics on a canvas of directions given by two small tables -- a cylinder or a sphere --, `estimate_focal` finds
the focal length from the pair homographies, `wide_transforms` makes the canvas, its tables and the matrices (a chain
normalised by its determinant, which keeps its sign past 90 degrees), and `panorama_wide` chains them.  On the plane's tables
they return the bytes of the homography calls.

    pano = panorama_wide(frames, 5, surface="cylinder", layout="NHWC")    # a WidePanorama: Panorama's fields, focal, cols, rows

Bundle adjustment: the chains above multiply pair motions, so the pairs' errors add up.  `bundle_adjust` fits one rotation per
frame and one focal length to the flows of all overlapping frame pairs at once -- `bundle_sums` (include/papof.h:
papof_bundle_sums_tensor) reduces every link's flow to the twenty fp64 sums of a robust Gauss-Newton evaluation on the device,
the host expands, damps and solves --; `chain_rotations`, `bundle_links` and `link_flows` make its start, its links and their
flows, `bundle_transforms` makes the canvas (the full circle where the pan closes), and `panorama_bundle` chains them.

    pano = panorama_bundle(frames, 5, focal=1150.0, layout="NHWC")        # a BundlePanorama: WidePanorama's fields, rotations, links, cost

Mesh stabilization: shake that varies across the image (parallax, rolling shutter) is not one matrix per frame.  `mesh_motion`
(include/papof.h: papof_mesh_motion_tensor) reduces each pair's flow to the lower median of its residual against the global
motion around every vertex of a coarse mesh (SteadyFlow / MeshFlow), `mesh_transforms` smooths the vertices' profiles in
time on the host, `warp_mesh` (papof_warp_mesh_tensor) is warp_affine plus the bilinearly interpolated displacement table,
and `stabilize_video_mesh` chains them behind flow_video_fb and global_motion.

    sv = stabilize_video_mesh(frames, 5, layout="NHWC", grid=(16, 16))   # a MeshStabilized: Stabilized's fields, mesh, vertex_motion, support

Full-frame mesh stabilization: `mosaic_mesh` (include/papof.h: papof_mosaic_mesh_tensor) is mosaic with a displacement table per
(output, source) slot, `neighbour_mesh` makes the tables that register the frames around a mesh-stabilized frame as its own
table registers it, and `stabilize_video_mesh_full` is stabilize_video_mesh whose borders those frames fill.

    sv = stabilize_video_mesh_full(frames, 5, layout="NHWC", fill_radius=15)   # a MeshStabilizedFull: MeshStabilized's fields, filled

Dirt and dropout removal: `detect_defects` (include/papof.h: papof_defect_detect_tensor) flags the pixels of a frame that lie
outside the range of the two points they map to in the neighbouring frames -- defects that live in one frame: dirt,
sparkle, dropouts, a bird --, `dilate_masks` (papof_mask_dilate_tensor) grows masks on the device, `repair_defects` is one
pass on given flows (detect, dilate, complete_flows, detect again, then inpaint_video's steps under the masks) and
`restore_video` runs the passes, estimating the flows again on each pass's video.  Persistent defects (line scratches) are
not found; a small object that outruns the flow is removed like a defect.

    rv = restore_video(frames, 4, layout="NHWC")   # rv.video, rv.masks, rv.detected (T, H, W) bool, rv.status

Deinterlacing: `deinterlace_fields` (include/papof.h: papof_deinterlace_tensor) turns a sequence of fields into full frames,
one per field: each frame keeps its field's lines and makes the others from the two neighbouring fields of that parity
along the flows between them (`field_flows`: the solver on the fields themselves), weighted by the phase of the landing
rows and the agreement of the two samples, over a four-tap cubic of the own field (`bob_fields`, the fallback);
`split_fields` makes the fields from woven frames and `deinterlace_video` chains field_flows and deinterlace_fields.  No gain
at the critical velocity; weaker end frames; telecined film goes through inverse_telecine instead.

    dv = deinterlace_video(split_fields(frames, layout="NHWC"), 4, layout="NHWC")   # dv.video (2 N, H, W, C), dv.confidence

Inverse telecine: film on interlaced video (3:2 pulldown, 2:2) repeats every film frame over two or three consecutive
fields, and weaving those gives the film frames exactly.  `field_metrics` (include/papof.h: papof_field_metrics_tensor)
reduces every field to integer counts of where it weaves worse with its next field than with its previous one and the
reverse, one HIP kernel; `match_fields` turns them into links, groups and a cadence report on the host; `weave_fields`
(papof_weave_fields_tensor) weaves fields by a table; `inverse_telecine` chains them and sends the fields without a partner
through bob_fields or deinterlace_fields, `inverse_telecine_video` computes the field flows for those when there are any.
Wrong at the critical vertical velocity; thresholds are relative to the noise; no cadence lock; no blended telecine.

    it = inverse_telecine(fields, layout="NHWC")   # it.video (N, H, W, C): the film frames, it.times, it.kinds, it.match.cadence

Shot boundaries: every *_video call takes its frames to be one shot.  `shot_histograms` (include/papof.h:
papof_cell_hist_tensor) reduces every frame to integer luma histograms per cell, one HIP kernel; `shot_distances` and
`detect_cuts` compare consecutive frames region by region on the host (cuts, one-frame flashes, runs of cuts), `detect_shots`
chains them, `split_shots` gives the frame ranges for running any call shot by shot, `cut_flows` marks the cut pairs of a
FlowFB with NaN flows -- which every consumer of flows already takes as "nothing to follow" -- and `flow_video_shots` is
flow_video_fb that spends no solve on a cut pair.  No gradual transitions; luma only; thresholds relative to the neighbourhood;
nothing downstream calls it by itself.

    fb, shots = flow_video_shots(frames, 5, layout="NHWC")   # shots.cuts, shots.ranges; fb: a FlowFB over all T - 1 pairs

Rolling shutter: `rectify_frames` (include/papof.h: papof_rs_rectify_tensor) resamples a video whose rows were read out one
after another -- row y of frame t at t + readout (y - a) / H -- to what a global shutter would have recorded at the frame's
time: every pixel's position one frame earlier and later is in the flows, the parabola through the three points is its
trajectory, and a few fixed-point iterations invert it per output pixel; with `matrices` the stabilizing warp is part of
the same resampling.  `rectify_flows` (papof_rs_flow_tensor) gives the rectified video's flows without a second estimation,
`rectify_video` chains flow_video_fb and both, and `stabilize_video_rs` is stabilize_video whose motion fit sees the
rectified flows and whose one warp also rectifies.  readout is the caller's (phones: 0.5 .. 0.9), it is not estimated; shake
near half the frame rate is not recovered; the end frames use a line; dead pixels are not filled.

    rv = rectify_video(frames, 5, 0.8, layout="NHWC")   # rv.video, rv.valid, rv.flow_fw, rv.flow_bw, rv.occlusion

Deblurring: `deblur` (include/papof.h: papof_deblur_tensor) is the inverse of motion_blur for footage whose shutter was open
while the camera shook -- multi-frame Richardson-Lucy deconvolution with a line kernel per pixel from the flows: each
iteration blurs a frame's estimate as the frames around it would have recorded it, divides the recorded frames by that and
multiplies the estimate by the mean of the ratios blurred backwards, two HIP kernels per iteration; `deblur_video` computes
the flows first (flow_video_fb), optionally again on its own result.  The shutter is the caller's; much under shake, little
under a steady pan; few iterations, no prior.

    dv = deblur_video(frames, 4, shutter=0.5, layout="NHWC")   # dv.video: the frames' shape, dv.support (T, H, W) uint8

Decoder surfaces: a decoder on the device hands over YCbCr planes with subsampled chroma (NV12, I420, NV16, YUY2 ...) and an
encoder wants them back.  `ycc_to_rgb` (include/papof.h: papof_ycc_to_rgb_tensor) and `rgb_to_ycc` (papof_rgb_to_ycc_tensor),
one HIP kernel each, are the way in and out with one stated integer rule: bilinear chroma at the stated siting, the matrix
and range of `ycc_tables` (BT.601, BT.709, BT.2020; limited or full), one rounding, and with interlaced=True the chroma of
each FIELD taken from that field's own chroma lines.  `nv12_planes`, `i420_planes` and `packed422_planes` make the three
planes as views of a surface (nothing is copied), `new_nv12` allocates one.  8-bit only; no 4:1:1 or 4:4:4; no transfer
function or gamut conversion; bilinear chroma; `interlaced` is the caller's knowledge; no other call takes surfaces.

    rgb = ycc_to_rgb(*nv12_planes(surface, 1080), interlaced=True)   # (T, 1080, W, 3) uint8 NHWC; then e.g.
    out = rgb_to_ycc(inverse_telecine(split_fields(rgb, layout="NHWC"), layout="NHWC").video, layout="NHWC")   # out.y, out.cb, out.cr

The luma plane of a surface is a one-channel video as it lies: `flow_video(y.unsqueeze(1), 5)` runs on it in place.

High-bit-depth surfaces: `ycc16_to_rgb` and `rgb_to_ycc16` (papof_ycc16_to_rgb_tensor, papof_rgb_to_ycc16_tensor) are the same
pair for samples of 9 to 16 bits in 16-bit words -- P010 / P012 / P016, P210, I010 / yuv420p10le, Y210 -- with the same taps and
an integer rule at the depth's own scale (`ycc_tables16`); a float32 result keeps every bit of a 10- or 12-bit level.
`p010_planes`, `i010_planes` and `y210_planes` make the views, `new_p010` allocates a surface.  No transfer function or gamut
mapping (PQ / HLG stay encoded); no 4:4:4; no uint16 RGB result.

    rgb = ycc16_to_rgb(*p010_planes(surface, 2160), depth=10, matrix="bt2020")   # (T, 2160, W, 3) float32 NHWC

torch is imported when a function is called, not when the package is imported.
"""
import collections
import ctypes
import fractions
import math
import threading

from . import capi

LAYOUTS = ("NCHW", "NHWC")
CONSISTENCY = (0.01, 0.5)  # (alpha1, alpha2) of Sundaram et al.

FlowFB = collections.namedtuple("FlowFB", "flow_fw flow_bw warpI2_fw warpI2_bw occlusion timing")
Tracks = collections.namedtuple("Tracks", "tracks visible")
TrackVideo = collections.namedtuple("TrackVideo", "tracks visible flow_fw flow_bw timing")
InterpPairs = collections.namedtuple("InterpPairs", "frames flow_fw flow_bw occlusion timing")
Interp = collections.namedtuple("Interp", "video flow_fw flow_bw occlusion timing")
Splat = collections.namedtuple("Splat", "out coverage")
METHODS = ("gather", "splat")
ALPHA = 20.0  # splat_weights: the weight of a pixel is exp(-ALPHA * its photometric error)
Motion = collections.namedtuple("Motion", "motion ok support")
Homography = collections.namedtuple("Homography", "motion ok support")
Stabilized = collections.namedtuple("Stabilized", "video valid transforms motion ok flow timing")
MeshMotion = collections.namedtuple("MeshMotion", "vertices support residuals")
MeshStabilized = collections.namedtuple("MeshStabilized", "video valid transforms motion ok flow timing mesh vertex_motion support")
MeshStabilizedFull = collections.namedtuple("MeshStabilizedFull", MeshStabilized._fields + ("filled",))
Filtered = collections.namedtuple("Filtered", "video support")
Denoised = collections.namedtuple("Denoised", "video support flow_fw flow_bw timing")
Flows = collections.namedtuple("Flows", "flow_fw flow_bw")
Propagated = collections.namedtuple("Propagated", "video status")
Inpainted = collections.namedtuple("Inpainted", "video status")
Defects = collections.namedtuple("Defects", "mask score support")
Restored = collections.namedtuple("Restored", "video masks detected status")
RestoredVideo = collections.namedtuple("RestoredVideo", Restored._fields + ("flow_fw", "flow_bw", "timing"))
Deinterlaced = collections.namedtuple("Deinterlaced", "video confidence")
DeinterlacedVideo = collections.namedtuple("DeinterlacedVideo", Deinterlaced._fields + ("flow_fw", "flow_bw", "timing"))
FieldMetrics = collections.namedtuple("FieldMetrics", "counts cell_rows first")
FieldMatch = collections.namedtuple("FieldMatch", "votes links groups cadence share")
Detelecined = collections.namedtuple("Detelecined", "video groups times kinds match")
DetelecinedVideo = collections.namedtuple("DetelecinedVideo", Detelecined._fields + ("flow_fw", "flow_bw", "timing"))
ShotHist = collections.namedtuple("ShotHist", "hist cell_rows bins size")
Surfaces = collections.namedtuple("Surfaces", "y cb cr")
Shots = collections.namedtuple("Shots", "cuts flashes gradual distances ranges")
Rectified = collections.namedtuple("Rectified", "video valid flow_fw flow_bw occlusion timing")
StabilizedRS = collections.namedtuple("StabilizedRS", "video valid transforms motion ok flow_fw flow_bw occlusion timing")
Consistent = collections.namedtuple("Consistent", "video flow_fw flow_bw timing")
Blurred = collections.namedtuple("Blurred", "video flow_fw flow_bw occlusion timing")
Deblurred = collections.namedtuple("Deblurred", "video support")
DeblurredVideo = collections.namedtuple("DeblurredVideo", Deblurred._fields + ("flow_fw", "flow_bw", "occlusion", "timing"))
RefinedFlows = collections.namedtuple("RefinedFlows", "flow_fw flow_bw occlusion")
MODELS = {"similarity": capi.MOTION_SIMILARITY, "affine": capi.MOTION_AFFINE}

_lock = threading.Lock()
_handles = {}  # device ordinal -> (Papof, lock of its calls)


def _torch():
    import torch
    return torch


def dtype_code(dtype):
    """PAPOF_DTYPE_* of an input dtype (TypeError for anything else)"""
    torch = _torch()
    codes = {torch.uint8: capi.DTYPE_U8, torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if dtype not in codes:
        raise TypeError("frames must be uint8, float32 or float64, got %s" % dtype)
    return codes[dtype]


def descriptor(t, layout):
    """(sizes, strides, dtype code) of a 4-D tensor in the logical order (frame, row, column, channel) of the C ABI; strides
    in elements.  Plain function of the tensor's metadata: works on CPU tensors."""
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    if t.dim() != 4:
        raise ValueError("expected a 4-D tensor, got shape %s" % (tuple(t.shape),))
    order = (0, 2, 3, 1) if layout == "NCHW" else (0, 1, 2, 3)
    sizes = tuple(int(t.shape[i]) for i in order)
    strides = tuple(int(t.stride(i)) for i in order)
    return sizes, strides, dtype_code(t.dtype)


def _struct(t, strides, code):
    d = capi.PapofTensor()
    d.data = t.data_ptr()
    d.dtype = code
    for i in range(4):
        d.stride[i] = strides[i]
    return d


def _on_gpu(t):
    """the tensor lives on a HIP device (tests stub this to walk the argument path with CPU tensors)"""
    return t.device.type == "cuda"


def _as4d(name, t):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dim() == 3:
        return t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError("%s must be a 4-D tensor (or 3-D: a batch of one), got shape %s" % (name, tuple(t.shape)))
    return t


def _check(named, layout, out_dtype, levels, min_frames=1, solver=None):
    """every argument error, before anything is launched: (4-D tensors, their descriptors, the output dtype, the solver's
    papof_params of the keywords `solver` -- None without any; an unknown keyword raises here)"""
    torch = _torch()
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    if int(levels) < 1:
        raise ValueError("pyramidLevels must be >= 1")
    ts = [_as4d(n, t) for n, t in named]
    descs = [descriptor(t, layout) for t in ts]
    if out_dtype is None:
        out_dtype = torch.float64
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.float32 or torch.float64, got %s" % out_dtype)
    if len(ts) == 2 and descs[1][0] != descs[0][0]:
        raise ValueError("im1 %s and im2 %s differ in shape" % (tuple(ts[0].shape), tuple(ts[1].shape)))
    if min(descs[0][0][1:]) < 1:
        raise ValueError("empty frames: shape %s" % (tuple(ts[0].shape),))
    if descs[0][0][0] < min_frames:
        raise ValueError("%s needs at least %d frames, got %d" % (named[0][0], min_frames, descs[0][0][0]))
    dev = ts[0].device
    for (n, _), t in zip(named, ts):
        if t.device != dev:
            raise ValueError("%s is on %s, %s on %s: all frames must be on one device" % (n, t.device, named[0][0], dev))
    if not _on_gpu(ts[0]):
        raise ValueError("frames must be on a HIP device (cuda:N), got %s" % dev)
    return ts, descs, out_dtype, capi.default_params(**solver) if solver else None


def _handle(device):
    """one Papof handle per device ordinal for the process, and the lock that serialises its calls"""
    with _lock:
        if device not in _handles:
            _torch().cuda.init()  # PyTorch first, then the handle: both share PyTorch's HIP runtime (README)
            _handles[device] = (capi.Papof(device), threading.Lock())
        return _handles[device]


def _alphas(consistency):
    """(use_check, alpha1, alpha2) of a `consistency` argument: (0, 0.0, 0.0) for None, else two finite numbers >= 0
    (ValueError / TypeError otherwise)"""
    if consistency is None:
        return 0, 0.0, 0.0
    try:
        a1, a2 = consistency
        a1, a2 = float(a1), float(a2)
    except (TypeError, ValueError):
        raise TypeError("consistency must be None or (alpha1, alpha2), got %r" % (consistency,)) from None
    if not (math.isfinite(a1) and math.isfinite(a2) and a1 >= 0 and a2 >= 0):
        raise ValueError("alpha1 and alpha2 must be finite and >= 0, got %r, %r" % (a1, a2))
    return 1, a1, a2


def _index(dev):
    return dev.index if dev.index is not None else _torch().cuda.current_device()


def _launch(dev, name, *args, workspace=None, timers=None):
    """gpu.L.<name>(handle, *args[, workspace, its bytes], stream[, timers]) under the lock of the handle of `dev`, in the
    device, on its current stream; a failing return code raises.  workspace: (the papof_*_workspace function, its arguments,
    the ValueError's text when it refuses them); the bytes come from PyTorch's allocator on the current stream, so they are
    reused only behind the work queued here.  timers: the ctypes array that follows the stream."""
    torch = _torch()
    index = _index(dev)
    gpu, lock = _handle(index)
    if workspace is not None:
        size, size_args, refusal = workspace
        nbytes = getattr(gpu.L, size)(*size_args)
        if nbytes < 0:
            raise ValueError(refusal)
    with lock, torch.cuda.device(index):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if workspace is not None else None
        extra = (ctypes.c_void_p(ws.data_ptr()), nbytes) if ws is not None else ()
        stream = torch.cuda.current_stream(index).cuda_stream
        rc = getattr(gpu.L, name)(gpu.h, *args, *extra, ctypes.c_void_p(stream or None), *(() if timers is None else (timers,)))
        del ws  # back to the allocator behind the call, on this stream
    capi._chk(rc, name)


def _new_frames(n, H, W, C, layout, out_dtype, dev):
    """a new (n, C, H, W) (NCHW) or (n, H, W, C) (NHWC) tensor of out_dtype and its descriptor"""
    out = _torch().empty((n, C, H, W) if layout == "NCHW" else (n, H, W, C), dtype=out_dtype, device=dev)
    return out, _struct(out, *descriptor(out, layout)[1:])


def _outputs(n_pairs, H, W, C, layout, out_dtype, dev):
    """a new flow tensor (B, 2, H, W) and warpI2 in `layout`, and their descriptors"""
    flow = _torch().empty((n_pairs, 2, H, W), dtype=out_dtype, device=dev)
    warp, d_warp = _new_frames(n_pairs, H, W, C, layout, out_dtype, dev)
    return flow, warp, _flow_struct(flow, _out_code(out_dtype)), d_warp


def _mask(n_pairs, H, W, dev):
    """a new uint8 mask (B, 2, H, W) -- channel 0 forward, 1 backward -- and its descriptor (pair, row, column, direction)"""
    occ = _torch().empty((n_pairs, 2, H, W), dtype=_torch().uint8, device=dev)
    return occ, _struct(occ, (2 * H * W, W, 1, H * W), capi.DTYPE_U8)


INIT_MAX = 1e6  # the largest magnitude of an initial flow's component (include/papof.h: papof_flow_batch_tensor_init)


def _check_init(name, init, n_pairs, H, W, dev):
    """the descriptor of an initial flow -- (B, 2, H, W), or (2, H, W) for every pair, float32 / float64 on the frames'
    device -- or None; every error (TypeError / ValueError) before anything of this library is launched.  The value bound is
    checked with torch on the tensor's device."""
    if init is None:
        return None
    torch = _torch()
    codes = {torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if not isinstance(init, torch.Tensor):
        raise TypeError("%s must be None or a torch.Tensor, got %s" % (name, type(init).__name__))
    if init.dtype not in codes:
        raise TypeError("%s must be float32 or float64, got %s" % (name, init.dtype))
    if init.dim() not in (3, 4) or init.shape[-3] != 2:
        raise ValueError("%s must be (B, 2, H, W) or (2, H, W), got shape %s" % (name, tuple(init.shape)))
    if tuple(init.shape[-2:]) != (H, W):
        raise ValueError("%s is %d x %d, the frames %d x %d" % (name, init.shape[-2], init.shape[-1], H, W))
    if init.dim() == 4 and init.shape[0] != n_pairs:
        raise ValueError("%s has %d flows for %d pairs" % (name, init.shape[0], n_pairs))
    if init.device != dev:
        raise ValueError("%s is on %s, the frames on %s" % (name, init.device, dev))
    if not bool((init.abs() <= INIT_MAX).all()):
        raise ValueError("%s has a component that is NaN, infinite or beyond %g in magnitude" % (name, INIT_MAX))
    if init.dim() == 3:
        strides = (0, init.stride(1), init.stride(2), init.stride(0))
    else:
        strides = (init.stride(0), init.stride(2), init.stride(3), init.stride(1))
    return _struct(init, strides, codes[init.dtype])


def _ref(d):
    return ctypes.byref(d) if d is not None else None


def _head(ts, descs, sequence, n_pairs, levels, params):
    """the arguments of the flow calls from n_pairs to params"""
    (_, H, W, C), _, _ = descs[0]
    d_in = [_struct(t, s, c) for t, (_, s, c) in zip(ts, descs)]
    return (n_pairs, 1 if sequence else 0, ctypes.byref(d_in[0]), None if sequence else ctypes.byref(d_in[1]), H, W, C,
            int(levels), _ref(params))


def _run(ts, descs, sequence, n_pairs, layout, out_dtype, levels, params, init_flow=None):
    (_, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    d_init = _check_init("init_flow", init_flow, n_pairs, H, W, dev)
    flow, warp, d_flow, d_warp = _outputs(n_pairs, H, W, C, layout, out_dtype, dev)
    head = _head(ts, descs, sequence, n_pairs, levels, params)
    t = (ctypes.c_double * capi.N_TIMERS)()
    if d_init is None:
        _launch(dev, "papof_flow_batch_tensor", *head, ctypes.byref(d_flow), ctypes.byref(d_warp), timers=t)
    else:
        _launch(dev, "papof_flow_batch_tensor_init", *head, ctypes.byref(d_init), ctypes.byref(d_flow), ctypes.byref(d_warp),
                timers=t)
    return flow, warp, capi.format_timing(list(t))


def flow_pairs(im1, im2, pyramidLevels, *, layout="NCHW", out_dtype=None, init_flow=None, **solver):
    """Flow of the independent pairs (im1[i], im2[i]): two tensors of one shape, (B, C, H, W) or (B, H, W, C) by `layout`.
    Returns (flow (B, 2, H, W), warpI2 (B, ...) in `layout`, the reference's dict of ten timers).
    init_flow: None (start from zero flow), or the flow each pair starts from -- (B, 2, H, W), or (2, H, W) for every pair,
    float32 or float64 on the frames' device, any strides, every component finite and at most 1e6 in magnitude; it enters
    the coarsest pyramid level through the frames' own pyramid, scaled to that level (include/papof.h:
    papof_flow_batch_tensor_init states the rule).  An all-zero init_flow gives the bits of none."""
    ts, descs, out_dtype, params = _check([("im1", im1), ("im2", im2)], layout, out_dtype, pyramidLevels, solver=solver)
    return _run(ts, descs, False, descs[0][0][0], layout, out_dtype, pyramidLevels, params, init_flow)


def flow_video(frames, pyramidLevels, *, layout="NCHW", out_dtype=None, init_flow=None, **solver):
    """Flow of the consecutive pairs (frames[i], frames[i + 1]) of T >= 2 frames (each frame's pyramid is built once).
    Returns (flow (T - 1, 2, H, W), warpI2 (T - 1, ...) in `layout`, the reference's dict of ten timers).
    init_flow: as flow_pairs's, with B = T - 1."""
    ts, descs, out_dtype, params = _check([("frames", frames)], layout, out_dtype, pyramidLevels, min_frames=2, solver=solver)
    return _run(ts, descs, True, descs[0][0][0] - 1, layout, out_dtype, pyramidLevels, params, init_flow)


def _run_fb(ts, descs, sequence, n_pairs, layout, out_dtype, levels, alphas, params, init_flow=None, init_flow_bw=None):
    torch = _torch()
    (_, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    d_init = [_check_init(n, f, n_pairs, H, W, dev) for n, f in (("init_flow", init_flow), ("init_flow_bw", init_flow_bw))]
    flow_fw, warp_fw, d_flow_fw, d_warp_fw = _outputs(n_pairs, H, W, C, layout, out_dtype, dev)
    flow_bw, warp_bw, d_flow_bw, d_warp_bw = _outputs(n_pairs, H, W, C, layout, out_dtype, dev)
    occ, d_occ = _mask(n_pairs, H, W, dev) if alphas[0] else (None, None)
    head = _head(ts, descs, sequence, n_pairs, levels, params)
    tail = (ctypes.byref(d_flow_fw), ctypes.byref(d_warp_fw), ctypes.byref(d_flow_bw), ctypes.byref(d_warp_bw), _ref(d_occ),
            *alphas[1:])
    t = (ctypes.c_double * capi.N_TIMERS)()
    if d_init == [None, None]:
        _launch(dev, "papof_flow_batch_tensor_fb", *head, *tail, timers=t)
    else:
        _launch(dev, "papof_flow_batch_tensor_fb_init", *head, _ref(d_init[0]), _ref(d_init[1]), *tail, timers=t)
    return FlowFB(flow_fw, flow_bw, warp_fw, warp_bw, occ.view(torch.bool) if occ is not None else None,
                  capi.format_timing(list(t)))


def flow_pairs_fb(im1, im2, pyramidLevels, *, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, init_flow=None,
                  init_flow_bw=None, **solver):
    """Both directions of the independent pairs (im1[i], im2[i]) in one launch chain, and their occlusion mask.
    Returns FlowFB(flow_fw, flow_bw (B, 2, H, W), warpI2_fw, warpI2_bw (B, ...) in `layout`, occlusion, timing):
    flow_fw / warpI2_fw are flow_pairs(im1, im2)'s, flow_bw / warpI2_bw flow_pairs(im2, im1)'s, bit for bit.  occlusion is a
    torch.bool tensor (B, 2, H, W), channel 0 the forward pixels (of im1), 1 the backward ones (of im2), from the check with
    consistency = (alpha1, alpha2) on the float64 flows (whatever out_dtype is) -- or None for consistency=None.
    init_flow / init_flow_bw: the initial flows of the forward / backward pairs, as flow_pairs's init_flow (None: zero); each
    direction is flow_pairs(..., init_flow=) on its frames, bit for bit."""
    alphas = _alphas(consistency)
    ts, descs, out_dtype, params = _check([("im1", im1), ("im2", im2)], layout, out_dtype, pyramidLevels, solver=solver)
    return _run_fb(ts, descs, False, descs[0][0][0], layout, out_dtype, pyramidLevels, alphas, params, init_flow,
                   init_flow_bw)


def flow_video_fb(frames, pyramidLevels, *, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, init_flow=None,
                  init_flow_bw=None, **solver):
    """Both directions of the consecutive pairs (frames[i], frames[i + 1]) of T >= 2 frames in one launch chain -- each
    frame's pyramid and features are built once for both -- and their occlusion mask: flow_pairs_fb on
    (frames[:-1], frames[1:]), with T - 1 pairs (and its init_flow / init_flow_bw)."""
    alphas = _alphas(consistency)
    ts, descs, out_dtype, params = _check([("frames", frames)], layout, out_dtype, pyramidLevels, min_frames=2, solver=solver)
    return _run_fb(ts, descs, True, descs[0][0][0] - 1, layout, out_dtype, pyramidLevels, alphas, params, init_flow,
                   init_flow_bw)


def fb_consistency(flow_fw, flow_bw, alpha1=CONSISTENCY[0], alpha2=CONSISTENCY[1]):
    """The forward-backward consistency check on two flow tensors (B, 2, H, W) of float32 or float64, any strides, on one
    HIP device: a torch.bool tensor (B, 2, H, W), True where occluded -- channel 0 forward, 1 backward, as flow_video_fb's
    occlusion, and the same mask for the same float64 flows (include/papof.h: papof_fb_check_tensor).  Enqueued on the
    current stream; returns without waiting."""
    _, a1, a2 = _alphas((alpha1, alpha2))
    codes = _check_flows(flow_fw, flow_bw)
    B, _, H, W = (int(x) for x in flow_fw.shape)
    d = [_flow_struct(f, c) for f, c in zip((flow_fw, flow_bw), codes)]
    occ, d_occ = _mask(B, H, W, flow_fw.device)
    _launch(flow_fw.device, "papof_fb_check_tensor", B, H, W, ctypes.byref(d[0]), ctypes.byref(d[1]), a1, a2,
            ctypes.byref(d_occ))
    return occ.view(_torch().bool)


def _check_queries(queries, dev):
    """queries: None (dense) or an (N, 3) float32 / float64 tensor with N >= 1 on `dev` -- TypeError / ValueError otherwise"""
    torch = _torch()
    if queries is None:
        return None
    if not isinstance(queries, torch.Tensor):
        raise TypeError("queries must be None or a torch.Tensor, got %s" % type(queries).__name__)
    if queries.dim() != 2 or queries.shape[1] != 3 or queries.shape[0] < 1:
        raise ValueError("queries must be (N, 3) rows (t0, x, y) with N >= 1, got shape %s" % (tuple(queries.shape),))
    if queries.dtype not in (torch.float32, torch.float64):
        raise TypeError("queries must be float32 or float64, got %s" % queries.dtype)
    if queries.device != dev:
        raise ValueError("queries are on %s, the flows on %s: both must be on one device" % (queries.device, dev))
    return queries


def _check_flow(name, f):
    """a (B, 2, H, W) float32 / float64 flow tensor with B, H, W >= 1: its dtype code -- TypeError / ValueError otherwise"""
    torch = _torch()
    codes = {torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if not isinstance(f, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(f).__name__))
    if f.dim() != 4 or f.shape[1] != 2 or min(f.shape) < 1:
        raise ValueError("%s must be (B, 2, H, W) with B, H, W >= 1, got shape %s" % (name, tuple(f.shape)))
    if f.dtype not in codes:
        raise TypeError("%s must be float32 or float64, got %s" % (name, f.dtype))
    return codes[f.dtype]


def _check_flows(flow_fw, flow_bw, shape=None, dev=None):
    """every argument error of a flow pair on one HIP device -- of `shape` on the frames' device `dev` when given -- before
    anything is launched: their dtype codes"""
    codes = tuple(_check_flow(n, f) for n, f in (("flow_fw", flow_fw), ("flow_bw", flow_bw)))
    if flow_fw.shape != flow_bw.shape:
        raise ValueError("flow_fw %s and flow_bw %s differ in shape" % (tuple(flow_fw.shape), tuple(flow_bw.shape)))
    if flow_fw.device != flow_bw.device:
        raise ValueError("flow_fw is on %s, flow_bw on %s: both must be on one device" % (flow_fw.device, flow_bw.device))
    if not _on_gpu(flow_fw):
        raise ValueError("flows must be on a HIP device (cuda:N), got %s" % flow_fw.device)
    if shape is not None and tuple(flow_fw.shape) != shape:
        raise ValueError("the flows must be %s for these frames, got %s" % (shape, tuple(flow_fw.shape)))
    if dev is not None and flow_fw.device != dev:
        raise ValueError("the flows are on %s, the frames on %s: all must be on one device" % (flow_fw.device, dev))
    return codes


def _check_occlusion(occlusion, shape, dev):
    """None, or a bool / uint8 occlusion mask of `shape` on `dev`: the mask as uint8 -- TypeError / ValueError otherwise"""
    if occlusion is None:
        return None
    torch = _torch()
    if not isinstance(occlusion, torch.Tensor):
        raise TypeError("occlusion must be None or a torch.Tensor, got %s" % type(occlusion).__name__)
    if occlusion.dtype not in (torch.bool, torch.uint8):
        raise TypeError("occlusion must be torch.bool or torch.uint8, got %s" % occlusion.dtype)
    if tuple(occlusion.shape) != shape:
        raise ValueError("occlusion must be (B, 2, H, W) = %s, got %s" % (shape, tuple(occlusion.shape)))
    if occlusion.device != dev:
        raise ValueError("occlusion is on %s, the flows on %s: all must be on one device" % (occlusion.device, dev))
    return occlusion.view(torch.uint8)


def _track(flow_fw, flow_bw, codes, queries, alphas):
    torch = _torch()
    T, H, W = int(flow_fw.shape[0]) + 1, int(flow_fw.shape[2]), int(flow_fw.shape[3])
    N = int(queries.shape[0]) if queries is not None else H * W
    dev = flow_fw.device
    d = [_flow_struct(f, c) for f, c in zip((flow_fw, flow_bw), codes)]
    d_q = None
    if queries is not None:
        q_code = capi.DTYPE_F32 if queries.dtype == torch.float32 else capi.DTYPE_F64
        d_q = _struct(queries, (queries.stride(0), 0, 0, queries.stride(1)), q_code)
    tracks = torch.empty((T, N, 2), dtype=torch.float64, device=dev)
    vis = torch.empty((T, N), dtype=torch.uint8, device=dev)
    d_tr = _struct(tracks, (tracks.stride(0), tracks.stride(1), 0, tracks.stride(2)), capi.DTYPE_F64)
    d_vis = _struct(vis, (vis.stride(0), vis.stride(1), 0, 0), capi.DTYPE_U8)
    _launch(dev, "papof_track_tensor", T, H, W, ctypes.byref(d[0]), ctypes.byref(d[1]), N if d_q is not None else 0, _ref(d_q),
            *alphas, ctypes.byref(d_tr), ctypes.byref(d_vis))
    return Tracks(tracks, vis.view(torch.bool))


def track_points(flow_fw, flow_bw, queries=None, *, consistency=CONSISTENCY):
    """Follow points through the flows of a video of T frames: flow_fw, flow_bw (T - 1, 2, H, W) float32 or float64 on one
    HIP device, any strides -- pair t from frame t to t + 1 and back, as flow_video_fb returns them.  queries: (N, 3) rows
    (t0, x, y) of float32 / float64 on the flows' device, each tracked forward from frame t0 and backward to frame 0; None:
    every pixel of frame 0, row-major (N = H * W, point n = (0, n % W, n // W)).  Returns Tracks(tracks (T, N, 2) float64
    (x, y), visible (T, N) torch.bool).  A step moves a visible point by the forward flow sampled bilinearly where it is;
    the point is lost where it leaves the image or -- consistency = (alpha1, alpha2); None: no check -- where the backward
    flow sampled where it lands does not bring it back (the test of fb_consistency).  A lost point stays lost in that
    direction: its position is NaN (0x7ff8000000000000) and visible False; an invalid query (t0 not an integer in [0, T - 1],
    (x, y) not a finite point of the image) is lost at every frame.  include/papof.h (papof_track_tensor) states it exactly.
    Enqueued on the current stream; returns without waiting.

    A long video in chunks: let the chunks overlap by one frame, and pass the last frame's positions as t0 = 0 queries of
    the next chunk -- torch.cat([torch.zeros(N, 1, dtype=torch.float64, device=dev), tracks[-1]], 1): a point lost so far is
    NaN there, an invalid query, and stays lost."""
    alphas = _alphas(consistency)
    codes = _check_flows(flow_fw, flow_bw)
    queries = _check_queries(queries, flow_fw.device)
    return _track(flow_fw, flow_bw, codes, queries, alphas)


def track_video(frames, pyramidLevels, queries=None, *, layout="NCHW", consistency=CONSISTENCY, **solver):
    """Flow and point tracks of a video of T >= 2 frames: flow_video_fb(frames, pyramidLevels, layout=layout,
    consistency=None, **solver) -- both float64 flows of every pair in one launch chain -- followed by track_points on
    them.  Returns TrackVideo(tracks (T, N, 2), visible (T, N), flow_fw, flow_bw (T - 1, 2, H, W), timing of the flow call).
    Every argument error raises before anything is launched; the flows are complete on return, the tracks are enqueued on
    the current stream behind them."""
    alphas = _alphas(consistency)
    ts, descs, out_dtype, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    queries = _check_queries(queries, ts[0].device)
    fb = _run_fb(ts, descs, True, descs[0][0][0] - 1, layout, out_dtype, pyramidLevels, _alphas(None), params)
    tr = _track(fb.flow_fw, fb.flow_bw, (capi.DTYPE_F64, capi.DTYPE_F64), queries, alphas)
    return TrackVideo(tr.tracks, tr.visible, fb.flow_fw, fb.flow_bw, fb.timing)


def _times(times, inside=True):
    """the times as a list of floats, each finite and (with `inside`) strictly inside (0, 1) -- TypeError / ValueError
    otherwise.  A tensor is read on the host (a device tensor waits for its stream)."""
    torch = _torch()
    if isinstance(times, torch.Tensor):
        if times.dim() > 1 or times.dtype == torch.bool or times.is_complex():
            raise TypeError("times must be a float, a sequence or a 1-D real tensor, got %s of shape %s"
                            % (times.dtype, tuple(times.shape)))
        ts = [float(x) for x in times.reshape(-1).tolist()]
    elif isinstance(times, (int, float)) and not isinstance(times, bool):
        ts = [float(times)]
    else:
        try:
            ts = [float(x) for x in times]
        except (TypeError, ValueError):
            raise TypeError("times must be a float, a sequence of floats or a 1-D tensor, got %r" % (times,)) from None
    if not ts:
        raise ValueError("times is empty")
    for x in ts:
        if not math.isfinite(x):
            raise ValueError("every time must be finite, got %r" % x)
        if inside and not 0.0 < x < 1.0:
            raise ValueError("every time must lie strictly inside (0, 1), got %r" % x)
    return ts


def _out_code(out_dtype):
    torch = _torch()
    codes = {torch.uint8: capi.DTYPE_U8, torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if out_dtype not in codes:
        raise TypeError("out_dtype must be torch.uint8, torch.float32 or torch.float64, got %s" % out_dtype)
    return codes[out_dtype]


def _out_dtype(out_dtype, default):
    """out_dtype, `default` for None -- TypeError for a dtype the kernels do not store"""
    out_dtype = default if out_dtype is None else out_dtype
    _out_code(out_dtype)
    return out_dtype


def _flow_struct(f, code):
    return _struct(f, (f.stride(0), f.stride(2), f.stride(3), f.stride(1)), code)


def _weight_struct(w):
    """the descriptor (item, row, column, -) of a checked weight tensor, None for None"""
    if w is None:
        return None
    code = capi.DTYPE_F32 if w.dtype == _torch().float32 else capi.DTYPE_F64
    return _struct(w, (w.stride(0), w.stride(1), w.stride(2), 0), code)


def _check_weight(name, w, shape, dev):
    """None, or a float32 / float64 weight tensor of `shape` = (B, H, W) on `dev`: w itself -- TypeError / ValueError
    otherwise"""
    if w is None:
        return None
    torch = _torch()
    codes = (torch.float32, torch.float64)
    if not isinstance(w, torch.Tensor):
        raise TypeError("%s must be None or a torch.Tensor, got %s" % (name, type(w).__name__))
    if w.dtype not in codes:
        raise TypeError("%s must be float32 or float64, got %s" % (name, w.dtype))
    if tuple(w.shape) != shape:
        raise ValueError("%s must be (B, H, W) = %s, got %s" % (name, shape, tuple(w.shape)))
    if w.device != dev:
        raise ValueError("%s is on %s, the frames on %s: all must be on one device" % (name, w.device, dev))
    return w


def _check_method(method, weights, shape, dev):
    """None for "gather", the two weight tensors (each may be None) for "splat" -- ValueError / TypeError otherwise"""
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (METHODS, method))
    if method == "gather":
        if weights is not None:
            raise ValueError("weights are for method=\"splat\"")
        return None
    if weights is None:
        return None, None
    if not isinstance(weights, (tuple, list)) or len(weights) != 2:
        raise TypeError("weights must be None or a pair (w_fw, w_bw), got %r" % (weights,))
    w_fw, w_bw = weights
    return _check_weight("w_fw", w_fw, shape, dev), _check_weight("w_bw", w_bw, shape, dev)


def _check_alpha(alpha):
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise TypeError("alpha must be a number, got %r" % (alpha,)) from None
    if not (math.isfinite(alpha) and alpha >= 0):
        raise ValueError("alpha must be finite and >= 0, got %r" % alpha)
    return alpha


def _interp(d_in, sequence, n_pairs, H, W, C, flows, codes, occlusion, times, out, d_out, time_stride, dev, splat=None):
    """papof_interp_tensor -- or, with splat = (the forward weights or None, the backward ones or None),
    papof_interp_splat_tensor -- on the current stream of `dev`, writing through d_out"""
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_occ = _flow_struct(occlusion, capi.DTYPE_U8) if occlusion is not None else None
    ts = (ctypes.c_double * len(times))(*times)
    head = (n_pairs, 1 if sequence else 0, ctypes.byref(d_in[0]), None if sequence else ctypes.byref(d_in[1]), H, W, C,
            ctypes.byref(d_f[0]), ctypes.byref(d_f[1]))
    tail = (_ref(d_occ), len(times), ts, ctypes.byref(d_out), time_stride)
    if splat is None:
        _launch(dev, "papof_interp_tensor", *head, *tail)
    else:
        d_w = [_weight_struct(w) for w in splat]
        _launch(dev, "papof_interp_splat_tensor", *head, _ref(d_w[0]), _ref(d_w[1]), *tail,
                workspace=("papof_splat_workspace", (2 * n_pairs, len(times), H, W, C),
                           "%d pairs of %d x %d x %d are too large to splat" % (n_pairs, H, W, C)))
    return out


def _new_interp_out(B, K, H, W, C, layout, out_dtype, dev):
    """a new (B, K, C, H, W) (NCHW) or (B, K, H, W, C) (NHWC) tensor, its descriptor and time stride"""
    torch = _torch()
    if layout == "NCHW":
        out = torch.empty((B, K, C, H, W), dtype=out_dtype, device=dev)
        strides = (out.stride(0), out.stride(3), out.stride(4), out.stride(2))
    else:
        out = torch.empty((B, K, H, W, C), dtype=out_dtype, device=dev)
        strides = (out.stride(0), out.stride(2), out.stride(3), out.stride(4))
    return out, _struct(out, strides, _out_code(out_dtype)), out.stride(1)


def interpolate(im1, im2, flow_fw, flow_bw, times, *, occlusion=None, layout="NCHW", out_dtype=None, method="gather",
                weights=None):
    """Motion-compensated interpolation between the frames of the pairs (im1[i], im2[i]): two tensors of one shape,
    (B, C, H, W) or (B, H, W, C) by `layout`, of uint8 (read as x / 255), float32 or float64, any strides, on one HIP
    device.  flow_fw, flow_bw: (B, 2, H, W) float32 / float64, im1 -> im2 and back, as flow_pairs_fb returns them.
    occlusion: None, or the (B, 2, H, W) bool / uint8 mask of flow_pairs_fb (channel 0: pixels of im1 occluded in im2,
    channel 1 the reverse).  times: a float, a sequence or a 1-D tensor of values strictly inside (0, 1), read on the host.
    Returns the frames at those times, (B, K, C, H, W) for NCHW or (B, K, H, W, C) for NHWC, K = len(times), of out_dtype:
    uint8 (clamp(rint(255 x), 0, 255)), float32 or float64 -- by default the frames' dtype (torch.promote_types of the two).
    Each output pixel p samples im1 at p + F_t->0 and im2 at p + F_t->1, F_t->0 = -(1 - t) t F01 + t^2 F10,
    F_t->1 = (1 - t)^2 F01 - (1 - t) t F10 with the flows at p, and blends the two with weights 1 - t and t, each lowered
    where the mask says its sample is hidden in the other frame; include/papof.h (papof_interp_tensor) states it exactly.
    method="splat" (papof_interp_splat_tensor) instead moves every pixel of im1 along t F01 and every pixel of im2 along
    (1 - t) F10, each along its OWN flow, and divides the two blended sums; `weights` is None (all ones) or a pair
    (w_fw, w_bw) of (B, H, W) float32 / float64 tensors for the pixels of im1 and of im2 (either may be None), as
    splat_weights makes them.  Only the pixels that nothing reaches are method="gather"'s, and only they use the mask.
    Enqueued on the current stream; returns without waiting."""
    ts, descs, _, _ = _check([("im1", im1), ("im2", im2)], layout, None, 1)
    times = _times(times)
    splat = _check_method(method, weights, descs[0][0][:3], ts[0].device)
    out_dtype = _out_dtype(out_dtype, _torch().promote_types(ts[0].dtype, ts[1].dtype))
    (B, H, W, C), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (B, 2, H, W), ts[0].device)
    occ = _check_occlusion(occlusion, (B, 2, H, W), ts[0].device)
    out, d_out, tstride = _new_interp_out(B, len(times), H, W, C, layout, out_dtype, ts[0].device)
    d_in = [_struct(t, s, c) for t, (_, s, c) in zip(ts, descs)]
    return _interp(d_in, False, B, H, W, C, (flow_fw, flow_bw), codes, occ, times, out, d_out, tstride, ts[0].device, splat)


def _photometric_weights(im, warped, alpha, layout):
    torch = _torch()
    a, b = (t.double() / 255.0 if t.dtype == torch.uint8 else t.double() for t in (im, warped))
    err = (a - b).abs().mean(dim=1 if layout == "NCHW" else 3)
    return torch.exp(torch.clamp(-alpha * err, min=-11.0))


def splat_weights(im, warped, alpha=ALPHA, *, layout="NCHW"):
    """The weights of the pixels of `im` for splat / interpolate(method="splat"): exp(clamp(-alpha * mean over channels of
    |im - warped|, min=-11)), a (B, H, W) float64 tensor made with torch operations on the tensors' device (uint8 read as
    x / 255).  `warped` is the other frame brought to this one -- the warpI2 that the flow calls return: a pixel whose flow
    is wrong or which is hidden in the other frame looks different there and counts for little where it lands.  The floor
    e^-11 (about 2^-15.9) keeps every weight far above the resolution 2^-32 of the splat's fixed point, so a pixel that
    only badly matched pixels reach is still covered."""
    alpha = _check_alpha(alpha)
    ts, _, _, _ = _check([("im", im), ("warped", warped)], layout, None, 1)
    return _photometric_weights(ts[0], ts[1], alpha, layout)


MAX_BOUND_LOG2 = 20  # include/papof.h: papof_splat_tensor


def _check_bound(bound):
    """bound as a float: 2^k with k an integer in [-20, 20] -- TypeError / ValueError otherwise"""
    try:
        bound = float(bound)
    except (TypeError, ValueError):
        raise TypeError("bound must be a number, got %r" % (bound,)) from None
    if not (math.isfinite(bound) and bound > 0 and math.frexp(bound)[0] == 0.5
            and abs(math.frexp(bound)[1] - 1) <= MAX_BOUND_LOG2):
        raise ValueError("bound must be a power of two from 2^-%d to 2^%d, got %r" % (MAX_BOUND_LOG2, MAX_BOUND_LOG2, bound))
    return bound


def splat(x, flow, times=1.0, *, weight=None, bound=1.0, fill=0.0, layout="NCHW", out_dtype=None):
    """Forward warping: every pixel of x -- (B, C, H, W) or (B, H, W, C) by `layout` (3-D: one item), uint8 (read as
    x / 255), float32 or float64, any strides, on a HIP device -- is moved along t times its own flow, flow (B, 2, H, W)
    float32 / float64, and deposited bilinearly on the four pixels around where it lands, for every t of `times`: a float,
    a sequence or a 1-D tensor of finite values read on the host (0 deposits in place, values outside [0, 1] extrapolate).
    weight: None (1.0) or (B, H, W) float32 / float64 -- a pixel counts with min(weight, 1) and not at all where its weight
    is <= 0 or not finite, its flow is not finite or it lands outside the image.  bound: a power of two, 2^-20 .. 2^20,
    that no |value| of x exceeds (1.0 for frames; larger values are clamped to it): splat(flow, flow, bound=1024.0) carries
    a flow field of at most 1024 pixels to the frame it points to.  Returns Splat(out, coverage): out (B, K, C, H, W) or
    (B, K, H, W, C), K = len(times), of out_dtype (uint8 as clamp(rint(255 v), 0, 255), float32 or float64; by default x's
    dtype), the weighted mean of what landed on each pixel, or `fill` where coverage < 2^-24 (a hole); coverage
    (B, K, H, W) float64, the sum of the weights that landed.  The sums are 64-bit fixed-point integers added atomically,
    so the result does not depend on the order of arrival: it is bitwise reproducible.  include/papof.h
    (papof_splat_tensor) states the rule exactly.  The workspace comes from PyTorch's allocator; enqueued on the current
    stream, returns without waiting."""
    torch = _torch()
    ts, descs, _, _ = _check([("x", x)], layout, None, 1)
    times = _times(times, inside=False)
    bound = _check_bound(bound)
    try:
        fill = float(fill)
    except (TypeError, ValueError):
        raise TypeError("fill must be a number, got %r" % (fill,)) from None
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    (B, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    f_code = _check_flow("flow", flow)
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("flow must be %s for this x, got %s" % ((B, 2, H, W), tuple(flow.shape)))
    if flow.device != dev:
        raise ValueError("flow is on %s, x on %s: all must be on one device" % (flow.device, dev))
    d_w = _weight_struct(_check_weight("weight", weight, (B, H, W), dev))
    K = len(times)
    out, d_out, tstride = _new_interp_out(B, K, H, W, C, layout, out_dtype, dev)
    coverage = torch.empty((B, K, H, W), dtype=torch.float64, device=dev)
    d_cov = _struct(coverage, coverage.stride(), capi.DTYPE_F64)
    d_x, d_flow = _struct(ts[0], strides, code), _flow_struct(flow, f_code)
    _launch(dev, "papof_splat_tensor", B, H, W, C, ctypes.byref(d_x), ctypes.byref(d_flow), _ref(d_w), K,
            (ctypes.c_double * K)(*times), bound, fill, ctypes.byref(d_out), tstride, ctypes.byref(d_cov),
            workspace=("papof_splat_workspace", (B, K, H, W, C),
                       "%d items of %d x %d x %d are too large to splat" % (B, H, W, C)))
    return Splat(out, coverage)


def interpolate_pairs(im1, im2, pyramidLevels, times, *, layout="NCHW", consistency=CONSISTENCY, out_dtype=None,
                      method="gather", alpha=ALPHA, **solver):
    """flow_pairs_fb(im1, im2, pyramidLevels, layout=layout, consistency=consistency, **solver) -- float64 flows whatever
    out_dtype is -- followed by interpolate on its flows and mask (None for consistency=None: no mask).  Returns
    InterpPairs(frames (B, K, ...) as interpolate's, flow_fw, flow_bw, occlusion, timing of the flow call).  Every argument
    error raises before anything is launched; the flows are complete on return, the frames are enqueued on the current
    stream behind them.  method="splat": interpolate's, with the weights splat_weights(im1, warpI2_fw, alpha) and
    splat_weights(im2, warpI2_bw, alpha) of the flow call's own warped frames."""
    torch = _torch()
    alphas = _alphas(consistency)
    _check_method(method, None, None, None)
    alpha = _check_alpha(alpha)
    ts, descs, _, params = _check([("im1", im1), ("im2", im2)], layout, None, pyramidLevels, solver=solver)
    times = _times(times)
    out_dtype = _out_dtype(out_dtype, torch.promote_types(ts[0].dtype, ts[1].dtype))
    (B, H, W, C), _, _ = descs[0]
    fb = _run_fb(ts, descs, False, B, layout, torch.float64, pyramidLevels, alphas, params)
    occ = fb.occlusion.view(torch.uint8) if fb.occlusion is not None else None
    out, d_out, tstride = _new_interp_out(B, len(times), H, W, C, layout, out_dtype, ts[0].device)
    d_in = [_struct(t, s, c) for t, (_, s, c) in zip(ts, descs)]
    _interp(d_in, False, B, H, W, C, (fb.flow_fw, fb.flow_bw), (capi.DTYPE_F64, capi.DTYPE_F64), occ, times, out, d_out,
            tstride, ts[0].device, _own_weights(method, ts[0], ts[1], fb, alpha, layout))
    return InterpPairs(out, fb.flow_fw, fb.flow_bw, fb.occlusion, fb.timing)


def _own_weights(method, im1, im2, fb, alpha, layout):
    """_interp's `splat` from the warped frames of the flow call fb (None for method="gather")"""
    if method == "gather":
        return None
    return tuple(_photometric_weights(im, warped, alpha, layout) for im, warped in ((im1, fb.warpI2_fw), (im2, fb.warpI2_bw)))


def _converted(frames, out_dtype):
    """frames in out_dtype by the kernel's conversions: the same dtype bit for bit; uint8 -> float as x / 255.0 in float64
    (then one rounding to float32); float -> uint8 as clamp(rint(255 x), 0, 255) in float64, NaN -> 0"""
    torch = _torch()
    if frames.dtype == out_dtype:
        return frames
    x = frames.double()
    if frames.dtype == torch.uint8:
        x = x / 255.0
    if out_dtype == torch.uint8:
        x = torch.nan_to_num(torch.round(255.0 * x), nan=0.0).clamp(0.0, 255.0)
    return x.to(out_dtype)


def interpolate_video(frames, pyramidLevels, factor=2, *, layout="NCHW", consistency=CONSISTENCY, out_dtype=None,
                      method="gather", alpha=ALPHA, **solver):
    """A video of T >= 2 frames at `factor` (an integer >= 2) times its frame rate: flow_video_fb(frames, pyramidLevels,
    layout=layout, consistency=consistency, **solver) -- float64 flows whatever out_dtype is -- then interpolate between
    every two consecutive frames at the times j / factor, j = 1 .. factor - 1.  Returns Interp(video, flow_fw, flow_bw,
    occlusion, timing of the flow call): video has (T - 1) factor + 1 frames in `layout` and out_dtype (by default the
    frames'); frame k factor is input frame k, copied bit for bit (converted as interpolate converts when out_dtype
    differs), and the frames between are written by the kernel straight into the video.  Every argument error raises
    before anything is launched; the flows are complete on return, the video is enqueued on the current stream.
    method="splat": as interpolate_pairs's, the weights from the flow call's own warped frames."""
    torch = _torch()
    alphas = _alphas(consistency)
    _check_method(method, None, None, None)
    alpha = _check_alpha(alpha)
    ts, descs, _, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    if isinstance(factor, bool) or not isinstance(factor, int) or factor < 2:
        raise ValueError("factor must be an integer >= 2, got %r" % (factor,))
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    (T, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    fb = _run_fb(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, alphas, params)
    video, _ = _new_frames((T - 1) * factor + 1, H, W, C, layout, out_dtype, dev)
    video[::factor].copy_(_converted(ts[0], out_dtype))
    _, vs, code = descriptor(video, layout)
    d_out = _struct(video[1], (factor * vs[0],) + vs[1:], code)
    occ = fb.occlusion.view(torch.uint8) if fb.occlusion is not None else None
    times = [j / factor for j in range(1, factor)]
    d_in = [_struct(t, s, c) for t, (_, s, c) in zip(ts, descs)]
    _interp(d_in, True, T - 1, H, W, C, (fb.flow_fw, fb.flow_bw), (capi.DTYPE_F64, capi.DTYPE_F64), occ, times, video, d_out,
            vs[0], dev, _own_weights(method, ts[0][:-1], ts[0][1:], fb, alpha, layout))
    return Interp(video, fb.flow_fw, fb.flow_bw, fb.occlusion, fb.timing)


def _check_fit(model, iters, scale):
    """(PAPOF_MOTION_* code, iterations, Cauchy scale) of global_motion's keywords -- TypeError / ValueError otherwise"""
    if model not in MODELS:
        raise ValueError("model must be one of %s, got %r" % (sorted(MODELS), model))
    return (MODELS[model],) + _check_irls(iters, scale)


def _check_irls(iters, scale):
    """(iterations, Cauchy scale) of a robust fit's keywords -- TypeError / ValueError otherwise"""
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError("iters must be an integer >= 1, got %r" % (iters,))
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError("scale must be a number, got %r" % (scale,))
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError("scale must be finite and > 0, got %r" % (scale,))
    return iters, float(scale)


def _motion_fit(flow, code, occlusion, model, iters, scale):
    torch = _torch()
    B, _, H, W = (int(x) for x in flow.shape)
    dev = flow.device
    motion = torch.empty((B, 2, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    support = torch.empty((B,), dtype=torch.float64, device=dev)
    d_flow = _flow_struct(flow, code)
    d_occ = _flow_struct(occlusion, capi.DTYPE_U8) if occlusion is not None else None
    d_m = _struct(motion, (motion.stride(0), motion.stride(1), motion.stride(2), 0), capi.DTYPE_F64)
    d_ok = _struct(ok, (ok.stride(0), 0, 0, 0), capi.DTYPE_U8)
    d_s = _struct(support, (support.stride(0), 0, 0, 0), capi.DTYPE_F64)
    _launch(dev, "papof_motion_fit_tensor", B, H, W, ctypes.byref(d_flow), _ref(d_occ), model, iters, scale, ctypes.byref(d_m),
            ctypes.byref(d_ok), ctypes.byref(d_s),
            workspace=("papof_motion_workspace", (B, H, W), "a %d x %d flow is too large for global_motion" % (H, W)))
    return Motion(motion, ok.view(torch.bool), support)


def global_motion(flow, *, occlusion=None, model="affine", iters=5, scale=1.0):
    """The global motion of each pair's forward flow: flow (B, 2, H, W) float32 / float64 on a HIP device, any strides, as
    flow_video returns it; occlusion None or the (B, 2, H, W) bool / uint8 mask of flow_video_fb (channel 0 is read: masked
    pixels are left out).  model: "similarity" (scale, rotation, translation) or "affine"; fitted by `iters` iterations of
    reweighted least squares in float64 with Cauchy weights 1 / (1 + e^2 / scale^2), e the pixel distance between where the
    flow sends a pixel and where the previous iteration's motion sends it.  Pixels whose flow is not finite or leaves the
    image are left out.  Returns Motion(motion (B, 2, 3) float64 -- the pixel-coordinate matrix sending (x, y, 1) of frame i
    to frame i + 1 --, ok (B,) bool -- False where no fit was possible (motion is the identity) --, support (B,) float64 --
    the last iteration's sum of weights over H * W).  include/papof.h (papof_motion_fit_tensor) states the rule exactly; the
    results are bitwise reproducible.  Enqueued on the current stream; returns without waiting."""
    model, iters, scale = _check_fit(model, iters, scale)
    code = _check_flow("flow", flow)
    occ = _check_occlusion(occlusion, tuple(flow.shape), flow.device)
    if not _on_gpu(flow):
        raise ValueError("flow must be on a HIP device (cuda:N), got %s" % flow.device)
    return _motion_fit(flow, code, occ, model, iters, scale)


def _check_matrices(matrices, n, dev, rows=2):
    torch = _torch()
    codes = {torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if not isinstance(matrices, torch.Tensor):
        raise TypeError("matrices must be a torch.Tensor, got %s" % type(matrices).__name__)
    if matrices.dtype not in codes:
        raise TypeError("matrices must be float32 or float64, got %s" % matrices.dtype)
    if tuple(matrices.shape) != (n, rows, 3):
        raise ValueError("matrices must be (B, %d, 3) = %s, got %s" % (rows, (n, rows, 3), tuple(matrices.shape)))
    if matrices.device != dev:
        raise ValueError("matrices are on %s, the frames on %s: both must be on one device" % (matrices.device, dev))
    return codes[matrices.dtype]


def _warp(ts, descs, matrices, m_code, layout, out_dtype, call="papof_warp_affine_tensor"):
    torch = _torch()
    (B, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(B, H, W, C, layout, out_dtype, dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], descs[0][1], descs[0][2])
    d_mat = _struct(matrices, (matrices.stride(0), matrices.stride(1), matrices.stride(2), 0), m_code)
    d_valid = _struct(valid, (valid.stride(0), valid.stride(1), valid.stride(2), 1), capi.DTYPE_U8)
    _launch(dev, call, B, H, W, C, ctypes.byref(d_in), ctypes.byref(d_mat), ctypes.byref(d_out),
            ctypes.byref(d_valid))
    return out, valid.view(torch.bool)


def warp_affine(frames, matrices, *, layout="NCHW", out_dtype=None):
    """Each frame resampled through its own affine matrix: frames (B, C, H, W) or (B, H, W, C) by `layout`, uint8 (read as
    x / 255), float32 or float64, any strides, on a HIP device; matrices (B, 2, 3) float32 / float64 on the same device.
    Output pixel (x, y) of frame i is frames[i] sampled bilinearly (the rule of interpolate) at M (x, y, 1), M = matrices[i],
    or 0 where that point is NaN or outside the frame.  Returns (frames_out in `layout` and out_dtype -- uint8 as
    clamp(rint(255 x), 0, 255), float32 or float64; by default the frames' dtype --, valid (B, H, W) bool: True where the
    point lay inside).  include/papof.h (papof_warp_affine_tensor) states it exactly.  Enqueued on the current stream;
    returns without waiting."""
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    m_code = _check_matrices(matrices, descs[0][0][0], ts[0].device)
    return _warp(ts, descs, matrices, m_code, layout, out_dtype)


def _check_path(radius, crop, size):
    if isinstance(radius, bool) or not isinstance(radius, int) or radius < 0:
        raise ValueError("radius must be an integer >= 0, got %r" % (radius,))
    if isinstance(crop, bool) or not isinstance(crop, (int, float)):
        raise TypeError("crop must be a number, got %r" % (crop,))
    if not (math.isfinite(crop) and 0 < crop <= 1):
        raise ValueError("crop must lie in (0, 1], got %r" % (crop,))
    if size is None:
        if crop != 1:
            raise ValueError("crop != 1 zooms about the image centre: give size=(H, W)")
        return 0.0, 0.0
    try:
        H, W = (int(x) for x in size)
    except (TypeError, ValueError):
        raise TypeError("size must be (H, W), got %r" % (size,)) from None
    if H < 1 or W < 1:
        raise ValueError("size must be positive, got %r" % (size,))
    return (W - 1) / 2.0, (H - 1) / 2.0


def _checked_motion(motion, kind=Motion):
    """a Motion or a (T - 1, 2, 3) tensor as it is, or with kind=Homography a Homography or a (T - 1, 3, 3) tensor --
    TypeError / ValueError otherwise"""
    rows = 2 if kind is Motion else 3
    m = motion.motion if isinstance(motion, kind) else motion
    if not isinstance(m, _torch().Tensor):
        raise TypeError("motion must be a torch.Tensor or a %s, got %s" % (kind.__name__, type(m).__name__))
    if m.dim() != 3 or tuple(m.shape[1:]) != (rows, 3) or m.shape[0] < 1:
        raise ValueError("motion must be (T - 1, %d, 3) with T >= 2, got shape %s" % (rows, tuple(m.shape)))
    return motion


def stabilizing_transforms(motion, radius=15, crop=1.0, *, size=None):
    """The sampling matrices that stabilize a video of T frames whose consecutive pairs move by `motion` -- a (T - 1, 2, 3)
    tensor (global_motion's, any device) or a Motion, whose pairs with ok False enter as the identity.  In float64 on the
    host (one small copy from the device; this is where stabilize_video waits), with 3 x 3 homogeneous matrices:
        P_0 = I,  P_{t+1} = A_t P_t                        (the camera path: frame 0's coordinates to frame t's)
        S_t = sum_k g_k P_{t+k} / sum_k g_k,  g_k = exp(-k^2 / (2 (radius / 2)^2)),  k in [-radius, radius] within the video
        M_t = P_t S_t^-1 Z,  Z q = c + crop (q - c)        (c = ((W - 1) / 2, (H - 1) / 2) of size = (H, W): a zoom that hides
                                                            the borders; size is needed only for crop < 1)
    and stabilized frame t is frame t sampled at M_t q (warp_affine(frames, M)).  radius = 0: no smoothing, S_t = P_t.
    Returns M (T, 2, 3) float64 on the motion's device."""
    motion = _checked_motion(motion)
    cx, cy = _check_path(radius, crop, size)
    A, dev = _pair_motions(motion)
    return _torch().from_numpy(path_transforms(A, radius, crop, cx, cy)).to(dev)


def camera_path(A):
    """the camera path P (T, 3, 3) of pair motions A (T - 1, 2, 3), numpy float64: P_0 = I, P_{t+1} = A_t P_t -- frame 0's
    coordinates to frame t's"""
    import numpy as np
    n = A.shape[0] + 1
    P = np.empty((n, 3, 3))
    P[0] = np.eye(3)
    for t in range(n - 1):
        At = np.eye(3)
        At[:2] = A[t]
        P[t + 1] = At @ P[t]
    return P


def path_transforms(A, radius, crop, cx, cy):
    """stabilizing_transforms on a numpy (T - 1, 2, 3) float64 array, c = (cx, cy): (T, 2, 3) float64"""
    import numpy as np
    n = A.shape[0] + 1
    P = camera_path(A)
    Z = np.array([[crop, 0.0, cx - crop * cx], [0.0, crop, cy - crop * cy], [0.0, 0.0, 1.0]])
    M = np.empty((n, 2, 3))
    for t in range(n):
        ks = range(max(-radius, -t), min(radius, n - 1 - t) + 1)
        g = [math.exp(-k * k / (2.0 * (radius / 2.0) ** 2)) if radius > 0 else 1.0 for k in ks]
        S = sum(gk * P[t + k] for gk, k in zip(g, ks)) / sum(g)
        M[t] = (P[t] @ np.linalg.inv(S) @ Z)[:2]
    return M


def stabilize_video(frames, pyramidLevels, *, layout="NCHW", model="similarity", radius=15, crop=1.0, iters=5, scale=1.0,
                    out_dtype=None, **solver):
    """A video of T >= 2 frames with its camera shake removed: flow_video(frames, pyramidLevels, layout=layout, **solver)
    (forward float64 flows), global_motion on them (model, iters, scale), stabilizing_transforms (radius, crop; the only
    wait) and warp_affine of the frames by those matrices.  Returns Stabilized(video (T, ...) in `layout` and out_dtype (by
    default the frames'), valid (T, H, W) bool, transforms (T, 2, 3) float64, motion (T - 1, 2, 3) float64, ok (T - 1,) bool,
    flow (T - 1, 2, H, W) float64, timing of the flow call).  Every argument error raises before anything is launched; the
    video is enqueued on the current stream."""
    ts, descs, _, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    code, iters, scale = _check_fit(model, iters, scale)
    (T, H, W, C), _, _ = descs[0]
    _check_path(radius, crop, (H, W))
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    flow, _, timing = _run(ts, descs, True, T - 1, layout, _torch().float64, pyramidLevels, params)
    m = _motion_fit(flow, capi.DTYPE_F64, None, code, iters, scale)
    M = stabilizing_transforms(m, radius, crop, size=(H, W))
    video, valid = _warp(ts, descs, M, capi.DTYPE_F64, layout, out_dtype)
    return Stabilized(video, valid, M, m.motion, m.ok, flow, timing)


# ---- spatially varying stabilization: per-vertex motion profiles and a mesh warp (SteadyFlow / MeshFlow)
MAX_CELLS = capi.MESH_MAX_CELLS  # include/papof.h: PAPOF_MESH_MAX_CELLS
GRID = (16, 16)
MIN_SUPPORT = 16


def _check_grid(grid, H, W):
    """(GH, GW) of a `grid` argument: integers with 1 <= GH <= min(MAX_CELLS, H - 1), 1 <= GW <= min(MAX_CELLS, W - 1)"""
    try:
        gh, gw = grid
    except (TypeError, ValueError):
        raise TypeError("grid must be (GH, GW), got %r" % (grid,)) from None
    for v in (gh, gw):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("grid must be two integers, got %r" % (grid,))
    if not (1 <= gh <= min(MAX_CELLS, H - 1) and 1 <= gw <= min(MAX_CELLS, W - 1)):
        raise ValueError("grid must lie in 1 .. min(%d, H - 1) x 1 .. min(%d, W - 1) for %d x %d frames, got %r"
                         % (MAX_CELLS, MAX_CELLS, H, W, grid))
    return gh, gw


def _check_mesh_motion_args(min_support, spatial):
    _int_at_least("min_support", min_support, 1)
    _check_bool("spatial", spatial)


def _check_plane_occlusion(occlusion, B, H, W, dev):
    """None, or a bool / uint8 mask (B, H, W) or (B, 2, H, W) (channel 0 is read) on `dev`: a uint8 (B, H, W) view"""
    if occlusion is None:
        return None
    torch = _torch()
    if not isinstance(occlusion, torch.Tensor):
        raise TypeError("occlusion must be None or a torch.Tensor, got %s" % type(occlusion).__name__)
    if occlusion.dtype not in (torch.bool, torch.uint8):
        raise TypeError("occlusion must be torch.bool or torch.uint8, got %s" % occlusion.dtype)
    if tuple(occlusion.shape) not in ((B, H, W), (B, 2, H, W)):
        raise ValueError("occlusion must be (B, H, W) = %s or (B, 2, H, W), got %s" % ((B, H, W), tuple(occlusion.shape)))
    if occlusion.device != dev:
        raise ValueError("occlusion is on %s, the flow on %s: both must be on one device" % (occlusion.device, dev))
    occ = occlusion.view(torch.uint8)
    return occ[:, 0] if occ.dim() == 4 else occ


def _check_pair_matrices(motion, B, dev):
    """None, or the pairs' (B, 2, 3) float64 matrices on `dev` of a tensor or a Motion (pairs with ok False: the identity,
    replaced on the device without a wait)"""
    if motion is None:
        return None
    torch = _torch()
    ok = None
    if isinstance(motion, Motion):
        motion, ok = motion.motion, motion.ok
    if not isinstance(motion, torch.Tensor):
        raise TypeError("motion must be None, a torch.Tensor or a Motion, got %s" % type(motion).__name__)
    if motion.dtype != torch.float64:
        raise TypeError("motion must be float64, got %s" % motion.dtype)
    if tuple(motion.shape) != (B, 2, 3):
        raise ValueError("motion must be (B, 2, 3) = %s, got %s" % ((B, 2, 3), tuple(motion.shape)))
    if motion.device != dev:
        raise ValueError("motion is on %s, the flow on %s: both must be on one device" % (motion.device, dev))
    if ok is not None:
        if not isinstance(ok, torch.Tensor) or tuple(ok.shape) != (B,) or ok.device != dev:
            raise ValueError("a Motion's ok must be (B,) = %s on the flow's device" % ((B,),))
        eye = torch.eye(2, 3, dtype=torch.float64, device=dev)
        motion = torch.where(ok.to(torch.bool).reshape(B, 1, 1), motion, eye)
    return motion


def _vertex_struct(t):
    """the descriptor (item, vertex row, vertex column, component) of a (N, GH + 1, GW + 1, 2) float64 tensor"""
    return _struct(t, tuple(t.stride(i) for i in range(4)), capi.DTYPE_F64)


def _mesh_motion(flow, code, occ, mats, gh, gw, min_support, spatial):
    torch = _torch()
    B, _, H, W = (int(x) for x in flow.shape)
    dev = flow.device
    vertices = torch.empty((B, gh + 1, gw + 1, 2), dtype=torch.float64, device=dev)
    residuals = torch.empty((B, gh + 1, gw + 1, 2), dtype=torch.float64, device=dev)
    support = torch.empty((B, gh + 1, gw + 1), dtype=torch.int32, device=dev)
    d_flow = _flow_struct(flow, code)
    d_occ = _struct(occ, (occ.stride(0), occ.stride(1), occ.stride(2), 0), capi.DTYPE_U8) if occ is not None else None
    d_m = _struct(mats, (mats.stride(0), mats.stride(1), mats.stride(2), 0), capi.DTYPE_F64) if mats is not None else None
    d_v, d_r = _vertex_struct(vertices), _vertex_struct(residuals)
    _launch(dev, "papof_mesh_motion_tensor", B, H, W, ctypes.byref(d_flow), _ref(d_occ), _ref(d_m), gh, gw, min_support,
            1 if spatial else 0, ctypes.byref(d_v), ctypes.byref(d_r), ctypes.c_void_p(support.data_ptr()),
            workspace=("papof_mesh_workspace", (B, gh, gw), "a %d x %d grid is too large for mesh_motion" % (gh, gw)))
    return MeshMotion(vertices, support, residuals)


def mesh_motion(flow, *, motion=None, occlusion=None, grid=GRID, min_support=MIN_SUPPORT, spatial=True):
    """The robust motion of each pair's flow at the vertices of a coarse mesh (the motion profiles' increments of SteadyFlow /
    MeshFlow): flow (B, 2, H, W) float32 / float64 on a HIP device, any strides; motion None or the pairs' global motions --
    a (B, 2, 3) float64 tensor (global_motion's) or a Motion, whose pairs with ok False enter as the identity --; occlusion
    None or a bool / uint8 mask (B, H, W), or the (B, 2, H, W) mask of flow_video_fb (channel 0 is read).  grid = (GH, GW)
    cells, 1 <= GH <= min(64, H - 1), 1 <= GW <= min(64, W - 1); vertex (i, j) sits at (j (W - 1) / GW, i (H - 1) / GH).
    Per vertex, the lower median per component of the residual flow - (A q - q) over the pixels within one cell of the vertex
    -- sampled on a lattice so that a window holds at most 1024, leaving out pixels whose flow is not finite, leaves the image
    or is occluded --; a vertex with fewer than min_support samples is invalid.  spatial=True replaces every vertex's
    residual by the lower median of the valid ones in its 3 x 3 vertex neighbourhood (an invalid vertex with no valid
    neighbour: 0, it follows the global motion); spatial=False gives invalid vertices 0 directly.  Returns
    MeshMotion(vertices (B, GH + 1, GW + 1, 2) float64 -- residual plus A v - v at the vertex --, support (B, GH + 1, GW + 1)
    int32 -- the samples of the vertex's window --, residuals (B, GH + 1, GW + 1, 2) float64).  include/papof.h
    (papof_mesh_motion_tensor) states the rule exactly; no atomics, bitwise reproducible, a pair's rows the same alone and
    in a batch.  Enqueued on the current stream; returns without waiting."""
    code = _check_flow("flow", flow)
    B, _, H, W = (int(x) for x in flow.shape)
    gh, gw = _check_grid(grid, H, W)
    _check_mesh_motion_args(min_support, spatial)
    occ = _check_plane_occlusion(occlusion, B, H, W, flow.device)
    if not _on_gpu(flow):
        raise ValueError("flow must be on a HIP device (cuda:N), got %s" % flow.device)
    mats = _check_pair_matrices(motion, B, flow.device)
    return _mesh_motion(flow, code, occ, mats, gh, gw, min_support, spatial)


def mesh_profiles(residuals, radius):
    """mesh_transforms on a numpy (T - 1, GH + 1, GW + 1, 2) float64 array of per-pair vertex residuals: the displacement
    tables (T, GH + 1, GW + 1, 2) float64.  C(0) = 0, C(t + 1) = C(t) + r(t) (the profile AT a vertex, not a trajectory);
    S(t) = sum_k g_k C(t + k) / sum_k g_k with path_transforms's weights g_k = exp(-k^2 / (2 (radius / 2)^2)), k in
    [-radius, radius] within the video; D(t) = C(t) - S(t).  radius = 0: D = 0 exactly."""
    return _profile_tables(_accumulated_profiles(residuals), radius)


def _accumulated_profiles(residuals):
    """C of mesh_profiles: (T, GH + 1, GW + 1, 2) float64, C(0) = 0, C(t + 1) = C(t) + r(t)"""
    import numpy as np
    r = np.asarray(residuals, np.float64)
    n = r.shape[0] + 1
    C = np.zeros((n,) + r.shape[1:])
    for t in range(n - 1):
        C[t + 1] = C[t] + r[t]
    return C


def _profile_tables(C, radius):
    """D of mesh_profiles from the accumulated profiles C"""
    import numpy as np
    n = C.shape[0]
    D = np.zeros_like(C)
    if radius == 0:
        return D
    for t in range(n):
        ks = range(max(-radius, -t), min(radius, n - 1 - t) + 1)
        g = [math.exp(-k * k / (2.0 * (radius / 2.0) ** 2)) for k in ks]
        S = sum(gk * C[t + k] for gk, k in zip(g, ks)) / sum(g)
        D[t] = C[t] - S
    return D


def _check_residuals(mesh_motion):
    r = mesh_motion.residuals if isinstance(mesh_motion, MeshMotion) else mesh_motion
    if not isinstance(r, _torch().Tensor):
        raise TypeError("mesh_motion must be a MeshMotion or a torch.Tensor of residuals, got %s" % type(r).__name__)
    if r.dim() != 4 or r.shape[3] != 2 or r.shape[0] < 1 or r.shape[1] < 2 or r.shape[2] < 2:
        raise ValueError("the residuals must be (T - 1, GH + 1, GW + 1, 2) with T >= 2, got shape %s" % (tuple(r.shape),))
    return r


def mesh_transforms(mesh_motion, radius=15):
    """The displacement tables that stabilize a video of T frames whose consecutive pairs' vertices move by `mesh_motion` --
    a MeshMotion, or its residuals (T - 1, GH + 1, GW + 1, 2) -- beyond the global motion: the residuals alone are used
    (vertices minus A v - v; the global part is stabilizing_transforms's).  In float64 on the host (one small copy from the
    device: a wait), mesh_profiles: the residuals accumulate to a profile per vertex, the profile is smoothed by the
    Gaussian of stabilizing_transforms, and the table is profile minus smoothed profile.  Returns (T, GH + 1, GW + 1, 2)
    float64 on the motion's device, for warp_mesh."""
    r = _check_residuals(mesh_motion)
    if isinstance(radius, bool) or not isinstance(radius, int) or radius < 0:
        raise ValueError("radius must be an integer >= 0, got %r" % (radius,))
    D = mesh_profiles(r.detach().to("cpu", _torch().float64).numpy(), radius)
    return _torch().from_numpy(D).to(r.device)


def _check_mesh(mesh, n, dev, H, W):
    """a (n, GH + 1, GW + 1, 2) float64 table on `dev` whose grid fits H x W frames: (GH, GW)"""
    torch = _torch()
    if not isinstance(mesh, torch.Tensor):
        raise TypeError("mesh must be a torch.Tensor, got %s" % type(mesh).__name__)
    if mesh.dtype != torch.float64:
        raise TypeError("mesh must be float64, got %s" % mesh.dtype)
    if mesh.dim() != 4 or mesh.shape[0] != n or mesh.shape[3] != 2:
        raise ValueError("mesh must be (B, GH + 1, GW + 1, 2) with B = %d, got shape %s" % (n, tuple(mesh.shape)))
    if mesh.device != dev:
        raise ValueError("mesh is on %s, the frames on %s: both must be on one device" % (mesh.device, dev))
    return _check_grid((int(mesh.shape[1]) - 1, int(mesh.shape[2]) - 1), H, W)


def _warp_mesh(ts, descs, matrices, m_code, mesh, gh, gw, layout, out_dtype):
    torch = _torch()
    (B, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(B, H, W, C, layout, out_dtype, dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], descs[0][1], descs[0][2])
    d_mat = _struct(matrices, (matrices.stride(0), matrices.stride(1), matrices.stride(2), 0), m_code)
    d_mesh = _vertex_struct(mesh)
    d_valid = _struct(valid, (valid.stride(0), valid.stride(1), valid.stride(2), 1), capi.DTYPE_U8)
    _launch(dev, "papof_warp_mesh_tensor", B, H, W, C, ctypes.byref(d_in), ctypes.byref(d_mat), ctypes.byref(d_mesh), gh, gw,
            ctypes.byref(d_out), ctypes.byref(d_valid))
    return out, valid.view(torch.bool)


def warp_mesh(frames, matrices, mesh, *, layout="NCHW", out_dtype=None):
    """warp_affine with a spatially varying displacement: output pixel q of frame i is frames[i] sampled at M q + d, d the
    bilinear interpolation of the frame's table mesh[i] -- mesh (B, GH + 1, GW + 1, 2) float64 (dx, dy) on the frames'
    device, any strides, the vertices of mesh_motion's mesh -- at the mesh coordinates of M q, clamped to the mesh.  frames,
    matrices, layout, out_dtype and the result (frames_out, valid (B, H, W) bool) as warp_affine's; a table of +0.0 gives
    warp_affine's bytes.  The displacement is looked up at the sampling point, not at the moved vertex: the backward
    approximation of MeshFlow's forward mesh render, different at second order in the displacement's gradient.
    include/papof.h (papof_warp_mesh_tensor) states the rule exactly.  Enqueued on the current stream; returns without
    waiting."""
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    (B, H, W, _), _, _ = descs[0]
    m_code = _check_matrices(matrices, B, ts[0].device)
    gh, gw = _check_mesh(mesh, B, ts[0].device, H, W)
    return _warp_mesh(ts, descs, matrices, m_code, mesh, gh, gw, layout, out_dtype)


def stabilize_video_mesh(frames, pyramidLevels, *, grid=GRID, radius=15, crop=1.0, model="similarity", iters=5, scale=1.0,
                         min_support=MIN_SUPPORT, spatial=True, consistency=CONSISTENCY, layout="NCHW", out_dtype=None,
                         **solver):
    """stabilize_video for shake that varies across the image (parallax, rolling shutter): flow_video_fb(frames,
    pyramidLevels, consistency=consistency, layout=layout, **solver) (float64 flows and the occlusion mask; with
    consistency=None, flow_video and no mask), global_motion on the forward flows (model, iters, scale), mesh_motion(flow_fw,
    motion=, occlusion=, grid=, min_support=, spatial=), stabilizing_transforms (radius, crop) and mesh_transforms (radius) --
    the waits, where stabilize_video waits -- and ONE warp_mesh.  Returns MeshStabilized(video, valid, transforms, motion, ok,
    flow, timing as stabilize_video's, mesh (T, GH + 1, GW + 1, 2) float64: the displacement tables, vertex_motion
    (T - 1, GH + 1, GW + 1, 2): mesh_motion's vertices, support (T - 1, GH + 1, GW + 1) int32).  With radius=0 the video and
    valid are stabilize_video's.  The base matrix is affine, the borders are not filled (stabilize_video_mesh_full fills
    them), the smoothing is neither causal nor adaptive (README).  Every argument error raises before anything is launched; the video is enqueued on the current
    stream."""
    p = _mesh_stabilizer(frames, pyramidLevels, grid, radius, crop, model, iters, scale, min_support, spatial, consistency, layout,
                         out_dtype, solver)
    D = mesh_transforms(p.mm, radius)
    video, valid = _warp_mesh(p.ts, p.descs, p.M, capi.DTYPE_F64, D, *p.grid, layout, p.out_dtype)
    return MeshStabilized(video, valid, p.M, p.m.motion, p.m.ok, p.flow, p.timing, D, p.mm.vertices, p.mm.support)


_MeshStabilizer = collections.namedtuple("_MeshStabilizer", "ts descs grid out_dtype flow timing m mm M")


def _mesh_stabilizer(frames, pyramidLevels, grid, radius, crop, model, iters, scale, min_support, spatial, consistency, layout,
                     out_dtype, solver, check=None):
    """stabilize_video_mesh and stabilize_video_mesh_full up to their last call: the argument checks (`check`: one more, of
    the frames' descriptors, before anything is launched), the flows, the global motion m, the mesh motion mm and the
    sampling matrices M"""
    ts, descs, _, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    code, iters, scale = _check_fit(model, iters, scale)
    (T, H, W, C), _, _ = descs[0]
    _check_path(radius, crop, (H, W))
    gh, gw = _check_grid(grid, H, W)
    _check_mesh_motion_args(min_support, spatial)
    alphas = _alphas(consistency)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    if check is not None:
        check()
    f64 = _torch().float64
    if alphas[0]:
        fb = _run_fb(ts, descs, True, T - 1, layout, f64, pyramidLevels, alphas, params)
        flow, timing, occ = fb.flow_fw, fb.timing, fb.occlusion.view(_torch().uint8)[:, 0]
    else:
        flow, _, timing = _run(ts, descs, True, T - 1, layout, f64, pyramidLevels, params)
        occ = None
    m = _motion_fit(flow, capi.DTYPE_F64, None, code, iters, scale)
    mm = _mesh_motion(flow, capi.DTYPE_F64, occ, _check_pair_matrices(m, T - 1, flow.device), gh, gw, min_support, spatial)
    M = stabilizing_transforms(m, radius, crop, size=(H, W))
    return _MeshStabilizer(ts, descs, (gh, gw), out_dtype, flow, timing, m, mm, M)


MAX_RADIUS = 16  # include/papof.h: papof_temporal_filter_tensor
MAX_CHANNELS = 4


def _check_filter(radius, sigma):
    """(radius, sigma as a float: 0.0 for None) of temporal_filter's keywords -- TypeError / ValueError otherwise"""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError("radius must be an integer in 1 .. %d, got %r" % (MAX_RADIUS, radius))
    if sigma is None:
        return radius, 0.0
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise TypeError("sigma must be None or a number, got %r" % (sigma,))
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError("sigma must be finite and >= 0, got %r" % (sigma,))
    return radius, float(sigma)


def _check_video(frames, layout, levels, out_dtype, name="frames", min_frames=2, solver=None):
    """the frames of the video calls, 1 .. MAX_CHANNELS channels: (ts, descs, out_dtype -- by default the frames' --, the
    solver's params) -- every error before anything is launched"""
    ts, descs, _, params = _check([(name, frames)], layout, None, levels, min_frames=min_frames, solver=solver)
    C = descs[0][0][3]
    if C > MAX_CHANNELS:
        raise ValueError("%s must have 1 .. %d channels, got %d (layout %s)" % (name, MAX_CHANNELS, C, layout))
    return ts, descs, _out_dtype(out_dtype, ts[0].dtype), params


def _filter(ts, descs, flows, codes, radius, sigma, alphas, layout, out_dtype):
    torch = _torch()
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(T, H, W, C, layout, out_dtype, dev)
    support = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], strides, code)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_sup = _struct(support, (support.stride(0), support.stride(1), support.stride(2), 1), capi.DTYPE_U8)
    _launch(dev, "papof_temporal_filter_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_f[0]), ctypes.byref(d_f[1]),
            radius, sigma, *alphas, ctypes.byref(d_out), ctypes.byref(d_sup))
    return Filtered(out, support)


def temporal_filter(frames, flow_fw, flow_bw, *, radius=2, sigma=0.15, consistency=CONSISTENCY, layout="NCHW",
                    out_dtype=None):
    """Motion-compensated temporal denoising of a video of T >= 2 frames: frames (T, C, H, W) or (T, H, W, C) by `layout`,
    C = 1 .. 4, uint8 (read as x / 255), float32 or float64, any strides, on a HIP device; flow_fw, flow_bw (T - 1, 2, H, W)
    float32 / float64 on the same device, pair t from frame t to t + 1 and back, as flow_video_fb returns them.
    Each pixel of frame t follows its chain through the flows to the frames t + 1 .. t + radius and t - 1 .. t - radius
    (radius 1 .. 16), hop by hop as track_points moves a point: a chain ends where it leaves the image or -- consistency =
    (alpha1, alpha2); None: no check -- where the reverse flow does not bring it back.  Every neighbour it reaches enters
    the average with the weight 1 / (1 + D / sigma^2), D the mean squared difference over the channels of its bilinear
    sample and the centre pixel (in [0, 1] units for uint8), so that a neighbour that looks different counts less;
    sigma=None (or 0): every reached neighbour has weight 1.  The centre has weight 1.
    sigma = 0.15, the default, was calibrated on the committed frames with Gaussian noise of standard deviation 10 / 255
    (tests/test_denoise_cpu.py): with radius 1 it raises the middle frame's PSNR by 4.06 dB (240x135) and 4.04 dB (480x270),
    the best of the values tried (0.03 .. 0.2), against 3.98 and 3.90 dB without the photometric weight and 4.77 dB for the
    ideal average of three aligned samples.
    Returns Filtered(video in `layout` and out_dtype -- uint8 as clamp(rint(255 x), 0, 255), float32 or float64; by default
    the frames' dtype --, support (T, H, W) uint8: the number of neighbours that entered).  include/papof.h
    (papof_temporal_filter_tensor) states the rule exactly.  Enqueued on the current stream; returns without waiting."""
    alphas = _alphas(consistency)
    radius, sigma = _check_filter(radius, sigma)
    ts, descs, out_dtype, _ = _check_video(frames, layout, 1, out_dtype)
    (T, H, W, C), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    return _filter(ts, descs, (flow_fw, flow_bw), codes, radius, sigma, alphas, layout, out_dtype)


def denoise_video(frames, pyramidLevels, *, radius=2, sigma=0.15, consistency=CONSISTENCY, layout="NCHW", out_dtype=None,
                  **solver):
    """A video of T >= 2 frames denoised along its motion: flow_video_fb(frames, pyramidLevels, layout=layout,
    consistency=None, out_dtype=torch.float64, **solver) -- both float64 flows of every pair in one launch chain -- followed
    by temporal_filter on them (radius, sigma, consistency).  Returns Denoised(video, support (T, H, W) uint8, flow_fw,
    flow_bw (T - 1, 2, H, W) float64, timing of the flow call).  Every argument error raises before anything is launched;
    the flows are complete on return, the video is enqueued on the current stream behind them."""
    torch = _torch()
    alphas = _alphas(consistency)
    radius, sigma = _check_filter(radius, sigma)
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    T = descs[0][0][0]
    fb = _run_fb(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, _alphas(None), params)
    f = _filter(ts, descs, (fb.flow_fw, fb.flow_bw), (capi.DTYPE_F64, capi.DTYPE_F64), radius, sigma, alphas, layout,
                out_dtype)
    return Denoised(f.video, f.support, fb.flow_fw, fb.flow_bw, fb.timing)


MAX_SAMPLES = 64  # include/papof.h: papof_motion_blur_tensor
MIN_OFFSET = 2.0 ** -20
SHAPES = ("box", "triangle")


def blur_schedule(shutter=0.5, samples=16, phase=-0.5, shape="box"):
    """The shutter of motion_blur as (offsets, weights), two lists of `samples` floats, computed on the host: sample k is
    taken at tau_k = shutter * ((k + 0.5) / samples + phase) frames from the frame (in that order in float64) with the
    weight 1 ("box") or 1 - |2 (k + 0.5) / samples - 1| ("triangle").  shutter: the exposure in frame intervals, in (0, 1];
    phase: where it opens, in shutters, in [-1, 0] -- -0.5 is centred on the frame, 0 opens at the frame, -1 closes at it;
    samples: an integer in 1 .. 64.  ValueError for anything else, and for a schedule with an offset that
    papof_motion_blur_tensor refuses (neither 0 nor of a magnitude in [2^-20, 1 - 2^-20])."""
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
        raise ValueError("samples must be an integer in 1 .. %d, got %r" % (MAX_SAMPLES, samples))
    for name, v in (("shutter", shutter), ("phase", phase)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
    shutter, phase = float(shutter), float(phase)
    if not 0.0 < shutter <= 1.0:
        raise ValueError("shutter must lie in (0, 1], got %r" % shutter)
    if not -1.0 <= phase <= 0.0:
        raise ValueError("phase must lie in [-1, 0], got %r" % phase)
    if shape not in SHAPES:
        raise ValueError("shape must be one of %s, got %r" % (SHAPES, shape))
    offsets = [shutter * ((k + 0.5) / samples + phase) for k in range(samples)]
    if shape == "box":
        weights = [1.0] * samples
    else:
        weights = [1.0 - abs(2.0 * (k + 0.5) / samples - 1.0) for k in range(samples)]
    for tau in offsets:
        if tau != 0.0 and not MIN_OFFSET <= abs(tau) <= 1.0 - MIN_OFFSET:
            raise ValueError("the schedule has the offset %r: neither 0 nor of a magnitude in [2^-20, 1 - 2^-20]" % tau)
    return offsets, weights


def _blur(ts, descs, flows, codes, occlusion, schedule, layout, out_dtype):
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    offsets, weights = schedule
    out, d_out = _new_frames(T, H, W, C, layout, out_dtype, dev)
    d_in = _struct(ts[0], strides, code)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_occ = _flow_struct(occlusion, capi.DTYPE_U8) if occlusion is not None else None
    n = len(offsets)
    _launch(dev, "papof_motion_blur_tensor", T, ctypes.byref(d_in), H, W, C, ctypes.byref(d_f[0]), ctypes.byref(d_f[1]),
            _ref(d_occ), n, (ctypes.c_double * n)(*offsets), (ctypes.c_double * n)(*weights), ctypes.byref(d_out))
    return out


def motion_blur(frames, flow_fw, flow_bw, *, shutter=0.5, samples=16, phase=-0.5, shape="box", occlusion=None, layout="NCHW",
                out_dtype=None):
    """Synthetic motion blur of a video of T >= 2 frames along its flows -- a longer shutter for a video shot, rendered or
    retimed with a short one: frames (T, C, H, W) or (T, H, W, C) by `layout`, uint8 (read as x / 255), float32 or float64,
    any strides, on a HIP device; flow_fw, flow_bw (T - 1, 2, H, W) float32 / float64 on the same device, pair t from frame t
    to t + 1 and back, and occlusion None or their (T - 1, 2, H, W) bool / uint8 mask, as flow_video_fb returns them.
    Every output pixel is the weighted mean of the scene at the `samples` times of blur_schedule(shutter, samples, phase,
    shape) around its frame; the scene at an in-between time is what interpolate makes of the pair that holds that time
    (pair (t, t + 1) after the frame, (t - 1, t) before it), and at offset 0 the frame itself.  All of it happens in one HIP
    kernel whose sums stay in registers.  The first frame has no pair before it and the last none after it: their samples on
    that side are dropped, so the end frames get a one-sided shutter (a frame with no sample left is returned as it is).
    It is the gather rule (the flows are read at the output pixel): at a motion boundary a sample reads the wrong flow, as
    interpolate(method="gather") does.  It adds blur and removes none.
    Returns a new tensor of the frames' shape in `layout` and out_dtype -- uint8 as clamp(rint(255 x), 0, 255), float32 or
    float64; by default the frames' dtype.  include/papof.h (papof_motion_blur_tensor) states the rule exactly.  Enqueued on
    the current stream; returns without waiting."""
    schedule = blur_schedule(shutter, samples, phase, shape)
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1, min_frames=2)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    (T, H, W, C), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    occ = _check_occlusion(occlusion, (T - 1, 2, H, W), ts[0].device)
    return _blur(ts, descs, (flow_fw, flow_bw), codes, occ, schedule, layout, out_dtype)


def blur_video(frames, pyramidLevels, *, shutter=0.5, samples=16, phase=-0.5, shape="box", layout="NCHW", out_dtype=None,
               consistency=CONSISTENCY, **solver):
    """A video of T >= 2 frames with a longer shutter: flow_video_fb(frames, pyramidLevels, layout=layout,
    consistency=consistency, **solver) -- float64 flows whatever out_dtype is -- followed by motion_blur on its flows and
    mask (None for consistency=None: no mask).  Returns Blurred(video, flow_fw, flow_bw, occlusion, timing of the flow call).
    Every argument error raises before anything is launched; the flows are complete on return, the video is enqueued on the
    current stream behind them."""
    torch = _torch()
    alphas = _alphas(consistency)
    schedule = blur_schedule(shutter, samples, phase, shape)
    ts, descs, _, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    T = descs[0][0][0]
    fb = _run_fb(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, alphas, params)
    occ = fb.occlusion.view(torch.uint8) if fb.occlusion is not None else None
    video = _blur(ts, descs, (fb.flow_fw, fb.flow_bw), (capi.DTYPE_F64, capi.DTYPE_F64), occ, schedule, layout, out_dtype)
    return Blurred(video, fb.flow_fw, fb.flow_bw, fb.occlusion, fb.timing)


MAX_DEBLUR_RADIUS = 4  # include/papof.h: papof_deblur_tensor
MAX_DEBLUR_ITERS = 256
MAX_DEBLUR_PASSES = 8
DEBLUR_ITERS = 6  # tests/test_deblur_cpu.py: with exact flows the gain peaks at 5 .. 6 iterations and falls behind them


def _check_deblur(radius, iters):
    return _int_in("radius", radius, 0, MAX_DEBLUR_RADIUS), _int_in("iters", iters, 1, MAX_DEBLUR_ITERS)


def _deblur(ts, descs, flows, codes, schedule, radius, iters, alphas, layout, out_dtype):
    torch = _torch()
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    offsets, weights = schedule
    out, d_out = _new_frames(T, H, W, C, layout, out_dtype, dev)
    support = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], strides, code)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_sup = _struct(support, (support.stride(0), support.stride(1), support.stride(2), 1), capi.DTYPE_U8)
    n = len(offsets)
    _launch(dev, "papof_deblur_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_f[0]), ctypes.byref(d_f[1]), n,
            (ctypes.c_double * n)(*offsets), (ctypes.c_double * n)(*weights), radius, iters, *alphas, ctypes.byref(d_out),
            ctypes.byref(d_sup),
            workspace=("papof_deblur_workspace", (T, H, W, C, radius),
                       "%d frames of %d x %d x %d are too large to deblur" % (T, H, W, C)))
    return Deblurred(out, support)


def deblur(frames, flow_fw, flow_bw, *, shutter=0.5, samples=16, phase=-0.5, shape="box", radius=1, iters=DEBLUR_ITERS,
           consistency=CONSISTENCY, layout="NCHW", out_dtype=None):
    """Deblurring of a video of T >= 2 frames along its flows -- the inverse of motion_blur, for footage whose shutter was
    open while the camera shook: frames (T, C, H, W) or (T, H, W, C) by `layout`, C = 1 .. 4, uint8 (read as x / 255),
    float32 or float64, any strides, on a HIP device; flow_fw, flow_bw (T - 1, 2, H, W) float32 / float64 on the same device,
    pair t from frame t to t + 1 and back, as flow_video_fb returns them.
    It is multi-frame Richardson-Lucy deconvolution (Richardson 1972, Lucy 1974; along motion paths Tai, Tan and Brown 2011;
    for video Kim and Lee 2015).  Every frame is taken to be the scene averaged over the times of blur_schedule(shutter,
    samples, phase, shape) along a straight line per pixel, its velocity -- half the difference of the forward and the
    backward flow -- times the sample's time.  Each of the `iters` (1 .. 256) iterations blurs the current estimate of a
    frame as each of the frames t, t +- 1 .. t +- radius (radius 0 .. 4) would have recorded it -- carried there along the
    chain of flows, hop by hop as temporal_filter does, a chain ending where it leaves the image or fails consistency =
    (alpha1, alpha2) (None: no check) --, divides the recorded frames by that, and multiplies the estimate by the mean over
    the frames of the ratios blurred backwards.  Two HIP kernels per iteration, fp64, bitwise reproducible.
    Measured on a shaking camera (tests/test_deblur_cpu.py: 7 frames, shutter 0.5, speeds of 2 .. 7 pixels per frame, uint8)
    with exact flows: 25.6 dB blurred, 36.4 dB after 6 iterations with radius 1, 40.0 dB with radius 2 and 26.8 dB with
    radius 0; with flows estimated on the blurred frames 30.7 dB.  The iterations are few on purpose: there is no prior, and
    beyond the default the result gets worse again (34.3 dB at 12).
    What it is not: the shutter is given, not estimated; one straight line per pixel and frame, so a path that curves inside
    the exposure is modelled only through the neighbours; the backward blur reads the velocity where it lands (the gather
    adjoint), which is wrong at motion boundaries; a steady pan, where every frame carries the same blur, gains little
    (2.6 dB at 8 iterations); ringing and noise grow with the iterations and there is no regulariser; the flows come from
    blurred frames.
    Returns Deblurred(video in `layout` and out_dtype -- uint8 as clamp(rint(255 x), 0, 255), float32 or float64; by default
    the frames' dtype --, support (T, H, W) uint8: the number of frames that entered a pixel's last update).
    include/papof.h (papof_deblur_tensor) states the rule exactly.  The workspace comes from PyTorch's allocator; enqueued
    on the current stream, returns without waiting."""
    alphas = _alphas(consistency)
    schedule = blur_schedule(shutter, samples, phase, shape)
    radius, iters = _check_deblur(radius, iters)
    ts, descs, out_dtype, _ = _check_video(frames, layout, 1, out_dtype)
    (T, H, W, C), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    return _deblur(ts, descs, (flow_fw, flow_bw), codes, schedule, radius, iters, alphas, layout, out_dtype)


def deblur_video(frames, pyramidLevels, *, passes=1, shutter=0.5, samples=16, phase=-0.5, shape="box", radius=1,
                 iters=DEBLUR_ITERS, consistency=CONSISTENCY, layout="NCHW", out_dtype=None, **solver):
    """A video of T >= 2 frames deblurred along its motion, `passes` (1 .. 8) passes: pass 0 is flow_video_fb(frames,
    pyramidLevels, layout=layout, consistency=consistency, out_dtype=torch.float64, **solver) followed by deblur on those
    flows; every later pass estimates the flows again on the previous pass's video -- sharper frames, better flows -- and
    runs deblur on the ORIGINAL frames with them (restore_video's pattern).  Returns DeblurredVideo(video, support, flow_fw,
    flow_bw (T - 1, 2, H, W) float64, occlusion and timing of the last flow call).  Every argument error raises before
    anything is launched; the flows are complete on return, the video is enqueued on the current stream behind them."""
    torch = _torch()
    alphas = _alphas(consistency)
    passes = _int_in("passes", passes, 1, MAX_DEBLUR_PASSES)
    schedule = blur_schedule(shutter, samples, phase, shape)
    radius, iters = _check_deblur(radius, iters)
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    T = descs[0][0][0]
    codes = (capi.DTYPE_F64, capi.DTYPE_F64)
    d = None
    for k in range(passes):
        src = ts if d is None else [d.video]
        fb = _run_fb(src, [descriptor(src[0], layout)], True, T - 1, layout, torch.float64, pyramidLevels, alphas, params)
        d = _deblur(ts, descs, (fb.flow_fw, fb.flow_bw), codes, schedule, radius, iters, alphas, layout,
                    out_dtype if k == passes - 1 else ts[0].dtype)
    return DeblurredVideo(d.video, d.support, fb.flow_fw, fb.flow_bw, fb.occlusion, fb.timing)


MAX_RELAX = 65536  # include/papof.h: papof_fill_holes_tensor
RELAX = 0  # Jacobi sweeps per level of fill_holes: calibrated in tests/test_inpaint_cpu.py (test_quality_calibration)


def _check_relax(relax):
    if isinstance(relax, bool) or not isinstance(relax, int) or not 0 <= relax <= MAX_RELAX:
        raise ValueError("relax must be an integer in 0 .. %d, got %r" % (MAX_RELAX, relax))
    return relax


def _check_masks(name, masks, n, H, W, dev):
    """(n, H, W) bool / uint8 masks on `dev` (2-D: one frame) as uint8 -- TypeError / ValueError otherwise"""
    torch = _torch()
    if not isinstance(masks, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(masks).__name__))
    if masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError("%s must be torch.bool or torch.uint8, got %s" % (name, masks.dtype))
    if masks.dim() == 2:
        masks = masks.unsqueeze(0)
    if tuple(masks.shape) != (n, H, W):
        raise ValueError("%s must be (N, H, W) = %s, got %s" % (name, (n, H, W), tuple(masks.shape)))
    if masks.device != dev:
        raise ValueError("%s is on %s, the frames on %s: all must be on one device" % (name, masks.device, dev))
    return masks.view(torch.uint8)


def _mask_struct(m):
    return _struct(m, (m.stride(0), m.stride(1), m.stride(2), 0), capi.DTYPE_U8)


def _fill(t, desc, mask, relax, layout, out_dtype):
    """papof_fill_holes_tensor of the 4-D tensor t (its descriptor `desc` in `layout`) under the uint8 mask: a new tensor"""
    (n, H, W, C), strides, code = desc
    out, d_out = _new_frames(n, H, W, C, layout, out_dtype, t.device)
    d_in = _struct(t, strides, code)
    d_mask = _mask_struct(mask)
    _launch(t.device, "papof_fill_holes_tensor", n, H, W, C, ctypes.byref(d_in), ctypes.byref(d_mask), relax,
            ctypes.byref(d_out), workspace=("papof_fill_workspace", (n, H, W, C),
                                            "%d frames of %d x %d x %d are too large for fill_holes" % (n, H, W, C)))
    return out


def fill_holes(x, mask, *, layout="NCHW", relax=RELAX, out_dtype=None):
    """A field filled inside a mask: x (N, C, H, W) or (N, H, W, C) by `layout` (3-D: one frame), C = 1 .. 4, uint8 (read
    as x / 255), float32 or float64, any strides, on a HIP device; mask (N, H, W) (2-D: one frame) bool / uint8 on the same
    device, nonzero (True) marking a hole.  Each frame's holes are filled by pull-push (Gortler et al. 1996): a pyramid of
    the known pixels' means down to 1 x 1, then from coarse to fine every unknown pixel takes the bilinear sample of the
    filled coarser level, followed by `relax` Jacobi sweeps (0 .. 65536) of the 4-neighbour average over the unknown pixels
    of each level.  A frame with no known pixel comes out as zeros.  Pixels outside the mask are stored from their input
    value (out_dtype == x's dtype: x's bytes).  Returns the filled tensor in `layout` and out_dtype (uint8 as
    clamp(rint(255 v), 0, 255), float32 or float64; by default x's dtype).  include/papof.h (papof_fill_holes_tensor)
    states the rule exactly.  The workspace comes from PyTorch's allocator; enqueued on the current stream, returns without
    waiting."""
    relax = _check_relax(relax)
    ts, descs, out_dtype, _ = _check_video(x, layout, 1, out_dtype, name="x", min_frames=1)
    n, H, W, _ = descs[0][0]
    m = _check_masks("mask", mask, n, H, W, ts[0].device)
    return _fill(ts[0], descs[0], m, relax, layout, out_dtype)


def _check_video_masks(ts, descs, masks):
    (T, H, W, _), _, _ = descs[0]
    return _check_masks("masks", masks, T, H, W, ts[0].device)


def _complete(flows, m, relax):
    return Flows(*(_fill(f, descriptor(f, "NCHW"), mk, relax, "NCHW", f.dtype) for f, mk in zip(flows, (m[:-1], m[1:]))))


def complete_flows(flow_fw, flow_bw, masks, *, relax=RELAX):
    """The flows of a video of T frames with the moving object under `masks` removed: flow_fw, flow_bw (T - 1, 2, H, W)
    float32 / float64 on a HIP device, pair t from frame t to t + 1 and back, as flow_video_fb returns them; masks
    (T, H, W) bool / uint8 on the same device.  flow_fw[t] is filled (fill_holes, relax) under masks[t], flow_bw[t] under
    masks[t + 1].  Returns Flows(flow_fw, flow_bw): new tensors of the flows' dtypes; enqueued on the current stream."""
    relax = _check_relax(relax)
    torch = _torch()
    if not isinstance(masks, torch.Tensor):
        raise TypeError("masks must be a torch.Tensor, got %s" % type(masks).__name__)
    _check_flows(flow_fw, flow_bw)
    T, H, W = int(flow_fw.shape[0]) + 1, int(flow_fw.shape[2]), int(flow_fw.shape[3])
    m = _check_masks("masks", masks, T, H, W, flow_fw.device)
    return _complete((flow_fw, flow_bw), m, relax)


def _check_radius(radius, T):
    if radius is None:
        return T - 1
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= T - 1:
        raise ValueError("radius must be None or an integer in 1 .. T - 1 = %d, got %r" % (T - 1, radius))
    return radius


def _propagate(ts, descs, m, flows, codes, radius, alphas, layout, out_dtype):
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(T, H, W, C, layout, out_dtype, dev)
    status = _torch().empty((T, H, W), dtype=_torch().uint8, device=dev)
    d_in = _struct(ts[0], strides, code)
    d_m = _mask_struct(m)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_st = _mask_struct(status)
    _launch(dev, "papof_propagate_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_m), ctypes.byref(d_f[0]),
            ctypes.byref(d_f[1]), radius, *alphas, ctypes.byref(d_out), ctypes.byref(d_st))
    return Propagated(out, status)


def propagate(frames, masks, flow_fw, flow_bw, *, radius=None, consistency=None, layout="NCHW", out_dtype=None):
    """The holes of a video of T >= 2 frames filled from other frames along the flows: frames (T, C, H, W) or (T, H, W, C)
    by `layout`, C = 1 .. 4, uint8 (read as x / 255), float32 or float64, any strides, on a HIP device; masks (T, H, W)
    bool / uint8 (nonzero: a hole); flow_fw, flow_bw (T - 1, 2, H, W) float32 / float64 -- completed (complete_flows) --
    pair t from frame t to t + 1 and back.  Each hole pixel of frame t follows its chain forward and backward, hop by hop as
    track_points moves a point (consistency = (alpha1, alpha2); None, the default: no check), up to `radius` frames (None:
    T - 1), and
    stops at the first frame where the four bilinear taps of its position are all outside that frame's mask; the frame
    sampled there is its candidate.  Two candidates are mixed with the weights 1 / distance, one is taken as it is; with none
    the pixel keeps its input value.  Returns Propagated(video in `layout` and out_dtype (by default the frames'), status
    (T, H, W) uint8: 0 not a hole, 1 filled, 2 still a hole).  include/papof.h (papof_propagate_tensor) states the rule
    exactly.  Enqueued on the current stream; returns without waiting.
    The defaults (relax 0, no check) were calibrated on a panning video with a moving occluder and the oracle's flows
    (tests/test_inpaint_cpu.py): inside completed flows the check only shortens the chains -- 34 % of the hole pixels found
    a candidate with it, 99.9 % without -- and inpaint_video's PSNR over the holes was 21.4 dB with it, 29.0 dB without,
    against 17.9 dB for fill_holes alone; Jacobi sweeps lowered it (25.4 dB with 8 per level)."""
    alphas = _alphas(consistency)
    ts, descs, out_dtype, _ = _check_video(frames, layout, 1, out_dtype)
    (T, H, W, _), _, _ = descs[0]
    radius = _check_radius(radius, T)
    m = _check_video_masks(ts, descs, masks)
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    return _propagate(ts, descs, m, (flow_fw, flow_bw), codes, radius, alphas, layout, out_dtype)


def inpaint_video(frames, masks, pyramidLevels, *, flows=None, radius=None, relax=RELAX, consistency=None,
                  layout="NCHW", out_dtype=None, **solver):
    """A video of T >= 2 frames with the regions under `masks` removed (Xu et al. 2019; Gao et al. 2020, without their
    learned parts): flow_video_fb(frames, pyramidLevels, layout=layout, consistency=None, out_dtype=torch.float64, **solver)
    -- or flows = (flow_fw, flow_bw) as it returns them --, complete_flows (relax), propagate (radius, consistency) into
    float64, and fill_holes (relax) of the pixels that are still holes.  masks: (T, H, W) bool / uint8 on the frames'
    device; dilate them by a few pixels: the object's motion bleeds into the flows just outside it.  Returns
    Inpainted(video in `layout` and out_dtype (by default the frames'; pixels outside the masks are their input values, of
    the frames' dtype: their bytes), status (T, H, W) uint8: 0 kept, 1 filled along the flows, 2 filled spatially).  Every
    argument error raises before anything is launched; the video is enqueued on the current stream."""
    torch = _torch()
    alphas = _alphas(consistency)
    relax = _check_relax(relax)
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    (T, H, W, _), _, _ = descs[0]
    radius = _check_radius(radius, T)
    m = _check_video_masks(ts, descs, masks)
    flow_fw, flow_bw, codes, _ = _given_or_run_fb(flows, ts, descs, layout, pyramidLevels, params)
    cf = _complete((flow_fw, flow_bw), m, relax)
    p = _propagate(ts, descs, m, cf, codes, radius, alphas, layout, torch.float64)
    video = _fill(p.video, descriptor(p.video, layout), (p.status == 2).view(torch.uint8), relax, layout, out_dtype)
    return Inpainted(video, p.status)


def _given_or_run_fb(flows, ts, descs, layout, levels, params):
    """the flows of the video ts[0]: flows = (flow_fw, flow_bw) checked against it -- the last argument check of its caller --
    or, for None, flow_video_fb's float64 flows without a mask.  Returns (flow_fw, flow_bw, their dtype codes, the timing of
    the flow call or None)."""
    (T, H, W, _), _, _ = descs[0]
    if flows is not None:
        if not isinstance(flows, (tuple, list)) or len(flows) != 2:
            raise TypeError("flows must be None or a pair (flow_fw, flow_bw), got %s" % type(flows).__name__)
        return (*flows, _check_flows(*flows, (T - 1, 2, H, W), ts[0].device), None)
    fb = _run_fb(ts, descs, True, T - 1, layout, _torch().float64, levels, _alphas(None), params)
    return fb.flow_fw, fb.flow_bw, (capi.DTYPE_F64, capi.DTYPE_F64), fb.timing


MAX_DILATE = 32  # include/papof.h: papof_mask_dilate_tensor
# the defaults of the defect calls: calibrated in tests/test_restore_cpu.py (test_quality_calibration)
DEFECT_THRESHOLD = 0.08
DEFECT_DILATE = 2
DEFECT_PASSES = 2
MAX_PASSES = 8


def _check_threshold(threshold):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise TypeError("threshold must be a number, got %r" % (threshold,))
    if not (math.isfinite(threshold) and threshold >= 0):
        raise ValueError("threshold must be finite and >= 0, got %r" % (threshold,))
    return float(threshold)


def _check_dilate(name, radius):
    return _int_in(name, radius, 0, MAX_DILATE)


def _detect(ts, descs, flows, codes, threshold, alphas):
    """papof_defect_detect_tensor of the checked video ts[0] on the flows: Defects(mask bool, score float64, support uint8)"""
    torch = _torch()
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    mask = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    score = torch.empty((T, H, W), dtype=torch.float64, device=dev)
    support = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], strides, code)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_m, d_sup = _mask_struct(mask), _mask_struct(support)
    d_sc = _struct(score, (score.stride(0), score.stride(1), score.stride(2), 0), capi.DTYPE_F64)
    _launch(dev, "papof_defect_detect_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_f[0]), ctypes.byref(d_f[1]),
            threshold, *alphas, ctypes.byref(d_m), ctypes.byref(d_sc), ctypes.byref(d_sup))
    return Defects(mask.view(torch.bool), score, support)


def _dilate(m, radius):
    """papof_mask_dilate_tensor of the uint8 masks m (T, H, W): a new uint8 tensor of 0 / 1"""
    T, H, W = (int(s) for s in m.shape)
    out = _torch().empty((T, H, W), dtype=_torch().uint8, device=m.device)
    d_m, d_out = _mask_struct(m), _mask_struct(out)
    _launch(m.device, "papof_mask_dilate_tensor", T, H, W, ctypes.byref(d_m), radius, ctypes.byref(d_out))
    return out


def detect_defects(frames, flow_fw, flow_bw, *, threshold=DEFECT_THRESHOLD, consistency=None, layout="NCHW"):
    """The defects that live in ONE frame of a video of T >= 3 frames -- film dirt and sparkle, analogue dropouts,
    transmission errors, a bird that crosses one frame -- found along the flows (Kokaram's spike detection index in its
    range form): frames (T, C, H, W) or (T, H, W, C) by `layout`, C = 1 .. 4, uint8 (read as x / 255), float32 or float64,
    any strides, on a HIP device; flow_fw, flow_bw (T - 1, 2, H, W) float32 / float64 on the same device, pair t from frame
    t to t + 1 and back, as flow_video_fb returns them.  Each pixel of frame t is carried to the frames t - 1 and t + 1
    (frame 0: 1 and 2; frame T - 1: T - 2 and T - 3), hop by hop as temporal_filter moves it (consistency = (alpha1,
    alpha2); None, the default: no check); where both are reached its score is the largest amount, over the channels, by
    which it lies outside the range of the two samples there, and it is flagged where score > threshold (in [0, 1] units).
    Returns Defects(mask (T, H, W) bool, score (T, H, W) float64, support (T, H, W) uint8: the references reached, 0 .. 2 --
    with fewer than 2 the pixel is not judged: score 0, not flagged).  include/papof.h (papof_defect_detect_tensor) states
    the rule exactly.  Not found: a defect that persists over frames (a line scratch, a sensor pixel under a static
    camera), a defect below the threshold; found though no defect: a small object that outruns the flow (a ball, rain --
    flow_video_ld's flows help); the end frames, with both references on one side, are weaker.  Enqueued on the current
    stream; returns without waiting."""
    alphas = _alphas(consistency)
    threshold = _check_threshold(threshold)
    ts, descs, _, _ = _check_video(frames, layout, 1, None, min_frames=3)
    (T, H, W, _), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    return _detect(ts, descs, (flow_fw, flow_bw), codes, threshold, alphas)


def dilate_masks(masks, radius):
    """Masks grown by `radius` pixels (0 .. 32) in every direction -- binary dilation by a square of side 2 radius + 1,
    clipped to the image: masks (T, H, W) (2-D: one frame) bool / uint8 on a HIP device, nonzero set.  Returns a new
    (T, H, W) bool tensor (radius 0: masks != 0).  One HIP kernel on the masks' bytes (include/papof.h:
    papof_mask_dilate_tensor); enqueued on the current stream, returns without waiting."""
    torch = _torch()
    radius = _check_dilate("radius", radius)
    if not isinstance(masks, torch.Tensor):
        raise TypeError("masks must be a torch.Tensor, got %s" % type(masks).__name__)
    if masks.dim() == 2:
        masks = masks.unsqueeze(0)
    if masks.dim() != 3 or min(masks.shape) < 1:
        raise ValueError("masks must be (T, H, W) with T, H, W >= 1 (or 2-D: one frame), got shape %s" % (tuple(masks.shape),))
    if not _on_gpu(masks):
        raise ValueError("masks must be on a HIP device (cuda:N), got %s" % masks.device)
    m = _check_masks("masks", masks, *(int(s) for s in masks.shape), masks.device)
    return _dilate(m, radius).view(torch.bool)


def _repair(ts, descs, flows, codes, given, threshold, dilate, radius, relax, alphas, layout, out_dtype):
    """repair_defects behind its argument checks: `given` the caller's uint8 masks or None"""
    torch = _torch()
    grown = lambda d: _dilate((d if given is None else d | (given != 0)).view(torch.uint8), dilate)  # noqa: E731
    first = _detect(ts, descs, flows, codes, threshold, alphas).mask
    second = _detect(ts, descs, _complete(flows, grown(first), relax), codes, threshold, alphas).mask
    detected = first | second
    m = grown(detected)
    p = _propagate(ts, descs, m, _complete(flows, m, relax), codes, radius, alphas, layout, torch.float64)
    video = _fill(p.video, descriptor(p.video, layout), (p.status == 2).view(torch.uint8), relax, layout, out_dtype)
    return Restored(video, m.view(torch.bool), detected, p.status)


def repair_defects(frames, flow_fw, flow_bw, *, masks=None, threshold=DEFECT_THRESHOLD, dilate=DEFECT_DILATE, radius=None,
                   relax=RELAX, consistency=None, layout="NCHW", out_dtype=None):
    """One pass of dirt and dropout removal on the caller's flows: frames and flows as detect_defects takes them (T >= 3);
    masks: None, or (T, H, W) bool / uint8 on the frames' device, pixels to repair whatever the detector says.
        1. detect_defects on the flows (threshold, consistency);  2. OR with `masks`;  3. dilate_masks by `dilate` (0 .. 32);
        4. complete_flows under that set (relax);  5. detect_defects on the completed flows -- a large defect drags the flow
        under it along, and what it hid shows once the flow there is its surroundings';  6. OR with 1. and `masks`;
        7. dilate_masks by `dilate`;  8. inpaint_video's steps on the flows as they were given under that set: complete_flows,
        propagate (radius, consistency) into float64, fill_holes (relax) of what is still a hole.
    Returns Restored(video in `layout` and out_dtype (by default the frames'; pixels outside `masks` are their input values,
    of the frames' dtype: their bytes), masks (T, H, W) bool: the repaired set of step 7, detected (T, H, W) bool: what the
    two detections flagged, undilated, status (T, H, W) uint8: 0 kept, 1 filled along the flows, 2 filled spatially).  The
    defaults were calibrated in tests/test_restore_cpu.py.  Every argument error raises before anything is launched; the
    video is enqueued on the current stream."""
    alphas = _alphas(consistency)
    threshold = _check_threshold(threshold)
    dilate = _check_dilate("dilate", dilate)
    relax = _check_relax(relax)
    ts, descs, out_dtype, _ = _check_video(frames, layout, 1, out_dtype, min_frames=3)
    (T, H, W, _), _, _ = descs[0]
    radius = _check_radius(radius, T)
    given = None if masks is None else _check_video_masks(ts, descs, masks)
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    return _repair(ts, descs, (flow_fw, flow_bw), codes, given, threshold, dilate, radius, relax, alphas, layout, out_dtype)


def restore_video(frames, pyramidLevels, *, passes=DEFECT_PASSES, masks=None, threshold=DEFECT_THRESHOLD, dilate=DEFECT_DILATE,
                  radius=None, relax=RELAX, consistency=None, layout="NCHW", out_dtype=None, **solver):
    """A video of T >= 3 frames with its one-frame defects removed, `passes` (1 .. 8) passes: pass 0 is flow_video_fb(frames,
    pyramidLevels, layout=layout, consistency=None, out_dtype=torch.float64, **solver) followed by repair_defects on those
    flows; every later pass estimates the flows again on the previous pass's video -- the defects no longer drag them
    along -- and runs repair_defects on the ORIGINAL frames with those flows and masks = `masks` OR everything detected so
    far.  Returns RestoredVideo(video, masks, detected -- of all passes --, status of the last pass, flow_fw, flow_bw
    (T - 1, 2, H, W) float64 and timing of the last flow call).  Every argument error raises before anything is launched;
    the flows are complete on return, the video is enqueued on the current stream behind them."""
    torch = _torch()
    alphas = _alphas(consistency)
    passes = _int_in("passes", passes, 1, MAX_PASSES)
    threshold = _check_threshold(threshold)
    dilate = _check_dilate("dilate", dilate)
    relax = _check_relax(relax)
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, min_frames=3, solver=solver)
    (T, _, _, _), _, _ = descs[0]
    radius = _check_radius(radius, T)
    given = None if masks is None else _check_video_masks(ts, descs, masks)
    codes = (capi.DTYPE_F64, capi.DTYPE_F64)
    r, detected = None, None
    for k in range(passes):
        src = ts if r is None else [r.video]
        fb = _run_fb(src, [descriptor(src[0], layout)], True, T - 1, layout, torch.float64, pyramidLevels, _alphas(None), params)
        known = given if detected is None else (detected if given is None else detected | (given != 0)).view(torch.uint8)
        r = _repair(ts, descs, (fb.flow_fw, fb.flow_bw), codes, known, threshold, dilate, radius, relax, alphas, layout,
                    out_dtype if k == passes - 1 else ts[0].dtype)
        detected = r.detected if detected is None else detected | r.detected
    return RestoredVideo(r.video, r.masks, detected, r.status, fb.flow_fw, fb.flow_bw, fb.timing)


# sigma of the deinterlacer's agreement weight: calibrated in tests/test_deinterlace_cpu.py (test_quality_calibration)
DEINT_SIGMA = 0.05
MAX_FIELD_HEIGHT = 2 ** 30 - 1  # include/papof.h: papof_deinterlace_tensor


def _check_parity(first):
    if isinstance(first, bool) or not isinstance(first, int) or first not in (0, 1):
        raise ValueError("first must be 0 or 1 (the parity of field 0's rows), got %r" % (first,))
    return first


def _check_deint_sigma(sigma):
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise TypeError("sigma must be a number, got %r" % (sigma,))
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0, got %r" % (sigma,))
    return float(sigma)


def _check_field_video(fields, layout, levels, out_dtype, solver=None):
    """the fields of the deinterlacing calls: _check_video's returns for T >= 4 fields"""
    ts, descs, out_dtype, params = _check_video(fields, layout, levels, out_dtype, name="fields", min_frames=4, solver=solver)
    if descs[0][0][1] > MAX_FIELD_HEIGHT:
        raise ValueError("fields must have at most %d rows, got %d" % (MAX_FIELD_HEIGHT, descs[0][0][1]))
    return ts, descs, out_dtype, params


def _deinterlace(ts, descs, first, mode, flows, codes, sigma, layout, out_dtype):
    """papof_deinterlace_tensor of the checked fields ts[0]: Deinterlaced(video, confidence float64 -- None in mode 0)"""
    torch = _torch()
    (T, Hf, W, C), strides, code = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(T, 2 * Hf, W, C, layout, out_dtype, dev)
    d_in = _struct(ts[0], strides, code)
    if mode:
        conf = torch.empty((T, Hf, W), dtype=torch.float64, device=dev)
        d_conf = _struct(conf, (conf.stride(0), conf.stride(1), conf.stride(2), 0), capi.DTYPE_F64)
        d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    else:
        conf, d_conf, d_f = None, None, (None, None)
    _launch(dev, "papof_deinterlace_tensor", T, Hf, W, C, ctypes.byref(d_in), first, mode, _ref(d_f[0]), _ref(d_f[1]), sigma,
            ctypes.byref(d_out), _ref(d_conf))
    return Deinterlaced(out, conf)


def split_fields(frames, top_first=True, *, layout="NCHW"):
    """Woven interlaced frames as the sequence of their fields, with torch operations on any device: frames (N, C, H, W) or
    (N, H, W, C) by `layout` (3-D: one frame), H even -> a new tensor (2 N, C, H / 2, W) or (2 N, H / 2, W, C): frame n
    gives fields 2 n and 2 n + 1, the top field (rows 0, 2, ...) before the bottom one when top_first, else after it.
    The deinterlacing calls take these fields with first = 0 for top_first, first = 1 otherwise."""
    frames = _as4d("frames", frames)
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    if not isinstance(top_first, (bool, int)) or top_first not in (0, 1):
        raise ValueError("top_first must be True or False, got %r" % (top_first,))
    axis = 2 if layout == "NCHW" else 1
    if min(frames.shape) < 1:
        raise ValueError("empty frames: shape %s" % (tuple(frames.shape),))
    if frames.shape[axis] % 2:
        raise ValueError("interlaced frames have an even number of rows, got %d (layout %s)" % (frames.shape[axis], layout))
    rows = lambda p: frames[:, :, p::2] if axis == 2 else frames[:, p::2]  # noqa: E731
    p0 = 0 if top_first else 1
    return _torch().stack((rows(p0), rows(1 - p0)), 1).flatten(0, 1)


def bob_fields(fields, first=0, *, layout="NCHW", out_dtype=None):
    """The spatial deinterlacer alone (papof_deinterlace_tensor, mode 0): T >= 4 fields (T, C, Hf, W) or (T, Hf, W, C) by
    `layout`, C = 1 .. 4, uint8 (read as x / 255), float32 or float64, any strides, on a HIP device; field k holds the rows
    of parity (k + first) & 1 of frame k.  Returns the video (T, ..., 2 Hf, W ...) in `layout` and out_dtype (by default the
    fields'): every frame keeps its field's lines and makes the others with the four-tap cubic (9 (a1 + b1) - (a3 + b3)) /
    16 of the lines above and below, rows clamped at the borders.  No flows are read.  Enqueued on the current stream;
    returns without waiting."""
    first = _check_parity(first)
    ts, descs, out_dtype, _ = _check_field_video(fields, layout, 1, out_dtype)
    return _deinterlace(ts, descs, first, 0, None, None, DEINT_SIGMA, layout, out_dtype).video


def field_flows(fields, pyramidLevels, *, layout="NCHW", **solver):
    """The flows that deinterlace_fields takes: flow_pairs_fb(fields[:-2], fields[2:], pyramidLevels, layout=layout,
    consistency=None, out_dtype=torch.float64, **solver) -- pair k from field k to field k + 2, two fields of one parity,
    which share a sampling lattice, so that the solver needs no special treatment; (T - 2, 2, Hf, W) float64 in field
    coordinates.  The pairs are independent: every field that is both a pair's second and another pair's first has its
    pyramid built twice (DESIGN.md section 35 has the measured cost against two flow_video_fb calls on the even and the
    odd fields).  Returns a FlowFB (occlusion None).  T >= 4."""
    ts, descs, _, params = _check_field_video(fields, layout, pyramidLevels, None, solver=solver)
    return _field_flows(ts, descs, layout, pyramidLevels, params)


def _field_flows(ts, descs, layout, levels, params):
    (T, Hf, W, C), strides, code = descs[0]
    pair = [ts[0][:-2], ts[0][2:]]
    d = [((T - 2, Hf, W, C), strides, code)] * 2
    return _run_fb(pair, d, False, T - 2, layout, _torch().float64, levels, _alphas(None), params)


def deinterlace_fields(fields, flow_fw, flow_bw, first=0, *, sigma=DEINT_SIGMA, layout="NCHW", out_dtype=None):
    """Motion-compensated deinterlacing of T >= 4 fields into T full frames, one per field (double rate): fields
    (T, C, Hf, W) or (T, Hf, W, C) by `layout`, C = 1 .. 4, uint8 (read as x / 255), float32 or float64, any strides, on a
    HIP device; field k holds the rows of parity (k + first) & 1 of frame k (split_fields: first = 0 for top_first);
    flow_fw, flow_bw (T - 2, 2, Hf, W) float32 / float64 on the same device in FIELD coordinates, pair k from field k to
    field k + 2 and back, as field_flows returns them.
    Frame t keeps its field's lines.  Each line it lacks is the blend (1 - q) s + q m of the bob's cubic s and of m, the
    fields t - 1 and t + 1 sampled where interpolate's gather rule at time 0.5 lands in them -- each sample weighted by
    c = 1 - 2 |Y - rint(Y)|, which is 1 on a field line and 0 halfway between two, where a sample carries no detail --,
    with q = max(c0, c1) / (1 + D / sigma^2), D the mean squared difference of the two samples over the channels; one
    sample only (the other out of the image, or an end frame): q = c / 2; none, or a NaN or infinite flow: the cubic.
    sigma = 0.05 was calibrated in tests/test_deinterlace_cpu.py.
    Returns Deinterlaced(video (T, ..., 2 Hf, W ...) in `layout` and out_dtype -- by default the fields'; uint8 to uint8
    keeps the kept lines' bytes --, confidence (T, Hf, W) float64: q of every made pixel).  include/papof.h
    (papof_deinterlace_tensor) states the rule exactly.  Not gained: anything at the critical velocity (an odd number of
    frame rows per field: the neighbouring fields hold the same lines, the output is bob_fields'); the end frames are
    weaker; the flows assume motion linear over two field periods; telecined film is inverse_telecine's case;
    interlaced 4:2:0 surfaces come in through ycc_to_rgb(..., interlaced=True).  Enqueued on the current stream; returns without waiting."""
    first = _check_parity(first)
    sigma = _check_deint_sigma(sigma)
    ts, descs, out_dtype, _ = _check_field_video(fields, layout, 1, out_dtype)
    (T, Hf, W, _), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (T - 2, 2, Hf, W), ts[0].device)
    return _deinterlace(ts, descs, first, 1, (flow_fw, flow_bw), codes, sigma, layout, out_dtype)


def deinterlace_video(fields, pyramidLevels, first=0, *, sigma=DEINT_SIGMA, layout="NCHW", out_dtype=None, **solver):
    """T >= 4 fields deinterlaced along their motion: field_flows(fields, pyramidLevels, layout=layout, **solver) followed
    by deinterlace_fields on those flows (first, sigma).  Returns DeinterlacedVideo(video, confidence, flow_fw, flow_bw
    (T - 2, 2, Hf, W) float64 in field coordinates, timing of the flow call).  Every argument error raises before anything
    is launched; the flows are complete on return, the video is enqueued on the current stream behind them."""
    first = _check_parity(first)
    sigma = _check_deint_sigma(sigma)
    ts, descs, out_dtype, params = _check_field_video(fields, layout, pyramidLevels, out_dtype, solver=solver)
    fb = _field_flows(ts, descs, layout, pyramidLevels, params)
    d = _deinterlace(ts, descs, first, 1, (fb.flow_fw, fb.flow_bw), (capi.DTYPE_F64, capi.DTYPE_F64), sigma, layout, out_dtype)
    return DeinterlacedVideo(d.video, d.confidence, fb.flow_fw, fb.flow_bw, fb.timing)


# ---- inverse telecine (include/papof.h: papof_field_metrics_tensor, papof_weave_fields_tensor)
MAX_CELL_ROWS = 64
CELL_COLUMNS = 64
MAX_Q = 65535                 # the thresholds' integer scale
COMB_THRESHOLD = 10 / 255     # tests/test_telecine_cpu.py: the scenes hold at noise of 2 / 255; 26 / 255 for 5 / 255
DIFF_THRESHOLD = 8 / 255
FREE, PREV, NEXT, VIDEO = 0, 1, 2, 3  # a field's vote: no evidence (static), woven with its previous / next field, with neither
ORPHANS = ("bob", "mc", "drop")


def _check_q(name, v):
    """a threshold in the fields' [0, 1] units as its integer rint(65535 v) (half to even)"""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s must be a number, got %r" % (name, v))
    if not (math.isfinite(v) and 0 <= v <= 1):
        raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
    return int(round(float(MAX_Q) * float(v)))


def _check_cell_rows(cell_rows):
    return _int_in("cell_rows", cell_rows, 1, MAX_CELL_ROWS)


def _check_telecine_fields(fields, layout, levels, out_dtype, solver=None):
    """the fields of the inverse-telecine calls: _check_video's returns for T >= 3 fields"""
    ts, descs, out_dtype, params = _check_video(fields, layout, levels, out_dtype, name="fields", min_frames=3, solver=solver)
    if descs[0][0][1] > MAX_FIELD_HEIGHT:
        raise ValueError("fields must have at most %d rows, got %d" % (MAX_FIELD_HEIGHT, descs[0][0][1]))
    return ts, descs, out_dtype, params


def _field_metrics(ts, descs, first, cell_rows, comb_q, diff_q):
    """papof_field_metrics_tensor of the checked fields ts[0]: a FieldMetrics"""
    torch = _torch()
    (T, Hf, W, C), strides, code = descs[0]
    dev = ts[0].device
    counts = torch.empty((T, 3, -(-Hf // cell_rows), -(-W // CELL_COLUMNS)), dtype=torch.int32, device=dev)
    d_in = _struct(ts[0], strides, code)
    _launch(dev, "papof_field_metrics_tensor", T, Hf, W, C, ctypes.byref(d_in), first, cell_rows, comb_q, diff_q,
            ctypes.c_void_p(counts.data_ptr()))
    return FieldMetrics(counts, cell_rows, first)


def field_metrics(fields, first=0, *, comb_threshold=COMB_THRESHOLD, diff_threshold=DIFF_THRESHOLD, cell_rows=16, layout="NCHW"):
    """How every field of a sequence weaves with its two neighbours (papof_field_metrics_tensor, one HIP kernel): T >= 3
    fields (T, C, Hf, W) or (T, Hf, W, C) by `layout`, C = 1 .. 4, uint8, float32 or float64, any strides, on a HIP device;
    field k holds the rows of parity (k + first) & 1 of frame k.  Values are quantised to 0 .. 65535 (a byte b is 257 b, a
    float v clamp(rint(65535 v), 0, 65535), NaN 0) and everything after that is integer.  For each interior field t every
    pixel of its lines is tested against the lines above and below it in field t - 1 and in field t + 1 -- two fields of one
    parity: the same rows --: M is how far the pixel lies outside the range of the two lines, the largest over the channels.
    Per cell of cell_rows (1 .. 64) x 64 pixels, plane 0 counts the pixels with M+ > M- + comb_threshold (the next field fits
    worse), plane 1 those with M- > M+ + comb_threshold, plane 2 those where the two neighbours differ by more than
    diff_threshold.  The thresholds are in the fields' [0, 1] units and become rint(65535 v).  Absolute comb counts do not
    separate film from video (vertical detail looks like combing); these relative ones do: the texture cancels.
    Returns FieldMetrics(counts (T, 3, ceil(Hf / cell_rows), ceil(W / 64)) int32 on the fields' device -- fields 0 and T - 1
    are zeros --, cell_rows, first).  Enqueued on the current stream; returns without waiting."""
    first = _check_parity(first)
    comb_q, diff_q = _check_q("comb_threshold", comb_threshold), _check_q("diff_threshold", diff_threshold)
    cell_rows = _check_cell_rows(cell_rows)
    ts, descs, _, _ = _check_telecine_fields(fields, layout, 1, None)
    return _field_metrics(ts, descs, first, cell_rows, comb_q, diff_q)


def _check_match_rule(cell_rows, margin, dominance):
    """(margin -- by default cell_rows * 64 // 64 --, dominance) of match_fields' keywords"""
    if margin is None:
        margin = cell_rows * CELL_COLUMNS // 64
    if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
        raise ValueError("margin must be None or an integer >= 0, got %r" % (margin,))
    if isinstance(dominance, bool) or not isinstance(dominance, (int, float)) or not (math.isfinite(dominance) and dominance >= 1):
        raise ValueError("dominance must be a finite number >= 1, got %r" % (dominance,))
    return margin, dominance


def _check_metrics(metrics):
    """the counts of a FieldMetrics as a numpy (T, 3, Gy, Gx) int64 array: one copy from the device"""
    import numpy as np
    torch = _torch()
    if not isinstance(metrics, FieldMetrics):
        raise TypeError("metrics must be a FieldMetrics (field_metrics' return), got %s" % type(metrics).__name__)
    counts = metrics.counts
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32:
        raise TypeError("metrics.counts must be an int32 tensor")
    if counts.dim() != 4 or counts.shape[0] < 3 or counts.shape[1] != 3 or min(counts.shape) < 1:
        raise ValueError("metrics.counts must be (T >= 3, 3, Gy, Gx), got shape %s" % (tuple(counts.shape),))
    return counts.detach().cpu().numpy().astype(np.int64)


def field_votes(counts, margin, dominance):
    """the votes (T,) uint8 of numpy counts (T, 3, Gy, Gx): match_fields' rule for one field after another"""
    import numpy as np

    def ev(A, B):
        ok = (A > margin) & (dominance * B <= A)
        return int((A - B)[ok].max()) if ok.any() else 0

    T = counts.shape[0]
    votes = np.full(T, FREE, np.uint8)
    for t in range(1, T - 1):
        A, B = counts[t, 0], counts[t, 1]
        ep, en, hi = ev(A, B), ev(B, A), int(max(A.max(), B.max()))
        votes[t] = PREV if ep > en else NEXT if en > ep else VIDEO if hi > margin else FREE
    return votes


def field_groups(links):
    """[start, length] (N, 2) int64 of the groups of numpy links (T - 1,): the maximal runs of linked fields, a run of 4 or
    more cut into groups of 2, the last one of 3 when the run is odd"""
    import numpy as np
    groups, start, T = [], 0, len(links) + 1
    for t in range(T):
        if t == T - 1 or not links[t]:
            L = t + 1 - start
            if L <= 3:
                groups.append((start, L))
            else:
                for k in range(L // 2):
                    groups.append((start + 2 * k, 3 if (L % 2 and k == L // 2 - 1) else 2))
            start = t + 1
    return np.array(groups, np.int64).reshape(-1, 2)


def field_cadence(votes, groups):
    """(cadence, share) of numpy votes and groups: match_fields' report"""
    T = len(votes)
    L = [int(n) for n in groups[:, 1]]
    if all(v == FREE for v in votes):
        return "static", 1.0
    near = lambda i: [L[k] for k in (i - 1, i + 1) if 0 <= k < len(L)]  # noqa: E731
    shares = {
        "3:2": sum(n for i, n in enumerate(L) if n in (2, 3) and 5 - n in near(i)) / T,
        "2:2": sum(n for n in L if n == 2) / T,
        "video": sum(n for n in L if n == 1) / T,
    }
    if len(L) >= 2 and all(n in (2, 3) for n in L) and all(a + b == 5 for a, b in zip(L, L[1:])):
        return "3:2", 1.0
    for name in ("2:2", "video"):
        if shares[name] == 1.0:
            return name, 1.0
    return "mixed", max(shares.values())


def match_fields(metrics, *, margin=None, dominance=3):
    """Which fields belong to one film frame, from field_metrics' counts: the host's rule, on one copy of the small table
    from the device -- THIS CALL WAITS for the stream that wrote it.  With A = plane 0 and B = plane 1 of an interior field t,
        ev(A, B) = the largest A - B over the cells where A > margin and dominance * B <= A, 0 without such a cell
        ep = ev(A, B), en = ev(B, A), hi = the largest entry of A and B
    field t votes PREV (1: it weaves with field t - 1) where ep > en, NEXT (2) where en > ep, otherwise VIDEO (3: it weaves
    with neither) where hi > margin and FREE (0: nothing moves, any partner does) elsewhere; fields 0 and T - 1 are FREE.
    margin defaults to cell_rows * 64 // 64 counts (16 for the default cell).  Fields t and t + 1 are linked where field t
    votes NEXT or FREE and field t + 1 votes PREV or FREE; the groups are the maximal runs of linked fields: a run of 1, 2
    or 3 fields is one group, a longer one -- a static stretch -- is cut into groups of 2, the last one of 3 when it is odd.
    Returns FieldMatch(votes (T,) uint8, links (T - 1,) bool, groups (N, 2) int64 rows [start, length] -- torch tensors on
    the host --, cadence, share).  cadence is a report and decides nothing: "static" where every vote is FREE, "3:2" where
    the lengths alternate 2 and 3, "2:2" where all are 2, "video" where all are 1, else "mixed"; share is the share of the
    fields in groups that follow the named pattern (a 2 or 3 next to a 3 or 2; a 2; a 1), for "mixed" the largest of the
    three."""
    import numpy as np
    torch = _torch()
    if not isinstance(metrics, FieldMetrics):
        raise TypeError("metrics must be a FieldMetrics (field_metrics' return), got %s" % type(metrics).__name__)
    margin, dominance = _check_match_rule(_check_cell_rows(metrics.cell_rows), margin, dominance)
    counts = _check_metrics(metrics)
    votes = field_votes(counts, margin, dominance)
    nxt, prv = np.isin(votes[:-1], (NEXT, FREE)), np.isin(votes[1:], (PREV, FREE))
    links = nxt & prv
    groups = field_groups(links)
    cadence, share = field_cadence(votes, groups)
    return FieldMatch(torch.from_numpy(votes), torch.from_numpy(links), torch.from_numpy(groups), cadence, share)


def _check_weave_table(table, T):
    """the weave's table as a contiguous int32 host tensor (N, 2), N >= 1, every entry in 0 .. T - 1"""
    import numpy as np
    torch = _torch()
    if isinstance(table, torch.Tensor):
        if table.dtype.is_floating_point or table.dtype.is_complex or table.dtype == torch.bool:
            raise TypeError("table must hold integers, got %s" % table.dtype)
        t = table.detach().to("cpu", torch.int64)
    else:
        try:
            a = np.asarray(table)
        except Exception:  # noqa: BLE001
            raise TypeError("table must be an integer tensor or an integer array, got %r" % (table,)) from None
        if a.dtype.kind not in "iu":
            raise TypeError("table must hold integers, got %s" % a.dtype)
        t = torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
    if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < 1:
        raise ValueError("table must be (N >= 1, 2): the fields of the even and of the odd rows, got shape %s" % (tuple(t.shape),))
    if int(t.min()) < 0 or int(t.max()) >= T:
        raise ValueError("table names fields %d .. %d of %d fields" % (int(t.min()), int(t.max()), T))
    return t.to(torch.int32).contiguous()


def _weave(ts, descs, table, layout, out_dtype):
    """papof_weave_fields_tensor of the checked fields ts[0] by the checked host table: the video"""
    (T, Hf, W, C), strides, code = descs[0]
    dev = ts[0].device
    N = int(table.shape[0])
    out, d_out = _new_frames(N, 2 * Hf, W, C, layout, out_dtype, dev)
    tab = table.to(dev)
    d_in = _struct(ts[0], strides, code)
    _launch(dev, "papof_weave_fields_tensor", T, Hf, W, C, ctypes.byref(d_in), N, ctypes.c_void_p(tab.data_ptr()),
            ctypes.byref(d_out))
    return out


def weave_fields(fields, table, *, layout="NCHW", out_dtype=None):
    """Frames woven from the fields that a table names (papof_weave_fields_tensor, one HIP kernel, one pass): fields (T, C,
    Hf, W) or (T, Hf, W, C) by `layout`, T >= 1, C = 1 .. 4, uint8, float32 or float64, any strides, on a HIP device; table
    (N, 2) integers of any integer dtype, on any device or a numpy array: row 2 j of frame n is row j of field table[n, 0],
    row 2 j + 1 is row j of field table[n, 1].  Fields may repeat and come in any order.  Returns the video (N, ..., 2 Hf, W
    ...) in `layout` and out_dtype (by default the fields'; uint8 to uint8 keeps the bytes).  The table is checked on the
    host (a device tensor waits for its stream); the kernel is enqueued on the current stream and the call returns without
    waiting."""
    ts, descs, out_dtype, _ = _check_video(fields, layout, 1, out_dtype, name="fields", min_frames=1)
    if descs[0][0][1] > MAX_FIELD_HEIGHT:
        raise ValueError("fields must have at most %d rows, got %d" % (MAX_FIELD_HEIGHT, descs[0][0][1]))
    return _weave(ts, descs, _check_weave_table(table, descs[0][0][0]), layout, out_dtype)


def telecine_plan(groups, first, orphans):
    """What inverse_telecine makes of numpy groups (N, 2): (table (M, 2) int64 -- the fields of the even and the odd rows of
    every output frame, an orphan's own field twice --, the rows of `groups` that give a frame, times (M,) float64, kinds
    (M,) uint8).  A group of 2 or 3 is woven from its first two fields; a group of 1 is an orphan, left out by "drop"."""
    import numpy as np
    keep = [i for i, (s, n) in enumerate(groups) if n >= 2 or orphans != "drop"]
    table, times, kinds = [], [], []
    for i in keep:
        s, n = int(groups[i, 0]), int(groups[i, 1])
        if n == 1:
            table.append((s, s))
            times.append(float(s))
            kinds.append(1)
        else:
            even = s if (s + first) & 1 == 0 else s + 1
            table.append((even, 2 * s + 1 - even))
            times.append(s + 0.5)
            kinds.append(0)
    return (np.array(table, np.int64).reshape(-1, 2), np.array(keep, np.int64), np.array(times, np.float64),
            np.array(kinds, np.uint8))


def _check_orphans(orphans):
    if orphans not in ORPHANS:
        raise ValueError("orphans must be one of %s, got %r" % (ORPHANS, orphans))
    return orphans


def _detelecine(ts, descs, first, match, orphans, deinterlacer, layout, out_dtype):
    """inverse_telecine behind the match: deinterlacer() gives the (T, ...) video that the orphans' frames are taken from"""
    torch = _torch()
    T = descs[0][0][0]
    table, keep, times, kinds = telecine_plan(match.groups.numpy(), first, orphans)
    if len(table) == 0:
        raise ValueError("every field is an orphan and orphans='drop' leaves no frame")
    extra = None
    if kinds.any():
        if T < 4:
            raise ValueError("field %d has no partner and the deinterlacer needs 4 fields, got %d: orphans='drop' leaves it out"
                             % (int(table[kinds != 0][0, 0]), T))
        extra = deinterlacer()
    video = _weave(ts, descs, torch.from_numpy(table).to(torch.int32), layout, out_dtype)
    if extra is not None:
        dev = video.device
        orphan = torch.from_numpy(kinds != 0)
        video[orphan.to(dev)] = extra[torch.from_numpy(table[:, 0])[orphan].to(dev)]
    return Detelecined(video, match.groups[torch.from_numpy(keep)], torch.from_numpy(times), torch.from_numpy(kinds), match)


def inverse_telecine(fields, first=0, *, orphans="bob", flow_fw=None, flow_bw=None, sigma=DEINT_SIGMA,
                     comb_threshold=COMB_THRESHOLD, diff_threshold=DIFF_THRESHOLD, cell_rows=16, margin=None, dominance=3,
                     layout="NCHW", out_dtype=None):
    """The film frames of a telecined sequence of fields: field_metrics (first, comb_threshold, diff_threshold, cell_rows),
    match_fields (margin, dominance) and weave_fields chained.  fields (T, C, Hf, W) or (T, Hf, W, C) by `layout`, T >= 3,
    as field_metrics takes them.  A group of 2 or 3 fields becomes one frame, woven from its first two fields (the third
    of a triple is the repeat).  A group of 1 -- a video insert, a field orphaned by an edit -- has no partner and goes by
    `orphans`: "bob": bob_fields' frame of it; "mc": deinterlace_fields' frame of it on flow_fw, flow_bw (T - 2, 2, Hf, W),
    which are then required (and refused otherwise), with sigma; "drop": it is left out.  The deinterlacer needs T >= 4:
    with T = 3 and an orphan, anything but "drop" raises; so does "drop" when every field is an orphan.
    Returns Detelecined(video (N, ..., 2 Hf, W ...) in `layout` and out_dtype -- by default the fields'; uint8 to uint8:
    the woven frames are the fields' bytes --, groups (N, 2) [start, length] of the frames, times (N,) float64: the mean
    field index of the fields used, kinds (N,) uint8: 0 woven, 1 orphan, match: the FieldMatch).  The output rate is not
    constant: times says when each frame was.  Not handled: the critical vertical velocity (an odd number of frame rows
    per film frame makes the WRONG pairing a line-doubled frame without a comb: the match inverts; a video pan near one
    row per field gets fields misvoted); the thresholds are relative to the noise (noise of 5 / 255 needs comb_threshold
    26 / 255); no cadence lock (static stretches are cut 2-2-2); no blended telecine; decoder surfaces come in through ycc_to_rgb(..., interlaced=True).  Every
    argument error raises before a launch; the call waits for the counts (match_fields), the video is enqueued on the
    current stream behind them."""
    first = _check_parity(first)
    orphans = _check_orphans(orphans)
    sigma = _check_deint_sigma(sigma)
    comb_q, diff_q = _check_q("comb_threshold", comb_threshold), _check_q("diff_threshold", diff_threshold)
    cell_rows = _check_cell_rows(cell_rows)
    ts, descs, out_dtype, _ = _check_telecine_fields(fields, layout, 1, out_dtype)
    (T, Hf, W, _), _, _ = descs[0]
    codes = None
    if orphans == "mc":
        if T < 4:
            raise ValueError("orphans='mc' needs at least 4 fields, got %d" % T)
        codes = _check_flows(flow_fw, flow_bw, (T - 2, 2, Hf, W), ts[0].device)
    elif flow_fw is not None or flow_bw is not None:
        raise ValueError("flow_fw and flow_bw are read with orphans='mc' only, got orphans=%r" % (orphans,))
    margin, dominance = _check_match_rule(cell_rows, margin, dominance)
    match = match_fields(_field_metrics(ts, descs, first, cell_rows, comb_q, diff_q), margin=margin, dominance=dominance)
    if orphans == "mc":
        deinterlacer = lambda: _deinterlace(ts, descs, first, 1, (flow_fw, flow_bw), codes, sigma, layout, out_dtype).video  # noqa: E731
    else:
        deinterlacer = lambda: _deinterlace(ts, descs, first, 0, None, None, DEINT_SIGMA, layout, out_dtype).video  # noqa: E731
    return _detelecine(ts, descs, first, match, orphans, deinterlacer, layout, out_dtype)


def inverse_telecine_video(fields, pyramidLevels, first=0, *, sigma=DEINT_SIGMA, comb_threshold=COMB_THRESHOLD,
                           diff_threshold=DIFF_THRESHOLD, cell_rows=16, margin=None, dominance=3, layout="NCHW", out_dtype=None,
                           **solver):
    """inverse_telecine with orphans="mc" on flows of its own: field_flows(fields, pyramidLevels, layout=layout, **solver)
    is computed only when the match leaves a group of 1.  Returns DetelecinedVideo(Detelecined's fields, flow_fw, flow_bw
    (T - 2, 2, Hf, W) float64 in field coordinates, timing of the flow call -- all three None when no field is an orphan)."""
    first = _check_parity(first)
    sigma = _check_deint_sigma(sigma)
    comb_q, diff_q = _check_q("comb_threshold", comb_threshold), _check_q("diff_threshold", diff_threshold)
    cell_rows = _check_cell_rows(cell_rows)
    ts, descs, out_dtype, params = _check_telecine_fields(fields, layout, pyramidLevels, out_dtype, solver=solver)
    margin, dominance = _check_match_rule(cell_rows, margin, dominance)
    match = match_fields(_field_metrics(ts, descs, first, cell_rows, comb_q, diff_q), margin=margin, dominance=dominance)
    flows = []

    def deinterlacer():
        fb = _field_flows(ts, descs, layout, pyramidLevels, params)
        flows.append(fb)
        return _deinterlace(ts, descs, first, 1, (fb.flow_fw, fb.flow_bw), (capi.DTYPE_F64, capi.DTYPE_F64), sigma, layout,
                            out_dtype).video

    d = _detelecine(ts, descs, first, match, "mc", deinterlacer, layout, out_dtype)
    fb = flows[0] if flows else None
    return DetelecinedVideo(*d, fb.flow_fw if fb else None, fb.flow_bw if fb else None, fb.timing if fb else None)


# ---- shot boundaries (include/papof.h: papof_cell_hist_tensor)
HIST_BINS = (4, 8, 16, 32, 64)
CUT_FLOOR = 0.2    # tests/test_shots_cpu.py: a one-frame flash of gain 1.8 reaches 0.306, a (4, 25) pan with noise 0.138
CUT_RATIO = 3.0
CUT_WINDOW = 4
CUT_POOL = (4, 2)  # cells per region, down and across: 64 x 128 pixels at 16-row cells


def _check_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, int) or bins not in HIST_BINS:
        raise ValueError("bins must be one of %s, got %r" % (HIST_BINS, bins))
    return bins


def _cell_hist(ts, descs, cell_rows, bins):
    """papof_cell_hist_tensor of the checked frames ts[0]: a ShotHist"""
    torch = _torch()
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    hist = torch.empty((T, -(-H // cell_rows), -(-W // CELL_COLUMNS), bins), dtype=torch.int32, device=dev)
    d_in = _struct(ts[0], strides, code)
    _launch(dev, "papof_cell_hist_tensor", T, H, W, C, ctypes.byref(d_in), cell_rows, bins, ctypes.c_void_p(hist.data_ptr()))
    return ShotHist(hist, cell_rows, bins, (H, W))


def shot_histograms(frames, *, cell_rows=16, bins=16, layout="NCHW"):
    """The luma histograms of every frame of a video per cell of cell_rows (1 .. 64) x 64 pixels (papof_cell_hist_tensor, one
    HIP kernel): T >= 1 frames (T, C, H, W) or (T, H, W, C) by `layout`, C = 1 .. 4, uint8, float32 or float64, any strides,
    on a HIP device.  Values are quantised to 0 .. 65535 as field_metrics does (a byte b is 257 b, a float v clamp(rint(65535
    v), 0, 65535), NaN 0) and everything after that is integer: the luma is channel 0 of 1 or 2 channels and (77 q0 + 150 q1 +
    29 q2) >> 8 of 3 or 4, its bin (L * bins) >> 16 with bins one of 4, 8, 16, 32, 64.
    Returns ShotHist(hist (T, ceil(H / cell_rows), ceil(W / 64), bins) int32 on the frames' device -- the cells at the bottom
    and right edges are clipped; every cell's bins add up to its pixel count --, cell_rows, bins, size (H, W)).  Enqueued on
    the current stream; returns without waiting."""
    cell_rows = _check_cell_rows(cell_rows)
    bins = _check_bins(bins)
    ts, descs, _, _ = _check_video(frames, layout, 1, None, min_frames=1)
    return _cell_hist(ts, descs, cell_rows, bins)


def _check_pool(pool):
    try:
        py, px = pool
    except (TypeError, ValueError):
        raise TypeError("pool must be (cells down, cells across), got %r" % (pool,)) from None
    for v in (py, px):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("pool must be two integers >= 1, got %r" % (pool,))
    return py, px


def _check_hist(hist):
    """the counts of a ShotHist as a numpy (T, Gy, Gx, bins) int64 array: one copy from the device"""
    import numpy as np
    torch = _torch()
    if not isinstance(hist, ShotHist):
        raise TypeError("hist must be a ShotHist (shot_histograms' return), got %s" % type(hist).__name__)
    h = hist.hist
    if not isinstance(h, torch.Tensor) or h.dtype != torch.int32:
        raise TypeError("hist.hist must be an int32 tensor")
    if h.dim() != 4 or min(h.shape) < 1:
        raise ValueError("hist.hist must be (T >= 1, Gy, Gx, bins), got shape %s" % (tuple(h.shape),))
    return h.detach().cpu().numpy().astype(np.int64)


def pool_cells(counts, pool):
    """numpy counts (T, Gy, Gx, bins) summed over regions of pool[0] x pool[1] cells -- histograms add --, the regions at the
    bottom and right edges clipped: (T, ceil(Gy / pool[0]), ceil(Gx / pool[1]), bins)"""
    import numpy as np
    py, px = pool
    return np.add.reduceat(np.add.reduceat(counts, np.arange(0, counts.shape[1], py), axis=1),
                           np.arange(0, counts.shape[2], px), axis=2)


def pooled_distances(regions, step):
    """(T - step,) float64 of numpy region histograms (T, Ry, Rx, bins): shot_distances' rule behind the pooling"""
    import numpy as np
    a, b = regions[:-step], regions[step:]
    if len(a) == 0:
        return np.zeros((0,), np.float64)
    d = np.abs(a - b).sum(-1).astype(np.float64) / (2.0 * a.sum(-1).astype(np.float64))
    return np.median(d.reshape(len(a), -1), axis=1)


def shot_distances(hist, *, pool=CUT_POOL, step=1):
    """How much the luma distribution changes from frame t to frame t + step, region by region: the host's measure on one
    copy of shot_histograms' counts -- THIS CALL WAITS for the stream that wrote them.  The cells are summed into regions of
    pool[0] x pool[1] cells (down, across; the edge regions clipped); per region d = sum_k |a_k - b_k| / (2 sum_k a_k) in
    float64, a and b the region's histograms in the two frames: 0 for equal histograms, 1 for disjoint ones; the pair's
    distance is numpy.median over the regions (the mean of the middle two of an even number).  A histogram forgets where a
    region's pixels are, so motion changes it only by what enters and leaves the region; the median forgets what happens in
    fewer than half of the regions.  Returns a (T - step,) float64 numpy array, empty for T <= step."""
    py, px = _check_pool(pool)
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError("step must be an integer >= 1, got %r" % (step,))
    return pooled_distances(pool_cells(_check_hist(hist), (py, px)), step)


def _check_cut_rule(floor, ratio, window):
    """(floor in [0, 1], ratio >= 1, window >= 1) of detect_cuts' keywords as (float, float, int) -- TypeError / ValueError
    otherwise"""
    for name, v in (("floor", floor), ("ratio", ratio)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s must be a number, got %r" % (name, v))
    if not 0 <= floor <= 1:  # (false for a NaN)
        raise ValueError("floor must lie in [0, 1], got %r" % (floor,))
    if not (math.isfinite(ratio) and ratio >= 1):
        raise ValueError("ratio must be finite and >= 1, got %r" % (ratio,))
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError("window must be an integer >= 1, got %r" % (window,))
    return float(floor), float(ratio), window


def split_shots(n_frames, cuts):
    """The frame ranges [(start, stop), ...] -- stop exclusive -- of a video of n_frames >= 1 frames cut between frames t and
    t + 1 for every t of `cuts` (integers in 0 .. n_frames - 2, in any order, none twice): frames[start:stop] is one shot, for
    running any *_video call shot by shot."""
    if isinstance(n_frames, bool) or not isinstance(n_frames, int) or n_frames < 1:
        raise ValueError("n_frames must be an integer >= 1, got %r" % (n_frames,))
    cuts = _check_cuts(cuts, n_frames - 1)
    edges = [0] + [t + 1 for t in cuts] + [n_frames]
    return list(zip(edges[:-1], edges[1:]))


def _check_cuts(cuts, n_pairs):
    """the cuts as a sorted list of distinct integers in 0 .. n_pairs - 1 -- TypeError / ValueError otherwise"""
    import numpy as np
    torch = _torch()
    if isinstance(cuts, torch.Tensor):
        cuts = cuts.detach().cpu().numpy()
    try:
        a = np.asarray(cuts if not isinstance(cuts, (set, frozenset)) else sorted(cuts))
    except Exception:  # noqa: BLE001
        raise TypeError("cuts must be a sequence of integers, got %r" % (cuts,)) from None
    if a.size == 0:
        return []
    if a.dtype.kind not in "iu" or a.ndim != 1:
        raise TypeError("cuts must be a sequence of integers, got %r" % (cuts,))
    out = sorted(int(t) for t in a)
    if out[0] < 0 or out[-1] >= n_pairs:
        raise ValueError("cuts must lie in 0 .. %d (a cut at t lies between frames t and t + 1), got %r" % (n_pairs - 1, out))
    if len(set(out)) != len(out):
        raise ValueError("cuts names a pair twice: %r" % (out,))
    return out


def cut_candidates(d, floor, ratio, window):
    """which pairs of numpy distances (N,) are candidates: detect_cuts' rule for one pair after another"""
    import numpy as np
    cand = np.zeros(len(d), bool)
    for t in range(len(d)):
        others = np.concatenate([d[max(0, t - window):t], d[t + 1:t + 1 + window]])
        base = float(np.median(others)) if len(others) else 0.0
        cand[t] = d[t] >= floor and d[t] >= ratio * base
    return cand


def detect_cuts(hist, *, floor=CUT_FLOOR, ratio=CUT_RATIO, window=CUT_WINDOW, pool=CUT_POOL):
    """The cuts of a video from shot_histograms' counts: the host's rule -- THIS CALL WAITS for the stream that wrote them.
    With d = shot_distances(hist, pool=pool), pair t (frames t and t + 1) is a candidate where d[t] >= floor and d[t] >= ratio
    times the median of the other d within `window` pairs either side (0 where there are none): the threshold is relative to
    what the shot's own motion does to the measure.  A maximal run of consecutive candidates is judged by its length: one pair
    is a cut; two pairs t, t + 1 are a FLASH at frame t + 1 -- and no cut -- where shot_distances(step=2)[t] < floor (frames t
    and t + 2 belong together), otherwise two cuts around a one-frame shot; three or more are cuts all of them, and (first,
    last) is reported in `gradual` as well: a dissolve and a run of one-frame shots get the same, safe treatment.
    The defaults were calibrated on scenes cut from the committed 1080p frame (tests/test_shots_cpu.py): inside a shot a pan
    of (4, 25) pixels per frame with noise stays below 0.138, an exposure ramp of 5 % per frame below 0.058; a cut to the
    adjacent region reaches 0.333, a flash of gain 1.8 0.306 at both its pairs.
    Returns Shots(cuts: the sorted pair indices t, a cut at t lies between frames t and t + 1; flashes: frame indices;
    gradual: (first, last) pairs; distances: d, a (T - 1,) float64 numpy array; ranges: split_shots(T, cuts))."""
    floor, ratio, window = _check_cut_rule(floor, ratio, window)
    py, px = _check_pool(pool)
    regions = pool_cells(_check_hist(hist), (py, px))
    T = regions.shape[0]
    d = pooled_distances(regions, 1)
    cand = cut_candidates(d, floor, ratio, window)
    cuts, flashes, gradual = [], [], []
    t = 0
    while t < len(d):
        if not cand[t]:
            t += 1
            continue
        n = 1
        while t + n < len(d) and cand[t + n]:
            n += 1
        if n == 2 and pooled_distances(regions[t:t + 3], 2)[0] < floor:
            flashes.append(t + 1)
        else:
            cuts.extend(range(t, t + n))
            if n >= 3:
                gradual.append((t, t + n - 1))
        t += n
    return Shots(cuts, flashes, gradual, d, split_shots(T, cuts))


def detect_shots(frames, *, cell_rows=16, bins=16, layout="NCHW", floor=CUT_FLOOR, ratio=CUT_RATIO, window=CUT_WINDOW,
                 pool=CUT_POOL):
    """detect_cuts(shot_histograms(frames, cell_rows=, bins=, layout=), floor=, ratio=, window=, pool=): the Shots of a video
    on a HIP device.  Every argument error raises before anything is enqueued; the call waits for the counts."""
    cell_rows, bins = _check_cell_rows(cell_rows), _check_bins(bins)
    _check_cut_rule(floor, ratio, window)
    _check_pool(pool)
    ts, descs, _, _ = _check_video(frames, layout, 1, None, min_frames=1)
    return detect_cuts(_cell_hist(ts, descs, cell_rows, bins), floor=floor, ratio=ratio, window=window, pool=pool)


def _kill_pairs(fb, pairs):
    """the pairs `pairs` (an index or a slice) of a FlowFB's tensors made a cut's, in place"""
    for f in (fb.flow_fw, fb.flow_bw):
        f[pairs] = math.nan
    if fb.occlusion is not None:
        fb.occlusion[pairs] = True
    for w in (fb.warpI2_fw, fb.warpI2_bw):
        if w is not None:
            w[pairs] = 0


def cut_flows(fb, cuts):
    """A FlowFB (flow_video_fb's return, or any FlowFB of (B, 2, H, W) flows) whose pairs `cuts` -- integers in 0 .. B - 1 --
    say that there is nothing to follow: both flows of the pair are the quiet NaN, which every consumer takes as its ABI
    states (track_points: lost; temporal_filter, propagate, super_resolve: the chain ends; fb_consistency: occluded;
    refine_flow, upsample_flow, the rolling-shutter calls: dead), occlusion is True in both channels and warpI2_* zero where
    they are present.  Every tensor of the result is a COPY: `fb` is left as it was and shares no storage with the result;
    timing is the same dict.  Torch operations on the tensors' device, enqueued on the current stream."""
    torch = _torch()
    if not isinstance(fb, FlowFB):
        raise TypeError("fb must be a FlowFB (flow_video_fb's return), got %s" % type(fb).__name__)
    for name, f in (("fb.flow_fw", fb.flow_fw), ("fb.flow_bw", fb.flow_bw)):
        _check_flow(name, f)
    if fb.flow_fw.shape != fb.flow_bw.shape:
        raise ValueError("fb.flow_fw %s and fb.flow_bw %s differ in shape" % (tuple(fb.flow_fw.shape), tuple(fb.flow_bw.shape)))
    B = int(fb.flow_fw.shape[0])
    for name, t in (("fb.warpI2_fw", fb.warpI2_fw), ("fb.warpI2_bw", fb.warpI2_bw), ("fb.occlusion", fb.occlusion)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[0] != B):
            raise ValueError("%s must be None or a 4-D tensor of %d pairs" % (name, B))
    cuts = _check_cuts(cuts, B)
    out = FlowFB(*(t.clone() if t is not None else None for t in fb[:5]), fb.timing)
    if cuts:
        _kill_pairs(out, torch.tensor(cuts, dtype=torch.int64, device=fb.flow_fw.device))
    return out


def flow_video_shots(frames, pyramidLevels, *, cuts=None, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, **solver):
    """flow_video_fb of a video that has cuts: T >= 2 frames as flow_video_fb takes them; cuts: the pair indices that are cuts
    (as split_shots takes them), or None: detect_shots(frames, layout=layout) at its defaults finds them (the frames then have
    1 .. 4 channels).  flow_video_fb runs on every shot of at least two frames -- no solve is spent on a cut pair --, and the
    result is one FlowFB over all T - 1 pairs: a shot's pairs are flow_video_fb's on that shot alone, byte for byte, a cut
    pair is what cut_flows makes of it (NaN flows, occluded, warpI2_* zero); timing is the sum of the shots' timers.  An
    initial flow is refused: it would have to know the cuts.  Returns (FlowFB, Shots) -- for given cuts Shots(cuts, [], [],
    None, ranges).  Every argument error raises before anything is enqueued; complete on return."""
    torch = _torch()
    if "init_flow" in solver or "init_flow_bw" in solver:
        raise TypeError("flow_video_shots takes no initial flow: run flow_video_fb on split_shots' ranges to give one per shot")
    alphas = _alphas(consistency)
    ts, descs, out_dtype, params = _check([("frames", frames)], layout, out_dtype, pyramidLevels, min_frames=2, solver=solver)
    (T, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    if cuts is None:
        if C > MAX_CHANNELS:
            raise ValueError("frames must have 1 .. %d channels to detect the cuts, got %d (layout %s)" % (MAX_CHANNELS, C, layout))
        shots = detect_cuts(_cell_hist(ts, descs, 16, 16))
    else:
        cuts = _check_cuts(cuts, T - 1)
        shots = Shots(cuts, [], [], None, split_shots(T, cuts))
    flow_fw, warp_fw, _, _ = _outputs(T - 1, H, W, C, layout, out_dtype, dev)
    flow_bw, warp_bw, _, _ = _outputs(T - 1, H, W, C, layout, out_dtype, dev)
    occ = torch.empty((T - 1, 2, H, W), dtype=torch.bool, device=dev) if alphas[0] else None
    keys = capi.timing_keys()
    total = dict.fromkeys(keys, 0.0)
    out = FlowFB(flow_fw, flow_bw, warp_fw, warp_bw, occ, None)
    for start, stop in shots.ranges:
        if stop - start >= 2:
            sub = ts[0][start:stop]
            fb = _run_fb([sub], [descriptor(sub, layout)], True, stop - start - 1, layout, out_dtype, pyramidLevels, alphas,
                         params)
            for dst, src in zip(out[:5], fb[:5]):
                if dst is not None:
                    dst[start:stop - 1] = src
            for k in keys:
                total[k] += float(fb.timing[k])
        if stop < T:
            _kill_pairs(out, stop - 1)
    return out._replace(timing={k: "%f" % total[k] for k in keys}), shots


# ---- decoder surfaces (include/papof.h: papof_ycc_to_rgb_tensor, papof_rgb_to_ycc_tensor)
YCC_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}  # (Kr, Kb)
YCC_RANGES = ("limited", "full")
SITING_H = {"left": 0, "center": 1}
SITING_V = {"center": 0, "top": 1}
PACKED_422 = {"yuyv": (0, 1, 3), "yvyu": (0, 3, 1), "uyvy": (1, 0, 2), "vyuy": (1, 2, 0)}  # the first byte of y, cb, cr
NV12_PITCH = 256  # new_nv12 rounds the width up to a multiple of this, as decoders pad their rows


def ycc_tables(matrix="bt709", range="limited", *, reverse=False):
    """The integers that the surface kernels take for a matrix ("bt601", "bt709", "bt2020") and a range ("limited": luma 16 ..
    235, chroma 16 .. 240; "full"), at the scale 2^14 (include/papof.h).  Forward (ycc_to_rgb): [y_off, cy, crv, cgu, cgv, cbu]
    with cy = rint(2^14 * 255 / 219) and crv = rint(2^14 * 2 (1 - Kr) * 255 / 224) etc. for limited range, the plain factors for
    full range.  reverse=True (rgb_to_ycc): [y_off, yr, yg, yb, ur, ug, vg, vb], yg what is left of the luma weights' sum, so that
    a grey maps exactly.  The device knows no standard: other integers in 0 .. 65535 passed to the C ABI are another matrix."""
    if matrix not in YCC_MATRICES:
        raise ValueError("matrix must be one of %s, got %r" % (tuple(YCC_MATRICES), matrix))
    if range not in YCC_RANGES:
        raise ValueError("range must be one of %s, got %r" % (YCC_RANGES, range))
    kr, kb = YCC_MATRICES[matrix]
    kg = 1.0 - kr - kb
    y_off, sy, sc = (16, 219.0 / 255.0, 224.0 / 255.0) if range == "limited" else (0, 1.0, 1.0)
    one = float(1 << 14)
    if not reverse:
        return [y_off, round(one / sy)] + [round(one * f / sc) for f in (
            2.0 * (1.0 - kr), 2.0 * kb * (1.0 - kb) / kg, 2.0 * kr * (1.0 - kr) / kg, 2.0 * (1.0 - kb))]
    yr, yb = round(one * sy * kr), round(one * sy * kb)
    return [y_off, yr, round(one * sy) - yr - yb, yb] + [round(one * sc * 0.5 * f) for f in (
        kr / (1.0 - kb), kg / (1.0 - kb), kg / (1.0 - kr), kb / (1.0 - kr))]


def _check_surface_rule(matrix, range, siting, interlaced, sub_v, reverse):
    """(the tables as a ctypes array, siting_h, siting_v, interlaced, sub_v) of the surface calls' keywords"""
    tables = ycc_tables(matrix, range, reverse=reverse)
    try:
        sh, sv = siting
    except (TypeError, ValueError):
        raise TypeError("siting must be (horizontal, vertical), got %r" % (siting,)) from None
    if not isinstance(sh, str) or sh not in SITING_H or not isinstance(sv, str) or sv not in SITING_V:
        raise ValueError("siting must be (one of %s, one of %s), got %r" % (tuple(SITING_H), tuple(SITING_V), siting))
    if not isinstance(interlaced, (bool, int)) or interlaced not in (0, 1):
        raise ValueError("interlaced must be True or False, got %r" % (interlaced,))
    if isinstance(sub_v, bool) or not isinstance(sub_v, int) or sub_v not in (1, 2):
        raise ValueError("sub_v must be 2 (4:2:0) or 1 (4:2:2), got %r" % (sub_v,))
    return (ctypes.c_int * len(tables))(*tables), SITING_H[sh], SITING_V[sv], int(interlaced), sub_v


def _check_interlaced_height(interlaced, H):
    if interlaced and (H % 2 or H < 4):
        raise ValueError("interlaced surfaces have an even number of rows, at least 4, got %d" % H)


def _as_plane(name, t):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.uint8:
        raise TypeError("%s must be uint8, got %s" % (name, t.dtype))
    if t.dim() == 2:
        return t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("%s must be a 3-D plane (T, rows, columns) (or 2-D: one frame), got shape %s" % (name, tuple(t.shape)))
    return t


def _check_planes(y, cb, cr, sub_v, interlaced, size=None, written=False, as_plane=None):
    """the three planes of a surface as 3-D uint8 tensors on one HIP device, cb and cr of ceil(H / sub_v) x ceil(W / 2)
    samples; size: the (T, H, W) they must have; written: no zero strides; as_plane: _as_plane16 for planes of 16-bit words"""
    ps = [(as_plane or _as_plane)(n, t) for n, t in (("y", y), ("cb", cb), ("cr", cr))]
    T, H, W = (int(v) for v in ps[0].shape)
    if min(T, H, W) < 1:
        raise ValueError("empty surface: y has shape %s" % (tuple(ps[0].shape),))
    if size is not None and (T, H, W) != size:
        raise ValueError("y must be %s for these frames, got %s" % (size, (T, H, W)))
    want = (T, -(-H // sub_v), -(-W // 2))
    for n, p in zip(("cb", "cr"), ps[1:]):
        if tuple(p.shape) != want:
            raise ValueError("%s must be %s for y %s and sub_v %d, got %s" % (n, want, (T, H, W), sub_v, tuple(p.shape)))
    _check_interlaced_height(interlaced, H)
    for n, p in zip(("y", "cb", "cr"), ps):
        if p.device != ps[0].device:
            raise ValueError("%s is on %s, y on %s: all planes must be on one device" % (n, p.device, ps[0].device))
        if written and min(p.stride()) < 1:
            raise ValueError("%s is written: its strides must be positive, got %s" % (n, tuple(p.stride())))
    if not _on_gpu(ps[0]):
        raise ValueError("surfaces must be on a HIP device (cuda:N), got %s" % ps[0].device)
    return ps, (T, H, W)


def _plane_struct(p):
    return _struct(p, (p.stride(0), p.stride(1), p.stride(2), 0), capi.DTYPE_U8)


def ycc_to_rgb(y, cb, cr, *, matrix="bt709", range="limited", siting=("left", "center"), interlaced=False, sub_v=2,
               layout="NHWC", out_dtype=None):
    """A decoder's YCbCr planes as RGB frames (papof_ycc_to_rgb_tensor, one HIP kernel): y (T, H, W) uint8, cb and cr (T,
    ceil(H / sub_v), ceil(W / 2)) uint8 (2-D planes: one frame) with any non-negative strides on a HIP device -- views of the
    decoder's surface (nv12_planes, i420_planes, packed422_planes) are read in place.  sub_v: 2 for 4:2:0, 1 for 4:2:2.
    siting: (horizontal "left" | "center", vertical "center" | "top"), where the chroma samples sit; ("left", "center") is
    MPEG-2's and H.264's default.  interlaced=True: the surface holds two woven fields, and every row takes its chroma from
    the chroma lines of its own field (H even, >= 4; the vertical siting is then the standard's field positions).  matrix and
    range: ycc_tables'.  The rule is integer and stated in include/papof.h: bilinear chroma with weights that add to 32, carried
    unrounded into the matrix at the scale 2^14, one rounding -- a uint8 result is within 0.5156 LSB of the real-valued rule.
    Returns a new (T, H, W, 3) (NHWC) or (T, 3, H, W) (NCHW) tensor of out_dtype: torch.uint8 (the default) or float32 /
    float64, which get the unrounded value in 0 .. 1.  Enqueued on the current stream; returns without waiting."""
    torch = _torch()
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    tables, sh, sv, inter, sub_v = _check_surface_rule(matrix, range, siting, interlaced, sub_v, False)
    out_dtype = torch.uint8 if out_dtype is None else out_dtype
    if out_dtype not in (torch.uint8, torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.uint8, torch.float32 or torch.float64, got %s" % (out_dtype,))
    ps, (T, H, W) = _check_planes(y, cb, cr, sub_v, inter)
    out, d_out = _new_frames(T, H, W, 3, layout, out_dtype, ps[0].device)
    d = [_plane_struct(p) for p in ps]
    _launch(ps[0].device, "papof_ycc_to_rgb_tensor", T, H, W, ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]), sub_v,
            sh, sv, inter, tables, ctypes.byref(d_out))
    return out


def rgb_to_ycc(frames, *, matrix="bt709", range="limited", siting=("left", "center"), interlaced=False, sub_v=2,
               layout="NHWC", out=None):
    """RGB frames as the YCbCr planes an encoder takes (papof_rgb_to_ycc_tensor, one HIP kernel): frames (T, H, W, 3) or (T,
    3, H, W) by `layout` (3-D: one frame), uint8, float32 or float64 (quantised to 0 .. 65535 as field_metrics does), any
    strides, on a HIP device.  Luma per pixel; chroma computed per pixel unrounded, reduced with the adjoint taps of
    ycc_to_rgb's siting -- (1, 2, 1) / 4 or (1, 1) / 2 across and down, (3, 1) / 4 and (1, 3) / 4 within each field when
    interlaced -- and rounded once per sample, in 64-bit integers (include/papof.h).  The keywords are ycc_to_rgb's;
    ycc_tables(..., reverse=True) gives the integers.  out: None, or (y, cb, cr) uint8 tensors of (T, H, W) and twice (T,
    ceil(H / sub_v), ceil(W / 2)) with positive strides that are written in place -- the planes of an NV12 surface, whose pitch
    padding stays as it was.  Returns Surfaces(y, cb, cr): new contiguous planes, or `out`'s.  Enqueued on the current
    stream; returns without waiting."""
    torch = _torch()
    tables, sh, sv, inter, sub_v = _check_surface_rule(matrix, range, siting, interlaced, sub_v, True)
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    (T, H, W, C), strides, code = descs[0]
    if C != 3:
        raise ValueError("frames must have 3 channels (R, G, B), got %d (layout %s)" % (C, layout))
    _check_interlaced_height(inter, H)
    dev = ts[0].device
    if out is None:
        Hc, Wc = -(-H // sub_v), -(-W // 2)
        ps = [torch.empty(s, dtype=torch.uint8, device=dev) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc))]
    else:
        try:
            oy, ocb, ocr = out
        except (TypeError, ValueError):
            raise TypeError("out must be None or (y, cb, cr), got %r" % (type(out).__name__,)) from None
        ps, _ = _check_planes(oy, ocb, ocr, sub_v, inter, size=(T, H, W), written=True)
        if ps[0].device != dev:
            raise ValueError("out is on %s, frames on %s" % (ps[0].device, dev))
    d = [_plane_struct(p) for p in ps]
    d_in = _struct(ts[0], strides, code)
    _launch(dev, "papof_rgb_to_ycc_tensor", T, H, W, ctypes.byref(d_in), sub_v, sh, sv, inter, tables, ctypes.byref(d[0]),
            ctypes.byref(d[1]), ctypes.byref(d[2]))
    return Surfaces(*ps)


def _as_surface(surface):
    torch = _torch()
    if not isinstance(surface, torch.Tensor):
        raise TypeError("surface must be a torch.Tensor, got %s" % type(surface).__name__)
    if surface.dtype != torch.uint8:
        raise TypeError("surface must be uint8, got %s" % surface.dtype)
    if surface.dim() == 2:
        return surface.unsqueeze(0)
    if surface.dim() != 3:
        raise ValueError("surface must be (T, rows, bytes per row) (or 2-D: one frame), got shape %s" % (tuple(surface.shape),))
    return surface


def _surface_size(height, width, pitch, unit="bytes"):
    if isinstance(height, bool) or not isinstance(height, int) or height < 1:
        raise ValueError("height must be an integer >= 1, got %r" % (height,))
    if width is None:
        width = pitch
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= pitch:
        raise ValueError("width must be an integer in 1 .. %d (the %s of a row), got %r" % (pitch, unit, width))
    return height, width


def nv12_planes(surface, height, order="uv", *, width=None, sub_v=2):
    """The planes of a semi-planar surface as views -- nothing is copied: surface (T, rows, pitch) uint8 (2-D: one frame) on any
    device holds `height` rows of luma and below them ceil(height / sub_v) rows of interleaved chroma, rows >= their sum.
    order "uv": Cb first (NV12; NV16 with sub_v=1), "vu": Cr first (NV21, NV61).  width: the luma columns in use (by default
    the whole pitch).  Returns Surfaces(y (T, height, width), cb, cr (T, ceil(height / sub_v), ceil(width / 2)), column
    stride 2)."""
    s = _as_surface(surface)
    if order not in ("uv", "vu"):
        raise ValueError("order must be 'uv' or 'vu', got %r" % (order,))
    if sub_v not in (1, 2):
        raise ValueError("sub_v must be 2 (4:2:0) or 1 (4:2:2), got %r" % (sub_v,))
    H, W = _surface_size(height, width, int(s.shape[2]))
    Hc, Wc = -(-H // sub_v), -(-W // 2)
    if s.shape[1] < H + Hc or s.shape[2] < 2 * Wc:
        raise ValueError("a surface of %d x %d (sub_v %d) needs %d rows of %d bytes, got shape %s" % (
            H, W, sub_v, H + Hc, 2 * Wc, tuple(s.shape)))
    c = s[:, H:H + Hc]
    first, second = c[:, :, 0:2 * Wc:2], c[:, :, 1:2 * Wc:2]
    return Surfaces(s[:, :H, :W], *((first, second) if order == "uv" else (second, first)))


def i420_planes(surface, height, order="uv", *, width=None):
    """The planes of a planar 4:2:0 surface as views: surface (T, rows, pitch) uint8 (2-D: one frame) whose rows are adjacent
    in memory (pitch even) holds `height` rows of luma at `pitch`, then ceil(height / 2) rows of one chroma plane at pitch / 2,
    then the other's.  order "uv": Cb first (I420), "vu": Cr first (YV12).  Returns Surfaces(y (T, height, width), cb, cr (T,
    ceil(height / 2), ceil(width / 2)))."""
    s = _as_surface(surface)
    if order not in ("uv", "vu"):
        raise ValueError("order must be 'uv' or 'vu', got %r" % (order,))
    pitch = int(s.shape[2])
    H, W = _surface_size(height, width, pitch)
    Hc, Wc = -(-H // 2), -(-W // 2)
    if pitch % 2 or s.stride(2) != 1 or s.stride(1) != pitch:
        raise ValueError("a planar surface has adjacent rows of an even number of bytes, got shape %s strides %s" % (
            tuple(s.shape), tuple(s.stride())))
    if s.shape[1] * pitch < H * pitch + 2 * Hc * (pitch // 2):
        raise ValueError("a planar surface of %d rows needs %d bytes per frame, got %d" % (
            H, H * pitch + 2 * Hc * (pitch // 2), s.shape[1] * pitch))
    at = lambda i: s.as_strided((s.shape[0], Hc, Wc), (s.stride(0), pitch // 2, 1),  # noqa: E731
                                s.storage_offset() + H * pitch + i * Hc * (pitch // 2))
    return Surfaces(s[:, :H, :W], *((at(0), at(1)) if order == "uv" else (at(1), at(0))))


def packed422_planes(surface, order="yuyv"):
    """The planes of a packed 4:2:2 surface as views: surface (T, H, 2 W) uint8 (2-D: one frame), W even, four bytes per two
    pixels in `order`: "yuyv" (YUY2), "uyvy", "yvyu" or "vyuy".  Returns Surfaces(y (T, H, W) at column stride 2, cb, cr (T,
    H, W / 2) at column stride 4) for ycc_to_rgb(..., sub_v=1)."""
    s = _as_surface(surface)
    if order not in PACKED_422:
        raise ValueError("order must be one of %s, got %r" % (tuple(PACKED_422), order))
    if s.shape[2] % 4 or min(s.shape) < 1:
        raise ValueError("a packed 4:2:2 row is a multiple of 4 bytes, got shape %s" % (tuple(s.shape),))
    oy, ou, ov = PACKED_422[order]
    return Surfaces(s[:, :, oy::2], s[:, :, ou::4], s[:, :, ov::4])


def new_nv12(T, H, W, device, *, pitch=None):
    """A zeroed NV12 surface for T frames of H x W and its planes: (surface (T, H + ceil(H / 2), pitch) uint8 on `device`,
    nv12_planes(surface, H, width=W)); pitch: by default W rounded up to a multiple of 256."""
    for n, v in (("T", T), ("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (n, v))
    if pitch is None:
        pitch = -(-W // NV12_PITCH) * NV12_PITCH
    if isinstance(pitch, bool) or not isinstance(pitch, int) or pitch < 2 * -(-W // 2):
        raise ValueError("pitch must be an integer >= %d, got %r" % (2 * -(-W // 2), pitch))
    surface = _torch().zeros((T, H + -(-H // 2), pitch), dtype=_torch().uint8, device=device)
    return surface, nv12_planes(surface, H, width=W)


# ---- decoder surfaces of 9 .. 16 bits per sample in 16-bit words (include/papof.h: papof_ycc16_to_rgb_tensor,
# papof_rgb_to_ycc16_tensor)
DEPTHS = (9, 16)  # the least and the greatest depth
ALIGNED = ("msb", "lsb")  # the sample in the high bits of its word (P010, P016, Y210 ...) or in the low ones (I010 ...)
P010_PITCH = 256  # new_p010 rounds a row's bytes up to a multiple of this


def _check_depth(depth, aligned):
    """the shift of a sample within its word"""
    if isinstance(depth, bool) or not isinstance(depth, int) or not DEPTHS[0] <= depth <= DEPTHS[1]:
        raise ValueError("depth must be an integer in %d .. %d, got %r" % (DEPTHS + (depth,)))
    if aligned not in ALIGNED:
        raise ValueError("aligned must be one of %s, got %r" % (ALIGNED, aligned))
    return 16 - depth if aligned == "msb" else 0


def ycc_tables16(matrix="bt709", range="limited", depth=10, *, peak=None, reverse=False):
    """The integers that the 16-bit surface kernels take for a matrix, a range and a depth d in 9 .. 16 (include/papof.h).
    Forward (ycc16_to_rgb): [y_off, cy, crv, cgu, cgv, cbu, peak] with the coefficients at the scale 2^(d+6) for an output
    level `peak` that means 1.0 (by default P = 2^d - 1; 255 for a uint8 result): cy = rint(2^(d+6) peak / Sy), the others
    rint(2^(d+6) f peak / Sc) of ycc_tables' four factors f, with y_off, Sy, Sc = 16 m, 219 m, 224 m (m = 2^(d-8)) for limited
    range and 0, P, P for full range.  reverse=True (rgb_to_ycc16): [y_off, yr, yg, yb, ur, ug, vg, vb] at the scale 2^14 Sy
    and 2^14 Sc, yg what is left of 2^14 Sy.  The roundings are exact (rational arithmetic, ties to even)."""
    if matrix not in YCC_MATRICES:
        raise ValueError("matrix must be one of %s, got %r" % (tuple(YCC_MATRICES), matrix))
    if range not in YCC_RANGES:
        raise ValueError("range must be one of %s, got %r" % (YCC_RANGES, range))
    _check_depth(depth, "msb")
    F = fractions.Fraction
    P, m = (1 << depth) - 1, 1 << (depth - 8)
    kr, kb = (F(repr(k)) for k in YCC_MATRICES[matrix])
    kg = 1 - kr - kb
    y_off, sy, sc = (16 * m, 219 * m, 224 * m) if range == "limited" else (0, P, P)
    if reverse:
        if peak is not None:
            raise ValueError("peak belongs to the forward tables")
        yr, yb = round((sy << 14) * kr), round((sy << 14) * kb)
        return [y_off, yr, (sy << 14) - yr - yb, yb] + [round((sc << 13) * f) for f in (
            kr / (1 - kb), kg / (1 - kb), kg / (1 - kr), kb / (1 - kr))]
    peak = P if peak is None else peak
    if isinstance(peak, bool) or not isinstance(peak, int) or not 1 <= peak <= 65535:
        raise ValueError("peak must be an integer in 1 .. 65535, got %r" % (peak,))
    one = peak << (depth + 6)
    tables = [y_off, round(F(one, sy))] + [round(one * f / sc) for f in (
        2 * (1 - kr), 2 * kb * (1 - kb) / kg, 2 * kr * (1 - kr) / kg, 2 * (1 - kb))] + [peak]
    if max(tables[1:6]) >= 1 << (depth + 8):
        raise ValueError("peak %d is too large for depth %d: a coefficient reaches %d, the kernels take less than 2^%d" % (
            peak, depth, max(tables[1:6]), depth + 8))
    return tables


def _as_plane16(name, t):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in (torch.uint16, torch.int16):
        raise TypeError("%s must be uint16 (or int16 with the same bits), got %s" % (name, t.dtype))
    if t.dim() == 2:
        return t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("%s must be a 3-D plane (T, rows, columns) (or 2-D: one frame), got shape %s" % (name, tuple(t.shape)))
    return t


def _plane_struct16(p):
    return _struct(p, (p.stride(0), p.stride(1), p.stride(2), 0), capi.DTYPE_U16)


def ycc16_to_rgb(y, cb, cr, *, depth=10, aligned="msb", matrix="bt709", range="limited", siting=("left", "center"),
                 interlaced=False, sub_v=2, layout="NHWC", out_dtype=None):
    """A decoder's high-bit-depth YCbCr planes as RGB frames (papof_ycc16_to_rgb_tensor, one HIP kernel): ycc_to_rgb for samples
    of `depth` = 9 .. 16 bits in 16-bit words.  y (T, H, W), cb and cr (T, ceil(H / sub_v), ceil(W / 2)), torch.uint16 or
    torch.int16 with the same bits (2-D planes: one frame), any non-negative strides, on a HIP device -- views of the decoder's
    surface (p010_planes, i010_planes, y210_planes) are read in place.  aligned: "msb", the sample in the high bits of its word
    (P010, P012, P016, P210, Y210), or "lsb" (I010 / yuv420p10le, I012); the word's other bits are not looked at.  matrix,
    range, siting, interlaced, sub_v, layout: ycc_to_rgb's.  The rule is ycc_to_rgb's with wider integers (include/papof.h;
    ycc_tables16 gives them): a float result is the level over 2^depth - 1, within 2^-6 LSB of `depth` bits of the real-valued
    rule before its own rounding, so no bit of the surface is lost; a uint8 result is within 0.5156 LSB of 8 bits.  Returns a
    new (T, H, W, 3) (NHWC) or (T, 3, H, W) (NCHW) tensor of out_dtype: torch.float32 (the default), float64 or uint8.
    Enqueued on the current stream; returns without waiting."""
    torch = _torch()
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    shift = _check_depth(depth, aligned)
    _, sh, sv, inter, sub_v = _check_surface_rule(matrix, range, siting, interlaced, sub_v, False)
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out_dtype not in (torch.uint8, torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.uint8, torch.float32 or torch.float64, got %s" % (out_dtype,))
    tables = ycc_tables16(matrix, range, depth, peak=255 if out_dtype == torch.uint8 else None)
    ps, (T, H, W) = _check_planes(y, cb, cr, sub_v, inter, as_plane=_as_plane16)
    out, d_out = _new_frames(T, H, W, 3, layout, out_dtype, ps[0].device)
    d = [_plane_struct16(p) for p in ps]
    _launch(ps[0].device, "papof_ycc16_to_rgb_tensor", T, H, W, ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]), depth,
            shift, sub_v, sh, sv, inter, (ctypes.c_int * 7)(*tables), ctypes.byref(d_out))
    return out


def rgb_to_ycc16(frames, *, depth=10, aligned="msb", matrix="bt709", range="limited", siting=("left", "center"),
                 interlaced=False, sub_v=2, layout="NHWC", out=None):
    """RGB frames as high-bit-depth YCbCr planes (papof_rgb_to_ycc16_tensor, one HIP kernel): rgb_to_ycc for samples of `depth` =
    9 .. 16 bits in 16-bit words, stored as level << shift with every other bit of the word 0 (aligned: ycc16_to_rgb's).
    frames and the other keywords as rgb_to_ycc's; ycc_tables16(..., reverse=True) gives the integers.  A sample is within 0.5
    + 2^-13 LSB of `depth` bits of the real-valued rule.  out: None, or (y, cb, cr) uint16 / int16 tensors with positive
    strides that are written in place -- the planes of a P010 surface (new_p010), whose pitch padding stays as it was.  Returns
    Surfaces(y, cb, cr): new contiguous torch.uint16 planes, or `out`'s.  Enqueued on the current stream; returns without
    waiting."""
    torch = _torch()
    shift = _check_depth(depth, aligned)
    _, sh, sv, inter, sub_v = _check_surface_rule(matrix, range, siting, interlaced, sub_v, True)
    tables = ycc_tables16(matrix, range, depth, reverse=True)
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    (T, H, W, C), strides, code = descs[0]
    if C != 3:
        raise ValueError("frames must have 3 channels (R, G, B), got %d (layout %s)" % (C, layout))
    _check_interlaced_height(inter, H)
    dev = ts[0].device
    if out is None:
        Hc, Wc = -(-H // sub_v), -(-W // 2)
        ps = [torch.empty(s, dtype=torch.uint16, device=dev) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc))]
    else:
        try:
            oy, ocb, ocr = out
        except (TypeError, ValueError):
            raise TypeError("out must be None or (y, cb, cr), got %r" % (type(out).__name__,)) from None
        ps, _ = _check_planes(oy, ocb, ocr, sub_v, inter, size=(T, H, W), written=True, as_plane=_as_plane16)
        if ps[0].device != dev:
            raise ValueError("out is on %s, frames on %s" % (ps[0].device, dev))
    d = [_plane_struct16(p) for p in ps]
    d_in = _struct(ts[0], strides, code)
    _launch(dev, "papof_rgb_to_ycc16_tensor", T, H, W, ctypes.byref(d_in), depth, shift, sub_v, sh, sv, inter,
            (ctypes.c_int * 8)(*tables), ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(d[2]))
    return Surfaces(*ps)


def _as_surface16(surface):
    """a surface as (T, rows, words): uint16 / int16 as it is, uint8 (T, rows, bytes) with its rows reinterpreted"""
    torch = _torch()
    if not isinstance(surface, torch.Tensor):
        raise TypeError("surface must be a torch.Tensor, got %s" % type(surface).__name__)
    if surface.dtype not in (torch.uint16, torch.int16, torch.uint8):
        raise TypeError("surface must be uint16, int16 or uint8 (bytes), got %s" % surface.dtype)
    s = surface
    if s.dim() == 2:
        s = s.unsqueeze(0)
    if s.dim() != 3:
        raise ValueError("surface must be (T, rows, words per row) (or 2-D: one frame), got shape %s" % (tuple(surface.shape),))
    if s.dtype == torch.uint8:
        if s.shape[2] % 2 or s.stride(2) != 1 or s.stride(0) % 2 or s.stride(1) % 2 or s.storage_offset() % 2:
            raise ValueError("a surface of bytes is read as 16-bit words: it needs adjacent bytes, an even pitch and frame "
                             "stride and a 2-byte-aligned storage offset, got shape %s strides %s offset %d" % (
                                 tuple(s.shape), tuple(s.stride()), s.storage_offset()))
        s = s.view(torch.uint16)
    return s


def p010_planes(surface, height, order="uv", *, width=None, sub_v=2):
    """The planes of a semi-planar surface of 16-bit words as views -- nothing is copied: P010 / P012 / P016 (sub_v=2) and P210 /
    P216 (sub_v=1).  surface (T, rows, words per row) uint16 / int16, or (T, rows, bytes per row) uint8 whose rows are
    reinterpreted (2-D: one frame), on any device, holds `height` rows of luma and below them ceil(height / sub_v) rows of
    interleaved chroma.  order "uv": Cb first, "vu": Cr first.  width: the luma columns in use (by default the whole pitch).
    Returns Surfaces(y (T, height, width), cb, cr (T, ceil(height / sub_v), ceil(width / 2)) at column stride 2)."""
    s = _as_surface16(surface)
    if order not in ("uv", "vu"):
        raise ValueError("order must be 'uv' or 'vu', got %r" % (order,))
    if sub_v not in (1, 2):
        raise ValueError("sub_v must be 2 (4:2:0) or 1 (4:2:2), got %r" % (sub_v,))
    H, W = _surface_size(height, width, int(s.shape[2]), "words")
    Hc, Wc = -(-H // sub_v), -(-W // 2)
    if s.shape[1] < H + Hc or s.shape[2] < 2 * Wc:
        raise ValueError("a surface of %d x %d (sub_v %d) needs %d rows of %d words, got shape %s" % (
            H, W, sub_v, H + Hc, 2 * Wc, tuple(s.shape)))
    c = s[:, H:H + Hc]
    first, second = c[:, :, 0:2 * Wc:2], c[:, :, 1:2 * Wc:2]
    return Surfaces(s[:, :H, :W], *((first, second) if order == "uv" else (second, first)))


def i010_planes(surface, height, order="uv", *, width=None, sub_v=2):
    """The planes of a planar surface of 16-bit words as views: I010 / yuv420p10le, I012 (sub_v=2), yuv422p10le (sub_v=1); read
    them with aligned="lsb".  surface as p010_planes', its rows adjacent in memory and of an even number of words: `height`
    rows of luma at the pitch, then ceil(height / sub_v) rows of one chroma plane at half the pitch, then the other's.  order
    "uv": Cb first.  Returns Surfaces(y (T, height, width), cb, cr (T, ceil(height / sub_v), ceil(width / 2)))."""
    s = _as_surface16(surface)
    if order not in ("uv", "vu"):
        raise ValueError("order must be 'uv' or 'vu', got %r" % (order,))
    if sub_v not in (1, 2):
        raise ValueError("sub_v must be 2 (4:2:0) or 1 (4:2:2), got %r" % (sub_v,))
    pitch = int(s.shape[2])
    H, W = _surface_size(height, width, pitch, "words")
    Hc, Wc = -(-H // sub_v), -(-W // 2)
    if pitch % 2 or s.stride(2) != 1 or s.stride(1) != pitch:
        raise ValueError("a planar surface has adjacent rows of an even number of words, got shape %s strides %s" % (
            tuple(s.shape), tuple(s.stride())))
    if s.shape[1] * pitch < H * pitch + 2 * Hc * (pitch // 2):
        raise ValueError("a planar surface of %d rows (sub_v %d) needs %d words per frame, got %d" % (
            H, sub_v, H * pitch + 2 * Hc * (pitch // 2), s.shape[1] * pitch))
    at = lambda i: s.as_strided((s.shape[0], Hc, Wc), (s.stride(0), pitch // 2, 1),  # noqa: E731
                                s.storage_offset() + H * pitch + i * Hc * (pitch // 2))
    return Surfaces(s[:, :H, :W], *((at(0), at(1)) if order == "uv" else (at(1), at(0))))


def y210_planes(surface, order="yuyv"):
    """The planes of a packed 4:2:2 surface of 16-bit words as views (Y210, Y216): surface (T, H, 2 W words) as p010_planes', W
    even, four words per two pixels in `order` ("yuyv": Y210's).  Returns Surfaces(y (T, H, W) at column stride 2, cb, cr (T,
    H, W / 2) at column stride 4) for ycc16_to_rgb(..., sub_v=1) and rgb_to_ycc16(..., sub_v=1, out=)."""
    s = _as_surface16(surface)
    if order not in PACKED_422:
        raise ValueError("order must be one of %s, got %r" % (tuple(PACKED_422), order))
    if s.shape[2] % 4 or min(s.shape) < 1:
        raise ValueError("a packed 4:2:2 row is a multiple of 4 words, got shape %s" % (tuple(s.shape),))
    oy, ou, ov = PACKED_422[order]
    return Surfaces(s[:, :, oy::2], s[:, :, ou::4], s[:, :, ov::4])


def new_p010(T, H, W, device, *, pitch=None):
    """A zeroed P010 / P016 surface for T frames of H x W and its planes: (surface (T, H + ceil(H / 2), pitch / 2) uint16 on
    `device`, p010_planes(surface, H, width=W)); pitch: a row's BYTES, even, by default 2 W rounded up to a multiple of 256."""
    for n, v in (("T", T), ("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (n, v))
    if pitch is None:
        pitch = -(-2 * W // P010_PITCH) * P010_PITCH
    if isinstance(pitch, bool) or not isinstance(pitch, int) or pitch % 2 or pitch < 4 * -(-W // 2):
        raise ValueError("pitch must be an even integer >= %d (bytes), got %r" % (4 * -(-W // 2), pitch))
    surface = _torch().zeros((T, H + -(-H // 2), pitch // 2), dtype=_torch().uint16, device=device)
    return surface, p010_planes(surface, H, width=W)


MAX_RS_ITERS = 8 # include/papof.h: papof_rs_rectify_tensor
_F64_FLOWS = (capi.DTYPE_F64, capi.DTYPE_F64)  # the dtype codes of flow_video_fb's float64 flows


def _check_shutter(readout, anchor, iters, name="iters"):
    """(readout, anchor, iterations of the solve) of the rolling-shutter calls as (float, float, int) -- TypeError /
    ValueError otherwise"""
    for n, v in (("readout", readout), ("anchor", anchor)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s must be a number, got %r" % (n, v))
    if not (math.isfinite(readout) and abs(readout) <= 1):
        raise ValueError("readout must be finite and at most 1 in magnitude (in frame intervals), got %r" % (readout,))
    if not 0 <= anchor <= 1:
        raise ValueError("anchor must lie in [0, 1], got %r" % (anchor,))
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= MAX_RS_ITERS:
        raise ValueError("%s must be an integer in 1 .. %d, got %r" % (name, MAX_RS_ITERS, iters))
    return float(readout), float(anchor), iters


def _flow_dtype(out_dtype, default):
    """the dtype of an output flow, `default` for None -- TypeError unless float32 or float64"""
    torch = _torch()
    out_dtype = default if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.float32 or torch.float64, got %s" % out_dtype)
    return out_dtype


def _rectify(ts, descs, flows, codes, shutter, matrices, m_code, layout, out_dtype):
    """papof_rs_rectify_tensor of the checked frames ts[0]: (video, valid (T, H, W) bool)"""
    torch = _torch()
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(T, H, W, C, layout, out_dtype, dev)
    valid = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], strides, code)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    d_mat = None
    if matrices is not None:
        d_mat = _struct(matrices, (matrices.stride(0), matrices.stride(1), matrices.stride(2), 0), m_code)
    d_valid = _struct(valid, (valid.stride(0), valid.stride(1), valid.stride(2), 1), capi.DTYPE_U8)
    _launch(dev, "papof_rs_rectify_tensor", T, H, W, C, ctypes.byref(d_in), ctypes.byref(d_f[0]), ctypes.byref(d_f[1]), *shutter,
            _ref(d_mat), ctypes.byref(d_out), ctypes.byref(d_valid))
    return out, valid.view(torch.bool)


def _rectify_flows(flows, codes, shutter, out_dtype):
    """papof_rs_flow_tensor of the checked flows: Flows(flow_fw, flow_bw) of out_dtype"""
    torch = _torch()
    B, _, H, W = (int(x) for x in flows[0].shape)
    dev = flows[0].device
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    outs = [torch.empty((B, 2, H, W), dtype=out_dtype, device=dev) for _ in range(2)]
    d_o = [_flow_struct(o, _out_code(out_dtype)) for o in outs]
    _launch(dev, "papof_rs_flow_tensor", B + 1, H, W, ctypes.byref(d_f[0]), ctypes.byref(d_f[1]), *shutter, ctypes.byref(d_o[0]),
            ctypes.byref(d_o[1]))
    return Flows(*outs)


def rectify_frames(frames, flow_fw, flow_bw, readout, *, anchor=0.5, iters=3, matrices=None, layout="NCHW", out_dtype=None):
    """A rolling-shutter video of T >= 2 frames resampled to a global shutter's: frames (T, C, H, W) or (T, H, W, C) by
    `layout`, C = 1 .. 4, uint8 (read as x / 255), float32 or float64, any strides, on a HIP device; flow_fw, flow_bw
    (T - 1, 2, H, W) float32 / float64 on the same device, as flow_video_fb returns them for these frames.
    readout: the time the sensor takes from the first row to the last, in frame intervals, |readout| <= 1 (negative: read
    from the bottom up; phones are around 0.5 .. 0.9); anchor in [0, 1]: the row, as a fraction of H - 1, whose exposure
    is the frame's time (0.5: the middle row stays where it is).  Row y was exposed readout (y - a) / H after the
    frame's time.  The flows give where the pixel was one frame earlier and later, each landing at its own row's time; the
    parabola through the three points, evaluated that much earlier, is its global-shutter position P + L(P) (a line on
    the two end frames).  Output pixel Q is the frame sampled bilinearly at the P with P + L(P) = Q, found by `iters` (1 .. 8)
    fixed-point iterations P <- Q - L(P) from P = Q (the error falls by about |readout| |v| / H per iteration, v the
    vertical velocity in pixels per frame).  matrices: None, or (T, 2, 3) float32 / float64 on the same device: Q is
    warp_affine's M (x, y, 1) -- stabilizing_transforms' matrices -- so that the video is resampled once.
    Returns (video in `layout` and out_dtype -- by default the frames' --, valid (T, H, W) bool); a pixel whose Q or
    iterate leaves the image, or whose flows are NaN or say that it crossed more than half of the sensor's readout in one
    frame, is 0 and not valid.  readout = 0 gives the frames (with matrices: warp_affine's result).  include/papof.h
    (papof_rs_rectify_tensor) states the rule exactly.  What it is not: readout is not estimated; shake near half the
    frame rate is not recoverable from one flow per frame; dead pixels are not filled (stabilize_video_full fills
    borders); the mesh, homography and mosaic calls take rectified videos and flows but have no readout of their own.
    Enqueued on the current stream; returns without waiting."""
    shutter = _check_shutter(readout, anchor, iters)
    ts, descs, out_dtype, _ = _check_video(frames, layout, 1, out_dtype)
    (T, H, W, _), _, _ = descs[0]
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    m_code = _check_matrices(matrices, T, ts[0].device) if matrices is not None else None
    return _rectify(ts, descs, (flow_fw, flow_bw), codes, shutter, matrices, m_code, layout, out_dtype)


def rectify_flows(flow_fw, flow_bw, readout, *, anchor=0.5, iters=3, out_dtype=None):
    """The flows of the video that rectify_frames makes, from the flows of the recorded one -- no second estimation:
    flow_fw, flow_bw (T - 1, 2, H, W) float32 / float64 on one HIP device, any strides; readout, anchor, iters as
    rectify_frames'.  For pixel q of rectified frame i: P is rectify_frames' sampling point, the recorded flow at P takes
    it to P' in the next frame, and the rectified flow is P' + L(P') - q.  Returns Flows(flow_fw, flow_bw) of out_dtype
    (float32 / float64; by default flow_fw's), NaN where the solve is dead, P' leaves the image or L(P') is dead:
    fb_consistency marks those occluded and global_motion leaves them out.  readout = 0 gives finite input flows back
    wherever they land in the image.  include/papof.h (papof_rs_flow_tensor) states the rule exactly.  Enqueued on the
    current stream; returns without waiting."""
    shutter = _check_shutter(readout, anchor, iters)
    codes = _check_flows(flow_fw, flow_bw)
    out_dtype = _flow_dtype(out_dtype, flow_fw.dtype)
    return _rectify_flows((flow_fw, flow_bw), codes, shutter, out_dtype)


def rectify_video(frames, pyramidLevels, readout, *, anchor=0.5, iters=3, layout="NCHW", out_dtype=None,
                  consistency=CONSISTENCY, **solver):
    """A rolling-shutter video of T >= 2 frames and its flows rectified: flow_video_fb(frames, pyramidLevels, layout=layout,
    consistency=None, out_dtype=torch.float64, **solver), rectify_frames and rectify_flows on those flows, and
    fb_consistency(*consistency) on the rectified flows (None: no mask), where every dead pixel is occluded.  Returns
    Rectified(video, valid (T, H, W) bool, flow_fw, flow_bw (T - 1, 2, H, W) float64 -- the rectified video's --, occlusion
    (T - 1, 2, H, W) bool or None, timing of the flow call).  Every argument error raises before anything is launched."""
    alphas = _alphas(consistency)
    shutter = _check_shutter(readout, anchor, iters)
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    fb, flows, occ = _rectified_flows(ts, descs, layout, pyramidLevels, params, shutter, alphas)
    video, valid = _rectify(ts, descs, (fb.flow_fw, fb.flow_bw), _F64_FLOWS, shutter, None, None, layout, out_dtype)
    return Rectified(video, valid, flows.flow_fw, flows.flow_bw, occ, fb.timing)


def _rectified_flows(ts, descs, layout, levels, params, shutter, alphas):
    """the flow half of rectify_video on checked arguments: (the FlowFB of the recorded video, the rectified Flows, their
    occlusion or None)"""
    torch = _torch()
    fb = _run_fb(ts, descs, True, descs[0][0][0] - 1, layout, torch.float64, levels, _alphas(None), params)
    flows = _rectify_flows((fb.flow_fw, fb.flow_bw), _F64_FLOWS, shutter, torch.float64)
    occ = fb_consistency(flows.flow_fw, flows.flow_bw, *alphas[1:]) if alphas[0] else None
    return fb, flows, occ


def stabilize_video_rs(frames, pyramidLevels, readout, *, anchor=0.5, rs_iters=3, layout="NCHW", model="similarity",
                       radius=15, crop=1.0, iters=5, scale=1.0, consistency=CONSISTENCY, out_dtype=None, **solver):
    """stabilize_video for a rolling-shutter camera: flow_video_fb (float64 flows), rectify_flows (readout, anchor, rs_iters
    iterations of the solve), fb_consistency on the rectified flows (consistency; None: no mask), global_motion on the
    rectified forward flows with that mask (model, iters, scale) -- the fit no longer sees the shear --,
    stabilizing_transforms (radius, crop; the only wait) and ONE rectify_frames(matrices=transforms): the video is
    resampled once.  Returns StabilizedRS(video, valid (T, H, W) bool, transforms (T, 2, 3) float64, motion (T - 1, 2, 3)
    float64, ok (T - 1,) bool, flow_fw, flow_bw (T - 1, 2, H, W) float64 -- the rectified flows --, occlusion or None,
    timing of the flow call).  Every argument error raises before anything is launched; the video is enqueued on the
    current stream."""
    alphas = _alphas(consistency)
    shutter = _check_shutter(readout, anchor, rs_iters, "rs_iters")
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    code, iters, scale = _check_fit(model, iters, scale)
    (_, H, W, _), _, _ = descs[0]
    _check_path(radius, crop, (H, W))
    fb, flows, occ = _rectified_flows(ts, descs, layout, pyramidLevels, params, shutter, alphas)
    m = _motion_fit(flows.flow_fw, capi.DTYPE_F64, None if occ is None else occ.view(_torch().uint8), code, iters, scale)
    M = stabilizing_transforms(m, radius, crop, size=(H, W))
    video, valid = _rectify(ts, descs, (fb.flow_fw, fb.flow_bw), _F64_FLOWS, shutter, M, capi.DTYPE_F64, layout, out_dtype)
    return StabilizedRS(video, valid, M, m.motion, m.ok, flows.flow_fw, flows.flow_bw, occ, fb.timing)


MAX_ITERS = 65536  # include/papof.h: papof_temporal_consistency_tensor
# the defaults of temporal_consistency: calibrated in tests/test_consistency_cpu.py (test_quality_calibration)
LAM = 4.0
SIGMA = 0.05
ITERS = 20


def _check_solve(lam, sigma, iters):
    """(lam, sigma, iters) of temporal_consistency's keywords as (float, float, int) -- TypeError / ValueError otherwise"""
    for n, v in (("lam", lam), ("sigma", sigma)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s must be a number, got %r" % (n, v))
        if not (math.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, got %r" % (n, v))
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= MAX_ITERS:
        raise ValueError("iters must be an integer in 0 .. %d, got %r" % (MAX_ITERS, iters))
    return float(lam), float(sigma), iters


def _check_processed(ts, descs, processed, layout, out_dtype):
    """processed (T, C_P, H, W) / (T, H, W, C_P) of the frames' T, H, W and device: (tensor, descriptor, out_dtype)"""
    p = _as4d("processed", processed)
    d = descriptor(p, layout)
    (T, H, W, _), _, _ = descs[0]
    if d[0][:3] != (T, H, W):
        raise ValueError("processed %s and frames %s differ in frames or size (layout %s)" % (tuple(p.shape),
                                                                                           tuple(ts[0].shape), layout))
    if not 1 <= d[0][3] <= MAX_CHANNELS:
        raise ValueError("processed must have 1 .. %d channels, got %d (layout %s)" % (MAX_CHANNELS, d[0][3], layout))
    if p.device != ts[0].device:
        raise ValueError("processed is on %s, the frames on %s: all must be on one device" % (p.device, ts[0].device))
    return p, d, _out_dtype(out_dtype, p.dtype)


def _check_first(first, layout, H, W, C, dev):
    """None, or the descriptor of one frame of C channels -- (C, H, W) / (H, W, C) by layout, or 4-D with one frame"""
    if first is None:
        return None
    f = _as4d("first", first)
    if f.shape[0] != 1:
        raise ValueError("first must be one frame, got shape %s" % (tuple(first.shape),))
    d = descriptor(f, layout)
    if d[0][1:] != (H, W, C):
        raise ValueError("first is %s, the output's frames are (H, W, C) = %s (layout %s)" % (tuple(first.shape), (H, W, C),
                                                                                            layout))
    if f.device != dev:
        raise ValueError("first is on %s, the frames on %s: all must be on one device" % (f.device, dev))
    return _struct(f, d[1], d[2])


def _consistency(ts, descs, p, d_p, flows, codes, d_first, lam, sigma, iters, alphas, layout, out_dtype):
    (T, H, W, CI), strides, code = descs[0]
    CP = d_p[0][3]
    out, d_out = _new_frames(T, H, W, CP, layout, out_dtype, ts[0].device)
    d_in = _struct(ts[0], strides, code)
    d_pr = _struct(p, d_p[1], d_p[2])
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)]
    _launch(ts[0].device, "papof_temporal_consistency_tensor", T, H, W, CI, CP, ctypes.byref(d_in), ctypes.byref(d_pr),
            ctypes.byref(d_f[0]), ctypes.byref(d_f[1]), _ref(d_first), lam, sigma, iters, *alphas, ctypes.byref(d_out),
            workspace=("papof_consistency_workspace", (H, W, CP),
                       "frames of %d x %d x %d are too large for temporal_consistency" % (H, W, CP)))
    return out


def temporal_consistency(frames, processed, flow_fw, flow_bw, *, lam=LAM, sigma=SIGMA, iters=ITERS, consistency=CONSISTENCY,
                         first=None, layout="NCHW", out_dtype=None):
    """Blind video temporal consistency (Bonneel et al., SIGGRAPH Asia 2015): `processed`, the output of a per-frame process
    (a network, a tone mapper, a colour grade) run on the video `frames`, made consistent along the frames' flows -- the
    flicker of processing each frame on its own removed without knowing the process.
    frames (T, C_I, H, W) or (T, H, W, C_I) by `layout`, processed (T, C_P, H, W) / (T, H, W, C_P), T >= 2, C_I and C_P in
    1 .. 4 (they may differ), uint8 (read as x / 255), float32 or float64, any strides, on one HIP device; flow_fw, flow_bw
    (T - 1, 2, H, W) float32 / float64 of the frames, pair t from frame t to t + 1 and back, as flow_video_fb returns them.
    Output frame 0 is `first` -- one frame of C_P channels, (C_P, H, W) / (H, W, C_P) by layout or 4-D with one frame -- or
    processed[0].  Each later output frame O_t keeps processed[t]'s spatial gradients and, where flow_bw[t - 1] lands inside
    the image and passes the forward-backward check (consistency = (alpha1, alpha2); None: no check), follows the previous
    output frame warped along it with the weight w = lam / (1 + D / sigma^2), D the mean squared difference of the frames
    along the hop (sigma 0: w = lam): a screened-Poisson solve per frame, started from a pull-push of the warped residual and
    relaxed by `iters` Jacobi sweeps (0 .. 65536).  lam = 0 gives processed back (in out_dtype; a float -0.0 as +0.0).
    The defaults lam = 4, sigma = 0.05, iters = 20 were calibrated on the committed frames with the oracle's flows
    (tests/test_consistency_cpu.py): 8 frames of 200 x 120 panned across the 1080p frame, processed with random per-frame,
    per-channel gains in [0.8, 1.2] and offsets in [-0.1, 0.1].  PSNR against the flicker-free target and the temporal
    warping error (mean squared O_t - warped O_{t-1} over the valid pixels):
        processed as is                    19.98 dB   1.44e-2
        lam 0.5, sigma 0.1, iters 50       35.58 dB   1.21e-4
        lam 1,   sigma 0.05, iters 20      36.73 dB   6.68e-5
        lam 4,   sigma 0.05, iters 20      39.10 dB   1.38e-5     (the defaults; 55.69 dB with processed = frames)
        lam 8,   sigma 0.05, iters 20      39.99 dB   5.29e-6     (53.11 dB with processed = frames)
    A larger lam follows the warped past more closely and blurs more where nothing flickers.
    Returns the consistent video in `layout` and out_dtype (uint8 as clamp(rint(255 x), 0, 255), float32 or float64; by
    default processed's dtype).  include/papof.h (papof_temporal_consistency_tensor) states the rule exactly.  The workspace
    comes from PyTorch's allocator; the T - 1 frames are enqueued back to back on the current stream, and the call returns
    without waiting.
    A long video in chunks: let the chunks overlap by one frame and pass the previous chunk's last output frame as `first`
    (with the same out_dtype): the previous output is read back from the stored output, so the chunks give the bytes of one
    call."""
    alphas = _alphas(consistency)
    lam, sigma, iters = _check_solve(lam, sigma, iters)
    ts, descs, _, _ = _check_video(frames, layout, 1, None)
    (T, H, W, _), _, _ = descs[0]
    p, d_p, out_dtype = _check_processed(ts, descs, processed, layout, out_dtype)
    codes = _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), ts[0].device)
    d_first = _check_first(first, layout, H, W, d_p[0][3], ts[0].device)
    return _consistency(ts, descs, p, d_p, (flow_fw, flow_bw), codes, d_first, lam, sigma, iters, alphas, layout,
                        out_dtype)


def consistent_video(frames, processed, pyramidLevels, *, flows=None, lam=LAM, sigma=SIGMA, iters=ITERS,
                     consistency=CONSISTENCY, first=None, layout="NCHW", out_dtype=None, **solver):
    """`processed` made temporally consistent along the flows of `frames` (T >= 2): flow_video_fb(frames, pyramidLevels,
    layout=layout, consistency=None, out_dtype=torch.float64, **solver) -- or flows = (flow_fw, flow_bw) as it returns them --
    followed by temporal_consistency (lam, sigma, iters, consistency, first, out_dtype).  Returns Consistent(video, flow_fw,
    flow_bw, timing of the flow call (None with given flows)).  Every argument error raises before anything is launched;
    the video is enqueued on the current stream behind the flows."""
    alphas = _alphas(consistency)
    lam, sigma, iters = _check_solve(lam, sigma, iters)
    ts, descs, _, params = _check_video(frames, layout, pyramidLevels, None, solver=solver)
    (T, H, W, _), _, _ = descs[0]
    p, d_p, out_dtype = _check_processed(ts, descs, processed, layout, out_dtype)
    d_first = _check_first(first, layout, H, W, d_p[0][3], ts[0].device)
    flow_fw, flow_bw, codes, timing = _given_or_run_fb(flows, ts, descs, layout, pyramidLevels, params)
    video = _consistency(ts, descs, p, d_p, (flow_fw, flow_bw), codes, d_first, lam, sigma, iters, alphas, layout,
                         out_dtype)
    return Consistent(video, flow_fw, flow_bw, timing)


MAX_REFINE_RADIUS = 15  # include/papof.h: papof_refine_flow_tensor
REFINE_BINS = 4096
RADIUS, SIGMA_S, SIGMA_C = 7, 7.0, 7.0 / 255.0  # Sun, Roth and Black: a 15 x 15 window, 7 pixels, 7 grey levels


def _check_refine(radius, sigma_s, sigma_c, iters):
    """(radius, sigma_s, sigma_c, iters) as int, float, float, int -- TypeError / ValueError otherwise"""
    for name, v in (("radius", radius), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("%s must be an int, got %r" % (name, v))
    if not 1 <= radius <= MAX_REFINE_RADIUS:
        raise ValueError("radius must be in 1 .. %d, got %d" % (MAX_REFINE_RADIUS, radius))
    if iters < 1 or iters > MAX_ITERS:
        raise ValueError("iters must be in 1 .. %d, got %d" % (MAX_ITERS, iters))
    sig = []
    for name, v in (("sigma_s", sigma_s), ("sigma_c", sigma_c)):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise TypeError("%s must be a number, got %r" % (name, v)) from None
        if not (math.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and > 0, got %r" % (name, v))
        sig.append(v)
    return radius, sig[0], sig[1], iters


def refine_tables(radius, sigma_s):
    """The two integer tables of refine_flow as numpy uint32 arrays, made by the library on the host (include/papof.h:
    papof_refine_tables): S ((2 radius + 1)^2,) = rint(32768 exp(-(dx^2 + dy^2) / (2 sigma_s^2))), row-major in (dy, dx), and
    R (4096,) = rint(65536 exp(-(k + 0.5) / 256))."""
    import numpy as np
    radius, sigma_s, _, _ = _check_refine(radius, sigma_s, 1.0, 1)
    S, R = np.zeros((2 * radius + 1) ** 2, np.uint32), np.zeros(REFINE_BINS, np.uint32)
    U = ctypes.POINTER(ctypes.c_uint)
    capi._chk(capi.load().papof_refine_tables(radius, sigma_s, S.ctypes.data_as(U), R.ctypes.data_as(U)), "papof_refine_tables")
    return S, R


def refine_q(sigma_c, channels, uint8):
    """The factor q of papof_refine_flow_tensor, in fp64: 128 / (sigma_c^2 C), over 255^2 for a uint8 guide"""
    q = 128.0 / (sigma_c * sigma_c * channels)
    return q / 65025.0 if uint8 else q


def _check_plane_mask(name, m, shape, dev):
    """None, or a bool / uint8 mask of `shape` = (B, H, W) on `dev`: its descriptor (item, row, column, -) and the uint8 view
    that owns the memory -- TypeError / ValueError otherwise"""
    if m is None:
        return None, None
    torch = _torch()
    if not isinstance(m, torch.Tensor):
        raise TypeError("%s must be None or a torch.Tensor, got %s" % (name, type(m).__name__))
    if m.dtype not in (torch.bool, torch.uint8):
        raise TypeError("%s must be torch.bool or torch.uint8, got %s" % (name, m.dtype))
    if tuple(m.shape) != shape:
        raise ValueError("%s must be (B, H, W) = %s, got %s" % (name, shape, tuple(m.shape)))
    if m.device != dev:
        raise ValueError("%s is on %s, the flow on %s: all must be on one device" % (name, m.device, dev))
    m = m.view(torch.uint8)
    return _struct(m, (m.stride(0), m.stride(1), m.stride(2), 0), capi.DTYPE_U8), m


def _check_refine_flow(flow, guide, occlusion, where, layout, out_dtype):
    """every argument error of refine_flow's tensors: (the guide as 4-D, its descriptor, the flow's code, the masks'
    descriptors and views, out_dtype)"""
    torch = _torch()
    ts, descs, _, _ = _check([("guide", guide)], layout, None, 1)
    (B, H, W, C), _, _ = descs[0]
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError("the guide must have 1 .. %d channels, got %d" % (MAX_CHANNELS, C))
    dev = ts[0].device
    code = _check_flow("flow", flow)
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("flow must be %s for this guide, got %s" % ((B, 2, H, W), tuple(flow.shape)))
    if flow.device != dev:
        raise ValueError("flow is on %s, the guide on %s: all must be on one device" % (flow.device, dev))
    out_dtype = flow.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.float32 or torch.float64, got %s" % out_dtype)
    occ = _check_plane_mask("occlusion", occlusion, (B, H, W), dev)
    wh = _check_plane_mask("where", where, (B, H, W), dev)
    return ts[0], descs[0], code, occ, wh, out_dtype


_tables = collections.OrderedDict()  # (device ordinal, radius, sigma_s[, factor]) -> the two tables on the device, the last 16 used
MAX_TABLES = 16


def _device_tables(dev, radius, sigma_s, factor=None):
    """refine_tables(radius, sigma_s) -- with a factor: upsample_tables(factor, radius, sigma_s) -- on `dev` as int32 tensors
    (entries below 2^31: the same bits).  They are uploaded once per (device, radius, sigma_s, factor) and the upload is
    waited for, so later calls read finished, immutable tables from any stream and enqueue no copy; only the first call with
    new parameters blocks the host."""
    torch = _torch()
    index = _index(dev)
    stream = torch.cuda.current_stream(index)
    key = (index, radius, sigma_s) if factor is None else (index, radius, sigma_s, factor)
    with _lock:
        got = _tables.pop(key, None)
        if got is None:
            made = refine_tables(radius, sigma_s) if factor is None else upsample_tables(factor, radius, sigma_s)
            with torch.cuda.device(index):
                got = tuple(torch.from_numpy(t.view("int32")).to(dev) for t in made)
            stream.synchronize()
        _tables[key] = got
        while len(_tables) > MAX_TABLES:
            _tables.popitem(last=False)
    for t in got:
        t.record_stream(stream)  # (an evicted table is reused only behind the kernels that read it)
    return got


def _refine(flow, code, guide, desc, occ, wh, radius, sigma_s, sigma_c, iters, out_dtype, passes=False):
    """papof_refine_flow_tensor on the current stream of the flow's device"""
    torch = _torch()
    (B, H, W, C), strides, g_code = desc
    dev = flow.device
    q = refine_q(sigma_c, C, g_code == capi.DTYPE_U8)
    d_S, d_R = _device_tables(dev, radius, sigma_s)
    out = torch.empty((B, 2, H, W), dtype=out_dtype, device=dev)
    count = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if passes else None
    d_count = _struct(count, (H * W, W, 1, 0), capi.DTYPE_U8) if passes else None
    d_flow, d_guide, d_out = _flow_struct(flow, code), _struct(guide, strides, g_code), _flow_struct(out, _out_code(out_dtype))
    _launch(dev, "papof_refine_flow_tensor", B, H, W, C, ctypes.byref(d_flow), ctypes.byref(d_guide), _ref(occ[0]), _ref(wh[0]),
            radius, ctypes.c_void_p(d_S.data_ptr()), ctypes.c_void_p(d_R.data_ptr()), q, iters, ctypes.byref(d_out),
            _ref(d_count), workspace=("papof_refine_workspace", (B, H, W, iters),
                                      "%d flows of %d x %d are too large to refine" % (B, H, W)))
    return (out, count) if passes else out


def refine_flow(flow, guide, *, occlusion=None, where=None, radius=RADIUS, sigma_s=SIGMA_S, sigma_c=SIGMA_C, iters=1,
                layout="NCHW", out_dtype=None):
    """Edge-aware refinement of flow fields: the weighted median filter of Sun, Roth and Black (2010) guided by an image.
    flow: (B, 2, H, W) float32 / float64, any strides, on a HIP device.  guide: (B, C, H, W) or (B, H, W, C) by `layout`
    (3-D: one item), C in 1 .. 4, uint8, float32 or float64 (a float guide is taken to be scaled to 0 .. 1, a uint8 guide
    to 0 .. 255), any strides -- usually the frame the flow starts from.  occlusion: None or a (B, H, W) bool / uint8 mask,
    nonzero = this pixel's flow is not to be trusted (it gets no vote and, filtered, takes its neighbours' motion); where:
    None or a (B, H, W) bool / uint8 mask, nonzero = filter this pixel, the others are copied.  Each output pixel is, per
    component, the lower weighted median of the flows in the (2 radius + 1)^2 window around it, radius in 1 .. 15, with the
    weights exp(-distance^2 / (2 sigma_s^2)) * exp(-d2 / (2 sigma_c^2)), d2 the mean squared difference of the guide over
    its channels (sigma_c in units of a guide scaled to 0 .. 1), zero for neighbours that are outside the image, occluded or
    not finite; a pixel whose window holds no weight keeps its flow.  The weights are products of two integer tables
    (refine_tables) and the sums 64-bit integers, so the result is the bits of one of the window's values and bitwise
    reproducible; include/papof.h (papof_refine_flow_tensor) states the rule exactly.  iters > 1 repeats the pass on its own
    output.  Returns the refined flow (B, 2, H, W) of out_dtype (float32 / float64; by default the flow's), a new tensor.
    The defaults are the paper's (15 x 15, 7 pixels, 7 grey levels).  Enqueued on the current stream; returns without
    waiting."""
    radius, sigma_s, sigma_c, iters = _check_refine(radius, sigma_s, sigma_c, iters)
    g, desc, code, occ, wh, out_dtype = _check_refine_flow(flow, guide, occlusion, where, layout, out_dtype)
    return _refine(flow, code, g, desc, occ, wh, radius, sigma_s, sigma_c, iters, out_dtype)


def refine_video_flows(frames, flow_fw, flow_bw, *, occlusion=None, consistency=CONSISTENCY, layout="NCHW", **refine):
    """Both directions of a video's flows refined in one launch: frames (T, C, H, W) or (T, H, W, C) by `layout`, T >= 2,
    flow_fw / flow_bw (T - 1, 2, H, W) and occlusion (None, or the (T - 1, 2, H, W) bool / uint8 mask) as flow_video_fb
    returns them.  The forward flows are guided by frames[:-1] and distrust the pixels of occlusion's channel 0, the
    backward flows by frames[1:] and channel 1; `refine`: refine_flow's radius, sigma_s, sigma_c, iters, out_dtype.
    Returns RefinedFlows(flow_fw, flow_bw, occlusion): the refined flows (views of one tensor) and the mask recomputed from
    them by fb_consistency(*consistency) -- None for consistency=None.  Every argument error raises before anything is
    launched."""
    torch = _torch()
    unknown = set(refine) - {"radius", "sigma_s", "sigma_c", "iters", "out_dtype"}
    if unknown:
        raise TypeError("unknown refinement parameter %r" % sorted(unknown)[0])
    _, a1, a2 = _alphas(consistency)
    radius, sigma_s, sigma_c, iters = _check_refine(refine.get("radius", RADIUS), refine.get("sigma_s", SIGMA_S),
                                                    refine.get("sigma_c", SIGMA_C), refine.get("iters", 1))
    ts, descs, _, _ = _check_video(frames, layout, 1, None)
    (T, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), dev)
    occ = _check_occlusion(occlusion, (T - 1, 2, H, W), dev)
    common = torch.promote_types(flow_fw.dtype, flow_bw.dtype)
    out_dtype = common if refine.get("out_dtype") is None else refine["out_dtype"]
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.float32 or torch.float64, got %s" % out_dtype)
    flows = torch.cat((flow_fw.to(common), flow_bw.to(common)))
    guide = torch.cat((ts[0][:-1], ts[0][1:]))
    mask = torch.cat((occ[:, 0], occ[:, 1])) if occ is not None else None
    g, desc, code, d_occ, wh, out_dtype = _check_refine_flow(flows, guide, mask, None, layout, out_dtype)
    out = _refine(flows, code, g, desc, d_occ, wh, radius, sigma_s, sigma_c, iters, out_dtype)
    fw, bw = out[:T - 1], out[T - 1:]
    return RefinedFlows(fw, bw, fb_consistency(fw, bw, a1, a2) if consistency is not None else None)


SuperResolved = collections.namedtuple("SuperResolved", "video coverage")
SuperResolvedVideo = collections.namedtuple("SuperResolvedVideo", "video coverage flow_fw flow_bw timing")
SCALES = (2, 3, 4)  # include/papof.h: papof_super_resolve_tensor
MIN_PRIOR = 2.0 ** -24
# the defaults of super_resolve: chosen in tests/test_superres_cpu.py (test_quality_estimated_flows) over a small grid
SR_SIGMA = 0.15
SR_PRIOR = 0.05
SR_ITERS = 2


def _check_sr(scale, radius, sigma, prior, iters):
    """(scale, radius, use_sigma, sigma, prior, iters) of super_resolve's keywords -- TypeError / ValueError otherwise"""
    for name, v in (("scale", scale), ("radius", radius), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("%s must be an int, got %r" % (name, v))
    if scale not in SCALES:
        raise ValueError("scale must be one of %s, got %r" % (SCALES, scale))
    if radius < 0:
        raise ValueError("radius must be >= 0, got %r" % radius)
    if not 0 <= iters <= MAX_ITERS:
        raise ValueError("iters must be in 0 .. %d, got %r" % (MAX_ITERS, iters))
    if sigma is not None:
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
            raise TypeError("sigma must be None or a number, got %r" % (sigma,))
        if not (math.isfinite(sigma) and sigma >= 0):
            raise ValueError("sigma must be finite and >= 0, got %r" % (sigma,))
    if isinstance(prior, bool) or not isinstance(prior, (int, float)):
        raise TypeError("prior must be a number, got %r" % (prior,))
    if not (math.isfinite(prior) and prior >= MIN_PRIOR):
        raise ValueError("prior must be finite and at least 2^-24, got %r" % (prior,))
    return scale, radius, 1 if sigma else 0, float(sigma or 0.0), float(prior), iters


def _check_sr_flows(flow_fw, flow_bw, T, H, W, dev):
    """the dtype codes of the flows of T frames -- for T = 1 two empty (0, 2, H, W) tensors, which are not read: None"""
    if T > 1:
        return _check_flows(flow_fw, flow_bw, (T - 1, 2, H, W), dev)
    torch = _torch()
    for name, f in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
        if not isinstance(f, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(f).__name__))
        if f.dtype not in (torch.float32, torch.float64):
            raise TypeError("%s must be float32 or float64, got %s" % (name, f.dtype))
        if tuple(f.shape) != (0, 2, H, W):
            raise ValueError("the flows must be %s for these frames, got %s" % ((0, 2, H, W), tuple(f.shape)))
    return None


def _check_sr_size(H, W, radius):
    """the bound of the fixed-point sums (include/papof.h: papof_super_resolve_tensor)"""
    if (2 * radius + 1) * H * W >= 2 ** 30:
        raise ValueError("(2 radius + 1) H W must stay below 2^30, got radius %d and %d x %d frames" % (radius, H, W))


def _super_resolve(ts, descs, flows, codes, scale, radius, use_sigma, sigma, alphas, prior, iters, layout, out_dtype):
    torch = _torch()
    (T, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(T, scale * H, scale * W, C, layout, out_dtype, dev)
    coverage = torch.empty((T, scale * H, scale * W), dtype=torch.float64, device=dev)
    d_cov = _struct(coverage, (coverage.stride(0), coverage.stride(1), coverage.stride(2), 1), capi.DTYPE_F64)
    d_in = _struct(ts[0], strides, code)
    d_f = [_flow_struct(f, c) for f, c in zip(flows, codes)] if codes is not None else [None, None]
    _launch(dev, "papof_super_resolve_tensor", T, H, W, C, scale, ctypes.byref(d_in), _ref(d_f[0]), _ref(d_f[1]), radius,
            use_sigma, sigma, *alphas, prior, iters, ctypes.byref(d_out), ctypes.byref(d_cov),
            workspace=("papof_sr_workspace", (T, H, W, C, scale, iters),
                       "%d frames of %d x %d x %d are too large to super-resolve" % (T, H, W, C)))
    return SuperResolved(out, coverage)


def super_resolve(frames, flow_fw, flow_bw, scale=2, *, radius=2, sigma=SR_SIGMA, consistency=CONSISTENCY, prior=SR_PRIOR,
                  iters=SR_ITERS, layout="NCHW", out_dtype=None):
    """Multi-frame super-resolution of a video of T >= 1 frames along its flows (shift and add, Farsiu et al. 2004, and
    back-projection, Irani and Peleg 1991): frames (T, C, H, W) or (T, H, W, C) by `layout`, C = 1 .. 4, uint8 (read as
    x / 255), float32 or float64, any strides, on a HIP device; flow_fw, flow_bw (T - 1, 2, H, W) float32 / float64 on the
    same device, pair t from frame t to t + 1 and back, as flow_video_fb returns them.  scale: 2, 3 or 4.
    Every pixel of every frame follows its chain through the flows to the frames up to `radius` before and after it, hop
    by hop as temporal_filter does (a chain ends where it leaves the image or -- consistency = (alpha1, alpha2); None: no
    check -- where the reverse flow does not bring it back), and is DEPOSITED where it lands, on that frame's grid made
    `scale` times finer (bilinearly, on the four fine pixels around the point), with the weight 1 / (1 + D / sigma^2), D the
    mean squared difference over the channels of the pixel and the frame it lands in (sigma=None or 0: weight 1).  Each
    frame deposits itself with weight 1.  The sums are 64-bit fixed-point integers added atomically: bitwise reproducible.
    Each fine pixel is then (sum of the deposits + prior * the cubic upsampling of the frame) / (sum of the weights +
    prior) -- prior >= 2^-24 keeps every pixel defined and is the whole answer where nothing lands -- and `iters` steps of
    back-projection follow: the difference between the frame and the scale x scale block means of the result, upsampled
    bilinearly, is added (iters=0: none).
    What this is not: the sensor model is the scale x scale box alone, so there is no deconvolution of the optics' blur
    beyond it, and there is no learned prior.  A video without sub-pixel motion has nothing to add: the result is then
    close to bilinear (scale 2) or cubic (scale 3) upsampling of each frame (tests/test_superres_cpu.py).
    Returns SuperResolved(video (T, C, scale H, scale W) or (T, scale H, scale W, C) of out_dtype -- uint8 as
    clamp(rint(255 x), 0, 255), float32 or float64; by default the frames' dtype --, coverage (T, scale H, scale W) float64:
    the sum of the weights that landed on each fine pixel).  include/papof.h (papof_super_resolve_tensor) states the rule
    exactly.  The workspace comes from PyTorch's allocator; enqueued on the current stream, returns without waiting."""
    alphas = _alphas(consistency)
    scale, radius, use_sigma, sigma, prior, iters = _check_sr(scale, radius, sigma, prior, iters)
    ts, descs, out_dtype, _ = _check_video(frames, layout, 1, out_dtype, min_frames=1)
    (T, H, W, C), _, _ = descs[0]
    _check_sr_size(H, W, radius)
    codes = _check_sr_flows(flow_fw, flow_bw, T, H, W, ts[0].device)
    return _super_resolve(ts, descs, (flow_fw, flow_bw), codes, scale, radius, use_sigma, sigma, alphas, prior, iters, layout,
                          out_dtype)


def super_resolve_video(frames, pyramidLevels, scale=2, *, flows=None, radius=2, sigma=SR_SIGMA, consistency=CONSISTENCY,
                        prior=SR_PRIOR, iters=SR_ITERS, layout="NCHW", out_dtype=None, **solver):
    """A video of T >= 2 frames super-resolved along its motion: flow_video_fb(frames, pyramidLevels, layout=layout,
    consistency=None, out_dtype=torch.float64, **solver) -- or flows = (flow_fw, flow_bw) as it returns them -- followed by
    super_resolve on them (scale, radius, sigma, consistency, prior, iters, out_dtype).  Returns
    SuperResolvedVideo(video, coverage, flow_fw, flow_bw, timing of the flow call (None with given flows)).  Every argument
    error raises before anything is launched; the video is enqueued on the current stream behind the flows."""
    alphas = _alphas(consistency)
    scale, radius, use_sigma, sigma, prior, iters = _check_sr(scale, radius, sigma, prior, iters)
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    (T, H, W, C), _, _ = descs[0]
    _check_sr_size(H, W, radius)
    flow_fw, flow_bw, codes, timing = _given_or_run_fb(flows, ts, descs, layout, pyramidLevels, params)
    sr = _super_resolve(ts, descs, (flow_fw, flow_bw), codes, scale, radius, use_sigma, sigma, alphas, prior, iters, layout,
                        out_dtype)
    return SuperResolvedVideo(sr.video, sr.coverage, flow_fw, flow_bw, timing)


STRIDES = (1, 2, 4, 8)  # include/papof.h: papof_match_tensor
MAX_PATCH = 7
MAX_SEARCH = 32
MAX_PENALTY = 65535
MAX_TOL = 2 * MAX_SEARCH
MATCH_STRIDE = 2
MATCH_PATCH = 3
MATCH_SEARCH = 20
MAX_MATCH_LEVELS = 4  # include/papof.h: papof_match_hier_tensor
MAX_REFINE = 3
MAX_TOP_STRIDE = 32
MAX_WINDOW = 32  # include/papof.h: papof_match_recentre_tensor

Matches = collections.namedtuple("Matches", "disp_fw disp_bw cost_fw cost_bw")
MatchInit = collections.namedtuple("MatchInit", "init_fw init_bw reliable")


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    return v


def _check_match(stride, patch, search, penalty):
    if isinstance(stride, bool) or not isinstance(stride, int) or stride not in STRIDES:
        raise ValueError("stride must be one of %s, got %r" % (STRIDES, stride))
    return (stride, _int_in("patch", patch, 1, MAX_PATCH), _int_in("search", search, 1, MAX_SEARCH),
            _int_in("penalty", penalty, 0, MAX_PENALTY))


def _check_hier(stride, levels, refine):
    """(levels, refine, the top level's stride) of the hierarchical search"""
    levels, refine = _int_in("levels", levels, 1, MAX_MATCH_LEVELS), _int_in("refine", refine, 1, MAX_REFINE)
    top = stride << (levels - 1)
    if top > MAX_TOP_STRIDE:
        raise ValueError("stride %d with %d levels gives a top level of stride %d: at most %d" % (stride, levels, top, MAX_TOP_STRIDE))
    return levels, refine, top


def _check_recentre(recentre, levels):
    """the window of the re-centred search, or None"""
    if recentre is None:
        return None
    recentre = _int_in("recentre", recentre, 1, MAX_WINDOW)
    if levels < 2:
        raise ValueError("recentre needs the hierarchical search for its tile origins: levels >= 2, got %d" % levels)
    return recentre


def _check_densify(tol, max_cost):
    """(tol, max_cost as the C ABI's double: -1.0 for None)"""
    tol = _int_in("tol", tol, 0, MAX_TOL)
    if max_cost is None:
        return tol, -1.0
    if isinstance(max_cost, bool) or not isinstance(max_cost, (int, float)) or not max_cost >= 0:
        raise ValueError("max_cost must be None or a number >= 0, got %r" % (max_cost,))
    return tol, float(max_cost)


def _check_match_frames(named, layout, out_dtype, levels, stride, min_frames=1, solver=None):
    """the frames of the matching calls: _check's results for 1 .. MAX_CHANNELS channels and frames of at least one cell"""
    ts, descs, out_dtype, params = _check(named, layout, out_dtype, levels, min_frames=min_frames, solver=solver)
    _, H, W, C = descs[0][0]
    if C > MAX_CHANNELS:
        raise ValueError("%s must have 1 .. %d channels, got %d (layout %s)" % (named[0][0], MAX_CHANNELS, C, layout))
    if H < stride or W < stride:
        raise ValueError("frames of %d x %d are smaller than one cell of stride %d" % (H, W, stride))
    return ts, descs, out_dtype, params


def _match(ts, descs, sequence, n_pairs, stride, patch, search, penalty, both, out_dtype, levels=1, refine=1, recentre=None):
    """papof_match_tensor, with levels > 1 papof_match_hier_tensor, or with a window papof_match_recentre_tensor, on the
    current stream of the frames' device"""
    torch = _torch()
    (_, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    h, w, n = H // stride, W // stride, n_pairs * (2 if both else 1)
    disp = torch.empty((n, 2, h, w), dtype=out_dtype, device=dev)
    cost = torch.empty((n, h, w), dtype=out_dtype, device=dev)
    code = _out_code(out_dtype)
    d_in = [_struct(t, s, c) for t, (_, s, c) in zip(ts, descs)]
    d_disp = _flow_struct(disp, code)
    d_cost = _struct(cost, (cost.stride(0), cost.stride(1), cost.stride(2), 0), code)
    if recentre is not None:
        _launch(dev, "papof_match_recentre_tensor", n_pairs, 1 if sequence else 0, ctypes.byref(d_in[0]),
                None if sequence else ctypes.byref(d_in[1]), H, W, C, stride, levels, patch, search, refine, recentre, penalty,
                1 if both else 0, ctypes.byref(d_disp), ctypes.byref(d_cost),
                workspace=("papof_match_recentre_workspace", (n_pairs, 1 if sequence else 0, H, W, stride, levels),
                           "%d pairs of %d x %d are too large to match" % (n_pairs, H, W)))
    elif levels == 1:
        _launch(dev, "papof_match_tensor", n_pairs, 1 if sequence else 0, ctypes.byref(d_in[0]),
                None if sequence else ctypes.byref(d_in[1]), H, W, C, stride, patch, search, penalty, 1 if both else 0,
                ctypes.byref(d_disp), ctypes.byref(d_cost),
                workspace=("papof_match_workspace", (n_pairs, 1 if sequence else 0, H, W, stride),
                           "%d pairs of %d x %d are too large to match" % (n_pairs, H, W)))
    else:
        _launch(dev, "papof_match_hier_tensor", n_pairs, 1 if sequence else 0, ctypes.byref(d_in[0]),
                None if sequence else ctypes.byref(d_in[1]), H, W, C, stride, levels, patch, search, refine, penalty,
                1 if both else 0, ctypes.byref(d_disp), ctypes.byref(d_cost),
                workspace=("papof_match_hier_workspace", (n_pairs, 1 if sequence else 0, H, W, stride, levels),
                           "%d pairs of %d x %d are too large to match" % (n_pairs, H, W)))
    if both:
        return Matches(disp[:n_pairs], disp[n_pairs:], cost[:n_pairs], cost[n_pairs:])
    return Matches(disp, None, cost, None)


def match_pairs(im1, im2, *, stride=MATCH_STRIDE, patch=MATCH_PATCH, search=MATCH_SEARCH, penalty=0, both=True, layout="NCHW",
                out_dtype=None, levels=1, refine=1, recentre=None):
    """Dense block matching of the independent pairs (im1[i], im2[i]): two tensors of one shape, (B, C, H, W) or
    (B, H, W, C) by `layout`, C = 1 .. 4, uint8, float32 or float64 (quantised to uint8 as rint(255 x)), any strides, on a HIP
    device.  Each frame is box-decimated by `stride` (1, 2, 4 or 8) to h x w = H // stride x W // stride cells; every cell of
    im1 gets the displacement d, |dx|, |dy| <= `search` (1 .. 32) cells, into im2 that minimises the sum of absolute
    differences over the (2 patch + 1)^2 window (patch 1 .. 7) and the channels, plus penalty * (|dx| + |dy|) (0 .. 65535);
    ties go to the shortest d, then the smallest dy, then dx.  include/papof.h (papof_match_tensor) states the rule exactly;
    it is integer arithmetic, so the result is bitwise reproducible.
    Returns Matches(disp_fw, disp_bw (B, 2, h, w): stride * d in full-resolution pixels, cost_fw, cost_bw (B, h, w)) of
    out_dtype (float64, or float32: both hold the integers exactly); the backward fields (im2 -> im1) are None for
    both=False.  The forward and backward fields are views of one tensor.
    This is a START for the solver (match_init, flow_pairs_ld), not a flow: whole cells only, and on repetitive texture
    only match_init's forward-backward test tells a wrong match.  With levels=1 it is one flat search: motion beyond
    stride * search pixels (40 at the defaults) is not found.
    levels = 2 .. 4 searches hierarchically (papof_match_hier_tensor states the rule): the flat search runs on the grid of
    stride * 2^(levels - 1) (at most 32) and every lower level tries, per cell, twice the vectors of its parent cell and
    of three neighbours of the parent, and zero, each +- `refine` (1 .. 3) cells.  The reach is stride * 2^(levels - 1) *
    search pixels plus the refinements -- 160 px at stride 2, levels 3, search 20 -- for about a tenth of the flat search's
    candidates, and the outputs have the same shapes and meaning.  Use it for pans and large structures that move beyond
    40 px.  Do NOT use it for an object smaller than the top level's window ((2 patch + 1) cells of the top stride: 56 px
    at the defaults with levels 3): the top level sees the background around it and the lower levels only refine what it
    found, so a small object that moves far is lost where the flat search finds it -- keep levels=1 there, or give
    recentre.
    recentre = None, or a window of 1 .. 32 cells with levels >= 2 (papof_match_recentre_tensor states the rule): the
    hierarchy's field only says where the flat search looks.  The finest grid is cut into tiles of 32 x 8 cells; a tile's
    origin is the lower median, per component, of the hierarchy's vectors over its cells; every cell of the tile takes the
    best of origin + e, |ex|, |ey| <= recentre, and of the hierarchy's own vector, by the flat search's cost and key.  A
    small object that moves up to stride * recentre pixels against a pan of up to the hierarchy's reach is found.  It is
    NOT a merge of two fields: the origin is one vector per tile, so a tile that a motion boundary halves serves one side;
    an object whose motion relative to its tile's dominant motion exceeds stride * recentre is still lost; and the cost
    returned is the flat search's on the finest grid, not the hierarchy's.
    The workspace comes from PyTorch's allocator; enqueued on the current stream, returns without waiting."""
    stride, patch, search, penalty = _check_match(stride, patch, search, penalty)
    levels, refine, top = _check_hier(stride, levels, refine)
    recentre = _check_recentre(recentre, levels)
    ts, descs, out_dtype, _ = _check_match_frames([("im1", im1), ("im2", im2)], layout, out_dtype, 1, top)
    return _match(ts, descs, False, descs[0][0][0], stride, patch, search, penalty, bool(both), out_dtype, levels, refine, recentre)


def match_video(frames, *, stride=MATCH_STRIDE, patch=MATCH_PATCH, search=MATCH_SEARCH, penalty=0, both=True, layout="NCHW",
                out_dtype=None, levels=1, refine=1, recentre=None):
    """match_pairs on the consecutive pairs (frames[i], frames[i + 1]) of T >= 2 frames, each frame decimated once per
    level: T - 1 pairs.  levels, refine: the hierarchical search of match_pairs, for pans and large structures beyond
    stride * search pixels; an object smaller than the top level's window keeps levels=1, or takes recentre (match_pairs'
    re-centred search: a window of 1 .. 32 cells around each tile's dominant vector, with levels >= 2)."""
    stride, patch, search, penalty = _check_match(stride, patch, search, penalty)
    levels, refine, top = _check_hier(stride, levels, refine)
    recentre = _check_recentre(recentre, levels)
    ts, descs, out_dtype, _ = _check_match_frames([("frames", frames)], layout, out_dtype, 1, top, min_frames=2)
    return _match(ts, descs, True, descs[0][0][0] - 1, stride, patch, search, penalty, bool(both), out_dtype, levels, refine,
                  recentre)


def _check_size(size, h, w):
    """(H, W, stride) of match_init's `size` for fields of h x w cells -- ValueError / TypeError otherwise"""
    try:
        H, W = size
    except (TypeError, ValueError):
        raise TypeError("size must be (H, W), got %r" % (size,)) from None
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in (H, W)):
        raise ValueError("size must be two integers >= 1, got %r" % (size,))
    for s in STRIDES:
        if (H // s, W // s) == (h, w):
            return H, W, s
    raise ValueError("fields of %d x %d cells belong to no stride of %s for frames of %d x %d" % (h, w, STRIDES, H, W))


def _check_cost(name, cost, shape, dev):
    torch = _torch()
    if not isinstance(cost, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(cost).__name__))
    if cost.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s must be float32 or float64, got %s" % (name, cost.dtype))
    if tuple(cost.shape) != shape:
        raise ValueError("%s must be (B, h, w) = %s, got %s" % (name, shape, tuple(cost.shape)))
    if cost.device != dev:
        raise ValueError("%s is on %s, the displacements on %s: all must be on one device" % (name, cost.device, dev))
    return capi.DTYPE_F32 if cost.dtype == torch.float32 else capi.DTYPE_F64


def _check_fields(disp_fw, disp_bw, cost_fw, cost_bw, size, need_cost):
    """every argument error of match_init's tensors: (H, W, stride, the displacements' codes, the costs' codes or None)"""
    codes = tuple(_check_flow(n, f) for n, f in (("disp_fw", disp_fw), ("disp_bw", disp_bw)))
    if disp_fw.shape != disp_bw.shape:
        raise ValueError("disp_fw %s and disp_bw %s differ in shape" % (tuple(disp_fw.shape), tuple(disp_bw.shape)))
    if disp_fw.device != disp_bw.device:
        raise ValueError("disp_fw is on %s, disp_bw on %s: both must be on one device" % (disp_fw.device, disp_bw.device))
    if not _on_gpu(disp_fw):
        raise ValueError("displacements must be on a HIP device (cuda:N), got %s" % disp_fw.device)
    B, _, h, w = (int(x) for x in disp_fw.shape)
    H, W, stride = _check_size(size, h, w)
    c_codes = None
    if need_cost or cost_fw is not None or cost_bw is not None:
        c_codes = tuple(_check_cost(n, c, (B, h, w), disp_fw.device) for n, c in (("cost_fw", cost_fw), ("cost_bw", cost_bw)))
    return H, W, stride, codes, c_codes


def _densify(disps, codes, costs, c_codes, H, W, stride, tol, max_cost):
    """papof_match_densify_tensor of both directions: (flow (2 B, 2, H, W) float64, hole mask (2 B, H, W) uint8), the B
    forward items first"""
    torch = _torch()
    B, dev = int(disps[0].shape[0]), disps[0].device
    flow = torch.empty((2 * B, 2, H, W), dtype=torch.float64, device=dev)
    mask = torch.empty((2 * B, H, W), dtype=torch.uint8, device=dev)
    d = [_flow_struct(f, c) for f, c in zip(disps, codes)]
    for k in (0, 1):
        d_cost = None
        if max_cost >= 0:
            c = costs[k]
            d_cost = _struct(c, (c.stride(0), c.stride(1), c.stride(2), 0), c_codes[k])
        part, part_mask = flow[k * B:(k + 1) * B], mask[k * B:(k + 1) * B]
        d_flow, d_mask = _flow_struct(part, capi.DTYPE_F64), _mask_struct(part_mask)
        _launch(dev, "papof_match_densify_tensor", B, H, W, stride, ctypes.byref(d[k]), ctypes.byref(d[1 - k]), _ref(d_cost), tol,
                max_cost, ctypes.byref(d_flow), ctypes.byref(d_mask))
    return flow, mask


def _match_init(disps, codes, costs, c_codes, H, W, stride, tol, max_cost, relax):
    """both directions densified, then ONE papof_fill_holes_tensor chain over the unreliable pixels of both"""
    torch = _torch()
    B = int(disps[0].shape[0])
    flow, mask = _densify(disps, codes, costs, c_codes, H, W, stride, tol, max_cost)
    init = _fill(flow, descriptor(flow, "NCHW"), mask, relax, "NCHW", torch.float64)
    reliable = (mask == 0).view(2, B, H, W).permute(1, 0, 2, 3)
    return MatchInit(init[:B], init[B:], reliable)


def match_init(disp_fw, disp_bw, cost_fw, cost_bw, size, *, tol=1, max_cost=None, relax=RELAX):
    """The initial flows of flow_pairs_fb from matched displacements: disp_fw, disp_bw (B, 2, h, w) and cost_fw, cost_bw
    (B, h, w) as match_pairs / match_video return them (float32 / float64 on one HIP device; the costs may be None with
    max_cost=None), size = (H, W) of the frames (the stride follows from it).  A cell p is reliable iff its displacement d
    lands on the grid and the opposite field brings it back: |d(p) + d_rev(p + d(p))| <= tol cells in both components
    (tol 0 .. 64) -- and, with max_cost, its cost is at most max_cost.  Every cell is replicated over its stride^2 pixels
    (the trailing rows and columns that the decimation dropped take their nearest cell) and the unreliable pixels are
    filled from the reliable ones by fill_holes (relax).  include/papof.h (papof_match_densify_tensor) states the rule.
    Returns MatchInit(init_fw, init_bw (B, 2, H, W) float64, reliable (B, 2, H, W) torch.bool: channel 0 the forward
    pixels, 1 the backward ones).  Enqueued on the current stream; returns without waiting."""
    tol, max_cost = _check_densify(tol, max_cost)
    relax = _check_relax(relax)
    H, W, stride, codes, c_codes = _check_fields(disp_fw, disp_bw, cost_fw, cost_bw, size, max_cost >= 0)
    return _match_init((disp_fw, disp_bw), codes, (cost_fw, cost_bw), c_codes, H, W, stride, tol, max_cost, relax)


def _run_ld(ts, descs, sequence, n_pairs, layout, out_dtype, levels, alphas, params, match, densify, hier):
    torch = _torch()
    (_, H, W, _), _, _ = descs[0]
    m = _match(ts, descs, sequence, n_pairs, *match, True, torch.float32, *hier)
    code = (capi.DTYPE_F32, capi.DTYPE_F32)
    init = _match_init((m.disp_fw, m.disp_bw), code, (m.cost_fw, m.cost_bw), code, H, W, match[0], *densify)
    return _run_fb(ts, descs, sequence, n_pairs, layout, out_dtype, levels, alphas, params, init.init_fw, init.init_bw)


def flow_pairs_ld(im1, im2, pyramidLevels=2, *, stride=MATCH_STRIDE, patch=MATCH_PATCH, search=MATCH_SEARCH, penalty=0, tol=1,
                  max_cost=None, relax=RELAX, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, match_levels=1, match_refine=1,
                  match_recentre=None, **solver):
    """Large-displacement flow of the independent pairs (im1[i], im2[i]): match_pairs (stride, patch, search, penalty),
    match_init (tol, max_cost, relax) and flow_pairs_fb(im1, im2, pyramidLevels, init_flow=init_fw, init_flow_bw=init_bw,
    ...) -- bit for bit what that call returns given match_init's flows, as FlowFB, so every call built on the flows takes
    the result as it is.  The matcher brings motion of up to stride * search pixels (40 by default) within the solver's
    reach, objects smaller than their displacement included, which no number of pyramid levels does; the solver then needs
    few levels (2 by default: the prior is accurate to a cell).  Frames of C = 1 .. 4 channels.  When NOT to use it: on
    ordinary video (motion of a few pixels) the cold flow_pairs_fb with 5 levels is as good and the matching is wasted
    work; the displacements are whole cells and only a start; and a wrong match on repetitive texture is only caught
    where the forward-backward test fails.  match_levels = 2 .. 4 and match_refine are match_pairs' levels and refine: the
    hierarchical search reaches stride * 2^(match_levels - 1) * search pixels (160 at stride 2, 3 levels, search 20) -- use
    it for pans and large structures that move beyond 40 px.  With match_levels=1 motion beyond stride * search is missed
    as before; with more, an object smaller than the top level's window ((2 patch + 1) cells of the top stride) is lost
    where the flat search finds it: keep match_levels=1 for small objects that move far, or give
    match_recentre (match_pairs' recentre: None, or a window of 1 .. 32 cells with match_levels >= 2) for a small object
    that moves against a pan -- within stride * match_recentre pixels of its tile's dominant motion.  Every argument error
    raises before anything is launched."""
    alphas = _alphas(consistency)
    match = _check_match(stride, patch, search, penalty)
    *hier, top = _check_hier(match[0], match_levels, match_refine)
    hier.append(_check_recentre(match_recentre, hier[0]))
    densify = (*_check_densify(tol, max_cost), _check_relax(relax))
    ts, descs, out_dtype, params = _check_match_frames([("im1", im1), ("im2", im2)], layout, out_dtype, pyramidLevels, top,
                                                       solver=solver)
    return _run_ld(ts, descs, False, descs[0][0][0], layout, out_dtype, pyramidLevels, alphas, params, match, densify, hier)


def flow_video_ld(frames, pyramidLevels=2, *, stride=MATCH_STRIDE, patch=MATCH_PATCH, search=MATCH_SEARCH, penalty=0, tol=1,
                  max_cost=None, relax=RELAX, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, match_levels=1, match_refine=1,
                  match_recentre=None, **solver):
    """flow_pairs_ld on the consecutive pairs (frames[i], frames[i + 1]) of T >= 2 frames: match_video, match_init and
    flow_video_fb(frames, pyramidLevels, init_flow=init_fw, init_flow_bw=init_bw, ...).  match_levels, match_refine as
    there: the hierarchical search for pans and large structures beyond stride * search pixels, not for small objects;
    match_recentre as there: the re-centred search for small objects that move against such a pan."""
    alphas = _alphas(consistency)
    match = _check_match(stride, patch, search, penalty)
    *hier, top = _check_hier(match[0], match_levels, match_refine)
    hier.append(_check_recentre(match_recentre, hier[0]))
    densify = (*_check_densify(tol, max_cost), _check_relax(relax))
    ts, descs, out_dtype, params = _check_match_frames([("frames", frames)], layout, out_dtype, pyramidLevels, top,
                                                       min_frames=2, solver=solver)
    return _run_ld(ts, descs, True, descs[0][0][0] - 1, layout, out_dtype, pyramidLevels, alphas, params, match, densify, hier)


FACTORS = (2, 3, 4)  # include/papof.h: papof_decimate_tensor, papof_upsample_flow_tensor
MAX_UPSAMPLE_RADIUS = 3
UPSAMPLE_BINS = 1024
UP_RADIUS, UP_SIGMA_S, UP_SIGMA_C = 2, 1.0, 0.05  # a 5 x 5 window of cells, 1 cell, 5 % of the guide's range


def _check_factor(factor):
    if isinstance(factor, bool) or not isinstance(factor, int):
        raise TypeError("factor must be an int, got %r" % (factor,))
    if factor not in FACTORS:
        raise ValueError("factor must be one of %s, got %d" % (FACTORS, factor))
    return factor


def _check_upsample(factor, radius, sigma_s, sigma_c):
    """(factor, radius, sigma_s, sigma_c) as int, int, float, float -- TypeError / ValueError otherwise"""
    factor = _check_factor(factor)
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise TypeError("radius must be an int, got %r" % (radius,))
    if not 0 <= radius <= MAX_UPSAMPLE_RADIUS:
        raise ValueError("radius must be in 0 .. %d, got %d" % (MAX_UPSAMPLE_RADIUS, radius))
    _, sigma_s, sigma_c, _ = _check_refine(1, sigma_s, sigma_c, 1)
    return factor, radius, sigma_s, sigma_c


def upsample_tables(factor, radius, sigma_s):
    """The two integer tables of upsample_flow as numpy uint32 arrays, made by the library on the host (include/papof.h:
    papof_upsample_tables): S (factor^2 (2 radius + 1)^2,), indexed by the pixel's phase within its cell (py, px) and the tap
    (dy, dx), 15 / 16 of the bilinear tent plus 1 / 16 of a Gaussian of sigma_s cells, and R (1024,) =
    max(1, rint(65536 exp(-(k + 0.5) / 64))); every entry of both is >= 1."""
    import numpy as np
    factor, radius, sigma_s, _ = _check_upsample(factor, radius, sigma_s, 1.0)
    S, R = np.zeros(factor * factor * (2 * radius + 1) ** 2, np.uint32), np.zeros(UPSAMPLE_BINS, np.uint32)
    U = ctypes.POINTER(ctypes.c_uint)
    capi._chk(capi.load().papof_upsample_tables(factor, radius, sigma_s, S.ctypes.data_as(U), R.ctypes.data_as(U)),
              "papof_upsample_tables")
    return S, R


def upsample_q(sigma_c, channels):
    """The factor q of papof_upsample_flow_tensor, in fp64: 32 / (sigma_c^2 C) (both guides are in the scale 0 .. 1)"""
    return 32.0 / (sigma_c * sigma_c * channels)


def _lr_size(H, W, factor):
    return -(-H // factor), -(-W // factor)


def _check_channels(name, C, layout):
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError("%s must have 1 .. %d channels, got %d (layout %s)" % (name, MAX_CHANNELS, C, layout))


def _decimate(t, desc, factor, layout, out_dtype):
    """papof_decimate_tensor on the current stream of the frames' device: the new tensor in `layout`"""
    (N, H, W, C), strides, code = desc
    h, w = _lr_size(H, W, factor)
    out, d_out = _new_frames(N, h, w, C, layout, out_dtype, t.device)
    d_in = _struct(t, strides, code)
    _launch(t.device, "papof_decimate_tensor", N, H, W, C, factor, ctypes.byref(d_in), ctypes.byref(d_out))
    return out


def decimate(frames, factor, *, layout="NCHW", out_dtype=None):
    """Box decimation of frames by `factor` in {2, 3, 4}: frames (N, C, H, W) or (N, H, W, C) by `layout` (3-D: one frame),
    C in 1 .. 4, uint8, float32 or float64, any strides, on a HIP device.  Returns a new tensor of out_dtype (float64 by
    default, or float32) in the same layout at ceil(H / factor) x ceil(W / factor): each pixel is the mean of the pixels of
    its factor x factor block that exist (edge blocks are clipped, so no row or column is dropped), a uint8 sample read as
    x / 255.0, summed in row-major order in float64 (include/papof.h: papof_decimate_tensor).  Enqueued on the current
    stream; returns without waiting."""
    factor = _check_factor(factor)
    ts, descs, out_dtype, _ = _check([("frames", frames)], layout, out_dtype, 1)
    _check_channels("frames", descs[0][0][3], layout)
    return _decimate(ts[0], descs[0], factor, layout, out_dtype)


def _check_guide_lr(guide_lr, shape, layout, dev):
    """a given low-resolution guide: the 4-D tensor and its descriptor -- TypeError / ValueError otherwise"""
    torch = _torch()
    g = _as4d("guide_lr", guide_lr)
    sizes, strides, code = descriptor(g, layout)
    if g.dtype not in (torch.float32, torch.float64):
        raise TypeError("guide_lr must be float32 or float64 (decimate's output), got %s" % g.dtype)
    if sizes != shape:
        raise ValueError("guide_lr must be %s (items, rows, columns, channels) for this guide and factor, got %s" % (shape, sizes))
    if g.device != dev:
        raise ValueError("guide_lr is on %s, the guide on %s: all must be on one device" % (g.device, dev))
    return g, (sizes, strides, code)


def _upsample(flow_lr, code, guide, desc, guide_lr, desc_lr, d_occ, factor, radius, sigma_s, sigma_c, out_dtype):
    """papof_upsample_flow_tensor on the current stream of the flow's device"""
    torch = _torch()
    (B, H, W, C), strides, g_code = desc
    dev = flow_lr.device
    d_S, d_R = _device_tables(dev, radius, sigma_s, factor)
    out = torch.empty((B, 2, H, W), dtype=out_dtype, device=dev)
    d_flow, d_guide, d_out = _flow_struct(flow_lr, code), _struct(guide, strides, g_code), _flow_struct(out, _out_code(out_dtype))
    d_lr = _struct(guide_lr, *desc_lr[1:])
    _launch(dev, "papof_upsample_flow_tensor", B, H, W, C, factor, ctypes.byref(d_flow), ctypes.byref(d_guide),
            ctypes.byref(d_lr), _ref(d_occ), radius, ctypes.c_void_p(d_S.data_ptr()), ctypes.c_void_p(d_R.data_ptr()),
            upsample_q(sigma_c, C), ctypes.byref(d_out))
    return out


def upsample_flow(flow_lr, guide, factor, *, guide_lr=None, occlusion=None, radius=UP_RADIUS, sigma_s=UP_SIGMA_S,
                  sigma_c=UP_SIGMA_C, layout="NCHW", out_dtype=None):
    """Edge-aware up-sampling of a flow that was estimated on decimated frames: joint bilateral upsampling (Kopf, Cohen,
    Lischinski, Uyttendaele 2007) guided by the full-resolution frame.
    flow_lr: (B, 2, h, w) float32 / float64, any strides, on a HIP device, in low-resolution pixels.  guide: (B, C, H, W) or
    (B, H, W, C) by `layout` (3-D: one item), C in 1 .. 4, uint8 (read as x / 255.0), float32 or float64 (taken to be scaled
    to 0 .. 1), with ceil(H / factor) = h and ceil(W / factor) = w -- usually the frame the flow starts from.  guide_lr:
    None -- decimate(guide, factor) is computed -- or that tensor, float32 / float64 in `layout`; a caller that has it passes
    it.  occlusion: None or a (B, h, w) bool / uint8 mask, nonzero = this cell's flow is not to be trusted.
    Each output pixel is `factor` times the weighted mean of the flows of the cells within `radius` (0 .. 3) of its own
    cell, weighted by an integer spatial table (the bilinear tent plus a Gaussian reach of sigma_s cells) times an integer
    range table of the colour difference between the guide at the pixel and the decimated guide at the cell,
    exp(-d2 / (2 sigma_c^2)) with d2 the mean squared difference over the channels; cells outside the grid, occluded or
    not finite have no weight, every other cell has some, and a pixel whose cells are all dead gets `factor` times its own
    cell's flow as it is.  Products and sums are float64 in a stated order: bitwise reproducible; include/papof.h
    (papof_upsample_flow_tensor) states the rule exactly.  Where the guide is flat the result is close to bilinear
    up-sampling; it invents no motion that the low-resolution grid lost.  Returns the flow (B, 2, H, W) of out_dtype
    (float32 / float64; by default flow_lr's), a new tensor.  Enqueued on the current stream; returns without waiting."""
    torch = _torch()
    factor, radius, sigma_s, sigma_c = _check_upsample(factor, radius, sigma_s, sigma_c)
    ts, descs, _, _ = _check([("guide", guide)], layout, None, 1)
    (B, H, W, C), _, _ = descs[0]
    _check_channels("the guide", C, layout)
    dev = ts[0].device
    h, w = _lr_size(H, W, factor)
    code = _check_flow("flow_lr", flow_lr)
    if tuple(flow_lr.shape) != (B, 2, h, w):
        raise ValueError("flow_lr must be %s for this guide and factor, got %s" % ((B, 2, h, w), tuple(flow_lr.shape)))
    if flow_lr.device != dev:
        raise ValueError("flow_lr is on %s, the guide on %s: all must be on one device" % (flow_lr.device, dev))
    out_dtype = flow_lr.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.float32 or torch.float64, got %s" % out_dtype)
    d_occ, _keep = _check_plane_mask("occlusion", occlusion, (B, h, w), dev)
    if guide_lr is not None:
        g_lr, desc_lr = _check_guide_lr(guide_lr, (B, h, w, C), layout, dev)
    else:
        g_lr = _decimate(ts[0], descs[0], factor, layout, torch.float64)
        desc_lr = descriptor(g_lr, layout)
    return _upsample(flow_lr, code, ts[0], descs[0], g_lr, desc_lr, d_occ, factor, radius, sigma_s, sigma_c, out_dtype)


def _check_lr(factor, refine_levels, radius, sigma_s, sigma_c):
    if isinstance(refine_levels, bool) or not isinstance(refine_levels, int):
        raise TypeError("refine_levels must be an int, got %r" % (refine_levels,))
    if refine_levels < 0:
        raise ValueError("refine_levels must be >= 0, got %d" % refine_levels)
    return (*_check_upsample(factor, radius, sigma_s, sigma_c), refine_levels)


def _run_lr(ts, descs, sequence, n_pairs, layout, out_dtype, levels, alphas, params, lr):
    torch = _torch()
    factor, radius, sigma_s, sigma_c, refine_levels = lr
    _check_channels("the frames", descs[0][0][3], layout)
    lo = [_decimate(t, d, factor, layout, torch.float64) for t, d in zip(ts, descs)]
    lo_descs = [descriptor(t, layout) for t in lo]
    low = _run_fb(lo, lo_descs, sequence, n_pairs, layout, out_dtype, levels, alphas, params)
    # forward flows: guided by the first frames, channel 0 of the mask; backward flows: the second frames, channel 1
    ends = ((ts[0][:-1], lo[0][:-1]), (ts[0][1:], lo[0][1:])) if sequence else ((ts[0], lo[0]), (ts[1], lo[1]))
    flows = []
    for k, (flow, (g, g_lr)) in enumerate(zip((low.flow_fw, low.flow_bw), ends)):
        d_occ, _keep = _check_plane_mask("occlusion", low.occlusion[:, k] if low.occlusion is not None else None,
                                         tuple(flow.shape[i] for i in (0, 2, 3)), flow.device)
        flows.append(_upsample(flow, _out_code(out_dtype), g, descriptor(g, layout), g_lr, descriptor(g_lr, layout), d_occ,
                               factor, radius, sigma_s, sigma_c, out_dtype))
    if refine_levels == 0:
        occ = fb_consistency(flows[0], flows[1], *alphas[1:]) if alphas[0] else None
        return FlowFB(flows[0], flows[1], None, None, occ, low.timing)
    return _run_fb(ts, descs, sequence, n_pairs, layout, out_dtype, refine_levels, alphas, params, flows[0], flows[1])


def flow_pairs_lr(im1, im2, pyramidLevels, *, factor=2, refine_levels=0, radius=UP_RADIUS, sigma_s=UP_SIGMA_S,
                  sigma_c=UP_SIGMA_C, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, **solver):
    """Flow of the independent pairs (im1[i], im2[i]) estimated at reduced resolution: decimate both frames by `factor`
    (2, 3 or 4), flow_pairs_fb(..., pyramidLevels, ...) on the decimated frames, upsample_flow (radius, sigma_s, sigma_c)
    of the forward flows guided by im1 with channel 0 of the low-resolution occlusion mask and of the backward flows guided
    by im2 with channel 1, and then
      refine_levels = 0: fb_consistency(*consistency) on the up-sampled flows -- nothing warps a frame at full resolution,
        so warpI2_fw and warpI2_bw are None (refine_levels=1 gives them) and timing is the low-resolution call's;
      refine_levels >= 1: flow_pairs_fb(im1, im2, refine_levels, init_flow=, init_flow_bw=) from the up-sampled flows at
        full resolution, bit for bit what that call returns.
    Returns a FlowFB, so every call built on the flows takes the result as it is.  The solver runs on 1 / factor^2 of the
    pixels and a pyramid level of the decimated frames is `factor` times coarser than the same level of the frames: use one
    level fewer at factor 2.  When NOT to use it: an object thinner than `factor` pixels is gone before the up-sampler sees
    it, sub-pixel detail inside regions is the low-resolution solver's, and small frames are bound by launches, not by
    pixels, and gain little.  Frames of C = 1 .. 4 channels; `solver` as flow_pairs_fb's.  Every argument error of this
    call's own arguments raises before anything is launched."""
    alphas = _alphas(consistency)
    lr = _check_lr(factor, refine_levels, radius, sigma_s, sigma_c)
    ts, descs, out_dtype, params = _check([("im1", im1), ("im2", im2)], layout, out_dtype, pyramidLevels, solver=solver)
    return _run_lr(ts, descs, False, descs[0][0][0], layout, out_dtype, pyramidLevels, alphas, params, lr)


def flow_video_lr(frames, pyramidLevels, *, factor=2, refine_levels=0, radius=UP_RADIUS, sigma_s=UP_SIGMA_S,
                  sigma_c=UP_SIGMA_C, layout="NCHW", out_dtype=None, consistency=CONSISTENCY, **solver):
    """flow_pairs_lr on the consecutive pairs (frames[i], frames[i + 1]) of T >= 2 frames: every frame is decimated once,
    flow_video_fb runs on the decimated frames, forward flows are up-sampled with frames[:-1] as guide and backward flows
    with frames[1:], as refine_video_flows pairs them."""
    alphas = _alphas(consistency)
    lr = _check_lr(factor, refine_levels, radius, sigma_s, sigma_c)
    ts, descs, out_dtype, params = _check([("frames", frames)], layout, out_dtype, pyramidLevels, min_frames=2, solver=solver)
    return _run_lr(ts, descs, True, descs[0][0][0] - 1, layout, out_dtype, pyramidLevels, alphas, params, lr)


# ---- video mosaics (include/papof.h: papof_mosaic_tensor) -------------------------------------------------------------------
Mosaic = collections.namedtuple("Mosaic", "out count")
Panorama = collections.namedtuple("Panorama", "image count matrices origin motion ok flow timing gains", defaults=(None,))
Overlap = collections.namedtuple("Overlap", "sums counts bound")
StabilizedFull = collections.namedtuple("StabilizedFull", "video valid filled transforms motion ok flow timing")
MOSAIC_MODES = {"first": capi.MOSAIC_FIRST, "mean": capi.MOSAIC_MEAN, "median": capi.MOSAIC_MEDIAN,
                "feather": capi.MOSAIC_FEATHER}
MAX_SOURCES = capi.MOSAIC_MAX_SOURCES  # source slots of one output
MAX_MEDIAN = capi.MOSAIC_MAX_MEDIAN    # of them under mode="median"
MAX_OVERLAP = capi.MOSAIC_MAX_OVERLAP  # of them in mosaic_overlap
OVERLAP_ONE = 2 ** 24                  # mosaic_overlap's fixed point: a luminance of `bound`
MAX_PIXELS = 2 ** 26                   # mosaic_transforms: the largest canvas it returns unasked


def _check_mode(mode):
    if mode not in MOSAIC_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MOSAIC_MODES), mode))
    return MOSAIC_MODES[mode]


def _check_canvas(size):
    try:
        Hc, Wc = size
    except (TypeError, ValueError):
        raise TypeError("size must be (H, W), got %r" % (size,)) from None
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in (Hc, Wc)):
        raise ValueError("size must be two integers >= 1, got %r" % (size,))
    return Hc, Wc


def _check_slots(mode, n, what="matrices have"):
    if not 1 <= n <= MAX_SOURCES:
        raise ValueError("%s %d sources per output, the kernel takes 1 .. %d" % (what, n, MAX_SOURCES))
    if mode == "median" and n > MAX_MEDIAN:
        raise ValueError("%s %d sources per output, mode=\"median\" takes 1 .. %d" % (what, n, MAX_MEDIAN))


def _check_mosaic_matrices(matrices, dev, rows=2):
    """(dtype code, n_out, N) of matrices (n_out, N, rows, 3) float32 / float64 on `dev` -- TypeError / ValueError otherwise"""
    torch = _torch()
    codes = {torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if not isinstance(matrices, torch.Tensor):
        raise TypeError("matrices must be a torch.Tensor, got %s" % type(matrices).__name__)
    if matrices.dtype not in codes:
        raise TypeError("matrices must be float32 or float64, got %s" % matrices.dtype)
    if matrices.dim() != 4 or tuple(matrices.shape[2:]) != (rows, 3) or min(matrices.shape[:2]) < 1:
        raise ValueError("matrices must be (n_out, N, %d, 3), got %s" % (rows, tuple(matrices.shape)))
    if matrices.device != dev:
        raise ValueError("matrices are on %s, the frames on %s: both must be on one device" % (matrices.device, dev))
    return codes[matrices.dtype], int(matrices.shape[0]), int(matrices.shape[1])


def _check_sources(sources, n_out, N, T):
    """the sources as a contiguous int32 host tensor (n_out, N), or None for None: "source k is frame k" (N = T); an integer
    tensor (any device: read on the host) or array otherwise, every entry < T -- TypeError / ValueError otherwise"""
    import numpy as np
    torch = _torch()
    if sources is None:
        if N != T:
            raise ValueError("sources=None is frame k for source k: matrices have %d sources for %d frames" % (N, T))
        return None
    if isinstance(sources, torch.Tensor):
        if sources.dtype.is_floating_point or sources.dtype.is_complex or sources.dtype == torch.bool:
            raise TypeError("sources must hold integers, got %s" % sources.dtype)
        s = sources.detach().to("cpu", torch.int64)
    else:
        try:
            a = np.asarray(sources)
        except Exception:  # noqa: BLE001
            raise TypeError("sources must be None, an integer tensor or an integer array, got %r" % (sources,)) from None
        if a.dtype.kind not in "iu":
            raise TypeError("sources must hold integers, got %s" % a.dtype)
        s = torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
    if tuple(s.shape) != (n_out, N):
        raise ValueError("sources must be (n_out, N) = %s as the matrices, got %s" % ((n_out, N), tuple(s.shape)))
    if int(s.max()) >= T:
        raise ValueError("sources name frame %d of %d frames" % (int(s.max()), T))
    return s.clamp(min=-1).to(torch.int32).contiguous()


def _check_gains(gains, n_out, N, dev):
    """None, or the (n_out, N) float32 / float64 gains on `dev` -- TypeError / ValueError otherwise"""
    torch = _torch()
    if gains is None:
        return None
    if not isinstance(gains, torch.Tensor):
        raise TypeError("gains must be None or a torch.Tensor, got %s" % type(gains).__name__)
    if gains.dtype not in (torch.float32, torch.float64):
        raise TypeError("gains must be float32 or float64, got %s" % gains.dtype)
    if tuple(gains.shape) != (n_out, N):
        raise ValueError("gains must be (n_out, N) = %s as the matrices, got %s" % ((n_out, N), tuple(gains.shape)))
    if gains.device != dev:
        raise ValueError("gains are on %s, the frames on %s: both must be on one device" % (gains.device, dev))
    return gains


# how a source reaches the canvas: the rows of its matrices (2: affine, 3: projective), the entry points of the mosaic and of
# the overlap statistics, and whether the canvas is a pair of tables (cols, rows) of directions instead of a size
_Rule = collections.namedtuple("_Rule", "rows blend overlap tables")
_AFFINE = _Rule(2, "papof_mosaic_blend_tensor", "papof_mosaic_overlap_tensor", False)
_PROJECTIVE = _Rule(3, "papof_mosaic_projective_tensor", "papof_mosaic_overlap_projective_tensor", False)
_RAYS = _Rule(3, "papof_mosaic_ray_tensor", "papof_mosaic_overlap_ray_tensor", True)
_MESH = _Rule(2, "papof_mosaic_mesh_tensor", None, True)  # the tables: (mesh (n_out, N, GH + 1, GW + 1, 2), GH, GW)


def _table_args(tables):
    """what follows the matrices in the entry points of a rule with tables: the ray rule's (cols, rows), or the mesh rule's
    (mesh (n_out * N, GH + 1, GW + 1, 2), GH, GW)"""
    if tables and tables[0].dim() == 4:
        mesh, gh, gw = tables
        return ctypes.byref(_vertex_struct(mesh)), gh, gw
    return tuple(ctypes.byref(_table_struct(t)) for t in tables)


def _mosaic_head(ts, descs, src, matrices, m_code, masks, Hc, Wc, tables):
    """the arguments that every entry point of the mosaics begins with, the rule's tables behind the matrices (a byref
    keeps its descriptor alive)"""
    (T, H, W, C), strides, code = descs[0]
    d_mask = _mask_struct(masks) if masks is not None else None
    return (T, H, W, C, ctypes.byref(_struct(ts[0], strides, code)), _ref(d_mask), int(src.shape[0]), int(src.shape[1]), Hc, Wc,
            ctypes.c_void_p(src.data_ptr()), ctypes.byref(_struct(matrices, tuple(matrices.stride()), m_code)),
            *_table_args(tables))


def _mosaic(ts, descs, src, matrices, m_code, masks, Hc, Wc, mode, layout, out_dtype, count=True, gains=None, rule=_AFFINE,
            tables=()):
    """papof_mosaic_tensor on checked arguments: src the int32 (n_out, N) sources on the frames' device, masks uint8 or None;
    count False: no count (None is returned for it; mode "first" then stops at the first live source).  With gains (checked)
    or mode "feather": papof_mosaic_blend_tensor.  rule _PROJECTIVE: matrices (n_out, N, 3, 3), papof_mosaic_projective_tensor.
    rule _RAYS: tables the checked (cols, rows), matrices (n_out, N, 3, 3): papof_mosaic_ray_tensor.  rule _MESH: tables the
    checked (mesh, GH, GW): papof_mosaic_mesh_tensor, with its workspace."""
    torch = _torch()
    dev = ts[0].device
    n_out = int(src.shape[0])
    out, d_out = _new_frames(n_out, Hc, Wc, descs[0][0][3], layout, out_dtype, dev)
    cnt = torch.empty((n_out, Hc, Wc), dtype=torch.uint8, device=dev) if count else None
    d_cnt = _mask_struct(cnt) if count else None
    if rule is _MESH:  # (n_out, N, ...) as (n_out * N, ...): a view where the strides allow, else a copy, held until the launch
        tables = (tables[0].reshape((-1,) + tuple(tables[0].shape[2:])),) + tuple(tables[1:])
    head = _mosaic_head(ts, descs, src, matrices, m_code, masks, Hc, Wc, tables)
    tail = (MOSAIC_MODES[mode], ctypes.byref(d_out), _ref(d_cnt))
    if rule is _AFFINE and gains is None and mode != "feather":
        _launch(dev, "papof_mosaic_tensor", *head, *tail)
        return out, cnt
    d_gain = None
    if gains is not None:
        d_gain = _struct(gains, (gains.stride(0), gains.stride(1), 0, 0),
                         capi.DTYPE_F32 if gains.dtype == torch.float32 else capi.DTYPE_F64)
    ws = None
    if rule is _MESH:
        ws = ("papof_mosaic_mesh_workspace", (n_out, int(src.shape[1])), "%d sources per output are too many" % int(src.shape[1]))
    _launch(dev, rule.blend, *head, _ref(d_gain), *tail, workspace=ws)
    return out, cnt


def _mosaic_inputs(rule, ts, descs, sources, matrices, canvas, masks):
    """what the mosaics and their overlaps check alike behind their frames, in mosaic's order: (Hc, Wc, m_code, n_out, N, the
    host sources or None, masks, the tables); canvas: the size, or with _RAYS (cols, rows), whose lengths are the size, or
    with _MESH (the size, the mesh)"""
    (T, H, W, _), _, _ = descs[0]
    dev = ts[0].device
    if rule is _MESH:
        Hc, Wc = _check_canvas(canvas[0])
    elif rule.tables:
        Wc, Hc = _check_table("cols", canvas[0], dev), _check_table("rows", canvas[1], dev)
    else:
        Hc, Wc = _check_canvas(canvas)
    m_code, n_out, N = _check_mosaic_matrices(matrices, dev, rule.rows)
    src = _check_sources(sources, n_out, N, T)
    m = _check_masks("masks", masks, T, H, W, dev) if masks is not None else None
    if rule is _MESH:
        return Hc, Wc, m_code, n_out, N, src, m, (canvas[1],) + _check_slot_mesh(canvas[1], n_out, N, dev, H, W)
    return Hc, Wc, m_code, n_out, N, src, m, tuple(canvas) if rule.tables else ()


def _mosaic_call(rule, frames, sources, matrices, canvas, mode, masks, layout, out_dtype, gains):
    """mosaic, mosaic_homography and mosaic_rays behind their docstrings"""
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    _check_mode(mode)
    Hc, Wc, m_code, n_out, N, src, m, tables = _mosaic_inputs(rule, ts, descs, sources, matrices, canvas, masks)
    _check_slots(mode, N)
    dev = ts[0].device
    gains = _check_gains(gains, n_out, N, dev)
    src = _device_sources(src, descs[0][0][0], n_out, dev)
    return Mosaic(*_mosaic(ts, descs, src, matrices, m_code, m, Hc, Wc, mode, layout, out_dtype, gains=gains, rule=rule,
                           tables=tables))


def _mosaic_overlap_call(rule, frames, sources, matrices, canvas, masks, step, bound, layout):
    """mosaic_overlap, mosaic_overlap_homography and mosaic_overlap_rays behind their docstrings"""
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    Hc, Wc, m_code, n_out, N, src, m, tables = _mosaic_inputs(rule, ts, descs, sources, matrices, canvas, masks)
    _check_overlap_slots(N)
    _int_at_least("step", step, 1)
    bound = _positive("bound", bound)
    src = _device_sources(src, descs[0][0][0], n_out, ts[0].device)
    return _mosaic_overlap(ts, descs, src, matrices, m_code, m, Hc, Wc, step, bound, rule, tables)


def _device_sources(src, T, n_out, dev):
    if src is None:  # made on the device, on the current stream
        return _torch().arange(T, dtype=_torch().int32, device=dev).repeat(n_out, 1)
    if dev.type == "cuda":  # from page-locked memory: the copy is queued, the host does not wait for the stream
        return src.pin_memory().to(dev, non_blocking=True)
    return src


def mosaic(frames, sources, matrices, size, *, mode="median", masks=None, layout="NCHW", out_dtype=None, gains=None):
    """Many frames, each through its own affine matrix, gathered into one output pixel and combined there: frames (T, C, H,
    W) or (T, H, W, C) by `layout`, uint8 (read as x / 255), float32 or float64, any strides, on a HIP device; size = (Hc,
    Wc) of the n_out outputs; matrices (n_out, N, 2, 3) float32 / float64 on the same device, N <= 255 sources per output
    (64 for the median); sources (n_out, N) integers, any device or a numpy array -- the frame of each source, negative: an
    empty slot -- or None: source k is frame k; masks None or (T, H, W) bool / uint8: nonzero pixels of a frame are left
    out.  At output pixel (x, y) source k is LIVE where matrices[o, k] (x, y, 1) lies inside its frame and, with masks, no
    bilinear tap of positive weight there is masked; its sample is the frame read bilinearly (the rule of warp_affine).
    mode "first": the live source with the smallest k; "mean": the live samples added in k order over their number;
    "median": per channel the lower median of the live samples, ties broken by k, NaN last -- the bits of one sample;
    "feather": the live samples weighted by w = 1 + the distance of the sampled point to its frame's nearest border, added
    in k order over the sum of the weights: no step where a frame ends.  gains None or (n_out, N) float32 / float64 on the
    frames' device (a stride of 0 broadcasts): every sample of source k is multiplied by gains[o, k] before the mode sees
    it (exposure_gains makes them); they are not inspected.  With gains None the first three modes are
    papof_mosaic_tensor as before; otherwise papof_mosaic_blend_tensor.  Returns Mosaic(out (n_out, C, Hc, Wc) or (n_out,
    Hc, Wc, C) of out_dtype (by default the frames'), 0 where no source is live; count (n_out, Hc, Wc) uint8: the live
    sources).  include/papof.h (papof_mosaic_tensor, papof_mosaic_blend_tensor) states it exactly;
    bitwise reproducible.  The sources are checked on the host (a device tensor of sources waits for its stream); the kernel
    is enqueued on the current stream and the call returns without waiting."""
    return _mosaic_call(_AFFINE, frames, sources, matrices, size, mode, masks, layout, out_dtype, gains)


def _check_overlap_slots(n, what="matrices have"):
    if not 1 <= n <= MAX_OVERLAP:
        raise ValueError("%s %d sources per output, the overlap statistics take 1 .. %d" % (what, n, MAX_OVERLAP))


def _mosaic_overlap(ts, descs, src, matrices, m_code, masks, Hc, Wc, step, bound, rule=_AFFINE, tables=()):
    """the overlap entry point of `rule` (papof_mosaic_overlap_tensor, _projective_tensor, _ray_tensor) on checked arguments,
    as _mosaic's"""
    torch = _torch()
    dev = ts[0].device
    n_out, N = int(src.shape[0]), int(src.shape[1])
    sums = torch.empty((n_out, N, N), dtype=torch.int64, device=dev)
    counts = torch.empty((n_out, N, N), dtype=torch.int64, device=dev)
    _launch(dev, rule.overlap, *_mosaic_head(ts, descs, src, matrices, m_code, masks, Hc, Wc, tables), step,
            ctypes.c_double(bound), ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(counts.data_ptr()))
    return Overlap(sums, counts, bound)


def mosaic_overlap(frames, sources, matrices, size, *, masks=None, step=2, bound=1.0, layout="NCHW"):
    """The pairwise overlap statistics of a mosaic, from which exposure_gains solves one gain per source (Brown and Lowe
    2007, section 6): frames, sources, matrices, size, masks and layout as mosaic's, N <= 64 sources per output.  At every
    `step`-th column and row of the canvas the luminance of each live source -- the mean of its channels' samples, divided
    by `bound` (finite, > 0: the value that counts as white), clamped to [0, 1], in 24-bit fixed point; a NaN luminance is
    left out -- is added into sums[o, i, j] for every source j live at that pixel, i itself included, and counts[o, i, j]
    counts the pixel: sums[o, i, j] / counts[o, i, j] / 2**24 * bound is the mean luminance of source i where it overlaps
    source j.  Returns Overlap(sums, counts (n_out, N, N) int64 on the frames' device, bound).  Integer sums: bitwise
    reproducible.  include/papof.h (papof_mosaic_overlap_tensor) states it exactly.  Enqueued on the current stream; the
    call returns without waiting."""
    return _mosaic_overlap_call(_AFFINE, frames, sources, matrices, size, masks, step, bound, layout)


def _positive(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s must be a number, got %r" % (name, v))
    if not (math.isfinite(v) and v > 0):
        raise ValueError("%s must be finite and > 0, got %r" % (name, v))
    return float(v)


def exposure_gains(overlap, *, sigma_n=10.0 / 255.0, sigma_g=0.1, anchor=None):
    """One gain per source from mosaic_overlap's statistics (Brown and Lowe 2007, section 6): per output, with N_ij =
    counts[i, j] for i != j and I_ij = sums[i, j] / counts[i, j] / 2**24 * bound (0 where the count is 0), the gains that
    minimise  sum over i != j of N_ij ((g_i I_ij - g_j I_ji)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2)  -- the sources agree
    where they overlap, and the prior keeps the gains near 1 (the error alone is minimal at g = 0).  The linear system is
    solved on the host in float64 (the call waits for the statistics); a source that overlaps no other gets 1.  anchor: None,
    or a source index k: every output's gains are divided by its g_k, so that source keeps its look.  Gains fix ratios, not
    the level.  Returns (n_out, N) float64 on the statistics' device: mosaic's `gains`."""
    import numpy as np
    torch = _torch()
    if not isinstance(overlap, Overlap):
        raise TypeError("overlap must be an Overlap (mosaic_overlap's), got %s" % type(overlap).__name__)
    sums, counts = overlap.sums, overlap.counts
    for name, t in (("sums", sums), ("counts", counts)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError("overlap.%s must be an int64 tensor" % name)
        if t.dim() != 3 or t.shape[1] != t.shape[2] or min(t.shape) < 1 or t.shape != sums.shape:
            raise ValueError("overlap.sums and .counts must be (n_out, N, N), got %s and %s" % (tuple(sums.shape),
                                                                                              tuple(counts.shape)))
    bound = _positive("overlap.bound", overlap.bound)
    sigma_n, sigma_g = _positive("sigma_n", sigma_n), _positive("sigma_g", sigma_g)
    n_out, N = int(sums.shape[0]), int(sums.shape[1])
    if anchor is not None and (isinstance(anchor, bool) or not isinstance(anchor, int) or not 0 <= anchor < N):
        raise ValueError("anchor must be None or a source index in 0 .. %d, got %r" % (N - 1, anchor))
    S = sums.detach().cpu().numpy().astype(np.float64)
    Nij = counts.detach().cpu().numpy().astype(np.float64)
    I = np.where(Nij > 0, S / np.maximum(Nij, 1.0) / OVERLAP_ONE * bound, 0.0)
    Nij = Nij * (1.0 - np.eye(N))
    n = Nij.sum(2)
    g = np.ones((n_out, N))
    for o in range(n_out):
        A = -2.0 * Nij[o] * I[o] * I[o].T / sigma_n ** 2
        A[np.diag_indices(N)] = (2.0 * Nij[o] * I[o] ** 2).sum(1) / sigma_n ** 2 + n[o] / sigma_g ** 2
        b = n[o] / sigma_g ** 2
        alone = n[o] == 0
        A[alone, alone] = 1.0
        b = np.where(alone, 1.0, b)
        g[o] = np.linalg.solve(A, b)
        if anchor is not None:
            g[o] = g[o] / g[o, anchor]
    return torch.from_numpy(g).to(sums.device)


def _pair_motions(motion):
    """the (T - 1, 2 or 3, 3) float64 numpy array (pairs of a Motion or Homography with ok False: the identity) and the device
    of a motion that _checked_motion has accepted"""
    import numpy as np
    ok = None
    if isinstance(motion, (Motion, Homography)):
        motion, ok = motion.motion, motion.ok
    A = motion.detach().to("cpu", _torch().float64).numpy()
    if ok is not None:
        A = np.where(ok.detach().cpu().numpy().reshape(-1, 1, 1), A, np.eye(A.shape[1], 3))
    return A, motion.device


def _int_at_least(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
    return v


def _check_ref(ref, T):
    if ref is None:
        return (T - 1) // 2
    if isinstance(ref, bool) or not isinstance(ref, int) or not 0 <= ref < T:
        raise ValueError("ref must be None or a frame index in 0 .. %d, got %r" % (T - 1, ref))
    return ref


def _as_it_is(m):
    return m


def _over_last(m):
    if not m[2, 2] > 0:  # (a NaN included) the sign of every denominator would flip
        raise ValueError("a motion along the chain has a [2][2] that is not > 0: it sends the image centre's "
                         "neighbourhood behind its horizon")
    return m / m[2, 2]


def _over_det(m):
    import numpy as np
    d = np.linalg.det(m)
    if not (np.isfinite(d) and d > 0):
        raise ValueError("a motion along the chain has a determinant that is not finite and > 0: it mirrors the image or is "
                         "singular")
    return m / np.cbrt(d)


def _chain(A, ref, unit, nothing):
    """(frame t to the reference frame, the reference frame to frame t) for the 3 x 3 pair motions A (T - 1, 3, 3), as the
    chain of the pair motions between t and ref, every factor and every product through the normaliser `unit` (_as_it_is,
    _over_last, _over_det) -- so that the reference frame and frames that do not move against it (pairs with ok False) map to
    their own integer corners exactly: no floor or ceiling of 1e-16.  ValueError, naming what there is `nothing` of, where a
    motion cannot be inverted"""
    import numpy as np
    T = A.shape[0] + 1
    to_ref = [np.eye(3)] * T
    with np.errstate(all="ignore"):
        try:
            for t in range(ref - 1, -1, -1):
                to_ref[t] = unit(to_ref[t + 1] @ unit(A[t]))
            for t in range(ref + 1, T):
                to_ref[t] = unit(to_ref[t - 1] @ unit(np.linalg.inv(unit(A[t - 1]))))
            return to_ref, [np.linalg.inv(m) for m in to_ref]
        except np.linalg.LinAlgError:
            raise ValueError("the camera path is singular: %s" % nothing) from None


def _corners(H, W):
    import numpy as np
    return np.array([[0.0, W - 1.0, 0.0, W - 1.0], [0.0, 0.0, H - 1.0, H - 1.0], [1.0, 1.0, 1.0, 1.0]])


def _planar_canvas(pts, margin, max_pixels):
    """the canvas around the finite points pts (T, 2, n) of the reference frame's plane: ((x0, y0), (Hc, Wc), the translation
    from canvas to plane) -- ValueError beyond max_pixels"""
    import numpy as np
    x0, y0 = math.floor(pts[:, 0].min()) - margin, math.floor(pts[:, 1].min()) - margin
    Wc, Hc = math.ceil(pts[:, 0].max()) + margin - x0 + 1, math.ceil(pts[:, 1].max()) + margin - y0 + 1
    if Hc * Wc > max_pixels:
        raise ValueError("the canvas is %d x %d, more than max_pixels = %d" % (Hc, Wc, max_pixels))
    return (x0, y0), (Hc, Wc), np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])


def mosaic_transforms(motion, size, *, ref=None, margin=0, max_pixels=MAX_PIXELS):
    """The canvas of a video's panorama and the matrices that fill it: motion a (T - 1, 2, 3) tensor (global_motion's, any
    device) or a Motion (pairs with ok False enter as the identity), size = (H, W) of the frames.  In float64 on the host,
    with P_t the camera path of stabilizing_transforms and `ref` (default (T - 1) // 2) the frame whose coordinates the
    canvas keeps: the corners of every frame are mapped into the reference frame by P_ref P_t^-1; (x0, y0) is the floor of
    their minima less `margin`, and the canvas reaches the ceiling of their maxima plus `margin`; canvas pixel q samples
    frame t at matrix_t q, matrix_t = P_t P_ref^-1 translate(x0, y0).  Returns (matrices (1, T, 2, 3) float64 on the
    motion's device -- mosaic's, for sources=None --, (Hc, Wc), (x0, y0)).  ValueError when the bounds are not finite or
    Hc * Wc > max_pixels: a chain that drifted, or a shot that is no pan."""
    import numpy as np
    torch = _torch()
    A, dev = _pair_motions(_checked_motion(motion))
    H, W = _check_canvas(size)
    T = A.shape[0] + 1
    ref = _check_ref(ref, T)
    _int_at_least("margin", margin, 0)
    _int_at_least("max_pixels", max_pixels, 1)
    last = np.tile([[[0.0, 0.0, 1.0]]], (T - 1, 1, 1))  # P_ref P_t^-1 as the chain of the pair motions, each with its last row
    to_ref, from_ref = _chain(np.concatenate([A, last], axis=1), ref, _as_it_is, "no canvas")
    corners = _corners(H, W)
    with np.errstate(all="ignore"):
        pts = np.stack([(m @ corners)[:2] for m in to_ref])  # (T, 2, 4)
    if not (np.isfinite(pts).all() and np.isfinite(np.array(from_ref)).all()):
        raise ValueError("the bounds of the canvas are not finite")
    origin, size, shift = _planar_canvas(pts, margin, max_pixels)
    M = np.stack([(m @ shift)[:2] for m in from_ref])[None]
    return torch.from_numpy(M).to(dev), size, origin


def neighbour_transforms(transforms, motion, radius):
    """The sources and matrices that fill each stabilized frame from the frames around it: transforms (T, 2, 3) the
    sampling matrices M_t of stabilizing_transforms, motion the pair motions they came from (a tensor or a Motion), radius
    >= 0 frames to either side (2 radius + 1 <= 255).  In float64 on the host: slot 0 is frame t itself through M_t; slot
    2 d - 1 is frame t - d and slot 2 d frame t + d, each through P_s P_t^-1 M_t -- the stabilized pixel to frame t, then
    along the camera path to frame s; the source is -1 where s is outside the video.  Returns (sources (T, 2 radius + 1)
    int32, matrices (T, 2 radius + 1, 2, 3) float64), both on the transforms' device: mosaic's, mode "first" prefers the
    frame itself, then the nearest in time."""
    import numpy as np
    torch = _torch()
    if not isinstance(transforms, torch.Tensor):
        raise TypeError("transforms must be a torch.Tensor, got %s" % type(transforms).__name__)
    A, _ = _pair_motions(_checked_motion(motion))
    T = A.shape[0] + 1
    if tuple(transforms.shape) != (T, 2, 3):
        raise ValueError("transforms must be (T, 2, 3) = %s as the motion, got %s" % ((T, 2, 3), tuple(transforms.shape)))
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= 2 * radius + 1 <= MAX_SOURCES:
        raise ValueError("radius must be an integer in 0 .. %d, got %r" % ((MAX_SOURCES - 1) // 2, radius))
    Mt = transforms.detach().to("cpu", torch.float64).numpy()
    P = camera_path(A)
    N = 2 * radius + 1
    src = np.full((T, N), -1, np.int32)
    mats = np.tile(np.eye(2, 3), (T, N, 1, 1))
    for t in range(T):
        M3 = np.vstack([Mt[t], [0.0, 0.0, 1.0]])
        try:
            back = np.linalg.inv(P[t]) @ M3
        except np.linalg.LinAlgError:
            raise ValueError("the camera path is singular at frame %d: no way back from it" % t) from None
        src[t, 0], mats[t, 0] = t, Mt[t]
        for d in range(1, radius + 1):
            for slot, s in ((2 * d - 1, t - d), (2 * d, t + d)):
                if 0 <= s < T:
                    src[t, slot], mats[t, slot] = s, (P[s] @ back)[:2]
    return torch.from_numpy(src).to(transforms.device), torch.from_numpy(mats).to(transforms.device)


def _check_bool(name, v):
    if not isinstance(v, bool):
        raise TypeError("%s must be True or False, got %r" % (name, v))


_PanoramaArgs = collections.namedtuple("_PanoramaArgs", "ts descs params out_dtype ref masks picked step mode layout exposure")


def _panorama_head(frames, pyramidLevels, solver, mode, ref, step, margin, masks, layout, out_dtype, exposure):
    """the argument checks that the four panoramas share, and what they need of them: the frames and their descriptors, the
    solver's params, the output dtype, the reference frame, the masks as uint8 and the frames `picked` for the mosaic"""
    ts, descs, _, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    (T, H, W, _), _, _ = descs[0]
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    _check_mode(mode)
    ref = _check_ref(ref, T)
    _int_at_least("step", step, 1)
    _int_at_least("margin", margin, 0)
    m = _check_masks("masks", masks, T, H, W, ts[0].device) if masks is not None else None
    picked = list(range(0, T, step))
    _check_bool("exposure", exposure)
    if exposure and len(picked) > MAX_OVERLAP:
        raise ValueError("step = %d deposits %d sources per output, exposure=True takes 1 .. %d: the video needs a larger step"
                         % (step, len(picked), MAX_OVERLAP))
    _check_slots(mode, len(picked), "step = %d deposits" % step)
    return _PanoramaArgs(ts, descs, params, out_dtype, ref, m, picked, step, mode, layout, exposure)


def _panorama_tail(p, rule, M, size, tables=()):
    """the picked frames through M (1, T, ., 3) onto the canvas: with exposure the overlap statistics and their gains,
    anchored at the reference frame when it is among the picked, then ONE mosaic -- (image, count, gains or None)"""
    src = _torch().tensor([p.picked], dtype=_torch().int32, device=p.ts[0].device)
    gains = None
    if p.exposure:
        ov = _mosaic_overlap(p.ts, p.descs, src, M[:, ::p.step], capi.DTYPE_F64, p.masks, *size, 2, 1.0, rule, tables)
        gains = exposure_gains(ov, anchor=p.picked.index(p.ref) if p.ref in p.picked else None)
    image, count = _mosaic(p.ts, p.descs, src, M[:, ::p.step], capi.DTYPE_F64, p.masks, *size, p.mode, p.layout, p.out_dtype,
                           gains=gains, rule=rule, tables=tables)
    return image[0], count[0], None if gains is None else gains[0]


def panorama(frames, pyramidLevels, *, mode="median", ref=None, step=1, margin=0, masks=None, model="affine", iters=5,
             scale=1.0, layout="NCHW", out_dtype=None, exposure=False, **solver):
    """The panorama of a panning video of T >= 2 frames -- with mode "median" its clean plate: what moved in front of the
    background is gone wherever the background shows in more than half of the frames that cover a pixel.
    flow_video(frames, pyramidLevels, layout=layout, **solver), global_motion on the flows (model, iters, scale),
    mosaic_transforms (ref, margin; the only wait) and ONE mosaic of the frames 0, step, 2 step, ... (masks: (T, H, W),
    nonzero pixels are left out).  The motion is chained over all pairs whatever the step.  At most 255 frames are
    deposited, 64 under "median" or with exposure=True: a larger video needs a larger `step`.  mode "feather" blends the
    frames by their distance to the border (mosaic).  exposure=True compensates the frames' exposure first: mosaic_overlap
    (step 2, bound 1.0: white is 1, as in uint8 frames and floats in [0, 1] -- float frames of another range clamp there and
    their gains degrade: compose the three calls with a bound of your own) and exposure_gains on the deposited frames,
    anchored at the reference frame when it is among them -- a second wait --, and the mosaic takes the gains.  Returns Panorama(image (C, Hc, Wc) or (Hc, Wc, C)
    of out_dtype (by default the frames'), count (Hc, Wc) uint8, matrices (T, 2, 3) float64 -- canvas to frame t, of every
    frame --, origin (x0, y0): the canvas pixel (0, 0) in the reference frame's coordinates, motion (T - 1, 2, 3), ok
    (T - 1,) bool, flow (T - 1, 2, H, W) float64, timing of the flow call, gains: None, or with exposure=True the float64
    gain of every deposited frame).  The model is affine (panorama_homography is the projective chain, for a camera that
    rotates) and there is no bundle adjustment; the exposure is one gain per frame, and feathering ghosts where the
    registration is off (README).  Every argument error raises before anything is launched."""
    p = _panorama_head(frames, pyramidLevels, solver, mode, ref, step, margin, masks, layout, out_dtype, exposure)
    code, iters, scale = _check_fit(model, iters, scale)
    (T, H, W, _), _, _ = p.descs[0]
    flow, _, timing = _run(p.ts, p.descs, True, T - 1, layout, _torch().float64, pyramidLevels, p.params)
    mo = _motion_fit(flow, capi.DTYPE_F64, None, code, iters, scale)
    M, size, origin = mosaic_transforms(mo, (H, W), ref=p.ref, margin=margin)
    image, count, gains = _panorama_tail(p, _AFFINE, M, size)
    return Panorama(image, count, M[0], origin, mo.motion, mo.ok, flow, timing, gains)


def stabilize_video_full(frames, pyramidLevels, *, fill_radius=15, layout="NCHW", model="similarity", radius=15, crop=1.0,
                         iters=5, scale=1.0, out_dtype=None, **solver):
    """stabilize_video whose frames have no empty border: where stabilized frame t does not cover a pixel, the frames
    t - 1, t + 1, t - 2, ... t +- fill_radius that saw it supply it, registered by the same global motions -- the final
    warp_affine replaced by ONE mosaic(..., mode="first") over neighbour_transforms.  Returns StabilizedFull(video, valid
    (T, H, W) bool as stabilize_video gives it -- where it holds, the video is stabilize_video's byte for byte --, filled
    (T, H, W) bool: not valid, and supplied by a neighbour; transforms, motion, ok, flow, timing as stabilize_video).
    Pixels that are neither stay 0.  Registration is by the global motion alone: where the scene has parallax a filled
    border mis-registers; there is no local motion inpainting (README).  Every argument error raises before anything is
    launched; the video is enqueued on the current stream."""
    ts, descs, _, params = _check([("frames", frames)], layout, None, pyramidLevels, min_frames=2, solver=solver)
    code, iters, scale = _check_fit(model, iters, scale)
    (T, H, W, C), _, _ = descs[0]
    _check_path(radius, crop, (H, W))
    _check_fill_radius(fill_radius)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    torch = _torch()
    flow, _, timing = _run(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, params)
    m = _motion_fit(flow, capi.DTYPE_F64, None, code, iters, scale)
    M = stabilizing_transforms(m, radius, crop, size=(H, W))
    src, mats = neighbour_transforms(M, m, fill_radius)
    video, count = _mosaic(ts, descs, src, mats, capi.DTYPE_F64, None, H, W, "first", layout, out_dtype)
    # valid: slot 0 alone, on one channel (a view), through the same kernel -- its count is the frame's own coverage
    one = ts[0][:, :1] if layout == "NCHW" else ts[0][..., :1]
    _, own = _mosaic([one], [descriptor(one, layout)], src[:, :1].contiguous(), mats[:, :1], capi.DTYPE_F64, None, H, W,
                     "first", layout, torch.uint8)
    valid = own > 0
    return StabilizedFull(video, valid, (count > 0) & ~valid, M, m.motion, m.ok, flow, timing)


# ---- full-frame mesh stabilization: the mosaic with a displacement table per slot (include/papof.h: papof_mosaic_mesh_tensor)
def _check_fill_radius(fill_radius):
    if isinstance(fill_radius, bool) or not isinstance(fill_radius, int) or not 0 <= 2 * fill_radius + 1 <= MAX_SOURCES:
        raise ValueError("fill_radius must be an integer in 0 .. %d, got %r" % ((MAX_SOURCES - 1) // 2, fill_radius))


def _check_slot_mesh(mesh, n_out, N, dev, H, W):
    """a (n_out, N, GH + 1, GW + 1, 2) float64 table on `dev` whose grid fits H x W frames: (GH, GW)"""
    torch = _torch()
    if not isinstance(mesh, torch.Tensor):
        raise TypeError("mesh must be a torch.Tensor, got %s" % type(mesh).__name__)
    if mesh.dtype != torch.float64:
        raise TypeError("mesh must be float64, got %s" % mesh.dtype)
    if mesh.dim() != 5 or tuple(mesh.shape[:2]) != (n_out, N) or mesh.shape[4] != 2:
        raise ValueError("mesh must be (n_out, N, GH + 1, GW + 1, 2) with (n_out, N) = %s as the matrices, got shape %s"
                         % ((n_out, N), tuple(mesh.shape)))
    if mesh.device != dev:
        raise ValueError("mesh is on %s, the frames on %s: both must be on one device" % (mesh.device, dev))
    return _check_grid((int(mesh.shape[2]) - 1, int(mesh.shape[3]) - 1), H, W)


def mosaic_mesh(frames, sources, matrices, mesh, size, *, mode="median", masks=None, layout="NCHW", out_dtype=None, gains=None):
    """mosaic with a spatially varying displacement per source: at output pixel q, source k of output o is sampled at
    M q + d, M = matrices[o, k] and d the bilinear interpolation of the slot's table mesh[o, k] at the mesh coordinates of
    M q, clamped to the mesh -- warp_mesh's rule, with a table per (output, source) instead of one per frame.  mesh (n_out, N,
    GH + 1, GW + 1, 2) float64 (dx, dy) on the frames' device, the vertices of mesh_motion's mesh on the FRAMES' H x W (the
    table is looked up in the source frame's coordinates); it is passed as (n_out * N, GH + 1, GW + 1, 2): a view where its
    strides allow (a contiguous tensor, a slice along one of its axes, an expanded one), a copy otherwise.  The source is live
    where the moved point lies inside its frame (and no tap is masked), and "feather" weighs by the moved point; every other
    argument, the four modes, the limits (255 sources, 64 for the median) and the result Mosaic(out, count) are mosaic's.  A
    table of +0.0 gives mosaic's bytes; one source per output, source o = frame o, on a canvas of the frames' size under
    mode "first" gives warp_mesh's out, and its valid as count.  A tile drops a source only by its matrix's corner box widened
    by the extremes of the source's table, which a small kernel reduces first: no byte depends on it.
    include/papof.h (papof_mosaic_mesh_tensor) states the rule exactly; bitwise reproducible.  Every argument error raises
    before anything is launched; enqueued on the current stream, returns without waiting."""
    return _mosaic_call(_MESH, frames, sources, matrices, (size, mesh), mode, masks, layout, out_dtype, gains)


def neighbour_mesh(mesh_motion, radius, fill_radius):
    """The displacement tables that go with neighbour_transforms(transforms, motion, fill_radius) when the video is stabilized
    by stabilizing_transforms and mesh_transforms(mesh_motion, radius): mesh_motion a MeshMotion or its residuals (T - 1,
    GH + 1, GW + 1, 2).  In float64 on the host (one small copy from the device: a wait), from mesh_profiles's accumulated
    profile C and tables D = C - S: E[t, slot of s] = D[t] + (C[s] - C[t]) -- the stabilized pixel to frame t by t's own table,
    then from t to s by what the vertex moved beyond the global motion in between -- in neighbour_transforms's slot order
    (slot 0: t itself, E[t, 0] = D[t], mesh_transforms's table; slot 2 d - 1: t - d; slot 2 d: t + d), +0.0 where s is
    outside the video.  Returns (T, 2 fill_radius + 1, GH + 1, GW + 1, 2) float64 on the motion's device, for mosaic_mesh.
    The profile is the motion AT a vertex's position, not along a trajectory, and registers a neighbour only as well as the
    profiles do (README)."""
    import numpy as np
    r = _check_residuals(mesh_motion)
    if isinstance(radius, bool) or not isinstance(radius, int) or radius < 0:
        raise ValueError("radius must be an integer >= 0, got %r" % (radius,))
    _check_fill_radius(fill_radius)
    C = _accumulated_profiles(r.detach().to("cpu", _torch().float64).numpy())
    D = _profile_tables(C, radius)
    T = C.shape[0]
    E = np.zeros((T, 2 * fill_radius + 1) + C.shape[1:])
    for t in range(T):
        E[t, 0] = D[t]
        for d in range(1, fill_radius + 1):
            for slot, s in ((2 * d - 1, t - d), (2 * d, t + d)):
                if 0 <= s < T:
                    E[t, slot] = D[t] + (C[s] - C[t])
    return _torch().from_numpy(E).to(r.device)


def stabilize_video_mesh_full(frames, pyramidLevels, *, fill_radius=15, grid=GRID, radius=15, crop=1.0, model="similarity",
                              iters=5, scale=1.0, min_support=MIN_SUPPORT, spatial=True, consistency=CONSISTENCY,
                              layout="NCHW", out_dtype=None, **solver):
    """stabilize_video_mesh whose frames have no empty border: where mesh-stabilized frame t does not cover a pixel, the
    frames t - 1, t + 1, t - 2, ... t +- fill_radius that saw it supply it, each registered by the global motions AND by its
    own displacement table -- stabilize_video_mesh's chain with the final warp_mesh replaced by ONE mosaic_mesh(...,
    mode="first") over neighbour_transforms and neighbour_mesh.  Every argument of stabilize_video_mesh, and fill_radius as
    stabilize_video_full's.  Returns MeshStabilizedFull: MeshStabilized's fields -- valid (T, H, W) bool as
    stabilize_video_mesh gives it (slot 0 alone): where it holds, the video is stabilize_video_mesh's byte for byte; mesh
    (T, GH + 1, GW + 1, 2): the frames' own tables -- and filled (T, H, W) bool: not valid, and supplied by a neighbour.
    Pixels that are neither stay 0.  With fill_radius=0 the video is stabilize_video_mesh's.  A neighbour registers as well
    as the vertex profiles do and no better; this is no local inpainting (README).  Every argument error raises before
    anything is launched; the video is enqueued on the current stream."""
    p = _mesh_stabilizer(frames, pyramidLevels, grid, radius, crop, model, iters, scale, min_support, spatial, consistency, layout,
                         out_dtype, solver, check=lambda: _check_fill_radius(fill_radius))
    torch = _torch()
    (T, H, W, C), _, _ = p.descs[0]
    src, mats = neighbour_transforms(p.M, p.m, fill_radius)
    E = neighbour_mesh(p.mm, radius, fill_radius)
    video, count = _mosaic(p.ts, p.descs, src, mats, capi.DTYPE_F64, None, H, W, "first", layout, p.out_dtype, rule=_MESH,
                           tables=(E,) + p.grid)
    # valid: slot 0 alone, on one channel (a view), through the same kernel -- its count is the frame's own coverage
    one = p.ts[0][:, :1] if layout == "NCHW" else p.ts[0][..., :1]
    _, own = _mosaic([one], [descriptor(one, layout)], src[:, :1].contiguous(), mats[:, :1], capi.DTYPE_F64, None, H, W,
                     "first", layout, torch.uint8, rule=_MESH, tables=(E[:, :1],) + p.grid)
    valid = own > 0
    return MeshStabilizedFull(video, valid, p.M, p.m.motion, p.m.ok, p.flow, p.timing, E[:, 0], p.mm.vertices, p.mm.support,
                              (count > 0) & ~valid)


# ---- the homography model: the calls above over 3 x 3 matrices
def _homography_fit(flow, code, occlusion, iters, scale):
    torch = _torch()
    B, _, H, W = (int(x) for x in flow.shape)
    dev = flow.device
    motion = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((B,), dtype=torch.uint8, device=dev)
    support = torch.empty((B,), dtype=torch.float64, device=dev)
    d_flow = _flow_struct(flow, code)
    d_occ = _flow_struct(occlusion, capi.DTYPE_U8) if occlusion is not None else None
    d_m = _struct(motion, (motion.stride(0), motion.stride(1), motion.stride(2), 0), capi.DTYPE_F64)
    d_ok = _struct(ok, (ok.stride(0), 0, 0, 0), capi.DTYPE_U8)
    d_s = _struct(support, (support.stride(0), 0, 0, 0), capi.DTYPE_F64)
    _launch(dev, "papof_homography_fit_tensor", B, H, W, ctypes.byref(d_flow), _ref(d_occ), iters, scale, ctypes.byref(d_m),
            ctypes.byref(d_ok), ctypes.byref(d_s),
            workspace=("papof_homography_workspace", (B, H, W), "a %d x %d flow is too large for global_homography" % (H, W)))
    return Homography(motion, ok.view(torch.bool), support)


def global_homography(flow, *, occlusion=None, iters=5, scale=1.0):
    """global_motion with a homography as the model -- the motion of the image under a camera that rotates: flow, occlusion,
    iters and scale as there.  Every valid pixel contributes its two rows of the direct linear transform in normalised
    coordinates, weighted by the Cauchy weight of its pixel distance to the previous iteration's homography over the square
    of that homography's denominator (so that the rows measure pixels); an 8 x 8 solve per iteration.  Returns
    Homography(motion (B, 3, 3) float64 with motion[:, 2, 2] == 1 -- (x, y, 1) of frame i to frame i + 1, up to the third
    coordinate --, ok (B,) bool -- False where no fit was possible (motion is the identity) --, support (B,) float64: the
    last iteration's sum of Cauchy weights over H * W).  A fit whose horizon would cross the image fails.  include/papof.h
    (papof_homography_fit_tensor) states the rule exactly; bitwise reproducible.  Enqueued on the current stream; returns
    without waiting."""
    iters, scale = _check_irls(iters, scale)
    code = _check_flow("flow", flow)
    occ = _check_occlusion(occlusion, tuple(flow.shape), flow.device)
    if not _on_gpu(flow):
        raise ValueError("flow must be on a HIP device (cuda:N), got %s" % flow.device)
    return _homography_fit(flow, code, occ, iters, scale)


def warp_homography(frames, matrices, *, layout="NCHW", out_dtype=None):
    """warp_affine through 3 x 3 matrices: matrices (B, 3, 3) float32 / float64 on the frames' device.  Output pixel (x, y) of
    frame i is frames[i] sampled at (Nx / D, Ny / D), (Nx, Ny, D) = M (x, y, 1), or 0 where D is not > 0 (behind the
    horizon) or the point is NaN or outside the frame.  Returns (frames_out, valid (B, H, W) bool) as warp_affine; on
    matrices whose last row is (0, 0, 1), its bytes.  include/papof.h (papof_warp_projective_tensor) states it exactly.
    Enqueued on the current stream; returns without waiting."""
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    m_code = _check_matrices(matrices, descs[0][0][0], ts[0].device, rows=3)
    return _warp(ts, descs, matrices, m_code, layout, out_dtype, "papof_warp_projective_tensor")


def mosaic_homography(frames, sources, matrices, size, *, mode="median", masks=None, layout="NCHW", out_dtype=None,
                      gains=None):
    """mosaic through 3 x 3 matrices: matrices (n_out, N, 3, 3) float32 / float64; every other argument, the four modes, the
    limits (255 sources, 64 for the median) and the result are mosaic's.  Source k is live at output pixel (x, y) where,
    with (Nx, Ny, D) = matrices[o, k] (x, y, 1), D > 0 and (Nx / D, Ny / D) lies inside its frame (and no tap is masked);
    from that point on everything is mosaic's rule.  On matrices whose last row is (0, 0, 1), mosaic's bytes and count.
    include/papof.h (papof_mosaic_projective_tensor) states it exactly; bitwise reproducible.  Enqueued on the current
    stream; returns without waiting."""
    return _mosaic_call(_PROJECTIVE, frames, sources, matrices, size, mode, masks, layout, out_dtype, gains)


def mosaic_overlap_homography(frames, sources, matrices, size, *, masks=None, step=2, bound=1.0, layout="NCHW"):
    """mosaic_overlap through 3 x 3 matrices (n_out, N, 3, 3), liveness as mosaic_homography's: the Overlap that
    exposure_gains takes.  include/papof.h (papof_mosaic_overlap_projective_tensor).  Enqueued on the current stream; returns
    without waiting."""
    return _mosaic_overlap_call(_PROJECTIVE, frames, sources, matrices, size, masks, step, bound, layout)


def homography_transforms(motion, size, *, ref=None, margin=0, max_pixels=MAX_PIXELS):
    """mosaic_transforms for pair homographies: motion a (T - 1, 3, 3) tensor (global_homography's, any device) or a
    Homography (pairs with ok False enter as the identity), size = (H, W) of the frames.  In float64 on the host, the chain
    built as there -- frame t to the reference frame as the product of the pair motions in between, each product divided by
    its [2][2], so the reference frame keeps its integer corners; a pair motion or a product whose [2][2] is not > 0 is
    refused, since dividing by it would turn a frame behind the horizon into one in front of it --; the corners of every frame are projected into the
    reference frame, (x0, y0) is the floor of their minima less `margin` and the canvas reaches the ceiling of their maxima
    plus `margin`; canvas pixel q samples frame t at matrix_t q (projectively), matrix_t = (frame t <- reference)
    translate(x0, y0) over its [2][2].  Returns (matrices (1, T, 3, 3) float64 on the motion's device -- mosaic_homography's,
    for sources=None --, (Hc, Wc), (x0, y0)).  ValueError when a corner of a frame has a denominator that is not > 0 in the
    reference frame (the frame crosses the horizon: a pan too wide for one plane), when the bounds are not finite or when
    Hc * Wc > max_pixels."""
    import numpy as np
    torch = _torch()
    A, dev = _pair_motions(_checked_motion(motion, Homography))
    H, W = _check_canvas(size)
    T = A.shape[0] + 1
    ref = _check_ref(ref, T)
    _int_at_least("margin", margin, 0)
    _int_at_least("max_pixels", max_pixels, 1)
    to_ref, from_ref = _chain(A, ref, _over_last, "no canvas")
    corners = _corners(H, W)
    with np.errstate(all="ignore"):
        pts = np.stack([m @ corners for m in to_ref])  # (T, 3, 4)
        if not (np.isfinite(pts).all() and np.isfinite(np.array(from_ref)).all()):
            raise ValueError("the bounds of the canvas are not finite")
        behind = ~(pts[:, 2] > 0).all(1)
        if behind.any():
            raise ValueError("frame %d crosses the horizon of the reference frame: the pan is too wide for one plane"
                             % int(np.argmax(behind)))
        pts = pts[:, :2] / pts[:, 2:]
        if not np.isfinite(pts).all():
            raise ValueError("the bounds of the canvas are not finite")
        origin, size, shift = _planar_canvas(pts, margin, max_pixels)
        M = np.stack([_over_last(m @ shift) for m in from_ref])[None]
    if not np.isfinite(M).all():
        raise ValueError("the bounds of the canvas are not finite")
    return torch.from_numpy(M).to(dev), size, origin


def panorama_homography(frames, pyramidLevels, *, mode="median", ref=None, step=1, margin=0, masks=None, iters=5, scale=1.0,
                        layout="NCHW", out_dtype=None, exposure=False, **solver):
    """panorama with the homography model, for a camera that rotates: flow_video, global_homography on the flows (iters,
    scale), homography_transforms (ref, margin; the only wait) and ONE mosaic_homography of the frames 0, step, 2 step, ...;
    exposure=True: mosaic_overlap_homography (step 2, bound 1.0) and exposure_gains first, as panorama.  Every argument, the
    limits and the errors are panorama's (there is no `model`).  Returns Panorama with matrices (T, 3, 3) float64 -- canvas to
    frame t, projectively -- and motion (T - 1, 3, 3).  The canvas is one plane: a pan that nears 90 degrees from the
    reference frame is refused by homography_transforms; there is no bundle adjustment, no lens distortion and no parallax
    (README).  Every argument error raises before anything is launched."""
    p = _panorama_head(frames, pyramidLevels, solver, mode, ref, step, margin, masks, layout, out_dtype, exposure)
    iters, scale = _check_irls(iters, scale)
    (T, H, W, _), _, _ = p.descs[0]
    flow, _, timing = _run(p.ts, p.descs, True, T - 1, layout, _torch().float64, pyramidLevels, p.params)
    mo = _homography_fit(flow, capi.DTYPE_F64, None, iters, scale)
    M, size, origin = homography_transforms(mo, (H, W), ref=p.ref, margin=margin)
    image, count, gains = _panorama_tail(p, _PROJECTIVE, M, size)
    return Panorama(image, count, M[0], origin, mo.motion, mo.ok, flow, timing, gains)


# ---- wide panoramas: the mosaic on a canvas of directions (include/papof.h: ray sampling)
WidePanorama = collections.namedtuple("WidePanorama", Panorama._fields + ("focal", "cols", "rows"))
SURFACES = ("cylinder", "sphere")


def _table_struct(t):
    return _struct(t, (t.stride(0), t.stride(1), 0, 0), capi.DTYPE_F32 if t.dtype == _torch().float32 else capi.DTYPE_F64)


def _check_table(name, t, dev):
    """the length n of the (n, 2) float32 / float64 table `t` on `dev` -- TypeError / ValueError otherwise"""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s must be float32 or float64, got %s" % (name, t.dtype))
    if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < 1:
        raise ValueError("%s must be (n, 2) with n >= 1, got %s" % (name, tuple(t.shape)))
    if t.device != dev:
        raise ValueError("%s are on %s, the frames on %s: both must be on one device" % (name, t.device, dev))
    return int(t.shape[0])


def mosaic_rays(frames, sources, matrices, cols, rows, *, mode="median", masks=None, layout="NCHW", out_dtype=None, gains=None):
    """mosaic_homography on a canvas of directions: cols (Wc, 2) with rows (u_x, w_x) and rows (Hc, 2) with rows (s_y, c_y),
    float32 / float64 on the frames' device (any strides), give canvas pixel (x, y) the ray d = (u_x c_y, s_y, w_x c_y); the
    canvas is (Hc, Wc) = the tables' lengths.  Source k is live where, with (Nx, Ny, D) = matrices[o, k] d, D > 0 and
    (Nx / D, Ny / D) lies inside its frame (and no tap is masked); from that point on everything is mosaic's rule, and every
    other argument, the four modes, the limits (255 sources, 64 for the median) and the result are mosaic_homography's.  The
    tables are the caller's -- wide_transforms makes a cylinder's (sin, cos of the column's angle; the row's height, 1) and a
    sphere's (sin, cos of the row's latitude) --, the device evaluates no sine.  On the plane's tables cols = (x, 1), rows =
    (y, 1): mosaic_homography's bytes and count.  include/papof.h (papof_mosaic_ray_tensor) states it exactly; bitwise
    reproducible.  Enqueued on the current stream; returns without waiting."""
    return _mosaic_call(_RAYS, frames, sources, matrices, (cols, rows), mode, masks, layout, out_dtype, gains)


def mosaic_overlap_rays(frames, sources, matrices, cols, rows, *, masks=None, step=2, bound=1.0, layout="NCHW"):
    """mosaic_overlap_homography on a canvas of directions (cols, rows: mosaic_rays'), liveness as mosaic_rays': the Overlap
    that exposure_gains takes.  include/papof.h (papof_mosaic_overlap_ray_tensor).  Enqueued on the current stream; returns
    without waiting."""
    return _mosaic_overlap_call(_RAYS, frames, sources, matrices, (cols, rows), masks, step, bound, layout)


def estimate_focal(motion, size):
    """The focal length in pixels of a camera that rotates, from its pair homographies (Szeliski and Shum 1997): motion a
    (T - 1, 3, 3) tensor or a Homography (pairs with ok False give nothing), size = (H, W) of the frames.  On the host in
    float64.  Per pair, with M the homography conjugated by the principal point ((W - 1) / 2, (H - 1) / 2), K^-1 M K is a
    scaled rotation for K = diag(f, f, 1): its first two rows (of frame i + 1's focal length) have equal norms and are
    orthogonal, and so have its first two columns (frame i's).  Each of the four conditions gives f^2 in closed form; one
    whose denominator is negligible (under 1e-6 of the magnitude of its own terms) or whose f^2 is not positive and finite is
    skipped.  Returns the median of the estimates
    as a float; ValueError naming focal= when no pair gives one -- a camera that does not rotate, or translates."""
    import numpy as np
    A, _ = _pair_motions(_checked_motion(motion, Homography))
    H, W = _check_canvas(size)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    C = np.array([[1.0, 0.0, cx], [0.0, 1.0, cy], [0.0, 0.0, 1.0]])
    Ci = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]])
    tiny = 1e-6  # a denominator below this share of the magnitude of its own terms is negligible: all cancellation
    est = []
    with np.errstate(all="ignore"):
        for a in A:
            m = Ci @ a @ C
            if not np.isfinite(m).all():
                continue
            try:
                (m0, m1, m2), (m3, m4, m5), (m6, m7, _) = _over_det(m).tolist()  # K^-1 m K is now a rotation
            except ValueError:  # a pair that mirrors or is singular gives nothing
                continue
            block = (m0 * m0 + m1 * m1) + (m3 * m3 + m4 * m4)
            last = m6 * m6 + m7 * m7
            for num, den, size_of_den in (
                    # rows 0 and 1 of K^-1 m K, (m0, m1, m2 / f) and (m3, m4, m5 / f): equal norms, then orthogonal
                    (m5 * m5 - m2 * m2, (m0 * m0 + m1 * m1) - (m3 * m3 + m4 * m4), block),
                    (-(m2 * m5), m0 * m3 + m1 * m4, block),
                    # columns 0 and 1, (m0, m3, f m6) and (m1, m4, f m7)
                    ((m0 * m0 + m3 * m3) - (m1 * m1 + m4 * m4), m7 * m7 - m6 * m6, last),
                    (-(m0 * m1 + m3 * m4), m6 * m7, last)):
                if abs(den) > tiny * size_of_den:
                    f2 = num / den
                    if f2 > 0 and math.isfinite(f2):
                        est.append(math.sqrt(f2))
    if not est:
        raise ValueError("no pair homography gives a focal length (the camera does not rotate between frames): pass focal=")
    return float(np.median(est))


def _check_focal(focal):
    if isinstance(focal, bool) or not isinstance(focal, (int, float)):
        raise TypeError("focal must be a number of pixels, got %r" % (focal,))
    if not (math.isfinite(focal) and focal > 0):
        raise ValueError("focal must be finite and > 0, got %r" % (focal,))
    return float(focal)


def _check_surface(surface):
    if surface not in SURFACES:
        raise ValueError("surface must be one of %s, got %r" % (SURFACES, surface))
    return surface


def _camera(f, H, W):
    """K = (f 0 cx; 0 f cy; 0 0 1) with the principal point at the frame's middle"""
    import numpy as np
    return np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def _centre_and_border(H, W):
    """the principal point, then every border pixel of a frame (edges bulge on a cylinder), homogeneous: (3, 1 + 2 W + 2 H)"""
    import numpy as np
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    border = np.concatenate([np.stack([xs, np.zeros(W)]), np.stack([xs, np.full(W, H - 1.0)]),
                             np.stack([np.zeros(H), ys]), np.stack([np.full(H, W - 1.0), ys])], axis=1)
    return np.vstack([np.concatenate([[[(W - 1) / 2.0], [(H - 1) / 2.0]], border], axis=1), np.ones((1, 1 + border.shape[1]))])


def _directions(rays, surface, ref):
    """(theta, v, the centres' theta) of the rays (T, 3, n), each frame's centre first: (atan2(x, z), y / hypot(x, z)) on the
    cylinder, (atan2(x, z), atan2(y, hypot(x, z))) on the sphere, theta unwrapped along the chain from frame ref -- each
    frame's centre within pi of its neighbour's, each point within pi of its centre.  ValueError where one is not finite.
    Call it with numpy's warnings off."""
    import numpy as np
    theta = np.arctan2(rays[:, 0], rays[:, 2])
    rho = np.hypot(rays[:, 0], rays[:, 2])
    v = rays[:, 1] / rho if surface == "cylinder" else np.arctan2(rays[:, 1], rho)
    if not (np.isfinite(theta).all() and np.isfinite(v).all()):
        raise ValueError("the bounds of the canvas are not finite")
    two_pi = 2.0 * math.pi
    centre = theta[:, 0].copy()
    for t in range(ref + 1, len(centre)):
        centre[t] = centre[t] - two_pi * np.round((centre[t] - centre[t - 1]) / two_pi)
    for t in range(ref - 1, -1, -1):
        centre[t] = centre[t] - two_pi * np.round((centre[t] - centre[t + 1]) / two_pi)
    return theta - two_pi * np.round((theta - centre[:, None]) / two_pi), v, centre


def _pan_columns(theta, f, margin):
    """(x0, Wc) of a pan of less than a full circle at 1 / f per column: column x is (x0 + x) / f"""
    x0 = math.floor(theta.min() * f) - margin
    return x0, math.ceil(theta.max() * f) + margin - x0 + 1


def _canvas_rows(v, f, surface, margin, Wc, max_pixels):
    """(y0, Hc, the table rows (Hc, 2)) of a canvas of directions of Wc columns at 1 / f per row: row y is (y0 + y) / f, (v, 1)
    of it on the cylinder and (sin v, cos v) on the sphere -- ValueError beyond max_pixels"""
    import numpy as np
    y0 = math.floor(v.min() * f) - margin
    Hc = math.ceil(v.max() * f) + margin - y0 + 1
    if Hc * Wc > max_pixels:
        raise ValueError("the canvas is %d x %d, more than max_pixels = %d" % (Hc, Wc, max_pixels))
    vv = (y0 + np.arange(Hc, dtype=np.float64)) / f
    return y0, Hc, np.stack([vv, np.ones(Hc)], axis=1) if surface == "cylinder" else np.stack([np.sin(vv), np.cos(vv)], axis=1)


def wide_transforms(motion, size, focal, *, surface="cylinder", ref=None, margin=0, max_pixels=MAX_PIXELS):
    """The canvas of a wide pan, as directions: motion a (T - 1, 3, 3) tensor (global_homography's, any device) or a
    Homography (pairs with ok False enter as the identity), size = (H, W) of the frames, focal the focal length in pixels
    (estimate_focal's), surface "cylinder" or "sphere" about the reference frame's vertical axis.  In float64 on the host, the
    chain built as homography_transforms builds it, but every pair motion and every product is divided by the cube root of its
    determinant, not by its [2][2] -- a scale that keeps its sign when a frame passes 90 degrees from the reference (the
    [2][2] goes through 0 there); a determinant that is not finite and > 0 is refused, and there is no horizon test: frames
    behind the reference are the purpose.  With K = (f 0 cx; 0 f cy; 0 0 1) and the principal point (cx, cy) = ((W - 1) / 2,
    (H - 1) / 2), matrix_t = (frame t <- reference) K sends a ray of the reference camera to frame t.  Every border pixel of
    every frame (edges bulge on a cylinder) is sent back to its ray (x, y, z) and to (theta, v) = (atan2(x, z), y / hypot(x,
    z)) on the cylinder or (atan2(x, z), atan2(y, hypot(x, z))) on the sphere, theta unwrapped along the chain: each frame's
    centre within pi of its neighbour's, each border point within pi of its centre.  One canvas pixel is 1 / f (radian, or
    height): the reference frame's centre keeps its scale.  Column x is theta_0 + x / f with cols[x] = (sin, cos) of it; row y
    is v_0 + y / f with rows[y] = (v, 1) on the cylinder, (sin v, cos v) on the sphere; (theta_0, v_0) is the floor of the
    bounds' minima in pixels, less `margin`.  Returns (matrices (1, T, 3, 3) float64 -- mosaic_rays', for sources=None --,
    cols (Wc, 2), rows (Hc, 2) float64, (Hc, Wc), origin = (theta_0, v_0)), the tensors on the motion's device.  ValueError
    when theta spans 2 pi or more, when the bounds are not finite (a cylinder under a camera pitched to the pole) or when
    Hc * Wc > max_pixels."""
    import numpy as np
    torch = _torch()
    A, dev = _pair_motions(_checked_motion(motion, Homography))
    H, W = _check_canvas(size)
    f = _check_focal(focal)
    _check_surface(surface)
    T = A.shape[0] + 1
    ref = _check_ref(ref, T)
    _int_at_least("margin", margin, 0)
    _int_at_least("max_pixels", max_pixels, 1)
    K, pts = _camera(f, H, W), _centre_and_border(H, W)
    to_ref, from_ref = _chain(A, ref, _over_det, "no canvas")
    with np.errstate(all="ignore"):
        Ki = np.linalg.inv(K)
        theta, v, _ = _directions(np.stack([Ki @ (m @ pts) for m in to_ref]), surface, ref)
        if not np.isfinite(np.array(from_ref)).all():
            raise ValueError("the bounds of the canvas are not finite")
        if not theta.max() - theta.min() < 2.0 * math.pi:
            raise ValueError("the pan spans %.1f degrees: a canvas holds less than 360" % math.degrees(theta.max() - theta.min()))
        x0, Wc = _pan_columns(theta, f, margin)
        y0, Hc, rows = _canvas_rows(v, f, surface, margin, Wc, max_pixels)
        th = (x0 + np.arange(Wc, dtype=np.float64)) / f
        cols = np.stack([np.sin(th), np.cos(th)], axis=1)
        M = np.stack([_over_det(m @ K) for m in from_ref])[None]
    if not np.isfinite(M).all():
        raise ValueError("the bounds of the canvas are not finite")
    return (torch.from_numpy(M).to(dev), torch.from_numpy(cols).to(dev), torch.from_numpy(rows).to(dev), (Hc, Wc),
            (x0 / f, y0 / f))


def panorama_wide(frames, pyramidLevels, *, focal=None, surface="cylinder", mode="median", ref=None, step=1, margin=0,
                  masks=None, iters=5, scale=1.0, layout="NCHW", out_dtype=None, exposure=False, **solver):
    """panorama_homography on a cylinder or a sphere, for a pan wider than a plane holds (the plane stretches 4 x at 60 degrees
    from the reference frame and ends at 90): flow_video, global_homography on the flows (iters, scale), estimate_focal on the
    homographies unless `focal` (pixels) is given, wide_transforms (surface, ref, margin; the only wait) and ONE mosaic_rays of
    the frames 0, step, 2 step, ...; exposure=True: mosaic_overlap_rays (step 2, bound 1.0) and exposure_gains first, as
    panorama.  Every other argument, the limits and the errors are panorama_homography's.  Returns WidePanorama: Panorama's
    fields -- matrices (T, 3, 3) float64, a ray of the reference camera to frame t; origin (theta_0, v_0), the direction of
    canvas pixel (0, 0) -- and focal, cols (Wc, 2), rows (Hc, 2): the canvas' tables.  A pan of 360 degrees or more is refused
    and a full circle does not close (no bundle adjustment); one focal length for all frames, no lens distortion, no parallax
    (README).  Every argument error raises before anything is launched."""
    p = _panorama_head(frames, pyramidLevels, solver, mode, ref, step, margin, masks, layout, out_dtype, exposure)
    iters, scale = _check_irls(iters, scale)
    _check_surface(surface)
    if focal is not None:
        focal = _check_focal(focal)
    (T, H, W, _), _, _ = p.descs[0]
    flow, _, timing = _run(p.ts, p.descs, True, T - 1, layout, _torch().float64, pyramidLevels, p.params)
    mo = _homography_fit(flow, capi.DTYPE_F64, None, iters, scale)
    if focal is None:
        focal = estimate_focal(mo, (H, W))
    M, cols, rows, size, origin = wide_transforms(mo, (H, W), focal, surface=surface, ref=p.ref, margin=margin)
    image, count, gains = _panorama_tail(p, _RAYS, M, size, (cols, rows))
    return WidePanorama(image, count, M[0], origin, mo.motion, mo.ok, flow, timing, gains, focal, cols, rows)


# ---- bundle adjustment for a camera that rotates (include/papof.h: papof_bundle_sums_tensor)
Bundle = collections.namedtuple("Bundle", "rotations focal cost accepted support ok")
BundlePanorama = collections.namedtuple("BundlePanorama", WidePanorama._fields + ("rotations", "links", "cost"))
MIN_DEN = 0.0625       # include/papof.h: PAPOF_HOMOGRAPHY_MIN_DEN
BUNDLE_SUMS = 20       # include/papof.h: the sums of a link
BUNDLE_MIN_VALID = 16  # a link with fewer valid samples contributes nothing
BUNDLE_DAMPING = 1e-4  # bundle_adjust's first damping
LINK_GRID = 16         # bundle_links: a LINK_GRID x LINK_GRID grid of frame i's pixels
LINK_CHUNK = 64        # link_flows: pairs per flow_pairs_fb call


def _nearest_rotation(m):
    """the rotation nearest to the 3 x 3 matrix m in the Frobenius norm: U V^T of its SVD, determinant + 1"""
    import numpy as np
    u, _, vt = np.linalg.svd(m)
    if np.linalg.det(u @ vt) < 0:
        u = u * np.array([1.0, 1.0, -1.0])
    return u @ vt


def _rodrigues(w):
    """exp([w]x) of the rotation vector w (3,)"""
    import numpy as np
    t = float(np.sqrt(w @ w))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-8:  # sin t / t and (1 - cos t) / t^2 to the second order
        return np.eye(3) + Kx + 0.5 * (Kx @ Kx)
    return np.eye(3) + (math.sin(t) / t) * Kx + ((1.0 - math.cos(t)) / (t * t)) * (Kx @ Kx)


def _check_rotations(name, rotations, n=None):
    """the (T, 3, 3) float64 numpy array and the device of `rotations`, a tensor of finite entries -- TypeError / ValueError
    otherwise"""
    import numpy as np
    torch = _torch()
    if not isinstance(rotations, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(rotations).__name__))
    if rotations.dim() != 3 or tuple(rotations.shape[1:]) != (3, 3) or rotations.shape[0] < 1:
        raise ValueError("%s must be (T, 3, 3) with T >= 1, got shape %s" % (name, tuple(rotations.shape)))
    if n is not None and rotations.shape[0] != n:
        raise ValueError("%s has %d matrices, %d are needed" % (name, rotations.shape[0], n))
    R = rotations.detach().to("cpu", torch.float64).numpy()
    if not np.isfinite(R).all():
        raise ValueError("%s has an entry that is not finite" % name)
    return R, rotations.device


def _check_links(links, T):
    """the (L, 2) int64 numpy array of `links`, pairs (i, j) of two different frames of 0 .. T - 1 -- TypeError / ValueError
    otherwise"""
    import numpy as np
    torch = _torch()
    if isinstance(links, torch.Tensor):
        links = links.detach().cpu().numpy()
    try:
        a = np.asarray(links)
    except Exception:
        raise TypeError("links must be an (L, 2) array of frame indices, got %s" % type(links).__name__) from None
    if a.dtype.kind not in "iu":
        raise TypeError("links must hold integers, got %s" % a.dtype)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError("links must be (L, 2) with L >= 1, got shape %s" % (a.shape,))
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= T or (a[:, 0] == a[:, 1]).any():
        raise ValueError("links must join two different frames of 0 .. %d" % (T - 1))
    return a


def chain_rotations(motion, size, focal, *, ref=None):
    """The absolute rotations of a chain of pair homographies: motion, size, focal and ref as wide_transforms', and its chain --
    frame t to the reference frame as the product of the pair motions in between, every factor and product divided by the
    cube root of its determinant (one that is not finite and > 0 is refused).  With K = (f 0 cx; 0 f cy; 0 0 1), K^-1 (frame
    t <- reference) K is a rotation when the homographies are exact and near one otherwise: each is replaced by the nearest
    rotation (U V^T of its SVD, determinant + 1).  Returns (T, 3, 3) float64 on the motion's device: frame t sees the ray d of
    the reference camera at K R_t d; R_ref is the identity.  The start of bundle_adjust."""
    import numpy as np
    torch = _torch()
    A, dev = _pair_motions(_checked_motion(motion, Homography))
    H, W = _check_canvas(size)
    f = _check_focal(focal)
    T = A.shape[0] + 1
    ref = _check_ref(ref, T)
    K = _camera(f, H, W)
    Ki = np.linalg.inv(K)
    _, from_ref = _chain(A, ref, _over_det, "no rotations")
    with np.errstate(all="ignore"):
        G = np.stack([Ki @ m @ K for m in from_ref])
    if not np.isfinite(G).all():
        raise ValueError("the camera path is not finite")
    return torch.from_numpy(np.stack([_nearest_rotation(g) for g in G])).to(dev)


def _link_overlap(R, H, W, f):
    """the share of the LINK_GRID x LINK_GRID grid of a frame's pixels that the rotations R (..., 3, 3) = R_j R_i^T send inside
    frame j with qz > MIN_DEN"""
    import numpy as np
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    gx, gy = np.meshgrid(np.linspace(0.0, W - 1.0, LINK_GRID), np.linspace(0.0, H - 1.0, LINK_GRID))
    p = np.stack([(gx.reshape(-1) - cx) / f, (gy.reshape(-1) - cy) / f, np.ones(LINK_GRID * LINK_GRID)])
    with np.errstate(all="ignore"):
        q = R @ p
        X, Y = f * q[..., 0, :] / q[..., 2, :] + cx, f * q[..., 1, :] / q[..., 2, :] + cy
        inside = (q[..., 2, :] > MIN_DEN) & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    return inside.mean(-1)


def _check_link_bounds(min_overlap, max_links):
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, float)):
        raise TypeError("min_overlap must be a number, got %r" % (min_overlap,))
    if not 0 < min_overlap <= 1:
        raise ValueError("min_overlap must be in (0, 1], got %r" % (min_overlap,))
    if max_links is not None:
        _int_at_least("max_links", max_links, 1)


def bundle_links(rotations, size, focal, *, min_overlap=0.3, max_links=None):
    """The frame pairs that a bundle adjustment joins: rotations (T, 3, 3) (chain_rotations', any device), size = (H, W) of the
    frames, focal in pixels.  On the host in float64.  The pair (i, j), i < j, is a link when at least `min_overlap` (in (0,
    1]) of a fixed 16 x 16 grid of frame i's pixels (the corners included) lands inside frame j in front of its horizon (qz >
    0.0625) under R_j R_i^T; the consecutive pairs (t, t + 1) are links whatever their overlap.  Returns the links sorted, as
    an (L, 2) int64 array (numpy).  On a full circle these include the pairs that close the loop, (0, T - 1) first.
    ValueError when L exceeds `max_links` (None: no bound)."""
    import numpy as np
    R, _ = _check_rotations("rotations", rotations)
    H, W = _check_canvas(size)
    f = _check_focal(focal)
    _check_link_bounds(min_overlap, max_links)
    T = R.shape[0]
    if T < 2:
        raise ValueError("rotations must hold at least 2 frames, got %d" % T)
    out = []
    for i in range(T - 1):
        share = _link_overlap(R[i + 1:] @ R[i].T, H, W, f)
        out += [(i, i + 1 + int(k)) for k in np.nonzero((share >= min_overlap) | (np.arange(T - 1 - i) == 0))[0]]
    if max_links is not None and len(out) > max_links:
        raise ValueError("%d links, more than max_links = %d: raise min_overlap" % (len(out), max_links))
    return np.array(out, dtype=np.int64)


def _rotation_flow(R, H, W, f, dev):
    """the flow of K R K^-1 for the rotations R (L, 3, 3) float64 on `dev`, in torch operations: (L, 2, H, W) float64, zero
    where the denominator is not > MIN_DEN or a component is not finite or beyond INIT_MAX"""
    torch = _torch()
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    x = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    px, py = (x - cx) / f, (y - cy) / f
    r = R.view(-1, 9, 1, 1)
    qx = (r[:, 0] * px + r[:, 1] * py) + r[:, 2]
    qy = (r[:, 3] * px + r[:, 4] * py) + r[:, 5]
    qz = (r[:, 6] * px + r[:, 7] * py) + r[:, 8]
    flow = torch.stack([f * qx / qz + cx - x, f * qy / qz + cy - y], 1)
    good = (qz > MIN_DEN).unsqueeze(1) & (flow.abs() <= INIT_MAX)  # (a NaN compares False)
    return torch.where(good.all(1, keepdim=True), flow, torch.zeros((), dtype=torch.float64, device=dev))


def _link_flows(ts, descs, links, R, f, levels, layout, out_dtype, alphas, params, chunk):
    torch = _torch()
    (T, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    Rt = torch.from_numpy(R).to(dev)
    out = []
    for k in range(0, len(links), chunk):
        li = torch.from_numpy(links[k:k + chunk, 0]).to(dev)
        lj = torch.from_numpy(links[k:k + chunk, 1]).to(dev)
        a, b = ts[0].index_select(0, li), ts[0].index_select(0, lj)
        fw = _rotation_flow(Rt[lj] @ Rt[li].transpose(1, 2), H, W, f, dev)
        bw = _rotation_flow(Rt[li] @ Rt[lj].transpose(1, 2), H, W, f, dev)
        pair = [a, b]
        d = [descriptor(t, layout) for t in pair]
        out.append(_run_fb(pair, d, False, len(li), layout, out_dtype, levels, alphas, params, fw, bw))
    if len(out) == 1:
        return out[0]
    cat = lambda i: torch.cat([o[i] for o in out]) if out[0][i] is not None else None  # noqa: E731
    timing = {k: "%f" % sum(float(o.timing[k]) for o in out) for k in out[0].timing}
    return FlowFB(cat(0), cat(1), cat(2), cat(3), cat(4), timing)


def link_flows(frames, links, rotations, focal, pyramidLevels=2, *, layout="NCHW", out_dtype=None, consistency=CONSISTENCY,
               chunk=LINK_CHUNK, **solver):
    """The flows of a bundle adjustment's links: flow_pairs_fb on (frames[i], frames[j]) for every row (i, j) of `links`
    ((L, 2) integers, bundle_links'), at most `chunk` pairs per call, each pair started from the flow that its rotations
    predict -- init_flow = the flow of K (R_j R_i^T) K^-1 and init_flow_bw its inverse's, made with torch operations from
    rotations (T, 3, 3) and focal; zero where the denominator is not > 0.0625 or the value is not finite or beyond 1e6.  So a
    pair of frames far apart in time and 60 px apart in the image is within the solver's reach at two pyramid levels.
    Returns a FlowFB over the L links in their order (timing: the calls' timers added).  Every argument error raises before
    anything is launched."""
    alphas = _alphas(consistency)
    ts, descs, out_dtype, params = _check([("frames", frames)], layout, out_dtype, pyramidLevels, min_frames=2, solver=solver)
    (T, H, W, C), _, _ = descs[0]
    R, _ = _check_rotations("rotations", rotations, T)
    f = _check_focal(focal)
    links = _check_links(links, T)
    _int_at_least("chunk", chunk, 1)
    return _link_flows(ts, descs, links, R, f, pyramidLevels, layout, out_dtype, alphas, params, chunk)


def _bundle_sums(flow, code, occlusion, rot, step, scale):
    torch = _torch()
    L, _, H, W = (int(x) for x in flow.shape)
    dev = flow.device
    sums = torch.empty((L, BUNDLE_SUMS), dtype=torch.float64, device=dev)
    d_flow = _flow_struct(flow, code)
    d_occ = _flow_struct(occlusion, capi.DTYPE_U8) if occlusion is not None else None
    d_rot = _struct(rot, (rot.stride(0), rot.stride(1), 0, 0), capi.DTYPE_F64)
    d_sums = _struct(sums, (sums.stride(0), sums.stride(1), 0, 0), capi.DTYPE_F64)
    _launch(dev, "papof_bundle_sums_tensor", L, H, W, step, ctypes.byref(d_flow), _ref(d_occ), ctypes.byref(d_rot), scale,
            ctypes.byref(d_sums),
            workspace=("papof_bundle_workspace", (L, H, W, step), "a %d x %d flow is too large for bundle_sums" % (H, W)))
    return sums


def _check_bundle(flow, occlusion, step, scale):
    """(the flow's dtype code, the mask as uint8, step, scale) of the arguments that bundle_sums and bundle_adjust share"""
    _, scale = _check_irls(1, scale)
    _int_at_least("step", step, 1)
    code = _check_flow("flow", flow)
    occ = _check_occlusion(occlusion, tuple(flow.shape), flow.device)
    if not _on_gpu(flow):
        raise ValueError("flow must be on a HIP device (cuda:N), got %s" % flow.device)
    return code, occ, step, scale


def bundle_sums(flow, rotations_ij, focal, *, occlusion=None, step=1, scale=1.0):
    """One evaluation of a bundle adjustment's links on the device: flow (L, 2, H, W) float32 / float64 on a HIP device, any
    strides -- link l's flow from its frame i to its frame j --, rotations_ij (L, 3, 3) the links' R_j R_i^T (any device),
    focal in pixels, occlusion None or the (L, 2, H, W) bool / uint8 mask of flow_pairs_fb (channel 0 is read).  Every
    step-th pixel of every step-th row is sampled; a sample counts where the flow stays inside the frame, is not masked and
    lies in front of the link's horizon.  Returns (L, 20) float64 on the flow's device: the upper triangle of sum w J^T J (10),
    sum w J^T e (4), sum w e^2, sum w, the number of valid samples, sum e^2 and two zeros -- J the Jacobian of the predicted
    point in a small rotation of the link and the focal length, e the observed less the predicted point, w = 1 / (1 + e^2 /
    scale^2).  include/papof.h (papof_bundle_sums_tensor) states every term and the order of the sums; bitwise reproducible,
    and a link's row does not depend on the other links.  Enqueued on the current stream; returns without waiting."""
    import numpy as np
    torch = _torch()
    code, occ, step, scale = _check_bundle(flow, occlusion, step, scale)
    R, _ = _check_rotations("rotations_ij", rotations_ij, int(flow.shape[0]))
    f = _check_focal(focal)
    rot = np.concatenate([R.reshape(-1, 9), np.full((R.shape[0], 1), f)], 1)
    return _bundle_sums(flow, code, occ, torch.from_numpy(rot).to(flow.device), step, scale)


def bundle_solve(evaluate, links, rotations, focal, *, iters=10, ref=0, fix_focal=False):
    """bundle_adjust's host half, in float64 numpy: Levenberg-Marquardt on one rotation per frame and one focal length, over
    `evaluate(R_ij (L, 3, 3), f) -> (L, 20)`, the links' sums at the parameters it is handed (bundle_sums' rule).  links (L,
    2) int64, rotations (T, 3, 3), focal a float.  A link whose count of valid samples (sum 16) is under 16 contributes
    nothing.  The cost is the contributing links' sum w e^2.  Per link the 4 x 4 block (sums 0 .. 9) and the right-hand side
    (10 .. 13) are those of d = (a, df) with a = omega_j - R omega_i: with P = (-R I 0; 0 0 1) they enter the system of
    (omega_0 .. omega_T-1, df) as P^T A P and P^T g; frame `ref`'s three rows and columns are dropped (the gauge) and df's with
    fix_focal.  A step solves (N + damping * diag N) d = g, with the damping starting at 1e-4, and is tried as R_t <- exp([omega_t]x)
    R_t (Rodrigues), f <- f + df: kept when the cost does not increase (the damping is divided by 10), else dropped (the
    damping is multiplied by 10 and the step retried from the kept parameters); a step that makes f not > 0, cannot be
    solved or after which a frame is reached by no contributing link is dropped likewise.  `iters` steps are tried: iters + 1
    evaluations.  Returns (rotations (T, 3, 3), focal, cost -- (iters + 1,) float64, the first evaluation's then every
    tried step's --, accepted (iters,) bool, the kept parameters' sums (L, 20)).  ValueError when at the start a frame is
    reached by no contributing link."""
    import numpy as np
    R = np.array(rotations, dtype=np.float64)
    f = float(focal)
    T, L = R.shape[0], len(links)
    li, lj = links[:, 0], links[:, 1]

    def sums_at(R, f):
        S = np.array(evaluate(R[lj] @ R[li].transpose(0, 2, 1), f), dtype=np.float64)
        live = S[:, 16] >= BUNDLE_MIN_VALID
        S = np.where(live[:, None], S, 0.0)
        reached = np.zeros(T, bool)
        reached[li[live]] = True
        reached[lj[live]] = True
        return S, reached

    S, reached = sums_at(R, f)
    if not reached.all():
        raise ValueError("frame %d is reached by no link with %d valid samples or more" % (int(np.argmin(reached)), BUNDLE_MIN_VALID))
    cost = [float(S[:, 14].sum())]
    kept = cost[0]  # the cost of the kept parameters
    accepted = []
    keep = np.ones(3 * T + 1, bool)
    keep[3 * ref:3 * ref + 3] = False
    keep[3 * T] = not fix_focal
    iu = np.triu_indices(4)
    lam = BUNDLE_DAMPING
    for _ in range(iters):
        N = np.zeros((3 * T + 1, 3 * T + 1))
        g = np.zeros(3 * T + 1)
        for l in range(L):
            if S[l, 16] == 0:
                continue
            A = np.zeros((4, 4))
            A[iu] = S[l, :10]
            A = A + np.triu(A, 1).T
            i, j = int(li[l]), int(lj[l])
            P = np.zeros((4, 7))
            P[:3, :3] = -(R[j] @ R[i].T)
            P[:3, 3:6] = np.eye(3)
            P[3, 6] = 1.0
            idx = np.r_[3 * i:3 * i + 3, 3 * j:3 * j + 3, 3 * T]
            N[np.ix_(idx, idx)] += P.T @ A @ P
            g[idx] += P.T @ S[l, 10:14]
        Nk, gk = N[np.ix_(keep, keep)], g[keep]
        trial = None
        with np.errstate(all="ignore"):
            try:
                d = np.zeros(3 * T + 1)
                d[keep] = np.linalg.solve(Nk + lam * np.diag(np.diag(Nk)), gk)
                if np.isfinite(d).all() and f + d[3 * T] > 0:
                    trial = (np.stack([_rodrigues(d[3 * t:3 * t + 3]) @ R[t] for t in range(T)]), f + float(d[3 * T]))
            except np.linalg.LinAlgError:
                pass
        if trial is None:
            cost.append(math.inf)
            accepted.append(False)
            lam *= 10.0
            continue
        S1, reached = sums_at(*trial)
        c1 = float(S1[:, 14].sum()) if reached.all() else math.inf
        cost.append(c1)
        if c1 <= kept:
            R, f = trial
            S, kept = S1, c1
            accepted.append(True)
            lam /= 10.0
        else:
            accepted.append(False)
            lam *= 10.0
    return R, f, np.array(cost), np.array(accepted, dtype=bool), S


def bundle_adjust(flow, links, rotations, focal, *, occlusion=None, iters=10, scale=1.0, step=1, ref=0, fix_focal=False):
    """Bundle adjustment of a camera that rotates: one joint robust least-squares fit of one rotation per frame and one
    shared focal length to the dense flows of every link -- flow (L, 2, H, W) on a HIP device and occlusion as bundle_sums',
    links (L, 2) integers (bundle_links'; row l = (i, j): flow[l] runs from frame i to frame j), rotations (T, 3, 3) the
    start (chain_rotations'), focal the start in pixels.  Levenberg-Marquardt (bundle_solve states it): each of the iters + 1
    evaluations is one bundle_sums on every `step`-th pixel with Cauchy scale `scale` and one copy of (L, 20) doubles to the
    host, which WAITS for it; the host expands the links' 4 x 4 blocks into the system of 3 (T - 1) + 1 unknowns (frame `ref`
    is fixed as the gauge, the focal length too with fix_focal=True), damps, solves and updates.  Returns Bundle(rotations
    (T, 3, 3) float64 on the flow's device, focal, cost (iters + 1,) float64 numpy -- the history, sum w e^2 over the links
    --, accepted (iters,) bool numpy, support (L,) float64 numpy -- each link's sum of weights over its sampled pixels at the
    returned parameters, 0 for a link that does not contribute --, ok: a step was accepted).  One focal length, no lens
    distortion, no translation (README).  Every argument error raises before anything is launched; ValueError when a frame is
    reached by no link with 16 valid samples."""
    import numpy as np
    torch = _torch()
    code, occ, step, scale = _check_bundle(flow, occlusion, step, scale)
    R, _ = _check_rotations("rotations", rotations)
    T = R.shape[0]
    links = _check_links(links, T)
    if len(links) != flow.shape[0]:
        raise ValueError("flow has %d fields for %d links" % (flow.shape[0], len(links)))
    f = _check_focal(focal)
    _int_at_least("iters", iters, 1)
    ref = _check_ref(ref, T)
    _check_bool("fix_focal", fix_focal)
    seen = np.zeros(T, bool)
    seen[links.reshape(-1)] = True
    if not seen.all():
        raise ValueError("frame %d is in no link" % int(np.argmin(seen)))
    H, W = int(flow.shape[2]), int(flow.shape[3])
    n = ((H - 1) // step + 1) * ((W - 1) // step + 1)

    def evaluate(Rij, fk):
        return bundle_sums(flow, torch.from_numpy(np.ascontiguousarray(Rij)), fk, occlusion=occ, step=step,
                           scale=scale).cpu().numpy()

    R, f, cost, accepted, S = bundle_solve(evaluate, links, R, f, iters=iters, ref=ref, fix_focal=fix_focal)
    return Bundle(torch.from_numpy(R).to(flow.device), f, cost, accepted, S[:, 15] / n, bool(accepted.any()))


def bundle_transforms(rotations, size, focal, *, surface="cylinder", ref=None, margin=0, max_pixels=MAX_PIXELS):
    """wide_transforms from absolute rotations: rotations (T, 3, 3) (bundle_adjust's, any device; frame t sees the ray d at K
    R_t d), size, focal, surface, margin and max_pixels as there; ref names the frame whose centre sets the canvas' middle
    (None: the middle frame) -- the rays are those of the rotations' own reference, which bundle_adjust keeps fixed.  The
    border pixels of every frame go back to their rays R_t^T K^-1 p and to (theta, v) as there, theta unwrapped along the
    frames' order.  Where theta spans less than 2 pi, the canvas is wide_transforms': column x is theta_0 + x / f.  Where it
    spans 2 pi or more the canvas is the FULL CIRCLE: Wc = round(2 pi f) columns at a pitch of 2 pi / Wc, column x at
    theta_ref - pi + x * pitch with theta_ref the direction of frame ref's centre, so that column Wc - 1's neighbour is
    column 0; mosaic_rays needs to know nothing, its liveness is "in front of the camera and inside the frame".  Rows as
    there, at 1 / f.  Returns (matrices (1, T, 3, 3) float64 = K R_t over the cube root of f^2, cols (Wc, 2), rows (Hc, 2),
    (Hc, Wc), origin = (theta_0, v_0)), the tensors on the rotations' device.  ValueError when the bounds are not finite or
    Hc * Wc > max_pixels."""
    import numpy as np
    torch = _torch()
    R, dev = _check_rotations("rotations", rotations)
    H, W = _check_canvas(size)
    f = _check_focal(focal)
    _check_surface(surface)
    T = R.shape[0]
    ref = _check_ref(ref, T)
    _int_at_least("margin", margin, 0)
    _int_at_least("max_pixels", max_pixels, 1)
    K = _camera(f, H, W)
    two_pi = 2.0 * math.pi
    with np.errstate(all="ignore"):
        theta, v, centre = _directions(R.transpose(0, 2, 1) @ (np.linalg.inv(K) @ _centre_and_border(H, W)), surface, ref)
        full = not theta.max() - theta.min() < two_pi
        if full:
            Wc, th0 = int(round(two_pi * f)), float(centre[ref]) - math.pi
        else:
            x0, Wc = _pan_columns(theta, f, margin)
            th0 = x0 / f
        y0, Hc, rows = _canvas_rows(v, f, surface, margin, Wc, max_pixels)
        cells = np.arange(Wc, dtype=np.float64)
        th = th0 + cells * (two_pi / Wc) if full else (x0 + cells) / f
        cols = np.stack([np.sin(th), np.cos(th)], axis=1)
        M = (K @ R / np.cbrt(f * f))[None]
    if not np.isfinite(M).all():
        raise ValueError("the bounds of the canvas are not finite")
    return (torch.from_numpy(M).to(dev), torch.from_numpy(cols).to(dev), torch.from_numpy(rows).to(dev), (Hc, Wc),
            (th0, y0 / f))


def panorama_bundle(frames, pyramidLevels, *, focal=None, surface="cylinder", mode="median", ref=None, step=1, margin=0,
                    masks=None, iters=5, scale=1.0, layout="NCHW", out_dtype=None, exposure=False, bundle_iters=10,
                    min_overlap=0.3, link_levels=2, bundle_step=1, max_links=None, fix_focal=False, **solver):
    """panorama_wide with a bundle adjustment between the homographies and the canvas, so that the pairs' errors no longer
    add up and a full circle can close: flow_video, global_homography on the flows (iters, scale), estimate_focal unless
    `focal` is given (now only the start), chain_rotations, a FIRST bundle_adjust of the consecutive links alone with the focal
    length held (it turns the chain of nearest rotations into the rotations that fit the flows at that focal length, which is
    what the next two steps start from), bundle_links (min_overlap, max_links), link_flows at `link_levels` pyramid levels for
    the links that are not consecutive frames, the bundle_adjust of all links (the focal length free unless fix_focal=True),
    bundle_transforms (surface, ref, margin) and ONE mosaic_rays of the frames 0, step, 2 step, ...; exposure=True:
    mosaic_overlap_rays (step 2, bound 1.0) and exposure_gains first.  Both adjustments take bundle_iters steps with the Cauchy
    scale `scale` on every bundle_step-th pixel and keep frame `ref` fixed.  The consecutive links reuse the video's forward
    flows; flow_video computes no backward flow, so they carry no occlusion mask (their pixels that leave the frame are what
    the Cauchy weight is for), while the other links carry link_flows' forward-backward mask.  Every other argument, the
    limits and the errors are panorama_wide's.  Returns BundlePanorama: WidePanorama's fields -- matrices (T, 3, 3) = K R_t up
    to scale, focal the adjusted focal length, motion / ok the pair homographies that started it -- and rotations (T, 3, 3),
    links (L, 2) int64 (numpy) and cost, the last bundle_adjust's history.  A pan of 360 degrees or more gets the full-circle
    canvas; whether the circle CLOSES depends on the start: a link's flow starts from what the rotations predict, so the pair
    that closes the loop is found and followed only when the chain misses it by less than the solver's reach (README: give
    focal= for a full circle).  The host waits once per evaluation; one focal length, no lens distortion, no translation or
    parallax, a few hundred frames at most (README).  Every argument error raises before anything is launched."""
    import numpy as np
    torch = _torch()
    p = _panorama_head(frames, pyramidLevels, solver, mode, ref, step, margin, masks, layout, out_dtype, exposure)
    iters, scale = _check_irls(iters, scale)
    _check_surface(surface)
    if focal is not None:
        focal = _check_focal(focal)
    _int_at_least("bundle_iters", bundle_iters, 1)
    _int_at_least("link_levels", link_levels, 1)
    _int_at_least("bundle_step", bundle_step, 1)
    _check_link_bounds(min_overlap, max_links)
    _check_bool("fix_focal", fix_focal)
    ts, descs, params, ref = p.ts, p.descs, p.params, p.ref
    (T, H, W, _), _, _ = descs[0]
    dev = ts[0].device
    flow, _, timing = _run(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, params)
    mo = _homography_fit(flow, capi.DTYPE_F64, None, iters, scale)
    if focal is None:
        focal = estimate_focal(mo, (H, W))
    chain = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    R0 = bundle_adjust(flow, chain, chain_rotations(mo, (H, W), focal, ref=ref), focal, iters=bundle_iters, scale=scale,
                       step=bundle_step, ref=ref, fix_focal=True).rotations
    links = bundle_links(R0, (H, W), focal, min_overlap=min_overlap, max_links=max_links)
    near = links[:, 1] == links[:, 0] + 1
    flows, occ = flow[torch.from_numpy(links[near, 0]).to(dev)], None
    if not near.all():
        far = _link_flows(ts, descs, links[~near], R0.cpu().numpy(), focal, link_levels, layout, torch.float64,
                          _alphas(CONSISTENCY), params, LINK_CHUNK)
        at = torch.from_numpy(near).to(dev)
        both = torch.empty((len(links), 2, H, W), dtype=torch.float64, device=dev)
        both[at], both[~at] = flows, far.flow_fw
        occ = torch.zeros((len(links), 2, H, W), dtype=torch.uint8, device=dev)
        occ[~at] = far.occlusion.view(torch.uint8)
        flows = both
    b = bundle_adjust(flows, links, R0, focal, occlusion=occ, iters=bundle_iters, scale=scale, step=bundle_step, ref=ref,
                      fix_focal=fix_focal)
    M, cols, rows, size, origin = bundle_transforms(b.rotations, (H, W), b.focal, surface=surface, ref=ref, margin=margin)
    image, count, gains = _panorama_tail(p, _RAYS, M, size, (cols, rows))
    return BundlePanorama(image, count, M[0], origin, mo.motion, mo.ok, flow, timing, gains, b.focal, cols, rows, b.rotations,
                          links, b.cost)


# ---- rotation-path stabilization: one homography per source row (include/papof.h: papof_warp_rows_tensor)
RotationStabilized = collections.namedtuple("RotationStabilized",
                                            "video valid tables rotations smoothed focal motion ok flow timing")
CameraRotations = collections.namedtuple("CameraRotations", "rotations focal motion ok")
MAX_KNOTS = capi.ROWS_MAX_KNOTS  # include/papof.h: PAPOF_ROWS_MAX_KNOTS
MAX_ROWS_ITERS = 8               # include/papof.h: papof_warp_rows_tensor


def _rotation_log(R):
    """the rotation vector w (3,) with exp([w]x) = R, |w| <= pi: with v = the vector of (R - R^T) / 2 = sin t a and
    c = (tr R - 1) / 2 = cos t, t = atan2(|v|, c) and w = v t / sin t.  |v| < 1e-8 with c > 0 is the small-angle branch:
    t / sin t = 1 + t^2 / 6 to the second order (w = v to rounding); |v| < 1e-8 with c <= 0 is a half turn, where v says
    nothing: the axis is the largest column of the symmetric part, (R + R^T) / 2 = c I + (1 - c) a a^T"""
    import numpy as np
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.sqrt(v @ v)), 0.5 * (float(np.trace(R)) - 1.0)
    t = math.atan2(s, c)
    if s >= 1e-8:
        return v * (t / s)
    if c > 0:
        return v * (1.0 + t * t / 6.0)
    B = (0.5 * (R + R.T) - c * np.eye(3)) / (1.0 - c)
    i = int(np.argmax(np.diag(B)))
    a = B[i] / math.sqrt(B[i, i])
    return t * (-a if a @ v < 0 else a)


def _check_rows_iters(iters):
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= MAX_ROWS_ITERS:
        raise ValueError("iters must be an integer in 1 .. %d, got %r" % (MAX_ROWS_ITERS, iters))
    return iters


def _check_knots(knots, H, rolling):
    if isinstance(knots, bool) or not isinstance(knots, int) or not 2 <= knots <= MAX_KNOTS:
        raise ValueError("knots must be an integer in 2 .. %d, got %r" % (MAX_KNOTS, knots))
    if rolling and knots > H:
        raise ValueError("knots must be at most the %d rows of the frames, got %d" % (H, knots))
    return knots


def smooth_rotations(rotations, radius=15):
    """A camera's rotations smoothed on the rotation group: rotations (T, 3, 3), any device (chain_rotations',
    bundle_adjust's: frame t sees the ray d at K R_t d).  In float64 on the host, one pass in the tangent space at each R_t:
        S_t = exp([sum_k g_k log(R_{t+k} R_t^T) / sum_k g_k]x) R_t,  g_k = exp(-k^2 / (2 (radius / 2)^2)),
    k in [-radius, radius] within the video -- stabilizing_transforms' Gaussian and window, on rotation vectors instead of
    matrix entries, so that every S_t is a rotation and there is no path of homographies to smooth.  A rotation at a
    constant rate about one axis comes back unchanged away from the ends of the video.  radius = 0 returns the rotations as
    they are.  Returns (T, 3, 3) float64 on the rotations' device."""
    import numpy as np
    R, dev = _check_rotations("rotations", rotations)
    _check_path(radius, 1.0, None)
    n = R.shape[0]
    S = R.copy()
    for t in range(n if radius > 0 else 0):
        ks = range(max(-radius, -t), min(radius, n - 1 - t) + 1)
        g = [math.exp(-k * k / (2.0 * (radius / 2.0) ** 2)) for k in ks]
        w = sum(gk * _rotation_log(R[t + k] @ R[t].T) for gk, k in zip(g, ks)) / sum(g)
        S[t] = _rodrigues(w) @ R[t]
    return _torch().from_numpy(S).to(dev)


def rotation_rows(rotations, smoothed, focal, size, readout, *, anchor=0.5, knots=17, crop=1.0):
    """The tables that warp_rows takes, for a camera that rotates and reads its rows one after another: rotations (T, 3, 3) the
    camera's, smoothed (T, 3, 3) the stabilized camera's (smooth_rotations'), any device; focal in pixels; size = (H, W);
    readout, anchor as rectify_frames' (source row y of frame t is read at t + tau(y), tau(y) = readout (y - a) / H,
    a = anchor (H - 1)); knots = Kn in 2 .. 4096 and <= H rows at which the family is sampled, knot k at row
    y_k = k (H - 1) / (Kn - 1); crop as stabilizing_transforms'.  In float64 on the host:
        M[t, k] = K R_t(tau(y_k)) S_t^T K^-1 Z,   K = (f 0 cx; 0 f cy; 0 0 1),   Z q = c + crop (q - c)
    and between the frames' own times the camera is the parabola through three rotation vectors at R_t,
        R_t(tau) = exp([w+ tau (tau + 1) / 2 + w- tau (tau - 1) / 2]x) R_t,   w+ = log(R_{t+1} R_t^T),  w- = log(R_{t-1} R_t^T),
    the rotational twin of rectify_frames' parabola; on the two end frames the line through the one neighbour (w+ tau, or
    -w- tau); a single frame does not move.  readout = 0 gives Kn = 1 whatever `knots` says: M[t, 0] = K R_t S_t^T K^-1 Z, and
    warp_rows of it is warp_homography's.  Returns (T, Kn, 3, 3) float64 on the rotations' device."""
    import numpy as np
    R, dev = _check_rotations("rotations", rotations)
    S, _ = _check_rotations("smoothed", smoothed, R.shape[0])
    f = _check_focal(focal)
    H, W = _check_canvas(size)
    readout, anchor, _ = _check_shutter(readout, anchor, 1)
    cx, cy = _check_path(0, crop, (H, W))
    Kn = _check_knots(knots, H, readout != 0)
    if readout == 0:
        Kn = 1
    T = R.shape[0]
    K = _camera(f, H, W)
    Ki = np.linalg.inv(K)
    Z = np.array([[crop, 0.0, cx - crop * cx], [0.0, crop, cy - crop * cy], [0.0, 0.0, 1.0]])
    a = anchor * (H - 1)
    tau = [readout * (k * (H - 1) / (Kn - 1) - a) / H for k in range(Kn)] if Kn > 1 else [0.0]
    M = np.empty((T, Kn, 3, 3))
    for t in range(T):
        wp = _rotation_log(R[t + 1] @ R[t].T) if t + 1 < T else None
        wm = _rotation_log(R[t - 1] @ R[t].T) if t > 0 else None
        right = S[t].T @ Ki @ Z
        for k, s in enumerate(tau):
            if wp is not None and wm is not None:
                w = wp * (s * (s + 1.0) / 2.0) + wm * (s * (s - 1.0) / 2.0)
            elif wp is not None:
                w = wp * s
            elif wm is not None:
                w = wm * -s
            else:
                w = np.zeros(3)
            M[t, k] = K @ (_rodrigues(w) @ R[t]) @ right
    return _torch().from_numpy(M).to(dev)


def _check_tables(tables, n, H, dev):
    """the dtype code and Kn of warp_rows' tables -- TypeError / ValueError otherwise"""
    torch = _torch()
    codes = {torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if not isinstance(tables, torch.Tensor):
        raise TypeError("tables must be a torch.Tensor, got %s" % type(tables).__name__)
    if tables.dtype not in codes:
        raise TypeError("tables must be float32 or float64, got %s" % tables.dtype)
    if tables.dim() != 4 or tables.shape[0] != n or tuple(tables.shape[2:]) != (3, 3):
        raise ValueError("tables must be (B, Kn, 3, 3) with B = %d, got %s" % (n, tuple(tables.shape)))
    Kn = int(tables.shape[1])
    if not 1 <= Kn <= MAX_KNOTS:
        raise ValueError("tables have %d knots per frame, the kernel takes 1 .. %d" % (Kn, MAX_KNOTS))
    if Kn > 1 and H < 2:
        raise ValueError("tables of %d knots need frames of at least two rows, got %d" % (Kn, H))
    if tables.device != dev:
        raise ValueError("tables are on %s, the frames on %s: both must be on one device" % (tables.device, dev))
    return codes[tables.dtype], Kn


def _warp_rows(ts, descs, tables, m_code, Kn, iters, layout, out_dtype):
    """papof_warp_rows_tensor of the checked frames ts[0]: (video, valid (B, H, W) bool)"""
    torch = _torch()
    (B, H, W, C), strides, code = descs[0]
    dev = ts[0].device
    out, d_out = _new_frames(B, H, W, C, layout, out_dtype, dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    d_in = _struct(ts[0], strides, code)
    d_tab = _struct(tables, tuple(tables.stride()), m_code)
    d_valid = _struct(valid, (valid.stride(0), valid.stride(1), valid.stride(2), 1), capi.DTYPE_U8)
    _launch(dev, "papof_warp_rows_tensor", B, H, W, C, ctypes.byref(d_in), ctypes.byref(d_tab), Kn, iters, ctypes.byref(d_out),
            ctypes.byref(d_valid))
    return out, valid.view(torch.bool)


def warp_rows(frames, tables, *, iters=3, layout="NCHW", out_dtype=None):
    """warp_homography with one matrix per SOURCE row: frames as warp_affine's; tables (B, Kn, 3, 3) float32 / float64 on the
    frames' device, any strides (rotation_rows'), Kn >= 1 matrices per frame, knot k at source row k (H - 1) / (Kn - 1).
    Output pixel (x, y) of frame i is frames[i] sampled at (Nx / D, Ny / D), (Nx, Ny, D) = M (x, y, 1), with M the table
    interpolated linearly, entry by entry, at the row Y the point lands in -- which depends on M: `iters` (1 .. 8) fixed-point
    iterations from Y = y, each clamping its row into the frame before it reads the table (the error falls by about
    |dY / dy_source| per iteration: the rows' rotation rate times the focal length, a few per cent for a hand-held camera).
    The last iterate decides: 0 and not valid where D is not > 0 or the point is NaN or outside the frame.  Kn = 1: no
    iteration, warp_homography's bytes.  Returns (frames_out, valid (B, H, W) bool) as warp_affine.  include/papof.h
    (papof_warp_rows_tensor) states it exactly; bitwise reproducible.  Enqueued on the current stream; returns without
    waiting."""
    _check_rows_iters(iters)
    ts, descs, _, _ = _check([("frames", frames)], layout, None, 1)
    out_dtype = _out_dtype(out_dtype, ts[0].dtype)
    (B, H, _, _), _, _ = descs[0]
    m_code, Kn = _check_tables(tables, B, H, ts[0].device)
    return _warp_rows(ts, descs, tables, m_code, Kn, iters, layout, out_dtype)


def _check_camera(size, readout, anchor, rs_iters, focal, iters, scale, bundle_iters, bundle_step):
    """the keywords that camera_rotations and stabilize_video_rotation share: ((H, W), shutter, focal or None, iters, scale)"""
    size = _check_canvas(size)
    shutter = _check_shutter(readout, anchor, rs_iters, "rs_iters")
    if focal is not None:
        focal = _check_focal(focal)
    iters, scale = _check_irls(iters, scale)
    _int_at_least("bundle_iters", bundle_iters, 1)
    _int_at_least("bundle_step", bundle_step, 1)
    return size, shutter, focal, iters, scale


def _camera_rotations(flow, occ, size, focal, iters, scale, bundle_iters, bundle_step, ref):
    """camera_rotations from its step 2 on, on checked arguments: flow the (rectified) float64 forward flows, occ their
    uint8 mask or None"""
    import numpy as np
    mo = _homography_fit(flow, capi.DTYPE_F64, occ, iters, scale)
    if focal is None:
        focal = estimate_focal(mo, size)
    T = int(flow.shape[0]) + 1
    chain = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    b = bundle_adjust(flow, chain, chain_rotations(mo, size, focal, ref=ref), focal, occlusion=occ, iters=bundle_iters,
                      scale=scale, step=bundle_step, ref=ref, fix_focal=True)
    return CameraRotations(b.rotations, focal, mo.motion, mo.ok)


def camera_rotations(flow_fw, size, *, flow_bw=None, readout=0.0, anchor=0.5, rs_iters=3, focal=None, iters=5, scale=1.0,
                     bundle_iters=10, bundle_step=1, ref=0):
    """One rotation per frame and a focal length from a video's flows -- the estimation chain of a camera that rotates, stated
    once: flow_fw (T - 1, 2, H, W) float32 / float64 on a HIP device (flow_video's), size = (H, W) of the frames.
    1. readout != 0 (a rolling shutter; readout, anchor as rectify_frames'): rectify_flows(flow_fw, flow_bw, readout,
       anchor=anchor, iters=rs_iters), for which flow_bw (flow_video_fb's) is required.  Whenever flow_bw is given,
       fb_consistency on the (rectified) flows masks the fits below; rectify_flows' NaNs are all masked, as in
       stabilize_video_rs.
    2. global_homography of the forward flows (iters, scale).
    3. estimate_focal, unless `focal` is given.
    4. chain_rotations (ref: the frame whose rotation is the identity).
    5. bundle_adjust of the consecutive links with the focal length held (bundle_iters, scale, bundle_step, ref): the chain
       of nearest rotations becomes the rotations that fit the flows.
    Returns CameraRotations(rotations (T, 3, 3) float64 on the flows' device -- frame t sees the ray d at K R_t d --, focal,
    motion (T - 1, 3, 3) float64 the pair homographies, ok (T - 1,) bool).  The host waits in steps 3 to 5.  Every argument
    error raises before anything is launched; ValueError as estimate_focal's and bundle_adjust's."""
    size, shutter, focal, iters, scale = _check_camera(size, readout, anchor, rs_iters, focal, iters, scale, bundle_iters,
                                                       bundle_step)
    torch = _torch()
    if flow_bw is None:
        if shutter[0] != 0:
            raise ValueError("readout != 0 rectifies the flows first: give flow_bw (flow_video_fb's)")
        _check_flow("flow_fw", flow_fw)
        if not _on_gpu(flow_fw):
            raise ValueError("flows must be on a HIP device (cuda:N), got %s" % flow_fw.device)
    else:
        codes = _check_flows(flow_fw, flow_bw)
    if tuple(flow_fw.shape[2:]) != size:
        raise ValueError("size %s is not the flows' %s" % (size, tuple(flow_fw.shape[2:])))
    ref = _check_ref(ref, int(flow_fw.shape[0]) + 1)
    occ = None
    if flow_bw is not None:
        fw, bw = flow_fw, flow_bw
        if shutter[0] != 0:
            fw, bw = _rectify_flows((flow_fw, flow_bw), codes, shutter, torch.float64)
        occ = fb_consistency(fw, bw).view(torch.uint8)
        flow_fw = fw
    return _camera_rotations(flow_fw.to(torch.float64), occ, size, focal, iters, scale, bundle_iters, bundle_step, ref)


def stabilize_video_rotation(frames, pyramidLevels, *, readout=0.0, anchor=0.5, rs_iters=3, focal=None, radius=15, crop=1.0,
                             knots=17, iters=3, layout="NCHW", out_dtype=None, fit_iters=5, scale=1.0, bundle_iters=10,
                             **solver):
    """stabilize_video for a hand-held camera that ROTATES, with or without a rolling shutter (Forssen and Ringaby 2010;
    Karpenko et al. 2011): flow_video_fb(consistency=None) when readout != 0, else flow_video (float64 flows);
    camera_rotations on them (readout, anchor, rs_iters, focal, fit_iters as its iters, scale, bundle_iters; ref = 0);
    smooth_rotations (radius); rotation_rows (readout, anchor, knots, crop) and ONE warp_rows (iters) of the recorded frames
    -- the stabilizing homography and the rectification of the rolling shutter in one resampling, where stabilize_video_rs
    removes an affine path and leaves the perspective wobble of a rotation.  Returns RotationStabilized(video (T, ...) in
    `layout` and out_dtype (by default the frames'), valid (T, H, W) bool, tables (T, Kn, 3, 3) float64 (Kn = 1 for
    readout = 0), rotations, smoothed (T, 3, 3) float64, focal, motion (T - 1, 3, 3) float64 and ok (T - 1,) bool the pair
    homographies, flow (T - 1, 2, H, W) float64 the recorded forward flows, timing of the flow call).  What it is not: pure
    rotation -- no translation, no parallax; one focal length; readout is given, not estimated; the end frames use a line;
    the borders are not filled (crop hides them); not causal: the whole video is read first.  The host waits in
    camera_rotations.  Every argument error raises before anything is launched; the video is enqueued on the current
    stream."""
    ts, descs, out_dtype, params = _check_video(frames, layout, pyramidLevels, out_dtype, solver=solver)
    (T, H, W, _), _, _ = descs[0]
    size, shutter, focal, fit_iters, scale = _check_camera((H, W), readout, anchor, rs_iters, focal, fit_iters, scale,
                                                           bundle_iters, 1)
    _check_path(radius, crop, size)
    _check_knots(knots, H, shutter[0] != 0)
    _check_rows_iters(iters)
    torch = _torch()
    occ = None
    if shutter[0] != 0:
        fb = _run_fb(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, _alphas(None), params)
        flow, timing = fb.flow_fw, fb.timing
        fw, bw = _rectify_flows((fb.flow_fw, fb.flow_bw), _F64_FLOWS, shutter, torch.float64)
        occ = fb_consistency(fw, bw).view(torch.uint8)
    else:
        flow, _, timing = _run(ts, descs, True, T - 1, layout, torch.float64, pyramidLevels, params)
        fw = flow
    cam = _camera_rotations(fw, occ, size, focal, fit_iters, scale, bundle_iters, 1, 0)
    S = smooth_rotations(cam.rotations, radius)
    tables = rotation_rows(cam.rotations, S, cam.focal, size, shutter[0], anchor=shutter[1], knots=knots, crop=crop)
    video, valid = _warp_rows(ts, descs, tables, capi.DTYPE_F64, int(tables.shape[1]), iters, layout, out_dtype)
    return RotationStabilized(video, valid, tables, cam.rotations, S, cam.focal, cam.motion, cam.ok, flow, timing)
