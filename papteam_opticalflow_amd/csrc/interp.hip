// papteam_opticalflow_amd/csrc/interp.hip -- motion-compensated frame interpolation (papof_interp_tensor).
//
// Why.  Frames between two frames (frame-rate up-conversion, slow motion; and Middlebury's interpolation error, Baker et al.,
// IJCV 2011, the accepted way to judge a flow without ground truth) from the forward flow, the backward flow and the
// occlusion mask that papof_flow_batch_tensor_fb returns.  Written with grid_sample it is about a dozen launches per
// intermediate frame and several full-frame temporaries through HBM.  Here one lane makes one output pixel of every time:
// the two flows at the pixel are read once, and each time costs two independent groups of bilinear taps (one per frame,
// with the mask's taps at the same offsets) and the stores.
//
// Semantics: include/papof.h, papof_interp_tensor.  The bilinear rule is k_fb_check's and k_track's (the reference's,
// src/ImageProcessing.h:138-157): truncation toward zero, fraction clamped to [0, 1], neighbours clamped into the image,
// taps accumulated from 0 in (m, n) order; fp64 without contraction (-ffp-contract=off).  The sampler and the pixel's rule
// (interp_pixel, which k_interp_splat of splat.hip applies where no splat lands) are sampler.h's.
//
// Mapping.  A block is a 64 x 4 tile of output pixels (InterpTile; the grid of tiles and pairs is grid.h's).  A wave is
// 64 neighbouring pixels of one row, whose taps share cache lines while the flow is smooth and whose stores are contiguous
// along a row.  The times are kernel arguments (at most kMaxTimes per launch; more are launched in groups): they are the
// same for every lane, so they sit in scalar registers with no load, and the call needs no device buffer and no copy to
// fill one -- nothing the caller has to keep alive after the call returns.  Every offset is 64-bit.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

// Times a.t[0 .. a.nt) are written at time slots j0 + j of out.
template <int FD>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_interp(const InterpArgs a, long long tile0, long long pair0,
                                                                 long long j0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    PAPOF_TILE_PIXEL(InterpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    interp_pixel<FD>(a, lut, pair0 + blockIdx.y, r, x, j0, [](int, long long) { return false; });
}

int launch_interp(hipStream_t st, InterpArgs a, int n_pairs, int n_times, const double* times) {
    const auto kernel = by_frame_dtype(a.f0.dtype == a.f1.dtype ? a.f0.dtype : -1, [](auto fd) { return k_interp<fd()>; });
    for (int j0 = 0; j0 < n_times; j0 += kMaxTimes) {
        a.nt = std::min(kMaxTimes, n_times - j0);
        std::copy(times + j0, times + j0 + a.nt, a.t);
        PAPOF_TRY(launch_tiles(InterpTile::count(a.H, a.W), n_pairs, [&](dim3 grid, long long t0, long long p0) {
            hipLaunchKernelGGL(kernel, grid, InterpTile::block(), 0, st, a, t0, p0, (long long)j0);
        }));
    }
    return PAPOF_OK;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_interp_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                   const papof_tensor* frames2, int height, int width, int c, const papof_tensor* flow_fw,
                                   const papof_tensor* flow_bw, const papof_tensor* occlusion, int n_times,
                                   const double* times, const papof_tensor* out, long long time_stride, void* stream) {
    if (!h || n_pairs < 1 || height < 1 || width < 1 || c < 1) return PAPOF_EINVAL;
    if (!in_frames(frames) || (sequence ? frames2 != nullptr : !in_frames(frames2))) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (occlusion && !described(occlusion, {PAPOF_DTYPE_U8}, {0, 1, 2, 3}, false)) return PAPOF_EINVAL;
    if (!out_frames(out) || time_stride < 0 || (n_times > 1 && time_stride == 0)) return PAPOF_EINVAL;
    if (n_times < 1 || !times) return PAPOF_EINVAL;
    for (int j = 0; j < n_times; j++)
        if (!std::isfinite(times[j]) || !(times[j] > 0.0 && times[j] < 1.0)) return PAPOF_EINVAL;
    InterpArgs a{};
    a.f0 = *frames;
    a.f1 = sequence ? *frames : *frames2;
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    if (occlusion) a.occ = *occlusion;
    a.out = *out;
    a.tstride = time_stride;
    a.H = height;
    a.W = width;
    a.C = c;
    a.seq = sequence ? 1 : 0;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_interp(static_cast<hipStream_t>(stream), a, n_pairs, n_times, times);
}
