// papteam_opticalflow_amd/csrc/track.hip -- point tracking through a video's flows (papof_track_tensor).
//
// Why.  The forward-backward check of k_fb_check comes from dense point trajectories (Sundaram, Brox, Keutzer 2010): a point is
// followed from frame to frame through the forward flow and dropped where the backward flow does not bring it back.  Each step
// is two DEPENDENT bilinear gathers (the flow at the point, then the reverse flow where it lands) and the consistency test;
// written with grid_sample it is ~4 launches per frame and the position round-trips through HBM each time.  Here one lane
// follows one (query, direction) through all T frames with its state in registers: one launch, no host synchronisation, and
// each (frame, point) entry of the outputs is written once.
//
// Semantics: include/papof.h, papof_track_tensor.  A step is sampler.h's hop: the flow sampled bilinearly by the reference's
// rule (src/ImageProcessing.h:138-157), the one k_fb_check applies to the backward flow, the landing point tested against
// the image and the reverse flow sampled there tested by fb_passes; fp64 without contraction (-ffp-contract=off).  At an
// integer position of finite flows the sampler returns the pixel's value, so a dense track's first step is k_fb_check's test
// on its pixel.
//
// Mapping.  Queries: blockIdx.y is the direction (0 forward from t0, 1 backward), the 256 lanes of a block are 256 consecutive
// queries, so a wave's stores at one frame are contiguous in the point index whenever its queries share t0.  Dense: a block
// is a 64 x 4 tile of frame 0's pixels (as k_fb_check's), forward only; a wave is 64 neighbouring pixels of one row, whose
// taps share cache lines while the flow is smooth, and whose stores are contiguous.  Every offset is 64-bit: N * T passes
// 2^31 for a dense 1080p clip of ~1000 frames.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr int kTrackTX = 64, kTrackTY = 4;      // dense: a 64 x 4 tile of start pixels per block
constexpr int kTrackQ = 256;                    // queries: lanes (queries of one direction) per block
constexpr long long kMaxQueryBlocks = 1LL << 22;  // queries: blocks per launch (2^30 lanes: the x extent stays below 2^32)

struct TrackArgs {
    papof_tensor fw, bw;  // flows (pair, row, column, component); pair t runs from frame t to t + 1
    papof_tensor q;       // queries (point, -, -, {t0, x, y}); unused when dense
    papof_tensor tr;      // float64 tracks (frame, point, -, {x, y})
    papof_tensor vis;     // uint8 visible (frame, point, -, -)
    long long n;          // points
    int T, H, W;
    int check;            // the consistency test is applied
    double a1, a2;
};

__device__ __forceinline__ void put(const TrackArgs& a, long long t, long long n, double x, double y, bool visible) {
    double* tr = static_cast<double*>(a.tr.data) + t * a.tr.stride[0] + n * a.tr.stride[1];
    tr[0] = x;
    tr[a.tr.stride[3]] = y;
    store_u8(a.vis, t * a.vis.stride[0] + n * a.vis.stride[1], visible ? 1 : 0);
}

// blockIdx.y: the direction (queries) or the tile row (dense, from tile row `first`: launches split at gridDim.y's bound);
// blockIdx.x: 256 queries from point `first`, or the tile column.
template <bool DENSE>
__global__ __launch_bounds__(256) void k_track(const TrackArgs a, long long first) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);  // lost or invalid: this NaN, bit for bit
    long long n;
    int dir = 0, s = 0;
    double x, y;
    bool alive;
    if (DENSE) {
        const int px = (int)blockIdx.x * kTrackTX + (int)threadIdx.x;
        const long long r = (first + blockIdx.y) * kTrackTY + threadIdx.y;
        if (px >= a.W || r >= a.H) return;
        n = r * a.W + px;
        x = (double)px;
        y = (double)r;
        alive = true;
    } else {
        n = first + (long long)blockIdx.x * kTrackQ + threadIdx.x;
        if (n >= a.n) return;
        dir = (int)blockIdx.y;
        const long long o = n * a.q.stride[0];
        const double t0 = load_flow(a.q, o);
        x = load_flow(a.q, o + a.q.stride[3]);
        y = load_flow(a.q, o + 2 * a.q.stride[3]);
        // (a NaN or an infinity fails a range test)
        alive = t0 >= 0 && t0 <= (double)(a.T - 1) && t0 == trunc(t0) && x >= 0 && x <= (double)(a.W - 1) && y >= 0 &&
                y <= (double)(a.H - 1);
        s = alive ? (int)t0 : 0;  // an invalid query: its forward lane writes every frame
    }
    if (!alive) x = y = qnan;
    if (dir == 0) put(a, s, n, x, y, alive);  // frame t0, written once
    // sampler.h's direction rule, kept as written: the direction is known only at run time, and the flows are selected
    // once, outside the loop (kernels that deviate)
    const papof_tensor& f = dir ? a.bw : a.fw;  // (dir is uniform over the block)
    const papof_tensor& b = dir ? a.fw : a.bw;
    const int steps = dir ? s : a.T - 1 - s;
    long long t = s;
    for (int k = 0; k < steps; k++) {
        const long long pair = dir ? t - 1 : t;  // backward: t -> t - 1 through flow_bw[t - 1], checked with flow_fw[t - 1]
        if (alive) {
            double X, Y;
            alive = hop(f, b, pair, a.H, a.W, a.check, a.a1, a.a2, x, y, X, Y);
            x = alive ? X : qnan;
            y = alive ? Y : qnan;
        }
        t += dir ? -1 : 1;
        put(a, t, n, x, y, alive);
    }
}

int launch_track(hipStream_t st, const TrackArgs& a, bool dense) {
    if (dense) {
        const long long tx = (a.W + kTrackTX - 1) / kTrackTX, ty = (a.H + kTrackTY - 1) / kTrackTY;
        // (tile columns along gridDim.x, tile rows as grid.h's items along gridDim.y, split at its bound)
        PAPOF_TRY(launch_tiles(tx, ty, [&](dim3 grid, long long, long long y0) {
            hipLaunchKernelGGL(k_track<true>, grid, dim3(kTrackTX, kTrackTY), 0, st, a, y0);
        }));
    } else {
        const long long blocks = (a.n + kTrackQ - 1) / kTrackQ;
        for (long long b0 = 0; b0 < blocks; b0 += kMaxQueryBlocks) {
            const unsigned nb = (unsigned)std::min(kMaxQueryBlocks, blocks - b0);
            hipLaunchKernelGGL(k_track<false>, dim3(nb, 2), dim3(kTrackQ), 0, st, a, b0 * kTrackQ);
            PAPOF_HIP(hipGetLastError());
        }
    }
    return PAPOF_OK;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_track_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* flow_fw,
                                  const papof_tensor* flow_bw, int n_queries, const papof_tensor* queries, int use_check,
                                  double alpha1, double alpha2, const papof_tensor* tracks, const papof_tensor* visible,
                                  void* stream) {
    if (!h || n_frames < 2 || height < 1 || width < 1) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (queries && (n_queries < 1 || !described(queries, kFlowDtypes, {0, 3}, false))) return PAPOF_EINVAL;
    if (!described(tracks, {PAPOF_DTYPE_F64}, {0, 1, 3}, true) || !described(visible, {PAPOF_DTYPE_U8}, {0, 1}, true))
        return PAPOF_EINVAL;
    if (!valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    TrackArgs a{};
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    if (queries) a.q = *queries;
    a.tr = *tracks;
    a.vis = *visible;
    a.n = queries ? (long long)n_queries : (long long)height * width;
    a.T = n_frames;
    a.H = height;
    a.W = width;
    a.check = use_check ? 1 : 0;
    a.a1 = alpha1;
    a.a2 = alpha2;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_track(static_cast<hipStream_t>(stream), a, queries == nullptr);
}
