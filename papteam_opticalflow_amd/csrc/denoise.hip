// papteam_opticalflow_amd/csrc/denoise.hip -- motion-compensated temporal denoising (papof_temporal_filter_tensor).
//
// Why.  The classic use of dense, consistency-checked flow (Liu and Freeman, "A high-quality video denoising algorithm based
// on reliable motion estimation", ECCV 2010; MCTF, the pre-filter of video encoders): each pixel of frame t is averaged with
// the points it maps to in frames t +- 1 .. t +- R, and a sample whose motion cannot be trusted is dropped or down-weighted.
// Written with grid_sample it is a handful of launches per frame and neighbour and a full-frame temporary per neighbour
// through HBM.  Here one lane makes one output pixel: it follows the pixel's chain through the flows with its position, the
// C centre values and the C running sums in registers, and writes each output element once.
//
// Semantics: include/papof.h, papof_temporal_filter_tensor.  A hop is sampler.h's, k_track's step: the flow sampled where the
// chain is, the new position tested against the image, the reverse flow sampled there and the consistency test; a chain that
// dies stays dead.  The samplers are sampler.h's (sample_flow, sample_frame), fp64 without contraction (-ffp-contract=off).  All forward samples are summed first, then all backward ones, in order of distance: the
// result is bitwise reproducible.
//
// Mapping.  A block is a 64 x 4 tile of output pixels (as k_interp's and k_fb_check's): blockIdx.x the tile, blockIdx.y the
// frame.  A wave is 64 neighbouring pixels of one row, whose taps share cache lines while the flow is smooth and whose
// stores are contiguous along a row.  No atomics, no workspace: every output element belongs to one lane.  Every offset is
// 64-bit.
#include "sampler.h"

#include <cmath>

namespace papof {

namespace {

constexpr int kFilterTX = 64, kFilterTY = 4;   // a 64 x 4 tile of output pixels per block (256 lanes: lut)
using FilterTile = Tile<kFilterTX, kFilterTY>;
constexpr int kMaxRadius = 16;

struct FilterArgs {
    papof_tensor fr;      // frames (frame, row, column, channel)
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy}); pair t runs from frame t to t + 1
    papof_tensor out;     // (frame, row, column, channel)
    papof_tensor sup;     // uint8 support (frame, row, column); data NULL: none
    int T, H, W, C, R;
    int check;            // the consistency test is applied
    double sigma, s2;     // sigma > 0: the photometric weight 1 / (1 + D / s2), s2 = sigma * sigma
    double a1, a2;
};

// The samples of one direction (dir = +-1: sampler.h, the direction rule) of frame t's pixel (x, r), added to num / den /
// support.
template <int FD>
__device__ __forceinline__ void chain(const FilterArgs& a, long long t, int dir, int steps, double X, double Y,
                                      const double* c, double* num, double& den, int& support, const double* lut) {
    const int H = a.H, W = a.W;
    for (int j = 1; j <= steps; j++) {
        const long long pair = chain_pair(t, dir, j), frame = chain_frame(t, dir, j);
        double nX, nY;
        if (!chain_hop(a, pair, dir, H, W, X, Y, nX, nY)) return;  // once dead, the chain stays dead
        X = nX;
        Y = nY;
        const Bilinear k = taps_at(X, Y, H, W);
        const long long base = frame * a.fr.stride[0];
        double g[kMaxChannels], D = 0.0;
#pragma unroll
        for (int ch = 0; ch < kMaxChannels; ch++)
            if (ch < a.C) {
                g[ch] = sample_frame<FD>(a.fr, base + ch * a.fr.stride[3], k, lut);
                const double d = g[ch] - c[ch];
                D += d * d;
            }
        const double w = a.sigma > 0 ? photometric_weight(D, a.C, a.s2) : 1.0;
        if (w > 0) {  // (false for a NaN)
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ch++)
                if (ch < a.C) num[ch] += w * g[ch];
            den += w;
            support += 1;
        }
    }
}

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y.
template <int FD>
__global__ __launch_bounds__(kFilterTX* kFilterTY) void k_temporal_filter(const FilterArgs a, long long tile0,
                                                                          long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kFilterTX>(lut);
    PAPOF_TILE_PIXEL(FilterTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    const long long pix = PAPOF_AT(a.fr, t, r, x);
    double c[kMaxChannels], num[kMaxChannels];
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < a.C) num[ch] = c[ch] = load_frame<FD>(a.fr, pix + ch * a.fr.stride[3], lut);
    double den = 1.0;
    int support = 0;
    const int fwd = chain_steps(a.T, t, +1, a.R), bwd = chain_steps(a.T, t, -1, a.R);
    chain<FD>(a, t, +1, fwd, (double)x, (double)r, c, num, den, support, lut);
    chain<FD>(a, t, -1, bwd, (double)x, (double)r, c, num, den, support, lut);
    const long long o = PAPOF_AT(a.out, t, r, x);
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < a.C) store(a.out, o + ch * a.out.stride[3], num[ch] / den);
    if (a.sup.data) store_u8(a.sup, PAPOF_AT(a.sup, t, r, x), (unsigned char)support);
}

int launch_filter(hipStream_t st, const FilterArgs& a) {
    const auto kernel = by_dtype(a.fr.dtype, [](auto fd) { return k_temporal_filter<fd()>; });
    return launch_grid<FilterTile>(a.H, a.W, a.T, st, 0, kernel, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_temporal_filter_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                            const papof_tensor* frames, const papof_tensor* flow_fw,
                                            const papof_tensor* flow_bw, int radius, double sigma, int use_check,
                                            double alpha1, double alpha2, const papof_tensor* out,
                                            const papof_tensor* support, void* stream) {
    if (!h || n_frames < 2 || height < 1 || width < 1 || c < 1 || c > kMaxChannels) return PAPOF_EINVAL;
    if (radius < 1 || radius > kMaxRadius || !std::isfinite(sigma) || sigma < 0) return PAPOF_EINVAL;
    if (!valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    if (!in_frames(frames)) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (!out_frames(out)) return PAPOF_EINVAL;
    if (!opt_out_mask(support)) return PAPOF_EINVAL;
    FilterArgs a{};
    a.fr = *frames;
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    a.out = *out;
    if (support) a.sup = *support;
    a.T = n_frames;
    a.H = height;
    a.W = width;
    a.C = c;
    a.R = radius;
    a.check = use_check ? 1 : 0;
    a.sigma = sigma;
    a.s2 = sigma * sigma;
    a.a1 = alpha1;
    a.a2 = alpha2;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_filter(static_cast<hipStream_t>(stream), a);
}
