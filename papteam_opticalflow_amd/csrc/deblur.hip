// papteam_opticalflow_amd/csrc/deblur.hip -- video deblurring: multi-frame Richardson-Lucy along the flows
// (papof_deblur_tensor, papof_deblur_workspace).
//
// Why.  A frame exposed while the camera shakes is the scene averaged along each pixel's path, and the flows give that
// path: shutter * velocity pixels, straight to first order.  Richardson-Lucy (Richardson 1972, Lucy 1974) inverts such a
// blur by repeating "blur the estimate, divide the recorded frame by it, blur the ratio backwards, multiply" -- with a
// line kernel per pixel taken from the flow (Tai, Tan, Brown, PAMI 2011), and over the frames around the target, each
// blurred in its own direction, so that one frame fills the spectral zeros of another (Kim and Lee, CVPR 2015).  Written
// with grid_sample an iteration is one launch and one full-frame temporary per sample, slot and pass; here a lane makes
// one line integral after another with the sums in registers.
//
// Semantics: include/papof.h, papof_deblur_tensor.  The taps, the flow sampler, the hop and the store are sampler.h's;
// fp64 without contraction (-ffp-contract=off), every sum in the stated order: the result is bitwise reproducible and does
// not depend on how the targets are grouped.
//
// Mapping.  A block is a 64 x 4 tile of pixels (the family's): blockIdx.x the tile.  blockIdx.y of k_deblur_ingest and
// k_deblur_update counts the targets of the round, that of k_deblur_ratio the (target, slot) pairs, slot innermost; all of
// them go through launch_tiles.  The sample table travels in the kernel arguments (k_motion_blur's way): it sits in scalar
// registers.  The taps of a sample are computed once and all C channels are accumulated from them (line_sum, used by both
// passes); C is a template argument, so the channel loops are straight code.
//
// Workspace.  One target takes (2 R + 2) planes of H * W * C float64, pixel-major with the channels contiguous -- the C
// values of a tap are one 8 C-byte run --: plane 0 its estimate L, plane 1 + j the ratios of slot j.  The chains are
// recomputed in every pass (at most R hops of 16 flow elements against 16 samples of 4 C taps): nothing else is kept.
// k_deblur_ingest writes L = fmax(frame, 0) once; the update of the last iteration also stores out and support.
// Every offset is 64-bit.  No atomics: every element belongs to one lane.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr int kMaxSamples = 64;
constexpr int kMaxRadius = 4;
constexpr int kMaxIters = 256;
constexpr long long kBudget = 2LL << 30;  // bytes papof_deblur_workspace asks for at most (one target's share if that is more)
constexpr double kEps = 1.0 / 1024.0;     // the floor of the re-blurred estimate

struct DeblurArgs {
    papof_tensor fr;      // the recorded video (frame, row, column, channel)
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy}); pair t runs from frame t to t + 1
    papof_tensor out;     // (frame, row, column, channel)
    papof_tensor sup;     // uint8 support (frame, row, column); data NULL: none
    double* ws;           // [target of the round][plane][pixel][channel]
    long long t0;         // the round's first target
    int T, H, W, R;
    int check;            // the forward-backward test is applied to every hop
    int last;             // k_deblur_update: this is the last iteration (out and support are stored)
    double a1, a2;
    int n;                // samples of the table: those of weight > 0, in the caller's order
    double wsum;          // their weights summed from 0 in that order
    double tau[kMaxSamples], w[kMaxSamples];
};

// slot j of target t is frame t, t + 1, t - 1, t + 2, t - 2, ...
__device__ __forceinline__ long long slot_frame(long long t, int j) { return j & 1 ? t + (j + 1) / 2 : t - j / 2; }

// The chain of the point (X, Y) from frame a to frame b, forward or backward (sampler.h, the direction rule).  False, for
// good, once a hop fails; a == b: the point, alive.
__device__ __forceinline__ bool chain_to(const DeblurArgs& p, long long a, long long b, double& X, double& Y) {
    double nX, nY;
    for (long long f = a; f < b; f++) {
        if (!hop_from(p, f, +1, X, Y, nX, nY)) return false;
        X = nX;
        Y = nY;
    }
    for (long long f = a; f > b; f--) {
        if (!hop_from(p, f, -1, X, Y, nX, nY)) return false;
        X = nX;
        Y = nY;
    }
    return true;
}

// the velocity of frame s from (fu, fv) of flow_fw[s] and (bu, bv) of flow_bw[s - 1] at one point (the side that an end
// frame lacks is not read)
__device__ __forceinline__ void velocity(const DeblurArgs& p, long long s, double fu, double fv, double bu, double bv,
                                         double& vx, double& vy) {
    if (s == 0) {
        vx = fu;
        vy = fv;
    } else if (s == p.T - 1) {
        vx = 0.0 - bu;
        vy = 0.0 - bv;
    } else {
        vx = 0.5 * (fu - bu);
        vy = 0.5 * (fv - bv);
    }
}

// ... at the integer pixel (x, r): the flows' own elements
__device__ __forceinline__ void velocity_at_pixel(const DeblurArgs& p, long long s, int x, long long r, double& vx, double& vy) {
    double fu = 0.0, fv = 0.0, bu = 0.0, bv = 0.0;
    if (s < p.T - 1) {
        const long long o = PAPOF_AT(p.fw, s, r, x);
        fu = load_flow(p.fw, o);
        fv = load_flow(p.fw, o + p.fw.stride[3]);
    }
    if (s > 0) {
        const long long o = PAPOF_AT(p.bw, s - 1, r, x);
        bu = load_flow(p.bw, o);
        bv = load_flow(p.bw, o + p.bw.stride[3]);
    }
    velocity(p, s, fu, fv, bu, bv, vx, vy);
}

// ... at the point (X, Y) of the image: both flows sampled at the point's taps, then combined
__device__ __forceinline__ void velocity_at_point(const DeblurArgs& p, long long s, double X, double Y, double& vx, double& vy) {
    const Bilinear k = taps_at(X, Y, p.H, p.W);
    double fu = 0.0, fv = 0.0, bu = 0.0, bv = 0.0;
    if (s < p.T - 1) sample_flow(p.fw, s * p.fw.stride[0], k, fu, fv);
    if (s > 0) sample_flow(p.bw, (s - 1) * p.bw.stride[0], k, bu, bv);
    velocity(p, s, fu, fv, bu, bv, vx, vy);
}

// The line integral of both passes: acc[ch] = sum over the table, k ascending, of w_k * (img sampled at (clamp(X + sgn tau_k
// vx, 0, W - 1), clamp(Y + sgn tau_k vy, 0, H - 1))), img one plane of the workspace (pixel, channel).  sgn = +-1.0: sgn *
// tau_k is exact, and X + (-tau_k) * vx is X - tau_k * vx bit for bit.  The taps of a sample serve all C channels.
template <int C>
__device__ __forceinline__ void line_sum(const DeblurArgs& p, const double* img, double X, double Y, double vx, double vy,
                                         double sgn, double* acc) {
#pragma unroll
    for (int ch = 0; ch < C; ch++) acc[ch] = 0.0;
    const double xmax = (double)(p.W - 1), ymax = (double)(p.H - 1);
    for (int k = 0; k < p.n; k++) {
        const double tk = sgn * p.tau[k], wk = p.w[k];
        const double Xs = fmin(fmax(X + tk * vx, 0.0), xmax), Ys = fmin(fmax(Y + tk * vy, 0.0), ymax);
        const Bilinear b = taps_at(Xs, Ys, p.H, p.W);
        double g[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) g[ch] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double* q = img + ((long long)b.row[i] * p.W + b.col[i]) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) g[ch] += q[ch] * b.w[i];
        }
#pragma unroll
        for (int ch = 0; ch < C; ch++) acc[ch] = acc[ch] + wk * g[ch];
    }
}

// the pixel (x, r) of this lane; false: outside the frame
__device__ __forceinline__ bool tile_pixel(const DeblurArgs& p, long long tile0, int& x, long long& r) {
    PAPOF_TILE_PIXEL(InterpTile, tile0, p.W, int, px, long long, pr);
    x = px;
    r = pr;
    return x < p.W && r < p.H;
}

// L of target t0 + g = fmax(frame, 0).  blockIdx.y: target g0 + y of the round.
template <int FD, int C>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_deblur_ingest(const DeblurArgs p, long long tile0, long long g0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    int x;
    long long r;
    if (!tile_pixel(p, tile0, x, r)) return;
    const long long g = g0 + blockIdx.y, plane = (long long)p.H * p.W * C;
    double* L = p.ws + g * (2 * p.R + 2) * plane + (r * p.W + x) * C;
    const long long pix = PAPOF_AT(p.fr, p.t0 + g, r, x);
#pragma unroll
    for (int ch = 0; ch < C; ch++) L[ch] = fmax(load_frame<FD>(p.fr, pix + ch * p.fr.stride[3], lut), 0.0);
}

// Pass A.  blockIdx.y: (target, slot) pair i0 + y of the round, slot innermost; the lane is pixel q of the slot's frame.
template <int FD, int C>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_deblur_ratio(const DeblurArgs p, long long tile0, long long i0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    const int slots = 2 * p.R + 1;
    const long long i = i0 + blockIdx.y, g = i / slots, t = p.t0 + g;
    const int j = (int)(i % slots);
    const long long s = slot_frame(t, j);
    if (s < 0 || s >= p.T) return;  // (the whole block: an absent slot)
    int x;
    long long r;
    if (!tile_pixel(p, tile0, x, r)) return;
    const long long plane = (long long)p.H * p.W * C;
    double* const base = p.ws + g * (2 * p.R + 2) * plane;
    double* ratio = base + (1 + j) * plane + (r * p.W + x) * C;
    double X = (double)x, Y = (double)r, vx, vy;
    const bool alive = chain_to(p, s, t, X, Y);
    velocity_at_pixel(p, s, x, r, vx, vy);
    if (!alive || !isfinite(vx) || !isfinite(vy)) {
#pragma unroll
        for (int ch = 0; ch < C; ch++) ratio[ch] = 1.0;
        return;
    }
    double est[C];
    line_sum<C>(p, base, X, Y, vx, vy, 1.0, est);
    const long long pix = PAPOF_AT(p.fr, s, r, x);
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
        const double b = fmax(load_frame<FD>(p.fr, pix + ch * p.fr.stride[3], lut), 0.0);
        ratio[ch] = b / fmax(est[ch] / p.wsum, kEps);
    }
}

// Pass B.  blockIdx.y: target g0 + y of the round; the lane is pixel p of the target.
template <int C>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_deblur_update(const DeblurArgs p, long long tile0, long long g0) {
    int x;
    long long r;
    if (!tile_pixel(p, tile0, x, r)) return;
    const long long g = g0 + blockIdx.y, t = p.t0 + g, plane = (long long)p.H * p.W * C;
    double* const base = p.ws + g * (2 * p.R + 2) * plane;
    double corr[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) corr[ch] = 0.0;
    int n = 0;
    for (int j = 0; j < 2 * p.R + 1; j++) {
        const long long s = slot_frame(t, j);
        if (s < 0 || s >= p.T) continue;
        double X = (double)x, Y = (double)r, vx, vy;
        if (!chain_to(p, t, s, X, Y)) continue;
        velocity_at_point(p, s, X, Y, vx, vy);
        if (!isfinite(vx) || !isfinite(vy)) continue;
        double cs[C];
        line_sum<C>(p, base + (1 + j) * plane, X, Y, vx, vy, -1.0, cs);
#pragma unroll
        for (int ch = 0; ch < C; ch++) corr[ch] += cs[ch] / p.wsum;
        n += 1;
    }
    double* L = base + (r * p.W + x) * C;
    const long long o = PAPOF_AT(p.out, t, r, x);
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
        double v = L[ch];
        if (n > 0) v = v * (corr[ch] / (double)n);
        if (p.last)
            store(p.out, o + ch * p.out.stride[3], v);
        else
            L[ch] = v;
    }
    if (p.last && p.sup.data)
        store_u8(p.sup, PAPOF_AT(p.sup, t, r, x), (unsigned char)n);
}

// bytes of one target's share of the workspace; < 0: refused
long long per_target_bytes(long long n_frames, long long h, long long w, long long c, long long radius) {
    if (n_frames < 2 || h < 1 || w < 1 || c < 1 || c > kMaxChannels || radius < 0 || radius > kMaxRadius) return -1;
    if (h >= (1LL << 30) || w >= (1LL << 30) || h * w >= (1LL << 30)) return -1;
    return 8 * c * h * w * (2 * radius + 2);
}

template <int FD, int C>
int run_deblur(hipStream_t st, DeblurArgs p, int iters, long long G) {
    for (long long t0 = 0; t0 < p.T; t0 += G) {
        const long long n = std::min<long long>(p.T - t0, G);
        p.t0 = t0;
        PAPOF_TRY(launch_grid<InterpTile>(p.H, p.W, n, st, 0, k_deblur_ingest<FD, C>, p));
        for (int it = 0; it < iters; it++) {
            p.last = it == iters - 1;
            PAPOF_TRY(launch_grid<InterpTile>(p.H, p.W, n * (2 * p.R + 1), st, 0, k_deblur_ratio<FD, C>, p));
            PAPOF_TRY(launch_grid<InterpTile>(p.H, p.W, n, st, 0, k_deblur_update<C>, p));
        }
    }
    return PAPOF_OK;
}

template <int FD>
int run_deblur_of(hipStream_t st, const DeblurArgs& p, int c, int iters, long long G) {
    return c == 1   ? run_deblur<FD, 1>(st, p, iters, G)
           : c == 2 ? run_deblur<FD, 2>(st, p, iters, G)
           : c == 3 ? run_deblur<FD, 3>(st, p, iters, G)
                    : run_deblur<FD, 4>(st, p, iters, G);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_deblur_workspace(int n_frames, int height, int width, int c, int radius) {
    const long long per = per_target_bytes(n_frames, height, width, c, radius);
    if (per < 0) return -1;
    return std::min<long long>(n_frames, std::max(1LL, kBudget / per)) * per;
}

extern "C" int papof_deblur_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                   const papof_tensor* flow_fw, const papof_tensor* flow_bw, int n_samples,
                                   const double* offsets, const double* weights, int radius, int iters, int use_check,
                                   double alpha1, double alpha2, const papof_tensor* out, const papof_tensor* support,
                                   void* workspace, long long workspace_bytes, void* stream) {
    if (!h) return PAPOF_EINVAL;
    const long long per = per_target_bytes(n_frames, height, width, c, radius);
    if (per < 0 || iters < 1 || iters > kMaxIters || !valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (!opt_out_mask(support)) return PAPOF_EINVAL;
    if (n_samples < 1 || n_samples > kMaxSamples || !offsets || !weights) return PAPOF_EINVAL;
    const double lo = std::ldexp(1.0, -20), hi = 1.0 - lo;
    DeblurArgs p{};
    for (int k = 0; k < n_samples; k++) {
        const double tau = offsets[k], w = weights[k];
        if (!(tau == 0.0 || (std::fabs(tau) >= lo && std::fabs(tau) <= hi))) return PAPOF_EINVAL;  // (a NaN fails both)
        if (!std::isfinite(w) || w < 0.0) return PAPOF_EINVAL;
        if (w > 0.0) {
            p.tau[p.n] = tau;
            p.w[p.n++] = w;
            p.wsum = p.wsum + w;
        }
    }
    if (!(p.wsum > 0.0) || !std::isfinite(p.wsum)) return PAPOF_EINVAL;
    if (!workspace || workspace_bytes < per) return PAPOF_EINVAL;
    p.fr = *frames;
    p.fw = *flow_fw;
    p.bw = *flow_bw;
    p.out = *out;
    if (support) p.sup = *support;
    p.ws = static_cast<double*>(workspace);
    p.T = n_frames;
    p.H = height;
    p.W = width;
    p.R = radius;
    p.check = use_check ? 1 : 0;
    p.a1 = alpha1;
    p.a2 = alpha2;
    const long long G = std::min<long long>(n_frames, workspace_bytes / per);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PAPOF_HIP(hipSetDevice(h->device));
    return frames->dtype == PAPOF_DTYPE_U8    ? run_deblur_of<PAPOF_DTYPE_U8>(st, p, c, iters, G)
           : frames->dtype == PAPOF_DTYPE_F32 ? run_deblur_of<PAPOF_DTYPE_F32>(st, p, c, iters, G)
                                              : run_deblur_of<PAPOF_DTYPE_F64>(st, p, c, iters, G);
}
