// papteam_opticalflow_amd/csrc/superres.hip -- multi-frame super-resolution along the flows (papof_super_resolve_tensor).
//
// Why.  Neighbouring frames of a video sample the scene at different sub-pixel phases.  Carried to one frame along the flows
// and placed on a finer grid they hold detail that no upsampling of a single frame recovers (shift and add: Farsiu,
// Robinson, Elad, Milanfar 2004; back-projection: Irani and Peleg 1991).  The operator is a SCATTER onto a finer grid
// through CHAINS of flows: k_splat scatters one hop onto the source's own grid, k_temporal_filter follows chains but
// gathers, and a gather smears every sample over a low-resolution pixel.
//
// Semantics: include/papof.h, papof_super_resolve_tensor.  The hop is sampler.h's (k_temporal_filter's, k_track's), the
// deposit k_splat's tap rule with bound 1 on the fine grid: 64-bit fixed-point integer sums, so the order in which the
// atomic adds arrive cannot change a bit.  fp64 without contraction (-ffp-contract=off) everywhere else.
//
// Mapping.
// k_sr_accumulate: a block is a 64 x 4 tile of SOURCE pixels (k_interp's tile), blockIdx.y the source frame.  A lane keeps
//   its C values and its position in registers and walks both chains once; one chain serves every target frame it passes.
//   The accumulator is planar, int64 [target][C + 1][S H][S W] with den's plane last (planar is 2.8 x faster
//   than interleaved); the adds are sampler.h's add64.  A wave's 64 lanes land S fine pixels apart, so the lanes exchange
//   their terms before they add (deposit): one wave-instruction then covers a contiguous run of the fine row at S = 2.
// k_sr_resolve: one lane per FINE pixel: the cubic base of the target frame, the division, coverage; X goes to the
//   workspace (fp64 planar [target][C][S H][S W]) or, without back-projection, to the typed output.
// k_sr_backproject: a block is a 16 x 8 tile of LOW-resolution pixels and the 16 S x 8 S fine pixels under it.  Per
//   channel it stages X of the tile and of a halo of one low-resolution pixel in LDS, forms the residuals of the
//   (16 + 2) x (8 + 2) low-resolution pixels in LDS and updates its fine pixels.  A residual is the same expression in every
//   block that forms it, so the bits do not depend on the tiling.  Jacobi: reads one X buffer, writes the other (or the typed
//   output in the last step).
// Every offset is 64-bit.  Nothing of the handle's arena is used; nothing waits on the host.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr double kFix = 4294967296.0;         // 2^32: the fixed point's scale
constexpr int kMinScale = 2, kMaxScale = 4;
constexpr long long kBudget = 1LL << 31;      // papof_sr_workspace: as many target frames as fit 2 GiB
constexpr int kBpX = 16, kBpY = 8;            // k_sr_backproject: the block's tile of low-resolution pixels
using LowTile = Tile<kBpX, kBpY, 256, 1>;     // ... under a row of 256 lanes

struct SrArgs {
    papof_tensor fr;          // frames (frame, row, column, channel)
    papof_tensor fw, bw;      // flows (pair, row, column, {vx, vy}); pair t runs from frame t to t + 1
    unsigned long long* acc;  // [target - t0][C + 1][S H][S W], den's plane last
    long long t0, t1;         // the targets of this round
    int T, H, W, C, R, S;
    int check, weighted;
    double s2, a1, a2;
};

// The deposit of (w, val[0 .. C)) at the low-resolution point (PX, PY) of target frame `target` (inside [t0, t1)), by ALL 64
// lanes of a wave at once; a lane that has nothing to deposit comes with w = 0 and any point of the image.
// A lane's two taps of a fine row are neighbours, x0 and x0 + 1, and its neighbour lane's lie S pixels further: issued lane
// by lane, one atomic wave-instruction touches every S-th int64 of a row, and a 64-byte request at the memory side carries
// 8 / S adds.  So the wave exchanges its terms first: lane j issues tap (j & 1) of lane (j >> 1) (then of lane 32 + (j >> 1)),
// and one wave-instruction covers the taps of 32 neighbouring source pixels, 2 of every S int64 (all of them at S = 2).
// Every (address, term) pair is still added exactly once, a term of 0 is not added (the sum is the same), and the sums
// are integers: the bits do not depend on who issues what.
__device__ __forceinline__ void deposit(const SrArgs& a, long long target, double PX, double PY, double w, const double* val) {
    const double S = (double)a.S;
    const double QX = S * (PX + 0.5) - 0.5, QY = S * (PY + 0.5) - 0.5;
    const long long FW = (long long)a.S * a.W, FH = (long long)a.S * a.H, plane = FW * FH;
    const double fx0 = floor(QX), fy0 = floor(QY);
    const long long x0 = (long long)fx0, y0 = (long long)fy0;
    const double fx = QX - fx0, fy = QY - fy0;
    unsigned long long* const at = a.acc + (target - a.t0) * (a.C + 1) * plane;
    double wb[4];
#pragma unroll
    for (int m = 0; m <= 1; m++)
#pragma unroll
        for (int n = 0; n <= 1; n++) {
            const long long tx = x0 + n, ty = y0 + m;
            const bool inside = tx >= 0 && tx < FW && ty >= 0 && ty < FH;
            const double b = (m ? fy : 1.0 - fy) * (n ? fx : 1.0 - fx);
            wb[2 * m + n] = inside ? w * b : 0.0;  // (a tap whose wb is 0 is dropped: its terms are 0)
        }
    const int lane = (int)threadIdx.x, sel = lane & 1;
    long long off[2][2];  // [m][half]: the fine pixel of the tap this lane issues
#pragma unroll
    for (int m = 0; m <= 1; m++)
#pragma unroll
        for (int h = 0; h <= 1; h++) off[m][h] = __shfl((y0 + m) * FW + x0, 32 * h + (lane >> 1)) + sel;
#pragma unroll
    for (int p = 0; p <= kMaxChannels; p++) {  // p = 0: den's plane (the last one), then the channels
        if (p > a.C) break;
        unsigned long long* const q = at + (p ? p - 1 : a.C) * plane;
        long long term[4];
#pragma unroll
        for (int k = 0; k < 4; k++) term[k] = (long long)rint((p ? wb[k] * val[p - 1] : wb[k]) * kFix);
#pragma unroll
        for (int m = 0; m <= 1; m++)
#pragma unroll
            for (int h = 0; h <= 1; h++) {
                const int src = 32 * h + (lane >> 1);
                const long long t0 = __shfl(term[2 * m], src), t1 = __shfl(term[2 * m + 1], src);
                const long long t = sel ? t1 : t0;
                if (t != 0) add64(q + off[m][h], t);
            }
    }
}

// One direction (dir = +-1: sampler.h, the direction rule) of source frame k's pixel.  The chain stops at the first target
// beyond this round's [t0, t1): what it would do there belongs to another round.  The loop is the WAVE's (deposit exchanges
// terms between the lanes): a lane whose chain is dead stays in it with weight 0, and the wave leaves once none of its
// chains is alive.
template <int FD>
__device__ __forceinline__ void walk(const SrArgs& a, long long k, int dir, int steps, bool alive, double X, double Y,
                                     const double* v, const double* val, const double* lut) {
    const int H = a.H, W = a.W;
    for (int n = 1; n <= steps; n++) {
        const long long pair = chain_pair(k, dir, n), target = chain_frame(k, dir, n);
        if (dir > 0 ? target >= a.t1 : target < a.t0) return;
        double nX, nY;
        alive = alive && chain_hop(a, pair, dir, H, W, X, Y, nX, nY);  // once dead, the chain stays dead
        if (__ballot(alive) == 0) return;
        X = alive ? nX : 0.0;
        Y = alive ? nY : 0.0;
        if (target < a.t0 || target >= a.t1) continue;
        double w = 0.0;
        if (alive) {
            const Bilinear t = taps_at(X, Y, H, W);
            const long long base = target * a.fr.stride[0];
            double D = 0.0;
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ch++)
                if (ch < a.C) {
                    const double d = v[ch] - sample_frame<FD>(a.fr, base + ch * a.fr.stride[3], t, lut);
                    D += d * d;
                }
            w = a.weighted ? photometric_weight(D, a.C, a.s2) : 1.0;
            w = w > 0 ? w : 0.0;  // (0 for a NaN: nothing is deposited)
        }
        deposit(a, target, X, Y, w, val);
    }
}

// grid.h's grid over the frame's 64 x 4 tiles of source pixels; blockIdx.y: source frame
// `frame0` + y.  A wave is one row of 64 source pixels.
template <int FD>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_sr_accumulate(const SrArgs a, long long tile0, long long frame0) {
    static_assert(kInterpTX == 64, "deposit: a wave is a row of the tile");
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    PAPOF_TILE_PIXEL(InterpTile, tile0, a.W, int, x, long long, r);
    if (r >= a.H) return;  // (the whole wave)
    const bool valid = x < a.W;
    const long long k = frame0 + blockIdx.y;
    const long long pix = PAPOF_AT(a.fr, k, r, x);
    double v[kMaxChannels], val[kMaxChannels];
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < a.C) {
            v[ch] = valid ? load_frame<FD>(a.fr, pix + ch * a.fr.stride[3], lut) : 0.0;
            val[ch] = fmin(fmax(v[ch], -1.0), 1.0);  // k_splat's clamp with bound 1: no sum can overflow
        }
    const double X = valid ? (double)x : 0.0, Y = (double)r;
    if (k >= a.t0 && k < a.t1) deposit(a, k, X, Y, valid ? 1.0 : 0.0, val);
    const int fwd = chain_steps(a.T, k, +1, a.R), bwd = chain_steps(a.T, k, -1, a.R);
    walk<FD>(a, k, +1, fwd, valid, X, Y, v, val, lut);
    walk<FD>(a, k, -1, bwd, valid, X, Y, v, val, lut);
}

// The four weights of the cubic convolution kernel (Keys 1981, a = -0.5) for the taps at -1, 0, 1, 2 around a point at
// fraction t of the way from tap 0 to tap 1.
__device__ __forceinline__ void cubic_weights(double t, double* w) {
    w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    w[1] = (1.5 * t - 2.5) * t * t + 1.0;
    w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    w[3] = (0.5 * t - 0.5) * t * t;
}

struct SrResolveArgs {
    papof_tensor fr;       // frames
    const long long* acc;  // k_sr_accumulate's
    double* X;             // [target - t0][C][S H][S W]; NULL: the typed store to out
    papof_tensor out;      // (frame, row, column, channel) of the fine grid
    papof_tensor cov;      // float64 (frame, row, column) of the fine grid; data NULL: not wanted
    long long t0;
    int H, W, C, S;
    double prior;
};

// grid.h's grid over the 64 x 4 tiles of FINE pixels; blockIdx.y: target t0 + `frame0` + y.
template <int FD>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_sr_resolve(const SrResolveArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    const long long FW = (long long)a.S * a.W, FH = (long long)a.S * a.H, plane = FW * FH;
    PAPOF_TILE_PIXEL(InterpTile, tile0, FW, long long, x, long long, r);
    if (x >= FW || r >= FH) return;
    const long long g = frame0 + blockIdx.y, t = a.t0 + g;
    const double S = (double)a.S;
    const double px = ((double)x + 0.5) / S - 0.5, py = ((double)r + 0.5) / S - 0.5;
    const double fx0 = floor(px), fy0 = floor(py);
    double wx[4], wy[4];
    cubic_weights(px - fx0, wx);
    cubic_weights(py - fy0, wy);
    long long rows[4], cols[4];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        rows[n] = clamp_to((int)fy0 - 1 + n, a.H) * a.fr.stride[1];
        cols[n] = clamp_to((int)fx0 - 1 + n, a.W) * a.fr.stride[2];
    }
    const long long* p = a.acc + g * (a.C + 1) * plane + r * FW + x;
    const double coverage = (double)p[a.C * plane] * (1.0 / kFix);
    if (a.cov.data)
        static_cast<double*>(a.cov.data)[PAPOF_AT(a.cov, t, r, x)] = coverage;
    const long long o = PAPOF_AT(a.out, t, r, x);
    for (int ch = 0; ch < a.C; ch++) {
        const long long base = t * a.fr.stride[0] + ch * a.fr.stride[3];
        double b = 0.0;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            double row = 0.0;
#pragma unroll
            for (int n = 0; n < 4; n++) row += wx[n] * load_frame<FD>(a.fr, base + rows[m] + cols[n], lut);
            b += wy[m] * row;
        }
        const double X = ((double)p[ch * plane] * (1.0 / kFix) + a.prior * b) / (coverage + a.prior);
        if (a.X)
            a.X[(g * a.C + ch) * plane + r * FW + x] = X;
        else
            store(a.out, o + ch * a.out.stride[3], X);
    }
}

struct SrBackArgs {
    papof_tensor fr;   // frames
    const double* Xin;  // [target - t0][C][S H][S W]
    double* Xout;      // the other buffer; NULL: the typed store to out (the last step)
    papof_tensor out;
    long long t0;
    int H, W, C, S;
};

// grid.h's grid over the kBpX x kBpY tiles of LOW-resolution pixels; blockIdx.y: target t0 + `frame0` + y.
template <int FD>
__global__ __launch_bounds__(256) void k_sr_backproject(const SrBackArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    __shared__ double xs[(kBpY + 2) * kMaxScale * (kBpX + 2) * kMaxScale];  // X of the tile and its halo
    __shared__ double res[(kBpY + 2) * (kBpX + 2)];                          // their residuals
    const int tid = threadIdx.x, S = a.S;
    if (FD == PAPOF_DTYPE_U8) fill_u8_lut(lut, tid);  // (the first barrier of the channel loop orders it)
    const long long FW = (long long)S * a.W, FH = (long long)S * a.H, plane = FW * FH;
    PAPOF_TILE_ORIGIN(LowTile, tile0, a.W, long long, lx0, long long, ly0);  // the tile's first low-resolution pixel
    const long long hx0 = lx0 - 1, hy0 = ly0 - 1;                       // the halo's
    const int sw = (kBpX + 2) * S, sh = (kBpY + 2) * S;                 // the staged fine pixels
    const long long g = frame0 + blockIdx.y, t = a.t0 + g;
    const double dS = (double)S, n2 = (double)(S * S);
    for (int ch = 0; ch < a.C; ch++) {
        const double* Xc = a.Xin + (g * a.C + ch) * plane;
        __syncthreads();  // the previous channel's reads of xs and res are done
        for (int i = tid; i < sw * sh; i += 256) {
            const long long gy = hy0 * S + i / sw, gx = hx0 * S + i % sw;
            if (gx >= 0 && gx < FW && gy >= 0 && gy < FH) xs[i] = Xc[gy * FW + gx];
        }
        __syncthreads();
        for (int i = tid; i < (kBpX + 2) * (kBpY + 2); i += 256) {
            const int hy = i / (kBpX + 2), hx = i % (kBpX + 2);
            const long long ly = hy0 + hy, lx = hx0 + hx;
            if (lx >= 0 && lx < a.W && ly >= 0 && ly < a.H) {
                double sum = 0.0;
                for (int m = 0; m < S; m++)
                    for (int n = 0; n < S; n++) sum += xs[(hy * S + m) * sw + hx * S + n];
                const double y = load_frame<FD>(a.fr, PAPOF_AT_CH(a.fr, t, ly, lx, ch), lut);
                res[i] = y - sum / n2;
            }
        }
        __syncthreads();
        for (int i = tid; i < kBpX * S * kBpY * S; i += 256) {
            const int fyl = i / (kBpX * S), fxl = i % (kBpX * S);
            const long long gy = ly0 * S + fyl, gx = lx0 * S + fxl;
            if (gx >= FW || gy >= FH) continue;
            const double px = ((double)gx + 0.5) / dS - 0.5, py = ((double)gy + 0.5) / dS - 0.5;
            const double fx0 = floor(px), fy0 = floor(py);
            const double fx = px - fx0, fy = py - fy0;
            const int x0 = clamp_to((int)fx0, a.W) - (int)hx0, x1 = clamp_to((int)fx0 + 1, a.W) - (int)hx0;
            const int y0 = clamp_to((int)fy0, a.H) - (int)hy0, y1 = clamp_to((int)fy0 + 1, a.H) - (int)hy0;
            const double top = (1.0 - fx) * res[y0 * (kBpX + 2) + x0] + fx * res[y0 * (kBpX + 2) + x1];
            const double bot = (1.0 - fx) * res[y1 * (kBpX + 2) + x0] + fx * res[y1 * (kBpX + 2) + x1];
            const double X = xs[(fyl + S) * sw + fxl + S] + ((1.0 - fy) * top + fy * bot);
            if (a.Xout)
                a.Xout[(g * a.C + ch) * plane + gy * FW + gx] = X;
            else
                store(a.out, PAPOF_AT_CH(a.out, t, gy, gx, ch), X);
        }
    }
}

// bytes of one target frame's share of the workspace; < 0: refused
long long per_target_bytes(long long n_frames, long long h, long long w, long long c, long long scale, long long iters) {
    if (n_frames < 1 || h < 1 || w < 1 || c < 1 || c > kMaxChannels || scale < kMinScale || scale > kMaxScale || iters < 0 || iters > 65536)
        return -1;
    if (h >= (1LL << 30) || w >= (1LL << 30) || h * w >= (1LL << 30)) return -1;
    return 8 * scale * scale * h * w * ((c + 1) + (iters > 0 ? 2 * c : 0));
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_sr_workspace(int n_frames, int height, int width, int c, int scale, int iters) {
    const long long per = per_target_bytes(n_frames, height, width, c, scale, iters);
    if (per < 0) return -1;
    return std::min<long long>(n_frames, std::max(1LL, kBudget / per)) * per;
}

extern "C" int papof_super_resolve_tensor(papof_handle* h, int n_frames, int height, int width, int c, int scale,
                                          const papof_tensor* frames, const papof_tensor* flow_fw,
                                          const papof_tensor* flow_bw, int radius, int use_sigma, double sigma, int use_check,
                                          double alpha1, double alpha2, double prior, int iters, const papof_tensor* out,
                                          const papof_tensor* coverage, void* workspace, long long workspace_bytes,
                                          void* stream) {
    if (!h) return PAPOF_EINVAL;
    const long long per = per_target_bytes(n_frames, height, width, c, scale, iters);
    if (per < 0 || radius < 0) return PAPOF_EINVAL;
    if ((2LL * radius + 1) * height * width >= (1LL << 30)) return PAPOF_EINVAL;
    if (!std::isfinite(sigma) || sigma < 0 || !valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    if (!std::isfinite(prior) || prior < 1.0 / 16777216.0) return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (n_frames > 1 && radius > 0 && !in_flow_pair(flow_fw, flow_bw))  // (no flow is read otherwise: they may be NULL)
        return PAPOF_EINVAL;
    if (coverage && !described(coverage, {PAPOF_DTYPE_F64}, {0, 1, 2}, true)) return PAPOF_EINVAL;
    if (!workspace || workspace_bytes < per) return PAPOF_EINVAL;
    const long long G = std::min<long long>(n_frames, workspace_bytes / per);
    const long long FW = (long long)scale * width, FH = (long long)scale * height, plane = FW * FH;
    hipStream_t st = static_cast<hipStream_t>(stream);

    SrArgs a{};
    a.fr = *frames;
    if (n_frames > 1 && radius > 0) {
        a.fw = *flow_fw;
        a.bw = *flow_bw;
    }
    a.acc = static_cast<unsigned long long*>(workspace);
    a.T = n_frames;
    a.H = height;
    a.W = width;
    a.C = c;
    a.R = radius;
    a.S = scale;
    a.check = use_check ? 1 : 0;
    a.weighted = use_sigma && sigma > 0 ? 1 : 0;
    a.s2 = sigma * sigma;
    a.a1 = alpha1;
    a.a2 = alpha2;
    double* const X0 = reinterpret_cast<double*>(static_cast<char*>(workspace) + G * 8 * (c + 1) * plane);
    double* const X1 = X0 + G * c * plane;
    SrResolveArgs q{};
    q.fr = *frames;
    q.acc = static_cast<const long long*>(workspace);
    q.X = iters > 0 ? X0 : nullptr;
    q.out = *out;
    if (coverage) q.cov = *coverage;
    q.H = height;
    q.W = width;
    q.C = c;
    q.S = scale;
    q.prior = prior;
    SrBackArgs p{};
    p.fr = *frames;
    p.out = *out;
    p.H = height;
    p.W = width;
    p.C = c;
    p.S = scale;

    const int fd = frames->dtype;
    const auto k_acc = by_dtype(fd, [](auto fd) { return k_sr_accumulate<fd()>; });
    const auto k_res = by_dtype(fd, [](auto fd) { return k_sr_resolve<fd()>; });
    const auto k_back = by_dtype(fd, [](auto fd) { return k_sr_backproject<fd()>; });
    PAPOF_HIP(hipSetDevice(h->device));
    for (long long t0 = 0; t0 < n_frames; t0 += G) {
        const long long t1 = std::min<long long>(n_frames, t0 + G), n = t1 - t0;
        const long long s0 = std::max<long long>(0, t0 - radius), s1 = std::min<long long>(n_frames, t1 + radius);
        a.t0 = q.t0 = p.t0 = t0;
        a.t1 = t1;
        PAPOF_HIP(hipMemsetAsync(workspace, 0, (size_t)(n * 8 * (c + 1) * plane), st));
        PAPOF_TRY(launch_tiles(InterpTile::count(height, width), s1 - s0, [&](dim3 grid, long long tile0, long long f0) {
            hipLaunchKernelGGL(k_acc, grid, InterpTile::block(), 0, st, a, tile0, s0 + f0);  // (source frames s0 ..)
        }));
        PAPOF_TRY(launch_grid<InterpTile>(FH, FW, n, st, 0, k_res, q));
        for (int it = 0; it < iters; it++) {
            p.Xin = it % 2 ? X1 : X0;
            p.Xout = it == iters - 1 ? nullptr : (it % 2 ? X0 : X1);
            PAPOF_TRY(launch_grid<LowTile>(height, width, n, st, 0, k_back, p));
        }
    }
    return PAPOF_OK;
}
