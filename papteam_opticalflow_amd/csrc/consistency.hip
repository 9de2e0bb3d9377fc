// papteam_opticalflow_amd/csrc/consistency.hip -- blind video temporal consistency (papof_temporal_consistency_tensor,
// papof_consistency_workspace).
//
// Why.  A per-frame process (a style-transfer or colorization network, a tone mapper, a colour grade) run on each frame of a
// video on its own flickers.  Bonneel et al. ("Blind video temporal consistency", SIGGRAPH Asia 2015) remove the flicker
// without knowing the process: each output frame keeps the processed frame's spatial gradients and follows the previous
// output frame, warped along the input video's flow, wherever the flow can be trusted -- one screened-Poisson solve per frame,
// and frame t cannot start before frame t - 1 is stored.
//
// Semantics: include/papof.h, papof_temporal_consistency_tensor.  The hop is k_temporal_filter's backward hop (sampler.h:
// hop), the samplers are sampler.h's, the pull-push is papof_fill_holes_tensor's (inpaint.hip) with confidences; fp64 without
// contraction (-ffp-contract=off).
//
// Mapping.  The frames are a chain on the caller's stream, enqueued back to back with no host synchronisation: per frame t
// one k_tc_setup (one lane per pixel: the hop, the two samples, the weight w and the residual r into level 0 of the
// workspace), one k_tc_pull per coarser level and one k_tc_push per level from coarse to fine (the start value), then
// ceil(iters / depth) launches of k_tc_jacobi, the last of which stores O_t into `out`.  k_tc_jacobi is LDS-tiled and
// temporally blocked as k_sor_blocked (sor.hip): a block owns a 64 x 32 region, its core tile grown by a ghost
// ring as deep as the sweeps it runs, keeps one channel's iterate in LDS, runs the sweeps there and writes back only the
// core, into the other iterate (ping-pong between launches).  A sweep reads only the previous iterate and every cell is
// computed by the same expression wherever it lies, so the bits do not depend on the depth (PAPOF_TC_DEPTH).  The
// workspace holds one frame's levels and is reused by every frame: stream order keeps frame t + 1's setup behind frame t's
// last read of it.  No atomics; every element is written by one lane.  Every offset is 64-bit.
#include "sampler.h"

#include <cstdint>
#include <cstdlib>
#include <vector>

namespace papof {

namespace {

constexpr int kTcBlock = 256;                  // lanes per block of the per-pixel kernels (256: the uint8 table)
constexpr int kJX = 64, kJW = 4, kJR = 8;      // k_tc_jacobi: a region of 64 columns x (4 waves x 8 rows)
constexpr int kJY = kJW * kJR;
constexpr int kMaxDepth = 15;                  // sweeps per launch: the core tile (64 - 2 g) x (32 - 2 g) stays >= 34 x 2
constexpr int kDefaultDepth = 8;               // measured: DESIGN.md 18, profiles/consistency_probe.txt
constexpr int kMaxIters = 1 << 16;

// One pyramid level of the start value, planar: a (h w confidences), v (C planes of h w values).  Level 0's v is r.
struct Lv {
    long long h, w;
    double* a;
    double* v;
};

// level 0: a, w, r[C], d0[C], d1[C]; every coarser level: a, v[C] -- all fp64
long long level_doubles(int l, long long px, int C) { return l == 0 ? (2 + 3LL * C) * px : (1 + (long long)C) * px; }

struct SetupArgs {
    papof_tensor fr;      // frames I (frame, row, column, channel)
    papof_tensor pr;      // processed P
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy}); pair t runs from frame t to t + 1
    papof_tensor out;     // O
    int H, W, CI, CP;
    int check;            // the consistency test is applied
    double lam, sigma, s2;
    double a1, a2;
};

// Frame 0: out[0] = store(first) if given, else store(P_0).
__global__ __launch_bounds__(kTcBlock) void k_tc_first(const papof_tensor src, const papof_tensor out, int H, int W, int C) {
    __shared__ double lut[256];
    stage_u8_lut<-1>(lut);
    const long long i = (long long)blockIdx.x * kTcBlock + threadIdx.x;
    if (i >= (long long)H * W) return;
    const long long r = i / W, c = i % W;
    const long long o = r * src.stride[1] + c * src.stride[2], q = r * out.stride[1] + c * out.stride[2];
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) store(out, q + ch * out.stride[3], load_frame<-1>(src, o + ch * src.stride[3], lut));
}

// Frame t >= 1, pixel (x, r): the backward hop through flow_bw[t - 1] (checked with flow_fw[t - 1]), w, a = w / lambda and
// r = O_{t-1}(X, Y) - P_t(x, r) into level 0 (w = a = r = 0 where the hop is not valid or w is not > 0).
__global__ __launch_bounds__(kTcBlock) void k_tc_setup(const SetupArgs A, const Lv L0, double* wv, long long t) {
    __shared__ double lut[256];
    stage_u8_lut<-1>(lut);
    const long long i = (long long)blockIdx.x * kTcBlock + threadIdx.x;
    const int H = A.H, W = A.W;
    if (i >= (long long)H * W) return;
    const long long HW = (long long)H * W;
    const int x = (int)(i % W);
    const long long r = i / W, pair = chain_pair(t, -1, 1);  // (frame t - 1's output is sampled: the pair's index)
    double X, Y;
    const bool valid = chain_hop(A, pair, -1, H, W, (double)x, (double)r, X, Y);  // (sampler.h, the direction rule)
    double w = 0.0, a = 0.0, res[kMaxChannels];
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++) res[ch] = 0.0;
    if (valid) {
        const Bilinear k = taps_at(X, Y, H, W);
        const long long pix = PAPOF_AT(A.fr, t, r, x);
        const long long prev = pair * A.fr.stride[0];
        double D = 0.0;
#pragma unroll
        for (int ch = 0; ch < kMaxChannels; ch++)
            if (ch < A.CI) {
                const double d = load_frame<-1>(A.fr, pix + ch * A.fr.stride[3], lut) -
                                 sample_frame<-1>(A.fr, prev + ch * A.fr.stride[3], k, lut);
                D += d * d;
            }
        D = D / (double)A.CI;
        w = A.sigma > 0 ? A.lam / (1.0 + D / A.s2) : A.lam;
        if (w > 0) {  // (false for a NaN)
            a = w / A.lam;
            const long long pp = PAPOF_AT(A.pr, t, r, x);
            const long long ob = pair * A.out.stride[0];
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ch++)
                if (ch < A.CP)
                    res[ch] = sample_frame<-1>(A.out, ob + ch * A.out.stride[3], k, lut) -
                              load_frame<-1>(A.pr, pp + ch * A.pr.stride[3], lut);
        } else {
            w = 0.0;
        }
    }
    L0.a[i] = a;
    wv[i] = w;
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < A.CP) L0.v[ch * HW + i] = res[ch];
}

// Pull, level F -> G = F + 1: over the children (2i + a, 2j + b) of G's pixel (i, j) that lie in F, a then b:
// A = sum of their confidences, S_k = sum of a v_k, both from 0; G: v_k = A > 0 ? S_k / A : 0, a = min(A, 1).
__global__ __launch_bounds__(kTcBlock) void k_tc_pull(const Lv F, const Lv G, int C) {
    const long long i = (long long)blockIdx.x * kTcBlock + threadIdx.x;
    if (i >= G.h * G.w) return;
    const long long r = i / G.w, c = i % G.w, fpx = F.h * F.w, gpx = G.h * G.w;
    double s[kMaxChannels], A = 0.0;
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++) s[ch] = 0.0;
#pragma unroll
    for (int a = 0; a <= 1; a++)
#pragma unroll
        for (int b = 0; b <= 1; b++) {
            const long long fr = 2 * r + a, fc = 2 * c + b;
            if (fr >= F.h || fc >= F.w) continue;
            const long long q = fr * F.w + fc;
            const double conf = F.a[q];
            A += conf;
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ch++)
                if (ch < C) s[ch] += conf * F.v[ch * fpx + q];
        }
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) G.v[ch * gpx + i] = A > 0 ? s[ch] / A : 0.0;
    G.a[i] = A < 1.0 ? A : 1.0;
}

// Push, level G = F + 1 (already pushed) -> F: dst_k = a v_k + (1 - a) g_k, g_k G's bilinear sample (sampler.h: taps_at) at
// (0.5 x - 0.25, 0.5 y - 0.25) clamped into G.  dst: F.v (in place) above level 0, the first iterate at level 0.
__global__ __launch_bounds__(kTcBlock) void k_tc_push(const Lv F, const Lv G, double* dst, int C) {
    const long long i = (long long)blockIdx.x * kTcBlock + threadIdx.x;
    if (i >= F.h * F.w) return;
    const long long r = i / F.w, c = i % F.w, fpx = F.h * F.w, gpx = G.h * G.w;
    double X = 0.5 * (double)c - 0.25, Y = 0.5 * (double)r - 0.25;
    X = X < 0 ? 0.0 : X;
    X = X > (double)(G.w - 1) ? (double)(G.w - 1) : X;
    Y = Y < 0 ? 0.0 : Y;
    Y = Y > (double)(G.h - 1) ? (double)(G.h - 1) : Y;
    const Bilinear k = taps_at(X, Y, (int)G.h, (int)G.w);
    const double a = F.a[i];
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) {
            double g = 0.0;
#pragma unroll
            for (int m = 0; m < 4; m++) g += G.v[ch * gpx + k.row[m] * G.w + k.col[m]] * k.w[m];
            dst[ch * fpx + i] = a * F.v[ch * fpx + i] + (1.0 - a) * g;
        }
}

struct JacobiArgs {
    const double* w;    // level 0's weights
    const double* r;    // level 0's residuals (C planes)
    const double* src;  // the iterate read (C planes)
    double* dst;        // the iterate written (C planes); NULL: the frame's last launch, O_t = store(P_t + delta) into out
    papof_tensor pr, out;
    long long t;        // the frame
    int H, W, C;
    int g;              // sweeps of this launch = the depth of the ghost ring
};

// `g` Jacobi sweeps on a 64 x 32 region: the core tile (64 - 2 g) x (32 - 2 g) grown by g cells on every side.  Lane
// (x, wave) owns column x and rows 8 wave .. 8 wave + 7 of the region.  LDS holds one channel's iterate of the region with a
// ring of +0.0 around it; cells outside the image hold +0.0 and are never written, so an absent neighbour enters as +0.0.
// After m sweeps a cell m or more cells inside the region's edge (or on the image's border) holds the exact iterate: after
// g sweeps, the core does.  blockIdx.x: core tile tile0 + x in row-major order.
__global__ __launch_bounds__(kJX* kJW) void k_tc_jacobi(const JacobiArgs A, long long tile0) {
    __shared__ double lut[256];
    __shared__ double s[kJY + 2][kJX + 2];
    const int lane = threadIdx.x, wave = threadIdx.y, tid = wave * kJX + lane;
    fill_u8_lut(lut, tid);
    const int g = A.g, cw = kJX - 2 * g, chh = kJY - 2 * g;
    // (grid.h's decode with the core's run-time extent and the ghost ring taken off, kept as written: DESIGN.md section 41)
    const long long ntx = (A.W + cw - 1) / cw, tile = tile0 + blockIdx.x;
    const long long x0 = (tile % ntx) * cw - g, y0 = (tile / ntx) * chh - g;  // the region's origin
    const long long HW = (long long)A.H * A.W;
    for (int k = tid; k < (kJY + 2) * (kJX + 2); k += kJX * kJW) s[k / (kJX + 2)][k % (kJX + 2)] = 0.0;
    const long long col = x0 + lane;
    bool in[kJR], core[kJR];
    double den[kJR];
    long long p[kJR];
#pragma unroll
    for (int j = 0; j < kJR; j++) {
        const int rl = wave * kJR + j;
        const long long row = y0 + rl;
        in[j] = col >= 0 && col < A.W && row >= 0 && row < A.H;
        core[j] = in[j] && lane >= g && lane < g + cw && rl >= g && rl < g + chh;
        p[j] = in[j] ? row * A.W + col : 0;
        den[j] = 0.0;
        if (in[j]) {
            const double n = (double)((row > 0) + (row < A.H - 1) + (col > 0) + (col < A.W - 1));
            den[j] = n + A.w[p[j]];
        }
    }
    __syncthreads();
    for (int ch = 0; ch < A.C; ch++) {
        const double* src = A.src + ch * HW;
        const double* r = A.r + ch * HW;
        double wr[kJR];
#pragma unroll
        for (int j = 0; j < kJR; j++) {
            wr[j] = 0.0;
            if (in[j]) {
                s[wave * kJR + j + 1][lane + 1] = src[p[j]];
                wr[j] = A.w[p[j]] * r[p[j]];
            }
        }
        __syncthreads();
        for (int it = 0; it < g; it++) {
            double nv[kJR];
#pragma unroll
            for (int j = 0; j < kJR; j++) {
                const int y = wave * kJR + j + 1, x = lane + 1;
                const double S = (s[y - 1][x] + s[y + 1][x]) + (s[y][x - 1] + s[y][x + 1]);
                nv[j] = den[j] != 0.0 ? (S + wr[j]) / den[j] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kJR; j++)
                if (in[j]) s[wave * kJR + j + 1][lane + 1] = nv[j];
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kJR; j++)
            if (core[j]) {
                const double d = s[wave * kJR + j + 1][lane + 1];
                if (A.dst) {
                    A.dst[ch * HW + p[j]] = d;
                } else {
                    const long long row = p[j] / A.W;
                    const long long pp = PAPOF_AT(A.pr, A.t, row, col);
                    const long long q = PAPOF_AT(A.out, A.t, row, col);
                    store(A.out, q + ch * A.out.stride[3], load_frame<-1>(A.pr, pp + ch * A.pr.stride[3], lut) + d);
                }
            }
        __syncthreads();  // (the next channel overwrites the region)
    }
}

int launch_pixels(hipStream_t st, long long px, void (*kernel)(const Lv, const Lv, int), const Lv& F, const Lv& G, int C) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((px + kTcBlock - 1) / kTcBlock)), dim3(kTcBlock), 0, st, F, G, C);
    PAPOF_HIP(hipGetLastError());
    return PAPOF_OK;
}

int launch_jacobi(hipStream_t st, JacobiArgs a) {
    const long long cw = kJX - 2 * a.g, chh = kJY - 2 * a.g;
    return launch_tiles(tile_count(a.H, a.W, cw, chh), 1, [&](dim3 grid, long long t0, long long) {
        hipLaunchKernelGGL(k_tc_jacobi, grid, dim3(kJX, kJW), 0, st, a, t0);
    });
}

int tc_depth() {
    const char* e = std::getenv("PAPOF_TC_DEPTH");  // A/B knob: sweeps per k_tc_jacobi launch (the bits do not change)
    return e ? std::max(1, std::min(kMaxDepth, std::atoi(e))) : kDefaultDepth;
}

int launch_consistency(hipStream_t st, const SetupArgs& A, const papof_tensor* first, int T, int iters, char* ws) {
    const long long H = A.H, W = A.W, HW = H * W;
    const int C = A.CP;
    const auto sizes = level_sizes(H, W);
    std::vector<Lv> L;
    double* p = reinterpret_cast<double*>(ws);
    double *wv = nullptr, *d0 = nullptr, *d1 = nullptr;
    for (size_t l = 0; l < sizes.size(); l++) {
        const long long px = sizes[l].first * sizes[l].second;
        Lv v{sizes[l].first, sizes[l].second, p, p + (l == 0 ? 2 * px : px)};
        if (l == 0) {
            wv = p + px;
            d0 = v.v + C * px;
            d1 = d0 + C * px;
        }
        L.push_back(v);
        p += level_doubles((int)l, px, C);
    }
    const unsigned blocks = (unsigned)((HW + kTcBlock - 1) / kTcBlock);  // <= kMaxTiles: papof_consistency_workspace
    papof_tensor f0 = first ? *first : A.pr;
    hipLaunchKernelGGL(k_tc_first, dim3(blocks), dim3(kTcBlock), 0, st, f0, A.out, A.H, A.W, C);
    PAPOF_HIP(hipGetLastError());
    const int depth = tc_depth(), top = (int)L.size() - 1;
    for (long long t = 1; t < T; t++) {
        hipLaunchKernelGGL(k_tc_setup, dim3(blocks), dim3(kTcBlock), 0, st, A, L[0], wv, t);
        PAPOF_HIP(hipGetLastError());
        for (int l = 0; l < top; l++)
            PAPOF_TRY(launch_pixels(st, L[l + 1].h * L[l + 1].w, k_tc_pull, L[l], L[l + 1], C));
        for (int l = top - 1; l >= 0; l--) {
            hipLaunchKernelGGL(k_tc_push, dim3((unsigned)((L[l].h * L[l].w + kTcBlock - 1) / kTcBlock)), dim3(kTcBlock), 0,
                               st, L[l], L[l + 1], l == 0 ? d0 : L[l].v, C);
            PAPOF_HIP(hipGetLastError());
        }
        // the start value: the pushed level 0 (a 1 x 1 frame has no coarser level: its start value is r itself)
        JacobiArgs j{wv, L[0].v, top == 0 ? L[0].v : d0, nullptr, A.pr, A.out, t, A.H, A.W, C, 0};
        int left = iters;
        do {
            j.g = std::min(left, depth);
            left -= j.g;
            j.dst = left > 0 ? (j.src == d0 ? d1 : d0) : nullptr;
            PAPOF_TRY(launch_jacobi(st, j));
            j.src = j.dst;
        } while (left > 0);
    }
    return PAPOF_OK;
}

// the bytes [lo, hi) a descriptor of sizes n[4] (non-negative strides) can touch
struct Span {
    std::uintptr_t lo, hi;
};

Span span(const papof_tensor& t, std::initializer_list<long long> n) {
    const long long es = dtype_bytes(t.dtype);
    unsigned long long last = 0;
    int i = 0;
    for (long long k : n) last += (unsigned long long)(k - 1) * (unsigned long long)t.stride[i++];
    const std::uintptr_t lo = reinterpret_cast<std::uintptr_t>(t.data);
    return {lo, lo + (std::uintptr_t)((last + 1) * es)};
}

bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_consistency_workspace(int height, int width, int c_out) {
    if (height < 1 || width < 1 || c_out < 1 || c_out > kMaxChannels) return -1;
    if ((long long)height * width > kMaxTiles * kTcBlock) return -1;
    long long n = 0;
    const auto s = level_sizes(height, width);
    for (size_t l = 0; l < s.size(); l++) n += level_doubles((int)l, s[l].first * s[l].second, c_out);
    return 8 * n;
}

extern "C" int papof_temporal_consistency_tensor(papof_handle* h, int n_frames, int height, int width, int c_frames,
                                                 int c_out, const papof_tensor* frames, const papof_tensor* processed,
                                                 const papof_tensor* flow_fw, const papof_tensor* flow_bw,
                                                 const papof_tensor* first, double lambda, double sigma, int iters,
                                                 int use_check, double alpha1, double alpha2, const papof_tensor* out,
                                                 void* workspace, long long workspace_bytes, void* stream) {
    if (!h || n_frames < 2 || height < 1 || width < 1 || c_frames < 1 || c_frames > kMaxChannels) return PAPOF_EINVAL;
    if (!std::isfinite(lambda) || lambda < 0 || !std::isfinite(sigma) || sigma < 0) return PAPOF_EINVAL;
    if (iters < 0 || iters > kMaxIters || !valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    const long long need = papof_consistency_workspace(height, width, c_out);
    if (need < 0 || !workspace || (reinterpret_cast<std::uintptr_t>(workspace) & 7) || workspace_bytes < need)
        return PAPOF_EINVAL;
    if (!in_frames(frames) || !in_frames(processed)) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (first && !described(first, kImageDtypes, {1, 2, 3}, false)) return PAPOF_EINVAL;
    if (!out_frames(out)) return PAPOF_EINVAL;
    const long long T = n_frames, H = height, W = width;
    const Span o = span(*out, {T, H, W, c_out});
    const Span ws{reinterpret_cast<std::uintptr_t>(workspace), reinterpret_cast<std::uintptr_t>(workspace) + (std::uintptr_t)need};
    std::vector<Span> ins{span(*frames, {T, H, W, c_frames}), span(*processed, {T, H, W, c_out}),
                          span(*flow_fw, {T - 1, H, W, 2}), span(*flow_bw, {T - 1, H, W, 2})};
    if (first) ins.push_back(span(*first, {1, H, W, c_out}));
    if (overlap(o, ws)) return PAPOF_EINVAL;
    for (const Span& s : ins)
        if (overlap(o, s) || overlap(ws, s)) return PAPOF_EINVAL;
    SetupArgs a{};
    a.fr = *frames;
    a.pr = *processed;
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    a.out = *out;
    a.H = height;
    a.W = width;
    a.CI = c_frames;
    a.CP = c_out;
    a.check = use_check ? 1 : 0;
    a.lam = lambda;
    a.sigma = sigma;
    a.s2 = sigma * sigma;
    a.a1 = alpha1;
    a.a2 = alpha2;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_consistency(static_cast<hipStream_t>(stream), a, first, n_frames, iters, static_cast<char*>(workspace));
}
