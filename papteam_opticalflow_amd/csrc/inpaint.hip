// papteam_opticalflow_amd/csrc/inpaint.hip -- flow-guided video completion (papof_fill_holes_tensor, papof_fill_workspace,
// papof_propagate_tensor).
//
// Why.  Removing an object, a logo or a damaged region from a video (Xu et al., CVPR 2019; Gao et al., ECCV 2020): every
// pixel under the caller's mask is filled with the background that the flows show in other frames, and what no frame shows
// is filled spatially.  Two pieces were missing: a fill of a field inside a mask -- the flows inside the hole describe the
// object and must be replaced before a chain can cross the hole, and the pixels no frame shows need a spatial fill -- and
// chains that stop at the nearest frame where the point is visible.  Written in PyTorch, both are dozens of launches per
// frame with a temporary per pyramid level or hop.
//
// Semantics: include/papof.h, papof_fill_holes_tensor and papof_propagate_tensor.  fp64 without contraction
// (-ffp-contract=off); the samplers are sampler.h's.
//
// Mapping.  The fill is pull-push (Gortler et al. 1996) followed by Jacobi relaxation on every level, all frames of the
// call in each launch (blockIdx.y the frame, blockIdx.x 256 consecutive pixels of the level in row-major order): one launch
// copies the input into level 0 of the workspace, one pull launch per coarser level, then from coarse to fine one push and
// `relax` sweeps per level, and one launch stores level 0.  Each level keeps two fp64 iterates (the known pixels' values
// live in the first only) and a byte per pixel that says whether it is known; a sweep reads one iterate and writes the
// other, so the result does not depend on the schedule.  The propagation is one launch, one lane per output pixel in 64 x 4
// tiles (as k_temporal_filter): the chain, the candidates and their distances stay in registers.  No atomics; every
// output element belongs to one lane.  Every offset is 64-bit.
#include "sampler.h"

#include <cstdint>
#include <vector>

namespace papof {

namespace {

constexpr int kFillBlock = 256;                // lanes per block of the fill kernels (256: the uint8 table)
constexpr int kPropTX = 64, kPropTY = 4;       // a 64 x 4 tile of output pixels per block of k_propagate
using PropTile = Tile<kPropTX, kPropTY>;
constexpr int kMaxRelax = 1 << 16;

// One pyramid level of the fill's workspace: all frames' (row, column, channel) values, row-major, channels innermost.
struct Level {
    long long h, w;
    double* v0;          // the known pixels' values, and the first iterate of the unknown ones
    double* v1;          // the second iterate of the unknown ones
    unsigned char* k;    // 1: known
};

// the bytes of one level of n frames with C channels: two fp64 iterates and the known bytes, rounded up to 8
long long level_bytes(long long n, long long h, long long w, int C) {
    const long long px = n * h * w;
    return 16LL * C * px + ((px + 7) / 8) * 8;
}

// The fp64 value of pixel p of a level: its own in v0 if it is known, else the iterate `it`.
__device__ __forceinline__ double value(const Level& L, const double* it, long long p, int C, int ch) {
    return L.k[p] ? L.v0[p * C + ch] : it[p * C + ch];
}

// Level 0 from the input: v0 = x (uint8: x / 255.0) where the mask is 0 and known = 1, else v0 = 0 and known = 0.
template <int FD>
__global__ __launch_bounds__(kFillBlock) void k_fill_base(const papof_tensor x, const papof_tensor mask, const Level L,
                                                          int C, long long f0) {
    __shared__ double lut[256];
    stage_u8_lut<FD>(lut);
    const long long i = (long long)blockIdx.x * kFillBlock + threadIdx.x;
    if (i >= L.h * L.w) return;
    const long long t = f0 + blockIdx.y, r = i / L.w, c = i % L.w, p = t * L.h * L.w + i;
    const bool known = load_u8(mask, PAPOF_AT(mask, t, r, c)) == 0;
    const long long o = PAPOF_AT(x, t, r, c);
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) L.v0[p * C + ch] = known ? load_frame<FD>(x, o + ch * x.stride[3], lut) : 0.0;
    L.k[p] = known ? 1 : 0;
}

// Pull, level F -> level G = F + 1: the known children (2i + a, 2j + b) of G's pixel (i, j), a then b, that lie in F;
// S = their sum from 0, N = their number; G's pixel is S / N and known if N > 0, else 0 and unknown.
__global__ __launch_bounds__(kFillBlock) void k_fill_pull(const Level F, const Level G, int C, long long f0) {
    const long long i = (long long)blockIdx.x * kFillBlock + threadIdx.x;
    if (i >= G.h * G.w) return;
    const long long t = f0 + blockIdx.y, r = i / G.w, c = i % G.w, p = t * G.h * G.w + i;
    double s[kMaxChannels];
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++) s[ch] = 0.0;
    int n = 0;
#pragma unroll
    for (int a = 0; a <= 1; a++)
#pragma unroll
        for (int b = 0; b <= 1; b++) {
            const long long fr = 2 * r + a, fc = 2 * c + b;
            if (fr >= F.h || fc >= F.w) continue;
            const long long q = (t * F.h + fr) * F.w + fc;
            if (!F.k[q]) continue;
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ch++)
                if (ch < C) s[ch] += F.v0[q * C + ch];
            n += 1;
        }
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) G.v0[p * C + ch] = n > 0 ? s[ch] / (double)n : 0.0;
    G.k[p] = n > 0 ? 1 : 0;
}

// Push, level G = F + 1 (filled; its unknown pixels' values in the iterate `git`) -> level F: an unknown pixel (x, y) of F
// takes G's bilinear sample (sampler.h: taps_at) at (0.5 x - 0.25, 0.5 y - 0.25) clamped into G, the first iterate.
__global__ __launch_bounds__(kFillBlock) void k_fill_push(const Level F, const Level G, const double* git, int C,
                                                          long long f0) {
    const long long i = (long long)blockIdx.x * kFillBlock + threadIdx.x;
    if (i >= F.h * F.w) return;
    const long long t = f0 + blockIdx.y, r = i / F.w, c = i % F.w, p = t * F.h * F.w + i;
    if (F.k[p]) return;
    double X = 0.5 * (double)c - 0.25, Y = 0.5 * (double)r - 0.25;
    X = X < 0 ? 0.0 : X;
    X = X > (double)(G.w - 1) ? (double)(G.w - 1) : X;
    Y = Y < 0 ? 0.0 : Y;
    Y = Y > (double)(G.h - 1) ? (double)(G.h - 1) : Y;
    const Bilinear k = taps_at(X, Y, (int)G.h, (int)G.w);
    const long long base = t * G.h * G.w;
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) {
            double g = 0.0;
#pragma unroll
            for (int m = 0; m < 4; m++) g += value(G, git, base + k.row[m] * G.w + k.col[m], C, ch) * k.w[m];
            F.v0[p * C + ch] = g;
        }
}

// One Jacobi sweep over the unknown pixels of a level: dst = ((v_N + v_S) + (v_W + v_E)) * 0.25 of the iterate src,
// neighbours clamped into the image (a known neighbour: its own value).
__global__ __launch_bounds__(kFillBlock) void k_fill_relax(const Level L, const double* src, double* dst, int C,
                                                           long long f0) {
    const long long i = (long long)blockIdx.x * kFillBlock + threadIdx.x;
    if (i >= L.h * L.w) return;
    const long long t = f0 + blockIdx.y, r = i / L.w, c = i % L.w, base = t * L.h * L.w, p = base + i;
    if (L.k[p]) return;
    const long long n = base + (r > 0 ? r - 1 : 0) * L.w + c, s = base + (r < L.h - 1 ? r + 1 : r) * L.w + c;
    const long long w = base + r * L.w + (c > 0 ? c - 1 : 0), e = base + r * L.w + (c < L.w - 1 ? c + 1 : c);
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C)
            dst[p * C + ch] = ((value(L, src, n, C, ch) + value(L, src, s, C, ch)) +
                               (value(L, src, w, C, ch) + value(L, src, e, C, ch))) * 0.25;
}

// out from level 0: a known pixel its own (input) value, an unknown one the final iterate, by sampler.h's store()
__global__ __launch_bounds__(kFillBlock) void k_fill_store(const Level L, const double* it, const papof_tensor out, int C,
                                                           long long f0) {
    const long long i = (long long)blockIdx.x * kFillBlock + threadIdx.x;
    if (i >= L.h * L.w) return;
    const long long t = f0 + blockIdx.y, r = i / L.w, c = i % L.w, p = t * L.h * L.w + i;
    const long long o = PAPOF_AT(out, t, r, c);
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < C) store(out, o + ch * out.stride[3], value(L, it, p, C, ch));
}

// Enqueues one kernel over every pixel of an h x w level of n frames (gridDim.y: the frame).
template <typename K, typename... A>
int launch_level(hipStream_t st, K kernel, long long n, long long h, long long w, const A&... args) {
    const long long blocks = (h * w + kFillBlock - 1) / kFillBlock;  // <= kMaxTiles: papof_fill_workspace
    return launch_tiles(blocks, n, [&](dim3 grid, long long, long long f0) {
        hipLaunchKernelGGL(kernel, grid, dim3(kFillBlock), 0, st, args..., f0);
    });
}

int launch_fill(hipStream_t st, const papof_tensor& x, const papof_tensor& mask, const papof_tensor& out, long long n,
                long long H, long long W, int C, int relax, char* ws) {
    const auto sizes = level_sizes(H, W);
    std::vector<Level> L;
    for (const auto& s : sizes) {
        const long long px = n * s.first * s.second;
        Level l{s.first, s.second, reinterpret_cast<double*>(ws), reinterpret_cast<double*>(ws) + px * C,
                reinterpret_cast<unsigned char*>(ws) + 16 * px * C};
        L.push_back(l);
        ws += level_bytes(n, s.first, s.second, C);
    }
    const auto base = by_dtype(x.dtype, [](auto fd) { return k_fill_base<fd()>; });
    PAPOF_TRY(launch_level(st, base, n, H, W, x, mask, L[0], C));
    const int top = (int)L.size() - 1;
    for (int l = 0; l < top; l++) PAPOF_TRY(launch_level(st, k_fill_pull, n, L[l + 1].h, L[l + 1].w, L[l], L[l + 1], C));
    // the iterate holding a level's unknown pixels once it is filled: v0 after an even number of sweeps, else v1 (the
    // coarsest level, 1 x 1, runs none: a sweep there would give its pixel back)
    auto final_it = [&](int l) -> const double* { return l < top && relax % 2 ? L[l].v1 : L[l].v0; };
    for (int l = top - 1; l >= 0; l--) {
        PAPOF_TRY(launch_level(st, k_fill_push, n, L[l].h, L[l].w, L[l], L[l + 1], final_it(l + 1), C));
        for (int s = 0; s < relax; s++) {
            const double* src = s % 2 ? L[l].v1 : L[l].v0;
            double* dst = s % 2 ? L[l].v0 : L[l].v1;
            PAPOF_TRY(launch_level(st, k_fill_relax, n, L[l].h, L[l].w, L[l], src, dst, C));
        }
    }
    return launch_level(st, k_fill_store, n, H, W, L[0], final_it(0), out, C);
}

struct PropArgs {
    papof_tensor fr;      // frames (frame, row, column, channel)
    papof_tensor mk;      // uint8 masks (frame, row, column)
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy}); pair t runs from frame t to t + 1
    papof_tensor out;     // (frame, row, column, channel)
    papof_tensor st;      // uint8 status (frame, row, column)
    int T, H, W, C, R;
    int check;            // the consistency test is applied
    double a1, a2;
};

// The candidate of one direction of frame t's hole pixel (x, r): the chain hops as k_temporal_filter's (denoise.hip) and
// stops at the first frame whose four clamped taps at the landing point are all outside that frame's mask.  dir = +-1:
// sampler.h, the direction rule, whose steps, pairs and frames these are.  The flow f that is read and the flow b it is checked
// with are the rule's too, chain_flow(a, dir) and chain_check(a, dir), chosen by the kernel in front of the call: with
// chain_hop's selection inside this loop the kernel's loop invariants were hoisted in another order (DESIGN.md section 45,
// kernels that deviate).  Returns the distance j, or 0 where the chain dies first.
template <int FD>
__device__ __forceinline__ int candidate(const PropArgs& a, const papof_tensor& f, const papof_tensor& b, long long t,
                                         int dir, int steps, double X, double Y, double* g, const double* lut) {
    const int H = a.H, W = a.W;
    const unsigned char* mk = static_cast<const unsigned char*>(a.mk.data);  // (the taps' bytes: one pointer for the loop)
    for (int j = 1; j <= steps; j++) {
        const long long pair = chain_pair(t, dir, j), frame = chain_frame(t, dir, j);
        double nX, nY;
        if (!hop(f, b, pair, H, W, a.check, a.a1, a.a2, X, Y, nX, nY)) return 0;  // once dead, the chain stays dead
        X = nX;
        Y = nY;
        const Bilinear k = taps_at(X, Y, H, W);
        const long long mb = frame * a.mk.stride[0];
        bool clear = true;
#pragma unroll
        for (int i = 0; i < 4; i++) clear = clear && mk[mb + k.row[i] * a.mk.stride[1] + k.col[i] * a.mk.stride[2]] == 0;
        if (clear) {
            const long long base = frame * a.fr.stride[0];
#pragma unroll
            for (int ch = 0; ch < kMaxChannels; ch++)
                if (ch < a.C) g[ch] = sample_frame<FD>(a.fr, base + ch * a.fr.stride[3], k, lut);
            return j;
        }
    }
    return 0;
}

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y.
template <int FD>
__global__ __launch_bounds__(kPropTX* kPropTY) void k_propagate(const PropArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kPropTX>(lut);
    PAPOF_TILE_PIXEL(PropTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    const long long pix = PAPOF_AT(a.fr, t, r, x);
    const long long o = PAPOF_AT(a.out, t, r, x);
    const bool hole = load_u8(a.mk, PAPOF_AT(a.mk, t, r, x)) != 0;
    double gf[kMaxChannels], gb[kMaxChannels];
    int df = 0, db = 0;
    if (hole) {
        const int fwd = chain_steps(a.T, t, +1, a.R), bwd = chain_steps(a.T, t, -1, a.R);
        df = candidate<FD>(a, chain_flow(a, +1), chain_check(a, +1), t, +1, fwd, (double)x, (double)r, gf, lut);
        db = candidate<FD>(a, chain_flow(a, -1), chain_check(a, -1), t, -1, bwd, (double)x, (double)r, gb, lut);
    }
    const double wf = df ? 1.0 / (double)df : 0.0, wb = db ? 1.0 / (double)db : 0.0;
#pragma unroll
    for (int ch = 0; ch < kMaxChannels; ch++)
        if (ch < a.C) {
            double v;
            if (df && db)
                v = (wf * gf[ch] + wb * gb[ch]) / (wf + wb);
            else if (df)
                v = gf[ch];
            else if (db)
                v = gb[ch];
            else
                v = load_frame<FD>(a.fr, pix + ch * a.fr.stride[3], lut);
            store(a.out, o + ch * a.out.stride[3], v);
        }
    // (store_u8 would evaluate the value before it reads a.st.data, and the kernel's tail is scheduled differently)
    static_cast<unsigned char*>(a.st.data)[PAPOF_AT(a.st, t, r, x)] = !hole ? 0 : (df || db) ? 1 : 2;
}

int launch_propagate(hipStream_t st, const PropArgs& a) {
    const auto kernel = by_dtype(a.fr.dtype, [](auto fd) { return k_propagate<fd()>; });
    return launch_grid<PropTile>(a.H, a.W, a.T, st, 0, kernel, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_fill_workspace(int n_frames, int height, int width, int c) {
    if (n_frames < 1 || height < 1 || width < 1 || c < 1 || c > kMaxChannels) return -1;
    if ((long long)height * width > kMaxTiles * kFillBlock) return -1;
    long long bytes = 0;
    for (const auto& s : level_sizes(height, width)) {
        const long long b = level_bytes(n_frames, s.first, s.second, c);
        if (b > (1LL << 60) - bytes) return -1;
        bytes += b;
    }
    return bytes;
}

extern "C" int papof_fill_holes_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* x,
                                       const papof_tensor* mask, int relax, const papof_tensor* out, void* workspace,
                                       long long workspace_bytes, void* stream) {
    if (!h || relax < 0 || relax > kMaxRelax) return PAPOF_EINVAL;
    const long long need = papof_fill_workspace(n_frames, height, width, c);
    if (need < 0 || !workspace || (reinterpret_cast<std::uintptr_t>(workspace) & 7) || workspace_bytes < need)
        return PAPOF_EINVAL;
    if (!in_frames(x) || !out_frames(out)) return PAPOF_EINVAL;
    if (!described(mask, {PAPOF_DTYPE_U8}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_fill(static_cast<hipStream_t>(stream), *x, *mask, *out, n_frames, height, width, c, relax,
                       static_cast<char*>(workspace));
}

extern "C" int papof_propagate_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                      const papof_tensor* frames, const papof_tensor* masks, const papof_tensor* flow_fw,
                                      const papof_tensor* flow_bw, int radius, int use_check, double alpha1, double alpha2,
                                      const papof_tensor* out, const papof_tensor* status, void* stream) {
    if (!h || n_frames < 2 || height < 1 || width < 1 || c < 1 || c > kMaxChannels) return PAPOF_EINVAL;
    if (radius < 1 || radius > n_frames - 1 || !valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    if (!in_frames(frames) || !described(masks, {PAPOF_DTYPE_U8}, {0, 1, 2}, false))
        return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (!out_frames(out) || !described(status, {PAPOF_DTYPE_U8}, {0, 1, 2}, true))
        return PAPOF_EINVAL;
    PropArgs a{};
    a.fr = *frames;
    a.mk = *masks;
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    a.out = *out;
    a.st = *status;
    a.T = n_frames;
    a.H = height;
    a.W = width;
    a.C = c;
    a.R = radius;
    a.check = use_check ? 1 : 0;
    a.a1 = alpha1;
    a.a2 = alpha2;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_propagate(static_cast<hipStream_t>(stream), a);
}
