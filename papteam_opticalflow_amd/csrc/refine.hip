// papteam_opticalflow_amd/csrc/refine.hip -- edge-aware flow refinement (papof_refine_flow_tensor): the image-guided weighted
// median filter of a flow field, the non-local term of Sun, Roth and Black ("Secrets of optical flow estimation and their
// principles", CVPR 2010) as a post-process.
//
// Why.  The solver's smoothness term is isotropic: it rounds every motion boundary off over several pixels and knows nothing
// of the image's edges.  Each output pixel here takes, per component, the weighted median of the flows in a (2 r + 1)^2
// window, the weights falling off with distance, with the guide image's colour difference, and to zero where the caller's
// occlusion mask (or a NaN) says the flow is not to be trusted.
//
// Semantics: include/papof.h, papof_refine_flow_tensor.  The weights are INTEGERS (two host-made tables multiplied), the
// sums 64-bit integers and the values are ordered by the monotone integer key of their float64 bits, so the result is a pure
// function of the inputs: the bits of one particular neighbour, whatever the order of evaluation.
//
// Mapping.  k_refine: a block is a 32 x 8 tile of output pixels (grid.h's grid of tiles and items), one lane per
// pixel.  The tile plus its halo of r is staged once in LDS: both components as keys, the guide (uint8 packed in one dword,
// float32 / float64 as they are), a dead byte folding "outside / occluded / not finite", and the two tables.  A tile with no
// `where` pixel copies its input and leaves after reading the mask.
// Selection without a sort: a weighted quickselect over the window in LDS.  Per component a lane keeps an interval
// (lo, hi] of keys that holds the answer (2 S(lo) < T <= 2 S(hi), S(k) the weight at or below k, T the window's weight, hi
// a value of the window) and narrows it with one pass over the window per pivot; the pass also gathers, on either side of the
// pivot, the smallest and largest key, the sum and the count of the values, from which the next pivot -- the MEAN of the side
// that holds the answer -- and the end (one distinct value left) follow without another pass.  A pivot is any key with
// min <= pivot < max, so every pass removes at least one distinct value, and since the answer does not depend on the pivots the
// mean's rounding is immaterial.  After kMeanPasses the pivot is the midpoint of the keys (at most 64 more passes, whatever the
// values).  u and v run in the same passes and share the weights, which are recomputed per pass (C subtractions, one fp64
// product, two table reads): a lane's 225 weights do not fit its registers.  Lanes of a wave end after different numbers
// of passes; the loop runs to the slowest.  Every offset is 64-bit.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr int kTX = 32, kTY = 8;      // the tile of output pixels (256 lanes)
using OutTile = Tile<kTX, kTY>;
constexpr int kMaxRadius = 15;
constexpr int kMaxIters = 65536;
constexpr int kBins = 4096;           // the range table's bins
constexpr int kMeanPasses = 12;       // passes whose pivot is a mean; the later ones bisect the keys
constexpr long long kKeyMin = (long long)0x8000000000000000ULL, kKeyMax = 0x7fffffffffffffffLL;

struct RefineArgs {
    papof_tensor flow;    // (item, row, column, {vx, vy})
    papof_tensor guide;   // (item, row, column, channel)
    papof_tensor occ;     // uint8 (item, row, column, -); data NULL: none
    papof_tensor where;   // uint8 (item, row, column, -); data NULL: everywhere
    papof_tensor out;     // (item, row, column, {vx, vy}), float32 / float64
    papof_tensor passes;  // uint8 (item, row, column, -); data NULL: not wanted
    const unsigned* S;    // [(2 r + 1)^2]
    const unsigned* R;    // [kBins]
    double q;
    int H, W, C, r;
};

// The monotone integer key of a double's bits (its own inverse): signed comparison of keys orders the values, -0.0 below +0.0.
__device__ __forceinline__ long long flip(long long b) { return b ^ ((b >> 63) & kKeyMax); }
__device__ __forceinline__ long long key_of(double v) { return flip(__double_as_longlong(v)); }
__device__ __forceinline__ double value_of(long long k) { return __longlong_as_double(flip(k)); }

__host__ __device__ inline long long guide_cell_bytes(int gd, int C) {
    return gd == PAPOF_DTYPE_U8 ? 4 : gd == PAPOF_DTYPE_F32 ? 4LL * C : 8LL * C;
}

// bytes of k_refine's LDS: keys of u and v, the guide, the range table, the spatial table, the dead bytes
long long lds_bytes(int gd, int C, int r) {
    const long long cells = (long long)(kTX + 2 * r) * (kTY + 2 * r), side = 2 * r + 1;
    return cells * (16 + guide_cell_bytes(gd, C)) + kBins * 4 + side * side * 4 + ((cells + 15) & ~15LL);
}

// the next pivot of an interval whose smallest and largest keys are mn < mx: mn <= pivot < mx
__device__ __forceinline__ long long next_pivot(long long mn, long long mx, double sum, int cnt, int pass) {
    if (pass < kMeanPasses) {
        const long long k = key_of(sum / (double)cnt);
        return k >= mn && k < mx ? k : mn;  // (a sum that overflowed, or a mean rounded up to mx: mn)
    }
    return mn + (long long)(((unsigned long long)mx - (unsigned long long)mn) >> 1);
}

// What a pass gathers on one side of the pivot: the weight, the extreme keys, the sum and the count of the values.
struct Side {
    unsigned long long w = 0;
    long long mn = kKeyMax, mx = kKeyMin;
    double sum = 0.0;
    int cnt = 0;
    __device__ __forceinline__ void add(long long k, unsigned wk) {
        w += wk;
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
        sum += value_of(k);
        cnt++;
    }
};

// One component's selection: the answer lies in (lo, hi], hi a value of the window; base = the weight at or below lo.
struct Select {
    long long lo = kKeyMin, hi = kKeyMin, piv = 0;
    unsigned long long base = 0;
    bool done = false;
    // the interval's smallest key is mn: finished if that is hi (the answer), else the next pivot
    __device__ __forceinline__ void narrowed(long long mn, double sum, int cnt, int pass) {
        if (mn == hi)
            done = true;
        else
            piv = next_pivot(mn, hi, sum, cnt, pass);
    }
    __device__ __forceinline__ void visit(long long k, unsigned w, Side& low, Side& high) const {
        if (done || !(k > lo && k <= hi)) return;
        if (k <= piv)
            low.add(k, w);
        else
            high.add(k, w);
    }
    __device__ __forceinline__ void decide(unsigned long long T, const Side& low, const Side& high, int pass) {
        if (done) return;
        const unsigned long long s = base + low.w;
        if (2 * s >= T) {  // the answer is at or below the pivot
            hi = low.mx;
            narrowed(low.mn, low.sum, low.cnt, pass);
        } else {
            base = s;
            lo = piv;
            narrowed(high.mn, high.sum, high.cnt, pass);
        }
    }
};

// GD: the guide's dtype.  grid.h's grid over the frame's 32 x 8 tiles; blockIdx.y: item
// `item0` + y.
template <int GD>
__global__ __launch_bounds__(kTX* kTY) void k_refine(const RefineArgs a, long long tile0, long long item0) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int r = a.r, C = a.C, H = a.H, W = a.W;
    const int PW = kTX + 2 * r, PH = kTY + 2 * r, cells = PW * PH, side = 2 * r + 1;
    long long* const keyU = reinterpret_cast<long long*>(smem);
    long long* const keyV = keyU + cells;
    unsigned char* const gbase = reinterpret_cast<unsigned char*>(keyV + cells);
    unsigned* const Rt = reinterpret_cast<unsigned*>(gbase + cells * guide_cell_bytes(GD, C));
    unsigned* const St = Rt + kBins;
    unsigned char* const dead = reinterpret_cast<unsigned char*>(St + side * side);
    const unsigned* const g8 = reinterpret_cast<const unsigned*>(gbase);
    const float* const g32 = reinterpret_cast<const float*>(gbase);
    const double* const g64 = reinterpret_cast<const double*>(gbase);

    const int tid = threadIdx.y * kTX + threadIdx.x;
    PAPOF_TILE_ORIGIN(OutTile, tile0, W, int, x0, int, y0);
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    const long long i = item0 + blockIdx.y;
    const bool inside = x < W && y < H;

    bool mine = inside;
    if (inside && a.where.data)
        mine = static_cast<const unsigned char*>(a.where.data)[PAPOF_AT(a.where, i, y, x)] != 0;  // (through load_u8 an s_nor takes its operands in the other order)
    const long long of = PAPOF_AT(a.flow, i, (long long)y, (long long)x);
    const long long oo = PAPOF_AT(a.out, i, (long long)y, (long long)x);
    const long long op = PAPOF_AT(a.passes, i, (long long)y, (long long)x);
    const bool any = __syncthreads_or(mine ? 1 : 0) != 0;
    if (inside && !mine) {  // copied
        store(a.out, oo, load_flow(a.flow, of));
        store(a.out, oo + a.out.stride[3], load_flow(a.flow, of + a.flow.stride[3]));
        if (a.passes.data) store_u8(a.passes, op, 0);
    }
    if (!any) return;

    // ---- stage the tile and its halo, and the tables
    for (int c = tid; c < cells; c += kTX * kTY) {
        const int cy = c / PW, cx = c - cy * PW;
        const int gy = y0 - r + cy, gx = x0 - r + cx;
        bool d = !(gx >= 0 && gx < W && gy >= 0 && gy < H);
        long long ku = 0, kv = 0;
        if (!d) {
            const long long o = PAPOF_AT(a.flow, i, (long long)gy, (long long)gx);
            const double u = load_flow(a.flow, o), v = load_flow(a.flow, o + a.flow.stride[3]);
            ku = key_of(u);
            kv = key_of(v);
            d = !(isfinite(u) && isfinite(v));
            if (a.occ.data)
                d = d || load_u8(a.occ, PAPOF_AT(a.occ, i, gy, gx)) != 0;
        }
        keyU[c] = ku;
        keyV[c] = kv;
        dead[c] = d ? 1 : 0;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const long long og = PAPOF_AT(a.guide, i, (long long)gy, (long long)gx);
        if (GD == PAPOF_DTYPE_U8) {
            unsigned pk = 0;
            if (in)
                for (int ch = 0; ch < C; ch++)
                    pk |= (unsigned)static_cast<const unsigned char*>(a.guide.data)[og + ch * a.guide.stride[3]] << (8 * ch);
            reinterpret_cast<unsigned*>(gbase)[c] = pk;
        } else if (GD == PAPOF_DTYPE_F32) {
            for (int ch = 0; ch < C; ch++)
                reinterpret_cast<float*>(gbase)[c * C + ch] =
                    in ? static_cast<const float*>(a.guide.data)[og + ch * a.guide.stride[3]] : 0.0f;
        } else {
            for (int ch = 0; ch < C; ch++)
                reinterpret_cast<double*>(gbase)[c * C + ch] =
                    in ? static_cast<const double*>(a.guide.data)[og + ch * a.guide.stride[3]] : 0.0;
        }
    }
    for (int k = tid; k < kBins; k += kTX * kTY) Rt[k] = a.R[k];
    for (int k = tid; k < side * side; k += kTX * kTY) St[k] = a.S[k];
    __syncthreads();
    if (!mine) return;

    // ---- the lane's pixel
    const int cc = ((int)threadIdx.y + r) * PW + (int)threadIdx.x + r;
    unsigned pc = 0;
    double gc[4] = {0.0, 0.0, 0.0, 0.0};
    if (GD == PAPOF_DTYPE_U8)
        pc = g8[cc];
    else
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
            if (ch < C) gc[ch] = GD == PAPOF_DTYPE_F32 ? (double)g32[cc * C + ch] : g64[cc * C + ch];
    const double q = a.q;

    // the weight of the neighbour in cell n whose spatial weight is s: 0 for a dead one
    auto weight = [&](int n, unsigned s) -> unsigned {
        double D;
        if (GD == PAPOF_DTYPE_U8) {
            const unsigned pn = g8[n];
            const int d0 = (int)(pc & 255u) - (int)(pn & 255u), d1 = (int)((pc >> 8) & 255u) - (int)((pn >> 8) & 255u);
            const int d2 = (int)((pc >> 16) & 255u) - (int)((pn >> 16) & 255u), d3 = (int)(pc >> 24) - (int)(pn >> 24);
            D = (double)(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);  // (exact: at most 4 * 255^2)
        } else {
            D = 0.0;
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
                if (ch < C) {
                    const double d = gc[ch] - (GD == PAPOF_DTYPE_F32 ? (double)g32[n * C + ch] : g64[n * C + ch]);
                    D = D + d * d;
                }
        }
        if (dead[n] || !isfinite(D)) return 0u;
        const int k = (int)fmin(D * q, (double)(kBins - 1));
        return s * Rt[k];
    };

    // pass 0: the window's weight, and per component the extreme keys, the sum and the count of the weighted values
    unsigned long long T = 0;
    Select su, sv;
    {
        long long mnu = kKeyMax, mnv = kKeyMax;
        double sumu = 0.0, sumv = 0.0;
        int cnt = 0;
        for (int dy = -r, si = 0; dy <= r; dy++)
            for (int dx = -r; dx <= r; dx++, si++) {
                const int n = cc + dy * PW + dx;
                const unsigned w = weight(n, St[si]);
                if (!w) continue;
                T += w;
                cnt++;
                const long long k0 = keyU[n], k1 = keyV[n];
                mnu = k0 < mnu ? k0 : mnu;
                su.hi = k0 > su.hi ? k0 : su.hi;
                sumu += value_of(k0);
                mnv = k1 < mnv ? k1 : mnv;
                sv.hi = k1 > sv.hi ? k1 : sv.hi;
                sumv += value_of(k1);
            }
        if (T == 0) {  // every neighbour dead: the input
            store(a.out, oo, load_flow(a.flow, of));
            store(a.out, oo + a.out.stride[3], load_flow(a.flow, of + a.flow.stride[3]));
            if (a.passes.data) store_u8(a.passes, op, 1);
            return;
        }
        su.narrowed(mnu, sumu, cnt, 0);
        sv.narrowed(mnv, sumv, cnt, 0);
    }

    int pass = 1;
    while (!(su.done && sv.done)) {
        Side ul, uh, vl, vh;  // of u and v, at or below the pivot and above it
        for (int dy = -r, si = 0; dy <= r; dy++)
            for (int dx = -r; dx <= r; dx++, si++) {
                const int n = cc + dy * PW + dx;
                const unsigned w = weight(n, St[si]);
                if (!w) continue;
                su.visit(keyU[n], w, ul, uh);
                sv.visit(keyV[n], w, vl, vh);
            }
        su.decide(T, ul, uh, pass);
        sv.decide(T, vl, vh, pass);
        pass++;
    }
    store(a.out, oo, value_of(su.hi));
    store(a.out, oo + a.out.stride[3], value_of(sv.hi));
    if (a.passes.data) store_u8(a.passes, op, (unsigned char)(pass > 255 ? 255 : pass));
}

long long plane_pair_bytes(long long n, long long h, long long w) {  // one float64 (n, 2, h, w) field; < 0: refused
    if (n < 1 || h < 1 || w < 1 || h > (1LL << 30) || w > (1LL << 30) || h * w >= (1LL << 30)) return -1;
    const long long per = h * w * 16;
    if (n > (1LL << 61) / per) return -1;
    return n * per;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_refine_workspace(int n, int height, int width, int iters) {
    const long long one = plane_pair_bytes(n, height, width);
    if (one < 0 || iters < 1 || iters > kMaxIters) return -1;
    return iters == 1 ? 0 : iters == 2 ? one : 2 * one;
}

extern "C" int papof_refine_tables(int radius, double sigma_s, unsigned* S, unsigned* R) {
    if (radius < 1 || radius > kMaxRadius || !std::isfinite(sigma_s) || !(sigma_s > 0) || !S || !R) return PAPOF_EINVAL;
    const double two = 2.0 * sigma_s * sigma_s;
    for (int dy = -radius, k = 0; dy <= radius; dy++)
        for (int dx = -radius; dx <= radius; dx++, k++)
            S[k] = (unsigned)std::rint(32768.0 * std::exp(-(double)(dx * dx + dy * dy) / two));
    for (int k = 0; k < kBins; k++) R[k] = (unsigned)std::rint(65536.0 * std::exp(-((double)k + 0.5) / 256.0));
    return PAPOF_OK;
}

extern "C" int papof_refine_flow_tensor(papof_handle* h, int n, int height, int width, int c, const papof_tensor* flow,
                                        const papof_tensor* guide, const papof_tensor* occlusion, const papof_tensor* where,
                                        int radius, const unsigned* S, const unsigned* R, double q, int iters,
                                        const papof_tensor* out, const papof_tensor* passes, void* workspace,
                                        long long workspace_bytes, void* stream) {
    if (!h) return PAPOF_EINVAL;
    const long long need = papof_refine_workspace(n, height, width, iters);
    if (need < 0 || c < 1 || c > 4 || radius < 1 || radius > kMaxRadius) return PAPOF_EINVAL;
    if (!in_flow(flow) || !in_frames(guide) || !out_flow(out))
        return PAPOF_EINVAL;
    if (!opt_in_mask(occlusion)) return PAPOF_EINVAL;
    if (!opt_in_mask(where)) return PAPOF_EINVAL;
    if (!opt_in_mask(passes)) return PAPOF_EINVAL;
    if (!S || !R || !std::isfinite(q) || q < 0) return PAPOF_EINVAL;
    if (need > 0 && (!workspace || workspace_bytes < need)) return PAPOF_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RefineArgs a{};
    a.guide = *guide;
    if (occlusion) a.occ = *occlusion;
    if (where) a.where = *where;
    a.S = S;
    a.R = R;
    a.q = q;
    a.H = height;
    a.W = width;
    a.C = c;
    a.r = radius;
    const long long HW = (long long)height * width, one = need > 0 ? plane_pair_bytes(n, height, width) : 0;
    papof_tensor mid[2];
    for (int k = 0; k < 2; k++) {
        mid[k].data = static_cast<char*>(workspace) + k * one;
        mid[k].dtype = PAPOF_DTYPE_F64;
        mid[k].stride[0] = 2 * HW;
        mid[k].stride[1] = width;
        mid[k].stride[2] = 1;
        mid[k].stride[3] = HW;
    }
    const int gd = guide->dtype;
    const auto kernel = by_dtype(gd, [](auto fd) { return k_refine<fd()>; });
    const size_t lds = (size_t)lds_bytes(gd, c, radius);
    PAPOF_HIP(hipSetDevice(h->device));
    if (lds > 64 * 1024) {  // (above the default bound of a launch's dynamic LDS; a refusal shows at the launch)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    for (int it = 0; it < iters; it++) {
        a.flow = it == 0 ? *flow : mid[(it - 1) & 1];
        a.out = it == iters - 1 ? *out : mid[it & 1];
        a.passes = passes && it == iters - 1 ? *passes : papof_tensor{};
        PAPOF_TRY(launch_grid<OutTile>(height, width, n, st, lds, kernel, a));
    }
    return PAPOF_OK;
}
