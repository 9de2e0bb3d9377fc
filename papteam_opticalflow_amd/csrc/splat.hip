// papteam_opticalflow_amd/csrc/splat.hip -- forward warping (papof_splat_tensor) and frame interpolation by splatting
// (papof_interp_splat_tensor).
//
// Why.  Every other sampler of this library gathers: it reads at "this pixel plus a flow".  Forward warping moves each
// source pixel along its own flow and deposits it where it lands (softmax splatting, Niklaus and Liu, CVPR 2020): the way a
// frame, a flow or a mask is carried to the frame it points to, and the interpolation that stays right at motion
// boundaries, where the output pixel in front of a moving object must not read the background's flow.
//
// Semantics: include/papof.h, papof_splat_tensor.  Many source pixels land on one target, so the sums are made with atomic
// adds -- and stay bitwise reproducible because they are INTEGER sums: every term is one product of doubles (fp64 without
// contraction, -ffp-contract=off) quantised by one rint to 32 fractional bits, and 64-bit integer addition is associative,
// so the order in which the adds arrive cannot change a bit.  A term is at most 2^32 in magnitude and a target receives at
// most one tap per source pixel, so with height * width < 2^30 a sum stays inside int64.
//
// Mapping.  k_splat: a block is a 64 x 4 tile of SOURCE pixels (k_interp's tile), over grid.h's grid of tiles and items;
// a lane reads its flow and weight once and loops over the times (kernel arguments, as k_interp's).  The accumulator is
// PLANAR, [item][time][C + 1][row][column] with the denominator's plane last: neighbouring lanes of a wave are neighbouring
// source pixels of a row, so while the flow is smooth one atomic wave-instruction covers 512 contiguous bytes of one plane
// (eight or nine 64-byte requests at the memory side).  Interleaved ([row][column][C + 1]: a pixel's C + 1 adds adjacent)
// the same instruction touched 32 requests and the kernel took 2.8 x as long.  The adds are no-return 64-bit
// integer atomics at agent scope (one global_atomic_add_x2 each, executed at the memory side; signed terms are added as
// their two's-complement bits).
// k_splat_resolve and k_interp_splat: one lane per TARGET pixel, the division and the strided, typed store.  Every offset is
// 64-bit.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr double kFix = 4294967296.0;      // 2^32: the fixed point's scale
constexpr long long kMinDen = 256;         // a coverage of 2^-24: below it a target is a hole
constexpr long long kOneTimeMax = 1LL << 30;  // papof_splat_workspace: the bytes beyond which times are split over launches

struct SplatArgs {
    papof_tensor x;       // (item, row, column, channel)
    papof_tensor flow;    // (item, row, column, {vx, vy})
    papof_tensor weight;  // (item, row, column, -); data NULL: 1.0 everywhere
    unsigned long long* acc;  // [item][time of this launch][C + 1][row][column], den's plane last
    double inv_bound;     // 1 / bound (a power of two: exact)
    int H, W, C;
    int nt;               // times of this launch
    double t[kMaxTimes];
};

// grid.h's grid over the frame's 64 x 4 tiles of source pixels; blockIdx.y: item
// `item0` + y.
template <int FD>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_splat(const SplatArgs a, long long tile0, long long item0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    PAPOF_TILE_PIXEL(InterpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const int H = a.H, W = a.W, C = a.C;
    const long long i = item0 + blockIdx.y;
    const long long of = PAPOF_AT(a.flow, i, r, x);
    const double u = load_flow(a.flow, of), v = load_flow(a.flow, of + a.flow.stride[3]);
    double w = 1.0;
    if (a.weight.data) w = load_flow(a.weight, PAPOF_AT(a.weight, i, r, x));
    if (!(isfinite(u) && isfinite(v) && isfinite(w)) || !(w > 0)) return;
    w = w > 1.0 ? 1.0 : w;
    const long long pix = PAPOF_AT(a.x, i, r, x);
    const long long C1 = C + 1, HW = H * (long long)W;
    for (int j = 0; j < a.nt; j++) {
        const double X = (double)x + a.t[j] * u, Y = (double)r + a.t[j] * v;
        if (!(X > -1.0 && X < (double)W && Y > -1.0 && Y < (double)H)) continue;
        const double fx0 = floor(X), fy0 = floor(Y);
        const int x0 = (int)fx0, y0 = (int)fy0;  // in [-1, W - 1], [-1, H - 1]
        const double fx = X - fx0, fy = Y - fy0;
        unsigned long long* const at = a.acc + (i * a.nt + j) * C1 * HW;
        double wb[4];
        long long off[4];
#pragma unroll
        for (int m = 0; m <= 1; m++)
#pragma unroll
            for (int n = 0; n <= 1; n++) {
                const int k = 2 * m + n, tx0 = x0 + n, ty0 = y0 + m;
                const bool inside = tx0 >= 0 && tx0 < W && ty0 >= 0 && ty0 < H;
                const double b = (m ? fy : 1.0 - fy) * (n ? fx : 1.0 - fx);
                wb[k] = inside ? w * b : 0.0;  // (a tap whose wb is 0 is dropped)
                off[k] = ty0 * (long long)W + tx0;
            }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (wb[k] != 0.0) add64(at + C * HW + off[k], (long long)rint(wb[k] * kFix));
        for (int ch = 0; ch < C; ch++) {
            double val = load_frame<FD>(a.x, pix + ch * a.x.stride[3], lut) * a.inv_bound;
            val = fmin(fmax(val, -1.0), 1.0);  // |x / bound| > 1 is the caller's error: clamped, so that no sum overflows
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (wb[k] != 0.0) add64(at + ch * HW + off[k], (long long)rint((wb[k] * val) * kFix));
        }
    }
}

struct ResolveArgs {
    const long long* acc;   // k_splat's accumulator, G = nt times per item
    papof_tensor out;       // (item, row, column, channel); time j at + j * tstride
    papof_tensor coverage;  // float64 (item, time, row, column); data NULL: not wanted
    long long tstride;
    double bound, fill;
    int H, W, C;
    int nt;
};

// grid.h's grid over the 64 x 4 tiles of TARGET pixels; blockIdx.y: item `item0` + y.  The launch's times are
// the time slots j0 .. j0 + a.nt of out and coverage.
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_splat_resolve(const ResolveArgs a, long long tile0, long long item0,
                                                                        long long j0) {
    PAPOF_TILE_PIXEL(InterpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const long long i = item0 + blockIdx.y, C1 = a.C + 1, HW = a.H * (long long)a.W;
    const long long outp = PAPOF_AT(a.out, i, r, x);
    for (int j = 0; j < a.nt; j++) {
        const long long* p = a.acc + (i * a.nt + j) * C1 * HW + r * a.W + x;
        const long long den = p[a.C * HW];
        if (a.coverage.data)
            static_cast<double*>(a.coverage.data)[PAPOF_AT_CH(a.coverage, i, j0 + j, r, x)] =  // (item, time, row, column)
                (double)den * (1.0 / kFix);
        const long long oj = outp + (j0 + j) * a.tstride;
        for (int ch = 0; ch < a.C; ch++)
            store(a.out, oj + ch * a.out.stride[3], den >= kMinDen ? ((double)p[ch * HW] / (double)den) * a.bound : a.fill);
    }
}

// papof_interp_splat_tensor's resolve: InterpArgs as k_interp's, acc0 / acc1 the accumulators of im1 along t F01 and of im2
// along (1 - t) F10, a.nt times per pair each.  Where the blended denominator is a hole the pixel is k_interp's.
template <int FD>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_interp_splat(const InterpArgs a, const long long* acc0,
                                                                       const long long* acc1, long long tile0, long long pair0,
                                                                       long long j0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    PAPOF_TILE_PIXEL(InterpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const long long i = pair0 + blockIdx.y, C1 = a.C + 1, HW = a.H * (long long)a.W;
    interp_pixel<FD>(a, lut, i, r, x, j0, [&](int j, long long oj) {
        const double t = a.t[j], s = 1.0 - t;
        const long long o = (i * a.nt + j) * C1 * HW + r * a.W + x;
        const double den = s * (double)acc0[o + a.C * HW] + t * (double)acc1[o + a.C * HW];
        if (!(den >= (double)kMinDen)) return false;  // a hole: k_interp's pixel
        for (int ch = 0; ch < a.C; ch++)
            store(a.out, oj + ch * a.out.stride[3], (s * (double)acc0[o + ch * HW] + t * (double)acc1[o + ch * HW]) / den);
        return true;
    });
}

constexpr long long kMaxSplatChannels = 1 << 20;  // (keeps the bytes of one time below 2^54)

long long one_time_bytes(long long n, long long h, long long w, long long c) {  // < 0: refused
    if (n < 1 || h < 1 || w < 1 || c < 1 || c > kMaxSplatChannels || h > (1LL << 30) || w > (1LL << 30) || h * w >= (1LL << 30))
        return -1;
    const long long per = h * w * (c + 1) * 8;
    if (n > (1LL << 62) / per) return -1;
    return n * per;
}

// times per launch group of a workspace of `bytes`: at most kMaxTimes (kernel arguments), at least 1
int group_of(long long bytes, long long one, int n_times) { return (int)std::min<long long>({bytes / one, kMaxTimes, n_times}); }

bool power_of_two_bound(double b) {
    int e;
    return std::isfinite(b) && b > 0 && std::frexp(b, &e) == 0.5 && e - 1 >= -20 && e - 1 <= 20;
}

int launch_splat(hipStream_t st, SplatArgs a, int n, int g, const double* times) {
    const auto kernel = by_dtype(a.x.dtype, [](auto fd) { return k_splat<fd()>; });
    a.nt = g;
    std::copy(times, times + g, a.t);
    return launch_grid<InterpTile>(a.H, a.W, n, st, 0, kernel, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_splat_workspace(int n, int n_times, int height, int width, int c) {
    const long long one = one_time_bytes(n, height, width, c);
    if (one < 0 || n_times < 1) return -1;
    const long long g = std::min<long long>({(long long)n_times, (long long)kMaxTimes, std::max(1LL, kOneTimeMax / one)});
    return g * one;
}

extern "C" int papof_splat_tensor(papof_handle* h, int n, int height, int width, int c, const papof_tensor* x,
                                  const papof_tensor* flow, const papof_tensor* weight, int n_times, const double* times,
                                  double bound, double fill, const papof_tensor* out, long long time_stride,
                                  const papof_tensor* coverage, void* workspace, long long workspace_bytes, void* stream) {
    if (!h) return PAPOF_EINVAL;
    const long long one = one_time_bytes(n, height, width, c);
    if (one < 0) return PAPOF_EINVAL;
    const auto all = {0, 1, 2, 3};
    if (!in_frames(x) || !in_flow(flow)) return PAPOF_EINVAL;
    if (!opt_in_plane(weight)) return PAPOF_EINVAL;
    if (!out_frames(out) || time_stride < 0 || (n_times > 1 && time_stride == 0)) return PAPOF_EINVAL;
    if (coverage && !described(coverage, {PAPOF_DTYPE_F64}, all, true)) return PAPOF_EINVAL;
    if (n_times < 1 || !times || !power_of_two_bound(bound)) return PAPOF_EINVAL;
    for (int j = 0; j < n_times; j++)
        if (!std::isfinite(times[j])) return PAPOF_EINVAL;
    if (!workspace || workspace_bytes < one) return PAPOF_EINVAL;
    const int g = group_of(workspace_bytes, one, n_times);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SplatArgs a{};
    a.x = *x;
    a.flow = *flow;
    if (weight) a.weight = *weight;
    a.acc = static_cast<unsigned long long*>(workspace);
    a.inv_bound = 1.0 / bound;
    a.H = height;
    a.W = width;
    a.C = c;
    ResolveArgs q{};
    q.acc = static_cast<const long long*>(workspace);
    q.out = *out;
    if (coverage) q.coverage = *coverage;
    q.tstride = time_stride;
    q.bound = bound;
    q.fill = fill;
    q.H = height;
    q.W = width;
    q.C = c;
    const long long tiles = InterpTile::count(height, width);
    PAPOF_HIP(hipSetDevice(h->device));
    for (int j0 = 0; j0 < n_times; j0 += g) {
        const int nt = std::min(g, n_times - j0);
        PAPOF_HIP(hipMemsetAsync(workspace, 0, (size_t)(one * nt), st));
        PAPOF_TRY(launch_splat(st, a, n, nt, times + j0));
        q.nt = nt;
        PAPOF_TRY(launch_tiles(tiles, n, [&](dim3 grid, long long t0, long long i0) {
            hipLaunchKernelGGL(k_splat_resolve, grid, InterpTile::block(), 0, st, q, t0, i0, (long long)j0);
        }));
    }
    return PAPOF_OK;
}

extern "C" int papof_interp_splat_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                         const papof_tensor* frames2, int height, int width, int c,
                                         const papof_tensor* flow_fw, const papof_tensor* flow_bw,
                                         const papof_tensor* weight_fw, const papof_tensor* weight_bw,
                                         const papof_tensor* occlusion, int n_times, const double* times,
                                         const papof_tensor* out, long long time_stride, void* workspace,
                                         long long workspace_bytes, void* stream) {
    if (!h || n_pairs < 1 || n_pairs > 0x3fffffff) return PAPOF_EINVAL;
    const long long one = one_time_bytes(2LL * n_pairs, height, width, c);
    if (one < 0) return PAPOF_EINVAL;
    const auto all = {0, 1, 2, 3};
    if (!in_frames(frames) || (sequence ? frames2 != nullptr : !in_frames(frames2))) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (!opt_in_plane(weight_fw) || !opt_in_plane(weight_bw)) return PAPOF_EINVAL;
    if (occlusion && !described(occlusion, {PAPOF_DTYPE_U8}, all, false)) return PAPOF_EINVAL;
    if (!out_frames(out) || time_stride < 0 || (n_times > 1 && time_stride == 0)) return PAPOF_EINVAL;
    if (n_times < 1 || !times) return PAPOF_EINVAL;
    for (int j = 0; j < n_times; j++)
        if (!std::isfinite(times[j]) || !(times[j] > 0.0 && times[j] < 1.0)) return PAPOF_EINVAL;
    if (!workspace || workspace_bytes < one) return PAPOF_EINVAL;
    const int g = group_of(workspace_bytes, one, n_times);
    hipStream_t st = static_cast<hipStream_t>(stream);
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
    SplatArgs s0{}, s1{};
    s0.x = a.f0;
    s1.x = a.f1;  // im2 of pair i: frame i + seq
    s1.x.data = static_cast<char*>(a.f1.data) + a.seq * a.f1.stride[0] * dtype_bytes(a.f1.dtype);
    s0.flow = a.fw;
    s1.flow = a.bw;
    if (weight_fw) s0.weight = *weight_fw;
    if (weight_bw) s1.weight = *weight_bw;
    s0.inv_bound = s1.inv_bound = 1.0;
    s0.H = s1.H = height;
    s0.W = s1.W = width;
    s0.C = s1.C = c;
    const auto kernel =
        by_frame_dtype(a.f0.dtype == a.f1.dtype ? a.f0.dtype : -1, [](auto fd) { return k_interp_splat<fd()>; });
    const long long tiles = InterpTile::count(height, width);
    PAPOF_HIP(hipSetDevice(h->device));
    for (int j0 = 0; j0 < n_times; j0 += g) {
        const int nt = std::min(g, n_times - j0);
        double back[kMaxTimes];
        for (int j = 0; j < nt; j++) back[j] = 1.0 - times[j0 + j];
        s0.acc = static_cast<unsigned long long*>(workspace);
        s1.acc = s0.acc + (one / 2 / 8) * nt;  // the second accumulator follows the first's n_pairs * nt times
        PAPOF_HIP(hipMemsetAsync(workspace, 0, (size_t)(one * nt), st));
        PAPOF_TRY(launch_splat(st, s0, n_pairs, nt, times + j0));
        PAPOF_TRY(launch_splat(st, s1, n_pairs, nt, back));
        a.nt = nt;
        std::copy(times + j0, times + j0 + nt, a.t);
        const long long* acc0 = reinterpret_cast<const long long*>(s0.acc);
        const long long* acc1 = reinterpret_cast<const long long*>(s1.acc);
        PAPOF_TRY(launch_tiles(tiles, n_pairs, [&](dim3 grid, long long t0, long long p0) {
            hipLaunchKernelGGL(kernel, grid, InterpTile::block(), 0, st, a, acc0, acc1, t0, p0, (long long)j0);
        }));
    }
    return PAPOF_OK;
}
