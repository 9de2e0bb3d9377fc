// papteam_opticalflow_amd/csrc/kernels.hip -- every stage of the hot path except the SOR sweeps.
//
// One thread per output pixel, 64 x 4 thread blocks with threadIdx.x along the row so that each
// wavefront reads/writes 512 contiguous bytes of a plane (planar fp64 layout, see common.h).
// All kernels are HBM-bound stencils / gathers (no dense contraction => no MFMA).  Floating-point
// operation ORDER follows the reference line by line (cited per kernel; paths relative to
// /root/reference/Code/Serial/) because the parity bar is bit-compatibility, and the file is compiled
// with -ffp-contract=off for the same reason.
#include "common.h"
#include "sampler.h"

#include <cmath>
#include <type_traits>

namespace papof {

namespace {

constexpr int BX = 64, BY = 4;

constexpr int tiles_of(int n, int t) { return (n + t - 1) / t; }  // tiles of t cells that cover n cells
inline dim3 grid2d(int W, int H, int planes = 1) { return dim3(tiles_of(W, BX), tiles_of(H, BY), planes); }
inline Rect region(const Rect* rc, int W, int H) { return rc ? *rc : Rect{0, 0, W, H}; }
inline dim3 grid2d(const Rect& r, int planes = 1) { return grid2d(r.x1 - r.x0, r.y1 - r.y0, planes); }

// Phase stamp: the first thread of a kernel's first block writes the constant 100 MHz clock where the host asked for
// it (flow_internal.h: PhaseClock in stamp mode) -- the start of the first kernel of a phase IS the start of the phase,
// at no cost to the stream (a HIP event between two kernels costs ~2.6 us of stream time; ~100 per call = 2 %).
__device__ __forceinline__ void stamp_now(unsigned long long* s) {
    if (s && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x | threadIdx.y) == 0u) *s = __builtin_amdgcn_s_memrealtime();
}
__global__ void k_stamp(unsigned long long* s) { stamp_now(s); }

__host__ __device__ __forceinline__ int clampi(int x, int n) {  // EnforceRange, src/ImageProcessing.h:34
    x = x < 0 ? 0 : x;
    return x > n - 1 ? n - 1 : x;
}

// Tiled kernels launched on a 1-D grid of xcd_grid(tiles) blocks (x; channels, if any, in z): workgroups are dealt round-robin
// over the 8 XCDs (observed; speed only), so block b works on tile (b % 8) * per + b / 8 -- a contiguous run of tiles (row-major)
// per XCD: the halo rows and columns neighbouring tiles both read are found in that XCD's L2.  false: no tile for this block.
__device__ __forceinline__ bool xcd_tile(int ntx, int nty, int& tx, int& ty) {
    const int ntiles = ntx * nty, per = (ntiles + 7) >> 3;
    const int vt = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per || vt >= ntiles) return false;
    ty = vt / ntx;
    tx = vt - ty * ntx;
    return true;
}
static inline unsigned xcd_grid(int ntx, int nty) { return 8u * (unsigned)(((size_t)ntx * nty + 7) / 8); }

// ------------------------------------------------------------------------------------------------
// The expressions of the kernels between two solves, each stated ONCE.  The fused kernels and the forms they
// grew out of all evaluate these, so bit parity with the reference holds by construction, not by identical edits.
// ------------------------------------------------------------------------------------------------
// correlation with 2 * half + 1 taps: accumulated from 0 in the order l = -half .. half (src/ImageProcessing.h:259-279);
// at(l) is the operand at offset l -- the caller's clamp, LDS row or register lives there.  HALF: the half-width as a
// compile-time constant (the 5-tap passes: tap_sum<2>), or -1: half_rt at run time
template <int HALF = -1, class At>
__device__ __forceinline__ double tap_sum(const Taps& f, At at, int half_rt = HALF) {
    const int half = HALF >= 0 ? HALF : half_rt;
    double acc = 0.0;
#pragma unroll
    for (int l = -half; l <= half; l++) acc += at(l) * f.t[l + half];
    return acc;
}

// Im = Im1s * 0.4 + Im2s * 0.6 (Multiplywith, Add(..., 0.6): src/OpticalFlow.cpp:92-93) and imdt = Im2s - Im1s (:97)
__device__ __forceinline__ void blend_imdt(double s1, double s2, double& blend, double& imdt) {
    double t = s1;
    t *= 0.4;
    t += s2 * 0.6;
    blend = t;
    imdt = s2 - s1;
}

// phi, src/OpticalFlow.cpp:295-331, from the flow at the cell, its right and its lower neighbour: forward differences, zero
// in the last column (!right) / row (!down) (src/Image.h:979-986, :1022-1029), phi = 0.5 / sqrt(ux^2 + uy^2 + vx^2 + vy^2 + eps)
__device__ __forceinline__ double phi_value(double uc, double vc, double ur, double vr, double ud, double vd, bool right,
                                            bool down) {
    const double ux = right ? ur - uc : 0.0;
    const double uy = down ? ud - uc : 0.0;
    const double vx = right ? vr - vc : 0.0;
    const double vy = down ? vd - vc : 0.0;
    const double t = ux * ux + uy * uy + vx * vx + vy * vy;
    return 0.5 / sqrt(t + 0.001 * 0.001);
}
// ... of the flow as it stands in memory (no increment): only neighbours that exist are loaded
__device__ __forceinline__ double phi_at(const double* __restrict__ u, const double* __restrict__ v, int i, int j, int H,
                                         int W) {
    const size_t o = (size_t)i * W + j;
    const double uc = u[o], vc = v[o];
    double ur = 0.0, vr = 0.0, ud = 0.0, vd = 0.0;
    if (j < W - 1) {
        ur = u[o + 1];
        vr = v[o + 1];
    }
    if (i < H - 1) {
        ud = u[o + W];
        vd = v[o + W];
    }
    return phi_value(uc, vc, ur, vr, ud, vd, j < W - 1, i < H - 1);
}

// ImageProcessing::warpImage, src/ImageProcessing.h:483-503: a pixel whose position leaves the image takes frame 1's value
__device__ __forceinline__ bool leaves_image(double x, double y, int W, int H) {
    return x < 0 || x > W - 1 || y < 0 || y > H - 1;
}
// BilinearInterpolate (:138-157) at a position INSIDE the image: 0 <= (int)x <= W - 1 needs no clamp from below, dx = x - (int)x
// is in [0, 1) as it is, |1 - dx| = 1 - dx and |0 - dx| = dx -- the values of bilinear_taps() below with a third of the
// instructions.  Taps in bilinear_apply()'s visiting order: g0 = (x0, y0), g1 = (x0, y1), g2 = (x1, y0), g3 = (x1, y1).
__device__ __forceinline__ double bilinear_inside(double g0, double g1, double g2, double g3, double dx, double dy) {
    const double ex = 1.0 - dx, ey = 1.0 - dy;
    double res = 0.0;
    res += g0 * (ex * ey);
    res += g1 * (ex * dy);
    res += g2 * (dx * ey);
    res += g3 * (dx * dy);
    return res;
}
// ... with the four taps gathered from a plane
__device__ __forceinline__ double bilinear_inside_at(const double* __restrict__ p, int W, int H, double x, double y) {
    const int x0 = (int)x, y0 = (int)y;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    return bilinear_inside(p[y0 * W + x0], p[y1 * W + x0], p[y0 * W + x1], p[y1 * W + x1], x - x0, y - y0);
}

// Samples of the Laplacian-noise guard (api.hip: LapGuard): estLaplacianNoise (src/OpticalFlow.cpp:594-639) averages
// d = |Im1 - warpIm2| over its VALID samples, those in (0, 1e6); one sample of at least thr = lap_wit_threshold() is a WITNESS
// that this mean is not below 1e-20.  `sampled`: a condition of the caller's in front of the comparison (k_flow_system).
__device__ __forceinline__ bool lap_valid(double d) { return d > 0 && d < 1000000; }
__device__ __forceinline__ bool lap_witness(double d, double thr, bool sampled = true) {
    return sampled && d >= thr && d < 1000000;
}
// thousands of stores to one word are not free: on a grid of more than 256 blocks one block in sixteen samples
__device__ __forceinline__ bool lap_one_in_sixteen(int tbx, int tby) { return ((tbx + 5 * tby) & 15) == 0; }
__device__ __forceinline__ bool lap_samples_here(int nblocks, int tbx, int tby) {
    return nblocks <= 256 || lap_one_in_sixteen(tbx, tby);
}

// ------------------------------------------------------------------------------------------------
// layout conversion (entry / exit of the call): HWC interleaved <-> planar
// ------------------------------------------------------------------------------------------------
__global__ void k_hwc_to_planar(const double* __restrict__ hwc, double* __restrict__ planar, int H, int W, int C) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j, np = (size_t)H * W;
    hwc += blockIdx.z * np * C;  // blockIdx.z: the frame of a batch (frames are contiguous on both sides)
    planar += blockIdx.z * np * C;
    for (int k = 0; k < C; k++) planar[k * np + o] = hwc[o * C + k];
}

// uint8 frames (what the caller decodes from JPEG): the caller's `im.astype(float) / 255.` (OpticalFlowCalculation.py:69-70)
// is done on load -- one IEEE fp64 division per sample, hence the same bits -- so 1 byte per sample crosses PCIe, not 8.
__global__ void k_hwc_u8_to_planar(const unsigned char* __restrict__ hwc, double* __restrict__ planar, int H, int W,
                                   int C) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j, np = (size_t)H * W;
    hwc += blockIdx.z * np * C;  // blockIdx.z: the frame of a batch
    planar += blockIdx.z * np * C;
    for (int k = 0; k < C; k++) planar[k * np + o] = (double)hwc[o * C + k] / 255.0;
}

__global__ void k_planar_to_hwc(const double* __restrict__ planar, double* __restrict__ hwc, int H, int W, int C) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j, np = (size_t)H * W;
    for (int k = 0; k < C; k++) hwc[o * C + k] = planar[k * np + o];
}

// Strided device tensors (include/papof.h: papof_tensor; papof_flow_batch_tensor) in and out.  One lane per element of the
// planar side, 64-bit indices throughout; strides are in elements along (frame | pair, row, column, channel | component).
__device__ __forceinline__ double tensor_load(const void* p, int dtype, long long o) {
    if (dtype == PAPOF_DTYPE_U8) return (double)static_cast<const unsigned char*>(p)[o] / 255.0;  // as k_hwc_u8_to_planar
    if (dtype == PAPOF_DTYPE_F32) return (double)static_cast<const float*>(p)[o];                 // exact widening
    return static_cast<const double*>(p)[o];
}

// frames -> the planar fp64 level-0 array [frame][channel][row][col] of the batch chain.  pairs != 0: frame 2p is a's frame p,
// frame 2p + 1 is b's frame p (the interleaving of fstep = 2); else frame f is a's frame f.
__global__ __launch_bounds__(256) void k_ingest_frames(const papof_tensor a, const papof_tensor b, int pairs,
                                                       double* __restrict__ planar, long long H, long long W, long long C,
                                                       long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long np = H * W, f = i / (np * C), r = i - f * np * C, c = r / np, px = r - c * np, row = px / W,
                    col = px - row * W;
    const bool second = pairs && (f & 1);
    const long long fi = pairs ? f >> 1 : f;
    const long long o = fi * (second ? b.stride[0] : a.stride[0]) + row * (second ? b.stride[1] : a.stride[1]) +
                        col * (second ? b.stride[2] : a.stride[2]) + c * (second ? b.stride[3] : a.stride[3]);
    planar[i] = tensor_load(second ? b.data : a.data, second ? b.dtype : a.dtype, o);
}

// The caller's initial flow (include/papof.h: papof_flow_batch_tensor_init): a component is refused when it is not a number
// of magnitude <= kInitMax (NaN and +-Inf fail the comparison).  k_init_check reads a strided float32 / float64 tensor
// (pair, row, column, component) where it is and raises *flag; k_init_sanitize writes +0.0 over every refused value of the
// ingested planar flow, so that no refused value reaches a sampler even if a refusal were missed.
constexpr double kInitMax = 1e6;
__device__ __forceinline__ bool init_refused(double x) { return !(fabs(x) <= kInitMax); }

__global__ __launch_bounds__(256) void k_init_check(const papof_tensor t, long long H, long long W, long long total,
                                                    unsigned* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long np = H * W, p = i / (np * 2), r = i - p * np * 2, c = r / np, px = r - c * np, row = px / W,
                    col = px - row * W;
    const long long o = p * t.stride[0] + row * t.stride[1] + col * t.stride[2] + c * t.stride[3];
    if (init_refused(tensor_load(t.data, t.dtype, o))) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void k_init_sanitize(double* __restrict__ planar, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (init_refused(planar[i])) planar[i] = 0.0;
}

// the chain's results -> a strided float32 / float64 tensor.  comp_major: src is [pair][K][H * W] (the flow: K = 2, u then v);
// else [pair][H * W][K] (warpI2, HWC).  The destination is (pair, row, column, K).
__global__ __launch_bounds__(256) void k_emit_outputs(const double* __restrict__ src, const papof_tensor dst, int comp_major,
                                                      long long H, long long W, long long K, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long np = H * W, p = i / (np * K), r = i - p * np * K;
    const long long k = comp_major ? r / np : r % K, px = comp_major ? r - k * np : r / K, row = px / W, col = px - row * W;
    const long long o = p * dst.stride[0] + row * dst.stride[1] + col * dst.stride[2] + k * dst.stride[3];
    const double v = src[i];
    if (dst.dtype == PAPOF_DTYPE_F32)
        static_cast<float*>(dst.data)[o] = (float)v;
    else
        static_cast<double*>(dst.data)[o] = v;
}

// Forward-backward consistency (Sundaram, Brox, Keutzer 2010; papof_fb_check_tensor, papof_flow_batch_tensor_fb).
// blockIdx.y = pair * 2 + direction; direction 0 follows the forward flow f = fw into the backward flow b = bw, direction
// 1 the reverse, on the pixels of the pair's second frame.  For pixel (r, x): (u, v) = f at the pixel, (X, Y) = (x + u, r + v),
// (bu, bv) = b sampled bilinearly at (X, Y) by the reference's rule (sampler.h: sample_flow), and the pixel is occluded
// where (X, Y) leaves [0, W - 1] x [0, H - 1] or fails sampler.h's fb_passes -- NaN counts as occluded.  f is loaded at the
// pixel, not sampled: a bilinear sample there would differ where a neighbour is not finite.  fp64 throughout, no contraction
// (the library's -ffp-contract=off).  mask: 1 byte per (pair, row, column, direction).  A block is a 64 x 4 tile of one
// direction of one pair: the four taps of neighbouring pixels share lines.
constexpr int kFbTX = 64, kFbTY = 4;
__global__ __launch_bounds__(kFbTX * kFbTY) void k_fb_check(const papof_tensor fw, const papof_tensor bw, const papof_tensor mask,
                                                         int H, int W, double a1, double a2) {
    const int tx = (W + kFbTX - 1) / kFbTX;
    const int x = (int)(blockIdx.x % tx) * kFbTX + threadIdx.x, r = (int)(blockIdx.x / tx) * kFbTY + threadIdx.y;
    if (x >= W || r >= H) return;
    const long long p = blockIdx.y >> 1;
    const int dir = blockIdx.y & 1;
    const papof_tensor& f = dir ? bw : fw;
    const papof_tensor& b = dir ? fw : bw;
    const long long of = p * f.stride[0] + r * f.stride[1] + x * f.stride[2];
    const double u = load_flow(f, of), v = load_flow(f, of + f.stride[3]);
    const double X = (double)x + u, Y = (double)r + v;
    bool occluded = true;
    if (X >= 0 && X <= (double)(W - 1) && Y >= 0 && Y <= (double)(H - 1)) {  // (false for a NaN: occluded)
        double bu, bv;
        sample_flow(b, p * b.stride[0], taps_at(X, Y, H, W), bu, bv);
        occluded = !fb_passes(u, v, bu, bv, a1, a2);
    }
    static_cast<unsigned char*>(mask.data)[p * mask.stride[0] + r * mask.stride[1] + x * mask.stride[2] + dir * mask.stride[3]] =
        occluded ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// separable correlation with clamped borders: src/ImageProcessing.h:259-279 (h), :350-369 (v).
// Accumulation into a zeroed destination, taps in order l = -fsize..fsize.
// ------------------------------------------------------------------------------------------------
__global__ void k_filter_h(const double* __restrict__ src, double* __restrict__ dst, int H, int W, Taps f, Rect rc) {
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t np = (size_t)H * W;
    const double* row = src + blockIdx.z * np + (size_t)i * W;
    dst[blockIdx.z * np + (size_t)i * W + j] = tap_sum(f, [&](int l) { return row[clampi(j + l, W)]; }, f.fsize);
}

__global__ void k_filter_v(const double* __restrict__ src, double* __restrict__ dst, int H, int W, Taps f, Rect rc) {
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t np = (size_t)H * W;
    const double* p = src + blockIdx.z * np + j;
    dst[blockIdx.z * np + (size_t)i * W + j] = tap_sum(f, [&](int l) { return p[(size_t)clampi(i + l, H) * W]; }, f.fsize);
}

// Both passes of a separable filter in ONE kernel (h pass into LDS, v pass out of it): the operations and their order
// are those of k_filter_h followed by k_filter_v -- the v pass reads the h-filtered values of the rows clamp(i + l), here
// rows of the block's LDS image -- so the bits are the same, but the h-filtered plane never goes to HBM (2.4 instead of
// 4 plane transfers at half-width 3).  A block owns kHvRows rows x 64 columns of one plane.
#ifndef PAPOF_V_HVROWS
#define PAPOF_V_HVROWS 64  // in-pair A/B (round 2): 16 / 32 / 64 / 96 / 128 rows: 10.99 / 10.98 / 10.92 / 10.91 / 10.94 ms per 1080p pair
#endif
constexpr int kHvRows = PAPOF_V_HVROWS, kHvMaxF = 4;
template <int F>  // F = the half-width of both passes as a compile-time constant (fully unrolled tap loops), or -1: run time
__global__ __launch_bounds__(256) void k_filter_hv(const double* __restrict__ src, double* __restrict__ dst, int H, int W,
                                                   Taps fh, Taps fv) {
    __shared__ double hs[kHvRows + 2 * kHvMaxF][BX];
    const int j = blockIdx.x * BX + threadIdx.x, i0 = blockIdx.y * kHvRows;
    const int f = F >= 0 ? F : fv.fsize, fx = F >= 0 ? F : fh.fsize;
    const size_t np = (size_t)H * W;
    const double* plane = src + blockIdx.z * np;
    if (j < W) {
        for (int r = threadIdx.y; r < kHvRows + 2 * f; r += BY) {
            const double* row = plane + (size_t)clampi(i0 + r - f, H) * W;
            hs[r][threadIdx.x] = tap_sum<F>(fh, [&](int l) { return row[clampi(j + l, W)]; }, fx);
        }
    }
    __syncthreads();
    if (j >= W) return;
    for (int r = threadIdx.y; r < kHvRows; r += BY) {
        const int i = i0 + r;
        if (i >= H) break;
        dst[blockIdx.z * np + (size_t)i * W + j] = tap_sum<F>(fv, [&](int l) { return hs[r + l + f][threadIdx.x]; }, f);
    }
}

// The same two passes with the source tile (halo included) staged in LDS first: every input value is loaded once, by a
// coalesced row read, instead of 2F+1 times through clamped indices (the kernel above is bound by its L1 traffic and index
// arithmetic).  Same operations in the same order: same bits.
#ifndef PAPOF_V_HVSTAGED
#define PAPOF_V_HVSTAGED 1  // same-box A/B (round 3, ms per 1080p pair): 10.536 without, 10.507 with 16-row tiles, 10.61 with 32
#endif
#ifndef PAPOF_V_HVSROWS
#define PAPOF_V_HVSROWS 16
#endif
constexpr int kHvsRows = PAPOF_V_HVSROWS;
template <int F>
__global__ __launch_bounds__(256) void k_filter_hv_staged(const double* __restrict__ src, double* __restrict__ dst, int H,
                                                          int W, Taps fh, Taps fv) {
    __shared__ double raw[kHvsRows + 2 * F][BX + 2 * F];
    __shared__ double hs[kHvsRows + 2 * F][BX];
    int tx, ty;
    if (!xcd_tile((W + BX - 1) / BX, (H + kHvsRows - 1) / kHvsRows, tx, ty)) return;  // whole workgroup, before any barrier
    const int j0 = tx * BX, i0 = ty * kHvsRows;
    const size_t np = (size_t)H * W;
    const double* plane = src + blockIdx.z * np;
    constexpr int kCells = (kHvsRows + 2 * F) * (BX + 2 * F);
    for (int c = threadIdx.y * BX + threadIdx.x; c < kCells; c += BX * BY) {
        const int r = c / (BX + 2 * F), cc = c - r * (BX + 2 * F);
        raw[r][cc] = plane[(size_t)clampi(i0 + r - F, H) * W + clampi(j0 + cc - F, W)];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < kHvsRows + 2 * F; r += BY) {
        hs[r][threadIdx.x] = tap_sum<F>(fh, [&](int l) { return raw[r][threadIdx.x + F + l]; });
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    if (j >= W) return;
    for (int r = threadIdx.y; r < kHvsRows; r += BY) {
        const int i = i0 + r;
        if (i >= H) break;
        dst[blockIdx.z * np + (size_t)i * W + j] = tap_sum<F>(fv, [&](int l) { return hs[r + l + F][threadIdx.x]; });
    }
}

// ------------------------------------------------------------------------------------------------
// bilinear sampling: src/ImageProcessing.h:138-157.  Integer part by truncation toward zero,
// fraction clamped to [0,1], taps visited x-offset outer / y-offset inner and ACCUMULATED from 0.
// The four weights are shared by all planes of a pixel.
// ------------------------------------------------------------------------------------------------
struct BilinearTaps {
    int o[4];     // plane offsets of the 4 taps in visiting order
    double s[4];  // their weights
};
struct BilinearAxis {
    int c[2];  // the two cells along one axis, clamped
    double d;  // the fraction, clamped to [0, 1]
};

__host__ __device__ __forceinline__ BilinearAxis bilinear_axis(int n, double x) {
    BilinearAxis a;
    const int xx = (int)x;
    double dx = x - xx;
    dx = dx > 1 ? 1.0 : dx;
    dx = dx < 0 ? 0.0 : dx;
    a.d = dx;
    a.c[0] = clampi(xx, n);
    a.c[1] = clampi(xx + 1, n);
    return a;
}

__device__ __forceinline__ BilinearTaps bilinear_taps(int W, int H, double x, double y) {
    BilinearTaps b;
    const BilinearAxis ax = bilinear_axis(W, x), ay = bilinear_axis(H, y);
#pragma unroll
    for (int m = 0; m <= 1; m++)
#pragma unroll
        for (int n = 0; n <= 1; n++) {
            b.o[m * 2 + n] = ay.c[n] * W + ax.c[m];
            b.s[m * 2 + n] = fabs((double)(1 - m) - ax.d) * fabs((double)(1 - n) - ay.d);
        }
    return b;
}

// the accumulate statement; at(t) is the operand of tap t = 2 m + n, the cell (x_m, y_n)
template <class At>
__device__ __forceinline__ double bilinear_sum(const BilinearTaps& b, At at) {
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 4; t++) acc += at(t) * b.s[t];
    return acc;
}
__device__ __forceinline__ double bilinear_apply(const double* __restrict__ p, const BilinearTaps& b) {
    return bilinear_sum(b, [&](int t) { return p[b.o[t]]; });
}

// ImageProcessing::ResizeImage, src/ImageProcessing.h:214-253 (both overloads: xr == yr for the ratio form).
// Optional post-scale = Image::Multiplywith (src/Image.h:1841-1850) for the flow up-sampling of
// src/OpticalFlow.cpp:809-812.
// the position of level pixel j in its source, along one axis (:226-227)
__host__ __device__ __forceinline__ double resize_pos(int j, double r) { return (double)(j + 1) / r - 1; }

__global__ void k_resize(const double* __restrict__ src, double* __restrict__ dst, int sh, int sw, int dh, int dw,
                         double xr, double yr, int use_post, double post, Rect rc, unsigned long long* stamp) {
    stamp_now(stamp);
    int tbx, tby;  // a contiguous run of blocks per XCD (xcd_tile): the four taps of neighbouring rows meet in one L2
    if (!xcd_tile((rc.x1 - rc.x0 + BX - 1) / BX, (rc.y1 - rc.y0 + BY - 1) / BY, tbx, tby)) return;
    const int j = rc.x0 + tbx * BX + threadIdx.x, i = rc.y0 + tby * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const BilinearTaps b = bilinear_taps(sw, sh, resize_pos(j, xr), resize_pos(i, yr));
    double r = bilinear_apply(src + blockIdx.z * (size_t)sh * sw, b);
    if (use_post) r *= post;
    dst[blockIdx.z * (size_t)dh * dw + (size_t)i * dw + j] = r;
}

// One pyramid level in ONE launch: k_filter_hv_staged<F> followed by k_resize, without the smoothed source plane between
// them (a level keeps 10-32 % of its source's pixels: most of that plane was written, read back once and never sampled).
// A block owns a kSrT x kSrT tile of level pixels of one plane.  The taps of its pixels lie in the source cells
// [u_lo, u_hi] x [v_lo, v_hi] (bilinear_axis() is monotone in the pixel, so the tile's first and last pixel bound them);
// that rectangle grown by F is staged in LDS by clamped row reads, the h pass runs on its rows at the 2 kSrT tap COLUMNS of
// the tile only, and each pixel takes the v pass of its four taps out of LDS and blends them.  The smoothed value at the tap
// (v, u) is tap_sum<F>(fv, l -> h[clamp(v + l)][u]) with h[r][u] = tap_sum<F>(fh, l -> src[r][clamp(u + l)]) -- the
// operations and the order of the two kernels; a value two taps share is identified by its clamped row and column.
// nx, ny: the LDS image's pitch and rows, the largest footprint of any tile (smooth_resize() below walks the same expressions).
constexpr int kSrT = 16;
template <int F>
__global__ __launch_bounds__(256) void k_smooth_resize(const double* __restrict__ src, double* __restrict__ dst, int sh,
                                                       int sw, int dh, int dw, double xr, double yr, Taps fh, Taps fv,
                                                       int nx, int ny) {
    extern __shared__ __align__(16) double sr_lds[];
    int tx, ty;
    if (!xcd_tile((dw + kSrT - 1) / kSrT, (dh + kSrT - 1) / kSrT, tx, ty)) return;  // whole workgroup, before any barrier
    const int j0 = tx * kSrT, i0 = ty * kSrT;
    const int j1 = min(j0 + kSrT, dw) - 1, i1 = min(i0 + kSrT, dh) - 1;  // the tile's last pixel
    // the positions of the tile's kSrT columns and kSrT rows in the source: one division each, by 2 kSrT threads for all
    // (a division per thread and use -- the corners, the h pass, the blend -- was most of the kernel's arithmetic)
    __shared__ double pos[2][kSrT];
    const int t = threadIdx.y * BX + threadIdx.x;
    if (t < kSrT)
        pos[0][t] = resize_pos(j0 + t, xr);
    else if (t < 2 * kSrT)
        pos[1][t - kSrT] = resize_pos(i0 + t - kSrT, yr);
    __syncthreads();
    const int u_lo = bilinear_axis(sw, pos[0][0]).c[0], u_hi = bilinear_axis(sw, pos[0][j1 - j0]).c[1];
    const int v_lo = bilinear_axis(sh, pos[1][0]).c[0], v_hi = bilinear_axis(sh, pos[1][i1 - i0]).c[1];
    const int nxa = u_hi - u_lo + 1 + 2 * F, nya = v_hi - v_lo + 1 + 2 * F;
    if (nxa > nx || nya > ny) return;  // (never: nx, ny are the maxima of these; nothing is written outside the LDS image)
    double* const raw = sr_lds;                  // [ny][nx]: source cell (clamp(v_lo - F + r), clamp(u_lo - F + c))
    double* const hs = sr_lds + (size_t)ny * nx;  // [ny][2][kSrT]: the h pass at the tile's tap columns x_m of its pixels
    const double* plane = src + blockIdx.z * (size_t)sh * sw;
    for (int r = threadIdx.y; r < nya; r += BY) {
        const double* row = plane + (size_t)clampi(v_lo - F + r, sh) * sw;
        for (int c = threadIdx.x; c < nxa; c += BX) raw[r * nx + c] = row[clampi(u_lo - F + c, sw)];
    }
    __syncthreads();
    {
        const int slot = t % (2 * kSrT), m = slot / kSrT, jj = j0 + slot % kSrT;
        if (jj <= j1) {
            const BilinearAxis ax = bilinear_axis(sw, pos[0][jj - j0]);
            const int cu = (m == 0 ? ax.c[0] : ax.c[1]) - u_lo + F;
            for (int r = t / (2 * kSrT); r < nya; r += BX * BY / (2 * kSrT)) {
                const double* at = raw + r * nx + cu;
                hs[r * (2 * kSrT) + slot] = tap_sum<F>(fh, [&](int l) { return at[l]; });
            }
        }
    }
    __syncthreads();
    const int ox = t % kSrT, j = j0 + ox, i = i0 + t / kSrT;
    if (j > j1 || i > i1) return;
    const double x = pos[0][j - j0], y = pos[1][i - i0];
    const BilinearAxis ay = bilinear_axis(sh, y);
    const BilinearTaps b = bilinear_taps(sw, sh, x, y);
    dst[blockIdx.z * (size_t)dh * dw + (size_t)i * dw + j] = bilinear_sum(b, [&](int k) {  // tap k = 2 m + n: (x_m, y_n)
        const double* at = hs + (ay.c[k % 2] - v_lo + F) * (2 * kSrT) + (k / 2) * kSrT + ox;
        return tap_sum<F>(fv, [&](int l) { return at[l * (2 * kSrT)]; });
    });
}

// ------------------------------------------------------------------------------------------------
// OpticalFlow::im2feature, src/OpticalFlow.cpp:911-961 (3-channel branch :934-955, 1-channel :918-933);
// desaturate src/Image.h:1461-1480 with colorType RGB; 5-point derivative taps {1,-8,0,8,-1}/12
// (src/Image.h:987-992) applied to the gray image with clamped borders.  Gray values of the stencil
// neighbours are recomputed (same three-term expression => same bits) instead of staged.
// ------------------------------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ double gray_at(const double* __restrict__ im, size_t np, size_t o) {
    if (C == 3) return im[o] * .299 + im[np + o] * .587 + im[2 * np + o] * .114;
    return im[o];
}

template <int C>
__global__ void k_im2feature(const double* __restrict__ im, double* __restrict__ feat, int H, int W, Taps d) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t np = (size_t)H * W, o = (size_t)i * W + j;
    double gx = 0.0, gy = 0.0;
#pragma unroll
    for (int l = -2; l <= 2; l++) gx += gray_at<C>(im, np, (size_t)i * W + clampi(j + l, W)) * d.t[l + 2];
#pragma unroll
    for (int l = -2; l <= 2; l++) gy += gray_at<C>(im, np, (size_t)clampi(i + l, H) * W + j) * d.t[l + 2];
    feat[o] = gray_at<C>(im, np, o);
    feat[np + o] = gx;
    feat[2 * np + o] = gy;
    if (C == 3) {
        feat[3 * np + o] = im[np + o] - im[o];
        feat[4 * np + o] = im[np + o] - im[2 * np + o];
    }
}

// The same through an LDS tile of gray values (one-GPU path): a block owns kFeatRows rows x 64 columns, evaluates gray
// ONCE per cell of the tile grown by the 5-tap filters' reach (same expression: same bits) and takes the two derivative
// sums out of LDS in the same order -- 4 instead of 27 cached loads per pixel.
#ifndef PAPOF_V_FEATROWS
#define PAPOF_V_FEATROWS 16
#endif
constexpr int kFeatRows = PAPOF_V_FEATROWS;
template <int C, bool BATCH = false>
__global__ __launch_bounds__(256) void k_im2feature_tiled(const double* __restrict__ im, double* __restrict__ feat, int H,
                                                          int W, Taps d, unsigned* __restrict__ nz, unsigned mark,
                                                          size_t b_im, size_t b_feat, size_t b_nz) {
    // nz (may be null): nz[k] is set when feature channel k has a non-zero value anywhere -- a channel that is all zero in BOTH
    // frames has no valid sample for estLaplacianNoise (every |Im1 - warpIm2| is exactly 0), so its LapPara is 0.001 whatever
    // the flow (api.hip: LapGuard).  One ballot per wave, at most one store per wave and channel.
    __shared__ double g[kFeatRows + 4][BX + 4];
    int tx, ty;
    if (!xcd_tile((W + BX - 1) / BX, (H + kFeatRows - 1) / kFeatRows, tx, ty)) return;  // whole workgroup, before any barrier
    const int j0 = tx * BX, i0 = ty * kFeatRows;
    const size_t np = (size_t)H * W;
    if (BATCH) {  // blockIdx.y: the frame of a batch (common.h: BatchK)
        im += blockIdx.y * b_im;
        feat += blockIdx.y * b_feat;
        if (nz != nullptr) nz += blockIdx.y * b_nz;
    }
    for (int c = threadIdx.y * BX + threadIdx.x; c < (kFeatRows + 4) * (BX + 4); c += BX * BY) {
        const int r = c / (BX + 4), cc = c - r * (BX + 4);
        g[r][cc] = gray_at<C>(im, np, (size_t)clampi(i0 + r - 2, H) * W + clampi(j0 + cc - 2, W));
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    bool any[5] = {false, false, false, false, false};
    if (j < W) {
        for (int r = threadIdx.y; r < kFeatRows; r += BY) {
            const int i = i0 + r;
            if (i >= H) break;
            const size_t o = (size_t)i * W + j;
            double gx = 0.0, gy = 0.0;
#pragma unroll
            for (int l = -2; l <= 2; l++) gx += g[r + 2][threadIdx.x + 2 + l] * d.t[l + 2];
#pragma unroll
            for (int l = -2; l <= 2; l++) gy += g[r + 2 + l][threadIdx.x + 2] * d.t[l + 2];
            const double f0 = g[r + 2][threadIdx.x + 2];
            feat[o] = f0;
            feat[np + o] = gx;
            feat[2 * np + o] = gy;
            any[0] |= f0 != 0.0;
            any[1] |= gx != 0.0;
            any[2] |= gy != 0.0;
            if (C == 3) {
                const double gg = im[np + o];
                const double f3 = gg - im[o], f4 = gg - im[2 * np + o];
                feat[3 * np + o] = f3;
                feat[4 * np + o] = f4;
                any[3] |= f3 != 0.0;
                any[4] |= f4 != 0.0;
            }
        }
    }
    if (nz != nullptr) {
#pragma unroll
        for (int k = 0; k < (C == 3 ? 5 : 3); k++)
            if (__ballot(any[k]) != 0ull && threadIdx.x == 0) nz[k] = mark;
    }
}

// The three derivative planes of the final bicubic warp in one launch (Image::warpImageBicubicRef, src/Image.h:2590-2594:
// imfilter_h, imfilter_v, imfilter_v of the first with {-.5, 0, .5}): gx, gy as k_filter_h / k_filter_v compute them,
// gxy = the v pass over gx, whose three rows are recomputed here with the h pass's own operations (same bits).
// The three expressions at one pixel, each stated once: at(dr, dc) is the image at the pixel's clamped neighbour dr rows down and
// dc columns right.  The zero middle tap is multiplied and added like the others, and every sum starts from 0.0 (tap_sum).
template <class At>
__device__ __forceinline__ double central3_h(const Taps& c3, At at) {  // imfilter_h
    return tap_sum<1>(c3, [&](int l) { return at(0, l); });
}
template <class At>
__device__ __forceinline__ double central3_v(const Taps& c3, At at) {  // imfilter_v
    return tap_sum<1>(c3, [&](int l) { return at(l, 0); });
}
template <class HRow>
__device__ __forceinline__ double central3_hv(const Taps& c3, HRow hrow) {  // imfilter_v of imfilter_h; hrow(l): central3_h l rows down
    return tap_sum<1>(c3, [&](int l) { return hrow(l); });
}

__global__ void k_central3_all(const double* __restrict__ src, double* __restrict__ gx, double* __restrict__ gy,
                               double* __restrict__ gxy, int H, int W, Taps c3) {
    int tbx, tby;
    if (!xcd_tile((W + BX - 1) / BX, (H + BY - 1) / BY, tbx, tby)) return;
    const int j = tbx * BX + threadIdx.x, i = tby * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t np = (size_t)H * W;
    const double* p = src + blockIdx.z * np;
    const auto at = [&](int dr, int dc) { return p[(size_t)clampi(i + dr, H) * W + clampi(j + dc, W)]; };
    const size_t o = blockIdx.z * np + (size_t)i * W + j;
    gx[o] = central3_h(c3, at);
    gy[o] = central3_v(c3, at);
    gxy[o] = central3_hv(c3, [&](int l) { return central3_h(c3, [&](int, int dc) { return at(l, dc); }); });  // its three h rows recomputed
}

// ------------------------------------------------------------------------------------------------
// OpticalFlow::warpFL -> ImageProcessing::warpImage, src/ImageProcessing.h:483-503.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void warp_pixel(const double* __restrict__ im1, const double* __restrict__ im2,
                                           double* __restrict__ out, double fx, double fy, int i, int j, int H,
                                           int W, int planes) {
    const size_t np = (size_t)H * W, o = (size_t)i * W + j;
    const double y = i + fy;
    const double x = j + fx;
    if (leaves_image(x, y, W, H)) {
        for (int k = 0; k < planes; k++) out[k * np + o] = im1[k * np + o];
        return;
    }
    for (int k = 0; k < planes; k++) out[k * np + o] = bilinear_inside_at(im2 + k * np, W, H, x, y);
}

__global__ void k_warp(const double* __restrict__ im1, const double* __restrict__ im2, const double* __restrict__ vx,
                       const double* __restrict__ vy, double* __restrict__ out, int H, int W, int planes, Rect rc,
                       unsigned long long* stamp) {
    stamp_now(stamp);
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t o = (size_t)i * W + j;
    warp_pixel(im1, im2, out, vx[o], vy[o], i, j, H, W, planes);
}

// ------------------------------------------------------------------------------------------------
// Second half of OpticalFlow::getDxs (src/OpticalFlow.cpp:89-97) for the warped frame: vertical pass of
// the 5-tap smoothing, then Im = Im1s*0.4 + Im2s*0.6 (Multiplywith :92, Add(...,0.6) :93) and
// imdt = Im2s - Im1s (:97).  Im1s (smoothed frame 1) is constant within a level and computed once.
// ------------------------------------------------------------------------------------------------
__global__ void k_smooth_v_blend(const double* __restrict__ tmp, const double* __restrict__ im1s,
                                 double* __restrict__ blend, double* __restrict__ imdt, int H, int W, Taps g, Rect rc) {
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t np = (size_t)H * W, o = blockIdx.z * np + (size_t)i * W + j;
    const double* p = tmp + blockIdx.z * np + j;
    const double s2 = tap_sum<2>(g, [&](int l) { return p[(size_t)clampi(i + l, H) * W]; });
    blend_imdt(im1s[o], s2, blend[o], imdt[o]);
}

// Both passes of the 5-tap smoothing of the warped frame + blend + imdt in ONE kernel (one-GPU path): a block owns
// kFuseRows rows x 64 columns of one plane, filters kFuseRows + 4 rows horizontally into LDS (same taps, same order as
// k_filter_h), then runs the vertical pass out of LDS (same order as k_smooth_v_blend).  The horizontally filtered
// plane never goes to HBM: 4 instead of 6 plane transfers per channel, same bits.
constexpr int kFuseRows = 16;
__global__ __launch_bounds__(256) void k_smooth_hv_blend(const double* __restrict__ warp,
                                                         const double* __restrict__ im1s,
                                                         double* __restrict__ blend, double* __restrict__ imdt, int H,
                                                         int W, Taps g, unsigned long long* stamp, int row0, int row1) {
    __shared__ double hs[kFuseRows + 4][BX];
    stamp_now(stamp);
    // rows row0 .. row1-1 are written (a strip of the plane; the whole plane otherwise)
    const int j = blockIdx.x * BX + threadIdx.x, i0 = row0 + blockIdx.y * kFuseRows;
    const size_t np = (size_t)H * W;
    const double* src = warp + blockIdx.z * np;
    if (j < W) {
        for (int r = threadIdx.y; r < kFuseRows + 4; r += BY) {
            const double* row = src + (size_t)clampi(i0 + r - 2, H) * W;
            hs[r][threadIdx.x] = tap_sum<2>(g, [&](int l) { return row[clampi(j + l, W)]; });
        }
    }
    __syncthreads();
    if (j >= W) return;
    for (int r = threadIdx.y; r < kFuseRows; r += BY) {
        const int i = i0 + r;
        if (i >= row1) break;
        const size_t o = blockIdx.z * np + (size_t)i * W + j;
        const double s2 = tap_sum<2>(g, [&](int l) { return hs[r + l + 2][threadIdx.x]; });
        blend_imdt(im1s[o], s2, blend[o], imdt[o]);
    }
}

// The same with the WARP folded in (one-GPU default path): the warped frame 2 (OpticalFlow::warpFL, src/OpticalFlow.cpp:
// 154-159, 516) is read by nobody but this smoothing, so it is never written to HBM -- a block evaluates warp_value() for
// every cell of its tile grown by the filters' reach (clamped coordinates, i.e. exactly the cells k_smooth_hv_blend would
// have loaded from the warped plane: same bits), keeps them in LDS, and runs both passes out of LDS.  Saves the plane's
// round trip (16 B x channels per pixel and iteration) and the warp kernel at the start of every level.
__device__ __forceinline__ double warp_value(const double* __restrict__ im1, const double* __restrict__ im2, double fx,
                                             double fy, int i, int j, int H, int W) {  // one plane of warp_pixel()
    const double y = i + fy;
    const double x = j + fx;
    if (leaves_image(x, y, W, H)) return im1[(size_t)i * W + j];
    return bilinear_inside_at(im2, W, H, x, y);
}
#ifndef PAPOF_V_WSROWS
#define PAPOF_V_WSROWS 16
#endif
#ifndef PAPOF_V_WSBATCH
#define PAPOF_V_WSBATCH 3
#endif
constexpr int kWsBatch = PAPOF_V_WSBATCH;  // cells per thread whose gathers are in flight together (k_warp_smooth_blend)
constexpr int kWsRows = PAPOF_V_WSROWS;  // rows per block of the warp-folded smoothing (32 rows: 0.13 ms per 1080p pair slower)
__global__ __launch_bounds__(256) void k_warp_smooth_blend(const double* __restrict__ im1, const double* __restrict__ im2,
                                                           const double* __restrict__ u, const double* __restrict__ v,
                                                           const double* __restrict__ im1s, double* __restrict__ blend,
                                                           double* __restrict__ imdt, int H, int W, Taps g,
                                                           unsigned long long* stamp, unsigned* __restrict__ wit,
                                                           double wit_thr, unsigned mark, double* __restrict__ phi_out) {
    // one channel per block (blockIdx.z).  [Also measured: one block looping over the channels with the sampling taps of its
    // cells kept in registers -- 0.2 ms per 1080p pair SLOWER (register pressure, ten barriers per block).]
    __shared__ double raw[kWsRows + 4][BX + 4];
    __shared__ double hs[kWsRows + 4][BX];
    stamp_now(stamp);
    const int j0 = blockIdx.x * BX, i0 = blockIdx.y * kWsRows;
    const size_t np = (size_t)H * W;
    const double *p1 = im1 + blockIdx.z * np, *p2 = im2 + blockIdx.z * np;
    // WITNESS for the Laplacian-noise guard (api.hip: LapGuard): estLaplacianNoise (src/OpticalFlow.cpp:594-639) averages
    // |Im1 - warpIm2| over its samples in (0, 1e6), and ONE sample of at least wit_thr = 2e-20 x pixels proves that mean is not
    // below 1e-20 (a sum of positives is at least its largest term), i.e. that the guard of :399-400 did not trip.  This kernel
    // evaluates exactly that warp -- frame 2 at the flow the previous outer iteration left -- so the first wave of every
    // block compares 64 cells spread over the tile (their frame-1 values are fetched here, beside the gathers: no latency of
    // their own; halo cells are clamped copies of image pixels, warped as such: as good a sample as any).
    // Where the grid is large, one block in sixteen samples: thousands of stores to one word are not free.
    // A level that is ONE block per channel is checked EXHAUSTIVELY instead (every cell of the tile): on the few-pixel levels of a
    // deep pyramid the flow can leave the image altogether -- every warped value is then frame 1's, no sample is valid and the
    // estimate is the constant 0.001; the block that has seen every pixel says so (kLapNone), which is a proof as well.
    const bool exhaustive = wit != nullptr && gridDim.x == 1u && gridDim.y == 1u;
    bool ex_hit = false, ex_valid = false;
    const bool sampler = wit != nullptr && !exhaustive && threadIdx.y == 0u &&
                         lap_samples_here((int)(gridDim.x * gridDim.y), (int)blockIdx.x, (int)blockIdx.y);
    constexpr int kWitStride = (kWsRows + 4) * (BX + 4) / 64;
    const int wr = (int)(threadIdx.x * kWitStride) / (BX + 4), wc = (int)(threadIdx.x * kWitStride) - wr * (BX + 4);
    double own1 = 0.0;
    if (sampler) own1 = p1[(size_t)clampi(i0 + wr - 2, H) * W + clampi(j0 + wc - 2, W)];
    // The tile's cells (halo of 2 included) are warped in BATCHES of kWsBatch cells per thread: first the flow of every cell of
    // the batch, then all their taps and the 4 x kWsBatch gathers, then the blends -- two dependent memory round trips per
    // batch instead of two per cell (the kernel was bound by those: 130 us at level 0 against ~45 us of HBM traffic).  The
    // expressions are warp_value()'s own: leaves_image() and bilinear_inside().
    constexpr int kCells = (kWsRows + 4) * (BX + 4), kPer = (kCells + BX * BY - 1) / (BX * BY);
    const int tid = threadIdx.y * BX + threadIdx.x;
#pragma unroll
    for (int q0 = 0; q0 < kPer; q0 += kWsBatch) {
        double fx[kWsBatch], fy[kWsBatch], val[kWsBatch][4];
        int off[kWsBatch];
#pragma unroll
        for (int q = 0; q < kWsBatch; q++) {
            const int c = min(tid + (q0 + q) * BX * BY, kCells - 1);  // (a thread beyond the tile repeats the last cell: discarded)
            const int r = c / (BX + 4), cc = c - r * (BX + 4);
            const int i = clampi(i0 + r - 2, H), j = clampi(j0 + cc - 2, W);
            off[q] = i * W + j;
            fx[q] = u[off[q]];
            fy[q] = v[off[q]];
        }
        bool outside[kWsBatch];
#pragma unroll
        for (int q = 0; q < kWsBatch; q++) {
            const int c = min(tid + (q0 + q) * BX * BY, kCells - 1);
            const int r = c / (BX + 4), cc = c - r * (BX + 4);
            const int i = clampi(i0 + r - 2, H), j = clampi(j0 + cc - 2, W);
            double y = i + fy[q], x = j + fx[q];
            outside[q] = leaves_image(x, y, W, H);  // such a pixel takes frame 1's value
            if (outside[q]) {  // (any valid position: its gathers are issued and not used)
                x = j;
                y = i;
            }
            // the gathers of bilinear_inside_at(), issued for the whole batch before the first blend
            const int x0 = (int)x, y0 = (int)y;
            const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
            val[q][0] = p2[y0 * W + x0];  // visiting order of bilinear_apply(): (m, n) = (0,0) (0,1) (1,0) (1,1), tap = (x_m, y_n)
            val[q][1] = p2[y1 * W + x0];
            val[q][2] = p2[y0 * W + x1];
            val[q][3] = p2[y1 * W + x1];
            fx[q] = x - x0;
            fy[q] = y - y0;
        }
#pragma unroll
        for (int q = 0; q < kWsBatch; q++) {
            const int c = tid + (q0 + q) * BX * BY;
            if (c >= kCells) continue;
            const int r = c / (BX + 4), cc = c - r * (BX + 4);
            const double res =
                outside[q] ? p1[off[q]] : bilinear_inside(val[q][0], val[q][1], val[q][2], val[q][3], fx[q], fy[q]);
            raw[r][cc] = res;
            if (exhaustive) {
                const double d = fabs(p1[off[q]] - res);
                ex_valid = ex_valid || lap_valid(d);
                ex_hit = ex_hit || lap_witness(d, wit_thr);
            }
        }
    }
    __syncthreads();
    if (exhaustive) {  // (block-uniform)
        const int any_hit = __syncthreads_or(ex_hit ? 1 : 0), any_valid = __syncthreads_or(ex_valid ? 1 : 0);
        if (tid == 0 && (any_hit || !any_valid)) wit[blockIdx.z] = any_hit ? mark : (mark ^ kLapNone);
    }
    if (sampler) {
        const double d = fabs(own1 - raw[wr][wc]);
        const unsigned long long hits = __ballot(lap_witness(d, wit_thr));
        if (hits != 0ull && threadIdx.x == 0u) wit[blockIdx.z] = mark;
    }
    for (int r = threadIdx.y; r < kWsRows + 4; r += BY) {
        hs[r][threadIdx.x] = tap_sum<2>(g, [&](int l) { return raw[r][threadIdx.x + 2 + l]; });
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    if (j >= W) return;
    for (int r = threadIdx.y; r < kWsRows; r += BY) {
        const int i = i0 + r;
        if (i >= H) break;
        const size_t o = blockIdx.z * np + (size_t)i * W + j;
        const double s2 = tap_sum<2>(g, [&](int l) { return hs[r + l + 2][threadIdx.x]; });
        blend_imdt(im1s[o], s2, blend[o], imdt[o]);
        // phi of the flow this outer iteration starts from (no increment), by the blocks of channel 0 -- no launch of its own,
        // and the update kernel is spared the scattered reads of its neighbours' increments
        if (phi_out != nullptr && blockIdx.z == 0) phi_out[(size_t)i * W + j] = phi_at(u, v, i, j, H, W);
    }
}

// index (in doubles) of cell (i, j) in an SOR operand plane.  Skew mode: paired planes, (phi,xy) (a1,a2) (b1,b2)
// (du,dv) interleaved, cell (i, j) at (i + j + qt) * hp + (i + rt) -- see common.h.
struct SkewIdx {
    int hp, qt, rt;        // coefficient planes
    int nb, npos_d;        // (du, dv) planes: bands, positions
    int dpar;              // which of the two (du, dv) planes holds the last sweep's values
    int band_rows, koff, poff;  // rows per band, climb of the bands up to the last sweep, position offset (common.h)
};
__device__ __forceinline__ size_t skew_cell(int i, int j, const SkewIdx& k) {
    return (size_t)(i + j + k.qt) * k.hp + (size_t)(i + k.rt);
}
template <bool SKEW>
__device__ __forceinline__ size_t sor_index(int i, int j, int W, const SkewIdx& k) {
    if (SKEW) return 2 * skew_cell(i, j, k);
    return (size_t)i * W + j;
}
// A tile of assembled cells on its way to the exact-order solver's planes: cells are COMPUTED in row-major order (coalesced
// plane reads), staged in LDS, and WRITTEN in skew order -- for one skew position (anti-diagonal) the COLS threads of a group
// store COLS neighbouring rows, contiguous in each paired plane (pa = (phi, xy), pb = (a1, a2), pc = (b1, b2)) -- instead of
// scattered 16-byte cells.  256 threads; the tile starts at (ib, j0), rows below row1 and columns below W exist.
struct SystemCell {  // the operands of one cell of the linear system (and imdx2, imdy2 for the stage entry points)
    double phi, xy, a1, a2, b1, b2, x2, y2;
};
struct double2s {
    double x, y;
};
template <int ROWS, int PITCH>  // (PITCH = the tile's columns + 1)
__device__ __forceinline__ void stage_cell(double (&stage)[6][ROWS][PITCH], int r, int jj, const SystemCell& s) {
    stage[0][r][jj] = s.phi;
    stage[1][r][jj] = s.xy;
    stage[2][r][jj] = s.a1;
    stage[3][r][jj] = s.a2;
    stage[4][r][jj] = s.b1;
    stage[5][r][jj] = s.b2;
}
template <int ROWS, int PITCH>
__device__ __forceinline__ void store_skew_tile(const double (&stage)[6][ROWS][PITCH], int tid, int ib, int j0, int row1,
                                                int W, const SkewIdx& sk, double2s* __restrict__ pa,
                                                double2s* __restrict__ pb, double2s* __restrict__ pc) {
    constexpr int COLS = PITCH - 1;
    const int g = tid / COLS, jj = tid - g * COLS;  // 256 / COLS groups of COLS threads; a group walks anti-diagonals
    const int j = j0 + jj;
    if (j >= W) return;
    for (int pp = g; pp <= ROWS + COLS - 2; pp += 256 / COLS) {  // pp = jj + (row in tile)
        const int r = pp - jj;
        if (r < 0 || r >= ROWS) continue;
        const int i = ib + r;
        if (i >= row1) continue;
        const size_t q = skew_cell(i, j, sk);
        pa[q] = double2s{stage[0][r][jj], stage[1][r][jj]};
        pb[q] = double2s{stage[2][r][jj], stage[3][r][jj]};
        pc[q] = double2s{stage[4][r][jj], stage[5][r][jj]};
    }
}

// cell of (du, dv)(i, j) after the last sweep in the banded ping-pong planes (common.h)
__device__ __forceinline__ size_t dudv_cell(int i, int j, const SkewIdx& k) {
    const int t = i + k.koff, b = t / k.band_rows, c = 1 + (t - b * k.band_rows);
    const size_t parity = (size_t)k.dpar * k.npos_d * k.nb * kLanes;
    return parity + ((size_t)(j + c + k.poff) * k.nb + b) * kLanes + c;
}

// ------------------------------------------------------------------------------------------------
// The flow increment (du, dv) of the previous inner fixed-point iteration, read where the solver left it
// (paired skewed plane or two row-major planes).  `du == nullptr` means the first inner iteration: du = dv = 0.
// ------------------------------------------------------------------------------------------------
struct Increment {
    const double *du, *dv;
    int skew;
    SkewIdx sk;
    const double* gm;  // Gaussian-mixture noise model (src/OpticalFlow.cpp:359-367): alpha[C], sigma[C], beta[C],
                       // sigma_square[C], beta_square[C] of GaussianMixture (src/NoiseModel.h); null = Laplacian (default)
    const double* lap; // Laplacian noise level per channel (LapPara, estLaplacianNoise src/OpticalFlow.cpp:594-639) for the guard of
                       // :399-400 -- psi of a channel stays 0 (Psi_1st.reset(), :333) while LapPara[k] < 1E-20; null = not consulted
                       // (the optimistic pass of flow_device: api.hip, LapGuard)
};
__device__ __forceinline__ void increment_at(const Increment& I, int i, int j, int W, double& du, double& dv) {
    if (I.du == nullptr) {
        du = 0.0;
        dv = 0.0;
    } else if (I.skew) {
        const size_t q = 2 * dudv_cell(i, j, I.sk);
        du = I.du[q];
        dv = I.du[q + 1];
    } else {
        du = I.du[(size_t)i * W + j];
        dv = I.dv[(size_t)i * W + j];
    }
}

// ------------------------------------------------------------------------------------------------
// phi, src/OpticalFlow.cpp:295-331: uu = u (+ du after the first inner iteration, :297-303), forward differences
// (zero in the last column / row, src/Image.h:979-986, :1022-1029), phi = 0.5/sqrt(ux^2+uy^2+vx^2+vy^2+eps).
// ------------------------------------------------------------------------------------------------
__global__ void k_phi(const double* __restrict__ u, const double* __restrict__ v, Increment I,
                      double* __restrict__ phi, int H, int W, Rect rc, unsigned long long* stamp) {
    stamp_now(stamp);
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t o = (size_t)i * W + j;
    double uc = u[o], vc = v[o], ur = 0.0, vr = 0.0, ud = 0.0, vd = 0.0;
    if (j < W - 1) {
        ur = u[o + 1];
        vr = v[o + 1];
    }
    if (i < H - 1) {
        ud = u[o + W];
        vd = v[o + W];
    }
    if (I.du != nullptr) {  // uu = u + du, vv = v + dv (Image::Add, src/Image.h:1857-1877)
        double a, b;
        increment_at(I, i, j, W, a, b);
        uc = uc + a;
        vc = vc + b;
        if (j < W - 1) {
            increment_at(I, i, j + 1, W, a, b);
            ur = ur + a;
            vr = vr + b;
        }
        if (i < H - 1) {
            increment_at(I, i + 1, j, W, a, b);
            ud = ud + a;
            vd = vd + b;
        }
    }
    phi[o] = phi_value(uc, vc, ur, vr, ud, vd, j < W - 1, i < H - 1);
}

// A cell's neighbourhood for the Laplacian and the diagonals: which neighbours exist, the plane's values at the cell and
// around it, and phi at the cell, to its left and above (the weights of the four differences).  EDGE = false: the cell is
// not on an image border, every neighbour exists -- no test, constant address offsets.  On a border the loads are branch-free:
// a neighbour that does not exist reads the cell itself and is not used.
struct Nbrs {
    bool left, right, up, down;
};
__device__ __forceinline__ Nbrs nbrs_at(int i, int j, int H, int W) { return Nbrs{j > 0, j < W - 1, i > 0, i < H - 1}; }
struct Cross {
    double c, l, r, u, d;
};
template <bool EDGE>
__device__ __forceinline__ Cross cross_at(const double* __restrict__ in, size_t o, int W, const Nbrs& n) {
    return Cross{in[o], in[!EDGE || n.left ? o - 1 : o], in[!EDGE || n.right ? o + 1 : o], in[!EDGE || n.up ? o - W : o],
                 in[!EDGE || n.down ? o + W : o]};
}
struct PhiAround {
    double c, l, u;
};
template <bool EDGE>
__device__ __forceinline__ PhiAround phi_around(const double* __restrict__ phi, size_t o, int W, const Nbrs& n) {
    return PhiAround{phi[o], phi[!EDGE || n.left ? o - 1 : o], phi[!EDGE || n.up ? o - W : o]};
}

// OpticalFlow::Laplacian at one cell, src/OpticalFlow.cpp:641-690: column W-1 receives no horizontal
// term and row H-1 no vertical term (the loops stop at W-2 / H-2).
template <bool EDGE>
__device__ __forceinline__ double laplacian_value(const Cross& x, const PhiAround& p, const Nbrs& n) {
    double out = 0.0;
    if (!EDGE || n.right) {
        out -= (x.r - x.c) * p.c;
        if (!EDGE || n.left) out += (x.c - x.l) * p.l;
    }
    if (!EDGE || n.down) {
        out -= (x.d - x.c) * p.c;
        if (!EDGE || n.up) out += (x.c - x.u) * p.u;
    }
    return out;
}

__global__ void k_laplacian(const double* __restrict__ in, const double* __restrict__ wt, double* __restrict__ out,
                            int H, int W) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j;
    const Nbrs n = nbrs_at(i, j, H, W);
    out[o] = laplacian_value<true>(cross_at<true>(in, o, W, n), phi_around<true>(wt, o, W, n), n);
}

// diagonal terms of the SOR update, src/OpticalFlow.cpp:468-501: coeff accumulated left, right, up, down,
// scaled by alpha; a = omega / (imd?2 + alpha*0.05 + coeff).  They do not change during the sweeps, so
// the two divisions per cell-update of the reference are hoisted out of the sweep loop (same bits:
// the reference evaluates (omega/denominator) * (rhs - sigma) left to right).
template <bool EDGE>
__device__ __forceinline__ void sor_diagonals(const PhiAround& p, const Nbrs& n, double imdx2, double imdy2, double alpha,
                                              double omega, double& a1, double& a2) {
    double coeff = 0.0;
    if (!EDGE || n.left) coeff += p.l;
    if (!EDGE || n.right) coeff += p.c;
    if (!EDGE || n.up) coeff += p.u;
    if (!EDGE || n.down) coeff += p.c;
    coeff *= alpha;
    a1 = omega / (imdx2 + alpha * 0.05 + coeff);
    a2 = omega / (imdy2 + alpha * 0.05 + coeff);
}

// ------------------------------------------------------------------------------------------------
// Fused assembly of the linear system of one fixed-point iteration (du = dv = 0, i.e. nInner == 1):
//   imdx/imdy  = 5-point derivatives of the blended image, src/OpticalFlow.cpp:95-96 (computed inline)
//   psi        = 1/(2 sqrt(imdt^2 + eps)) per channel, :377-406
//   imdxy,...  = channel means of (psi*a)*b, :414-427 with src/Image.h:1747-1763 and :1537-1545
//   rhs        = -imdtd? - alpha*Laplacian(flow, phi), :437-448
//   a1, a2     = hoisted SOR diagonals (above)
// Reads 2*planes + 3 streams, writes 6 SOR operand planes in the layout the solver wants.
// ------------------------------------------------------------------------------------------------
// psi of the Laplacian noise model, src/OpticalFlow.cpp:401-404, from t = (imdt + imdx * du + imdy * dv)^2
__device__ __forceinline__ double psi_value(double t) { return 1 / (2 * sqrt(t + 0.001 * 0.001)); }

// the channel sums of (psi * a) * b, :414-427 with src/Image.h:1747-1763 (a single channel is assigned, not accumulated),
// and their means over the channels, src/Image.h:1537-1545
struct PsiTerms {
    double xy = 0.0, x2 = 0.0, y2 = 0.0, tx = 0.0, ty = 0.0;
    __device__ __forceinline__ void add(double psi, double gx, double gy, double gt, bool single) {
        const double pgx = psi * gx, pgy = psi * gy;
        if (single) {
            xy = pgx * gy;
            x2 = pgx * gx;
            y2 = pgy * gy;
            tx = pgx * gt;
            ty = pgy * gt;
        } else {
            xy += pgx * gy;
            x2 += pgx * gx;
            y2 += pgy * gy;
            tx += pgx * gt;
            ty += pgy * gt;
        }
    }
    __device__ __forceinline__ void mean(int planes) {
        if (planes > 1) {
            xy = xy / planes;
            x2 = x2 / planes;
            y2 = y2 / planes;
            tx = tx / planes;
            ty = ty / planes;
        }
    }
};

// rhs = -imdtd? - alpha * Laplacian(flow, phi) (:437-448) and the hoisted diagonals, from the channel means
template <bool EDGE>
__device__ __forceinline__ SystemCell system_cell(const PsiTerms& s, const PhiAround& p, const Cross& cu, const Cross& cv,
                                                  const Nbrs& n, double alpha, double omega) {
    SystemCell c;
    c.b1 = -s.tx - alpha * laplacian_value<EDGE>(cu, p, n);
    c.b2 = -s.ty - alpha * laplacian_value<EDGE>(cv, p, n);
    sor_diagonals<EDGE>(p, n, s.x2, s.y2, alpha, omega, c.a1, c.a2);
    c.phi = p.c;
    c.xy = s.xy;
    c.x2 = s.x2;
    c.y2 = s.y2;
    return c;
}

// EDGE = false: the cell is at least 2 pixels away from every image border, so no index needs clamping and every
// neighbour exists -- the same operations in the same order with constant address offsets (the kernel is bound by
// instruction issue, a third of it index arithmetic for the clamps).
// PLANES > 0: the channel count as a compile-time constant -- the channel loop is unrolled, so the stencil loads of all
// channels are in flight together instead of one channel's per memory round trip (same operations, same order).
// FAST: the default branches, known at compile time -- Laplacian noise model without a consulted estimate (I.gm == I.lap ==
// nullptr) and no increment of an earlier inner iteration (I.du == nullptr): no branch is left inside the channel loop, so
// the stencil loads of all channels really are in flight together (the uniform branches cut the loop into basic blocks, each
// with its own wait: five memory round trips per cell).
template <bool EDGE = true, int PLANES = 0, bool FAST = false>
__device__ __forceinline__ SystemCell assemble_cell(const double* __restrict__ blend, const double* __restrict__ imdt,
                                                    const double* __restrict__ phi, const double* __restrict__ u,
                                                    const double* __restrict__ v, int i, int j, int H, int W,
                                                    int planes_rt, double alpha, double omega, const Taps& d,
                                                    const Increment& I) {
    const int planes = PLANES > 0 ? PLANES : planes_rt;
    const size_t np = (size_t)H * W, o = (size_t)i * W + j;
    PsiTerms s;
    double du = 0.0, dv = 0.0;
    if (!FAST) increment_at(I, i, j, W, du, dv);
    const auto channel = [&](int k) {
        const double* im = blend + k * np;
        double gx, gy;
        if (EDGE) {
            gx = tap_sum<2>(d, [&](int l) { return im[(size_t)i * W + clampi(j + l, W)]; });
            gy = tap_sum<2>(d, [&](int l) { return im[(size_t)clampi(i + l, H) * W + j]; });
        } else {
            const double* p = im + o;
            gx = tap_sum<2>(d, [&](int l) { return p[l]; });
            gy = tap_sum<2>(d, [&](int l) { return p[(ptrdiff_t)l * W]; });
        }
        const double gt = imdt[k * np + o];
        double t = gt;  // imdt + imdx*du + imdy*dv (src/OpticalFlow.cpp:384); du = dv = 0 in the first inner iteration
        if (!FAST && I.du != nullptr) t = gt + gx * du + gy * dv;
        t *= t;
        double psi;
        if (FAST) {
            psi = psi_value(t);
        } else if (I.gm != nullptr) {  // :392-396 with GaussianMixture::Gaussian (src/NoiseModel.h:120-126).  The reference's PI there is
                                // 3.1415927: Stochastic.h:19 defines it before NoiseModel.h's #ifndef (oracle/papof_oracle.c).
                                // exp() is the device library's (<= 1 ulp, not glibc's bits): tolerance-checked branch.
            const double* g = I.gm;
            const double alpha_k = g[k], sigma = g[planes + k], beta = g[2 * planes + k];
            const double s2 = g[3 * planes + k], b2 = g[4 * planes + k];
            const double prob1 = exp(-t / (2 * s2)) / (2 * 3.1415927 * sigma) * alpha_k;
            const double prob2 = exp(-t / (2 * b2)) / (2 * 3.1415927 * beta) * (1 - alpha_k);
            const double prob11 = prob1 / (2 * s2);
            const double prob22 = prob2 / (2 * b2);
            psi = (prob11 + prob22) / (prob1 + prob2);
        } else if (I.lap != nullptr && I.lap[k] < 1E-20) {
            psi = 0.0;  // :399-400 `continue` on the freshly reset Psi_1st (:333)
        } else {
            psi = psi_value(t);
        }
        s.add(psi, gx, gy, gt, planes == 1);
    };
    if (PLANES > 0) {
#pragma unroll
        for (int k = 0; k < PLANES; k++) channel(k);
    } else {
#pragma unroll 1
        for (int k = 0; k < planes; k++) channel(k);
    }
    s.mean(planes);
    const Nbrs n = nbrs_at(i, j, H, W);
    return system_cell<EDGE>(s, phi_around<EDGE>(phi, o, W, n), cross_at<EDGE>(u, o, W, n), cross_at<EDGE>(v, o, W, n), n,
                             alpha, omega);
}

// row-major operands (red-black / Jacobi modes): one thread per cell
__global__ void k_assemble(const double* __restrict__ blend, const double* __restrict__ imdt,
                           const double* __restrict__ phi, const double* __restrict__ u,
                           const double* __restrict__ v, int H, int W, int planes, double alpha, double omega,
                           double* __restrict__ o_phi, double* __restrict__ o_xy, double* __restrict__ o_a1,
                           double* __restrict__ o_a2, double* __restrict__ o_b1, double* __restrict__ o_b2,
                           double* __restrict__ o_x2, double* __restrict__ o_y2, Taps d, Increment I, Rect rc,
                           unsigned long long* stamp) {
    stamp_now(stamp);
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t o = (size_t)i * W + j;
    const SystemCell c = assemble_cell(blend, imdt, phi, u, v, i, j, H, W, planes, alpha, omega, d, I);
    o_phi[o] = c.phi;
    o_xy[o] = c.xy;
    o_a1[o] = c.a1;
    o_a2[o] = c.a2;
    o_b1[o] = c.b1;
    o_b2[o] = c.b2;
    if (o_x2) o_x2[o] = c.x2;
    if (o_y2) o_y2[o] = c.y2;
}

// Skewed, paired operands of the exact-order solver.  A block owns a tile of kAsmRows rows x kTileJ columns
// (stage_cell / store_skew_tile above: 256 contiguous bytes per paired plane and skew position).
#ifndef PAPOF_V_ASMCOLS
#define PAPOF_V_ASMCOLS 16
#endif
constexpr int kTileJ = PAPOF_V_ASMCOLS;  // columns of the assembly kernel's tile = cells of one contiguous chunk it writes
#ifndef PAPOF_V_ASMROWS
#define PAPOF_V_ASMROWS 16  // same-box A/B (round 3, ms per 1080p pair): 62 rows 10.93-10.96, 31: 10.80, 24: 10.91, 16: 10.73-10.83, 12: 10.76-10.78, 8: 10.85-10.87
#endif
constexpr int kAsmRows = PAPOF_V_ASMROWS;  // rows of the assembly kernel's tile (its LDS stage bounds the workgroups per CU)
template <int PLANES, bool FAST>
__global__ __launch_bounds__(256) void k_assemble_skew(const double* __restrict__ blend,
                                                       const double* __restrict__ imdt,
                                                       const double* __restrict__ phi, const double* __restrict__ u,
                                                       const double* __restrict__ v, int H, int W, int planes,
                                                       double alpha, double omega, SkewIdx sk,
                                                       double2s* __restrict__ pa, double2s* __restrict__ pb,
                                                       double2s* __restrict__ pc, double* __restrict__ o_x2,
                                                       double* __restrict__ o_y2, Taps d, Increment I,
                                                       unsigned long long* stamp, int row0, int row1) {
    __shared__ double stage[6][kAsmRows][kTileJ + 1];
    stamp_now(stamp);
    // tiles start at row0 and rows row0 .. row1-1 are written (a strip of the plane; the whole plane otherwise)
    const int ib = row0 + blockIdx.y * kAsmRows, j0 = blockIdx.x * kTileJ, tid = threadIdx.x;
    // block-uniform: no cell of this tile is closer than 2 pixels to an image border
    const bool interior = ib >= 2 && ib + kAsmRows + 2 <= H && j0 >= 2 && j0 + kTileJ + 2 <= W;
    for (int c = tid; c < kAsmRows * kTileJ; c += 256) {
        const int r = c / kTileJ, jj = c - r * kTileJ;
        const int i = ib + r, j = j0 + jj;
        if (i < row1 && j < W) {
            const SystemCell s =
                interior ? assemble_cell<false, PLANES, FAST>(blend, imdt, phi, u, v, i, j, H, W, planes, alpha, omega, d, I)
                         : assemble_cell<true, PLANES, FAST>(blend, imdt, phi, u, v, i, j, H, W, planes, alpha, omega, d, I);
            stage_cell(stage, r, jj, s);
            if (o_x2) o_x2[(size_t)i * W + j] = s.x2;
            if (o_y2) o_y2[(size_t)i * W + j] = s.y2;
        }
    }
    __syncthreads();
    store_skew_tile(stage, tid, ib, j0, row1, W, sk, pa, pb, pc);
}

// ------------------------------------------------------------------------------------------------
// k_flow_system: k_warp_smooth_blend + k_assemble_skew<PLANES, FAST> in ONE kernel (default branches, exact-order layout) -- the
// warped, smoothed and blended tile goes to the derivative / psi / coefficient stage through LDS, so `blend` and `imdt` (166 MB
// written and read again per level-0 iteration) never go to HBM.  A block owns kFT x kFT cells and works, channel by channel,
// on tiles indexed by PIXEL (position - origin; only pixels inside the image are computed, a consumer looks its neighbour
// clamp(p + l) up): the warp on the tile + 4, its smoothing on + 2 (which is where the blend and imdt live), the derivatives on
// the tile.  phi of the tile (and its upper / left neighbours) is computed from (u, v) into LDS.  Every expression and its
// order are those of the two kernels it replaces: same bits.
// The flow of the tile + 4 is read from memory ONCE, by the tap pass, and parked in LDS: phi and the cell's cross of (u, v)
// take it from there.  `sdu` (null: none): the increment the previous outer iteration's solve left, where and as
// k_update_warp_phi reads it -- the flow is then u + du, v + dv everywhere in this kernel (that kernel's load, add: its bits),
// and the tile's own cells write it to (u_out, v_out), the OTHER pair of planes: neighbouring blocks read the old pair and the
// increment only.  A run-time, wave-uniform argument, and all of it in front of the channel loop.
// ------------------------------------------------------------------------------------------------
constexpr int kFT = 16, kFH = 4, kFW = kFT + 2 * kFH;  // tile rows and columns, halo, tile rows with halo
// [162 - 164 registers (at most 168: three workgroups per CU, tests/test_codegen_flow_system.py); forcing four or five waves per
// SIMD spills: 11.2 / 12.8 ms per 1080p pair against 10.35]
// SKEW: the operands go to the exact-order solver's paired, skewed planes (pa, pb, pc); otherwise to six row-major planes
// (q[0..5] = phi, xy, a1, a2, b1, b2: the one-workgroup solver of the small levels, k_sor_tiny).
struct SixPlanes {
    double* q[6];
};
typedef double tap_pair __attribute__((ext_vector_type(2), aligned(8)));  // two neighbouring elements of a plane: ONE 16-byte load
__device__ __forceinline__ double plane_ld(const double* plane, unsigned byte_off) {  // uniform base + 32-bit lane offset
    return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(plane) + byte_off);
}
__device__ __forceinline__ tap_pair plane_ld2(const double* plane, unsigned byte_off) {
    return *reinterpret_cast<const tap_pair*>(reinterpret_cast<const char*>(plane) + byte_off);
}
template <int PLANES, bool SKEW, bool BATCH = false, bool W1 = false>
__global__ __launch_bounds__(256, 1) void k_flow_system(const double* __restrict__ im1, const double* __restrict__ im2,
                                                     const double* __restrict__ u, const double* __restrict__ v,
                                                     const double* __restrict__ im1s, int H, int W, double alpha,
                                                     double omega, SkewIdx sk, SixPlanes out, Taps g, Taps d,
                                                     unsigned long long* stamp, unsigned* __restrict__ wit, double wit_thr,
                                                     unsigned mark, int row0, int row1, BatchK bk,
                                                     const double* __restrict__ sdu, const double* __restrict__ sdv,
                                                     double* __restrict__ u_out, double* __restrict__ v_out) {
    if (BATCH) {  // blockIdx.y: the pair of a batch (common.h: BatchK; no increment there: flow_system())
        const size_t p = blockIdx.y;
        im1s += batch_frames(bk, p, im1, im2);  // (a backward pair: image 1's smoothed features are frame 2's)
        u += p * bk.uv;
        v += p * bk.uv;
        if (wit != nullptr) wit += p * bk.wit;
#pragma unroll
        for (int q = 0; q < 6; q++) out.q[q] += p * bk.sp;
    }
    // rows row0 .. row1-1 are assembled (a rank's range of rows, tiles.hip: bands_flow; the whole plane otherwise): (u, v) are
    // read on rows row0 - 4 .. row1 + 3 only, the smoothed frame 1 on row0 - 2 .. row1 + 1
    constexpr int NT = kFT * kFT, HWc = kFT + 2 * kFH;  // threads = cells of the tile; columns of the tile with its halo
    __shared__ double raw[kFW][HWc + 1];            // warped frame 2, pixels (ib - 4 .. ib + 19) x (j0 - 4 .. j0 + 19)
    __shared__ double hs[kFW][kFT + 4 + 1];         // h-smoothed, columns j0 - 2 .. j0 + 17
    __shared__ double bl[kFT + 4][kFT + 4 + 1];     // blend, pixels (ib - 2 .. ib + 17) x (j0 - 2 .. j0 + 17)
    __shared__ double it[kFT][kFT + 1];             // imdt of the tile
    __shared__ double ph[kFT + 1][kFT + 1 + 1];     // phi, pixels (ib - 1 .. ib + 15) x (j0 - 1 .. j0 + 15)
    __shared__ double stage[6][kFT][kFT + 1];
    __shared__ double fu[kFW][HWc + 1], fv[kFW][HWc + 1];  // the flow (with the increment) on the pixels of raw
    stamp_now(stamp);
    // Workgroups are dealt round-robin over the 8 XCDs (observed; speed only): give each XCD a contiguous run of tiles, so
    // that the halo pixels neighbouring tiles both gather are found in that XCD's L2 (as k_sor_blocked does)
    const int ntx = (W + kFT - 1) / kFT, ntiles = ntx * ((row1 - row0 + kFT - 1) / kFT), per = (ntiles + 7) >> 3;
    const int vt = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per || vt >= ntiles) return;  // whole workgroup, before any barrier
    const int tby = vt / ntx, tbx = vt - tby * ntx;
    const int ib = row0 + tby * kFT, j0 = tbx * kFT, tid = threadIdx.x;
    const size_t np = (size_t)H * W;
    const int vy0 = max(0, row0 - kFH), vy1 = min(H, row1 + kFH);  // rows on which the operands are valid
    const bool interior = ib >= vy0 + kFH && ib + kFT <= row1 && ib + kFT + kFH <= vy1 && j0 >= kFH && j0 + kFT + kFH <= W;  // block-uniform
    // ---- bilinear taps of the tile's pixels, once for all channels: (x0, y0), (dx, dy), or "outside" (frame 1's value)
    // The 576 pixels are three slots per thread: pixel tid, pixel tid + 256 (10 rows and 16 columns further on in the 24-wide
    // tile) and pixel 512 + lane.  The third slot is ONE wave's worth of pixels: every wave holds its taps and the four waves
    // take turns at it, channel by channel (wave k & 3 on channel k; a scalar test), so that no wave gathers and blends for
    // pixels that do not exist and none is always the last at the barrier.
    // All addressing is per-lane 32-bit BYTE offsets into a channel plane, computed here once (flow_system() refuses planes
    // beyond 2^29 elements); the channel's plane is a wave-uniform base.
    constexpr int kPer = (kFW * HWc + NT - 1) / NT;  // 3 (576 pixels, NT = 16 x 16)
    static_assert(kFW * HWc == 2 * NT + 64 && NT + 16 < kFW * HWc, "the three slots of the warp");
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr bool w1 = W1;  // W == 1, one column: no pair of taps to load (an instantiation of its own, flow_system())
    unsigned t_o[kPer], t_b0[kPer], t_b1[kPer];  // byte offsets of the own pixel and of the taps' two footprint rows
    int t_ra[kPer];  // the pixel's place in raw
    double t_dx[kPer], t_dy[kPer];
    bool t_in[kPer], t_out[kPer], t_hi[kPer];
    {
        int r = tid / HWc, cc = tid - r * HWc;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            if (q == 1) {  // + 256 pixels
                cc += NT - 10 * HWc;
                r += 10;
                if (cc >= HWc) {
                    cc -= HWc;
                    r++;
                }
            } else if (q == 2) {  // pixel 512 + lane
                cc = lane + (2 * NT - (2 * NT / HWc) * HWc);
                r = 2 * NT / HWc;
                if (cc >= HWc) {
                    cc -= HWc;
                    r++;
                }
                if (cc >= HWc) {
                    cc -= HWc;
                    r++;
                }
            }
            const int i = ib - kFH + r, j = j0 - kFH + cc;
            t_ra[q] = r * (HWc + 1) + cc;
            t_in[q] = i >= vy0 && i < vy1 && j >= 0 && j < W;
            const int o = t_in[q] ? i * W + j : 0;
            t_o[q] = (unsigned)o * 8u;
            double x = 0.0, y = 0.0;  // (a cell outside the image: any valid position, its value is not used)
            t_out[q] = false;
            if (t_in[q]) {
                double pu = u[o], pv = v[o];
                if (sdu != nullptr) {
                    double a, b;
                    if (SKEW) {
                        const double2s c = reinterpret_cast<const double2s*>(sdu)[dudv_cell(i, j, sk)];
                        a = c.x;
                        b = c.y;
                    } else {
                        a = sdu[o];
                        b = sdv[o];
                    }
                    pu += a;
                    pv += b;
                }
                (&fu[0][0])[t_ra[q]] = pu;  // (the third slot: by every wave, the same value)
                (&fv[0][0])[t_ra[q]] = pv;
                y = i + pv;
                x = j + pu;
                t_out[q] = leaves_image(x, y, W, H);
                if (t_out[q]) {
                    x = j;
                    y = i;
                }
            }
            // the taps (y0, x0), (y0, x1 = min(x0 + 1, W - 1)) of a footprint row lie side by side: ONE 16-byte load at
            // xb = min(x0, W - 2) holds both -- (lo, hi), or (hi, hi) where x0 is the last column (the same operands)
            const int x0 = (int)x, y0 = (int)y, y1 = min(y0 + 1, H - 1);
            const int xb = w1 ? 0 : min(x0, W - 2);
            t_hi[q] = x0 == W - 1;
            t_b0[q] = (unsigned)(y0 * W + xb) * 8u;
            t_b1[q] = (unsigned)(y1 * W + xb) * 8u;
            t_dx[q] = x - x0;
            t_dy[q] = y - y0;
        }
    }
    // a pixel that leaves the image takes frame 1's value: loaded (beside the gathers, which such a pixel does around itself in
    // frame 2, unused) only in a wave that has such a pixel -- a scalar test
    const bool wout = __ballot(t_out[0] || t_out[1] || t_out[2]) != 0ull;
    __syncthreads();
    // ---- phi of the tile and its upper / left neighbours, from the parked flow: pixel (i, j), its right and its lower
    // neighbour are pixels of the tile + 4 on rows the operands are valid on (i + 1 <= row1 < vy1 where it is used)
    for (int c = tid; c < (kFT + 1) * (kFT + 1); c += NT) {
        const int r = c / (kFT + 1), cc = c - r * (kFT + 1);
        const int i = ib - 1 + r, j = j0 - 1 + cc;
        if (i < 0 || i >= min(H, row1) || j < 0 || j >= W) continue;
        const double *const pu = &fu[r + kFH - 1][cc + kFH - 1], *const pv = &fv[r + kFH - 1][cc + kFH - 1];
        const double uc = pu[0], vc = pv[0];
        double ur = 0.0, vr = 0.0, ud = 0.0, vd = 0.0;
        if (j < W - 1) {
            ur = pu[1];
            vr = pv[1];
        }
        if (i < H - 1) {
            ud = pu[HWc + 1];
            vd = pv[HWc + 1];
        }
        ph[r][cc] = phi_value(uc, vc, ur, vr, ud, vd, j < W - 1, i < H - 1);
    }
    const int orow = tid / kFT, ocol = tid - orow * kFT;  // this thread's cell of the tile
    const int oi = ib + orow, oj = j0 + ocol;
    const bool own = oi < row1 && oj < W;
    PsiTerms s;
    // witnesses of the Laplacian-noise guard (k_warp_smooth_blend): one block in sixteen on large grids, its first wave
    const bool sampler = wit != nullptr && tid < 64 &&
                         lap_samples_here(ntiles, tbx, tby);
    // The global operands of a channel are PREFETCHED while the previous channel is worked on (a workgroup barrier does not
    // wait for loads in flight): the gathers (and frame 1's value for a pixel that leaves the image) right behind P1, the smoothed
    // frame 1 of the blend's pixels right behind P3 -- the phases between are LDS only.
    constexpr int kP3 = ((kFT + 4) * (kFT + 4) + NT - 1) / NT;  // 2
    // the blend's pixels of a thread, (row, column) of the tile + 2, and their (clamped) place in the smoothed frame 1
    int s_r[kP3], s_c[kP3];
    unsigned s_o[kP3];
    // P2: two neighbouring columns per thread (240 threads), P3: two neighbouring rows (200 threads) -- six LDS reads feed the
    // two sums where ten did, and each phase is one pass; every sum keeps its own order
    static_assert(kP3 == 2 && kFW * (kFT + 4) / 2 <= NT && (kFT + 4) * (kFT + 4) / 2 <= NT, "two outputs per thread");
    const int h_r = tid / ((kFT + 4) / 2), h_c = 2 * (tid - h_r * ((kFT + 4) / 2));  // P2: row of raw, first of the two columns of hs
    {
        const int t = min(tid, (kFT + 4) * (kFT + 4) / 2 - 1), rp = t / (kFT + 4);
        s_r[0] = 2 * rp;
        s_r[1] = 2 * rp + 1;
        s_c[0] = s_c[1] = t - rp * (kFT + 4);
    }
#pragma unroll
    for (int q = 0; q < kP3; q++)  // (branch-free: a position outside the image reads its clamped pixel and is not used)
        s_o[q] = (unsigned)(clampi(ib - 2 + s_r[q], H) * W + clampi(j0 - 2 + s_c[q], W)) * 8u;
    double* const rawf = &raw[0][0];
    tap_pair ga[kPer], gb[kPer];  // the taps of the footprint's upper and lower row
    double f1v[kPer] = {0.0, 0.0, 0.0}, s1v[kP3], wv = 0.0;
    const auto load_gathers = [&](int k) {
        const double *p1 = im1 + k * np, *p2 = im2 + k * np;
        const bool third = (k & 3) == wave;
#pragma unroll
        for (int q = 0; q < kPer; q++) {  // branch-free per lane: a cell outside the image reads pixel 0 and is not used
            if (q == 2 && !third) continue;
            if (w1) {
                ga[q].x = plane_ld(p2, t_b0[q]);  // (both taps of the row are this element)
                gb[q].x = plane_ld(p2, t_b1[q]);
            } else {
                ga[q] = plane_ld2(p2, t_b0[q]);
                gb[q] = plane_ld2(p2, t_b1[q]);
            }
            if (wout) f1v[q] = plane_ld(p1, t_o[q]);
        }
        if (sampler) wv = plane_ld(p1, t_o[0]);
    };
    const auto load_s1 = [&](int k) {
        const double* ps = im1s + k * np;
#pragma unroll
        for (int q = 0; q < kP3; q++) s1v[q] = plane_ld(ps, s_o[q]);
    };
    const auto two_sums = [&](const double(&x)[6], double& a0, double& a1) {
        a0 = tap_sum<2>(g, [&](int l) { return x[l + 2]; });
        a1 = tap_sum<2>(g, [&](int l) { return x[l + 3]; });
    };
    load_gathers(0);
    load_s1(0);
#pragma unroll 1
    for (int k = 0; k < PLANES; k++) {
        // -- P1: the warp
        bool hit = false;
        const bool third = (k & 3) == wave;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            if (q == 2 && !third) continue;
            // bilinear_inside(g0, g1, g2, g3, dx, dy), KEPT IN PLACE: through the function (any form of it: values, references, a
            // weights struct, a lambda) the exec-mask handling of every instance changes -- 25886 -> 25617 instructions over the
            // 16 instances, SGPR spills to VGPR lanes 116 -> 146, one instance gains a private segment (profiles/level_once_isa.txt)
            const double dx = t_dx[q], dy = t_dy[q], ex = 1.0 - dx, ey = 1.0 - dy;
            const double g0 = !w1 && t_hi[q] ? ga[q].y : ga[q].x, g1 = !w1 && t_hi[q] ? gb[q].y : gb[q].x;
            const double g2 = w1 ? ga[q].x : ga[q].y, g3 = w1 ? gb[q].x : gb[q].y;
            double res = 0.0;
            res += g0 * (ex * ey);
            res += g1 * (ex * dy);
            res += g2 * (dx * ey);
            res += g3 * (dx * dy);
            res = t_out[q] ? f1v[q] : res;  // a pixel that leaves the image takes frame 1's value
            if (t_in[q]) rawf[t_ra[q]] = res;
            if (sampler && q == 0) {
                const double dd = fabs(wv - res);
                hit = lap_witness(dd, wit_thr, t_in[q]);
            }
        }
        if (sampler) {
            const unsigned long long hits = __ballot(hit);
            if (hits != 0ull && tid == 0) wit[k] = mark;
        }
        if (k + 1 < PLANES) load_gathers(k + 1);
        __syncthreads();
        // -- P2: horizontal pass on every row of the tile, columns j0 - 2 .. j0 + 17
        if (tid < kFW * (kFT + 4) / 2) {
            const double* const row = raw[h_r];
            double x[6], a0, a1;
            if (interior) {  // (block-uniform: every pixel of the tile + 4 is inside the image -- no clamps, no tests)
#pragma unroll
                for (int m = 0; m < 6; m++) x[m] = row[h_c + m];
                two_sums(x, a0, a1);
                hs[h_r][h_c] = a0;
                hs[h_r][h_c + 1] = a1;
            } else {
                const int i = ib - kFH + h_r, j = j0 - 2 + h_c;
                const bool ok0 = j >= 0 && j < W, ok1 = j + 1 >= 0 && j + 1 < W;
                if (i >= 0 && i < H && (ok0 || ok1)) {
#pragma unroll
                    for (int m = 0; m < 6; m++) x[m] = row[clampi(j - 2 + m, W) - (j0 - kFH)];
                    two_sums(x, a0, a1);
                    if (ok0) hs[h_r][h_c] = a0;
                    if (ok1) hs[h_r][h_c + 1] = a1;
                }
            }
        }
        __syncthreads();
        // -- P3: vertical pass, blend and imdt on (ib - 2 .. ib + 17) x (j0 - 2 .. j0 + 17)
        if (tid < (kFT + 4) * (kFT + 4) / 2) {
            const int r0 = s_r[0], cc = s_c[0], i = ib - 2 + r0, j = j0 - 2 + cc;
            const bool okj = j >= 0 && j < W, ok0 = okj && i >= 0 && i < H, ok1 = okj && i + 1 >= 0 && i + 1 < H;
            if (ok0 || ok1) {
                double x[6], a[2];
                if (interior) {
#pragma unroll
                    for (int m = 0; m < 6; m++) x[m] = hs[r0 + m][cc];
                } else {
#pragma unroll
                    for (int m = 0; m < 6; m++) x[m] = hs[clampi(i - 2 + m, H) - (ib - kFH)][cc];
                }
                two_sums(x, a[0], a[1]);
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    if (!(e ? ok1 : ok0)) continue;
                    const int r = r0 + e;
                    double dt;
                    blend_imdt(s1v[e], a[e], bl[r][cc], dt);
                    if (r >= 2 && r < kFT + 2 && cc >= 2 && cc < kFT + 2) it[r - 2][cc - 2] = dt;
                }
            }
        }
        if (k + 1 < PLANES) load_s1(k + 1);
        __syncthreads();
        // -- P4: derivatives, psi and the channel's terms of the own cell (assemble_cell, FAST)
        if (own) {
            // tap_sum<2>(d, ...) four times, KEPT IN PLACE: through the function the kernel is at its SGPR limit elsewhere -- eight
            // instances gain a private segment, SGPR spills to VGPR lanes 116 -> 171 (profiles/level_once_isa.txt)
            double gx = 0.0, gy = 0.0;
            if (interior) {
#pragma unroll
                for (int l = -2; l <= 2; l++) gx += bl[orow + 2][ocol + 2 + l] * d.t[l + 2];
#pragma unroll
                for (int l = -2; l <= 2; l++) gy += bl[orow + 2 + l][ocol + 2] * d.t[l + 2];
            } else {
#pragma unroll
                for (int l = -2; l <= 2; l++) gx += bl[orow + 2][clampi(oj + l, W) - (j0 - 2)] * d.t[l + 2];
#pragma unroll
                for (int l = -2; l <= 2; l++) gy += bl[clampi(oi + l, H) - (ib - 2)][ocol + 2] * d.t[l + 2];
            }
            const double gt = it[orow][ocol];
            double t = gt;
            t *= t;
            s.add(psi_value(t), gx, gy, gt, PLANES == 1);
        }
        // (the next channel's P1 writes raw, last read in P2; its P3 writes bl / it, read above: two barriers lie between)
    }
    if (own) {
        s.mean(PLANES);
        const size_t o = (size_t)oi * W + oj;
        const Nbrs n = nbrs_at(oi, oj, H, W);
        const PhiAround p{ph[orow + 1][ocol + 1], n.left ? ph[orow + 1][ocol] : 0.0, n.up ? ph[orow][ocol + 1] : 0.0};  // phi from LDS
        // cross_at<true>() on the parked flow: a neighbour that does not exist reads the cell itself and is not used
        const auto cross = [&](const double* c) {
            return Cross{c[0], c[n.left ? -1 : 0], c[n.right ? 1 : 0], c[n.up ? -(HWc + 1) : 0], c[n.down ? HWc + 1 : 0]};
        };
        const Cross cu = cross(&fu[orow + kFH][ocol + kFH]), cv = cross(&fv[orow + kFH][ocol + kFH]);
        if (u_out != nullptr) {  // the flow with the increment: what k_update_warp_phi would have written
            u_out[o] = cu.c;
            v_out[o] = cv.c;
        }
        const SystemCell c = system_cell<true>(s, p, cu, cv, n, alpha, omega);
        if (SKEW) {
            stage_cell(stage, orow, ocol, c);
        } else {
            out.q[0][o] = c.phi;
            out.q[1][o] = c.xy;
            out.q[2][o] = c.a1;
            out.q[3][o] = c.a2;
            out.q[4][o] = c.b1;
            out.q[5][o] = c.b2;
        }
    }
    if (!SKEW) return;
    __syncthreads();
    store_skew_tile(stage, tid, ib, j0, row1, W, sk, reinterpret_cast<double2s*>(out.q[0]),
                    reinterpret_cast<double2s*>(out.q[2]), reinterpret_cast<double2s*>(out.q[4]));
}

// stage helper: SOR operands from already assembled row-major planes (tests / micro-benchmark)
template <bool SKEW>
__global__ void k_sor_prep(const double* __restrict__ phi, const double* __restrict__ imdxy,
                           const double* __restrict__ imdx2, const double* __restrict__ imdy2,
                           const double* __restrict__ rhs1, const double* __restrict__ rhs2, int H, int W,
                           double alpha, double omega, SkewIdx sk, double* __restrict__ o_phi,
                           double* __restrict__ o_xy, double* __restrict__ o_a1, double* __restrict__ o_a2,
                           double* __restrict__ o_b1, double* __restrict__ o_b2) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j;
    double a1, a2;
    const Nbrs n = nbrs_at(i, j, H, W);
    sor_diagonals<true>(phi_around<true>(phi, o, W, n), n, imdx2[o], imdy2[o], alpha, omega, a1, a2);
    const size_t q = sor_index<SKEW>(i, j, W, sk);
    o_phi[q] = phi[o];
    o_xy[q] = imdxy[o];
    o_a1[q] = a1;
    o_a2[q] = a2;
    o_b1[q] = rhs1[o];
    o_b2[q] = rhs2[o];
}

template <bool SKEW>
__global__ void k_sor_unpack(const double* __restrict__ sdu, const double* __restrict__ sdv,
                             double* __restrict__ du, double* __restrict__ dv, int H, int W, SkewIdx sk) {
    const int j = blockIdx.x * BX + threadIdx.x, i = blockIdx.y * BY + threadIdx.y;
    if (j >= W || i >= H) return;
    const size_t o = (size_t)i * W + j;
    if (SKEW) {
        const size_t q = 2 * dudv_cell(i, j, sk);
        du[o] = sdu[q];
        dv[o] = sdu[q + 1];
    } else {
        du[o] = sdu[o];
        dv[o] = sdv[o];
    }
}

// ------------------------------------------------------------------------------------------------
// Phase 6, src/OpticalFlow.cpp:513-516: u += du, v += dv (Image::Add, src/Image.h:1925-1941) and re-warp
// frame 2 with the updated flow -- fused, the update of a pixel only feeds its own warp.
// ------------------------------------------------------------------------------------------------
__global__ void k_update_warp(const double* __restrict__ sdu, const double* __restrict__ sdv, double* __restrict__ u,
                              double* __restrict__ v, const double* __restrict__ im1,
                              const double* __restrict__ im2, double* __restrict__ warp, int H, int W, int planes, Rect rc,
                              int do_warp, unsigned long long* stamp) {
    stamp_now(stamp);
    const int j = rc.x0 + blockIdx.x * BX + threadIdx.x, i = rc.y0 + blockIdx.y * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t o = (size_t)i * W + j;
    double fu = u[o], fv = v[o];
    fu += sdu[o];
    fv += sdv[o];
    u[o] = fu;
    v[o] = fv;
    if (do_warp) warp_pixel(im1, im2, warp, fu, fv, i, j, H, W, planes);
}

// One-GPU path of Phase 6 with the NEXT outer iteration's Phase 2 folded in: u_out = u + du, v_out = v + dv go to
// another pair of planes (the neighbours' old values are still read below), the re-warp uses the new flow, and -- when
// phi_out is given -- phi = 0.5 / sqrt(ux^2 + uy^2 + vx^2 + vy^2 + eps) of the NEW flow (src/OpticalFlow.cpp:295-331, the
// expressions of k_phi) is written as well: u_new(i, j+1) = u(i, j+1) + du(i, j+1) is the same addition its own thread
// performs, hence the same bits.  Saves one launch and one pass over (u, v) per outer iteration.
template <bool SKEW, bool BATCH = false>
__global__ void k_update_warp_phi(const double* __restrict__ sdu, const double* __restrict__ sdv, SkewIdx sk,
                                  const double* __restrict__ u, const double* __restrict__ v,
                                  double* __restrict__ u_out, double* __restrict__ v_out,
                                  const double* __restrict__ im1, const double* __restrict__ im2,
                                  double* __restrict__ warp, double* __restrict__ phi_out, int H, int W, int planes,
                                  int do_warp, unsigned long long* stamp, int row0, int row1, unsigned* __restrict__ wit,
                                  double wit_thr, unsigned mark, BatchK bk) {
    stamp_now(stamp);
    if (BATCH) {  // blockIdx.y: the pair of a batch (common.h: BatchK; warp and phi_out are not used there)
        const size_t p = blockIdx.y;
        sdu += p * bk.d;
        sdv += p * bk.d;
        u += p * bk.uv;
        v += p * bk.uv;
        u_out += p * bk.uv;
        v_out += p * bk.uv;
        batch_frames(bk, p, im1, im2);
        if (wit != nullptr) wit += p * bk.wit;
    }
    int tbx, tby;  // a contiguous run of blocks per XCD (xcd_tile): blocks above each other share the lines of the banded (du, dv)
    if (!xcd_tile((W + BX - 1) / BX, (row1 - row0 + BY - 1) / BY, tbx, tby)) return;
    const int j = tbx * BX + threadIdx.x, i = row0 + tby * BY + threadIdx.y;  // rows row0 .. row1-1
    if (j >= W || i >= row1) return;
    const size_t o = (size_t)i * W + j;
    const auto inc = [&](int ii, int jj, double& a, double& b) {
        if (SKEW) {
            const double2s c = reinterpret_cast<const double2s*>(sdu)[dudv_cell(ii, jj, sk)];
            a = c.x;
            b = c.y;
        } else {
            a = sdu[(size_t)ii * W + jj];
            b = sdv[(size_t)ii * W + jj];
        }
    };
    double a, b;
    inc(i, j, a, b);
    double fu = u[o], fv = v[o];
    fu += a;
    fv += b;
    u_out[o] = fu;
    v_out[o] = fv;
    // WITNESS for the Laplacian-noise guard (see k_warp_smooth_blend, which takes the witnesses wherever another outer
    // iteration follows on the level): behind the LAST update of a level nobody evaluates the warp at the new flow, so here the
    // first `planes` threads of every block evaluate it at their own pixel, one channel each.
    if (wit != nullptr) {
        const int bw = min(W - tbx * BX, BX), bh = min(row1 - (row0 + tby * BY), BY);  // the block's pixels
        const int lin = threadIdx.y * bw + threadIdx.x;
        const size_t np = (size_t)H * W;
        if (np <= 65536) {  // a coarse level: few blocks, so every thread samples (channel = its number within the block mod planes)
            for (int k = bw * bh >= planes ? lin % planes : lin; k < planes; k += bw * bh) {
                const double w = warp_value(im1 + k * np, im2 + k * np, fu, fv, i, j, H, W);
                const double d = fabs(im1[k * np + o] - w);
                if (lap_witness(d, wit_thr)) wit[k] = mark;
            }
        } else if (lap_one_in_sixteen(tbx, tby))  // a large grid
        for (int k = lin; k < planes; k += bw * bh) {  // (one trip of one thread per channel, unless the block has fewer pixels)
            const double w = warp_value(im1 + k * np, im2 + k * np, fu, fv, i, j, H, W);
            const double d = fabs(im1[k * np + o] - w);
            if (lap_witness(d, wit_thr)) wit[k] = mark;
        }
    }
    if (phi_out != nullptr) {
        double ur = 0.0, vr = 0.0, ud = 0.0, vd = 0.0;
        if (j < W - 1) {
            inc(i, j + 1, a, b);
            ur = u[o + 1];
            vr = v[o + 1];
            ur += a;
            vr += b;
        }
        if (i < H - 1) {
            inc(i + 1, j, a, b);
            ud = u[o + W];
            vd = v[o + W];
            ud += a;
            vd += b;
        }
        phi_out[o] = phi_value(fu, fv, ur, vr, ud, vd, j < W - 1, i < H - 1);
    }
    if (do_warp) warp_pixel(im1, im2, warp, fu, fv, i, j, H, W, planes);
}

// ------------------------------------------------------------------------------------------------
// Final warp of the ORIGINAL frames: Image::warpImageBicubicRef src/Image.h:2624-2701 with the Hermite
// coefficients of BicubicCoeff :2497-2530, then threshold() :2031-2045.  gx, gy, gxy are the central
// differences {-0.5,0,0.5} of frame 2 (imfilter_h / imfilter_v / imfilter_v(gx), :2590-2594).
// Corners A=(x0,y0) B=(x1,y0) C=(x0,y1) D=(x1,y1); cXY multiplies dx^X dy^Y; term order as in the
// reference expressions.  Output goes straight to the interleaved HWC buffer handed back to the caller.
// ------------------------------------------------------------------------------------------------
// GRAD: the derivatives at the four corners are taken from frame 2 itself (k_bicubic_grad below), not from gx, gy, gxy
// CC: the channel count as a compile-time constant (the loop over the channels is unrolled: the loads of the next channel are
// in flight while this one is evaluated), or -1: C at run time
template <bool BATCH, bool GRAD, int CC = -1>
__device__ __forceinline__ void bicubic_pixel(const double* __restrict__ im1, const double* __restrict__ im2,
                                              const double* __restrict__ gx, const double* __restrict__ gy,
                                              const double* __restrict__ gxy, const Taps& c3, const double* __restrict__ vx,
                                              const double* __restrict__ vy, double* __restrict__ out, int H, int W, int C,
                                              const Rect& rc, unsigned long long* stamp, int planar_out, int clamp,
                                              const BatchK& bk) {
    if (BATCH) {  // blockIdx.y: the pair of a batch (common.h: BatchK)
        const size_t p = blockIdx.y;
        // gx, gy, gxy are image 2's planes: pair 0's frame 2, or -- a backward pair -- its frame 1, one frame back
        const ptrdiff_t o1 = (ptrdiff_t)batch_frames(bk, p, im1, im2);
        const ptrdiff_t o2 = bk.bw != 0 && p >= bk.bw ? o1 - 2 * (ptrdiff_t)bk.fr : o1;
        gx += o2;
        gy += o2;
        gxy += o2;
        vx += p * bk.uv;
        vy += p * bk.uv;
        out += p * bk.out;
    }
    // planar_out / clamp: the in-loop use on the feature planes (src/OpticalFlow.cpp:517-521 with threshold(), :816
    // without); the final warp of the originals writes interleaved HWC and always clamps.
    stamp_now(stamp);
    int tbx, tby;  // a contiguous run of blocks per XCD (xcd_tile)
    if (!xcd_tile((rc.x1 - rc.x0 + BX - 1) / BX, (rc.y1 - rc.y0 + BY - 1) / BY, tbx, tby)) return;
    const int j = rc.x0 + tbx * BX + threadIdx.x, i = rc.y0 + tby * BY + threadIdx.y;
    if (j >= rc.x1 || i >= rc.y1) return;
    const size_t np = (size_t)H * W, o = (size_t)i * W + j;
    const size_t ostride = planar_out ? np : 1, obase = planar_out ? o : o * C;
    const double x = j + vx[o];
    const double y = i + vy[o];
    if (x < 0 || x > W - 1 || y < 0 || y > H - 1) {
        for (int k = 0; k < C; k++) {
            double r = im1[k * np + o];
            if (clamp) {
                r = r < 0 ? 0.0 : r;
                r = r > 1 ? 1.0 : r;
            }
            out[obase + k * ostride] = r;
        }
        return;
    }
    int x0 = (int)x, y0 = (int)y;
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = clampi(x0, W);
    x1 = clampi(x1, W);
    y0 = clampi(y0, H);
    y1 = clampi(y1, H);
    const double dx = x - x0, dy = y - y0;
    const double dx2 = dx * dx, dy2 = dy * dy;
    const double dx3 = dx * dx2, dy3 = dy * dy2;
    const size_t a = (size_t)y0 * W + x0, b = (size_t)y0 * W + x1, c = (size_t)y1 * W + x0, d = (size_t)y1 * W + x1;
    // GRAD: the 4 x 4 cells of frame 2 around the corners -- rows clamp(y0 - 1), y0, y1, clamp(y1 + 1), columns alike.  The
    // neighbours of corner row y0 are rows 0, 1, 2 of them and those of y1 rows 1, 2, 3, except where y1 == y0 (the last row):
    // then y1's upper neighbour is row 0 -- a choice kept as a fifth row (nb: corner row 0 or 1, offset d -> row), and alike for
    // x1's left neighbour, so that every operand is the cell k_central3_all reads at the corner: same values, same bits.
    size_t ro[4], co[4];
    if (GRAD) {
        ro[0] = (size_t)clampi(y0 - 1, H) * W, ro[1] = (size_t)y0 * W, ro[2] = (size_t)y1 * W, ro[3] = (size_t)clampi(y1 + 1, H) * W;
        co[0] = clampi(x0 - 1, W), co[1] = x0, co[2] = x1, co[3] = clampi(x1 + 1, W);
    }
    const auto nb = [](int corner, int d) { return corner == 0 ? 1 + d : (d == -1 ? 4 : 2 + d); };
    const int nc = CC > 0 ? CC : C;
#pragma unroll
    for (int k = 0; k < nc; k++) {
        const double* f = im2 + k * np;
        double fA, fB, fC, fD, xA, xB, xC, xD, yA, yB, yC, yD, zA, zB, zC, zD;
        if (GRAD) {
            double e[5][4], h[5][2];  // the cells, and central3_h of each row of them at the columns x0 and x1
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) e[r][q] = f[ro[r] + co[q]];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double left1 = x1 != x0 ? e[r][1] : e[r][0];  // x1's left neighbour
                h[r][0] = central3_h(c3, [&](int, int dc) { return e[r][1 + dc]; });
                h[r][1] = central3_h(c3, [&](int, int dc) { return dc == -1 ? left1 : e[r][2 + dc]; });
            }
#pragma unroll
            for (int q = 1; q <= 2; q++) e[4][q] = y1 != y0 ? e[1][q] : e[0][q];  // y1's upper neighbour: the cells of x0 and x1,
#pragma unroll
            for (int cx = 0; cx < 2; cx++) h[4][cx] = y1 != y0 ? h[1][cx] : h[0][cx];  // and the h pass there (the same row: same bits)
            const auto corner = [&](int cy, int cx, double& fv, double& dxv, double& dyv, double& dxyv) {
                fv = e[1 + cy][1 + cx];
                dxv = h[1 + cy][cx];
                dyv = central3_v(c3, [&](int dr, int) { return e[nb(cy, dr)][1 + cx]; });
                dxyv = central3_hv(c3, [&](int l) { return h[nb(cy, l)][cx]; });
            };
            corner(0, 0, fA, xA, yA, zA);
            corner(0, 1, fB, xB, yB, zB);
            corner(1, 0, fC, xC, yC, zC);
            corner(1, 1, fD, xD, yD, zD);
        } else {
            const double *px = gx + k * np, *py = gy + k * np, *pz = gxy + k * np;
            fA = f[a], fB = f[b], fC = f[c], fD = f[d];
            xA = px[a], xB = px[b], xC = px[c], xD = px[d];
            yA = py[a], yB = py[b], yC = py[c], yD = py[d];
            zA = pz[a], zB = pz[b], zC = pz[c], zD = pz[d];
        }
        const double c00 = fA;
        const double c10 = xA;
        const double c20 = -3 * fA + 3 * fB - 2 * xA - xB;
        const double c30 = 2 * fA - 2 * fB + xA + xB;
        const double c01 = yA;
        const double c11 = zA;
        const double c21 = -3 * yA + 3 * yB - 2 * zA - zB;
        const double c31 = 2 * yA - 2 * yB + zA + zB;
        const double c02 = -3 * fA + 3 * fC - 2 * yA - yC;
        const double c12 = -3 * xA + 3 * xC - 2 * zA - zC;
        const double c22 = 9 * fA - 9 * fB - 9 * fC + 9 * fD + 6 * xA + 3 * xB - 6 * xC - 3 * xD + 6 * yA - 6 * yB +
                           3 * yC - 3 * yD + 4 * zA + 2 * zB + 2 * zC + zD;
        const double c32 = -6 * fA + 6 * fB + 6 * fC - 6 * fD - 3 * xA - 3 * xB + 3 * xC + 3 * xD - 4 * yA + 4 * yB -
                           2 * yC + 2 * yD - 2 * zA - 2 * zB - zC - zD;
        const double c03 = 2 * fA - 2 * fC + yA + yC;
        const double c13 = 2 * xA - 2 * xC + zA + zC;
        const double c23 = -6 * fA + 6 * fB + 6 * fC - 6 * fD - 4 * xA - 2 * xB + 4 * xC + 2 * xD - 3 * yA + 3 * yB -
                           3 * yC + 3 * yD - 2 * zA - zB - 2 * zC - zD;
        const double c33 = 4 * fA - 4 * fB - 4 * fC + 4 * fD + 2 * xA + 2 * xB - 2 * xC - 2 * xD + 2 * yA - 2 * yB +
                           2 * yC - 2 * yD + zA + zB + zC + zD;
        double r = c00 + c01 * dy + c02 * dy2 + c03 * dy3 + c10 * dx + c11 * dx * dy + c12 * dx * dy2 +
                   c13 * dx * dy3 + c20 * dx2 + c21 * dx2 * dy + c22 * dx2 * dy2 + c23 * dx2 * dy3 + c30 * dx3 +
                   c31 * dx3 * dy + c32 * dx3 * dy2 + c33 * dx3 * dy3;
        if (clamp) {
            r = r < 0 ? 0.0 : r;
            r = r > 1 ? 1.0 : r;
        }
        out[obase + k * ostride] = r;
    }
}

template <bool BATCH>  // BATCH: blockIdx.y = the pair of a batch (a separate instantiation: the single call's code is untouched --
                       // offsetting the pointers in the one kernel changed its register allocation and cost 47 us at 1080p)
__global__ void k_bicubic(const double* __restrict__ im1, const double* __restrict__ im2,
                          const double* __restrict__ gx, const double* __restrict__ gy,
                          const double* __restrict__ gxy, const double* __restrict__ vx,
                          const double* __restrict__ vy, double* __restrict__ out, int H, int W, int C, Rect rc,
                          unsigned long long* stamp, int planar_out, int clamp, BatchK bk) {
    bicubic_pixel<BATCH, false>(im1, im2, gx, gy, gxy, Taps{}, vx, vy, out, H, W, C, rc, stamp, planar_out, clamp, bk);
}

// The same warp without derivative planes: 16 loads per pixel and channel from frame 2's 4 x 4 cells instead of 4 from each of
// four planes, and no launch that writes three planes to be read back once (the final warp of a call; a single pair)
__global__ void k_bicubic_grad(const double* __restrict__ im1, const double* __restrict__ im2, Taps c3,
                               const double* __restrict__ vx, const double* __restrict__ vy, double* __restrict__ out, int H,
                               int W, int C, Rect rc, unsigned long long* stamp, int planar_out, int clamp) {
    bicubic_pixel<false, true, -1>(im1, im2, nullptr, nullptr, nullptr, c3, vx, vy, out, H, W, C, rc, stamp, planar_out, clamp,
                                   BatchK{});
}
// ... for three channels, the loop over them unrolled: 98 registers where the loop takes 110, and held to the 96 of five waves per
// SIMD (the allocator gets there without scratch; the kernel is bound by its fp64 arithmetic and the waves that hide its latency)
__global__ __attribute__((amdgpu_waves_per_eu(5, 5))) void k_bicubic_grad3(
    const double* __restrict__ im1, const double* __restrict__ im2, Taps c3, const double* __restrict__ vx,
    const double* __restrict__ vy, double* __restrict__ out, int H, int W, int C, Rect rc, unsigned long long* stamp,
    int planar_out, int clamp) {
    bicubic_pixel<false, true, 3>(im1, im2, nullptr, nullptr, nullptr, c3, vx, vy, out, H, W, C, rc, stamp, planar_out, clamp,
                                  BatchK{});
}

// ------------------------------------------------------------------------------------------------
// The reference's 16-bit flow encoding, OpticalFlow::SaveOpticalFlow / LoadOpticalFlow (src/OpticalFlow.cpp:963-1015):
// q = (unsigned short)((min(max(f, -200), 200) + 200) * 160), (vx, vy) interleaved per pixel (AssembleFlow,
// src/OpticalFlow.h:70-79); back: f = (double)q / 160 - 200.
// ------------------------------------------------------------------------------------------------
__global__ void k_flow_quantize16(const double* __restrict__ vx, const double* __restrict__ vy,
                                  unsigned short* __restrict__ q, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = vx[i], b = vy[i];
    a = (a < -200) ? -200.0 : a;
    a = (a > 200) ? 200.0 : a;
    b = (b < -200) ? -200.0 : b;
    b = (b > 200) ? 200.0 : b;
    q[i * 2] = (unsigned short)((a + 200) * 160);
    q[i * 2 + 1] = (unsigned short)((b + 200) * 160);
}

__global__ void k_flow_dequantize16(const unsigned short* __restrict__ q, double* __restrict__ vx,
                                    double* __restrict__ vy, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vx[i] = (double)q[i * 2] / 160 - 200;
    vy[i] = (double)q[i * 2 + 1] / 160 - 200;
}

// ------------------------------------------------------------------------------------------------
// Flow visualisation of the reference's caller, generateOutputFlowImageFile (Code/Serial/OpticalFlowCalculation.py:
// 143-162): hue = angle / 2 in degrees, saturation 255, value = magnitude min-max normalised to 0..255, converted
// HSV -> BGR as OpenCV's 8-bit path does (float32: h * 6/180, sector table, round to nearest).  PARITY UNPINNED: cv2 is
// not installed here, and cv2.cartToPolar uses a polynomial atan2 (~0.3 degrees), so a hue may differ by one step
// from an OpenCV run; this kernel uses the exact atan2.
// ------------------------------------------------------------------------------------------------
__global__ void k_flow_mag_minmax(const double* __restrict__ vx, const double* __restrict__ vy, size_t n,
                                  double* __restrict__ partial) {  // partial[2*block] = min, [2*block+1] = max
    __shared__ double smin[256], smax[256];
    double lo = INFINITY, hi = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double m = sqrt(vx[i] * vx[i] + vy[i] * vy[i]);
        lo = m < lo ? m : lo;
        hi = m > hi ? m : hi;
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = smin[0];
        partial[2 * blockIdx.x + 1] = smax[0];
    }
}

__global__ void k_flow_bgr(const double* __restrict__ vx, const double* __restrict__ vy, size_t n,
                           const double* __restrict__ partial, int nblocks, unsigned char* __restrict__ bgr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < nblocks; b++) {
        lo = fmin(lo, partial[2 * b]);
        hi = fmax(hi, partial[2 * b + 1]);
    }
    const double x = vx[i], y = vy[i];
    const double mag = sqrt(x * x + y * y);
    double ang = atan2(y, x);  // cv2.cartToPolar: radians in [0, 2 pi)
    if (ang < 0) ang += 2 * M_PI;
    const unsigned char H = (unsigned char)(int)(ang * 180 / M_PI / 2);
    const double scale = hi > lo ? 255.0 / (hi - lo) : 0.0;  // cv2.normalize(..., 0, 255, NORM_MINMAX)
    const unsigned char V = (unsigned char)(int)((mag - lo) * scale);
    // OpenCV HSV2BGR, 8-bit, S = 255
    const float v = V * (1.f / 255.f);
    float h = H * (6.f / 180.f);
    int sector = (int)floorf(h);
    h -= sector;
    sector = ((sector % 6) + 6) % 6;
    const float tab[4] = {v, 0.f, v * (1.f - h), v * h};
    const int sd[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
    bgr[i * 3] = (unsigned char)(int)rintf(tab[sd[sector][0]] * 255.f);
    bgr[i * 3 + 1] = (unsigned char)(int)rintf(tab[sd[sector][1]] * 255.f);
    bgr[i * 3 + 2] = (unsigned char)(int)rintf(tab[sd[sector][2]] * 255.f);
}

}  // namespace

// ================================================================================================
// host-side tap tables and launch wrappers
// ================================================================================================
Taps gaussian_taps(double sigma, int fsize) {  // src/Image.h:1203-1219
    Taps f{};
    f.fsize = fsize;
    double sum = 0;
    const double s2 = sigma * sigma * 2;
    for (int i = -fsize; i <= fsize; i++) {
        f.t[i + fsize] = std::exp(-(double)(i * i) / s2);
        sum += f.t[i + fsize];
    }
    for (int i = 0; i < 2 * fsize + 1; i++) f.t[i] /= sum;
    return f;
}

Taps smooth5_taps() {  // src/OpticalFlow.cpp:84
    Taps f{};
    f.fsize = 2;
    const double g[5] = {0.02, 0.11, 0.74, 0.11, 0.02};
    for (int i = 0; i < 5; i++) f.t[i] = g[i];
    return f;
}

Taps deriv5_taps() {  // src/Image.h:987-992
    Taps f{};
    f.fsize = 2;
    const double d[5] = {1, -8, 0, 8, -1};
    for (int i = 0; i < 5; i++) {
        f.t[i] = d[i];
        f.t[i] /= 12;
    }
    return f;
}

Taps central3_taps() {  // src/Image.h:2589
    Taps f{};
    f.fsize = 1;
    f.t[0] = -0.5;
    f.t[1] = 0;
    f.t[2] = 0.5;
    return f;
}

#define LAUNCH_CHECK() PAPOF_HIP(hipGetLastError())

const SkewIdx kNoSkew{};  // operands that are not in the exact-order solver's skewed layout
const BatchK kNoBatch{};  // a single call (common.h: BatchK)

// The rows row0 .. row1-1 of a plane that a wrapper works on (row1 < 0: down to the last row).  false: nothing to launch,
// rc says why -- PAPOF_EINVAL for a range outside the plane, PAPOF_OK for an empty one.
static bool rows_of(int row0, int& row1, int H, int& rc) {
    if (row1 < 0) row1 = H;
    rc = row0 < 0 || row1 > H ? PAPOF_EINVAL : PAPOF_OK;
    return rc == PAPOF_OK && row1 > row0;
}

// the witness threshold of the Laplacian-noise guard: a sample of 2e-20 x pixels keeps the mean over at most that many
// samples at or above 1e-20 (lap_witness())
static double lap_wit_threshold(int H, int W) { return 2e-20 * (double)H * (double)W; }

// run-time flags -> template arguments: f(std::bool_constant<flag>...), every call of f returning the same type (a kernel)
template <class F>
static auto with_flags(F f) {
    return f();
}
template <class F, class... Rest>
static auto with_flags(F f, bool flag, Rest... rest) {
    return flag ? with_flags([&](auto... t) { return f(std::true_type{}, t...); }, rest...)
                : with_flags([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}

int hwc_to_planar(papof_handle* h, const double* hwc, double* planar, int H, int W, int C, int frames) {
    hipLaunchKernelGGL(k_hwc_to_planar, grid2d(W, H, frames), dim3(BX, BY), 0, h->stream, hwc, planar, H, W, C);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int hwc_u8_to_planar(papof_handle* h, const unsigned char* hwc, double* planar, int H, int W, int C, int frames) {
    hipLaunchKernelGGL(k_hwc_u8_to_planar, grid2d(W, H, frames), dim3(BX, BY), 0, h->stream, hwc, planar, H, W, C);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int ingest_frames(papof_handle* h, const papof_tensor& a, const papof_tensor* b, double* planar, int H, int W, int C,
                  int frames) {
    const long long total = (long long)frames * H * W * C, blocks = (total + 255) / 256;
    if (total <= 0) return PAPOF_OK;
    if (blocks > 0x7fffffffLL) return PAPOF_EINVAL;
    hipLaunchKernelGGL(k_ingest_frames, dim3((unsigned)blocks), dim3(256), 0, h->stream, a, b ? *b : a, b ? 1 : 0, planar,
                       (long long)H, (long long)W, (long long)C, total);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int init_check(papof_handle* h, const papof_tensor& t, int pairs, int H, int W, unsigned* flag) {
    const long long total = (long long)pairs * H * W * 2, blocks = (total + 255) / 256;
    if (total <= 0) return PAPOF_OK;
    if (blocks > 0x7fffffffLL) return PAPOF_EINVAL;
    hipLaunchKernelGGL(k_init_check, dim3((unsigned)blocks), dim3(256), 0, h->stream, t, (long long)H, (long long)W, total,
                       flag);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int init_sanitize(papof_handle* h, double* planar, size_t n) {
    const long long total = (long long)n, blocks = (total + 255) / 256;
    if (total <= 0) return PAPOF_OK;
    if (blocks > 0x7fffffffLL) return PAPOF_EINVAL;
    hipLaunchKernelGGL(k_init_sanitize, dim3((unsigned)blocks), dim3(256), 0, h->stream, planar, total);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

bool filter_hv_needs_tmp(const Taps& fh, const Taps& fv) { return fh.fsize > kHvMaxF || fv.fsize > kHvMaxF; }

int emit_outputs(papof_handle* h, const double* src, const papof_tensor& dst, bool comp_major, int H, int W, int K, int pairs) {
    const long long total = (long long)pairs * H * W * K, blocks = (total + 255) / 256;
    if (total <= 0) return PAPOF_OK;
    if (blocks > 0x7fffffffLL) return PAPOF_EINVAL;
    hipLaunchKernelGGL(k_emit_outputs, dim3((unsigned)blocks), dim3(256), 0, h->stream, src, dst, comp_major ? 1 : 0,
                       (long long)H, (long long)W, (long long)K, total);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int fb_check(papof_handle* h, hipStream_t st, const papof_tensor& fw, const papof_tensor& bw, const papof_tensor& mask,
             int pairs, int H, int W, double a1, double a2) {
    const long long tiles = (long long)tiles_of(W, kFbTX) * tiles_of(H, kFbTY);
    if (pairs <= 0 || tiles <= 0) return PAPOF_OK;
    if (tiles > kMaxTiles) return PAPOF_EINVAL;
    const auto at = [](const papof_tensor& t, long long items) {  // the same tensor from pair `items` on
        papof_tensor r = t;
        r.data = static_cast<char*>(t.data) + items * t.stride[0] * dtype_bytes(t.dtype);
        return r;
    };
    for (int p0 = 0; p0 < pairs; p0 += 32767) {  // (gridDim.y: two directions of at most 32767 pairs per launch)
        const int n = std::min(32767, pairs - p0);
        hipLaunchKernelGGL(k_fb_check, dim3((unsigned)tiles, 2 * n), dim3(kFbTX, kFbTY), 0, st, at(fw, p0), at(bw, p0),
                           at(mask, p0), H, W, a1, a2);
        LAUNCH_CHECK();
    }
    return PAPOF_OK;
}

int planar_to_hwc(papof_handle* h, const double* planar, double* hwc, int H, int W, int C) {
    hipLaunchKernelGGL(k_planar_to_hwc, grid2d(W, H), dim3(BX, BY), 0, h->stream, planar, hwc, H, W, C);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int filter_h(papof_handle* h, const double* src, double* dst, int H, int W, int planes, const Taps& f, const Rect* rc) {
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_filter_h, grid2d(r, planes), dim3(BX, BY), 0, h->stream, src, dst, H, W, f, r);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int filter_v(papof_handle* h, const double* src, double* dst, int H, int W, int planes, const Taps& f, const Rect* rc) {
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_filter_v, grid2d(r, planes), dim3(BX, BY), 0, h->stream, src, dst, H, W, f, r);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int central3_planes(papof_handle* h, const double* src, double* gx, double* gy, double* gxy, int H, int W, int planes) {
    hipLaunchKernelGGL(k_central3_all, dim3(xcd_grid(tiles_of(W, BX), tiles_of(H, BY)), 1, planes), dim3(BX, BY), 0, h->stream, src, gx, gy, gxy, H, W,
                       central3_taps());
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// dst = v-filter(h-filter(src)) in one launch when both half-widths fit the fused kernel, else through `tmp` (two passes)
int filter_hv(papof_handle* h, const double* src, double* dst, double* tmp, int H, int W, int planes, const Taps& fh,
              const Taps& fv) {
    if (fh.fsize > kHvMaxF || fv.fsize > kHvMaxF) {
        if (!tmp) return PAPOF_EINVAL;
        PAPOF_TRY(filter_h(h, src, tmp, H, W, planes, fh));
        return filter_v(h, tmp, dst, H, W, planes, fv);
    }
    const dim3 grid(tiles_of(W, BX), tiles_of(H, kHvRows), planes), block(BX, BY);
    const int f = fh.fsize == fv.fsize ? fh.fsize : -1;
    if (PAPOF_V_HVSTAGED && f >= 1 && f <= 3) {
        const dim3 sgrid(xcd_grid(tiles_of(W, BX), tiles_of(H, kHvsRows)), 1, planes);
        if (f == 1)
            hipLaunchKernelGGL(k_filter_hv_staged<1>, sgrid, block, 0, h->stream, src, dst, H, W, fh, fv);
        else if (f == 2)
            hipLaunchKernelGGL(k_filter_hv_staged<2>, sgrid, block, 0, h->stream, src, dst, H, W, fh, fv);
        else
            hipLaunchKernelGGL(k_filter_hv_staged<3>, sgrid, block, 0, h->stream, src, dst, H, W, fh, fv);
        LAUNCH_CHECK();
        return PAPOF_OK;
    }
    if (f == 1)
        hipLaunchKernelGGL(k_filter_hv<1>, grid, block, 0, h->stream, src, dst, H, W, fh, fv);
    else if (f == 2)
        hipLaunchKernelGGL(k_filter_hv<2>, grid, block, 0, h->stream, src, dst, H, W, fh, fv);
    else if (f == 3)
        hipLaunchKernelGGL(k_filter_hv<3>, grid, block, 0, h->stream, src, dst, H, W, fh, fv);
    else
        hipLaunchKernelGGL(k_filter_hv<-1>, grid, block, 0, h->stream, src, dst, H, W, fh, fv);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int resize(papof_handle* h, const double* src, double* dst, int sh, int sw, int planes, int dh, int dw, double xr,
           double yr, bool use_post, double post, const Rect* rc) {
    const Rect r = region(rc, dw, dh);
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_resize, dim3(xcd_grid(tiles_of(r.x1 - r.x0, BX), tiles_of(r.y1 - r.y0, BY)), 1, planes), dim3(BX, BY), 0, h->stream, src, dst, sh, sw, dh, dw, xr, yr,
                       use_post ? 1 : 0, post, r, take_stamp(h));
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// One pyramid level, smoothed and resized in one launch (k_smooth_resize).  smooth_resize_fits(): the half-widths are the fused
// kernel's and the largest tile's source footprint fits a workgroup's LDS; otherwise the caller takes filter_hv() and resize().
namespace {
constexpr size_t kSrMaxLds = 64 * 1024;
struct SrShape {
    int nx, ny;
    size_t lds;
};
SrShape sr_shape(int f, int sh, int sw, int dh, int dw, double xr, double yr) {
    const auto span = [](int n_src, int n_dst, double r) {  // most source cells between a tile's first and last tap
        int s = 0;
        for (int p0 = 0; p0 < n_dst; p0 += kSrT)
            s = std::max(s, bilinear_axis(n_src, resize_pos(std::min(p0 + kSrT, n_dst) - 1, r)).c[1] -
                                bilinear_axis(n_src, resize_pos(p0, r)).c[0] + 1);
        return s;
    };
    SrShape s;
    s.nx = (span(sw, dw, xr) + 2 * f) | 1;  // (an odd pitch: the rows of the LDS image start in different banks)
    s.ny = span(sh, dh, yr) + 2 * f;
    s.lds = ((size_t)s.ny * s.nx + (size_t)s.ny * 2 * kSrT) * sizeof(double);
    return s;
}
}  // namespace

bool smooth_resize_fits(const Taps& fh, const Taps& fv, int sh, int sw, int dh, int dw, double xr, double yr) {
    if (fh.fsize != fv.fsize || fh.fsize < 1 || fh.fsize > kHvMaxF || dh < 1 || dw < 1 || !(xr > 0) || !(yr > 0)) return false;
    return sr_shape(fh.fsize, sh, sw, dh, dw, xr, yr).lds <= kSrMaxLds;
}

int smooth_resize(papof_handle* h, const double* src, double* dst, int sh, int sw, int planes, int dh, int dw, double xr,
                  double yr, const Taps& fh, const Taps& fv) {
    if (!smooth_resize_fits(fh, fv, sh, sw, dh, dw, xr, yr)) return PAPOF_EINVAL;
    const SrShape s = sr_shape(fh.fsize, sh, sw, dh, dw, xr, yr);
    const dim3 grid(xcd_grid(tiles_of(dw, kSrT), tiles_of(dh, kSrT)), 1, planes), block(BX, BY);
#define PAPOF_SR(FF)                                                                                                        \
    do {                                                                                                                    \
        static bool attr_set = false;  /* (more than 48 KB of dynamic LDS is asked for once per kernel) */                  \
        if (!attr_set) {                                                                                                    \
            PAPOF_HIP(hipFuncSetAttribute((const void*)k_smooth_resize<FF>, hipFuncAttributeMaxDynamicSharedMemorySize,     \
                                          (int)kSrMaxLds));                                                                 \
            attr_set = true;                                                                                                \
        }                                                                                                                   \
        hipLaunchKernelGGL(k_smooth_resize<FF>, grid, block, s.lds, h->stream, src, dst, sh, sw, dh, dw, xr, yr, fh, fv,    \
                           s.nx, s.ny);                                                                                     \
    } while (0)
    switch (fh.fsize) {
        case 1: PAPOF_SR(1); break;
        case 2: PAPOF_SR(2); break;
        case 3: PAPOF_SR(3); break;
        default: PAPOF_SR(4); break;
    }
#undef PAPOF_SR
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int im2feature(papof_handle* h, const double* im, double* feat, int H, int W, int C, unsigned* nz, int frames, size_t nz_stride) {
    // frames > 1 (a batch): frame f reads im + f * (C planes), writes feat + f * (5 or 3 planes), flags nz + f * nz_stride
    const size_t np = (size_t)H * W;
    if (C == 3) {
        hipLaunchKernelGGL((frames > 1 ? k_im2feature_tiled<3, true> : k_im2feature_tiled<3, false>), dim3(xcd_grid(tiles_of(W, BX), tiles_of(H, kFeatRows)), frames), dim3(BX, BY), 0,
                           h->stream, im, feat, H, W, deriv5_taps(), nz, h->lap_epoch, 3 * np, 5 * np, nz_stride);
    } else if (C == 1) {
        hipLaunchKernelGGL((frames > 1 ? k_im2feature_tiled<1, true> : k_im2feature_tiled<1, false>), dim3(xcd_grid(tiles_of(W, BX), tiles_of(H, kFeatRows)), frames), dim3(BX, BY), 0,
                           h->stream, im, feat, H, W, deriv5_taps(), nz, h->lap_epoch, np, 3 * np, nz_stride);
    } else {  // src/OpticalFlow.cpp:956-957: any other channel count is passed through
        if (frames != 1) return PAPOF_EINVAL;
        PAPOF_HIP(hipMemcpyAsync(feat, im, sizeof(double) * (size_t)H * W * C, hipMemcpyDeviceToDevice, h->stream));
        return PAPOF_OK;
    }
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int warp_bilinear(papof_handle* h, const double* im1, const double* im2, const double* vx, const double* vy,
                  double* out, int H, int W, int planes, const Rect* rc) {
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_warp, grid2d(r), dim3(BX, BY), 0, h->stream, im1, im2, vx, vy, out, H, W, planes, r,
                       take_stamp(h));
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int smooth_v_blend(papof_handle* h, const double* tmp, const double* im1s, double* blend, double* imdt, int H,
                   int W, int planes, const Rect* rc) {
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_smooth_v_blend, grid2d(r, planes), dim3(BX, BY), 0, h->stream, tmp, im1s, blend, imdt, H, W,
                       smooth5_taps(), r);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

static SkewIdx skew_idx(const SorPlanes& sp) {
    return SkewIdx{sp.sd.hp, sp.sd.qt, sp.sd.rt, sp.sd.nb, sp.sd.npos_d, sp.sd.dpar, sp.sd.band_rows, sp.sd.koff, sp.sd.poff};
}

// `prev` = operands of the previous inner iteration's solve (nullptr in the first one: du = dv = 0)
static Increment increment_of(const SorPlanes* prev, const double* gm = nullptr, const double* lap = nullptr) {
    if (!prev) return Increment{nullptr, nullptr, 0, kNoSkew, gm, lap};
    return Increment{prev->du, prev->dv, prev->skew ? 1 : 0, prev->skew ? skew_idx(*prev) : kNoSkew,
                     gm, lap};
}

int smooth_hv_blend(papof_handle* h, const double* warp, const double* im1s, double* blend, double* imdt, int H,
                    int W, int planes, int row0, int row1) {
    int rc;
    if (!rows_of(row0, row1, H, rc)) return rc;
    hipLaunchKernelGGL(k_smooth_hv_blend, dim3(tiles_of(W, BX), tiles_of(row1 - row0, kFuseRows), planes),
                       dim3(BX, BY), 0, h->stream, warp, im1s, blend, imdt, H, W, smooth5_taps(), take_stamp(h), row0,
                       row1);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int warp_smooth_blend(papof_handle* h, const double* im1, const double* im2, const double* u, const double* v,
                      const double* im1s, double* blend, double* imdt, int H, int W, int planes, unsigned* wit,
                      double* phi_out) {
    hipLaunchKernelGGL(k_warp_smooth_blend, dim3(tiles_of(W, BX), tiles_of(H, kWsRows), planes), dim3(BX, BY), 0,
                       h->stream, im1, im2, u, v, im1s, blend, imdt, H, W, smooth5_taps(), take_stamp(h), wit,
                       lap_wit_threshold(H, W), h->lap_epoch, phi_out);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int compute_phi(papof_handle* h, const double* u, const double* v, const SorPlanes* prev, double* phi, int H, int W,
                const Rect* rc) {
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_phi, grid2d(r), dim3(BX, BY), 0, h->stream, u, v, increment_of(prev), phi, H, W, r,
                       take_stamp(h));
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int assemble_system(papof_handle* h, const double* blend, const double* imdt, const double* phi, const double* u,
                    const double* v, int H, int W, int planes, double alpha, double omega, const SorPlanes& out,
                    double* opt_imdx2, double* opt_imdy2, const SorPlanes* prev, const Rect* rc, const double* gm,
                    const double* lap) {
    const Increment I = increment_of(prev, gm, lap);
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    if (out.skew) {
        if (rc && (r.x0 != 0 || r.x1 != W)) return PAPOF_EINVAL;  // skew layout: whole rows only (strips of a plane)
        // 5 feature channels (colour frames) and 3 (gray frames) have their own instantiation with the channel loop unrolled
        const bool fast = I.du == nullptr && I.gm == nullptr && I.lap == nullptr;  // the default branches (assemble_cell: FAST; 0.04 ms)
        // Where its 109 us at level 0 go (variants of the kernel under rocprofv3, round 3): without the three plane stores 79 us
        // (100 MB at the ~3.3 TB/s a plain fill reaches too), without the stencil loads 82, without sqrt / division 106 -- loads and
        // stores, not arithmetic.  Not kept: tiles of 16x32 / 24x32 / 32x32 / 32x16 (512-byte chunks: 0 ... +0.12 ms per 1080p pair),
        // non-temporal plane stores (+0.26 ms: the solver wants the planes where these stores leave them), the blended tile
        // staged in LDS (+0.05 ms).
        const auto kern = planes == 5   ? (fast ? k_assemble_skew<5, true> : k_assemble_skew<5, false>)
                          : planes == 3 ? (fast ? k_assemble_skew<3, true> : k_assemble_skew<3, false>)
                                        : k_assemble_skew<0, false>;
        hipLaunchKernelGGL(kern, dim3(tiles_of(W, kTileJ), tiles_of(r.y1 - r.y0, kAsmRows)),
                           dim3(256), 0, h->stream, blend, imdt, phi, u, v, H, W, planes, alpha, omega, skew_idx(out),
                           (double2s*)out.phi, (double2s*)out.a1, (double2s*)out.b1, opt_imdx2, opt_imdy2,
                           deriv5_taps(), I, take_stamp(h), r.y0, r.y1);
    } else {
        hipLaunchKernelGGL(k_assemble, grid2d(r), dim3(BX, BY), 0, h->stream, blend, imdt, phi, u, v, H, W, planes,
                           alpha, omega, out.phi, out.xy, out.a1, out.a2, out.b1, out.b2, opt_imdx2, opt_imdy2,
                           deriv5_taps(), I, r, take_stamp(h));
    }
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// k_flow_system: the default branches of warp_smooth_blend() + assemble_system() in one launch (exact-order layout, 5 or 3
// feature channels); returns PAPOF_EINVAL where it does not apply
int flow_system(papof_handle* h, const double* im1, const double* im2, const double* u, const double* v, const double* im1s,
                int H, int W, int planes, double alpha, double omega, const SorPlanes& out, unsigned* wit, int row0, int row1,
                int batch, const BatchK* bk, const SorPlanes* inc, double* u_out, double* v_out) {
    if (planes != 5 && planes != 3) return PAPOF_EINVAL;
    // an increment: whole planes of one pair, in the layout of the operands, and the other pair of planes for the sums
    if (inc && (batch > 1 || row0 != 0 || (row1 >= 0 && row1 != H) || inc->skew != out.skew || !inc->du || !u_out || !v_out ||
                u_out == u || v_out == v))
        return PAPOF_EINVAL;
    if (!inc && (u_out || v_out)) return PAPOF_EINVAL;
    if ((unsigned long long)H * (unsigned long long)W > (1ull << 29)) return PAPOF_EINVAL;  // 32-bit byte offsets into a plane
    int rc;
    if (!rows_of(row0, row1, H, rc)) return rc;
    const dim3 grid(xcd_grid(tiles_of(W, kFT), tiles_of(row1 - row0, kFT)), batch);  // (the kernel maps block -> tile, as xcd_tile does)
    const SixPlanes six{{out.phi, out.xy, out.a1, out.a2, out.b1, out.b2}};
    const auto kern = with_flags([](auto five, auto skew, auto batched, auto one_column) {
        return &k_flow_system<five.value ? 5 : 3, skew.value, batched.value, one_column.value>;
    }, planes == 5, out.skew, batch > 1, W == 1);
    hipLaunchKernelGGL(kern, grid, dim3(kFT * kFT), 0, h->stream, im1, im2, u, v, im1s, H, W, alpha, omega,
                       out.skew ? skew_idx(out) : kNoSkew, six, smooth5_taps(), deriv5_taps(),
                       take_stamp(h), wit, lap_wit_threshold(H, W), h->lap_epoch, row0, row1, bk ? *bk : kNoBatch,
                       inc ? inc->du : nullptr, inc ? inc->dv : nullptr, u_out, v_out);
    h->chain_stats[0]++;
    h->chain_stats[1] += inc != nullptr;
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int laplacian(papof_handle* h, const double* in, const double* weight, double* out, int H, int W) {
    hipLaunchKernelGGL(k_laplacian, grid2d(W, H), dim3(BX, BY), 0, h->stream, in, weight, out, H, W);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int update_warp_phi(papof_handle* h, const SorPlanes& sp, const double* u, const double* v, double* u_out, double* v_out,
                    const double* im1, const double* im2, double* warp, double* phi_out, int H, int W, int planes,
                    bool do_warp, int row0, int row1, unsigned* wit, int batch, const BatchK* bk) {
    if (batch > 1 && (warp || phi_out || do_warp)) return PAPOF_EINVAL;
    if (u == u_out || v == v_out) return PAPOF_EINVAL;
    int rc;
    if (!rows_of(row0, row1, H, rc)) return rc;
    const dim3 grid(xcd_grid(tiles_of(W, BX), tiles_of(row1 - row0, BY)), batch);
    const auto kern = with_flags([](auto skew, auto batched) { return &k_update_warp_phi<skew.value, batched.value>; },
                                 sp.skew, batch > 1);
    hipLaunchKernelGGL(kern, grid, dim3(BX, BY), 0, h->stream, sp.du, sp.dv, sp.skew ? skew_idx(sp) : kNoSkew, u, v, u_out,
                       v_out, im1, im2, warp, phi_out, H, W, planes, do_warp ? 1 : 0, take_stamp(h), row0, row1, wit,
                       lap_wit_threshold(H, W), h->lap_epoch, bk ? *bk : kNoBatch);
    h->chain_stats[2]++;
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// tile path: u += du, v += dv on a region, no warp (the warp follows the halo exchange of u, v)
int update_flow(papof_handle* h, const SorPlanes& sp, double* u, double* v, int H, int W, const Rect& r) {
    if (sp.skew) return PAPOF_EINVAL;
    if (r.empty()) return PAPOF_OK;
    hipLaunchKernelGGL(k_update_warp, grid2d(r), dim3(BX, BY), 0, h->stream, sp.du, sp.dv, u, v, nullptr, nullptr, nullptr,
                       H, W, 0, r, 0, take_stamp(h));
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int flow_quantize16(papof_handle* h, const double* vx, const double* vy, unsigned short* q, size_t n) {
    if (!n) return PAPOF_OK;
    hipLaunchKernelGGL(k_flow_quantize16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, vx, vy, q, n);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int flow_dequantize16(papof_handle* h, const unsigned short* q, double* vx, double* vy, size_t n) {
    if (!n) return PAPOF_OK;
    hipLaunchKernelGGL(k_flow_dequantize16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, q, vx, vy, n);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int flow_to_bgr(papof_handle* h, const double* vx, const double* vy, size_t n, double* partial /* 2 * 256 */,
                unsigned char* bgr) {
    if (!n) return PAPOF_OK;
    const int nblocks = 256;
    hipLaunchKernelGGL(k_flow_mag_minmax, dim3(nblocks), dim3(256), 0, h->stream, vx, vy, n, partial);
    hipLaunchKernelGGL(k_flow_bgr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, vx, vy, n, partial,
                       nblocks, bgr);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int bicubic_warp(papof_handle* h, const double* im1, const double* im2, const double* gx, const double* gy,
                 const double* gxy, const double* vx, const double* vy, double* out_hwc, int H, int W, int C,
                 const Rect* rc, bool planar_out, bool clamp, int batch, const BatchK* bk) {
    const Rect r = region(rc, W, H);
    if (r.empty()) return PAPOF_OK;
    if (!gx) {  // no derivative planes: they are taken from frame 2 itself
        if (gy || gxy || batch > 1) return PAPOF_EINVAL;
        hipLaunchKernelGGL(C == 3 ? k_bicubic_grad3 : k_bicubic_grad, dim3(xcd_grid(tiles_of(r.x1 - r.x0, BX), tiles_of(r.y1 - r.y0, BY))), dim3(BX, BY), 0, h->stream, im1, im2,
                           central3_taps(), vx, vy, out_hwc, H, W, C, r, take_stamp(h), planar_out ? 1 : 0, clamp ? 1 : 0);
        LAUNCH_CHECK();
        return PAPOF_OK;
    }
    hipLaunchKernelGGL(batch > 1 ? k_bicubic<true> : k_bicubic<false>, dim3(xcd_grid(tiles_of(r.x1 - r.x0, BX), tiles_of(r.y1 - r.y0, BY)), batch), dim3(BX, BY), 0, h->stream, im1, im2, gx, gy, gxy, vx, vy, out_hwc, H, W,
                       C, r, take_stamp(h), planar_out ? 1 : 0, clamp ? 1 : 0, bk ? *bk : kNoBatch);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// ------------------------------------------------------------------------------------------------
// OpticalFlow::estGaussianMixture, src/OpticalFlow.cpp:539-591 (prior 0.9): three EM iterations over all pixels and
// channels.  One iteration = one reduction kernel (per channel: sum w1, sum w2, sum w1*d^2, sum w2*d^2 with the weights
// of the CURRENT parameters, :551-575; the reference stores the weights, here they are recomputed -- same expressions)
// + one single-block kernel that sums the per-block partials in a fixed order and applies the M step (:576-583, with
// the reference's quirk of accumulating onto the reset values 0.05 / 0.5).  The reference sums sequentially over the
// pixels; a parallel sum rounds differently in the last bits: this branch is checked with a tolerance.
// Deterministic: fixed grid, fixed in-block tree, fixed order over the blocks.
// ------------------------------------------------------------------------------------------------
constexpr int kGmBlocks = 256, kGmThreads = 256, kGmMaxC = 8;
static __global__ __launch_bounds__(kGmThreads) void k_gm_partial(const double* __restrict__ im1,
                                                           const double* __restrict__ im2, size_t np, int C,
                                                           const double* __restrict__ gm, double* __restrict__ partial) {
    __shared__ double red[kGmThreads];
    double acc[kGmMaxC][4];
    for (int k = 0; k < kGmMaxC; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
    for (size_t o = (size_t)blockIdx.x * kGmThreads + threadIdx.x; o < np; o += (size_t)kGmBlocks * kGmThreads) {
#pragma unroll
        for (int k = 0; k < kGmMaxC; k++) {
            if (k >= C) break;
            double t = im1[k * np + o] - im2[k * np + o];
            t *= t;
            const double alpha_k = gm[k], sigma = gm[C + k], beta = gm[2 * C + k], s2 = gm[3 * C + k], b2 = gm[4 * C + k];
            double w1 = exp(-t / (2 * s2)) / (2 * 3.1415927 * sigma) * alpha_k;
            double w2 = exp(-t / (2 * b2)) / (2 * 3.1415927 * beta) * (1 - alpha_k);
            const double s = w1 + w2;
            w1 /= s;
            w2 /= s;
            acc[k][0] += w1;
            acc[k][1] += w2;
            acc[k][2] += w1 * t;
            acc[k][3] += w2 * t;
        }
    }
    for (int k = 0; k < C; k++)
        for (int q = 0; q < 4; q++) {
            red[threadIdx.x] = acc[k][q];
            __syncthreads();
            for (int s = kGmThreads / 2; s > 0; s >>= 1) {
                if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
                __syncthreads();
            }
            if (threadIdx.x == 0) partial[((size_t)blockIdx.x * kGmMaxC + k) * 4 + q] = red[0];
            __syncthreads();
        }
}

static __global__ void k_gm_mstep(const double* __restrict__ partial, int C, double prior, double* __restrict__ gm) {
    const int k = threadIdx.x;
    if (k >= C) return;
    double t1 = 0.0, t2 = 0.0, s1 = 0.05, s2 = 0.5;  // para.reset() before the accumulation (:564, src/NoiseModel.h:97-107)
    for (int b = 0; b < kGmBlocks; b++) {
        const double* p = partial + ((size_t)b * kGmMaxC + k) * 4;
        t1 += p[0];
        t2 += p[1];
        s1 += p[2];
        s2 += p[3];
    }
    const double alpha = t1 / (t1 + t2) * (1 - prior) + 0.95 * prior;
    const double sigma = sqrt(s1 / t1);
    const double beta = sqrt(s2 / t2) * (1 - prior) + 0.3 * prior;
    gm[k] = alpha;
    gm[C + k] = sigma;
    gm[2 * C + k] = beta;
    gm[3 * C + k] = sigma * sigma;
    gm[4 * C + k] = beta * beta;
}

int gm_scratch_doubles() { return kGmBlocks * kGmMaxC * 4; }

// gm (device, 5 * C doubles) in/out; scratch: gm_scratch_doubles() doubles
int est_gaussian_mixture(papof_handle* h, const double* im1, const double* im2, int H, int W, int C, double* gm,
                         double* scratch) {
    if (C > kGmMaxC) return PAPOF_EINVAL;
    for (int it = 0; it < 3; it++) {
        hipLaunchKernelGGL(k_gm_partial, dim3(kGmBlocks), dim3(kGmThreads), 0, h->stream, im1, im2, (size_t)H * W, C, gm,
                           scratch);
        hipLaunchKernelGGL(k_gm_mstep, dim3(1), dim3(64), 0, h->stream, scratch, C, 0.9, gm);
    }
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// ------------------------------------------------------------------------------------------------
// OpticalFlow::estLaplacianNoise, src/OpticalFlow.cpp:594-639, for the EXACT pass of the Laplacian-noise guard (api.hip:
// LapGuard; only calls whose optimistic pass found a channel without a witness get here): per channel the mean of
// |Im1 - warpIm2| over the samples in (0, 1e6), 0.001 when there is none.  The warped frame is evaluated on the fly (it is
// never materialised on this path; u == nullptr: im2 is the warped frame, the bicubic branch).  One reduction kernel (per block: sum and count in a fixed tree) + one single-block
// kernel that adds the blocks' partials in block order: deterministic; the reference adds sequentially over the pixels, so
// the mean can differ in its last bits -- it only feeds the `< 1E-20` test.
// ------------------------------------------------------------------------------------------------
constexpr int kLapBlocks = 256, kLapThreads = 256, kLapMaxC = 8;
static __global__ __launch_bounds__(kLapThreads) void k_lap_partial(const double* __restrict__ im1,
                                                             const double* __restrict__ im2,
                                                             const double* __restrict__ u, const double* __restrict__ v,
                                                             int H, int W, int C, double* __restrict__ partial) {
    __shared__ double red[kLapThreads];
    const size_t np = (size_t)H * W;
    double acc[kLapMaxC][2];
    for (int k = 0; k < kLapMaxC; k++) acc[k][0] = acc[k][1] = 0.0;
    for (size_t o = (size_t)blockIdx.x * kLapThreads + threadIdx.x; o < np; o += (size_t)kLapBlocks * kLapThreads) {
        const int i = (int)(o / W), j = (int)(o - (size_t)i * W);
        const double fu = u ? u[o] : 0.0, fv = u ? v[o] : 0.0;  // u == nullptr: im2 IS the warped frame (bicubic branch)
#pragma unroll
        for (int k = 0; k < kLapMaxC; k++) {
            if (k >= C) break;
            const double w = u ? warp_value(im1 + k * np, im2 + k * np, fu, fv, i, j, H, W) : im2[k * np + o];
            const double d = fabs(im1[k * np + o] - w);
            if (lap_valid(d)) {
                acc[k][0] += d;
                acc[k][1] += 1.0;
            }
        }
    }
    for (int k = 0; k < C; k++)
        for (int q = 0; q < 2; q++) {
            red[threadIdx.x] = acc[k][q];
            __syncthreads();
            for (int s = kLapThreads / 2; s > 0; s >>= 1) {
                if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
                __syncthreads();
            }
            if (threadIdx.x == 0) partial[((size_t)blockIdx.x * kLapMaxC + k) * 2 + q] = red[0];
            __syncthreads();
        }
}
static __global__ void k_lap_finish(const double* __restrict__ partial, int C, double* __restrict__ lap) {
    const int k = threadIdx.x;
    if (k >= C) return;
    double s = 0.0, n = 0.0;
    for (int b = 0; b < kLapBlocks; b++) {
        s += partial[((size_t)b * kLapMaxC + k) * 2];
        n += partial[((size_t)b * kLapMaxC + k) * 2 + 1];
    }
    lap[k] = n == 0 ? 0.001 : s / n;
}
// The witness / no-valid-sample check of k_warp_smooth_blend's exhaustive mode for the LAST outer iteration of a one-block
// level (nobody evaluates the warp at that flow): one block per channel over every pixel.
static __global__ __launch_bounds__(256) void k_lap_small(const double* __restrict__ im1, const double* __restrict__ im2,
                                                       const double* __restrict__ u, const double* __restrict__ v, int H,
                                                       int W, unsigned* __restrict__ wit, double wit_thr, unsigned mark,
                                                       BatchK bk) {
    const int np = H * W;
    {   // blockIdx.y: the pair of a batch (common.h: BatchK)
        const size_t p = blockIdx.y;
        batch_frames(bk, p, im1, im2);
        u += p * bk.uv;
        v += p * bk.uv;
        wit += p * bk.wit;
    }
    const double *p1 = im1 + (size_t)blockIdx.x * np, *p2 = im2 + (size_t)blockIdx.x * np;
    bool hit = false, valid = false;
    for (int o = threadIdx.x; o < np; o += 256) {
        const int i = o / W, j = o - i * W;
        const double d = fabs(p1[o] - warp_value(p1, p2, u[o], v[o], i, j, H, W));
        valid = valid || lap_valid(d);
        hit = hit || lap_witness(d, wit_thr);
    }
    const int any_hit = __syncthreads_or(hit ? 1 : 0), any_valid = __syncthreads_or(valid ? 1 : 0);
    if (threadIdx.x == 0 && (any_hit || !any_valid)) wit[blockIdx.x] = any_hit ? mark : (mark ^ kLapNone);
}
// The same two flags over a RANGE OF ROWS (every pixel of rows r0 .. r1-1), for a rank of the exact-order band split
// (tiles.hip: bands_flow): wit[k] = mark when a sample witnesses, val[k] = mark when the rows hold a valid sample at all.
// Proofs combine over the ranks: a witness anywhere, or no valid sample anywhere.
static __global__ __launch_bounds__(256) void k_lap_rows(const double* __restrict__ im1, const double* __restrict__ im2,
                                                      const double* __restrict__ u, const double* __restrict__ v, int H,
                                                      int W, int r0, int r1, unsigned* __restrict__ wit,
                                                      unsigned* __restrict__ val, double wit_thr, unsigned mark) {
    const size_t np = (size_t)H * W;
    const double *p1 = im1 + blockIdx.y * np, *p2 = im2 + blockIdx.y * np;
    bool hit = false, valid = false;
    const int n = (r1 - r0) * W;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) {
        const int i = r0 + c / W, j = c - (c / W) * W;
        const size_t o = (size_t)i * W + j;
        const double d = fabs(p1[o] - warp_value(p1, p2, u[o], v[o], i, j, H, W));
        valid = valid || lap_valid(d);
        hit = hit || lap_witness(d, wit_thr);
    }
    const int any_hit = __syncthreads_or(hit ? 1 : 0), any_valid = __syncthreads_or(valid ? 1 : 0);
    if (threadIdx.x == 0) {
        if (any_hit) wit[blockIdx.y] = mark;
        if (any_valid) val[blockIdx.y] = mark;
    }
}
int lap_rows_check(papof_handle* h, const double* im1, const double* im2, const double* u, const double* v, int H, int W,
                   int C, int r0, int r1, unsigned* wit, unsigned* val, unsigned mark) {
    if (r1 <= r0) return PAPOF_OK;
    const int blocks = std::min(256, ((r1 - r0) * W + 255) / 256);
    hipLaunchKernelGGL(k_lap_rows, dim3(blocks, C), dim3(256), 0, h->stream, im1, im2, u, v, H, W, r0, r1, wit, val,
                       lap_wit_threshold(H, W), mark);
    LAUNCH_CHECK();
    return PAPOF_OK;
}
bool lap_one_block_level(int H, int W) { return H <= kWsRows && W <= BX; }
int lap_small_check(papof_handle* h, const double* im1, const double* im2, const double* u, const double* v, int H, int W,
                    int C, unsigned* wit, int batch, const BatchK* bk) {
    hipLaunchKernelGGL(k_lap_small, dim3(C, batch), dim3(256), 0, h->stream, im1, im2, u, v, H, W, wit,
                       lap_wit_threshold(H, W), h->lap_epoch, bk ? *bk : kNoBatch);
    LAUNCH_CHECK();
    return PAPOF_OK;
}
int lap_scratch_doubles() { return kLapBlocks * kLapMaxC * 2; }
int est_laplacian_noise(papof_handle* h, const double* im1, const double* im2, const double* u, const double* v, int H,
                        int W, int C, double* lap, double* scratch) {
    if (C > kLapMaxC) return PAPOF_EINVAL;
    hipLaunchKernelGGL(k_lap_partial, dim3(kLapBlocks), dim3(kLapThreads), 0, h->stream, im1, im2, u, v, H, W, C, scratch);
    hipLaunchKernelGGL(k_lap_finish, dim3(1), dim3(64), 0, h->stream, scratch, C, lap);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

// closes the last phase of a call: a one-thread kernel that only writes the pending stamp (if any)
int stamp_only(papof_handle* h) {
    unsigned long long* s = take_stamp(h);
    if (!s) return PAPOF_OK;
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, h->stream, s);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int sor_prep(papof_handle* h, const double* phi, const double* imdxy, const double* imdx2, const double* imdy2,
             const double* rhs1, const double* rhs2, int H, int W, double alpha, double omega, const SorPlanes& out) {
    if (out.skew)
        hipLaunchKernelGGL(k_sor_prep<true>, grid2d(W, H), dim3(BX, BY), 0, h->stream, phi, imdxy, imdx2, imdy2,
                           rhs1, rhs2, H, W, alpha, omega, skew_idx(out), out.phi, out.xy, out.a1, out.a2, out.b1,
                           out.b2);
    else
        hipLaunchKernelGGL(k_sor_prep<false>, grid2d(W, H), dim3(BX, BY), 0, h->stream, phi, imdxy, imdx2, imdy2,
                           rhs1, rhs2, H, W, alpha, omega, kNoSkew, out.phi, out.xy, out.a1, out.a2, out.b1,
                           out.b2);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

int sor_unpack(papof_handle* h, const SorPlanes& sp, double* du, double* dv, int H, int W) {
    if (sp.skew)
        hipLaunchKernelGGL(k_sor_unpack<true>, grid2d(W, H), dim3(BX, BY), 0, h->stream, sp.du, sp.dv, du, dv, H, W,
                           skew_idx(sp));
    else
        hipLaunchKernelGGL(k_sor_unpack<false>, grid2d(W, H), dim3(BX, BY), 0, h->stream, sp.du, sp.dv, du, dv, H,
                           W, kNoSkew);
    LAUNCH_CHECK();
    return PAPOF_OK;
}

}  // namespace papof
