// papteam_opticalflow_amd/csrc/sampler.h -- the bilinear sampler of the device-tensor kernels that read frames at
// non-integer points (interp.hip: k_interp, motion.hip: k_warp_affine, denoise.hip: k_temporal_filter), written once.
//
// The rule is the reference's (src/ImageProcessing.h:138-157), as k_fb_check and k_track apply it: truncation toward zero,
// fraction clamped to [0, 1], neighbours clamped into the image, taps accumulated from 0 in (m, n) order; fp64 without
// contraction (-ffp-contract=off).  Frames are papof_tensor descriptors (frame, row, column, channel) of uint8 (x / 255.0, as
// k_ingest_frames computes it), float32 (widened exactly) or float64.
#pragma once

#include "common.h"

namespace papof {

namespace {

// The 256 quotients k / 255.0 of a uint8 sample, one per lane of a 256-lane block: the block fills its table once and
// synchronises before the first load_frame (the same bits as a division per tap, without the fp64 division).
__device__ __forceinline__ void fill_u8_lut(double* lut, int k) { lut[k] = (double)k / 255.0; }

// FD: the dtype of the frame tensors, fixed at compile time (the common case: one branch-free gather per tap), or -1: read
// from each descriptor.  A uint8 sample is looked up in the block's table (fill_u8_lut).
template <int FD>
__device__ __forceinline__ double load_frame(const papof_tensor& t, long long o, const double* lut) {
    const int d = FD >= 0 ? FD : t.dtype;
    if (d == PAPOF_DTYPE_U8) return lut[static_cast<const unsigned char*>(t.data)[o]];
    if (d == PAPOF_DTYPE_F32) return (double)static_cast<const float*>(t.data)[o];
    return static_cast<const double*>(t.data)[o];
}

__device__ __forceinline__ double load_flow(const papof_tensor& t, long long o) {
    return t.dtype == PAPOF_DTYPE_F32 ? (double)static_cast<const float*>(t.data)[o] : static_cast<const double*>(t.data)[o];
}

__device__ __forceinline__ int clamp_to(int x, int n) {  // EnforceRange, src/ImageProcessing.h:34
    x = x < 0 ? 0 : x;
    return x > n - 1 ? n - 1 : x;
}

// The four taps of the bilinear rule at (X, Y), a point of [0, W - 1] x [0, H - 1], in (m, n) order: their (row, column)
// offsets in elements of a tensor whose row and column strides are s1, s2 -- for frames and mask alike, offsets are computed
// per tensor -- and their weights.
struct Taps {
    int row[4], col[4];
    double w[4];
};

__device__ __forceinline__ Taps taps_at(double X, double Y, int H, int W) {
    Taps k;
    const int xx = (int)X, yy = (int)Y;
    double dx = X - xx, dy = Y - yy;
    dx = dx > 1 ? 1.0 : dx;
    dx = dx < 0 ? 0.0 : dx;
    dy = dy > 1 ? 1.0 : dy;
    dy = dy < 0 ? 0.0 : dy;
#pragma unroll
    for (int m = 0; m <= 1; m++)
#pragma unroll
        for (int n = 0; n <= 1; n++) {
            k.row[2 * m + n] = clamp_to(yy + n, H);
            k.col[2 * m + n] = clamp_to(xx + m, W);
            k.w[2 * m + n] = fabs((double)(1 - m) - dx) * fabs((double)(1 - n) - dy);
        }
    return k;
}

// (u, v) = the flow t (pair, row, column, {vx, vy}) sampled at the taps from `base` (the pair's offset): k_track's sample()
// (track.hip), both components accumulated from 0 in (m, n) order.
__device__ __forceinline__ void sample_flow(const papof_tensor& t, long long base, const Taps& k, double& u, double& v) {
    u = 0.0;
    v = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const long long o = base + k.row[i] * t.stride[1] + k.col[i] * t.stride[2];
        u += load_flow(t, o) * k.w[i];
        v += load_flow(t, o + t.stride[3]) * k.w[i];
    }
}

template <int FD>
__device__ __forceinline__ double sample_frame(const papof_tensor& t, long long base, const Taps& k, const double* lut) {
    double g = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) g += load_frame<FD>(t, base + k.row[i] * t.stride[1] + k.col[i] * t.stride[2], lut) * k.w[i];
    return g;
}

// stores as papof_interp_tensor states: float64 as is, float32 with one round-to-nearest, uint8 = clamp(rint(255 v), 0, 255)
// (half to even; NaN -> 0)
__device__ __forceinline__ void store(const papof_tensor& t, long long o, double v) {
    if (t.dtype == PAPOF_DTYPE_U8)  // clamp(rint(255 out), 0, 255), half to even; NaN -> 0 (fmax)
        static_cast<unsigned char*>(t.data)[o] = (unsigned char)fmin(fmax(rint(255.0 * v), 0.0), 255.0);
    else if (t.dtype == PAPOF_DTYPE_F32)
        static_cast<float*>(t.data)[o] = (float)v;
    else
        static_cast<double*>(t.data)[o] = v;
}

}  // namespace

}  // namespace papof
