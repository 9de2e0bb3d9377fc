// papteam_opticalflow_amd/csrc/sampler.h -- what the device-tensor video kernels share, written once: the bilinear sampler of
// frames and flows at non-integer points (k_interp, k_warp_affine, k_temporal_filter, k_propagate, the fill and consistency
// kernels, k_track, k_fb_check), the forward-backward test and the hop of a point through a pair's flows (k_track,
// k_temporal_filter, k_propagate, k_tc_setup; the test also k_fb_check), the interpolation rule at one output pixel (k_interp,
// k_interp_splat, k_motion_blur), the block's table of uint8 quotients (stage_u8_lut), and on the host the pyramid level
// sizes of the fill and consistency workspaces.  The (tile, item) grid these kernels are launched over -- tile decode, tile
// count, split launches, the choice of an instance by dtype -- is grid.h's.
//
// Two decisions that several files must know are stated here once: the direction rule of a chain of
// hops through a video's flows (chain_flow, chain_check, chain_pair, chain_frame, chain_steps, chain_hop, hop_from: which
// flow a hop reads, which it is checked with, through which pair, how many steps), and the element format of a
// papof_tensor (PAPOF_AT, PAPOF_AT_CH, load_u8, store_u8, store_plane; kMaxChannels).
//
// The rule is the reference's (src/ImageProcessing.h:138-157): truncation toward zero, fraction clamped to [0, 1], neighbours
// clamped into the image, taps accumulated from 0 in (m, n) order; fp64 without contraction (-ffp-contract=off).  Frames are
// papof_tensor descriptors (frame, row, column, channel) of uint8 (x / 255.0, as k_ingest_frames computes it), float32
// (widened exactly) or float64.
#pragma once

#include "common.h"
#include "grid.h"

namespace papof {

namespace {

// The 256 quotients k / 255.0 of a uint8 sample, one per lane of a 256-lane block: the block fills its table once and
// synchronises before the first load_frame (the same bits as a division per tap, without the fp64 division).
__device__ __forceinline__ void fill_u8_lut(double* lut, int k) { lut[k] = (double)k / 255.0; }

// The prologue of a kernel whose frames are of dtype FD and whose block is TX lanes wide (0: a row of lanes) and 256 lanes in
// all: each lane fills the quotient of its linear index and the block synchronises, where a uint8 sample can occur (FD uint8, or -1: read
// from each descriptor).  It stands before any lane's early return: every lane of the block reaches the barrier.
template <int FD, int TX = 0>
__device__ __forceinline__ void stage_u8_lut(double* lut) {
    if (FD == PAPOF_DTYPE_U8 || FD < 0) {
        fill_u8_lut(lut, TX ? threadIdx.y * TX + threadIdx.x : threadIdx.x);
        __syncthreads();
    }
}

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

constexpr int kMaxChannels = 4;  // channels of a frame tensor (registers per lane: centre values, sums, samples)

// ---- the elements of a papof_tensor: offsets in elements, 64-bit, by the descriptor's strides ----
//   PAPOF_AT(t, i, r, x)         element (i, r, x, 0) of t: item (frame, pair ...) i, row r, column x
//   PAPOF_AT_CH(t, i, r, x, ch)  element (i, r, x, ch)
// Every index is widened by the 64-bit stride it multiplies: the offset is 64-bit whatever the indices' types.
//
// Why macros, as grid.h's decode: a function at(t, i, r, x) was written first, taking long long, then the caller's types,
// then references.  A callee is optimised on its own before it is inlined, and the sum's operands are ordered there, not
// among the kernel's values: k_temporal_filter's address chain came out as data + r s1 + t s0 where it was data + t s0 + r s1,
// and its scalar address arithmetic was scheduled differently (profiles/flow_chain_isa.txt).  Text expanded in place
// leaves every kernel as it was.
#define PAPOF_AT(t, i, r, x) ((i) * (t).stride[0] + (r) * (t).stride[1] + (x) * (t).stride[2])
#define PAPOF_AT_CH(t, i, r, x, ch) ((i) * (t).stride[0] + (r) * (t).stride[1] + (x) * (t).stride[2] + (ch) * (t).stride[3])

// a byte of a uint8 descriptor (mask, support, status, valid plane) at offset o
__device__ __forceinline__ unsigned char load_u8(const papof_tensor& t, long long o) {
    return static_cast<const unsigned char*>(t.data)[o];
}

__device__ __forceinline__ void store_u8(const papof_tensor& t, long long o, unsigned char v) {
    static_cast<unsigned char*>(t.data)[o] = v;
}

// v into a float32 (one round-to-nearest) or float64 plane (score, coverage ...)
__device__ __forceinline__ void store_plane(const papof_tensor& t, long long o, double v) {
    if (t.dtype == PAPOF_DTYPE_F32)
        static_cast<float*>(t.data)[o] = (float)v;
    else
        static_cast<double*>(t.data)[o] = v;
}

__device__ __forceinline__ int clamp_to(int x, int n) {  // EnforceRange, src/ImageProcessing.h:34
    x = x < 0 ? 0 : x;
    return x > n - 1 ? n - 1 : x;
}

// The four taps of the bilinear rule at (X, Y), a point of [0, W - 1] x [0, H - 1], in (m, n) order: their (row, column)
// offsets in elements of a tensor whose row and column strides are s1, s2 -- for frames and mask alike, offsets are computed
// per tensor -- and their weights.  (common.h's Taps are the 1-D correlation taps of the flow's filters.)
struct Bilinear {
    int row[4], col[4];
    double w[4];
};

__device__ __forceinline__ Bilinear taps_at(double X, double Y, int H, int W) {
    Bilinear k;
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

// (u, v) = the flow t (pair, row, column, {vx, vy}) sampled at the taps from `base` (the pair's offset), both components
// accumulated from 0 in (m, n) order.
__device__ __forceinline__ void sample_flow(const papof_tensor& t, long long base, const Bilinear& k, double& u, double& v) {
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
__device__ __forceinline__ double sample_frame(const papof_tensor& t, long long base, const Bilinear& k, const double* lut) {
    double g = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) g += load_frame<FD>(t, base + k.row[i] * t.stride[1] + k.col[i] * t.stride[2], lut) * k.w[i];
    return g;
}

// The forward-backward test (Sundaram, Brox, Keutzer 2010) of a flow (u, v) and the reverse flow (bu, bv) where it lands:
// |(u, v) + (bu, bv)|^2 <= a1 (|(u, v)|^2 + |(bu, bv)|^2) + a2, false for a NaN.
__device__ __forceinline__ bool fb_passes(double u, double v, double bu, double bv, double a1, double a2) {
    const double du = u + bu, dv = v + bv;
    const double e = du * du + dv * dv;
    const double mag = (u * u + v * v) + (bu * bu + bv * bv);
    return e <= a1 * mag + a2;
}

// One hop of the point (X, Y) through pair `pair` of the flow f (pair, row, column, {vx, vy}): (nX, nY) = (X, Y) + f sampled
// at (X, Y).  True where (nX, nY) lies in [0, W - 1] x [0, H - 1] (false for a NaN) and, with `check`, the reverse flow b
// sampled there passes fb_passes.
__device__ __forceinline__ bool hop(const papof_tensor& f, const papof_tensor& b, long long pair, int H, int W, int check,
                                    double a1, double a2, double X, double Y, double& nX, double& nY) {
    double u, v;
    sample_flow(f, pair * f.stride[0], taps_at(X, Y, H, W), u, v);
    nX = X + u;
    nY = Y + v;
    bool alive = nX >= 0 && nX <= (double)(W - 1) && nY >= 0 && nY <= (double)(H - 1);
    if (alive && check) {
        double bu, bv;
        sample_flow(b, pair * b.stride[0], taps_at(nX, nY, H, W), bu, bv);
        alive = fb_passes(u, v, bu, bv, a1, a2);
    }
    return alive;
}

// ---- THE DIRECTION RULE of a chain of hops through a video's flows, stated once ----
// Pair p of flow_fw runs from frame p to p + 1, pair p of flow_bw from frame p + 1 to p.  So
//   a hop forward from frame t reads flow_fw[t] and is checked with flow_bw[t];
//   a hop backward from frame t reads flow_bw[t - 1] and is checked with flow_fw[t - 1];
//   a chain of radius R from frame t takes min(R, T - 1 - t) steps forward and min(R, t) steps backward;
//   step j >= 1 of a chain from t in direction dir = +-1 leaves frame t + dir (j - 1) and reaches frame t + dir j;
//   a hop that fails ends the chain: the caller makes no further hop (once dead, a chain stays dead).
// The functions below are the rule.  Those that read the flows are templated on the kernel's Args: any struct with fw, bw,
// H, W, check, a1, a2, read where the kernels read them; with a literal dir the selection folds away.  hop() above stays the
// primitive for what has no direction (k_fb_check, the interpolation rule).
//
// chain_hop takes H and W from its caller although they are a's: a chain loop keeps `const int H = a.H, W = a.W` in front of
// it for taps_at at the landing point, and the hop uses the same two values, read once per chain and not once per hop (read
// inside the hop, (double)(W - 1) and (double)(H - 1) stay in the loop until a late pass hoists them).  hop_from, with no
// loop of its own, reads them itself.

// the flow a hop in direction dir reads, and the reverse flow it is checked with
template <typename A>
__device__ __forceinline__ const papof_tensor& chain_flow(const A& a, int dir) { return dir > 0 ? a.fw : a.bw; }
template <typename A>
__device__ __forceinline__ const papof_tensor& chain_check(const A& a, int dir) { return dir > 0 ? a.bw : a.fw; }

// the steps a chain of radius R may take from frame t of T
__device__ __forceinline__ int chain_steps(int T, long long t, int dir, int R) {
    return dir > 0 ? (T - 1 - t < R ? (int)(T - 1 - t) : R) : (t < R ? (int)t : R);
}

// the pair that step j of the chain from frame t hops through, and the frame it reaches
__device__ __forceinline__ long long chain_pair(long long t, int dir, int j) { return dir > 0 ? t + j - 1 : t - j; }
__device__ __forceinline__ long long chain_frame(long long t, int dir, int j) { return t + dir * j; }

// the hop of (X, Y) through pair `pair` in direction dir: which flow is read and which it is checked with
template <typename A>
__device__ __forceinline__ bool chain_hop(const A& a, long long pair, int dir, int H, int W, double X, double Y, double& nX,
                                          double& nY) {
    return hop(chain_flow(a, dir), chain_check(a, dir), pair, H, W, a.check, a.a1, a.a2, X, Y, nX, nY);
}

// one hop from frame `from` to frame from + dir: step 1 of the chain from `from` (a dir known only at run time chooses
// between the two hops, each with its flows fixed)
template <typename A>
__device__ __forceinline__ bool hop_from(const A& a, long long from, int dir, double X, double Y, double& nX, double& nY) {
    return dir > 0 ? chain_hop(a, chain_pair(from, +1, 1), +1, a.H, a.W, X, Y, nX, nY)
                   : chain_hop(a, chain_pair(from, -1, 1), -1, a.H, a.W, X, Y, nX, nY);
}

// The photometric weight of a sample against its centre (k_temporal_filter, k_sr_accumulate): D the squared differences
// summed over the C channels, 1 / (1 + mean / s2).
__device__ __forceinline__ double photometric_weight(double D, int C, double s2) {
    D = D / (double)C;
    return 1.0 / (1.0 + D / s2);
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

// One term of a scattered fixed-point sum (k_splat, k_sr_accumulate): a no-return 64-bit integer atomic add at agent scope
// (one global_atomic_add_x2, executed at the memory side; a signed term is added as its two's-complement bits).
__device__ __forceinline__ void add64(unsigned long long* p, long long v) {
    (void)__hip_atomic_fetch_add(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the rule of papof_interp_tensor at one output pixel, shared by k_interp (interp.hip) and by k_interp_splat
// (splat.hip: the pixels that no splat reaches) ----
constexpr int kInterpTX = 64, kInterpTY = 4;   // a 64 x 4 tile of pixels per block (256 lanes: lut)
using InterpTile = Tile<kInterpTX, kInterpTY>;
constexpr int kMaxTimes = 16;                  // times per launch (kernel arguments)

struct InterpArgs {
    papof_tensor f0, f1;  // frames of I0 and I1 (frame, row, column, channel); I1 of pair i is f1's frame i + seq
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy})
    papof_tensor occ;     // uint8 mask (pair, row, column, {O0, O1}); data NULL: none
    papof_tensor out;     // (pair, row, column, channel); time j at + j * tstride
    long long tstride;
    int H, W, C;
    int seq;
    int nt;               // times of this launch
    double t[kMaxTimes];
};

__device__ __forceinline__ double sample_mask(const papof_tensor& t, long long base, const Bilinear& k) {  // bytes as 0 / 1
    const unsigned char* m = static_cast<const unsigned char*>(t.data);
    double o = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) o += (m[base + k.row[i] * t.stride[1] + k.col[i] * t.stride[2]] ? 1.0 : 0.0) * k.w[i];
    return o;
}

// ---- the rule at one output pixel and one time t, in the three steps that k_interp / k_interp_splat (interp_pixel) and
// k_motion_blur (blur.hip) share: where the two samples land, their weights, the blend ----
struct InterpPoints {
    double s, t;      // 1 - t, t
    bool in0, in1;    // q0, q1 in [0, W - 1] x [0, H - 1] (false for a NaN)
    Bilinear k0, k1;  // the taps at q0 and q1 ((0, 0)'s where the point is not in the image)
};

// (u, v) = F01, (bu, bv) = F10 at the pixel (x, r)
__device__ __forceinline__ InterpPoints interp_points(int x, long long r, double u, double v, double bu, double bv, double t,
                                                      int H, int W) {
    InterpPoints p;
    p.t = t;
    p.s = 1.0 - t;
    const double s = p.s;
    const double tt = t * t, st = s * t, ss = s * s;
    const double a0 = tt * bu - st * u, b0 = tt * bv - st * v;  // F_t->0 = -s t F01 + t^2 F10
    const double a1 = ss * u - st * bu, b1 = ss * v - st * bv;  // F_t->1 =  s^2 F01 - s t F10
    const double X0 = (double)x + a0, Y0 = (double)r + b0, X1 = (double)x + a1, Y1 = (double)r + b1;
    // (false for a NaN)
    p.in0 = X0 >= 0 && X0 <= (double)(W - 1) && Y0 >= 0 && Y0 <= (double)(H - 1);
    p.in1 = X1 >= 0 && X1 <= (double)(W - 1) && Y1 >= 0 && Y1 <= (double)(H - 1);
    p.k0 = taps_at(p.in0 ? X0 : 0.0, p.in0 ? Y0 : 0.0, H, W);
    p.k1 = taps_at(p.in1 ? X1 : 0.0, p.in1 ? Y1 : 0.0, H, W);
    return p;
}

struct InterpWeights {
    double c0, c1, den;
};

// o0, o1: the mask sampled at q0 (channel 0) and q1 (channel 1) where both points are in the image and there is a mask, else 0
__device__ __forceinline__ InterpWeights interp_weights(const InterpPoints& p, double o0, double o1) {
    const double w0 = p.in0 ? p.s * (1.0 - o1) : 0.0, w1 = p.in1 ? p.t * (1.0 - o0) : 0.0;
    const bool weighted = w0 + w1 > 0;
    InterpWeights q;
    q.c0 = weighted ? w0 : p.s;
    q.c1 = weighted ? w1 : p.t;
    q.den = weighted ? w0 + w1 : (p.in0 ? p.s : 0.0) + (p.in1 ? p.t : 0.0);
    return q;
}

// one channel where in0 || in1: g0, g1 the frames sampled at q0 and q1 (each read only where its point is in the image)
__device__ __forceinline__ double interp_blend(const InterpPoints& p, const InterpWeights& q, double g0, double g1) {
    const double num = p.in0 && p.in1 ? q.c0 * g0 + q.c1 * g1 : (p.in0 ? q.c0 * g0 : q.c1 * g1);
    return num / q.den;
}

// Pixel (x, r) of pair i at the times a.t[0 .. a.nt), written at time slots j0 + j of out -- except the times j for which
// done(j, offset of the pixel at that time slot in out) is true: those the caller has written (k_interp: none).
template <int FD, typename D>
__device__ __forceinline__ void interp_pixel(const InterpArgs& a, const double* lut, long long i, long long r, int x,
                                             long long j0, D done) {
    const int H = a.H, W = a.W;
    const long long of = PAPOF_AT(a.fw, i, r, x);
    const long long ob = PAPOF_AT(a.bw, i, r, x);
    const double u = load_flow(a.fw, of), v = load_flow(a.fw, of + a.fw.stride[3]);
    const double bu = load_flow(a.bw, ob), bv = load_flow(a.bw, ob + a.bw.stride[3]);
    const long long base0 = i * a.f0.stride[0], base1 = (i + a.seq) * a.f1.stride[0];
    const long long baseo = i * a.occ.stride[0];
    const long long pix0 = base0 + r * a.f0.stride[1] + x * a.f0.stride[2];
    const long long pix1 = base1 + r * a.f1.stride[1] + x * a.f1.stride[2];
    const long long outp = PAPOF_AT(a.out, i, r, x);
    for (int j = 0; j < a.nt; j++) {
        const long long oj = outp + (j0 + j) * a.tstride;
        if (done(j, oj)) continue;
        const InterpPoints p = interp_points(x, r, u, v, bu, bv, a.t[j], H, W);
        double o0 = 0.0, o1 = 0.0;
        if (a.occ.data && p.in0 && p.in1) {
            o0 = sample_mask(a.occ, baseo, p.k0);
            o1 = sample_mask(a.occ, baseo + a.occ.stride[3], p.k1);
        }
        const InterpWeights q = interp_weights(p, o0, o1);
        for (int ch = 0; ch < a.C; ch++) {
            double val;
            if (p.in0 || p.in1) {
                const double g0 = p.in0 ? sample_frame<FD>(a.f0, base0 + ch * a.f0.stride[3], p.k0, lut) : 0.0;
                const double g1 = p.in1 ? sample_frame<FD>(a.f1, base1 + ch * a.f1.stride[3], p.k1, lut) : 0.0;
                val = interp_blend(p, q, g0, g1);
            } else {
                val = p.s * load_frame<FD>(a.f0, pix0 + ch * a.f0.stride[3], lut) + p.t * load_frame<FD>(a.f1, pix1 + ch * a.f1.stride[3], lut);
            }
            store(a.out, oj + ch * a.out.stride[3], val);
        }
    }
}

// The pyramid of the fill's and the consistency solve's workspaces: level l + 1 is ceil(h / 2) x ceil(w / 2) of level l, from
// H x W down to 1 x 1.
std::vector<std::pair<long long, long long>> level_sizes(long long H, long long W) {
    std::vector<std::pair<long long, long long>> s{{H, W}};
    while (s.back().first > 1 || s.back().second > 1) s.push_back({(s.back().first + 1) / 2, (s.back().second + 1) / 2});
    return s;
}

}  // namespace

}  // namespace papof
