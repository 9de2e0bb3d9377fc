// papteam_opticalflow_amd/csrc/rolling.hip -- rolling-shutter rectification of a video (papof_rs_rectify_tensor) and of its
// flows (papof_rs_flow_tensor) along the flows.
//
// Why.  A rolling shutter exposes row y of frame t at t + readout * (y - a) / H: a pan shears the picture, a tilt stretches
// it, shake becomes wobble, and every motion fit on the flows sees that distortion.  The forward and backward flows give each
// pixel's position one frame earlier and one frame later, each at its landing row's own time; the parabola through the three
// points, evaluated at the frame's time, is the pixel's global-shutter position (Liang, Chang, Chen, "Analysis and
// compensation of rolling shutter effect", IEEE TIP 2008, take one velocity per row from block motion; Grundmann et al.,
// "Calibration-free rolling shutter removal", ICCP 2012, fit homography mixtures; here the dense flows are at hand).  The
// output pixel needs the inverse: a fixed-point solve of a few iterations.  Written with grid_sample it is iters + 1
// samplings of two flow fields with full-frame temporaries between them and one more for the frames; here one lane makes one
// output pixel with its iterate in registers, 2 x 4 flow taps per iteration, then the C-channel frame gather.
//
// Semantics: include/papof.h, papof_rs_rectify_tensor.  The samplers are sampler.h's (taps_at, sample_flow, sample_frame),
// fp64 without contraction (-ffp-contract=off); the fp64 divisions are IEEE (the restatement's bits).
//
// Mapping.  A block is a 64 x 4 tile of output pixels (as k_warp_affine's), over grid.h's grid of tiles and frames --
// for k_rs_flow the (pair, direction) slot.  The frame, hence which of the three forms of the displacement applies, is
// uniform over the block; the s == 0 row and a solve that dies early diverge within a wave and cost that wave nothing more
// than the longest lane.  No atomics, no workspace: every output element belongs to one lane.  Every offset is 64-bit.
#include "sampler.h"

#include <cmath>

namespace papof {

namespace {

constexpr int kRsTX = 64, kRsTY = 4;  // a 64 x 4 tile of output pixels per block (256 lanes: lut)
using RsTile = Tile<kRsTX, kRsTY>;
constexpr int kRsMaxIters = 8;
constexpr int kRsMaxC = 4;

struct RsRule {
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy}): fw[t] from frame t to t + 1, bw[t - 1] from frame t to t - 1
    int T, H, W, iters;
    double r, a;          // readout / H, anchor * (H - 1)
};

struct RsRectifyArgs {
    RsRule g;
    papof_tensor fr;     // (frame, row, column, channel)
    papof_tensor mat;    // float32 / float64 (frame, row, column): 2 x 3 (HAS_MATRICES)
    papof_tensor out;    // (frame, row, column, channel)
    papof_tensor valid;  // uint8 (frame, row, column); data NULL: none
    int C;
};

struct RsFlowArgs {
    RsRule g;
    papof_tensor out_fw, out_bw;  // float32 / float64 (pair, row, column, {vx, vy})
};

__device__ __forceinline__ bool rs_inside(const RsRule& g, double X, double Y) {  // (false for a NaN)
    return X >= 0 && X <= (double)(g.W - 1) && Y >= 0 && Y <= (double)(g.H - 1);
}

// L_t(P) at P = (X, Y), a point of the image: true where alive
__device__ __forceinline__ bool rs_displacement(const RsRule& g, long long t, double X, double Y, double& Lx, double& Ly) {
    const double s = (g.a - Y) * g.r;
    Lx = 0.0;
    Ly = 0.0;
    if (s == 0) return true;
    const Bilinear k = taps_at(X, Y, g.H, g.W);
    double Fu = 0.0, Fv = 0.0, Bu = 0.0, Bv = 0.0;
    if (t < g.T - 1) sample_flow(g.fw, t * g.fw.stride[0], k, Fu, Fv);
    if (t > 0) sample_flow(g.bw, (t - 1) * g.bw.stride[0], k, Bu, Bv);
    const double tf = 1.0 + g.r * Fv, tb = g.r * Bv - 1.0;
    if (t == 0) {
        if (!(tf >= 0.5)) return false;
        const double cF = s / tf;
        Lx = cF * Fu;
        Ly = cF * Fv;
    } else if (t == g.T - 1) {
        if (!(tb <= -0.5)) return false;
        const double cB = s / tb;
        Lx = cB * Bu;
        Ly = cB * Bv;
    } else {
        if (!(tf >= 0.5 && tb <= -0.5)) return false;
        const double cF = (s * (s - tb)) / (tf * (tf - tb)), cB = (s * (s - tf)) / (tb * (tb - tf));
        Lx = cF * Fu + cB * Bu;
        Ly = cF * Fv + cB * Bv;
    }
    return true;
}

// the P with P + L_t(P) = Q after g.iters iterations from P_0 = Q: true where alive
__device__ __forceinline__ bool rs_solve(const RsRule& g, long long t, double Qx, double Qy, double& Px, double& Py) {
    Px = Qx;
    Py = Qy;
    if (!rs_inside(g, Qx, Qy)) return false;
    for (int k = 0; k < g.iters; k++) {
        double Lx, Ly;
        if (!rs_displacement(g, t, Px, Py, Lx, Ly)) return false;
        Px = Qx - Lx;
        Py = Qy - Ly;
        if (!rs_inside(g, Px, Py)) return false;
    }
    return true;
}

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y
template <int FD, bool HAS_MATRICES>
__global__ __launch_bounds__(kRsTX* kRsTY) void k_rs_rectify(const RsRectifyArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kRsTX>(lut);
    const int H = a.g.H, W = a.g.W;
    const long long t = frame0 + blockIdx.y;
    PAPOF_TILE_PIXEL(RsTile, tile0, W, int, x, long long, r);
    if (x >= W || r >= H) return;
    double Qx = (double)x, Qy = (double)r;
    if (HAS_MATRICES) {
        const long long mb = t * a.mat.stride[0];
        double m[6];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) m[3 * i + j] = load_flow(a.mat, mb + i * a.mat.stride[1] + j * a.mat.stride[2]);
        const double xd = Qx, rd = Qy;
        Qx = (m[0] * xd + m[1] * rd) + m[2];
        Qy = (m[3] * xd + m[4] * rd) + m[5];
    }
    double Px, Py;
    const bool alive = rs_solve(a.g, t, Qx, Qy, Px, Py);
    if (a.valid.data)
        store_u8(a.valid, PAPOF_AT(a.valid, t, r, x), alive);
    const long long outp = PAPOF_AT(a.out, t, r, x);
    if (!alive) {
        for (int ch = 0; ch < a.C; ch++) store(a.out, outp + ch * a.out.stride[3], 0.0);
        return;
    }
    const Bilinear k = taps_at(Px, Py, H, W);
    const long long base = t * a.fr.stride[0];
    for (int ch = 0; ch < a.C; ch++) store(a.out, outp + ch * a.out.stride[3], sample_frame<FD>(a.fr, base + ch * a.fr.stride[3], k, lut));
}

// blockIdx.x: the tile, as k_rs_rectify's; blockIdx.y: slot `slot0` + y, slot 2 i the forward and 2 i + 1 the backward flow
// of pair i
__global__ __launch_bounds__(kRsTX* kRsTY) void k_rs_flow(const RsFlowArgs a, long long tile0, long long slot0) {
    const int H = a.g.H, W = a.g.W;
    const long long slot = slot0 + blockIdx.y, i = slot >> 1;
    const bool back = slot & 1;
    PAPOF_TILE_PIXEL(RsTile, tile0, W, int, x, long long, r);
    if (x >= W || r >= H) return;
    const long long t = back ? i + 1 : i, t2 = back ? i : i + 1;  // the pixel's frame, and the frame its flow lands in
    const papof_tensor& f = back ? a.g.bw : a.g.fw;
    const papof_tensor& o = back ? a.out_bw : a.out_fw;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);  // dead: this NaN, bit for bit
    const double xd = (double)x, rd = (double)r;
    double u = qnan, v = qnan, Px, Py;
    if (rs_solve(a.g, t, xd, rd, Px, Py)) {
        double Fu, Fv, Lx, Ly;
        sample_flow(f, i * f.stride[0], taps_at(Px, Py, H, W), Fu, Fv);
        const double X2 = Px + Fu, Y2 = Py + Fv;
        if (rs_inside(a.g, X2, Y2) && rs_displacement(a.g, t2, X2, Y2, Lx, Ly)) {
            u = ((Px - xd) + Fu) + Lx;
            v = ((Py - rd) + Fv) + Ly;
            u = u != u ? qnan : u;
            v = v != v ? qnan : v;
        }
    }
    const long long op = PAPOF_AT(o, i, r, x);
    store(o, op, u);
    store(o, op + o.stride[3], v);
}

template <bool HAS_MATRICES>
int launch_rectify(hipStream_t st, const RsRectifyArgs& a) {
    const int fd = a.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_rs_rectify<fd(), HAS_MATRICES>; });
    return launch_grid<RsTile>(a.g.H, a.g.W, a.g.T, st, 0, kernel, a);
}

int launch_rs_flow(hipStream_t st, const RsFlowArgs& a) {
    return launch_grid<RsTile>(a.g.H, a.g.W, 2LL * (a.g.T - 1), st, 0, k_rs_flow, a);
}

// the arguments both calls share: false where the header refuses them
bool rs_rule(RsRule& g, int n_frames, int height, int width, const papof_tensor* flow_fw, const papof_tensor* flow_bw,
             double readout, double anchor, int iters) {
    if (n_frames < 2 || height < 1 || width < 1 || iters < 1 || iters > kRsMaxIters) return false;
    if (!std::isfinite(readout) || std::fabs(readout) > 1.0 || !(anchor >= 0.0 && anchor <= 1.0)) return false;
    if (!in_flow_pair(flow_fw, flow_bw)) return false;
    g.fw = *flow_fw;
    g.bw = *flow_bw;
    g.T = n_frames;
    g.H = height;
    g.W = width;
    g.iters = iters;
    g.r = readout / (double)height;
    g.a = anchor * (double)(height - 1);
    return true;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_rs_rectify_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                       const papof_tensor* flow_fw, const papof_tensor* flow_bw, double readout, double anchor,
                                       int iters, const papof_tensor* matrices, const papof_tensor* out,
                                       const papof_tensor* valid, void* stream) {
    RsRectifyArgs a{};
    if (!h || c < 1 || c > kRsMaxC || !rs_rule(a.g, n_frames, height, width, flow_fw, flow_bw, readout, anchor, iters))
        return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (!opt_in_plane(matrices)) return PAPOF_EINVAL;
    if (!opt_out_mask(valid)) return PAPOF_EINVAL;
    a.fr = *frames;
    if (matrices) a.mat = *matrices;
    a.out = *out;
    if (valid) a.valid = *valid;
    a.C = c;
    PAPOF_HIP(hipSetDevice(h->device));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return matrices ? launch_rectify<true>(st, a) : launch_rectify<false>(st, a);
}

extern "C" int papof_rs_flow_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* flow_fw,
                                    const papof_tensor* flow_bw, double readout, double anchor, int iters,
                                    const papof_tensor* out_fw, const papof_tensor* out_bw, void* stream) {
    RsFlowArgs a{};
    if (!h || !rs_rule(a.g, n_frames, height, width, flow_fw, flow_bw, readout, anchor, iters)) return PAPOF_EINVAL;
    if (!out_flow(out_fw) || !out_flow(out_bw)) return PAPOF_EINVAL;
    a.out_fw = *out_fw;
    a.out_bw = *out_bw;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_rs_flow(static_cast<hipStream_t>(stream), a);
}
