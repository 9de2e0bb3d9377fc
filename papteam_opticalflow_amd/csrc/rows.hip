// papteam_opticalflow_amd/csrc/rows.hip -- the projective warp whose matrix depends on the SOURCE row a pixel lands in
// (papof_warp_rows_tensor): the device half of rotation-path stabilization of a rolling-shutter camera.
//
// Why.  A hand-held camera rotates, R(tau), and a rolling shutter exposes source row y of frame t at t + readout * (y - a) / H,
// so every source row has its own homography K R(t + tau(y)) S^T K^-1 onto the stabilized camera S (Forssen and Ringaby,
// "Rectifying rolling shutter video from hand-held devices", CVPR 2010; Karpenko et al., "Digital video stabilization and
// rolling shutter correction using gyroscopes", Stanford CSTR 2011-03).  The host samples that family at Kn knot rows; an
// output pixel needs the row it lands in, which depends on the matrix: a fixed-point solve of a few iterations.  Written
// with gathers it is `iters` index_select / lerp / divide passes over full-frame temporaries of nine planes; here one lane
// makes one output pixel with its iterate in registers, 2 x 9 table entries per iteration, then the C-channel frame gather.
//
// Semantics: include/papof.h, papof_warp_rows_tensor.  fp64 without contraction (-ffp-contract=off); IEEE divisions.
//
// Mapping.  k_warp_affine's: a block is a 64 x 4 tile of output pixels, over grid.h's grid of tiles and frames.  The lanes
// of a wave share the output row and, but for the few waves whose iterate straddles a knot, the interval k, so the two
// knots' loads are one address per wave (a broadcast from the cache); the table is read through global addresses, not staged
// (DESIGN.md has the reasons).  Bounds: s = Yc * g is formed from a clamped Yc in [0, H - 1] that is never a NaN, so the
// conversion to int sees 0 <= s <= about Kn - 1 <= PAPOF_ROWS_MAX_KNOTS, and k is clamped to Kn - 2 before an address is
// formed.  No atomics, no workspace: every output element belongs to one lane.  Every offset is 64-bit.
#include "sampler.h"

#include <cmath>

namespace papof {

namespace {

constexpr int kRowsTX = 64, kRowsTY = 4;  // a 64 x 4 tile of output pixels per block (256 lanes: lut)
using RowsTile = Tile<kRowsTX, kRowsTY>;
constexpr int kRowsMaxIters = 8;

struct RowsArgs {
    papof_tensor fr;     // (frame, row, column, channel)
    papof_tensor tab;    // float32 / float64 (frame, knot, row, column): Kn matrices of 3 x 3 per frame
    papof_tensor out;    // (frame, row, column, channel)
    papof_tensor valid;  // uint8 (frame, row, column); data NULL: none
    int H, W, C;
    int Kn, iters;
    double g;            // (double)(Kn - 1) / (double)(H - 1); unused for Kn == 1
};

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y
template <int FD>
__global__ __launch_bounds__(kRowsTX* kRowsTY) void k_warp_rows(const RowsArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kRowsTX>(lut);
    const long long i = frame0 + blockIdx.y;
    PAPOF_TILE_PIXEL(RowsTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const double xd = (double)x, rd = (double)r, H1 = (double)(a.H - 1);
    const long long mb = i * a.tab.stride[0];
    double X = 0.0, Y = rd, D = 0.0;
    if (a.Kn == 1) {  // one matrix: k_warp_projective
        double m[9];
#pragma unroll
        for (int q = 0; q < 9; q++) m[q] = load_flow(a.tab, mb + (q / 3) * a.tab.stride[2] + (q % 3) * a.tab.stride[3]);
        D = (m[6] * xd + m[7] * rd) + m[8];
        X = ((m[0] * xd + m[1] * rd) + m[2]) / D;
        Y = ((m[3] * xd + m[4] * rd) + m[5]) / D;
    } else {
        for (int j = 0; j < a.iters; j++) {
            double Yc = Y;
            if (!(Y >= 0))  // (a NaN goes here)
                Yc = 0.0;
            else if (Y > H1)
                Yc = H1;
            const double s = Yc * a.g;  // in [0, about Kn - 1]: never a NaN, never beyond an int
            int k = (int)s;
            if (k > a.Kn - 2) k = a.Kn - 2;
            const double f = s - (double)k;
            const long long ka = mb + k * a.tab.stride[1], kb = ka + a.tab.stride[1];
            double m[9];
#pragma unroll
            for (int q = 0; q < 9; q++) {
                const long long o = (q / 3) * a.tab.stride[2] + (q % 3) * a.tab.stride[3];
                const double A = load_flow(a.tab, ka + o), B = load_flow(a.tab, kb + o);
                m[q] = A + f * (B - A);
            }
            D = (m[6] * xd + m[7] * rd) + m[8];
            X = ((m[0] * xd + m[1] * rd) + m[2]) / D;
            Y = ((m[3] * xd + m[4] * rd) + m[5]) / D;
        }
    }
    const bool in = D > 0 && X >= 0 && X <= (double)(a.W - 1) && Y >= 0 && Y <= H1;  // (false for a NaN)
    if (a.valid.data)
        store_u8(a.valid, PAPOF_AT(a.valid, i, r, x), in);
    const long long outp = PAPOF_AT(a.out, i, r, x);
    if (!in) {
        for (int ch = 0; ch < a.C; ch++) store(a.out, outp + ch * a.out.stride[3], 0.0);
        return;
    }
    const Bilinear k = taps_at(X, Y, a.H, a.W);
    const long long base = i * a.fr.stride[0];
    for (int ch = 0; ch < a.C; ch++) store(a.out, outp + ch * a.out.stride[3], sample_frame<FD>(a.fr, base + ch * a.fr.stride[3], k, lut));
}

int launch_warp_rows(hipStream_t st, const RowsArgs& a, int n_frames) {
    const int fd = a.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_warp_rows<fd()>; });
    return launch_grid<RowsTile>(a.H, a.W, n_frames, st, 0, kernel, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_warp_rows_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                      const papof_tensor* matrices, int n_knots, int iters, const papof_tensor* out,
                                      const papof_tensor* valid, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1) return PAPOF_EINVAL;
    if (n_knots < 1 || n_knots > PAPOF_ROWS_MAX_KNOTS) return PAPOF_EINVAL;
    if (n_knots > 1 && (height < 2 || iters < 1 || iters > kRowsMaxIters)) return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (!in_flow(matrices)) return PAPOF_EINVAL;
    if (!opt_out_mask(valid)) return PAPOF_EINVAL;
    RowsArgs a{};
    a.fr = *frames;
    a.tab = *matrices;
    a.out = *out;
    if (valid) a.valid = *valid;
    a.H = height;
    a.W = width;
    a.C = c;
    a.Kn = n_knots;
    a.iters = iters;
    a.g = n_knots > 1 ? (double)(n_knots - 1) / (double)(height - 1) : 0.0;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_warp_rows(static_cast<hipStream_t>(stream), a, n_frames);
}
