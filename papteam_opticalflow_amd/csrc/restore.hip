// papteam_opticalflow_amd/csrc/restore.hip -- dirt and dropout removal: the detector of one-frame defects along the flows
// (papof_defect_detect_tensor) and the dilation of its masks (papof_mask_dilate_tensor).
//
// Why.  Film dirt and sparkle, analogue dropouts, transmission errors, a bird that crosses one frame: defects that live in a
// single frame.  k_temporal_filter keeps them by construction (the centre IS the defect, so every neighbour looks unlike it
// and is down-weighted), and the completion kernels of inpaint.hip remove them only under masks that somebody paints.  The
// detector makes the masks: Kokaram's spike detection index in its range form (A. Kokaram, "Motion Picture Restoration",
// Springer 1998, ch. 6; the ROD detector of Nadenau and Mitra 1997 with two references) -- a pixel is a defect when, in some
// channel, it lies outside the range of the two points it maps to in two other frames by more than a threshold.  The repair
// needs no kernel of its own: tensors.repair_defects hands the dilated masks to complete_flows, propagate and fill_holes.
//
// What it is not.  A defect that persists over frames (a line scratch, a dead sensor pixel under a static camera) agrees with
// its references and is not found.  A small object that outruns the flow (a ball, rain) disagrees with them and is found.
// A defect below the threshold stays.  The end frames take both references from one side and are weaker there.
//
// Semantics: include/papof.h, papof_defect_detect_tensor and papof_mask_dilate_tensor.  A hop is sampler.h's, exactly
// k_temporal_filter's; the samplers are sampler.h's (sample_flow, sample_frame), fp64 without contraction
// (-ffp-contract=off): the result is bitwise reproducible.
//
// Mapping, k_defect_detect.  k_temporal_filter's: a block is a 64 x 4 tile of pixels, blockIdx.x the tile, blockIdx.y the
// frame; one lane makes one pixel's mask, score and support with its C centre values and the two landing points in
// registers, and samples the references only where both are alive.  No atomics, no workspace, every offset 64-bit.
//
// Mapping, k_mask_dilate.  A block is a tile of 64 columns x 16 rows, four waves.  A row of 64 mask bytes is one 64-bit word
// (__ballot: bit i is column x0 + i); with the words of the 64 columns to its left and right -- of which only the nearest
// `radius` lanes load -- the horizontal pass is shifts and ORs on three wave-uniform words, one word per input row into
// LDS; the vertical pass ORs the 2 radius + 1 words around an output row (LDS broadcasts) and every lane stores its bit.
// Rows and columns beyond the image are zeros, which is the rule's clipping of the window.
#include "sampler.h"

#include <cmath>

namespace papof {

namespace {

constexpr int kDetectTX = 64, kDetectTY = 4;  // a 64 x 4 tile of pixels per block (256 lanes: lut)
using DetectTile = Tile<kDetectTX, kDetectTY>;

struct DetectArgs {
    papof_tensor fr;      // frames (frame, row, column, channel)
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy}); pair t runs from frame t to t + 1
    papof_tensor mask;    // uint8 (frame, row, column)
    papof_tensor score;   // float32 / float64 (frame, row, column); data NULL: none
    papof_tensor sup;     // uint8 (frame, row, column); data NULL: none
    int T, H, W, C;
    int check;            // the consistency test is applied
    double thr, a1, a2;
};

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y.
template <int FD>
__global__ __launch_bounds__(kDetectTX* kDetectTY) void k_defect_detect(const DetectArgs a, long long tile0,
                                                                        long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kDetectTX>(lut);
    PAPOF_TILE_PIXEL(DetectTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    // the references t + o1 and t + o2: (-1, +1) inside the video, (+1, +2) at frame 0, (-1, -2) at frame T - 1
    const int o1 = t == 0 ? 1 : -1, o2 = t == 0 ? 2 : (t == a.T - 1 ? -2 : 1);
    double X1, Y1, X2, Y2;
    const bool alive1 = hop_from(a, t, o1, (double)x, (double)r, X1, Y1);  // (sampler.h, the direction rule)
    bool alive2;
    if (o1 * o2 < 0)  // two chains of one hop
        alive2 = hop_from(a, t, o2, (double)x, (double)r, X2, Y2);
    else              // one chain of two hops: dead after the first, it stays dead
        alive2 = alive1 && hop_from(a, t + o1, o1, X1, Y1, X2, Y2);
    const int support = (alive1 ? 1 : 0) + (alive2 ? 1 : 0);
    double s = 0.0;
    if (support == 2) {
        const Bilinear k1 = taps_at(X1, Y1, a.H, a.W), k2 = taps_at(X2, Y2, a.H, a.W);
        const long long pix = PAPOF_AT(a.fr, t, r, x);
        const long long base1 = (t + o1) * a.fr.stride[0], base2 = (t + o2) * a.fr.stride[0];
#pragma unroll
        for (int ch = 0; ch < kMaxChannels; ch++)
            if (ch < a.C) {
                const double c = load_frame<FD>(a.fr, pix + ch * a.fr.stride[3], lut);
                const double g1 = sample_frame<FD>(a.fr, base1 + ch * a.fr.stride[3], k1, lut);
                const double g2 = sample_frame<FD>(a.fr, base2 + ch * a.fr.stride[3], k2, lut);
                const double lo = g2 < g1 ? g2 : g1, hi = g2 > g1 ? g2 : g1;
                const double above = c - hi, below = lo - c;
                const double d = below > above ? below : above;
                s = d > s ? d : s;  // (false for a NaN)
            }
    }
    store_u8(a.mask, PAPOF_AT(a.mask, t, r, x), support == 2 && s > a.thr ? 1 : 0);
    if (a.score.data) store_plane(a.score, PAPOF_AT(a.score, t, r, x), s);
    if (a.sup.data) store_u8(a.sup, PAPOF_AT(a.sup, t, r, x), (unsigned char)support);
}

int launch_detect(hipStream_t st, const DetectArgs& a) {
    const auto kernel = by_dtype(a.fr.dtype, [](auto fd) { return k_defect_detect<fd()>; });
    return launch_grid<DetectTile>(a.H, a.W, a.T, st, 0, kernel, a);
}

constexpr int kDilateTX = 64, kDilateWaves = 4;  // a wave is the 64 columns of one row: one word
constexpr int kDilateTY = 16;                    // output rows per block
using DilateTile = Tile<kDilateTX, kDilateTY, kDilateTX, kDilateWaves>;
constexpr int kMaxDilate = 32;                   // radius: the left and right words reach 64 columns

struct DilateArgs {
    papof_tensor in, out;  // uint8 (frame, row, column)
    int T, H, W, R;
};

// grid.h's grid over the frame's 64 x 16 tiles; blockIdx.y: frame `frame0` + y.  No lane
// leaves before the last __ballot and the barrier: a lane beyond the image votes 0 and stores nothing.
__global__ __launch_bounds__(kDilateTX* kDilateWaves) void k_mask_dilate(const DilateArgs a, long long tile0,
                                                                         long long frame0) {
    __shared__ unsigned long long hrow[kDilateTY + 2 * kMaxDilate];  // input rows r0 - R .. r0 + 15 + R, dilated along x
    PAPOF_TILE_ORIGIN(DilateTile, tile0, a.W, int, x0, long long, r0);
    const long long t = frame0 + blockIdx.y;
    const int lane = (int)threadIdx.x, wave = (int)threadIdx.y, R = a.R;
    const unsigned char* m = static_cast<const unsigned char*>(a.in.data) + t * a.in.stride[0];
    const long long sx = a.in.stride[2];
    const int xm = x0 + lane, xl = xm - kDilateTX, xr = xm + kDilateTX;
    for (int i = wave; i < kDilateTY + 2 * R; i += kDilateWaves) {
        const long long r = r0 - R + i;
        const bool row = r >= 0 && r < a.H;
        const unsigned char* mr = m + (row ? r : 0) * a.in.stride[1];
        // (&& reads only where what stands before it holds: no load beyond the image)
        const unsigned long long M = __ballot(row && xm < a.W && mr[xm * sx] != 0);
        const unsigned long long L = __ballot(row && lane >= kDilateTX - R && xl >= 0 && mr[xl * sx] != 0);
        const unsigned long long Rt = __ballot(row && lane < R && xr < a.W && mr[xr * sx] != 0);
        unsigned long long h = M;
        for (int k = 1; k <= R; k++) h |= (M >> k) | (M << k) | (Rt << (kDilateTX - k)) | (L >> (kDilateTX - k));
        if (lane == 0) hrow[i] = h;
    }
    __syncthreads();
    unsigned char* out = static_cast<unsigned char*>(a.out.data) + t * a.out.stride[0];
    for (int j = wave; j < kDilateTY; j += kDilateWaves) {
        const long long r = r0 + j;
        if (r >= a.H) break;
        unsigned long long v = 0;
        for (int i = j; i <= j + 2 * R; i++) v |= hrow[i];  // rows r - R .. r + R
        if (xm < a.W) out[r * a.out.stride[1] + xm * a.out.stride[2]] = (unsigned char)((v >> lane) & 1ull);
    }
}

int launch_dilate(hipStream_t st, const DilateArgs& a) {
    return launch_grid<DilateTile>(a.H, a.W, a.T, st, 0, k_mask_dilate, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_defect_detect_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                          const papof_tensor* frames, const papof_tensor* flow_fw,
                                          const papof_tensor* flow_bw, double threshold, int use_check, double alpha1,
                                          double alpha2, const papof_tensor* mask, const papof_tensor* score,
                                          const papof_tensor* support, void* stream) {
    if (!h || n_frames < 3 || height < 1 || width < 1 || c < 1 || c > kMaxChannels) return PAPOF_EINVAL;
    if (!std::isfinite(threshold) || threshold < 0) return PAPOF_EINVAL;
    if (!valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    if (!in_frames(frames)) return PAPOF_EINVAL;
    if (!in_flow_pair(flow_fw, flow_bw)) return PAPOF_EINVAL;
    if (!described(mask, {PAPOF_DTYPE_U8}, {0, 1, 2}, true)) return PAPOF_EINVAL;
    if (!opt_out_plane(score)) return PAPOF_EINVAL;
    if (!opt_out_mask(support)) return PAPOF_EINVAL;
    DetectArgs a{};
    a.fr = *frames;
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    a.mask = *mask;
    if (score) a.score = *score;
    if (support) a.sup = *support;
    a.T = n_frames;
    a.H = height;
    a.W = width;
    a.C = c;
    a.check = use_check ? 1 : 0;
    a.thr = threshold;
    a.a1 = alpha1;
    a.a2 = alpha2;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_detect(static_cast<hipStream_t>(stream), a);
}

extern "C" int papof_mask_dilate_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* mask,
                                        int radius, const papof_tensor* out, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || radius < 0 || radius > kMaxDilate) return PAPOF_EINVAL;
    if (!described(mask, {PAPOF_DTYPE_U8}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!described(out, {PAPOF_DTYPE_U8}, {0, 1, 2}, true)) return PAPOF_EINVAL;
    if (mask->data == out->data) return PAPOF_EINVAL;
    DilateArgs a{};
    a.in = *mask;
    a.out = *out;
    a.T = n_frames;
    a.H = height;
    a.W = width;
    a.R = radius;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_dilate(static_cast<hipStream_t>(stream), a);
}
