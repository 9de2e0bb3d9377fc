// papteam_opticalflow_amd/csrc/blur.hip -- synthetic motion blur along the flows (papof_motion_blur_tensor).
//
// Why.  A frame exposed over a shutter interval is the average of the scene over that interval, and interp_points /
// interp_weights / interp_blend (sampler.h) already state the scene at an in-between time: a longer shutter for a video is
// the weighted mean, over K times inside the shutter, of what papof_interp_tensor returns.  Written with that call it is two
// calls per video, K full float64 frames written and read again (1.6 GB for a 1080p RGB frame at K = 16) and a chain of
// launches for the weighted sum.  Here one lane makes one output pixel: the flows of the two pairs around the frame are read
// once, the sums stay in registers, and one frame is written.
//
// Semantics: include/papof.h, papof_motion_blur_tensor.  Every sample is papof_interp_tensor's value (the three steps of
// sampler.h, the same bits); fp64 without contraction (-ffp-contract=off), samples accumulated in the table's order.
//
// Mapping.  A block is a 64 x 4 tile of output pixels (k_interp's), over grid.h's grid of tiles and frames.  The sample
// table (offsets and weights, at most kMaxSamples) travels in the kernel arguments: it is the same for every lane, so it
// sits in scalar registers, and the call needs no device buffer and nothing the caller has to keep alive.  A sample with
// offset < 0 lies in the pair (f - 1, f), one with offset > 0 in (f, f + 1).  The geometry of a sample (taps, weights,
// denominator) is computed once and shared by the channels (blur_sample).
//
// Two loop forms.  The sums are rounded sample by sample in the table's order.  A table whose negative offsets come first,
// then its zeros, then its positive ones -- every table of tensors.blur_schedule -- is walked by SORTED = true: one loop per
// side and the frame's own samples between them; an end frame skips the loop of the side it lacks.  Any other order is
// walked by ONE loop that chooses the side per sample (SORTED = false).  Both run the same blur_sample in the same order.
// The split is worth its second instantiation: the side and the skips are wave-uniform, but as branches INSIDE the one
// loop they made the register allocator keep the held taps in two register sets and copy all of them at every iteration
// (60 v_mov_b64 per sample, 204 VGPRs, 2 waves per SIMD, for uint8 C = 3); with loops whose bodies have no uniform branch
// the taps are updated in place (152 VGPRs, 3 waves).
//
// Tap reuse.  Consecutive samples of a pixel usually land in the same bilinear cell (a 2-pixel path holds 16 samples in at
// most 3 cells), and k_interp is paced by the lane's gathers, not by HBM (profiles/interp_probe.txt).  The four taps of each
// of the two frames (per channel, as float64) and the mask's four bytes (as 4 bits) stay in registers, tagged with the pair
// and the cell; a sample gathers only when its tag differs.  The taps are the same values either way: the bits do not
// change (PAPOF_BLUR_REUSE=0 gathers for every sample: the A/B knob of tools/blur_probe.py).
//
// Channels.  NC channels are carried through the sample loop at once: NC = 3 for C = 3 (24 taps in 48 registers), NC = 1
// otherwise -- C = 1 directly, any other C channel-outermost, one pass of the whole sample loop per channel.  Each channel's
// arithmetic is the same sequence in either form.
#include "sampler.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace papof {

namespace {

constexpr int kMaxSamples = 64;

struct BlurArgs {
    papof_tensor fr;      // the video (frame, row, column, channel)
    papof_tensor fw, bw;  // flows (pair, row, column, {vx, vy})
    papof_tensor occ;     // uint8 mask (pair, row, column, {O0, O1}); data NULL: none
    papof_tensor out;     // (frame, row, column, channel)
    int H, W, C, T;
    int n;                // samples of the table: those of weight > 0, in the caller's order
    int n_neg, n_mid;     // of a sorted table: its leading samples of offset < 0 and those of offset 0 behind them
    int reuse;
    double tau[kMaxSamples], w[kMaxSamples];
};

// The four taps of one frame at one bilinear cell, for NC channels, and the mask's taps there as bits (m, n) -> 2 m + n.
template <int NC>
struct TapCache {
    long long pair;  // -1: empty
    int cx, cy;      // the cell: column and row of tap (0, 0)
    unsigned mask;
    double v[NC][4];
};

// The taps k of the frame at `base` (its first channel of the NC) and of the mask channel at `baseo`, unless c holds them.
template <int FD, int NC>
__device__ __forceinline__ void fetch_taps(TapCache<NC>& c, int reuse, long long pair, const Bilinear& k,
                                           const papof_tensor& fr, long long base, const papof_tensor& occ, long long baseo,
                                           const double* lut) {
    if (reuse && c.pair == pair && c.cx == k.col[0] && c.cy == k.row[0]) return;
    c.pair = pair;
    c.cx = k.col[0];
    c.cy = k.row[0];
#pragma unroll
    for (int ch = 0; ch < NC; ch++)
#pragma unroll
        for (int i = 0; i < 4; i++)
            c.v[ch][i] = load_frame<FD>(fr, base + ch * fr.stride[3] + k.row[i] * fr.stride[1] + k.col[i] * fr.stride[2], lut);
    c.mask = 0;
    if (occ.data) {
        const unsigned char* m = static_cast<const unsigned char*>(occ.data);
#pragma unroll
        for (int i = 0; i < 4; i++) c.mask |= (m[baseo + k.row[i] * occ.stride[1] + k.col[i] * occ.stride[2]] ? 1u : 0u) << i;
    }
}

// sample_frame's and sample_mask's sums over held taps: from 0 in (m, n) order
__device__ __forceinline__ double weigh(const double* v, const Bilinear& k) {
    double g = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) g += v[i] * k.w[i];
    return g;
}

__device__ __forceinline__ double weigh_mask(unsigned bits, const Bilinear& k) {
    double o = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) o += ((bits >> i) & 1u ? 1.0 : 0.0) * k.w[i];
    return o;
}

// One sample of the pixel (x, r) for the NC channels from `chan`: papof_interp_tensor's value for the pair `pair` at time
// t, with the pair's flows fl = (u, v, bu, bv) at the pixel, added to the sums with the weight w.  side: 1 if this frame is
// the pair's I0 (a sample after the frame), 0 if it is its I1; centre: this frame at the pixel.
template <int FD, int NC>
__device__ __forceinline__ void blur_sample(const BlurArgs& a, const double* lut, int x, long long r, long long pix,
                                            long long chan, long long pair, int side, const double* fl, double t, double w,
                                            const double* centre, TapCache<NC>& c0, TapCache<NC>& c1, double* acc,
                                            double& wsum) {
    const InterpPoints p = interp_points(x, r, fl[0], fl[1], fl[2], fl[3], t, a.H, a.W);
    const long long base0 = pair * a.fr.stride[0] + chan, base1 = base0 + a.fr.stride[0];
    const long long baseo = pair * a.occ.stride[0];
    if (p.in0) fetch_taps<FD, NC>(c0, a.reuse, pair, p.k0, a.fr, base0, a.occ, baseo, lut);
    if (p.in1) fetch_taps<FD, NC>(c1, a.reuse, pair, p.k1, a.fr, base1, a.occ, baseo + a.occ.stride[3], lut);
    double o0 = 0.0, o1 = 0.0;
    if (a.occ.data && p.in0 && p.in1) {
        o0 = weigh_mask(c0.mask, p.k0);
        o1 = weigh_mask(c1.mask, p.k1);
    }
    const InterpWeights q = interp_weights(p, o0, o1);
#pragma unroll
    for (int ch = 0; ch < NC; ch++) {
        double val;
        if (p.in0 || p.in1) {
            const double g0 = p.in0 ? weigh(c0.v[ch], p.k0) : 0.0;
            const double g1 = p.in1 ? weigh(c1.v[ch], p.k1) : 0.0;
            val = interp_blend(p, q, g0, g1);
        } else {  // the two frames at the pixel itself: one of them is this frame
            const double other = load_frame<FD>(a.fr, (side ? base1 : base0) + pix + ch * a.fr.stride[3], lut);
            val = side ? p.s * centre[ch] + p.t * other : p.s * other + p.t * centre[ch];
        }
        acc[ch] = acc[ch] + w * val;
    }
    wsum = wsum + w;
}

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y.
template <int FD, int NC, bool SORTED>
__global__ __launch_bounds__(kInterpTX* kInterpTY) void k_motion_blur(const BlurArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kInterpTX>(lut);
    PAPOF_TILE_PIXEL(InterpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const long long f = frame0 + blockIdx.y;
    const bool has[2] = {f > 0, f < a.T - 1};  // the pairs (f - 1, f) and (f, f + 1)
    double fl[2][4] = {};                      // their flows at the pixel: u, v, bu, bv
#pragma unroll
    for (int side = 0; side < 2; side++)
        if (has[side]) {
            const long long of = PAPOF_AT(a.fw, f - 1 + side, r, x);
            const long long ob = PAPOF_AT(a.bw, f - 1 + side, r, x);
            fl[side][0] = load_flow(a.fw, of);
            fl[side][1] = load_flow(a.fw, of + a.fw.stride[3]);
            fl[side][2] = load_flow(a.bw, ob);
            fl[side][3] = load_flow(a.bw, ob + a.bw.stride[3]);
        }
    const long long pix = r * a.fr.stride[1] + x * a.fr.stride[2];  // the pixel within a frame
    const long long outp = PAPOF_AT(a.out, f, r, x);
    for (int ch0 = 0; ch0 < a.C; ch0 += NC) {
        const long long chan = ch0 * a.fr.stride[3];
        double centre[NC], acc[NC];
#pragma unroll
        for (int ch = 0; ch < NC; ch++) {
            centre[ch] = load_frame<FD>(a.fr, f * a.fr.stride[0] + pix + chan + ch * a.fr.stride[3], lut);
            acc[ch] = 0.0;
        }
        double wsum = 0.0;
        TapCache<NC> c0, c1;  // of I0 and I1 of the sample's pair
        c0.pair = c1.pair = -1;
        if (SORTED) {  // a.n_neg samples before the frame, a.n_mid at it, the rest after it
            if (has[0])
                for (int k = 0; k < a.n_neg; k++)
                    blur_sample<FD, NC>(a, lut, x, r, pix, chan, f - 1, 0, fl[0], 1.0 + a.tau[k], a.w[k], centre, c0, c1, acc, wsum);
            for (int k = a.n_neg; k < a.n_neg + a.n_mid; k++) {
#pragma unroll
                for (int ch = 0; ch < NC; ch++) acc[ch] = acc[ch] + a.w[k] * centre[ch];
                wsum = wsum + a.w[k];
            }
            if (has[1])
                for (int k = a.n_neg + a.n_mid; k < a.n; k++)
                    blur_sample<FD, NC>(a, lut, x, r, pix, chan, f, 1, fl[1], a.tau[k], a.w[k], centre, c0, c1, acc, wsum);
        } else {
            for (int k = 0; k < a.n; k++) {
                const double tau = a.tau[k], w = a.w[k];
                const int side = tau > 0.0 ? 1 : 0;  // (wave-uniform, as everything that decides the path of a sample)
                if (tau == 0.0) {
#pragma unroll
                    for (int ch = 0; ch < NC; ch++) acc[ch] = acc[ch] + w * centre[ch];
                    wsum = wsum + w;
                } else if (has[side]) {
                    blur_sample<FD, NC>(a, lut, x, r, pix, chan, f - 1 + side, side, side ? fl[1] : fl[0],
                                        side ? tau : 1.0 + tau, w, centre, c0, c1, acc, wsum);
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < NC; ch++)
            store(a.out, outp + (ch0 + ch) * a.out.stride[3], wsum > 0 ? acc[ch] / wsum : centre[ch]);
    }
}

template <int FD>
int launch_blur_of(hipStream_t st, BlurArgs a) {
    int k = 0;  // the table is sorted if, behind its negative offsets and its zeros, only positive ones are left
    for (a.n_neg = 0; k < a.n && a.tau[k] < 0.0; k++) a.n_neg++;
    for (a.n_mid = 0; k < a.n && a.tau[k] == 0.0; k++) a.n_mid++;
    for (; k < a.n && a.tau[k] > 0.0;) k++;
    const bool sorted = k == a.n;
    const auto kernel = a.C == 3 ? (sorted ? k_motion_blur<FD, 3, true> : k_motion_blur<FD, 3, false>)
                                 : (sorted ? k_motion_blur<FD, 1, true> : k_motion_blur<FD, 1, false>);
    return launch_grid<InterpTile>(a.H, a.W, a.T, st, 0, kernel, a);
}

int launch_blur(hipStream_t st, const BlurArgs& a) {
    return a.fr.dtype == PAPOF_DTYPE_U8    ? launch_blur_of<PAPOF_DTYPE_U8>(st, a)
           : a.fr.dtype == PAPOF_DTYPE_F32 ? launch_blur_of<PAPOF_DTYPE_F32>(st, a)
                                           : launch_blur_of<PAPOF_DTYPE_F64>(st, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_motion_blur_tensor(papof_handle* h, int n_frames, const papof_tensor* frames, int height, int width,
                                        int c, const papof_tensor* flow_fw, const papof_tensor* flow_bw,
                                        const papof_tensor* occlusion, int n_samples, const double* offsets,
                                        const double* weights, const papof_tensor* out, void* stream) {
    if (!h || n_frames < 2 || height < 1 || width < 1 || c < 1) return PAPOF_EINVAL;
    const auto all = {0, 1, 2, 3};
    if (!in_frames(frames) || !in_flow_pair(flow_fw, flow_bw))
        return PAPOF_EINVAL;
    if (occlusion && !described(occlusion, {PAPOF_DTYPE_U8}, all, false)) return PAPOF_EINVAL;
    if (!out_frames(out)) return PAPOF_EINVAL;
    if (n_samples < 1 || n_samples > kMaxSamples || !offsets || !weights) return PAPOF_EINVAL;
    const double lo = std::ldexp(1.0, -20), hi = 1.0 - lo;
    BlurArgs a{};
    double sum = 0.0;
    for (int k = 0; k < n_samples; k++) {
        const double tau = offsets[k], w = weights[k];
        if (!(tau == 0.0 || (std::fabs(tau) >= lo && std::fabs(tau) <= hi))) return PAPOF_EINVAL;  // (a NaN fails both)
        if (!std::isfinite(w) || w < 0.0) return PAPOF_EINVAL;
        sum += w;
        if (w > 0.0) {
            a.tau[a.n] = tau;
            a.w[a.n++] = w;
        }
    }
    if (!(sum > 0.0)) return PAPOF_EINVAL;
    a.fr = *frames;
    a.fw = *flow_fw;
    a.bw = *flow_bw;
    if (occlusion) a.occ = *occlusion;
    a.out = *out;
    a.H = height;
    a.W = width;
    a.C = c;
    a.T = n_frames;
    const char* e = std::getenv("PAPOF_BLUR_REUSE");  // A/B knob: gather every sample's taps anew (the bits do not change)
    a.reuse = !(e && std::atoi(e) == 0);
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_blur(static_cast<hipStream_t>(stream), a);
}
