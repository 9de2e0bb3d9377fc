// papteam_opticalflow_amd/csrc/mosaic.hip -- video mosaics (papof_mosaic_tensor): many frames, each through its own affine
// matrix, gathered into one output pixel and combined there -- the first that covers it, their mean, or their median.
//
// Why.  A panorama, a clean plate (the temporal median of the registered frames) and the borders of a stabilized video are
// all the same gather; built from warp_affine they are one full-canvas fp64 temporary per source, then a sort over the
// stack.  Here the samples of a pixel never leave the CU.
//
// Semantics: include/papof.h, papof_mosaic_tensor.  fp64 without contraction (-ffp-contract=off); the bilinear rule is
// sampler.h's, unchanged.
//
// k_mosaic.  A block is a 64 x TY tile of output pixels of one output (blockIdx.x the tile, blockIdx.y the output), a lane
// one pixel.
//   1. Culling: lane k of the block maps the tile's four corners through matrix (o, k).  Every step of
//      X = (m00 x + m01 r) + m02 is monotone in x and in r under rounding, so over the tile X and Y take their extremes at
//      the corners: a source whose corner box (widened by a pixel) misses the frame is live at no pixel of the tile, and
//      dropping it changes no byte.  Sources < 0 and matrices with an entry that is not finite (X or Y is then +-inf or NaN
//      at every pixel) go the same way.  The survivors are compacted into an LDS list in k order (ballot + prefix).
//   2. The block walks that list; the index is made uniform (readfirstlane): the source and its matrix are loads at one address.
//   3. FIRST and MEAN keep up to four channels in registers per walk.  MEDIAN walks once per channel: the lane's live
//      samples go to LDS laid out [sample][lane] (a lane reads and writes its own column only: no barrier, no conflict), and
//      the element of rank (n - 1) / 2 under (value, k) is found by counting, for each candidate, the samples before it.
// The instance is chosen by n_src: MEDIAN holds 8, 16, 32 or 64 samples per lane, in tiles of 64 x 4, 64 x 4, 64 x 2 and
// 64 x 1 (16, 32, 32 and 32 KiB of samples per block): DESIGN.md section 25 has the registers and the occupancy of each.
#include "sampler.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace papof {

namespace {

constexpr int kMosTX = 64;     // tile width: one wave per tile row
constexpr int kMaxSrc = 256;   // the list's capacity (n_src <= PAPOF_MOSAIC_MAX_SOURCES = 255)

struct MosaicArgs {
    papof_tensor fr;     // (frame, row, column, channel)
    papof_tensor mask;   // uint8 (frame, row, column); data NULL: none
    papof_tensor mat;    // float32 / float64 (out, k, row, column): 2 x 3
    papof_tensor out;    // (out, row, column, channel)
    papof_tensor count;  // uint8 (out, row, column); data NULL: none
    const int* src;      // (out, k)
    int H, W, C;         // the frames
    int Hc, Wc;          // the outputs
    int n_src;
    int cull;            // 0: every source >= 0 is walked by every tile (measurements)
};

// a sorts before b: a < b, or a is a number and b is NaN
__device__ __forceinline__ bool sorts_before(double a, double b) { return a < b || (a == a && b != b); }

template <int FD, int MODE, int CAP, int TY>
__global__ __launch_bounds__(kMosTX* TY) void k_mosaic(const MosaicArgs a, long long tile0, long long out0) {
    constexpr int NT = kMosTX * TY;
    constexpr int CH = MODE == PAPOF_MOSAIC_MEDIAN ? 1 : 4;  // channels per walk of the list
    __shared__ double lut[256];
    __shared__ unsigned short list[kMaxSrc];
    __shared__ int wcount[TY];
    __shared__ double smp[MODE == PAPOF_MOSAIC_MEDIAN ? CAP * NT : 1];
    const int tid = threadIdx.y * kMosTX + threadIdx.x;
    if (FD == PAPOF_DTYPE_U8)
        for (int j = tid; j < 256; j += NT) fill_u8_lut(lut, j);
    const long long o = out0 + blockIdx.y;
    const long long tx = (a.Wc + kMosTX - 1) / kMosTX, tile = tile0 + blockIdx.x;
    const int x0 = (int)(tile % tx) * kMosTX;
    const long long r0 = (tile / tx) * TY;
    const int* src = a.src + o * a.n_src;
    const long long mo = o * a.mat.stride[0];
    const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);

    // ---- 1. the sources that can reach this tile, in k order
    int total = 0;
    {
        const double xa = (double)x0, xb = (double)std::min(x0 + kMosTX - 1, a.Wc - 1);
        const double ra = (double)r0, rb = (double)std::min(r0 + TY - 1, (long long)a.Hc - 1);
        for (int base = 0; base < a.n_src; base += NT) {
            const int k = base + tid;
            bool keep = k < a.n_src && src[k] >= 0;
            if (keep && a.cull) {
                double m[6];
                const long long mb = mo + k * a.mat.stride[1];
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) m[3 * r + c] = load_flow(a.mat, mb + r * a.mat.stride[2] + c * a.mat.stride[3]);
                bool finite = true;
#pragma unroll
                for (int j = 0; j < 6; j++) finite = finite && isfinite(m[j]);
                const double X0 = (m[0] * xa + m[1] * ra) + m[2], X1 = (m[0] * xb + m[1] * ra) + m[2];
                const double X2 = (m[0] * xa + m[1] * rb) + m[2], X3 = (m[0] * xb + m[1] * rb) + m[2];
                const double Y0 = (m[3] * xa + m[4] * ra) + m[5], Y1 = (m[3] * xb + m[4] * ra) + m[5];
                const double Y2 = (m[3] * xa + m[4] * rb) + m[5], Y3 = (m[3] * xb + m[4] * rb) + m[5];
                // (a NaN corner -- an overflow meeting its opposite -- proves nothing: every comparison is false, the source stays)
                const bool missx = (X0 < -1.0 && X1 < -1.0 && X2 < -1.0 && X3 < -1.0) ||
                                   (X0 > W1 + 1.0 && X1 > W1 + 1.0 && X2 > W1 + 1.0 && X3 > W1 + 1.0);
                const bool missy = (Y0 < -1.0 && Y1 < -1.0 && Y2 < -1.0 && Y3 < -1.0) ||
                                   (Y0 > H1 + 1.0 && Y1 > H1 + 1.0 && Y2 > H1 + 1.0 && Y3 > H1 + 1.0);
                keep = finite && !missx && !missy;
            }
            const unsigned long long vote = __ballot(keep);
            if (threadIdx.x == 0) wcount[threadIdx.y] = __popcll(vote);
            __syncthreads();
            int before = total, all = total;
#pragma unroll
            for (int w = 0; w < TY; w++) {
                before += w < (int)threadIdx.y ? wcount[w] : 0;
                all += wcount[w];
            }
            if (keep) list[before + __popcll(vote & ((1ULL << threadIdx.x) - 1ULL))] = (unsigned short)k;
            total = all;
            __syncthreads();
        }
    }
    const int x = x0 + (int)threadIdx.x;
    const long long r = r0 + threadIdx.y;
    if (x >= a.Wc || r >= a.Hc) return;  // (no barrier below)

    // ---- 2, 3. the walk
    const double xd = (double)x, rd = (double)r;
    const long long outp = o * a.out.stride[0] + r * a.out.stride[1] + x * a.out.stride[2];
    const unsigned char* mk = static_cast<const unsigned char*>(a.mask.data);
    const bool all_sources = a.count.data != nullptr || MODE != PAPOF_MOSAIC_FIRST;
    for (int c0 = 0; c0 < a.C; c0 += CH) {
        double acc[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) acc[j] = 0.0;
        int n = 0;
        for (int i = 0; i < total; i++) {
            const int k = __builtin_amdgcn_readfirstlane((int)list[i]);
            const long long s = src[k];
            const long long mb = mo + k * a.mat.stride[1];
            double m[6];
#pragma unroll
            for (int rr = 0; rr < 2; rr++)
#pragma unroll
                for (int c = 0; c < 3; c++) m[3 * rr + c] = load_flow(a.mat, mb + rr * a.mat.stride[2] + c * a.mat.stride[3]);
            const double X = (m[0] * xd + m[1] * rd) + m[2], Y = (m[3] * xd + m[4] * rd) + m[5];
            if (!(X >= 0 && X <= W1 && Y >= 0 && Y <= H1)) continue;  // (false for a NaN)
            const Bilinear t = taps_at(X, Y, a.H, a.W);
            if (mk) {
                bool masked = false;
                const long long b = s * a.mask.stride[0];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    masked = masked || (t.w[j] > 0 && mk[b + t.row[j] * a.mask.stride[1] + t.col[j] * a.mask.stride[2]] != 0);
                if (masked) continue;
            }
            const long long base = s * a.fr.stride[0] + c0 * a.fr.stride[3];
            if (MODE == PAPOF_MOSAIC_MEDIAN) {
                smp[n * NT + tid] = sample_frame<FD>(a.fr, base, t, lut);
            } else if (MODE == PAPOF_MOSAIC_MEAN || n == 0) {
#pragma unroll
                for (int j = 0; j < CH; j++)
                    if (c0 + j < a.C) {
                        const double g = sample_frame<FD>(a.fr, base + j * a.fr.stride[3], t, lut);
                        acc[j] = MODE == PAPOF_MOSAIC_MEAN ? acc[j] + g : g;
                    }
            }
            n++;
            if (!all_sources) break;
        }
        if (c0 == 0 && a.count.data)
            static_cast<unsigned char*>(a.count.data)[o * a.count.stride[0] + r * a.count.stride[1] + x * a.count.stride[2]] =
                (unsigned char)n;
        if (MODE == PAPOF_MOSAIC_MEDIAN) {
            // the sample with exactly (n - 1) / 2 samples before it under (value, k): the compaction kept the k order
            const int want = (n - 1) / 2;
            double v = 0.0;
            for (int i = 0; i < n; i++) {
                const double vi = smp[i * NT + tid];
                int rank = 0;
                for (int j = 0; j < n; j++) {
                    const double vj = smp[j * NT + tid];
                    rank += sorts_before(vj, vi) || (j < i && !sorts_before(vi, vj));
                }
                if (rank == want) {
                    v = vi;
                    break;
                }
            }
            store(a.out, outp + c0 * a.out.stride[3], v);
        } else {
#pragma unroll
            for (int j = 0; j < CH; j++)
                if (c0 + j < a.C) {
                    double v = acc[j];
                    if (MODE == PAPOF_MOSAIC_MEAN) v = n > 0 ? v / (double)n : 0.0;
                    store(a.out, outp + (c0 + j) * a.out.stride[3], v);
                }
        }
    }
}

template <int MODE, int CAP, int TY>
int launch_mosaic_as(hipStream_t st, const MosaicArgs& a, int n_out) {
    const int fd = a.fr.dtype;
    const auto kernel = fd == PAPOF_DTYPE_U8 ? k_mosaic<PAPOF_DTYPE_U8, MODE, CAP, TY>
                        : fd == PAPOF_DTYPE_F32 ? k_mosaic<PAPOF_DTYPE_F32, MODE, CAP, TY>
                                                : k_mosaic<PAPOF_DTYPE_F64, MODE, CAP, TY>;
    const long long tiles = ((a.Wc + kMosTX - 1) / (long long)kMosTX) * ((a.Hc + TY - 1) / (long long)TY);
    return launch_tiles(tiles, n_out, [&](dim3 grid, long long t0, long long o0) {
        hipLaunchKernelGGL(kernel, grid, dim3(kMosTX, TY), 0, st, a, t0, o0);
    });
}

int launch_mosaic(hipStream_t st, const MosaicArgs& a, int n_out, int mode) {
    if (mode == PAPOF_MOSAIC_FIRST) return launch_mosaic_as<PAPOF_MOSAIC_FIRST, 0, 4>(st, a, n_out);
    if (mode == PAPOF_MOSAIC_MEAN) return launch_mosaic_as<PAPOF_MOSAIC_MEAN, 0, 4>(st, a, n_out);
    if (a.n_src <= 8) return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 8, 4>(st, a, n_out);
    if (a.n_src <= 16) return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 16, 4>(st, a, n_out);
    if (a.n_src <= 32) return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 32, 2>(st, a, n_out);
    return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 64, 1>(st, a, n_out);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_mosaic_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                   const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                   const int* sources, const papof_tensor* matrices, int mode, const papof_tensor* out,
                                   const papof_tensor* count, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1 || n_out < 1 || out_height < 1 || out_width < 1) return PAPOF_EINVAL;
    if (n_src < 1 || n_src > PAPOF_MOSAIC_MAX_SOURCES || !sources) return PAPOF_EINVAL;
    if (mode != PAPOF_MOSAIC_FIRST && mode != PAPOF_MOSAIC_MEAN && mode != PAPOF_MOSAIC_MEDIAN) return PAPOF_EINVAL;
    if (mode == PAPOF_MOSAIC_MEDIAN && n_src > PAPOF_MOSAIC_MAX_MEDIAN) return PAPOF_EINVAL;
    const auto I = {(int)PAPOF_DTYPE_U8, (int)PAPOF_DTYPE_F32, (int)PAPOF_DTYPE_F64};
    if (!described(frames, I, {0, 1, 2, 3}, false) || !described(out, I, {0, 1, 2, 3}, true)) return PAPOF_EINVAL;
    if (masks && !described(masks, {PAPOF_DTYPE_U8}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!described(matrices, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1, 2, 3}, false)) return PAPOF_EINVAL;
    if (count && !described(count, {PAPOF_DTYPE_U8}, {0, 1, 2}, true)) return PAPOF_EINVAL;
    MosaicArgs a{};
    a.fr = *frames;
    if (masks) a.mask = *masks;
    a.mat = *matrices;
    a.out = *out;
    if (count) a.count = *count;
    a.src = sources;
    a.H = height;
    a.W = width;
    a.C = c;
    a.Hc = out_height;
    a.Wc = out_width;
    a.n_src = n_src;
    const char* e = std::getenv("PAPOF_MOSAIC_CULL");  // "0": no tile-level culling (tools/mosaic_probe.py measures its worth)
    a.cull = !(e && e[0] == '0');
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_mosaic(static_cast<hipStream_t>(stream), a, n_out, mode);
}

// Every instance launch_mosaic dispatches to has a lane per slot (n_src <= 64 * TY), so phase 1's loop over the slots runs once.
static_assert(kMaxSrc <= kMosTX * 4 && 8 <= kMosTX * 4 && 16 <= kMosTX * 4 && 32 <= kMosTX * 2 &&
                  PAPOF_MOSAIC_MAX_MEDIAN <= kMosTX * 1 && PAPOF_MOSAIC_MAX_SOURCES < kMaxSrc,
              "k_mosaic: a lane per slot in one pass of phase 1");
