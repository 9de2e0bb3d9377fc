// papteam_opticalflow_amd/csrc/shots.hip -- shot boundaries, the device's part: every frame of a video reduced to luma
// histograms per cell (papof_cell_hist_tensor).  The rule that turns them into cuts is the host's (tensors.py:
// shot_distances, detect_cuts), on the small count tensor, as match_fields is for telecine.hip's counts.
//
// Why.  Every *_video call takes its frames to be one shot.  Across a cut the solver spends a solve on a pair without motion
// and returns noise; the calls behind it average two scenes.  The measure that finds a cut must not fire on motion: a
// histogram of a region forgets where its pixels are, so a pan changes it only by what enters and leaves, and the median
// over many regions forgets an object that crosses a few of them.  The kernel counts per cell of cell_rows x 64 pixels; the
// host adds cells to regions (histograms add), which keeps the region's size the host's choice.
//
// Semantics: include/papof.h.  Every value is quantised to 0 .. 65535 first (cells.h: load_q, k_field_metrics's rule) and
// everything after that is integer: the counts are exact.
//
// Mapping, k_cell_hist: k_field_metrics's.  One wave per cell, lane = column; a block is four horizontally adjacent cells;
// blockIdx.x the block of cells, blockIdx.y the frame, all T frames through launch_tiles.  The lane walks the cell's rows,
// kRowsAhead at a time with all their loads issued before the first vote.  Packed uint8 rows (NHWC frames) are loaded as
// aligned dwords by the wave (cells.h: packed_pixel), everything else lane by lane; only the channels the luma reads are
// loaded (one of 1 or 2, three of 3 or 4).  Lane k counts bin k: per row the wave votes once per BIT of the bin index
// (log2(bins) __ballots, not one per bin: with an accumulator and a vote per bin the 64-bin instance spilled 474 SGPRs), lane
// k intersects the votes, each inverted where its own bit is clear, with the mask of the lanes that hold a pixel of the row,
// and adds the population count: the lanes whose bin is k.  No lane leaves before the last vote; no atomics, no workspace,
// no LDS; every element of `hist` is written exactly once; every offset 64-bit.
#include "cells.h"

namespace papof {

namespace {

constexpr int kHistRowsAhead = 4;  // rows of a cell whose loads are in flight together (k_field_metrics's depth)
constexpr int kLumaC = 3;          // the channels the luma reads at most

struct HistArgs {
    papof_tensor fr;  // frames (frame, row, column, channel)
    int* out;         // (frame, cy, cx, bin)
    int H, W, C;
    int cell_rows;
    int Gy, Gx;
};

// The luma's channels of pixel x0 + lane of the row at `row` (the offset of its frame and row): PACKED through packed_pixel
// as the pixel's word, else q of NCH channels; a lane beyond the image (not `live`) gets values that mean nothing.  Called by
// all lanes of the wave; x0, row and n = the segment's pixels are wave-uniform.
template <int FD, bool PACKED, int NCH>
__device__ __forceinline__ void load_luma_row(const HistArgs& a, long long row, long long x0, int n, int lane, bool live,
                                              int (&v)[kLumaC]) {
    if (PACKED) {
        v[0] = (int)packed_pixel(static_cast<const unsigned char*>(a.fr.data) + row + x0 * a.C, n * a.C, lane, a.C);
    } else {  // (a lane beyond the image reads the cell's first column: no branch around a load)
        const long long o = row + (x0 + (live ? lane : 0)) * a.fr.stride[2];
#pragma unroll
        for (int k = 0; k < NCH; k++) v[k] = load_q<FD>(a.fr, o + k * a.fr.stride[3]);
    }
}

// L of a row that load_luma_row made: q0, or (77 q0 + 150 q1 + 29 q2) >> 8 of three channels (<= 65535: the weights add to 256)
template <bool PACKED, int NCH>
__device__ __forceinline__ int luma(const int (&v)[kLumaC]) {
    const unsigned w = (unsigned)v[0];
    if (NCH == 1) return PACKED ? 257 * (int)(w & 255u) : v[0];
    if (PACKED) return (77 * 257 * (int)(w & 255u) + 150 * 257 * (int)((w >> 8) & 255u) + 29 * 257 * (int)((w >> 16) & 255u)) >> 8;
    return (77 * v[0] + 150 * v[1] + 29 * v[2]) >> 8;
}

// blockIdx.x: block `tile0` + x of the Gy x ceil(Gx / 4) blocks of cells in row-major order; blockIdx.y: frame `frame0` + y.
// A step is free of branches: a row index beyond the cell is clamped into the frame for the load and its votes are dropped.
template <int FD, bool PACKED, int NCH, int BINS>
__global__ __launch_bounds__(kCellW* kCellsX) void k_cell_hist(const HistArgs a, long long tile0, long long frame0) {
    const long long bx = (a.Gx + kCellsX - 1) / kCellsX, tile = tile0 + blockIdx.x;
    const int lane = threadIdx.x, cx = (int)(tile % bx) * kCellsX + (int)threadIdx.y;
    const long long cy = tile / bx, t = frame0 + blockIdx.y;
    if (cx >= a.Gx) return;  // (the whole wave)
    const long long x0 = (long long)cx * kCellW;
    const int n = (int)(a.W - x0 < kCellW ? a.W - x0 : kCellW);  // the cell's columns
    const bool live = lane < n;
    const long long own = t * a.fr.stride[0], last = a.H - 1;
    constexpr int kBits = BINS == 4 ? 2 : BINS == 8 ? 3 : BINS == 16 ? 4 : BINS == 32 ? 5 : 6;  // log2(BINS)
    const long long j0 = cy * a.cell_rows, j1 = j0 + a.cell_rows < a.H ? j0 + a.cell_rows : a.H;
    // f[i]: all ones where bit i of the lane's own bin (= its index) is CLEAR: vote i xor f[i] has the lanes that agree with it
    unsigned f[kBits];
#pragma unroll
    for (int i = 0; i < kBits; i++) f[i] = ((lane >> i) & 1) ? 0u : ~0u;
    const unsigned long long cell = __ballot(live);  // the lanes that hold a pixel of the cell
    unsigned mine = 0;
    for (long long jb = j0; jb < j1; jb += kHistRowsAhead) {
        int v[kHistRowsAhead][kLumaC] = {};
#pragma unroll
        for (int i = 0; i < kHistRowsAhead; i++) {
            const long long j = jb + i < last ? jb + i : last;
            load_luma_row<FD, PACKED, NCH>(a, own + j * a.fr.stride[1], x0, n, lane, live, v[i]);
        }
#pragma unroll
        for (int i = 0; i < kHistRowsAhead; i++) {
            const unsigned long long rowm = jb + i < j1 ? cell : 0ull;  // a row of this cell (wave-uniform)
            const int bin = (luma<PACKED, NCH>(v[i]) * BINS) >> 16;
            unsigned lo = (unsigned)rowm, hi = (unsigned)(rowm >> 32);
#pragma unroll
            for (int b = 0; b < kBits; b++) {
                const unsigned long long vote = __ballot((bin >> b) & 1);
                lo &= (unsigned)vote ^ f[b];
                hi &= (unsigned)(vote >> 32) ^ f[b];
            }
            mine += __popc(lo) + __popc(hi);
        }
    }
    if (lane < BINS) a.out[((t * a.Gy + cy) * a.Gx + cx) * BINS + lane] = (int)mine;
}

template <int FD, bool PACKED, int NCH>
auto hist_kernel_bins(int bins) {
    return bins == 4    ? k_cell_hist<FD, PACKED, NCH, 4>
           : bins == 8  ? k_cell_hist<FD, PACKED, NCH, 8>
           : bins == 16 ? k_cell_hist<FD, PACKED, NCH, 16>
           : bins == 32 ? k_cell_hist<FD, PACKED, NCH, 32>
                        : k_cell_hist<FD, PACKED, NCH, 64>;
}

// the instance for c channels and `bins` bins: the channel and vote loops are unrolled without a branch
template <int FD, bool PACKED>
auto hist_kernel(int c, int bins) {
    return c < 3 ? hist_kernel_bins<FD, PACKED, 1>(bins) : hist_kernel_bins<FD, PACKED, 3>(bins);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_cell_hist_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                      int cell_rows, int bins, int* hist, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1 || c > kMaxC || !hist) return PAPOF_EINVAL;
    if (cell_rows < 1 || cell_rows > kMaxCellRows) return PAPOF_EINVAL;
    if (bins != 4 && bins != 8 && bins != 16 && bins != 32 && bins != 64) return PAPOF_EINVAL;
    if (!in_frames(frames)) return PAPOF_EINVAL;
    HistArgs a{};
    a.fr = *frames;
    a.out = hist;
    a.H = height;
    a.W = width;
    a.C = c;
    a.cell_rows = cell_rows;
    a.Gy = (int)(((long long)height + cell_rows - 1) / cell_rows);
    a.Gx = (int)(((long long)width + kCellW - 1) / kCellW);
    PAPOF_HIP(hipSetDevice(h->device));
    // packed: uint8 whose channels and pixels are adjacent (NHWC frames as decoders return them, and any one-channel rows)
    const bool packed = a.fr.dtype == PAPOF_DTYPE_U8 && a.fr.stride[2] == c && (c == 1 || a.fr.stride[3] == 1);
    const auto kernel = packed                          ? hist_kernel<PAPOF_DTYPE_U8, true>(c, bins)
                        : a.fr.dtype == PAPOF_DTYPE_U8  ? hist_kernel<PAPOF_DTYPE_U8, false>(c, bins)
                        : a.fr.dtype == PAPOF_DTYPE_F32 ? hist_kernel<PAPOF_DTYPE_F32, false>(c, bins)
                                                        : hist_kernel<PAPOF_DTYPE_F64, false>(c, bins);
    return launch_grid<CellTile>(a.Gy, a.Gx, n_frames, static_cast<hipStream_t>(stream), 0, kernel, a);
}
