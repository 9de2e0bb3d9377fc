// papteam_opticalflow_amd/csrc/telecine.hip -- inverse telecine of a sequence of fields: which neighbour each field was
// scanned with (papof_field_metrics_tensor) and the weave of matched fields into the film's frames
// (papof_weave_fields_tensor).
//
// Why.  Film on interlaced video -- 3:2 pulldown on NTSC, 2:2 on PAL -- repeats every film frame over two or three
// consecutive fields.  Those fields show ONE instant: the flows between them are zero, the lines a field lacks stand in its
// partner exactly, and a deinterlacer that makes them up (deinterlace.hip) returns 60 half-invented frames where 24 exact
// ones exist.  The inverse is to find the partner of every field and to weave.
//
// The measure.  Field t is woven, line by line, once with field t - 1 and once with field t + 1 -- two fields of one parity:
// the same rows at the same places -- and a pixel of its line is combed where it lies outside the range of the lines above
// and below it by more than a threshold.  Absolute comb counts do not separate film from video: on real frames vertical
// detail looks like combing (8 .. 18 % of a 16 x 64 cell at 10 / 255 on the committed 1080p frame).  The counts taken
// pixel by pixel AGAINST THE OTHER CANDIDATE do: the texture cancels, a film field has (winner, loser) counts like (463, 0),
// a video field (30, 30), a static field (0, 0).  The kernel reduces every field to three integer counts per cell of
// cell_rows x 64 pixels; the rule that turns them into links is the host's (tensors.py: match_fields).
//
// Semantics: include/papof.h.  Every value is quantised to 0 .. 65535 first and everything after that is integer: the counts
// are exact and do not depend on an order of summation.
//
// Mapping, k_field_metrics.  One wave per cell, lane = column; a block is four horizontally adjacent cells; blockIdx.x the
// block of cells, blockIdx.y the field, all T fields in one launch.  The lane walks the cell's rows and keeps the previous
// row of both neighbours in registers, so that every row of the three fields is loaded once per cell plus one halo row; the
// three counts are __ballot + __popcll into wave-uniform accumulators (as k_mask_dilate packs its mask bits), and three
// lanes store them.  No lane leaves before the last __ballot or __shfl.  Packed uint8 rows (NHWC frames) are loaded as
// aligned dwords by the wave and handed to their lanes across the wave (cells.h: packed_pixel); everything else lane by lane.  No
// atomics, no workspace, every element of `metrics` is written exactly once -- fields 0 and T - 1, which have one
// neighbour, get zeros --, every offset 64-bit.
//
// Mapping, k_weave_fields.  k_deinterlace's: a block is a 64 x 4 tile of field pixels, blockIdx.x the tile, blockIdx.y the
// frame; one lane writes rows 2 j and 2 j + 1 of its column from row j of the frame's two fields: one pass, every output
// element written once.
#include "cells.h"

namespace papof {

namespace {

constexpr int kRowsAhead = 4;  // rows of a cell whose loads are in flight together (1: 1.12 x, 8: 1.14 x the kernel's time at 4)

struct MetricArgs {
    papof_tensor fl;  // fields (field, row, column, channel)
    int* out;         // (field, plane, cy, cx)
    int T, Hf, W, C;
    int first, cell_rows, comb_q, diff_q;
    int Gy, Gx;
};

// m(b; a, c): how far b lies outside the range of a and c
__device__ __forceinline__ int comb(int b, int a, int c) {
    const int da = a - b, dc = c - b;
    if ((da > 0 && dc > 0) || (da < 0 && dc < 0)) return min(abs(da), abs(dc));
    return 0;
}

// q of the C channels of pixel x0 + lane of the row at `row` (the offset of its field and row): PACKED (uint8, channels and
// pixels adjacent) through packed_pixel, else one load per channel; a lane beyond the image (not `live`) gets values that
// mean nothing.  Called by all lanes of the wave; x0, row and n = the segment's pixels are wave-uniform.
template <int FD, bool PACKED, int C>
__device__ __forceinline__ void load_row(const MetricArgs& a, long long row, long long x0, int n, int lane, bool live,
                                         int (&v)[kMaxC]) {
    if (PACKED) {  // (the word as it is, in v[0]: chan() takes it apart where it is used, which keeps a row in one register)
        v[0] = (int)packed_pixel(static_cast<const unsigned char*>(a.fl.data) + row + x0 * C, n * C, lane, C);
    } else {  // (a lane beyond the image reads the cell's first column: no branch around a load)
        const long long o = row + (x0 + (live ? lane : 0)) * a.fl.stride[2];
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = load_q<FD>(a.fl, o + k * a.fl.stride[3]);
    }
}

// channel k of a row that load_row made
template <bool PACKED>
__device__ __forceinline__ int chan(const int (&v)[kMaxC], int k) {
    return PACKED ? 257 * (int)(((unsigned)v[0] >> (8 * k)) & 255u) : v[k];
}

// blockIdx.x: block `tile0` + x of the Gy x ceil(Gx / 4) blocks of cells in row-major order; blockIdx.y: field `frame0` + y.
// The walk down a cell is a chain of dependent steps -- load three rows, vote, next row --, and with one row per step it is
// the loads' latency that the kernel takes (profiles/telecine_probe.txt): the rows are taken kRowsAhead at a time, all their
// loads issued before the first vote.  A step is free of branches: a row index beyond the field or the cell is clamped into
// the field for the load and its votes are dropped (`valid`, wave-uniform).
template <int FD, bool PACKED, int C>
__global__ __launch_bounds__(kCellW* kCellsX) void k_field_metrics(const MetricArgs a, long long tile0, long long frame0) {
    const long long bx = (a.Gx + kCellsX - 1) / kCellsX, tile = tile0 + blockIdx.x;
    const int lane = threadIdx.x, cx = (int)(tile % bx) * kCellsX + (int)threadIdx.y;
    const long long cy = tile / bx, t = frame0 + blockIdx.y;
    if (cx >= a.Gx) return;  // (the whole wave)
    const long long x0 = (long long)cx * kCellW;
    const int n = (int)(a.W - x0 < kCellW ? a.W - x0 : kCellW);  // the cell's columns
    const bool live = lane < n;
    unsigned n0 = 0, n1 = 0, n2 = 0;
    if (t >= 1 && t <= a.T - 2) {
        const int p = (int)((t + a.first) & 1), last = a.Hf - 1;
        const int j0 = (int)cy * a.cell_rows, j1 = j0 + a.cell_rows < a.Hf ? j0 + a.cell_rows : a.Hf;
        const long long own = t * a.fl.stride[0], prv = (t - 1) * a.fl.stride[0], nxt = (t + 1) * a.fl.stride[0];
        // the neighbours' rows above and below the own row j: j - 1 + p and j + p; `am`, `ap`: the row above of fields t - 1, t + 1
        int am[kMaxC] = {0, 0, 0, 0}, ap[kMaxC] = {0, 0, 0, 0};
        {
            const long long r = (long long)clamp_to(j0 - 1 + p, a.Hf) * a.fl.stride[1];
            load_row<FD, PACKED, C>(a, prv + r, x0, n, lane, live, am);
            load_row<FD, PACKED, C>(a, nxt + r, x0, n, lane, live, ap);
        }
        for (int jb = j0; jb < j1; jb += kRowsAhead) {
            int cm[kRowsAhead][kMaxC] = {}, cp[kRowsAhead][kMaxC] = {}, b[kRowsAhead][kMaxC] = {};
#pragma unroll
            for (int i = 0; i < kRowsAhead; i++) {
                const long long r = (long long)clamp_to(jb + i + p, a.Hf) * a.fl.stride[1];
                load_row<FD, PACKED, C>(a, prv + r, x0, n, lane, live, cm[i]);
                load_row<FD, PACKED, C>(a, nxt + r, x0, n, lane, live, cp[i]);
                load_row<FD, PACKED, C>(a, own + (long long)clamp_to(jb + i, a.Hf) * a.fl.stride[1], x0, n, lane, live, b[i]);
            }
#pragma unroll
            for (int i = 0; i < kRowsAhead; i++) {
                const int j = jb + i;
                const bool valid = j < j1 && j + p <= last && j - 1 + p >= 0;  // j is a centre row of this cell (wave-uniform)
                const int(&um)[kMaxC] = i ? cm[i ? i - 1 : 0] : am;  // the rows above: the rows below of the step before
                const int(&up)[kMaxC] = i ? cp[i ? i - 1 : 0] : ap;
                int Mm = 0, Mp = 0, nd = 0;
#pragma unroll
                for (int k = 0; k < C; k++) {
                        const int bk = chan<PACKED>(b[i], k), a0 = chan<PACKED>(um, k), c0 = chan<PACKED>(cm[i], k);
                        const int a1 = chan<PACKED>(up, k), c1 = chan<PACKED>(cp[i], k);
                        Mm = max(Mm, comb(bk, a0, c0));
                        Mp = max(Mp, comb(bk, a1, c1));
                        nd = max(nd, max(abs(a1 - a0), abs(c1 - c0)));
                }
                const bool count = live && valid;
                n0 += __popcll(__ballot(count && Mp > Mm + a.comb_q));
                n1 += __popcll(__ballot(count && Mm > Mp + a.comb_q));
                n2 += __popcll(__ballot(count && nd > a.diff_q));
            }
#pragma unroll
            for (int k = 0; k < kMaxC; k++) {
                am[k] = cm[kRowsAhead - 1][k];
                ap[k] = cp[kRowsAhead - 1][k];
            }
        }
    }
    if (lane < 3) {
        const long long cells = (long long)a.Gy * a.Gx;
        a.out[(t * 3 + lane) * cells + cy * a.Gx + cx] = (int)(lane == 0 ? n0 : lane == 1 ? n1 : n2);
    }
}

// the instance for c channels: the channel loops are unrolled without a branch, so that no load waits behind one
template <int FD, bool PACKED>
auto metrics_kernel(int c) {
    return c == 1 ? k_field_metrics<FD, PACKED, 1> : c == 2 ? k_field_metrics<FD, PACKED, 2>
           : c == 3 ? k_field_metrics<FD, PACKED, 3> : k_field_metrics<FD, PACKED, 4>;
}

constexpr int kWeaveTX = 64, kWeaveTY = 4;  // a 64 x 4 tile of field pixels per block (256 lanes: lut)
using WeaveTile = Tile<kWeaveTX, kWeaveTY>;

struct WeaveArgs {
    papof_tensor fl;   // fields (field, row, column, channel)
    papof_tensor out;  // (frame, row, column, channel), 2 Hf rows
    const int* table;  // (frame, {field of the even rows, field of the odd rows})
    int Hf, W, C;
};

// grid.h's grid over the field's 64 x 4 tiles; blockIdx.y: frame `frame0` + y.
template <int FD>
__global__ __launch_bounds__(kWeaveTX* kWeaveTY) void k_weave_fields(const WeaveArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kWeaveTX>(lut);
    PAPOF_TILE_PIXEL(WeaveTile, tile0, a.W, int, x, long long, j);
    if (x >= a.W || j >= a.Hf) return;
    const long long n = frame0 + blockIdx.y;
    const long long pix = j * a.fl.stride[1] + x * a.fl.stride[2];
    const long long o = n * a.out.stride[0] + 2 * j * a.out.stride[1] + x * a.out.stride[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const long long f = (long long)a.table[2 * n + r] * a.fl.stride[0] + pix;
#pragma unroll
        for (int ch = 0; ch < kMaxC; ch++)
            if (ch < a.C)
                store(a.out, o + r * a.out.stride[1] + ch * a.out.stride[3], load_frame<FD>(a.fl, f + ch * a.fl.stride[3], lut));
    }
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_field_metrics_tensor(papof_handle* h, int n_fields, int field_height, int width, int c,
                                          const papof_tensor* fields, int first, int cell_rows, int comb_q, int diff_q,
                                          int* metrics, void* stream) {
    if (!h || n_fields < 3 || field_height < 1 || field_height > 0x3fffffff || width < 1 || c < 1 || c > kMaxC)
        return PAPOF_EINVAL;
    if ((first != 0 && first != 1) || cell_rows < 1 || cell_rows > kMaxCellRows) return PAPOF_EINVAL;
    if (comb_q < 0 || comb_q > kMaxQ || diff_q < 0 || diff_q > kMaxQ || !metrics) return PAPOF_EINVAL;
    if (!in_frames(fields)) return PAPOF_EINVAL;
    MetricArgs a{};
    a.fl = *fields;
    a.out = metrics;
    a.T = n_fields;
    a.Hf = field_height;
    a.W = width;
    a.C = c;
    a.first = first;
    a.cell_rows = cell_rows;
    a.comb_q = comb_q;
    a.diff_q = diff_q;
    a.Gy = (field_height + cell_rows - 1) / cell_rows;
    a.Gx = (int)(((long long)width + kCellW - 1) / kCellW);
    PAPOF_HIP(hipSetDevice(h->device));
    // packed: uint8 whose channels and pixels are adjacent (NHWC frames as decoders return them, and any one-channel rows)
    const bool packed = a.fl.dtype == PAPOF_DTYPE_U8 && a.fl.stride[2] == c && (c == 1 || a.fl.stride[3] == 1);
    const auto kernel = packed                            ? metrics_kernel<PAPOF_DTYPE_U8, true>(c)
                        : a.fl.dtype == PAPOF_DTYPE_U8    ? metrics_kernel<PAPOF_DTYPE_U8, false>(c)
                        : a.fl.dtype == PAPOF_DTYPE_F32   ? metrics_kernel<PAPOF_DTYPE_F32, false>(c)
                                                          : metrics_kernel<PAPOF_DTYPE_F64, false>(c);
    return launch_grid<CellTile>(a.Gy, a.Gx, a.T, static_cast<hipStream_t>(stream), 0, kernel, a);
}

extern "C" int papof_weave_fields_tensor(papof_handle* h, int n_fields, int field_height, int width, int c,
                                         const papof_tensor* fields, int n_frames, const int* table,
                                         const papof_tensor* video, void* stream) {
    if (!h || n_fields < 1 || field_height < 1 || field_height > 0x3fffffff || width < 1 || c < 1 || c > kMaxC)
        return PAPOF_EINVAL;
    if (n_frames < 1 || !table) return PAPOF_EINVAL;
    if (!in_frames(fields) || !out_frames(video)) return PAPOF_EINVAL;
    if (video->data == fields->data) return PAPOF_EINVAL;
    WeaveArgs a{};
    a.fl = *fields;
    a.out = *video;
    a.table = table;
    a.Hf = field_height;
    a.W = width;
    a.C = c;
    PAPOF_HIP(hipSetDevice(h->device));
    const auto kernel = by_dtype(a.fl.dtype, [](auto fd) { return k_weave_fields<fd()>; });
    return launch_grid<WeaveTile>(a.Hf, a.W, n_frames, static_cast<hipStream_t>(stream), 0, kernel, a);
}
