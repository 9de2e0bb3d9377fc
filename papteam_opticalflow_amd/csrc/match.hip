// papteam_opticalflow_amd/csrc/match.hip -- dense block matching on device tensors (papof_match_tensor,
// papof_match_densify_tensor): the integer displacement of every cell of a decimated frame that minimises a sum of absolute
// differences over a patch, as a start for the coarse-to-fine solver on motions that do not survive its pyramid.
//
// Semantics: include/papof.h, papof_match_tensor.  Everything is integer arithmetic on uint8 samples, so the result is a pure
// function of the inputs; tests/_match_ref.py restates it in numpy and the device's bytes are held to that.
//
// Mapping.  k_match_prepare: one lane per coarse pixel of a frame; it reads the stride^2 x C samples through the descriptor,
// quantises, box-decimates and stores the pixel as ONE packed dword (channel c in byte c, missing channels 0), so that one
// v_sad_u8 is the absolute difference of a pixel pair over all its channels.
// k_match: a block is a 32 x 8 tile of coarse pixels (grid.h's grid of tiles and items), one lane per pixel.  A's
// tile with a halo of `patch` and B's tile with a halo of `patch + search` are staged once in LDS, coordinates clamped as
// the rule clamps them; a lane outside the grid computes on clamped data and stores nothing.  A lane evaluates kG = 4
// horizontally neighbouring candidates at a time: per window row it reads the row of A (2 P + 1 dwords) and the row of B
// under the four candidates (2 P + 4 dwords) into registers and issues 4 (2 P + 1) v_sad_u8 on them -- (4 P + 5) LDS
// reads for 4 (2 P + 1) SADs, against two reads per SAD for the candidate-by-candidate loop.  The last group of a row
// computes the candidates past dx = search for nothing: 3 of 44 at search 20 with kG = 4, 7 of 48 with kG = 8 (what bounds
// the kernel and the other kG measured: DESIGN.md section 22).  Rows of dy and groups of dx that no cell of the block's
// tile may take (they leave the grid for all of them) are skipped, block-uniformly.  The window is a template
// parameter (P = 1 .. 7) so that both rows are registers with constant indices.  The 32 lanes of a half-wave read 32
// consecutive dwords of one LDS row: no bank conflict whatever the row pitch.  The running best is one 64-bit key per lane
// (cost, dx^2 + dy^2, dy, dx packed from the top), so the order of the visit does not matter.
// k_match_densify: one lane per full-resolution pixel; the forward-backward test of its cell, the flow and the hole mask.
//
// Hierarchical search (papof_match_hier_tensor; tests/_hmatch_ref.py restates it).  k_match_prepare decimates the frames
// once per level (strides up to 32; from 8 up its sibling k_match_prepare_wide, 16 or 64 lanes per cell), k_match runs on the top level and leaves its displacements as packed dwords (dx in the
// low half, dy in the high half, two's complement) in the workspace, and k_match_refine<P> takes every lower level from its
// parents: a block is again a 32 x 8 tile and an item, one lane per cell.  A's tile (halo P) and B's window around the zero
// predictor (halo P + r) are staged in LDS; the doubled vectors of the tile's parents -- the 16 x 4 parent cells and the
// ring their side neighbours reach, 19 x 7 with both clamps -- go to LDS too and are reduced to a bounding box with LDS
// atomics.  Where the box spreads over at most kSpread cells in x and in y the block stages ONE window of B that covers
// every parent-predicted candidate of the tile and the lanes walk their candidates from LDS: the 2 r + 1 candidates
// adjacent in dx of a predictor share their register rows as k_match's kG candidates do -- (2 P + 1) + (2 P + 1 + 2 r)
// LDS reads for (2 r + 1) (2 P + 1) v_sad_u8.  Where it spreads further (a motion boundary crosses the tile) the block reads
// B through clamped global addresses; the choice is block-uniform and both paths read the same values in the same order,
// so they give the same bytes (PAPOF_MATCH_STAGED=0 sends every tile down the global path).  kSpread = 16: with P = 7 and
// r = 3 the three tiles are 1012 + 1456 + 2992 dwords = 21.8 KB, so seven blocks share a CU's 160 KB of LDS.
//
// Re-centred search (papof_match_recentre_tensor; tests/_recentre_ref.py restates it).  The hierarchical chain runs down to
// level 0 and leaves d_h there as packed dwords; k_match_origin, one block per 32 x 8 tile and item, selects per component
// the lower median of the tile's vectors by rank counting in LDS (one writer, no atomics) and writes one packed origin per
// tile; k_match_recentre<P>, k_match's sibling, stages B's window displaced by that origin and runs k_match's loop on it with
// k_match_refine's 26 + 18 + 10 + 10 bit key, then takes the lane's own d_h where the window did not hold it.  LDS is
// k_match's with `window` for `search`: 43264 bytes at window 32, patch 7, three blocks per CU.  All on the caller's stream.
#include "sampler.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace papof {

namespace {

constexpr int kTX = 32, kTY = 8;  // the tile of coarse pixels (256 lanes)
using GridTile = Tile<kTX, kTY>;
constexpr int kG = 4;             // candidates along dx that a lane evaluates together (1, 8, 16)
constexpr int kMaxPatch = 7, kMaxSearch = 32, kMaxPenalty = 65535;

constexpr int kMaxLevels = 4, kMaxRefine = 3, kMaxTopStride = 32;
constexpr int kSpread = 16;           // k_match_refine: the largest spread of the doubled parent vectors that is staged
constexpr int kRingW = 19, kRingH = 7;  // k_match_refine: the parents of a tile, from (x0 / 2 - 2, y0 / 2 - 2)

inline bool valid_stride(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }

// a displacement in cells as one dword: dx in the low half, dy in the high half (|d| <= 277 at every level)
__device__ __forceinline__ unsigned pack_d(int dx, int dy) { return ((unsigned)dx & 0xffffu) | ((unsigned)dy << 16); }
__device__ __forceinline__ int unpack_dx(unsigned v) { return (int)(short)(v & 0xffffu); }
__device__ __forceinline__ int unpack_dy(unsigned v) { return (int)(short)(v >> 16); }

// groups of kG candidates that cover dx = -search .. search
__host__ __device__ inline int groups_of(int search) { return (2 * search + 1 + kG - 1) / kG; }

// the sizes of k_match's staged tiles, in dwords
__host__ __device__ inline int a_width(int P) { return kTX + 2 * P; }
__host__ __device__ inline int a_height(int P) { return kTY + 2 * P; }
__host__ __device__ inline int b_width(int P, int search) { return kTX + 2 * P + kG * groups_of(search); }
__host__ __device__ inline int b_height(int P, int search) { return kTY + 2 * (P + search); }

long long lds_bytes(int P, int search) {
    return 4LL * (a_width(P) * a_height(P) + b_width(P, search) * b_height(P, search));
}

struct PrepArgs {
    papof_tensor in;   // (frame, row, column, channel)
    unsigned* packed;  // [frame][h][w], from the first frame of `in`
    int h, w, C, stride;
};

// one sample as the rule's uint8: uint8 as it is, float32 / float64 as clamp(rint(255 x), 0, 255), NaN -> 0
__device__ __forceinline__ unsigned quantise(const papof_tensor& t, long long o) {
    if (t.dtype == PAPOF_DTYPE_U8) return static_cast<const unsigned char*>(t.data)[o];
    const double x = t.dtype == PAPOF_DTYPE_F32 ? (double)static_cast<const float*>(t.data)[o] : static_cast<const double*>(t.data)[o];
    return (unsigned)fmin(fmax(rint(255.0 * x), 0.0), 255.0);  // (fmax drops the NaN)
}

// blockIdx.x: 256 coarse pixels from `cell0` in row-major order; blockIdx.y: frame `frame0` + y
__global__ __launch_bounds__(256) void k_match_prepare(const PrepArgs a, long long cell0, long long frame0) {
    const long long cell = (cell0 + blockIdx.x) * 256 + threadIdx.x, cells = (long long)a.h * a.w;
    if (cell >= cells) return;
    const long long f = frame0 + blockIdx.y;
    const int y = (int)(cell / a.w), x = (int)(cell - (long long)y * a.w), s = a.stride;
    const long long base = PAPOF_AT(a.in, f, (long long)y * s, (long long)x * s);
    const unsigned area = (unsigned)(s * s);
    unsigned pk = 0;
    for (int c = 0; c < a.C; c++) {
        unsigned sum = 0;
        for (int j = 0; j < s; j++)
            for (int i = 0; i < s; i++) sum += quantise(a.in, base + j * a.in.stride[1] + i * a.in.stride[2] + c * a.in.stride[3]);
        pk |= ((sum + area / 2) / area) << (8 * c);
    }
    a.packed[f * cells + cell] = pk;
}

// The same for the strides of the hierarchical search's upper levels (8 .. 32), where one lane per cell would read up to
// 1024 x C samples one after the other: G lanes share a cell (G a power of two <= 64, a divisor of stride^2: the lanes of
// one wave), each sums every G-th sample of the cell in row-major order, and the partial sums meet through the wave's
// shuffles.  A lane's sums stay below 1024 x 255 < 2^18.  blockIdx.x: 256 / G cells from `cell0` x 256 / G.
template <int G>
__global__ __launch_bounds__(256) void k_match_prepare_wide(const PrepArgs a, long long cell0, long long frame0) {
    const long long cell = (cell0 + blockIdx.x) * (256 / G) + threadIdx.x / G, cells = (long long)a.h * a.w;
    if (cell >= cells) return;  // (the G lanes of a cell leave together)
    const int t = (int)threadIdx.x % G, s = a.stride;
    const long long f = frame0 + blockIdx.y;
    const int y = (int)(cell / a.w), x = (int)(cell - (long long)y * a.w);
    const long long base = PAPOF_AT(a.in, f, (long long)y * s, (long long)x * s);
    unsigned sum[4] = {0, 0, 0, 0};
    for (int idx = t; idx < s * s; idx += G) {
        const int j = idx / s, i = idx - j * s;
        const long long o = base + j * a.in.stride[1] + i * a.in.stride[2];
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < a.C) sum[c] += quantise(a.in, o + c * a.in.stride[3]);
    }
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int m = G / 2; m > 0; m >>= 1) sum[c] += __shfl_xor(sum[c], m);
    if (t != 0) return;
    const unsigned area = (unsigned)(s * s);
    unsigned pk = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) pk |= ((sum[c] + area / 2) / area) << (8 * c);  // (a missing channel: (0 + area / 2) / area = 0)
    a.packed[f * cells + cell] = pk;
}

struct MatchArgs {
    const unsigned* packed;  // [frame][h][w]
    papof_tensor disp;       // (item, row, column, {dx, dy})
    papof_tensor cost;       // (item, row, column, -)
    int h, w, stride, search, penalty;
    int n_pairs, seq;
    unsigned* out;           // k_match<P, true>: [item][h][w] packed displacements in cells, instead of disp and cost
};

// P: the patch radius.  grid.h's grid over the grid's 32 x 8 tiles; blockIdx.y: item
// `item0` + y -- items below n_pairs run forward (A the pair's first frame), the others backward.
// PACKED: the top level of the hierarchical search -- the match goes to a.out as one packed dword.
template <int P, bool PACKED = false>
__global__ __launch_bounds__(kTX* kTY) void k_match(const MatchArgs a, long long tile0, long long item0) {
    extern __shared__ __align__(16) unsigned smem_match[];
    constexpr int WN = 2 * P + 1;
    const int s = a.search, h = a.h, w = a.w, ng = groups_of(s);
    const int AW = a_width(P), AH = a_height(P), BW = b_width(P, s), BH = b_height(P, s);
    unsigned* const As = smem_match;
    unsigned* const Bs = As + AW * AH;

    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y, tid = ly * kTX + lx;
    PAPOF_TILE_ORIGIN(GridTile, tile0, w, int, x0, int, y0);
    const int x = x0 + lx, y = y0 + ly;
    const long long item = item0 + blockIdx.y, cells = (long long)h * w;
    const bool back = item >= a.n_pairs;
    const long long pair = back ? item - a.n_pairs : item;
    const long long first = pair, second = a.seq ? pair + 1 : a.n_pairs + pair;
    const unsigned* const A = a.packed + (back ? second : first) * cells;
    const unsigned* const B = a.packed + (back ? first : second) * cells;

    // ---- stage both tiles, every coordinate clamped into the grid
    for (int c = tid; c < AW * AH; c += kTX * kTY) {
        const int cy = c / AW, cx = c - cy * AW;
        As[c] = A[(long long)clamp_to(y0 - P + cy, h) * w + clamp_to(x0 - P + cx, w)];
    }
    for (int c = tid; c < BW * BH; c += kTX * kTY) {
        const int cy = c / BW, cx = c - cy * BW;
        Bs[c] = B[(long long)clamp_to(y0 - P - s + cy, h) * w + clamp_to(x0 - P - s + cx, w)];
    }
    __syncthreads();

    // ---- the lane's candidates: rows of dy, groups of kG along dx
    unsigned long long best = ~0ULL;
    for (int dyi = 0; dyi <= 2 * s; dyi++) {
        const int dy = dyi - s;
        if (y0 + kTY - 1 + dy < 0 || y0 + dy >= h) continue;  // inadmissible for every cell of the tile
        const bool row_in = y + dy >= 0 && y + dy < h;
        for (int g = 0; g < ng; g++) {
            if (x0 + kTX - 1 + kG * g + kG - 1 - s < 0 || x0 + kG * g - s >= w) continue;  // likewise
            unsigned acc[kG];
#pragma unroll
            for (int j = 0; j < kG; j++) acc[j] = 0;
            for (int oy = 0; oy < WN; oy++) {
                const unsigned* const ar = As + (ly + oy) * AW + lx;
                const unsigned* const br = Bs + (ly + oy + dyi) * BW + lx + kG * g;
                unsigned av[WN], bv[WN + kG - 1];
#pragma unroll
                for (int k = 0; k < WN; k++) av[k] = ar[k];
#pragma unroll
                for (int k = 0; k < WN + kG - 1; k++) bv[k] = br[k];
#pragma unroll
                for (int k = 0; k < WN; k++)
#pragma unroll
                    for (int j = 0; j < kG; j++) acc[j] = __builtin_amdgcn_sad_u8(av[k], bv[k + j], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < kG; j++) {
                const int dx = kG * g + j - s;
                const bool ok = dx <= s && row_in && x + dx >= 0 && x + dx < w;
                const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                const unsigned long long c = acc[j] + (unsigned)(a.penalty * (ax + ay));
                const unsigned long long key = (c << 26) | ((unsigned long long)(dx * dx + dy * dy) << 14) |
                                               ((unsigned long long)(dy + 64) << 7) | (unsigned long long)(dx + 64);
                best = ok && key < best ? key : best;
            }
        }
    }
    if (x >= w || y >= h) return;
    const int bdx = (int)(best & 127) - 64, bdy = (int)((best >> 7) & 127) - 64;
    if constexpr (PACKED) {
        a.out[item * cells + (long long)y * w + x] = pack_d(bdx, bdy);
        return;
    }
    const long long od = PAPOF_AT(a.disp, item, (long long)y, (long long)x);
    store(a.disp, od, (double)(a.stride * bdx));
    store(a.disp, od + a.disp.stride[3], (double)(a.stride * bdy));
    store(a.cost, PAPOF_AT(a.cost, item, (long long)y, (long long)x),
          (double)(best >> 26));
}

struct DensifyArgs {
    papof_tensor disp, rev;  // (item, row, column, {dx, dy}) on the coarse grid, in full-resolution pixels
    papof_tensor cost;       // (item, row, column, -); data NULL: not read
    papof_tensor flow;       // float64 (item, row, column, {vx, vy}) at full resolution
    papof_tensor mask;       // uint8 (item, row, column, -): nonzero = a hole
    double max_cost;         // < 0: no bound
    int H, W, h, w, stride, tol;
};

// blockIdx.x: 256 pixels from `pix0` in row-major order; blockIdx.y: item `item0` + y
__global__ __launch_bounds__(256) void k_match_densify(const DensifyArgs a, long long pix0, long long item0) {
    const long long pix = (pix0 + blockIdx.x) * 256 + threadIdx.x;
    if (pix >= (long long)a.H * a.W) return;
    const long long i = item0 + blockIdx.y;
    const int Y = (int)(pix / a.W), X = (int)(pix - (long long)Y * a.W);
    const int y = min(Y / a.stride, a.h - 1), x = min(X / a.stride, a.w - 1);
    const long long od = PAPOF_AT(a.disp, i, (long long)y, (long long)x);
    const double fx = load_flow(a.disp, od), fy = load_flow(a.disp, od + a.disp.stride[3]);
    const double dx = fx / (double)a.stride, dy = fy / (double)a.stride;
    const double qx = (double)x + dx, qy = (double)y + dy;
    // a whole number of cells that lands inside the grid (false for a NaN)
    bool ok = rint(dx) == dx && rint(dy) == dy && qx >= 0 && qx <= (double)(a.w - 1) && qy >= 0 && qy <= (double)(a.h - 1);
    if (ok) {
        const long long orv = PAPOF_AT(a.rev, i, (long long)(int)qy, (long long)(int)qx);
        const double ex = dx + load_flow(a.rev, orv) / (double)a.stride;
        const double ey = dy + load_flow(a.rev, orv + a.rev.stride[3]) / (double)a.stride;
        ok = fabs(ex) <= (double)a.tol && fabs(ey) <= (double)a.tol;
    }
    if (ok && a.max_cost >= 0)
        ok = load_flow(a.cost, PAPOF_AT(a.cost, i, (long long)y, (long long)x)) <= a.max_cost;
    const long long of = PAPOF_AT(a.flow, i, (long long)Y, (long long)X);
    static_cast<double*>(a.flow.data)[of] = ok ? fx : 0.0;
    static_cast<double*>(a.flow.data)[of + a.flow.stride[3]] = ok ? fy : 0.0;
    // (store_u8 would evaluate the value before it reads a.mask.data: the kernel's tail is scheduled differently)
    static_cast<unsigned char*>(a.mask.data)[PAPOF_AT(a.mask, i, (long long)Y, (long long)X)] = ok ? 0 : 1;
}

bool valid_frame_size(int height, int width, int stride) {
    return valid_stride(stride) && height >= stride && width >= stride && (long long)height * width < (1LL << 30);
}

template <int P, bool PACKED = false>
int launch_match(hipStream_t st, const MatchArgs& a, long long items) {
    const size_t lds = (size_t)lds_bytes(P, a.search);
    return launch_grid<GridTile>(a.h, a.w, items, st, lds, k_match<P, PACKED>, a);
}

// the top level of the hierarchical search
int launch_match_packed(hipStream_t st, const MatchArgs& a, long long items, int patch) {
    switch (patch) {
        case 1: return launch_match<1, true>(st, a, items);
        case 2: return launch_match<2, true>(st, a, items);
        case 3: return launch_match<3, true>(st, a, items);
        case 4: return launch_match<4, true>(st, a, items);
        case 5: return launch_match<5, true>(st, a, items);
        case 6: return launch_match<6, true>(st, a, items);
        default: return launch_match<7, true>(st, a, items);
    }
}

// ---- the hierarchical search
struct RefineArgs {
    const unsigned* packed;  // the level's frames [frame][h][w]
    const unsigned* parent;  // [item][h1][w1]: the packed displacements of the level above
    unsigned* out;           // levels above 0: [item][h][w] packed displacements
    papof_tensor disp, cost;  // level 0: as MatchArgs
    int h, w, h1, w1, stride, refine, penalty;
    int n_pairs, seq, last, staged;
};

// the sizes of k_match_refine's staged tiles, in dwords: A as k_match's, B around the zero predictor, B under the parents
__host__ __device__ inline int z_width(int P, int r) { return kTX + 2 * (P + r); }
__host__ __device__ inline int z_height(int P, int r) { return kTY + 2 * (P + r); }

long long refine_lds_bytes(int P, int r) {
    return 4LL * (a_width(P) * a_height(P) + z_width(P, r) * z_height(P, r) +
                  (z_width(P, r) + kSpread) * (z_height(P, r) + kSpread));
}

// The 2 R + 1 candidates (px - R .. px + R, dy) of every dy = py - R .. py + R around one predictor (px, py), for the
// cell (x, y) = lane (lx, ly).  STAGED: B's rows come from the LDS window `bw` of pitch `pitch`, whose entry (0, 0) is
// B(clamp(y0 - P + py - R), clamp(x0 - P + px - R)) for the block's (x0, y0) -- bw already points at the lane's column and
// row 0; otherwise from B through clamped addresses.  Either way the same values meet the same v_sad_u8 in the same order.
template <int P, int R, bool STAGED>
__device__ __forceinline__ void refine_predictor(unsigned long long& best, const unsigned* As, int AW, const unsigned* bw,
                                                 int pitch, const unsigned* B, int h, int w, int x, int y, int lx, int ly,
                                                 int px, int py, int penalty) {
    constexpr int WN = 2 * P + 1, NC = 2 * R + 1;
#pragma unroll 1
    for (int eyi = 0; eyi < NC; eyi++) {
        const int dy = py + eyi - R;
        unsigned acc[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) acc[j] = 0;
#pragma unroll 1
        for (int oy = 0; oy < WN; oy++) {
            const unsigned* const ar = As + (ly + oy) * AW + lx;
            unsigned av[WN], bv[WN + NC - 1];
#pragma unroll
            for (int k = 0; k < WN; k++) av[k] = ar[k];
            if constexpr (STAGED) {
                const unsigned* const br = bw + (oy + eyi) * pitch;
#pragma unroll
                for (int k = 0; k < WN + NC - 1; k++) bv[k] = br[k];
            } else {
                const unsigned* const br = B + (long long)clamp_to(y - P + oy + dy, h) * w;
#pragma unroll
                for (int k = 0; k < WN + NC - 1; k++) bv[k] = br[clamp_to(x - P + k + px - R, w)];
            }
#pragma unroll
            for (int k = 0; k < WN; k++)
#pragma unroll
                for (int j = 0; j < NC; j++) acc[j] = __builtin_amdgcn_sad_u8(av[k], bv[k + j], acc[j]);
        }
        const bool row_in = y + dy >= 0 && y + dy < h;
#pragma unroll
        for (int j = 0; j < NC; j++) {
            const int dx = px + j - R;
            const bool ok = row_in && x + dx >= 0 && x + dx < w;
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const unsigned long long c = acc[j] + (unsigned)(penalty * (ax + ay));
            // (cost, dx^2 + dy^2, dy, dx) in 26 + 18 + 10 + 10 bits: |d| <= 277, a cost below 2^26
            const unsigned long long key = (c << 38) | ((unsigned long long)(unsigned)(dx * dx + dy * dy) << 20) |
                                           ((unsigned long long)(unsigned)(dy + 512) << 10) | (unsigned long long)(unsigned)(dx + 512);
            best = ok && key < best ? key : best;
        }
    }
}

// P: the patch radius.  blockIdx as k_match's.  Level l's cells from the packed displacements of level l + 1.
template <int P>
__global__ __launch_bounds__(kTX* kTY) void k_match_refine(const RefineArgs a, long long tile0, long long item0) {
    extern __shared__ __align__(16) unsigned smem_refine[];
    __shared__ int ring_x[kRingW * kRingH], ring_y[kRingW * kRingH], box[4];
    const int r = a.refine, h = a.h, w = a.w, h1 = a.h1, w1 = a.w1;
    const int AW = a_width(P), AH = a_height(P), ZW = z_width(P, r), ZH = z_height(P, r);
    unsigned* const As = smem_refine;
    unsigned* const Zs = As + AW * AH;
    unsigned* const Ws = Zs + ZW * ZH;

    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y, tid = ly * kTX + lx;
    PAPOF_TILE_ORIGIN(GridTile, tile0, w, int, x0, int, y0);
    const int x = x0 + lx, y = y0 + ly;
    const long long item = item0 + blockIdx.y, cells = (long long)h * w, cells1 = (long long)h1 * w1;
    const bool back = item >= a.n_pairs;
    const long long pair = back ? item - a.n_pairs : item;
    const long long first = pair, second = a.seq ? pair + 1 : a.n_pairs + pair;
    const unsigned* const A = a.packed + (back ? second : first) * cells;
    const unsigned* const B = a.packed + (back ? first : second) * cells;

    // ---- the parents' doubled vectors and their bounding box
    const int rx0 = x0 / 2 - 2, ry0 = y0 / 2 - 2;
    if (tid == 0) {
        box[0] = box[2] = 0x7fffffff;
        box[1] = box[3] = -0x7fffffff;
    }
    __syncthreads();
    if (tid < kRingW * kRingH) {
        const int ry = tid / kRingW, rx = tid - ry * kRingW;
        const unsigned v = a.parent[item * cells1 + (long long)clamp_to(ry0 + ry, h1) * w1 + clamp_to(rx0 + rx, w1)];
        const int vx = 2 * unpack_dx(v), vy = 2 * unpack_dy(v);
        ring_x[tid] = vx;
        ring_y[tid] = vy;
        atomicMin(&box[0], vx);
        atomicMax(&box[1], vx);
        atomicMin(&box[2], vy);
        atomicMax(&box[3], vy);
    }
    // ---- stage A's tile and B's window around the zero predictor, every coordinate clamped into the grid
    for (int c = tid; c < AW * AH; c += kTX * kTY) {
        const int cy = c / AW, cx = c - cy * AW;
        As[c] = A[(long long)clamp_to(y0 - P + cy, h) * w + clamp_to(x0 - P + cx, w)];
    }
    for (int c = tid; c < ZW * ZH; c += kTX * kTY) {
        const int cy = c / ZW, cx = c - cy * ZW;
        Zs[c] = B[(long long)clamp_to(y0 - P - r + cy, h) * w + clamp_to(x0 - P - r + cx, w)];
    }
    __syncthreads();
    const int min_x = box[0], min_y = box[2];
    const long long spread_x = (long long)box[1] - min_x, spread_y = (long long)box[3] - min_y;
    const bool staged = a.staged && spread_x <= kSpread && spread_y <= kSpread;  // block-uniform
    const int WP = ZW + (int)(staged ? spread_x : 0);
    if (staged) {  // ---- ONE window of B under every parent-predicted candidate of the tile
        const int WH = ZH + (int)spread_y;
        for (int c = tid; c < WP * WH; c += kTX * kTY) {
            const int cy = c / WP, cx = c - cy * WP;
            Ws[c] = B[(long long)clamp_to(y0 - P - r + min_y + cy, h) * w + clamp_to(x0 - P - r + min_x + cx, w)];
        }
        __syncthreads();
    }

    // ---- the lane's predictors: its parent, the side neighbours in x, in y and in both, and zero
    const int px = min(x >> 1, w1 - 1), py = min(y >> 1, h1 - 1);
    const int nx = clamp_to(px + ((x & 1) ? 1 : -1), w1), ny = clamp_to(py + ((y & 1) ? 1 : -1), h1);
    const int ipx = clamp_to(px - rx0, kRingW), inx = clamp_to(nx - rx0, kRingW);
    const int ipy = clamp_to(py - ry0, kRingH), iny = clamp_to(ny - ry0, kRingH);
    unsigned long long best = ~0ULL;
#pragma unroll 1
    for (int k = 0; k < 5; k++) {
        const int ri = (k & 2 ? iny : ipy) * kRingW + (k & 1 ? inx : ipx);
        const int vx = k == 4 ? 0 : ring_x[ri], vy = k == 4 ? 0 : ring_y[ri];
        const bool lds = k == 4 || staged;
        const unsigned* const bw = k == 4 ? Zs + ly * ZW + lx : staged ? Ws + (ly + vy - min_y) * WP + lx + (vx - min_x) : Zs;
        const int pitch = k == 4 ? ZW : WP;
#define PAPOF_REFINE(R)                                                                                                  \
    if (lds)                                                                                                             \
        refine_predictor<P, R, true>(best, As, AW, bw, pitch, B, h, w, x, y, lx, ly, vx, vy, a.penalty);                 \
    else                                                                                                                 \
        refine_predictor<P, R, false>(best, As, AW, bw, pitch, B, h, w, x, y, lx, ly, vx, vy, a.penalty)
        if (r == 1) {
            PAPOF_REFINE(1);
        } else if (r == 2) {
            PAPOF_REFINE(2);
        } else {
            PAPOF_REFINE(3);
        }
#undef PAPOF_REFINE
    }
    if (x >= w || y >= h) return;
    const int bdx = (int)(best & 1023) - 512, bdy = (int)((best >> 10) & 1023) - 512;
    if (!a.last) {
        a.out[item * cells + (long long)y * w + x] = pack_d(bdx, bdy);
        return;
    }
    const long long od = PAPOF_AT(a.disp, item, (long long)y, (long long)x);
    store(a.disp, od, (double)(a.stride * bdx));
    store(a.disp, od + a.disp.stride[3], (double)(a.stride * bdy));
    store(a.cost, PAPOF_AT(a.cost, item, (long long)y, (long long)x),
          (double)(best >> 38));
}

template <int P>
int launch_refine(hipStream_t st, const RefineArgs& a, long long items) {
    const size_t lds = (size_t)refine_lds_bytes(P, a.refine);
    return launch_grid<GridTile>(a.h, a.w, items, st, lds, k_match_refine<P>, a);
}

// k_match_prepare of both frame tensors at one stride, into `packed` ([frame][h][w], the first tensor's frames first)
// (the hierarchical call's: strides from 8 up go to k_match_prepare_wide; papof_match_tensor launches what it always did)
int launch_prepare(hipStream_t st, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2, int height,
                   int width, int c, int stride, unsigned* packed) {
    PrepArgs p{};
    p.h = height / stride;
    p.w = width / stride;
    p.C = c;
    p.stride = stride;
    const long long cells = (long long)p.h * p.w, blocks = (cells + 255) / 256;
    const long long n_first = sequence ? (long long)n_pairs + 1 : n_pairs;
    for (int k = 0; k < (sequence ? 1 : 2); k++) {
        p.in = k == 0 ? *frames : *frames2;
        p.packed = packed + (k == 0 ? 0 : n_first * cells);
        const long long n = k == 0 ? n_first : n_pairs;
        if (stride >= 16)
            PAPOF_TRY(launch_tiles((cells + 3) / 4, n, [&](dim3 grid, long long c0, long long f0) {
                hipLaunchKernelGGL(k_match_prepare_wide<64>, grid, dim3(256), 0, st, p, c0, f0);
            }));
        else if (stride == 8)
            PAPOF_TRY(launch_tiles((cells + 15) / 16, n, [&](dim3 grid, long long c0, long long f0) {
                hipLaunchKernelGGL(k_match_prepare_wide<16>, grid, dim3(256), 0, st, p, c0, f0);
            }));
        else
            PAPOF_TRY(launch_tiles(blocks, n, [&](dim3 grid, long long c0, long long f0) {
                hipLaunchKernelGGL(k_match_prepare, grid, dim3(256), 0, st, p, c0, f0);
            }));
    }
    return PAPOF_OK;
}

// ---- the re-centred search (papof_match_recentre_tensor; tests/_recentre_ref.py restates it)
constexpr int kMaxWindow = 32;

struct OriginArgs {
    const unsigned* dh;  // [item][h][w]: the hierarchy's packed displacements of level 0
    unsigned* origin;    // [item][tile]: the packed origin of every 32 x 8 tile
    int h, w;
};

// blockIdx.x: tile `tile0` + x; blockIdx.y: item `item0` + y; one lane per cell of the tile.  The tile's packed vectors go
// to LDS; every in-grid lane counts, per component, the cells before its own in the order (value, lane): the lane whose
// count is the rank (n - 1) / 2 holds the lower median.  Every rank is held by exactly one lane: one writer, no atomics.
__global__ __launch_bounds__(kTX* kTY) void k_match_origin(const OriginArgs a, long long tile0, long long item0) {
    __shared__ unsigned vec[kTX * kTY];
    __shared__ int med[2];
    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y, tid = ly * kTX + lx;
    const long long ty = (a.h + kTY - 1) / kTY;
    PAPOF_TILE_ORIGIN(GridTile, tile0, a.w, int, x0, int, y0);
    const int tw = min(kTX, a.w - x0), th = min(kTY, a.h - y0), n = tw * th;  // the tile clipped to the grid
    const long long item = item0 + blockIdx.y;
    const bool in = lx < tw && ly < th;
    const unsigned mine = in ? a.dh[item * a.h * a.w + (long long)(y0 + ly) * a.w + x0 + lx] : 0u;
    vec[tid] = mine;
    __syncthreads();
    if (in) {
        const int mx = unpack_dx(mine), my = unpack_dy(mine);
        int before_x = 0, before_y = 0;
        for (int j = 0; j < th; j++)
            for (int i = 0; i < tw; i++) {
                const int k = j * kTX + i;
                const unsigned v = vec[k];
                const int vx = unpack_dx(v), vy = unpack_dy(v);
                before_x += vx < mx || (vx == mx && k < tid);
                before_y += vy < my || (vy == my && k < tid);
            }
        if (before_x == (n - 1) / 2) med[0] = mx;
        if (before_y == (n - 1) / 2) med[1] = my;
    }
    __syncthreads();
    if (tid == 0) a.origin[item * (tx * ty) + tile] = pack_d(med[0], med[1]);
}

struct RecentreArgs {
    const unsigned* packed;  // level 0's frames [frame][h][w]
    const unsigned* dh;      // [item][h][w]: the hierarchy's packed displacements
    const unsigned* origin;  // [item][tile]
    papof_tensor disp;       // (item, row, column, {dx, dy})
    papof_tensor cost;       // (item, row, column, -)
    int h, w, stride, window, penalty;
    int n_pairs, seq;
};

// (cost, dx^2 + dy^2, dy, dx) in 26 + 18 + 10 + 10 bits, k_match_refine's key: |d| <= 277 + 32 = 309 < 512 per component,
// dx^2 + dy^2 <= 2 * 309^2 = 190962 < 2^18, a cost of at most 15 * 15 * 4 * 255 + 65535 * 618 = 40730130 < 2^26
__device__ __forceinline__ unsigned long long wide_key(unsigned sad, int dx, int dy, int penalty) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const unsigned long long c = sad + (unsigned)(penalty * (ax + ay));
    return (c << 38) | ((unsigned long long)(unsigned)(dx * dx + dy * dy) << 20) | ((unsigned long long)(unsigned)(dy + 512) << 10) |
           (unsigned long long)(unsigned)(dx + 512);
}

// k_match's sibling: the same tile, lanes, LDS tiles (sizes at `window` for `search`), register rows of kG candidates and
// running 64-bit key, with B's window displaced by the tile's origin (ox, oy) -- the candidates are d = o + e, |ex|, |ey| <=
// window -- and with k_match_refine's wider key.  The rows and groups that no cell of the tile may take are skipped with the
// origin added.  Then the lane's own d_h(p): where it lies inside the window it HAS been evaluated from LDS (it is
// admissible, so neither its row nor its group was skipped) and counts once; where it lies outside, the lane reads B's
// (2 P + 1)^2 cells through clamped global addresses -- the values the staged window would hold, were it wider.
template <int P>
__global__ __launch_bounds__(kTX* kTY) void k_match_recentre(const RecentreArgs a, long long tile0, long long item0) {
    extern __shared__ __align__(16) unsigned smem_recentre[];
    constexpr int WN = 2 * P + 1;
    const int s = a.window, h = a.h, w = a.w, ng = groups_of(s);
    const int AW = a_width(P), AH = a_height(P), BW = b_width(P, s), BH = b_height(P, s);
    unsigned* const As = smem_recentre;
    unsigned* const Bs = As + AW * AH;

    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y, tid = ly * kTX + lx;
    const long long ty = (h + kTY - 1) / kTY;
    PAPOF_TILE_ORIGIN(GridTile, tile0, w, int, x0, int, y0);
    const int x = x0 + lx, y = y0 + ly;
    const long long item = item0 + blockIdx.y, cells = (long long)h * w;
    const bool back = item >= a.n_pairs;
    const long long pair = back ? item - a.n_pairs : item;
    const long long first = pair, second = a.seq ? pair + 1 : a.n_pairs + pair;
    const unsigned* const A = a.packed + (back ? second : first) * cells;
    const unsigned* const B = a.packed + (back ? first : second) * cells;
    const unsigned org = a.origin[item * (tx * ty) + tile];  // block-uniform
    const int ox = unpack_dx(org), oy = unpack_dy(org);

    // ---- stage both tiles, every coordinate clamped into the grid; B's around the origin
    for (int c = tid; c < AW * AH; c += kTX * kTY) {
        const int cy = c / AW, cx = c - cy * AW;
        As[c] = A[(long long)clamp_to(y0 - P + cy, h) * w + clamp_to(x0 - P + cx, w)];
    }
    for (int c = tid; c < BW * BH; c += kTX * kTY) {
        const int cy = c / BW, cx = c - cy * BW;
        Bs[c] = B[(long long)clamp_to(y0 - P - s + oy + cy, h) * w + clamp_to(x0 - P - s + ox + cx, w)];
    }
    __syncthreads();

    // ---- the lane's candidates around the origin: rows of dy, groups of kG along dx
    unsigned long long best = ~0ULL;
    for (int eyi = 0; eyi <= 2 * s; eyi++) {
        const int dy = oy + eyi - s;
        if (y0 + kTY - 1 + dy < 0 || y0 + dy >= h) continue;  // inadmissible for every cell of the tile
        const bool row_in = y + dy >= 0 && y + dy < h;
        for (int g = 0; g < ng; g++) {
            const int gx = ox + kG * g - s;  // the group's first dx
            if (x0 + kTX - 1 + gx + kG - 1 < 0 || x0 + gx >= w) continue;  // likewise
            unsigned acc[kG];
#pragma unroll
            for (int j = 0; j < kG; j++) acc[j] = 0;
            for (int wy = 0; wy < WN; wy++) {
                const unsigned* const ar = As + (ly + wy) * AW + lx;
                const unsigned* const br = Bs + (ly + wy + eyi) * BW + lx + kG * g;
                unsigned av[WN], bv[WN + kG - 1];
#pragma unroll
                for (int k = 0; k < WN; k++) av[k] = ar[k];
#pragma unroll
                for (int k = 0; k < WN + kG - 1; k++) bv[k] = br[k];
#pragma unroll
                for (int k = 0; k < WN; k++)
#pragma unroll
                    for (int j = 0; j < kG; j++) acc[j] = __builtin_amdgcn_sad_u8(av[k], bv[k + j], acc[j]);
            }
#pragma unroll
            for (int j = 0; j < kG; j++) {
                const int dx = gx + j;
                const bool ok = kG * g + j <= 2 * s && row_in && x + dx >= 0 && x + dx < w;
                const unsigned long long key = wide_key(acc[j], dx, dy, a.penalty);
                best = ok && key < best ? key : best;
            }
        }
    }
    if (x >= w || y >= h) return;

    // ---- the hierarchy's own vector, where the window has not held it
    const unsigned own = a.dh[item * cells + (long long)y * w + x];
    const int hx = unpack_dx(own), hy = unpack_dy(own);
    if (hx - ox < -s || hx - ox > s || hy - oy < -s || hy - oy > s) {
        unsigned sad = 0;
#pragma unroll 1
        for (int wy = 0; wy < WN; wy++) {  // (rolled: the rare path must not set the kernel's register count)
            const unsigned* const ar = As + (ly + wy) * AW + lx;
            const unsigned* const br = B + (long long)clamp_to(y - P + wy + hy, h) * w;
#pragma unroll
            for (int k = 0; k < WN; k++) sad = __builtin_amdgcn_sad_u8(ar[k], br[clamp_to(x - P + k + hx, w)], sad);
        }
        const unsigned long long key = wide_key(sad, hx, hy, a.penalty);
        best = key < best ? key : best;
    }
    const int bdx = (int)(best & 1023) - 512, bdy = (int)((best >> 10) & 1023) - 512;
    const long long od = PAPOF_AT(a.disp, item, (long long)y, (long long)x);
    store(a.disp, od, (double)(a.stride * bdx));
    store(a.disp, od + a.disp.stride[3], (double)(a.stride * bdy));
    store(a.cost, PAPOF_AT(a.cost, item, (long long)y, (long long)x),
          (double)(best >> 38));
}

template <int P>
int launch_recentre(hipStream_t st, const RecentreArgs& a, long long items) {
    const size_t lds = (size_t)lds_bytes(P, a.window);
    return launch_grid<GridTile>(a.h, a.w, items, st, lds, k_match_recentre<P>, a);
}

bool valid_hier(int height, int width, int stride, int levels) {
    if (levels < 1 || levels > kMaxLevels || !valid_frame_size(height, width, stride)) return false;
    const int top = stride << (levels - 1);
    return top <= kMaxTopStride && height >= top && width >= top;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_match_workspace(int n_pairs, int sequence, int height, int width, int stride) {
    if (n_pairs < 1 || height < 1 || width < 1 || !valid_frame_size(height, width, stride)) return -1;
    const long long frames = sequence ? (long long)n_pairs + 1 : 2LL * n_pairs;
    const long long per = 4LL * (height / stride) * (width / stride);
    if (frames > (1LL << 62) / per) return -1;
    return frames * per;
}

extern "C" int papof_match_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                  const papof_tensor* frames2, int height, int width, int c, int stride, int patch, int search,
                                  int penalty, int both, const papof_tensor* disp, const papof_tensor* cost, void* workspace,
                                  long long workspace_bytes, void* stream) {
    if (!h) return PAPOF_EINVAL;
    const long long need = papof_match_workspace(n_pairs, sequence, height, width, stride);
    if (need < 0 || c < 1 || c > 4 || patch < 1 || patch > kMaxPatch || search < 1 || search > kMaxSearch || penalty < 0 ||
        penalty > kMaxPenalty)
        return PAPOF_EINVAL;
    if (!in_frames(frames) || (!sequence && !in_frames(frames2)))
        return PAPOF_EINVAL;
    if (!out_flow(disp) || !described(cost, kFlowDtypes, {0, 1, 2}, true)) return PAPOF_EINVAL;
    if (!workspace || (reinterpret_cast<std::uintptr_t>(workspace) & 3) || workspace_bytes < need) return PAPOF_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PAPOF_HIP(hipSetDevice(h->device));

    const int ch = height / stride, cw = width / stride;
    const long long cells = (long long)ch * cw, blocks = (cells + 255) / 256;
    PrepArgs p{};
    p.h = ch;
    p.w = cw;
    p.C = c;
    p.stride = stride;
    const long long n_first = sequence ? (long long)n_pairs + 1 : n_pairs;
    for (int k = 0; k < (sequence ? 1 : 2); k++) {
        p.in = k == 0 ? *frames : *frames2;
        p.packed = static_cast<unsigned*>(workspace) + (k == 0 ? 0 : n_first * cells);
        PAPOF_TRY(launch_tiles(blocks, k == 0 ? n_first : n_pairs, [&](dim3 grid, long long c0, long long f0) {
            hipLaunchKernelGGL(k_match_prepare, grid, dim3(256), 0, st, p, c0, f0);
        }));
    }

    MatchArgs a{};
    a.packed = static_cast<const unsigned*>(workspace);
    a.disp = *disp;
    a.cost = *cost;
    a.h = ch;
    a.w = cw;
    a.stride = stride;
    a.search = search;
    a.penalty = penalty;
    a.n_pairs = n_pairs;
    a.seq = sequence ? 1 : 0;
    const long long items = both ? 2LL * n_pairs : n_pairs;
    switch (patch) {
        case 1: return launch_match<1>(st, a, items);
        case 2: return launch_match<2>(st, a, items);
        case 3: return launch_match<3>(st, a, items);
        case 4: return launch_match<4>(st, a, items);
        case 5: return launch_match<5>(st, a, items);
        case 6: return launch_match<6>(st, a, items);
        default: return launch_match<7>(st, a, items);
    }
}

extern "C" long long papof_match_hier_workspace(int n_pairs, int sequence, int height, int width, int stride, int levels) {
    if (n_pairs < 1 || height < 1 || width < 1 || !valid_hier(height, width, stride, levels)) return -1;
    const long long frames = sequence ? (long long)n_pairs + 1 : 2LL * n_pairs;
    long long dwords = 0;
    for (int l = 0; l < levels; l++) {
        const long long cells = (long long)(height / (stride << l)) * (width / (stride << l));
        const long long per = frames + (l > 0 ? 2LL * n_pairs : 0);  // the frames; above level 0 a displacement per item too
        if (per > ((1LL << 60) - dwords) / cells) return -1;
        dwords += per * cells;
    }
    return 4 * dwords;
}

// papof_match_hier_tensor; with `field0` its level 0 leaves packed displacements there ([item][h_0][w_0]) instead of disp and
// cost (levels >= 2: the re-centred search's d_h)
static int match_hier(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2, int height,
                      int width, int c, int stride, int levels, int patch, int search, int refine, int penalty, int both,
                      const papof_tensor* disp, const papof_tensor* cost, void* workspace, long long workspace_bytes, void* stream,
                      unsigned* field0) {
    if (!h || refine < 1 || refine > kMaxRefine) return PAPOF_EINVAL;
    const long long need = papof_match_hier_workspace(n_pairs, sequence, height, width, stride, levels);
    if (need < 0) return PAPOF_EINVAL;
    if (levels == 1)
        return papof_match_tensor(h, n_pairs, sequence, frames, frames2, height, width, c, stride, patch, search, penalty, both, disp,
                                  cost, workspace, workspace_bytes, stream);
    if (c < 1 || c > 4 || patch < 1 || patch > kMaxPatch || search < 1 || search > kMaxSearch || penalty < 0 || penalty > kMaxPenalty)
        return PAPOF_EINVAL;
    if (!in_frames(frames) || (!sequence && !in_frames(frames2)))
        return PAPOF_EINVAL;
    if (!out_flow(disp) || !described(cost, kFlowDtypes, {0, 1, 2}, true)) return PAPOF_EINVAL;
    if (!workspace || (reinterpret_cast<std::uintptr_t>(workspace) & 3) || workspace_bytes < need) return PAPOF_EINVAL;
    const char* const env = std::getenv("PAPOF_MATCH_STAGED");
    const int staged = !(env && std::strcmp(env, "0") == 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PAPOF_HIP(hipSetDevice(h->device));

    // the workspace: the packed frames of levels 0 .. levels - 1, then the packed displacements of levels 1 .. levels - 1
    const long long n_frames = sequence ? (long long)n_pairs + 1 : 2LL * n_pairs, items = both ? 2LL * n_pairs : n_pairs;
    unsigned* packed[kMaxLevels];
    unsigned* field[kMaxLevels] = {};
    unsigned* at = static_cast<unsigned*>(workspace);
    for (int l = 0; l < levels; l++) {
        packed[l] = at;
        at += n_frames * (height / (stride << l)) * (width / (stride << l));
    }
    for (int l = 1; l < levels; l++) {
        field[l] = at;
        at += 2LL * n_pairs * (height / (stride << l)) * (width / (stride << l));
    }
    for (int l = 0; l < levels; l++)
        PAPOF_TRY(launch_prepare(st, n_pairs, sequence, frames, frames2, height, width, c, stride << l, packed[l]));

    const int top = levels - 1;
    MatchArgs m{};
    m.packed = packed[top];
    m.h = height / (stride << top);
    m.w = width / (stride << top);
    m.stride = stride << top;
    m.search = search;
    m.penalty = penalty;
    m.n_pairs = n_pairs;
    m.seq = sequence ? 1 : 0;
    m.out = field[top];
    PAPOF_TRY(launch_match_packed(st, m, items, patch));

    for (int l = top - 1; l >= 0; l--) {
        RefineArgs a{};
        a.packed = packed[l];
        a.parent = field[l + 1];
        a.out = l == 0 ? field0 : field[l];
        a.disp = *disp;
        a.cost = *cost;
        a.h = height / (stride << l);
        a.w = width / (stride << l);
        a.h1 = height / (stride << (l + 1));
        a.w1 = width / (stride << (l + 1));
        a.stride = stride;
        a.refine = refine;
        a.penalty = penalty;
        a.n_pairs = n_pairs;
        a.seq = sequence ? 1 : 0;
        a.last = l == 0 && !field0;
        a.staged = staged;
        int rc;
        switch (patch) {
            case 1: rc = launch_refine<1>(st, a, items); break;
            case 2: rc = launch_refine<2>(st, a, items); break;
            case 3: rc = launch_refine<3>(st, a, items); break;
            case 4: rc = launch_refine<4>(st, a, items); break;
            case 5: rc = launch_refine<5>(st, a, items); break;
            case 6: rc = launch_refine<6>(st, a, items); break;
            default: rc = launch_refine<7>(st, a, items); break;
        }
        PAPOF_TRY(rc);
    }
    return PAPOF_OK;
}

extern "C" int papof_match_hier_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                       const papof_tensor* frames2, int height, int width, int c, int stride, int levels, int patch,
                                       int search, int refine, int penalty, int both, const papof_tensor* disp,
                                       const papof_tensor* cost, void* workspace, long long workspace_bytes, void* stream) {
    return match_hier(h, n_pairs, sequence, frames, frames2, height, width, c, stride, levels, patch, search, refine, penalty, both,
                      disp, cost, workspace, workspace_bytes, stream, nullptr);
}

extern "C" long long papof_match_recentre_workspace(int n_pairs, int sequence, int height, int width, int stride, int levels) {
    const long long hier = papof_match_hier_workspace(n_pairs, sequence, height, width, stride, levels);
    if (hier < 0 || levels < 2) return -1;
    const long long ch = height / stride, cw = width / stride;
    const long long per = ch * cw + GridTile::count(ch, cw);  // d_h and the origins of one item
    if (2LL * n_pairs > ((1LL << 60) - hier / 4) / per) return -1;
    return hier + 4 * 2LL * n_pairs * per;
}

extern "C" int papof_match_recentre_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                           const papof_tensor* frames2, int height, int width, int c, int stride, int levels,
                                           int patch, int search, int refine, int window, int penalty, int both,
                                           const papof_tensor* disp, const papof_tensor* cost, void* workspace,
                                           long long workspace_bytes, void* stream) {
    if (!h || levels < 2 || window < 1 || window > kMaxWindow) return PAPOF_EINVAL;
    const long long need = papof_match_recentre_workspace(n_pairs, sequence, height, width, stride, levels);
    if (need < 0 || workspace_bytes < need) return PAPOF_EINVAL;
    // the workspace: the hierarchical call's, then d_h [item][h_0][w_0], then the origins [item][tile], 2 n_pairs items each
    const long long hier = papof_match_hier_workspace(n_pairs, sequence, height, width, stride, levels);
    const int ch = height / stride, cw = width / stride;
    unsigned* const dh = static_cast<unsigned*>(workspace) + hier / 4;
    unsigned* const origin = dh + 2LL * n_pairs * ch * cw;
    // (every remaining refusal is the hierarchical call's, made before it enqueues anything)
    PAPOF_TRY(match_hier(h, n_pairs, sequence, frames, frames2, height, width, c, stride, levels, patch, search, refine, penalty, both,
                         disp, cost, workspace, workspace_bytes, stream, dh));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long items = both ? 2LL * n_pairs : n_pairs;
    OriginArgs o{};
    o.dh = dh;
    o.origin = origin;
    o.h = ch;
    o.w = cw;
    PAPOF_TRY(launch_grid<GridTile>(ch, cw, items, st, 0, k_match_origin, o));
    RecentreArgs a{};
    a.packed = static_cast<const unsigned*>(workspace);  // level 0's frames come first
    a.dh = dh;
    a.origin = origin;
    a.disp = *disp;
    a.cost = *cost;
    a.h = ch;
    a.w = cw;
    a.stride = stride;
    a.window = window;
    a.penalty = penalty;
    a.n_pairs = n_pairs;
    a.seq = sequence ? 1 : 0;
    switch (patch) {
        case 1: return launch_recentre<1>(st, a, items);
        case 2: return launch_recentre<2>(st, a, items);
        case 3: return launch_recentre<3>(st, a, items);
        case 4: return launch_recentre<4>(st, a, items);
        case 5: return launch_recentre<5>(st, a, items);
        case 6: return launch_recentre<6>(st, a, items);
        default: return launch_recentre<7>(st, a, items);
    }
}

extern "C" int papof_match_densify_tensor(papof_handle* h, int n, int height, int width, int stride, const papof_tensor* disp,
                                          const papof_tensor* disp_rev, const papof_tensor* cost, int tol, double max_cost,
                                          const papof_tensor* flow, const papof_tensor* mask, void* stream) {
    if (!h || n < 1 || height < 1 || width < 1 || !valid_frame_size(height, width, stride) || tol < 0 || tol > 2 * kMaxSearch ||
        std::isnan(max_cost))
        return PAPOF_EINVAL;
    if (!in_flow_pair(disp, disp_rev)) return PAPOF_EINVAL;
    if (max_cost >= 0 && !described(cost, kFlowDtypes, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!described(flow, {PAPOF_DTYPE_F64}, {0, 1, 2, 3}, true) || !described(mask, {PAPOF_DTYPE_U8}, {0, 1, 2}, true))
        return PAPOF_EINVAL;
    DensifyArgs a{};
    a.disp = *disp;
    a.rev = *disp_rev;
    if (max_cost >= 0) a.cost = *cost;
    a.flow = *flow;
    a.mask = *mask;
    a.max_cost = max_cost >= 0 ? max_cost : -1.0;
    a.H = height;
    a.W = width;
    a.h = height / stride;
    a.w = width / stride;
    a.stride = stride;
    a.tol = tol;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PAPOF_HIP(hipSetDevice(h->device));
    const long long blocks = ((long long)height * width + 255) / 256;
    return launch_tiles(blocks, n, [&](dim3 grid, long long p0, long long i0) {
        hipLaunchKernelGGL(k_match_densify, grid, dim3(256), 0, st, a, p0, i0);
    });
}
