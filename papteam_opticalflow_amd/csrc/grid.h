// papteam_opticalflow_amd/csrc/grid.h -- the (tile, item) grid of the device-tensor video kernels, stated once: how a plane
// of H x W pixels is cut into tiles, how a block finds its tile, how a grid beyond the bounds of one launch is split, and
// the choice of a kernel's instance by the dtype of its frame tensors.
//
// What it guarantees:
//   - blockIdx.x is a tile and blockIdx.y an item (a frame, pair, slot, link ...).  A launch carries the indices of its
//     first tile and item, `tile0` and `item0`; the tile index tile0 + blockIdx.x is 64-bit and is formed before any use, so
//     the second launch of a split grid decodes as the first does.  The item is item0 + blockIdx.y, which the kernel adds.
//   - tiles are numbered in row-major order over ceil(W / TX) columns; items are outermost in the order of launches.
//   - the host's count of tiles and the device's decode come from the same Tile<TX, TY>, so they cannot disagree.
//
// A new kernel takes (args, long long tile0, long long item0), names its tile shape `using T = Tile<TX, TY>;`, starts with
// `PAPOF_TILE_PIXEL(T, tile0, W, int, x, long long, r); if (x >= W || r >= H) return;` (one lane per pixel; after the LUT's
// barrier, sampler.h: stage_u8_lut) or with PAPOF_TILE_ORIGIN (a block that walks its tile), and is launched with
// launch_grid<T>.
#pragma once

#include "common.h"

#include <algorithm>
#include <type_traits>

namespace papof {

namespace {

constexpr long long kMaxTiles = 0x7fffffffLL;  // gridDim.x
constexpr long long kMaxFrames = 65535;        // gridDim.y

// A (tile, frame) grid of `tiles` x `frames` blocks in launches that fit the grid's bounds, frames outermost: launch(grid,
// tile0, frame0) enqueues one of them, whose blockIdx.x is tile tile0 + x and blockIdx.y frame frame0 + y.
template <typename L>
int launch_tiles(long long tiles, long long frames, L launch) {
    for (long long f0 = 0; f0 < frames; f0 += kMaxFrames)
        for (long long t0 = 0; t0 < tiles; t0 += kMaxTiles) {
            launch(dim3((unsigned)std::min(kMaxTiles, tiles - t0), (unsigned)std::min(kMaxFrames, frames - f0)), t0, f0);
            PAPOF_HIP(hipGetLastError());
        }
    return PAPOF_OK;
}

// The tiles of tx x ty pixels that cover an H x W plane.
inline long long tile_count(long long H, long long W, long long tx, long long ty) { return ((W + tx - 1) / tx) * ((H + ty - 1) / ty); }

// A tile of TX x TY pixels (or cells, or rows of a strip: whatever the plane is made of), worked on by a block of BX x BY
// lanes -- one lane per pixel unless stated otherwise.
template <int TX, int TY, int BX = TX, int BY = TY>
struct Tile {
    static long long count(long long H, long long W) { return tile_count(H, W, TX, TY); }
    static constexpr int kX = TX, kY = TY;
    static dim3 block() { return dim3(BX, BY); }
};

// The device's side of a Tile T: which tile this block works on, and which pixel this lane.
//   PAPOF_TILE_ORIGIN(T, tile0, W, XT, x0, RT, r0)  declares `const XT x0` and `const RT r0`, the first column and row of tile
//                                                   tile0 + blockIdx.x of a plane W wide;
//   PAPOF_TILE_PIXEL(T, tile0, W, XT, x, RT, r)     declares `const XT x` and `const RT r`, the origin plus threadIdx: the
//                                                   kernel goes on with `if (x >= W || r >= H) return;`.
// XT and RT are the coordinate types of the kernel (int where it indexes within a plane, long long where it forms offsets
// directly).  Both also leave `tx` (tiles per row) and `tile` (this block's tile, 64-bit) in scope.
//
// Why macros, where member functions of Tile would read better: functions were tried first (origin(), and a pixel() that
// returned the bounds test).  pixel()'s result reached the optimiser as one merged condition where the kernels have two
// branches, and changed their code.  origin() compiled to the same instructions, but the saved assembly, which this project
// compares byte for byte across a refactor (profiles/tile_grid_isa.txt), also names IR blocks in comments (`; %Flow81`) with
// a counter that every repeated value name in the kernel's own body advances; arithmetic moved into a function no longer
// advances it, so every such comment of a converted kernel changed.  Text expanded in place is the one form that leaves
// the file as it was.  DESIGN.md section 41 lists turning them into functions as a follow-up.
#define PAPOF_TILE_ORIGIN(T, tile0, W, XT, x0_, RT, r0_)                         \
    const long long tx = ((W) + T::kX - 1) / T::kX, tile = (tile0) + blockIdx.x; \
    const XT x0_ = (XT)(tile % tx) * T::kX;                                      \
    const RT r0_ = (RT)(tile / tx) * T::kY
#define PAPOF_TILE_PIXEL(T, tile0, W, XT, x_, RT, r_)                            \
    const long long tx = ((W) + T::kX - 1) / T::kX, tile = (tile0) + blockIdx.x; \
    const XT x_ = (XT)(tile % tx) * T::kX + (XT)threadIdx.x;                     \
    const RT r_ = (RT)(tile / tx) * T::kY + (RT)threadIdx.y

// launch_tiles over the tiles T of an H x W plane and `items` items: kernel(args..., tile0, item0) on blocks of T::block().
template <typename T, typename K, typename... A>
int launch_grid(long long H, long long W, long long items, hipStream_t st, size_t lds, K kernel, const A&... args) {
    return launch_tiles(T::count(H, W), items, [&](dim3 grid, long long t0, long long i0) {
        hipLaunchKernelGGL(kernel, grid, T::block(), lds, st, args..., t0, i0);
    });
}

// The kernel instance for the dtype of the frame tensors: pick(Dtype<FD>{}) returns the instance whose FD template parameter
// is `dtype`, e.g. by_dtype(d, [](auto fd) { return k_warp<fd(), true>; }).  by_frame_dtype also knows FD = -1 (the frame
// tensors differ in dtype: read from each descriptor, sampler.h: load_frame).  The instances are named in the order float32,
// float64, uint8 (float64, -1, float32, uint8): that order is the order of the kernels in the code object, which stays as it
// was when every launcher wrote the selection out.
template <int D>
using Dtype = std::integral_constant<int, D>;

template <typename P>
auto by_dtype(int dtype, P pick) {
    return dtype == PAPOF_DTYPE_F32  ? pick(Dtype<PAPOF_DTYPE_F32>{})
           : dtype != PAPOF_DTYPE_U8 ? pick(Dtype<PAPOF_DTYPE_F64>{})
                                     : pick(Dtype<PAPOF_DTYPE_U8>{});
}

template <typename P>
auto by_frame_dtype(int dtype, P pick) {
    return dtype == PAPOF_DTYPE_F64                               ? pick(Dtype<PAPOF_DTYPE_F64>{})
           : dtype != PAPOF_DTYPE_F32 && dtype != PAPOF_DTYPE_U8 ? pick(Dtype<-1>{})
           : dtype == PAPOF_DTYPE_F32                             ? pick(Dtype<PAPOF_DTYPE_F32>{})
                                                                  : pick(Dtype<PAPOF_DTYPE_U8>{});
}

}  // namespace

}  // namespace papof
