// papteam_opticalflow_amd/csrc/cells.h -- what the kernels that reduce frames to integer counts per cell share (telecine.hip:
// k_field_metrics, shots.hip: k_cell_hist): the cell, the quantisation of an element and the wave's load of a packed uint8
// row.  One wave per cell of up to kMaxCellRows x kCellW pixels, lane = column; a block is kCellsX horizontally adjacent cells.
#pragma once
#include "sampler.h"

#include <cmath>

namespace papof {

namespace {

constexpr int kCellW = 64;     // columns of a cell: one wave
constexpr int kCellsX = 4;     // cells of a block
using CellTile = Tile<kCellsX, 1, kCellW, kCellsX>;  // over the Gy x Gx plane of cells: a tile is kCellsX cells of one row
constexpr int kMaxCellRows = 64;
constexpr int kMaxQ = 65535;
constexpr int kMaxC = 4;

// the quantised value of an element: 257 b of a byte; of a float 0 for a NaN, else clamp(rint(65535.0 v), 0, 65535) in fp64
template <int FD>
__device__ __forceinline__ int load_q(const papof_tensor& t, long long o) {
    if (FD == PAPOF_DTYPE_U8) return 257 * (int)static_cast<const unsigned char*>(t.data)[o];
    const double v = FD == PAPOF_DTYPE_F32 ? (double)static_cast<const float*>(t.data)[o] : static_cast<const double*>(t.data)[o];
    return (int)fmin(fmax(rint(65535.0 * v), 0.0), (double)kMaxQ);  // (fmax: NaN -> 0)
}

// The C bytes of pixel `lane` of a packed uint8 row segment (channels adjacent, pixels adjacent) that starts at p and has
// n bytes, 1 <= n <= 64 C, as one word, channel k in byte k -- p and n wave-uniform, called by ALL lanes of the wave.  The
// wave loads the segment once as aligned dwords (lane i the i-th; the last one, which is the 65th of a misaligned segment
// of four channels, by every lane) and each lane takes the two dwords that hold its pixel from the lanes that loaded them
// (ds_bpermute): one load and one register per row, where a lane that gathers its bytes itself has C of each.  (By itself
// this measured no faster than the gathers; it is what keeps k_field_metrics's twelve rows in flight within 76 VGPRs.)  The
// aligned words that hold the segment's first and last byte are read whole: up to 3 bytes on either side of it, of the
// same 4-byte word and therefore of the same page.  A lane beyond the segment gets bytes that mean nothing.
__device__ __forceinline__ unsigned packed_pixel(const unsigned char* p, int n, int lane, int C) {
    const unsigned mis = (unsigned)(reinterpret_cast<unsigned long long>(p) & 3);
    const unsigned* q = reinterpret_cast<const unsigned*>(p - mis);
    const int ndw = (int)((mis + n + 3) >> 2);  // <= 65
    const unsigned d = q[lane < ndw ? lane : ndw - 1];  // (no branch around a load: the rows' loads are issued together)
    const unsigned e = q[ndw - 1];                      // the 65th where there is one (one address for the wave)
    const unsigned o = mis + lane * C;          // <= 3 + 63 * 4: its first dword is one of the 64
    const int i = (int)(o >> 2);
    const unsigned lo = __shfl(d, i), up = __shfl(d, (i + 1) & 63);
    return __builtin_amdgcn_alignbyte(i + 1 == 64 ? e : up, lo, o & 3);
}

}  // namespace

}  // namespace papof
