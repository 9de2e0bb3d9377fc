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
// k_mosaic.  A block is a 64 x TY tile of output pixels of one output (grid.h's grid of tiles and outputs), a lane
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
//
// papof_mosaic_blend_tensor is the same kernel over BlendArgs: every live sample is multiplied by the gain of its slot, and
// PAPOF_MOSAIC_FEATHER weighs it by the distance of (X, Y) to the frame's border.  The instances over MosaicArgs (the gain
// is the constant 1.0 there) are what papof_mosaic_tensor launches, and this call too without gains.
//
// Every rule below is chosen at compile time by the argument type, and each is stated once: phase 1 is cull_slots with one
// keep-test per rule (affine_keep, projective_keep, ray_keep, mesh_keep), a pixel's point is slot_point, and whether that
// point is live (inside the frame, no masked tap) is live_taps.  Both kernels call these.
//
// papof_mosaic_projective_tensor and papof_mosaic_overlap_projective_tensor are the same two kernels over ProjArgs: the
// matrices are 3 x 3 and a pixel's point is (X, Y) = (Nx / D, Ny / D), live only where D > 0 (include/papof.h: projective
// sampling).
//   Culling under the projective rule (projective_keep, quotients_keep).  Canvas coordinates are >= 0.  D, Nx and Ny are each
//   (a x + b r) + c: every step is monotone in x and in r under rounding, overflow to +-inf included.  A NaN at a pixel
//   arises in one of two ways.  (i) inf - inf in a x + b r, or that sum meeting an infinite c of the other sign: |a x| and
//   |b r| grow with x and r, so the same infinities meet at the tile's far corner (xb, rb), which is NaN too.  (ii) 0 * inf:
//   an infinite entry a or b (the last row's; (1) below removes the others) times x = 0 or r = 0 -- that pixel lies on the
//   tile's edge x = xa = 0 or r = ra = 0, and the product is the same NaN at the corner of that edge.  So a NaN at a pixel
//   means a NaN at a corner: when no corner value is NaN, no pixel's is, and the min and max over the four corners bound
//   every pixel's D, Nx and Ny.
//     (1) An entry of the first two rows that is not finite makes Nx or Ny +-inf or NaN at every pixel, and a quotient of it
//         +-inf or NaN: live nowhere, dropped.  (An infinite entry of the LAST row can leave X = Nx / inf = 0 inside the
//         frame: such a matrix goes through the corner test like any other.)
//     (2) A NaN corner value proves nothing: kept.
//     (3) D_max <= 0: D > 0 at no pixel: dropped.
//     (4) D_min <= 0 < D_max: the horizon may cross the tile: kept.
//     (5) 0 < D_min: correctly rounded division is monotone in each operand -- N / D does not decrease with N, and for D > 0
//         does not increase with D when N >= 0 and does not decrease with D when N < 0.  So for every pixel
//         fl(Nx / D) <= fl(Nx_max / D) <= max(fl(Nx_max / D_min), fl(Nx_max / D_max)), and likewise
//         fl(Nx / D) >= min(fl(Nx_min / D_min), fl(Nx_min / D_max)).  When both upper quotients are < -1, or both lower ones
//         > W - 1 + 1 (the affine box's one-pixel margin), X is outside [0, W - 1] at every pixel: dropped; the same for Y and
//         H.  A quotient inf / inf is NaN, every comparison with it false: kept.
//   Dropping changes no byte, as in the affine case.  The interval is looser than the affine corner box -- it pairs the
//   extreme numerator with the extreme denominator, which need not meet at one pixel: DESIGN.md section 27 has the share of
//   slots it keeps.
//
// papof_mosaic_ray_tensor and papof_mosaic_overlap_ray_tensor are the same two kernels over RayArgs: the canvas pixel is a
// direction d = (u_x c_r, s_r, w_x c_r) read from two tables (include/papof.h: ray sampling), and the 3 x 3 matrix is applied
// to it: (D, Nx, Ny) = rows 2, 0, 1 of m times d, each (a dx + b dy) + c dz.  The ray is computed once per pixel, outside the
// walk.
//   Culling under the ray rule (ray_box, ray_keep, quotients_keep).  The corners of a tile bound nothing here (sin is not
//   monotone over 64 columns), so the block bounds the tile's rays by intervals, from the tables themselves: lane x of a wave
//   reads (u, w) of its column and a butterfly of min and max reduces them over the tile's columns; (s, c) are reduced over its
//   <= 4 rows.
//   These min and max hand a NaN on (nan_min, nan_max; fmin and fmax would drop it).  Only pixels whose values are numbers
//   matter: a live pixel has D > 0 and X, Y inside, so none of dx, dz, the nine products, D, Nx, Ny is NaN there (a NaN
//   operand makes every later step NaN).  Call such a pixel clean.
//     (a) dx = fl(u c) with u in [u_lo, u_hi], c in [c_lo, c_hi].  For fixed c, fl(u c) is monotone in u (rounding is
//         monotone, overflow to +-inf included), and for fixed u monotone in c; so a clean pixel's dx lies between the min and
//         the max of the four endpoint products -- unless one of those is NaN (0 * inf: an infinite table entry against a
//         zero one), which makes the bound NaN.  The same for dz; dy = s needs no product.
//     (b) A term fl(m d) with d in [d_lo, d_hi] is monotone in d, so a clean pixel's term lies between the smaller and the
//         larger of fl(m d_lo), fl(m d_hi) -- or one of them is NaN (0 * inf again: an infinite entry of the last row against
//         a bound that is 0, or a zero entry against an infinite bound) and so is the bound.
//     (c) fl(fl(t0 + t1) + t2) is monotone in each term; the sum of the three lower (upper) term bounds is a lower (upper)
//         bound of a clean pixel's D, Nx, Ny, or NaN (inf - inf: the lower bounds hold -inf and +inf at once).
//   So when none of the six bounds is NaN they bound D, Nx and Ny at every clean pixel, and rules (1) to (5) above apply word
//   for word with them in place of the corner extremes: (1) an entry of the first two rows that is not finite makes Nx or Ny
//   +-inf or NaN at every pixel (m d is +-inf, or NaN where d = 0); (2) a NaN bound proves nothing: kept; (3), (4), (5) as
//   there.  The caller is never trusted for the ranges: they are read from the very entries the pixels read.
//   PAPOF_MOSAIC_CULL=0 skips the reduction and the test.  The intervals ignore that u and w (sin and cos of one angle)
//   move together, so they are looser than the projective corner test: DESIGN.md section 28 has the share of slots kept.
//
// papof_mosaic_mesh_tensor is k_mosaic over MeshMosaicArgs: BlendArgs whose affine point (X0, Y0) is moved by the displacement
// (dx, dy) of the SLOT's own table, looked up at (X0, Y0) by papof_warp_mesh_tensor's rule (include/papof.h: the mosaic under
// the mesh rule) -- the borders of a mesh-stabilized frame filled from its neighbours, each registered by its own table.  The
// four entries per (pixel, slot) are read through global addresses: an output at fill radius 15 has 31 tables (143 KB at
// 17 x 17), too many to stage, few enough to stay in the cache.
//   Culling under the mesh rule (k_mesh_bounds, mesh_widening, mesh_keep, mesh_point).  The affine corner box alone is wrong
//   here: a table can carry a source into a tile that its matrix misses.  k_mesh_bounds, ahead of k_mosaic on the stream, one
//   wave per slot, reduces the slot's table to lo <= t.dx <= hi over its entries t, and the same for dy, with min and max that
//   hand a NaN on (nan_min, nan_max).  Only pixels whose X and Y are numbers matter -- a NaN is live nowhere --: call such a
//   pixel clean; none of its weights, terms, partial sums, X0 or Y0 is a NaN (a NaN operand makes every later step NaN).
//     (a) A weight w = fl(|a - fx| * |b - fy|), a, b in {0, 1}: gx is clamped to [0, GW] and the cell index to [0, GW - 1],
//         so fx = gx - j lies in [0, 1] (exactly: both are integers or gx < 2^53), |a - fx| in [0, 1], and the rounded product
//         of two numbers of [0, 1] lies in [0, 1].
//     (b) A term fl(t * w) with lo <= t <= hi and w in [0, 1]: t * w lies between 0 and t, hence in [l, u] with l = min(lo, 0),
//         u = max(hi, 0); l and u are doubles and rounding is monotone, so fl(t * w) lies in [l, u] too (an infinite entry
//         against w = 0 is a NaN term: not a clean pixel).
//     (c) dx = fl(fl(fl(fl(0 + t0) + t1) + t2) + t3) over four such terms.  fl(p + q) is monotone in p and in q, so by
//         induction over the partial sums dx >= ((l + l) + l) + l =: L and dx <= ((u + u) + u) + u =: U, both evaluated in
//         fp64 in the order written (fl(0 + t0) = t0 >= l): the very chain of additions at its extreme terms, no epsilon.
//     (d) X = fl(X0 + dx) is monotone in both operands, and over a tile X0 takes its extremes at the corners (phase 1's
//         affine argument): at every clean pixel fl(X0_min + L) <= X <= fl(X0_max + U).
//   Phase 1 drops a slot when fl(c + U) < -1 at all four corner values c of X0, or fl(c + L) > W - 1 + 1 at all four, or the
//   same for Y with H (the affine box's one-pixel margin, kept): by (d) X or Y is then outside the frame at every clean pixel,
//   the slot is live at no pixel of the tile, and dropping it changes no byte.  A NaN bound (a NaN entry, or +inf and -inf
//   meeting in L + ... ) or a NaN corner makes every comparison false: kept.  A matrix entry that is not finite makes X0 or Y0
//   +-inf or NaN at every pixel and X or Y with it (inf + dx is inf or NaN): dropped as before.
//   The walk uses the same bound per pixel, before the table is read: fl(X0 + U) < 0 or fl(X0 + L) > W - 1 (or the same for
//   Y) means, by (c) and the monotone sum, X < 0 or X > W - 1 or a pixel that is not clean: not live, skipped without a load.
//   The slot's index is uniform, so its four bounds are scalar loads.  With `count` every slot is walked at every pixel, and
//   most of a neighbour's pixels are far outside.  PAPOF_MOSAIC_CULL=0 skips k_mesh_bounds, the bounds' use and both tests.
//
// k_mosaic_overlap (papof_mosaic_overlap_tensor).  A block is a 64 x 2 tile of SAMPLED pixels (every step-th column and
// row).  Phases 1 and 2 as above, each lane writing the fixed-point luminance q of its live slots to LDS [slot][pixel] and
// the 64-bit set of them.  Then the roles turn: lane j is source j (64 / NS pixels side by side where NS < 64), wave w owns
// the rows i = w (mod 2) of an LDS table [i][lane], and for every pixel and every live i a lane whose own bit j is set adds
// q[i] and 1 into its column of row i -- no LDS atomics, no conflicts.  The rows that were touched go out as 64-bit integer
// atomic adds, one row of contiguous addresses per instruction.  Integer sums: the same bits in any order.  DESIGN.md
// section 26 has the instances and what was measured.
#include "sampler.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace papof {

namespace {

constexpr int kMosTX = 64;     // tile width: one wave per tile row
template <int TY>
using MosTile = Tile<kMosTX, TY>;
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

struct BlendArgs : MosaicArgs {
    papof_tensor gains;  // float32 / float64 (out, k); data NULL: every gain is 1
};

struct ProjArgs : BlendArgs {};  // mat is (out, k, row, column): 3 x 3, the projective rule of include/papof.h

template <typename A>
constexpr bool kProjective = std::is_same<A, ProjArgs>::value;

struct RayArgs : BlendArgs {  // mat is 3 x 3 as ProjArgs', applied to the ray of the pixel: the ray rule of include/papof.h
    papof_tensor cols;        // float32 / float64 (column, {u, w})
    papof_tensor rows;        // float32 / float64 (row, {s, c})
};

template <typename A>
constexpr bool kRay = std::is_same<A, RayArgs>::value;

struct MeshMosaicArgs : BlendArgs {  // mat is 2 x 3 as BlendArgs'; the point is moved by the table of its slot
    papof_tensor mesh;               // float64 (slot, vertex row, vertex column, {dx, dy}), slot = out * n_src + k
    const double* bounds;            // (slot, {dx lo, dx hi, dy lo, dy hi}): k_mesh_bounds'; read only where cull
    int GH, GW;                      // the cells of the mesh, on the FRAMES' H x W
};

template <typename A>
constexpr bool kMesh = std::is_same<A, MeshMosaicArgs>::value;

__device__ __forceinline__ double slot_gain(const MosaicArgs&, long long, int) { return 1.0; }
__device__ __forceinline__ double slot_gain(const BlendArgs& b, long long o, int k) {
    return b.gains.data ? load_flow(b.gains, o * b.gains.stride[0] + k * b.gains.stride[1]) : 1.0;
}

// a sorts before b: a < b, or a is a number and b is NaN
__device__ __forceinline__ bool sorts_before(double a, double b) { return a < b || (a == a && b != b); }

// min and max that hand a NaN on (fmin and fmax drop it)
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a || b != b) ? a + b : fmin(a, b); }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

// The ROWS x 3 matrix at offset mb
template <int ROWS>
__device__ __forceinline__ void load_mat(const MosaicArgs& a, long long mb, double (&m)[3 * ROWS]) {
#pragma unroll
    for (int r = 0; r < ROWS; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) m[3 * r + c] = load_flow(a.mat, mb + r * a.mat.stride[2] + c * a.mat.stride[3]);
}

// A matrix row applied to the pixel p = (x, r): (a x + b r) + c; under the ray rule to its ray p = d: (a dx + b dy) + c dz
template <bool RAY = false>
__device__ __forceinline__ double row_at(const double* row, const double* p) {
    return (row[0] * p[0] + row[1] * p[1]) + (RAY ? row[2] * p[2] : row[2]);
}

// False where an entry of a matrix's first two rows is not finite: X and Y (Nx and Ny, and their quotients) are then +-inf or
// NaN at every pixel, live nowhere (phase 1 of the header comment, and rule (1) there)
__device__ __forceinline__ bool rows_finite(const double* m) {
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 6; j++) finite = finite && isfinite(m[j]);
    return finite;
}

// The affine corner box of one coordinate (the header comment, phase 1): true where its values v at the tile's four corners are
// all < -1 or all > top + 1.  WIDEN: the values are fl(v + U) below and fl(v + L) above (the mesh rule, (d)).  A NaN: false.
template <bool WIDEN>
__device__ __forceinline__ bool box_misses(const double (&v)[4], double top, double L, double U) {
    const auto low = [&](int j) { return WIDEN ? v[j] + L : v[j]; };
    const auto upp = [&](int j) { return WIDEN ? v[j] + U : v[j]; };
    return (upp(0) < -1.0 && upp(1) < -1.0 && upp(2) < -1.0 && upp(3) < -1.0) ||
           (low(0) > top + 1.0 && low(1) > top + 1.0 && low(2) > top + 1.0 && low(3) > top + 1.0);
}

// Phase 1 over the 2 x 3 matrix m, its first two rows finite: false where the slot is live at no pixel of [xa, xb] x [ra, rb]
// (the header comment, phase 1; WIDEN: under the mesh rule, its point moved by L[q] <= d <= U[q], the header's (d) there)
template <bool WIDEN>
__device__ __forceinline__ bool box_keep(const MosaicArgs& a, const double (&m)[6], double xa, double xb, double ra, double rb,
                                         const double* L = nullptr, const double* U = nullptr) {
    const double c[4][2] = {{xa, ra}, {xb, ra}, {xa, rb}, {xb, rb}};
    double X[4], Y[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        X[j] = row_at(m, c[j]);
        Y[j] = row_at(m + 3, c[j]);
    }
    // (a NaN corner -- an overflow meeting its opposite -- or bound proves nothing: every comparison is false, the slot stays)
    const bool missx = box_misses<WIDEN>(X, (double)(a.W - 1), WIDEN ? L[0] : 0.0, WIDEN ? U[0] : 0.0);
    const bool missy = box_misses<WIDEN>(Y, (double)(a.H - 1), WIDEN ? L[1] : 0.0, WIDEN ? U[1] : 0.0);
    return !missx && !missy;
}

// Phase 1 over a 2 x 3 matrix (at offset mb): the corner box of the header comment, phase 1
__device__ __forceinline__ bool affine_keep(const MosaicArgs& a, long long mb, double xa, double xb, double ra, double rb) {
    double m[6];
    load_mat<2>(a, mb, m);
    const bool box = box_keep<false>(a, m, xa, xb, ra, rb);
    return rows_finite(m) & box;  // (no short circuit: with it mosaic_overlap measured 2 % slower)
}

// Rules (2) to (5) of the header comment on the bounds lo[q] <= (D, Nx, Ny)[q] <= hi[q] over a tile, for a matrix that passed
// rule (1), rows_finite: false where the slot is live at no pixel of the tile.  nan: rule (2)'s test, true where a bound, or a
// value the bounds were taken from, is a NaN.
__device__ __forceinline__ bool quotients_keep(const MosaicArgs& a, bool nan, const double (&lo)[3], const double (&hi)[3]) {
    if (nan) return true;            // proves nothing
    if (!(hi[0] > 0)) return false;  // D > 0 at no pixel
    if (!(lo[0] > 0)) return true;   // the horizon may cross the tile
    const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);
    // (a quotient inf / inf is NaN: every comparison is false, the source stays)
    const bool missx = (hi[1] / lo[0] < -1.0 && hi[1] / hi[0] < -1.0) || (lo[1] / lo[0] > W1 + 1.0 && lo[1] / hi[0] > W1 + 1.0);
    const bool missy = (hi[2] / lo[0] < -1.0 && hi[2] / hi[0] < -1.0) || (lo[2] / lo[0] > H1 + 1.0 && lo[2] / hi[0] > H1 + 1.0);
    return !missx && !missy;
}

// Phase 1 over a 3 x 3 matrix (at offset mb): false where the slot is live at no pixel of [xa, xb] x [ra, rb]: the bounds of
// D, Nx and Ny are their extremes over the four corners (the header comment has the proof)
__device__ __forceinline__ bool projective_keep(const MosaicArgs& a, long long mb, double xa, double xb, double ra, double rb) {
    double m[9];
    load_mat<3>(a, mb, m);
    if (!rows_finite(m)) return false;  // (1)
    const double c[4][2] = {{xa, ra}, {xb, ra}, {xa, rb}, {xb, rb}};
    double lo[3], hi[3];
    bool nan = false;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const double* row = m + 3 * ((q + 2) % 3);
        const double v0 = row_at(row, c[0]), v1 = row_at(row, c[1]), v2 = row_at(row, c[2]), v3 = row_at(row, c[3]);
        nan = nan || v0 != v0 || v1 != v1 || v2 != v2 || v3 != v3;
        lo[q] = fmin(fmin(v0, v1), fmin(v2, v3));
        hi[q] = fmax(fmax(v0, v1), fmax(v2, v3));
    }
    return quotients_keep(a, nan, lo, hi);
}

// ---- the ray rule
// A value that every active lane of the wave holds alike, moved to scalar registers
__device__ __forceinline__ double wave_uniform(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// The ray of canvas pixel (x, r): d = (u_x * c_r, s_r, w_x * c_r).  A wave is one row of the tile (blocks are 64 x TY), so its
// lanes share r: s_r and c_r are held once per wave, and d[1] costs the walk no vector registers.
__device__ __forceinline__ void ray_of(const RayArgs& a, long long x, long long r, double d[3]) {
    const long long oc = x * a.cols.stride[0], orow = r * a.rows.stride[0];
    const double u = load_flow(a.cols, oc), w = load_flow(a.cols, oc + a.cols.stride[1]);
    const double s = wave_uniform(load_flow(a.rows, orow)), c = wave_uniform(load_flow(a.rows, orow + a.rows.stride[1]));
    d[0] = u * c;
    d[1] = s;
    d[2] = w * c;
}

// The bounds lo[j] <= d[j] <= hi[j] of the rays of a tile, read from the tables by the block itself: the lanes of a wave hold
// the tile's columns (`x` this lane's, clamped into the canvas by the caller), the tile's rows are ra, ra + dr, ..., rb.  Every
// wave of the block computes the same twelve numbers; all 64 lanes of the wave must be here.  A NaN table entry makes its
// bounds NaN (the header comment has the proof of what these bound).
__device__ __forceinline__ void ray_box(const RayArgs& a, long long x, long long ra, long long rb, long long dr, double lo[3],
                                        double hi[3]) {
    const long long oc = x * a.cols.stride[0];
    double ulo = load_flow(a.cols, oc), wlo = load_flow(a.cols, oc + a.cols.stride[1]);
    double uhi = ulo, whi = wlo;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        ulo = nan_min(ulo, __shfl_xor(ulo, d));
        uhi = nan_max(uhi, __shfl_xor(uhi, d));
        wlo = nan_min(wlo, __shfl_xor(wlo, d));
        whi = nan_max(whi, __shfl_xor(whi, d));
    }
    double slo = load_flow(a.rows, ra * a.rows.stride[0]), clo = load_flow(a.rows, ra * a.rows.stride[0] + a.rows.stride[1]);
    double shi = slo, chi = clo;
    for (long long r = ra + dr; r <= rb; r += dr) {
        const double s = load_flow(a.rows, r * a.rows.stride[0]), c = load_flow(a.rows, r * a.rows.stride[0] + a.rows.stride[1]);
        slo = nan_min(slo, s);
        shi = nan_max(shi, s);
        clo = nan_min(clo, c);
        chi = nan_max(chi, c);
    }
    const double x0 = ulo * clo, x1 = ulo * chi, x2 = uhi * clo, x3 = uhi * chi;
    const double z0 = wlo * clo, z1 = wlo * chi, z2 = whi * clo, z3 = whi * chi;
    // (the same in every lane after the butterfly: held in scalar registers, ray_keep's products take them from there)
    lo[0] = wave_uniform(nan_min(nan_min(x0, x1), nan_min(x2, x3)));
    hi[0] = wave_uniform(nan_max(nan_max(x0, x1), nan_max(x2, x3)));
    lo[1] = wave_uniform(slo);
    hi[1] = wave_uniform(shi);
    lo[2] = wave_uniform(nan_min(nan_min(z0, z1), nan_min(z2, z3)));
    hi[2] = wave_uniform(nan_max(nan_max(z0, z1), nan_max(z2, z3)));
}

// Phase 1 under the ray rule: false where the slot of the 3 x 3 matrix at mb is live at no pixel of the tile whose rays lie in
// [lo, hi] (ray_box; the header comment has the proof)
__device__ __forceinline__ bool ray_keep(const MosaicArgs& a, long long mb, const double lo[3], const double hi[3]) {
    double m[9];
    load_mat<3>(a, mb, m);
    if (!rows_finite(m)) return false;  // (1)
    double blo[3], bhi[3];              // the bounds of D, Nx, Ny
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int row = 3 * ((q + 2) % 3);
        double l[3], h[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double p0 = m[row + j] * lo[j], p1 = m[row + j] * hi[j];
            l[j] = nan_min(p0, p1);
            h[j] = nan_max(p0, p1);
        }
        blo[q] = (l[0] + l[1]) + l[2];
        bhi[q] = (h[0] + h[1]) + h[2];
    }
    bool nan = false;
#pragma unroll
    for (int q = 0; q < 3; q++) nan = nan || blo[q] != blo[q] || bhi[q] != bhi[q];
    return quotients_keep(a, nan, blo, bhi);
}

// ---- the mesh rule
// The extremes of every slot's table: blockIdx.x is slot `slot0` + x, the block one wave.  bounds[slot] = (dx lo, dx hi, dy lo,
// dy hi) over the (GH + 1) x (GW + 1) entries (at least four); a NaN entry makes its two bounds NaN.
__global__ __launch_bounds__(64) void k_mesh_bounds(const papof_tensor mesh, int VH, int VW, double* bounds, long long slot0,
                                                    long long) {
    const long long slot = slot0 + blockIdx.x;
    const double* t = static_cast<const double*>(mesh.data) + slot * mesh.stride[0];
    double xl = HUGE_VAL, xh = -HUGE_VAL, yl = HUGE_VAL, yh = -HUGE_VAL;
    for (int v = threadIdx.x; v < VH * VW; v += 64) {
        const long long e = (v / VW) * mesh.stride[1] + (v % VW) * mesh.stride[2];
        const double dx = t[e], dy = t[e + mesh.stride[3]];
        xl = nan_min(xl, dx);
        xh = nan_max(xh, dx);
        yl = nan_min(yl, dy);
        yh = nan_max(yh, dy);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        xl = nan_min(xl, __shfl_xor(xl, d));
        xh = nan_max(xh, __shfl_xor(xh, d));
        yl = nan_min(yl, __shfl_xor(yl, d));
        yh = nan_max(yh, __shfl_xor(yh, d));
    }
    if (threadIdx.x == 0) {
        double* b = bounds + slot * 4;
        b[0] = xl;
        b[1] = xh;
        b[2] = yl;
        b[3] = yh;
    }
}

// L <= dx <= U and the same for dy at every clean pixel of the slot whose bounds are b (the header comment, (a) to (c)): the
// four-term sum at its extreme terms, in the order the rule adds them.  A NaN bound stays a NaN.
__device__ __forceinline__ void mesh_widening(const double* b, double (&L)[2], double (&U)[2]) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double l = nan_min(b[2 * q], 0.0), u = nan_max(b[2 * q + 1], 0.0);
        L[q] = ((l + l) + l) + l;
        U[q] = ((u + u) + u) + u;
    }
}

// Phase 1 under the mesh rule: false where slot `slot` (its 2 x 3 matrix at mb) is live at no pixel of [xa, xb] x [ra, rb]: the
// affine corner box widened by the slot's bounds (the header comment has the proof)
__device__ __forceinline__ bool mesh_keep(const MeshMosaicArgs& a, long long mb, long long slot, double xa, double xb, double ra,
                                          double rb) {
    double m[6];
    load_mat<2>(a, mb, m);
    if (!rows_finite(m)) return false;  // X0 or Y0 is +-inf or NaN at every pixel, and X or Y with it
    double L[2], U[2];
    mesh_widening(a.bounds + slot * 4, L, U);
    return box_keep<true>(a, m, xa, xb, ra, rb, L, U);
}

// The affine point (X, Y) = (X0, Y0) moved by the displacement of slot `slot`'s table there: papof_warp_mesh_tensor's rule
// word for word (mesh.hip: k_warp_mesh, the table read from global memory).  False -- before the table is read -- where the
// slot's bounds prove that the moved point is outside the frame (the header comment; `slot` is uniform: scalar loads).
__device__ __forceinline__ bool mesh_point(const MeshMosaicArgs& a, long long slot, double& X, double& Y) {
    const double X0 = X, Y0 = Y;
    if (a.cull) {
        double L[2], U[2];
        mesh_widening(a.bounds + slot * 4, L, U);
        if (X0 + U[0] < 0 || X0 + L[0] > (double)(a.W - 1) || Y0 + U[1] < 0 || Y0 + L[1] > (double)(a.H - 1)) return false;
    }
    const double* mesh = static_cast<const double*>(a.mesh.data) + slot * a.mesh.stride[0];
    // mesh coordinates clamped to the mesh; a NaN stays one, takes cell 0 and makes (X, Y) a NaN
    double gx = (X0 * (double)a.GW) / (double)(a.W - 1), gy = (Y0 * (double)a.GH) / (double)(a.H - 1);
    gx = gx < 0 ? 0.0 : (gx > (double)a.GW ? (double)a.GW : gx);
    gy = gy < 0 ? 0.0 : (gy > (double)a.GH ? (double)a.GH : gy);
    const int cj = gx >= 0 ? std::min((int)gx, a.GW - 1) : 0, ci = gy >= 0 ? std::min((int)gy, a.GH - 1) : 0;
    const double fx = gx - (double)cj, fy = gy - (double)ci;
    double dx = 0.0, dy = 0.0;
#pragma unroll
    for (int mm = 0; mm <= 1; mm++)
#pragma unroll
        for (int nn = 0; nn <= 1; nn++) {
            const double w = fabs((double)(1 - mm) - fx) * fabs((double)(1 - nn) - fy);
            const long long e = (ci + nn) * a.mesh.stride[1] + (cj + mm) * a.mesh.stride[2];
            dx += mesh[e] * w;
            dy += mesh[e + a.mesh.stride[3]] * w;
        }
    X = X0 + dx;
    Y = Y0 + dy;
    return true;
}

// Phase 1, for a block of 64 x TY lanes: the slots of output o (src its sources, mo the offset of its matrices, slot0 the index
// of its first slot) that can be live somewhere in the pixel rectangle [xa, xb] x [ra, rb], compacted into `list` in k order;
// returns their number.  Ends with a barrier: list, and what the block wrote to LDS before the call, are visible after it.
template <int TY, typename A>
__device__ __forceinline__ int cull_slots(const A& a, const int* src, long long mo, long long slot0, double xa, double xb,
                                          double ra, double rb, unsigned short* list, int* wcount, const double* lo = nullptr,
                                          const double* hi = nullptr) {  // (lo, hi: RayArgs' ray_box, instead of the rectangle)
    constexpr int NT = kMosTX * TY;
    const int tid = threadIdx.y * kMosTX + threadIdx.x;
    int total = 0;
    for (int base = 0; base < a.n_src; base += NT) {
        const int k = base + tid;
        bool keep = k < a.n_src && src[k] >= 0;
        if (keep && a.cull) {
            const long long mb = mo + k * a.mat.stride[1];
            if constexpr (kProjective<A>)
                keep = projective_keep(a, mb, xa, xb, ra, rb);
            else if constexpr (kRay<A>)
                keep = ray_keep(a, mb, lo, hi);
            else if constexpr (kMesh<A>)
                keep = mesh_keep(a, mb, slot0 + k, xa, xb, ra, rb);
            else
                keep = affine_keep(a, mb, xa, xb, ra, rb);
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
    return total;
}

// The point (X, Y) of a pixel in slot `slot`, whose matrix is at mb, under the rule of A (include/papof.h): p is the pixel
// (x, r), under the ray rule its ray.  False where the point does not exist: D is not > 0 (a NaN included), or mesh_point's
// early-out.
template <typename A>
__device__ __forceinline__ bool slot_point(const A& a, long long mb, const double* p, long long slot, double& X, double& Y) {
    if constexpr (kProjective<A> || kRay<A>) {
        double m[9];
        load_mat<3>(a, mb, m);
        const double D = row_at<kRay<A>>(m + 6, p);
        X = row_at<kRay<A>>(m, p) / D;
        Y = row_at<kRay<A>>(m + 3, p) / D;
        return D > 0;
    } else {
        double m[6];
        load_mat<2>(a, mb, m);
        X = row_at(m, p);
        Y = row_at(m + 3, p);
        if constexpr (kMesh<A>) return mesh_point(a, slot, X, Y);
        return true;
    }
}

// The mask rule: true where a tap of positive weight of frame s is masked
__device__ __forceinline__ bool taps_masked(const MosaicArgs& a, long long s, const Bilinear& t) {
    const unsigned char* mk = static_cast<const unsigned char*>(a.mask.data);
    bool masked = false;
    const long long b = s * a.mask.stride[0];
#pragma unroll
    for (int j = 0; j < 4; j++)
        masked = masked || (t.w[j] > 0 && mk[b + t.row[j] * a.mask.stride[1] + t.col[j] * a.mask.stride[2]] != 0);
    return masked;
}

// Liveness: the taps of the point (X, Y) in frame s, live where the point is inside the frame and, under masks, none of its
// taps of positive weight is masked (the taps are set only where the point is inside).  Returned by value: through a reference
// the BlendArgs instances of k_mosaic took 73 VGPRs for 67, a wave per SIMD less.
struct LiveTaps : Bilinear {
    bool live;
};
// EARLY: leave at the first test that fails, instead of one exit.  The same tests either way; measured,
// the early exits cost mosaic_overlap 2 % and mosaic_homography's MEDIAN 2.6 %, the single exit mosaic_rays' MEDIAN 3 %.
template <typename A>
constexpr bool kEarlyLive = kRay<A>;
template <bool EARLY>
__device__ __forceinline__ LiveTaps live_taps(const MosaicArgs& a, long long s, double X, double Y) {
    LiveTaps t;
    t.live = X >= 0 && X <= (double)(a.W - 1) && Y >= 0 && Y <= (double)(a.H - 1);  // (false for a NaN)
    if constexpr (EARLY) {
        if (!t.live) return t;
        static_cast<Bilinear&>(t) = taps_at(X, Y, a.H, a.W);
        t.live = false;
        if (a.mask.data)
            if (taps_masked(a, s, t)) return t;
        t.live = true;
    } else if (t.live) {
        static_cast<Bilinear&>(t) = taps_at(X, Y, a.H, a.W);
        if (a.mask.data) t.live = !taps_masked(a, s, t);
    }
    return t;
}

// A: MosaicArgs (papof_mosaic_tensor), or BlendArgs: the sample of a live slot times its gain, and MODE FEATHER; or ProjArgs:
// BlendArgs under the projective rule; or RayArgs: BlendArgs under the ray rule; or MeshMosaicArgs: BlendArgs under the mesh rule
template <int FD, int MODE, int CAP, int TY, typename A>
__global__ __launch_bounds__(kMosTX* TY) void k_mosaic(const A a, long long tile0, long long out0) {
    constexpr bool BLEND = std::is_same<A, BlendArgs>::value || kProjective<A> || kRay<A> || kMesh<A>;
    static_assert(BLEND || MODE != PAPOF_MOSAIC_FEATHER, "k_mosaic: FEATHER is a blend mode");
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
    PAPOF_TILE_ORIGIN(MosTile<TY>, tile0, a.Wc, int, x0, long long, r0);
    const int* src = a.src + o * a.n_src;
    const long long mo = o * a.mat.stride[0];
    const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);

    // ---- 1. the sources that can reach this tile, in k order
    const long long rb = std::min(r0 + TY - 1, (long long)a.Hc - 1);
    double lo[3], hi[3];  // RayArgs: the bounds of the tile's rays
    if constexpr (kRay<A>)
        if (a.cull) ray_box(a, std::min(x0 + (int)threadIdx.x, a.Wc - 1), r0, rb, 1, lo, hi);
    const int total = cull_slots<TY>(a, src, mo, o * a.n_src, (double)x0, (double)std::min(x0 + kMosTX - 1, a.Wc - 1),
                                     (double)r0, (double)rb, list, wcount, lo, hi);
    const int x = x0 + (int)threadIdx.x;
    const long long r = r0 + threadIdx.y;
    if (x >= a.Wc || r >= a.Hc) return;  // (no barrier below)

    // ---- 2, 3. the walk
    const long long outp = PAPOF_AT(a.out, o, r, x);
    const bool all_sources = a.count.data != nullptr || MODE != PAPOF_MOSAIC_FIRST;
    double p[3] = {(double)x, (double)r};  // the pixel, or (RayArgs) its ray: once for every source and channel
    if constexpr (kRay<A>) ray_of(a, x, r, p);
    for (int c0 = 0; c0 < a.C; c0 += CH) {
        double acc[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) acc[j] = 0.0;
        double den = 0.0;  // FEATHER: the sum of the weights
        int n = 0;
        for (int i = 0; i < total; i++) {
            const int k = __builtin_amdgcn_readfirstlane((int)list[i]);
            const long long s = src[k];
            double X, Y;
            if (!slot_point(a, mo + k * a.mat.stride[1], p, o * a.n_src + k, X, Y)) continue;
            const LiveTaps t = live_taps<kEarlyLive<A>>(a, s, X, Y);
            if (!t.live) continue;
            const long long base = s * a.fr.stride[0] + c0 * a.fr.stride[3];
            const double gain = slot_gain(a, o, k);  // (MosaicArgs: the constant 1.0, and 1.0 * x is x: no instruction)
            if (MODE == PAPOF_MOSAIC_MEDIAN) {
                smp[n * NT + tid] = gain * sample_frame<FD>(a.fr, base, t, lut);
            } else if (MODE == PAPOF_MOSAIC_FEATHER) {
                const double w = fmin(fmin(X, W1 - X), fmin(Y, H1 - Y)) + 1.0;  // 1 on the frame's border
#pragma unroll
                for (int j = 0; j < CH; j++)
                    if (c0 + j < a.C) acc[j] = acc[j] + w * (gain * sample_frame<FD>(a.fr, base + j * a.fr.stride[3], t, lut));
                den = den + w;
            } else if (MODE == PAPOF_MOSAIC_MEAN || n == 0) {
#pragma unroll
                for (int j = 0; j < CH; j++)
                    if (c0 + j < a.C) {
                        const double g = gain * sample_frame<FD>(a.fr, base + j * a.fr.stride[3], t, lut);
                        acc[j] = MODE == PAPOF_MOSAIC_MEAN ? acc[j] + g : g;
                    }
            }
            n++;
            if (!all_sources) break;
        }
        if (c0 == 0 && a.count.data)
            store_u8(a.count, PAPOF_AT(a.count, o, r, x), (unsigned char)n);
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
                    if (MODE == PAPOF_MOSAIC_FEATHER) v = n > 0 ? v / den : 0.0;
                    store(a.out, outp + (c0 + j) * a.out.stride[3], v);
                }
        }
    }
}

template <int MODE, int CAP, int TY, typename A>
int launch_mosaic_as(hipStream_t st, const A& a, int n_out) {
    const int fd = a.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_mosaic<fd(), MODE, CAP, TY, A>; });
    return launch_grid<MosTile<TY>>(a.Hc, a.Wc, n_out, st, 0, kernel, a);
}

template <typename A>
int launch_mosaic(hipStream_t st, const A& a, int n_out, int mode) {
    const int n_src = a.n_src;
    if (mode == PAPOF_MOSAIC_FEATHER) {
        if constexpr (!std::is_same<A, MosaicArgs>::value) return launch_mosaic_as<PAPOF_MOSAIC_FEATHER, 0, 4>(st, a, n_out);
        return PAPOF_EINVAL;
    }
    if (mode == PAPOF_MOSAIC_FIRST) return launch_mosaic_as<PAPOF_MOSAIC_FIRST, 0, 4>(st, a, n_out);
    if (mode == PAPOF_MOSAIC_MEAN) return launch_mosaic_as<PAPOF_MOSAIC_MEAN, 0, 4>(st, a, n_out);
    if (n_src <= 8) return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 8, 4>(st, a, n_out);
    if (n_src <= 16) return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 16, 4>(st, a, n_out);
    if (n_src <= 32) return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 32, 2>(st, a, n_out);
    return launch_mosaic_as<PAPOF_MOSAIC_MEDIAN, 64, 1>(st, a, n_out);
}

// ---- papof_mosaic_overlap_tensor
constexpr int kOvTY = 2;                   // a 64 x 2 tile of sampled pixels: two waves, and a column's sum fits 32 bits
using OvTile = Tile<kMosTX, kOvTY>;
constexpr int kOvNT = kMosTX * kOvTY;
constexpr double kOvOne = 16777216.0;      // q = rint(t * 2^24)

template <typename A>
struct OverlapArgsOf {
    A m;                         // MosaicArgs or ProjArgs; out, count and gains are not used
    unsigned long long* sums;    // (out, i, j), contiguous
    unsigned long long* counts;
    double bound;
    int step;
    int nsx, nsr;                // sampled columns and rows: ceil(Wc / step), ceil(Hc / step)
};

// NS: the slots the tables hold (n_src <= NS), a power of two <= 64
template <int FD, int NS, typename A>
__global__ __launch_bounds__(kOvNT) void k_mosaic_overlap(const OverlapArgsOf<A> args, long long tile0, long long out0) {
    constexpr int G = 64 / NS;  // pixels side by side in phase 3
    const A& a = args.m;
    __shared__ double lut[256];
    __shared__ unsigned short list[64];
    __shared__ int wcount[kOvTY];
    __shared__ unsigned long long live[kOvNT];  // bit k: slot k is live at the pixel (and its luminance a number)
    __shared__ unsigned qs[NS * kOvNT];         // [slot][pixel], written where the bit is set
    __shared__ unsigned tsum[NS * 64];          // [i][lane]: a lane adds <= kOvNT / G values <= 2^24, < 2^32
    __shared__ unsigned tcnt[NS * 64];
    const int tid = threadIdx.y * kMosTX + threadIdx.x;
    if (FD == PAPOF_DTYPE_U8)
        for (int j = tid; j < 256; j += kOvNT) fill_u8_lut(lut, j);
    for (int j = tid; j < NS * 64; j += kOvNT) {
        tsum[j] = 0;
        tcnt[j] = 0;
    }
    const long long o = out0 + blockIdx.y;
    PAPOF_TILE_ORIGIN(OvTile, tile0, args.nsx, int, sx0, long long, sr0);
    const int* src = a.src + o * a.n_src;
    const long long mo = o * a.mat.stride[0];
    const long long step = args.step;

    // ---- 1. the sources that can reach the tile's pixels (all of them lie in the rectangle of its corners)
    double lo[3], hi[3];  // RayArgs: the bounds of the rays of the tile's sampled pixels
    if constexpr (kRay<A>)
        if (a.cull)
            ray_box(a, std::min(sx0 + (int)threadIdx.x, args.nsx - 1) * step, sr0 * step,
                    std::min(sr0 + kOvTY - 1, (long long)args.nsr - 1) * step, step, lo, hi);
    const int total = cull_slots<kOvTY>(a, src, mo, o * a.n_src, (double)(sx0 * step),
                                        (double)(std::min(sx0 + kMosTX - 1, args.nsx - 1) * step), (double)(sr0 * step),
                                        (double)(std::min(sr0 + kOvTY - 1, (long long)args.nsr - 1) * step), list, wcount, lo, hi);

    // ---- 2. the walk: the luminance of every live slot, in fixed point
    const int sx = sx0 + (int)threadIdx.x;
    const long long sr = sr0 + threadIdx.y;
    unsigned long long mine = 0;
    if (sx < args.nsx && sr < args.nsr) {
        double p[3] = {(double)(sx * step), (double)(sr * step)};  // the pixel, or (RayArgs) its ray
        if constexpr (kRay<A>) ray_of(a, sx * step, sr * step, p);
        for (int i = 0; i < total; i++) {
            const int k = __builtin_amdgcn_readfirstlane((int)list[i]);
            const long long s = src[k];
            double X, Y;
            if (!slot_point(a, mo + k * a.mat.stride[1], p, o * a.n_src + k, X, Y)) continue;
            const LiveTaps t = live_taps<kEarlyLive<A>>(a, s, X, Y);
            if (!t.live) continue;
            const long long base = s * a.fr.stride[0];
            double y = 0.0;
            for (int ch = 0; ch < a.C; ch++) y = y + sample_frame<FD>(a.fr, base + ch * a.fr.stride[3], t, lut);
            y = y / (double)a.C;
            if (y != y) continue;
            double q = y / args.bound;
            q = q < 0.0 ? 0.0 : q;
            q = q > 1.0 ? 1.0 : q;
            qs[k * kOvNT + tid] = (unsigned)(long long)rint(q * kOvOne);
            mine |= 1ULL << k;
        }
    }
    live[tid] = mine;
    __syncthreads();

    // ---- 3. lane = (pixel of G, source j); wave w owns the rows i = w (mod kOvTY) of the tables
    const int lane = threadIdx.x;
    const int sub = lane / NS, j = lane % NS;
    unsigned long long rows = 0;
    for (int i = threadIdx.y; i < NS; i += kOvTY) rows |= 1ULL << i;
    unsigned touched_lo = 0, touched_hi = 0;
    for (int pb = 0; pb < kOvNT; pb += G) {
        unsigned long long any = 0;
        for (int g = 0; g < G; g++) any |= live[pb + g];  // (one address each: a broadcast)
        any &= rows;
        unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)any), hi = __builtin_amdgcn_readfirstlane((unsigned)(any >> 32));
        if (!(lo | hi)) continue;
        touched_lo |= lo;
        touched_hi |= hi;
        const int p = pb + sub;
        const unsigned long long m = live[p];
        const bool has = (m >> j) & 1;
        for (int half = 0; half < 2; half++) {
            unsigned bits = half ? hi : lo;
            while (bits) {
                const int i = 32 * half + __builtin_ctz(bits);
                bits &= bits - 1;
                if (has && ((m >> i) & 1)) {
                    tsum[i * 64 + lane] += qs[i * kOvNT + p];
                    tcnt[i * 64 + lane] += 1;
                }
            }
        }
    }

    // ---- the rows this wave touched: one contiguous row of 64-bit integer adds per instruction
    const long long N = a.n_src;
    for (int half = 0; half < 2; half++) {
        unsigned bits = half ? touched_hi : touched_lo;
        while (bits) {
            const int i = 32 * half + __builtin_ctz(bits);
            bits &= bits - 1;
            if (lane < NS) {
                unsigned long long sum = 0, cnt = 0;
                for (int g = 0; g < G; g++) {
                    sum += tsum[i * 64 + g * NS + lane];
                    cnt += tcnt[i * 64 + g * NS + lane];
                }
                if (cnt != 0) {  // (bit `lane` was set at some pixel: lane < n_src, as i is)
                    const long long e = (o * N + i) * N + lane;
                    add64(args.sums + e, (long long)sum);
                    add64(args.counts + e, (long long)cnt);
                }
            }
        }
    }
}

template <int NS, typename A>
int launch_overlap_as(hipStream_t st, const OverlapArgsOf<A>& a, int n_out) {
    const int fd = a.m.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_mosaic_overlap<fd(), NS, A>; });
    return launch_grid<OvTile>(a.nsr, a.nsx, n_out, st, 0, kernel, a);
}

// The arguments the three calls share, checked and gathered; out and count are the caller's to check and set
bool mosaic_args_from(MosaicArgs& a, const papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                      const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width, const int* sources,
                      const papof_tensor* matrices) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1 || n_out < 1 || out_height < 1 || out_width < 1) return false;
    if (n_src < 1 || n_src > PAPOF_MOSAIC_MAX_SOURCES || !sources) return false;
    if (!in_frames(frames)) return false;
    if (!opt_in_mask(masks)) return false;
    if (!in_flow(matrices)) return false;
    a.fr = *frames;
    if (masks) a.mask = *masks;
    a.mat = *matrices;
    a.src = sources;
    a.H = height;
    a.W = width;
    a.C = c;
    a.Hc = out_height;
    a.Wc = out_width;
    a.n_src = n_src;
    const char* e = std::getenv("PAPOF_MOSAIC_CULL");  // "0": no tile-level culling (tools/mosaic_probe.py measures its worth)
    a.cull = !(e && e[0] == '0');
    return true;
}

bool mosaic_outputs(MosaicArgs& a, const papof_tensor* out, const papof_tensor* count) {
    if (!out_frames(out)) return false;
    if (!opt_out_mask(count)) return false;
    a.out = *out;
    if (count) a.count = *count;
    return true;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_mosaic_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                   const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                   const int* sources, const papof_tensor* matrices, int mode, const papof_tensor* out,
                                   const papof_tensor* count, void* stream) {
    MosaicArgs a{};
    if (!mosaic_args_from(a, h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources, matrices))
        return PAPOF_EINVAL;
    if (mode != PAPOF_MOSAIC_FIRST && mode != PAPOF_MOSAIC_MEAN && mode != PAPOF_MOSAIC_MEDIAN) return PAPOF_EINVAL;
    if (mode == PAPOF_MOSAIC_MEDIAN && n_src > PAPOF_MOSAIC_MAX_MEDIAN) return PAPOF_EINVAL;
    if (!mosaic_outputs(a, out, count)) return PAPOF_EINVAL;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_mosaic(static_cast<hipStream_t>(stream), a, n_out, mode);
}

// The tables of the ray rule, checked and gathered
static bool ray_tables(RayArgs& a, const papof_tensor* cols, const papof_tensor* rows) {
    if (!described(cols, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1}, false)) return false;
    if (!described(rows, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1}, false)) return false;
    a.cols = *cols;
    a.rows = *rows;
    return true;
}

// What papof_mosaic_mesh_tensor takes beyond the blend call
struct MeshTables {
    const papof_tensor* mesh;
    int grid_rows, grid_cols;
    void* workspace;
    long long workspace_bytes;
};

// The tables of the mesh rule, checked and gathered (the grid's bounds are papof_warp_mesh_tensor's, against the frames)
static bool mesh_tables(MeshMosaicArgs& a, const MeshTables* t, int height, int width, int n_out, int n_src) {
    if (!t || !described(t->mesh, {PAPOF_DTYPE_F64}, {0, 1, 2, 3}, false)) return false;
    const int gh = t->grid_rows, gw = t->grid_cols;
    if (gh < 1 || gw < 1 || gh > PAPOF_MESH_MAX_CELLS || gw > PAPOF_MESH_MAX_CELLS || gh > height - 1 || gw > width - 1) return false;
    const long long need = papof_mosaic_mesh_workspace(n_out, n_src);
    if (need < 0 || !t->workspace || t->workspace_bytes < need) return false;
    a.mesh = *t->mesh;
    a.bounds = static_cast<const double*>(t->workspace);
    a.GH = gh;
    a.GW = gw;
    return true;
}

// papof_mosaic_blend_tensor (A = BlendArgs), papof_mosaic_projective_tensor (A = ProjArgs), papof_mosaic_ray_tensor (A =
// RayArgs, with its tables) and papof_mosaic_mesh_tensor (A = MeshMosaicArgs, with its tables and workspace)
template <typename A>
static int mosaic_blend(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                        const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width, const int* sources,
                        const papof_tensor* matrices, const papof_tensor* gains, int mode, const papof_tensor* out,
                        const papof_tensor* count, void* stream, const papof_tensor* cols = nullptr,
                        const papof_tensor* rows = nullptr, const MeshTables* tables = nullptr) {
    A b{};
    if constexpr (kRay<A>)
        if (!ray_tables(b, cols, rows)) return PAPOF_EINVAL;
    if constexpr (kMesh<A>)
        if (!mesh_tables(b, tables, height, width, n_out, n_src)) return PAPOF_EINVAL;
    if (!mosaic_args_from(b, h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                          matrices))
        return PAPOF_EINVAL;
    if (mode < PAPOF_MOSAIC_FIRST || mode > PAPOF_MOSAIC_FEATHER) return PAPOF_EINVAL;
    if (mode == PAPOF_MOSAIC_MEDIAN && n_src > PAPOF_MOSAIC_MAX_MEDIAN) return PAPOF_EINVAL;
    if (gains && !described(gains, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1}, false)) return PAPOF_EINVAL;
    if (!mosaic_outputs(b, out, count)) return PAPOF_EINVAL;
    PAPOF_HIP(hipSetDevice(h->device));
    if constexpr (std::is_same<A, BlendArgs>::value)
        if (!gains && mode != PAPOF_MOSAIC_FEATHER)  // every gain 1: the instances papof_mosaic_tensor launches
            return launch_mosaic(static_cast<hipStream_t>(stream), static_cast<const MosaicArgs&>(b), n_out, mode);
    if (gains) b.gains = *gains;
    if constexpr (kMesh<A>)
        if (b.cull)  // the extremes of every slot's table, ahead of k_mosaic on the stream
            PAPOF_TRY(launch_tiles((long long)n_out * n_src, 1, [&](dim3 grid, long long s0, long long f0) {
                hipLaunchKernelGGL(k_mesh_bounds, grid, dim3(64), 0, static_cast<hipStream_t>(stream), b.mesh, b.GH + 1,
                                   b.GW + 1, static_cast<double*>(tables->workspace), s0, f0);
            }));
    return launch_mosaic(static_cast<hipStream_t>(stream), b, n_out, mode);
}

extern "C" int papof_mosaic_blend_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                         const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                         const int* sources, const papof_tensor* matrices, const papof_tensor* gains, int mode,
                                         const papof_tensor* out, const papof_tensor* count, void* stream) {
    return mosaic_blend<BlendArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                                   matrices, gains, mode, out, count, stream);
}

extern "C" int papof_mosaic_projective_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                              const papof_tensor* frames, const papof_tensor* masks, int n_out, int n_src,
                                              int out_height, int out_width, const int* sources, const papof_tensor* matrices,
                                              const papof_tensor* gains, int mode, const papof_tensor* out,
                                              const papof_tensor* count, void* stream) {
    return mosaic_blend<ProjArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                                  matrices, gains, mode, out, count, stream);
}

// papof_mosaic_overlap_tensor (A = MosaicArgs), papof_mosaic_overlap_projective_tensor (A = ProjArgs) and
// papof_mosaic_overlap_ray_tensor (A = RayArgs, with its tables)
template <typename A>
static int mosaic_overlap(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                          const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width, const int* sources,
                          const papof_tensor* matrices, int step, double bound, long long* sums, long long* counts,
                          void* stream, const papof_tensor* cols = nullptr, const papof_tensor* rows = nullptr) {
    OverlapArgsOf<A> a{};
    if constexpr (kRay<A>)
        if (!ray_tables(a.m, cols, rows)) return PAPOF_EINVAL;
    if (!mosaic_args_from(a.m, h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                          matrices))
        return PAPOF_EINVAL;
    if (n_src > PAPOF_MOSAIC_MAX_OVERLAP || step < 1 || !std::isfinite(bound) || !(bound > 0) || !sums || !counts)
        return PAPOF_EINVAL;
    a.sums = reinterpret_cast<unsigned long long*>(sums);
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    a.bound = bound;
    a.step = step;
    a.nsx = (out_width - 1) / step + 1;
    a.nsr = (out_height - 1) / step + 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PAPOF_HIP(hipSetDevice(h->device));
    const size_t bytes = sizeof(long long) * (size_t)n_out * n_src * n_src;
    PAPOF_HIP(hipMemsetAsync(sums, 0, bytes, st));
    PAPOF_HIP(hipMemsetAsync(counts, 0, bytes, st));
    if (n_src <= 8) return launch_overlap_as<8>(st, a, n_out);
    if (n_src <= 16) return launch_overlap_as<16>(st, a, n_out);
    if (n_src <= 32) return launch_overlap_as<32>(st, a, n_out);
    return launch_overlap_as<64>(st, a, n_out);
}

extern "C" int papof_mosaic_overlap_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                           const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                           const int* sources, const papof_tensor* matrices, int step, double bound,
                                           long long* sums, long long* counts, void* stream) {
    return mosaic_overlap<MosaicArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                                      matrices, step, bound, sums, counts, stream);
}

extern "C" int papof_mosaic_overlap_projective_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                                      const papof_tensor* frames, const papof_tensor* masks, int n_out, int n_src,
                                                      int out_height, int out_width, const int* sources,
                                                      const papof_tensor* matrices, int step, double bound, long long* sums,
                                                      long long* counts, void* stream) {
    return mosaic_overlap<ProjArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                                    matrices, step, bound, sums, counts, stream);
}

extern "C" int papof_mosaic_ray_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                       const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                       const int* sources, const papof_tensor* matrices, const papof_tensor* cols,
                                       const papof_tensor* rows, const papof_tensor* gains, int mode, const papof_tensor* out,
                                       const papof_tensor* count, void* stream) {
    return mosaic_blend<RayArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                                 matrices, gains, mode, out, count, stream, cols, rows);
}

extern "C" int papof_mosaic_overlap_ray_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                               const papof_tensor* frames, const papof_tensor* masks, int n_out, int n_src,
                                               int out_height, int out_width, const int* sources, const papof_tensor* matrices,
                                               const papof_tensor* cols, const papof_tensor* rows, int step, double bound,
                                               long long* sums, long long* counts, void* stream) {
    return mosaic_overlap<RayArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width, sources,
                                   matrices, step, bound, sums, counts, stream, cols, rows);
}

extern "C" long long papof_mosaic_mesh_workspace(int n_out, int n_src) {
    if (n_out < 1 || n_src < 1 || n_src > PAPOF_MOSAIC_MAX_SOURCES) return -1;
    return 32LL * n_out * n_src;
}

extern "C" int papof_mosaic_mesh_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                        const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                        const int* sources, const papof_tensor* matrices, const papof_tensor* mesh,
                                        int grid_rows, int grid_cols, const papof_tensor* gains, int mode,
                                        const papof_tensor* out, const papof_tensor* count, void* workspace,
                                        long long workspace_bytes, void* stream) {
    const MeshTables tables{mesh, grid_rows, grid_cols, workspace, workspace_bytes};
    return mosaic_blend<MeshMosaicArgs>(h, n_frames, height, width, c, frames, masks, n_out, n_src, out_height, out_width,
                                        sources, matrices, gains, mode, out, count, stream, nullptr, nullptr, &tables);
}

// Every instance launch_mosaic dispatches to has a lane per slot (n_src <= 64 * TY), so phase 1's loop over the slots runs once.
static_assert(kMaxSrc <= kMosTX * 4 && 8 <= kMosTX * 4 && 16 <= kMosTX * 4 && 32 <= kMosTX * 2 &&
                  PAPOF_MOSAIC_MAX_MEDIAN <= kMosTX * 1 && PAPOF_MOSAIC_MAX_SOURCES < kMaxSrc,
              "k_mosaic: a lane per slot in one pass of phase 1");
static_assert(PAPOF_MOSAIC_MAX_OVERLAP <= 64 && PAPOF_MOSAIC_MAX_OVERLAP <= kOvNT && (long long)kOvNT * 16777216LL < (1LL << 32),
              "k_mosaic_overlap: a bit and a lane per slot, a column's sum in 32 bits");
