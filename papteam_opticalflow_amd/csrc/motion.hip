// papteam_opticalflow_amd/csrc/motion.hip -- global motion of a flow field (papof_motion_fit_tensor) and the affine warp of
// frames (papof_warp_affine_tensor): the two device halves of video stabilization.
//
// Why.  Global camera motion (stabilization, camera-motion compensation, shot-boundary checks) is a robust parametric fit to
// a pair's flow.  Written with torch.linalg.lstsq it is a copy of the flow into a (pixels x parameters) system and several
// launches per IRLS iteration; here it is a reduction of fourteen fp64 sums over the flow, read once per iteration, and a
// 4 x 4 or 3 x 3 solve.
//
// Semantics: include/papof.h, papof_motion_fit_tensor and papof_warp_affine_tensor.  fp64 without contraction
// (-ffp-contract=off).
//
// Reduction.  Bitwise reproducible from run to run and on every device, so there are no atomics.  Launch 1 (k_motion_sums):
// a block is a 64 x 32 tile of pixels of one pair (grid.h's grid of tiles and pairs), a lane one column and 8 rows
// (threadIdx.y + 4 k) in increasing row order; the lanes of a wave are summed by a fixed shuffle tree (__shfl_down, 32 .. 1),
// the four waves in wave order through LDS, and the block writes one row of fourteen doubles to the workspace.  The number
// of blocks of a pair is a function of (H, W) alone.  Launch 2 (k_motion_solve): one wave per pair; lane l adds the rows
// l, l + 64, l + 128, ... in increasing order, the lanes are summed by the same shuffle tree, and lane 0 solves and writes
// the pair's matrix to its state row and to the outputs.  The next iteration's launch 1 reads that matrix as uniform loads.
// Every offset is 64-bit; launch 1 is split at gridDim.y = 65535 pairs.
//
// The homography model (papof_homography_fit_tensor, papof_warp_projective_tensor) is the same structure: k_homography_sums
// reduces twenty-five sums (the 8 x 8 normal equations of the direct linear transform need twenty-three, the count and the
// sum of the Cauchy weights are the other two) in the order above into rows of 32 doubles, k_homography_solve adds them and
// eliminates the 8 x 9 system in lane 0, in registers; k_warp_projective is k_warp_affine with (X, Y) = (Nx / D, Ny / D).
//
// Warp.  k_warp_affine: a block is a 64 x 4 tile of output pixels (grid.h's grid of tiles and frames), as k_interp's;
// the block reads its frame's matrix once (uniform loads) and samples with sampler.h's bilinear rule.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr int kFitTX = 64, kFitTY = 4, kFitRows = 8;  // a lane: one column, kFitRows rows kFitTY apart
constexpr int kFitTH = kFitTY * kFitRows;            // a block: 64 x 32 pixels
using FitTile = Tile<kFitTX, kFitTH, kFitTX, kFitTY>;  // a strip of kFitTH rows under a block of kFitTY
constexpr int kSums = 14;                             // include/papof.h: the order of the sums
constexpr int kRow = 16;                              // doubles per partial row (kSums used)
constexpr int kState = 8;                             // doubles per pair: matrix (6), ok (1), finished (1)
constexpr int kWarpTX = 64, kWarpTY = 4;              // a 64 x 4 tile of output pixels per block (256 lanes: lut)
using WarpTile = Tile<kWarpTX, kWarpTY>;

long long fit_blocks(int H, int W) {
    return FitTile::count(H, W);
}

struct FitArgs {
    papof_tensor flow;  // (pair, row, column, {vx, vy})
    papof_tensor occ;   // uint8 (pair, row, column, {fw, bw}); data NULL: none
    const double* state;
    double* part;       // (pair, block, kRow)
    long long blocks;   // per pair
    int H, W;
    int iter;
    double cx, cy, s, c2;
};

struct SolveArgs {
    double* state;        // (pair, kState)
    const double* part;
    papof_tensor motion;  // float64 (pair, row, column)
    papof_tensor ok;      // uint8 (pair)
    papof_tensor support; // float64 (pair)
    long long blocks;
    int model;
    int iter;
    double cx, cy, s, hw;
};

// the sum of acc over the 64 lanes of the wave, in lane 0: a fixed tree
__device__ __forceinline__ void wave_sum(double (&acc)[kSums]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < kSums; k++) acc[k] += __shfl_down(acc[k], off, 64);
}

__global__ __launch_bounds__(kFitTX* kFitTY) void k_motion_sums(const FitArgs a, long long pair0) {
    __shared__ double red[kFitTY][kSums];
    const long long i = pair0 + blockIdx.y;
    const double* st = a.state + i * kState;
    if (a.iter > 0 && st[7] != 0.0) return;  // the pair's iteration 0 failed: finished (uniform over the block)
    double m[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (a.iter > 0)
#pragma unroll
        for (int k = 0; k < 6; k++) m[k] = st[k];
    PAPOF_TILE_PIXEL(FitTile, 0LL, a.W, int, x, long long, r0);  // (one launch holds every strip: fit_blocks <= kMaxTiles)
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; k++) acc[k] = 0.0;
    if (x < a.W) {
        const double xd = (double)x, xh = (xd - a.cx) / a.s;
        const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);
        for (int j = 0; j < kFitRows; j++) {
            const long long r = r0 + (long long)j * kFitTY;
            if (r >= a.H) break;
            const long long o = PAPOF_AT(a.flow, i, r, x);
            const double u = load_flow(a.flow, o), v = load_flow(a.flow, o + a.flow.stride[3]);
            const double rd = (double)r, X = xd + u, Y = rd + v;
            bool valid = X >= 0 && X <= W1 && Y >= 0 && Y <= H1;  // false for a NaN or an infinity
            if (valid && a.occ.data)
                valid = load_u8(a.occ, PAPOF_AT(a.occ, i, r, x)) == 0;
            if (!valid) continue;
            double w = 1.0;
            if (a.iter > 0) {
                const double ex = X - ((m[0] * xd + m[1] * rd) + m[2]), ey = Y - ((m[3] * xd + m[4] * rd) + m[5]);
                const double e2 = ex * ex + ey * ey;
                w = 1.0 / (1.0 + e2 / a.c2);
                acc[13] += w * e2;
            }
            const double yh = (rd - a.cy) / a.s, Xh = (X - a.cx) / a.s, Yh = (Y - a.cy) / a.s;
            acc[0] += w * (xh * xh);
            acc[1] += w * (xh * yh);
            acc[2] += w * (yh * yh);
            acc[3] += w * xh;
            acc[4] += w * yh;
            acc[5] += w;
            acc[6] += w * (xh * Xh);
            acc[7] += w * (yh * Xh);
            acc[8] += w * Xh;
            acc[9] += w * (xh * Yh);
            acc[10] += w * (yh * Yh);
            acc[11] += w * Yh;
            acc[12] += 1.0;
        }
    }
    wave_sum(acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kSums; k++) red[threadIdx.y][k] = acc[k];
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < kSums) {
        const int k = threadIdx.x;
        a.part[(i * a.blocks + tile) * kRow + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// Gaussian elimination in natural order without row exchanges on the N x N matrix of `g` with R right-hand sides (columns
// N .. N + R - 1); false where a pivot is not > tol (NaN included).  x[r] solves the system of right-hand side r.
template <int N, int R>
__device__ bool eliminate(double (&g)[N][N + R], double tol, double (&x)[R][N]) {
    for (int k = 0; k < N; k++) {
        const double piv = g[k][k];
        if (!(piv > tol)) return false;
        for (int i = k + 1; i < N; i++) {
            const double f = g[i][k] / piv;
            for (int j = k; j < N + R; j++) g[i][j] = g[i][j] - f * g[k][j];
        }
    }
    for (int r = 0; r < R; r++)
        for (int i = N - 1; i >= 0; i--) {
            double v = g[i][N + r];
            for (int j = i + 1; j < N; j++) v = v - g[i][j] * x[r][j];
            x[r][i] = v / g[i][i];
        }
    return true;
}

// the pixel-coordinate matrix m of the normalised sums S (include/papof.h); false where the iteration fails
__device__ bool fit_solve(const double (&S)[kSums], int model, double cx, double cy, double s, double (&m)[6]) {
    const double sw = S[5];
    if (!(sw > 0)) return false;
    const double tol = 1e-12 * sw;
    double L0, L1, L2, L3, tx, ty;
    if (model == PAPOF_MOTION_AFFINE) {
        double g[3][5] = {{S[0], S[1], S[3], S[6], S[9]}, {S[1], S[2], S[4], S[7], S[10]}, {S[3], S[4], S[5], S[8], S[11]}};
        double p[2][3];
        if (!eliminate<3, 2>(g, tol, p)) return false;
        L0 = p[0][0], L1 = p[0][1], tx = p[0][2], L2 = p[1][0], L3 = p[1][1], ty = p[1][2];
    } else {
        const double s2 = S[0] + S[2];
        double g[4][5] = {{s2, 0.0, S[3], S[4], S[6] + S[10]},
                          {0.0, s2, -S[4], S[3], S[9] - S[7]},
                          {S[3], -S[4], sw, 0.0, S[8]},
                          {S[4], S[3], 0.0, sw, S[11]}};
        double p[1][4];
        if (!eliminate<4, 1>(g, tol, p)) return false;
        L0 = p[0][0], L1 = -p[0][1], L2 = p[0][1], L3 = p[0][0], tx = p[0][2], ty = p[0][3];
    }
    m[0] = L0;
    m[1] = L1;
    m[2] = (cx + s * tx) - (L0 * cx + L1 * cy);
    m[3] = L2;
    m[4] = L3;
    m[5] = (cy + s * ty) - (L2 * cx + L3 * cy);
    for (int k = 0; k < 6; k++)
        if (!isfinite(m[k])) return false;
    return true;
}

__global__ __launch_bounds__(64) void k_motion_solve(const SolveArgs a, long long pair0) {
    const long long i = pair0 + blockIdx.x;
    double* st = a.state + i * kState;
    if (a.iter > 0 && st[7] != 0.0) return;
    const double* p = a.part + i * a.blocks * kRow;
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; k++) acc[k] = 0.0;
    for (long long b = threadIdx.x; b < a.blocks; b += 64)
#pragma unroll
        for (int k = 0; k < kSums; k++) acc[k] += p[b * kRow + k];
    wave_sum(acc);
    if (threadIdx.x != 0) return;
    double m[6];
    if (fit_solve(acc, a.model, a.cx, a.cy, a.s, m)) {
        for (int k = 0; k < 6; k++) st[k] = m[k];
        st[6] = 1.0;
        st[7] = 0.0;
    } else if (a.iter == 0) {  // the identity, ok = 0, no further iterations
        const double id[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        for (int k = 0; k < 6; k++) st[k] = id[k];
        st[6] = 0.0;
        st[7] = 1.0;
    }  // else: the last successful iteration's matrix stays
    double* mo = static_cast<double*>(a.motion.data) + i * a.motion.stride[0];
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 3; c++) mo[r * a.motion.stride[1] + c * a.motion.stride[2]] = st[3 * r + c];
    static_cast<unsigned char*>(a.ok.data)[i * a.ok.stride[0]] = st[6] != 0.0 ? 1 : 0;  // (store_u8 evaluates the value first: other schedule)
    static_cast<double*>(a.support.data)[i * a.support.stride[0]] = acc[5] / a.hw;
}

int launch_fit(hipStream_t st, FitArgs f, SolveArgs s, int n_pairs, int n_iter) {
    for (int it = 0; it < n_iter; it++) {
        f.iter = s.iter = it;
        PAPOF_TRY(launch_tiles(f.blocks, n_pairs, [&](dim3 grid, long long, long long p0) {  // (blocks <= kMaxTiles)
            hipLaunchKernelGGL(k_motion_sums, grid, FitTile::block(), 0, st, f, p0);
        }));
        hipLaunchKernelGGL(k_motion_solve, dim3((unsigned)n_pairs), dim3(64), 0, st, s, 0LL);
        PAPOF_HIP(hipGetLastError());
    }
    return PAPOF_OK;
}

// ---- the homography model (papof_homography_fit_tensor): the affine fit's structure over twenty-five sums and an 8 x 8 solve
constexpr int kHSums = 25;   // include/papof.h: the order of the sums
constexpr int kHRow = 32;    // doubles per partial row (kHSums used)
constexpr int kHState = 12;  // doubles per pair: matrix (9), ok (1), finished (1), unused (1)

template <int N>
__device__ __forceinline__ void wave_sum_of(double (&acc)[N]) {  // wave_sum's tree over N sums
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] += __shfl_down(acc[k], off, 64);
}

// FitArgs as k_motion_sums takes them; the state rows are kHState wide and the partial rows kHRow
__global__ __launch_bounds__(kFitTX* kFitTY) void k_homography_sums(const FitArgs a, long long pair0) {
    __shared__ double red[kFitTY][kHSums];
    const long long i = pair0 + blockIdx.y;
    const double* st = a.state + i * kHState;
    if (a.iter > 0 && st[10] != 0.0) return;  // the pair's iteration 0 failed: finished (uniform over the block)
    double m[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (a.iter > 0)
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = st[k];
    const double dc = (m[6] * a.cx + m[7] * a.cy) + m[8];  // the denominator at the image centre
    PAPOF_TILE_PIXEL(FitTile, 0LL, a.W, int, x, long long, r0);  // (one launch holds every strip: fit_blocks <= kMaxTiles)
    double acc[kHSums];
#pragma unroll
    for (int k = 0; k < kHSums; k++) acc[k] = 0.0;
    if (x < a.W) {
        const double xd = (double)x, xh = (xd - a.cx) / a.s;
        const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);
        for (int j = 0; j < kFitRows; j++) {
            const long long r = r0 + (long long)j * kFitTY;
            if (r >= a.H) break;
            const long long o = PAPOF_AT(a.flow, i, r, x);
            const double u = load_flow(a.flow, o), v = load_flow(a.flow, o + a.flow.stride[3]);
            const double rd = (double)r, X = xd + u, Y = rd + v;
            bool valid = X >= 0 && X <= W1 && Y >= 0 && Y <= H1;  // false for a NaN or an infinity
            if (valid && a.occ.data)
                valid = load_u8(a.occ, PAPOF_AT(a.occ, i, r, x)) == 0;
            if (!valid) continue;
            acc[23] += 1.0;
            double w = 1.0, c = 1.0;
            if (a.iter > 0) {
                const double d = (m[6] * xd + m[7] * rd) + m[8], dn = d / dc;
                if (!(dn > PAPOF_HOMOGRAPHY_MIN_DEN)) continue;  // at or behind the previous iterate's horizon (NaN included)
                const double ex = X - ((m[0] * xd + m[1] * rd) + m[2]) / d, ey = Y - ((m[3] * xd + m[4] * rd) + m[5]) / d;
                const double e2 = ex * ex + ey * ey;
                c = 1.0 / (1.0 + e2 / a.c2);
                w = c / (dn * dn);
            }
            const double yh = (rd - a.cy) / a.s, Xh = (X - a.cx) / a.s, Yh = (Y - a.cy) / a.s;
            const double xx = xh * xh, xy = xh * yh, yy = yh * yh, q = Xh * Xh + Yh * Yh;
            acc[0] += w * xx;
            acc[1] += w * xy;
            acc[2] += w * yy;
            acc[3] += w * xh;
            acc[4] += w * yh;
            acc[5] += w;
            acc[6] += w * (xx * Xh);
            acc[7] += w * (xy * Xh);
            acc[8] += w * (yy * Xh);
            acc[9] += w * (xh * Xh);
            acc[10] += w * (yh * Xh);
            acc[11] += w * Xh;
            acc[12] += w * (xx * Yh);
            acc[13] += w * (xy * Yh);
            acc[14] += w * (yy * Yh);
            acc[15] += w * (xh * Yh);
            acc[16] += w * (yh * Yh);
            acc[17] += w * Yh;
            acc[18] += w * (xx * q);
            acc[19] += w * (xy * q);
            acc[20] += w * (yy * q);
            acc[21] += w * (xh * q);
            acc[22] += w * (yh * q);
            acc[24] += c;
        }
    }
    wave_sum_of(acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kHSums; k++) red[threadIdx.y][k] = acc[k];
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < kHSums) {
        const int k = threadIdx.x;
        a.part[(i * a.blocks + tile) * kHRow + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// the pixel-coordinate homography m (m[8] = 1) of the normalised sums S (include/papof.h); false where the iteration fails
__device__ bool homography_solve(const double (&S)[kHSums], double cx, double cy, double s, double W1, double H1,
                                 double (&m)[9]) {
    const double sw = S[5];
    if (!(sw > 0)) return false;
    double g[8][9] = {{S[0], S[1], S[3], 0.0, 0.0, 0.0, -S[6], -S[7], S[9]},
                      {S[1], S[2], S[4], 0.0, 0.0, 0.0, -S[7], -S[8], S[10]},
                      {S[3], S[4], S[5], 0.0, 0.0, 0.0, -S[9], -S[10], S[11]},
                      {0.0, 0.0, 0.0, S[0], S[1], S[3], -S[12], -S[13], S[15]},
                      {0.0, 0.0, 0.0, S[1], S[2], S[4], -S[13], -S[14], S[16]},
                      {0.0, 0.0, 0.0, S[3], S[4], S[5], -S[15], -S[16], S[17]},
                      {-S[6], -S[7], -S[9], -S[12], -S[13], -S[15], S[18], S[19], -S[21]},
                      {-S[7], -S[8], -S[10], -S[13], -S[14], -S[16], S[19], S[20], -S[22]}};
    double p[1][8];
    if (!eliminate<8, 1>(g, 1e-12 * sw, p)) return false;
    const double hn[3][3] = {{p[0][0], p[0][1], p[0][2]}, {p[0][3], p[0][4], p[0][5]}, {p[0][6], p[0][7], 1.0}};
    // M = T^-1 Hn T up to the factor s: A = Hn (s T), then T^-1 A, then every entry over the last
    double A[3][3];
    for (int r = 0; r < 3; r++) {
        A[r][0] = hn[r][0];
        A[r][1] = hn[r][1];
        A[r][2] = s * hn[r][2] - (hn[r][0] * cx + hn[r][1] * cy);
    }
    const double z = A[2][2];
    if (!(z > 0)) return false;
    for (int c = 0; c < 3; c++) {
        m[c] = (s * A[0][c] + cx * A[2][c]) / z;
        m[3 + c] = (s * A[1][c] + cy * A[2][c]) / z;
        m[6 + c] = A[2][c] / z;
    }
    for (int k = 0; k < 9; k++)
        if (!isfinite(m[k])) return false;
    // the denominator at the four image corners: the fitted motion keeps the whole image in front of its horizon
    return m[8] > 0 && m[6] * W1 + m[8] > 0 && m[7] * H1 + m[8] > 0 && (m[6] * W1 + m[7] * H1) + m[8] > 0;
}

// SolveArgs as k_motion_solve takes them (model unused); motion is (pair, 3, 3)
__global__ __launch_bounds__(64) void k_homography_solve(const SolveArgs a, double W1, double H1) {
    const long long i = blockIdx.x;
    double* st = a.state + i * kHState;
    if (a.iter > 0 && st[10] != 0.0) return;
    const double* p = a.part + i * a.blocks * kHRow;
    double acc[kHSums];
#pragma unroll
    for (int k = 0; k < kHSums; k++) acc[k] = 0.0;
    for (long long b = threadIdx.x; b < a.blocks; b += 64)
#pragma unroll
        for (int k = 0; k < kHSums; k++) acc[k] += p[b * kHRow + k];
    wave_sum_of(acc);
    if (threadIdx.x != 0) return;
    double m[9];
    if (homography_solve(acc, a.cx, a.cy, a.s, W1, H1, m)) {
        for (int k = 0; k < 9; k++) st[k] = m[k];
        st[9] = 1.0;
        st[10] = 0.0;
    } else if (a.iter == 0) {  // the identity, ok = 0, no further iterations
        for (int k = 0; k < 9; k++) st[k] = k % 4 == 0 ? 1.0 : 0.0;
        st[9] = 0.0;
        st[10] = 1.0;
    }  // else: the last successful iteration's matrix stays
    double* mo = static_cast<double*>(a.motion.data) + i * a.motion.stride[0];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) mo[r * a.motion.stride[1] + c * a.motion.stride[2]] = st[3 * r + c];
    static_cast<unsigned char*>(a.ok.data)[i * a.ok.stride[0]] = st[9] != 0.0 ? 1 : 0;  // (store_u8 evaluates the value first: other schedule)
    static_cast<double*>(a.support.data)[i * a.support.stride[0]] = acc[24] / a.hw;
}

int launch_homography_fit(hipStream_t st, FitArgs f, SolveArgs s, int n_pairs, int n_iter) {
    for (int it = 0; it < n_iter; it++) {
        f.iter = s.iter = it;
        PAPOF_TRY(launch_tiles(f.blocks, n_pairs, [&](dim3 grid, long long, long long p0) {  // (blocks <= kMaxTiles)
            hipLaunchKernelGGL(k_homography_sums, grid, FitTile::block(), 0, st, f, p0);
        }));
        hipLaunchKernelGGL(k_homography_solve, dim3((unsigned)n_pairs), dim3(64), 0, st, s, (double)(f.W - 1), (double)(f.H - 1));
        PAPOF_HIP(hipGetLastError());
    }
    return PAPOF_OK;
}

struct WarpArgs {
    papof_tensor fr;     // (frame, row, column, channel)
    papof_tensor mat;    // float32 / float64 (frame, row, column): 2 x 3
    papof_tensor out;    // (frame, row, column, channel)
    papof_tensor valid;  // uint8 (frame, row, column); data NULL: none
    int H, W, C;
};

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y
template <int FD>
__global__ __launch_bounds__(kWarpTX* kWarpTY) void k_warp_affine(const WarpArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kWarpTX>(lut);
    const long long i = frame0 + blockIdx.y;
    const long long mb = i * a.mat.stride[0];
    double m[6];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) m[3 * r + c] = load_flow(a.mat, mb + r * a.mat.stride[1] + c * a.mat.stride[2]);
    PAPOF_TILE_PIXEL(WarpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const double xd = (double)x, rd = (double)r;
    const double X = (m[0] * xd + m[1] * rd) + m[2], Y = (m[3] * xd + m[4] * rd) + m[5];
    const bool in = X >= 0 && X <= (double)(a.W - 1) && Y >= 0 && Y <= (double)(a.H - 1);  // (false for a NaN)
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

int launch_warp(hipStream_t st, const WarpArgs& a, int n_frames) {
    const int fd = a.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_warp_affine<fd()>; });
    return launch_grid<WarpTile>(a.H, a.W, n_frames, st, 0, kernel, a);
}

// k_warp_affine's tiling over 3 x 3 matrices: (X, Y) = (Nx / D, Ny / D), inside only where D > 0 (include/papof.h)
template <int FD>
__global__ __launch_bounds__(kWarpTX* kWarpTY) void k_warp_projective(const WarpArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    stage_u8_lut<FD, kWarpTX>(lut);
    const long long i = frame0 + blockIdx.y;
    const long long mb = i * a.mat.stride[0];
    double m[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) m[3 * r + c] = load_flow(a.mat, mb + r * a.mat.stride[1] + c * a.mat.stride[2]);
    PAPOF_TILE_PIXEL(WarpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const double xd = (double)x, rd = (double)r;
    const double D = (m[6] * xd + m[7] * rd) + m[8];
    const double X = ((m[0] * xd + m[1] * rd) + m[2]) / D, Y = ((m[3] * xd + m[4] * rd) + m[5]) / D;
    const bool in = D > 0 && X >= 0 && X <= (double)(a.W - 1) && Y >= 0 && Y <= (double)(a.H - 1);  // (false for a NaN)
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

int launch_warp_projective(hipStream_t st, const WarpArgs& a, int n_frames) {
    const int fd = a.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_warp_projective<fd()>; });
    return launch_grid<WarpTile>(a.H, a.W, n_frames, st, 0, kernel, a);
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_motion_workspace(int n_pairs, int height, int width) {
    if (n_pairs < 1 || height < 1 || width < 1) return -1;
    const long long blocks = fit_blocks(height, width);
    if (blocks > kMaxTiles) return -1;
    return 8LL * n_pairs * (kState + blocks * kRow);
}

extern "C" int papof_motion_fit_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow,
                                       const papof_tensor* occlusion, int model, int n_iter, double scale,
                                       const papof_tensor* motion, const papof_tensor* ok, const papof_tensor* support,
                                       void* workspace, long long workspace_bytes, void* stream) {
    if (!h || n_pairs < 1 || height < 1 || width < 1 || n_iter < 1) return PAPOF_EINVAL;
    if (model != PAPOF_MOTION_SIMILARITY && model != PAPOF_MOTION_AFFINE) return PAPOF_EINVAL;
    if (!std::isfinite(scale) || !(scale > 0)) return PAPOF_EINVAL;
    if (!in_flow(flow)) return PAPOF_EINVAL;
    if (!opt_in_mask(occlusion)) return PAPOF_EINVAL;
    if (!described(motion, {PAPOF_DTYPE_F64}, {0, 1, 2}, true) || !described(ok, {PAPOF_DTYPE_U8}, {0}, true) ||
        !described(support, {PAPOF_DTYPE_F64}, {0}, true))
        return PAPOF_EINVAL;
    const long long need = papof_motion_workspace(n_pairs, height, width);
    if (need < 0 || !workspace || workspace_bytes < need) return PAPOF_EINVAL;
    const double cx = (width - 1) / 2.0, cy = (height - 1) / 2.0, s = std::max(width, height) / 2.0;
    FitArgs f{};
    f.flow = *flow;
    if (occlusion) f.occ = *occlusion;
    f.state = static_cast<const double*>(workspace);
    f.part = static_cast<double*>(workspace) + (long long)n_pairs * kState;
    f.blocks = fit_blocks(height, width);
    f.H = height;
    f.W = width;
    f.cx = cx;
    f.cy = cy;
    f.s = s;
    f.c2 = scale * scale;
    SolveArgs sa{};
    sa.state = static_cast<double*>(workspace);
    sa.part = f.part;
    sa.motion = *motion;
    sa.ok = *ok;
    sa.support = *support;
    sa.blocks = f.blocks;
    sa.model = model;
    sa.cx = cx;
    sa.cy = cy;
    sa.s = s;
    sa.hw = (double)height * (double)width;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_fit(static_cast<hipStream_t>(stream), f, sa, n_pairs, n_iter);
}

extern "C" int papof_warp_affine_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                        const papof_tensor* frames, const papof_tensor* matrices, const papof_tensor* out,
                                        const papof_tensor* valid, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1) return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (!described(matrices, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!opt_out_mask(valid)) return PAPOF_EINVAL;
    WarpArgs a{};
    a.fr = *frames;
    a.mat = *matrices;
    a.out = *out;
    if (valid) a.valid = *valid;
    a.H = height;
    a.W = width;
    a.C = c;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_warp(static_cast<hipStream_t>(stream), a, n_frames);
}

extern "C" long long papof_homography_workspace(int n_pairs, int height, int width) {
    if (n_pairs < 1 || height < 1 || width < 1) return -1;
    const long long blocks = fit_blocks(height, width);
    if (blocks > kMaxTiles) return -1;
    return 8LL * n_pairs * (kHState + blocks * kHRow);
}

extern "C" int papof_homography_fit_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow,
                                           const papof_tensor* occlusion, int n_iter, double scale, const papof_tensor* motion,
                                           const papof_tensor* ok, const papof_tensor* support, void* workspace,
                                           long long workspace_bytes, void* stream) {
    if (!h || n_pairs < 1 || height < 1 || width < 1 || n_iter < 1) return PAPOF_EINVAL;
    if (!std::isfinite(scale) || !(scale > 0)) return PAPOF_EINVAL;
    if (!in_flow(flow)) return PAPOF_EINVAL;
    if (!opt_in_mask(occlusion)) return PAPOF_EINVAL;
    if (!described(motion, {PAPOF_DTYPE_F64}, {0, 1, 2}, true) || !described(ok, {PAPOF_DTYPE_U8}, {0}, true) ||
        !described(support, {PAPOF_DTYPE_F64}, {0}, true))
        return PAPOF_EINVAL;
    const long long need = papof_homography_workspace(n_pairs, height, width);
    if (need < 0 || !workspace || workspace_bytes < need) return PAPOF_EINVAL;
    FitArgs f{};
    f.flow = *flow;
    if (occlusion) f.occ = *occlusion;
    f.state = static_cast<const double*>(workspace);
    f.part = static_cast<double*>(workspace) + (long long)n_pairs * kHState;
    f.blocks = fit_blocks(height, width);
    f.H = height;
    f.W = width;
    f.cx = (width - 1) / 2.0;
    f.cy = (height - 1) / 2.0;
    f.s = std::max(width, height) / 2.0;
    f.c2 = scale * scale;
    SolveArgs sa{};
    sa.state = static_cast<double*>(workspace);
    sa.part = f.part;
    sa.motion = *motion;
    sa.ok = *ok;
    sa.support = *support;
    sa.blocks = f.blocks;
    sa.cx = f.cx;
    sa.cy = f.cy;
    sa.s = f.s;
    sa.hw = (double)height * (double)width;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_homography_fit(static_cast<hipStream_t>(stream), f, sa, n_pairs, n_iter);
}

extern "C" int papof_warp_projective_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                            const papof_tensor* frames, const papof_tensor* matrices, const papof_tensor* out,
                                            const papof_tensor* valid, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1) return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (!described(matrices, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!opt_out_mask(valid)) return PAPOF_EINVAL;
    WarpArgs a{};
    a.fr = *frames;
    a.mat = *matrices;
    a.out = *out;
    if (valid) a.valid = *valid;
    a.H = height;
    a.W = width;
    a.C = c;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_warp_projective(static_cast<hipStream_t>(stream), a, n_frames);
}
