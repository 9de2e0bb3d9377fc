// papteam_opticalflow_amd/csrc/bundle.hip -- the device half of bundle adjustment for a camera that rotates
// (papof_bundle_sums_tensor): per link (an ordered frame pair with a flow field) the twenty fp64 sums of one robust
// Gauss-Newton evaluation -- the 4 x 4 normal equations in a small rotation of the link and the shared focal length, the cost,
// the weights and the count.
//
// Why.  A chain of pair homographies adds the pairs' errors up.  One joint least-squares fit over every
// overlapping frame pair needs, per evaluation, each link's flow read once and reduced against the link's current rotation;
// everything else -- which frames a link joins, the gauge, the damping, the solve -- is linear algebra on a few hundred
// unknowns and lives on the host (tensors.py: bundle_adjust).  The kernel never knows how many frames there are.
//
// Semantics: include/papof.h, papof_bundle_sums_tensor.  fp64 without contraction (-ffp-contract=off).
//
// Reduction.  motion.hip's, over SAMPLED pixels: no atomics, bitwise reproducible from run to run.  Launch 1 (k_bundle_sums):
// a block is a 64 x 32 tile of sampled pixels of one link (grid.h's grid of tiles and links), a lane one sampled
// column and 8 sampled rows (threadIdx.y + 4 k) in increasing row order; the lanes of a wave are summed by a fixed shuffle
// tree (__shfl_down, 32 .. 1), the four waves in wave order through LDS, and the block writes one row of 32 doubles (twenty
// used) to the workspace.  The link's row of ten doubles (R row-major, f) is read as uniform loads.  Launch 2
// (k_bundle_reduce): one wave per link; lane l adds the rows l, l + 64, l + 128, ... in increasing order, the lanes are summed
// by the same tree, and lanes 0 .. 19 write the link's sums.  Every offset is 64-bit; launch 1 is split at gridDim.y = 65535
// links.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr int kBTX = 64, kBTY = 4, kBRows = 8;  // a lane: one sampled column, kBRows sampled rows kBTY apart
constexpr int kBTH = kBTY * kBRows;             // a block: 64 x 32 sampled pixels
using SampleTile = Tile<kBTX, kBTH, kBTX, kBTY>;  // a strip of kBTH sampled rows under a block of kBTY
constexpr int kBSums = 20;                      // include/papof.h: the order of the sums
constexpr int kBRow = 32;                       // doubles per partial row (kBSums used)

long long sampled(int n, int step) { return (n - 1) / (long long)step + 1; }

long long bundle_blocks(int H, int W, int step) {
    return ((sampled(W, step) + kBTX - 1) / kBTX) * ((sampled(H, step) + kBTH - 1) / kBTH);
}

struct BundleArgs {
    papof_tensor flow;  // (link, row, column, {vx, vy})
    papof_tensor occ;   // uint8 (link, row, column, {fw, bw}); data NULL: none
    papof_tensor rot;   // float64 (link, k): R row-major (9), f
    papof_tensor out;   // float64 (link, k): the twenty sums
    double* part;       // (link, block, kBRow)
    long long blocks;   // per link
    long long Ws, Hs;   // sampled columns and rows
    int H, W, step;
    double cx, cy, c2;
};

__device__ __forceinline__ void wave_sum20(double (&acc)[kBSums]) {  // motion.hip's tree
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < kBSums; k++) acc[k] += __shfl_down(acc[k], off, 64);
}

__global__ __launch_bounds__(kBTX* kBTY) void k_bundle_sums(const BundleArgs a, long long link0) {
    __shared__ double red[kBTY][kBSums];
    const long long i = link0 + blockIdx.y;
    const double* rp = static_cast<const double*>(a.rot.data) + i * a.rot.stride[0];
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rp[k * a.rot.stride[1]];
    const double f = rp[9 * a.rot.stride[1]];
    PAPOF_TILE_PIXEL(SampleTile, 0LL, a.Ws, long long, sx, long long, sr0);  // (one launch holds every strip: blocks <= kMaxTiles)
    double acc[kBSums];
#pragma unroll
    for (int k = 0; k < kBSums; k++) acc[k] = 0.0;
    if (sx < a.Ws) {
        const long long x = sx * a.step;
        const double xd = (double)x, px = (xd - a.cx) / f;
        const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);
        for (int j = 0; j < kBRows; j++) {
            const long long sr = sr0 + (long long)j * kBTY;
            if (sr >= a.Hs) break;
            const long long r = sr * a.step;
            const long long o = PAPOF_AT(a.flow, i, r, x);
            const double u = load_flow(a.flow, o), v = load_flow(a.flow, o + a.flow.stride[3]);
            const double rd = (double)r, X = xd + u, Y = rd + v;
            bool valid = X >= 0 && X <= W1 && Y >= 0 && Y <= H1;  // false for a NaN or an infinity
            if (valid && a.occ.data)
                valid = load_u8(a.occ, PAPOF_AT(a.occ, i, r, x)) == 0;
            if (!valid) continue;
            const double py = (rd - a.cy) / f;
            const double qx = (R[0] * px + R[1] * py) + R[2], qy = (R[3] * px + R[4] * py) + R[5];
            const double qz = (R[6] * px + R[7] * py) + R[8];
            if (!(qz > PAPOF_HOMOGRAPHY_MIN_DEN)) continue;  // at or behind the link's horizon (NaN included)
            const double gx = qx / qz, gy = qy / qz, fgx = f * gx, fgy = f * gy;
            const double ex = X - (fgx + a.cx), ey = Y - (fgy + a.cy);
            const double e2 = ex * ex + ey * ey;
            const double w = 1.0 / (1.0 + e2 / a.c2);
            // the Jacobian of the predicted point in (a_x, a_y, a_z, f): include/papof.h
            const double jx0 = -(fgx * gy), jx1 = f + fgx * gx, jx2 = -fgy, jx3 = gx + (R[2] - gx * R[8]) / qz;
            const double jy0 = -(f + fgy * gy), jy1 = fgx * gy, jy2 = fgx, jy3 = gy + (R[5] - gy * R[8]) / qz;
            acc[0] += w * (jx0 * jx0 + jy0 * jy0);
            acc[1] += w * (jx0 * jx1 + jy0 * jy1);
            acc[2] += w * (jx0 * jx2 + jy0 * jy2);
            acc[3] += w * (jx0 * jx3 + jy0 * jy3);
            acc[4] += w * (jx1 * jx1 + jy1 * jy1);
            acc[5] += w * (jx1 * jx2 + jy1 * jy2);
            acc[6] += w * (jx1 * jx3 + jy1 * jy3);
            acc[7] += w * (jx2 * jx2 + jy2 * jy2);
            acc[8] += w * (jx2 * jx3 + jy2 * jy3);
            acc[9] += w * (jx3 * jx3 + jy3 * jy3);
            acc[10] += w * (jx0 * ex + jy0 * ey);
            acc[11] += w * (jx1 * ex + jy1 * ey);
            acc[12] += w * (jx2 * ex + jy2 * ey);
            acc[13] += w * (jx3 * ex + jy3 * ey);
            acc[14] += w * e2;
            acc[15] += w;
            acc[16] += 1.0;
            acc[17] += e2;
        }
    }
    wave_sum20(acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kBSums; k++) red[threadIdx.y][k] = acc[k];
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < kBSums) {
        const int k = threadIdx.x;
        a.part[(i * a.blocks + tile) * kBRow + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

__global__ __launch_bounds__(64) void k_bundle_reduce(const BundleArgs a) {
    __shared__ double tot[kBSums];
    const long long i = blockIdx.x;
    const double* p = a.part + i * a.blocks * kBRow;
    double acc[kBSums];
#pragma unroll
    for (int k = 0; k < kBSums; k++) acc[k] = 0.0;
    for (long long b = threadIdx.x; b < a.blocks; b += 64)
#pragma unroll
        for (int k = 0; k < kBSums; k++) acc[k] += p[b * kBRow + k];
    wave_sum20(acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kBSums; k++) tot[k] = acc[k];
    __syncthreads();
    if (threadIdx.x < kBSums)
        static_cast<double*>(a.out.data)[i * a.out.stride[0] + threadIdx.x * a.out.stride[1]] = tot[threadIdx.x];
}

int launch_bundle(hipStream_t st, const BundleArgs& a, int n_links) {
    PAPOF_TRY(launch_tiles(a.blocks, n_links, [&](dim3 grid, long long, long long l0) {  // (blocks <= kMaxTiles)
        hipLaunchKernelGGL(k_bundle_sums, grid, SampleTile::block(), 0, st, a, l0);
    }));
    hipLaunchKernelGGL(k_bundle_reduce, dim3((unsigned)n_links), dim3(64), 0, st, a);
    PAPOF_HIP(hipGetLastError());
    return PAPOF_OK;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_bundle_workspace(int n_links, int height, int width, int step) {
    if (n_links < 1 || height < 1 || width < 1 || step < 1) return -1;
    const long long blocks = bundle_blocks(height, width, step);
    if (blocks > kMaxTiles) return -1;
    return 8LL * n_links * blocks * kBRow;
}

extern "C" int papof_bundle_sums_tensor(papof_handle* h, int n_links, int height, int width, int step,
                                        const papof_tensor* flow, const papof_tensor* occlusion,
                                        const papof_tensor* rotations, double scale, const papof_tensor* sums, void* workspace,
                                        long long workspace_bytes, void* stream) {
    if (!h || n_links < 1 || height < 1 || width < 1 || step < 1) return PAPOF_EINVAL;
    if (!std::isfinite(scale) || !(scale > 0)) return PAPOF_EINVAL;
    if (!in_flow(flow)) return PAPOF_EINVAL;
    if (!opt_in_mask(occlusion)) return PAPOF_EINVAL;
    if (!described(rotations, {PAPOF_DTYPE_F64}, {0, 1}, false) || !described(sums, {PAPOF_DTYPE_F64}, {0, 1}, true))
        return PAPOF_EINVAL;
    const long long need = papof_bundle_workspace(n_links, height, width, step);
    if (need < 0 || !workspace || workspace_bytes < need) return PAPOF_EINVAL;
    BundleArgs a{};
    a.flow = *flow;
    if (occlusion) a.occ = *occlusion;
    a.rot = *rotations;
    a.out = *sums;
    a.part = static_cast<double*>(workspace);
    a.blocks = bundle_blocks(height, width, step);
    a.Ws = sampled(width, step);
    a.Hs = sampled(height, step);
    a.H = height;
    a.W = width;
    a.step = step;
    a.cx = (width - 1) / 2.0;
    a.cy = (height - 1) / 2.0;
    a.c2 = scale * scale;
    PAPOF_HIP(hipSetDevice(h->device));
    return launch_bundle(static_cast<hipStream_t>(stream), a, n_links);
}
