// papteam_opticalflow_amd/csrc/mesh.hip -- spatially varying stabilization (SteadyFlow, Liu et al. CVPR 2014; MeshFlow, Liu
// et al. ECCV 2016): the robust motion of a flow field at the vertices of a coarse mesh (papof_mesh_motion_tensor) and the
// affine warp of frames plus a bilinearly interpolated displacement mesh (papof_warp_mesh_tensor).
//
// Semantics: include/papof.h, papof_mesh_motion_tensor and papof_warp_mesh_tensor.  fp64 without contraction
// (-ffp-contract=off).
//
// Medians.  k_mesh_median: one block of 256 lanes per (vertex, pair) (blockIdx.x the vertex in row-major order, blockIdx.y
// the pair).  Lane t computes the residuals of the window's samples t, t + 256, t + 512, t + 768 (at most kMeshSamples = 1024
// per window: the host chooses the lattice step so) and stores their order-preserving integer keys in LDS -- the largest key
// for a sample that does not count --, the block counts the valid samples with the barrier's population count, and every
// lane counts, for each of its samples, the samples before it in the order (key, sample index): the sample whose count is
// the rank (n - 1) / 2 writes its bits.  Every rank is held by exactly one sample, so there is one writer, no atomics, and
// the result depends on nothing but the pair's own flow: bitwise reproducible, alone or in a batch.  k_mesh_spatial, behind
// it on the stream: one lane per (vertex, pair) selects the lower median of the valid medians of the 3 x 3 vertex
// neighbourhood the same way (at most nine keys in registers), or passes the vertex's own, and adds the global motion at the
// vertex.
//
// Warp.  k_warp_mesh: k_warp_affine's 64 x 4 tiling and dtype instances.  The block stages its frame's displacement table in
// LDS once (meshes of at most kMeshStaged vertices: 33 x 33, 17 KB; larger ones, up to 65 x 65, are read from global memory
// -- the table of a frame is small enough to stay in the cache), each lane finds its cell, interpolates the four vertex
// displacements and samples with sampler.h's bilinear rule.
#include "sampler.h"

#include <algorithm>
#include <cmath>

namespace papof {

namespace {

constexpr int kMeshLanes = 256;                      // lanes of a k_mesh_median block
constexpr int kMeshRounds = 4;                       // samples per lane
constexpr int kMeshSamples = kMeshLanes * kMeshRounds;  // include/papof.h: at most 1024 samples per window
constexpr int kMeshStaged = 33 * 33;                 // vertices of a table that k_warp_mesh stages in LDS
constexpr int kWarpTX = 64, kWarpTY = 4;             // a 64 x 4 tile of output pixels per block (256 lanes: lut)
using WarpTile = Tile<kWarpTX, kWarpTY>;
constexpr long long kKeyNone = 0x7fffffffffffffffLL; // the key of a sample that does not count (a NaN's: NaNs do not count)

// the bits of a double as a signed integer that orders as the double does (-0 before +0), and back
__device__ __forceinline__ long long key_of(double v) {
    const long long b = __double_as_longlong(v);
    return b ^ ((b >> 63) & 0x7fffffffffffffffLL);
}
__device__ __forceinline__ double value_of(long long k) { return __longlong_as_double(k ^ ((k >> 63) & 0x7fffffffffffffffLL)); }

struct MeshArgs {
    papof_tensor flow;     // (pair, row, column, {vx, vy})
    papof_tensor occ;      // uint8 (pair, row, column); data NULL: none
    papof_tensor mat;      // float64 (pair, row, column): 2 x 3; data NULL: the identity
    double* raw;           // workspace (pair, vertex, {x, y}): the window medians of the residuals
    papof_tensor vert;     // float64 (pair, vertex row, vertex column, {x, y})
    papof_tensor resid;    // float64, as vert
    int* support;          // (pair, vertex), dense
    int H, W, GH, GW;
    int step;
    int min_support;
    int spatial;
};

__device__ __forceinline__ void load_matrix(const papof_tensor& mat, long long pair, double (&m)[6]) {
    m[0] = 1.0, m[1] = 0.0, m[2] = 0.0, m[3] = 0.0, m[4] = 1.0, m[5] = 0.0;
    if (!mat.data) return;
    const double* p = static_cast<const double*>(mat.data) + pair * mat.stride[0];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) m[3 * r + c] = p[r * mat.stride[1] + c * mat.stride[2]];
}

// the first and last lattice coordinate and the number of them in the window of vertex index v of G cells on N pixels
__device__ __forceinline__ void window_axis(int v, int G, int N, int step, int& first, int& count) {
    const long long n1 = N - 1;
    const long long lo = v == 0 ? 0 : ((v - 1) * n1 + G - 1) / G;         // ceil((v - 1) (N - 1) / G)
    const long long hi = std::min(n1, ((long long)(v + 1) * n1) / G);     // floor((v + 1) (N - 1) / G), clipped
    const long long f = ((lo + step - 1) / step) * step;
    first = (int)f;
    count = f <= hi ? (int)((hi - f) / step) + 1 : 0;
}

// blockIdx.x: the vertex, row-major over (GH + 1) x (GW + 1); blockIdx.y: pair `pair0` + y
__global__ __launch_bounds__(kMeshLanes) void k_mesh_median(const MeshArgs a, long long vertex0, long long pair0) {
    __shared__ long long key[2][kMeshSamples];
    const long long b = pair0 + blockIdx.y;
    const int vertex = (int)(vertex0 + blockIdx.x), VW = a.GW + 1;
    const int vi = vertex / VW, vj = vertex % VW;
    const int tid = threadIdx.x;
    double m[6];
    load_matrix(a.mat, b, m);
    int xs, nx, ys, ny;
    window_axis(vj, a.GW, a.W, a.step, xs, nx);
    window_axis(vi, a.GH, a.H, a.step, ys, ny);
    const int total = std::min(nx * ny, kMeshSamples);  // (the step keeps nx * ny <= kMeshSamples: include/papof.h)
    const double W1 = (double)(a.W - 1), H1 = (double)(a.H - 1);
    long long mine[2][kMeshRounds];
    int n = 0;
#pragma unroll
    for (int r = 0; r < kMeshRounds; r++) {
        const int k = tid + r * kMeshLanes;
        bool valid = false;
        double rx = 0.0, ry = 0.0;
        if (k < total) {
            const int x = xs + (k % nx) * a.step;
            const long long y = ys + (k / nx) * a.step;
            const long long o = PAPOF_AT(a.flow, b, y, x);
            const double u = load_flow(a.flow, o), v = load_flow(a.flow, o + a.flow.stride[3]);
            const double xd = (double)x, yd = (double)y, X = xd + u, Y = yd + v;
            valid = X >= 0 && X <= W1 && Y >= 0 && Y <= H1;  // false for a NaN or an infinity
            if (valid && a.occ.data)
                valid = load_u8(a.occ, PAPOF_AT(a.occ, b, y, x)) == 0;
            rx = u - (((m[0] * xd + m[1] * yd) + m[2]) - xd);
            ry = v - (((m[3] * xd + m[4] * yd) + m[5]) - yd);
            valid = valid && rx == rx && ry == ry;  // (a NaN only through a matrix that is not finite)
        }
        mine[0][r] = valid ? key_of(rx) : kKeyNone;
        mine[1][r] = valid ? key_of(ry) : kKeyNone;
        key[0][k] = mine[0][r];
        key[1][k] = mine[1][r];
        n += __syncthreads_count(valid);  // (the last one is the barrier behind the keys)
    }
    const long long out = (b * (a.GH + 1) * VW + vertex) * 2;
    if (tid == 0) {
        a.support[b * (a.GH + 1) * VW + vertex] = n;
        if (n == 0) a.raw[out] = a.raw[out + 1] = 0.0;
    }
    if (n == 0) return;
    const int rank = (n - 1) / 2;
    int before[2][kMeshRounds];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int r = 0; r < kMeshRounds; r++) before[c][r] = 0;
    for (int j = 0; j < total; j++) {
        const long long kx = key[0][j], ky = key[1][j];  // (one address per wave: a broadcast)
#pragma unroll
        for (int r = 0; r < kMeshRounds; r++) {
            const int k = tid + r * kMeshLanes;
            before[0][r] += (kx < mine[0][r] || (kx == mine[0][r] && j < k)) ? 1 : 0;
            before[1][r] += (ky < mine[1][r] || (ky == mine[1][r] && j < k)) ? 1 : 0;
        }
    }
#pragma unroll
    for (int r = 0; r < kMeshRounds; r++) {
        // (a sample that does not count has the largest key: at least n samples come before it, never `rank`)
        if (mine[0][r] != kKeyNone && before[0][r] == rank) a.raw[out] = value_of(mine[0][r]);
        if (mine[1][r] != kKeyNone && before[1][r] == rank) a.raw[out + 1] = value_of(mine[1][r]);
    }
}

// the lower median of k[0 .. n), 1 <= n <= 9, in the order (key, index)
__device__ __forceinline__ long long lower_median9(const long long (&k)[9], int n) {
    const int rank = (n - 1) / 2;
    long long got = k[0];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        int before = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) before += (j < n && (k[j] < k[i] || (k[j] == k[i] && j < i))) ? 1 : 0;
        if (i < n && before == rank) got = k[i];
    }
    return got;
}

// a lane per vertex: blockIdx.x * 64 + threadIdx.x the vertex, blockIdx.y: pair `pair0` + y
__global__ __launch_bounds__(64) void k_mesh_spatial(const MeshArgs a, long long block0, long long pair0) {
    const long long b = pair0 + blockIdx.y;
    const int VW = a.GW + 1, VH = a.GH + 1;
    const long long vertex = (block0 + blockIdx.x) * 64 + threadIdx.x;
    if (vertex >= (long long)VW * VH) return;
    const int vi = (int)(vertex / VW), vj = (int)(vertex % VW);
    const int* sup = a.support + b * VH * VW;
    const double* raw = a.raw + b * VH * VW * 2;
    double rx = 0.0, ry = 0.0;
    if (a.spatial) {
        long long kx[9], ky[9];
        int n = 0;
#pragma unroll
        for (int di = -1; di <= 1; di++)
#pragma unroll
            for (int dj = -1; dj <= 1; dj++) {
                const int i = vi + di, j = vj + dj;
                const bool in = i >= 0 && i < VH && j >= 0 && j < VW;
                const bool ok = in && sup[(in ? i : 0) * VW + (in ? j : 0)] >= a.min_support;
                const long long o = ((long long)(in ? i : 0) * VW + (in ? j : 0)) * 2;
                const long long cx = key_of(raw[o]), cy = key_of(raw[o + 1]);
                // the valid neighbours packed to the front, in (di, dj) order (unrolled: registers, no indexed array)
#pragma unroll
                for (int s = 0; s < 9; s++)
                    if (ok && s == n) kx[s] = cx, ky[s] = cy;
                n += ok ? 1 : 0;
            }
#pragma unroll
        for (int s = 0; s < 9; s++)
            if (s >= n) kx[s] = ky[s] = kKeyNone;
        if (n > 0) {
            rx = value_of(lower_median9(kx, n));
            ry = value_of(lower_median9(ky, n));
        }
    } else if (sup[vertex] >= a.min_support) {
        rx = raw[vertex * 2];
        ry = raw[vertex * 2 + 1];
    }
    double m[6];
    load_matrix(a.mat, b, m);
    const double px = ((double)vj * (double)(a.W - 1)) / (double)a.GW, py = ((double)vi * (double)(a.H - 1)) / (double)a.GH;
    const double gx = ((m[0] * px + m[1] * py) + m[2]) - px, gy = ((m[3] * px + m[4] * py) + m[5]) - py;
    const long long orr = PAPOF_AT(a.resid, b, vi, vj);
    static_cast<double*>(a.resid.data)[orr] = rx;
    static_cast<double*>(a.resid.data)[orr + a.resid.stride[3]] = ry;
    const long long ov = PAPOF_AT(a.vert, b, vi, vj);
    static_cast<double*>(a.vert.data)[ov] = rx + gx;
    static_cast<double*>(a.vert.data)[ov + a.vert.stride[3]] = ry + gy;
}

// include/papof.h: the smallest step for which a window holds at most kMeshSamples samples
int mesh_step(int H, int W, int GH, int GW) {
    const long long Lx = (2LL * (W - 1)) / GW, Ly = (2LL * (H - 1)) / GH;
    long long s = 1;
    while ((Lx / s + 1) * (Ly / s + 1) > kMeshSamples) s++;
    return (int)s;
}

struct WarpMeshArgs {
    papof_tensor fr;     // (frame, row, column, channel)
    papof_tensor mat;    // float32 / float64 (frame, row, column): 2 x 3
    papof_tensor mesh;   // float64 (frame, vertex row, vertex column, {dx, dy})
    papof_tensor out;    // (frame, row, column, channel)
    papof_tensor valid;  // uint8 (frame, row, column); data NULL: none
    int H, W, C, GH, GW;
};

// grid.h's grid over the frame's 64 x 4 tiles; blockIdx.y: frame `frame0` + y.  STAGED: the
// frame's table is copied to LDS, (vertex row, vertex column, {dx, dy}) dense
template <int FD, bool STAGED>
__global__ __launch_bounds__(kWarpTX* kWarpTY) void k_warp_mesh(const WarpMeshArgs a, long long tile0, long long frame0) {
    __shared__ double lut[256];
    __shared__ double table[STAGED ? kMeshStaged * 2 : 1];
    const int lane = threadIdx.y * kWarpTX + threadIdx.x;
    const long long i = frame0 + blockIdx.y;
    const int VW = a.GW + 1, VH = a.GH + 1;
    const double* mesh = static_cast<const double*>(a.mesh.data) + i * a.mesh.stride[0];
    if (FD == PAPOF_DTYPE_U8 || FD < 0) fill_u8_lut(lut, lane);  // (256 lanes: one quotient each)
    if (STAGED)
        for (int e = lane; e < VH * VW * 2; e += kWarpTX * kWarpTY) {
            const int v = e >> 1;
            table[e] = mesh[(v / VW) * a.mesh.stride[1] + (v % VW) * a.mesh.stride[2] + (e & 1) * a.mesh.stride[3]];
        }
    if (STAGED || FD == PAPOF_DTYPE_U8 || FD < 0) __syncthreads();
    const long long mb = i * a.mat.stride[0];
    double m[6];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) m[3 * r + c] = load_flow(a.mat, mb + r * a.mat.stride[1] + c * a.mat.stride[2]);
    PAPOF_TILE_PIXEL(WarpTile, tile0, a.W, int, x, long long, r);
    if (x >= a.W || r >= a.H) return;
    const double xd = (double)x, rd = (double)r;
    const double X0 = (m[0] * xd + m[1] * rd) + m[2], Y0 = (m[3] * xd + m[4] * rd) + m[5];
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
            double tdx, tdy;
            if (STAGED) {
                const int e = ((ci + nn) * VW + (cj + mm)) * 2;
                tdx = table[e];
                tdy = table[e + 1];
            } else {
                const long long e = (ci + nn) * a.mesh.stride[1] + (cj + mm) * a.mesh.stride[2];
                tdx = mesh[e];
                tdy = mesh[e + a.mesh.stride[3]];
            }
            dx += tdx * w;
            dy += tdy * w;
        }
    const double X = X0 + dx, Y = Y0 + dy;
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

template <bool STAGED>
int launch_warp_mesh(hipStream_t st, const WarpMeshArgs& a, int n_frames) {
    const int fd = a.fr.dtype;
    const auto kernel = by_dtype(fd, [](auto fd) { return k_warp_mesh<fd(), STAGED>; });
    return launch_grid<WarpTile>(a.H, a.W, n_frames, st, 0, kernel, a);
}

bool valid_grid(int height, int width, int gh, int gw) {
    return gh >= 1 && gw >= 1 && gh <= PAPOF_MESH_MAX_CELLS && gw <= PAPOF_MESH_MAX_CELLS && gh <= height - 1 && gw <= width - 1;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" long long papof_mesh_workspace(int n_pairs, int grid_rows, int grid_cols) {
    if (n_pairs < 1 || grid_rows < 1 || grid_cols < 1 || grid_rows > PAPOF_MESH_MAX_CELLS || grid_cols > PAPOF_MESH_MAX_CELLS)
        return -1;
    return 16LL * n_pairs * (grid_rows + 1) * (grid_cols + 1);
}

extern "C" int papof_mesh_motion_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow,
                                        const papof_tensor* occlusion, const papof_tensor* motion, int grid_rows, int grid_cols,
                                        int min_support, int spatial, const papof_tensor* vertices,
                                        const papof_tensor* residuals, int* support, void* workspace,
                                        long long workspace_bytes, void* stream) {
    if (!h || n_pairs < 1 || height < 1 || width < 1 || min_support < 1) return PAPOF_EINVAL;
    if (!valid_grid(height, width, grid_rows, grid_cols)) return PAPOF_EINVAL;
    if (!in_flow(flow)) return PAPOF_EINVAL;
    if (!opt_in_mask(occlusion)) return PAPOF_EINVAL;
    if (motion && !described(motion, {PAPOF_DTYPE_F64}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!described(vertices, {PAPOF_DTYPE_F64}, {0, 1, 2, 3}, true) || !described(residuals, {PAPOF_DTYPE_F64}, {0, 1, 2, 3}, true) ||
        !support)
        return PAPOF_EINVAL;
    const long long need = papof_mesh_workspace(n_pairs, grid_rows, grid_cols);
    if (need < 0 || !workspace || workspace_bytes < need) return PAPOF_EINVAL;
    MeshArgs a{};
    a.flow = *flow;
    if (occlusion) a.occ = *occlusion;
    if (motion) a.mat = *motion;
    a.raw = static_cast<double*>(workspace);
    a.vert = *vertices;
    a.resid = *residuals;
    a.support = support;
    a.H = height;
    a.W = width;
    a.GH = grid_rows;
    a.GW = grid_cols;
    a.step = mesh_step(height, width, grid_rows, grid_cols);
    a.min_support = min_support;
    a.spatial = spatial != 0;
    PAPOF_HIP(hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long V = (long long)(grid_rows + 1) * (grid_cols + 1);
    PAPOF_TRY(launch_tiles(V, n_pairs, [&](dim3 grid, long long v0, long long p0) {
        hipLaunchKernelGGL(k_mesh_median, grid, dim3(kMeshLanes), 0, st, a, v0, p0);
    }));
    return launch_tiles((V + 63) / 64, n_pairs, [&](dim3 grid, long long b0, long long p0) {
        hipLaunchKernelGGL(k_mesh_spatial, grid, dim3(64), 0, st, a, b0, p0);
    });
}

extern "C" int papof_warp_mesh_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                      const papof_tensor* matrices, const papof_tensor* mesh, int grid_rows, int grid_cols,
                                      const papof_tensor* out, const papof_tensor* valid, void* stream) {
    if (!h || n_frames < 1 || height < 1 || width < 1 || c < 1) return PAPOF_EINVAL;
    if (!valid_grid(height, width, grid_rows, grid_cols)) return PAPOF_EINVAL;
    if (!in_frames(frames) || !out_frames(out)) return PAPOF_EINVAL;
    if (!described(matrices, {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, {0, 1, 2}, false)) return PAPOF_EINVAL;
    if (!described(mesh, {PAPOF_DTYPE_F64}, {0, 1, 2, 3}, false)) return PAPOF_EINVAL;
    if (!opt_out_mask(valid)) return PAPOF_EINVAL;
    WarpMeshArgs a{};
    a.fr = *frames;
    a.mat = *matrices;
    a.mesh = *mesh;
    a.out = *out;
    if (valid) a.valid = *valid;
    a.H = height;
    a.W = width;
    a.C = c;
    a.GH = grid_rows;
    a.GW = grid_cols;
    PAPOF_HIP(hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((grid_rows + 1) * (grid_cols + 1) <= kMeshStaged) return launch_warp_mesh<true>(st, a, n_frames);
    return launch_warp_mesh<false>(st, a, n_frames);
}
