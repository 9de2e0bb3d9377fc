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
// k_match: a block is a 32 x 8 tile of coarse pixels (blockIdx.x the tile, blockIdx.y the item), one lane per pixel.  A's
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
#include "sampler.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace papof {

namespace {

constexpr int kTX = 32, kTY = 8;  // the tile of coarse pixels (256 lanes)
constexpr int kG = 4;             // candidates along dx that a lane evaluates together (1, 8, 16)
constexpr int kMaxPatch = 7, kMaxSearch = 32, kMaxPenalty = 65535;

inline bool valid_stride(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }

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
    const long long base = f * a.in.stride[0] + (long long)y * s * a.in.stride[1] + (long long)x * s * a.in.stride[2];
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

struct MatchArgs {
    const unsigned* packed;  // [frame][h][w]
    papof_tensor disp;       // (item, row, column, {dx, dy})
    papof_tensor cost;       // (item, row, column, -)
    int h, w, stride, search, penalty;
    int n_pairs, seq;
};

// P: the patch radius.  blockIdx.x: tile `tile0` + x of the grid's 32 x 8 tiles in row-major order; blockIdx.y: item
// `item0` + y -- items below n_pairs run forward (A the pair's first frame), the others backward.
template <int P>
__global__ __launch_bounds__(kTX* kTY) void k_match(const MatchArgs a, long long tile0, long long item0) {
    extern __shared__ __align__(16) unsigned smem_match[];
    constexpr int WN = 2 * P + 1;
    const int s = a.search, h = a.h, w = a.w, ng = groups_of(s);
    const int AW = a_width(P), AH = a_height(P), BW = b_width(P, s), BH = b_height(P, s);
    unsigned* const As = smem_match;
    unsigned* const Bs = As + AW * AH;

    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y, tid = ly * kTX + lx;
    const long long tx = (w + kTX - 1) / kTX, tile = tile0 + blockIdx.x;
    const int x0 = (int)(tile % tx) * kTX, y0 = (int)(tile / tx) * kTY;
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
    const long long od = item * a.disp.stride[0] + (long long)y * a.disp.stride[1] + (long long)x * a.disp.stride[2];
    store(a.disp, od, (double)(a.stride * bdx));
    store(a.disp, od + a.disp.stride[3], (double)(a.stride * bdy));
    store(a.cost, item * a.cost.stride[0] + (long long)y * a.cost.stride[1] + (long long)x * a.cost.stride[2],
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
    const long long od = i * a.disp.stride[0] + (long long)y * a.disp.stride[1] + (long long)x * a.disp.stride[2];
    const double fx = load_flow(a.disp, od), fy = load_flow(a.disp, od + a.disp.stride[3]);
    const double dx = fx / (double)a.stride, dy = fy / (double)a.stride;
    const double qx = (double)x + dx, qy = (double)y + dy;
    // a whole number of cells that lands inside the grid (false for a NaN)
    bool ok = rint(dx) == dx && rint(dy) == dy && qx >= 0 && qx <= (double)(a.w - 1) && qy >= 0 && qy <= (double)(a.h - 1);
    if (ok) {
        const long long orv = i * a.rev.stride[0] + (long long)(int)qy * a.rev.stride[1] + (long long)(int)qx * a.rev.stride[2];
        const double ex = dx + load_flow(a.rev, orv) / (double)a.stride;
        const double ey = dy + load_flow(a.rev, orv + a.rev.stride[3]) / (double)a.stride;
        ok = fabs(ex) <= (double)a.tol && fabs(ey) <= (double)a.tol;
    }
    if (ok && a.max_cost >= 0)
        ok = load_flow(a.cost, i * a.cost.stride[0] + (long long)y * a.cost.stride[1] + (long long)x * a.cost.stride[2]) <= a.max_cost;
    const long long of = i * a.flow.stride[0] + (long long)Y * a.flow.stride[1] + (long long)X * a.flow.stride[2];
    static_cast<double*>(a.flow.data)[of] = ok ? fx : 0.0;
    static_cast<double*>(a.flow.data)[of + a.flow.stride[3]] = ok ? fy : 0.0;
    static_cast<unsigned char*>(a.mask.data)[i * a.mask.stride[0] + (long long)Y * a.mask.stride[1] +
                                             (long long)X * a.mask.stride[2]] = ok ? 0 : 1;
}

bool valid_frame_size(int height, int width, int stride) {
    return valid_stride(stride) && height >= stride && width >= stride && (long long)height * width < (1LL << 30);
}

template <int P>
int launch_match(hipStream_t st, const MatchArgs& a, long long items) {
    const size_t lds = (size_t)lds_bytes(P, a.search);
    const long long tiles = ((a.w + kTX - 1) / (long long)kTX) * ((a.h + kTY - 1) / (long long)kTY);
    return launch_tiles(tiles, items, [&](dim3 grid, long long t0, long long i0) {
        hipLaunchKernelGGL(k_match<P>, grid, dim3(kTX, kTY), lds, st, a, t0, i0);
    });
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
    const auto I = {(int)PAPOF_DTYPE_U8, (int)PAPOF_DTYPE_F32, (int)PAPOF_DTYPE_F64};
    const auto F = {(int)PAPOF_DTYPE_F32, (int)PAPOF_DTYPE_F64};
    if (!described(frames, I, {0, 1, 2, 3}, false) || (!sequence && !described(frames2, I, {0, 1, 2, 3}, false)))
        return PAPOF_EINVAL;
    if (!described(disp, F, {0, 1, 2, 3}, true) || !described(cost, F, {0, 1, 2}, true)) return PAPOF_EINVAL;
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

extern "C" int papof_match_densify_tensor(papof_handle* h, int n, int height, int width, int stride, const papof_tensor* disp,
                                          const papof_tensor* disp_rev, const papof_tensor* cost, int tol, double max_cost,
                                          const papof_tensor* flow, const papof_tensor* mask, void* stream) {
    if (!h || n < 1 || height < 1 || width < 1 || !valid_frame_size(height, width, stride) || tol < 0 || tol > 2 * kMaxSearch ||
        std::isnan(max_cost))
        return PAPOF_EINVAL;
    const auto F = {(int)PAPOF_DTYPE_F32, (int)PAPOF_DTYPE_F64};
    if (!described(disp, F, {0, 1, 2, 3}, false) || !described(disp_rev, F, {0, 1, 2, 3}, false)) return PAPOF_EINVAL;
    if (max_cost >= 0 && !described(cost, F, {0, 1, 2}, false)) return PAPOF_EINVAL;
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
