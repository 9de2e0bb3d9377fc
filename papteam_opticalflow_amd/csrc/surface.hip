// papteam_opticalflow_amd/csrc/surface.hip -- decoder surfaces: 8-bit YCbCr planes with subsampled chroma (4:2:0, 4:2:2) to
// RGB frames and back (papof_ycc_to_rgb_tensor, papof_rgb_to_ycc_tensor).  The way in and out of every *_video call for
// video that comes from a decoder and goes to an encoder on the device.
//
// Why.  Each user wrote this conversion in PyTorch operations with a siting, matrix, range and rounding of their own, so two
// users' "same video" differed by a few levels before the bit-exact kernels saw it; and interlaced 4:2:0 keeps the chroma of
// each FIELD on alternating chroma lines, which an up-sampling that takes the frame for progressive mixes across two
// instants.  One stated integer rule (include/papof.h) that numpy reproduces to the byte, with the field positions in it.
//
// Semantics: include/papof.h.  The device knows no standard: the host hands it a luma offset and coefficients at 2^14.
//
// Mapping.  k_ycc_to_rgb: one lane per luma pixel, tiles of 64 x 4 (grid.h), blockIdx.y the frame.  A lane reads its luma
// byte and the 2 x 2 chroma samples of its taps from either plane through the descriptors' strides -- nine byte loads, all
// issued before the first product; neighbouring lanes share chroma bytes, which the cache serves -- and writes three elements.
// k_rgb_to_ycc: one lane per CHROMA sample over the Hc x Wc plane: it writes the luma of its 2 x sub_v pixels and reduces the
// per-pixel chroma numerators of its up to 3 x 3 taps in 64-bit integers, one rounding.  Both read and write lane by lane
// through the strides, so NV12, NV21, I420, YV12, NV16, YUY2 and UYVY views, any pitch and any alignment take the same code.
// k_ycc_to_rgb_nv: the instance for what a decoder usually hands over -- interleaved chroma (NV12, NV21, NV16), a width that
// is a multiple of 4, everything dword-aligned, uint8 or float32 out (ycc_fast says exactly when; the host chooses from the
// descriptors).  One lane per FOUR adjacent pixels of a row: the luma as one dword; per chroma row the dword that holds both
// planes' samples 2 i and 2 i + 1 and its two neighbours (three loads where the generic lanes issue sixteen byte loads; the
// neighbours are the adjacent lanes' own dwords and come from the cache); the result as three dwords (uint8 NHWC), one
// dword per plane (uint8 NCHW) or 16-byte stores (float32).  It computes the generic instance's integers: the same bytes.
// Vector stores only; no atomics, no workspace, no LDS, nothing of the handle's memory; every offset 64-bit.
//
// k_ycc16_to_rgb, k_ycc16_to_rgb_nv, k_rgb_to_ycc16 (papof_ycc16_to_rgb_tensor, papof_rgb_to_ycc16_tensor): the same three for
// surfaces of 9 .. 16 bits per sample in 16-bit words (P010, P016, P210, I010, Y210), below the 8-bit kernels, which stay as they
// were.  The same taps, tiles and lane mappings; 64-bit numerators.
#include "cells.h"

namespace papof {

namespace {

using SurfTile = Tile<64, 4>;  // of luma pixels (k_ycc_to_rgb) or of chroma samples (k_rgb_to_ycc)

constexpr int kMaxCoef = 65535;
constexpr int kOne19 = 255 << 19;  // the numerator of 1.0 (level 255) at the scale 2^19

struct YccArgs {
    papof_tensor y, cb, cr, rgb;
    int H, W, Hc, Wc;
    int sub_v, sh, sv, interlaced;
    int y_off, cy, crv, cgu, cgv, cbu;
};

struct RgbArgs {
    papof_tensor rgb, y, cb, cr;
    int H, W, Hc, Wc;
    int sub_v, sh, sv, interlaced;
    int y_off, yr, yg, yb, ur, ug, vg, vb;
};

struct Taps {
    int a, b, wa, wb;  // index a with weight wa, index b with weight wb
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the chroma columns of luma column x and their weights, which add to 4
__device__ __forceinline__ Taps h_taps(int x, int Wc, int sh) {
    const int k = x >> 1, odd = x & 1;
    Taps t;
    if (sh == 0) {
        t.a = k, t.b = k + odd, t.wa = odd ? 2 : 4;
    } else {
        t.a = odd ? k : k - 1, t.b = odd ? k + 1 : k, t.wa = odd ? 3 : 1;
    }
    t.wb = 4 - t.wa;
    t.a = clampi(t.a, 0, Wc - 1), t.b = clampi(t.b, 0, Wc - 1);
    return t;
}

// the rows OF THE CHROMA PLANES of luma row y and their weights, which add to 8
__device__ __forceinline__ Taps v_taps(int y, int Hc, int sub_v, int sv, int interlaced) {
    Taps t;
    if (sub_v == 1) {
        t.a = t.b = y, t.wa = 8;
    } else if (interlaced) {
        const int p = y & 1, m = y >> 2, n = (Hc - p + 1) >> 1;  // n: the field's own chroma rows
        const bool upper = (y & 2) == 0;                           // y = 4 m or 4 m + 1: between samples m - 1 and m
        t.a = upper ? m - 1 : m, t.b = t.a + 1;
        t.wa = (y & 3) * 2 + 1;  // 1, 3, 5, 7 at y & 3 = 0, 1, 2, 3
        t.a = 2 * clampi(t.a, 0, n - 1) + p, t.b = 2 * clampi(t.b, 0, n - 1) + p;
    } else {
        const int j = y >> 1, odd = y & 1;
        if (sv == 0) {
            t.a = odd ? j : j - 1, t.b = t.a + 1, t.wa = odd ? 6 : 2;
        } else {
            t.a = j, t.b = j + odd, t.wa = odd ? 4 : 8;
        }
        t.a = clampi(t.a, 0, Hc - 1), t.b = clampi(t.b, 0, Hc - 1);
    }
    t.wb = 8 - t.wa;
    return t;
}

// clamp((N + 2^18) >> 19, 0, 255), written as the clamp of the sum to 0 .. 2^27 - 1 and then the shift, which is the same
// number.  Shift first and clamp second is the pattern the compiler selects v_ashr_pk_u8_i32 for where two levels are packed,
// and the code it made around that instruction took the upper half of its result for zero: on an MI355X bytes 2 and 3 of a
// packed dword came out ORed with stray bits (tests/test_gpu_surface.py found it).  This form does not select it.
__device__ __forceinline__ unsigned level_u8(int N) { return (unsigned)clampi(N + (1 << 18), 0, (256 << 19) - 1) >> 19; }
__device__ __forceinline__ double level_f64(int N) { return (double)clampi(N, 0, kOne19) / (double)kOne19; }
__device__ __forceinline__ float level_f32(int N) { return (float)level_f64(N); }

template <int OD>
__device__ __forceinline__ void store_level(const papof_tensor& o, long long off, int N) {
    if (OD == PAPOF_DTYPE_U8)
        static_cast<unsigned char*>(o.data)[off] = (unsigned char)level_u8(N);
    else if (OD == PAPOF_DTYPE_F32)
        static_cast<float*>(o.data)[off] = level_f32(N);
    else
        static_cast<double*>(o.data)[off] = level_f64(N);
}

// blockIdx.x: tile `tile0` + x of the luma plane, blockIdx.y: frame `frame0` + y; one lane per luma pixel
template <int OD>
__global__ __launch_bounds__(SurfTile::kX* SurfTile::kY) void k_ycc_to_rgb(const YccArgs a, long long tile0, long long frame0) {
    using T = SurfTile;
    PAPOF_TILE_PIXEL(T, tile0, a.W, int, x, int, r);
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    const Taps hx = h_taps(x, a.Wc, a.sh), vy = v_taps(r, a.Hc, a.sub_v, a.sv, a.interlaced);
    const unsigned char* py = static_cast<const unsigned char*>(a.y.data) + t * a.y.stride[0];
    const unsigned char* pu = static_cast<const unsigned char*>(a.cb.data) + t * a.cb.stride[0];
    const unsigned char* pv = static_cast<const unsigned char*>(a.cr.data) + t * a.cr.stride[0];
    const long long ua = vy.a * a.cb.stride[1], ub = vy.b * a.cb.stride[1], va = vy.a * a.cr.stride[1], vb = vy.b * a.cr.stride[1];
    const long long uxa = hx.a * a.cb.stride[2], uxb = hx.b * a.cb.stride[2], vxa = hx.a * a.cr.stride[2], vxb = hx.b * a.cr.stride[2];
    const int Y = py[r * a.y.stride[1] + x * a.y.stride[2]];
    const int u00 = pu[ua + uxa], u01 = pu[ua + uxb], u10 = pu[ub + uxa], u11 = pu[ub + uxb];
    const int v00 = pv[va + vxa], v01 = pv[va + vxb], v10 = pv[vb + vxa], v11 = pv[vb + vxb];
    const int U = vy.wa * (hx.wa * u00 + hx.wb * u01) + vy.wb * (hx.wa * u10 + hx.wb * u11) - 4096;
    const int V = vy.wa * (hx.wa * v00 + hx.wb * v01) + vy.wb * (hx.wa * v10 + hx.wb * v11) - 4096;
    const int L = 32 * a.cy * (Y - a.y_off);
    const long long o = t * a.rgb.stride[0] + r * a.rgb.stride[1] + x * a.rgb.stride[2], sc = a.rgb.stride[3];
    store_level<OD>(a.rgb, o, L + a.crv * V);
    store_level<OD>(a.rgb, o + sc, L - a.cgu * U - a.cgv * V);
    store_level<OD>(a.rgb, o + 2 * sc, L + a.cbu * U);
}

using NvTile = Tile<256, 4, 64, 4>;  // of luma pixels: a lane owns four adjacent columns of one row

// the four samples 2 i - 1 .. 2 i + 2 of one plane of interleaved chroma, clamped to the row: `cur` is dword i of the row
// (both planes' samples 2 i, 2 i + 1), `prev` and `next` its neighbours, `sh` the plane's first byte (0 or 8 bits)
__device__ __forceinline__ void nv_window(unsigned prev, unsigned cur, unsigned next, bool first, bool last, int sh, int (&w)[4]) {
    w[1] = (int)((cur >> sh) & 255u), w[2] = (int)((cur >> (16 + sh)) & 255u);
    w[0] = first ? w[1] : (int)((prev >> (16 + sh)) & 255u);
    w[3] = last ? w[2] : (int)((next >> sh) & 255u);
}

// 4 times the horizontally interpolated chroma at the lane's four columns 4 i .. 4 i + 3 (h_taps' weights, written out)
__device__ __forceinline__ void nv_across(const int (&w)[4], int sh, int (&h)[4]) {
    if (sh == 0) {
        h[0] = 4 * w[1], h[1] = 2 * w[1] + 2 * w[2], h[2] = 4 * w[2], h[3] = 2 * w[2] + 2 * w[3];
    } else {
        h[0] = w[0] + 3 * w[1], h[1] = 3 * w[1] + w[2], h[2] = w[1] + 3 * w[2], h[3] = 3 * w[2] + w[3];
    }
}

// blockIdx.x: tile `tile0` + x of the luma plane in tiles of 256 x 4, blockIdx.y: frame `frame0` + y.  vu: Cr is the first
// byte of a chroma pair (NV21).  What ycc_fast promises: W % 4 == 0, so a lane's four columns are inside together and a
// chroma row is W / 4 whole dwords; every row of every tensor starts on a dword (float32 out: on 16 bytes).
template <int OD, bool NHWC>
__global__ __launch_bounds__(256) void k_ycc_to_rgb_nv(const YccArgs a, int vu, long long tile0, long long frame0) {
    using T = NvTile;
    PAPOF_TILE_ORIGIN(T, tile0, a.W, int, x0, int, r0);
    const int x = x0 + 4 * (int)threadIdx.x, r = r0 + (int)threadIdx.y;
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    const Taps vy = v_taps(r, a.Hc, a.sub_v, a.sv, a.interlaced);
    const papof_tensor& c = vu ? a.cr : a.cb;  // the plane whose byte comes first
    const unsigned char* pc = static_cast<const unsigned char*>(c.data) + t * c.stride[0];
    const int i = x >> 2, n = a.W >> 2, ip = i > 0 ? i - 1 : 0, in = i + 1 < n ? i + 1 : n - 1;
    const unsigned* ra = reinterpret_cast<const unsigned*>(pc + vy.a * c.stride[1]);
    const unsigned* rb = reinterpret_cast<const unsigned*>(pc + vy.b * c.stride[1]);
    const unsigned yw = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(a.y.data) + t * a.y.stride[0] +
                                                           r * a.y.stride[1] + x);
    const unsigned a0 = ra[ip], a1 = ra[i], a2 = ra[in], b0 = rb[ip], b1 = rb[i], b2 = rb[in];
    int P[2][4];  // 32 times the chroma of the first and of the second plane of the pair, minus 128
    for (int k = 0; k < 2; k++) {
        int wa[4], wb[4], ha[4], hb[4];
        nv_window(a0, a1, a2, i == 0, i == n - 1, 8 * k, wa);
        nv_window(b0, b1, b2, i == 0, i == n - 1, 8 * k, wb);
        nv_across(wa, a.sh, ha);
        nv_across(wb, a.sh, hb);
        for (int d = 0; d < 4; d++) P[k][d] = vy.wa * ha[d] + vy.wb * hb[d] - 4096;
    }
    int N[4][3];
    for (int d = 0; d < 4; d++) {
        const int U = vu ? P[1][d] : P[0][d], V = vu ? P[0][d] : P[1][d];
        const int L = 32 * a.cy * ((int)((yw >> (8 * d)) & 255u) - a.y_off);
        N[d][0] = L + a.crv * V, N[d][1] = L - a.cgu * U - a.cgv * V, N[d][2] = L + a.cbu * U;
    }
    const long long o = t * a.rgb.stride[0] + r * a.rgb.stride[1];
    if (OD == PAPOF_DTYPE_U8 && NHWC) {
        unsigned b[12];
        for (int d = 0; d < 4; d++)
            for (int k = 0; k < 3; k++) b[3 * d + k] = level_u8(N[d][k]);
        unsigned* q = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.rgb.data) + o + 3LL * x);
        for (int k = 0; k < 3; k++) q[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    } else if (OD == PAPOF_DTYPE_U8) {
        for (int k = 0; k < 3; k++)
            *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.rgb.data) + o + k * a.rgb.stride[3] + x) =
                level_u8(N[0][k]) | (level_u8(N[1][k]) << 8) | (level_u8(N[2][k]) << 16) | (level_u8(N[3][k]) << 24);
    } else if (NHWC) {
        float4* q = reinterpret_cast<float4*>(static_cast<float*>(a.rgb.data) + o + 3LL * x);
        float f[12];
        for (int d = 0; d < 4; d++)
            for (int k = 0; k < 3; k++) f[3 * d + k] = level_f32(N[d][k]);
        for (int k = 0; k < 3; k++) q[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    } else {
        for (int k = 0; k < 3; k++)
            *reinterpret_cast<float4*>(static_cast<float*>(a.rgb.data) + o + k * a.rgb.stride[3] + x) =
                make_float4(level_f32(N[0][k]), level_f32(N[1][k]), level_f32(N[2][k]), level_f32(N[3][k]));
    }
}

__device__ __forceinline__ unsigned char level_of(long long n, long long d) {  // clamp(floor(n / d), 0, 255)
    if (n <= 0) return 0;
    const long long v = n / d;
    return (unsigned char)(v > 255 ? 255 : v);
}

// blockIdx.x: tile `tile0` + x of the CHROMA plane, blockIdx.y: frame `frame0` + y; one lane per chroma sample (k, j), which
// also writes the luma of columns 2 k, 2 k + 1 of rows sub_v j .. sub_v j + sub_v - 1
template <int FD>
__global__ __launch_bounds__(SurfTile::kX* SurfTile::kY) void k_rgb_to_ycc(const RgbArgs a, long long tile0, long long frame0) {
    using T = SurfTile;
    PAPOF_TILE_PIXEL(T, tile0, a.Wc, int, k, int, j);
    if (k >= a.Wc || j >= a.Hc) return;
    const long long t = frame0 + blockIdx.y;
    constexpr long long D = 257LL << 14;
    const long long base = t * a.rgb.stride[0], s1 = a.rgb.stride[1], s2 = a.rgb.stride[2], s3 = a.rgb.stride[3];
    unsigned char* py = static_cast<unsigned char*>(a.y.data) + t * a.y.stride[0];
    for (int dy = 0; dy < a.sub_v; dy++)
        for (int dx = 0; dx < 2; dx++) {
            const int r = a.sub_v * j + dy, x = 2 * k + dx;
            if (r >= a.H || x >= a.W) continue;
            const long long o = base + r * s1 + x * s2;
            const long long R = load_q<FD>(a.rgb, o), G = load_q<FD>(a.rgb, o + s3), B = load_q<FD>(a.rgb, o + 2 * s3);
            py[r * a.y.stride[1] + x * a.y.stride[2]] = level_of(a.yr * R + a.yg * G + a.yb * B + a.y_off * D + D / 2, D);
        }
    // the taps: nc columns with weights wc, nr rows with weights wr, each adding to 4
    int cols[3], wc[3], rows[3], wr[3], nc, nr;
    if (a.sh == 0) {
        nc = 3, cols[0] = 2 * k - 1, cols[1] = 2 * k, cols[2] = 2 * k + 1, wc[0] = 1, wc[1] = 2, wc[2] = 1;
    } else {
        nc = 2, cols[0] = 2 * k, cols[1] = 2 * k + 1, cols[2] = 0, wc[0] = 2, wc[1] = 2, wc[2] = 0;
    }
    for (int i = 0; i < 3; i++) cols[i] = clampi(cols[i], 0, a.W - 1);
    rows[2] = 0, wr[2] = 0;
    if (a.sub_v == 1) {
        nr = 1, rows[0] = j, wr[0] = 4, rows[1] = 0, wr[1] = 0;
    } else if (a.interlaced) {
        const int p = j & 1, m = j >> 1, last = a.H - 2 + p;  // the field's last row
        nr = 2, rows[0] = 4 * m + p, rows[1] = rows[0] + 2 < last ? rows[0] + 2 : last, wr[0] = p ? 1 : 3, wr[1] = 4 - wr[0];
    } else if (a.sv == 0) {
        nr = 2, rows[0] = 2 * j, rows[1] = 2 * j + 1, wr[0] = 2, wr[1] = 2;
    } else {
        nr = 3, rows[0] = 2 * j - 1, rows[1] = 2 * j, rows[2] = 2 * j + 1, wr[0] = 1, wr[1] = 2, wr[2] = 1;
    }
    if (!(a.sub_v == 2 && a.interlaced))
        for (int i = 0; i < 3; i++) rows[i] = clampi(rows[i], 0, a.H - 1);
    long long Su = 0, Sv = 0;
    for (int i = 0; i < nr; i++)
        for (int c = 0; c < nc; c++) {
            const long long o = base + rows[i] * s1 + cols[c] * s2;
            const long long R = load_q<FD>(a.rgb, o), G = load_q<FD>(a.rgb, o + s3), B = load_q<FD>(a.rgb, o + 2 * s3);
            const long long w = wr[i] * wc[c];
            Su += w * ((long long)(a.ur + a.ug) * B - a.ur * R - a.ug * G);
            Sv += w * ((long long)(a.vg + a.vb) * R - a.vg * G - a.vb * B);
        }
    const long long half = 128 * 16 * D + 8 * D;
    static_cast<unsigned char*>(a.cb.data)[t * a.cb.stride[0] + j * a.cb.stride[1] + k * a.cb.stride[2]] = level_of(Su + half, 16 * D);
    static_cast<unsigned char*>(a.cr.data)[t * a.cr.stride[0] + j * a.cr.stride[1] + k * a.cr.stride[2]] = level_of(Sv + half, 16 * D);
}

// ---- surfaces of 9 .. 16 bits per sample in 16-bit words (papof_ycc16_to_rgb_tensor, papof_rgb_to_ycc16_tensor): the taps,
// the tiles and the lane mappings of the 8-bit kernels above; a sample is (word >> shift) & P, a stored word level << shift;
// every product is int32 x int32 -> int64 (one v_mad_i64_i32), every sum 64-bit (include/papof.h has the bounds)
struct Ycc16Args {
    papof_tensor y, cb, cr, rgb;
    int H, W, Hc, Wc;
    int sub_v, sh, sv, interlaced;
    int shift, mask, mid32, rsh;  // mask: P; mid32: 2^(d+4), 32 times neutral chroma; rsh: d + 11, the shift of a uint8 level
    int y_off, cy, crv, cgu, cgv, cbu;
    long long one;  // peak * 2^(d+11): the numerator of 1.0
};

struct Rgb16Args {
    papof_tensor rgb, y, cb, cr;
    int H, W, Hc, Wc;
    int sub_v, sh, sv, interlaced;
    int shift, mask, mid;  // mask: P; mid: 2^(d-1), neutral chroma
    int y_off, yr, yg, yb, ur, ug, vg, vb;
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

// level_u8's form at 64 bits: the sum clamped to 0 .. 2^(d+19) - 1 first, shifted second
__device__ __forceinline__ unsigned level16_u8(const Ycc16Args& a, long long N) {
    return (unsigned)(clampll(N + (1LL << (a.rsh - 1)), 0, (256LL << a.rsh) - 1) >> a.rsh);
}
__device__ __forceinline__ double level16_f64(const Ycc16Args& a, long long N) { return (double)clampll(N, 0, a.one) / (double)a.one; }
__device__ __forceinline__ float level16_f32(const Ycc16Args& a, long long N) { return (float)level16_f64(a, N); }

// N_r, N_g, N_b of a luma sample and of 32 times its chroma minus neutral
__device__ __forceinline__ void numerators16(const Ycc16Args& a, int Y, int U, int V, long long (&N)[3]) {
    const long long L = 32 * ((long long)a.cy * (Y - a.y_off));
    N[0] = L + (long long)a.crv * V, N[1] = L - (long long)a.cgu * U - (long long)a.cgv * V, N[2] = L + (long long)a.cbu * U;
}

template <int OD>
__device__ __forceinline__ void store_level16(const Ycc16Args& a, long long off, long long N) {
    if (OD == PAPOF_DTYPE_U8)
        static_cast<unsigned char*>(a.rgb.data)[off] = (unsigned char)level16_u8(a, N);
    else if (OD == PAPOF_DTYPE_F32)
        static_cast<float*>(a.rgb.data)[off] = level16_f32(a, N);
    else
        static_cast<double*>(a.rgb.data)[off] = level16_f64(a, N);
}

// k_ycc_to_rgb's mapping and nine loads, of 16-bit words: any format, pitch and alignment
template <int OD>
__global__ __launch_bounds__(SurfTile::kX* SurfTile::kY) void k_ycc16_to_rgb(const Ycc16Args a, long long tile0, long long frame0) {
    using T = SurfTile;
    PAPOF_TILE_PIXEL(T, tile0, a.W, int, x, int, r);
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    const Taps hx = h_taps(x, a.Wc, a.sh), vy = v_taps(r, a.Hc, a.sub_v, a.sv, a.interlaced);
    const unsigned short* py = static_cast<const unsigned short*>(a.y.data) + t * a.y.stride[0];
    const unsigned short* pu = static_cast<const unsigned short*>(a.cb.data) + t * a.cb.stride[0];
    const unsigned short* pv = static_cast<const unsigned short*>(a.cr.data) + t * a.cr.stride[0];
    const long long ua = vy.a * a.cb.stride[1], ub = vy.b * a.cb.stride[1], va = vy.a * a.cr.stride[1], vb = vy.b * a.cr.stride[1];
    const long long uxa = hx.a * a.cb.stride[2], uxb = hx.b * a.cb.stride[2], vxa = hx.a * a.cr.stride[2], vxb = hx.b * a.cr.stride[2];
    const int s = a.shift, m = a.mask;
    const int Y = (py[r * a.y.stride[1] + x * a.y.stride[2]] >> s) & m;
    const int u00 = (pu[ua + uxa] >> s) & m, u01 = (pu[ua + uxb] >> s) & m, u10 = (pu[ub + uxa] >> s) & m, u11 = (pu[ub + uxb] >> s) & m;
    const int v00 = (pv[va + vxa] >> s) & m, v01 = (pv[va + vxb] >> s) & m, v10 = (pv[vb + vxa] >> s) & m, v11 = (pv[vb + vxb] >> s) & m;
    const int U = vy.wa * (hx.wa * u00 + hx.wb * u01) + vy.wb * (hx.wa * u10 + hx.wb * u11) - a.mid32;
    const int V = vy.wa * (hx.wa * v00 + hx.wb * v01) + vy.wb * (hx.wa * v10 + hx.wb * v11) - a.mid32;
    long long N[3];
    numerators16(a, Y, U, V, N);
    const long long o = t * a.rgb.stride[0] + r * a.rgb.stride[1] + x * a.rgb.stride[2], sc = a.rgb.stride[3];
    for (int k = 0; k < 3; k++) store_level16<OD>(a, o + k * sc, N[k]);
}

// the four samples 2 i - 1 .. 2 i + 2 of one plane of interleaved 16-bit chroma, clamped to the row.  A dword holds one sample
// of both planes: `lo` and `hi` are the dwords of the lane's own 8 bytes (samples 2 i, 2 i + 1), `prev` the dword in front of
// them and `next` the one behind; `sh` is the plane's first bit within a dword (0 or 16) plus the samples' shift
__device__ __forceinline__ void nv16_window(unsigned prev, unsigned lo, unsigned hi, unsigned next, bool first, bool last, int sh, int mask,
                                            int (&w)[4]) {
    w[1] = (int)(lo >> sh) & mask, w[2] = (int)(hi >> sh) & mask;
    w[0] = first ? w[1] : (int)(prev >> sh) & mask;
    w[3] = last ? w[2] : (int)(next >> sh) & mask;
}

// k_ycc_to_rgb_nv's mapping for P010 / P016 / P210: a lane owns four adjacent luma columns of one row.  The luma is one 8-byte
// load; per chroma row the 8 bytes that hold both planes' samples 2 i and 2 i + 1, and of the neighbouring lanes' 8 bytes the
// dword each that holds samples 2 i - 1 and 2 i + 2.  What ycc16_fast promises: W % 4 == 0, so a lane's four columns are
// inside together and a chroma row is W / 4 whole groups of 8 bytes; every row of the planes starts on 8 bytes, of rgb on a
// dword (float32: on 16 bytes).  vu: Cr is the first word of a chroma pair.
template <int OD, bool NHWC>
__global__ __launch_bounds__(256) void k_ycc16_to_rgb_nv(const Ycc16Args a, int vu, long long tile0, long long frame0) {
    using T = NvTile;
    PAPOF_TILE_ORIGIN(T, tile0, a.W, int, x0, int, r0);
    const int x = x0 + 4 * (int)threadIdx.x, r = r0 + (int)threadIdx.y;
    if (x >= a.W || r >= a.H) return;
    const long long t = frame0 + blockIdx.y;
    const Taps vy = v_taps(r, a.Hc, a.sub_v, a.sv, a.interlaced);
    const papof_tensor& c = vu ? a.cr : a.cb;  // the plane whose word comes first
    const unsigned short* pc = static_cast<const unsigned short*>(c.data) + t * c.stride[0];
    const int i = x >> 2, n = a.W >> 2, ip = i > 0 ? i - 1 : 0, in = i + 1 < n ? i + 1 : n - 1;
    const unsigned* ra = reinterpret_cast<const unsigned*>(pc + vy.a * c.stride[1]);
    const unsigned* rb = reinterpret_cast<const unsigned*>(pc + vy.b * c.stride[1]);
    const uint2 yw = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(a.y.data) + t * a.y.stride[0] + r * a.y.stride[1] + x);
    const uint2 a1 = reinterpret_cast<const uint2*>(ra)[i], b1 = reinterpret_cast<const uint2*>(rb)[i];
    const unsigned a0 = ra[2 * ip + 1], a2 = ra[2 * in], b0 = rb[2 * ip + 1], b2 = rb[2 * in];
    int P[2][4];  // 32 times the chroma of the first and of the second plane of the pair, minus neutral
    for (int k = 0; k < 2; k++) {
        int wa[4], wb[4], ha[4], hb[4];
        nv16_window(a0, a1.x, a1.y, a2, i == 0, i == n - 1, 16 * k + a.shift, a.mask, wa);
        nv16_window(b0, b1.x, b1.y, b2, i == 0, i == n - 1, 16 * k + a.shift, a.mask, wb);
        nv_across(wa, a.sh, ha);
        nv_across(wb, a.sh, hb);
        for (int d = 0; d < 4; d++) P[k][d] = vy.wa * ha[d] + vy.wb * hb[d] - a.mid32;
    }
    long long N[4][3];
    for (int d = 0; d < 4; d++) {
        const int Y = (int)((d < 2 ? yw.x : yw.y) >> (16 * (d & 1) + a.shift)) & a.mask;
        numerators16(a, Y, vu ? P[1][d] : P[0][d], vu ? P[0][d] : P[1][d], N[d]);
    }
    const long long o = t * a.rgb.stride[0] + r * a.rgb.stride[1];
    if (OD == PAPOF_DTYPE_U8 && NHWC) {
        unsigned b[12];
        for (int d = 0; d < 4; d++)
            for (int k = 0; k < 3; k++) b[3 * d + k] = level16_u8(a, N[d][k]);
        unsigned* q = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.rgb.data) + o + 3LL * x);
        for (int k = 0; k < 3; k++) q[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    } else if (OD == PAPOF_DTYPE_U8) {
        for (int k = 0; k < 3; k++)
            *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.rgb.data) + o + k * a.rgb.stride[3] + x) =
                level16_u8(a, N[0][k]) | (level16_u8(a, N[1][k]) << 8) | (level16_u8(a, N[2][k]) << 16) | (level16_u8(a, N[3][k]) << 24);
    } else if (NHWC) {
        float4* q = reinterpret_cast<float4*>(static_cast<float*>(a.rgb.data) + o + 3LL * x);
        float f[12];
        for (int d = 0; d < 4; d++)
            for (int k = 0; k < 3; k++) f[3 * d + k] = level16_f32(a, N[d][k]);
        for (int k = 0; k < 3; k++) q[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    } else {
        for (int k = 0; k < 3; k++)
            *reinterpret_cast<float4*>(static_cast<float*>(a.rgb.data) + o + k * a.rgb.stride[3] + x) =
                make_float4(level16_f32(a, N[0][k]), level16_f32(a, N[1][k]), level16_f32(a, N[2][k]), level16_f32(a, N[3][k]));
    }
}

constexpr long long kE = 65535LL << 14;  // one level of q at the coefficients' scale, whatever the depth

__device__ __forceinline__ unsigned short word_of(long long n, long long d, int P, int shift) {  // clamp(floor(n / d), 0, P) << shift
    if (n <= 0) return 0;
    const long long v = n / d;
    return (unsigned short)((int)(v > P ? P : v) << shift);
}

// k_rgb_to_ycc's taps as a function: nc columns with weights wc, nr rows with weights wr, each adding to 4.  (k_rgb_to_ycc keeps
// them in its own body: calling this from it changed its instructions, and the 8-bit kernels' code is held as it was.)
__device__ __forceinline__ void adjoint_taps(const Rgb16Args& a, int k, int j, int (&cols)[3], int (&wc)[3], int& nc, int (&rows)[3],
                                             int (&wr)[3], int& nr) {
    if (a.sh == 0) {
        nc = 3, cols[0] = 2 * k - 1, cols[1] = 2 * k, cols[2] = 2 * k + 1, wc[0] = 1, wc[1] = 2, wc[2] = 1;
    } else {
        nc = 2, cols[0] = 2 * k, cols[1] = 2 * k + 1, cols[2] = 0, wc[0] = 2, wc[1] = 2, wc[2] = 0;
    }
    for (int i = 0; i < 3; i++) cols[i] = clampi(cols[i], 0, a.W - 1);
    rows[2] = 0, wr[2] = 0;
    if (a.sub_v == 1) {
        nr = 1, rows[0] = j, wr[0] = 4, rows[1] = 0, wr[1] = 0;
    } else if (a.interlaced) {
        const int p = j & 1, m = j >> 1, last = a.H - 2 + p;  // the field's last row
        nr = 2, rows[0] = 4 * m + p, rows[1] = rows[0] + 2 < last ? rows[0] + 2 : last, wr[0] = p ? 1 : 3, wr[1] = 4 - wr[0];
    } else if (a.sv == 0) {
        nr = 2, rows[0] = 2 * j, rows[1] = 2 * j + 1, wr[0] = 2, wr[1] = 2;
    } else {
        nr = 3, rows[0] = 2 * j - 1, rows[1] = 2 * j, rows[2] = 2 * j + 1, wr[0] = 1, wr[1] = 2, wr[2] = 1;
    }
    if (!(a.sub_v == 2 && a.interlaced))
        for (int i = 0; i < 3; i++) rows[i] = clampi(rows[i], 0, a.H - 1);
}

// k_rgb_to_ycc's mapping: one lane per chroma sample (k, j), which also writes the luma of its 2 x sub_v pixels; 16-bit vector
// stores of level << shift
template <int FD>
__global__ __launch_bounds__(SurfTile::kX* SurfTile::kY) void k_rgb_to_ycc16(const Rgb16Args a, long long tile0, long long frame0) {
    using T = SurfTile;
    PAPOF_TILE_PIXEL(T, tile0, a.Wc, int, k, int, j);
    if (k >= a.Wc || j >= a.Hc) return;
    const long long t = frame0 + blockIdx.y;
    const long long base = t * a.rgb.stride[0], s1 = a.rgb.stride[1], s2 = a.rgb.stride[2], s3 = a.rgb.stride[3];
    unsigned short* py = static_cast<unsigned short*>(a.y.data) + t * a.y.stride[0];
    for (int dy = 0; dy < a.sub_v; dy++)
        for (int dx = 0; dx < 2; dx++) {
            const int r = a.sub_v * j + dy, x = 2 * k + dx;
            if (r >= a.H || x >= a.W) continue;
            const long long o = base + r * s1 + x * s2;
            const long long R = load_q<FD>(a.rgb, o), G = load_q<FD>(a.rgb, o + s3), B = load_q<FD>(a.rgb, o + 2 * s3);
            py[r * a.y.stride[1] + x * a.y.stride[2]] = word_of(a.yr * R + a.yg * G + a.yb * B + a.y_off * kE + kE / 2, kE, a.mask, a.shift);
        }
    int cols[3], wc[3], rows[3], wr[3], nc, nr;
    adjoint_taps(a, k, j, cols, wc, nc, rows, wr, nr);
    long long Su = 0, Sv = 0;
    for (int i = 0; i < nr; i++)
        for (int c = 0; c < nc; c++) {
            const long long o = base + rows[i] * s1 + cols[c] * s2;
            const long long R = load_q<FD>(a.rgb, o), G = load_q<FD>(a.rgb, o + s3), B = load_q<FD>(a.rgb, o + 2 * s3);
            const long long w = wr[i] * wc[c];
            Su += w * (((long long)a.ur + a.ug) * B - a.ur * R - a.ug * G);
            Sv += w * (((long long)a.vg + a.vb) * R - a.vg * G - a.vb * B);
        }
    const long long half = a.mid * 16 * kE + 8 * kE;
    static_cast<unsigned short*>(a.cb.data)[t * a.cb.stride[0] + j * a.cb.stride[1] + k * a.cb.stride[2]] = word_of(Su + half, 16 * kE, a.mask, a.shift);
    static_cast<unsigned short*>(a.cr.data)[t * a.cr.stride[0] + j * a.cr.stride[1] + k * a.cr.stride[2]] = word_of(Sv + half, 16 * kE, a.mask, a.shift);
}

// a uint8 plane (frame, row, column): stride[3] is not read
inline bool in_plane_u8(const papof_tensor* t) { return described(t, {PAPOF_DTYPE_U8}, {0, 1, 2}, false); }
inline bool out_plane_u8(const papof_tensor* t) { return described(t, {PAPOF_DTYPE_U8}, {0, 1, 2}, true); }

// what both calls refuse of their sizes and codes, and of the first `n` of their tables
inline bool surface_args(int n_frames, int height, int width, int sub_v, int sh, int sv, int interlaced, const int* tables, int n) {
    if (n_frames < 1 || height < 1 || width < 1 || (sub_v != 1 && sub_v != 2) || !tables) return false;
    if ((sh != 0 && sh != 1) || (sv != 0 && sv != 1)) return false;
    if (interlaced && (height % 2 != 0 || height < 4)) return false;
    if (tables[0] < 0 || tables[0] > 255) return false;
    for (int i = 1; i < n; i++)
        if (tables[i] < 0 || tables[i] > kMaxCoef) return false;
    return true;
}

inline bool aligned(const papof_tensor& t, long long unit, long long bytes) {  // data, row and frame starts on `bytes` bytes
    return reinterpret_cast<unsigned long long>(t.data) % bytes == 0 && t.stride[0] * unit % bytes == 0 && t.stride[1] * unit % bytes == 0;
}

// what the instances that store whole dwords need of rgb: uint8 or float32, NHWC or NCHW, every row of it on a dword (float32:
// on 16 bytes)
inline bool rgb_fast(const papof_tensor& rgb) {
    if (rgb.dtype == PAPOF_DTYPE_F64) return false;
    const long long unit = rgb.dtype == PAPOF_DTYPE_U8 ? 1 : 4, bytes = rgb.dtype == PAPOF_DTYPE_U8 ? 4 : 16;
    const bool nhwc = rgb.stride[3] == 1 && rgb.stride[2] == 3, nchw = rgb.stride[2] == 1 && rgb.stride[3] * unit % bytes == 0;
    return (nhwc || nchw) && aligned(rgb, unit, bytes);
}

// k_ycc_to_rgb_nv serves these descriptors: 0 no, 1 with Cb first (NV12, NV16), 2 with Cr first (NV21, NV61)
inline int ycc_fast(int width, const papof_tensor& y, const papof_tensor& cb, const papof_tensor& cr, const papof_tensor& rgb) {
    if (width % 4 != 0 || y.stride[2] != 1 || !aligned(y, 1, 4)) return 0;
    if (cb.stride[2] != 2 || cr.stride[2] != 2 || cb.stride[1] != cr.stride[1] || cb.stride[0] != cr.stride[0]) return 0;
    const unsigned char *u = static_cast<const unsigned char*>(cb.data), *v = static_cast<const unsigned char*>(cr.data);
    const int order = v == u + 1 ? 1 : u == v + 1 ? 2 : 0;
    if (!order || !aligned(order == 1 ? cb : cr, 1, 4)) return 0;
    return rgb_fast(rgb) ? order : 0;
}

// a U16 plane (frame, row, column), strides in 16-bit words: stride[3] is not read
inline bool in_plane_u16(const papof_tensor* t) { return described(t, {PAPOF_DTYPE_U16}, {0, 1, 2}, false); }
inline bool out_plane_u16(const papof_tensor* t) { return described(t, {PAPOF_DTYPE_U16}, {0, 1, 2}, true); }

// what the two 16-bit calls refuse of their sizes and codes, and of the first `n` of their tables: six of the forward call,
// coefficients 0 .. 2^(d+8) - 1, or eight of the reverse call, coefficients 0 .. 2^30
inline bool surface16_args(int n_frames, int height, int width, int depth, int shift, int sub_v, int sh, int sv, int interlaced,
                           const int* tables, int n) {
    if (n_frames < 1 || height < 1 || width < 1 || (sub_v != 1 && sub_v != 2) || !tables) return false;
    if (depth < 9 || depth > 16 || shift < 0 || shift > 16 - depth) return false;
    if ((sh != 0 && sh != 1) || (sv != 0 && sv != 1)) return false;
    if (interlaced && (height % 2 != 0 || height < 4)) return false;
    if (tables[0] < 0 || tables[0] > (1 << depth) - 1) return false;
    const long long max_coef = n == 6 ? (1LL << (depth + 8)) - 1 : 1LL << 30;
    for (int i = 1; i < n; i++)
        if (tables[i] < 0 || tables[i] > max_coef) return false;
    return true;
}

// k_ycc16_to_rgb_nv serves these descriptors: 0 no, 1 with Cb first (P010, P016, P210), 2 with Cr first
inline int ycc16_fast(int width, const papof_tensor& y, const papof_tensor& cb, const papof_tensor& cr, const papof_tensor& rgb) {
    if (width % 4 != 0 || y.stride[2] != 1 || !aligned(y, 2, 8)) return 0;
    if (cb.stride[2] != 2 || cr.stride[2] != 2 || cb.stride[1] != cr.stride[1] || cb.stride[0] != cr.stride[0]) return 0;
    const unsigned short *u = static_cast<const unsigned short*>(cb.data), *v = static_cast<const unsigned short*>(cr.data);
    const int order = v == u + 1 ? 1 : u == v + 1 ? 2 : 0;
    if (!order || !aligned(order == 1 ? cb : cr, 2, 8)) return 0;
    return rgb_fast(rgb) ? order : 0;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" int papof_ycc_to_rgb_fast(int width, const papof_tensor* y, const papof_tensor* cb, const papof_tensor* cr,
                                     const papof_tensor* rgb) {
    if (width < 1 || !in_plane_u8(y) || !in_plane_u8(cb) || !in_plane_u8(cr) || !out_frames(rgb)) return PAPOF_EINVAL;
    return ycc_fast(width, *y, *cb, *cr, *rgb) != 0;
}

extern "C" int papof_ycc_to_rgb_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* y,
                                       const papof_tensor* cb, const papof_tensor* cr, int sub_v, int siting_h, int siting_v,
                                       int interlaced, const int* tables, const papof_tensor* rgb, void* stream) {
    if (!h || !surface_args(n_frames, height, width, sub_v, siting_h, siting_v, interlaced, tables, 6)) return PAPOF_EINVAL;
    if (!in_plane_u8(y) || !in_plane_u8(cb) || !in_plane_u8(cr) || !out_frames(rgb)) return PAPOF_EINVAL;
    YccArgs a{};
    a.y = *y, a.cb = *cb, a.cr = *cr, a.rgb = *rgb;
    a.H = height, a.W = width, a.Hc = (height + sub_v - 1) / sub_v, a.Wc = (width + 1) / 2;
    a.sub_v = sub_v, a.sh = siting_h, a.sv = siting_v, a.interlaced = interlaced != 0;
    a.y_off = tables[0], a.cy = tables[1], a.crv = tables[2], a.cgu = tables[3], a.cgv = tables[4], a.cbu = tables[5];
    PAPOF_HIP(hipSetDevice(h->device));
    if (const int order = ycc_fast(width, *y, *cb, *cr, *rgb)) {
        const bool nhwc = rgb->stride[3] == 1 && rgb->stride[2] == 3;
        const auto fast = rgb->dtype == PAPOF_DTYPE_U8 ? (nhwc ? k_ycc_to_rgb_nv<PAPOF_DTYPE_U8, true> : k_ycc_to_rgb_nv<PAPOF_DTYPE_U8, false>)
                                                       : (nhwc ? k_ycc_to_rgb_nv<PAPOF_DTYPE_F32, true> : k_ycc_to_rgb_nv<PAPOF_DTYPE_F32, false>);
        return launch_grid<NvTile>(a.H, a.W, n_frames, static_cast<hipStream_t>(stream), 0, fast, a, order == 2 ? 1 : 0);
    }
    const auto kernel = by_dtype(rgb->dtype, [](auto od) { return k_ycc_to_rgb<od()>; });
    return launch_grid<SurfTile>(a.H, a.W, n_frames, static_cast<hipStream_t>(stream), 0, kernel, a);
}

extern "C" int papof_rgb_to_ycc_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* rgb, int sub_v,
                                       int siting_h, int siting_v, int interlaced, const int* tables, const papof_tensor* y,
                                       const papof_tensor* cb, const papof_tensor* cr, void* stream) {
    if (!h || !surface_args(n_frames, height, width, sub_v, siting_h, siting_v, interlaced, tables, 8)) return PAPOF_EINVAL;
    if (!in_frames(rgb) || !out_plane_u8(y) || !out_plane_u8(cb) || !out_plane_u8(cr)) return PAPOF_EINVAL;
    RgbArgs a{};
    a.rgb = *rgb, a.y = *y, a.cb = *cb, a.cr = *cr;
    a.H = height, a.W = width, a.Hc = (height + sub_v - 1) / sub_v, a.Wc = (width + 1) / 2;
    a.sub_v = sub_v, a.sh = siting_h, a.sv = siting_v, a.interlaced = interlaced != 0;
    a.y_off = tables[0], a.yr = tables[1], a.yg = tables[2], a.yb = tables[3];
    a.ur = tables[4], a.ug = tables[5], a.vg = tables[6], a.vb = tables[7];
    PAPOF_HIP(hipSetDevice(h->device));
    const auto kernel = by_dtype(rgb->dtype, [](auto fd) { return k_rgb_to_ycc<fd()>; });
    return launch_grid<SurfTile>(a.Hc, a.Wc, n_frames, static_cast<hipStream_t>(stream), 0, kernel, a);
}

extern "C" int papof_ycc16_to_rgb_fast(int width, const papof_tensor* y, const papof_tensor* cb, const papof_tensor* cr,
                                       const papof_tensor* rgb) {
    if (width < 1 || !in_plane_u16(y) || !in_plane_u16(cb) || !in_plane_u16(cr) || !out_frames(rgb)) return PAPOF_EINVAL;
    return ycc16_fast(width, *y, *cb, *cr, *rgb) != 0;
}

extern "C" int papof_ycc16_to_rgb_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* y,
                                         const papof_tensor* cb, const papof_tensor* cr, int depth, int shift, int sub_v,
                                         int siting_h, int siting_v, int interlaced, const int* tables, const papof_tensor* rgb,
                                         void* stream) {
    if (!h || !surface16_args(n_frames, height, width, depth, shift, sub_v, siting_h, siting_v, interlaced, tables, 6))
        return PAPOF_EINVAL;
    if (!in_plane_u16(y) || !in_plane_u16(cb) || !in_plane_u16(cr) || !out_frames(rgb)) return PAPOF_EINVAL;
    const int peak = tables[6];
    if (peak < 1 || peak > 65535 || (rgb->dtype == PAPOF_DTYPE_U8 && peak != 255)) return PAPOF_EINVAL;
    Ycc16Args a{};
    a.y = *y, a.cb = *cb, a.cr = *cr, a.rgb = *rgb;
    a.H = height, a.W = width, a.Hc = (height + sub_v - 1) / sub_v, a.Wc = (width + 1) / 2;
    a.sub_v = sub_v, a.sh = siting_h, a.sv = siting_v, a.interlaced = interlaced != 0;
    a.shift = shift, a.mask = (1 << depth) - 1, a.mid32 = 1 << (depth + 4), a.rsh = depth + 11;
    a.y_off = tables[0], a.cy = tables[1], a.crv = tables[2], a.cgu = tables[3], a.cgv = tables[4], a.cbu = tables[5];
    a.one = (long long)peak << (depth + 11);
    PAPOF_HIP(hipSetDevice(h->device));
    if (const int order = ycc16_fast(width, *y, *cb, *cr, *rgb)) {
        const bool nhwc = rgb->stride[3] == 1 && rgb->stride[2] == 3;
        const auto fast = rgb->dtype == PAPOF_DTYPE_U8 ? (nhwc ? k_ycc16_to_rgb_nv<PAPOF_DTYPE_U8, true> : k_ycc16_to_rgb_nv<PAPOF_DTYPE_U8, false>)
                                                       : (nhwc ? k_ycc16_to_rgb_nv<PAPOF_DTYPE_F32, true> : k_ycc16_to_rgb_nv<PAPOF_DTYPE_F32, false>);
        return launch_grid<NvTile>(a.H, a.W, n_frames, static_cast<hipStream_t>(stream), 0, fast, a, order == 2 ? 1 : 0);
    }
    const auto kernel = by_dtype(rgb->dtype, [](auto od) { return k_ycc16_to_rgb<od()>; });
    return launch_grid<SurfTile>(a.H, a.W, n_frames, static_cast<hipStream_t>(stream), 0, kernel, a);
}

extern "C" int papof_rgb_to_ycc16_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* rgb, int depth,
                                         int shift, int sub_v, int siting_h, int siting_v, int interlaced, const int* tables,
                                         const papof_tensor* y, const papof_tensor* cb, const papof_tensor* cr, void* stream) {
    if (!h || !surface16_args(n_frames, height, width, depth, shift, sub_v, siting_h, siting_v, interlaced, tables, 8))
        return PAPOF_EINVAL;
    if (!in_frames(rgb) || !out_plane_u16(y) || !out_plane_u16(cb) || !out_plane_u16(cr)) return PAPOF_EINVAL;
    Rgb16Args a{};
    a.rgb = *rgb, a.y = *y, a.cb = *cb, a.cr = *cr;
    a.H = height, a.W = width, a.Hc = (height + sub_v - 1) / sub_v, a.Wc = (width + 1) / 2;
    a.sub_v = sub_v, a.sh = siting_h, a.sv = siting_v, a.interlaced = interlaced != 0;
    a.shift = shift, a.mask = (1 << depth) - 1, a.mid = 1 << (depth - 1);
    a.y_off = tables[0], a.yr = tables[1], a.yg = tables[2], a.yb = tables[3];
    a.ur = tables[4], a.ug = tables[5], a.vg = tables[6], a.vb = tables[7];
    PAPOF_HIP(hipSetDevice(h->device));
    const auto kernel = by_dtype(rgb->dtype, [](auto fd) { return k_rgb_to_ycc16<fd()>; });
    return launch_grid<SurfTile>(a.Hc, a.Wc, n_frames, static_cast<hipStream_t>(stream), 0, kernel, a);
}
