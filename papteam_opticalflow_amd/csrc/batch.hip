// papteam_opticalflow_amd/csrc/batch.hip -- B frame pairs of ONE shape in ONE launch chain (papof_flow_batch*).
//
// Why.  The reference's own benchmark walks collections of SMALL frames (Code/Serial/TestSuite.py:69-81, :91: 101 pairs per
// collection, 240x135 ... 1920x1080, pyramidLevels 2 / 4 / 8 / 15).  One 240x135 pair on the reference schedule is ~210 kernel
// launches of a few microseconds of work each and 45 hand-off-bound solves on a chip it cannot fill.  Running many pairs side
// by side as independent calls (flow_collection: one handle, stream and host thread per sequence) plateaus at ~2 ms per pair
// with 16 in flight, and the limiter is the DEVICE's dispatch of ~84 k small dependent kernels per second over 16 queues -- the
// host spends 1.0 of 24 ms per call enqueueing, while every little kernel is stretched to 50-65 us
// (profiles/r04_collection_trace_240.txt, r04_collection_concurrency_240x16.txt).  Here the pairs of a batch share every
// launch: each buffer of the call is an ARRAY over the pairs (or frames), the per-pixel kernels take the pair from blockIdx.y
// (common.h: BatchK; plane-parallel kernels simply see C x frames planes), and ONE solver launch holds the tasks of all pairs
// (sor.hip: ExactArgs::bs_*, TinyArgs::bstride).  Same kernels, same operations per pair: every pair's results are bit-identical
// to the single call's (tests/test_gpu_batch.py).
//
// Scope: the default branches in the reference's own sweep order (exact order, n_inner = 1, bilinear warping, Laplacian noise
// model, 1 or 3 input channels, fewer than 16 solver bands per level); anything else -- and a batch of one -- runs as
// consecutive single calls through the same entry point.  A consecutive-pairs batch (`sequence`: pair i = frames i, i + 1, a
// video) builds every frame's pyramid and features once.
//
// The Laplacian-noise guard (api.hip: LapGuard; src/OpticalFlow.cpp:399-400): the batch runs the OPTIMISTIC pass with one block
// of witness flags per pair and non-zero flags per frame (few-pixel levels: an exhaustive check behind every update); a pair that
// ends without a proof for a consulted estimate (duplicate frames) is run again through the single call, which has the exact
// pass.  Results: the reference's, either way.
//
// Device tensors (papof_flow_batch_tensor): the same chain with frames read where they are -- strided uint8 / float32 / float64
// tensors, k_ingest_frames writes the level-0 array, no staging block -- and results written by k_emit_outputs into the
// caller's strided tensors before anything else runs on the arena.  What the chain does not cover, a batch of one and a
// re-run pair run one pair at a time on the device, their frames converted into a scratch block of the handle.
//
// Both directions (papof_flow_batch_tensor_fb): B backward pairs join the B forward ones as solver pairs B .. 2B - 1 on the
// same per-frame arrays -- the kernels that read frames swap a backward pair's two (common.h: BatchK::bw) -- and k_fb_check
// turns the two fp64 flows into the occlusion mask before the arena is reused.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "common.h"
#include "flow_internal.h"

namespace papof {

namespace {

double now_sec() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct BatchOut {
    const double* uv = nullptr;    // [pair][2][H * W]: the final flow (with_bw: the B forward pairs, then the B backward ones)
    const double* warp = nullptr;  // [pair][H * W * C]
    std::vector<int> unproven;     // pairs whose Laplacian-noise guard could not be proven open: run them through the single call
};

// The frames of a batch: host pointers (uploaded into the arena's staging block), or strided device tensors that
// k_ingest_frames reads where they are (papof_flow_batch_tensor; no staging block, nothing crosses PCIe).
struct BatchFrames {
    const void* const* host = nullptr;  // nF frames, HWC, float64 or uint8 (u8)
    bool u8 = false;
    const papof_tensor* a = nullptr;    // device frames: a sequence, or the first frames of the pairs ...
    const papof_tensor* b = nullptr;    // ... and their second frames (pairs only)
    // the caller's initial flows (papof_flow_batch_tensor_init), from the batch's first pair on: of the B forward pairs and of
    // the B backward ones (with_bw); NULL: zero.  Both NULL: the chain starts from zero flow exactly as it always has.
    const papof_tensor* init_fw = nullptr;
    const papof_tensor* init_bw = nullptr;
};

bool batch_applies(const papof_handle* h, int B, int H, int W, int C, int levels, const papof_params& P) {
    if (B < 2 || !h->use_dpp) return false;
    if (P.sor_mode != PAPOF_SOR_EXACT || P.n_inner != 1 || P.interpolation != PAPOF_INTERP_BILINEAR ||
        P.noise_model != PAPOF_NOISE_LAPLACIAN)
        return false;
    if (C != 1 && C != 3) return false;
    const int n_sor_max = CallPlan::n_sor_at(P, levels - 1);
    if (skew_dims(H, W, n_sor_max, 1, 1).nb >= 16) return false;  // big frames: the two-sweeps-per-wave kernel; they fill the chip alone
    return CallPlan::slots_for(P, levels) <= kLapMaxSlots;
}

// One launch of the solver holds the tasks of ALL pairs, and all of them must be resident (sor.hip: resident_tasks): a
// collection larger than that -- or than a few GB of arena -- goes through in sub-batches of the same shape.
int batch_max(int H, int W, int C, int levels, const papof_params& P) {
    const int n_sor_max = CallPlan::n_sor_at(P, levels - 1);
    const int nb0 = skew_dims(H, W, n_sor_max, 1, 1).nb;
    const size_t per_pair = arena_bytes_for(H, W, C, levels, n_sor_max, P.ratio);
    int max_b = (int)std::max<size_t>(2, std::min<size_t>((size_t)1024 / (size_t)nb0, ((size_t)24 << 30) / per_pair));
    if (const char* e = std::getenv("PAPOF_BATCH_MAX")) max_b = std::max(2, std::min(max_b, std::atoi(e)));  // (and the tests')
    return max_b;
}

// Everything on h->stream, one stream: B pairs fill the chip by themselves.  with_bw: the B backward pairs as well (pair B + p = pair
// p with its two frames exchanged; BatchK::bw), 2B solver pairs on the same per-frame arrays -- only the per-pair work doubles.
int flow_batch_device(papof_handle* h, int B, int sequence, bool with_bw, const BatchFrames& frames, int H, int W, int C, int levels,
                      const papof_params& P, double* timing, BatchOut& out) {
    CallPlan cp;
    PAPOF_TRY(call_plan(H, W, C, levels, P, cp));
    const std::vector<Level>& L = cp.L;
    const std::vector<PyrPlan>& plan = cp.plan;
    const double ratio = cp.ratio;
    const int fstep = sequence ? 1 : 2, nF = sequence ? B + 1 : 2 * B;
    const int NP = with_bw ? 2 * B : B;  // solver pairs: per-pair arrays, operands, witness blocks
    if (NP < 2) return PAPOF_EINVAL;     // the pair-to-pair strides below are read off pairs 0 and 1: a lone pair is the single call's
    const int fc = cp.fc, n_sor_max = cp.n_sor_max;
    const size_t np0 = (size_t)H * W;
    const bool guard = h->lap_guard && h->lap_flags_dev != nullptr;
    const bool u8 = frames.u8, staged = frames.host != nullptr;
    // ---- arena: one block, arrays over frames / pairs
    size_t pyr_px = 0;
    for (const Level& l : L) pyr_px += (size_t)l.w * l.h;
    size_t cells = 0, cells_d = 0;
    skew_capacity(H, W, n_sor_max, cells, cells_d);
    const size_t tiny_cells = std::min<size_t>(kTinyMaxCells, np0);
    size_t bytes = 0;
    if (staged) bytes += (size_t)nF * np0 * C * (u8 ? 1 : 8) + 4096;                // the uploaded frames
    bytes += (size_t)nF * pyr_px * (C + 2 * fc) * 8 + (size_t)levels * 3 * 4096;     // pyramids, features, smoothed features
    bytes += (size_t)nF * np0 * C * 8 * 5 + 5 * 4096;                               // two filter temporaries, three derivative planes
    bytes += (size_t)NP * (4 * np0 * 8 + np0 * C * 8) + 3 * 4096;                   // two flow pairs, the warped image
    bytes += (size_t)NP * ((3 * 2 * ((cells + kLanes + 63) / 64 * 64) + 2 * (cells_d + kLanes)) * 8 + 2 * 4096);  // solver operands
    bytes += (size_t)NP * (8 * (tiny_cells * 8 + 256));                             // row-major operands of k_sor_tiny's levels
    bytes += (size_t)(NP + nF) * kLapFlagWords * 4 + 8192;                          // guard flags
    bytes += (size_t)1 << 20;
    h->seq.valid = false;  // (the arena is laid out anew: a kept sequence pyramid does not survive a batch)
    PAPOF_TRY(ensure_arena(h, bytes));
    Arena& A = h->arena;
    A.off = 0;
    A.overflow = false;
    h->events_used = 0;
    h->sor_log.clear();
    h->sor_launches = 0;
    hipStream_t const st = h->stream;

    unsigned char* stage = staged ? static_cast<unsigned char*>(A.alloc((size_t)nF * np0 * C * (u8 ? 1 : 8))) : nullptr;
    std::vector<double*> Lp(levels), F(levels), S(levels);
    for (int k = 0; k < levels; k++) {
        const size_t n = (size_t)L[k].w * L[k].h;
        Lp[k] = A.f64((size_t)nF * n * C);
        F[k] = A.f64((size_t)nF * n * fc);
        S[k] = A.f64((size_t)nF * n * fc);
    }
    double* tmp_a = A.f64((size_t)nF * np0 * C);
    double* tmp_b = A.f64((size_t)nF * np0 * C);
    double* gx = A.f64((size_t)nF * np0 * C);
    double* gy = A.f64((size_t)nF * np0 * C);
    double* gxy = A.f64((size_t)nF * np0 * C);
    double* uvA = A.f64((size_t)NP * 2 * np0);
    double* uvB = A.f64((size_t)NP * 2 * np0);
    double* warp = A.f64((size_t)NP * np0 * C);
    unsigned* wit = reinterpret_cast<unsigned*>(A.alloc((size_t)NP * kLapFlagWords * sizeof(unsigned)));
    unsigned* nzf = reinterpret_cast<unsigned*>(A.alloc((size_t)nF * kLapNzWords * sizeof(unsigned)));
    if (A.overflow) return PAPOF_ENOMEM;
    // the pairs' solver operands: identical allocation sequences, hence a constant stride from pair to pair
    std::vector<SorPlanes> SP(NP), ST(NP);
    for (int p = 0; p < NP; p++) PAPOF_TRY(sor_alloc_planes(A, H, W, PAPOF_SOR_EXACT, n_sor_max, SP[p]));
    for (int p = 0; p < NP; p++) PAPOF_TRY(sor_alloc_tiny_planes(A, tiny_cells, ST[p]));
    if (A.overflow) return PAPOF_ENOMEM;
    const size_t sp_stride = (size_t)(SP[1].phi - SP[0].phi), spd_stride = (size_t)(SP[1].du - SP[0].du);
    const size_t st_stride = (size_t)(ST[1].phi - ST[0].phi);
    for (int p = 1; p < NP; p++)
        if ((size_t)(SP[p].phi - SP[0].phi) != p * sp_stride || (size_t)(SP[p].du - SP[0].du) != p * spd_stride ||
            (size_t)(ST[p].phi - ST[0].phi) != p * st_stride || (size_t)(ST[p].du - ST[0].du) != p * st_stride)
            return PAPOF_EDEVICE;

    // ---- counters of every solve of every pair (plain layout; a k_sor_tiny level has none), cleared once
    const auto tiny_level = [&](int k) { return sor_tiny_fits(h, L[k].h, L[k].w, cp.n_sor[k]); };
    const SolveCounters LC(
        cp, [&](int k) { return tiny_level(k) ? 0 : (size_t)skew_dims(L[k].h, L[k].w, cp.n_sor[k], 1, 1).nb * cp.n_sor[k] * 32; },
        (size_t)NP);
    const size_t prog_total = LC.total;
    PAPOF_TRY(sor_counters_ensure(h, prog_total));

    // ---- timers: the total, and the solver kernels' own time (events around their launches)
    PhaseClock total{h, true}, sorclk{h, true};
    sorclk.only_sor = true;
    total.phase(PAPOF_T_TOTAL);

    // ---- uploads, layout conversion, pyramids, features (frames are planes x frames for the plane-parallel kernels)
    const size_t frame_bytes = np0 * C * (u8 ? 1 : 8);
    if (staged) {
        const void* const* hf = frames.host;
        bool flat_in = true;  // frames stacked in one host block (the Python binding's): one copy
        for (int f = 1; f < nF && flat_in; f++)
            flat_in = (const unsigned char*)hf[f] == (const unsigned char*)hf[0] + (size_t)f * frame_bytes;
        if (flat_in) {
            PAPOF_HIP(hipMemcpyAsync(stage, hf[0], (size_t)nF * frame_bytes, hipMemcpyHostToDevice, st));
        } else {
            for (int f = 0; f < nF; f++)
                PAPOF_HIP(hipMemcpyAsync(stage + (size_t)f * frame_bytes, hf[f], frame_bytes, hipMemcpyHostToDevice, st));
        }
    }
    if (prog_total && !sor_counters_clear(h, 0, prog_total)) return PAPOF_EDEVICE;
    PAPOF_TRY(lap_next_epoch(h, st));
    const unsigned epoch = h->lap_epoch;  // a flag is set when it holds this call's number
    if (guard) {
        PAPOF_HIP(hipMemsetAsync(wit, 0, (size_t)NP * kLapFlagWords * sizeof(unsigned), st));
        PAPOF_HIP(hipMemsetAsync(nzf, 0, (size_t)nF * kLapNzWords * sizeof(unsigned), st));
    }
    if (!staged)
        PAPOF_TRY(ingest_frames(h, *frames.a, sequence ? nullptr : frames.b, Lp[0], H, W, C, nF));
    else if (u8)
        PAPOF_TRY(hwc_u8_to_planar(h, stage, Lp[0], H, W, C, nF));
    else
        PAPOF_TRY(hwc_to_planar(h, reinterpret_cast<const double*>(stage), Lp[0], H, W, C, nF));
    for (int i = 1; i < levels; i++)
        PAPOF_TRY(smooth_and_resize(h, Lp[plan[i].src_level], Lp[i], tmp_a, tmp_b, plan[i], C * nF, L[i].h, L[i].w));
    const Taps g5 = smooth5_taps();
    const bool nz_known = guard && (size_t)levels * 8 <= (size_t)kLapNzWords;
    for (int k = 0; k < levels; k++) {
        PAPOF_TRY(im2feature(h, Lp[k], F[k], L[k].h, L[k].w, C, nz_known ? nzf + (size_t)k * 8 : nullptr, nF, kLapNzWords));
        PAPOF_TRY(filter_hv(h, F[k], S[k], nullptr, L[k].h, L[k].w, fc * nF, g5, g5));
    }
    PAPOF_TRY(central3_planes(h, Lp[0], gx, gy, gxy, H, W, C * nF));

    // ---- levels, coarse to fine (src/OpticalFlow.cpp:784-823); (u, v) of pair p: planes 2p, 2p + 1 at the level's pitch
    double *uv = uvA, *uv2 = uvB;
    int pw = 0, ph = 0, slot = 0;
    std::vector<int> slot_level;
    h->sor_mark = [](void* c, int on) { static_cast<PhaseClock*>(c)->phase(on ? PAPOF_T_PHASE5_SOR : -1); };
    h->sor_mark_ctx = &sorclk;
    const auto levels_loop = [&]() -> int {
        for (int k = levels - 1; k >= 0; k--) {
            const int lw = L[k].w, lh = L[k].h;
            const size_t np = (size_t)lw * lh;
            const int K = cp.n_sor[k], n_outer = cp.n_outer[k];
            if (k == levels - 1 && (frames.init_fw || frames.init_bw)) {
                // the caller's initial flows of all pairs (reduce_init): uvA, uvB and the warped image are free until here
                double* r = nullptr;
                PAPOF_TRY(reduce_init(h, frames.init_fw, frames.init_bw, B, with_bw ? B : 0, H, W, L, plan, ratio, uvB, uvA, warp,
                                      (size_t)NP * C, r));
                if (r != uv) std::swap(uv, uv2);
            } else if (k == levels - 1) {
                PAPOF_HIP(hipMemsetAsync(uv, 0, (size_t)NP * 2 * np * sizeof(double), st));  // :801-806 (the warp is folded in)
            } else {  // :809-812: bilinear up-sampling times 1 / ratio, all pairs' u and v in one launch
                PAPOF_TRY(resize(h, uv, uv2, ph, pw, 2 * NP, lh, lw, (double)lw / pw, (double)lh / ph, true, 1 / ratio));
                std::swap(uv, uv2);
            }
            const bool tiny = tiny_level(k);
            SorPlanes sp = tiny ? ST[0] : SP[0];
            if (!tiny) {
                PAPOF_TRY(sor_bind_plain(h, sp, lh, lw, K));
                PAPOF_TRY(sor_reset_planes_batch(h, sp, NP, sp_stride));
            }
            BatchK bk{};
            bk.im = (size_t)fstep * np * fc;
            bk.uv = 2 * np;
            bk.sp = tiny ? st_stride : sp_stride;
            bk.d = tiny ? st_stride : spd_stride;
            bk.wit = kLapFlagWords;
            bk.bw = with_bw ? B : 0;
            bk.fr = np * fc;
            const SorBatch bt{NP, sp_stride, spd_stride, LC.lv[k].per, st_stride};
            const double *f1 = F[k], *f2 = F[k] + np * fc, *s1 = S[k];
            // Few-pixel levels (the deep end of an 8- or 15-level pyramid): the flow leaves the image altogether in some iterations,
            // every warped value is then frame 1's and there is NO valid sample -- which only a look at every pixel can tell from
            // "no witness among the samples".  There the estimate behind EVERY update is checked exhaustively (one small block per
            // pair and channel): a witness, or the constant 0.001 (kLapNone).
            const bool exhaustive = guard && np <= 4096;
            for (int count = 0; count < n_outer; count++) {
                unsigned* const w_prev = guard && !exhaustive && count > 0 ? wit + lap_wit_word(slot - 1) : nullptr;
                PAPOF_TRY(flow_system(h, f1, f2, uv, uv + np, s1, lh, lw, fc, P.alpha, P.omega, sp, w_prev, 0, -1, NP, &bk));
                h->sor_prog_next = tiny ? nullptr : LC.solve(h, k, (size_t)count * NP);  // the NP pairs' counters of this solve
                const int rc = sor_solve(h, sp, lh, lw, P.alpha, P.omega, K, PAPOF_SOR_EXACT, &bt);
                h->sor_prog_next = nullptr;
                PAPOF_TRY(rc);
                // the estimate behind the level's last update is witnessed by the update kernel itself (nobody evaluates that warp)
                unsigned* const w_now = guard && !exhaustive && count + 1 == n_outer ? wit + lap_wit_word(slot) : nullptr;
                PAPOF_TRY(update_warp_phi(h, sp, uv, uv + np, uv2, uv2 + np, f1, f2, nullptr, nullptr, lh, lw, fc, false, 0, -1,
                                          w_now, NP, &bk));
                std::swap(uv, uv2);
                if (exhaustive) PAPOF_TRY(lap_small_check(h, f1, f2, uv, uv + np, lh, lw, fc, wit + lap_wit_word(slot), NP, &bk));
                slot_level.push_back(k);
                slot++;
            }
            pw = lw;
            ph = lh;
        }
        // ---- :841-842: bicubic warp of the ORIGINAL frame 2 of every pair, clamped to [0, 1]
        BatchK bk{};
        bk.im = (size_t)fstep * np0 * C;
        bk.uv = 2 * np0;
        bk.out = np0 * C;
        bk.bw = with_bw ? B : 0;
        bk.fr = np0 * C;
        PAPOF_TRY(bicubic_warp(h, Lp[0], Lp[0] + np0 * C, gx + np0 * C, gy + np0 * C, gxy + np0 * C, uv, uv + np0, warp, H, W, C,
                               nullptr, false, true, NP, &bk));
        return PAPOF_OK;
    };
    const int rc_levels = levels_loop();
    h->sor_mark = nullptr;
    h->sor_mark_ctx = nullptr;
    total.phase(-1);
    if (rc_levels != PAPOF_OK) {
        hipStreamSynchronize(st);
        return rc_levels;
    }
    std::vector<unsigned> hw, hn;
    PAPOF_HIP(hipStreamSynchronize(st));
    PAPOF_TRY(sor_check(h));
    if (guard) {
        hw.resize((size_t)NP * kLapFlagWords);
        hn.resize((size_t)nF * kLapNzWords);
        PAPOF_HIP(hipMemcpy(hw.data(), wit, hw.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        PAPOF_HIP(hipMemcpy(hn.data(), nzf, hn.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (int p = 0; p < NP; p++) {
            bool open = true;
            const bool back = p >= B;  // a backward pair: the frames of pair p - B, exchanged
            const int f1 = (back ? p - B : p) * fstep, fa = back ? f1 + 1 : f1, fb = back ? f1 : f1 + 1;
            for (int s = 0; s + 1 < slot && open; s++)  // the estimate behind the call's last update is never consulted
                for (int c = 0; c < fc; c++) {
                    // (beyond kLapNzWords / 8 levels there are no non-zero flags, and no words to read them from)
                    const size_t nzw = nz_known ? (size_t)slot_level[s] * 8 + c : 0;
                    if (!lap_proven(hw[(size_t)p * kLapFlagWords + lap_wit_word(s) + c], epoch, nz_known,
                                    hn[(size_t)fa * kLapNzWords + nzw], hn[(size_t)fb * kLapNzWords + nzw]))
                        open = false;
                }
            if (!open) out.unproven.push_back(p);
        }
    }
    PAPOF_TRY(collect_total_and_sor(total, sorclk, timing));
    out.uv = uv;
    out.warp = warp;
    return PAPOF_OK;
}

}  // namespace

int flow_batch_host(papof_handle* h, int n_pairs, int sequence, const void* const* frames, bool u8, int H, int W, int C, int levels,
                    const papof_params* params, double* const* vx, double* const* vy, double* const* warpI2, double* timing_sec) {
    if (!h || n_pairs < 1 || !frames || !vx || !vy || !warpI2 || H < 1 || W < 1 || C < 1 || levels < 1) return PAPOF_EINVAL;
    const int nF = sequence ? n_pairs + 1 : 2 * n_pairs;
    for (int f = 0; f < nF; f++)
        if (!frames[f]) return PAPOF_EINVAL;
    for (int p = 0; p < n_pairs; p++)
        if (!vx[p] || !vy[p] || !warpI2[p]) return PAPOF_EINVAL;
    const papof_params P = params_or_default(params);
    PAPOF_TRY(check_params(P, levels));
    PAPOF_HIP(hipSetDevice(h->device));
    const double t0 = now_sec();
    double tm[PAPOF_N_TIMERS];
    std::memset(tm, 0, sizeof tm);
    const auto single = [&](int p) -> int {  // the ordinary call on pair p (it has every branch, and the guard's exact pass)
        const void* a = frames[sequence ? p : 2 * p];
        const void* b = frames[sequence ? p + 1 : 2 * p + 1];
        double t1[PAPOF_N_TIMERS];
        const int rc = u8 ? papof_flow_u8(h, (const unsigned char*)a, (const unsigned char*)b, H, W, C, levels, &P, vx[p], vy[p],
                                          warpI2[p], t1)
                          : papof_flow(h, (const double*)a, (const double*)b, H, W, C, levels, &P, vx[p], vy[p], warpI2[p], t1);
        if (rc == PAPOF_OK)
            for (int i = 0; i < PAPOF_N_TIMERS; i++) tm[i] += t1[i];
        return rc;
    };
    const auto all_single = [&]() -> int {  // the pairs one after the other
        h->batch_singles += n_pairs;
        for (int p = 0; p < n_pairs; p++) PAPOF_TRY(single(p));
        if (timing_sec) std::memcpy(timing_sec, tm, sizeof tm);
        return PAPOF_OK;
    };
    if (!batch_applies(h, n_pairs, H, W, C, levels, P)) return all_single();
    // sub-batches (batch_max)
    {
        const int max_b = batch_max(H, W, C, levels, P);
        if (n_pairs > max_b) {
            const int step = sequence ? 1 : 2;
            for (int p0 = 0; p0 < n_pairs;) {
                int nb_ = std::min(max_b, n_pairs - p0);
                if (n_pairs - (p0 + nb_) == 1 && nb_ > 2) nb_ -= 1;  // leave two pairs for the last sub-batch rather than one
                double t1[PAPOF_N_TIMERS];
                PAPOF_TRY(flow_batch_host(h, nb_, sequence, frames + (size_t)p0 * step, u8, H, W, C, levels, &P, vx + p0, vy + p0,
                                          warpI2 + p0, t1));
                for (int i = 0; i < PAPOF_N_TIMERS; i++) tm[i] += t1[i];
                p0 += nb_;
            }
            if (timing_sec) std::memcpy(timing_sec, tm, sizeof tm);
            return PAPOF_OK;
        }
    }
    BatchOut out;
    {
        BatchFrames bf;
        bf.host = frames;
        bf.u8 = u8;
        const int rc = flow_batch_device(h, n_pairs, sequence, false, bf, H, W, C, levels, P, tm, out);
        if (rc == PAPOF_ENOMEM) {  // no room for the arrays of a batch on this device
            std::memset(tm, 0, sizeof tm);
            return all_single();
        }
        PAPOF_TRY(rc);
        h->batch_chains++;
        h->batch_chain_pairs += n_pairs;
    }
    const size_t np0 = (size_t)H * W;
    // Result arrays laid out as the device's ([pair][vx, vy][H x W] and [pair][H x W x c] in one block each -- what the Python
    // binding allocates, page-locked) come back as TWO copies; anything else as three per pair.
    bool flat = true;
    for (int p = 0; p < n_pairs && flat; p++)
        flat = vx[p] == vx[0] + (size_t)p * 2 * np0 && vy[p] == vx[p] + np0 && warpI2[p] == warpI2[0] + (size_t)p * np0 * C;
    if (flat) {
        PAPOF_HIP(hipMemcpyAsync(vx[0], out.uv, (size_t)n_pairs * 2 * np0 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        PAPOF_HIP(hipMemcpyAsync(warpI2[0], out.warp, (size_t)n_pairs * np0 * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        for (int p = 0; p < n_pairs; p++) {
            PAPOF_HIP(hipMemcpyAsync(vx[p], out.uv + (size_t)p * 2 * np0, np0 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            PAPOF_HIP(hipMemcpyAsync(vy[p], out.uv + (size_t)p * 2 * np0 + np0, np0 * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
            PAPOF_HIP(hipMemcpyAsync(warpI2[p], out.warp + (size_t)p * np0 * C, np0 * C * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
        }
    }
    PAPOF_HIP(hipStreamSynchronize(h->stream));
    for (int p : out.unproven) {
        h->lap_reruns++;
        h->batch_reruns++;
        PAPOF_TRY(single(p));
    }
    tm[PAPOF_T_TOTAL] = now_sec() - t0;  // the caller's view: uploads, the launch chain, downloads, re-runs
    if (timing_sec) std::memcpy(timing_sec, tm, sizeof tm);
    return PAPOF_OK;
}

namespace {

papof_tensor shifted(const papof_tensor& t, long long items) {  // the same tensor from item `items` of its first axis on
    papof_tensor r = t;
    r.data = static_cast<char*>(t.data) + items * t.stride[0] * dtype_bytes(t.dtype);
    return r;
}

// the descriptors of the tensor calls: frames of any dtype (a zero stride: an expanded tensor), and the float32 / float64 flow
// and warp outputs, every stride positive
const std::initializer_list<int> kAxes = {0, 1, 2, 3}, kFloat = {PAPOF_DTYPE_F32, PAPOF_DTYPE_F64};
bool valid_frames(const papof_tensor* t) {
    return described(t, {PAPOF_DTYPE_U8, PAPOF_DTYPE_F32, PAPOF_DTYPE_F64}, kAxes, false);
}
bool valid_output(const papof_tensor* t) { return described(t, kFloat, kAxes, true); }

// The outputs of papof_flow_batch_tensor (flow, warp) and of papof_flow_batch_tensor_fb (also the backward pairs' flow_bw,
// warp_bw and, when occ is given, the forward-backward check with a1, a2).
struct TensorOut {
    const papof_tensor* flow = nullptr;
    const papof_tensor* warp = nullptr;
    const papof_tensor* flow_bw = nullptr;  // NULL: forward pairs only
    const papof_tensor* warp_bw = nullptr;
    const papof_tensor* occ = nullptr;
    double a1 = 0, a2 = 0;
};

// the caller's initial flows (papof_flow_batch_tensor_init, _fb_init): of the forward pairs, of the backward pairs; NULL: zero
struct TensorInit {
    const papof_tensor* fw = nullptr;
    const papof_tensor* bw = nullptr;
};

papof_tensor planar_flow(const double* uv, int H, int W) {  // the chain's [pair][2][H * W] fp64 flows as a tensor
    papof_tensor t;
    t.data = const_cast<double*>(uv);
    t.dtype = PAPOF_DTYPE_F64;
    t.stride[0] = 2LL * H * W;
    t.stride[1] = W;
    t.stride[2] = 1;
    t.stride[3] = (long long)H * W;
    return t;
}

// papof_flow_batch_tensor(_fb) behind its checks and its entry wait: flow_batch_host's orchestration on device tensors.  The
// frames are read where they are (k_ingest_frames), the results leave the arena through k_emit_outputs before anything else
// runs on it, and what the batched chain does not cover runs pair by pair on the device.  With backward pairs, a sub-batch of
// nb frame pairs is 2nb solver pairs (the batch bound counts solver pairs), and the forward-backward check runs on the fp64
// flows before anything else is laid out in the arena (or the scratch) -- the mask does not depend on the output dtype.
// tm accumulates the phases.
int flow_batch_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor& fa, const papof_tensor* fb, int H, int W,
                      int C, int levels, const papof_params& P, const TensorOut& o, const TensorInit& ini, double* tm) {
    const size_t np0 = (size_t)H * W, frame = np0 * C;
    const bool with_bw = o.flow_bw != nullptr;
    // an initial flow from pair p on, in `buf` (NULL where there is none)
    const auto init_at = [](const papof_tensor* t, int p, papof_tensor& buf) -> const papof_tensor* {
        if (!t) return nullptr;
        buf = shifted(*t, p);
        return &buf;
    };
    // one pair on its own: its two frames into the handle's scratch (planar fp64; not in the arena, which the single call lays
    // out anew), the device call (both passes of the guard), the results out; with backward pairs, the single call on the
    // exchanged frames as well, and the check on the two fp64 flows
    const auto single = [&](int p) -> int {
        const size_t bytes = (with_bw ? 2 * frame + 4 * np0 + 2 * frame : 2 * frame + 2 * np0 + frame) * sizeof(double);
        if (h->tensor_scratch_bytes < bytes) {
            if (h->tensor_scratch) {
                PAPOF_HIP(hipStreamSynchronize(h->stream));
                PAPOF_HIP(hipFree(h->tensor_scratch));
            }
            h->tensor_scratch = nullptr;
            h->tensor_scratch_bytes = 0;
            if (hipMalloc((void**)&h->tensor_scratch, bytes) != hipSuccess) {
                h->tensor_scratch = nullptr;
                return PAPOF_ENOMEM;
            }
            h->tensor_scratch_bytes = bytes;
        }
        double *f = h->tensor_scratch, *uv = f + 2 * frame, *wp = uv + (with_bw ? 4 : 2) * np0;
        const papof_tensor a = shifted(fa, p);
        if (sequence) {
            PAPOF_TRY(ingest_frames(h, a, nullptr, f, H, W, C, 2));
        } else {
            const papof_tensor b = shifted(*fb, p);
            PAPOF_TRY(ingest_frames(h, a, &b, f, H, W, C, 2));
        }
        double t1[PAPOF_N_TIMERS];
        papof_tensor ifw, ibw;
        PAPOF_TRY(flow_device_planar(h, f, f + frame, H, W, C, levels, P, uv, uv + np0, wp, t1, init_at(ini.fw, p, ifw)));
        PAPOF_TRY(emit_outputs(h, uv, shifted(*o.flow, p), true, H, W, 2, 1));
        PAPOF_TRY(emit_outputs(h, wp, shifted(*o.warp, p), false, H, W, C, 1));
        for (int i = 0; i < PAPOF_N_TIMERS; i++) tm[i] += t1[i];
        if (with_bw) {
            double *uvb = uv + 2 * np0, *wpb = wp + frame;
            PAPOF_TRY(flow_device_planar(h, f + frame, f, H, W, C, levels, P, uvb, uvb + np0, wpb, t1, init_at(ini.bw, p, ibw)));
            PAPOF_TRY(emit_outputs(h, uvb, shifted(*o.flow_bw, p), true, H, W, 2, 1));
            PAPOF_TRY(emit_outputs(h, wpb, shifted(*o.warp_bw, p), false, H, W, C, 1));
            for (int i = 0; i < PAPOF_N_TIMERS; i++) tm[i] += t1[i];
            if (o.occ)
                PAPOF_TRY(fb_check(h, h->stream, planar_flow(uv, H, W), planar_flow(uvb, H, W), shifted(*o.occ, p), 1, H, W, o.a1,
                                   o.a2));
        }
        return PAPOF_OK;
    };
    if (!batch_applies(h, n_pairs, H, W, C, levels, P)) {
        h->batch_singles += n_pairs;
        for (int p = 0; p < n_pairs; p++) PAPOF_TRY(single(p));
        return PAPOF_OK;
    }
    const int max_b = with_bw ? std::max(1, batch_max(H, W, C, levels, P) / 2) : batch_max(H, W, C, levels, P);
    for (int p0 = 0; p0 < n_pairs;) {
        int nb = std::min(max_b, n_pairs - p0);
        if (n_pairs - (p0 + nb) == 1 && nb > 2) nb -= 1;  // leave two pairs for the last sub-batch rather than one
        if (nb == 1 && !with_bw) {  // a bound of two leaves an odd collection's last pair alone: the single call, as the host entry's
            h->batch_singles++;
            PAPOF_TRY(single(p0));
            p0 += 1;
            continue;
        }
        const papof_tensor a = shifted(fa, p0), b = sequence ? a : shifted(*fb, p0);
        BatchFrames bf;
        bf.a = &a;
        bf.b = sequence ? nullptr : &b;
        papof_tensor ifw, ibw;
        bf.init_fw = init_at(ini.fw, p0, ifw);
        bf.init_bw = with_bw ? init_at(ini.bw, p0, ibw) : nullptr;
        BatchOut out;
        double t1[PAPOF_N_TIMERS];
        const int rc = flow_batch_device(h, nb, sequence, with_bw, bf, H, W, C, levels, P, t1, out);
        if (rc == PAPOF_ENOMEM) {  // no room for the arrays of a batch on this device: the pairs one after the other
            h->batch_singles += nb;
            for (int p = p0; p < p0 + nb; p++) PAPOF_TRY(single(p));
            p0 += nb;
            continue;
        }
        PAPOF_TRY(rc);
        h->batch_chains++;
        h->batch_chain_pairs += with_bw ? 2 * nb : nb;
        for (int i = 0; i < PAPOF_N_TIMERS; i++) tm[i] += t1[i];
        PAPOF_TRY(emit_outputs(h, out.uv, shifted(*o.flow, p0), true, H, W, 2, nb));
        PAPOF_TRY(emit_outputs(h, out.warp, shifted(*o.warp, p0), false, H, W, C, nb));
        if (!with_bw) {
            for (int p : out.unproven) {
                h->lap_reruns++;
                h->batch_reruns++;
                PAPOF_TRY(single(p0 + p));
            }
            p0 += nb;
            continue;
        }
        const double* uvb = out.uv + (size_t)nb * 2 * np0;
        PAPOF_TRY(emit_outputs(h, uvb, shifted(*o.flow_bw, p0), true, H, W, 2, nb));
        PAPOF_TRY(emit_outputs(h, out.warp + (size_t)nb * frame, shifted(*o.warp_bw, p0), false, H, W, C, nb));
        if (o.occ)
            PAPOF_TRY(fb_check(h, h->stream, planar_flow(out.uv, H, W), planar_flow(uvb, H, W), shifted(*o.occ, p0), nb, H, W,
                               o.a1, o.a2));
        // an unproven solver pair -- forward pair q or backward pair nb + q -- runs again through the single call; both
        // directions of frame pair q do, because its mask needs both fp64 flows and the arena does not outlive the single call
        std::vector<char> redo(nb, 0);
        for (int p : out.unproven) {
            h->lap_reruns++;
            redo[p < nb ? p : p - nb] = 1;
        }
        for (int q = 0; q < nb; q++)
            if (redo[q]) {
                h->batch_reruns++;  // frame pairs, whichever of the two directions lacked its proof
                PAPOF_TRY(single(p0 + q));
            }
        p0 += nb;
    }
    return PAPOF_OK;
}

// the entry of papof_flow_batch_tensor(_fb) after the descriptors' checks: parameters, entry wait, the call, complete on return
int tensor_entry(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2, int height,
                 int width, int c, int pyramid_levels, const papof_params* params, const TensorOut& o, void* stream,
                 double* timing_sec, const TensorInit& ini) {
    const papof_params P = params_or_default(params);
    PAPOF_TRY(check_params(P, pyramid_levels));
    PAPOF_HIP(hipSetDevice(h->device));
    const double t0 = now_sec();
    // stream order on entry: the handle's streams (non-blocking, hence also for the null stream) start behind what the caller
    // has queued so far
    if (!h->entry_event) PAPOF_HIP(hipEventCreateWithFlags(&h->entry_event, hipEventDisableTiming));
    PAPOF_HIP(hipEventRecord(h->entry_event, static_cast<hipStream_t>(stream)));
    PAPOF_HIP(hipStreamWaitEvent(h->stream, h->entry_event, 0));
    if (h->prep_stream) PAPOF_HIP(hipStreamWaitEvent(h->prep_stream, h->entry_event, 0));
    if (ini.fw || ini.bw) {  // the initial flows' values, behind the entry wait and before anything is written: refused -> EINVAL
        if (!h->init_flag_dev) PAPOF_HIP(hipMalloc((void**)&h->init_flag_dev, sizeof(unsigned)));
        PAPOF_HIP(hipMemsetAsync(h->init_flag_dev, 0, sizeof(unsigned), h->stream));
        for (const papof_tensor* t : {ini.fw, ini.bw})
            if (t) PAPOF_TRY(init_check(h, *t, n_pairs, height, width, h->init_flag_dev));
        unsigned refused = 0;
        PAPOF_HIP(hipMemcpyAsync(&refused, h->init_flag_dev, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        PAPOF_HIP(hipStreamSynchronize(h->stream));
        if (refused) return PAPOF_EINVAL;
    }
    double tm[PAPOF_N_TIMERS];
    std::memset(tm, 0, sizeof tm);
    const int rc = flow_batch_tensor(h, n_pairs, sequence, *frames, frames2, height, width, c, pyramid_levels, P, o, ini, tm);
    const hipError_t se = hipStreamSynchronize(h->stream);  // complete on return: the emits are the last work of the call
    PAPOF_TRY(rc);
    if (se != hipSuccess) {
        set_last_error("hipStreamSynchronize", se, __FILE__, __LINE__);
        return PAPOF_EDEVICE;
    }
    tm[PAPOF_T_TOTAL] = now_sec() - t0;  // the caller's view
    if (timing_sec) std::memcpy(timing_sec, tm, sizeof tm);
    return PAPOF_OK;
}

}  // namespace

}  // namespace papof

using namespace papof;

extern "C" {

int papof_flow_batch(papof_handle* h, int n_pairs, int sequence, const double* const* frames, int height, int width, int c,
                     int pyramid_levels, const papof_params* params, double* const* vx, double* const* vy, double* const* warpI2,
                     double timing_sec[PAPOF_N_TIMERS]) {
    return flow_batch_host(h, n_pairs, sequence, reinterpret_cast<const void* const*>(frames), false, height, width, c,
                           pyramid_levels, params, vx, vy, warpI2, timing_sec);
}

int papof_flow_batch_u8(papof_handle* h, int n_pairs, int sequence, const unsigned char* const* frames, int height, int width,
                        int c, int pyramid_levels, const papof_params* params, double* const* vx, double* const* vy,
                        double* const* warpI2, double timing_sec[PAPOF_N_TIMERS]) {
    return flow_batch_host(h, n_pairs, sequence, reinterpret_cast<const void* const*>(frames), true, height, width, c,
                           pyramid_levels, params, vx, vy, warpI2, timing_sec);
}

int papof_flow_batch_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2,
                            int height, int width, int c, int pyramid_levels, const papof_params* params, const papof_tensor* flow,
                            const papof_tensor* warpI2, void* stream, double timing_sec[PAPOF_N_TIMERS]) {
    return papof_flow_batch_tensor_init(h, n_pairs, sequence, frames, frames2, height, width, c, pyramid_levels, params, nullptr, flow,
                                        warpI2, stream, timing_sec);
}

int papof_flow_batch_tensor_fb(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                               const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                               const papof_params* params, const papof_tensor* flow_fw, const papof_tensor* warp_fw,
                               const papof_tensor* flow_bw, const papof_tensor* warp_bw, const papof_tensor* occlusion,
                               double alpha1, double alpha2, void* stream, double timing_sec[PAPOF_N_TIMERS]) {
    return papof_flow_batch_tensor_fb_init(h, n_pairs, sequence, frames, frames2, height, width, c, pyramid_levels, params, nullptr,
                                           nullptr, flow_fw, warp_fw, flow_bw, warp_bw, occlusion, alpha1, alpha2, stream,
                                           timing_sec);
}

int papof_flow_batch_tensor_init(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                 const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                                 const papof_params* params, const papof_tensor* init, const papof_tensor* flow,
                                 const papof_tensor* warpI2, void* stream, double timing_sec[PAPOF_N_TIMERS]) {
    if (!h || n_pairs < 1 || height < 1 || width < 1 || c < 1 || pyramid_levels < 1) return PAPOF_EINVAL;
    if (!valid_frames(frames) || !valid_output(flow) || !valid_output(warpI2)) return PAPOF_EINVAL;
    if (sequence ? frames2 != nullptr : !valid_frames(frames2)) return PAPOF_EINVAL;
    if (init && !described(init, kFloat, kAxes, false)) return PAPOF_EINVAL;
    return tensor_entry(h, n_pairs, sequence, frames, frames2, height, width, c, pyramid_levels, params,
                        TensorOut{.flow = flow, .warp = warpI2}, stream, timing_sec, TensorInit{.fw = init});
}

int papof_flow_batch_tensor_fb_init(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                    const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                                    const papof_params* params, const papof_tensor* init_fw, const papof_tensor* init_bw,
                                    const papof_tensor* flow_fw, const papof_tensor* warp_fw, const papof_tensor* flow_bw,
                                    const papof_tensor* warp_bw, const papof_tensor* occlusion, double alpha1, double alpha2,
                                    void* stream, double timing_sec[PAPOF_N_TIMERS]) {
    if (!h || n_pairs < 1 || height < 1 || width < 1 || c < 1 || pyramid_levels < 1) return PAPOF_EINVAL;
    if (!valid_frames(frames) || !valid_output(flow_fw) || !valid_output(warp_fw) || !valid_output(flow_bw) ||
        !valid_output(warp_bw))
        return PAPOF_EINVAL;
    if (sequence ? frames2 != nullptr : !valid_frames(frames2)) return PAPOF_EINVAL;
    if (occlusion && !described(occlusion, {PAPOF_DTYPE_U8}, kAxes, true)) return PAPOF_EINVAL;
    if (!valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    if ((init_fw && !described(init_fw, kFloat, kAxes, false)) || (init_bw && !described(init_bw, kFloat, kAxes, false)))
        return PAPOF_EINVAL;
    const TensorOut o{.flow = flow_fw, .warp = warp_fw, .flow_bw = flow_bw, .warp_bw = warp_bw, .occ = occlusion, .a1 = alpha1,
                      .a2 = alpha2};
    return tensor_entry(h, n_pairs, sequence, frames, frames2, height, width, c, pyramid_levels, params, o, stream, timing_sec,
                        TensorInit{.fw = init_fw, .bw = init_bw});
}

int papof_batch_stats(papof_handle* h, long long out[4]) {
    if (!h || !out) return PAPOF_EINVAL;
    out[0] = h->batch_chains;
    out[1] = h->batch_chain_pairs;
    out[2] = h->batch_singles;
    out[3] = h->batch_reruns;
    return PAPOF_OK;
}

int papof_fb_check_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow_fw,
                          const papof_tensor* flow_bw, double alpha1, double alpha2, const papof_tensor* occlusion,
                          void* stream) {
    if (!h || n_pairs < 1 || height < 1 || width < 1) return PAPOF_EINVAL;
    if (!described(flow_fw, kFloat, kAxes, false) || !described(flow_bw, kFloat, kAxes, false)) return PAPOF_EINVAL;
    if (!described(occlusion, {PAPOF_DTYPE_U8}, kAxes, true) || !valid_alphas(alpha1, alpha2)) return PAPOF_EINVAL;
    PAPOF_HIP(hipSetDevice(h->device));
    return fb_check(h, static_cast<hipStream_t>(stream), *flow_fw, *flow_bw, *occlusion, n_pairs, height, width, alpha1, alpha2);
}

}  // extern "C"
