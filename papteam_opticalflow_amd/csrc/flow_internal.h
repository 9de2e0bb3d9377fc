// papteam_opticalflow_amd/csrc/flow_internal.h -- pieces of the orchestrator (api.hip) shared with the batched
// (batch.hip) and the multi-GPU (tiles.hip) orchestrators.  Internal; nothing here is part of the C ABI.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace papof {

void set_last_error_text(const std::string& text);

// ---- phase timers ----
// Event mode (default): every phase boundary is a HIP event recorded on the handle's current stream (no synchronisation).
// Stamp mode (`stamps`, the main-stream clock of flow_device): a phase boundary costs NOTHING on the stream -- the first
// kernel launched after phase() writes the GPU's constant 100 MHz clock into a slot when it starts
// (kernels.hip: stamp_now; device memory, copied back once at the end of the call: a kernel that writes host-mapped
// memory pays for it when it ends), and a phase lasts from its stamp to the next one.  A HIP event between two kernels costs
// ~2.6 us of stream time, and a call has ~100 phase boundaries: measured 11.8 vs 11.5 ms per 1080p pair.  Only
// Phase5_SOR keeps a HIP event pair as well (the roofline of the dominant kernel is priced on those events).
// Internal eleventh timer (arrays handed to PhaseClock::collect hold PAPOF_N_TIMERS + 1 values): the kernel that does the work
// of Phase1 ... Phase4 in one launch (kernels.hip: k_flow_system); api.hip apportions it to those four when it reports.
constexpr int kTimerFused = PAPOF_N_TIMERS;
struct PhaseClock {
    papof_handle* h;
    bool on;
    std::vector<std::pair<int, std::pair<size_t, size_t>>> spans;  // (timer index, (event a, event b))
    size_t open = 0;
    int open_idx = -1;
    int err = PAPOF_OK;
    bool only_sor = false;  // measurement aid (PAPOF_PHASE_EVENTS=0): nothing but Phase5_SOR (and the total) is measured
    bool stamps = false;
    std::vector<std::pair<int, int>> marks;  // stamp mode: (slot, timer index) in stream order
    std::vector<double> sor_span_sec;        // collect(): seconds of every Phase5_SOR span, in stream order (one per solve)
    std::vector<int> sor_owner;              // stamp mode: the timer whose span runs across that solve (see phase())
    size_t new_event() {
        if (h->events_used == h->events.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) {
                err = PAPOF_EDEVICE;
                return 0;
            }
            h->events.push_back(e);
        }
        hipEventRecord(h->events[h->events_used], h->stream);
        return h->events_used++;
    }
    // close the running span (if any) and open a new one attributed to timer `idx` (-1: none)
    void phase(int idx) {
        if (!on) return;
        if (stamps) {
            if (open_idx == PAPOF_T_PHASE5_SOR) {
                const size_t e = new_event();
                spans.push_back({PAPOF_T_PHASE5_SOR, {open, e}});
            }
            if (idx == PAPOF_T_PHASE5_SOR) {
                open = new_event();
                sor_owner.push_back(marks.empty() ? PAPOF_T_PHASE4_LINEARSYSTEM : marks.back().second);
            }
            const bool sor_edge = idx == PAPOF_T_PHASE5_SOR;
            open_idx = idx;
            // The solver kernels carry no stamp (a store at the head of the critical task of the exact-order kernels was
            // measured to cost ~12 us per solve): the span that contains a solve keeps running as Phase4 (or kTimerFused) until
            // the update kernel's stamp, and collect() subtracts the solver's own (event-measured) time from it.
            if (only_sor || !h->stamps_dev || sor_edge) return;
            if (h->next_stamp && !marks.empty()) {
                marks.back().second = idx;  // no stamping kernel ran in the previous phase: it is absorbed by its predecessor
            } else if (h->stamps_used < h->stamps_cap) {
                const int slot = h->stamps_used++;
                h->next_stamp = h->stamps_dev + slot;
                marks.push_back({slot, idx});
            }
            return;
        }
        if (only_sor && idx != PAPOF_T_PHASE5_SOR && idx != PAPOF_T_TOTAL) {
            if (open_idx < 0) return;  // nothing running: no event needed
            idx = -1;
        }
        const size_t e = new_event();
        if (open_idx >= 0) spans.push_back({open_idx, {open, e}});
        open = e;
        open_idx = idx;
    }
    void collect(double* t) {  // after the stream has drained
        if (!on) return;
        for (auto& s : spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, h->events[s.second.first], h->events[s.second.second]) == hipSuccess)
                t[s.first] += ms * 1e-3;
            if (s.first == PAPOF_T_PHASE5_SOR) sor_span_sec.push_back(ms * 1e-3);
        }
        // h->stamps holds the slots 0 .. stamps_fetched-1 (copied back by fetch_stamps() before the stream was drained)
        for (size_t i = 0; i + 1 < marks.size(); i++) {
            const int idx = marks[i].second;
            if (marks[i + 1].first >= h->stamps_fetched) break;
            const unsigned long long a = h->stamps[marks[i].first], b = h->stamps[marks[i + 1].first];
            if (idx >= 0 && idx != PAPOF_T_PHASE5_SOR && b >= a) t[idx] += (double)(b - a) * 1e-8;  // 100 MHz ticks
        }
        if (stamps && !marks.empty()) {  // the spans that ran across the solves: take the solver kernels' time out
            for (size_t i = 0; i < sor_span_sec.size() && i < sor_owner.size(); i++)
                if (sor_owner[i] >= 0) t[sor_owner[i]] -= sor_span_sec[i];
            for (int own : {(int)PAPOF_T_PHASE4_LINEARSYSTEM, kTimerFused})
                if (t[own] < 0.0) t[own] = 0.0;
        }
    }
};

// The Laplacian-noise guard's verdict on ONE consulted estimate (api.hip: LapGuard; a flag is set when it holds the number
// of the pass, `epoch`): it is proven by a witness -- a sample, or kLapNone: an exhaustive "no valid sample at all" -- or by a
// channel that is all zero in both frames of the level (nz_known: im2feature collected the non-zero flags; nz_a, nz_b: the
// channel's flag words of the two frames, one and the same word where the frames share their flags)
inline bool lap_proven(unsigned wit, unsigned epoch, bool nz_known, unsigned nz_a, unsigned nz_b) {
    const bool witness = wit == epoch || wit == (epoch ^ kLapNone);
    const bool all_zero = nz_known && nz_a != epoch && nz_b != epoch;
    return witness || all_zero;
}

struct Level {
    int w, h;
    double *p1, *p2;  // planar pyramid levels of frame 1 / frame 2
};
// how GaussianPyramid::ConstructPyramidLevels (src/GaussianPyramid.cpp:79-108) derives a level: source level, filter, rate
struct PyrPlan {
    int sw, sh, src_level, fsize;
    double sigma, rate;
};

// ---- the call plan: what every orchestrator (flow_pass, flow_batch_device, tiles_flow, bands_flow) derives from
// (H, W, C, levels, P) before it touches the device ----
inline double effective_ratio(double ratio) { return ratio > 0.98 || ratio < 0.4 ? 0.75 : ratio; }  // src/GaussianPyramid.cpp:82-83
papof_params params_or_default(const papof_params* params);  // the caller's parameter block, or papof_default_params()
struct CallPlan {
    double ratio = 0.75;  // the effective one
    int levels = 0, fc = 0;
    std::vector<Level> L;
    std::vector<PyrPlan> plan;
    std::vector<int> n_sor, n_outer;  // the schedule of level k (src/OpticalFlow.cpp:784-823 as the Python entry point drives it)
    int n_sor_max = 0;                // ... and its largest sweep count, the coarsest level's
    long slots = 0;                   // outer iterations of the whole call: the Laplacian-noise guard's witness slots
    bool from_level0 = true;          // every pyramid level is derived from level 0 (else deeper ones chain through finer levels)
    static int n_sor_at(const papof_params& P, int k) { return P.n_sor + k * P.n_sor_per_level; }
    static int n_outer_at(const papof_params& P, int k) { return P.n_outer + k * P.n_outer_per_level; }
    static long slots_for(const papof_params& P, int levels) {
        long s = 0;
        for (int k = 0; k < levels; k++) s += n_outer_at(P, k);
        return s;
    }
};
int call_plan(int H, int W, int C, int levels, const papof_params& P, CallPlan& cp);  // check_params + pyramid_plan + the schedule

// ---- the progress counters of every exact-order solve of a call: one block behind the handle's 32 control words, laid out
// level by level and cleared at once.  `words(k)`: unsigneds per solve of level k (the path's own layout; 0: the level has
// none); `solves_per_outer`: solves per outer iteration (n_inner of the single call, the solver pairs of a batch).
inline unsigned* counters_base(const papof_handle* h) { return h->sync_words + 32; }  // the block: also the counters of a lone solve
struct SolveCounters {
    struct PerLevel {
        size_t off = 0, per = 0;  // offset (unsigneds) of the level's first solve, stride per solve
    };
    std::vector<PerLevel> lv;
    size_t total = 0;
    SolveCounters() = default;
    template <class Words>
    SolveCounters(const CallPlan& cp, Words words, size_t solves_per_outer) : lv(cp.levels) {
        for (int k = 0; k < cp.levels; k++) {
            lv[k].per = words(k);
            lv[k].off = total;
            total += lv[k].per * (size_t)cp.n_outer[k] * solves_per_outer;
        }
    }
    // the counters of solve i of level k (in the level's stream order)
    unsigned* solve(const papof_handle* h, int k, size_t i) const { return counters_base(h) + lv[k].off + i * lv[k].per; }
};

// the number of the Laplacian-noise guard's next pass (papof_handle::lap_epoch): a flag is set when it holds the number of the
// pass that wrote it -- no clearing, nothing stale can be taken for a proof; 2^31 passes later it starts over on cleared flags
// (the handle's flag block holds pass numbers that are never cleared otherwise, and `epoch ^ kLapNone` must not be 0)
int lap_next_epoch(papof_handle* h, hipStream_t stream);

// the report of the orchestrators that measure the total and the solver kernels' own time only (after the stream has drained)
inline int collect_total_and_sor(PhaseClock& total, PhaseClock& sorclk, double* timing) {
    if (total.err != PAPOF_OK || sorclk.err != PAPOF_OK) return PAPOF_EDEVICE;
    double tm[PAPOF_N_TIMERS + 1] = {};  // + kTimerFused
    sorclk.collect(tm);
    total.collect(tm);
    for (int i = 0; timing && i < PAPOF_N_TIMERS; i++) timing[i] = tm[i];
    return PAPOF_OK;
}

// ---- the preparation stream ----
struct StreamSwap {  // the launch wrappers enqueue on h->stream
    papof_handle* h;
    hipStream_t saved;
    StreamSwap(papof_handle* hh, hipStream_t s) : h(hh), saved(hh->stream) { h->stream = s; }
    ~StreamSwap() { h->stream = saved; }
};
// one untimed event per level, one for the final warp's planes and one for this fork: with `overlap` the preparation stream
// starts after whatever has been queued on the main stream (the frame uploads)
int fork_prep(papof_handle* h, int levels, bool overlap);

size_t arena_bytes_for(int H, int W, int C, int levels, int n_sor_max, double ratio);
int ensure_arena(papof_handle* h, size_t bytes);
int check_params(const papof_params& P, int levels);
int pyramid_plan(int H, int W, double ratio, int nlev, std::vector<Level>& L, std::vector<PyrPlan>& plan);
int build_pyramid(papof_handle* h, const std::vector<Level>& L, const std::vector<PyrPlan>& plan, int C, bool second,
                  double* tmp_a, double* tmp_b);
size_t pyramid_tmp_elems(const std::vector<Level>& L, const std::vector<PyrPlan>& plan, int C);  // of each of tmp_a, tmp_b
int smooth_and_resize(papof_handle* h, const double* src, double* dst, double* tmp_a, double* tmp_b, const PyrPlan& p, int C,
                      int dh, int dw);  // one pyramid level from its source level; C may count the planes of SEVERAL contiguous frames
int feature_channels(int C);
// batch.hip: B frame pairs of one shape in one launch chain (host frames in, host results out; papof_flow_batch_tensor: device
// tensors in and out); falls back to single calls
int flow_batch_host(papof_handle* h, int n_pairs, int sequence, const void* const* frames, bool u8, int H, int W, int C, int levels,
                    const papof_params* params, double* const* vx, double* const* vy, double* const* warpI2, double* timing_sec);
// the device call on two planar fp64 frames already on the device (api.hip: flow_device, both passes of the guard), from the
// caller's initial flow of the pair (init: one pair of a strided float32 / float64 tensor; NULL: zero); returns with the results written
int flow_device_planar(papof_handle* h, const double* f1, const double* f2, int H, int W, int C, int levels,
                       const papof_params& P, double* d_vx, double* d_vy, double* d_warp, double* timing,
                       const papof_tensor* init = nullptr);
// the initial flow's coarsest level for the pairs of a call (api.hip: the rule of include/papof.h)
int reduce_init(papof_handle* h, const papof_tensor* a, const papof_tensor* b, int pairs_a, int pairs_b, int H, int W,
                const std::vector<Level>& L, const std::vector<PyrPlan>& plan, double ratio, double* X, double* Y, double* T,
                size_t t_planes, double*& out);

}  // namespace papof
