/* include/papof.h -- C ABI of the MI355X-native coarse-to-fine optical-flow hot path.
 *
 * Drop-in boundary.  This library replaces everything beneath the reference's only FFI seam:
 *
 *   Code/Serial/coarse2Fine.pxd:8-12 and Code/Serial/src/Coarse2FineFlowWrapper.h:12-15
 *       map<string,string> Coarse2FineFlowWrapper(double* vx, double* vy, double* warpI2,
 *                                                 const double* Im1, const double* Im2,
 *                                                 int pyramidLevels, int h, int w, int c);
 *   (Code/Parallel/coarse2Fine.pxd:11 inserts `int nCores` after pyramidLevels)
 *
 * which Code/Serial/pyflow.pyx:61-66 calls with caller-allocated, C-contiguous float64 buffers
 * (Im1, Im2, warpI2: h*w*c, channel-interleaved; vx, vy: h*w).  The C++ std::map return value cannot
 * cross a C ABI, so the ten timers the reference publishes (src/OpticalFlow.cpp:850-860) come back in
 * `timing_sec[10]`, in the map's sorted key order (PAPOF_TIMING_KEYS); the Python/Cython side formats
 * them into the dict of strings pyflow.coarse2fine_flow returns.
 *
 * Conventions: plain pointers and sizes only; no exceptions cross the boundary; every function returns
 * PAPOF_OK (0) or a negative PAPOF_E* code; the caller owns every buffer; the library retains nothing
 * between calls except the device arena inside a papof_handle.  The compute path is HIP on gfx950 only:
 * there is NO CPU fallback -- without a usable GPU every compute entry point returns PAPOF_ENODEVICE.
 */
#ifndef PAPOF_H
#define PAPOF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAPOF_VERSION 115 /* 0.1.15: papof_homography_fit_tensor / papof_homography_workspace / papof_warp_projective_tensor / papof_mosaic_projective_tensor / papof_mosaic_overlap_projective_tensor (the homography model: the fit, the warp, the mosaic and the overlap statistics over 3 x 3 matrices) -- additions only, the number stays; papof_motion_blur_tensor (synthetic motion blur: the shutter's samples of papof_interp_tensor's rule summed in one kernel) -- an addition only, the number stays; papof_match_tensor / papof_match_workspace / papof_match_densify_tensor (dense block matching of decimated uint8 frames, a start for the solver on large displacements) -- additions only, the number stays; papof_splat_tensor / papof_splat_workspace (forward warping: deterministic splatting along a flow, 64-bit fixed-point sums), papof_interp_splat_tensor (frame interpolation by splatting both frames) -- additions only, the number stays; papof_fill_holes_tensor / papof_fill_workspace (a field filled inside a mask: pull-push and Jacobi relaxation), papof_propagate_tensor (holes filled from other frames along the flows): flow-guided video completion; 0.1.14: papof_temporal_filter_tensor (motion-compensated temporal denoising along a video's forward and backward flows); 0.1.13: papof_motion_fit_tensor / papof_motion_workspace (global motion of a flow field, IRLS in fp64), papof_warp_affine_tensor (frames warped by per-frame affine matrices): video stabilization; 0.1.12: papof_flow_batch_tensor_init / papof_flow_batch_tensor_fb_init (the device-tensor calls started from a caller's initial flow); 0.1.11: papof_interp_tensor (motion-compensated frame interpolation from forward and backward flows and an occlusion mask); 0.1.10: papof_set_graph_mode removed (hipGraph replay, PAPOF_GRAPH, is retired; so are PAPOF_HOST_COPY / PAPOF_HOST_THREADS, PAPOF_HOSTIO and PAPOF_PREP_CUS); 0.1.9: papof_strip_plan removed (the strips schedule, PAPOF_STRIPS, is retired); 0.1.8: papof_track_tensor (point tracks through a video's forward and backward flows); 0.1.7: papof_flow_batch_tensor_fb (forward and backward pairs in one launch chain, occlusion masks), papof_fb_check_tensor; 0.1.6: papof_flow_batch_tensor (strided device tensors in and out, ordered on the caller's stream), papof_tensor / PAPOF_DTYPE_*; 0.1.5: papof_flow_batch / papof_flow_batch_u8, papof_last_host_times, PAPOF_RCCL_LIB / PAPOF_TILES_TIMEOUT_S; 0.1.4: the Laplacian-noise guard (papof_lap_guard_stats); 0.1.3: papof_last_sor_solves, exact-order band split over ranks (papof_tiles_*, PAPOF_SOR_EXACT); 0.1.2: measurement / test aids (papof_last_sor_stats, papof_strip_plan, papof_test_sor_strips); 0.1.1: papof_params gained interpolation / noise_model */

enum {
    PAPOF_OK = 0,
    PAPOF_EINVAL = -1,     /* NULL pointer, non-positive size, pyramid_levels < 1 (UB in the reference:
                              src/GaussianPyramid.cpp:87-88), unsupported parameter */
    PAPOF_ENODEVICE = -2,  /* no gfx950 device / HIP runtime error at start-up */
    PAPOF_ENOMEM = -3,     /* device or host allocation failed */
    PAPOF_EDEVICE = -4,    /* a HIP call failed mid-flight (papof_last_error() has the text) */
    PAPOF_ETIMEOUT = -5    /* a bounded device-side wait expired (exact-order SOR progress counters) */
};

/* Order of the SOR sweep (src/OpticalFlow.cpp:458-505). */
enum {
    PAPOF_SOR_EXACT = 0,    /* the reference's in-place sweep->row->column order, bit-compatible results */
    PAPOF_SOR_REDBLACK = 1, /* in-place two-colour sweeps: throughput mode, NOT reference parity      */
    PAPOF_SOR_JACOBI = 2    /* every cell from the previous sweep: correctness-gate mode (config 2)   */
};

/* The reference's two non-default branches, selected there by file-scope statics that its Python entry point cannot
 * reach (src/OpticalFlow.cpp:32-34). */
enum {
    PAPOF_INTERP_BILINEAR = 0, /* warpFL (the default, src/OpticalFlow.cpp:33)                                     */
    PAPOF_INTERP_BICUBIC = 1   /* in-loop Image::warpImageBicubicRef (+ threshold) on the feature images, :517-521, :816 */
};
enum {
    PAPOF_NOISE_LAPLACIAN = 0, /* psi = 1 / (2 sqrt(t^2 + eps)) (the default, :34, :399-402)                        */
    PAPOF_NOISE_GMIXTURE = 1   /* two-component Gaussian mixture per channel (:359-367, :389-397), re-estimated by EM
                                  after every outer iteration (estGaussianMixture, :539-591).  Uses exp() and global
                                  sums: NOT bit-compatible with the reference (device exp <= 1 ulp, parallel sums), and
                                  with this model the reference's own iteration amplifies a 1e-13 perturbation ~7x per
                                  outer iteration (measured on its arithmetic): one SmoothFlowSOR call of 3 outer
                                  iterations agrees to 1e-9, whole calls only within that conditioning  */
};

/* Solver parameters.  The reference hard-codes all of them (src/OpticalFlow.cpp:747-751, :451, :823);
 * papof_default_params() reproduces those values, so passing NULL == the reference. */
typedef struct papof_params {
    double alpha;          /* 0.012  regularisation weight                      src/OpticalFlow.cpp:747 */
    double ratio;          /* 0.75   pyramid down-sampling ratio                :748                    */
    int n_outer;           /* 7      outer fixed-point iterations at level 0    :749                    */
    int n_outer_per_level; /* 1      ... plus this many per pyramid level k     :823 (nOuter+k)         */
    int n_inner;           /* 1      inner fixed-point iterations               :750                    */
    int n_sor;             /* 30     SOR sweeps at level 0                      :751                    */
    int n_sor_per_level;   /* 3      ... plus this many per pyramid level k     :823 (nCG+k*3)          */
    double omega;          /* 1.8    over-relaxation factor                     :451                    */
    int sor_mode;          /* PAPOF_SOR_*                                                                */
    int phase_timing;      /* All ten reference timers are always measured (HIP events on the streams, no synchronisation).
                              0: flow-independent work (pyramids = Construction, features = Allocation, derivative planes of
                                 the final warp = PostProcessing) runs on a second stream BESIDE the solver phases, so the
                                 ten values overlap in time and add up to more than the total;
                              1: everything on one stream: phases do not overlap (slower by the lost overlap);
                              2: as 0, but only "Total C++ Execution" and "Phase5_SOR" are measured (the other eight read 0):
                                 no phase stamps at all -- what bench.py's device-resident headline runs with, as in round 1
                                 (the stamps cost <= 0.1 ms per 1080p call).
                              Phase5_SOR is the solver kernels' own duration in both cases.  Phase3_PsiData and
                              Phase4_LinearSystem are ONE fused kernel here: its time is apportioned 30 : 70; on the default
                              branches phi (Phase2_Derivatives) is written by the warp-and-smooth kernel of Phase1_Generate
                              and reported as a fixed 4 % of it; where ONE kernel does Phase1 ... Phase4 (k_flow_system: default
                              branches, one GPU) its time is apportioned 51 : 2 : 14 : 33.  Between two outer iterations of
                              a level that kernel also carries Phase6_Update (u += du, v += dv: one scattered 16-byte load
                              per warped pixel and two 8-byte stores per cell, no measurable part of the launch -- it is no
                              slower than without them): Phase6 then has no kernel of its own and reads the gap in front of
                              the launch; its share stays inside the four.                                                */
    int interpolation;     /* PAPOF_INTERP_*  (0 = the reference's default)                                          */
    int noise_model;       /* PAPOF_NOISE_*   (0 = the reference's default)                                          */
} papof_params;

/* Index of each reference timer in timing_sec[] == sorted std::map key order, src/OpticalFlow.cpp:850-860 */
enum {
    PAPOF_T_ALLOCATION = 0,
    PAPOF_T_CONSTRUCTION = 1,
    PAPOF_T_PHASE1_GENERATE = 2,
    PAPOF_T_PHASE2_DERIVATIVES = 3,
    PAPOF_T_PHASE3_PSIDATA = 4,
    PAPOF_T_PHASE4_LINEARSYSTEM = 5,
    PAPOF_T_PHASE5_SOR = 6,
    PAPOF_T_PHASE6_UPDATE = 7,
    PAPOF_T_POSTPROCESSING = 8,
    PAPOF_T_TOTAL = 9,
    PAPOF_N_TIMERS = 10
};

typedef struct papof_handle papof_handle; /* device arena + stream; one per GPU, not thread-safe */

int papof_version(void);
void papof_default_params(papof_params* p);
const char* papof_strerror(int code);
const char* papof_last_error(void); /* text of the last HIP failure on this thread ("" if none) */
const char* papof_timing_key(int index); /* "Allocation" ... "Total C++ Execution" */
int papof_device_count(void);            /* number of visible gfx950 devices (0 if none / no driver) */

int papof_create(int device, papof_handle** out);
void papof_destroy(papof_handle* h);

/* ---- THE drop-in entry point: replaces Coarse2FineFlowWrapper (src/Coarse2FineFlowWrapper.cpp:14-51).
 * Host buffers in, host buffers out, uses a process-wide lazily created handle on device 0
 * (or $PAPOF_DEVICE).  Internally serialised by a mutex (the reference is not re-entrant either:
 * file-scope timers, src/OpticalFlow.cpp:39-64). */
int papof_coarse2fine_flow(const double* im1, const double* im2, int h, int w, int c, int pyramid_levels,
                           const papof_params* params /* NULL = reference defaults */, double* vx, double* vy,
                           double* warpI2, double timing_sec[PAPOF_N_TIMERS] /* may be NULL */);

/* Same, on an explicit handle (arena reuse across the 101 pairs of a collection, TestSuite.py:69-81). */
int papof_flow(papof_handle* h, const double* im1, const double* im2, int height, int width, int c,
               int pyramid_levels, const papof_params* params, double* vx, double* vy, double* warpI2,
               double timing_sec[PAPOF_N_TIMERS]);

/* Same, with every buffer already resident in this handle's device memory (HWC in, planar vx/vy and HWC
 * warpI2 out; all fp64).  Enqueues on the handle's stream and returns after the stream has drained. */
int papof_flow_device(papof_handle* h, const double* d_im1, const double* d_im2, int height, int width, int c,
                      int pyramid_levels, const papof_params* params, double* d_vx, double* d_vy,
                      double* d_warpI2, double timing_sec[PAPOF_N_TIMERS]);

/* ---- uint8 frames.  The reference's caller decodes a JPEG to uint8 and hands
 * `im.astype(float) / 255.` to pyflow (Code/Serial/OpticalFlowCalculation.py:65-70); these entry points take the
 * uint8 samples (HWC interleaved) and do that one IEEE division per sample on the device while the frame is
 * planarised -- the same bits, 1 byte instead of 8 per sample over PCIe.  Outputs as papof_flow. */
int papof_flow_u8(papof_handle* h, const unsigned char* im1, const unsigned char* im2, int height, int width,
                  int c, int pyramid_levels, const papof_params* params, double* vx, double* vy, double* warpI2,
                  double timing_sec[PAPOF_N_TIMERS]);
int papof_flow_device_u8(papof_handle* h, const unsigned char* d_im1, const unsigned char* d_im2, int height,
                         int width, int c, int pyramid_levels, const papof_params* params, double* d_vx,
                         double* d_vy, double* d_warpI2, double timing_sec[PAPOF_N_TIMERS]);

/* ---- sequence mode.  The reference's TestSuite walks a 102-frame collection as 101
 * overlapping pairs (Code/Serial/TestSuite.py:69-81: frame n -> n+1, then n+1 -> n+2, ...), rebuilding the
 * pyramid of every frame twice.  Here the handle keeps the pyramid of the last pushed frame in its arena: each
 * push uploads ONE frame, builds ONE pyramid and returns the flow from the previous frame to this one --
 * bit-identical to papof_flow(previous, frame).  *have_flow = 0 for the push that primes a sequence (first push,
 * after papof_seq_reset, or when shape / levels / ratio differ from the kept frame: a new sequence starts),
 * 1 otherwise; outputs are written only when *have_flow == 1.  Any other call on the handle ends the sequence. */
int papof_seq_reset(papof_handle* h);
int papof_seq_push(papof_handle* h, const double* frame, int height, int width, int c, int pyramid_levels,
                   const papof_params* params, double* vx, double* vy, double* warpI2,
                   double timing_sec[PAPOF_N_TIMERS], int* have_flow);
int papof_seq_push_u8(papof_handle* h, const unsigned char* frame, int height, int width, int c,
                      int pyramid_levels, const papof_params* params, double* vx, double* vy, double* warpI2,
                      double timing_sec[PAPOF_N_TIMERS], int* have_flow);
/* frame already resident in device memory (fp64 HWC, or uint8 HWC when is_u8 != 0) */
int papof_seq_push_device(papof_handle* h, const void* d_frame, int is_u8, int height, int width, int c,
                          int pyramid_levels, const papof_params* params, double* d_vx, double* d_vy,
                          double* d_warpI2, double timing_sec[PAPOF_N_TIMERS], int* have_flow);

/* ---- ONE frame pair sharded as 2-D tiles over several GPUs (BASELINE.json configs[4]: 1920x1080
 * tiled 2x4 across 8 GPUs with RCCL halo exchange over xGMI).  One rank per GPU / process; every rank holds both
 * frames; rank 0 receives the assembled (vx, vy, warpI2).  Red-black SOR order (PAPOF_SOR_REDBLACK, n_inner = 1): a
 * red-black half-sweep reads only the other colour's previous values, so the tiled result is bit-identical to
 * papof_flow_device() in that mode on one GPU.  (PAPOF_SOR_EXACT: see papof_bands_plan below.)  `halo` = ghost-zone depth in half-sweeps (one (du, dv) exchange per
 * `halo` half-sweeps; 0 = default 10).  All calls below except _grid/_rect/_halo_message are collective. */
typedef struct papof_tiles papof_tiles;
#define PAPOF_TILES_ID_BYTES 128
#define PAPOF_BAND_ROWS 62 /* rows per solver band of the exact-order kernel (sor.hip) */
/* rows x cols grid for n ranks (8 -> 2 x 4: tiles of 480 x 540 at 1080p, 4 -> 2 x 2, 2 -> 1 x 2) */
int papof_tiles_grid(int nranks, int* rows, int* cols);
/* rect = {x0, y0, x1, y1} (half-open) of rank's tile of a width x height plane */
int papof_tiles_rect(int width, int height, int rows, int cols, int rank, int rect[4]);
/* the rectangle rank `src` sends to rank `dst` when every rank needs its tile grown by `halo` pixels (empty: x1 <= x0);
 * pure function of its arguments -- both ends of a message compute it, nothing is negotiated */
int papof_tiles_halo_message(int width, int height, int rows, int cols, int halo, int src, int dst, int rect[4]);
/* PAPOF_SOR_EXACT on a tile group: the reference's own sweep order, split into `nranks` horizontal ranges of SOLVER BANDS
 * (csrc/tiles.hip: bands_flow; the rows x cols grid is ignored) -- bit-identical to papof_flow_device(), i.e. the sharded
 * configuration that meets the 1e-4 parity bar; default branches, n_inner = 1, at most 128 sweeps.  Every rank runs the
 * bands [B0, B1) of every solve; the one 16-byte cell per step that crosses a cut goes, with the producer's progress, straight
 * into the planes of the rank below (LOCAL transport: one process, one device), or -- transports that cannot address peer
 * memory from a kernel: RCCL -- as one message per solve and cut after the producer's kernel has finished (the ranks then take
 * turns within a solve).  papof_bands_plan: for a height x width level with n_sor sweeps, out = {B0, B1, first / one-past-last
 * coefficient row the rank's tasks touch, first / one-past-last row whose final increments it holds (a partition)}. */
int papof_bands_plan(int height, int width, int n_sor, int nranks, int rank, int out[6]);
/* RCCL transport: rank 0 obtains an id (ncclGetUniqueId) and hands it to every rank by whatever means the launcher
 * has (bench.py: torch.distributed broadcast); then every rank creates its member of the group on its own handle. */
int papof_tiles_unique_id(unsigned char id[PAPOF_TILES_ID_BYTES]);
int papof_tiles_create(papof_handle* h, const unsigned char id[PAPOF_TILES_ID_BYTES], int rank, int nranks, int rows,
                       int cols, int halo, papof_tiles** out);
/* LOCAL transport: all `nranks` ranks live in this process (one handle each, e.g. all on one device); messages are
 * device-to-device copies.  Each out[r] must then be driven by its own host thread.  Same orchestration code as the
 * RCCL transport; exists so that the tiled path can be parity-tested on a one-GPU box. */
int papof_tiles_create_local(papof_handle* const* handles, int nranks, int rows, int cols, int halo,
                             papof_tiles** out /* nranks entries */);
int papof_tiles_flow_device(papof_tiles* t, const double* d_im1, const double* d_im2, int height, int width, int c,
                            int pyramid_levels, const papof_params* params /* NULL = reference schedule, red-black */,
                            double* d_vx, double* d_vy, double* d_warpI2 /* rank 0 only; may be NULL elsewhere */,
                            double timing_sec[PAPOF_N_TIMERS]);
int papof_tiles_stats(const papof_tiles* t, long* exchanges, size_t* bytes); /* of the last call, this rank */
/* what the TRANSPORT reports about the group (RCCL: ncclCommCount / ncclCommUserRank of this member's communicator), and
 * the tile grid / ghost depth in use: lets a multi-GPU bench line show that RCCL saw N ranks and the rows x cols split */
int papof_tiles_comm_info(const papof_tiles* t, int* nranks_seen, int* rank_seen, int* rows, int* cols, int* halo);
void papof_tiles_destroy(papof_tiles* t);

/* Whether a call spreads over several streams of its own (the preparation beside the coarse levels' solves, PCIe copies beside
 * kernels: the default, fastest for ONE call at a time) or stays on the handle's one stream (on = 0; also PAPOF_OVERLAP=0 when
 * the handle is created).  With several handles in flight -- a collection of pairs, flow_collection() -- the other handles'
 * calls fill the idle time and one stream per handle is faster (fewer hardware queues shared): 240x135 pairs on the
 * reference schedule 3.2 -> 2.2 ms per pair with 16 in flight, 480x270 4.9 -> 3.4.  Results are the same bits. */
int papof_set_stream_overlap(papof_handle* h, int on);

/* Device memory helpers for callers without a HIP binding (bench.py, ctypes users). */
int papof_dev_alloc(papof_handle* h, size_t bytes, void** out);
int papof_dev_free(papof_handle* h, void* p);
int papof_dev_upload(papof_handle* h, void* dst, const void* src, size_t bytes);
int papof_dev_download(papof_handle* h, void* dst, const void* src, size_t bytes);
void* papof_stream(papof_handle* h); /* the hipStream_t every kernel of this handle is launched on */
/* Page-locked host memory for RESULT arrays (hipHostMalloc).  The reference's pyflow.pyx allocates vx, vy, warpI2 itself
 * for every call (np.zeros, Code/Serial/pyflow.pyx:44-52): 83 MB of fresh pages per 1080p pair, i.e. ~20 k first-touch
 * page faults, a staged device-to-host copy, and an munmap when the caller drops them.  A binding that takes its result
 * arrays from here (and recycles them when they are garbage-collected: papteam_opticalflow_amd/dropin/pyflow.pyx,
 * capi.py) gets the results by direct DMA into memory that is already resident.  Any host pointer works as an output
 * of papof_flow / papof_coarse2fine_flow; these are merely the fastest ones. */
int papof_host_alloc(size_t bytes, void** out);
int papof_host_free(void* p);

/* ---- stage entry points (host buffers, reference HWC layout): one per reference function on the path,
 * used by the parity tests to check each kernel in isolation against the oracle. ---- */

/* GaussianPyramid::ConstructPyramidLevels, src/GaussianPyramid.cpp:79-108.  dims[2i]=width, dims[2i+1]=
 * height of level i; data==NULL returns only dims.  *n_elems = total doubles of all levels. */
int papof_stage_pyramid(papof_handle* h, const double* im, int height, int width, int c, double ratio,
                        int levels, int* dims, double* data, long* n_elems);
/* Image::GaussianSmoothing, src/Image.h:1203-1225 (fsize <= 8). */
int papof_stage_gaussian(papof_handle* h, const double* im, int height, int width, int c, double sigma,
                         int fsize, double* out);
/* Image::imresize(result, ratio) src/Image.h:751-763 ; out is int(h*ratio) x int(w*ratio). */
int papof_stage_resize_ratio(papof_handle* h, const double* im, int height, int width, int c, double ratio,
                             double* out);
/* Image::imresize(w,h) src/Image.h:778-783. */
int papof_stage_resize_wh(papof_handle* h, const double* im, int height, int width, int c, int dst_w,
                          int dst_h, double* out);
/* OpticalFlow::im2feature, src/OpticalFlow.cpp:911-961; returns (in *fc) 5 for c==3, 3 for c==1, else c. */
int papof_stage_im2feature(papof_handle* h, const double* im, int height, int width, int c, double* out,
                           int* fc);
/* OpticalFlow::warpFL, src/OpticalFlow.cpp:154-159. */
int papof_stage_warpFL(papof_handle* h, const double* im1, const double* im2, const double* vx,
                       const double* vy, int height, int width, int c, double* out);
/* OpticalFlow::getDxs, src/OpticalFlow.cpp:80-122. */
int papof_stage_getDxs(papof_handle* h, const double* im1, const double* im2, int height, int width, int c,
                       double* imdx, double* imdy, double* imdt);
/* Linear system of one inner iteration with du=dv=0 (src/OpticalFlow.cpp:295-448): outputs phi, imdxy,
 * imdx2, imdy2 and the two right-hand sides, each height*width. */
int papof_stage_linear_system(papof_handle* h, const double* im1, const double* warp, const double* u,
                              const double* v, int height, int width, int c, double alpha, double* phi,
                              double* imdxy, double* imdx2, double* imdy2, double* rhs1, double* rhs2);
/* OpticalFlow::Laplacian, src/OpticalFlow.cpp:641-690. */
int papof_stage_laplacian(papof_handle* h, const double* in, const double* weight, int height, int width,
                          double* out);
/* The SOR sweeps, src/OpticalFlow.cpp:451-505, starting from du=dv=0. */
int papof_stage_sor(papof_handle* h, const double* phi, const double* imdxy, const double* imdx2,
                    const double* imdy2, const double* rhs1, const double* rhs2, int height, int width,
                    double alpha, double omega, int n_sor, int sor_mode, double* du, double* dv);
/* One pyramid level: OpticalFlow::SmoothFlowSOR, src/OpticalFlow.cpp:238-536.
 * warp, u, v are in/out. */
int papof_stage_smoothflow(papof_handle* h, const double* im1, const double* im2, double* warp, double* u,
                           double* v, int height, int width, int c, double alpha, int n_outer, int n_inner,
                           int n_sor, double omega, int sor_mode);
/* GaussianPyramid::ConstructPyramid (the min-width variant the reference does not call, src/GaussianPyramid.cpp:47-77)
 * differs from ConstructPyramidLevels in its level count only: *levels = (int)(log((double)min_width / width) /
 * log(ratio)) after the same clamp of the ratio (:50-53); pass it as `levels` / `pyramid_levels` anywhere. */
int papof_pyramid_levels_for_min_width(int width, double ratio, int min_width, int* levels);
/* SmoothFlowSOR with the non-default branches: interpolation / noise_model as in papof_params; gm (5 * c doubles: alpha,
 * sigma, beta, sigma^2, beta^2 per channel; NULL = GaussianMixture::reset() values) is in/out when noise_model = GMIXTURE. */
int papof_stage_smoothflow_ex(papof_handle* h, const double* im1, const double* im2, double* warp, double* u,
                              double* v, int height, int width, int c, double alpha, int n_outer, int n_inner,
                              int n_sor, double omega, int sor_mode, int interpolation, int noise_model, double* gm);
/* OpticalFlow::estGaussianMixture, src/OpticalFlow.cpp:539-591 (prior 0.9); gm in/out as above. */
int papof_stage_est_gaussian_mixture(papof_handle* h, const double* im1, const double* im2, int height, int width,
                                     int c, double* gm);
/* Image::warpImageBicubicRef alone (clamp = 0: the first warp of a level, src/OpticalFlow.cpp:816) or with threshold(). */
int papof_stage_bicubic_warp_ex(papof_handle* h, const double* im1, const double* im2, const double* vx,
                                const double* vy, int height, int width, int c, int clamp, double* out);
/* Image::warpImageBicubicRef + threshold, src/Image.h:2587-2701, :2031-2045 (final warp of the originals). */
int papof_stage_bicubic_warp(papof_handle* h, const double* im1, const double* im2, const double* vx,
                             const double* vy, int height, int width, int c, double* out);

/* ---- the step after the path: the reference's 16-bit flow encoding,
 * OpticalFlow::SaveOpticalFlow / LoadOpticalFlow (src/OpticalFlow.cpp:963-1015) with AssembleFlow / DissembleFlow
 * (src/OpticalFlow.h:70-91): out[(i*width + j)*2 + {0,1}] = (unsigned short)((clamp(v{x,y}, -200, 200) + 200) * 160);
 * back: (double)q / 160 - 200.  The file Image<unsigned short>::saveImage writes around it (src/Image.h:825-837:
 * 16-byte type name, width, height, channels as int, one bool) is plain host I/O: papteam_opticalflow_amd.save_flow16. */
int papof_flow_quantize16(papof_handle* h, const double* vx, const double* vy, int height, int width,
                          unsigned short* out);
int papof_flow_dequantize16(papof_handle* h, const unsigned short* q, int height, int width, double* vx,
                            double* vy);

/* Flow visualisation of the reference's caller, generateOutputFlowImageFile (Code/Serial/OpticalFlowCalculation.py:
 * 143-162, disabled there at :137 and dependent on cv2): hue = direction, value = magnitude (min-max normalised),
 * saturation 255, HSV -> BGR the way OpenCV's 8-bit conversion does; bgr is height*width*3 bytes, B first.
 * PARITY UNPINNED: OpenCV is not installed in this environment and its cartToPolar uses an approximate atan2. */
int papof_flow_to_bgr(papof_handle* h, const double* vx, const double* vy, int height, int width,
                      unsigned char* bgr);

/* ---- measurement hook for bench.py: time `reps` back-to-back SOR solves of `n_sor` sweeps on synthetic
 * coefficient planes already resident in HBM (SURVEY.md §8d micro-benchmark), with HIP events recorded
 * on the handle's stream.  Returns average milliseconds per solve in *ms_per_solve. */
int papof_bench_sor(papof_handle* h, int height, int width, int n_sor, int sor_mode, int reps, unsigned seed,
                    double* ms_per_solve);

/* Measurement aid for bench.py: how a solve of `n_sor` sweeps on a height x width plane is issued in `sor_mode` on this
 * handle -- solver-kernel launches per solve, and the sweeps one launch runs (exact order: 1, or 2 with two sweeps per
 * wave; red-black: HALF-sweeps per launch of the LDS-tiled, temporally blocked kernel; Jacobi: sweeps per launch). */
int papof_sor_plan(papof_handle* h, int height, int width, int n_sor, int sor_mode, int* launches, int* depth);

/* Which instance of the one-workgroup exact-order solver (k_sor_tiny) a height x width plane selects -- a host-only query: no
 * handle, no device.  *cells_per_tile = cells of a tile (the instance's template parameter), *waves = wavefronts of the
 * launch; both 0 when no instance holds the plane (more than 8192 cells, more lanes than a workgroup has, or more than 150 KiB
 * of LDS): the hyperplane kernels solve it.  PAPOF_SOR_TINY=0 (read when a handle is created) sends every plane to them. */
int papof_sor_tiny_shape(int height, int width, int* cells_per_tile, int* waves);

/* Measurement aid for bench.py: what the LAST papof_flow* / papof_seq_push* call on this handle launched -- exact-order
 * solver kernels in all.  *strip_streams_sec is always 0: it was the share of Phase5_SOR that ran on the strip streams,
 * and the strips schedule is gone (the argument stays for the ABI). */
int papof_last_sor_stats(papof_handle* h, int* launches, double* strip_streams_sec);

/* Measurement aid for bench.py (roofline.by_level / by_kernel): the solves of the LAST papof_flow* / papof_seq_push* call on
 * this handle, in stream order.  *n = their number; for i < min(*n, cap): info[6 i ..] = {height, width, sweeps, kind,
 * depth, launches} with kind 0 = k_sor_exact, 1 = k_sor_fused, 2 = k_sor_group, 3 / 4 = k_sor_blocked red-black / Jacobi,
 * 5 = one launch per (half-)sweep, 6 = k_sor_tiny (exact order, whole plane in one workgroup); depth = software-pipeline depth R (exact order) or (half-)sweeps per launch (blocked);
 * sec[i] = the solver kernels' own HIP-event seconds of that solve (0 when the call collected no timers). */
int papof_last_sor_solves(papof_handle* h, int cap, int* n, int* info, double* sec);

/* The Laplacian-noise guard of the reference (src/OpticalFlow.cpp:399-400: psi of a feature channel stays 0 while the
 * channel's noise estimate, estLaplacianNoise :594-639, is below 1E-20 -- duplicate frames, flat synthetic images).  A call
 * runs WITHOUT the estimate while it collects proofs that the guard could not have tripped (csrc/api.hip: LapGuard); a call
 * that ends without them is run again inside the same papof_flow* call with the estimate after every outer iteration and
 * the guard in the assembly, and the handle then stays in that exact pass until a call proves it unnecessary again.  Results
 * are the reference's either way.  out[0] = calls that were run twice, out[1] = calls run in the exact pass from the start,
 * out[2] = 1 when the next call will start in the exact pass, out[3] = 0 when PAPOF_LAP_GUARD=0 switched the guard off (an
 * A/B switch for its cost: results then differ from the reference's on tripping inputs).  The bicubic branch and the
 * papof_stage_smoothflow* entry points always take the exact pass; the Gaussian-mixture branch has no such
 * guard (:381-397).  One pair over several ranks (papof_tiles_*): the exact-order band split has no exact pass, so it PROVES
 * per call that the guard cannot have tripped (every rank checks every pixel of its rows behind every update; the flags of
 * all ranks are gathered) or returns PAPOF_EINVAL on every rank with a message that names the one-GPU call; the red-black
 * tiles -- not the reference's sweep order anyway -- run without the guard. */
int papof_lap_guard_stats(papof_handle* h, int out[4]);

/* B = n_pairs frame pairs of ONE shape in ONE launch chain (csrc/batch.hip) -- the reference's benchmark walks collections of
 * small frames (Code/Serial/TestSuite.py:69-81: 101 pairs per collection; :91: 240x135 ... 1920x1080), and a 240x135 pair
 * alone is ~210 launches of a few microseconds each: here every launch serves all pairs of the batch.  Host buffers in and out,
 * as papof_flow / papof_flow_u8.  sequence != 0: pair i = (frames[i], frames[i + 1]), n_pairs + 1 frames -- a video; every
 * frame's pyramid and features are built once.  sequence == 0: pair i = (frames[2 i], frames[2 i + 1]), 2 n_pairs frames.
 * vx[i], vy[i] (height x width) and warpI2[i] (height x width x c) receive pair i's results: bit-identical to
 * papof_flow(frames of pair i).  timing_sec: Total = the caller's wall time of the batch, Phase5_SOR = the solver kernels' own
 * time; the other phases are not separated in a batch.  What the batched chain covers: the default branches in the reference's
 * own sweep order (PAPOF_SOR_EXACT, n_inner = 1, bilinear, Laplacian noise model), 1 or 3 channels, fewer than 16 solver
 * bands per level (frames up to ~900 rows); anything else -- and n_pairs = 1 -- runs as consecutive single calls through this
 * same entry point.  A pair whose Laplacian-noise guard (papof_lap_guard_stats) cannot be proven open in the batch is run again
 * through the single call.  Any sequence kept by papof_seq_push* on the handle ends. */
int papof_flow_batch(papof_handle* h, int n_pairs, int sequence, const double* const* frames, int height, int width, int c,
                     int pyramid_levels, const papof_params* params, double* const* vx, double* const* vy,
                     double* const* warpI2, double timing_sec[PAPOF_N_TIMERS]);
int papof_flow_batch_u8(papof_handle* h, int n_pairs, int sequence, const unsigned char* const* frames, int height,
                        int width, int c, int pyramid_levels, const papof_params* params, double* const* vx,
                        double* const* vy, double* const* warpI2, double timing_sec[PAPOF_N_TIMERS]);

/* Which way the frame pairs of papof_flow_batch* (host frames and device tensors alike) went, cumulative over the handle's
 * life: out[0] = launch chains run, out[1] = solver pairs run inside them (a forward-backward call's frame pair is two),
 * out[2] = frame pairs run as single calls because the batched chain does not cover them (see above; a batch or a remainder
 * of one pair) or had no room for them, out[3] = frame pairs run again as single calls because their Laplacian-noise guard
 * was left unproven in the chain (forward-backward: once per frame pair, whichever direction lacked the proof).  Results do
 * not depend on the way taken; a test that compares the batch with the single calls reads here that the chain ran. */
int papof_batch_stats(papof_handle* h, long long out[4]);

/* Strided 4-D device tensors (PyTorch's, or anyone's): element type and the distance, in ELEMENTS, between neighbours along
 * the logical axes (frame or pair, row, column, channel or component).  NCHW and NHWC are different strides of the same
 * description; a zero stride repeats an element (an expanded tensor). */
enum { PAPOF_DTYPE_U8 = 0, PAPOF_DTYPE_F32 = 1, PAPOF_DTYPE_F64 = 2 };
/* 16-bit words, strides in words: only the plane descriptors of papof_ycc16_to_rgb_tensor, papof_ycc16_to_rgb_fast and
 * papof_rgb_to_ycc16_tensor take it; every other entry point refuses it with PAPOF_EINVAL. */
enum { PAPOF_DTYPE_U16 = 3 };
typedef struct papof_tensor {
    void* data;          /* device memory on the handle's device */
    int dtype;           /* PAPOF_DTYPE_* */
    long long stride[4]; /* elements between neighbours along (frame|pair, row, column, channel|component) */
} papof_tensor;

/* papof_flow_batch on frames that are already in device memory, as strided tensors of uint8 (scaled by 1/255 as
 * papof_flow_u8 does), float32 (widened exactly) or float64 samples, with results written into strided float32 (one
 * round-to-nearest conversion) or float64 tensors.  sequence != 0: `frames` holds n_pairs + 1 frames, pair i = (i, i + 1),
 * frames2 must be NULL; sequence == 0: pair i = (frames[i], frames2[i]), n_pairs frames each.  flow: (pair, row, column,
 * {vx, vy}); warpI2: (pair, row, column, channel).  Every pair's results are bit-identical to papof_flow on the fp64 values
 * of its frames.  The batched chain covers what papof_flow_batch's covers; anything else, a batch of one, and a pair whose
 * Laplacian-noise guard cannot be proven open run pair by pair on the device (no frame crosses PCIe on any path).
 * Stream contract: `stream` is the caller's hipStream_t (NULL: the null stream) on the handle's device.  The call records
 * an event there on entry and the handle's streams wait for it, so inputs produced on that stream are read after they are
 * written; the call returns once every output is written (the guard's proof needs the host).  It is stream-ordered on
 * entry and complete on return, not asynchronous.  PAPOF_EINVAL, before anything is enqueued: a NULL descriptor or data
 * pointer, an unknown dtype, a uint8 output, a negative stride, a zero stride on an output, frames2 given in sequence mode
 * or missing in pair mode.  timing_sec as papof_flow_batch: Total = the caller's wall time, Phase5_SOR = the solver
 * kernels' own time.  Any sequence kept by papof_seq_push* on the handle ends. */
int papof_flow_batch_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                            const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                            const papof_params* params, const papof_tensor* flow, const papof_tensor* warpI2, void* stream,
                            double timing_sec[PAPOF_N_TIMERS]);

/* papof_flow_batch_tensor in both directions, with the forward-backward consistency check (Sundaram, Brox, Keutzer 2010).
 * Pair i runs forward (image 1 -> image 2: flow_fw, warp_fw) and backward (image 2 -> image 1: flow_bw, warp_bw) in ONE
 * launch chain: every frame's pyramid, features and derivative planes are built once and serve both directions, only the
 * per-pair work (systems, solves, updates, the final warp) doubles.  Each direction's results are bit-identical to
 * papof_flow on its frames (backward: the frames exchanged).  Frames, flows and warps, fallbacks, sub-batches (a sub-batch of
 * n frame pairs counts 2n against the batch bound), the stream contract and timing_sec are papof_flow_batch_tensor's.
 * occlusion: NULL (both flows, no check), or a PAPOF_DTYPE_U8 tensor (pair, row, column, {fw, bw}) that receives 1 where the
 * pixel is occluded and 0 elsewhere -- computed from the fp64 flows before they are written, so it does not depend on the
 * outputs' dtype.  For pixel (r, x) of the forward direction, with f = flow_fw, b = flow_bw of the pair:
 *     (u, v) = f(r, x);  (X, Y) = (x + u, r + v);  (bu, bv) = b sampled bilinearly at (X, Y) by the reference's rule
 *     (src/ImageProcessing.h:138-157: truncation toward zero, fraction clamped to [0, 1], neighbours clamped into the image);
 *     e = (u + bu)^2 + (v + bv)^2;  m = (u^2 + v^2) + (bu^2 + bv^2);
 *     occluded = X < 0 || X > width - 1 || Y < 0 || Y > height - 1 || !(e <= alpha1 * m + alpha2)   (NaN: occluded)
 * in fp64 without fused multiply-adds; the backward direction swaps f and b.  Sundaram et al.: alpha1 = 0.01, alpha2 = 0.5.
 * PAPOF_EINVAL, before anything is enqueued: everything papof_flow_batch_tensor refuses (for all four outputs), an occlusion
 * tensor that is not uint8 or has a zero or negative stride, a negative or non-finite alpha. */
int papof_flow_batch_tensor_fb(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                               const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                               const papof_params* params, const papof_tensor* flow_fw, const papof_tensor* warp_fw,
                               const papof_tensor* flow_bw, const papof_tensor* warp_bw, const papof_tensor* occlusion,
                               double alpha1, double alpha2, void* stream, double timing_sec[PAPOF_N_TIMERS]);

/* papof_flow_batch_tensor (and _fb) started from the caller's initial flow instead of zero (refining a flow from elsewhere,
 * large motion given a prior, a two-pass video flow).  init, init_fw, init_bw: NULL (zero flow: the calls above, bit for bit),
 * or a float32 (widened exactly) or float64 tensor (pair, row, column, {vx, vy}) of the frames' height and width with any
 * non-negative strides (a zero pair stride: one flow for every pair).  _fb_init: init_fw starts the forward pairs, init_bw
 * the backward ones; either may be NULL (zero for that direction).  Everything else is papof_flow_batch_tensor's (_fb's).
 *
 * The rule.  L = pyramid_levels; ratio = params->ratio, or 0.75 where it lies outside [0.4, 0.98] (the pyramid's clamp; the
 * up-sampling between levels multiplies by 1 / ratio).  The frames' Gaussian pyramid (papof_stage_pyramid: level i from level
 * src(i) of the same plan, Gaussian smoothing then bilinear resize) is applied to the initial flow as a two-channel image,
 * P_k(init) its level k; it is the pyramid papof_stage_pyramid returns for the (height, width, 2) array (vx, vy) bit for
 * bit.  s = 1.0 multiplied by ratio L - 1 times in fp64.  Then the coarsest level L - 1 starts from
 *     L == 1:  (u, v) = init;
 *     L >= 2:  (u, v) = P_{L-1}(init) * s, one fp64 rounding per element,
 * instead of (0, 0), and it is entered as every finer level is (src/OpticalFlow.cpp:813-816): frame 2's features are warped
 * at (u, v) -- warpFL with bilinear interpolation, warpImageBicubicRef without threshold with bicubic -- instead of being
 * copied.  Everything after that is unchanged: the levels' solves, the up-sampling, the Laplacian-noise guard with LapPara
 * starting at 0.02 on the coarsest level's first iteration, the final bicubic warp.  On the default branches the warp at the
 * flow is part of the solve already, so an all-zero init gives the bits of no init (the flow planes are +0.0 either way).
 * PAPOF_EINVAL, before anything is enqueued: what the call without init refuses, a non-NULL init descriptor with NULL data,
 * a dtype other than F32 / F64, a negative stride.  PAPOF_EINVAL after the entry wait, with nothing written to any output: a
 * component that is NaN, +-Inf or larger than 1e6 in magnitude.  (The device step that reads init also writes 0 in place of
 * any such value, so none reaches a sampler.) */
int papof_flow_batch_tensor_init(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                 const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                                 const papof_params* params, const papof_tensor* init, const papof_tensor* flow,
                                 const papof_tensor* warpI2, void* stream, double timing_sec[PAPOF_N_TIMERS]);
int papof_flow_batch_tensor_fb_init(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                    const papof_tensor* frames2, int height, int width, int c, int pyramid_levels,
                                    const papof_params* params, const papof_tensor* init_fw, const papof_tensor* init_bw,
                                    const papof_tensor* flow_fw, const papof_tensor* warp_fw, const papof_tensor* flow_bw,
                                    const papof_tensor* warp_bw, const papof_tensor* occlusion, double alpha1, double alpha2,
                                    void* stream, double timing_sec[PAPOF_N_TIMERS]);

/* The forward-backward consistency check of papof_flow_batch_tensor_fb on any two flow tensors: flow_fw, flow_bw float32
 * (widened exactly) or float64, (pair, row, column, {vx, vy}), any non-negative strides; occlusion as there.  For the same
 * float64 flows it is the same mask.  Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null
 * stream) and returns without waiting: ordered behind the work queued there so far, and ahead of what follows.
 * PAPOF_EINVAL, before anything is enqueued: a NULL descriptor or data pointer, a flow that is not float32 / float64, a
 * negative flow stride, the occlusion tensor's refusals and the alphas' above. */
int papof_fb_check_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow_fw,
                          const papof_tensor* flow_bw, double alpha1, double alpha2, const papof_tensor* occlusion,
                          void* stream);

/* Point tracking through the flows of a video of n_frames = T frames (dense point trajectories, Sundaram, Brox, Keutzer
 * 2010), one HIP kernel (track.hip: k_track) that follows every point through all T frames with its state in registers.
 * flow_fw, flow_bw: the T - 1 pairs' flows as papof_fb_check_tensor takes them -- float32 (widened exactly) or float64,
 * (pair, row, column, {vx, vy}), any non-negative strides; pair t runs from frame t to frame t + 1 (flow_fw[t]) and back
 * (flow_bw[t]), as papof_flow_batch_tensor_fb returns them.
 * queries: n_queries rows (t0, x, y) (CoTracker's convention), float32 or float64, stride[0] between points, stride[3]
 * between t0, x and y; or NULL -- dense: every pixel of frame 0 in row-major order, N = height * width, point n =
 * (0, n mod width, n div width).
 * tracks: float64 (frame, point, -, {x, y}), stride[0] frames, stride[1] points, stride[3] x to y; visible: uint8 (frame,
 * point, -, -), stride[0] frames, stride[1] points; other strides are ignored.  For each query:
 *     frame t0: position (x, y) exactly, visible.
 *     forward steps t -> t + 1 for t >= t0: f = flow_fw[t], b = flow_bw[t];
 *     backward steps t -> t - 1 for t <= t0: f = flow_bw[t - 1], b = flow_fw[t - 1]  (a query mid-clip is tracked both ways).
 * One step from a visible position (x, y), in fp64 without fused multiply-adds:
 *     (u, v) = f sampled bilinearly at (x, y)  -- the rule of papof_fb_check_tensor (src/ImageProcessing.h:138-157):
 *     (X, Y) = (x + u, y + v)                     truncation toward zero, fraction clamped to [0, 1], neighbours clamped
 *                                                 into the image, taps accumulated from 0 in (m, n) order
 *     lost if !(X >= 0 && X <= width - 1 && Y >= 0 && Y <= height - 1)                (NaN: lost)
 *     use_check != 0 only:  (bu, bv) = b sampled bilinearly at (X, Y);
 *                           e = (u + bu)^2 + (v + bv)^2;  m = (u^2 + v^2) + (bu^2 + bv^2);
 *                           lost if !(e <= alpha1 * m + alpha2)                       (NaN: lost)
 *     else the position at the next frame is (X, Y), visible.
 * A point lost in one direction stays lost in that direction: its position is the quiet NaN 0x7ff8000000000000 in both
 * coordinates and visible is 0.  A query is invalid -- that NaN and 0 at every frame -- where t0 is not an integer in
 * [0, T - 1], x or y is not finite, or (x, y) lies outside [0, width - 1] x [0, height - 1]; the kernel decides it on the
 * device.  At an integer position of finite flows the bilinear sample is the pixel's value, so in the dense mode visible[1]
 * is papof_fb_check_tensor's forward mask of pair 0, negated, wherever the flows are finite.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting:
 * ordered behind the work queued there so far, and ahead of what follows.
 * PAPOF_EINVAL, before anything is enqueued: a NULL descriptor (queries aside) or data pointer, flows or queries that are not
 * float32 / float64, tracks that are not float64, visible that is not uint8, a negative stride or a zero stride of tracks
 * or visible along an axis in use, n_frames < 2, height or width < 1, n_queries < 1 with queries given, a negative or non-finite alpha. */
int papof_track_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* flow_fw,
                       const papof_tensor* flow_bw, int n_queries, const papof_tensor* queries, int use_check, double alpha1,
                       double alpha2, const papof_tensor* tracks, const papof_tensor* visible, void* stream);

/* Motion-compensated frame interpolation (frame-rate up-conversion; Middlebury's interpolation error, Baker et al., IJCV
 * 2011): the frames at times t in (0, 1) between the two frames of each pair, from its forward flow, its backward flow and,
 * optionally, its occlusion mask -- one HIP kernel (interp.hip: k_interp), one lane per output pixel for every time.
 * frames, frames2: as papof_flow_batch_tensor takes them -- uint8 (x / 255.0, as the flow's ingest), float32 (widened
 * exactly) or float64, (frame, row, column, channel), any non-negative strides, the dtype decided per tensor; sequence != 0:
 * pair i = (frames[i], frames[i + 1]), frames2 NULL; sequence == 0: pair i = (frames[i], frames2[i]).
 * flow_fw (F01), flow_bw (F10): float32 / float64, (pair, row, column, {vx, vy}), any non-negative strides.
 * occlusion: NULL (O0 = O1 = 0), or uint8 (pair, row, column, {fw, bw}) as papof_flow_batch_tensor_fb writes it, any
 * non-negative strides: O0 is channel 0 (pixels of I0), O1 channel 1 (pixels of I1); a nonzero byte reads as 1.0.
 * times: n_times values, each finite and strictly inside (0, 1).
 * out: uint8, float32 or float64; element (pair i, time j, row r, column x, channel ch) at
 *     out.data + i * stride[0] + j * time_stride + r * stride[1] + x * stride[2] + ch * stride[3]   (elements).
 * For pixel p = (x, r) of pair i and each time t, in fp64 without fused multiply-adds, in this order:
 *     s = 1 - t;  (u, v) = F01(r, x);  (bu, bv) = F10(r, x)        -- the flows at p itself (linear motion)
 *     a0 = (t*t)*bu - (s*t)*u;  b0 = (t*t)*bv - (s*t)*v             -- F_t->0 = -s t F01 + t^2 F10
 *     a1 = (s*s)*u - (s*t)*bu;  b1 = (s*s)*v - (s*t)*bv             -- F_t->1 =  s^2 F01 - s t F10
 *     q0 = (x + a0, r + b0);  q1 = (x + a1, r + b1)
 *     in0 = q0 in [0, width - 1] x [0, height - 1]  (false for NaN);  in1 likewise for q1
 *     g0 = I0 sampled bilinearly at q0 (in0 only), g1 = I1 at q1 (in1 only), per channel -- the rule of
 *         papof_fb_check_tensor (src/ImageProcessing.h:138-157): truncation toward zero, fraction clamped to [0, 1],
 *         neighbours clamped into the image, taps accumulated from 0 in (m, n) order; the mask is sampled by the same rule
 *     w0 = in0 ? s * (1 - (in1 ? O1 sampled at q1 : 0)) : 0
 *     w1 = in1 ? t * (1 - (in0 ? O0 sampled at q0 : 0)) : 0
 *     out = (w0*g0 + w1*g1) / (w0 + w1)           if w0 + w1 > 0
 *         = (s*g0 + t*g1) / (s*[in0] + t*[in1])    else if in0 || in1
 *         = s*I0(r, x) + t*I1(r, x)                else
 *     where the term of an unavailable sample is omitted from the numerator (only in0: w0*g0, resp. s*g0).
 * A point of I0 occluded in I1 (O0 = 1) makes g1 unreliable and the reverse for O1 and g0.  The result is stored as float64,
 * float32 (one round-to-nearest) or uint8 = clamp(rint(255 * out), 0, 255) with rint rounding half to even (NaN: 0).
 * Known answer: under constant integer motion F01 = 2d, F10 = -2d, the frame at t = 0.5 is I0 shifted by d (and I1 shifted
 * back by d) wherever both samples stay in the image: q0 = p - d and q1 = p + d are integer points, so g0 = I0(p - d),
 * g1 = I1(p + d), w0 = w1 = 0.5 without a mask, and out = g0 whenever I1(p + d) = I0(p - d).
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting:
 * ordered behind the work queued there so far, and ahead of what follows.  The times travel as kernel arguments.
 * PAPOF_EINVAL, before anything is enqueued: a NULL descriptor (occlusion aside) or data pointer, frames that are not
 * uint8 / float32 / float64, flows that are not float32 / float64, an occlusion mask that is not uint8, an output that is
 * not uint8 / float32 / float64, a negative stride, a zero stride of out or a zero time_stride with n_times > 1, frames2
 * given in sequence mode or missing in pair mode, n_times < 1, times NULL, a time that is not finite or not strictly inside
 * (0, 1), height, width or c < 1, n_pairs < 1. */
int papof_interp_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2,
                        int height, int width, int c, const papof_tensor* flow_fw, const papof_tensor* flow_bw,
                        const papof_tensor* occlusion, int n_times, const double* times, const papof_tensor* out,
                        long long time_stride, void* stream);

/* Global motion of a flow field (video stabilization, camera-motion compensation): one parametric motion per pair fitted to
 * its forward flow by iteratively reweighted least squares (IRLS) with Cauchy weights, in fp64 without fused multiply-adds --
 * two HIP kernels per iteration for all pairs (motion.hip: k_motion_sums, k_motion_solve).
 * flow: float32 (widened exactly) or float64, (pair, row, column, {vx, vy}), any non-negative strides, as
 * papof_fb_check_tensor takes it.  occlusion: NULL, or uint8 (pair, row, column, {fw, bw}) as papof_flow_batch_tensor_fb
 * writes it, any non-negative strides; only channel 0 is read.  model: PAPOF_MOTION_SIMILARITY (scale, rotation,
 * translation: 4 parameters) or PAPOF_MOTION_AFFINE (6).  n_iter >= 1 iterations; scale: the Cauchy scale c in pixels.
 * For pixel (r, x) of a pair, with (u, v) = flow(r, x), H = height, W = width:
 *     valid = (x + u, r + v) in [0, W - 1] x [0, H - 1] (false where u or v is NaN or infinite) and, with a mask, mask == 0
 *     cx = (W - 1) / 2;  cy = (H - 1) / 2;  s = max(W, H) / 2
 *     x^ = (x - cx) / s;  y^ = (r - cy) / s;  X^ = ((x + u) - cx) / s;  Y^ = ((r + v) - cy) / s
 *     iteration 0:       w = valid                                                   (e^2 = 0)
 *     iteration k >= 1:  e_x = (x + u) - ((m00 * x + m01 * r) + m02);  e_y = (r + v) - ((m10 * x + m11 * r) + m12)
 *                        e^2 = e_x * e_x + e_y * e_y;  w = valid ? 1 / (1 + e^2 / (c * c)) : 0
 *                        with M = (m00 m01 m02; m10 m11 m12) the pair's matrix after iteration k - 1
 * and the fourteen sums over the pair's valid pixels, in this order (S0 .. S13):
 *     S0 = sum w (x^ x^)   S1 = sum w (x^ y^)   S2 = sum w (y^ y^)   S3 = sum w x^   S4 = sum w y^   S5 = sum w
 *     S6 = sum w (x^ X^)   S7 = sum w (y^ X^)   S8 = sum w X^        S9 = sum w (x^ Y^)   S10 = sum w (y^ Y^)   S11 = sum w Y^
 *     S12 = sum valid      S13 = sum w e^2
 * The order of the additions is fixed (a lane's pixels, then a fixed tree over lanes, waves and blocks: motion.hip), the
 * same on every run and device, so the results are bitwise reproducible; it is not a row-major running sum.
 * Solve, in normalised coordinates, by Gaussian elimination in natural order without row exchanges:
 *     affine:      (S0 S1 S3; S1 S2 S4; S3 S4 S5) (a00, a01, tx) = (S6, S7, S8),  the same matrix (a10, a11, ty) = (S9, S10, S11)
 *                  X^ = a00 x^ + a01 y^ + tx,  Y^ = a10 x^ + a11 y^ + ty
 *     similarity:  with q = S0 + S2,
 *                  ( q   0    S3  S4 ) (a )   ( S6 + S10 )
 *                  ( 0   q   -S4  S3 ) (b ) = ( S9 - S7  )        X^ = a x^ - b y^ + tx,  Y^ = b x^ + a y^ + ty
 *                  ( S3 -S4   S5  0  ) (tx)   ( S8       )        (a00 = a11 = a, a01 = -b, a10 = b)
 *                  ( S4  S3   0   S5 ) (ty)   ( S11      )
 * and back to pixels: M's linear part is (a00 a01; a10 a11); m02 = (cx + s tx) - (a00 cx + a01 cy),
 * m12 = (cy + s ty) - (a10 cx + a11 cy).  M sends a pixel (x, r) of frame i to its position in frame i + 1.
 * An iteration fails where S5 <= 0, where a pivot of the elimination is not > 1e-12 * S5, or where an entry of M is not
 * finite.  A failed iteration k >= 1 leaves the matrix of the last successful one; a failed iteration 0 gives the identity and
 * ok = 0, and the pair runs no further iterations.
 * motion: float64 (pair, row, column) = M, strides [0..2] > 0 (stride[3] ignored); ok: uint8 (pair), 1 where some iteration
 * succeeded, stride[0] > 0; support: float64 (pair) = S5 of the pair's last iteration / (H * W), stride[0] > 0.
 * workspace: device memory of at least papof_motion_workspace(n_pairs, height, width) bytes, 8-byte aligned, owned by the
 * caller, used by nothing else until the work enqueued here has run (on one stream: PyTorch's allocator on that stream).
 * The handle's arena is not used.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting:
 * ordered behind the work queued there so far, and ahead of what follows.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (occlusion aside) or data pointer, a flow that is not
 * float32 / float64, a mask that is not uint8, a motion or support that is not float64, an ok that is not uint8, a negative
 * stride of flow or occlusion, a zero or negative stride of an output along an axis in use, a model that is not
 * PAPOF_MOTION_*, n_iter < 1, a scale that is not finite or not > 0, n_pairs, height or width < 1, a NULL workspace or
 * workspace_bytes below papof_motion_workspace's value. */
enum { PAPOF_MOTION_SIMILARITY = 0, PAPOF_MOTION_AFFINE = 1 };
int papof_motion_fit_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow,
                            const papof_tensor* occlusion, int model, int n_iter, double scale, const papof_tensor* motion,
                            const papof_tensor* ok, const papof_tensor* support, void* workspace, long long workspace_bytes,
                            void* stream);

/* Bytes of the workspace of papof_motion_fit_tensor: 8 * n_pairs * (8 + 16 * ceil(width / 64) * ceil(height / 32)) -- a
 * state row per pair and one row of partial sums per 64 x 32 block of pixels; -1 for n_pairs, height or width < 1 or
 * more than 2^31 - 1 blocks per pair. */
long long papof_motion_workspace(int n_pairs, int height, int width);

/* Frames warped by one affine matrix each (motion.hip: k_warp_affine): out(i, r, x, ch) = frames[i] sampled at (X, Y), with
 * M = matrices[i] and, in fp64 without fused multiply-adds,
 *     X = (m00 * x + m01 * r) + m02;  Y = (m10 * x + m11 * r) + m12
 * inside [0, width - 1] x [0, height - 1]: the bilinear rule of papof_interp_tensor (src/ImageProcessing.h:138-157:
 * truncation toward zero, fraction clamped to [0, 1], neighbours clamped into the image, taps accumulated from 0 in (m, n)
 * order); outside it, or for a NaN position: 0.
 * frames: uint8 (x / 255.0), float32 (widened exactly) or float64, (frame, row, column, channel), any non-negative strides.
 * matrices: float32 (widened exactly) or float64 (frame, row, column), 2 x 3, any non-negative strides (stride[3] ignored).
 * out: uint8, float32 or float64 (frame, row, column, channel), strides > 0, stored as papof_interp_tensor stores (uint8 =
 * clamp(rint(255 v), 0, 255), half to even).  valid: NULL, or uint8 (frame, row, column), strides [0..2] > 0: 1 where
 * (X, Y) lies in the image, else 0.  out and valid must not overlap the inputs.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (valid aside) or data pointer, frames or out that are
 * not uint8 / float32 / float64, matrices that are not float32 / float64, a valid that is not uint8, a negative stride, a
 * zero stride of out or valid along an axis in use, n_frames, height, width or c < 1. */
int papof_warp_affine_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                             const papof_tensor* matrices, const papof_tensor* out, const papof_tensor* valid, void* stream);

/* Motion-compensated temporal denoising (Liu and Freeman, ECCV 2010; the MCTF pre-filter of video encoders): each pixel of
 * a video of n_frames = T frames is averaged with the points it maps to in frames t +- 1 .. t +- radius, following the
 * video's forward and backward flows hop by hop and dropping a neighbour where the motion fails the forward-backward check
 * -- one HIP kernel (denoise.hip: k_temporal_filter), one lane per output pixel.
 * frames: uint8 (x / 255.0, as the flow's ingest), float32 (widened exactly) or float64, (frame, row, column, channel), any
 * non-negative strides, c = C channels, 1 <= C <= 4.
 * flow_fw, flow_bw: the T - 1 pairs' flows as papof_track_tensor takes them -- float32 (widened exactly) or float64, (pair,
 * row, column, {vx, vy}), any non-negative strides; pair t runs from frame t to frame t + 1 (flow_fw[t]) and back (flow_bw[t]).
 * out: uint8, float32 or float64, (frame, row, column, channel), strides > 0; out must not overlap frames.
 * support: NULL, or uint8 (frame, row, column), strides [0..2] > 0 (stride[3] ignored): the number of neighbours that entered.
 * radius R: 1 .. 16; sigma >= 0 and finite (0: no photometric weight); use_check != 0: the consistency test with alpha1,
 * alpha2 (finite, >= 0).  For the centre pixel p = (x, r) of frame t, with H, W, C, radius R, s2 = sigma * sigma, in fp64
 * without fused multiply-adds:
 *
 * c_k   = frame[t](r, x, k)                         (uint8 as x / 255.0, float32 widened, float64 as is)
 * num_k = c_k;  den = 1.0;  support = 0
 * forward:  (X, Y) = (x, r), alive;  for j = 1 .. min(R, T - 1 - t):
 *               hop from frame t + j - 1 to t + j exactly as k_track's step: flow_fw[t + j - 1] sampled at (X, Y) -> (X + u, Y + v);
 *               alive &= inside [0, W - 1] x [0, H - 1];  with the check: flow_bw[t + j - 1] sampled there,
 *               alive &= (u + bu)^2 + (v + bv)^2 <= a1 * ((u*u + v*v) + (bu*bu + bv*bv)) + a2      (NaN -> not alive)
 *               once not alive, the chain stays dead
 *               if alive: g_k = frame[t + j] sampled at (X, Y) (sampler.h taps, k = 0 .. C-1)
 *                         D = 0; for k: d = g_k - c_k; D += d * d;   D = D / C
 *                         w = sigma > 0 ? 1.0 / (1.0 + D / s2) : 1.0
 *                         if w > 0 (false for NaN): num_k += w * g_k; den += w; support += 1
 * backward: the same from (x, r) for j = 1 .. min(R, t), hop t - j + 1 -> t - j through flow_bw[t - j], checked with flow_fw[t - j]
 * out_k = num_k / den      stored by sampler.h's store() rule (uint8: clamp(rint(255 v), 0, 255), NaN -> 0)
 *
 * The samplers are papof_track_tensor's (flows) and papof_interp_tensor's (frames): the reference's bilinear rule
 * (src/ImageProcessing.h:138-157), truncation toward zero, fraction clamped to [0, 1], neighbours clamped into the image,
 * taps accumulated from 0 in (m, n) order.  All of the forward sums come first, then all of the backward ones, each in order
 * of j: the result is bitwise reproducible.  Where nothing enters, den is 1 and the output is the input value.  float32 out is
 * one round-to-nearest; uint8 rounds half to even.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting:
 * ordered behind the work queued there so far, and ahead of what follows.  No device memory besides the tensors is used.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (support aside) or data pointer, frames or out that
 * are not uint8 / float32 / float64, flows that are not float32 / float64, a support that is not uint8, a negative stride,
 * a zero stride of out or support along an axis in use, n_frames < 2, height or width < 1, c outside 1 .. 4, radius
 * outside 1 .. 16, a sigma that is not finite or negative, an alpha that is not finite or negative. */
int papof_temporal_filter_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                 const papof_tensor* flow_fw, const papof_tensor* flow_bw, int radius, double sigma,
                                 int use_check, double alpha1, double alpha2, const papof_tensor* out,
                                 const papof_tensor* support, void* stream);

/* Flow-guided video completion, 1 of 2 (inpaint.hip: k_fill_*): a field filled inside a mask -- the flows under a removed
 * object before chains can cross it (c = 2), the pixels of a video that no frame shows (papof_propagate_tensor's status 2).
 * x: n_frames frames of height x width x c, 1 <= c <= 4, uint8 (x / 255.0), float32 (widened exactly) or float64, (frame, row,
 * column, channel), any non-negative strides.  mask: uint8 (frame, row, column), any non-negative strides (stride[3]
 * ignored); nonzero marks a hole.  out: uint8, float32 or float64 (frame, row, column, channel), strides > 0, stored by
 * sampler.h's store() rule (uint8: clamp(rint(255 v), 0, 255), half to even; NaN -> 0); out must not overlap x or mask.
 * relax: Jacobi sweeps per level, 0 .. 65536.  Per frame and channel, in fp64 without fused multiply-adds:
 *
 * level 0 (h x w = height x width): v = x, known where mask == 0; v = 0, unknown elsewhere
 * pull, l = 0, 1, ..: level l + 1 is ceil(h / 2) x ceil(w / 2), down to 1 x 1 (levels 0 .. L);  pixel (i, j) of level l + 1:
 *     S = 0; N = 0;  for a = 0, 1: for b = 0, 1: if (2i + a, 2j + b) (row, column) lies in level l and is known there:
 *                                                     S += v_l(2i + a, 2j + b); N += 1
 *     N > 0: v = S / N, known;  N = 0: v = 0, unknown
 * push, l = L - 1 down to 0: a known pixel of level l keeps its value; an unknown pixel (x, y) (column, row) takes
 *     X = clamp(0.5 * x - 0.25, 0, w' - 1),  Y = clamp(0.5 * y - 0.25, 0, h' - 1)    (h' x w': level l + 1, already filled)
 *     v = sum over the four taps of level l + 1 at (X, Y), from 0 in (m, n) order, of v_{l+1}(tap) * weight
 *     (the bilinear rule of papof_interp_tensor: truncation toward zero, fraction clamped to [0, 1], neighbours clamped into
 *     the level)
 *   then `relax` Jacobi sweeps over the unknown pixels of level l, each reading only the previous iterate:
 *     v(x, y) <- ((v(x, y - 1) + v(x, y + 1)) + (v(x - 1, y) + v(x + 1, y))) * 0.25,  neighbours clamped into the level
 *   (level L, 1 x 1, runs none: a sweep there gives its pixel back)
 * out = level 0: a pixel outside the mask is stored from its own input value (out of x's dtype: x's bytes), a hole from v.
 *
 * A frame with no known pixel comes out as zeros.  The result does not depend on the schedule: it is bitwise reproducible.
 * workspace: device memory of at least papof_fill_workspace(n_frames, height, width, c) bytes, 8-byte aligned, owned by the
 * caller, used by nothing else until the work enqueued here has run (on one stream: PyTorch's allocator on that stream).
 * The handle's arena is not used.  All frames go in every launch (blockIdx.y): 2 + L * (2 + relax) launches per call.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor or data pointer, x or out that are not uint8 / float32
 * / float64, a mask that is not uint8, a negative stride, a zero stride of out, n_frames, height or width < 1, c outside
 * 1 .. 4, relax outside 0 .. 65536, a NULL or misaligned workspace, or workspace_bytes below papof_fill_workspace's value. */
int papof_fill_holes_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* x,
                            const papof_tensor* mask, int relax, const papof_tensor* out, void* workspace,
                            long long workspace_bytes, void* stream);

/* Bytes of the workspace of papof_fill_holes_tensor: the sum over its levels l = 0 .. L (h_l x w_l, as stated there) of
 * 16 * c * P + 8 * ceil(P / 8), P = n_frames * h_l * w_l -- two fp64 iterates and a known byte per pixel; -1 for n_frames,
 * height or width < 1, c outside 1 .. 4, or height * width above 2^31 - 1 blocks of 256 pixels. */
long long papof_fill_workspace(int n_frames, int height, int width, int c);

/* Flow-guided video completion, 2 of 2 (inpaint.hip: k_propagate): the holes of T = n_frames frames filled from other frames
 * along the flows, one lane per output pixel.
 * frames: uint8 (x / 255.0), float32 (widened exactly) or float64, (frame, row, column, channel), any non-negative strides,
 * c = C channels, 1 <= C <= 4.  masks: uint8 (frame, row, column), any non-negative strides; nonzero marks a hole.
 * flow_fw, flow_bw: the T - 1 (completed) flows as papof_track_tensor takes them, float32 / float64 (pair, row, column,
 * {vx, vy}), any non-negative strides; pair t runs from frame t to frame t + 1 (flow_fw[t]) and back (flow_bw[t]).
 * out: uint8, float32 or float64 (frame, row, column, channel), strides > 0, sampler.h's store() rule; status: uint8 (frame,
 * row, column), strides [0..2] > 0; neither may overlap the inputs.  radius R: 1 .. T - 1; use_check != 0: the consistency
 * test with alpha1, alpha2 (finite, >= 0).  For pixel p = (x, r) of frame t, in fp64 without fused multiply-adds:
 *
 * masks[t](r, x) == 0:  out = frame[t](r, x) (its own input value), status = 0
 * a hole:
 *   forward:  (X, Y) = (x, r), alive;  for j = 1 .. min(R, T - 1 - t):
 *                 hop from frame t + j - 1 to t + j exactly as papof_temporal_filter_tensor's: flow_fw[t + j - 1] sampled at
 *                 (X, Y) -> (X + u, Y + v); alive &= inside [0, W - 1] x [0, H - 1]; with the check, flow_bw[t + j - 1]
 *                 sampled there, alive &= (u + bu)^2 + (v + bv)^2 <= a1 * ((u*u + v*v) + (bu*bu + bv*bv)) + a2 (NaN -> not
 *                 alive); a chain that dies stays dead and gives no candidate
 *                 if alive and masks[t + j] is 0 at all four clamped taps of (X, Y) (sampler.h: taps_at; whatever their
 *                 weights): g_f = frame[t + j] sampled at (X, Y) (per channel), d_f = j; the chain stops
 *   backward: the same from (x, r) for j = 1 .. min(R, t), hop t - j + 1 -> t - j through flow_bw[t - j], checked with
 *             flow_fw[t - j]: g_b, d_b
 *   both:     w_f = 1.0 / d_f, w_b = 1.0 / d_b, out_k = (w_f * g_f,k + w_b * g_b,k) / (w_f + w_b), status = 1
 *   one:      out = that candidate's g, status = 1
 *   none:     out = frame[t](r, x) (its own input value), status = 2
 *
 * The samplers are papof_temporal_filter_tensor's.  Enqueued on `stream` (the caller's hipStream_t on the handle's device,
 * NULL: the null stream) and returns without waiting.  No device memory besides the tensors is used; no atomics.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor or data pointer, frames or out that are not uint8 /
 * float32 / float64, masks or status that are not uint8, flows that are not float32 / float64, a negative stride, a zero
 * stride of out or status along an axis in use, n_frames < 2, height or width < 1, c outside 1 .. 4, radius outside
 * 1 .. n_frames - 1, an alpha that is not finite or negative. */
int papof_propagate_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                           const papof_tensor* masks, const papof_tensor* flow_fw, const papof_tensor* flow_bw, int radius,
                           int use_check, double alpha1, double alpha2, const papof_tensor* out, const papof_tensor* status,
                           void* stream);

/* Blind video temporal consistency (Bonneel et al., SIGGRAPH Asia 2015; consistency.hip): a video P that a per-frame process
 * made from the video I, made consistent along I's flows -- each output frame keeps P_t's spatial gradients and follows the
 * previous output frame, warped along the flow, where the flow can be trusted.  One screened-Poisson solve per frame, the
 * frames a chain: frame t starts when frame t - 1 is stored.  Callers discover it by its symbol.
 * frames I: uint8 (x / 255.0), float32 (widened exactly) or float64, (frame, row, column, channel), any non-negative strides,
 * c_frames = C_I channels.  processed P: the same dtypes, (frame, row, column, channel), any non-negative strides, c_out = C_P
 * channels; 1 <= C_I, C_P <= 4 (they may differ).  flow_fw, flow_bw: the T - 1 pairs' flows as papof_track_tensor takes them,
 * float32 / float64 (pair, row, column, {vx, vy}), any non-negative strides; pair t - 1 runs from frame t - 1 to t:
 * flow_bw[t - 1] lives on frame t's grid and points into frame t - 1.  first: NULL (frame 0 is P_0), or one frame of C_P
 * channels, uint8 / float32 / float64 (ignored, row, column, channel), strides [1..3] >= 0.  out O: uint8, float32 or float64
 * (frame, row, column, channel), strides > 0, C_P channels, stored by sampler.h's store() rule (uint8: clamp(rint(255 v), 0,
 * 255), half to even; NaN -> 0); out must not overlap an input or the workspace.  lambda >= 0, sigma >= 0, both finite;
 * iters 0 .. 65536; use_check != 0: the consistency test with alpha1, alpha2 (finite, >= 0).
 * In fp64 without fused multiply-adds, with H, W, n(p) = the number of p's 4-neighbours inside the image:
 *
 * O_0 = store(first) if first != NULL, else store(P_0)
 * frame t = 1 .. T - 1, pixel p = (x, r):
 *   hop, exactly as papof_temporal_filter_tensor's backward hop: (u, v) = flow_bw[t - 1] sampled at (x, r) (sampler.h taps),
 *     (X, Y) = (x + u, r + v); valid = inside [0, W - 1] x [0, H - 1]; with the check, (fu, fv) = flow_fw[t - 1] sampled at
 *     (X, Y), valid &= (u + fu)^2 + (v + fv)^2 <= a1 * ((u*u + v*v) + (fu*fu + fv*fv)) + a2      (NaN -> not valid)
 *   if valid: D = 0; for k < C_I: d = I_t,k(p) - I_{t-1},k sampled at (X, Y); D += d * d;   D = D / C_I
 *             w = sigma > 0 ? lambda / (1.0 + D / (sigma * sigma)) : lambda
 *   w = 0 where not valid or where w is not > 0 (lambda = 0, a NaN); then a = 0 and r_k = 0; else a = w / lambda and
 *             r_k = (O_{t-1},k read back in out's dtype, sampled at (X, Y)) - P_t,k(p)                      (k < C_P)
 *   start value delta0 (per channel), pull-push with confidences (papof_fill_holes_tensor's levels, child order and push
 *   point): level 0 holds (a, r); level l + 1 is ceil(h / 2) x ceil(w / 2), down to 1 x 1 (levels 0 .. L)
 *     pull, pixel (i, j) of level l + 1: over the children (2i + a', 2j + b') inside level l, a' then b', from 0:
 *           A = sum of a_child;  S_k = sum of a_child * v_child,k;   v_k = A > 0 ? S_k / A : 0;   a = min(A, 1)
 *     push, l = L - 1 down to 0 (level L keeps its pulled value): g_k = level l + 1 (already pushed) sampled by the taps at
 *           (clamp(0.5 x - 0.25, 0, w' - 1), clamp(0.5 y - 0.25, 0, h' - 1)), accumulated from 0 in (m, n) order;
 *           v_k <- a * v_k + (1.0 - a) * g_k
 *     delta0 = level 0 after its push (a 1 x 1 frame, L = 0: r itself)
 *   iters Jacobi sweeps of (L + diag w) delta = w r, L the 4-neighbour graph Laplacian with Neumann borders; each reads only
 *   the previous iterate:
 *     S = ((delta(x, r - 1) + delta(x, r + 1)) + (delta(x - 1, r) + delta(x + 1, r))), a neighbour outside the image
 *         entering as +0.0 (as leaving it out, but for the sign of a zero sum)
 *     den = n(p) + w;   delta(p) <- den != 0 ? (S + w * r_k) / den : 0      (den = 0: a 1 x 1 frame with w = 0)
 *   O_t,k(p) = store(P_t,k(p) + delta_k(p))
 *
 * This is Jacobi on the minimiser of sum over edges of (grad O - grad P)^2 + sum over p of w (O - Ohat)^2, O = P_t + delta.
 * lambda = 0: w = a = r = 0 everywhere and delta = +0.0, so O = store(P + 0.0): with out of P's dtype, P's bytes, but for a
 * float -0.0 of P, which comes back as +0.0.  O_{t-1} is read back from out, so a video cut into chunks that overlap by one
 * frame, each chunk given the previous chunk's last output frame as `first` (of out's dtype), gives the bytes of one call.
 * The result does not depend on the schedule or on PAPOF_TC_DEPTH (sweeps per launch): it is bitwise reproducible.
 * workspace: device memory of at least papof_consistency_workspace(height, width, c_out) bytes, 8-byte aligned, owned by
 * the caller, used by nothing else until the work enqueued here has run (on one stream: PyTorch's allocator on that
 * stream); it holds one frame's levels and is reused by every frame.  The handle's arena is not used.  Per frame t >= 1:
 * 1 + 2 L + max(1, ceil(iters / depth)) launches, depth = PAPOF_TC_DEPTH (1 .. 15, default 8); one more for frame 0.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream), back to back with no host
 * synchronisation, and returns without waiting.  No atomics.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (first aside) or data pointer, frames, processed,
 * first or out that are not uint8 / float32 / float64, flows that are not float32 / float64, a negative stride, a zero
 * stride of out, out overlapping an input or the workspace, the workspace overlapping an input, n_frames < 2, height or
 * width < 1, c_frames or c_out outside 1 .. 4, a lambda or sigma that is not finite or negative, iters outside 0 .. 65536,
 * an alpha that is not finite or negative, a NULL or misaligned workspace, or workspace_bytes below
 * papof_consistency_workspace's value. */
int papof_temporal_consistency_tensor(papof_handle* h, int n_frames, int height, int width, int c_frames, int c_out,
                                      const papof_tensor* frames, const papof_tensor* processed, const papof_tensor* flow_fw,
                                      const papof_tensor* flow_bw, const papof_tensor* first, double lambda, double sigma,
                                      int iters, int use_check, double alpha1, double alpha2, const papof_tensor* out,
                                      void* workspace, long long workspace_bytes, void* stream);

/* Bytes of the workspace of papof_temporal_consistency_tensor: 8 * ((2 + 3 c_out) P_0 + sum over levels l = 1 .. L of
 * (1 + c_out) P_l), P_l = h_l * w_l (the levels stated there) -- level 0's confidences, weights, residuals and two iterates,
 * each coarser level's confidences and values, all fp64; -1 for height or width < 1, c_out outside 1 .. 4, or
 * height * width above 2^31 - 1 blocks of 256 pixels. */
long long papof_consistency_workspace(int height, int width, int c_out);

/* Forward warping (splatting): every source pixel of x is moved along its own flow and deposited, bilinearly, where it lands
 * (softmax splatting, Niklaus and Liu, CVPR 2020, with the caller's weights) -- how a frame, a flow or a mask is carried to
 * the frame it points to.  Three steps on `stream`: the accumulator is cleared (hipMemsetAsync), k_splat (splat.hip; one lane
 * per SOURCE pixel) adds, k_splat_resolve (one lane per TARGET pixel) divides and stores.
 * x: uint8 (x / 255.0, as the flow's ingest), float32 (widened exactly) or float64, (item, row, column, channel), any
 * non-negative strides.  flow: float32 / float64, (item, row, column, {vx, vy}).  weight: NULL (1.0 everywhere) or float32 /
 * float64, (item, row, column, -): stride[3] is not read.  times: n_times finite values (0: the identity deposit; outside
 * [0, 1]: extrapolation).  bound = 2^k, k an integer in [-20, 20]: values are scaled by 1 / bound (exact) before they are
 * quantised; 1.0 for frames, for a flow field a bound on |x|.  A value with |x / bound| > 1 is the caller's error: the kernel
 * clamps x / bound to [-1, 1] (fmin(fmax(., -1), 1): a NaN reads as -1), so that no sum can overflow.
 * For source pixel (i, j) of item b and time t, in fp64 without fused multiply-adds:
 *     (u, v) = flow[b, j, i];  w = weight[b, j, i]
 *     skip the pixel if u, v or w is not finite, or !(w > 0);   w = min(w, 1)
 *     X = i + t * u;  Y = j + t * v;       skip unless -1 < X < width and -1 < Y < height
 *     x0 = floor(X); y0 = floor(Y); fx = X - x0; fy = Y - y0
 *     for (m, n) in (0,0), (0,1), (1,0), (1,1):    target (x0 + n, y0 + m); the tap is dropped if it is outside the image
 *         b_mn = (m ? fy : 1 - fy) * (n ? fx : 1 - fx);   wb = w * b_mn;   the tap is dropped if wb == 0
 *         den[target]    += (int64) rint(wb * 4294967296.0)
 *         num[target, c] += (int64) rint((wb * clamp(x[c] * (1 / bound))) * 4294967296.0)         for each channel c
 * with rint rounding half to even.  Then, per target pixel:
 *     coverage = (double) den * 2^-32
 *     out[c]   = den >= 256 (a coverage of 2^-24) ? ((double) num[c] / (double) den) * bound : fill
 * A hole is coverage < 2^-24.  out: uint8, float32 or float64, stored as papof_interp_tensor stores; element (item b, time k,
 * row, column, channel) at out.data + b * stride[0] + k * time_stride + row * stride[1] + column * stride[2] + c * stride[3].
 * coverage: NULL, or float64 with the axes (item, time, row, column).
 * The sums are made with 64-bit integer atomic adds: integer addition is associative, so the order of arrival cannot change
 * a bit and the results are bitwise reproducible.  Every term is at most 2^32 in magnitude and a target receives at most
 * one tap per source pixel, so with height * width < 2^30 no sum leaves int64.
 * workspace: device memory, 8-byte aligned, owned by the caller for the duration of the enqueued work -- the accumulator,
 * int64 planes [item][time][c + 1][row][column] with den's last.  One time of all items takes T1 = 8 n height width (c + 1) bytes;
 * workspace_bytes must be at least T1, and the call makes the times in groups of min(n_times, 16, workspace_bytes / T1) per
 * clear-add-resolve round, with the same results for every grouping.  papof_splat_workspace returns
 * min(n_times, 16, max(1, 2^30 / T1)) * T1: every time at once up to 1 GiB, never less than one time.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL descriptor (weight and coverage aside) or data pointer, a dtype other
 * than those above, a negative stride, a zero stride of out or coverage or a zero time_stride with n_times > 1, n, height,
 * width, c or n_times < 1, height * width >= 2^30, c > 2^20, a workspace beyond 2^62 bytes, times NULL or not finite, a
 * bound that is not such a power of two, a NULL or too small workspace. */
int papof_splat_tensor(papof_handle* h, int n, int height, int width, int c, const papof_tensor* x, const papof_tensor* flow,
                       const papof_tensor* weight, int n_times, const double* times, double bound, double fill,
                       const papof_tensor* out, long long time_stride, const papof_tensor* coverage, void* workspace,
                       long long workspace_bytes, void* stream);

/* Bytes of the workspace papof_splat_tensor is best given (stated there); -1 where that call refuses the sizes. */
long long papof_splat_workspace(int n, int n_times, int height, int width, int c);

/* Frame interpolation by splatting: papof_interp_tensor's arguments (frames, flows, mask, times strictly inside (0, 1), out
 * and time_stride, sequence mode) plus the weights of the two frames' pixels -- weight_fw for the pixels of I0, weight_bw
 * for those of I1, each NULL (1.0) or float32 / float64 (pair, row, column, -) -- and a workspace.  For each time t, I0 is
 * accumulated along t * F01 with weight_fw into (num0, den0) and I1 along (1 - t) * F10 with weight_bw into (num1, den1),
 * both by papof_splat_tensor's rule with bound = 1; then, per target pixel (k_interp_splat), with s = 1 - t:
 *     den = s * (double) den0 + t * (double) den1;      num[c] = s * (double) num0[c] + t * (double) num1[c]
 *     out[c] = den >= 256.0 ? num[c] / den : the value papof_interp_tensor's rule gives at this pixel (with the mask, if given)
 * The occlusion mask affects only that fallback: the pixels hidden in the OTHER frame are the ones that must be splatted.
 * Unlike papof_interp_tensor, whose flows are read at the output pixel, every pixel moves along its own flow: the result
 * stays right at motion boundaries.  workspace: as papof_splat_tensor's with 2 n_pairs items (the two accumulators of a
 * group of times, one after the other): papof_splat_workspace(2 * n_pairs, n_times, height, width, c).
 * PAPOF_EINVAL, before anything is enqueued: as papof_interp_tensor and papof_splat_tensor. */
int papof_interp_splat_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                              const papof_tensor* frames2, int height, int width, int c, const papof_tensor* flow_fw,
                              const papof_tensor* flow_bw, const papof_tensor* weight_fw, const papof_tensor* weight_bw,
                              const papof_tensor* occlusion, int n_times, const double* times, const papof_tensor* out,
                              long long time_stride, void* workspace, long long workspace_bytes, void* stream);

/* Edge-aware flow refinement: the image-guided weighted median filter of a flow field (the non-local term of Sun, Roth and
 * Black, "Secrets of optical flow estimation and their principles", CVPR 2010, as a post-process).  One kernel per pass on
 * `stream` (k_refine, refine.hip: one lane per output pixel, the tile and its halo staged in LDS, a weighted quickselect).
 * flow: float32 (widened exactly) or float64, (item, row, column, {vx, vy}), any non-negative strides.  guide: uint8, float32
 * (widened exactly) or float64, (item, row, column, channel), c channels, c in 1 .. 4; its RAW values enter the rule (a
 * uint8 sample as the integer 0 .. 255): the guide's scale and the division by c live in q.  occlusion: NULL, or uint8
 * (item, row, column, -), nonzero = this pixel's flow is not to be trusted.  where: NULL (every pixel), or uint8 (item, row,
 * column, -), nonzero = filter this pixel; the others are copied.  stride[3] of the masks is not read.
 * radius r in 1 .. 15; S: DEVICE pointer to the (2 r + 1)^2 spatial weights, row-major in (dy, dx); R: DEVICE pointer to the
 * 4096 range weights; S[.] * R[.] must stay below 2^31 (papof_refine_tables' do); q finite and >= 0; iters in 1 .. 65536.
 * For output pixel p of an item, and every neighbour p' = p + (dx, dy), |dx|, |dy| <= r, inside the image:
 *     D = (g_0(p) - g_0(p'))^2 + (g_1(p) - g_1(p'))^2 + ...     fp64, channels added in order from 0, no fused multiply-add
 *     p' is DEAD (w = 0) if D is not finite, if a component of flow[p'] is not finite, or if occlusion[p'] != 0;
 *     otherwise  k = (int) min(D * q, 4095.0)   (one fp64 product)   and   w = S[(dy + r) * (2 r + 1) + dx + r] * R[k]
 *     T = sum of w                                                        (unsigned 64-bit)
 *     per component (vx, then vy) separately: out = the smallest value x among the neighbours with w > 0 for which
 *         2 * sum{w : value <= x} >= T                                    (the lower weighted median)
 * Values are ordered by the monotone integer key of their float64 bits (b ^ ((b >> 63) & 0x7fff...f), compared as signed
 * 64-bit integers), so -0.0 sorts below +0.0 and the result is the bits of one particular neighbour.  There is no float
 * sum, so nothing depends on an order of evaluation: the result is a pure function of the inputs, bitwise reproducible.
 * If T = 0 (every neighbour dead) or where[p] = 0 the output is flow[p].  The centre is an ordinary neighbour: dead if
 * occluded or not finite, which is how such a pixel takes its neighbours' motion.
 * iters > 1 repeats the pass on its own output (guide, masks and tables unchanged); the intermediate fields are float64 in
 * the workspace, so a float64 flow stored as float32 is rounded once, to nearest, at the end.  out: float32 / float64,
 * (item, row, column, {vx, vy}), positive strides; it must not overlap flow (a block reads its neighbours' pixels).
 * passes: NULL, or uint8 (item, row, column, -): a measurement aid, the passes over the window that the pixel's lane made in
 * the last iteration (0: copied; 1: T = 0 or both components constant; saturating at 255).
 * Tables as papof_refine_tables fills them, with q = 128 / (sigma_c^2 c) for a float guide in 0 .. 1 and
 * 128 / (sigma_c^2 c 255^2) for a uint8 guide, give the weight exp(-(dx^2 + dy^2) / (2 sigma_s^2)) * exp(-d2 / (2 sigma_c^2)),
 * d2 the mean over channels of the squared difference of the guide scaled to 0 .. 1, sampled in 4096 bins up to
 * d2 = 32 sigma_c^2 and zero beyond.
 * workspace: device memory, 8-byte aligned, owned by the caller for the duration of the enqueued work;
 * papof_refine_workspace gives its bytes (0 for iters = 1: workspace may then be NULL).
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (occlusion, where and passes aside) or data pointer,
 * a dtype other than those above, a negative stride or a zero stride of out, n, height or width < 1, height * width >= 2^30,
 * a workspace beyond 2^62 bytes, c outside 1 .. 4, radius outside 1 .. 15, S or R NULL, q negative or not finite,
 * iters outside 1 .. 65536, a NULL or too small workspace where one is needed. */
int papof_refine_flow_tensor(papof_handle* h, int n, int height, int width, int c, const papof_tensor* flow,
                             const papof_tensor* guide, const papof_tensor* occlusion, const papof_tensor* where, int radius,
                             const unsigned* S, const unsigned* R, double q, int iters, const papof_tensor* out,
                             const papof_tensor* passes, void* workspace, long long workspace_bytes, void* stream);

/* Bytes of papof_refine_flow_tensor's workspace: 0 for iters = 1, one float64 field (16 n height width) for iters = 2, two
 * for more; -1 where that call refuses the sizes (n, height or width < 1, iters outside 1 .. 65536, height * width >= 2^30,
 * beyond 2^62). */
long long papof_refine_workspace(int n, int height, int width, int iters);

/* The tables of papof_refine_flow_tensor on the HOST, with libm's exp:
 *     S[(dy + r) * (2 r + 1) + dx + r] = rint(32768 * exp(-(dx^2 + dy^2) / (2 sigma_s^2))),   |dx|, |dy| <= r = radius
 *     R[k] = rint(65536 * exp(-(k + 0.5) / 256)),   k = 0 .. 4095        (R[0] = 65408, R[4095] = 0; no sigma enters)
 * PAPOF_EINVAL: radius outside 1 .. 15, sigma_s not finite or <= 0, S or R NULL. */
int papof_refine_tables(int radius, double sigma_s, unsigned* S, unsigned* R);

/* Flow at reduced resolution (upsample.hip): the box decimation of frames, and the edge-aware up-sampling of a flow that was
 * estimated on the decimated frames, guided by the full-resolution frame: joint bilateral upsampling (Kopf, Cohen,
 * Lischinski, Uyttendaele, SIGGRAPH 2007).  In both calls the low-resolution grid of an H x W frame at `factor` f in 2 .. 4
 * is h x w = ceil(H / f) x ceil(W / f), and cell (y, x) covers the pixels (f y .. f y + f - 1, f x .. f x + f - 1) that exist.
 *
 * Box decimation, one kernel on `stream` (k_decimate: one lane per low-resolution pixel).  frames: uint8 (a sample k is
 * k / 255.0, one fp64 division), float32 (widened exactly) or float64, (item, row, column, channel), c channels, c in
 * 1 .. 4, any non-negative strides.  out: float32 / float64, (item, row, column, channel) at h x w, positive strides.
 *     out[y, x, ch] = (sum of the samples of cell (y, x), added from 0.0 in row-major order, fp64) / (their number)
 * One fp64 division; a float32 out is rounded once, to nearest.  Edge cells are clipped, so no row or column is dropped and a
 * height or width of 1 is legal.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor or data pointer, a dtype other than those above, a
 * negative stride or a zero stride of out, n, height or width < 1, c outside 1 .. 4, factor outside 2 .. 4. */
int papof_decimate_tensor(papof_handle* h, int n, int height, int width, int c, int factor, const papof_tensor* frames,
                          const papof_tensor* out, void* stream);

/* Edge-aware up-sampling of a low-resolution flow, one kernel on `stream` (k_upsample_flow: one lane per output pixel on a
 * 32 x 8 tile, the tile's low-resolution window staged in LDS).
 * flow_lr: float32 (widened exactly) or float64, (item, row, column, {vx, vy}) at h x w, in low-resolution pixels.  guide:
 * uint8 (k / 255.0), float32 or float64, (item, row, column, channel) at height x width, c channels in 1 .. 4.  guide_lr:
 * float32 / float64 at h x w, the guide as the decimation above gives it (a float guide is taken as it is: guide and guide_lr
 * must be in one scale).  occlusion: NULL, or uint8 (item, row, column, -) at h x w, nonzero = this cell's flow is not to be
 * trusted; stride[3] is not read.  Any non-negative strides.  radius r in 0 .. 3; S: DEVICE pointer to the f^2 (2 r + 1)^2
 * spatial weights, R: DEVICE pointer to the 1024 range weights, as the tables call below fills them (every entry of both
 * >= 1 and S[.] * R[.] < 2^53); q finite and >= 0.
 * For output pixel (Y, X) of an item, with centre cell (cy, cx) = (Y / f, X / f) and phase (py, px) = (Y % f, X % f), and
 * every tap (dy, dx), |dy|, |dx| <= r, rows outer (dy, then dx, ascending), whose cell (cy + dy, cx + dx) is in the grid:
 *     the cell is DEAD if a component of flow_lr there is not finite or occlusion there is nonzero: it is skipped;
 *     D = (g_0(Y, X) - gl_0(cell))^2 + (g_1(Y, X) - gl_1(cell))^2 + ...   fp64, channels added in order from 0.0, no fused
 *                                                                          multiply-add
 *     k = (int)(D * q) if D * q < 1023.0, else 1023 (a NaN included)      (one fp64 product)
 *     w = S[((py * f + px) * (2 r + 1) + dy + r) * (2 r + 1) + dx + r] * R[k]     (an integer, exact as a float64)
 *     su = su + w * vx(cell),  sv = sv + w * vy(cell),  sw = sw + w        (fp64 products and sums from 0.0; sw exact)
 *     out(Y, X) = (su / sw * f, sv / sw * f)                               (one division and one product per component)
 * The flow is scaled by f because it is measured in pixels.  Every live tap has w >= 1, so sw = 0 only when every tap is
 * dead: the output is then (f * vx, f * vy) of the centre cell as it is, occluded or not, NaN and infinities included.
 * Nothing depends on an order of evaluation other than the stated one: the result is a pure function of the inputs.
 * out: float32 / float64, (item, row, column, {vx, vy}) at height x width, positive strides, overlapping no input.
 * Tables as filled below with q = 32 / (sigma_c^2 c) give the range weight exp(-d2 / (2 sigma_c^2)), d2 the mean over
 * the channels of the squared difference of guides scaled to 0 .. 1, in 1024 bins up to d2 = 32 sigma_c^2.
 * Enqueued on `stream` and returns without waiting, like the decimation.  PAPOF_EINVAL, before anything is enqueued: a NULL
 * handle, descriptor (occlusion aside) or data pointer, a dtype other than those above, a negative stride or a zero stride
 * of out, n, height or width < 1, c outside 1 .. 4, factor outside 2 .. 4, radius outside 0 .. 3, S or R NULL, q negative
 * or not finite. */
int papof_upsample_flow_tensor(papof_handle* h, int n, int height, int width, int c, int factor, const papof_tensor* flow_lr,
                               const papof_tensor* guide, const papof_tensor* guide_lr, const papof_tensor* occlusion,
                               int radius, const unsigned* S, const unsigned* R, double q, const papof_tensor* out,
                               void* stream);

/* The tables of the up-sampling on the HOST, with libm's exp.  With (ty, tx) = (dy - (py - (f - 1) / 2) / f,
 * dx - (px - (f - 1) / 2) / f), the tap's cell centre seen from the pixel, in cells:
 *     S[((py * f + px) * (2 r + 1) + dy + r) * (2 r + 1) + dx + r] =
 *         max(1, rint(32768 * (15 / 16 * max(0, 1 - |tx|) * max(0, 1 - |ty|) + 1 / 16 * exp(-(tx^2 + ty^2) / (2 sigma_s^2)))))
 *     R[k] = max(1, rint(65536 * exp(-(k + 0.5) / 64))),   k = 0 .. 1023      (R[0] = 65026; 1 from k = 684 on)
 * The tent is the bilinear weight: where the guide is flat the result is bilinear up-sampling to within 1 / 16; the Gaussian
 * is the reach beyond the four nearest cells that lets a pixel next to an edge find cells of its own side.
 * PAPOF_EINVAL: factor outside 2 .. 4, radius outside 0 .. 3, sigma_s not finite or <= 0, S or R NULL. */
int papof_upsample_tables(int factor, int radius, double sigma_s, unsigned* S, unsigned* R);

/* Multi-frame super-resolution along the flows (superres.hip): every pixel of every frame is carried along the chains of
 * flows to the frames around it and deposited on a grid `scale` times finer (shift and add: Farsiu, Robinson, Elad, Milanfar
 * 2004), the sums are resolved against a cubic upsampling of the target frame, and `iters` steps of back-projection
 * (Irani and Peleg 1991) against the target frame alone follow.  The sensor model is the scale x scale box; there is no
 * deconvolution of the optics' blur beyond it and no learned prior.  Per round on `stream`: the accumulator is cleared
 * (hipMemsetAsync), k_sr_accumulate (one lane per SOURCE pixel) adds, k_sr_resolve (one lane per FINE pixel) divides,
 * k_sr_backproject (one block per tile of low-resolution pixels) runs `iters` times.
 * frames: n_frames = T >= 1 frames of height x width x c (H, W, C), 1 <= c <= 4, uint8 (x / 255.0), float32 (widened
 * exactly) or float64, (frame, row, column, channel), any non-negative strides.  flow_fw, flow_bw: float32 / float64, (pair,
 * row, column, {vx, vy}), T - 1 pairs, pair t from frame t to t + 1 and back; not read (may be NULL) when T = 1 or radius = 0.
 * scale S: 2, 3 or 4.  out: uint8, float32 or float64, (frame, row, column, channel) of T frames of S H x S W, strides > 0.
 * coverage: NULL, or float64 (frame, row, column) of S H x S W, strides [0..2] > 0 (stride[3] is not read).
 * A low-resolution coordinate p and the fine-grid coordinate q of the same point: q = S * (p + 0.5) - 0.5 (pixel centres).
 * In fp64 without fused multiply-adds, with R = radius, s2 = sigma * sigma:
 *
 * Accumulate.  For every source pixel (i, j) (column, row) of every frame k:
 *     v_c = frame[k](j, i, c);   val_c = fmin(fmax(v_c, -1), 1)       (papof_splat_tensor's clamp with bound 1)
 *     deposit(k, (i, j), 1.0)
 *     forward:  (X, Y) = (i, j);  for n = 1 .. min(R, T - 1 - k): hop from frame k + n - 1 to k + n exactly as
 *               papof_temporal_filter_tensor's (flow_fw[k + n - 1] sampled at (X, Y), the image test, with use_check the
 *               test against flow_bw[k + n - 1] sampled where it lands); once dead, the chain stays dead.  If alive:
 *                   g_c = frame[k + n] sampled at (X, Y) (sampler.h taps);  D = 0; for c: d = v_c - g_c; D += d * d;  D = D / C
 *                   w = (use_sigma != 0 and sigma > 0) ? 1.0 / (1.0 + D / s2) : 1.0
 *                   if w > 0 (false for NaN): deposit(k + n, (X, Y), w)
 *     backward: the same for n = 1 .. min(R, k), hop k - n + 1 -> k - n through flow_bw[k - n], checked with flow_fw[k - n],
 *               into the targets k - n.
 *     deposit(t, (PX, PY), w):  QX = S * (PX + 0.5) - 0.5;  QY = S * (PY + 0.5) - 0.5;  then papof_splat_tensor's taps on
 *         target t's fine grid:  x0 = floor(QX); y0 = floor(QY); fx = QX - x0; fy = QY - y0
 *         for (m, n) in (0,0), (0,1), (1,0), (1,1):  fine pixel (x0 + n, y0 + m), dropped outside the S W x S H grid
 *             b_mn = (m ? fy : 1 - fy) * (n ? fx : 1 - fx);   wb = w * b_mn;   dropped if wb == 0
 *             den[t, pixel]    += (int64) rint(wb * 4294967296.0)
 *             num[t, pixel, c] += (int64) rint((wb * val_c) * 4294967296.0)
 * A fine pixel receives at most one tap of each source pixel of at most 2 R + 1 frames and every term is at most 2^32 in
 * magnitude, so with (2 R + 1) H W < 2^30 no sum leaves int64; integer sums: the order of arrival cannot change a bit.
 *
 * Resolve.  For the fine pixel (x, y) of target t:  px = (x + 0.5) / S - 0.5;  py = (y + 0.5) / S - 0.5;
 *     x0 = floor(px); tx = px - x0;  y0 = floor(py); ty = py - y0
 *     the cubic convolution weights (Keys 1981, a = -0.5) of the taps at -1, 0, 1, 2, for f = tx (wx) and f = ty (wy):
 *         w[0] = ((-0.5 * f + 1.0) * f - 0.5) * f;     w[1] = (1.5 * f - 2.5) * f * f + 1.0
 *         w[2] = ((-1.5 * f + 2.0) * f + 0.5) * f;     w[3] = (0.5 * f - 0.5) * f * f
 *     base_c = 0; for m = 0 .. 3: { row = 0; for n = 0 .. 3: row += wx[n] * frame[t](clamp(y0 - 1 + m), clamp(x0 - 1 + n), c);
 *                                   base_c += wy[m] * row }           (indices clamped into the image)
 *     coverage = (double) den * 2^-32
 *     X_c = ((double) num_c * 2^-32 + prior * base_c) / (coverage + prior)
 * prior > 0 makes every pixel defined and is the whole answer where nothing lands.
 *
 * Back-projection, `iters` Jacobi steps (all of X is read before any of it is replaced), per target t and channel:
 *     per low-resolution pixel (i, j):  sum = 0; for m = 0 .. S-1: for n = 0 .. S-1: sum += X(S j + m, S i + n)
 *                                       r(j, i) = frame[t](j, i, c) - sum / (S * S)
 *     per fine pixel, with px, py, x0, y0, tx, ty as above and x1 = x0 + 1, y1 = y0 + 1, all four indices clamped:
 *         top = (1 - tx) * r(y0, x0) + tx * r(y0, x1);   bot = (1 - tx) * r(y1, x0) + tx * r(y1, x1)
 *         X' = X + ((1 - ty) * top + ty * bot)
 * out = X stored by sampler.h's store() rule (uint8: clamp(rint(255 v), 0, 255), half to even, NaN -> 0; float32: one
 * round-to-nearest).
 *
 * workspace: device memory, 8-byte aligned, owned by the caller for the duration of the enqueued work.  One target frame
 * takes P = 8 S^2 H W ((c + 1) + (iters > 0 ? 2 c : 0)) bytes: the accumulator, int64 planes [target][c + 1][S H][S W] with
 * den's last, and with iters > 0 the two float64 buffers [target][c][S H][S W] of X.  workspace_bytes must be at least P; the
 * call makes the targets in rounds of G = min(T, workspace_bytes / P) -- the targets [t0, t0 + G) accumulate from the sources
 * [t0 - R, t0 + G + R) -- with the same results for every grouping.  papof_sr_workspace returns min(T, max(1, 2^31 / P)) * P:
 * as many target frames as fit 2 GiB, never less than one.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting;
 * nothing of the handle's own memory is used.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (coverage aside; the flows where they are not read)
 * or data pointer, a dtype other than those above, a negative stride, a zero stride of out or coverage, n_frames, height or
 * width < 1, c outside 1 .. 4, scale outside 2 .. 4, radius < 0, (2 radius + 1) * height * width >= 2^30, a sigma or alpha
 * that is not finite or negative, a prior that is not finite or below 2^-24, iters outside 0 .. 65536, a NULL or too small
 * workspace. */
int papof_super_resolve_tensor(papof_handle* h, int n_frames, int height, int width, int c, int scale,
                               const papof_tensor* frames, const papof_tensor* flow_fw, const papof_tensor* flow_bw,
                               int radius, int use_sigma, double sigma, int use_check, double alpha1, double alpha2,
                               double prior, int iters, const papof_tensor* out, const papof_tensor* coverage,
                               void* workspace, long long workspace_bytes, void* stream);

/* Bytes of the workspace papof_super_resolve_tensor is best given (stated there); -1 where that call refuses the sizes
 * (n_frames, height or width < 1, c outside 1 .. 4, scale outside 2 .. 4, iters outside 0 .. 65536, height * width >= 2^30). */
long long papof_sr_workspace(int n_frames, int height, int width, int c, int scale, int iters);

/* Dense block matching (match.hip): for every cell of a decimated frame A the integer displacement into frame B that
 * minimises a sum of absolute differences over a patch -- a start (papof_flow_batch_tensor_fb_init's init) for the solver
 * on motion that does not survive its pyramid.  It is brute force over one window: stride * search bounds the motion, the
 * displacements are whole cells, and repetitive texture is only caught by the forward-backward test of
 * papof_match_densify_tensor.  Everything is integer arithmetic, so the result is a pure function of the inputs.
 * frames: uint8, float32 or float64, (frame, row, column, channel), height x width x c, c in 1 .. 4, any non-negative
 * strides.  sequence != 0: n_pairs + 1 frames in `frames`, pair i = (frame i, frame i + 1), frames2 not read; else n_pairs
 * frames in each of frames and frames2, pair i = (frames[i], frames2[i]).
 * Quantise.  A uint8 sample is taken as it is; a float32 (widened exactly) or float64 sample x becomes
 *     rint(255.0 * x) clamped to 0 .. 255 (half to even), NaN -> 0.            Channels c .. 3 are 0.
 * Decimate.  stride S in {1, 2, 4, 8}; the grid is h = height / S, w = width / S (integer division: the trailing rows and
 * columns are dropped); per channel the coarse pixel (y, x) = (sum of the S x S samples from (S y, S x) + S * S / 2) / (S * S)
 * in integers.  Each frame is decimated once (k_match_prepare), one packed dword per coarse pixel in the workspace.
 * Cost.  With P = patch, for the coarse pixel p = (x, y) of A and the displacement d = (dx, dy), |dx|, |dy| <= search:
 *     cost(p, d) = sum over ox, oy in -P .. P and over the channels of
 *                      | A(clamp(y + oy, h), clamp(x + ox, w)) - B(clamp(y + oy + dy, h), clamp(x + ox + dx, w)) |
 *                  + penalty * (|dx| + |dy|)                                   clamp(v, n) = min(max(v, 0), n - 1)
 * d is admissible iff 0 <= x + dx < w and 0 <= y + dy < h (d = 0 always is).
 * Argmin.  The match is the admissible d with the smallest key (cost, dx * dx + dy * dy, dy, dx), compared
 * lexicographically: among equal costs the shortest, then the smallest dy, then the smallest dx.
 * patch in 1 .. 7, search in 1 .. 32, penalty in 0 .. 65535: a cost stays below 2^24, exact in float32.
 * Items: n_pairs forward (A the pair's first frame), then with both != 0 n_pairs backward (A the second, B the first).
 * disp: float32 / float64, (item, row, column, {dx, dy}) of h x w, holding S * d -- full-resolution pixels, exact integers;
 * cost: float32 / float64, (item, row, column, -) of h x w, the match's cost; strides positive (cost's stride[3] is not read).
 * workspace: device memory, 4-byte aligned, owned by the caller for the duration of the enqueued work;
 * papof_match_workspace gives its bytes.  Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the
 * null stream; k_match_prepare per frame tensor, then k_match: one block per 32 x 8 tile of cells and item) and returns
 * without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (frames2 in sequence mode aside) or data pointer, a
 * dtype other than those above, a negative stride or a zero stride of disp or cost, n_pairs < 1, stride not 1, 2, 4 or 8,
 * height or width < stride, height * width >= 2^30, c outside 1 .. 4, patch outside 1 .. 7, search outside 1 .. 32, penalty
 * outside 0 .. 65535, a NULL, misaligned or too small workspace. */
int papof_match_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2,
                       int height, int width, int c, int stride, int patch, int search, int penalty, int both,
                       const papof_tensor* disp, const papof_tensor* cost, void* workspace, long long workspace_bytes,
                       void* stream);

/* Bytes of papof_match_tensor's workspace: 4 (height / stride) (width / stride) per frame, n_pairs + 1 frames in sequence
 * mode and 2 n_pairs otherwise; -1 where that call refuses the sizes. */
long long papof_match_workspace(int n_pairs, int sequence, int height, int width, int stride);

/* Hierarchical block matching (match.hip): papof_match_tensor's search carried from a coarse level down, so that the reach
 * is stride * 2^(levels - 1) * search pixels plus the refinements, at a fraction of the flat search's candidates.  Integer
 * arithmetic throughout: the result is a pure function of the inputs (tests/_hmatch_ref.py restates it).  The frames,
 * sequence, c, patch, search, penalty, both, disp, cost and stream are papof_match_tensor's; levels L in 1 .. 4, refine r
 * in 1 .. 3.
 * Levels.  Level l (0 = finest) has the stride S_l = stride * 2^l and the grid h_l x w_l = height / S_l x width / S_l.
 * The frames of level l are the quantised frames decimated by S_l DIRECTLY, by papof_match_tensor's rule
 * (sum of the S_l x S_l samples + S_l * S_l / 2) / (S_l * S_l) -- not a decimation of level l - 1.  S_(L-1) <= 32, and the
 * frame holds at least one cell of the top level.
 * Top level L - 1.  papof_match_tensor's rule unchanged on its grid, with `search` and `penalty`: d_(L-1) in that level's cells.
 * Level l < L - 1, cell (x, y).  With the level above h' x w' and clamp(v, n) = min(max(v, 0), n - 1):
 *     parent           px = min(x >> 1, w' - 1), py = min(y >> 1, h' - 1)
 *     side neighbour   nx = clamp(px + (x odd ? +1 : -1), w'), ny = clamp(py + (y odd ? +1 : -1), h')
 *     predictors       2 * d_(l+1) at (px, py), (nx, py), (px, ny), (nx, ny), and the zero vector
 *     candidates       d = predictor + (ex, ey), |ex|, |ey| <= r
 * d is admissible iff 0 <= x + dx < w_l and 0 <= y + dy < h_l (d = 0 always is).  cost(p, d) is papof_match_tensor's on grid
 * l: the clamped-window sum of absolute differences over (2 patch + 1)^2 cells and the channels + penalty * (|dx| + |dy|).
 * d_l is the admissible candidate with the smallest key (cost, dx * dx + dy * dy, dy, dx), compared lexicographically; a
 * candidate that several predictors give counts once.
 * Result.  disp = stride * d_0 and cost = cost_0 on the h_0 x w_0 grid: the shapes, dtypes and meaning of
 * papof_match_tensor's outputs, so papof_match_densify_tensor takes them as they are.  With levels == 1 the call IS
 * papof_match_tensor (refine is checked and not used) and returns its bytes.
 * Bounds.  |d| <= 32 * 8 + 3 * 7 = 277 cells per component at every level and a cost stays below 15 * 15 * 4 * 255 +
 * 65535 * 554 < 2^26, so the key is held exactly in 26 + 18 + 10 + 10 bits.
 * When not to use it: a structure smaller than the top level's window (2 patch + 1 cells of stride S_(L-1)) is matched
 * there with the background around it and the lower levels only refine that; small objects that move far keep levels 1.
 * workspace: papof_match_hier_workspace's bytes, 4-byte aligned -- the packed frames of every level, then one packed
 * displacement dword per cell and item of every level above 0.  Enqueued on `stream` (k_match_prepare per level and frame
 * tensor, k_match on the top level, k_match_refine per lower level from the top down: one block per 32 x 8 tile of cells and
 * item) and returns without waiting.  The environment variable PAPOF_MATCH_STAGED=0, read per call, makes every tile of
 * k_match_refine read B through global addresses instead of its LDS window; the bytes are the same.
 * PAPOF_EINVAL, before anything is enqueued: what papof_match_tensor refuses, levels outside 1 .. 4, refine outside 1 .. 3,
 * stride * 2^(levels - 1) > 32, height or width < stride * 2^(levels - 1), a workspace below papof_match_hier_workspace. */
int papof_match_hier_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames, const papof_tensor* frames2,
                            int height, int width, int c, int stride, int levels, int patch, int search, int refine, int penalty,
                            int both, const papof_tensor* disp, const papof_tensor* cost, void* workspace,
                            long long workspace_bytes, void* stream);

/* Bytes of papof_match_hier_tensor's workspace: with F = n_pairs + 1 frames in sequence mode and 2 n_pairs otherwise,
 * 4 * (F * sum over l = 0 .. levels - 1 of h_l w_l + 2 n_pairs * sum over l = 1 .. levels - 1 of h_l w_l) -- with levels == 1
 * papof_match_workspace's; -1 where that call refuses the sizes. */
long long papof_match_hier_workspace(int n_pairs, int sequence, int height, int width, int stride, int levels);

/* Re-centred block search (match.hip): the hierarchical search says, tile by tile, where the flat search's window is
 * centred, so that a small structure that moves against a large pan -- blind spot of both: the flat search ends at stride *
 * search pixels, the hierarchy matches a structure smaller than its top window with the background around it -- is found.
 * Integer arithmetic throughout: the result is a pure function of the inputs (tests/_recentre_ref.py restates it).  The
 * arguments are papof_match_hier_tensor's, with levels L in 2 .. 4, and window in 1 .. 32.
 * Hierarchy.  papof_match_hier_tensor's rule unchanged, down to level 0: d_h(p) for every cell p of the finest grid h_0 x w_0.
 * Tile origin.  The finest grid is cut into tiles of 32 x 8 cells (32 along x) from (0, 0), the last ones clipped to the
 * grid.  The origin o = (o_x, o_y) of a tile and item is, per component, the lower median of d_h over the tile's n in-grid
 * cells: the value of rank (n - 1) / 2 (integer division, ranks from 0) in ascending order.  The tile size is part of the
 * rule, not of a kernel's launch.
 * Candidates of the cell p of a tile: o + (ex, ey), |ex|, |ey| <= window, and d_h(p) itself; a candidate that occurs twice
 * counts once.  d is admissible iff 0 <= x + dx < w_0 and 0 <= y + dy < h_0, papof_match_tensor's test; d_h(p) always is, by
 * the hierarchy's rule, so every cell has a match even where its whole window is inadmissible.
 * Cost and argmin.  papof_match_tensor's on grid 0: the clamped-window sum of absolute differences over (2 patch + 1)^2 cells
 * and the channels + penalty * (|dx| + |dy|); the match is the admissible candidate with the smallest key (cost, dx * dx +
 * dy * dy, dy, dx), compared lexicographically.
 * Result.  disp = stride * d and cost on the h_0 x w_0 grid, in papof_match_tensor's shapes and dtypes, so
 * papof_match_densify_tensor takes them as they are.  Items, `both` and `sequence` as in the hierarchical call.
 * Two properties follow.  (a) Every cell's key is <= the key of the hierarchical result at that cell: the candidates hold
 * d_h(p).  (b) On a tile whose origin is (0, 0), with window == search, a cell whose d_h lies within the window gets
 * papof_match_tensor's result at the finest stride.
 * Bounds.  |d| <= 277 + 32 = 309 cells per component, so dx * dx + dy * dy <= 190962 < 2^18 and d + 512 lies in 0 .. 1023; a
 * cost stays at or below 15 * 15 * 4 * 255 + 65535 * 618 = 40730130 < 2^26 (the hierarchical rule's bound with 618 for 554):
 * the key is still held exactly in 26 + 18 + 10 + 10 bits.
 * What it is not: the origin is one vector per tile, so a tile that a motion boundary halves serves one side (the other
 * keeps d_h or what the window happens to hold); a structure whose motion relative to its tile's origin exceeds window cells
 * is still lost; and the cost is the flat search's on grid 0, not comparable with a coarser level's.
 * workspace: papof_match_recentre_workspace's bytes, 4-byte aligned -- the hierarchical call's workspace, then one packed
 * displacement dword per level-0 cell and item (d_h), then one per tile and item (the origins).  Enqueued on `stream` (the
 * hierarchical call's chain with level 0 writing d_h, k_match_origin: one block per tile and item, k_match_recentre: one
 * block per tile and item) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: what papof_match_hier_tensor refuses, levels < 2, window outside 1 .. 32, a
 * workspace below papof_match_recentre_workspace. */
int papof_match_recentre_tensor(papof_handle* h, int n_pairs, int sequence, const papof_tensor* frames,
                                const papof_tensor* frames2, int height, int width, int c, int stride, int levels, int patch,
                                int search, int refine, int window, int penalty, int both, const papof_tensor* disp,
                                const papof_tensor* cost, void* workspace, long long workspace_bytes, void* stream);

/* Bytes of papof_match_recentre_tensor's workspace: papof_match_hier_workspace's + 4 * 2 n_pairs * (h_0 w_0 + ceil(h_0 / 8)
 * ceil(w_0 / 32)); -1 where the hierarchical call refuses the sizes or levels < 2. */
long long papof_match_recentre_workspace(int n_pairs, int sequence, int height, int width, int stride, int levels);

/* A full-resolution initial flow and its hole mask from matched displacements (k_match_densify, one lane per pixel).
 * disp, disp_rev: float32 / float64, (item, row, column, {dx, dy}) on the h x w grid of papof_match_tensor (h = height /
 * stride, w = width / stride), in full-resolution pixels: the field to densify and the field of the opposite direction.
 * cost: float32 / float64 (item, row, column, -), read only if max_cost >= 0 (else it may be NULL).
 * In fp64, for the cell p = (x, y) of item i:  dx = disp_x(p) / stride, dy = disp_y(p) / stride;  p is RELIABLE iff
 *     dx and dy are whole numbers, q = (x + dx, y + dy) lies on the grid (false for a NaN),
 *     |dx + disp_rev_x(q) / stride| <= tol and |dy + disp_rev_y(q) / stride| <= tol   (false for a NaN),
 *     and, if max_cost >= 0, cost(p) <= max_cost.
 * The pixel (X, Y) of the height x width frame belongs to the cell (min(X / stride, w - 1), min(Y / stride, h - 1)) -- the
 * dropped trailing rows and columns take their nearest cell.  flow: float64 (item, row, column, {vx, vy}), the cell's disp
 * where reliable and 0.0 elsewhere; mask: uint8 (item, row, column, -), 0 where reliable and 1 elsewhere: the hole mask
 * that papof_fill_holes_tensor takes.  Strides of flow and mask positive (the mask's stride[3] is not read).
 * Enqueued on `stream` and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (cost with max_cost < 0 aside) or data pointer, a
 * dtype other than those above, a negative stride or a zero stride of flow or mask, n < 1, stride not 1, 2, 4 or 8, height
 * or width < stride, height * width >= 2^30, tol outside 0 .. 64, max_cost NaN. */
int papof_match_densify_tensor(papof_handle* h, int n, int height, int width, int stride, const papof_tensor* disp,
                               const papof_tensor* disp_rev, const papof_tensor* cost, int tol, double max_cost,
                               const papof_tensor* flow, const papof_tensor* mask, void* stream);

/* Synthetic motion blur along the flows (a longer shutter for a video shot, rendered or retimed with a short one): every
 * frame becomes the weighted mean of the scene at n_samples times inside a shutter interval around it, the scene at an
 * in-between time being what papof_interp_tensor states -- one HIP kernel (blur.hip: k_motion_blur), one lane per output
 * pixel, the sums in registers.
 * frames: ONE video of n_frames >= 2 frames, uint8 (x / 255.0), float32 (widened exactly) or float64, (frame, row, column,
 * channel), any non-negative strides.  flow_fw[i], flow_bw[i]: the flows of the pair (i, i + 1) there and back, as
 * papof_flow_batch_tensor_fb returns them in sequence mode: float32 / float64, (pair, row, column, {vx, vy}), n_frames - 1
 * pairs, any non-negative strides.  occlusion: NULL, or that call's uint8 mask (pair, row, column, {fw, bw}), as
 * papof_interp_tensor takes it.  out: uint8, float32 or float64, (frame, row, column, channel), strides > 0.
 * offsets[k] = tau_k, the time of sample k relative to the frame, in frames: exactly 0, or 2^-20 <= |tau_k| <= 1 - 2^-20.
 * weights[k] = w_k: finite and >= 0, their sum > 0.  1 <= n_samples <= 64.  Both arrays are read before the call returns
 * (they travel as kernel arguments).
 * For frame f, pixel p and channel ch, in fp64 without fused multiply-adds, with acc = wsum = 0 and k ascending:
 *     w_k == 0:    the sample is skipped
 *     tau_k == 0:  S_k = I_f(p)                                  (uint8: x / 255.0)
 *     tau_k > 0:   S_k = the value papof_interp_tensor gives at p for the pair (f, f + 1) at t = tau_k, with flow_fw[f],
 *                  flow_bw[f] and occlusion[f]; skipped on the last frame
 *     tau_k < 0:   S_k = that value for the pair (f - 1, f) at t = 1.0 + tau_k, with flow_fw[f - 1], flow_bw[f - 1] and
 *                  occlusion[f - 1]; skipped on frame 0
 *     each kept sample:  acc = acc + w_k * S_k;  wsum = wsum + w_k
 *     out = acc / wsum, or I_f(p) if no sample was kept
 * stored as papof_interp_tensor stores: float64 as is, float32 with one round-to-nearest, uint8 = clamp(rint(255 * out), 0,
 * 255) with rint rounding half to even (NaN: 0).  The end frames therefore get a one-sided shutter.  It is the gather rule:
 * the flows are read at the output pixel, so at a motion boundary a sample reads the wrong flow, as papof_interp_tensor does.
 * Known answers: identical frames and zero flows return the frames (for uint8 the same bytes); with offsets that are all
 * >= 0 the last frame, and with offsets that are all <= 0 frame 0, is returned as it is (converted as stated).
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (occlusion aside) or data pointer, frames or an output
 * that are not uint8 / float32 / float64, flows that are not float32 / float64, a mask that is not uint8, a negative stride,
 * a zero stride of out, n_frames < 2, height, width or c < 1, n_samples outside 1 .. 64, offsets or weights NULL, an offset
 * that is not 0 and not of a magnitude in [2^-20, 1 - 2^-20] (a NaN included), a weight that is negative or not finite, a
 * sum of weights that is not > 0. */
int papof_motion_blur_tensor(papof_handle* h, int n_frames, const papof_tensor* frames, int height, int width, int c,
                             const papof_tensor* flow_fw, const papof_tensor* flow_bw, const papof_tensor* occlusion,
                             int n_samples, const double* offsets, const double* weights, const papof_tensor* out,
                             void* stream);

/* Video mosaics (mosaic.hip: k_mosaic): many frames, each through its own affine matrix, gathered into one output pixel and
 * combined there -- the panorama of a panning shot, its clean plate (the per-pixel temporal median: what moved is gone),
 * and the borders of a stabilized frame filled from the frames around it.  One kernel, one lane per output pixel, the
 * samples of a pixel held in registers or LDS: no full-canvas temporary per source, no atomics.
 * frames: n_frames frames of height x width x c (H, W, C), uint8 (x / 255.0), float32 (widened exactly) or float64, (frame,
 * row, column, channel), any non-negative strides.  masks: NULL, or uint8 (frame, row, column), any non-negative strides
 * (stride[3] is not read): nonzero = this pixel of the frame is left out.
 * There are n_out outputs of out_height x out_width (Hc, Wc), each with n_src = N source slots.  sources: DEVICE pointer
 * to n_out * N int32, contiguous (out, k): the frame of slot k, or a negative number for an empty slot; an index
 * >= n_frames is the caller's error (it is not checked here).  matrices: float32 (widened exactly) or float64, (out, k, row,
 * column), 2 x 3 each, any non-negative strides.
 * At output pixel (o, r, x), in fp64 without fused multiply-adds, everything papof_warp_affine_tensor states reused as it
 * stands, the slots are visited in the order k = 0 .. N - 1:
 *     s = sources[o, k];  s < 0: the slot is dead
 *     M = matrices[o, k];  X = (m00 * x + m01 * r) + m02;  Y = (m10 * x + m11 * r) + m12
 *     the slot is LIVE when (X, Y) lies in [0, W - 1] x [0, H - 1] (false for a NaN) and, with masks, the mask of frame s
 *     is 0 at every tap of the bilinear rule at (X, Y) whose weight is > 0 (a tap of weight 0 is not looked at)
 *     its sample, per channel, is frames[s] under the bilinear rule of papof_interp_tensor at (X, Y) (truncation toward
 *     zero, fraction clamped to [0, 1], neighbours clamped into the image, taps accumulated from 0.0 in (m, n) order)
 * n = the number of live slots; count (NULL, or uint8 (out, row, column), strides [0..2] > 0) receives n.  n = 0: every
 * channel is 0.  Otherwise, by mode:
 *     PAPOF_MOSAIC_FIRST   the sample of the live slot with the smallest k
 *     PAPOF_MOSAIC_MEAN    the live samples added from 0.0 in k order, divided by (double)n
 *     PAPOF_MOSAIC_MEDIAN  per channel, the live samples ordered by (value, k): a sorts before b when a < b, or when a is
 *                          not NaN and b is; samples that compare equal (-0.0 and +0.0 included) and NaNs among themselves
 *                          are ordered by k.  The result is the element at index (n - 1) / 2 (the lower median): the bits
 *                          of one sample, the same on every run.
 * out: uint8, float32 or float64, (out, row, column, channel), strides > 0, stored as papof_interp_tensor stores (uint8 =
 * clamp(rint(255 v), 0, 255), half to even, NaN -> 0).  out and count must not overlap the inputs.
 * A tile of output pixels drops a slot whose matrix sends the tile's corners to a box that misses the frame: every step of
 * X and Y is monotone in x and r under rounding, so this changes no byte.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting;
 * the handle's arena is not used.  PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (masks and count
 * aside), data pointer or sources, frames or out that are not uint8 / float32 / float64, matrices that are not float32 /
 * float64, masks or count that are not uint8, a negative stride, a zero stride of out or count along an axis in use,
 * n_frames, height, width, c, n_out, out_height or out_width < 1, n_src outside 1 .. PAPOF_MOSAIC_MAX_SOURCES, a mode that
 * is none of the three, PAPOF_MOSAIC_MEDIAN with n_src > PAPOF_MOSAIC_MAX_MEDIAN. */
enum { PAPOF_MOSAIC_FIRST = 0, PAPOF_MOSAIC_MEAN = 1, PAPOF_MOSAIC_MEDIAN = 2 };
enum { PAPOF_MOSAIC_MAX_SOURCES = 255, PAPOF_MOSAIC_MAX_MEDIAN = 64 };
int papof_mosaic_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                        const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width, const int* sources,
                        const papof_tensor* matrices, int mode, const papof_tensor* out, const papof_tensor* count,
                        void* stream);

/* Seamless mosaics: papof_mosaic_tensor with a gain per slot and a feathered mode (k_mosaic, the same kernel), and the
 * pairwise overlap statistics from which the gains are solved (k_mosaic_overlap; Brown and Lowe 2007, section 6).  Frames,
 * masks, sources, matrices and LIVENESS are exactly those of the call above -- its (X, Y), inside test, tap-wise mask rule
 * and sampler, its tile culling --; fp64 without fused multiply-adds, slots visited in the order k = 0 .. N - 1.
 *
 * The blend call.  gains: NULL (every gain is 1), or float32 (widened exactly) / float64 over (out, k), strides [0..1] >= 0
 * (0 broadcasts; strides [2..3] are not read).  The VALUE of a live slot is v = g * sample per channel, g = gains[o, k].
 * FIRST, MEAN and MEDIAN are the rules above applied to v -- the median orders the compensated values and returns the bits
 * of one g * sample; with gains NULL the three give the bytes of the call above (1.0 * x is x).  Gains are not inspected: a
 * NaN gain makes a NaN value, which the median orders last.
 *     PAPOF_MOSAIC_FEATHER  w = min(min(X, W1 - X), min(Y, H1 - Y)) + 1.0 with W1 = (double)(W - 1), H1 = (double)(H - 1):
 *                           >= 1 for a live slot, 1 on the frame's border.  num[ch] and den start at 0.0 and add w * v and
 *                           w in k order; out = num[ch] / den, 0 when no slot is live.
 * count as above.  PAPOF_EINVAL: the list above, with n_src <= PAPOF_MOSAIC_MAX_SOURCES for FEATHER too, a mode outside
 * 0 .. 3, gains that are not float32 / float64 or have a negative stride or NULL data.
 *
 * The overlap call.  sums, counts: DEVICE pointers to n_out * N * N int64 each, contiguous (out, i, j); the call zeroes them
 * on `stream` first.  It visits every output pixel with x % step == 0 and r % step == 0 and every live slot there:
 *     y = the channels' samples added from 0.0 in channel order, divided by (double)c; a NaN y takes the slot out at this pixel
 *     t = y / bound clamped to [0, 1];  q = (long long)rint(t * 16777216.0), half to even
 * and for every ordered pair (i, j) of slots left at the pixel, i = j included: counts[o, i, j] += 1, sums[o, i, j] += q_i.
 * So sums[o, i, j] / counts[o, i, j] / 2^24 * bound is the mean luminance of slot i where it overlaps slot j.  The sums are
 * integers -- any order of the additions gives the same bits --, and with q <= 2^24 and fewer than 2^31 pixels they stay
 * below 2^55.  PAPOF_EINVAL: the list above (out and count aside), n_src outside 1 .. PAPOF_MOSAIC_MAX_OVERLAP, step < 1, a
 * bound that is not finite and > 0, sums or counts NULL. */
enum { PAPOF_MOSAIC_FEATHER = 3 }; /* the blend call only */
enum { PAPOF_MOSAIC_MAX_OVERLAP = 64 };
int papof_mosaic_blend_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                              const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                              const int* sources, const papof_tensor* matrices, const papof_tensor* gains, int mode,
                              const papof_tensor* out, const papof_tensor* count, void* stream);
int papof_mosaic_overlap_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                const int* sources, const papof_tensor* matrices, int step, double bound, long long* sums,
                                long long* counts, void* stream);

/* The homography model: the calls above over 3 x 3 matrices, for a camera that rotates (a pan on a tripod or in a hand moves
 * the image by a homography, not by an affine map).  A parallel family: the affine calls are unchanged.
 *
 * PROJECTIVE SAMPLING (the rule of the warp, the mosaic and the overlap call below).  m: a 3 x 3 matrix, float32 (widened
 * exactly) or float64.  At output pixel (x, r), in fp64 without fused multiply-adds:
 *     D = (m20 * x + m21 * r) + m22;  Nx = (m00 * x + m01 * r) + m02;  Ny = (m10 * x + m11 * r) + m12
 *     X = Nx / D;  Y = Ny / D                      (two divisions, not a reciprocal and two products)
 *     live / inside iff D > 0 and 0 <= X <= W - 1 and 0 <= Y <= H - 1 (every comparison false for a NaN)
 * and from (X, Y) on everything is the affine call's rule: the taps, the tap-wise mask rule, the gains, the feather weight,
 * the modes, the count and the sampler.  A matrix whose last row is exactly (0, 0, 1) has D = 1.0, X = Nx and Y = Ny: the
 * projective calls on such matrices return the BYTES of the affine calls on their top two rows.
 *
 * papof_warp_projective_tensor (motion.hip: k_warp_projective): papof_warp_affine_tensor with matrices (frame, row, column),
 * 3 x 3; out is 0 and valid 0 where the pixel is not inside.  Arguments and PAPOF_EINVAL as there.
 *
 * papof_mosaic_projective_tensor (mosaic.hip: k_mosaic over ProjArgs): papof_mosaic_blend_tensor -- all four modes, gains
 * NULL or given -- with matrices (out, k, row, column), 3 x 3.  papof_mosaic_overlap_projective_tensor: the overlap call
 * likewise.  Arguments, limits (PAPOF_MOSAIC_MAX_SOURCES, _MAX_MEDIAN, _MAX_OVERLAP), PAPOF_MOSAIC_CULL and PAPOF_EINVAL as
 * there.  Tile culling, which changes no byte: with the min and max of D, Nx and Ny over the tile's four corners (each is
 * monotone in x and r under rounding, so these bound every pixel's when no corner value is NaN), a slot is dropped when an entry of its first two rows
 * is not finite, when no corner has D > 0, or when every corner has D > 0 and the interval
 * [min(Nx_min / D_min, Nx_min / D_max), max(Nx_max / D_min, Nx_max / D_max)], widened by a pixel, misses [0, W - 1] (the
 * same for Y and H); correctly rounded division is monotone in each operand, so the interval holds every pixel's computed
 * X.  A NaN corner value or quotient and a D of mixed sign prove nothing: the slot stays.  mosaic.hip has the proof.
 *
 * papof_homography_fit_tensor (motion.hip: k_homography_sums, k_homography_solve): papof_motion_fit_tensor's arguments
 * without `model`; motion: float64 (pair, row, column) = the 3 x 3 matrix M with m22 == 1.0 that sends (x, r, 1) of frame i to
 * frame i + 1 (divide by the third coordinate).  Valid pixels, cx, cy, s, x^, y^, X^, Y^ are that call's.  The unknowns are
 * h0 .. h7 of Hn = (h0 h1 h2; h3 h4 h5; h6 h7 1) in normalised coordinates; a valid pixel contributes the two rows
 *     (x^, y^, 1, 0, 0, 0, -x^ X^, -y^ X^ | X^)   and   (0, 0, 0, x^, y^, 1, -x^ Y^, -y^ Y^ | Y^),   each weighted by w:
 *     iteration 0:       w = c = 1
 *     iteration k >= 1:  with M the pair's matrix after iteration k - 1,
 *                        d = (m20 * x + m21 * r) + m22;  dn = d / ((m20 * cx + m21 * cy) + m22)
 *                        !(dn > PAPOF_HOMOGRAPHY_MIN_DEN): the pixel is left out of this iteration (it still counts in S23)
 *                        e_x = (x + u) - ((m00 * x + m01 * r) + m02) / d;  e_y = (r + v) - ((m10 * x + m11 * r) + m12) / d
 *                        e^2 = e_x * e_x + e_y * e_y;  c = 1 / (1 + e^2 / (scale * scale));  w = c / (dn * dn)
 * (1 / dn^2 turns the algebraic rows into the geometric error of the previous iterate).  With xx = x^ * x^, xy = x^ * y^,
 * yy = y^ * y^ and q = X^ * X^ + Y^ * Y^, every product grouped as written, the twenty-five sums are
 *     S0 = sum w xx          S1 = sum w xy          S2 = sum w yy          S3 = sum w x^           S4 = sum w y^          S5 = sum w
 *     S6 = sum w (xx * X^)   S7 = sum w (xy * X^)   S8 = sum w (yy * X^)   S9 = sum w (x^ * X^)    S10 = sum w (y^ * X^)  S11 = sum w X^
 *     S12 = sum w (xx * Y^)  S13 = sum w (xy * Y^)  S14 = sum w (yy * Y^)  S15 = sum w (x^ * Y^)   S16 = sum w (y^ * Y^)  S17 = sum w Y^
 *     S18 = sum w (xx * q)   S19 = sum w (xy * q)   S20 = sum w (yy * q)   S21 = sum w (x^ * q)    S22 = sum w (y^ * q)
 *     S23 = sum valid        S24 = sum c
 * added in papof_motion_fit_tensor's fixed order (no atomics: bitwise reproducible).  The normal equations
 *     (  S0   S1   S3    0    0    0   -S6   -S7 ) (h0)   (  S9  )
 *     (  S1   S2   S4    0    0    0   -S7   -S8 ) (h1)   (  S10 )
 *     (  S3   S4   S5    0    0    0   -S9  -S10 ) (h2)   (  S11 )
 *     (   0    0    0   S0   S1   S3  -S12  -S13 ) (h3) = (  S15 )
 *     (   0    0    0   S1   S2   S4  -S13  -S14 ) (h4)   (  S16 )
 *     (   0    0    0   S3   S4   S5  -S15  -S16 ) (h5)   (  S17 )
 *     ( -S6  -S7  -S9 -S12 -S13 -S15   S18   S19 ) (h6)   ( -S21 )
 *     ( -S7  -S8 -S10 -S13 -S14 -S16   S19   S20 ) (h7)   ( -S22 )
 * are solved by Gaussian elimination in natural order without row exchanges; a pivot not > 1e-12 * S5 fails the iteration.
 * Back to pixels, M = T^-1 Hn T with T = (1/s 0 -cx/s; 0 1/s -cy/s; 0 0 1), computed up to the factor s as
 *     A[i][0] = Hn[i][0];  A[i][1] = Hn[i][1];  A[i][2] = s * Hn[i][2] - (Hn[i][0] * cx + Hn[i][1] * cy)       (A = Hn (s T))
 *     B[0][j] = s * A[0][j] + cx * A[2][j];  B[1][j] = s * A[1][j] + cy * A[2][j];  B[2][j] = A[2][j]          (B = T^-1 A)
 *     M[i][j] = B[i][j] / B[2][2]
 * The iteration fails where S5 <= 0, at a pivot, where B[2][2] is not > 0, where an entry of M is not finite, or where the
 * denominator (m20 * x + m21 * r) + m22 is not > 0 at one of the four image corners.  Failure semantics, ok, the workspace
 * rules and PAPOF_EINVAL are papof_motion_fit_tensor's (a failed iteration 0: the 3 x 3 identity, ok = 0, no further
 * iterations).  support = S24 of the pair's last iteration / (H * W): comparable with the affine fit's.
 * papof_homography_workspace: 8 * n_pairs * (12 + 32 * ceil(width / 64) * ceil(height / 32)) bytes, or -1 as
 * papof_motion_workspace. */
#define PAPOF_HOMOGRAPHY_MIN_DEN 0.0625
long long papof_homography_workspace(int n_pairs, int height, int width);
int papof_homography_fit_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow,
                                const papof_tensor* occlusion, int n_iter, double scale, const papof_tensor* motion,
                                const papof_tensor* ok, const papof_tensor* support, void* workspace, long long workspace_bytes,
                                void* stream);
int papof_warp_projective_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                 const papof_tensor* matrices, const papof_tensor* out, const papof_tensor* valid, void* stream);
int papof_mosaic_projective_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                   const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                   const int* sources, const papof_tensor* matrices, const papof_tensor* gains, int mode,
                                   const papof_tensor* out, const papof_tensor* count, void* stream);
int papof_mosaic_overlap_projective_tensor(papof_handle* h, int n_frames, int height, int width, int c,
                                           const papof_tensor* frames, const papof_tensor* masks, int n_out, int n_src,
                                           int out_height, int out_width, const int* sources, const papof_tensor* matrices,
                                           int step, double bound, long long* sums, long long* counts, void* stream);

/* Wide panoramas: the mosaic and the overlap call on a canvas whose pixels are DIRECTIONS, not points of one plane -- a
 * cylinder or a sphere around a camera that rotates by more than a plane can hold.  A parallel family: the affine and the
 * projective calls are unchanged.
 *
 * RAY SAMPLING (the rule of the two calls below).  The canvas is given by two tables, float32 (widened exactly) or float64:
 * cols (column, {u, w}), out_width rows, and rows (row, {s, c}), out_height rows (strides: stride[0] between entries,
 * stride[1] between the two numbers of one).  m: a 3 x 3 matrix as above.  At output pixel (x, r), in fp64 without fused
 * multiply-adds:
 *     dx = u_x * c_r;  dy = s_r;  dz = w_x * c_r                                  (the pixel's ray)
 *     D = (m20 * dx + m21 * dy) + m22 * dz;  Nx = (m00 * dx + m01 * dy) + m02 * dz;  Ny = (m10 * dx + m11 * dy) + m12 * dz
 *     X = Nx / D;  Y = Ny / D                      (two divisions, not a reciprocal and two products)
 *     live / inside iff D > 0 and 0 <= X <= W - 1 and 0 <= Y <= H - 1 (every comparison false for a NaN)
 * and from (X, Y) on everything is the affine call's rule: the taps, the tap-wise mask rule, the gains, the feather weight,
 * the modes, the count and the sampler.  The device evaluates no sine: the tables are the caller's (a cylinder is cols =
 * (sin t_x, cos t_x), rows = (h_r, 1); a sphere is rows = (sin p_r, cos p_r)).  The plane's tables cols = (x, 1), rows = (r, 1)
 * give dx = x, dy = r, dz = 1.0 and m22 * 1.0 = m22: the ray calls on them return the BYTES of the projective calls.
 *
 * papof_mosaic_ray_tensor (mosaic.hip: k_mosaic over RayArgs): papof_mosaic_projective_tensor with the two tables after the
 * matrices.  papof_mosaic_overlap_ray_tensor: the overlap call likewise (the tables are indexed by the canvas pixel, every
 * step-th of them sampled).  Arguments, limits (PAPOF_MOSAIC_MAX_SOURCES, _MAX_MEDIAN, _MAX_OVERLAP), PAPOF_MOSAIC_CULL and
 * PAPOF_EINVAL as there; a table that is NULL, has no data, another dtype or a negative stride is PAPOF_EINVAL before any
 * launch.  Tile culling, which changes no byte: the block reduces u and w over the tile's columns and s and c over its rows to
 * their minima and maxima (a NaN entry makes them NaN); [dx_min, dx_max] and [dz_min, dz_max] are the min and max of the four
 * endpoint products, [dy_min, dy_max] = [s_min, s_max]; the bounds of D, Nx and Ny are their expressions evaluated with, per
 * term, the smaller (larger) of the two endpoint products m * d_min, m * d_max.  Every step is a correctly rounded monotone
 * operation, so these bound every pixel's value that is not NaN.  From there the projective rule: a slot is dropped when an
 * entry of its first two rows is not finite, when D_max <= 0, or when D_min > 0 and the interval [min(Nx_min / D_min, Nx_min /
 * D_max), max(Nx_max / D_min, Nx_max / D_max)], widened by a pixel, misses [0, W - 1] (the same for Y and H).  A NaN bound or
 * quotient and a D of mixed sign prove nothing: the slot stays.  mosaic.hip has the proof. */
int papof_mosaic_ray_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                            const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width, const int* sources,
                            const papof_tensor* matrices, const papof_tensor* cols, const papof_tensor* rows,
                            const papof_tensor* gains, int mode, const papof_tensor* out, const papof_tensor* count,
                            void* stream);
int papof_mosaic_overlap_ray_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                                    const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                                    const int* sources, const papof_tensor* matrices, const papof_tensor* cols,
                                    const papof_tensor* rows, int step, double bound, long long* sums, long long* counts,
                                    void* stream);

/* Bundle adjustment for a camera that rotates: the device half.  A parallel family: no call above changes.
 *
 * A LINK l is an ordered frame pair (i, j) with a flow field from frame i to frame j.  The unknowns of the adjustment are one
 * rotation per frame and one focal length; the host (tensors.py: bundle_adjust) owns them, and per evaluation hands the device,
 * per link, the row rot[l] = (R00 R01 R02 R10 R11 R12 R20 R21 R22 f) of ten float64 with R = R_j R_i^T.  The device never
 * knows how many frames there are.
 *
 * papof_bundle_sums_tensor (bundle.hip: k_bundle_sums, k_bundle_reduce): flow float32 (widened exactly) / float64 (link, row,
 * column, {vx, vy}), any strides >= 0; occlusion NULL or uint8 (link, row, column, .): a pixel whose byte is not 0 is left
 * out; rotations float64 (link, k), k = 0 .. 9, strides >= 0; sums float64 (link, k), k = 0 .. 19, strides > 0.  The SAMPLED
 * pixels are (x, r) = (step * a, step * b), a = 0 .. Ws - 1, b = 0 .. Hs - 1, Ws = (width - 1) / step + 1, Hs = (height - 1)
 * / step + 1 (integer division).  With (cx, cy) = ((width - 1) / 2, (height - 1) / 2), in fp64 without fused multiply-adds
 * and grouped as written, at a sampled pixel:
 *     X = x + u;  Y = r + v                                                       (the observed point)
 *     valid iff 0 <= X <= width - 1 and 0 <= Y <= height - 1 (false for a NaN or an infinity) and the occlusion byte is 0
 *     px = (x - cx) / f;  py = (r - cy) / f
 *     qx = (R00 * px + R01 * py) + R02;  qy = (R10 * px + R11 * py) + R12;  qz = (R20 * px + R21 * py) + R22
 *     valid only if qz > PAPOF_HOMOGRAPHY_MIN_DEN (false for a NaN)
 *     gx = qx / qz;  gy = qy / qz;  fgx = f * gx;  fgy = f * gy
 *     e_x = X - (fgx + cx);  e_y = Y - (fgy + cy)                                 (observed - predicted)
 *     e2 = e_x * e_x + e_y * e_y;  w = 1 / (1 + e2 / (scale * scale))             (the Cauchy weight)
 * The Jacobian of the predicted point in four parameters -- a small rotation a applied to q as dq = a x q, and f (through
 * p as well: d(fgx + cx)/df = gx + (R02 - gx R22) / qz) --:
 *     Jx = ( -(fgx * gy),   f + fgx * gx,   -fgy,   gx + (R02 - gx * R22) / qz )
 *     Jy = ( -(f + fgy * gy),   fgx * gy,    fgx,   gy + (R12 - gy * R22) / qz )
 * The twenty sums over the link's valid sampled pixels, with (a, b) running over the upper triangle in the order (0,0) (0,1)
 * (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3):
 *     S0 .. S9    = sum w * (Jx[a] * Jx[b] + Jy[a] * Jy[b])                        (sum w J^T J)
 *     S10 .. S13  = sum w * (Jx[a] * e_x + Jy[a] * e_y),  a = 0 .. 3               (sum w J^T e)
 *     S14 = sum w * e2      S15 = sum w      S16 = sum 1 (the valid pixels)      S17 = sum e2      S18 = S19 = 0 (spare)
 * Frame j's update omega_j enters a link as a = omega_j and frame i's as a = -R omega_i; the Gauss-Newton step solves
 * (sum w J^T J) d = sum w J^T e.  Fixed order, no atomics, bitwise reproducible: papof_motion_fit_tensor's order over 64 x 32
 * tiles of SAMPLED pixels (a lane: sampled column a, sampled rows threadIdx.y + 4 k in increasing order; the wave's shuffle
 * tree 32 .. 1; the four waves in wave order; blockIdx.x the tile in row-major order, blockIdx.y the link, split at 65535);
 * then one wave per link adds the tiles' rows l, l + 64, ... per lane in increasing order and the lanes by the same tree.
 * A link's sums do not depend on the other links of the call.  Nothing waits; the sums are on `stream` when it is reached.
 * PAPOF_EINVAL before any launch: a NULL handle, n_links / height / width / step < 1, a scale that is not finite and > 0, a
 * descriptor that is NULL, has no data, another dtype or a negative stride (sums: a stride that is not > 0), a workspace that
 * is NULL or smaller than
 * papof_bundle_workspace: 8 * n_links * 32 * ceil(Ws / 64) * ceil(Hs / 32) bytes, or -1 where an argument is < 1 or a link
 * has more than 2^31 - 1 tiles. */
long long papof_bundle_workspace(int n_links, int height, int width, int step);
int papof_bundle_sums_tensor(papof_handle* h, int n_links, int height, int width, int step, const papof_tensor* flow,
                             const papof_tensor* occlusion, const papof_tensor* rotations, double scale,
                             const papof_tensor* sums, void* workspace, long long workspace_bytes, void* stream);

/* Spatially varying stabilization (SteadyFlow, Liu, Yuan, Tan, Sun, CVPR 2014; MeshFlow, Liu, Tan, Yuan, Sun, Zeng, ECCV
 * 2016): the robust motion of a flow field at the vertices of a coarse mesh, and the affine warp plus a displacement mesh.
 * A parallel family: no call above changes.
 *
 * THE MESH.  grid_rows = GH and grid_cols = GW cells on frames of height = H rows and width = W columns, 1 <= GH <= min(H - 1,
 * PAPOF_MESH_MAX_CELLS) and 1 <= GW <= min(W - 1, PAPOF_MESH_MAX_CELLS).  Vertex (i, j), i = 0 .. GH, j = 0 .. GW, sits at
 *     px = (j * (W - 1)) / GW;  py = (i * (H - 1)) / GH          (fp64: the product of two exact integers, then one division)
 *
 * papof_mesh_motion_tensor (mesh.hip: k_mesh_median, k_mesh_spatial): the lower median, per component, of the flow's residual
 * against the pair's global motion over a window around every vertex.
 * flow: float32 (widened exactly) or float64 (pair, row, column, {vx, vy}), any non-negative strides.  occlusion: NULL, or
 * uint8 (pair, row, column), any non-negative strides (stride[3] ignored): a pixel whose byte is not 0 is left out.  motion:
 * NULL (every pair: the identity, exactly the matrix (1 0 0; 0 1 0)), or float64 (pair, row, column), 2 x 3, any non-negative
 * strides: M = (m00 m01 m02; m10 m11 m12), papof_motion_fit_tensor's.
 * WINDOW of vertex (i, j): the pixels (x, r) within one cell width and one cell height of the vertex, clipped to the image, in
 * integers:
 *     x_lo = max(0, ceil((j - 1) (W - 1) / GW));  x_hi = min(W - 1, floor((j + 1) (W - 1) / GW));  r_lo, r_hi likewise with i, H, GH
 * LATTICE: with Lx = floor(2 (W - 1) / GW) and Ly = floor(2 (H - 1) / GH), step is the smallest integer s >= 1 with
 * (floor(Lx / s) + 1) * (floor(Ly / s) + 1) <= 1024 -- no window, clipped or not, then holds more than 1024 lattice points.
 * The SAMPLES of a window are its pixels with x % step == 0 and r % step == 0, in row-major order (r outer, x inner).
 * At a sample, in fp64 without fused multiply-adds and grouped as written, with (u, v) the flow there:
 *     valid iff 0 <= x + u <= W - 1 and 0 <= r + v <= H - 1 (false where u or v is NaN or infinite), the occlusion byte is 0,
 *               and neither rx nor ry below is a NaN (one can be only through a matrix that is not finite)
 *     rx = u - (((m00 * x + m01 * r) + m02) - x);  ry = v - (((m10 * x + m11 * r) + m12) - r)          (the residual)
 * SELECTION, per component separately: n = the number of valid samples (the same for both components); the n residuals are
 * ordered by their bit patterns as signed numbers -- numerically, with -0 before +0 -- and by sample order among equal bit
 * patterns, and the one of rank (n - 1) / 2 (integer division, ranks from 0: the LOWER median) is taken: the result is the
 * bits of one sample (of two different samples for x and y, in general).  n = 0: (0, 0).  support(i, j) = n; the vertex is
 * VALID iff n >= min_support.
 * SPATIAL PASS (MeshFlow's second filter), spatial != 0: the residual of vertex (i, j) is, per component, the lower median --
 * the same order and rank -- of the window medians of the VALID vertices among (i + di, j + dj), di, dj = -1 .. 1 in row-major
 * order, itself included, inside the mesh; (0, 0) where none is valid, so that the vertex follows the global motion.
 * spatial == 0: the vertex's own window median where it is valid, else (0, 0).
 * OUTPUT: residuals(i, j) = (Rx, Ry) as above; vertices(i, j) = (Rx + gx, Ry + gy) with the global motion at the vertex
 *     gx = ((m00 * px + m01 * py) + m02) - px;  gy = ((m10 * px + m11 * py) + m12) - py
 * Subtracting the global motion first keeps the median of a clipped border window unbiased under rotation and zoom; on an
 * exactly affine flow every residual is zero to rounding.
 * vertices, residuals: float64 (pair, vertex row, vertex column, {x, y}), strides > 0.  support: n_pairs * (GH + 1) * (GW + 1)
 * int32, contiguous (pair, vertex row, vertex column), device memory.  workspace: device memory of at least
 * papof_mesh_workspace(n_pairs, grid_rows, grid_cols) = 16 * n_pairs * (GH + 1) * (GW + 1) bytes (the window medians between
 * the two kernels; -1 for an argument < 1 or a grid beyond PAPOF_MESH_MAX_CELLS), 8-byte aligned, the caller's, used by
 * nothing else until the work enqueued here has run.  No atomics: the results are bitwise reproducible, and a pair's rows are
 * the same alone and in a batch.  Enqueued on `stream` and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (occlusion and motion aside), data pointer or support,
 * a flow that is not float32 / float64, a mask that is not uint8, a motion, vertices or residuals that is not float64, a
 * negative stride, a zero stride of an output, a grid outside the bounds above, min_support < 1, n_pairs, height or width
 * < 1, a NULL workspace or workspace_bytes below papof_mesh_workspace's value.
 *
 * papof_warp_mesh_tensor (mesh.hip: k_warp_mesh): papof_warp_affine_tensor with a displacement added to the sampling point,
 * interpolated bilinearly from the frame's table mesh: float64 (frame, vertex row, vertex column, {dx, dy}), any non-negative
 * strides.  At output pixel (x, r) of frame i, with M = matrices[i], D = mesh[i], in fp64 without fused multiply-adds and
 * grouped as written:
 *     X0 = (m00 * x + m01 * r) + m02;  Y0 = (m10 * x + m11 * r) + m12                 (papof_warp_affine_tensor's point)
 *     gx = (X0 * GW) / (W - 1);  gx = gx < 0 ? 0 : (gx > GW ? GW : gx);  gy likewise with Y0, GH, H    (a NaN stays a NaN)
 *     j = gx >= 0 ? min((int)gx, GW - 1) : 0;  fx = gx - j;  i likewise;  fy = gy - i   (truncation; a NaN takes cell 0)
 *     dx = dy = 0;  for m = 0, 1: for n = 0, 1:  w = |(1 - m) - fx| * |(1 - n) - fy|;
 *                                                dx += D(i + n, j + m).dx * w;  dy += D(i + n, j + m).dy * w
 *     X = X0 + dx;  Y = Y0 + dy
 * -- the weights and the (m, n) order of the sampler's taps.  Inside [0, W - 1] x [0, H - 1] (false for a NaN, which a NaN
 * in one of the cell's four table entries gives) the frame is sampled at (X, Y) and stored as papof_warp_affine_tensor does,
 * and valid = 1; outside, out = 0 and valid = 0.  A table whose entries are all +0.0 gives the BYTES of
 * papof_warp_affine_tensor.  The displacement is looked up at the sampling point X0, not at the moved vertex: this is the
 * backward approximation of MeshFlow's forward mesh render, and differs from it at second order in the displacement's
 * gradient.  Arguments otherwise and PAPOF_EINVAL as papof_warp_affine_tensor's, and a mesh that is NULL, has no data, is not
 * float64 or has a negative stride, or a grid outside the bounds above. */
#define PAPOF_MESH_MAX_CELLS 64
long long papof_mesh_workspace(int n_pairs, int grid_rows, int grid_cols);
int papof_mesh_motion_tensor(papof_handle* h, int n_pairs, int height, int width, const papof_tensor* flow,
                             const papof_tensor* occlusion, const papof_tensor* motion, int grid_rows, int grid_cols,
                             int min_support, int spatial, const papof_tensor* vertices, const papof_tensor* residuals,
                             int* support, void* workspace, long long workspace_bytes, void* stream);
int papof_warp_mesh_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                           const papof_tensor* matrices, const papof_tensor* mesh, int grid_rows, int grid_cols,
                           const papof_tensor* out, const papof_tensor* valid, void* stream);

/* Full-frame mesh stabilization: the mosaic under the mesh rule (mosaic.hip: k_mosaic over MeshMosaicArgs, behind
 * k_mesh_bounds) -- papof_mosaic_blend_tensor with a displacement table per SLOT, so that the frames around a mesh-stabilized
 * frame fill its borders registered as the mesh registers them.  A parallel call: no call above changes.
 * Arguments: the blend call's, and
 *     mesh: float64 (slot, vertex row, vertex column, {dx, dy}), any non-negative strides, slot = o * n_src + k (a descriptor
 *           has four strides: the (out, k) pair is one axis); n_out * n_src tables of (GH + 1) x (GW + 1) vertices
 *     grid_rows = GH, grid_cols = GW: THE MESH's bounds above against the FRAMES' height = H and width = W -- the table is
 *           looked up in the coordinates of the source frame
 *     workspace: device memory of at least papof_mosaic_mesh_workspace(n_out, n_src) = 32 * n_out * n_src bytes (four doubles
 *           per slot: the extremes of its table; -1 for n_out < 1 or n_src outside 1 .. PAPOF_MOSAIC_MAX_SOURCES), 8-byte
 *           aligned, the caller's, used by nothing else until the work enqueued here has run
 * At output pixel (x, r) of output o and slot k with s = sources[o, k] >= 0, M = matrices[o, k], D = mesh[o * n_src + k], in
 * fp64 without fused multiply-adds and grouped as written:
 *     X0 = (m00 * x + m01 * r) + m02;  Y0 = (m10 * x + m11 * r) + m12                          (papof_mosaic_tensor's point)
 *     (dx, dy): word for word the rule of papof_warp_mesh_tensor above at (X0, Y0) with the table D -- gx, gy and their clamp,
 *               the truncation to the cell (j, i), fx, fy, the four weights w = |(1 - m) - fx| * |(1 - n) - fy| and the sums
 *               dx += D(i + n, j + m).dx * w, dy likewise, from 0 in (m, n) order
 *     X = X0 + dx;  Y = Y0 + dy
 * The slot is LIVE when (X, Y) lies in [0, W - 1] x [0, H - 1] (false for a NaN, which a NaN in one of the cell's four entries
 * gives) and, with masks, the mask of frame s is 0 at every tap of the bilinear rule at (X, Y) whose weight is > 0.  Its
 * sample is frames[s] under the bilinear rule at (X, Y); PAPOF_MOSAIC_FEATHER's weight is taken at (X, Y).  Everything behind
 * the point is the blend call's: the gains, the four modes, count, the limits PAPOF_MOSAIC_MAX_SOURCES and _MAX_MEDIAN.
 *     INVARIANT A.  With every table entry +0.0 (dx = dy = +0.0 then, and X0 + 0.0 orders and samples as X0 does) the call
 *     returns the BYTES of papof_mosaic_blend_tensor: in all four modes, with and without gains, masks and count.
 *     INVARIANT B.  With n_src = 1, sources[o] = o, a canvas of the frames' size and PAPOF_MOSAIC_FIRST, out is
 *     papof_warp_mesh_tensor's out byte for byte (matrices[o, 0] and mesh[o] that call's), and count is its valid.
 * Culling: the corner box of papof_mosaic_tensor alone would be wrong here -- a table can carry a source into a tile that its
 * matrix misses.  k_mesh_bounds, ahead of k_mosaic on the stream, reduces every slot's table to the extremes of its dx and of
 * its dy (a NaN entry makes them NaN), and a tile drops a slot only when its corner box WIDENED by the bound
 * ((l + l) + l) + l <= d <= ((u + u) + u) + u, l = min(lo, 0), u = max(hi, 0) -- the four-term sum of the rule above at its
 * extreme terms -- misses the frame (mosaic.hip has the proof that this changes no byte); a NaN bound keeps the slot, a matrix
 * entry that is not finite drops it as before.  The same bound lets a pixel skip a slot before it reads the table.
 * PAPOF_MOSAIC_CULL=0 skips the reduction, the bounds' use and both tests.  The overlap statistics have no mesh twin.
 * Enqueued on `stream` and returns without waiting; bitwise reproducible, an output the same alone and in a batch.
 * PAPOF_EINVAL, before anything is enqueued: papof_mosaic_blend_tensor's list, a mesh that is NULL, has no data, is not float64
 * or has a negative stride, a grid outside the bounds above, a NULL workspace or workspace_bytes below
 * papof_mosaic_mesh_workspace's value. */
long long papof_mosaic_mesh_workspace(int n_out, int n_src);
int papof_mosaic_mesh_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                             const papof_tensor* masks, int n_out, int n_src, int out_height, int out_width,
                             const int* sources, const papof_tensor* matrices, const papof_tensor* mesh, int grid_rows,
                             int grid_cols, const papof_tensor* gains, int mode, const papof_tensor* out,
                             const papof_tensor* count, void* workspace, long long workspace_bytes, void* stream);

/* Dirt and dropout removal, 1 of 2 (restore.hip: k_defect_detect): the detector of defects that live in ONE frame of a video
 * of n_frames = T >= 3 frames -- film dirt and sparkle, dropouts, transmission errors, a bird that crosses one frame --,
 * Kokaram's spike detection index in its range form, one lane per pixel: a pixel is flagged when, in some channel, it lies
 * outside the range of the two points it maps to in two other frames by more than `threshold`.  The masks feed
 * papof_mask_dilate_tensor, papof_fill_holes_tensor (the flows under them) and papof_propagate_tensor.  A parallel call: no
 * call above changes.
 * frames, flow_fw, flow_bw: as papof_temporal_filter_tensor takes them -- frames uint8 (x / 255.0), float32 (widened exactly)
 * or float64, (frame, row, column, channel), any non-negative strides, c = C channels, 1 <= C <= 4; the T - 1 pairs' flows
 * float32 (widened exactly) or float64, (pair, row, column, {vx, vy}), any non-negative strides, pair t from frame t to
 * frame t + 1 (flow_fw[t]) and back (flow_bw[t]).
 * mask: uint8 (frame, row, column), strides [0..2] > 0 (stride[3] ignored): 1 a defect, 0 not.  score: NULL, or float32 (one
 * round-to-nearest) / float64, (frame, row, column), strides [0..2] > 0.  support: NULL, or uint8 (frame, row, column),
 * strides [0..2] > 0.  None of them may overlap an input.
 * threshold: finite, >= 0, in the frames' [0, 1] units; use_check != 0: the consistency test with alpha1, alpha2 (finite,
 * >= 0).  For the pixel p = (x, r) of frame t, in fp64 without fused multiply-adds:
 *
 * references: the frames t + o1 and t + o2, (o1, o2) = (-1, +1) for 0 < t < T - 1, (+1, +2) for t = 0, (-1, -2) for t = T - 1
 * hops:       each reference is reached from (X, Y) = (x, r) hop by hop exactly as papof_temporal_filter_tensor reaches it: a
 *             forward hop from frame f to f + 1 through flow_fw[f] checked with flow_bw[f], a backward hop from f to f - 1
 *             through flow_bw[f - 1] checked with flow_fw[f - 1]; alive &= inside [0, W - 1] x [0, H - 1], and with the check
 *             alive &= (u + bu)^2 + (v + bv)^2 <= a1 * ((u*u + v*v) + (bu*bu + bv*bv)) + a2  (NaN -> not alive).  Inside the
 *             video the two references are two chains of one hop; at an end frame they are the first and the second hop of
 *             ONE chain, which stays dead once it died: reference 2 is then never alive without reference 1.
 * support   = the number of references alive (0 .. 2)
 * support < 2:  score = 0.0, mask = 0 -- the pixel is not judged
 * otherwise:    c_k = frame[t](r, x, k);  g1_k, g2_k = frame[t + o1], frame[t + o2] sampled at their landing points (sampler.h
 *               taps);  s = 0.0;  for k = 0 .. C - 1:
 *                   lo = g2_k < g1_k ? g2_k : g1_k;   hi = g2_k > g1_k ? g2_k : g1_k
 *                   a = c_k - hi;   b = lo - c_k;   d = b > a ? b : a;   s = d > s ? d : s
 *               (every comparison is false for a NaN: a NaN never raises s -- a NaN c_k or g1_k silences channel k; a NaN g2_k
 *               leaves lo = hi = g1_k, a range of one point)
 *               score = s;  mask = s > threshold
 *
 * A centre between its two references scores 0.  The samplers are papof_temporal_filter_tensor's.  What the detector is
 * not: a defect that persists over frames (a line scratch, a sensor pixel under a static camera) agrees with its references
 * and is not found; a small object that outruns the flow (a ball, rain) is found; a defect of less than the threshold stays;
 * the end frames, whose references lie on one side, are weaker.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * No device memory besides the tensors is used; no atomics; bitwise reproducible.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (score and support aside) or data pointer, frames that
 * are not uint8 / float32 / float64, flows or a score that are not float32 / float64, a mask or support that is not uint8, a
 * negative stride, a zero stride of mask, score or support along an axis in use, n_frames < 3, height or width < 1, c
 * outside 1 .. 4, a threshold that is not finite or negative, an alpha that is not finite or negative. */
int papof_defect_detect_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                               const papof_tensor* flow_fw, const papof_tensor* flow_bw, double threshold, int use_check,
                               double alpha1, double alpha2, const papof_tensor* mask, const papof_tensor* score,
                               const papof_tensor* support, void* stream);

/* Dirt and dropout removal, 2 of 2 (restore.hip: k_mask_dilate): binary dilation of n_frames masks of height x width by a
 * square of side 2 * radius + 1 -- the margin that the completion calls ask for around a mask, because a defect's damage to
 * the flows reaches beyond it.
 * mask: uint8 (frame, row, column), any non-negative strides (stride[3] ignored); nonzero is set.  out: uint8 (frame, row,
 * column), strides [0..2] > 0; out must not overlap mask.  radius: 0 .. 32.
 *
 * out(t, r, x) = 1 where mask(t, r', x') != 0 for some max(r - radius, 0) <= r' <= min(r + radius, height - 1) and
 *                max(x - radius, 0) <= x' <= min(x + radius, width - 1); 0 otherwise
 *
 * (radius 0: the mask as 0 / 1.)  Enqueued on `stream` and returns without waiting; no device memory besides the tensors.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor or data pointer, a mask or out that is not uint8, a
 * negative stride, a zero stride of out along an axis in use, n_frames, height or width < 1, radius outside 0 .. 32, or an
 * out that starts where mask does. */
int papof_mask_dilate_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* mask, int radius,
                             const papof_tensor* out, void* stream);

/* Motion-compensated deinterlacing (deinterlace.hip: k_deinterlace): n_fields = T >= 4 fields of field_height = Hf rows become T
 * full frames of 2 Hf rows, one per field (double rate).  Frame t keeps its own field's lines; the lines it lacks have the
 * parity of fields t - 1 and t + 1, whose flows -- two fields of one parity share a sampling lattice -- are the solver's on the
 * fields themselves, and are the frame in between those two at time 0.5: papof_interp_tensor's gather rule on the field
 * lattice, protected per pixel by the phase of the landing rows and by the agreement of the two samples, over a four-tap cubic
 * of the own field.  A parallel call: no call above changes.
 * fields: uint8 (x / 255.0), float32 (widened exactly) or float64, (field, row, column, channel), any non-negative strides,
 * c = C channels, 1 <= C <= 4.  Field k holds the rows of parity p_k = (k + first) & 1 of frame k; first is 0 or 1.
 * flow_fw, flow_bw: the T - 2 pairs' flows, float32 (widened exactly) or float64, (pair, row, column, {vx, vy}), any
 * non-negative strides, in FIELD coordinates (rows of Hf): pair k runs from field k to field k + 2 (flow_fw[k]) and back from
 * field k + 2 to field k (flow_bw[k]).  mode 0 reads no flows: both may be NULL.
 * video: uint8 / float32 / float64, (frame, row, column, channel) with 2 Hf rows, strides [0..3] > 0; it must not overlap
 * fields.  confidence: NULL, or float32 (one round-to-nearest) / float64, (frame, row, column) with Hf rows, strides [0..2] >
 * 0: q of each made pixel.  sigma: finite, > 0, in the fields' [0, 1] units.
 * For the column x and the field row j of frame t, p = p_t, pm = 1 - p, in fp64 in the stated order without fused multiply-adds;
 * load is the field's value as fp64, store papof_interp_tensor's (float64 as is, float32 with one round-to-nearest, uint8 =
 * clamp(rint(255 v), 0, 255), half to even, NaN -> 0), sample the bilinear sampler of papof_interp_tensor on an Hf x W field:
 *
 * kept line:  video[t](2 j + p, x, k) = store(load(field[t](j, x, k)))  -- uint8 to uint8: the input's bytes
 * made line:  video[t](2 j + pm, x, k) = store(out_k), confidence[t](j, x) = q, with
 *   spatial:  the own field's rows at frame distance -1, +1, -3, +3 of the made line, indices clamped into [0, Hf - 1]:
 *             a1, b1, a3, b3 = field[t] rows j, j + 1, j - 1, j + 2 for pm = 1 and rows j - 1, j, j - 2, j + 1 for pm = 0
 *             s_k = (9.0 * (a1_k + b1_k) - (a3_k + b3_k)) * 0.0625           (no clamp)
 *   mode 0:   out_k = s_k, q = 0 (the bob)
 *   temporal, 1 <= t <= T - 2:  (u, v) = flow_fw[t - 1](j, x), (bu, bv) = flow_bw[t - 1](j, x); the landing points of
 *             papof_interp_tensor at time 0.5 on the field lattice,
 *                 (X0, Y0) = (x + (0.25 * bu - 0.25 * u), j + (0.25 * bv - 0.25 * v)) in field t - 1
 *                 (X1, Y1) = (x + (0.25 * u - 0.25 * bu), j + (0.25 * v - 0.25 * bv)) in field t + 1
 *             in_i = 0 <= X_i <= W - 1 and 0 <= Y_i <= Hf - 1 (false for a NaN)
 *   temporal, t = 0:      one point, (X1, Y1) = (x + 0.5 * u, j + 0.5 * v) in field 1 with (u, v) = flow_fw[1](j, x); in0 = false
 *   temporal, t = T - 1:  one point, (X0, Y0) = (x + 0.5 * bu, j + 0.5 * bv) in field T - 2 with (bu, bv) = flow_bw[T - 4](j, x);
 *             in1 = false
 *   phase:    c_i = in_i ? 1.0 - 2.0 * |Y_i - rint(Y_i)| : 0.0  (rint: half to even) -- a sample on a field line counts fully, one
 *             halfway between two lines, which carries no detail, does not count
 *   samples:  g0_k, g1_k = field[t - 1], field[t + 1] sampled at (X0, Y0), (X1, Y1), each only where c_i > 0
 *   c0 > 0 and c1 > 0:   m_k = (c0 * g0_k + c1 * g1_k) / (c0 + c1)
 *                        D = 0.0; for k = 0 .. C - 1: d = g0_k - g1_k; D = D + d * d
 *                        q = (c1 > c0 ? c1 : c0) / (1.0 + (D / C) / (sigma * sigma))
 *   only c_i > 0:        m_k = gi_k, q = 0.5 * c_i
 *   neither:             q = 0.0
 *   blend:    out_k = s_k where q == 0 -- every NaN or infinite flow and every point out of the image: a NaN never reaches the
 *             output through a zero weight --, else out_k = (1.0 - q) * s_k + q * m_k
 *
 * A static scene with zero flows has c0 = c1 = 1, D = 0, q = 1 and out_k = 0 * s_k + g0_k: the interior frames are the
 * progressive video exactly.  What it is not: at the critical velocity (an odd number of frame rows per field) the
 * neighbouring fields hold the current field's lines, c = 0 and the output is mode 0's; the end frames, with one neighbour
 * and q <= 0.5, are weaker; the flows assume motion linear over two field periods; telecined film is not its case
 * (papof_field_metrics_tensor and papof_weave_fields_tensor below find and weave the fields of one film frame); chroma
 * subsampling is papof_ycc_to_rgb_tensor's business, in front of this call.
 * One lane writes both rows 2 j and 2 j + 1 of its column: every output element is written once.  Enqueued on `stream` (the
 * caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.  No device memory besides
 * the tensors is used; no atomics; bitwise reproducible.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (confidence aside, and the flows in mode 0) or data
 * pointer, fields or a video that are not uint8 / float32 / float64, flows or a confidence that are not float32 / float64, a
 * negative stride, a zero stride of video or confidence along an axis in use, n_fields < 4, field_height < 1 or > 2^30 - 1,
 * width < 1, c outside 1 .. 4, first or mode outside {0, 1}, a sigma that is not finite or not > 0, or a video that starts
 * where fields does. */
int papof_deinterlace_tensor(papof_handle* h, int n_fields, int field_height, int width, int c, const papof_tensor* fields,
                             int first, int mode, const papof_tensor* flow_fw, const papof_tensor* flow_bw, double sigma,
                             const papof_tensor* video, const papof_tensor* confidence, void* stream);

/* Inverse telecine, part 1 (telecine.hip: k_field_metrics): for every field of a sequence, how much worse it weaves with its
 * next field than with its previous one, and the reverse, as integer counts per cell.  Film on interlaced video (3:2 pulldown,
 * 2:2) repeats each film frame over two or three consecutive fields; those fields show one instant, and weaving them gives
 * the film frame exactly, where papof_deinterlace_tensor would make up lines that the neighbouring field holds.  Absolute comb
 * counts do not separate film from video -- vertical detail looks like combing --; the counts below compare the two candidate
 * weaves pixel by pixel, at the same rows of two fields of one parity, so that the texture cancels.  A parallel call: no call
 * above changes.
 * fields: n_fields = T >= 3 fields of field_height = Hf rows, width = W; uint8, float32 or float64, (field, row, column,
 * channel), any non-negative strides, c = C channels, 1 <= C <= 4.  Field k holds the rows of parity (k + first) & 1 of frame
 * k; first is 0 or 1.  cell_rows: 1 .. 64.  comb_q, diff_q: integer thresholds, 0 .. 65535.
 * metrics: DEVICE pointer to T * 3 * Gy * Gx int32, contiguous (field, plane, cy, cx), Gy = ceil(Hf / cell_rows), Gx =
 * ceil(W / 64).  Every element is written exactly once; fields 0 and T - 1 get zeros.
 * Everything is integer.  q(uint8 b) = 257 * b; q(float v) = 0 for a NaN, else clamp(rint(65535.0 * v), 0, 65535), the
 * product in fp64, rint half to even.
 * For 1 <= t <= T - 2, p = (t + first) & 1, the centre rows are j = 1 .. Hf - 1 with (ja, jc) = (j - 1, j) for p = 0 and
 * j = 0 .. Hf - 2 with (ja, jc) = (j, j + 1) for p = 1: the lines above and below frame row 2 j + p, which the neighbouring
 * fields hold.  At a centre row j, a column x and a channel k:
 *
 *   b = q(field[t](j, x, k));  a-, c- = q(field[t - 1](ja | jc, x, k));  a+, c+ = q(field[t + 1](ja | jc, x, k))
 *   m(b; a, c) = min(|a - b|, |c - b|) when (a > b and c > b) or (a < b and c < b), else 0
 *   M- = max over k of m(b; a-, c-);  M+ = max over k of m(b; a+, c+)
 *   nd = max over k of max(|a+ - a-|, |c+ - c-|)
 *
 * and cell (j / cell_rows, x / 64) counts, in plane 0, M+ > M- + comb_q (the next field fits worse here); in plane 1,
 * M- > M+ + comb_q; in plane 2, nd > diff_q (the neighbours differ: field t + 1 does not repeat field t - 1).
 * One wave per cell, the counts by ballot: no atomics, no device memory besides the tensors, nothing of the handle's; the
 * result does not depend on what `metrics` held.  Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL:
 * the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor, data pointer or metrics, fields that are not uint8 /
 * float32 / float64, a negative stride, n_fields < 3, field_height < 1 or > 2^30 - 1, width < 1, c outside 1 .. 4, first
 * outside {0, 1}, cell_rows outside 1 .. 64, or a threshold outside 0 .. 65535. */
int papof_field_metrics_tensor(papof_handle* h, int n_fields, int field_height, int width, int c, const papof_tensor* fields,
                               int first, int cell_rows, int comb_q, int diff_q, int* metrics, void* stream);

/* Inverse telecine, part 2 (telecine.hip: k_weave_fields): n_frames = N frames of 2 Hf rows woven from the fields that a
 * table names.  fields: as above, n_fields = T >= 1.  table: DEVICE pointer to N * 2 int32, (frame, {the field of the even
 * rows, the field of the odd rows}).  video: uint8 / float32 / float64, (frame, row, column, channel) with 2 Hf rows, strides
 * [0..3] > 0; it must not overlap fields.
 *
 *   video[n](2 j + r, x, k) = store(load(field[table[n, r]](j, x, k))),  r = 0, 1
 *
 * with papof_deinterlace_tensor's load and store of a kept line: uint8 to uint8 keeps the input's bytes.  One pass, every output
 * element written once.  An index outside 0 .. T - 1 is the caller's error (as the sources of papof_mosaic_tensor): it is
 * not checked.  Enqueued on `stream` and returns without waiting; no device memory besides the tensors.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor, data pointer or table, fields or a video that are not
 * uint8 / float32 / float64, a negative stride, a zero stride of video along an axis in use, n_fields or n_frames < 1,
 * field_height < 1 or > 2^30 - 1, width < 1, c outside 1 .. 4, or a video that starts where fields does. */
int papof_weave_fields_tensor(papof_handle* h, int n_fields, int field_height, int width, int c, const papof_tensor* fields,
                              int n_frames, const int* table, const papof_tensor* video, void* stream);

/* Shot boundaries, the device's part (shots.hip: k_cell_hist): every frame of a video reduced to histograms of its luma per
 * cell of cell_rows x 64 pixels, as integer counts.  The calls above take their frames to be one continuous shot; the host
 * compares the histograms of consecutive frames region by region to find the cuts (tensors.py: shot_distances, detect_cuts)
 * and hands them over in the flows themselves: a NaN flow is "lost" to papof_track_tensor, "not alive" to
 * papof_temporal_filter_tensor, papof_propagate_tensor and papof_super_resolve_tensor, "occluded" to papof_fb_check_tensor
 * and "dead" to papof_refine_flow_tensor, papof_upsample_flow_tensor and papof_rs_rectify_tensor.  A parallel call: no call
 * above changes.
 * frames: n_frames = T >= 1 frames of height x width = H x W >= 1 x 1; uint8, float32 or float64, (frame, row, column,
 * channel), any non-negative strides, c = C channels, 1 <= C <= 4.  cell_rows: 1 .. 64.  bins: 4, 8, 16, 32 or 64.
 * hist: DEVICE pointer to T * Gy * Gx * bins int32, contiguous (frame, cy, cx, bin), Gy = ceil(H / cell_rows), Gx =
 * ceil(W / 64); the cells at the bottom and right edges are clipped to the frame.  Every element is written exactly once.
 * Everything is integer.  q as papof_field_metrics_tensor's: q(uint8 b) = 257 * b; q(float v) = 0 for a NaN, else
 * clamp(rint(65535.0 * v), 0, 65535), the product in fp64, rint half to even.  At a pixel with channels q0 .. q(C-1):
 *
 *   L = q0                                     for C = 1 or 2  (a second channel is not read)
 *   L = (77 * q0 + 150 * q1 + 29 * q2) >> 8    for C = 3 or 4  (a fourth channel is not read); 0 <= L <= 65535
 *   bin = (L * bins) >> 16
 *
 * and hist[t, cy, cx, k] is the number of pixels (y, x) of frame t with y / cell_rows = cy, x / 64 = cx and bin = k: the bins of
 * a cell add up to the cell's pixel count.
 * One wave per cell, the counts by ballot: no atomics, no device memory besides the tensors, nothing of the handle's; the
 * result does not depend on what `hist` held.  Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL:
 * the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor, data pointer or hist, frames that are not uint8 /
 * float32 / float64, a negative stride, n_frames, height or width < 1, c outside 1 .. 4, cell_rows outside 1 .. 64, or bins
 * not one of 4, 8, 16, 32, 64. */
int papof_cell_hist_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                           int cell_rows, int bins, int* hist, void* stream);

/* Decoder surfaces, the way in (surface.hip: k_ycc_to_rgb): 8-bit YCbCr planes with subsampled chroma, as a video decoder
 * leaves them on the device, to RGB frames for the calls above.  A parallel call: no call above changes.
 * n_frames = T >= 1 frames of height x width = H x W >= 1 x 1 luma samples.  y: uint8 (frame, row, column); cb, cr: uint8
 * (frame, row, column) of Hc x Wc samples, Wc = ceil(W / 2), Hc = ceil(H / sub_v), sub_v = 2 (4:2:0) or 1 (4:2:2); stride[3] of
 * the three is not read; any non-negative strides.  One descriptor per plane makes every common format a view of the
 * decoder's memory: NV12 / NV21 (column stride 2, cr one byte beside cb or the reverse), I420 / YV12, NV16, YUY2 / UYVY (y at
 * column stride 2, chroma at 4); a row pitch beyond the width is a stride.  rgb: uint8, float32 or float64 (frame, row,
 * column, channel) of 3 channels, strides [0..3] > 0 (NCHW and NHWC are strides); it must not overlap the planes.
 * tables: HOST pointer to six int32 {y_off, cy, crv, cgu, cgv, cbu}: the luma offset, 0 .. 255, and five coefficients at the
 * scale 2^14, each 0 .. 65535 -- the standard is the host's (tensors.py: ycc_tables), the device knows none.  For Kr, Kb, Kg =
 * 1 - Kr - Kb and limited range they are 16, rint(2^14 * 255 / 219), and rint(2^14 * f * 255 / 224) of f = 2 (1 - Kr),
 * 2 Kb (1 - Kb) / Kg, 2 Kr (1 - Kr) / Kg, 2 (1 - Kb); for full range 0, 2^14 and rint(2^14 * f).
 * siting_h: 0 "left" (chroma k at luma column 2 k) or 1 "center" (at 2 k + 0.5).  siting_v: 0 "center" (chroma j at row
 * 2 j + 0.5) or 1 "top" (at 2 j).  interlaced != 0: chroma row 2 i + p of the frame belongs to field p and sits at frame row
 * 4 i + 0.5 (p = 0) or 4 i + 2.5 (p = 1), the MPEG-2 / H.264 field positions; siting_v is then not used.
 * Everything is integer.  (a, b | wa, wb) is chroma index a with weight wa and index b with weight wb, both indices clamped
 * to the valid range.  At luma pixel (x, y):
 *
 *   horizontally, k = x >> 1:    left:    x even (k, k | 4, 0)        x odd (k, k + 1 | 2, 2)
 *                                center:  x even (k - 1, k | 1, 3)    x odd (k, k + 1 | 3, 1)         clamped to 0 .. Wc - 1
 *   vertically, sub_v = 1:       (y, y | 8, 0), whatever siting_v and interlaced
 *   sub_v = 2, j = y >> 1:       center:  y even (j - 1, j | 2, 6)    y odd (j, j + 1 | 6, 2)
 *                                top:     y even (j, j | 8, 0)        y odd (j, j + 1 | 4, 4)         clamped to 0 .. Hc - 1
 *   sub_v = 2, interlaced, p = y & 1, m = y >> 2, indices i of field p's own chroma rows, of which there are
 *   n = (Hc - p + 1) >> 1:       y = 4 m: (m - 1, m | 1, 7)   y = 4 m + 2: (m, m + 1 | 5, 3)
 *                                y = 4 m + 1: (m - 1, m | 3, 5)   y = 4 m + 3: (m, m + 1 | 7, 1)      clamped to 0 .. n - 1
 *                                and index i is row 2 i + p of the chroma planes
 *   C32 = sum over the four taps of wx * wy * c      (the weights add to 32; carried unrounded: chroma is not rounded twice)
 *   L = 32 * cy * (Y - y_off);  U = Cb32 - 4096;  V = Cr32 - 4096
 *   N_r = L + crv * V;   N_g = L - cgu * U - cgv * V;   N_b = L + cbu * U
 *   uint8:             clamp((N + 2^18) >> 19, 0, 255), an arithmetic shift
 *   float32, float64:  clamp(N, 0, 255 * 2^19) / (255 * 2^19) in fp64 (float32: one more rounding), the unrounded value
 *
 * No intermediate leaves int32: |L| <= 32 * 65535 * 255 < 2^29, |U|, |V| <= 4096 so a chroma term is at most 65535 * 4096
 * < 2^28, and |N| + 2^18 < 2^29 + 2 * 2^28 + 2^18 < 2^31.
 * Precision: with the tables of a standard a uint8 result is within 0.5 + 511 * 2^-15 = 0.5156 LSB of that standard's
 * real-valued matrix on the same bilinear chroma: 0.5 of the one rounding, and 2^-15 LSB per level of |Y - y_off| <= 255 and of
 * |C - 128| <= 128, twice for green, of the coefficients' own rounding to 2^-14.
 * One pass, every element of rgb written exactly once: the result does not depend on what rgb held.  No atomics, no device
 * memory besides the tensors, nothing of the handle's.  Enqueued on `stream` (the caller's hipStream_t on the handle's
 * device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor, data pointer or tables; planes that are not uint8; an
 * rgb that is not uint8 / float32 / float64; a negative stride, or a zero stride of rgb; n_frames, height or width < 1; sub_v
 * not 1 or 2; siting_h or siting_v not 0 or 1; y_off outside 0 .. 255 or a coefficient outside 0 .. 65535; interlaced with an
 * odd height or a height < 4. */
int papof_ycc_to_rgb_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* y,
                            const papof_tensor* cb, const papof_tensor* cr, int sub_v, int siting_h, int siting_v,
                            int interlaced, const int* tables, const papof_tensor* rgb, void* stream);

/* Which of its two kernel instances papof_ycc_to_rgb_tensor runs for these descriptors (no device is touched): 1 for the one
 * that loads and stores whole dwords, 0 for the one that goes lane by lane through the strides.  Both write the same bytes;
 * a test that means to cover one of them reads here that it did.  1 needs all of: width a multiple of 4; y with column
 * stride 1; cb and cr with column stride 2, equal row and frame strides and adjacent first bytes (cr = cb + 1: NV12, NV16;
 * cb = cr + 1: NV21); a uint8 or float32 rgb with strides [2], [3] of (3, 1) (NHWC) or with stride[2] = 1 and stride[3] a
 * multiple of 4 bytes (uint8) or 4 elements (float32) (NCHW); and the first byte, the rows and the frames of y, of the chroma
 * pair and of rgb on 4-byte boundaries (a float32 rgb: 16-byte).  PAPOF_EINVAL: width < 1, or a descriptor that
 * papof_ycc_to_rgb_tensor refuses. */
int papof_ycc_to_rgb_fast(int width, const papof_tensor* y, const papof_tensor* cb, const papof_tensor* cr,
                          const papof_tensor* rgb);

/* Decoder surfaces, the way out (surface.hip: k_rgb_to_ycc): RGB frames to 8-bit YCbCr planes with subsampled chroma, for an
 * encoder.  Sizes, planes, sub_v, the siting codes and interlaced as above; y, cb and cr are written (strides [0..2] > 0,
 * stride[3] not read), so the call writes straight into an NV12 surface and leaves its pitch padding alone.  rgb: uint8,
 * float32 or float64 (frame, row, column, channel) of 3 channels, any non-negative strides.
 * tables: HOST pointer to eight int32 {y_off, yr, yg, yb, ur, ug, vg, vb}: the luma offset, 0 .. 255, and seven coefficients
 * at the scale 2^14, each 0 .. 65535.  With sy = 219 / 255 and sc = 224 / 255 for limited range, 1 and 1 for full range:
 * yr = rint(2^14 sy Kr), yb = rint(2^14 sy Kb), yg = rint(2^14 sy) - yr - yb; ur, ug = rint(2^14 sc * 0.5 * (Kr, Kg) /
 * (1 - Kb)); vg, vb = rint(2^14 sc * 0.5 * (Kg, Kb) / (1 - Kr)).  The weight of B in Cb is ur + ug and that of R in Cr is
 * vg + vb, so a grey pixel has chroma 128 exactly, and full-range luma of a grey byte is that byte.
 * Everything is 64-bit integer.  q as papof_cell_hist_tensor's, of the three channels R, G, B of a pixel; D = 257 * 2^14, one
 * level of a byte:
 *
 *   Y  = clamp(floor((yr R + yg G + yb B + y_off D + D / 2) / D), 0, 255)                  per luma pixel
 *   Nu = (ur + ug) B - ur R - ug G;   Nv = (vg + vb) R - vg G - vb B                       per luma pixel, unrounded
 *   S  = sum over the taps of wx * wy * N     (the adjoint taps below; wx and wy each add to 4)
 *   Cb, Cr = clamp(floor((S + 128 * 16 D + 8 D) / (16 D)), 0, 255)                         one rounding per chroma sample
 *
 *   horizontally, chroma k:   left:    columns 2 k - 1, 2 k, 2 k + 1 with (1, 2, 1)    center:  2 k, 2 k + 1 with (2, 2)
 *                             columns clamped to 0 .. W - 1
 *   vertically, sub_v = 1:    row j with (4)
 *   sub_v = 2, chroma j:      center:  rows 2 j, 2 j + 1 with (2, 2)    top:  2 j - 1, 2 j, 2 j + 1 with (1, 2, 1)
 *                             rows clamped to 0 .. H - 1
 *   sub_v = 2, interlaced:    chroma row 2 m (top field) from luma rows 4 m, 4 m + 2 with (3, 1); chroma row 2 m + 1 (bottom
 *                             field) from rows 4 m + 1, 4 m + 3 with (1, 3); the second row clamped to the field's last
 *                             row, H - 2 + p
 *
 * Precision: with the tables of a standard a sample is within 0.5 + 2.5 * 255 * 2^-14 = 0.5389 LSB of the standard's
 * real-valued matrix and the same taps on q / 257 (three coefficients, one of them a difference of three roundings).
 * One pass, every sample of the three planes written exactly once, nothing else; no atomics, no device memory besides the
 * tensors.  Enqueued on `stream` and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor, data pointer or tables; planes that are not uint8; an
 * rgb that is not uint8 / float32 / float64; a negative stride, or a zero stride of a plane along (frame, row, column);
 * n_frames, height or width < 1; sub_v not 1 or 2; siting_h or siting_v not 0 or 1; y_off outside 0 .. 255 or a coefficient
 * outside 0 .. 65535; interlaced with an odd height or a height < 4. */
int papof_rgb_to_ycc_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* rgb, int sub_v,
                            int siting_h, int siting_v, int interlaced, const int* tables, const papof_tensor* y,
                            const papof_tensor* cb, const papof_tensor* cr, void* stream);

/* High-bit-depth decoder surfaces, the way in (surface.hip: k_ycc16_to_rgb, k_ycc16_to_rgb_nv): YCbCr planes of 9 .. 16 bits
 * per sample in 16-bit little-endian words -- P010, P012, P016, P210, P216, Y210, Y216, planar yuv420p10le / I010, I012,
 * yuv422p10le -- to RGB frames.  A parallel call: papof_ycc_to_rgb_tensor and everything behind it stay as they are.
 * Sizes, sub_v, siting_h, siting_v, interlaced, rgb and the plane shapes as papof_ycc_to_rgb_tensor's.  y, cb, cr:
 * PAPOF_DTYPE_U16 (frame, row, column), strides in WORDS, any non-negative strides, stride[3] not read: P010 has cb and cr at
 * column stride 2, cr one word beside cb; Y210 has y at column stride 2 and chroma at 4.
 * depth = d in 9 .. 16, P = 2^d - 1.  The sample of a word is s = (word >> shift) & P: shift = 16 - d for the MSB-aligned
 * formats (P010, P012, P016, P210, P216, Y210, Y216), 0 for the LSB-aligned ones (I010, I012, yuv422p10le); 0 <= shift <=
 * 16 - d.  The word's other bits are not looked at.
 * tables: HOST pointer to seven int32 {y_off, cy, crv, cgu, cgv, cbu, peak}: the luma offset, 0 .. P; five coefficients at the
 * scale 2^(d+6), each 0 .. 2^(d+8) - 1; and peak = Q in 1 .. 65535, the output level that means 1.0.  The standard is the host's
 * (tensors.py: ycc_tables16).  With m = 2^(d-8), for limited range y_off = 16 m, cy = rint(2^(d+6) Q / (219 m)) and the chroma
 * coefficients rint(2^(d+6) f Q / (224 m)) of the four factors f of papof_ycc_to_rgb_tensor; for full range y_off = 0 and both
 * divisors are P.  Q = 255 for a uint8 rgb, Q = P for float32 / float64 (the float is then the d-bit level over P); the device
 * divides by nothing but the constant Q * 2^(d+11).  At d = 8, Q = 255 these would be papof_ycc_to_rgb_tensor's tables and rule.
 * Everything is exact integer arithmetic; every product is int32 x int32 -> int64.  With the taps of
 * papof_ycc_to_rgb_tensor word for word (h_taps, v_taps, the field positions under interlaced; weights adding to 32):
 *
 *   C32 = sum over the four taps of wx * wy * c                                 (< 2^21; chroma carried unrounded)
 *   L = 32 * cy * (Y - y_off);  U = Cb32 - 2^(d+4);  V = Cr32 - 2^(d+4)
 *   N_r = L + crv * V;   N_g = L - cgu * U - cgv * V;   N_b = L + cbu * U
 *   uint8 (needs peak = 255):  clamp((N + 2^(d+10)) >> (d+11), 0, 255), an arithmetic shift
 *   float32, float64:          clamp(N, 0, Q * 2^(d+11)) / (Q * 2^(d+11)) in fp64 (float32: one more rounding)
 *
 * Bounds: |L| <= 32 * (2^(d+8) - 1) * P < 2^(2d+13); |U|, |V| <= 2^(d+4), so a chroma term is < 2^(2d+12) and green's two
 * < 2^(2d+13); |N| < 2^(2d+14) <= 2^46, and Q * 2^(d+11) < 2^43 is exact in fp64.
 * Precision: N / 2^(d+11) is the level in output LSB (1 / Q of full scale).  A coefficient is off its real value by at most
 * 0.5 at the scale 2^(d+6), which costs 2^-(d+7) LSB per level of |Y - y_off| <= P < 2^d (at most 2^-7) and per level of
 * |C - 2^(d-1)| <= 2^(d-1) (at most 2^-8, counted twice for green: 2^-7): less than 2^-6 LSB.  A float result is within 2^-6
 * LSB of d bits (Q = P) of the standard's real-valued matrix on the same bilinear chroma, a uint8 result within 0.5 + 2^-6 =
 * 0.5156 LSB of 8 bits.
 * One pass, every element of rgb written exactly once; no atomics, no device memory besides the tensors, nothing of the
 * handle's.  Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream), returns without
 * waiting.
 * PAPOF_EINVAL, before anything is enqueued: what papof_ycc_to_rgb_tensor refuses of the handle, descriptors, sizes and codes;
 * planes that are not PAPOF_DTYPE_U16; depth outside 9 .. 16; shift outside 0 .. 16 - depth; y_off outside 0 .. P, a
 * coefficient outside 0 .. 2^(d+8) - 1, peak outside 1 .. 65535; peak != 255 with a uint8 rgb. */
int papof_ycc16_to_rgb_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* y,
                              const papof_tensor* cb, const papof_tensor* cr, int depth, int shift, int sub_v, int siting_h,
                              int siting_v, int interlaced, const int* tables, const papof_tensor* rgb, void* stream);

/* Which of its two kernel instances papof_ycc16_to_rgb_tensor runs for these descriptors (no device is touched): 1 for the one
 * that loads 8 bytes at a time and stores whole dwords (P010 / P016 / P210 as decoders hand them over), 0 for the one that goes
 * lane by lane through the strides.  Both write the same bytes.  1 needs all of: width a multiple of 4; y with column stride 1;
 * cb and cr with column stride 2, equal row and frame strides and adjacent first words (cr = cb + 1 word, or the reverse);
 * the first word, the rows and the frames of y and of the chroma pair on 8-byte boundaries; and rgb as papof_ycc_to_rgb_fast
 * requires it.  PAPOF_EINVAL: width < 1, or a descriptor that papof_ycc16_to_rgb_tensor refuses. */
int papof_ycc16_to_rgb_fast(int width, const papof_tensor* y, const papof_tensor* cb, const papof_tensor* cr,
                            const papof_tensor* rgb);

/* High-bit-depth decoder surfaces, the way out (surface.hip: k_rgb_to_ycc16): RGB frames to planes of d = depth bits in 16-bit
 * words.  rgb, q, the adjoint taps and the field rule as papof_rgb_to_ycc_tensor's; depth, shift and the planes as
 * papof_ycc16_to_rgb_tensor's, written (strides [0..2] > 0).  The stored word is level << shift: all its other bits are 0.
 * tables: HOST pointer to eight int32 {y_off, yr, yg, yb, ur, ug, vg, vb}: the luma offset, 0 .. P, and seven coefficients,
 * each 0 .. 2^30.  With Sy = 219 m, Sc = 224 m (m = 2^(d-8)) for limited range and Sy = Sc = P for full range:
 * yr = rint(2^14 Sy Kr), yb = rint(2^14 Sy Kb), yg = 2^14 Sy - yr - yb; ur, ug = rint(2^14 Sc * 0.5 * (Kr, Kg) / (1 - Kb));
 * vg, vb = rint(2^14 Sc * 0.5 * (Kg, Kb) / (1 - Kr)).  Arithmetic is 64-bit integer; E = 65535 * 2^14 for every depth:
 *
 *   Y      = clamp(floor((yr R + yg G + yb B + y_off E + E / 2) / E), 0, P)             (the sum < 2^48)
 *   Nu     = (ur + ug) B - ur R - ug G;   Nv = (vg + vb) R - vg G - vb B                per luma pixel, unrounded, |N| < 2^47
 *   S      = sum over the adjoint taps of wx * wy * N                                   (weights add to 16; |S| < 2^51)
 *   Cb, Cr = clamp(floor((S + 2^(d-1) * 16 E + 8 E) / (16 E)), 0, P)                    one rounding per chroma sample
 *
 * A grey pixel has chroma exactly 2^(d-1); full-range luma of a grey q is rint(P q / 65535), which is q itself at d = 16.
 * Precision: a sample is within 0.5 + 2^-13 LSB of d bits of the standard's real-valued matrix and the same taps on q / 65535:
 * 0.5 of the one rounding; two coefficients off by at most 0.5 and the third, a difference, by at most 1 at the scale 2^14.
 * One pass, every sample of the three planes written exactly once, nothing else; no atomics, no device memory besides the
 * tensors.  Enqueued on `stream` and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: what papof_rgb_to_ycc_tensor refuses of the handle, descriptors, sizes and codes;
 * planes that are not PAPOF_DTYPE_U16; depth outside 9 .. 16; shift outside 0 .. 16 - depth; y_off outside 0 .. P or a
 * coefficient outside 0 .. 2^30. */
int papof_rgb_to_ycc16_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* rgb, int depth,
                              int shift, int sub_v, int siting_h, int siting_v, int interlaced, const int* tables,
                              const papof_tensor* y, const papof_tensor* cb, const papof_tensor* cr, void* stream);

/* Rolling-shutter rectification along the flows (rolling.hip: k_rs_rectify, k_rs_flow).  A rolling shutter reads the rows of
 * a frame one after another: row y of frame t of H rows is exposed at the time t + readout * (y - a) / H, in frame intervals,
 * with a = anchor * (H - 1) the row that is exposed at the frame's own time.  The video's dense flows give every pixel's
 * position one frame earlier and one frame later, each at its landing row's own time: three points of its trajectory.  The
 * parabola through them, evaluated at the frame's time, is where a global shutter would have seen the pixel.
 * n_frames = T >= 2 frames of height x width = H x W.  flow_fw, flow_bw: the T - 1 pairs' flows as
 * papof_temporal_filter_tensor takes them: flow_fw[t] from frame t to t + 1, flow_bw[t - 1] from frame t to t - 1.
 * readout: finite, |readout| <= 1 (negative: a sensor read from the bottom up); anchor in [0, 1]; iters 1 .. 8.
 * In fp64 in the stated order without fused multiply-adds, with r = readout / (double)H and a = anchor * (double)(H - 1):
 *
 * The displacement L_t(P) of a point P = (X, Y) of [0, W - 1] x [0, H - 1] of frame t, and whether it is alive:
 *   s = (a - Y) * r                          (the time from the row's exposure to the frame's time)
 *   s == 0:  L = (+0, +0), alive, no flow is read (readout = 0; the anchor row)
 *   else     (Fu, Fv) = flow_fw[t] (t < T - 1) and (Bu, Bv) = flow_bw[t - 1] (t > 0) sampled at P (sampler.h: taps_at,
 *            sample_flow: papof_track_tensor's sampler)
 *            tf = 1.0 + r * Fv;  tb = r * Bv - 1.0          (the times at which the point is at P + F and at P + B)
 *   0 < t < T - 1:  alive = tf >= 0.5 && tb <= -0.5 (false for a NaN)
 *            cF = (s * (s - tb)) / (tf * (tf - tb));  cB = (s * (s - tf)) / (tb * (tb - tf))
 *            L = (cF * Fu + cB * Bu, cF * Fv + cB * Bv)
 *   t = 0:          alive = tf >= 0.5;   cF = s / tf;  L = (cF * Fu, cF * Fv)        (a line: there is no backward flow)
 *   t = T - 1:      alive = tb <= -0.5;  cB = s / tb;  L = (cB * Bu, cB * Bv)
 * The solve for an output point Q, the P with P + L_t(P) = Q:
 *   P_0 = Q;  P_(k+1) = (Qx - Lx_t(P_k), Qy - Ly_t(P_k)) for k = 0 .. iters - 1
 *   alive only if Q, every P_k and P_iters lie in [0, W - 1] x [0, H - 1] (false for a NaN) and every evaluation was alive; the
 *   first failure ends the solve.
 *
 * papof_rs_rectify_tensor: out(t, y, x, ch) = frames[t] sampled bilinearly at P_iters of Q, and valid(t, y, x) = 1; where the
 * solve is dead, out = 0 and valid = 0 (papof_warp_affine_tensor's convention).  Q = (x, y) for matrices = NULL; else, with
 * M = matrices[t], Q = (X, Y) of papof_warp_affine_tensor: X = (m00 * x + m01 * y) + m02;  Y = (m10 * x + m11 * y) + m12 -- the
 * stabilizing warp and the rectification in one resampling.  frames, matrices, out, valid: layouts, strides, dtypes and
 * stores as papof_warp_affine_tensor's, c = 1 .. 4 channels.  readout = 0 without matrices gives store(load(frames)), with
 * matrices papof_warp_affine_tensor's out and valid.
 *
 * papof_rs_flow_tensor: the flows of the rectified video from the flows of the recorded one, both directions of every pair in
 * one launch.  out_fw[i](q), q = (x, y) a pixel of rectified frame i, i < T - 1:
 *   P = P_iters of the solve for Q = q in frame i;  (Fu, Fv) = flow_fw[i] sampled at P;  P' = (Px + Fu, Py + Fv) must lie in
 *   the image;  L' = L_(i+1)(P') must be alive (one evaluation, no iteration)
 *   out = (((Px - x) + Fu) + L'x, ((Py - y) + Fv) + L'y)
 * out_bw[i](q), q a pixel of rectified frame i + 1: the same with the solve in frame i + 1, flow_bw[i] and L_i.
 * Where anything is dead, and where a component comes out as a NaN, the component is the NaN 0x7ff8000000000000.  out_fw,
 * out_bw: float32 (one round-to-nearest) or float64, (pair, row, column, {vx, vy}), strides > 0; they must not overlap the
 * inputs.  readout = 0 gives finite input flows back wherever their landing point lies in the image (a NaN or infinite
 * neighbour enters a sample through its zero weight, as everywhere in sampler.h).
 *
 * What it is not: readout is the caller's, it is not estimated; motion that changes faster than three samples one frame apart
 * can follow (shake near half the frame rate) is not recovered; the end frames use a line; dead pixels are not filled.
 * One lane makes one output pixel, its iterate in registers; no device memory besides the tensors, no atomics; bitwise
 * reproducible.  Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns
 * without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (matrices and valid aside) or data pointer, frames or
 * out that are not uint8 / float32 / float64, flows, matrices or output flows that are not float32 / float64, a valid that is
 * not uint8, a negative stride, a zero stride of an output along an axis in use, n_frames < 2, height or width < 1, c outside
 * 1 .. 4, a readout that is not finite or beyond 1 in magnitude, an anchor outside [0, 1] (a NaN included), iters outside
 * 1 .. 8. */
int papof_rs_rectify_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                            const papof_tensor* flow_fw, const papof_tensor* flow_bw, double readout, double anchor, int iters,
                            const papof_tensor* matrices, const papof_tensor* out, const papof_tensor* valid, void* stream);
int papof_rs_flow_tensor(papof_handle* h, int n_frames, int height, int width, const papof_tensor* flow_fw,
                         const papof_tensor* flow_bw, double readout, double anchor, int iters, const papof_tensor* out_fw,
                         const papof_tensor* out_bw, void* stream);

/* Video deblurring: multi-frame Richardson-Lucy deconvolution along the flows (deblur.hip: k_deblur_ratio, k_deblur_update).
 * A frame exposed over a shutter is the scene averaged along each pixel's path, shutter * velocity pixels long; the flows give
 * the velocity, and the frames around a target, carried to it along the chains of flows, are blurred in other directions and
 * fill the spectral zeros of its own blur.  papof_motion_blur_tensor is the forward model; this is its inverse.
 * frames: ONE video of n_frames = T >= 2 frames of height x width x c (H, W, C), C = 1 .. 4, uint8 (x / 255.0), float32
 * (widened exactly) or float64, (frame, row, column, channel), any non-negative strides.  flow_fw, flow_bw: the T - 1 pairs'
 * flows as papof_temporal_filter_tensor takes them: float32 / float64, (pair, row, column, {vx, vy}), flow_fw[t] from frame t
 * to t + 1, flow_bw[t] from frame t + 1 to t, any non-negative strides.  out: uint8, float32 or float64, (frame, row, column,
 * channel), strides > 0; it must not overlap frames.  support: NULL, or uint8 (frame, row, column), strides > 0 (stride[3] is
 * not read).  offsets[k] = tau_k and weights[k] = w_k: the shutter's sample table, as papof_motion_blur_tensor takes it: tau_k
 * exactly 0 or 2^-20 <= |tau_k| <= 1 - 2^-20, w_k finite and >= 0 with a sum > 0, 1 <= n_samples <= 64; read before the call
 * returns.  radius = R in 0 .. 4, iters in 1 .. 256; use_check, alpha1, alpha2: the forward-backward test of every hop, as
 * papof_temporal_filter_tensor's.
 *
 * Everything is fp64 in the stated order without fused multiply-adds.  "Sampled at (X, Y)" is sampler.h's bilinear rule
 * (taps_at: truncation toward zero, neighbours clamped into the image, the four taps accumulated from 0 in (m, n) order).
 * clamp(v, 0, n) = fmin(fmax(v, 0.0), n).  wsum = the w_k > 0 summed from 0, k ascending; a sample with w_k == 0 is skipped
 * everywhere.  EPS = 2^-10.
 *   Data:      b_s(q, ch) = fmax(frames[s](q, ch), 0.0) (a NaN becomes 0).  L_t = b_t to start.
 *   Velocity   of frame s at a pixel, per component: 0 < s < T - 1: v = 0.5 * (flow_fw[s] - flow_bw[s - 1]); s = 0: v =
 *              flow_fw[0]; s = T - 1: v = 0.0 - flow_bw[T - 2].  At a point (X, Y) (pass B, every slot): both flows are sampled
 *              at (X, Y) (sample_flow) and combined the same way.  Non-finite: a component that is a NaN or infinite.
 *   Slots      of target t, in this order: s = t, t + 1, t - 1, t + 2, t - 2, ..., t + R, t - R; a slot outside 0 .. T - 1 is
 *              absent.
 *   Chains:    the chain of a point from frame a to frame b is the hop of papof_temporal_filter_tensor repeated: a < b through
 *              flow_fw[a], flow_fw[a + 1], ..., each tested against flow_bw of the same pair; a > b through flow_bw[a - 1],
 *              flow_bw[a - 2], ..., each tested against flow_fw.  A hop fails where it leaves [0, W - 1] x [0, H - 1] (or is a
 *              NaN) or, with use_check, fails the test; the chain is then dead for good.  a == b: the point itself, alive.
 *   Pass A (ratios), per target t, slot s, pixel q = (x, y) of frame s and channel ch:
 *              (X, Y), alive = the chain of q from s to t;  (vx, vy) = the velocity of s at the pixel q
 *              dead, or a non-finite velocity:  ratio_{t,s}(q, ch) = 1.0
 *              else  est = 0;  k ascending:  est = est + w_k * (L_t(., ch) sampled at (clamp(X + tau_k * vx, 0, W - 1),
 *                    clamp(Y + tau_k * vy, 0, H - 1)));   est = est / wsum;   ratio_{t,s}(q, ch) = b_s(q, ch) / fmax(est, EPS)
 *   Pass B (update), per target t and pixel p, with corr_ch = 0 and n = 0, for the slots in order:
 *              (X, Y), alive = the chain of p from t to s; dead: the slot is skipped
 *              (vx, vy) = the velocity of s at the point (X, Y); non-finite: the slot is skipped
 *              cs = 0;  k ascending:  cs = cs + w_k * (ratio_{t,s}(., ch) sampled at (clamp(X - tau_k * vx, 0, W - 1),
 *                    clamp(Y - tau_k * vy, 0, H - 1)));   corr_ch = corr_ch + cs / wsum;   n = n + 1
 *              n > 0:  L_t(p, ch) = L_t(p, ch) * (corr_ch / (double)n);  else L_t(p, ch) stays
 * All of pass A of an iteration comes before its pass B.  After `iters` iterations out = L, stored as papof_interp_tensor
 * stores (float64 as is, float32 with one round-to-nearest, uint8 = clamp(rint(255 * L), 0, 255), half to even, NaN: 0), and
 * support = the n of the last iteration.  Pass B is the gather form of the adjoint: exact where the velocity is locally
 * constant, wrong at motion boundaries.  A target reads only the recorded frames and its own L: any grouping of the targets
 * gives the same bytes.
 * Known answers: n_samples = 1 with offset 0, weight 1 and R = 0 returns finite frames whose values are 0 or >= EPS as they
 * are (every ratio is then b / b = 1.0 or 0.0 / EPS), whatever the flows; zero flows, R = 0 and uint8 frames return the same
 * bytes for any table; flows that are all NaN return store(fmax(frames, 0)) with support 0.
 *
 * Workspace (the caller's, device memory, as papof_super_resolve_tensor's): one target takes P = 8 * C * H * W * (2 R + 2)
 * bytes -- its L and its 2 R + 1 ratio images in float64, pixel-major with the channels contiguous; the chains are recomputed
 * in every pass, nothing else is kept.  The call runs the targets in rounds of G = min(T, workspace_bytes / P).
 * papof_deblur_workspace returns min(T, max(1, 2 GiB / P)) * P, or -1 for sizes the call refuses.
 * What it is not: the shutter (the table) is the caller's, it is not estimated; one straight line per pixel and frame -- a
 * path that curves inside the exposure is modelled only through the neighbours; no prior or regulariser: ringing and noise
 * grow with the iterations; a steady pan, where every frame has the same blur, gains little.
 * Enqueued on `stream` (the caller's hipStream_t on the handle's device, NULL: the null stream) and returns without waiting.
 * PAPOF_EINVAL, before anything is enqueued: a NULL handle, descriptor (support aside) or data pointer, frames or out that
 * are not uint8 / float32 / float64, flows that are not float32 / float64, a support that is not uint8, a negative stride, a
 * zero stride of out or support, n_frames < 2, height or width < 1, c outside 1 .. 4, height * width >= 2^30, radius outside
 * 0 .. 4, iters outside 1 .. 256, alphas that are negative or not finite, n_samples outside 1 .. 64, offsets or weights NULL,
 * an offset that is not 0 and not of a magnitude in [2^-20, 1 - 2^-20] (a NaN included), a weight that is negative or not
 * finite, a sum of weights that is not > 0 or not finite, a workspace that is NULL or smaller than P. */
int papof_deblur_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                        const papof_tensor* flow_fw, const papof_tensor* flow_bw, int n_samples, const double* offsets,
                        const double* weights, int radius, int iters, int use_check, double alpha1, double alpha2,
                        const papof_tensor* out, const papof_tensor* support, void* workspace, long long workspace_bytes,
                        void* stream);
long long papof_deblur_workspace(int n_frames, int height, int width, int c, int radius);

/* The projective warp with one matrix per SOURCE row (rows.hip: k_warp_rows): rotation-path stabilization of a camera with a
 * rolling shutter.  A camera that rotates by R(tau) and reads source row y of frame t at the time t + readout * (y - a) / H
 * sends the stabilized camera's pixel q to K R(t + tau(y)) S^T K^-1 q, y the row that point lands in (Forssen and Ringaby
 * 2010; Karpenko et al. 2011): a homography per source row, sampled by the caller at n_knots rows, and a fixed-point solve for
 * the landing row.  The call is papof_warp_projective_tensor with these differences: matrices is a TABLE, float32 (widened
 * exactly) or float64, indexed (frame, knot, row, column) -- n_knots = Kn >= 1 matrices of 3 x 3 per frame, any non-negative
 * strides, stride[1] between a frame's knots --; for Kn >= 2 knot k belongs to source row k * (H - 1) / (Kn - 1); and `iters`
 * in 1 .. 8 is the number of fixed-point iterations.  In fp64 in the stated order without fused multiply-adds, output pixel
 * (x, r) of frame i:
 *   Kn == 1:  M = knot 0; D, Nx, Ny, X = Nx / D, Y = Ny / D of PROJECTIVE SAMPLING above.  No iteration is run and iters is not
 *             read: the call returns the bytes of papof_warp_projective_tensor on (frame, row, column) = the table without
 *             its knot axis.
 *   Kn >= 2:  Y_0 = (double)r;  g = (double)(Kn - 1) / (double)(H - 1)  (one division).  For j = 0 .. iters - 1:
 *     clamp    Yc = Y_j if 0 <= Y_j <= H - 1;  Yc = +0.0 if !(Y_j >= 0) (a NaN goes here);  Yc = (double)(H - 1) if Y_j > H - 1
 *     index    s = Yc * g;  k = (int)s, and k = Kn - 2 if k > Kn - 2;  f = s - (double)k
 *     lerp     m_ab = A_ab + f * (B_ab - A_ab) for the nine entries, A = knot k, B = knot k + 1
 *     project  D = (m20 * x + m21 * r) + m22;  Nx = (m00 * x + m01 * r) + m02;  Ny = (m10 * x + m11 * r) + m12
 *     update   X = Nx / D;  Y_(j+1) = Ny / D     (two divisions, as in the projective rule)
 *   The last iteration's X, Y = Y_iters and D decide: inside iff D > 0 and 0 <= X <= W - 1 and 0 <= Y <= H - 1 (every comparison
 *   false for a NaN).  An earlier iterate may leave the frame, be a NaN or have D <= 0: only the clamp sees it.
 * From (X, Y) on, the taps, the sampler, the stores, valid, and the 0 where the pixel is not inside are
 * papof_warp_projective_tensor's.  A table whose knots are all equal gives the bytes of Kn == 1 unless an entry is -0.0
 * (A + f * 0.0 is A for every other finite A).  The (int) conversion sees only a clamped s that is not a NaN, and k is clamped
 * before an address is formed: no table, however hostile, is read out of bounds.
 * One lane makes one output pixel on papof_warp_affine_tensor's 64 x 4 tiling, its iterate in registers; no device memory
 * besides the tensors, no atomics; bitwise reproducible.  Enqueued on `stream` (the caller's hipStream_t on the handle's
 * device, NULL: the null stream) and returns without waiting.
 * What it is not: the table is the caller's (tensors.rotation_rows makes it from rotations); between knots the matrix is
 * interpolated entry by entry, not on the rotation group; pixels that are not inside are not filled.
 * PAPOF_EINVAL, before anything is enqueued: papof_warp_projective_tensor's list (a NULL handle, descriptor -- valid aside --
 * or data pointer, frames or out that are not uint8 / float32 / float64, a valid that is not uint8, a zero stride of an
 * output, n_frames, height, width or c < 1), n_knots < 1 or > PAPOF_ROWS_MAX_KNOTS, n_knots > 1 with height < 2, iters outside
 * 1 .. 8 when n_knots > 1, a table that is not float32 / float64, a negative stride. */
enum { PAPOF_ROWS_MAX_KNOTS = 4096 };
int papof_warp_rows_tensor(papof_handle* h, int n_frames, int height, int width, int c, const papof_tensor* frames,
                           const papof_tensor* matrices, int n_knots, int iters, const papof_tensor* out,
                           const papof_tensor* valid, void* stream);

/* Measurement aid (tools/collection_trace.py): host-side wall seconds of the LAST papof_flow* / papof_seq_push* call on this
 * handle -- out[0] from the call's entry until everything was enqueued (the runtime's launch path: ~200 launches for a
 * 240x135 pair on the reference schedule), out[1] the wait for the streams that followed, out[2] from the call's entry until
 * the host began to enqueue the coarsest level's solves (what it enqueues first delays the main stream's first kernel). */
int papof_last_host_times(papof_handle* h, double out[3]);

/* Measurement / test aid: what the LAST papof_flow* / papof_seq_push* call on this handle enqueued -- out[0] k_flow_system
 * launches (one kernel from the flow to the linear system), out[1] those of them that carried the previous outer iteration's
 * increment (no update kernel in front of them), out[2] update kernel launches (k_update_warp_phi), out[3] fills of the
 * solver's (du, dv) planes in front of a solve. */
int papof_last_chain_stats(papof_handle* h, long long out[4]);

/* Test aid: one exact-order solve of `n_sor` sweeps on synthetic height x width planes (the micro-benchmark's), once
 * whole and `reps` times as two band launches on two streams -- bands < split_band on a stream of the call's own, the
 * rest `delay_us` microseconds later on the handle's stream (sor.hip: sor_solve_bands).  *mismatches = 16-byte cells of the solver's
 * (du, dv) planes, intermediate sweeps included, that differ from the whole solve's (0 expected); *bands = bands of the
 * layout.  PAPOF_EINVAL when this layout cannot be solved in band ranges (<= 8 bands, < 3 sweeps, split out of range). */
int papof_test_sor_strips(papof_handle* h, int height, int width, int n_sor, int split_band, int reps, int delay_us,
                          long long* mismatches, int* bands);

/* Test aid: write the repeating 8-byte `pattern` (say a NaN) over every byte of every device block of the handle whose
 * contents no later call may rely on, so that a test can show that call N + 1 does not depend on what call N -- or a
 * corrupt frame -- left behind.  Waits for the handle's own streams (main, preparation, copy), fills on the main stream,
 * waits again.  Filled: the arena over its whole capacity (not only what the last call carved out of it), the host path's
 * staging block, the device-tensor path's one-pair scratch, the exact Laplacian-noise pass's reduction scratch and its
 * LapPara (8 doubles: every pass that reads them copies the constant 0.02 over them first, solve_levels and the smooth-flow
 * stage, so no call may rely on them either).  *bytes (may be NULL) = bytes filled; 0 on a handle that has run nothing
 * but for that small Laplacian-noise block.  The kept sequence is reset as by papof_seq_reset: its pyramid lived in the arena.
 * Left alone, because a pattern there would test nothing about data dependences:
 *   - the solver's progress counters and abort word: kernels spin on them, garbage could only hang the device;
 *   - the Laplacian-noise guard's flags: a flag is set when it EQUALS the pass number, a pattern could forge a proof;
 *   - LapPara's initial value 0.02: a constant written once when the handle is made;
 *   - the phase stamps (device slots and pinned host copy): they carry clock readings for the timers, never a result's data;
 *   - the refusal flag of a caller's initial flow: cleared by the call that uses it, its value decides a return code.
 * A caller that ran the device-tensor calls on a stream of its own waits for that stream first.
 * PAPOF_EINVAL: a NULL handle. */
int papof_test_poison(papof_handle* h, unsigned long long pattern, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* PAPOF_H */
