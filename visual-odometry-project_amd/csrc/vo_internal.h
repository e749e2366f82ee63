// Internal (C++) declarations shared by the HIP translation units of libvo_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vo_hip.h"

// A lazily grown device allocation owned by the context.
struct vo_buf {
  void* p = nullptr;
  size_t cap = 0;
};

struct vo_prof_slot {
  double total_ms = 0.0;
  int64_t launches = 0;
};

struct vo_prof_pair {
  int k;
  hipEvent_t a, b;
};

struct vo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  char err[512] = {0};
  // When set, the next launch that supports it (state_regroup_klt, klt_track16) is made with hipExtLaunchKernelGGL and this
  // event as its stop event: the event IS the kernel's completion signal, no marker packet behind the kernel (a marker
  // costs the queue ~4 us before the next dispatch, and a waiting queue one more hop).  Cleared by that launch.
  hipEvent_t next_stop = nullptr;

  // profiling
  bool prof_on = false;
  int prof_kernel = -1;
  int prof_every = 1;                 // bracket every n-th launch of a profiled kernel only (events perturb the stream)
  unsigned prof_seen[VO_K_COUNT] = {0};
  vo_prof_slot prof[VO_K_COUNT];
  std::vector<hipEvent_t> ev_free;
  typedef vo_prof_pair pending_ev;
  std::vector<pending_ev> ev_pending;

  // workspace (device)
  vo_buf img, img2, scores, kp, desc;
  vo_buf nms_keys_l1, nms_idx_l1, nms_keys_a1, nms_idx_a1;   // candidate lists
  vo_buf nms_keys_c, nms_idx_c;                              // compacted candidates
  vo_buf nms_hist, nms_ctl, nms_sel, nms_cand, nms_alive, nms_segcnt, nms_rank;
  bool nms_alive_dirty = false;
  int nms_parity = 0;            // NMS calls alternate between two histograms (the idle one is cleared meanwhile)
  int nms_S = 0;                 // sequences per launch of the last NMS call (the histograms' layout depends on it)
  float* nms_kp_f32 = nullptr;   // optional: the NMS also writes its keypoints as float pairs here (device)
  vo_buf scratch[16];
  vo_buf match_arrived;          // knn2_mfma_kernel's per-query-block arrival counters (zero between calls)
  int match_last_path = -1;      // the kernel the last vo_match_knn2_ratio / vo_match_knn2 kept (VO_MATCH_PATH_*; -1: none ran)
  bool lds_opt_in[2] = {false, false};         // hipFuncSetAttribute is per device: remembered per context (response, NMS)
  hipStream_t aux_stream = nullptr;            // vo_sift: the octaves' last two layers and extrema run beside the next octave
  hipStream_t aux_stream2 = nullptr;           //          (octave 0 on the first, the smaller octaves on the second)
  std::vector<hipEvent_t> aux_events;
  vo_buf sift_arena;
  // pinned host staging
  void* h_pin = nullptr;
  size_t h_pin_cap = 0;
  // bytes the device-resident forms of the bootstrap stages (vo_good_features_batch_dev, vo_fundamental_*_dev) copied between
  // host and device: scalars and the RANSAC batch's samples / counts; vo_pipeline_bootstrap_seq reports the difference
  int64_t bytes_h2d = 0, bytes_d2h = 0;
  // the device 8-point RANSAC's workspace (bootstrap.hip: vo_fundamental_ransac_dev), grown to the largest lane count and
  // population seen; the threshold table goes up when the confidence or the budget change, not per call
  vo_buf f8_ctl, f8_raws, f8_F, f8_counts, f8_risky, f8_masks, f8_table, f8_samples;
  std::vector<double> f8_table_host;
  double f8_table_conf = 0.0;
  // window bundle adjustment (window_ba.hip): the solver's per-window workspace, the builder's row x slot match table
  vo_buf ba_work, ba_match;
};

// a launch that takes vo_ctx::next_stop as its stop event when one is set (and clears it)
template <class K, class... A>
inline void vo_launch_stop(vo_ctx* ctx, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (ctx->next_stop) {
    hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, nullptr, ctx->next_stop, 0, args...);
    ctx->next_stop = nullptr;
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  }
}

int vo_set_error(vo_ctx* ctx, int code, const char* fmt, ...);
int vo_ensure(vo_ctx* ctx, vo_buf& b, size_t bytes);
int vo_ensure_pinned(vo_ctx* ctx, size_t bytes);

#define VO_HIP_TRY(ctx, expr)                                                         \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return vo_set_error((ctx), VO_EHIP, "%s failed: %s (%s:%d)", #expr,             \
                          hipGetErrorString(e_), __FILE__, __LINE__);                 \
  } while (0)

#define VO_TRY(expr)                 \
  do {                               \
    int s_ = (expr);                 \
    if (s_ != VO_OK) return s_;      \
  } while (0)

#define VO_REQUIRE(ctx, cond, ...)                                  \
  do {                                                              \
    if (!(cond)) return vo_set_error((ctx), VO_EINVAL, __VA_ARGS__); \
  } while (0)

// Brackets one kernel launch with an event pair when profiling is enabled for it.
struct vo_prof_scope {
  vo_ctx* c;
  int k;
  hipEvent_t a = nullptr, b = nullptr;
  vo_prof_scope(vo_ctx* ctx, int kernel);
  ~vo_prof_scope();
};

static inline int vo_check_launch(vo_ctx* ctx, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return vo_set_error(ctx, VO_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return VO_OK;
}

static inline int vo_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- the window arena (window_ba.hip, window_structure.hip, structure_loop.hip; defined in vo_ctx.hip) ----
constexpr int VO_WINDOW_WMAX = 16;      // slots per window
// S windows of W slots, at most L_cap landmarks and M_cap observations each; `who` heads the message
int vo_check_window_shape(vo_ctx* ctx, const char* who, int S, int W, int L_cap, int M_cap);
// The Levenberg-Marquardt parameters vo_ba_params and vo_structure_params share, checked, 0 replaced by its default.
struct vo_lm_params {
  int max_iter, max_trials;
  double huber, lambda0, step_tol;
};
int vo_resolve_lm_params(vo_ctx* ctx, const char* who, int max_iter, int max_trials, double huber_px, double lambda0,
                         double step_tol, vo_lm_params* out);

// Tile order of the image kernels.  Workgroups are dealt to the eight XCDs round-robin by their linear id (ids equal
// mod 8 share an L2 -- observed, not promised: speed only), so with tile = id neighbouring tiles never share an L2
// and every halo byte is fetched once per tile that needs it.  This map gives the workgroups of one XCD a contiguous
// range of the n tiles instead (row-major: whole bands of the image); it is a bijection for any n.
__device__ __forceinline__ unsigned vo_xcd_tile(unsigned id, unsigned n) {
  const unsigned q = n >> 3, r = n & 7u, x = id & 7u, j = id >> 3;
  return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + j;
}

struct vo_cam2 {      // the two intrinsic matrices of the two-view bootstrap (bootstrap.hip), row-major
  double K1[9], K2[9];
};

// ---- internal entry points shared between translation units (not part of the C ABI) ----
// Frame ingest (ingest.hip).  vo_undist: the undistortion of one camera as the kernel takes it, by value -- the pinhole
// camera of the output (fx, fy, cx, cy), the intrinsics of the distorted image (..r) and (k1, k2, p1, p2, k3).
struct vo_undist {
  double fx, fy, cx, cy, fxr, fyr, cxr, cyr, k1, k2, p1, p2, k3;
};
// K, K_raw (NULL: K) row-major 3x3, dist 5 coefficients (NULL: none); refuses non-finite values and a singular K
int vo_undist_make(vo_ctx* ctx, const char* who, const double* K, const double* dist, const double* K_raw, vo_undist* out);
// The pixels in front of the first 4-byte boundary of an output image.  The grey kernel loads and stores dwords: a
// three-channel input goes to its buffer's (4-byte aligned) start + vo_ingest_head(out), so that the first whole group of
// four pixels starts on a dword in both images (head + 3 * head = 4 * head).
static inline size_t vo_ingest_head(const void* out) { return (size_t)((4 - ((uintptr_t)out & 3)) & 3); }
// One launch on `st`: d_in (channels = 1: H x W grey, 3: H x W x 3 B, G, R) -> d_out (H x W grey), undistorted when und is
// given.  channels = 1 needs und (a plain copy is the caller's).  No synchronisation; ctx only receives an error text.
int vo_ingest_dev(vo_ctx* ctx, hipStream_t st, const uint8_t* d_in, int channels, int H, int W, const vo_undist* und,
                  uint8_t* d_out);
// How a context's own stream is created.  cu_lo..cu_hi: its kernels run on those compute units only (cu_hi < cu_lo: no
// mask); priority: -1 / +1 the least / greatest the device offers, 0 the default -- a mask wins over a priority.
struct vo_stream_cfg {
  int cu_lo = 0, cu_hi = -1;
  int priority = 0;
  bool operator==(const vo_stream_cfg& o) const { return cu_lo == o.cu_lo && cu_hi == o.cu_hi && priority == o.priority; }
};
// cus "lo-hi" (anything else: no mask), priority "low" / "high" (anything else: the default); either may be NULL
vo_stream_cfg vo_stream_cfg_parse(const char* cus, const char* priority);
// vo_create with the stream's configuration given (vo_create reads it from VO_STREAM_CUS / VO_STREAM_PRIORITY); unused when
// `stream` is the caller's
int vo_create_stream(int device, void* stream, const vo_stream_cfg& cfg, vo_ctx** out);
// P3P hypotheses + inlier counts of the frame loop (p3p.hip): sample indices derived on the device from raw
// generator outputs in a ring, population size and stream position read on the device.
struct vo_hyp_batch {     // several sequences per launch (grid.y = sequence); the output arrays are S blocks of Hyp entries
  int S = 1;
  size_t X = 0, x = 0;    // doubles between the sequences' landmark / keypoint arrays
  size_t raws = 0;        // words between their generator rings
  size_t ctl = 0;         // bytes between their control blocks (d_n, d_rawpos, d_flag, d_ts point into them)
  const double* cam = nullptr;   // (optional) per-sequence intrinsics in device memory: sequence q's K (row-major 3x3) at
  size_t cam_stride = 0;         // cam + q * cam_stride; NULL: the K the call is given, for every sequence
};
int vo_p3p_hypotheses_ring_dev(vo_ctx* ctx, const double* d_X, const double* d_x, const int32_t* d_n, int n_cap,
                               const double* K, const uint32_t* d_raws, const uint64_t* d_rawpos, uint32_t raw_mask,
                               int Hyp, double thr_sq, double* d_R, double* d_t, uint8_t* d_valid, int32_t* d_counts,
                               uint64_t* d_masks, uint32_t* d_flag, uint64_t* d_ts = nullptr,
                               const vo_hyp_batch* batch = nullptr);
// SIFT tracker mode of the frame pipeline: device-resident detect + describe (sift.hip: extern "C" vo_sift_dev) and
// matching (match.hip)
extern "C" int vo_match_u8_dev(vo_ctx* ctx, const uint8_t* d_q, const int32_t* d_nq, int cap_q, const uint8_t* d_t,
                               const int32_t* d_nt, int cap_t, double ratio, int32_t* d_pairs, int32_t* d_npairs,
                               int row_bytes = 128);
// ... for S sequences in one launch (blockIdx.z = sequence): sequence z's query / train rows at + z * q_stride / t_stride
// bytes, its counts at d_nq + z * nq_stride / d_nt + z * nt_stride, its pairs at d_pairs + z * 2 * cap_q, its pair count
// at d_npairs[z]
extern "C" int vo_match_u8_batch_dev(vo_ctx* ctx, const uint8_t* d_q, size_t q_stride, const int32_t* d_nq, int nq_stride,
                                     int cap_q, const uint8_t* d_t, size_t t_stride, const int32_t* d_nt, int nt_stride,
                                     int cap_t, int S, double ratio, int32_t* d_pairs, int32_t* d_npairs, int row_bytes);
// ... and its first half alone: the 2-NN lists (nearest, second nearest train index; squared distances as float64) of
// sequence z at d_best / d_d2 + z * 2 * cap_q, rows past its query count not written.  Exported by libvo_hip.so without
// being part of the C ABI of vo_hip.h (no stability promise): tests/test_gpu_matcher.py reaches both through
// vo/_native.py's Context.knn2_u8_batch_dev / match_u8_batch_dev.
extern "C" int vo_knn2_u8_batch_dev(vo_ctx* ctx, const uint8_t* d_q, size_t q_stride, const int32_t* d_nq, int nq_stride,
                                    int cap_q, const uint8_t* d_t, size_t t_stride, const int32_t* d_nt, int nt_stride,
                                    int cap_t, int S, int row_bytes, int32_t* d_best, double* d_d2);
// vo_sift_all_batch_dev (sift.hip) with d_found[q] (nullable): image q's keypoint count whether or not it fits `rows`, -1
// when its candidate / keypoint lists overflowed -- what the SIFT tracker mode names when a frame does not fit
extern "C" int vo_sift_all_found_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, int rows,
                                     float* d_kp, size_t kp_stride, float* d_desc, uint8_t* d_desc_u8, size_t desc_stride,
                                     int32_t* d_n, int32_t* d_over, int32_t* d_found);
// raw (2r+1)^2 patches of the zero-padded image as BYTES, rows padded with zeros to row_bytes (harris.hip)
extern "C" int vo_patch_descriptors_u8_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, const double* d_kp_xy, int N,
                                           int r, uint8_t* d_desc, int row_bytes);
// ... for S sequences in one launch: sequence q's image, keypoints and rows at + q * img_stride / kp_stride (doubles) /
// desc_stride (bytes)
extern "C" int vo_patch_descriptors_u8_batch_dev(vo_ctx* ctx, const uint8_t* d_img, size_t img_stride, int S, int H, int W,
                                                 const double* d_kp_xy, size_t kp_stride, int N, int r, uint8_t* d_desc,
                                                 size_t desc_stride, int row_bytes);
// Device-resident forms of the two-view bootstrap's stages (goodfeatures.hip, bootstrap.hip): inputs in HBM, results left
// there.  vo_fundamental_hypotheses / vo_fundamental_fit / vo_relative_pose upload, call these and download (vo_good_features
// runs the stages of vo_good_features_batch_dev at S = 1).  All work on ctx->stream; the hypothesis form synchronises (the
// counts come back), the others do not.
// vo_good_features_batch_dev (vo_hip.h) with the number of round launches (0 .. 24; the ABI call: 24) and the rounds path's
// candidate limit (1 .. 131 072; the ABI call: 131 072) given.  Results never depend on either: an image the rounds do not
// finish, or whose candidates exceed the limit, is finished by the one-workgroup walk.  Like the other extern "C" entry
// points of this file it is exported by libvo_hip.so without being part of the C ABI of vo_hip.h (no stability promise):
// tests/test_gpu_good_features_batch.py binds it by hand to reach both hand-overs to the walk.
extern "C" int vo_good_features_batch_rounds_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                                                 const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality,
                                                 double min_dist, int block, float* d_xy, size_t xy_stride, int32_t* d_n,
                                                 int32_t* d_over, int32_t* d_info, int n_rounds, int cand_limit);
constexpr int VO_GFB_ROUNDS = 24, VO_GFB_CANDIDATES = 131072;      // what the ABI call passes for the two
// ... and with a gate per image: d_go (optional, S ints on the device) -- an image whose word is 0 is left out of the map
// and the candidate kernels, has no candidates, and every later stage falls through for it (no sort work, no rounds, no
// walk); its d_n / d_over are 0.  The frame loop's re-detect (pipeline_step.hip, vo_pipeline_config.detector = 1).
int vo_good_features_batch_gated_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                                     const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality,
                                     double min_dist, int block, float* d_xy, size_t xy_stride, int32_t* d_n, int32_t* d_over,
                                     int32_t* d_info, int n_rounds, int cand_limit, const int* d_go);
// the argument checks of the batched forms alone (what vo_pipeline_create refuses a Shi-Tomasi configuration with)
int vo_good_features_batch_check(vo_ctx* ctx, int S, int H, int W, double quality, double min_dist, int block);
//   hypotheses: samples (host, Hyp x 8, checked against N) are the only array uploaded; counts (host, Hyp) the only one
//   downloaded; d_F Hyp x 9, d_counts Hyp, d_masks Hyp x cdiv(N, 64) words (nullable) are the caller's device buffers
int vo_fundamental_hypotheses_dev(vo_ctx* ctx, const double* d_p1, const double* d_p2, int N, const int32_t* samples, int Hyp,
                                  int normalize_samples, int error_kind, double threshold, int32_t* d_samples, double* d_F,
                                  int32_t* d_counts, uint64_t* d_masks, int32_t* counts);
//   fit: over the correspondences d_mask selects (nullable: all); d_F 9 doubles; d_n_used (nullable) their count
//   (exported like the entry points above: tests/test_gpu_twoview_reference.py binds it by hand to read d_n_used)
extern "C" int vo_fundamental_fit_dev(vo_ctx* ctx, const double* d_p1, const double* d_p2, int N, const uint8_t* d_mask, int normalize,
                           double* d_F, int32_t* d_n_used);
//   relative pose: d_M 12, d_X N x 3, d_mask_out N (nullable), d_M4 48 (nullable)
int vo_relative_pose_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int N, const uint8_t* d_inliers, const double* K1,
                         const double* K2, const double* d_F, double* d_M, double* d_X, uint8_t* d_mask_out, double* d_M4);
// the next `count` 32-bit outputs of NumPy's PCG64 Generator (ransac_host.hip); advances *rng
void vo_rng_raw32(vo_pcg64* rng, int count, uint32_t* out);
// The 8-point RANSAC loop of the two-view bootstrap on the device (bootstrap.hip): sampler, hypotheses, scores and the
// sequential accept / adapt rule, for L lanes through one set of launches.
enum { VO_F8_RUN = 0,       // the loop wants a (another) batch of samples
       VO_F8_DONE = 1,      // the loop has ended with a model of >= 8 inliers; its mask is unpacked
       VO_F8_HOST = 2,      // the device cannot finish it: a draw NumPy might have rejected inside the consumed prefix, a
                            // population of 8, a budget the threshold table does not hold -- the host sampler redoes it
       VO_F8_FAILED = 3 };  // fewer than 8 correspondences, or no model with 8 inliers
struct vo_f8_ctl {          // one lane's loop state in device memory
  vo_pcg64 rng;             // where the loop starts
  int32_t n;                // population; -1 on upload: read from the device count
  int32_t status;
  int32_t best_count, best_idx, consumed, batch;
  int64_t n_done, n_it;
  double orat;
};
struct vo_f8_lanes {        // lane q's blocks: p1 / p2 + q * pts, inliers + q * inl, F + q * F, its count at d_n[q * n]
  int L = 1;
  size_t pts = 0, inl = 0, F = 0;
  int n = 0;
};
struct vo_f8_params {
  int normalize_samples, error_kind;
  double threshold, outlier_ratio, confidence;
  int64_t max_iterations;   // < 0: unbounded
};
struct vo_f8_result {
  int32_t status;           // VO_F8_DONE or VO_F8_FAILED
  int32_t n, best_count, consumed, finished_by_host;
  int64_t iterations;
};
// d_p1 / d_p2: n_cap pairs per lane; the populations from d_n (device) or n_host (d_n == NULL).  rngs[q]: where lane q's
// loop starts, advanced by what it consumed.  d_inl: n_cap bytes per lane (the accepted model's inliers); d_F: the closing
// fit over them (9 doubles per lane).  Synchronises: res[q] is complete when it returns.
int vo_fundamental_ransac_dev(vo_ctx* ctx, const double* d_p1, const double* d_p2, int n_cap, const int32_t* d_n,
                              const int32_t* n_host, const vo_f8_params& prm, vo_pcg64* rngs, uint8_t* d_inl, double* d_F,
                              const vo_f8_lanes* lanes, vo_f8_result* res);
// The relative pose of every lane vo_fundamental_ransac_dev just finished (status VO_F8_DONE in the context's control blocks;
// the others are skipped): lane q's points, inliers and F as above, its camera K at d_cam + d_seq[q] * cam_stride (doubles)
// for both views; M (12 doubles) at d_M + q * lanes.F, X (n x 3) at d_X + q * X_stride, mask at d_mask_out + q * lanes.inl.
int vo_relative_pose_lanes_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, const vo_f8_lanes& lanes, const uint8_t* d_inl,
                               const double* d_F, const double* d_cam, size_t cam_stride, const int32_t* d_seq, double* d_M,
                               double* d_X, size_t X_stride, uint8_t* d_mask_out);
// Device-resident forms of the calibrated two-view bootstrap (essential5.hip): points in HBM, K1 / K2 host pointers (their
// closed-form inverses travel as launch arguments).  The caller's device blocks of one batch of Hyp samples:
struct vo_e5_work {
  int32_t* samples = nullptr;   // Hyp x 5
  double* E = nullptr;          // Hyp x 10 x 9
  double* F = nullptr;          // Hyp x 10 x 9: K2^-T E K1^-1, what the scorer reads
  int32_t* n_sol = nullptr;     // Hyp
  int32_t* counts = nullptr;    // Hyp x 10
  uint64_t* masks = nullptr;    // Hyp x 10 x cdiv(N, 64) words (nullable)
  int32_t* best = nullptr;      // 3 Hyp words: best counts (Hyp), best solution indices (Hyp), valid bytes (Hyp)
};
//   hypotheses: samples (host, Hyp x 5, checked against N) are the only array uploaded; best_count, best_sol (host, Hyp
//   each) and valid (host, Hyp bytes), each nullable, the only ones downloaded: 9 bytes per sample.  Synchronises.
int vo_essential_hypotheses_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int N, const double* K1, const double* K2,
                                const int32_t* samples, int Hyp, int error_kind, double threshold, const vo_e5_work& w,
                                int32_t* best_count, int32_t* best_sol, uint8_t* valid);
//   the loop: d_E 9 doubles, d_inl N bytes (the accepted model and its mask row); *rng advanced by what the loop consumed.
//   Uses the context's scratch blocks 2 .. 8.  Synchronises.
int vo_essential_ransac_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int N, const double* K1, const double* K2,
                            int error_kind, double threshold, double outlier_ratio, double confidence, int64_t max_iterations,
                            vo_pcg64* rng, double* d_E, uint8_t* d_inl, int64_t* iterations, int32_t* best_count);
// DLT with a device-resident point count (dlt.hip)
int vo_triangulate_dlt_ndev(vo_ctx* ctx, const double* d_x1, const double* d_x2, const int32_t* d_n, int n_cap,
                            const double* d_C1, const double* d_C2, double* d_X);
// pose refinement with a device-resident point count and either kind of inlier mask (refine.hip)
int vo_refine_pose_ndev(vo_ctx* ctx, const double* d_X, const double* d_x, int N, const int32_t* d_n, const double* K,
                        const uint8_t* d_mask8, const uint64_t* d_mask_bits, const double* d_Rt0, int max_iter,
                        double* d_out14, unsigned tag);
// KLT with a device-resident keypoint count (klt.hip).  src (optional): the frame loop's view of its points --
// keypoints 0 .. *n-1 come from d_prev_xy; when *n < frac * *num_features (the re-detect rule, klt.py:207-230)
// the detector's n_det keypoints follow as points *n .. *n + n_det - 1.
struct vo_klt_source {
  const int32_t* n = nullptr;
  const int32_t* num_features = nullptr;
  double frac = 0.0;
  const double* det_kp = nullptr;
  int n_det = 0;
  unsigned long long* ts = nullptr;   // (optional) receives wall_clock64() when the kernel's first work item starts
  const int* det_go = nullptr;        // (optional, one int per sequence) 0: det_kp was not produced, nothing is appended
  const int32_t* n_det_dev = nullptr; // (optional, one int per sequence) the detector's count read on the device instead of
                                      // n_det (a Shi-Tomasi re-detect; below 0: the detector failed, nothing is appended)
};
// several sequences per launch (grid.y = sequence): element strides from one sequence's block to the next
struct vo_klt_batch {
  int S = 1;
  size_t pyr = 0;      // bytes between the sequences' pyramid buffers (same for prev and next)
  size_t xy = 0;       // floats between their keypoint arrays (prev_xy and next_xy)
  size_t out = 0;      // elements between their status / err arrays
  size_t ctl = 0;      // bytes between their control blocks (vo_klt_source.n / num_features / ts point into them)
  size_t det = 0;      // doubles between their detector keypoint lists
};
int vo_klt_track_ndev(vo_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_prev_pyr, const uint8_t* d_next,
                      const uint8_t* d_next_pyr, int H, int W, int n_levels, const float* d_prev_xy, int N,
                      const int32_t* d_n, int win, int max_iter, double eps, double min_eig, float* d_next_xy,
                      uint8_t* d_status, float* d_err, const vo_klt_source* src = nullptr,
                      const vo_klt_batch* batch = nullptr, double fb_max = 0.0, float* d_fb = nullptr);
// (fb_max, d_fb) != (0, null): the forward-backward launch (vo_hip.h, vo_klt_track_fb); d_fb strides like d_err
int vo_pyramid_build_batch_dev(vo_ctx* ctx, const uint8_t* d_img, size_t img_stride, int S, int H, int W, int n_levels,
                               uint8_t* d_pyr, size_t pyr_stride);
// Several sequences per launch (harris.hip): S images at d_img + s * img_stride -> S score maps at d_scores + s * H * W;
// S score maps -> S keypoint lists at d_kp_xy + s * kp_stride (doubles).  S = 1 is what the C ABI's _dev forms call.
// d_go (optional, S ints on the device): sequences whose word is 0 are skipped by every kernel of the chain
int vo_harris_response_batch_dev(vo_ctx* ctx, const uint8_t* d_img, size_t img_stride, int S, int H, int W, int patch,
                                 double kappa, double* d_scores, const int* d_go = nullptr);
int vo_nms_keypoints_batch_dev(vo_ctx* ctx, const double* d_scores, int S, int H, int W, int N, int r, double* d_kp_xy,
                               size_t kp_stride, const int* d_go = nullptr);
