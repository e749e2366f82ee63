/*
 * vo_hip.h -- C ABI of libvo_hip.so, the MI355X (gfx950) implementation of the
 * per-frame visual-odometry front-end of saegsali/visual-odometry-project.
 *
 * The reference has no FFI layer: its hot path is reached through Python classes
 * (SURVEY.md section 8b).  Each entry point below replaces the arithmetic of one
 * reference call site, cited as  [ref: path:line]  relative to the reference
 * checkout; the Python package  visual-odometry-project_amd/vo  keeps the
 * reference's class/method names and binds these symbols with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - plain C: pointers, sizes, scalars.  No C++ or torch types.
 *  - return 0 (VO_OK) or a negative vo_status; text via vo_last_error().  Nothing
 *    aborts or throws across the boundary.
 *  - there is NO CPU fallback: every compute entry point runs HIP kernels on the
 *    context's device and fails with VO_EHIP if that is impossible.
 *  - "host" entry points take caller-owned host arrays (C-contiguous), copy in/out
 *    and synchronise before returning.  "_dev" entry points take DEVICE pointers,
 *    enqueue on the context's stream and return without synchronising.
 *  - a vo_ctx owns one HIP stream and a device workspace; it is not thread-safe
 *    (one context per host thread / per GPU).
 *  - keypoints are (x, y) pairs; images are row-major uint8, H rows by W columns.
 */
#ifndef VO_HIP_H
#define VO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vo_ctx vo_ctx;

typedef enum vo_status {
  VO_OK = 0,
  VO_EINVAL = -1,        /* bad argument (shape, range, null pointer)           */
  VO_ENOMEM = -2,        /* host or device allocation failed                    */
  VO_EHIP = -3,          /* HIP runtime error (no device, launch failure, ...)  */
  VO_ECAPACITY = -4,     /* an internal candidate list overflowed its capacity  */
  VO_ETRACKING = -5      /* fewer than 4 triangulated tracks survive: no pose   */
} vo_status;

/* ---- context ---------------------------------------------------------------- */

/* device: HIP ordinal.  stream: an existing hipStream_t to enqueue on (e.g. the
 * caller's torch stream), or NULL to create a private non-blocking stream.      */
int vo_create(int device, void* stream, vo_ctx** out);
void vo_destroy(vo_ctx* ctx);
const char* vo_last_error(const vo_ctx* ctx);
int vo_version(void);
int vo_sync(vo_ctx* ctx);                       /* hipStreamSynchronize           */
void* vo_stream(vo_ctx* ctx);                   /* the hipStream_t in use         */

/* Device memory helpers so a non-HIP host (ctypes) can keep inputs resident.     */
int vo_dev_alloc(vo_ctx* ctx, size_t bytes, void** out);
int vo_dev_free(vo_ctx* ctx, void* p);
int vo_dev_upload(vo_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int vo_dev_download(vo_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* Per-kernel timing with hipEvents on the context's stream.  While enabled every
 * launch of kernel `kernel_id` (VO_K_*) is bracketed by an event pair; the
 * accumulated time and launch count are read back with vo_prof_read (which
 * synchronises).  kernel_id < 0 brackets every kernel.                          */
enum {
  VO_K_HARRIS_RESPONSE = 0,
  VO_K_NMS_CANDIDATES = 1,
  VO_K_NMS_THRESHOLD = 2,
  VO_K_NMS_COMPACT = 3,
  VO_K_NMS_SELECT = 4,
  VO_K_PATCH_DESC = 5,
  VO_K_PYR_DOWN = 6,
  VO_K_KLT_TRACK = 7,
  VO_K_DLT = 8,
  VO_K_P3P_SOLVE = 9,
  VO_K_P3P_SCORE = 10,
  VO_K_REPROJ = 11,
  VO_K_MATCH = 12,
  VO_K_GATHER = 13,
  VO_K_NMS_ROUND = 14,
  VO_K_NMS_COLLECT = 15,
  VO_K_NMS_RANK = 16,
  VO_K_NMS_EMIT = 17,
  VO_K_SIFT_SCALESPACE = 18,
  VO_K_SIFT_DETECT = 19,
  VO_K_SIFT_DESCRIBE = 20,
  VO_K_REFINE = 21,
  VO_K_STATE_CANDIDATES = 22,
  VO_K_STATE_REGROUP = 23,
  VO_K_RANSAC_REPLAY = 24,
  VO_K_STATE_LANDMARKS = 25,
  VO_K_EXPORT = 26,
  VO_K_SHI_TOMASI_CHAIN = 27,   /* the frame loop's Shi-Tomasi re-detect, all of its launches (vo_pipeline_config.detector = 1) */
  VO_K_WINDOW_BA = 28,          /* vo_window_ba_dev's solver kernel */
  VO_K_WINDOW_BUILD = 29,       /* vo_window_from_tracks_dev, both of its launches */
  VO_K_TWOVIEW_HYP = 30,        /* the two-view hypothesis kernel of a call: f8_hyp_kernel or e5_hyp_kernel */
  VO_K_TWOVIEW_SCORE = 31,      /* ... and its scorer: f_score_kernel or e5_score_kernel */
  VO_K_WINDOW_STRUCTURE = 32,   /* vo_window_structure_dev, both of its launches */
  VO_K_LOOP_RECORD = 33,        /* vo_structure_loop_post: the record into the ring and its ids into the table */
  VO_K_LOOP_JOIN = 34,          /* ... the header check and the join, one workgroup per lane */
  VO_K_LOOP_WRITE = 35,         /* ... the entry and the write-back (also when it is queued again behind a redone step) */
  VO_K_BRIEF_DESCRIBE = 36,     /* vo_brief_describe_dev's kernel */
  VO_K_HAMMING_KNN2 = 37,       /* vo_hamming_knn2_dev's kernel */
  VO_K_COUNT = 38
};
int vo_prof_enable(vo_ctx* ctx, int kernel_id);
/* bracket only every n-th launch of a profiled kernel (default 1): the event pair itself costs
 * the stream a few microseconds, vo_prof_read then reports the sampled launches           */
int vo_prof_set_sampling(vo_ctx* ctx, int every);
int vo_prof_disable(vo_ctx* ctx);
int vo_prof_read(vo_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);
int vo_prof_reset(vo_ctx* ctx);
const char* vo_kernel_name(int kernel_id);

/* ---- Harris response + greedy NMS ------------------------------------------
 * [ref: src/vo/features/harris.py:99-137]  response: true-convolution Sobel ->
 * int products -> patch x patch box sums -> det - kappa*trace^2 (three IEEE
 * roundings, no FMA) -> clamp <0 -> zero border of patch/2+1.  scores: H*W
 * float64 in image coordinates, bit-identical to the reference.
 * [ref: src/vo/features/harris.py:139-152]  greedy argmax NMS, radius r,
 * including its slicing semantics.  kp_xy: N*2 float64 (x, y),
 * bit-identical to the reference's keypoints (N,2,1).
 * patch must be odd, 3..31; 0 <= r <= 32; 1 <= N <= 16384.                      */
int vo_harris_response(vo_ctx* ctx, const uint8_t* img, int H, int W, int patch,
                       double kappa, double* scores);
int vo_harris_keypoints(vo_ctx* ctx, const uint8_t* img, int H, int W, int patch,
                        double kappa, int N, int r, double* kp_xy,
                        double* scores /* nullable */);
int vo_nms_keypoints(vo_ctx* ctx, const double* scores, int H, int W, int N, int r,
                     double* kp_xy);
/* The detector on S frames of one size in one set of launches (the sequence is the grid's extra dimension: several
 * sequences per GPU advance together).  imgs: S*H*W bytes; kp_xy: S*N*2; scores: S*H*W or NULL.
 * Results are those of S calls of vo_harris_keypoints.                                                     */
int vo_harris_keypoints_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, int patch, double kappa, int N,
                              int r, double* kp_xy, double* scores /* nullable */);
int vo_harris_response_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, int patch,
                           double kappa, double* d_scores);
int vo_nms_keypoints_dev(vo_ctx* ctx, const double* d_scores, int H, int W, int N,
                         int r, double* d_kp_xy);

/* [ref: src/vo/features/harris.py:160-194]  raw (2r+1)^2 patches of the
 * zero-padded image, row-major, as float64.  desc: N*(2r+1)^2.                  */
int vo_patch_descriptors(vo_ctx* ctx, const uint8_t* img, int H, int W,
                         const double* kp_xy, int N, int r, double* desc);
int vo_patch_descriptors_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W,
                             const double* d_kp_xy, int N, int r, double* d_desc);

/* ---- pyramidal KLT -----------------------------------------------------------
 * [ref: src/vo/features/klt.py:233-249]  cv2.calcOpticalFlowPyrLK(prev, next,
 * prevPts, None, winSize=(win,win), maxLevel=max_level, criteria=(EPS|COUNT,
 * max_iter, eps)), default minEigThreshold = 1e-4, flags = 0.  Outputs as OpenCV:
 * next_xy N*2 float32, status N uint8, err N float32 (mean |patch diff| / 32).
 * Pyramid level l+1 is ((H+1)/2, (W+1)/2); the number of levels actually used is
 * vo_klt_num_levels (the builder stops when a level is not larger than the
 * window).  The _dev form takes the images and, for each, the buffer that
 * vo_pyramid_build_dev filled (vo_pyramid_bytes): an opaque layout holding every
 * level, level 0 included, with a reflect-101 border so the tracker's blocks are
 * plain in-bounds reads.  The tracker reads the levels from those buffers only. */
int vo_klt_num_levels(int H, int W, int win, int max_level);
size_t vo_pyramid_bytes(int H, int W, int n_levels);
int vo_pyr_down(vo_ctx* ctx, const uint8_t* img, int H, int W, uint8_t* out);
int vo_pyramid_build_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, int n_levels,
                         uint8_t* d_pyr);
int vo_klt_track(vo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int H, int W,
                 const float* prev_xy, int N, int win, int max_level, int max_iter,
                 double eps, double min_eig, float* next_xy, uint8_t* status, float* err);
int vo_klt_track_dev(vo_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_prev_pyr,
                     const uint8_t* d_next, const uint8_t* d_next_pyr, int H, int W,
                     int n_levels, const float* d_prev_xy, int N, int win, int max_iter,
                     double eps, double min_eig, float* d_next_xy, uint8_t* d_status,
                     float* d_err);

/* Forward-backward consistency check (opt-in; the calls above are untouched by it).
 * Inputs are those of vo_klt_track plus fb_max in pixels: fb_max > 0, +inf allowed;
 * a NaN or a value <= 0 returns VO_EINVAL with a message and writes nothing.
 *   1. Forward.   (next_xy, status_f, err) is exactly what vo_klt_track(prev, next,
 *      prev_xy, ...) returns; next_xy and err are returned unchanged, bit for bit,
 *      for every point.
 *   2. Backward.  Only for points with status_f = 1: the same tracker, same win,
 *      levels, criteria and min_eig, with the images exchanged, starting from the
 *      float32 next_xy[i] as stored, gives (back_xy, status_b).  The backward err is
 *      not used.
 *   3. Distance.  fb[i] = dx*dx + dy*dy with dx = back_x - prev_x, dy = back_y -
 *      prev_y: float32 arithmetic in that order, no contraction, in px^2.
 *      fb[i] = +inf where status_f = 0 or status_b = 0.
 *   4. Status.    status[i] = status_f & status_b & (fb[i] <= thr2), thr2 =
 *      (float)(fb_max * fb_max), the product formed in double.  A tie is kept.
 * By construction the result equals two vo_klt_track calls and a compare.  One
 * launch does both passes: the lanes that tracked a point forward keep it in
 * registers and run the level loop again with the pyramids exchanged.  fb: N float32.
 * In the frame pipeline the check is vo_pipeline_set_klt_fb; the pipeline's two-view
 * bootstrap (vo_pipeline_bootstrap_seq) keeps the plain tracker -- out of scope.   */
int vo_klt_track_fb(vo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int H, int W,
                    const float* prev_xy, int N, int win, int max_level, int max_iter,
                    double eps, double min_eig, double fb_max, float* next_xy,
                    uint8_t* status, float* err, float* fb);
int vo_klt_track_fb_dev(vo_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_prev_pyr,
                        const uint8_t* d_next, const uint8_t* d_next_pyr, int H, int W,
                        int n_levels, const float* d_prev_xy, int N, int win, int max_iter,
                        double eps, double min_eig, double fb_max, float* d_next_xy,
                        uint8_t* d_status, float* d_err, float* d_fb);

/* ---- DLT triangulation --------------------------------------------------------
 * [ref: src/vo/landmarks/triangulation.py:352-389, 38-86; src/vo/helpers.py:57-83]
 * per point A = [[x1]_x C1 ; [x2]_x C2] (6x4), smallest right singular vector,
 * de-homogenised.  x1, x2: n*2 pixels; C1: 3x4 row-major, or n of them when
 * c1_per_point != 0 (triangulate_candidates); C2: 3x4; X: n*3.                  */
int vo_triangulate_dlt(vo_ctx* ctx, const double* x1, const double* x2, int n,
                       const double* C1, int c1_per_point, const double* C2, double* X);
int vo_triangulate_dlt_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int n,
                           const double* d_C1, int c1_per_point, const double* d_C2,
                           double* d_X);

/* ---- two-view bootstrap ----------------------------------------------------------
 * [ref: src/vo/landmarks/triangulation.py:110-350, src/vo/helpers.py:31-54; called once per sequence, src/main.py:204-230]
 * vo_fundamental_hypotheses: the model_fn / error_fn pair of _find_fundamental_matrix_ransac (:134-145) for Hyp samples
 *   at once -- samples: Hyp*8 indices into the N correspondences p1, p2 (N*2 each; the reference hands the loop
 *   Hartley-normalised points, :147-149).  Per sample: Kronecker rows (:203-205), null vector of the 8x9 system
 *   (:209-212), rank-2 projection (:214-217) -> F Hyp*9 row-major.  normalize_samples != 0: the sample's own Hartley
 *   normalisation around the fit (_find_fundamental_matrix(is_normalized=False), :195-198, :220-221).  error_kind 0:
 *   (p2^T F p1)^2 (:140-145); 1: the larger squared distance to the epipolar lines of the two images.  inlier =
 *   error < threshold (src/vo/algorithms/ransac.py:104-106); counts Hyp, masks Hyp*ceil(N/64) words (nullable).
 *   The sequential accept / adapt rule over (counts) is vo_ransac_replay's (every sample has a model: valid = 1).
 * vo_fundamental_fit: _find_fundamental_matrix (:165-222) over the correspondences whose mask byte is set (NULL: all):
 *   what RANSAC's closing model_fn(population[inliers]) computes (ransac.py:123-127).  normalize as above.  The null
 *   vector of the N x 9 system is the smallest eigenvector of Q^T Q; where lambda8 < 1e-5 lambda1 (small baselines,
 *   near-planar scenes) a second pass over the points takes the smallest eigenvector of (Q V)^T (Q V) for V the
 *   eigenvectors of the first -- nearly diagonal -- which corrects what squaring Q's conditioning cost.
 *   All three entry points and vo_triangulate_dlt are pinned to 50-digit values (tests/twoview_cases.py): the fit to
 *   2.5e-10 of the unit-norm F where sigma8 / sigma1 of Q is 1e-5, to 4e-13 and better on ordinary scenes.
 * vo_essential_decompose: _decompose_essential_matrix (:245-277): E 3x3 -> M4 4*12, [R_j | (-1)^i T] at index 2i+j.
 *   The four candidates are the reference's set; which of the two rotations is "R_0" and which sign of T comes first
 *   depends on the signs the SVD routine picks (LAPACK's in the reference) and may differ.
 * vo_relative_pose: _find_relative_pose (:279-350) given F: E = K2^T F K1, the four candidates, the cheirality votes
 *   over the correspondences whose inliers byte is set (NULL: all) by DLT against K1 [I|0] (:313-332, strict `>`),
 *   the winner's triangulation of ALL N correspondences -> M 12 (3x4), X N*3 (frame 1), mask_out N (nullable):
 *   inliers & in front of both cameras (:341-348), M4 48 (nullable).                                              */
int vo_fundamental_hypotheses(vo_ctx* ctx, const double* p1, const double* p2, int N, const int32_t* samples, int Hyp,
                              int normalize_samples, int error_kind, double threshold, double* F, int32_t* counts,
                              uint64_t* masks);
int vo_fundamental_fit(vo_ctx* ctx, const double* p1, const double* p2, int N, const uint8_t* mask, int normalize,
                       double* F);
int vo_essential_decompose(vo_ctx* ctx, const double* E, double* M4);
int vo_relative_pose(vo_ctx* ctx, const double* x1, const double* x2, int N, const uint8_t* inliers, const double* K1,
                     const double* K2, const double* F, double* M, double* X, uint8_t* mask_out, double* M4);

/* ---- P3P hypotheses + reprojection scoring -------------------------------------
 * [ref: src/vo/pose_estimation/p3p.py:51-79]   model_fn: cv2.solvePnP(P3P) on the 4
 *       sampled correspondences -> (R, t) world->camera, or None
 * [ref: src/vo/pose_estimation/p3p.py:81-108]  error_fn: squared reprojection error
 * [ref: src/vo/algorithms/ransac.py:104-106]   inliers = error < thr (strict); count
 * X: N*3 landmarks, x: N*2 pixels, K: 3x3 row-major (HOST pointer in both forms),
 * samples: Hyp*4 indices into the N correspondences.  Outputs per hypothesis:
 * R Hyp*9, t Hyp*3, valid Hyp (0 = the reference's "model is None"), counts Hyp,
 * masks Hyp*ceil(N/64) 64-bit words (bit i%64 of word i/64 = point i is an inlier;
 * nullable).  vo_reproj_inliers scores one pose: mask N bytes and/or err N.     */
int vo_p3p_hypotheses(vo_ctx* ctx, const double* X, const double* x, int N, const double* K,
                      const int32_t* samples, int Hyp, double thr_sq, double* R, double* t,
                      uint8_t* valid, int32_t* counts, uint64_t* masks);
int vo_p3p_hypotheses_dev(vo_ctx* ctx, const double* d_X, const double* d_x, int N,
                          const double* K, const int32_t* d_samples, int Hyp, double thr_sq,
                          double* d_R, double* d_t, uint8_t* d_valid, int32_t* d_counts,
                          uint64_t* d_masks);
int vo_reproj_inliers(vo_ctx* ctx, const double* X, const double* x, int N, const double* K,
                      const double* R, const double* t, double thr_sq, uint8_t* mask,
                      double* err);
int vo_reproj_inliers_dev(vo_ctx* ctx, const double* d_X, const double* d_x, int N,
                          const double* K, const double* d_Rt, double thr_sq,
                          uint8_t* d_mask, double* d_err);
/* The frame loop's hypothesis kernel takes the decision `error < thr_sq` (ransac.py:104-106) on the sum of squares
 * s, where error = fl(fl(sqrt(s))^2) is what error_fn computes (p3p.py:81-108: norm, then square):
 * vo_inlier_sum_sq_limit returns the largest double s whose error is below thr_sq (-1: there is none), and
 * `s <= limit` is the same decision because rounding and sqrt are monotone.  Host arithmetic only.          */
double vo_inlier_sum_sq_limit(double thr_sq);

/* ---- pose refinement --------------------------------------------------------------
 * [ref: src/vo/pose_estimation/p3p.py:188-213 _nonlinear_refinement; helpers.py:86-142]
 * Minimises sum_i |x_i - proj(K, R X_i + t)|^2 over the pose, from (R0, t0), over the points
 * whose mask byte is non-zero (all points if the mask is NULL) -- the objective the reference
 * hands to scipy.optimize.least_squares.  Gauss-Newton on the left-multiplied increment with
 * the analytic Jacobian, at most max_iter (<= 100) accepted steps, fp64; converges to the
 * minimiser itself (SciPy's default tolerances stop within ~1e-4 of it).  Outputs R (9,
 * row-major), t (3), the number of accepted steps and the final cost (sum of squared pixel
 * errors).  The _dev form takes Rt0 = R0 then t0 (12 doubles) and writes 14 doubles:
 * R, t, iterations, cost.
 *
 * The rule (tests/refine_reference.py states it in NumPy; the stand-alone kernel and the frame loop's pose kernel
 * share one routine):
 *   cost    e_i = x_i - proj(K, R X_i + t) over the active points (mask byte != 0; every non-zero byte means the
 *           same; the coordinates of the others are never used);  cost = sum_i |e_i|^2.  No cheirality test: a point
 *           behind the camera counts with its (finite) residual.
 *   rows    with p = R X + t, a = fx / p_z, b = fy / p_z, c = -fx p_x / p_z^2, d = -fy p_y / p_z^2 the rows of
 *           J = d proj / d (v, w) are  [a 0 c  c p_y  a p_z - c p_x  -a p_y]  and  [0 b d  d p_y - b p_z  -d p_x  b p_x].
 *   sums    28 of them over the active points: the 21 entries of the upper triangle of A = sum J^T J (the entry (0,1) is
 *           zero), the 6 of g = sum J^T e, and the cost.  Their order of summation is not part of the rule.
 *   solve   A d = g by Gauss-Jordan elimination without pivoting, in the order of the rows; a pivot that is not
 *           positive (NaN included) refuses the solve and ends the refinement with the pose it has.
 *   step    d = (v, w):  T <- [Exp(w) | v] T,  i.e.  R <- E R,  t <- E t + v  with  E = I + A [w]x + B [w]x^2,
 *           A = sin(th) / th, B = (1 - cos th) / th^2, th = |w|;  for th^2 < 1/16 both by their series in th^2 through
 *           th^16 (nested, 1 - th^2/6 (1 - th^2/20 (...)) and 1/2 (1 - th^2/12 (1 - th^2/30 (...)))), sin and cos otherwise.
 *   order   the start pose is evaluated.  Then, repeatedly: `max_iter` accepted steps -> stop;  solve (refused -> stop);
 *           the trial pose is formed and the step tested, |d| <= 1e-9 (1 + |t_trial|) -> stop, the step is neither taken
 *           nor evaluated;  the trial is evaluated;  unless cost_new <= cost -> stop, the previous pose and its cost stay
 *           (a NaN cost rejects);  the trial is accepted and counted;  cost - cost_new <= 1e-16 cost -> stop.
 *   result  the pose of the last accepted step (the start if none), the number of accepted steps, and the cost of
 *           exactly that pose.
 *   fewer than three active points (N = 0 and an all-zero mask included), or a start cost that is not finite: the pose
 *           is returned unchanged bit for bit, iterations = 0, and the cost is the cost of the active points at the start
 *           (0 for none, the non-finite value otherwise).                                                            */
int vo_refine_pose(vo_ctx* ctx, const double* X, const double* x, int N, const double* K,
                   const uint8_t* inlier_mask, const double* R0, const double* t0, int max_iter,
                   double* R, double* t, int32_t* iterations, double* cost);
int vo_refine_pose_dev(vo_ctx* ctx, const double* d_X, const double* d_x, int N, const double* K,
                       const uint8_t* d_mask, const double* d_Rt0, int max_iter, double* d_out14);

/* ---- descriptor matching ---------------------------------------------------------
 * [ref: src/vo/features/harris.py:246-262, src/vo/features/sift.py:38-54]
 * cv2.BFMatcher().knnMatch(q, t, k=2) + ratio test + first-come uniqueness on the train
 * index, queries in order.  q: nq*D, t: nt*D float32; pairs: up to nq (query, train)
 * rows; n_pairs: rows written.  Distances are exact for integer-valued descriptors.   */
int vo_match_knn2_ratio(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int D,
                        double ratio, int32_t* pairs, int32_t* n_pairs);
int vo_knn2_dev(vo_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int D,
                int32_t* d_best, double* d_d2);
/* The two nearest neighbours themselves, before the ratio test
 * [ref: src/vo/features/harris.py:246-249, src/vo/features/sift.py:38-44: the (m, n) pairs knnMatch returns].
 * Host pointers, like vo_match_knn2_ratio, and the same choice of kernel: best: nq*2 train
 * indices (nearest, second nearest; -1 where absent), d2: nq*2 squared distances as float64
 * (0.0 where absent), ordered by (squared distance, train index).  *path: the kernel whose
 * result was kept -- VO_MATCH_PATH_FLOAT (float64 accumulation in index order),
 * VO_MATCH_PATH_BYTE_DOT (packed byte dot product) or VO_MATCH_PATH_MFMA (matrix cores,
 * D = 128 or 361); -1 when nq or nt is 0 and no kernel ran.  vo_match_last_path: the same
 * for the context's last vo_match_knn2_ratio / vo_match_knn2 call.                      */
enum { VO_MATCH_PATH_FLOAT = 0, VO_MATCH_PATH_BYTE_DOT = 1, VO_MATCH_PATH_MFMA = 2 };
int vo_match_knn2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int D,
                  int32_t* best, double* d2, int* path);
int vo_match_last_path(vo_ctx* ctx);

/* ---- BRIEF-256 binary descriptors and Hamming matching (brief.hip) --------------------
 * The project's own definition, in the spirit of ORB's rBRIEF (it is not OpenCV's pattern; the reference has no binary
 * descriptor).  Everything is integer arithmetic except the centre and the ratio test's one multiply, so the kernels
 * equal tests/brief_reference.py bit for bit on every input.
 *   image    uint8 H x W, zero outside (as vo_patch_descriptors): rows stay index-aligned with the keypoints, no
 *            keypoint is dropped.
 *   centre   cx = floor(x + 0.5), cy = floor(y + 0.5) in float64, (x, y) as in kp_xy of vo_harris_keypoints.  A
 *            non-finite coordinate, or a centre outside [-16, W + 16) x [-16, H + 16), gives an all-zero descriptor
 *            and bin 0.
 *   S(y, x)  the sum of I over the 5 x 5 box centred on (y, x): an integer, at most 6375.
 *   pattern  256 pairs (a_i, b_i) of integer offsets inside the disc of radius 13, a_i != b_i, no pair twice, drawn by
 *            np.random.default_rng(VO_BRIEF_SEED) from an isotropic Gaussian of sigma = 13 / 2 with rejection, and 30
 *            rotated tables: table k turns every offset by 12 k degrees and rounds half away from zero in float64.
 *            tools/make_brief_pattern.py draws them (its header lists every rejection rule), asserts that no rotated
 *            coordinate lies within 1e-9 of a rounding boundary and that every rotated offset stays within radius 14
 *            (so a descriptor reads at most 16 pixels from its centre), and writes csrc/brief_pattern.h.
 *   bits     bit i = 1 iff S(c + a_i^k) < S(c + b_i^k), k the keypoint's bin (0 when not oriented); bit i is stored
 *            in byte i / 8 at position i % 8, least significant first.  A descriptor is 32 bytes.
 *   bin      (oriented = 1) on the raw image: m10 = sum dx I, m01 = sum dy I over dx^2 + dy^2 <= 15^2;
 *            k = argmax_k (m10 C[k] + m01 Sn[k]) in int64, C[k] = round(16384 cos(2 pi k / 30)), Sn[k] likewise for
 *            sin (both in csrc/brief_pattern.h); ties go to the lowest k, so a flat patch has bin 0.
 * vo_brief_describe: host pointers; kp_xy N x 2 float64, desc N x 32 bytes, bin N bytes or NULL (the bins; all 0 when
 * oriented = 0); 1 <= N <= 16384, oriented 0 or 1.  vo_brief_describe_dev: device pointers, enqueued on the context's
 * stream, neither synchronises nor reads back.  vo_brief_pattern: the 30 x 256 x 4 table (ax, ay, bx, by) the library
 * was built with.  A refused call returns VO_EINVAL with a message and writes nothing.                              */
int vo_brief_describe(vo_ctx* ctx, const uint8_t* img, int H, int W, const double* kp_xy, int N, int oriented,
                      uint8_t* desc, uint8_t* bin /* nullable */);
int vo_brief_describe_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, const double* d_kp_xy, int N, int oriented,
                          uint8_t* d_desc, uint8_t* d_bin /* nullable */);
int vo_brief_pattern(int8_t* out);
/* Hamming 2-NN.  Rows of row_bytes bytes, row_bytes a multiple of 4 in 4 .. 64.  For every query the two train rows
 * smallest under the total order (distance, train index): best nq x 2 train indices, dist nq x 2 distances, both int32;
 * an absent neighbour is -1 with distance 0, as vo_match_knn2 has it.  vo_match_hamming_knn2: host pointers, nq and nt
 * may be 0.  vo_hamming_knn2_dev: device pointers on a 4-byte boundary, nq >= 1, nt >= 0, enqueued on the context's
 * stream without synchronising.
 * vo_match_hamming_ratio: the pair list.  Queries are taken in order; query q gives (q, best) iff nt >= 2,
 * float64(d1) < ratio * float64(d2) with one IEEE multiply, d1 <= max_dist when max_dist >= 0, and best was not taken by
 * an earlier query that met the same three conditions -- the first-come rule of vo_match_knn2_ratio.  pairs: up to nq
 * (query, train) rows; n_pairs: rows written.                                                                       */
int vo_match_hamming_knn2(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int row_bytes,
                          int32_t* best, int32_t* dist);
int vo_hamming_knn2_dev(vo_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int row_bytes,
                        int32_t* d_best, int32_t* d_dist);
int vo_match_hamming_ratio(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int row_bytes,
                           double ratio, int max_dist, int32_t* pairs, int32_t* n_pairs);
/* The batch forms the frame pipeline's FAST + BRIEF tracker mode is made of: device pointers only, every count in device
 * memory, enqueued on the context's stream; neither synchronises nor reads anything back.  The one-image entry points
 * above launch the same kernels with S = 1.
 * vo_brief_describe_batch_dev: image q at d_imgs + q * img_stride, its keypoints at d_kp_xy + q * xy_stride * 2 (the
 * layout vo_fast_keypoints_batch_dev writes), its count in d_n[q]; rows 0 .. min(max(d_n[q], 0), N) - 1 are described into
 * d_desc + q * desc_stride (bytes), their bins into d_bin + q * xy_stride (nullable).  Rows at and beyond the count are
 * not written.  VO_EINVAL: a null pointer, S outside 1 .. 65535, N outside 1 .. 16384, img_stride < H W, xy_stride < N,
 * desc_stride < 32 N.
 * vo_match_hamming_batch_dev: vo_match_hamming_ratio's rule for S sequences, arguments as the pipeline's other matcher
 * takes them: sequence z's queries at d_q + z * q_stride (bytes), their number at d_nq[z * nq_stride] (ints; it may be a
 * field of an array of structures), train rows and count likewise; a count is clamped to 0 .. cap.  Its pairs go to
 * d_pairs + z * cap_q * 2 (query, train; query order), their number to d_npairs[z]; rows of d_pairs at and beyond that
 * number are not written, rows of d_q / d_t at and beyond a count never read.  The workspace (2-NN lists and one owner
 * table per sequence) belongs to the context and grows with the largest call.  VO_EINVAL: a null pointer, row_bytes
 * not a multiple of 4 in 4 .. 64, rows or strides off a 4-byte boundary, a capacity < 1, S outside 1 .. 65535, S > 1
 * with blocks that overlap or a count stride of 0, ratio NaN.                                                       */
int vo_brief_describe_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                                const double* d_kp_xy, size_t xy_stride /* rows */, const int32_t* d_n /* S counts */,
                                int N /* rows launched per image */, int oriented, uint8_t* d_desc,
                                size_t desc_stride /* bytes */, uint8_t* d_bin /* nullable */);
int vo_match_hamming_batch_dev(vo_ctx* ctx, const uint8_t* d_q, size_t q_stride, const int32_t* d_nq, int nq_stride /* ints */,
                               int cap_q, const uint8_t* d_t, size_t t_stride, const int32_t* d_nt, int nt_stride, int cap_t,
                               int S, int row_bytes, double ratio, int max_dist, int32_t* d_pairs /* S x cap_q x 2 */,
                               int32_t* d_npairs /* S */);

/* ---- FAST-9 corners (fast.hip) ------------------------------------------------------------
 * The project's own definition, in the spirit of Rosten's FAST-9/16 segment test (the reference has no such detector, and
 * nothing is compared against OpenCV's).  Everything is integer arithmetic, so the kernels equal tests/fast_reference.py
 * bit for bit on every input, with no margins.
 *   circle   radius 3, sixteen offsets (dx, dy) clockwise from the top, c_0 .. c_15:
 *            (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3)
 *   score    for p = (x, y) with 3 <= x < W - 3 and 3 <= y < H - 3, I the centre byte, all arithmetic int32:
 *              s(p) = max over k = 0..15 of max( min_{j=0..8} (c_{(k+j) mod 16} - I), min_{j=0..8} (I - c_{(k+j) mod 16}) )
 *            -- nine contiguous circle pixels, the wrap included.  p is a corner iff s(p) > threshold, 0 <= threshold <=
 *            254: exactly "nine contiguous pixels all brighter than I + threshold, or all darker than I - threshold",
 *            strict.  The score map is H x W uint8: s(p) for a corner (1 .. 255), 0 otherwise and on the border of 3.  An
 *            image with H < 7 or W < 7 has an all-zero map and no corners: a result, not an error.
 *   nonmax   (nonmax = 1) with index = y W + x, a corner survives iff none of its eight neighbours is a corner that beats
 *            it: one of higher score, or of the same score and lower index.  A local maximum under a total order, decided
 *            from the map alone and not a greedy walk: of a plateau a a a in one row only the first survives, although
 *            the second, which suppresses the third, is itself suppressed.  Two survivors are never adjacent, so they
 *            number at most ceil((H-6)/2) ceil((W-6)/2).  nonmax = 0: every corner survives.
 *   cut      n = min(N, survivors), 1 <= N <= 16384; the n survivors first in the order (score descending, index
 *            ascending).  kp_xy: n rows of float64 (x, y), integer-valued -- the layout vo_harris_keypoints writes and
 *            vo_brief_describe_dev reads; kp_score (nullable): their n scores; total (nullable): the survivors before the
 *            cut.  Rows at and beyond n are not written.
 * vo_fast_score: the map, host arrays.  vo_fast_keypoints: one image, host arrays; vo_fast_keypoints_batch: S images of
 * one size, kp_xy S blocks of N rows, kp_score (nullable) S blocks of N bytes, n S counts.  All three upload, run the
 * stages of the _dev form (S = 1 for one image) and download.
 * vo_fast_keypoints_batch_dev: device pointers; enqueues a fixed launch sequence on the context's stream and neither
 * synchronises nor reads anything back.  Image q at d_imgs + q * img_stride, its rows at d_kp_xy + q * xy_stride * 2
 * (xy_stride rows, at least N), its scores at d_kp_score + q * xy_stride (nullable), its count in d_n[q], its survivors
 * before the cut in d_total[q] (nullable).  The workspace (two H x W byte maps, two words per image row, N indices and scores
 * and a control block per image) belongs to the context and grows with the largest call; no list of survivors is kept,
 * so there is no capacity to exceed.
 * VO_EINVAL, with the context usable afterwards and nothing written: a null pointer (but the nullable ones), H or W < 1,
 * H W >= 2^31, threshold outside 0 .. 254, nonmax other than 0 or 1, N outside 1 .. 16384, S outside 1 .. 65535,
 * img_stride < H W, xy_stride < N.                                                                                   */
int vo_fast_score(vo_ctx* ctx, const uint8_t* img, int H, int W, int threshold, uint8_t* score);
int vo_fast_keypoints(vo_ctx* ctx, const uint8_t* img, int H, int W, int threshold, int nonmax, int N, double* kp_xy,
                      uint8_t* kp_score /* nullable */, int32_t* n);
int vo_fast_keypoints_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, int threshold, int nonmax, int N,
                            double* kp_xy /* S N 2 */, uint8_t* kp_score /* S N, nullable */, int32_t* n /* S */);
int vo_fast_keypoints_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, int threshold,
                                int nonmax, int N, double* d_kp_xy, size_t xy_stride /* rows, >= N */,
                                uint8_t* d_kp_score /* nullable */, int32_t* d_n, int32_t* d_total /* nullable */);

/* ---- Shi-Tomasi corners -----------------------------------------------------------
 * [ref: src/vo/features/klt.py:98]  cv2.goodFeaturesToTrack(img, mask, maxCorners,
 * qualityLevel, minDistance, blockSize).  xy: vo_good_features_capacity(H, W, max_corners)
 * rows of 2 float32 -- max_corners, or (H*W+3)/4 + 64 when max_corners <= 0; n: corners
 * found.  vo_min_eigen_map exposes the H*W float32 map.  All stages run on the device:
 * eigenvalue map, thresholded 3x3 maxima, descending order (value, then address) and the
 * greedy minimum-distance rule over OpenCV's cell grid, as parallel rounds over all
 * candidates (one launch per round) or, where those cannot take the image, as one
 * workgroup's walk: the stages of vo_good_features_batch_dev below for one image.
 *
 * The rule in full (tests/good_features_reference.py states it in exact integers and float64;
 * oracle/csrc/goodfeatures.c and the kernels are held to it):
 *   gradients  gx = [-1 0 1; -2 0 2; -1 0 1] and gy = its transpose, as a correlation on the
 *              uint8 image, border reflect-101 (.. 2 1 | 0 1 2 ..); integers, |g| <= 1020.
 *   sums       Sxx, Sxy, Syy = sums of gx gx, gx gy, gy gy over the block x block box at offsets
 *              -(block/2) .. block - 1 - block/2 in x and in y (an even box reaches one pixel
 *              further up and left than down and right); outside the image the product images
 *              are reflected, reflect-101, as often as it takes (a box wider than the image
 *              passes both edges repeatedly; a side of 1 has one pixel).  Exact integers,
 *              block in 1..31.  (OpenCV sums the scaled products in float32 in its own order:
 *              the one documented difference.)
 *   scale      s = 1 / (4 * block * 255); s2 = (float)(s * s), the product made in double.
 *   value      float32, every operation rounded once, no contraction:
 *                a = (float)Sxx * s2 * 0.5f;  b = (float)Sxy * s2;  c = (float)Syy * s2 * 0.5f;
 *                eig = (a + c) - sqrtf((a - c) * (a - c) + b * b)
 *              the smaller eigenvalue of s^2 [Sxx Sxy; Sxy Syy], within 10 * 2^-24 * (a + c) of
 *              it (first order; the error goes with the trace, not with the eigenvalue), and
 *              exactly 0 where the sums are 0.  It may be negative by that much on an edge.
 *   threshold  m = the largest eig over the pixels with mask != 0 (all of them without a mask,
 *              border pixels included); thr = (float)((double)m * quality).  No allowed pixel:
 *              no corner.  quality > 0.
 *   keep       a pixel is a candidate when all five hold: eig > thr; eig != 0; mask != 0 there;
 *              it lies in rows 1..H-2 and columns 1..W-2; eig equals the largest value of its
 *              3x3 neighbourhood after values <= thr are replaced by 0 (forbidden and border
 *              neighbours count; tied neighbours are all kept).
 *   order      eig descending; equal values: the higher address y * W + x first.
 *   distance   in that order a candidate is accepted unless an already accepted corner has
 *              dx*dx + dy*dy < min_dist * min_dist (double; a corner exactly min_dist away is
 *              kept).  The test is made only when min_dist >= 1: below that (0 included) every
 *              candidate is accepted.
 *   limit      the first max_corners accepted corners; max_corners <= 0: all of them.
 *   output     (x, y) as float32 whole numbers, in the order of acceptance.                 */
int vo_good_features(vo_ctx* ctx, const uint8_t* img, int H, int W, const uint8_t* mask,
                     int max_corners, double quality, double min_dist, int block, float* xy,
                     int32_t* n);
int vo_min_eigen_map(vo_ctx* ctx, const uint8_t* img, int H, int W, int block, float* eig);
/* S images of one size per set of launches [ref: src/vo/features/klt.py:98, one call per
 * image there].  Image q's corners are those of vo_good_features on image q alone, bit for
 * bit and in order.  The _dev form enqueues a fixed launch sequence on the context's stream
 * and neither synchronises nor reads anything back: image q at d_imgs + q * img_stride, its
 * mask at d_masks + q * mask_stride (d_masks NULL: none), its corners at d_xy + q *
 * xy_stride * 2 (xy_stride rows, at least vo_good_features_capacity(H, W, max_corners)),
 * their number in d_n[q].  d_over[q] (nullable): 0 ok, 1 the local maxima exceed the
 * candidate capacity (H*W/4 + 64), 2 the minimum-distance walk's cell slots overflowed; when
 * it is non-zero d_n[q] = 0 and nothing of image q is written, the other images are as
 * without it.  d_info (nullable) receives four words per image: candidates, path (0 the
 * parallel rounds, 1 the one-workgroup walk, 2 min_dist < 1: the sorted list's head), round
 * launches used, reserved.  vo_good_features_batch uploads, calls the _dev form and
 * downloads (xy: S blocks of capacity rows); a non-zero d_over[q] is VO_ECAPACITY naming q.
 * Argument rules as for vo_good_features; a refused call leaves the context usable.        */
int vo_good_features_capacity(int H, int W, int max_corners);
int vo_good_features_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                               const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality,
                               double min_dist, int block, float* d_xy, size_t xy_stride, int32_t* d_n,
                               int32_t* d_over, int32_t* d_info);
int vo_good_features_batch(vo_ctx* ctx, const uint8_t* imgs, const uint8_t* masks, int S, int H, int W,
                           int max_corners, double quality, double min_dist, int block, float* xy, int32_t* n);

/* ---- SIFT ---------------------------------------------------------------------------
 * [ref: src/vo/features/sift.py:10,17]  cv2.SIFT_create().detectAndCompute(image, None)
 * with OpenCV's defaults (3 layers/octave, contrast 0.04, edge 10, sigma 1.6, image
 * doubled first).  kp: cap*6 float32 (x, y, size, angle, response, octave) in image
 * coordinates, ordered as KeyPointsFilter::removeDuplicatedSorted leaves them; desc:
 * cap*128 float32 (integer-valued 0..255).  If more than `cap` keypoints are found the
 * `cap` strongest by response are kept (KeyPointsFilter::retainBest).  cap <= 0: keep every
 * keypoint, as the reference does (nfeatures = 0); kp / desc must then hold
 * vo_sift_capacity(H, W) rows, the library's own list capacity for that image size --
 * more keypoints than that is VO_ECAPACITY, never a silent truncation.                  */
int vo_sift_capacity(int H, int W);
int vo_sift(vo_ctx* ctx, const uint8_t* img, int H, int W, int cap, float* kp, float* desc,
            int32_t* n);
/* The same with the frame and the results in device memory, enqueued on the context's stream (no synchronisation):
 * d_kp cap*6 float32, d_desc cap*128 float32 and / or d_desc_u8 cap*128 bytes (the descriptor values are whole numbers
 * 0..255; either may be NULL), d_n one int32.  1 <= cap <= 4000: the final order, the duplicate filter and the cap run
 * on the device too (one workgroup sorts the cap + ties described rows).                                          */
int vo_sift_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, int cap, float* d_kp, float* d_desc, uint8_t* d_desc_u8,
                int32_t* d_n);
/* [ref: src/vo/features/sift.py:10,17]  detectAndCompute on S images of one size in one set of launches (the image is
 * the grid's extra dimension; every image has its own scale space, lists and counters).  Image q's results are those of
 * vo_sift_dev / vo_sift on that image alone, bit for bit.  _dev: image q at d_imgs + q * img_stride bytes; its keypoints
 * at d_kp + q * kp_stride * 6, its descriptors at d_desc / d_desc_u8 + q * desc_stride * 128 (either may be NULL), its
 * count in d_n[q]; d_over[q] = 1 when image q's candidate / keypoint lists overflowed (d_over may be NULL).
 * vo_sift_batch: as vo_sift per image, imgs S*H*W; image q's rows at kp + q * R * 6, desc + q * R * 128 with R = cap,
 * or R = vo_sift_capacity(H, W) when cap <= 0; an overflow in any image is VO_ECAPACITY naming the image.  Device
 * memory grows linearly in S (about 295 MB per 1376x1241 image).                                                     */
/* S images of one size; results are those of S calls of vo_sift_dev / vo_sift. */
int vo_sift_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride /* bytes, >= H*W */, int S, int H, int W,
                      int cap /* 1..4000 */, float* d_kp, size_t kp_stride /* rows, >= cap */, float* d_desc,
                      uint8_t* d_desc_u8, size_t desc_stride /* rows, >= cap */, int32_t* d_n /* S */,
                      int32_t* d_over /* S, nullable: 1 = candidate / keypoint list overflow */);
int vo_sift_batch(vo_ctx* ctx, const uint8_t* imgs /* S*H*W */, int S, int H, int W, int cap, float* kp, float* desc,
                  int32_t* n /* S */);
/* [ref: src/vo/features/sift.py:10,17]  cv2.SIFT_create() (nfeatures = 0: every keypoint) .detectAndCompute on S images of
 * one size with the final order made on the device for any count: image q's keypoints are those of vo_sift(cap <= 0) on
 * that image alone, in its order, bit for bit.  Layout as vo_sift_batch_dev with `rows` output rows per image
 * (1 <= rows <= vo_sift_capacity(H, W)).  d_over[q] = 0: image q succeeded; 1: its candidate / keypoint lists
 * overflowed; 2: it has more than `rows` keypoints.  When d_over[q] != 0, d_n[q] = 0 and nothing of image q is written
 * (never a truncated list).  Counts stay on the device: a fixed launch sequence, no host synchronisation.            */
int vo_sift_all_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride /* bytes, >= H*W */, int S, int H, int W,
                          int rows, float* d_kp, size_t kp_stride /* rows, >= rows */, float* d_desc, uint8_t* d_desc_u8,
                          size_t desc_stride /* rows, >= rows */, int32_t* d_n /* S */,
                          int32_t* d_over /* S, nullable: 0 ok, 1 list overflow, 2 more than `rows` keypoints */);

/* ---- Harris corners with sub-pixel refinement ---------------------------------------
 * [ref: src/vo/features/klt.py:99-112]  find_corners(use_goodFeaturesToTrack=False):
 *   cornerHarris(img, block, ksize, k) -> dilate(3x3) -> threshold(rel * max) ->
 *   connectedComponentsWithStats (8-connected; row 0 = background) ->
 *   cornerSubPix(img, float32(centroids), (win_w, win_h), (-1, -1), (EPS | COUNT, max_iter, eps))
 * on every centroid row, background included (NaN when the background is empty; it stays NaN).
 * Labels are numbered in the order of their first 2x2 block (row-major block order), as
 * OpenCV's block-based labelling numbers them.  ksize must be 3; block 1..31; win 1..15;
 * max_iter 1..100 (the criteria's count, clamped as OpenCV clamps it); eps >= 0 (the
 * criteria's epsilon; steps are compared with its square).  The image must be at least
 * (2 win_h + 5) x (2 win_w + 5).  A refused call leaves the context usable.
 * vo_harris_subpix_capacity(H, W) = ceil(H/2) * ceil(W/2) + 1 rows bounds the result exactly. */
int vo_harris_subpix_capacity(int H, int W);
/* [ref: src/vo/features/klt.py:99-112]  S images of one size, enqueued on the context's stream (no
 * synchronisation; the image is the grid's extra dimension).  Image q at d_imgs + q * img_stride bytes;
 * its rows (x, y float32) at d_xy + q * xy_stride * 2, its row count in d_n[q].  Stage outputs, each
 * nullable: d_response H*W float32 and d_labels H*W int32 per image (at + q * H * W), d_centroids
 * (x, y float64) per row (at + q * xy_stride * 2).  Image q's results are those of a call on it alone. */
int vo_harris_subpix_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride /* bytes, >= H*W */, int S, int H,
                               int W, int block, int ksize, double k, double rel, int win_w, int win_h, int max_iter,
                               double eps, float* d_xy, size_t xy_stride /* rows, >= capacity */, int32_t* d_n /* S */,
                               float* d_response, int32_t* d_labels, double* d_centroids);
/* [ref: src/vo/features/klt.py:99-112]  The same from host memory: imgs S*H*W; image q's rows at
 * xy + q * C * 2 (C = vo_harris_subpix_capacity(H, W)), its count in n[q]; response / labels
 * (S*H*W) and centroids (S*C*2) are nullable. */
int vo_harris_subpix_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, int block, int ksize, double k,
                           double rel, int win_w, int win_h, int max_iter, double eps, float* xy, int32_t* n,
                           float* response, int32_t* labels, double* centroids);
/* [ref: src/vo/features/klt.py:99-112]  One image: vo_harris_subpix_batch with S = 1. */
int vo_harris_subpix_corners(vo_ctx* ctx, const uint8_t* img, int H, int W, int block, int ksize, double k, double rel,
                             int win_w, int win_h, int max_iter, double eps, float* xy, int32_t* n, float* response,
                             int32_t* labels, double* centroids);

/* ---- RANSAC control (host-side, bit-compatible with the reference) --------------
 * [ref: src/vo/algorithms/ransac.py:52, 92-94]  the sample stream of
 *   np.random.default_rng(2023).choice(np.arange(pop), replace=False, size=s)
 * vo_pcg64 is NumPy's PCG64 bit-generator state (Generator.bit_generator.state:
 * 128-bit state and increment split into 64-bit halves, plus the buffered 32-bit
 * half).  vo_rng_choice draws `count` samples of s indices and advances the state.
 * [ref: src/vo/algorithms/ransac.py:58-67, 90-121]  vo_ransac_replay walks
 * pre-computed hypotheses (valid, inlier count) through the reference's sequential
 * accept / adaptive-iteration rule; vo_ransac_state holds the fields that persist
 * on the reference's RANSAC object between calls.  max_iterations < 0 = unbounded. */
typedef struct vo_pcg64 {
  uint64_t state_hi, state_lo, inc_hi, inc_lo;
  uint32_t has_uint32, uinteger;
} vo_pcg64;
typedef struct vo_ransac_state {
  double outlier_ratio, confidence;
  int64_t max_iterations, n_iterations;
  int32_t s, adaptive;
} vo_ransac_state;
int vo_rng_choice(vo_pcg64* rng, int pop, int s, int count, int32_t* out);
/* One Generator.choice(pop, 8, replace=False) from the 15 outputs raw[0..14] it consumes when no draw is rejected (eight
 * Floyd draws, seven for the shuffle): host arithmetic, the function the device sampler runs.  *possibly_rejected = 1
 * when one of the draws could have been rejected (the generator may then stand elsewhere).  pop >= 9 (VO_EINVAL below:
 * at pop = 8 the first draw consumes no output). */
int vo_rng_choice8_from_raw(const uint32_t* raw, int pop, int32_t* out, int* possibly_rejected);
/* ---- the two-view bootstrap's RANSAC loop on the device (bootstrap.hip) ----
 * vo_fundamental_ransac: the whole loop of _find_fundamental_matrix_ransac (:110-163; src/vo/algorithms/ransac.py:69-129,
 *   s = 8) in one call, with nothing of it on the host: the generator's outputs are made on the device from *rng, every
 *   sample is derived from them in the hypothesis kernel, one wavefront replays the accept / adapt rule (strict `>`,
 *   outlier ratio clipped to [0.01, 0.99], the bound through a table made with the host's libm) over batches of 2048
 *   samples, and the closing fit runs over the accepted model's inliers.  F 9, inlier_mask N bytes; iterations,
 *   best_count, finished_by_host nullable.  *rng: where the loop starts; advanced by what it consumed.  The results equal
 *   vo_rng_choice + vo_fundamental_hypotheses + vo_ransac_replay + vo_fundamental_fit composed on the host.  That
 *   composition is also the fall-back, reported as *finished_by_host = 1: a loop whose consumed samples hold a draw NumPy
 *   might have rejected, N = 8 (the first Floyd draw consumes no output), max_iterations < 0 (unbounded) or > 65536.
 *   VO_ETRACKING: no model with 8 inliers.
 * vo_rng_raw32_device: the next `count` 32-bit outputs of *rng (a buffered half first, then each 64-bit output low half,
 *   high half) made by the kernel that feeds the loop above, brought to the host; *rng advanced as NumPy's would be. */
int vo_fundamental_ransac(vo_ctx* ctx, const double* p1, const double* p2, int N, int normalize_samples, int error_kind,
                          double threshold, double outlier_ratio, double confidence, int64_t max_iterations,
                          vo_pcg64* rng, double* F, uint8_t* inlier_mask, int64_t* iterations, int32_t* best_count,
                          int32_t* finished_by_host);
int vo_rng_raw32_device(vo_ctx* ctx, vo_pcg64* rng, int count, uint32_t* out);
/* ---- calibrated two-view bootstrap (essential5.hip) ----
 * [ref: src/vo/landmarks/triangulation.py:224-243, _find_essential_matrix]  The reference reaches E through the 8-point F,
 * E = K2^T F K1.  These two reach it from the calibration directly: the five-point minimal solver (Nister 2004) inside the
 * reference's RANSAC loop (src/vo/algorithms/ransac.py:69-129, s = 5).  K1, K2: 3x3 row-major pinhole matrices (HOST
 * pointers); their inverses are formed in closed form from fx, fy, cx, cy, a skew entry is not read.
 * vo_essential_hypotheses: for each of Hyp samples (samples: Hyp*5 indices into the N correspondences x1, x2, N*2 pixels
 *   each) every real essential matrix consistent with its five correspondences:
 *     1. x^ = K^-1 (x, y, 1) in both images
 *     2. the rows kron(x^1, x^2) (the reference's row convention, :203-205) of the 5x9 system; Householder QR of its
 *        transpose; the last four columns of the orthogonal factor span the null space: E = x X + y Y + z Z + W with
 *        E[b][a] = e[3a + b].  A column norm below 1e-10 of the largest: the null space is not four-dimensional (a repeated
 *        correspondence), n_sol = 0
 *     3. det E = 0 and 2 E E^T E - tr(E E^T) E = 0: a 10x20 matrix over the monomials of (x, y, z)
 *     4. Gauss-Jordan elimination with partial pivoting; a pivot below 1e-12 of the matrix's largest entry: n_sol = 0
 *     5. the degree-10 polynomial in z (the determinant of Nister's 3x3 polynomial matrix); a leading coefficient below
 *        1e-13 of the largest coefficient: n_sol = 0
 *     6. every real root: isolated between the real roots of the derivative (from the ninth derivative down, inside the
 *        Cauchy bound), 40 bisection steps on a derivative, 64 bisection and 4 safeguarded Newton steps on the polynomial
 *     7. x, y from the two rows of the polynomial matrix at z whose cross product has the largest third component
 *     8. unit Frobenius norm, the entry of largest magnitude positive (the first in row-major order on ties)
 *   E: Hyp*10*9, the n_sol[h] matrices of sample h in ascending z, the rows behind them zero; never a NaN or Inf.
 *   Every solution is scored as the fundamental matrix F = K2^-T E K1^-1 over all N correspondences in pixels with the
 *   arithmetic of vo_fundamental_hypotheses (error_kind 0: (p2^T F p1)^2; 1: the larger squared distance to the two
 *   epipolar lines; inlier = error < threshold): counts Hyp*10 (an absent solution: 0), masks Hyp*10*ceil(N/64) words
 *   (nullable; an absent solution's row is empty), best_sol Hyp: the lowest index among the sample's solutions with the
 *   largest count, -1 when it has none.
 * vo_essential_ransac: the loop of ransac.py:69-129 with s = 5, composed on the host: samples are drawn ahead from a copy of
 *   *rng by vo_rng_choice(rng, N, 5, 2048) in batches of 2048; hypotheses and scores are made on the device; per batch only
 *   valid = (n_sol > 0), the best count and the best solution index of every sample come back (9 bytes per sample);
 *   vo_ransac_replay with s = 5 walks the accept / adapt rule over them (a sample without a solution is the reference's
 *   "model is None"); *rng is advanced by the samples the loop consumed; only the accepted model's E (9) and its mask row
 *   (inlier_mask, N bytes) are downloaded at the end.  There is NO closing fit: the result is the accepted minimal-sample
 *   model (as cv2.findEssentialMat returns one).  iterations, best_count nullable.
 *   VO_ETRACKING: as many samples as the loop's first bound (min(max_iterations, the bound of outlier_ratio)) were drawn
 *   and none had a real solution; *rng stands behind them.
 * Both: N < 5, a null pointer, a non-finite K (or fx, fy = 0), error_kind outside {0, 1}, a sample index outside [0, N),
 *   an outlier ratio or confidence outside (0, 1), max_iterations = 0: VO_EINVAL, nothing written.                        */
int vo_essential_hypotheses(vo_ctx* ctx, const double* x1, const double* x2, int N, const double* K1, const double* K2,
                            const int32_t* samples, int Hyp, int error_kind, double threshold, double* E, int32_t* n_sol,
                            int32_t* counts, int32_t* best_sol, uint64_t* masks);
int vo_essential_ransac(vo_ctx* ctx, const double* x1, const double* x2, int N, const double* K1, const double* K2,
                        int error_kind, double threshold, double outlier_ratio, double confidence, int64_t max_iterations,
                        vo_pcg64* rng, double* E, uint8_t* inlier_mask, int64_t* iterations, int32_t* best_count);
int64_t vo_ransac_num_iterations(double confidence, double outlier_ratio, int s);
int vo_ransac_replay(vo_ransac_state* st, const uint8_t* valid, const int32_t* counts, int B,
                     int N, int64_t* n_done, int32_t* best_count, int32_t* best_idx,
                     int idx_offset, int* consumed, int* finished);

/* ---- device-resident frame pipeline ------------------------------------------------
 * The steady-state loop of the reference driver [ref: src/main.py:248-286], KLT tracker mode
 * [ref: src/vo/features/tracker.py:56-57], with everything the reference carries from frame to
 * frame kept in HBM: the Features arrays (keypoints, state codes, landmarks, track starts, track
 * start poses, candidate mask) [ref: src/vo/primitives/features.py:4-54], State's current and
 * previous pose [ref: src/vo/primitives/state.py:9-15], the estimator's RANSAC fields and its
 * position in the generator's output stream [ref: src/vo/algorithms/ransac.py:42-56], and
 * KLTTracker._num_features.  The pipeline takes IMAGES ONLY; one step = one frame:
 *   side streams: pyramid(next); Harris response + greedy NMS on next (the detector whose
 *                 keypoints the next step appends when too few tracks survive; launched for
 *                 every frame, executed per sequence within detect_margin of that limit)
 *   re-detect     [ref: src/vo/features/klt.py:207-230, 117-189]  length < 0.8 * _num_features:
 *                 the detector's keypoints of `prev` are appended as unmatched features
 *   KLT           [ref: klt.py:233-249]  every feature prev -> next, keep status & err < thr
 *   Matches       [ref: src/vo/primitives/matches.py:26-212]  regroup into [triangulated |
 *                 matched | newly matched], landmarks / track starts / start poses carried over
 *   estimate_pose [ref: src/vo/pose_estimation/p3p.py:123-186, use_opencv=False]  `hyp` samples
 *                 drawn with the reference's generator, solved and scored; the sequential
 *                 accept / adapt rule [ref: ransac.py:90-121] replayed on the device; refinement
 *                 over the inliers [ref: p3p.py:188-213]
 *   State         [ref: src/vo/primitives/state.py:38-50, 162-172, 135-160, 174-219]  pose,
 *                 reset_outliers, compute_candidates (bearing angle >= threshold)
 *   triangulate_candidates [ref: src/vo/landmarks/triangulation.py:38-86]  one start pose per
 *                 track; update_with_world_landmarks + _check_landmarks [ref: state.py:69-107]
 * No stage waits for the host: a step is a chain of launches, its result a record the last
 * kernel writes to host-visible memory.  The two-view bootstrap [ref: main.py:204-230] runs on
 * the host (vo/driver.py) and hands its Features / poses over with vo_pipeline_set_state, or inside
 * the pipeline from two stored frames (vo_pipeline_bootstrap_seq).                              */
typedef struct vo_pipeline vo_pipeline;
typedef struct vo_pipeline_config {
  int32_t H, W, n_frames;        /* n_frames: frame store in HBM (vo_pipeline_set_frame slots)   */
  int32_t n_keypoints, harris_patch, nms_radius;      /* detector: harris.py:16-25               */
  double harris_kappa;
  int32_t klt_win, klt_max_level, klt_max_iter, hyp;
  double klt_eps, klt_min_eig, klt_err_threshold;      /* klt.py:29-39                            */
  double p3p_thr_sq, ransac_outlier_ratio, ransac_confidence;
  int64_t ransac_max_iterations;                       /* < 0: unbounded                          */
  double K[9];
  double Kinv[9];                /* inverse intrinsics as the caller computes them (the reference:
                                    np.linalg.inv, camera.py:88); all zero = computed here        */
  int32_t refine_iters;          /* > 0: refine the accepted pose over its inliers (vo_refine_pose) */
  int32_t feature_cap;           /* capacity of the Features arrays; 0 = 2 * n_keypoints          */
  double bearing_threshold;      /* State(bearing_threshold), state.py:8; 0 = 0.0075             */
  double redetect_fraction;      /* klt.py:212; 0 = 0.8                                           */
  int32_t debug_fault_every;     /* test hook: every n-th step takes the host recovery path      */
  int32_t redetect_start_pose;   /* start pose of re-detected keypoints: 0 = np.eye(4), as the reference's
                                    update_features writes it (klt.py:148-153) -- away from the origin such
                                    tracks triangulate against the wrong baseline; 1 = the current pose,
                                    what State.reset_outliers gives a restarted track (state.py:170-172) */
  double detect_margin;          /* the detector chain is launched for every frame (its keypoints are what the NEXT
                                    step appends when fewer than redetect_fraction of the tracks are left, and that
                                    count is known one step too late for a launch without a host turn); a sequence
                                    sits it out unless its count, extrapolated by detect_losses times the last
                                    step's loss, is below (redetect_fraction + detect_margin) * num_features.  A
                                    sequence that falls through all of that in one frame is finished through the
                                    host path (detector run then).  0 = 0.01; < 0 = the detector runs on every
                                    frame.  The reference detects only below the limit itself.             */
  int32_t debug_never_detect;    /* test hook: the detector runs only when forced (state hand-over, host path)  */
  double detect_losses;          /* how many of the last step's losses the count is extrapolated by in the detector's
                                    decision (see detect_margin).  0 = 2.5                                          */
  int32_t sequences;             /* S independent frame streams advancing in lock step through the same
                                    launches (the sequence is the grid's extra dimension; SURVEY.md 8e: streams
                                    are independent, so they batch).  0 = 1.  Every sequence has its own frame
                                    store, Features, State, RANSAC object and generator; the plain entry points
                                    address sequence 0, the _seq forms any of them.  KLT and Harris tracker
                                    modes: any S; SIFT tracker mode: one.  The FAST tracker mode: any S. */
  int32_t tracker_mode;          /* 0: KLT tracker with the Harris detector (everything above); 1: SIFT
                                    [ref: src/vo/features/tracker.py:60-61, src/vo/features/sift.py:23-56] -- per frame
                                    detect + describe (every keypoint with sift_cap = -1, as the reference keeps; else
                                    the sift_cap strongest),
                                    2-NN + ratio + first-come uniqueness against the descriptors the current Features
                                    carry, Matches regroup from the pair list with the descriptors following their
                                    keypoints [ref: src/vo/primitives/matches.py:51-58, 134-141], then the same pose
                                    estimation and State bookkeeping.  One sequence per pipeline; the state handed over
                                    needs its descriptors too (vo_pipeline_set_descriptors).  debug_fault_every > 0 has
                                    no effect in this mode.
                                    2: Harris [ref: tracker.py:58-59, src/vo/features/harris.py:50-84, 196-264] -- per
                                    frame the detector's n_keypoints keypoints (response + greedy NMS, every frame),
                                    their raw 19x19 patches (descriptor_radius 9) as bytes, 2-NN + 0.85 ratio +
                                    uniqueness on the matrix cores (361 values padded to 384), then as mode 1.  Any
                                    number of sequences: patches, matcher, regroup and descriptor gather take all of
                                    them in one launch each; lanes (vo_pipeline_set_active_seq / _restart_seq) are KLT
                                    mode only.  debug_fault_every > 0 forces the fault at the pair regroup.
                                    3: FAST + BRIEF (the project's own ORB-style front end, vo/features/fast.py) -- per
                                    frame the up to n_keypoints strongest FAST-9 corners (non-maximum suppression on;
                                    however many the frame has: the count stays on the device) and their BRIEF-256
                                    descriptors (32-byte rows) on the detection stream, a Hamming 2-NN with the ratio
                                    (0.8) / distance (64) / first-come rule on the main stream, then as mode 2: any
                                    number of sequences, every stage one launch for all of them, the same refusals
                                    (detector = 1, lanes, bootstrap, the tracker's forward-backward check, the
                                    structure loop), debug_fault_every > 0 at the pair regroup.  Descriptor rows
                                    handed over or read back carry 32 values.
                                    Threshold, orientation and distance limit: vo_pipeline_set_fast_brief.           */
  int32_t sift_cap;              /* keypoints kept per frame in SIFT mode: 1..4000 (<= feature_cap) the strongest;
                                    0 = n_keypoints; -1 = every keypoint [ref: src/vo/features/sift.py:10, nfeatures = 0]
                                    up to feature_cap -- a frame with more, or whose SIFT lists overflow, fails its step
                                    with VO_ECAPACITY (never a truncated list).  Below -1: refused.                   */
  int32_t track_ids;             /* 1: every feature carries a persistent track id (see "Track ids" below; the
                                    vo_pipeline_*_track_ids_seq / _export_tracks_post_seq entry points).  0 = off: nothing
                                    is allocated and the regroup kernels are the ones without a word of it.  (The field
                                    takes the four bytes that were padding in front of match_ratio: every other field
                                    keeps its offset and the structure its size.)                                     */
  double match_ratio;            /* 0 = the reference's: 0.8 in SIFT mode (sift.py:49), 0.85 in Harris mode (harris.py:255);
                                    0.8 in FAST mode                                                                  */
  int32_t detector;              /* tracker_mode 0: what refills the feature set when fewer than redetect_fraction of the
                                    tracks are left.  0: Harris response + greedy NMS, exactly n_keypoints keypoints
                                    (harris_patch, harris_kappa, nms_radius above).  1: Shi-Tomasi corners, the reference's
                                    cv2.goodFeaturesToTrack [ref: src/vo/features/klt.py:24-26, 87-98, 207-230] with
                                    maxCorners = n_keypoints, no mask (klt.py:216-222 leaves it all-255 whenever features
                                    exist): the step appends however many corners the frame has (none included), and
                                    KLTTracker._num_features becomes that count (klt.py:114), so the re-detect limit
                                    moves with every refill.  A frame whose candidate lists overflow fails its step with
                                    VO_ECAPACITY naming the frame.  Refused with tracker_mode != 0.                   */
  int32_t st_block;              /* Shi-Tomasi blockSize, 1..31; 0 = 7                                              */
  double st_quality;             /* qualityLevel; 0 = 0.01                                                          */
  double st_min_distance;        /* minDistance; 0 = 8                                                              */
} vo_pipeline_config;
typedef struct vo_step_result {
  double R[9], t[3];            /* world -> camera pose of `next` (best hypothesis)   */
  int32_t n_tracked;            /* features of the new frame (survivors of the KLT filter) */
  int32_t n_inliers;            /* inliers of the returned pose                       */
  int32_t best_index;           /* index of the accepted hypothesis                   */
  int32_t hyp_valid;            /* hypotheses with a P3P solution among those scored  */
  int64_t ransac_iterations;    /* iterations the reference loop would have counted   */
  int32_t draws_consumed;       /* samples consumed from the generator                */
  int32_t refine_iterations;    /* accepted refinement steps; -1: not refined         */
  double R_refined[9], t_refined[3];   /* refined pose (= R, t when not refined)      */
  double refine_cost;           /* sum of squared inlier reprojection errors after it */
  int32_t n_features_in;        /* features handed to the tracker (after a re-detect) */
  int32_t redetected;           /* 1: the detector's keypoints were appended          */
  int32_t n_triangulated;       /* tracked features with a landmark: the P3P population */
  int32_t n_candidates;         /* tracks that passed the bearing test and were triangulated */
  int32_t n_dropped;            /* landmarks the cheirality check removed             */
  int32_t n_landmarks;          /* features in state 2 after the step                 */
  int32_t fault;                /* internal: reason the step left the device-only path */
  int32_t recovered;            /* 1: the step was finished through the host path     */
  int32_t detector_ran;         /* 1: the detector was executed on this step's `prev` frame (detect_margin) */
  int32_t reserved;             /* recovered steps: the reason as fault bits (1 few landmarks, 2 a draw NumPy might have
                                   rejected, 4 rule not done after `hyp` samples, 8 capacity, 16 forced, 32 detector skipped) */
  uint64_t raw_pos;             /* generator outputs consumed so far (32-bit words)   */
  double T_wc[12];              /* camera -> world pose after the step, rows 0..2 (State.curr_pose) */
  uint64_t ts[8];               /* device clock (100 MHz ticks) at the start of: tracker, regroup, hypotheses, pose,
                                   landmark stage, at the end of the step (the record's last write); [6], [7]:
                                   inside the pose kernel, RANSAC replay done / refinement done               */
  uint32_t seq_head, seq_tail;  /* internal; the last two words.  In the mapped record: seq_head = the step's sequence
                                   number XOR every other 32-bit word of the record, seq_tail = the number + a
                                   position-weighted sum of those words, so that a copy taken while some of its lines
                                   were still on their way is recognised (vo_record_check); in what the collect calls
                                   return both equal the number                                                    */
} vo_step_result;
/* The self-check of a result record in mapped host memory (the GPU's stores to host memory arrive line by line, in no
 * particular order): _seal closes a record for step `seq` the way the device does, _check returns 1 when the copy is one
 * whole record of that step.  Host arithmetic only.                                                              */
void vo_record_seal(vo_step_result* rec, unsigned seq);
int vo_record_check(const vo_step_result* rec, unsigned seq);
int vo_pipeline_create(vo_ctx* ctx, const vo_pipeline_config* cfg, vo_pipeline** out);
void vo_pipeline_destroy(vo_pipeline* p);
/* A closed pipeline's two side streams and their workspace are kept for the next pipeline of the same configuration (creating
 * and destroying them per pipeline stalled inside the runtime about once in 400 cycles); this destroys what is kept.  Nothing in
 * the reference corresponds to it (its objects are garbage-collected).                                                      */
void vo_pipeline_release_cached(void);
/* 1 when a binding should call vo_pipeline_release_cached from its own exit hook (the library's own policy: under a profiler,
 * or VO_SIDE_POOL_ATEXIT=1), 0 when what is kept is left to the end of the process.                                       */
int vo_pipeline_release_cached_at_exit(void);
/* frame store: copies a host image into slot idx of the frame store.  The caller's buffer is free on return (it is
 * copied into a pinned staging buffer of that slot); the transfer itself is queued in front of the pyramid that reads
 * the slot and the call does not wait for it.  A slot that a step in flight reads is refused (VO_EINVAL), and so is the
 * slot of the frame submitted last once a state exists: the next step tracks FROM that image.                       */
int vo_pipeline_set_frame(vo_pipeline* p, int idx, const uint8_t* img);
int vo_pipeline_seed(vo_pipeline* p, const vo_pcg64* rng);
int vo_pipeline_get_rng(vo_pipeline* p, vo_pcg64* rng);      /* estimator generator state after the last collected step */
/* Hands over the Features of frame idx (the reference's state.curr_frame.features after the
 * bootstrap) and State's poses: n features -- kp n*2 float64 (the tracker reads them rounded to
 * float32, as cv2.calcOpticalFlowPyrLK takes them), state n bytes (0/1/2), landmarks
 * n*3, tracks n*2, poses n*16 (4x4 row-major, camera-to-world; NaN rows where the reference holds
 * NaN) -- plus curr / prev pose as 4x4 camera-to-world AND world-to-camera matrices (the
 * reference forms the latter with np.linalg.inv; passing both keeps every later product the
 * same), and KLTTracker._num_features.  The pyramid and the detector's keypoints of frame idx are
 * made by the first submit after it.                                                            */
int vo_pipeline_set_state(vo_pipeline* p, int idx, int n, const double* kp, const uint8_t* state,
                          const double* landmarks, const double* tracks, const double* poses,
                          const double* T_wc, const double* T_cw, const double* T_wc_prev,
                          const double* T_cw_prev, int num_features);
/* A stream that is walked more than once (bench.py: 100 resident frames, pass after pass): _checkpoint keeps a copy of
 * every sequence's Features / State as they are now -- nothing in flight -- in HBM; _rewind puts that copy back as the
 * state of the frame it was taken at and queues that frame's pyramid and detection, all asynchronously on the pipeline's
 * streams (nothing in flight; no host synchronisation).  What lives on the reference's estimator object across frames
 * (RANSAC.n_iterations / outlier_ratio [ref: src/vo/algorithms/ransac.py:47-56], the generator) is NOT rewound.      */
/* Descriptor tracker modes: the descriptors (n x 128 float32 in SIFT mode, n x 361 in Harris mode; whole numbers
 * 0..255) of the features handed over by the last vo_pipeline_set_state, in the same order.  The plain form is
 * sequence 0's, the _seq form sequence seq's (the features handed over by vo_pipeline_set_state_seq for it).     */
int vo_pipeline_set_descriptors(vo_pipeline* p, const float* desc, int n);
int vo_pipeline_set_descriptors_seq(vo_pipeline* p, int seq, const float* desc, int n);
/* The inverse: the descriptors the current Features of sequence seq carry (they follow their keypoints through every
 * regroup), n x 361 (Harris) or n x 128 (SIFT) whole-number float32 in feature order; *n_out = n (desc may be NULL to
 * ask for n only; desc holds up to vo_pipeline_feature_cap rows).  Nothing may be in flight.                      */
int vo_pipeline_get_descriptors_seq(vo_pipeline* p, int seq, float* desc, int32_t* n_out);
int vo_pipeline_checkpoint(vo_pipeline* p);
int vo_pipeline_rewind(vo_pipeline* p);
/* Downloads the current Features (arrays sized to the capacity vo_pipeline_feature_cap returns;
 * any pointer may be NULL); n_out: feature count.  Nothing may be in flight.                  */
int vo_pipeline_feature_cap(vo_pipeline* p);
int vo_pipeline_get_state(vo_pipeline* p, int32_t* n_out, double* kp, uint8_t* state, uint8_t* candidate_mask,
                          double* landmarks, double* tracks, double* poses, double* T_wc, double* T_wc_prev,
                          vo_ransac_state* rs, int32_t* num_features);
/* keypoints the detector found on the frame submitted last (n_keypoints*2 float64)              */
int vo_pipeline_get_detection(vo_pipeline* p, double* kp_xy);
/* The same for sequence seq with the count: kp_xy holds n_keypoints*2 float64, *n_out = how many of them the detector
 * found (detector 0: always n_keypoints; detector 1: the frame's Shi-Tomasi corners, 0..n_keypoints).  A frame the
 * detector sat out is detected now, for that sequence alone.  Nothing may be in flight.                          */
int vo_pipeline_get_detection_seq(vo_pipeline* p, int seq, double* kp_xy, int32_t* n_out);
/* One frame.  submit enqueues all GPU work of the step prev_idx -> next_idx and returns; collect
 * waits for the oldest submitted step's record.  At most two steps may be in flight (the frame
 * store and the per-frame buffers rotate over three slots); with submit(k+1) before collect(k)
 * the host's launches overlap the GPU's work.  step = submit + collect.                        */
int vo_pipeline_step(vo_pipeline* p, int prev_idx, int next_idx, vo_step_result* out);
int vo_pipeline_submit(vo_pipeline* p, int prev_idx, int next_idx);
int vo_pipeline_collect(vo_pipeline* p, vo_step_result* out);
/* Test / integration entry: the bookkeeping of one frame with everything the estimators would
 * produce given by the caller -- Matches(frame1 = current features, frame2 = Features(new_kp),
 * pairs) [ref: matches.py:11-212], update_with_world_pose(T), outliers[triangulate_inliers] =
 * ~p3p_inliers, reset_outliers, compute_candidates [phase 1]; triangulate_candidates,
 * update_with_world_landmarks [phase 2].  phases: 1, 2 or 3.  Synchronous.                     */
int vo_pipeline_bookkeeping(vo_pipeline* p, int phases, const double* new_kp, int n2, const int32_t* pairs,
                            int M, const double* T_wc, const double* T_cw, const uint8_t* p3p_inliers);
/* vo_prof_read / vo_prof_reset over all of the pipeline's streams                              */
int vo_pipeline_prof_read(vo_pipeline* p, int kernel_id, double* total_ms, int64_t* launches);
int vo_pipeline_prof_reset(vo_pipeline* p);
/* Shared-map record of the last collected step -> DEVICE memory (async):
 * [T_cw 4x4 row-major (16, the refined pose) | n (1) | n landmarks x 3 (the step's P3P
 * population, n <= cap)], all f64, 17 + 3*cap doubles.  The caller all-gathers records over RCCL
 * (bench.py), one or several frames per collective:
 *   _post  queues the record on the pipeline's stream and returns at once;
 *   _join  orders the pipeline's stream and `consumer` (hipStream_t; NULL = the context's
 *          stream) both ways: work enqueued on `consumer` after the call sees every record
 *          posted so far, and records posted after the call are written after everything
 *          `consumer` held at the time of the call (an exchange still reading the buffer).   */
int vo_pipeline_export_state_post(vo_pipeline* p, const vo_step_result* r, int cap, double* d_record);
int vo_pipeline_export_state_post_seq(vo_pipeline* p, int seq, const vo_step_result* r, int cap, double* d_record);
int vo_pipeline_export_state_join(vo_pipeline* p, void* consumer);
/* Track ids (vo_pipeline_config.track_ids = 1; every entry point below returns VO_EINVAL naming track_ids without it).
 * The reference carries Features.uids [ref: src/vo/features/klt.py:49, 147, 228, 263-265; src/vo/primitives/features.py:255-256]
 * drawn from NumPy's global generator and lost at every Matches regroup; what is kept here is their intent, a stable
 * identity per image track, under a deterministic rule.  Per sequence every feature carries two int32 -- id, the track's
 * identity, and born, the value of the sequence's step counter for the frame the track was first seen on -- and the
 * sequence carries next_id:
 *   hand-over (vo_pipeline_set_state(_seq), _restart_seq, _bootstrap, _bootstrap_seq, _bootstrap_lanes): the n features get
 *     ids 0 .. n-1 in feature order, born = 0, next_id = n (vo_pipeline_set_track_ids_seq may replace them afterwards);
 *   KLT mode, step k (k = steps completed before it): when the step re-detects, appended keypoint j (position n + j of the
 *     tracker's input, either detector) gets id = next_id + j, born = k, and next_id grows by the appended count -- a
 *     keypoint the KLT filter then drops has still used up its id; every survivor keeps id and born through the filter and
 *     the regroup;
 *   SIFT and Harris modes, step k: a feature written from pair (i1, i2) keeps the id and born of old feature i1; the
 *     unmatched new keypoints, in ascending new-keypoint index (the order the regroup writes them), get id = next_id + r,
 *     born = k + 1, and next_id grows by their count;
 *   pose, reset_outliers, candidates, landmark insertion, the cheirality check: nothing moves, id and born stay (a track
 *     whose landmark is reset is still the same image track);
 *   a step that faults changes nothing, and a step that is redone (host path, a step enqueued again behind a continued
 *     RANSAC loop, a forced fault of the regroup or of the pose kernel) issues the ids it would have issued the first time;
 *   vo_pipeline_checkpoint / _rewind restore ids and next_id (ids issued after the checkpoint are issued again on the next
 *     pass); born follows the step counter, which is not rewound.
 * Ids are unique within a sequence between two hand-overs; sequences number independently.
 *   _get_track_ids_seq: the current Features' ids / born (arrays of vo_pipeline_feature_cap int32; any pointer may be NULL),
 *     *n_out the feature count, *next_id the next id to issue.  Nothing may be in flight.
 *   _set_track_ids_seq: replaces them: n must be the sequence's feature count, ids distinct, >= 0 and < next_id; born NULL =
 *     left as it is.  Nothing may be in flight; a refused call changes nothing.
 *   _export_tracks_post_seq: queues, on the pipeline's stream, the observation record of the step collected last for
 *     sequence seq (r: its result) into DEVICE memory: a 16-byte header {int32 n, step, next_id, seq} -- the feature count,
 *     the step counter and next_id as that step left them -- then min(n, cap) rows of 48 bytes {int32 id, born; float32 x, y;
 *     int32 state; int32 candidate; float64 X, Y, Z} in feature order, the landmark NaN where the feature has none (state
 *     != 2).  d_record: 16-byte aligned, vo_pipeline_tracks_record_bytes(cap) bytes.  Like the shared-map record it may be
 *     posted with one further step in flight; ordering against a consumer is vo_pipeline_export_state_join.            */
size_t vo_pipeline_tracks_record_bytes(int cap);
int vo_pipeline_get_track_ids_seq(vo_pipeline* p, int seq, int32_t* ids, int32_t* born, int32_t* n_out, int32_t* next_id);
int vo_pipeline_set_track_ids_seq(vo_pipeline* p, int seq, const int32_t* ids, const int32_t* born, int n, int32_t next_id);
int vo_pipeline_export_tracks_post_seq(vo_pipeline* p, int seq, const vo_step_result* r, int cap, void* d_record);
/* the ransac.py:58-67 iteration bound through the pipeline's threshold table (what the device
 * evaluates); equals vo_ransac_num_iterations clipped to max_iterations                         */
int64_t vo_pipeline_ransac_bound(vo_pipeline* p, double outlier_ratio);
/* Several sequences per pipeline (vo_pipeline_config.sequences = S): the sequences step together --
 * vo_pipeline_submit enqueues frame slot prev_idx -> next_idx of EVERY sequence in one set of launches,
 * vo_pipeline_collect_all waits for all S records (outs: S entries; vo_pipeline_collect returns sequence
 * 0's).  A sequence whose step leaves the device-only path is redone alone through the host path; the
 * others are not held up on the device.  vo_pipeline_seed gives every sequence's estimator the same
 * generator state (each then advances by its own draws).                                        */
int vo_pipeline_sequences(vo_pipeline* p);
int vo_pipeline_set_frame_seq(vo_pipeline* p, int seq, int idx, const uint8_t* img);
/* The same from PINNED host memory (vo_host_alloc; a frame grabber's or a decoder's output buffer): no staging copy on the
 * host, and the DMA runs on a stream of its own beside the pipeline's kernels instead of in front of the frame's pyramid --
 * a frame uploaded while the previous step is still in flight costs the step nothing.  The buffer must not change until
 * the upload is over: vo_pipeline_frame_uploaded(idx, wait) -- 1 when it is (wait != 0: blocks until then), 0 when not --
 * or the collect of a step that read the slot.  Replaces the image hand-over of the reference's per-frame loop
 * (src/main.py:248-251: frame.image goes into Tracker.track as a host array).                                         */
int vo_pipeline_set_frame_pinned(vo_pipeline* p, int seq, int idx, const uint8_t* pinned_img);
int vo_pipeline_frame_uploaded(vo_pipeline* p, int idx, int wait);
/* Hint: frame slot idx will be the `next_idx` of the coming vo_pipeline_submit.  Its pyramid (klt.py:233-249 builds it
 * inside cv2.calcOpticalFlowPyrLK, per call) is built now, behind the tracker of the step submitted last, so the coming
 * step's tracker does not start behind a pyramid that its own, later, submit enqueues.  Results do not depend on the hint;
 * a wrong one costs one wasted pyramid.  KLT tracker mode; a no-op otherwise and before the first step.                 */
int vo_pipeline_prepare(vo_pipeline* p, int idx);
/* The tracker's forward-backward check in the frame loop (the rule: "pyramidal KLT", vo_klt_track_fb).  fb_max > 0 pixels
 * (+inf allowed): from the next submitted step on, the step's tracker launch is the forward-backward one and the KLT filter
 * reads its status, status_f & status_b & (fb <= fb_max^2), next to err < klt_err_threshold.  0 switches the check off, which
 * is the state at creation: the pipeline then makes the launches it always made.  Any number of sequences; steps that go
 * through the host path (recovery) track the same way.  Requires nothing in flight and the KLT tracker mode: refused with a
 * message in the descriptor modes, as is a negative or NaN value.  vo_pipeline_config is not involved.  The two-view
 * bootstrap (vo_pipeline_bootstrap_seq) keeps its plain tracker.  _get_ reads the value back (0: off).                    */
int vo_pipeline_set_klt_fb(vo_pipeline* p, double fb_max);
int vo_pipeline_get_klt_fb(vo_pipeline* p, double* fb_max);
/* The settings of the FAST + BRIEF tracker mode (tracker_mode = 3), FASTBRIEFDetector's defaults at creation (20, not
 * oriented, 64; match_ratio = 0 means 0.8 in this mode).  fast_threshold: 0 = 20, valid 0 .. 254; brief_oriented: 0 or 1;
 * brief_max_distance: the largest Hamming distance a pair may have, 0 = 64, < 0 = no limit, at most 256.  A value out of
 * range is refused with a message naming it, as is a pipeline in another mode or with a step in flight; the settings hold
 * from the next submitted step on.  vo_pipeline_config is not involved: its layout is the one it was.  _get_ reads the
 * values in force back.                                                                                               */
int vo_pipeline_set_fast_brief(vo_pipeline* p, int fast_threshold, int brief_oriented, int brief_max_distance);
int vo_pipeline_get_fast_brief(vo_pipeline* p, int32_t* fast_threshold, int32_t* brief_oriented, int32_t* brief_max_distance);
int vo_host_alloc(vo_ctx* ctx, size_t bytes, void** out);
int vo_host_free(vo_ctx* ctx, void* p);          /* ctx may be NULL */
/* ---- frame ingest: three-channel frames and lens undistortion on the device ------------------------------------
 * What a frame goes through between a camera's buffer and a frame slot.  Both operations are defined in integers and
 * float64, and tests/frame_ingest_oracle.py computes the same bytes (OpenCV parity is not claimed).
 *   grey:      g = (1868 B + 9617 G + 4899 R + 8192) >> 14, channels in the order B, G, R -- what cv2.imread hands the
 *              reference and its cvtColor call sites convert [ref: src/vo/features/klt.py:58-62, harris.py:41-48].
 *   undistort: the reference's Camera takes distortion coefficients and leaves undistort / distort_points empty
 *              [ref: src/vo/sensors/camera.py:38-54].  Here: dist = (k1, k2, p1, p2, k3), K the pinhole camera of the
 *              output, K_raw the intrinsics of the distorted image (NULL: K).  For output pixel (u, v), in float64 without
 *              contraction:  x = (u - cx) / fx, y = (v - cy) / fy, r2 = x x + y y,
 *                kr = 1 + ((k3 r2 + k2) r2 + k1) r2,
 *                xd = (x kr + p1 (2 x) y) + p2 (r2 + 2 x x),  yd = (y kr + p1 (r2 + 2 y y)) + p2 (2 x) y,
 *                us = fx_raw xd + cx_raw, vs = fy_raw yd + cy_raw;
 *              the source position is rounded to 1/32 pixel (ties to even, clamped to +-2^24 / 32 first) and the four
 *              neighbours are blended with the integer weights (32 - a)(32 - b), a (32 - b), (32 - a) b, a b, + 512, >> 10;
 *              a neighbour outside the image counts as 0.  Non-finite coefficients or intrinsics: VO_EINVAL.
 * vo_gray_from_bgr / vo_undistort_image: one image, host arrays (bgr H x W x 3, the others H x W bytes).
 * vo_pipeline_set_distortion_seq: lane seq's coefficients (5 doubles) and K_raw from now on; the pinhole camera is the
 *   lane's K (vo_pipeline_set_camera_seq), with K_raw NULL also the distorted image's, as it is at each upload.  dist NULL
 *   or all zero with K_raw NULL: no undistortion.  Nothing may be in flight.  Applies to frames uploaded after the call;
 *   slots already filled keep their contents.
 * vo_pipeline_set_frame_bgr_seq / _bgr_pinned: vo_pipeline_set_frame_seq / _pinned for an H x W x 3 image -- same slot
 *   rules, same events, same pinned bookkeeping.  The slot receives undistort(gray(image)).  The DMA lands in a raw buffer
 *   (one per stream, made on first use) and the ingest kernel follows it on the same stream -- the tracker's for the plain
 *   call, the upload stream for the pinned one; what waits for the upload waits for the kernel.  The grey entry points
 *   undistort too when the lane has coefficients; without them they are one copy and no kernel, as before.
 * vo_pipeline_get_frame_seq: downloads slot idx of lane seq (H x W bytes).  Nothing may be in flight.               */
int vo_gray_from_bgr(vo_ctx* ctx, const uint8_t* bgr, int H, int W, uint8_t* gray);
int vo_undistort_image(vo_ctx* ctx, const uint8_t* img, int H, int W, const double K[9], const double dist[5],
                       const double K_raw[9], uint8_t* out);
int vo_pipeline_set_distortion_seq(vo_pipeline* p, int seq, const double dist[5], const double K_raw[9]);
int vo_pipeline_set_frame_bgr_seq(vo_pipeline* p, int seq, int idx, const uint8_t* bgr);
int vo_pipeline_set_frame_bgr_pinned(vo_pipeline* p, int seq, int idx, const uint8_t* bgr_pinned);
int vo_pipeline_get_frame_seq(vo_pipeline* p, int seq, int idx, uint8_t* out);
int vo_pipeline_set_state_seq(vo_pipeline* p, int seq, int idx, int n, const double* kp, const uint8_t* state,
                              const double* landmarks, const double* tracks, const double* poses,
                              const double* T_wc, const double* T_cw, const double* T_wc_prev,
                              const double* T_cw_prev, int num_features);
int vo_pipeline_get_state_seq(vo_pipeline* p, int seq, int32_t* n_out, double* kp, uint8_t* state,
                              uint8_t* candidate_mask, double* landmarks, double* tracks, double* poses,
                              double* T_wc, double* T_wc_prev, vo_ransac_state* rs, int32_t* num_features);
int vo_pipeline_get_rng_seq(vo_pipeline* p, int seq, vo_pcg64* rng);
int vo_pipeline_collect_all(vo_pipeline* p, vo_step_result* outs);
/* ---- lanes: many recordings through one pipeline ------------------------------------------------------------
 * Each sequence of an S-sequence pipeline is a lane that can hold one recording after another, each handled as the
 * reference handles a recording per process [ref: src/main.py:168-230, per recording: its camera, its bootstrap, a fresh
 * RANSAC object and generator].  All three need nothing in flight (vo.driver.run_batch_on_device drains before them).
 *
 * _set_camera_seq: lane seq's intrinsics from now on (Kinv NULL: computed as at create).  Every kernel reads its
 *   sequence's entry of a device table of S cameras (P3P hypotheses, pose + refinement, candidates, DLT, landmarks), and
 *   so does the host recovery path.  A pipeline starts with cfg.K in every entry.
 * _set_active_seq(seq, 0): the lane goes idle.  No kernel of a step works on it (its pyramid is left out of the launch, its
 *   detector does not run, the tracker gets no features, the main chain's kernels return on the control block's
 *   VO_FAULT_IDLE bit), it consumes no draws and it never enters the host recovery path.  collect_all still returns S
 *   records; an idle lane's record has n_features_in = -1, fault = 256 (VO_FAULT_IDLE), best_index = -1,
 *   refine_iterations = -1, raw_pos = its generator position, every other field 0.  _set_active_seq(seq, 1) only
 *   accepts a lane that is active already: an idle lane comes back through _restart_seq.  While a lane is idle its frame
 *   in the slot the next submit starts from may be replaced (vo_pipeline_set_frame_seq / _pinned), which is how a
 *   restart gets its recording's first frame there.
 * _restart_seq: a new recording for lane seq alone -- the arrays of vo_pipeline_set_state_seq for frame slot idx, which
 *   must be the `prev` of the next submit; a fresh RANSAC object [ref: src/vo/algorithms/ransac.py:47-56]; the lane's
 *   generator from *rng (NULL: the state of the last vo_pipeline_seed, i.e. what a fresh pipeline seeded the same way
 *   starts from).  The pyramid and the detection of that frame are made for this lane only; the other lanes' Features,
 *   control blocks, generators and pyramids are not touched.  A pyramid vo_pipeline_prepare built is dropped.  The lane
 *   is active afterwards.  Cost: the drain before it (the look-ahead step is lost once) and one lane's pyramid +
 *   detection, waited for (lanes).  KLT tracker mode.                                                   */
int vo_pipeline_set_camera_seq(vo_pipeline* p, int seq, const double K[9], const double Kinv[9]);
int vo_pipeline_set_active_seq(vo_pipeline* p, int seq, int active);
int vo_pipeline_restart_seq(vo_pipeline* p, int seq, int idx, int n, const double* kp, const uint8_t* state,
                            const double* landmarks, const double* tracks, const double* poses,
                            const double* T_wc, const double* T_cw, const double* T_wc_prev,
                            const double* T_cw_prev, int num_features, const vo_pcg64* rng);

/* ---- two-view bootstrap inside the pipeline ------------------------------------------------------------------
 * A sequence enters the pipeline from two frames of its frame store instead of from finished Features arrays: what
 * vo.driver.bootstrap computes on the host [ref: src/main.py:204-230] for frames idx_a, idx_b of sequence seq, followed by
 * the hand-over vo_pipeline_set_state_seq / vo_pipeline_restart_seq make with its result.  KLT tracker mode.
 *   1. Shi-Tomasi corners of frame a (vo_good_features_batch_dev) [ref: src/vo/features/klt.py:24-26, 98];
 *      num_features = their count [ref: klt.py:114];
 *   2. pyramids of a and b with the bootstrap's own window / level count, LK a -> b, keep status & err <
 *      klt_err_threshold [ref: klt.py:233-262]; the identity-pair Matches regroup of fresh Features keeps the survivors
 *      in order, all in state 1, tracks starting at the frame-a corner with start pose identity
 *      [ref: src/vo/primitives/matches.py:26-212];
 *   3. 8-point RANSAC over the survivors (vo_fundamental_hypotheses' kernels: per-sample Hartley frame, squared pixel
 *      distance to the epipolar lines in both images, a fresh generator default_rng(2023) [ref: src/vo/algorithms/
 *      ransac.py:52], closing fit over all inliers), then vo_relative_pose's kernel
 *      [ref: src/vo/landmarks/triangulation.py:110-163, 279-350];
 *   4. update_with_local_pose, update_with_local_landmarks (with _check_landmarks against both cameras), reset_outliers
 *      [ref: src/vo/primitives/state.py:24-67, 90-107, 162-172], written into the lane's current Features block and its
 *      control block (T_cw = M, T_wc its closed-form inverse, previous pose = identity): a feature ends in state 2 with
 *      its landmark, its track start at the frame-a corner and start pose identity, or in state 0 with track start = its
 *      own keypoint and start pose = the current pose; none is left in state 1;
 *   5. on a pipeline that is not running yet what vo_pipeline_set_state_seq does (idx_b under its rules for idx; the
 *      RANSAC object fresh on the lane's first hand-over; the generator stays as seeded unless rng is given); on a
 *      running pipeline what vo_pipeline_restart_seq does (idx_b must be the `prev` of the next submit; fresh RANSAC
 *      object; the lane's generator from *rng, NULL: the state of the last vo_pipeline_seed; lane active; a prepared
 *      pyramid dropped; this lane's pyramid + detection of frame b made for it alone; other lanes untouched).
 * idx_a is any other slot.  Nothing may be in flight.  The call is synchronous.
 * No array sized by pixels or by features crosses between host and device: what crosses is counted in bytes_h2d /
 * bytes_d2h -- scalars: parameters and the RANSAC loop's control block up; counts, status words, F, M and the landmark
 * count down (the loop's sampler and accept / adapt rule run on the device, see vo_fundamental_ransac; the first call with
 * given confidence / budget also uploads the bound's threshold table, 8 bytes per iteration of the budget).
 * Failures are status codes: VO_ETRACKING for fewer than 8 corners or survivors or a RANSAC without a model of 8 inliers,
 * VO_ECAPACITY for candidate lists or a corner count beyond the feature capacity.  Until step 4 only workspace is
 * written, so A FAILED CALL LEAVES THE LANE AS IT WAS before it: Features, control block, generator, activity.
 * (route: reserved for the reference's own RANSAC route -- population normalised once, algebraic error -- must be 0.) */
typedef struct vo_bootstrap_params {      /* 0 in a field = the default named here */
  int32_t max_corners;                    /* Shi-Tomasi corners on frame a; 0 = cfg.n_keypoints [ref: klt.py:24-26] */
  double  quality, min_distance;          /* 0.01, 8                                             */
  int32_t block;                          /* 7                                                   */
  int32_t klt_win, klt_max_level;         /* tracker a -> b; 0 / -1 = the pipeline's own         */
  double  threshold_px;                   /* epipolar distance, 0 = 0.25 [ref: src/main.py:185-193] */
  double  outlier_ratio, confidence;      /* 0.9, 0.999                                          */
  int32_t max_iterations;                 /* 0 = 2000                                            */
  int32_t route;                          /* 0                                                   */
} vo_bootstrap_params;
typedef struct vo_bootstrap_result {
  int32_t n_corners, n_tracked, n_ransac_inliers, n_landmarks, n_features;
  int32_t reserved;                       /* 1: the RANSAC loop was finished by the host sampler  */
  int64_t ransac_iterations;
  double  M[12];                          /* camera a -> camera b, 3x4 row-major, |t| = 1        */
  int64_t bytes_h2d, bytes_d2h;           /* what the call copied between host and device        */
} vo_bootstrap_result;
int vo_pipeline_bootstrap_seq(vo_pipeline* p, int seq, int idx_a, int idx_b, const vo_bootstrap_params* prm /* NULL: defaults */,
                              const vo_pcg64* rng, vo_bootstrap_result* out);
int vo_pipeline_bootstrap(vo_pipeline* p, int idx_a, int idx_b, const vo_bootstrap_params* prm, vo_bootstrap_result* out);
/* Several lanes in one call: lanes seqs[0 .. n_lanes-1] (in range, distinct) go through ONE set of launches -- the lane is a
 * grid dimension of every stage, Shi-Tomasi included -- and each ends exactly as if vo_pipeline_bootstrap_seq(p, seqs[i], idx_a,
 * idx_b, prm, rngs ? &rngs[i] : NULL, &outs[i]) had been called for it alone, in the order given.  The call-level rules are
 * the one-lane call's; a refused call (VO_EINVAL) changes nothing.  A lane that FAILS (VO_ETRACKING: fewer than 8 corners or
 * survivors, no model with 8 inliers; VO_ECAPACITY) gets its code in status[i] (nullable) and stays as it was, the other
 * lanes go through; the call returns VO_OK when every lane did, otherwise the first failing lane's code, the lane named in
 * the error text.  outs[i].bytes_h2d / bytes_d2h: the CALL's traffic divided by n_lanes (rounded up).  outs[i].reserved:
 * 1 = the lane's RANSAC loop was finished by the host sampler (see vo_fundamental_ransac), 0 = on the device. */
int vo_pipeline_bootstrap_lanes(vo_pipeline* p, int n_lanes, const int32_t* seqs, int idx_a, int idx_b,
                                const vo_bootstrap_params* prm, const vo_pcg64* rngs, vo_bootstrap_result* outs, int32_t* status);
/* the generator the bootstrap's RANSAC starts from: np.random.default_rng(2023)'s PCG64 state */
void vo_bootstrap_default_rng(vo_pcg64* rng);

/* ---- Window bundle adjustment ------------------------------------------------------------------
 * Nothing in the reference corresponds to it (its poses stay as the P3P refinement left them, its landmarks as their two-view
 * triangulation made them): a local back end over the last W frames, fed from the observation records above.
 *
 * One window: W poses (world -> camera; R row-major then t, 12 doubles: vo_refine_pose_dev's Rt0), L landmarks (3 doubles),
 * M observations (slot, u, v) grouped by landmark -- lm_start[L + 1] is the CSR, landmark i owns observations lm_start[i] ..
 * lm_start[i + 1] - 1, at least one, their slots strictly ascending -- and one K (3x3 row-major; fx, fy, cx, cy are read).
 * The leading n_fixed >= 1 slots are held (default 2: the six gauge freedoms and the scale).
 *   cost    e = x - proj(K, R X + t);  rho = |e|^2 when huber_px == 0, else Huber's: |e|^2 for |e| <= d, 2 d |e| - d^2 above
 *           (d = huber_px), with the IRLS weight w = min(1, d / |e|) (w = 1 for the squared loss);  cost = sum rho
 *   step    Levenberg-Marquardt on the weighted normal equations at the current point.  Pose increment (v, w) on the left,
 *           T <- [Exp(w) | v] T, Exp by Rodrigues' formula (vo_refine_pose's parametrisation); landmark increment additive.
 *           Per observation with p = R X + t, a = fx / p_z, b = fy / p_z, c = -fx p_x / p_z^2, d = -fy p_y / p_z^2:
 *             J_pose = [a 0 c  c p_y  a p_z - c p_x  -a p_y;  0 b d  d p_y - b p_z  -d p_x  b p_x],  J_lm = [a 0 c; 0 b d] R.
 *           U_j = sum w J_pose^T J_pose and g_p,j = sum w J_pose^T e over the observations of free pose j;  V_i = sum w
 *           J_lm^T J_lm and g_l,i = sum w J_lm^T e over those of landmark i (every slot);  W_ij = w J_pose^T J_lm for an
 *           observation of a free pose.  Damping: the diagonals of U and V times (1 + lambda).  Reduced system over the
 *           free poses: S = U* - sum_i W_i V_i*^-1 W_i^T, b = g_p - sum_i W_i V_i*^-1 g_l,i, dense, 6 (W - n_fixed) square,
 *           solved by Cholesky without pivoting; landmarks by back-substitution, dX_i = V_i*^-1 (g_l,i - sum_j W_ij^T d_j).
 *           A landmark seen from held slots only adds nothing to S and is still refined.  A pivot that is not positive, in
 *           a 3x3 or in S, rejects the trial.
 *   control lambda starts at lambda0.  Before every trial, in this order: `max_iter` accepted steps -> status 1;
 *           `max_trials` trials -> status 2; lambda > 1e12 -> status 3.  The system is solved (a rejected solve counts as a
 *           trial).  |delta| <= step_tol (1 + |x|) -- delta: every pose and landmark increment, x: the free poses'
 *           translations and every landmark, 2-norms -- ends the solve with status 0: the step is not taken and not counted.
 *           Otherwise the trial is counted and evaluated: accepted iff every observation has p_z > 0 at the trial point and
 *           cost_new <= cost; then lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.
 *   refused status 4, the window bit for bit as it was: L <= 0 or M <= 0 (empty) or beyond the capacities; no free pose
 *           (n_fixed >= W); a CSR that is not one (see above) or a slot outside 0 .. W - 1; a non-finite observation, pose,
 *           landmark or intrinsic; an observation with p_z <= 0 at the start.
 * All of it fp64.  Every sum has one fixed order (per landmark in CSR order, landmarks ascending; workgroup sums by a
 * butterfly and a fixed-order add; no floating-point atomics): the same call gives the same bits, and a window gives the same
 * bits alone as inside a batch.
 *
 * vo_window_ba_dev: S windows per call, one workgroup each, no host read until the caller asks for the results.  Window q:
 *   d_counts + 4 q     int32 {L, M, -, -} (the header vo_window_from_tracks_dev writes)
 *   d_K + 9 q          d_poses + 12 W q (in place)      d_X + 3 L_cap q (in place)
 *   d_lm_start + (L_cap + 1) q      d_obs_slot + M_cap q      d_obs_xy + 2 M_cap q      d_results + q
 * W <= 16, 1 <= M_cap <= L_cap W.  The workspace (vo_window_ba_workspace_bytes) is the context's and grows on demand.
 * Enqueued on the context's stream; does not synchronise.  vo_window_ba: the same from host arrays (uploads, runs, downloads
 * poses, X and results, synchronises).  Bad arguments: VO_EINVAL with a message.                                       */
typedef struct vo_ba_params {             /* 0 in a field = the default named here */
  int32_t max_iter;                       /* accepted steps, <= 50; default 10 */
  int32_t max_trials;                     /* trials, <= 1000; default 2 * max_iter */
  int32_t n_fixed;                        /* leading slots held; default 2 */
  int32_t reserved;
  double huber_px;                        /* Huber threshold in pixels; 0 = squared loss */
  double lambda0;                         /* default 1e-3 */
  double step_tol;                        /* default 1e-10 */
} vo_ba_params;
typedef struct vo_ba_result {
  int32_t status;                         /* 0 converged, 1 max_iter, 2 max_trials, 3 lambda beyond 1e12, 4 refused */
  int32_t iterations, trials;             /* accepted steps; trials counted */
  int32_t n_obs;                          /* M */
  double cost0, cost;                     /* at the start, at the result */
  double lambda;                          /* as the solve left it */
} vo_ba_result;
size_t vo_window_ba_workspace_bytes(int S, int W, int L_cap, int M_cap);
int vo_window_ba_dev(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* d_counts, const double* d_K, double* d_poses,
                     double* d_X, const int32_t* d_lm_start, const int32_t* d_obs_slot, const double* d_obs_xy,
                     const vo_ba_params* prm /* NULL: defaults */, vo_ba_result* d_results);
int vo_window_ba(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* counts, const double* K, double* poses, double* X,
                 const int32_t* lm_start, const int32_t* obs_slot, const double* obs_xy, const vo_ba_params* prm,
                 vo_ba_result* results);
/* The window of W observation records exactly as vo_pipeline_export_tracks_post_seq wrote them (d_records: a HOST array of W
 * device pointers, oldest first; rows beyond `cap` of a record are ignored), built on the device, no host turn:
 *   landmarks     the rows of the newest record with state == 2 and finite X, Y, Z whose id occurs in at least one other
 *                 record of the window, in row order; the first L_cap of them.  d_X: that row's X, Y, Z; d_lm_id: its id.
 *   observations  per landmark, for each slot in ascending order in which its id occurs (any state: it is the same image
 *                 track; the first row carrying the id), (slot, (double)x, (double)y).
 *   d_head        int32 {L, M, flags, 0}; flags: 1 when the first landmark left out was left out for L_cap, 2 when for M_cap
 *                 (the list ends at the last landmark whose observations fit wholly), 0 when none was.  d_lm_start[L] = M.
 * The join compares ids and copies; nothing is rounded.  The poses of the window are the caller's (vo_step_result).  Enqueued
 * on the context's stream (order it behind the records with vo_pipeline_export_state_join when that is another stream).  */
int vo_window_from_tracks_dev(vo_ctx* ctx, int W, const void* const* d_records, int cap, int L_cap, int M_cap, int32_t* d_head,
                              int32_t* d_lm_start, int32_t* d_obs_slot, double* d_obs_xy, double* d_X, int32_t* d_lm_id);
/* The one write of a back end into a pipeline: the features of sequence seq whose track id is d_ids[k] (device, n of them; the
 * first k for an id given twice) AND whose state is 2 take the landmark d_X[3 k ..] (device); every other byte of the state,
 * the poses included, stays as it was.  Nothing may be in flight; needs vo_pipeline_config.track_ids (VO_EINVAL naming it).
 * Enqueued on the pipeline's stream; synchronises.                                                                      */
int vo_pipeline_update_landmarks_seq(vo_pipeline* p, int seq, int n, const int32_t* d_ids, const double* d_X);

/* ---- Window structure refinement ------------------------------------------------------------------
 * The window bundle adjustment with every pose held -- the configuration it refuses (n_fixed >= W) and the cheap one: the
 * poses stay as the per-frame P3P refinement left them, and each landmark is a least-squares problem of its own in three
 * unknowns over the observations of its track.  No Schur complement, no reduced system; landmarks never meet.
 *
 * The window is vo_window_ba_dev's, array for array and stride for stride (d_counts {L, M, -, -}, d_K, d_poses W x 12 -- read
 * only here --, d_X in place, d_lm_start, d_obs_slot, d_obs_xy); W <= 16, S windows per call.  Per landmark i, over its
 * observations k = lm_start[i] .. lm_start[i + 1] - 1, with e, rho, the IRLS weight w, p, a b c d and J_lm = [a 0 c; 0 b d] R
 * exactly as above:
 *   sums    V = sum w J_lm^T J_lm;  g = sum w J_lm^T e;  cost = sum rho.  Every sum runs over the landmark's observations in
 *           one fixed order.
 *   step    the diagonal of V times (1 + lambda); the 3x3 system solved by Cholesky without pivoting, dX = V*^-1 g.  A pivot
 *           that is not positive rejects the trial: it is counted and lambda <- 10 lambda.
 *   control lambda starts at lambda0.  Before every trial, in this order: `max_iter` accepted steps -> status 1;
 *           `max_trials` trials -> status 2; lambda > 1e12 -> status 3.  Then the system is solved.
 *   stop    the step is not taken and not counted, status 0, when |dX| <= step_tol (1 + |X|) or g . dX <= f_tol cost (g . dX:
 *           the decrease the linearisation predicts).  The second test is what makes the counts a property of the window and
 *           not of the summation order: these problems converge quadratically to rounding level, where a trial changes the
 *           cost by 1e-15 of itself and cost_new <= cost is a coin toss; a trial that is evaluated is predicted to lower the
 *           cost by more than f_tol of it.
 *   accept  otherwise the trial is counted; accepted iff every observation has p_z > 0 at X + dX and cost_new <= cost: then
 *           lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.
 *   refused status 4, X bit for bit as it was, iterations = trials = 0, costs and min_cos 0: a landmark with fewer than 2
 *           observations or more than W (n_obs: the CSR's count when it lies in 0 .. W, else 0); slots not strictly ascending
 *           in 0 .. W - 1; a non-finite observation or X; an observation with p_z <= 0, or a cost that is not finite, at the
 *           start.  A window with L > L_cap, M outside 0 .. M_cap, lm_start[L] != M or a non-finite pose or intrinsic
 *           refuses every one of its landmarks (n_obs 0); L <= 0 has none.  One bad landmark never touches its neighbours.
 *   min_cos the smallest cosine between any two of the landmark's world-frame observation rays, R^T ((u - cx) / fx,
 *           (v - cy) / fy, 1) normalised.
 *   gate    a refined landmark is kept iff status is 0 or 1, and gate_px == 0 or sqrt(sum |e|^2 / n_obs) <= gate_px (the
 *           squared residuals at the result, also under Huber), and min_parallax == 0 or min_cos <= cos(min_parallax).  A
 *           landmark that is not kept has X bit for bit as it was; cost is still the one the refinement reached.
 * All of it fp64, no floating-point atomics: the same call gives the same bits, and a window gives the same bits alone as
 * inside a batch.
 *
 * vo_window_structure_dev: window q's rows at d_results + L_cap q (rows i < min(L, L_cap) are written, the others left) and
 * its summary at d_summary + q; two launches (the landmarks; one workgroup per window for the summary), enqueued on the
 * context's stream, no synchronisation.  vo_window_structure: the same from host arrays (uploads, runs, downloads X, the
 * results -- rows that are not written read 0 -- and the summaries, synchronises).  Bad arguments: VO_EINVAL with a message. */
typedef struct vo_structure_params {      /* 0 in a field = the default named here */
  int32_t max_iter;                       /* accepted steps, <= 50; default 10 */
  int32_t max_trials;                     /* trials, <= 1000; default 2 * max_iter */
  double huber_px;                        /* Huber threshold in pixels; 0 = squared loss */
  double lambda0;                         /* default 1e-3 */
  double step_tol;                        /* default 1e-10 */
  double f_tol;                           /* default 1e-9 */
  double gate_px;                         /* RMS reprojection gate in pixels; 0 = no gate */
  double min_parallax;                    /* radians, < pi; 0 = no gate */
} vo_structure_params;
typedef struct vo_structure_result {      /* per landmark */
  int32_t status;                         /* 0 converged, 1 max_iter, 2 max_trials, 3 lambda beyond 1e12, 4 refused */
  int32_t iterations, trials;             /* accepted steps; trials counted */
  int32_t n_obs;
  double cost0, cost;                     /* at the start, at the refined point */
  double min_cos;
  int32_t kept;                           /* 1: X is the refined point, 0: X is the input */
  int32_t reserved;
} vo_structure_result;
typedef struct vo_structure_summary {     /* per window */
  int32_t L;                              /* as d_counts gave it */
  int32_t n_refused, n_kept;
  int32_t max_iterations;
  double cost0, cost;                     /* sums over the landmarks not refused, in one fixed order */
} vo_structure_summary;
int vo_window_structure_dev(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* d_counts, const double* d_K,
                            const double* d_poses, double* d_X, const int32_t* d_lm_start, const int32_t* d_obs_slot,
                            const double* d_obs_xy, const vo_structure_params* prm /* NULL: defaults */,
                            vo_structure_result* d_results /* S * L_cap */, vo_structure_summary* d_summary /* S */);
int vo_window_structure(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* counts, const double* K,
                        const double* poses, double* X, const int32_t* lm_start, const int32_t* obs_slot, const double* obs_xy,
                        const vo_structure_params* prm, vo_structure_result* results, vo_structure_summary* summary);

/* ---- Structure loop ------------------------------------------------------------------
 * The structure refinement above, run behind every collected step of a KLT-mode pipeline (tracker_mode 0, track_ids) without
 * giving up the look-ahead: the last W observation records of every lane stay in a ring on the device, and ONE call per
 * collected step, vo_structure_loop_post, queues everything on the pipeline's main stream.  The host does not wait and reads
 * nothing back; one further step may be in flight.
 *
 * Call order.  post(k) is called after step k has been collected, with at most one further step, k + 1, in flight
 * (vo_pipeline_export_tracks_post_seq's condition).  It queues items 1 to 5, in this order, on the main stream: they run behind
 * step k + 1 and in front of whatever is submitted next.
 *   1. record   the observation record of step k -- byte for byte what vo_pipeline_export_tracks_post_seq writes, with cap = the
 *               pipeline's feature capacity -- into the lane's ring slot, and the refined pose of step k (R_refined, t_refined
 *               of its vo_step_result, 12 doubles) into the lane's pose ring.  An idle lane (its result's n_features_in == -1)
 *               posts nothing and its window starts again.
 *   2. window   the lane's last W records, oldest = slot 0.  The window is FULL iff W records have been posted since the last
 *               reset, every step counter follows its predecessor by one, and no next_id decreases.  The host knows only how
 *               many records were posted; the headers are checked on the device.  A window that is not full has L = 0, and
 *               items 3 to 5 do nothing for that lane.
 *   3. join     head, lm_start, obs_slot, obs_xy, X, lm_id: array for array and bit for bit what vo_window_from_tracks_dev gives
 *               for the same W records with cap = the feature capacity and the loop's L_cap, M_cap -- the two cut flags and the
 *               "first row carrying the id" rule included.  The poses of the window come from the pose ring in age order, K
 *               from the lane's camera.
 *   4. refine   vo_window_structure_dev's kernels on that window with the loop's vo_structure_params: results, summary and X per
 *               lane are bit for bit what a stand-alone call gives.
 *   5. write    (feedback = 1 only) into the features as step k + 1 left them, or as step k left them when nothing was in
 *               flight.  A feature takes the refined landmark of window landmark i iff its track id is lm_id[i], AND its state
 *               is 2, AND landmark i is kept and its X differs in at least one bit from the window's input, AND the feature's
 *               landmark is still bit for bit the window's input X of i.  The last condition makes one step of lag safe: a
 *               track whose landmark was reset and triangulated again during step k + 1 keeps its new landmark.  Nothing else
 *               of the state is written.
 * Faulted steps.  A lane whose sticky fault word is set when the write-back runs (step k + 1 left the device-only path; a
 *   logical flag, what vo_pipeline_config.debug_fault_every forces) is left untouched, like every kernel behind such a step;
 *   vo_pipeline_collect_all queues that lane's write-back again behind the redone step and in front of the chains it enqueues
 *   again, so the redone step's features receive it exactly as they would have without the fault.
 * Ordering.  All of it is main-stream work enqueued before the next submit, so nothing of step k + 2 that reads landmarks runs
 *   before the write-back; the tracker, detection and upload streams read keypoints, images and pyramids only.
 * Hand-over.  vo_structure_loop_reset_seq forgets a lane's window (call it wherever a lane is handed a new state: ids start
 *   again).  A restart or bootstrap without it is still caught by the header check, as is a rewind.
 * Results.  Every post leaves one vo_structure_loop_entry per lane (an idle lane: step = -1, all else 0), copied
 *   asynchronously into a pinned ring of the last 64 posts.  vo_structure_loop_poll(post_index -- posts count from 0 --, wait,
 *   entries[S]): VO_OK with the entries; 1 when wait = 0 and the copy has not landed yet (it has once a step submitted after the
 *   post has been collected); wait != 0 blocks on the post's event.  post itself never synchronises with running work.
 *
 * vo_structure_loop_create: window 2 .. 16; L_cap 0 = the pipeline's feature capacity; M_cap 0 = L_cap * window; params: all 0 =
 *   vo_structure_params' defaults (checked at the first post).  One loop per pipeline; VO_EINVAL with a message for a pipeline
 *   without track_ids, tracker_mode != 0, a window out of range, a second loop, and at post for two steps in flight.
 * vo_structure_loop_download_seq: lane seq's last window -- head (4), poses (W x 12), lm_start (L_cap + 1), obs_slot (M_cap),
 *   obs_xy (M_cap x 2), X_in (L_cap x 3, the join's), lm_id (L_cap), X (L_cap x 3, refined), results (L_cap), summary, entry;
 *   any pointer may be NULL; entries beyond L / M are not defined.  Synchronises: for tests and tools.
 * vo_structure_loop_destroy waits for the stream and releases the loop; vo_pipeline_destroy does it for a loop still attached. */
typedef struct vo_structure_loop vo_structure_loop;
typedef struct vo_structure_loop_config {
  int32_t window;                         /* W, 2 .. 16 */
  int32_t L_cap, M_cap;                   /* 0 = the feature capacity, L_cap * window */
  int32_t feedback;                       /* 1: item 5 */
  vo_structure_params params;
} vo_structure_loop_config;
typedef struct vo_structure_loop_entry {  /* per lane and post */
  int32_t step;                           /* the posted record's step counter; -1: the lane posted nothing */
  int32_t full;
  int32_t L, M, flags;                    /* the join's head */
  int32_t n_written;                      /* features the write-back wrote */
  vo_structure_summary summary;
} vo_structure_loop_entry;
int vo_structure_loop_create(vo_pipeline* p, const vo_structure_loop_config* cfg, vo_structure_loop** out);
int vo_structure_loop_post(vo_structure_loop* loop, const vo_step_result* results /* S, as vo_pipeline_collect_all returned them */);
int vo_structure_loop_posts(vo_structure_loop* loop);      /* posts made so far */
int vo_structure_loop_reset_seq(vo_structure_loop* loop, int seq);
int vo_structure_loop_poll(vo_structure_loop* loop, int post_index, int wait, vo_structure_loop_entry* entries);
int vo_structure_loop_download_seq(vo_structure_loop* loop, int seq, int32_t* head, double* poses, int32_t* lm_start, int32_t* obs_slot,
                                   double* obs_xy, double* X_in, int32_t* lm_id, double* X, vo_structure_result* results,
                                   vo_structure_summary* summary, vo_structure_loop_entry* entry);
int vo_structure_loop_destroy(vo_structure_loop* loop);

/* ---- shared map over RCCL ------------------------------------------------------------------
 * The reference is one process and one thread (README.md:49); frame streams shard at sequence granularity (one
 * process per GPU) and the ranks share {pose, landmarks} through ONE collective: an all-gather of a
 * fixed-size record per rank, [T_cw 4x4 (16) | n (1) | n landmarks x 3, n <= cap] float64 = 17 + 3 cap doubles
 * (what vo_pipeline_export_state_post writes).  A host that is not PyTorch (bench.py drives the same exchange through
 * torch.distributed) makes a communicator from an id rank 0 creates and hands to the other ranks by its own means
 * (MPI, a file, a socket):
 *   vo_comm_unique_id   128 bytes (ncclUniqueId)
 *   vo_comm_create      ncclCommInitRank on the context's device; collective: every rank calls it
 *   vo_allgather_state_dev  ncclAllGather of doubles_per_rank doubles per rank, device pointers, asynchronous on
 *                       `stream` (NULL: the context's).  One or several frames' records per call: records of k frames
 *                       posted back to back are one message of k (17 + 3 cap) doubles.
 *   vo_allgather_state  host arrays, one record, synchronous: pose16 (T_cw), landmarks n*3 -> all: world records.
 * RCCL is opened at the first call (the process's own copy if it has one), not linked.                          */
#define VO_COMM_ID_BYTES 128
typedef struct vo_comm vo_comm;
int vo_comm_unique_id(vo_ctx* ctx, void* id128);
int vo_comm_create(vo_ctx* ctx, int world, int rank, const void* id128, vo_comm** out);
void vo_comm_destroy(vo_comm* c);
int vo_comm_world(const vo_comm* c);
int vo_allgather_state_dev(vo_ctx* ctx, vo_comm* c, const double* d_records, size_t doubles_per_rank, double* d_all,
                           void* stream);
int vo_allgather_state(vo_ctx* ctx, vo_comm* c, const double* pose16, const double* landmarks, int n, int cap,
                       double* all);

#ifdef __cplusplus
}
#endif
#endif /* VO_HIP_H */
