// Frame pipeline: the two-view bootstrap from two frames of the frame store (vo_hip.h, vo_pipeline_bootstrap_seq).
//
// The stages are the kernels the host route (vo/driver.py: bootstrap) calls one ABI call at a time -- Shi-Tomasi corners,
// pyramids + LK, 8-point hypotheses / scores / closing fit, relative pose -- in their device-resident forms; the
// bookkeeping between them, NumPy on the host route, is three small kernels here:
//   boot_gather_kernel      klt.py:244-262 + matches.py:26-212 for fresh Features and identity pairs: the survivors of
//                           status & err < thr, in order, as the float64 (n, 2) pairs the bootstrap kernels read.  The
//                           fresh frame-a Features block is never materialised: all its fields are constants (state 0,
//                           track = keypoint, pose = identity, landmark NaN) that the apply kernel writes where they survive.
//   boot_unpack_mask_kernel the accepted hypothesis' packed inlier row -> one byte per correspondence
//   bootstrap_apply_kernel  driver.py: bootstrap after triangulate_matches (update_with_local_pose,
//                           update_with_local_landmarks incl. _check_landmarks, reset_outliers) into the lane's current
//                           Features block and control block
// Everything before the apply kernel writes workspace only, so a failed call leaves the lane as it was.
#include "pipeline.h"

#pragma clang fp contract(off)

namespace {

constexpr int BOOT_BATCH = 2048;     // RANSAC samples per launch (what crosses PCIe per batch: 64 KiB up, 8 KiB down)

// One workgroup walks the n0 tracked corners in order, 256 at a time (ballot + prefix: the survivors keep their order).
__global__ __launch_bounds__(256) void boot_gather_kernel(const float* __restrict__ xy_a, const float* __restrict__ xy_b,
                                                          const uint8_t* __restrict__ status, const float* __restrict__ err,
                                                          float err_thr, int n0, double* __restrict__ p1,
                                                          double* __restrict__ p2, int32_t* __restrict__ n_out) {
  __shared__ int s_cnt[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int base = 0;
  for (int i0 = 0; i0 < n0; i0 += 256) {
    const int i = i0 + t;
    const bool keep = i < n0 && status[i] != 0 && err[i] < err_thr;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_cnt[wv] = (int)__popcll(bal);
    __syncthreads();
    int before = (int)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wv) before += s_cnt[w];
      total += s_cnt[w];
    }
    if (keep) {
      const int k = base + before;       // k <= i < n0 <= the arrays' capacity
      p1[2 * k] = (double)xy_a[2 * i];
      p1[2 * k + 1] = (double)xy_a[2 * i + 1];
      p2[2 * k] = (double)xy_b[2 * i];
      p2[2 * k + 1] = (double)xy_b[2 * i + 1];
    }
    base += total;
    __syncthreads();
  }
  if (t == 0) *n_out = base;
}

__global__ __launch_bounds__(256) void boot_unpack_mask_kernel(const unsigned long long* __restrict__ row, int n,
                                                               uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) mask[i] = (uint8_t)((row[i >> 6] >> (i & 63)) & 1ull);
}

struct boot_apply_args {
  int n, num_features;
  int keep_ransac, keep_raw_pos;       // 1: the control block's RANSAC fields / generator position stay
  int64_t n_iterations;
  double outlier_ratio;
  uint64_t raw_pos;
};

// One workgroup (n <= feature capacity).  mask = RANSAC inlier AND in front of both cameras (relative_pose_kernel's), X the
// winner's triangulation of every correspondence, M camera a -> camera b.  With prev_pose = identity:
//   curr_pose = inv(M4) (closed form: [R^T | -R^T t]), world landmarks = X;
//   update_with_local_landmarks: masked features -> state 2 with X, then _check_landmarks drops those behind either camera;
//   reset_outliers(behind), reset_outliers(~mask): state 0, track = own keypoint, start pose = curr_pose.
__global__ __launch_bounds__(256) void bootstrap_apply_kernel(boot_apply_args a, const double* __restrict__ p1,
                                                              const double* __restrict__ p2, const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ X, const double* __restrict__ Min,
                                                              vo_feat F, vo_seq_ctl* __restrict__ ctl,
                                                              int32_t* __restrict__ n_land_out) {
  __shared__ double s_M[12], s_T[12];
  __shared__ int s_land;
  const int t = threadIdx.x;
  if (t < 12) s_M[t] = Min[t];
  if (t == 0) s_land = 0;
  __syncthreads();
  if (t < 12) {
    const int r = t >> 2, c = t & 3;
    s_T[t] = c < 3 ? s_M[4 * c + r] : -(s_M[r] * s_M[3] + s_M[4 + r] * s_M[7] + s_M[8 + r] * s_M[11]);
  }
  __syncthreads();
  int mine = 0;
  for (int i = t; i < a.n; i += 256) {
    const double kx = p2[2 * i], ky = p2[2 * i + 1];
    F.kp[2 * i] = (float)kx;             // (LK's float32 output widened by the gather: exact both ways)
    F.kp[2 * i + 1] = (float)ky;
    F.kp64[2 * i] = kx;
    F.kp64[2 * i + 1] = ky;
    F.cand[i] = 0;
    bool tri = mask[i] != 0;
    const double x = X[3 * i], y = X[3 * i + 1], z = X[3 * i + 2];
    if (tri) {
      // _check_landmarks (state.py:90-107): depth in the current camera (T_cw = M) and in the previous one (identity)
      const double z_curr = s_M[8] * x + s_M[9] * y + s_M[10] * z + s_M[11];
      if (z_curr < 0.0 || z < 0.0) tri = false;
    }
    if (tri) {
      F.state[i] = 2;
      F.land[3 * i] = x;
      F.land[3 * i + 1] = y;
      F.land[3 * i + 2] = z;
      F.track[2 * i] = p1[2 * i];
      F.track[2 * i + 1] = p1[2 * i + 1];
#pragma unroll
      for (int k = 0; k < 12; ++k) F.pose[(size_t)k * F.pitch + i] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
      ++mine;
    } else {
      F.state[i] = 0;
      F.land[3 * i] = F.land[3 * i + 1] = F.land[3 * i + 2] = NAN;
      F.track[2 * i] = kx;
      F.track[2 * i + 1] = ky;
#pragma unroll
      for (int k = 0; k < 12; ++k) F.pose[(size_t)k * F.pitch + i] = s_T[k];
    }
  }
  if (mine) atomicAdd(&s_land, mine);
  __syncthreads();
  if (t == 0) {
    // the control block starts over as in a hand-over (pipeline_state.hip: upload_state)
    const uint64_t raw_pos = a.keep_raw_pos ? ctl->raw_pos : a.raw_pos;
    const int64_t n_it = a.keep_ransac ? ctl->n_iterations : a.n_iterations;
    const double orat = a.keep_ransac ? ctl->outlier_ratio : a.outlier_ratio;
    vo_seq_ctl h;
    memset(&h, 0, sizeof(h));
    h.n = a.n;
    h.n2 = a.n;
    h.num_features = a.num_features;
    h.raw_pos = raw_pos;
    h.n_iterations = n_it;
    h.outlier_ratio = orat;
    for (int k = 0; k < 12; ++k) {
      const double id = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
      h.T_cw[k] = s_M[k];
      h.T_wc[k] = s_T[k];
      h.T_cw_prev[k] = id;
      h.T_wc_prev[k] = id;
    }
    *ctl = h;
    *n_land_out = s_land;
  }
}

}  // namespace

// the bootstrap's workspace, made at the first call and kept (the pyramids grow when a call asks for more levels)
struct vo_pipeline_boot {
  uint8_t* pyr[2] = {nullptr, nullptr};
  size_t pyr_bytes = 0;
  double *p1 = nullptr, *p2 = nullptr, *X = nullptr, *F = nullptr, *Fhyp = nullptr;   // F: [0..8] F, [16..27] M
  uint8_t *inl = nullptr, *mask = nullptr;
  int32_t *cnt = nullptr, *samples = nullptr, *counts = nullptr;
  uint64_t* masks = nullptr;
};
typedef vo_pipeline_boot boot_ws;

static int boot_workspace(vo_pipeline* p, size_t pyr_bytes) {
  if (!p->boot) {
    p->boot = new vo_pipeline_boot();
    boot_ws& w = *p->boot;
    const size_t cap = (size_t)p->cap, words = (cap + 63) / 64;
    VO_TRY(dev_alloc(p, &w.p1, cap * 2));
    VO_TRY(dev_alloc(p, &w.p2, cap * 2));
    VO_TRY(dev_alloc(p, &w.X, cap * 3));
    VO_TRY(dev_alloc(p, &w.F, (size_t)32));
    VO_TRY(dev_alloc(p, &w.Fhyp, (size_t)BOOT_BATCH * 9));
    VO_TRY(dev_alloc(p, &w.inl, cap));
    VO_TRY(dev_alloc(p, &w.mask, cap));
    VO_TRY(dev_alloc(p, &w.cnt, (size_t)4));
    VO_TRY(dev_alloc(p, &w.samples, (size_t)BOOT_BATCH * 8));
    VO_TRY(dev_alloc(p, &w.counts, (size_t)BOOT_BATCH));
    VO_TRY(dev_alloc(p, &w.masks, (size_t)BOOT_BATCH * words));
  }
  boot_ws& w = *p->boot;
  if (w.pyr_bytes < pyr_bytes) {         // (a smaller one stays the pipeline's until it is destroyed)
    w.pyr_bytes = 0;
    VO_TRY(dev_alloc(p, &w.pyr[0], pyr_bytes));
    VO_TRY(dev_alloc(p, &w.pyr[1], pyr_bytes));
    w.pyr_bytes = pyr_bytes;
  }
  return VO_OK;
}

void vo_pipeline_boot_free(vo_pipeline* p) {
  delete p->boot;
  p->boot = nullptr;
}

extern "C" {

void vo_bootstrap_default_rng(vo_pcg64* rng) {
  if (!rng) return;
  // np.random.default_rng(2023).bit_generator.state (SeedSequence(2023) -> PCG64)
  rng->state_hi = 0x184ac32b7f221091ull;
  rng->state_lo = 0xffd70343e3ad6855ull;
  rng->inc_hi = 0xd87b422d4eb3d641ull;
  rng->inc_lo = 0x40701e5547692d8dull;
  rng->has_uint32 = 0;
  rng->uinteger = 0;
}

int vo_pipeline_bootstrap_seq(vo_pipeline* p, int seq, int idx_a, int idx_b, const vo_bootstrap_params* prm,
                              const vo_pcg64* rng, vo_bootstrap_result* out) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  VO_REQUIRE(ctx, out, "pipeline_bootstrap: null result");
  memset(out, 0, sizeof(*out));
  VO_REQUIRE(ctx, c.tracker_mode == 0, "pipeline_bootstrap: KLT tracker mode only (the descriptor modes match descriptors)");
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_bootstrap: bad sequence index");
  VO_REQUIRE(ctx, idx_a >= 0 && idx_a < c.n_frames && idx_b >= 0 && idx_b < c.n_frames, "pipeline_bootstrap: bad frame index");
  VO_REQUIRE(ctx, idx_a != idx_b, "pipeline_bootstrap: the two frames are the same slot %d", idx_a);
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_bootstrap: %d submitted step(s) not collected", p->n_flight);
  // a running pipeline: the lane is restarted (vo_pipeline_restart_seq's rules); else this is a hand-over (_set_state_seq's)
  const bool restart = p->have_state && p->primed;
  if (restart) {
    VO_REQUIRE(ctx, p->seeded, "pipeline_bootstrap: seed the pipeline first");
    VO_REQUIRE(ctx, idx_b == p->prev_frame, "pipeline_bootstrap: frame slot %d is not the one the next step starts from (%d)",
               idx_b, p->prev_frame);
  } else {
    VO_REQUIRE(ctx, !(p->S > 1 && p->have_state && idx_b != p->prev_frame),
               "pipeline_bootstrap: sequence %d is handed over for frame %d, the others of this hand-over for frame %d", seq,
               idx_b, p->prev_frame);
  }
  vo_bootstrap_params q;
  memset(&q, 0, sizeof(q));
  if (prm) q = *prm;
  VO_REQUIRE(ctx, q.route == 0, "pipeline_bootstrap: route %d is not implemented", (int)q.route);
  const int max_corners = q.max_corners > 0 ? q.max_corners : c.n_keypoints;
  const double quality = q.quality > 0 ? q.quality : 0.01, min_dist = q.min_distance > 0 ? q.min_distance : 8.0;
  const int block = q.block > 0 ? q.block : 7;
  const int win = q.klt_win > 0 ? q.klt_win : c.klt_win;
  const int max_level = q.klt_max_level >= 0 && prm ? q.klt_max_level : c.klt_max_level;
  const double thr_px = q.threshold_px > 0 ? q.threshold_px : 0.25;
  const double orat0 = q.outlier_ratio > 0 ? q.outlier_ratio : 0.9, conf = q.confidence > 0 ? q.confidence : 0.999;
  const int64_t max_it = q.max_iterations > 0 ? q.max_iterations : 2000;
  VO_REQUIRE(ctx, max_corners <= p->cap, "pipeline_bootstrap: %d corners exceed the feature capacity %d", max_corners, p->cap);
  VO_REQUIRE(ctx, orat0 < 1.0 && conf < 1.0, "pipeline_bootstrap: outlier ratio and confidence must be below 1");
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the two frames are in HBM once their uploads (tracker's stream / the pinned upload stream) are over
  for (int idx : {idx_a, idx_b}) {
    VO_HIP_TRY(ctx, hipEventSynchronize(p->evImg[idx]));
    if (p->n_pinned[idx] > 0) VO_HIP_TRY(ctx, hipEventSynchronize(p->evUp[idx]));
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  const int64_t h2d0 = ctx->bytes_h2d, d2h0 = ctx->bytes_d2h;
  int64_t d2h = 0;                       // this file's own copies (scalars; it uploads nothing itself)
  const int nl = vo_klt_num_levels(c.H, c.W, win, max_level);
  VO_TRY(boot_workspace(p, vo_pyramid_bytes(c.H, c.W, nl)));
  boot_ws& w = *p->boot;
  const uint8_t *img_a = p->img(seq, idx_a), *img_b = p->img(seq, idx_b);

  // 1. Shi-Tomasi corners of frame a
  const float* d_xy = nullptr;
  int32_t n0 = 0;
  VO_TRY(vo_good_features_dev(ctx, img_a, c.H, c.W, nullptr, max_corners, quality, min_dist, block, &d_xy, &n0));
  out->n_corners = n0;
  out->bytes_d2h = ctx->bytes_d2h - d2h0;
  if (n0 < 8) return vo_set_error(ctx, VO_ETRACKING, "pipeline_bootstrap: %d corners on frame %d, the 8-point algorithm needs 8", n0, idx_a);
  if (n0 > p->cap) return vo_set_error(ctx, VO_ECAPACITY, "pipeline_bootstrap: %d corners exceed the feature capacity %d", n0, p->cap);

  // 2. pyramids with the bootstrap's level count, LK a -> b, the survivors as float64 pairs
  VO_TRY(vo_pyramid_build_batch_dev(ctx, img_a, 0, 1, c.H, c.W, nl, w.pyr[0], 0));
  VO_TRY(vo_pyramid_build_batch_dev(ctx, img_b, 0, 1, c.H, c.W, nl, w.pyr[1], 0));
  float* d_next = p->d_next + (size_t)seq * p->cap * 2;      // (the lane's tracker outputs: a step rewrites them)
  uint8_t* d_status = p->d_status + (size_t)seq * p->cap;
  float* d_err = p->d_err + (size_t)seq * p->cap;
  VO_TRY(vo_klt_track_ndev(ctx, img_a, w.pyr[0], img_b, w.pyr[1], c.H, c.W, nl, d_xy, n0, nullptr, win, c.klt_max_iter, c.klt_eps,
                           c.klt_min_eig, d_next, d_status, d_err));
  hipLaunchKernelGGL(boot_gather_kernel, dim3(1), dim3(256), 0, st, d_xy, (const float*)d_next, (const uint8_t*)d_status,
                     (const float*)d_err, (float)c.klt_err_threshold, (int)n0, w.p1, w.p2, w.cnt);
  VO_TRY(vo_check_launch(ctx, "boot_gather_kernel"));
  int32_t n = 0;
  VO_HIP_TRY(ctx, mcpy(st, &n, w.cnt, 4, hipMemcpyDeviceToHost));
  d2h += 4;
  out->n_tracked = n;
  out->bytes_d2h = ctx->bytes_d2h - d2h0 + d2h;
  if (n < 8) return vo_set_error(ctx, VO_ETRACKING, "pipeline_bootstrap: %d of %d corners tracked, the 8-point algorithm needs 8", n, n0);

  // 3. 8-point RANSAC: samples from the reference's generator on the host, hypotheses + counts on the device, the
  //    sequential accept / adapt rule over the counts on the host (vo_ransac_replay), the accepted row unpacked on the device
  const int words = vo_cdiv(n, 64);
  vo_ransac_state rs;
  rs.outlier_ratio = orat0;
  rs.confidence = conf;
  rs.max_iterations = max_it;
  rs.s = 8;
  rs.adaptive = 1;
  {
    const int64_t k0 = vo_ransac_num_iterations(conf, orat0, 8);
    rs.n_iterations = k0 < max_it ? k0 : max_it;
  }
  vo_pcg64 gen;
  vo_bootstrap_default_rng(&gen);
  std::vector<int32_t> samples((size_t)BOOT_BATCH * 8), counts((size_t)BOOT_BATCH);
  const std::vector<uint8_t> valid((size_t)BOOT_BATCH, 1);
  int64_t n_done = 0;
  int32_t best_count = -1, best_idx = -1;
  int finished = 0;
  for (int batch = 0; !finished; ++batch) {
    vo_pcg64 spec = gen;                 // speculative copy: the generator moves by what the rule consumed
    if (vo_rng_choice(&spec, n, 8, BOOT_BATCH, samples.data()) != VO_OK)
      return vo_set_error(ctx, VO_EINVAL, "pipeline_bootstrap: cannot draw 8 of %d", n);
    VO_TRY(vo_fundamental_hypotheses_dev(ctx, w.p1, w.p2, n, samples.data(), BOOT_BATCH, 1, 1, thr_px * thr_px, w.samples, w.Fhyp,
                                         w.counts, w.masks, counts.data()));
    const int32_t before = best_idx;
    int consumed = 0;
    if (vo_ransac_replay(&rs, valid.data(), counts.data(), BOOT_BATCH, n, &n_done, &best_count, &best_idx, batch * BOOT_BATCH,
                         &consumed, &finished) != VO_OK)
      return vo_set_error(ctx, VO_EINVAL, "pipeline_bootstrap: vo_ransac_replay failed");
    if (best_idx != before) {
      const int row = best_idx - batch * BOOT_BATCH;       // 0 .. BOOT_BATCH - 1: an index of this batch
      hipLaunchKernelGGL(boot_unpack_mask_kernel, dim3(vo_cdiv(n, 256)), dim3(256), 0, st,
                         (const unsigned long long*)w.masks + (size_t)row * words, (int)n, w.inl);
      VO_TRY(vo_check_launch(ctx, "boot_unpack_mask_kernel"));
    }
    vo_rng_choice(&gen, n, 8, consumed, samples.data());
  }
  out->ransac_iterations = n_done;
  out->n_ransac_inliers = best_count < 0 ? 0 : best_count;
  out->bytes_h2d = ctx->bytes_h2d - h2d0;
  out->bytes_d2h = ctx->bytes_d2h - d2h0 + d2h;
  if (best_idx < 0 || best_count < 8)
    return vo_set_error(ctx, VO_ETRACKING, "pipeline_bootstrap: RANSAC found no model with 8 inliers among %d correspondences (best: %d)",
                        n, (int)best_count);
  VO_TRY(vo_fundamental_fit_dev(ctx, w.p1, w.p2, n, w.inl, 1, w.F, nullptr));
  const double* K = p->cams[(size_t)seq].K;
  VO_TRY(vo_relative_pose_dev(ctx, w.p1, w.p2, n, w.inl, K, K, w.F, w.F + 16, w.X, w.mask, nullptr));

  // 4. + 5. the lane's Features block and control block
  boot_apply_args a;
  a.n = n;
  a.num_features = n0;
  a.keep_ransac = (!restart && p->seq_state[seq] != 0) ? 1 : 0;
  a.keep_raw_pos = (restart || rng) ? 0 : 1;
  a.raw_pos = p->gen_upto[seq];
  a.outlier_ratio = c.ransac_outlier_ratio;        // RANSAC.__init__ (ransac.py:47-56), as upload_state writes it
  {
    const int64_t k0 = vo_ransac_num_iterations(c.ransac_confidence, c.ransac_outlier_ratio, 4);
    a.n_iterations = (c.ransac_max_iterations >= 0 && c.ransac_max_iterations < k0) ? c.ransac_max_iterations : k0;
  }
  hipLaunchKernelGGL(bootstrap_apply_kernel, dim3(1), dim3(256), 0, st, a, (const double*)w.p1, (const double*)w.p2,
                     (const uint8_t*)w.mask, (const double*)w.X, (const double*)(w.F + 16), vo_feat_seq(p->F[p->cur], (size_t)seq),
                     p->d_ctl + seq, w.cnt + 1);
  VO_TRY(vo_check_launch(ctx, "bootstrap_apply_kernel"));
  int32_t n_land = 0;
  VO_HIP_TRY(ctx, hipMemcpyAsync(out->M, w.F + 16, 96, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, mcpy(st, &n_land, w.cnt + 1, 4, hipMemcpyDeviceToHost));
  d2h += 100;
  out->n_landmarks = n_land;
  out->n_features = n;
  out->bytes_h2d = ctx->bytes_h2d - h2d0;
  out->bytes_d2h = ctx->bytes_d2h - d2h0 + d2h;
  // host side of the hand-over (pipeline_state.hip: vo_pipeline_set_state_seq / vo_pipeline_restart_seq)
  if (restart || rng) {
    const vo_pcg64 g = rng ? *rng : p->seed_rng;
    p->rng[seq] = g;
    p->raw_gen[seq] = g;
    p->pos_known[seq] = p->gen_upto[seq];
    p->pos_dev[seq] = p->gen_upto[seq];
  }
  p->idle[seq] = 0;
  p->seq_state[seq] = 1;
  if (restart) {
    p->prepared_idx = p->prepared_slot = -1;
    VO_TRY(prime(p, true, seq, 1));
  } else {
    p->slot = 0;
    p->prev_frame = idx_b;
    p->have_state = true;
    p->primed = false;
  }
  return VO_OK;
}

int vo_pipeline_bootstrap(vo_pipeline* p, int idx_a, int idx_b, const vo_bootstrap_params* prm, vo_bootstrap_result* out) {
  return vo_pipeline_bootstrap_seq(p, 0, idx_a, idx_b, prm, nullptr, out);
}

}  // extern "C"
