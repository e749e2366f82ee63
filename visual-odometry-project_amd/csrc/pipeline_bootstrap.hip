// Frame pipeline: the two-view bootstrap from two frames of the frame store, for any subset of the lanes through one set
// of launches (vo_hip.h, vo_pipeline_bootstrap_lanes; vo_pipeline_bootstrap_seq is its one-lane call).
//
// The stages are the kernels the host route (vo/driver.py: bootstrap) calls one ABI call at a time -- Shi-Tomasi corners,
// pyramids + LK, the 8-point RANSAC loop with its closing fit, relative pose -- in their device-resident forms, with the
// lane as a grid dimension of every stage (Shi-Tomasi: vo_good_features_batch_dev, straight into the lanes' blocks); the
// bookkeeping between them, NumPy on the host route, is three small kernels here:
//   boot_corners_kernel     the lanes' corner counts as the following stages read them (a lane with fewer than 8
//                           corners, or whose detection failed, sits out)
//   boot_gather_kernel      klt.py:244-262 + matches.py:26-212 for fresh Features and identity pairs: the survivors of
//                           status & err < thr, in order, as the float64 (n, 2) pairs the bootstrap kernels read.  The
//                           fresh frame-a Features block is never materialised: all its fields are constants (state 0,
//                           track = keypoint, pose = identity, landmark NaN) that the apply kernel writes where they survive.
//   bootstrap_apply_kernel  driver.py: bootstrap after triangulate_matches (update_with_local_pose,
//                           update_with_local_landmarks incl. _check_landmarks, reset_outliers) into the lane's current
//                           Features block and control block
// Everything before the apply kernel writes workspace only, and the apply kernel skips a lane whose RANSAC did not end
// with a model, so a lane that fails is left as it was while the others go through.
#include "pipeline.h"

#pragma clang fp contract(off)

namespace {

// Lane k of a call (its position in the call, not its number) owns block k of every workspace array.
struct boot_lanes {
  size_t xy;        // floats between the lanes' corner / tracker-output arrays
  size_t out;       // elements between their status / err arrays
  size_t pts;       // doubles between their p1 / p2 arrays
};

// Shi-Tomasi's counts -> the lanes' count blocks.  cnt: four ints per lane -- [0] corners the following stages work on (0:
// the lane sits out), [3] what the host is told with the result: the corners found, or -d_over when the detection failed
__global__ __launch_bounds__(64) void boot_corners_kernel(int L, int cap, const int32_t* __restrict__ n, const int32_t* __restrict__ over,
                                                          int32_t* __restrict__ cnt) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= L) return;
  const int n0 = n[k], ov = over[k];
  cnt[4 * k] = (ov == 0 && n0 >= 8 && n0 <= cap) ? n0 : 0;
  cnt[4 * k + 1] = 0;
  cnt[4 * k + 2] = 0;
  cnt[4 * k + 3] = ov ? -ov : n0;
}

// One workgroup per lane walks its n0 tracked corners in order, 256 at a time (ballot + prefix: the survivors keep their
// order).  cnt: four ints per lane -- [0] corners (in), [1] survivors (out).
__global__ __launch_bounds__(256) void boot_gather_kernel(const float* __restrict__ xy_a, const float* __restrict__ xy_b,
                                                          const uint8_t* __restrict__ status, const float* __restrict__ err,
                                                          float err_thr, boot_lanes ln, double* __restrict__ p1,
                                                          double* __restrict__ p2, int32_t* __restrict__ cnt) {
  __shared__ int s_cnt[4];
  const size_t q = blockIdx.x;
  xy_a += q * ln.xy;
  xy_b += q * ln.xy;
  status += q * ln.out;
  err += q * ln.out;
  p1 += q * ln.pts;
  p2 += q * ln.pts;
  cnt += q * 4;
  const int n0 = cnt[0];
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
  if (t == 0) cnt[1] = base;
}

struct boot_apply_lane {      // what the host knows of a lane (uploaded: 24 bytes per lane)
  int32_t seq;                // the lane's number
  int32_t keep_ransac, keep_raw_pos;       // 1: the control block's RANSAC fields / generator position stay
  int32_t pad;
  uint64_t raw_pos;
};
struct boot_apply_args {
  int64_t n_iterations;
  double outlier_ratio;
  size_t pts, X, F, mask;     // strides of the workspace blocks (doubles, doubles, doubles, bytes)
};

// One workgroup per lane (n <= feature capacity); lanes whose RANSAC did not end with a model are left as they were.
// mask = RANSAC inlier AND in front of both cameras (relative_pose_kernel's), X the winner's triangulation of every
// correspondence, M camera a -> camera b.  With prev_pose = identity:
//   curr_pose = inv(M4) (closed form: [R^T | -R^T t]), world landmarks = X;
//   update_with_local_landmarks: masked features -> state 2 with X, then _check_landmarks drops those behind either camera;
//   reset_outliers(behind), reset_outliers(~mask): state 0, track = own keypoint, start pose = curr_pose.
__global__ __launch_bounds__(256) void bootstrap_apply_kernel(boot_apply_args g, const boot_apply_lane* __restrict__ lanes,
                                                              const vo_f8_ctl* __restrict__ f8, const double* __restrict__ p1,
                                                              const double* __restrict__ p2, const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ X, const double* __restrict__ Min,
                                                              vo_feat Fall, vo_seq_ctl* __restrict__ ctls,
                                                              int32_t* __restrict__ cnt) {
  const size_t q = blockIdx.x;
  if (f8[q].status != VO_F8_DONE) return;
  const boot_apply_lane a = lanes[q];
  const int a_n = f8[q].n, a_num_features = cnt[4 * q];
  p1 += q * g.pts;
  p2 += q * g.pts;
  mask += q * g.mask;
  X += q * g.X;
  Min += q * g.F;
  const vo_feat F = vo_feat_seq(Fall, (size_t)a.seq);
  vo_seq_ctl* ctl = ctls + a.seq;
  int32_t* n_land_out = cnt + 4 * q + 2;
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
  for (int i = t; i < a_n; i += 256) {
    const double kx = p2[2 * i], ky = p2[2 * i + 1];
    F.kp[2 * i] = (float)kx;             // (LK's float32 output widened by the gather: exact both ways)
    F.kp[2 * i + 1] = (float)ky;
    F.kp64[2 * i] = kx;
    F.kp64[2 * i + 1] = ky;
    F.cand[i] = 0;
    if (F.ids) F.ids[i] = make_int2(i, 0);     // (track ids: a hand-over numbers the features in their order, born 0)
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
    const int64_t n_it = a.keep_ransac ? ctl->n_iterations : g.n_iterations;
    const double orat = a.keep_ransac ? ctl->outlier_ratio : g.outlier_ratio;
    vo_seq_ctl h;
    memset(&h, 0, sizeof(h));
    h.n = a_n;
    h.n2 = a_n;
    h.num_features = a_num_features;
    h.nf[0] = h.nf[1] = a_num_features;
    h.next_id[0] = h.next_id[1] = a_n;
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

// The bootstrap's workspace: one block per lane of a call (by its position in the call), grown to the largest lane count
// seen and kept (the pyramids also grow when a call asks for more levels).  Superseded blocks stay the pipeline's until it
// is destroyed.
struct vo_pipeline_boot {
  int lanes = 0;
  size_t pyr_bytes = 0;
  uint8_t* pyr[2] = {nullptr, nullptr};          // [lanes][pyr_bytes]
  float *xy = nullptr, *next = nullptr, *err = nullptr;     // corners of frame a, LK's outputs: [lanes][cap * 2], [lanes][cap]
  uint8_t* status = nullptr;
  double *p1 = nullptr, *p2 = nullptr, *X = nullptr, *F = nullptr;   // F: 32 doubles per lane, [0..8] F, [16..27] M
  uint8_t *inl = nullptr, *mask = nullptr;
  int32_t *cnt = nullptr, *seq = nullptr;        // cnt: four ints per lane (corners, survivors, landmarks, corners found)
  int32_t* gf = nullptr;                         // Shi-Tomasi's d_n [lanes], d_over [lanes]
  boot_apply_lane* apply = nullptr;
};
typedef vo_pipeline_boot boot_ws;

static int boot_workspace(vo_pipeline* p, int L, size_t pyr_bytes) {
  if (!p->boot) p->boot = new vo_pipeline_boot();
  boot_ws& w = *p->boot;
  const size_t cap = (size_t)p->cap;
  if (w.lanes < L) {
    w.lanes = 0;
    w.pyr_bytes = 0;
    VO_TRY(dev_alloc(p, &w.xy, L * cap * 2));
    VO_TRY(dev_alloc(p, &w.next, L * cap * 2));
    VO_TRY(dev_alloc(p, &w.err, L * cap));
    VO_TRY(dev_alloc(p, &w.status, L * cap));
    VO_TRY(dev_alloc(p, &w.p1, L * cap * 2));
    VO_TRY(dev_alloc(p, &w.p2, L * cap * 2));
    VO_TRY(dev_alloc(p, &w.X, L * cap * 3));
    VO_TRY(dev_alloc(p, &w.F, (size_t)L * 32));
    VO_TRY(dev_alloc(p, &w.inl, L * cap));
    VO_TRY(dev_alloc(p, &w.mask, L * cap));
    VO_TRY(dev_alloc(p, &w.cnt, (size_t)L * 4));
    VO_TRY(dev_alloc(p, &w.seq, (size_t)L));
    VO_TRY(dev_alloc(p, &w.gf, (size_t)L * 2));
    VO_TRY(dev_alloc(p, &w.apply, (size_t)L));
    w.lanes = L;
  }
  if (w.pyr_bytes < pyr_bytes) {
    w.pyr_bytes = 0;
    VO_TRY(dev_alloc(p, &w.pyr[0], (size_t)w.lanes * pyr_bytes));
    VO_TRY(dev_alloc(p, &w.pyr[1], (size_t)w.lanes * pyr_bytes));
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

int vo_pipeline_bootstrap_lanes(vo_pipeline* p, int n_lanes, const int32_t* seqs, int idx_a, int idx_b,
                                const vo_bootstrap_params* prm, const vo_pcg64* rngs, vo_bootstrap_result* outs, int32_t* status) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  const int L = n_lanes;
  VO_REQUIRE(ctx, outs && seqs && L >= 1, "pipeline_bootstrap: null result or no lane");
  VO_REQUIRE(ctx, c.tracker_mode == 0, "pipeline_bootstrap: KLT tracker mode only (the descriptor modes match descriptors)");
  VO_REQUIRE(ctx, L <= p->S, "pipeline_bootstrap: %d lanes named, the pipeline has %d", L, p->S);
  for (int k = 0; k < L; ++k) {
    VO_REQUIRE(ctx, seqs[k] >= 0 && seqs[k] < p->S, "pipeline_bootstrap: bad sequence index %d", (int)seqs[k]);
    for (int j = 0; j < k; ++j) VO_REQUIRE(ctx, seqs[j] != seqs[k], "pipeline_bootstrap: sequence %d is named twice", (int)seqs[k]);
  }
  VO_REQUIRE(ctx, idx_a >= 0 && idx_a < c.n_frames && idx_b >= 0 && idx_b < c.n_frames, "pipeline_bootstrap: bad frame index");
  VO_REQUIRE(ctx, idx_a != idx_b, "pipeline_bootstrap: the two frames are the same slot %d", idx_a);
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_bootstrap: %d submitted step(s) not collected", p->n_flight);
  // a running pipeline: the lanes are restarted (vo_pipeline_restart_seq's rules); else this is a hand-over (_set_state_seq's)
  const bool restart = p->have_state && p->primed;
  if (restart) {
    VO_REQUIRE(ctx, p->seeded, "pipeline_bootstrap: seed the pipeline first");
    VO_REQUIRE(ctx, idx_b == p->prev_frame, "pipeline_bootstrap: frame slot %d is not the one the next step starts from (%d)",
               idx_b, p->prev_frame);
  } else {
    VO_REQUIRE(ctx, !(p->S > 1 && p->have_state && idx_b != p->prev_frame),
               "pipeline_bootstrap: sequence %d is handed over for frame %d, the others of this hand-over for frame %d",
               (int)seqs[0], idx_b, p->prev_frame);
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
  memset(outs, 0, sizeof(*outs) * (size_t)L);
  std::vector<int32_t> code((size_t)L, VO_OK);
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
  int64_t h2d = 0, d2h = 0;              // this file's own copies (scalars)
  const int nl = vo_klt_num_levels(c.H, c.W, win, max_level);
  const size_t pyr_bytes = vo_pyramid_bytes(c.H, c.W, nl);
  VO_TRY(boot_workspace(p, L, pyr_bytes));
  boot_ws& w = *p->boot;
  const size_t cap = (size_t)p->cap;
  // the first failure's text is the call's (the lane named in it); every lane's code goes to status[]
  int first_fail = -1;
  char first_msg[sizeof(ctx->err)] = {0};
  auto fail = [&](int k, int rc) {
    code[(size_t)k] = rc;
    if (first_fail < 0) {
      first_fail = k;
      snprintf(first_msg, sizeof(first_msg), "%s", ctx->err);
    }
  };

  // 1. Shi-Tomasi corners of frame a, straight into the lanes' blocks (one call per run of consecutive lanes); their counts
  //    stay on the device and reach the host with the result's download
  for (int k = 0; k < L;) {
    int run = 1;
    while (k + run < L && seqs[k + run] == seqs[k] + run) ++run;
    VO_TRY(vo_good_features_batch_dev(ctx, p->img(seqs[k], idx_a), p->img_stride(), run, c.H, c.W, nullptr, 0, max_corners, quality,
                                      min_dist, block, w.xy + (size_t)k * cap * 2, cap, w.gf + k, w.gf + L + k, nullptr));
    k += run;
  }
  hipLaunchKernelGGL(boot_corners_kernel, dim3(vo_cdiv(L, 64)), dim3(64), 0, st, L, p->cap, (const int32_t*)w.gf,
                     (const int32_t*)(w.gf + L), w.cnt);
  VO_TRY(vo_check_launch(ctx, "boot_corners_kernel"));
  const int n0_max = max_corners;

  vo_f8_lanes ln;
  ln.L = L;
  ln.pts = cap * 2;
  ln.inl = cap;
  ln.F = 32;
  ln.n = 4;
  std::vector<vo_f8_result> rs((size_t)L);
  std::vector<vo_pcg64> gens((size_t)L);
  {
    // 2. pyramids with the bootstrap's level count (one launch per run of consecutive lanes), LK a -> b for all lanes, the
    //    survivors as float64 pairs
    for (int k = 0; k < L;) {
      int run = 1;
      while (k + run < L && seqs[k + run] == seqs[k] + run) ++run;
      VO_TRY(vo_pyramid_build_batch_dev(ctx, p->img(seqs[k], idx_a), p->img_stride(), run, c.H, c.W, nl, w.pyr[0] + (size_t)k * pyr_bytes, pyr_bytes));
      VO_TRY(vo_pyramid_build_batch_dev(ctx, p->img(seqs[k], idx_b), p->img_stride(), run, c.H, c.W, nl, w.pyr[1] + (size_t)k * pyr_bytes, pyr_bytes));
      k += run;
    }
    vo_klt_source src;                   // the lanes' corner counts are read on the device (no detector keypoints: frac = 0)
    src.n = w.cnt;
    src.num_features = w.cnt;
    vo_klt_batch kb;
    kb.S = L;
    kb.pyr = pyr_bytes;
    kb.xy = cap * 2;
    kb.out = cap;
    kb.ctl = 16;
    VO_TRY(vo_klt_track_ndev(ctx, p->img(seqs[0], idx_a), w.pyr[0], p->img(seqs[0], idx_b), w.pyr[1], c.H, c.W, nl, w.xy, n0_max, nullptr,
                             win, c.klt_max_iter, c.klt_eps, c.klt_min_eig, w.next, w.status, w.err, &src, &kb));
    boot_lanes bl;
    bl.xy = cap * 2;
    bl.out = cap;
    bl.pts = cap * 2;
    hipLaunchKernelGGL(boot_gather_kernel, dim3(L), dim3(256), 0, st, (const float*)w.xy, (const float*)w.next,
                       (const uint8_t*)w.status, (const float*)w.err, (float)c.klt_err_threshold, bl, w.p1, w.p2, w.cnt);
    VO_TRY(vo_check_launch(ctx, "boot_gather_kernel"));

    // 3. 8-point RANSAC on the device (sampler, hypotheses, scores, the accept / adapt rule), its closing fit, the relative
    //    pose: grid x lanes.  The survivor counts never come to the host on their own: they arrive with the loops' control
    //    blocks (one download for all lanes); a lane with fewer than 8 survivors leaves every kernel at once.
    vo_f8_params fp;
    fp.normalize_samples = 1;
    fp.error_kind = 1;
    fp.threshold = thr_px * thr_px;
    fp.outlier_ratio = orat0;
    fp.confidence = conf;
    fp.max_iterations = max_it;
    for (int k = 0; k < L; ++k) vo_bootstrap_default_rng(&gens[(size_t)k]);
    VO_TRY(vo_fundamental_ransac_dev(ctx, w.p1, w.p2, p->cap, w.cnt + 1, nullptr, fp, gens.data(), w.inl, w.F, &ln, rs.data()));
    std::vector<boot_apply_lane> al((size_t)L);
    for (int k = 0; k < L; ++k) {
      const int seq = seqs[k];
      boot_apply_lane& a = al[(size_t)k];
      memset(&a, 0, sizeof(a));
      a.seq = seq;
      a.keep_ransac = (!restart && p->seq_state[seq] != 0) ? 1 : 0;
      a.keep_raw_pos = (restart || rngs) ? 0 : 1;
      a.raw_pos = p->gen_upto[seq];
    }
    VO_HIP_TRY(ctx, hipMemcpyAsync(w.seq, seqs, (size_t)L * 4, hipMemcpyHostToDevice, st));
    VO_HIP_TRY(ctx, hipMemcpyAsync(w.apply, al.data(), (size_t)L * sizeof(boot_apply_lane), hipMemcpyHostToDevice, st));
    h2d += (int64_t)L * (4 + (int64_t)sizeof(boot_apply_lane));
    VO_TRY(vo_relative_pose_lanes_dev(ctx, w.p1, w.p2, ln, w.inl, w.F, (const double*)p->d_cams, sizeof(vo_cam) / 8, w.seq, w.F + 16,
                                      w.X, cap * 3, w.mask));

    // 4. + 5. the lanes' Features blocks and control blocks (a lane without a model is left as it was)
    boot_apply_args g;
    g.outlier_ratio = c.ransac_outlier_ratio;        // RANSAC.__init__ (ransac.py:47-56), as upload_state writes it
    {
      const int64_t k0 = vo_ransac_num_iterations(c.ransac_confidence, c.ransac_outlier_ratio, 4);
      g.n_iterations = (c.ransac_max_iterations >= 0 && c.ransac_max_iterations < k0) ? c.ransac_max_iterations : k0;
    }
    g.pts = cap * 2;
    g.X = cap * 3;
    g.F = 32;
    g.mask = cap;
    hipLaunchKernelGGL(bootstrap_apply_kernel, dim3(L), dim3(256), 0, st, g, (const boot_apply_lane*)w.apply,
                       (const vo_f8_ctl*)ctx->f8_ctl.p, (const double*)w.p1, (const double*)w.p2, (const uint8_t*)w.mask,
                       (const double*)w.X, (const double*)(w.F + 16), p->F[p->cur], p->d_ctl, w.cnt);
    VO_TRY(vo_check_launch(ctx, "bootstrap_apply_kernel"));
    std::vector<double> hF((size_t)L * 32);
    std::vector<int32_t> hcnt((size_t)L * 4);
    VO_HIP_TRY(ctx, hipMemcpyAsync(hF.data(), w.F, (size_t)L * 256, hipMemcpyDeviceToHost, st));
    VO_HIP_TRY(ctx, mcpy(st, hcnt.data(), w.cnt, (size_t)L * 16, hipMemcpyDeviceToHost));
    d2h += (int64_t)L * (256 + 16);
    for (int k = 0; k < L; ++k) {        // the corner stage's failures first: they are the earliest of the call
      const int32_t found = hcnt[(size_t)k * 4 + 3];
      const int n0 = found < 0 ? 0 : found;
      outs[k].n_corners = n0;
      if (found == -1)
        fail(k, vo_set_error(ctx, VO_ECAPACITY, "pipeline_bootstrap: the local maxima on frame %d of sequence %d exceed Shi-Tomasi's candidate capacity",
                             idx_a, (int)seqs[k]));
      else if (found < 0)
        fail(k, vo_set_error(ctx, VO_ECAPACITY, "pipeline_bootstrap: Shi-Tomasi's minimum-distance walk overflowed a grid cell on frame %d of sequence %d",
                             idx_a, (int)seqs[k]));
      else if (n0 < 8)
        fail(k, vo_set_error(ctx, VO_ETRACKING, "pipeline_bootstrap: %d corners on frame %d of sequence %d, the 8-point algorithm needs 8",
                             n0, idx_a, (int)seqs[k]));
      else if (n0 > p->cap)
        fail(k, vo_set_error(ctx, VO_ECAPACITY, "pipeline_bootstrap: %d corners of sequence %d exceed the feature capacity %d", n0,
                             (int)seqs[k], p->cap));
    }
    for (int k = 0; k < L; ++k) {
      if (code[(size_t)k] != VO_OK) continue;
      const vo_f8_result& r = rs[(size_t)k];
      vo_bootstrap_result& o = outs[k];
      o.n_tracked = r.n;
      if (r.n < 8) {
        fail(k, vo_set_error(ctx, VO_ETRACKING, "pipeline_bootstrap: %d of %d corners of sequence %d tracked, the 8-point algorithm needs 8",
                             (int)r.n, (int)o.n_corners, (int)seqs[k]));
        continue;
      }
      o.ransac_iterations = r.iterations;
      o.n_ransac_inliers = r.best_count < 0 ? 0 : r.best_count;
      o.reserved = r.finished_by_host;
      if (r.status != VO_F8_DONE) {
        fail(k, vo_set_error(ctx, VO_ETRACKING,
                             "pipeline_bootstrap: RANSAC found no model with 8 inliers among %d correspondences of sequence %d (best: %d)",
                             (int)r.n, (int)seqs[k], (int)r.best_count));
        continue;
      }
      memcpy(o.M, hF.data() + (size_t)k * 32 + 16, 96);
      o.n_landmarks = hcnt[(size_t)k * 4 + 2];
      o.n_features = r.n;
    }
  }
  // what crossed PCIe, divided among the call's lanes
  {
    const int64_t up = ctx->bytes_h2d - h2d0 + h2d, down = ctx->bytes_d2h - d2h0 + d2h;
    for (int k = 0; k < L; ++k) {
      outs[k].bytes_h2d = (up + L - 1) / L;
      outs[k].bytes_d2h = (down + L - 1) / L;
    }
  }
  // host side of the hand-over (pipeline_state.hip: vo_pipeline_set_state_seq / vo_pipeline_restart_seq), lane by lane
  bool any_ok = false;
  for (int k = 0; k < L; ++k) {
    if (status) status[k] = code[(size_t)k];
    if (code[(size_t)k] != VO_OK) continue;
    any_ok = true;
    const int seq = seqs[k];
    if (restart || rngs) {
      const vo_pcg64 g = rngs ? rngs[k] : p->seed_rng;
      p->rng[seq] = g;
      p->raw_gen[seq] = g;
      p->pos_known[seq] = p->gen_upto[seq];
      p->pos_dev[seq] = p->gen_upto[seq];
    }
    p->idle[seq] = 0;
    p->seq_state[seq] = 1;
  }
  if (any_ok) {
    if (restart) {
      p->prepared_idx = p->prepared_slot = -1;
      for (int k = 0; k < L;) {          // frame b's pyramid + detection, one call per run of consecutive restarted lanes
        if (code[(size_t)k] != VO_OK) {
          ++k;
          continue;
        }
        int run = 1;
        while (k + run < L && code[(size_t)(k + run)] == VO_OK && seqs[k + run] == seqs[k] + run) ++run;
        VO_TRY(prime(p, true, seqs[k], run));
        k += run;
      }
    } else {
      p->slot = 0;
      p->prev_frame = idx_b;
      p->have_state = true;
      p->primed = false;
    }
  }
  if (first_fail >= 0) {
    snprintf(ctx->err, sizeof(ctx->err), "%s", first_msg);
    return code[(size_t)first_fail];
  }
  return VO_OK;
}

int vo_pipeline_bootstrap_seq(vo_pipeline* p, int seq, int idx_a, int idx_b, const vo_bootstrap_params* prm,
                              const vo_pcg64* rng, vo_bootstrap_result* out) {
  if (!p) return VO_EINVAL;
  VO_REQUIRE(p->ctx, out, "pipeline_bootstrap: null result");
  memset(out, 0, sizeof(*out));
  const int32_t s = seq;
  return vo_pipeline_bootstrap_lanes(p, 1, &s, idx_a, idx_b, prm, rng, out, nullptr);
}

int vo_pipeline_bootstrap(vo_pipeline* p, int idx_a, int idx_b, const vo_bootstrap_params* prm, vo_bootstrap_result* out) {
  return vo_pipeline_bootstrap_seq(p, 0, idx_a, idx_b, prm, nullptr, out);
}

}  // extern "C"
