// Calibrated two-view bootstrap (include/vo_hip.h, "calibrated two-view bootstrap"): the five-point essential-matrix solver
// inside the reference's RANSAC loop (src/vo/algorithms/ransac.py:69-129, s = 5), beside _find_essential_matrix
// (src/vo/landmarks/triangulation.py:224-243), as three kernels:
//
//   e5_hyp_kernel    one lane per RANSAC sample of 5 correspondences: x^ = K^-1 x, the solver of essential5_device.h (null
//                    space, ten cubic constraints, Gauss-Jordan on the 10x20 matrix in LDS, the degree-10 polynomial, its
//                    real roots, back-substitution) -> up to ten E per sample, and F = K2^-T E K1^-1 of each for the scorer
//   e5_score_kernel  every solution as a fundamental matrix against every correspondence in pixels: f_score_body
//                    (fscore_device.h), the arithmetic of f_score_kernel; an absent solution scores 0 with an empty mask row
//   e5_best_kernel   per sample: valid = (n_sol > 0), the best count over its solutions, the lowest index that reaches it
//
// fp64 throughout, no FMA contraction, no atomics; every sum has one order, so a sample's outputs depend on the sample alone.
#include "essential5_device.h"
#include "fscore_device.h"
#include "vo_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int E5_HB = 32;            // samples (lanes) per workgroup of e5_hyp_kernel: 32 * 200 doubles of LDS
constexpr int E5_BATCH = 2048;       // samples per batch of the RANSAC loop
constexpr int E5_SOL = 10;

struct e5_cams {
  double K1i[9], K2i[9];             // the closed-form inverses of the two pinhole matrices
};

__global__ __launch_bounds__(E5_HB) void e5_hyp_kernel(const double* __restrict__ x1, const double* __restrict__ x2, int N,
                                                       const int* __restrict__ samples, int Hyp, e5_cams cams,
                                                       double* __restrict__ Eout, double* __restrict__ Fout,
                                                       int* __restrict__ n_sol) {
  __shared__ double s_work[vo_e5::E5_WORK][E5_HB];          // [element][lane]
  const int lane = threadIdx.x;
  const int h = blockIdx.x * E5_HB + lane;
  if (h >= Hyp) return;
  double h1[5][3], h2[5][3];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int i = min(max(samples[5 * h + k], 0), N - 1);
    const double u1 = x1[2 * i], v1 = x1[2 * i + 1], u2 = x2[2 * i], v2 = x2[2 * i + 1];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      h1[k][r] = cams.K1i[3 * r] * u1 + cams.K1i[3 * r + 1] * v1 + cams.K1i[3 * r + 2];
      h2[k][r] = cams.K2i[3 * r] * u2 + cams.K2i[3 * r + 1] * v2 + cams.K2i[3 * r + 2];
    }
  }
  double* E = Eout + (size_t)90 * h;
  const int n = vo_e5::solve<E5_HB>(h1, h2, &s_work[0][lane], E);
  n_sol[h] = n;
  // F = K2i^T (E K1i), every entry summed left to right; an absent solution's rows stay zero
  double* F = Fout + (size_t)90 * h;
  for (int s = 0; s < E5_SOL; ++s) {
    double e[9], A[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = E[9 * s + k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        A[3 * r + c] = e[3 * r] * cams.K1i[c] + e[3 * r + 1] * cams.K1i[3 + c] + e[3 * r + 2] * cams.K1i[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        F[9 * s + 3 * r + c] = s < n ? cams.K2i[r] * A[c] + cams.K2i[3 + r] * A[3 + c] + cams.K2i[6 + r] * A[6 + c] : 0.0;
  }
}

// grid.x = solution slot (sample * 10 + solution)
__global__ __launch_bounds__(256) void e5_score_kernel(const double* __restrict__ p1, const double* __restrict__ p2, int N,
                                                       const double* __restrict__ Fs, const int* __restrict__ n_sol, int kind,
                                                       double thr, int* __restrict__ counts,
                                                       unsigned long long* __restrict__ masks, int words) {
  __shared__ int s_cnt[4];
  const int slot = blockIdx.x;
  if (slot % E5_SOL >= n_sol[slot / E5_SOL]) {              // (the whole workgroup takes this branch or none of it does)
    if (threadIdx.x == 0) counts[slot] = 0;
    if (masks)
      for (int w = threadIdx.x; w < words; w += 256) masks[(size_t)slot * words + w] = 0ull;
    return;
  }
  vo_fscore::f_score_body(p1, p2, N, Fs, kind, thr, counts, masks, words, s_cnt);
}

__global__ __launch_bounds__(256) void e5_best_kernel(const int* __restrict__ n_sol, const int* __restrict__ counts, int Hyp,
                                                      int* __restrict__ best_count, int* __restrict__ best_sol,
                                                      uint8_t* __restrict__ valid) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= Hyp) return;
  const int n = min(max(n_sol[h], 0), E5_SOL);
  int best = 0, arg = -1;
  for (int s = 0; s < n; ++s) {
    const int c = counts[E5_SOL * h + s];
    if (arg < 0 || c > best) {                              // strict `>`: the lowest index of equals
      best = c;
      arg = s;
    }
  }
  best_count[h] = best;
  best_sol[h] = arg;
  valid[h] = n > 0 ? 1 : 0;
}

// the accepted model: its mask row as bytes, its E
__global__ __launch_bounds__(256) void e5_keep_kernel(const unsigned long long* __restrict__ row, int n,
                                                      const double* __restrict__ Eslot, uint8_t* __restrict__ mask,
                                                      double* __restrict__ Ekeep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) mask[i] = (uint8_t)((row[i >> 6] >> (i & 63)) & 1ull);
  if (i < 9) Ekeep[i] = Eslot[i];
}

bool pinhole_inverse(const double* K, double* Ki) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(K[k])) return false;
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  if (fx == 0.0 || fy == 0.0) return false;
  const double ki[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
  for (int k = 0; k < 9; ++k) {
    if (!std::isfinite(ki[k])) return false;
    Ki[k] = ki[k];
  }
  return true;
}

}  // namespace

// ---- device-resident forms (vo_internal.h) ----

int vo_essential_hypotheses_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int N, const double* K1, const double* K2,
                                const int32_t* samples, int Hyp, int error_kind, double threshold, const vo_e5_work& w,
                                int32_t* best_count, int32_t* best_sol, uint8_t* valid) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_x1 && d_x2 && K1 && K2 && samples && w.samples && w.E && w.F && w.n_sol && w.counts && w.best,
             "essential_hypotheses: null pointer");
  VO_REQUIRE(ctx, N >= 5 && Hyp >= 1 && Hyp <= (1 << 20), "essential_hypotheses: need N >= 5, 1 <= Hyp <= 2^20");
  VO_REQUIRE(ctx, error_kind == 0 || error_kind == 1, "essential_hypotheses: error_kind must be 0 or 1");
  e5_cams cams;
  VO_REQUIRE(ctx, pinhole_inverse(K1, cams.K1i) && pinhole_inverse(K2, cams.K2i),
             "essential_hypotheses: K must be finite with non-zero focal lengths");
  for (size_t k = 0; k < (size_t)5 * Hyp; ++k)
    VO_REQUIRE(ctx, samples[k] >= 0 && samples[k] < N, "essential_hypotheses: sample index %d out of range", (int)samples[k]);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int words = vo_cdiv(N, 64);
  hipStream_t st = ctx->stream;
  int32_t* d_best_count = w.best;
  int32_t* d_best_sol = w.best + Hyp;
  uint8_t* d_valid = (uint8_t*)(w.best + 2 * (size_t)Hyp);
  VO_HIP_TRY(ctx, hipMemcpyAsync(w.samples, samples, (size_t)Hyp * 20, hipMemcpyHostToDevice, st));
  {
    vo_prof_scope prof(ctx, VO_K_TWOVIEW_HYP);
    hipLaunchKernelGGL(e5_hyp_kernel, dim3(vo_cdiv(Hyp, E5_HB)), dim3(E5_HB), 0, st, d_x1, d_x2, N, (const int*)w.samples, Hyp,
                       cams, w.E, w.F, (int*)w.n_sol);
  }
  VO_TRY(vo_check_launch(ctx, "e5_hyp_kernel"));
  {
    vo_prof_scope prof(ctx, VO_K_TWOVIEW_SCORE);
    hipLaunchKernelGGL(e5_score_kernel, dim3(Hyp * E5_SOL), dim3(256), 0, st, d_x1, d_x2, N, (const double*)w.F,
                       (const int*)w.n_sol, error_kind, threshold, (int*)w.counts, (unsigned long long*)w.masks, words);
  }
  VO_TRY(vo_check_launch(ctx, "e5_score_kernel"));
  hipLaunchKernelGGL(e5_best_kernel, dim3(vo_cdiv(Hyp, 256)), dim3(256), 0, st, (const int*)w.n_sol, (const int*)w.counts, Hyp,
                     (int*)d_best_count, (int*)d_best_sol, d_valid);
  VO_TRY(vo_check_launch(ctx, "e5_best_kernel"));
  // valid, the best counts and the best solution indices: 9 bytes per sample
  if (best_count) VO_HIP_TRY(ctx, hipMemcpyAsync(best_count, d_best_count, (size_t)Hyp * 4, hipMemcpyDeviceToHost, st));
  if (best_sol) VO_HIP_TRY(ctx, hipMemcpyAsync(best_sol, d_best_sol, (size_t)Hyp * 4, hipMemcpyDeviceToHost, st));
  if (valid) VO_HIP_TRY(ctx, hipMemcpyAsync(valid, d_valid, (size_t)Hyp, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->bytes_h2d += (int64_t)Hyp * 20;
  ctx->bytes_d2h += (int64_t)Hyp * ((best_count ? 4 : 0) + (best_sol ? 4 : 0) + (valid ? 1 : 0));
  return VO_OK;
}

// the workspace of one batch of Hyp samples over N correspondences in the context's scratch blocks 2 .. 8
static int e5_workspace(vo_ctx* ctx, int N, int Hyp, bool want_masks, vo_e5_work* w) {
  vo_buf* s = ctx->scratch;
  const int words = vo_cdiv(N, 64);
  VO_TRY(vo_ensure(ctx, s[2], (size_t)Hyp * 20));
  VO_TRY(vo_ensure(ctx, s[3], (size_t)Hyp * 720));
  VO_TRY(vo_ensure(ctx, s[4], (size_t)Hyp * 720));
  VO_TRY(vo_ensure(ctx, s[5], (size_t)Hyp * 4));
  VO_TRY(vo_ensure(ctx, s[6], (size_t)Hyp * 40));
  if (want_masks) VO_TRY(vo_ensure(ctx, s[7], (size_t)Hyp * E5_SOL * words * 8));
  VO_TRY(vo_ensure(ctx, s[8], (size_t)Hyp * 12));
  w->samples = (int32_t*)s[2].p;
  w->E = (double*)s[3].p;
  w->F = (double*)s[4].p;
  w->n_sol = (int32_t*)s[5].p;
  w->counts = (int32_t*)s[6].p;
  w->masks = want_masks ? (uint64_t*)s[7].p : nullptr;
  w->best = (int32_t*)s[8].p;
  return VO_OK;
}

int vo_essential_ransac_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int N, const double* K1, const double* K2,
                            int error_kind, double threshold, double outlier_ratio, double confidence, int64_t max_iterations,
                            vo_pcg64* rng, double* d_E, uint8_t* d_inl, int64_t* iterations, int32_t* best_count_out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_x1 && d_x2 && K1 && K2 && rng && d_E && d_inl, "essential_ransac: null pointer");
  VO_REQUIRE(ctx, N >= 5, "essential_ransac: the five-point algorithm needs 5 correspondences");
  VO_REQUIRE(ctx, error_kind == 0 || error_kind == 1, "essential_ransac: error_kind must be 0 or 1");
  VO_REQUIRE(ctx, outlier_ratio > 0.0 && outlier_ratio < 1.0 && confidence > 0.0 && confidence < 1.0,
             "essential_ransac: outlier ratio and confidence must be inside (0, 1)");
  VO_REQUIRE(ctx, max_iterations != 0, "essential_ransac: a budget of 0 iterations");
  {
    e5_cams probe;
    VO_REQUIRE(ctx, pinhole_inverse(K1, probe.K1i) && pinhole_inverse(K2, probe.K2i),
               "essential_ransac: K must be finite with non-zero focal lengths");
  }
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  vo_e5_work w;
  VO_TRY(e5_workspace(ctx, N, E5_BATCH, true, &w));
  const int words = vo_cdiv(N, 64);
  vo_ransac_state rs;
  rs.outlier_ratio = outlier_ratio;
  rs.confidence = confidence;
  rs.max_iterations = max_iterations;
  rs.s = 5;
  rs.adaptive = 1;
  int64_t k0 = vo_ransac_num_iterations(confidence, outlier_ratio, 5);
  if (k0 < 0 || k0 > ((int64_t)1 << 62)) k0 = (int64_t)1 << 62;
  rs.n_iterations = (max_iterations >= 0 && max_iterations < k0) ? max_iterations : k0;
  const int64_t draw_limit = rs.n_iterations;          // samples drawn without one real solution before the loop gives up
  std::vector<int32_t> samples((size_t)E5_BATCH * 5), counts((size_t)E5_BATCH), sols((size_t)E5_BATCH);
  std::vector<uint8_t> valid((size_t)E5_BATCH);
  int64_t n_done = 0, total = 0;
  int32_t best_count = -1;
  int finished = 0;
  while (!finished) {
    vo_pcg64 spec = *rng;                  // speculative copy: the generator moves by what the rule consumed
    if (vo_rng_choice(&spec, N, 5, E5_BATCH, samples.data()) != VO_OK)
      return vo_set_error(ctx, VO_EINVAL, "essential_ransac: cannot draw 5 of %d", N);
    VO_TRY(vo_essential_hypotheses_dev(ctx, d_x1, d_x2, N, K1, K2, samples.data(), E5_BATCH, error_kind, threshold, w,
                                       counts.data(), sols.data(), valid.data()));
    int32_t idx = -1;                      // the batch's index of the model the rule accepted last, if it accepted one
    int consumed = 0;
    if (vo_ransac_replay(&rs, valid.data(), counts.data(), E5_BATCH, N, &n_done, &best_count, &idx, 0, &consumed,
                         &finished) != VO_OK)
      return vo_set_error(ctx, VO_EINVAL, "essential_ransac: vo_ransac_replay failed");
    if (idx >= 0) {
      const size_t slot = (size_t)idx * E5_SOL + (size_t)sols[(size_t)idx];
      hipLaunchKernelGGL(e5_keep_kernel, dim3(vo_cdiv(max(N, 9), 256)), dim3(256), 0, st,
                         (const unsigned long long*)w.masks + slot * words, N, (const double*)w.E + slot * 9, d_inl, d_E);
      VO_TRY(vo_check_launch(ctx, "e5_keep_kernel"));
    }
    vo_rng_choice(rng, N, 5, consumed, samples.data());
    total += consumed;
    if (!finished && best_count < 0 && total >= draw_limit) break;
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  if (iterations) *iterations = n_done;
  if (best_count_out) *best_count_out = best_count;
  if (best_count < 0)
    return vo_set_error(ctx, VO_ETRACKING, "essential_ransac: no sample with a real solution among %lld drawn from %d correspondences",
                        (long long)total, N);
  return VO_OK;
}

extern "C" {

int vo_essential_hypotheses(vo_ctx* ctx, const double* x1, const double* x2, int N, const double* K1, const double* K2,
                            const int32_t* samples, int Hyp, int error_kind, double threshold, double* E, int32_t* n_sol,
                            int32_t* counts, int32_t* best_sol, uint64_t* masks) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, x1 && x2 && K1 && K2 && samples && E && n_sol && counts && best_sol, "essential_hypotheses: null pointer");
  VO_REQUIRE(ctx, N >= 5 && Hyp >= 1 && Hyp <= (1 << 20), "essential_hypotheses: need N >= 5, 1 <= Hyp <= 2^20");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int words = vo_cdiv(N, 64);
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)N * 16));
  vo_e5_work w;
  VO_TRY(e5_workspace(ctx, N, Hyp, masks != nullptr, &w));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, x1, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, x2, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_TRY(vo_essential_hypotheses_dev(ctx, (const double*)s[0].p, (const double*)s[1].p, N, K1, K2, samples, Hyp, error_kind,
                                     threshold, w, nullptr, best_sol, nullptr));
  VO_HIP_TRY(ctx, hipMemcpyAsync(E, w.E, (size_t)Hyp * 720, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(n_sol, w.n_sol, (size_t)Hyp * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(counts, w.counts, (size_t)Hyp * 40, hipMemcpyDeviceToHost, st));
  if (masks) VO_HIP_TRY(ctx, hipMemcpyAsync(masks, w.masks, (size_t)Hyp * E5_SOL * words * 8, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_essential_ransac(vo_ctx* ctx, const double* x1, const double* x2, int N, const double* K1, const double* K2,
                        int error_kind, double threshold, double outlier_ratio, double confidence, int64_t max_iterations,
                        vo_pcg64* rng, double* E, uint8_t* inlier_mask, int64_t* iterations, int32_t* best_count) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, x1 && x2 && K1 && K2 && rng && E && inlier_mask, "essential_ransac: null pointer");
  VO_REQUIRE(ctx, N >= 5, "essential_ransac: the five-point algorithm needs 5 correspondences");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[9], 128));
  VO_TRY(vo_ensure(ctx, s[10], (size_t)N));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, x1, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, x2, (size_t)N * 16, hipMemcpyHostToDevice, st));
  int64_t it = 0;
  int32_t best = -1;
  vo_pcg64 gen = *rng;
  const int rc = vo_essential_ransac_dev(ctx, (const double*)s[0].p, (const double*)s[1].p, N, K1, K2, error_kind, threshold,
                                         outlier_ratio, confidence, max_iterations, &gen, (double*)s[9].p, (uint8_t*)s[10].p,
                                         &it, &best);
  if (rc == VO_EINVAL) return rc;                        // refused: nothing written
  *rng = gen;
  if (iterations) *iterations = it;
  if (best_count) *best_count = best;
  if (rc != VO_OK) return rc;
  VO_HIP_TRY(ctx, hipMemcpyAsync(E, s[9].p, 72, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(inlier_mask, s[10].p, (size_t)N, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

}  // extern "C"
