// Structure-only refinement of a window on the device (vo_hip.h, "Window structure refinement").
//
// The window bundle adjustment (window_ba.hip) with every pose held: each landmark is a Levenberg-Marquardt problem of its
// own in three unknowns over the observations of its track.  Nothing couples two landmarks, so nothing is shared but the
// window's poses.
//
// window_structure_kernel: 16 lanes per landmark (a track has at most W <= 16 observations), four landmarks per wave,
// sixteen per workgroup of 256 threads, grid (ceil(L_cap / 16), S).  Lane r of a row owns observation lm_start[i] + r: its
// slot's pose, its pixel and everything derived from them stay in registers for the whole solve; lanes beyond the track add
// +0.0.  The window's poses and intrinsics go through LDS once per workgroup (the only barrier).  The sums of a landmark
// (V's six, g's three, the costs) go over its row by a xor butterfly of width 16: fp64 addition is commutative, so every lane
// of a row ends with the same bits, takes every decision alike and carries the control state (cost, lambda, counters) in
// registers.  A row leaves the loop when its landmark is done; the wave runs until its four rows are.  No atomics, no grid
// barrier, no spin; X is written once, at the end, and only for a landmark that is kept.
//
// window_structure_summary_kernel: one workgroup per window adds up the rows in a fixed order.
#include <cmath>

#include "vo_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int WS_T = 256;                         // threads per workgroup
constexpr int WS_ROW = 16;                        // lanes per landmark
constexpr int WS_LM = WS_T / WS_ROW;              // landmarks per workgroup
constexpr double WS_LAMBDA_MAX = 1e12, WS_LAMBDA_MIN = 1e-12;

struct ws_args {
  int W, L_cap, M_cap;
  const int32_t* counts;      // S x 4: L, M, -, -
  const double* K;            // S x 9
  const double* poses;        // S x W x 12
  double* X;                  // S x L_cap x 3
  const int32_t* lm_start;    // S x (L_cap + 1)
  const int32_t* obs_slot;    // S x M_cap
  const double* obs_xy;       // S x M_cap x 2
  vo_structure_result* res;   // S x L_cap
  vo_structure_summary* sum;  // S
  int max_iter, max_trials;
  double huber, lambda0, step_tol, f_tol, gate_px, cos_limit;      // cos_limit: cos(min_parallax), 2 without the gate
};

// the sum of v over the 16 lanes of a row, the same bits in every lane
__device__ __forceinline__ double row_sum(double v) {
#pragma unroll
  for (int off = WS_ROW / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, WS_ROW);
  return v;
}

__device__ __forceinline__ double row_min(double v) {
#pragma unroll
  for (int off = WS_ROW / 2; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, WS_ROW));
  return v;
}

// this lane's row of a wave-wide ballot
__device__ __forceinline__ unsigned row_bits(bool pred) {
  const unsigned long long b = __ballot(pred);
  return (unsigned)(b >> (threadIdx.x & 48)) & 0xffffu;
}

struct ws_obs {       // one observation: its slot's pose (R row-major, t), its pixel
  double P[12];
  double u, v;
};

struct ws_point {     // an observation at a landmark position
  double px, py, pz, iz, eu, ev, r2, rho;
};

__device__ __forceinline__ ws_point ws_eval(const ws_obs& o, double fx, double fy, double cx, double cy, double huber, double X0,
                                            double X1, double X2) {
  ws_point q;
  q.px = o.P[0] * X0 + o.P[1] * X1 + o.P[2] * X2 + o.P[9];
  q.py = o.P[3] * X0 + o.P[4] * X1 + o.P[5] * X2 + o.P[10];
  q.pz = o.P[6] * X0 + o.P[7] * X1 + o.P[8] * X2 + o.P[11];
  q.iz = 1.0 / q.pz;
  q.eu = o.u - (fx * q.px * q.iz + cx);
  q.ev = o.v - (fy * q.py * q.iz + cy);
  q.r2 = q.eu * q.eu + q.ev * q.ev;
  q.rho = q.r2;
  if (huber > 0.0) {
    const double r = sqrt(q.r2);
    if (r > huber) q.rho = 2.0 * huber * r - huber * huber;
  }
  return q;
}

__global__ __launch_bounds__(WS_T) void window_structure_kernel(ws_args a) {
  __shared__ double s_pose[VO_WINDOW_WMAX * 12 + 4];
  const int tid = threadIdx.x, r = tid & (WS_ROW - 1);
  const size_t q = blockIdx.y;
  const int W = a.W;
  const int L = a.counts[4 * q], M = a.counts[4 * q + 1];
  const int rows = min(max(L, 0), a.L_cap);
  if ((int)blockIdx.x * WS_LM >= rows) return;                       // (the same in every thread)
  const int i = blockIdx.x * WS_LM + (tid >> 4);
  const int32_t* const lm_start = a.lm_start + q * ((size_t)a.L_cap + 1);
  const int32_t* const obs_slot = a.obs_slot + q * (size_t)a.M_cap;
  const double* const obs_xy = a.obs_xy + q * (size_t)a.M_cap * 2;
  double* const Xq = a.X + q * (size_t)a.L_cap * 3;
  vo_structure_result* const res = a.res + q * (size_t)a.L_cap;

  // ---- the window: poses and intrinsics into LDS, checked on the way ----
  bool wbad = L > a.L_cap || M < 0 || M > a.M_cap;
  if (!wbad) wbad = lm_start[L] != M;
  if (tid < 12 * W) {
    const double v = a.poses[q * (size_t)W * 12 + tid];
    s_pose[tid] = v;
    wbad = wbad || !isfinite(v);
  } else if (tid >= VO_WINDOW_WMAX * 12 && tid < VO_WINDOW_WMAX * 12 + 4) {
    const int k = tid - VO_WINDOW_WMAX * 12;
    const double v = a.K[q * 9 + (k == 0 ? 0 : k == 1 ? 4 : k == 2 ? 2 : 5)];        // fx, fy, cx, cy
    s_pose[tid] = v;
    wbad = wbad || !isfinite(v);
  }
  wbad = __syncthreads_or(wbad) != 0;
  const double fx = s_pose[VO_WINDOW_WMAX * 12], fy = s_pose[VO_WINDOW_WMAX * 12 + 1], cx = s_pose[VO_WINDOW_WMAX * 12 + 2],
               cy = s_pose[VO_WINDOW_WMAX * 12 + 3];

  // ---- the landmark of this row ----
  const bool live = i < rows;                                        // (from here on everything is the same along a row)
  int s = 0, n = 0, n_rep = 0;
  bool refused = wbad || !live;
  if (!refused) {
    s = lm_start[i];
    const int e = lm_start[i + 1];
    n = e - s;
    const bool sound = s >= 0 && e <= M && n >= 0 && n <= W;
    n_rep = sound ? n : 0;
    refused = !sound || n < 2;
  }
  const bool mine = !refused && r < n;
  ws_obs o;
  int slot = 0;
  o.u = cx;
  o.v = cy;
  if (mine) {
    slot = obs_slot[s + r];
    o.u = obs_xy[2 * (size_t)(s + r)];
    o.v = obs_xy[2 * (size_t)(s + r) + 1];
  }
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  if (live) {
    X0 = Xq[3 * (size_t)i];
    X1 = Xq[3 * (size_t)i + 1];
    X2 = Xq[3 * (size_t)i + 2];
  }
  {
    const int prev = __shfl_up(slot, 1, WS_ROW);
    bool bad = mine && (slot < 0 || slot >= W || (r > 0 && slot <= prev) || !(isfinite(o.u) && isfinite(o.v)));
    bad = bad || !(isfinite(X0) && isfinite(X1) && isfinite(X2));
    refused = refused || row_bits(bad) != 0;
  }
  const bool on = mine && !refused;                                  // this lane carries an observation of a sound track
#pragma unroll
  for (int k = 0; k < 12; ++k) o.P[k] = (k == 0 || k == 4 || k == 8 || k == 11) ? 1.0 : 0.0;      // (an idle lane: a harmless camera)
  if (on) {
#pragma unroll
    for (int k = 0; k < 12; ++k) o.P[k] = s_pose[12 * slot + k];
  } else {
    o.u = cx;
    o.v = cy;
  }
  const double huber = a.huber;
  double cost = 0.0, sq = 0.0;
  if (!refused) {
    const ws_point p0 = ws_eval(o, fx, fy, cx, cy, huber, X0, X1, X2);
    cost = row_sum(on ? p0.rho : 0.0);
    sq = row_sum(on ? p0.r2 : 0.0);
    refused = row_bits(on && !(p0.pz > 0.0)) != 0 || !isfinite(cost);
  }
  if (refused) {
    if (live && r == 0) {
      vo_structure_result out;
      out.status = 4;
      out.iterations = 0;
      out.trials = 0;
      out.n_obs = n_rep;
      out.cost0 = 0.0;
      out.cost = 0.0;
      out.min_cos = 0.0;
      out.kept = 0;
      out.reserved = 0;
      res[i] = out;
    }
    return;
  }

  // ---- the smallest cosine between two of its rays ----
  double min_cos;
  {
    const double dx = (o.u - cx) / fx, dy = (o.v - cy) / fy;
    double wx = o.P[0] * dx + o.P[3] * dy + o.P[6];
    double wy = o.P[1] * dx + o.P[4] * dy + o.P[7];
    double wz = o.P[2] * dx + o.P[5] * dy + o.P[8];
    const double nrm = sqrt(wx * wx + wy * wy + wz * wz);
    wx = wx / nrm;
    wy = wy / nrm;
    wz = wz / nrm;
    double mc = INFINITY;
#pragma unroll
    for (int k = 1; k < WS_ROW; ++k) {
      const double ox = __shfl_xor(wx, k, WS_ROW), oy = __shfl_xor(wy, k, WS_ROW), oz = __shfl_xor(wz, k, WS_ROW);
      const double c = wx * ox + wy * oy + wz * oz;
      if (on && (r ^ k) < n) mc = fmin(mc, c);
    }
    min_cos = row_min(mc);
  }

  // ---- Levenberg-Marquardt on the three unknowns ----
  const double cost0 = cost;
  double lam = a.lambda0;
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  int it = 0, trials = 0, status;
  bool need_lin = true;
  for (;;) {
    if (it >= a.max_iter) {
      status = 1;
      break;
    }
    if (trials >= a.max_trials) {
      status = 2;
      break;
    }
    if (lam > WS_LAMBDA_MAX) {
      status = 3;
      break;
    }
    if (need_lin) {
      need_lin = false;
      const ws_point p = ws_eval(o, fx, fy, cx, cy, huber, X0, X1, X2);
      double w = 1.0;
      if (huber > 0.0) {
        const double rr = sqrt(p.eu * p.eu + p.ev * p.ev);
        if (rr > huber) w = huber / rr;
      }
      const double ca = fx * p.iz, cc = -fx * p.px * p.iz * p.iz;
      const double cb = fy * p.iz, cd = -fy * p.py * p.iz * p.iz;
      double Jl0[3], Jl1[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        Jl0[m] = ca * o.P[m] + cc * o.P[6 + m];
        Jl1[m] = cb * o.P[3 + m] + cd * o.P[6 + m];
      }
      int k = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int m = c; m < 3; ++m) {
          const double t = (w * Jl0[c]) * Jl0[m] + (w * Jl1[c]) * Jl1[m];
          V[k++] = row_sum(on ? t : 0.0);
        }
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double t = (w * Jl0[m]) * p.eu + (w * Jl1[m]) * p.ev;
        g[m] = row_sum(on ? t : 0.0);
      }
    }
    // the damped system by Cholesky: V = [0 1 2; . 3 4; . . 5]
    const double damp = 1.0 + lam;
    const double v00 = V[0] * damp, v01 = V[1], v02 = V[2], v11 = V[3] * damp, v12 = V[4], v22 = V[5] * damp;
    const double l00 = sqrt(v00);
    const double l10 = v01 / l00, l20 = v02 / l00;
    const double d1 = v11 - l10 * l10;
    const double l11 = sqrt(d1);
    const double l21 = (v12 - l20 * l10) / l11;
    const double d2 = v22 - l20 * l20 - l21 * l21;
    const double l22 = sqrt(d2);
    if (!(v00 > 0.0 && d1 > 0.0 && d2 > 0.0)) {
      ++trials;
      lam *= 10.0;
      continue;
    }
    const double y0 = g[0] / l00;
    const double y1 = (g[1] - l10 * y0) / l11;
    const double y2 = (g[2] - l20 * y0 - l21 * y1) / l22;
    const double dX2 = y2 / l22;
    const double dX1 = (y1 - l21 * dX2) / l11;
    const double dX0 = (y0 - l10 * dX1 - l20 * dX2) / l00;
    const double dn = sqrt(dX0 * dX0 + dX1 * dX1 + dX2 * dX2), xn = sqrt(X0 * X0 + X1 * X1 + X2 * X2);
    const double pred = g[0] * dX0 + g[1] * dX1 + g[2] * dX2;
    if (dn <= a.step_tol * (1.0 + xn) || pred <= a.f_tol * cost) {
      status = 0;                                 // a step this small, or one that promises this little, is not taken (nor counted)
      break;
    }
    ++trials;
    const double T0 = X0 + dX0, T1 = X1 + dX1, T2 = X2 + dX2;
    const ws_point pt = ws_eval(o, fx, fy, cx, cy, huber, T0, T1, T2);
    const double cost_new = row_sum(on ? pt.rho : 0.0);
    const double sq_new = row_sum(on ? pt.r2 : 0.0);
    const bool behind = row_bits(on && !(pt.pz > 0.0)) != 0;
    if (!behind && cost_new <= cost) {
      X0 = T0;
      X1 = T1;
      X2 = T2;
      cost = cost_new;
      sq = sq_new;
      ++it;
      lam = fmax(lam / 10.0, WS_LAMBDA_MIN);
      need_lin = true;
    } else {
      lam *= 10.0;
    }
  }

  // ---- the gate; X is written only when the landmark is kept ----
  bool kept = status == 0 || status == 1;
  if (a.gate_px > 0.0) kept = kept && sqrt(sq / (double)n) <= a.gate_px;
  kept = kept && min_cos <= a.cos_limit;
  if (r == 0) {
    if (kept && it > 0) {
      Xq[3 * (size_t)i] = X0;
      Xq[3 * (size_t)i + 1] = X1;
      Xq[3 * (size_t)i + 2] = X2;
    }
    vo_structure_result out;
    out.status = status;
    out.iterations = it;
    out.trials = trials;
    out.n_obs = n;
    out.cost0 = cost0;
    out.cost = cost;
    out.min_cos = min_cos;
    out.kept = kept ? 1 : 0;
    out.reserved = 0;
    res[i] = out;
  }
}

// One workgroup per window: thread t adds rows t, t + 256, ... in ascending order, a butterfly adds the 64 partials of a wave,
// thread 0 the four wave totals in wave order.
__global__ __launch_bounds__(WS_T) void window_structure_summary_kernel(ws_args a) {
  __shared__ double s_d[WS_T / 64][2];
  __shared__ int s_i[WS_T / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t q = blockIdx.x;
  const int L = a.counts[4 * q];
  const int rows = min(max(L, 0), a.L_cap);
  const vo_structure_result* res = a.res + q * (size_t)a.L_cap;
  double c0 = 0.0, c1 = 0.0;
  int n_ref = 0, n_kept = 0, max_it = 0;
  for (int i = tid; i < rows; i += WS_T) {
    const vo_structure_result x = res[i];
    if (x.status == 4) {
      ++n_ref;
    } else {
      c0 += x.cost0;
      c1 += x.cost;
    }
    n_kept += x.kept;
    max_it = max(max_it, x.iterations);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    c0 = c0 + __shfl_xor(c0, off);
    c1 = c1 + __shfl_xor(c1, off);
    n_ref += __shfl_xor(n_ref, off);
    n_kept += __shfl_xor(n_kept, off);
    max_it = max(max_it, __shfl_xor(max_it, off));
  }
  if (lane == 0) {
    s_d[wv][0] = c0;
    s_d[wv][1] = c1;
    s_i[wv][0] = n_ref;
    s_i[wv][1] = n_kept;
    s_i[wv][2] = max_it;
  }
  __syncthreads();
  if (tid == 0) {
    vo_structure_summary out;
    out.L = L;
    out.n_refused = 0;
    out.n_kept = 0;
    out.max_iterations = 0;
    out.cost0 = 0.0;
    out.cost = 0.0;
    for (int w = 0; w < WS_T / 64; ++w) {
      out.cost0 += s_d[w][0];
      out.cost += s_d[w][1];
      out.n_refused += s_i[w][0];
      out.n_kept += s_i[w][1];
      out.max_iterations = max(out.max_iterations, s_i[w][2]);
    }
    a.sum[q] = out;
  }
}

int resolve_params(vo_ctx* ctx, const vo_structure_params* prm, ws_args* a) {
  vo_structure_params p;
  memset(&p, 0, sizeof(p));
  if (prm) p = *prm;
  vo_lm_params lm;
  VO_TRY(vo_resolve_lm_params(ctx, "window_structure", p.max_iter, p.max_trials, p.huber_px, p.lambda0, p.step_tol, &lm));
  a->max_iter = lm.max_iter;
  a->max_trials = lm.max_trials;
  a->huber = lm.huber;
  a->lambda0 = lm.lambda0;
  a->step_tol = lm.step_tol;
  VO_REQUIRE(ctx, p.f_tol >= 0.0 && std::isfinite(p.f_tol), "window_structure: f_tol must be 0 (default 1e-9) or positive");
  a->f_tol = p.f_tol > 0.0 ? p.f_tol : 1e-9;
  VO_REQUIRE(ctx, p.gate_px >= 0.0 && std::isfinite(p.gate_px), "window_structure: gate_px must be 0 (no gate) or a positive number of pixels");
  a->gate_px = p.gate_px;
  VO_REQUIRE(ctx, p.min_parallax >= 0.0 && p.min_parallax < 3.141592653589793,
             "window_structure: min_parallax must be 0 (no gate) or an angle below pi, in radians");
  a->cos_limit = p.min_parallax > 0.0 ? std::cos(p.min_parallax) : 2.0;
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_window_structure_dev(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* d_counts, const double* d_K,
                            const double* d_poses, double* d_X, const int32_t* d_lm_start, const int32_t* d_obs_slot,
                            const double* d_obs_xy, const vo_structure_params* prm, vo_structure_result* d_results,
                            vo_structure_summary* d_summary) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_counts && d_K && d_poses && d_X && d_lm_start && d_obs_slot && d_obs_xy && d_results && d_summary,
             "window_structure: null pointer");
  VO_TRY(vo_check_window_shape(ctx, "window_structure", S, W, L_cap, M_cap));
  ws_args a;
  VO_TRY(resolve_params(ctx, prm, &a));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  a.W = W;
  a.L_cap = L_cap;
  a.M_cap = M_cap;
  a.counts = d_counts;
  a.K = d_K;
  a.poses = d_poses;
  a.X = d_X;
  a.lm_start = d_lm_start;
  a.obs_slot = d_obs_slot;
  a.obs_xy = d_obs_xy;
  a.res = d_results;
  a.sum = d_summary;
  {
    vo_prof_scope ps(ctx, VO_K_WINDOW_STRUCTURE);
    hipLaunchKernelGGL(window_structure_kernel, dim3(vo_cdiv(L_cap, WS_LM), S), dim3(WS_T), 0, ctx->stream, a);
  }
  VO_TRY(vo_check_launch(ctx, "window_structure_kernel"));
  {
    vo_prof_scope ps(ctx, VO_K_WINDOW_STRUCTURE);
    hipLaunchKernelGGL(window_structure_summary_kernel, dim3(S), dim3(WS_T), 0, ctx->stream, a);
  }
  return vo_check_launch(ctx, "window_structure_summary_kernel");
}

int vo_window_structure(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* counts, const double* K,
                        const double* poses, double* X, const int32_t* lm_start, const int32_t* obs_slot, const double* obs_xy,
                        const vo_structure_params* prm, vo_structure_result* results, vo_structure_summary* summary) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, counts && K && poses && X && lm_start && obs_slot && obs_xy && results && summary, "window_structure: null pointer");
  VO_TRY(vo_check_window_shape(ctx, "window_structure", S, W, L_cap, M_cap));
  const size_t s = (size_t)S;
  const size_t bytes[9] = {s * 16,        s * 72,         s * W * 96,
                           s * L_cap * 24, s * ((size_t)L_cap + 1) * 4,
                           s * M_cap * 4, s * M_cap * 16, s * L_cap * sizeof(vo_structure_result),
                           s * sizeof(vo_structure_summary)};
  const void* src[7] = {counts, K, poses, X, lm_start, obs_slot, obs_xy};
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  for (int k = 0; k < 9; ++k) VO_TRY(vo_ensure(ctx, ctx->scratch[k], bytes[k]));
  for (int k = 0; k < 7; ++k) VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch[k].p, src[k], bytes[k], hipMemcpyHostToDevice, st));
  vo_buf* b = ctx->scratch;
  VO_HIP_TRY(ctx, hipMemsetAsync(b[7].p, 0, bytes[7], st));
  VO_TRY(vo_window_structure_dev(ctx, S, W, L_cap, M_cap, (const int32_t*)b[0].p, (const double*)b[1].p, (const double*)b[2].p,
                                 (double*)b[3].p, (const int32_t*)b[4].p, (const int32_t*)b[5].p, (const double*)b[6].p, prm,
                                 (vo_structure_result*)b[7].p, (vo_structure_summary*)b[8].p));
  VO_HIP_TRY(ctx, hipMemcpyAsync(X, b[3].p, bytes[3], hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(results, b[7].p, bytes[7], hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(summary, b[8].p, bytes[8], hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

}  // extern "C"
