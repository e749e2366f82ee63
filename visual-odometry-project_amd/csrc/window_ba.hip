// Sliding-window bundle adjustment on the device (vo_hip.h, "Window bundle adjustment").
//
// Nothing in the reference corresponds to it: the reference keeps the pose of every frame as the P3P refinement left it and a
// landmark as its two-view triangulation made it.  This is the local back end a front end of this kind is usually given:
// Levenberg-Marquardt over the last W poses and the landmarks they share, on the Schur complement of the landmarks.
//
// window_ba_kernel: one workgroup of 512 threads per window, alive for the whole solve -- no host read between trials, no
// hand-over between workgroups, so nothing to wait for but __syncthreads().  Every thread carries the same control state
// (cost, lambda, counters) in registers: each decision is taken from values all threads read alike (a workgroup sum, a flag
// in LDS behind a barrier).  The work of a trial, each part with the owner of every sum fixed:
//   linearise   one thread per landmark walks its observations in CSR order: residual, weight, the two Jacobians and
//               W = w Jp^T Jl per observation (workspace), V_i and g_l,i per landmark; then one thread per (free pose, entry)
//               adds the 21 + 6 entries of U_j and g_p,j over the landmarks in ascending order
//   damp        one thread per landmark: V* = V with diag (1 + lambda), its 3x3 Cholesky inverse, Y = W V*^-1 per observation
//   reduce      one thread per entry of the lower triangle of S adds  Y_ij W_ik^T  over the landmarks in ascending order
//               (a table landmark x slot -> observation finds the pair); S lives packed in LDS (90 x 91 / 2 doubles at W = 16,
//               n_fixed = 1: 32 KB), b beside it
//   solve       Cholesky by columns in LDS (thread r owns row r; a pivot that is not positive rejects the trial), forward and
//               back substitution by columns
//   step        landmarks by back-substitution, poses by [Exp(w) | v] T; |delta| and |x| are workgroup sums
//   evaluate    one thread per landmark: cost and the number of points not in front at the trial point (workgroup sums)
// A workgroup sum: per-thread partial in ascending landmark order, a butterfly over the wave's 64 lanes, the eight wave totals
// added in wave order by every thread.  No atomics on floating-point values anywhere: two runs give the same bits.
//
// window_match_kernel / window_build_kernel: the window of W observation records (vo_pipeline_export_tracks_post_seq); the
// join compares ids only and copies the rest.
#include <cmath>

#include "pose_step_device.h"
#include "window_join_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int BA_T = 512;
constexpr int BA_NMAX = 6 * (VO_WINDOW_WMAX - 1);        // unknowns of the reduced system
constexpr int BA_OBS_D = 57;                      // doubles of workspace per observation: Jp 12, Jl 6, w, e 2, W 18, Y 18
constexpr int BA_LM_D = 18;                       // per landmark: V 6, g 3, V*^-1 6, trial X 3
constexpr double BA_LAMBDA_MAX = 1e12, BA_LAMBDA_MIN = 1e-12;

struct ba_args {
  int W, L_cap, M_cap;
  const int32_t* counts;      // S x 4: L, M, (flags, reserved: what vo_window_from_tracks_dev leaves there)
  const double* K;            // S x 9
  double* poses;              // S x W x 12
  double* X;                  // S x L_cap x 3
  const int32_t* lm_start;    // S x (L_cap + 1)
  const int32_t* obs_slot;    // S x M_cap
  const double* obs_xy;       // S x M_cap x 2
  double* work;               // S x window_doubles(L_cap, M_cap)
  vo_ba_result* res;          // S
  int max_iter, max_trials, n_fixed;
  double huber, lambda0, step_tol;
};

__host__ __device__ inline size_t window_doubles(int L_cap, int M_cap) {
  return (size_t)BA_OBS_D * (size_t)M_cap + (size_t)(BA_LM_D + VO_WINDOW_WMAX / 2) * (size_t)L_cap;
}

__device__ __forceinline__ int low(int r, int c) { return (r * (r + 1)) / 2 + c; }                    // c <= r

// sums of v[0 .. NV-1] over the workgroup, in every thread (see the head of the file for the order)
template <int NV>
__device__ __forceinline__ void block_sums(double* v, double (*s_red)[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] = v[k] + __shfl_xor(v[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) s_red[wv][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < BA_T / 64; ++w) t += s_red[w][k];
    v[k] = t;
  }
  __syncthreads();
}

struct ba_cam {
  double fx, fy, cx, cy;
};

// cost and the number of observations with p_z <= 0 (or not a number) at (pose, X): this thread's landmarks
__device__ __forceinline__ void eval_partial(const double* pose, const double* __restrict__ X, int L,
                                             const int32_t* __restrict__ lm_start, const int32_t* __restrict__ obs_slot,
                                             const double* __restrict__ obs_xy, const ba_cam& cam, double huber, double* out2) {
  double cost = 0.0, back = 0.0;
  for (int i = threadIdx.x; i < L; i += BA_T) {
    const double X0 = X[3 * i], X1 = X[3 * i + 1], X2 = X[3 * i + 2];
    const int e = lm_start[i + 1];
    for (int o = lm_start[i]; o < e; ++o) {
      const double* P = pose + 12 * obs_slot[o];
      const double px = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[9];
      const double py = P[3] * X0 + P[4] * X1 + P[5] * X2 + P[10];
      const double pz = P[6] * X0 + P[7] * X1 + P[8] * X2 + P[11];
      if (!(pz > 0.0)) back += 1.0;
      const double iz = 1.0 / pz;
      const double eu = obs_xy[2 * o] - (cam.fx * px * iz + cam.cx);
      const double ev = obs_xy[2 * o + 1] - (cam.fy * py * iz + cam.cy);
      const double r2 = eu * eu + ev * ev;
      double rho = r2;
      if (huber > 0.0) {
        const double r = sqrt(r2);
        if (r > huber) rho = 2.0 * huber * r - huber * huber;
      }
      cost += rho;
    }
  }
  out2[0] = cost;
  out2[1] = back;
}

__global__ __launch_bounds__(BA_T) void window_ba_kernel(ba_args a) {
  __shared__ double s_S[(BA_NMAX * (BA_NMAX + 1)) / 2];
  __shared__ double s_diag[BA_NMAX], s_b[BA_NMAX], s_y[BA_NMAX];
  __shared__ double s_U[(VO_WINDOW_WMAX - 1) * 27];
  __shared__ double s_pose[VO_WINDOW_WMAX * 12], s_try[VO_WINDOW_WMAX * 12];
  __shared__ double s_red[BA_T / 64][4];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const int W = a.W;
  const int L = a.counts[4 * q], M = a.counts[4 * q + 1];
  double* const poses = a.poses + q * (size_t)W * 12;
  double* const X = a.X + q * (size_t)a.L_cap * 3;
  const int32_t* const lm_start = a.lm_start + q * ((size_t)a.L_cap + 1);
  const int32_t* const obs_slot = a.obs_slot + q * (size_t)a.M_cap;
  const double* const obs_xy = a.obs_xy + q * (size_t)a.M_cap * 2;
  double* const work = a.work + q * window_doubles(a.L_cap, a.M_cap);
  double* const wobs = work;                                              // M_cap x BA_OBS_D
  double* const wlm = work + (size_t)BA_OBS_D * a.M_cap;                  // L_cap x BA_LM_D
  int* const tab = (int*)(wlm + (size_t)BA_LM_D * a.L_cap);               // L_cap x VO_WINDOW_WMAX: landmark, slot -> observation
  vo_ba_result* const res = a.res + q;
  const int nfix = a.n_fixed, nf = W - nfix, n = 6 * nf;
  const double huber = a.huber;

  auto refuse = [&]() {
    if (tid == 0) {
      res->status = 4;
      res->iterations = 0;
      res->trials = 0;
      res->n_obs = M > 0 && M <= a.M_cap ? M : 0;
      res->cost0 = 0.0;
      res->cost = 0.0;
      res->lambda = a.lambda0;
    }
  };
  // ---- refusals: nothing of the window is written ----
  if (L <= 0 || L > a.L_cap || M <= 0 || M > a.M_cap || nf < 1) {        // (the same in every thread)
    refuse();
    return;
  }
  if (tid == 0) s_flag = 0;
  __syncthreads();
  ba_cam cam;
  {
    const double* K = a.K + q * 9;
    cam.fx = K[0];
    cam.fy = K[4];
    cam.cx = K[2];
    cam.cy = K[5];
    bool bad = !(isfinite(cam.fx) && isfinite(cam.fy) && isfinite(cam.cx) && isfinite(cam.cy));
    if (tid < 12 * W) {
      const double v = poses[tid];
      s_pose[tid] = v;
      s_try[tid] = v;
      bad = bad || !isfinite(v);
    }
    for (int i = tid; i < L; i += BA_T) {
      const int s = lm_start[i], e = lm_start[i + 1];
      bad = bad || (i == 0 && s != 0) || (i == L - 1 && e != M) || !(s >= 0 && e > s && e <= M);
      bad = bad || !(isfinite(X[3 * i]) && isfinite(X[3 * i + 1]) && isfinite(X[3 * i + 2]));
    }
    for (int o = tid; o < M; o += BA_T) {
      const int s = obs_slot[o];
      bad = bad || s < 0 || s >= W || !(isfinite(obs_xy[2 * o]) && isfinite(obs_xy[2 * o + 1]));
    }
    if (bad) s_flag = 1;
  }
  __syncthreads();
  if (s_flag) {
    refuse();
    return;
  }
  __syncthreads();
  {
    // the table landmark x slot -> observation (the CSR is sound here: every range lies in 0 .. M); slots ascend strictly
    bool bad = false;
    for (int i = tid; i < L; i += BA_T) {
      int* row = tab + (size_t)VO_WINDOW_WMAX * i;
#pragma unroll
      for (int s = 0; s < VO_WINDOW_WMAX; ++s) row[s] = -1;
      int prev = -1;
      const int e = lm_start[i + 1];
      for (int o = lm_start[i]; o < e; ++o) {
        const int s = obs_slot[o];
        bad = bad || s <= prev;
        prev = s;
        row[s] = o;
      }
    }
    if (bad) s_flag = 1;
  }
  __syncthreads();
  if (s_flag) {
    refuse();
    return;
  }
  double cost, lam = a.lambda0;
  {
    double v[2];
    eval_partial(s_pose, X, L, lm_start, obs_slot, obs_xy, cam, huber, v);
    block_sums<2>(v, s_red);
    if (v[1] != 0.0 || !isfinite(v[0])) {
      refuse();
      return;
    }
    cost = v[0];
  }
  const double cost0 = cost;
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
    if (lam > BA_LAMBDA_MAX) {
      status = 3;
      break;
    }
    if (need_lin) {
      need_lin = false;
      // ---- linearise at (s_pose, X) ----
      for (int i = tid; i < L; i += BA_T) {
        const double X0 = X[3 * i], X1 = X[3 * i + 1], X2 = X[3 * i + 2];
        double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        const int e = lm_start[i + 1];
        for (int o = lm_start[i]; o < e; ++o) {
          const double* P = s_pose + 12 * obs_slot[o];
          const double px = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[9];
          const double py = P[3] * X0 + P[4] * X1 + P[5] * X2 + P[10];
          const double pz = P[6] * X0 + P[7] * X1 + P[8] * X2 + P[11];
          const double iz = 1.0 / pz;
          const double eu = obs_xy[2 * o] - (cam.fx * px * iz + cam.cx);
          const double ev = obs_xy[2 * o + 1] - (cam.fy * py * iz + cam.cy);
          double w = 1.0;
          if (huber > 0.0) {
            const double r = sqrt(eu * eu + ev * ev);
            if (r > huber) w = huber / r;
          }
          const double ca = cam.fx * iz, cc = -cam.fx * px * iz * iz;
          const double cb = cam.fy * iz, cd = -cam.fy * py * iz * iz;
          const double Jp0[6] = {ca, 0.0, cc, cc * py, ca * pz - cc * px, -ca * py};
          const double Jp1[6] = {0.0, cb, cd, -cb * pz + cd * py, -cd * px, cb * px};
          double Jl0[3], Jl1[3];
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            Jl0[m] = ca * P[m] + cc * P[6 + m];
            Jl1[m] = cb * P[3 + m] + cd * P[6 + m];
          }
          double* d = wobs + (size_t)BA_OBS_D * o;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            d[r] = Jp0[r];
            d[6 + r] = Jp1[r];
          }
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            d[12 + m] = Jl0[m];
            d[15 + m] = Jl1[m];
          }
          d[18] = w;
          d[19] = eu;
          d[20] = ev;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int m = 0; m < 3; ++m) d[21 + 3 * r + m] = (w * Jp0[r]) * Jl0[m] + (w * Jp1[r]) * Jl1[m];
          int k = 0;
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int m = r; m < 3; ++m) V[k++] += (w * Jl0[r]) * Jl0[m] + (w * Jl1[r]) * Jl1[m];
#pragma unroll
          for (int m = 0; m < 3; ++m) g[m] += (w * Jl0[m]) * eu + (w * Jl1[m]) * ev;
        }
        double* d = wlm + (size_t)BA_LM_D * i;
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = V[k];
#pragma unroll
        for (int m = 0; m < 3; ++m) d[6 + m] = g[m];
      }
      __syncthreads();
      for (int u = tid; u < nf * 27; u += BA_T) {
        const int j = u / 27, t = u - 27 * j;
        int r = 0, c = 0;
        if (t < 21) {
          int rest = t;
          while (rest >= 6 - r) {
            rest -= 6 - r;
            ++r;
          }
          c = r + rest;
        } else {
          r = t - 21;
        }
        double acc = 0.0;
        const int c0 = t < 21 ? c : 19, c1 = t < 21 ? 6 + c : 20;      // the second factor: J_pose's column c, or e
        for (int i0 = 0; i0 < L; i0 += 4) {                             // (four landmarks' loads in flight; added in order)
          bool on[4];
          double term[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int o = tab[(size_t)VO_WINDOW_WMAX * min(i0 + v, L - 1) + nfix + j];
            on[v] = i0 + v < L && o >= 0;
            const double* d = wobs + (size_t)BA_OBS_D * (on[v] ? o : 0);
            const double w = d[18];
            term[v] = (w * d[r]) * d[c0] + (w * d[6 + r]) * d[c1];
          }
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (on[v]) acc += term[v];
        }
        s_U[u] = acc;
      }
      __syncthreads();
    }
    // ---- damp: V*^-1 per landmark, Y = W V*^-1 per observation of a free pose ----
    const double damp = 1.0 + lam;
    {
      bool bad = false;
      for (int i = tid; i < L; i += BA_T) {
        double* d = wlm + (size_t)BA_LM_D * i;
        const double v00 = d[0] * damp, v01 = d[1], v02 = d[2], v11 = d[3] * damp, v12 = d[4], v22 = d[5] * damp;
        const double l00 = sqrt(v00);
        const double l10 = v01 / l00, l20 = v02 / l00;
        const double d1 = v11 - l10 * l10;
        const double l11 = sqrt(d1);
        const double l21 = (v12 - l20 * l10) / l11;
        const double d2 = v22 - l20 * l20 - l21 * l21;
        const double l22 = sqrt(d2);
        if (!(v00 > 0.0 && d1 > 0.0 && d2 > 0.0)) {
          bad = true;
          continue;
        }
        const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
        const double m10 = -l10 * m00 * m11;
        const double m21 = -l21 * m11 * m22;
        const double m20 = -(l20 * m00 + l21 * m10) * m22;
        double I[9];
        I[0] = m00 * m00 + m10 * m10 + m20 * m20;
        I[1] = I[3] = m10 * m11 + m20 * m21;
        I[2] = I[6] = m20 * m22;
        I[4] = m11 * m11 + m21 * m21;
        I[5] = I[7] = m21 * m22;
        I[8] = m22 * m22;
        d[9] = I[0];
        d[10] = I[1];
        d[11] = I[2];
        d[12] = I[4];
        d[13] = I[5];
        d[14] = I[8];
        const int e = lm_start[i + 1];
        for (int o = lm_start[i]; o < e; ++o) {
          if (obs_slot[o] < nfix) continue;
          double* wo = wobs + (size_t)BA_OBS_D * o;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int m = 0; m < 3; ++m)
              wo[39 + 3 * r + m] = wo[21 + 3 * r] * I[m] + wo[22 + 3 * r] * I[3 + m] + wo[23 + 3 * r] * I[6 + m];
        }
      }
      if (bad) s_flag = 1;
    }
    __syncthreads();
    bool rejected = s_flag != 0;
    __syncthreads();
    if (!rejected) {
      // ---- reduce: S (packed lower triangle) and b ----
      for (int u = tid; u < (n * (n + 1)) / 2; u += BA_T) {
        int row = (int)((sqrt(8.0 * u + 1.0) - 1.0) * 0.5);          // u = low(row, col), col <= row
        while (low(row + 1, 0) <= u) ++row;
        while (low(row, 0) > u) --row;
        const int col = u - low(row, 0);
        const int j = row / 6, r = row - 6 * j, k = col / 6, c = col - 6 * k;
        double acc = 0.0;
        // four landmarks per pass, their loads in flight together; the terms are added in landmark order all the same
        for (int i0 = 0; i0 < L; i0 += 4) {
          bool both[4];
          double t[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int* tr = tab + (size_t)VO_WINDOW_WMAX * min(i0 + v, L - 1) + nfix;
            const int oj = tr[j], ok = tr[k];
            both[v] = i0 + v < L && oj >= 0 && ok >= 0;
            const double* y = wobs + (size_t)BA_OBS_D * (both[v] ? oj : 0) + 39 + 3 * r;
            const double* w = wobs + (size_t)BA_OBS_D * (both[v] ? ok : 0) + 21 + 3 * c;
            t[v] = y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
          }
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (both[v]) acc += t[v];
        }
        double base = 0.0;
        if (j == k) {
          base = s_U[27 * j + tri_index(c, r)];
          if (r == c) base *= damp;
        }
        s_S[u] = base - acc;
      }
      if (tid < n) {
        const int j = tid / 6, r = tid - 6 * j;
        double acc = 0.0;
        for (int i = 0; i < L; ++i) {
          const int o = tab[(size_t)VO_WINDOW_WMAX * i + nfix + j];
          if (o < 0) continue;
          const double* y = wobs + (size_t)BA_OBS_D * o + 39 + 3 * r;
          const double* g = wlm + (size_t)BA_LM_D * i + 6;
          acc += y[0] * g[0] + y[1] * g[1] + y[2] * g[2];
        }
        s_b[tid] = s_U[27 * j + 21 + r] - acc;
      }
      __syncthreads();
      // ---- Cholesky by columns: thread r owns row r ----
      for (int k = 0; k < n; ++k) {
        const int r = k + tid;
        double v = 0.0;
        if (r < n) {
          v = s_S[low(r, k)];
          for (int m = 0; m < k; ++m) v -= s_S[low(r, m)] * s_S[low(k, m)];
          s_S[low(r, k)] = v;
        }
        __syncthreads();
        const double piv = s_S[low(k, k)];
        if (!(piv > 0.0)) {                       // (the same value in every thread)
          rejected = true;
          break;
        }
        const double s = sqrt(piv);
        if (r == k) s_diag[k] = s;
        if (r > k && r < n) s_S[low(r, k)] = v / s;
        __syncthreads();
      }
    }
    if (rejected) {
      __syncthreads();
      if (tid == 0) s_flag = 0;
      __syncthreads();
      ++trials;
      lam *= 10.0;
      continue;
    }
    // ---- solve L y = b, L^T d = y by columns; d ends in s_b ----
    for (int k = 0; k < n; ++k) {
      const double yk = s_b[k] / s_diag[k];
      if (tid == k) s_y[k] = yk;
      if (tid > k && tid < n) s_b[tid] -= s_S[low(tid, k)] * yk;
      __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
      const double xk = s_y[k] / s_diag[k];
      if (tid == k) s_b[k] = xk;
      if (tid < k) s_y[tid] -= s_S[low(k, tid)] * xk;
      __syncthreads();
    }
    // ---- step: trial poses, trial landmarks, |delta| and |x| ----
    double nrm[2] = {0.0, 0.0};
    if (tid < n) nrm[0] += s_b[tid] * s_b[tid];
    if (tid < nf) {
      const double* P = s_pose + 12 * (nfix + tid);
      const double* d = s_b + 6 * tid;
      nrm[1] += P[9] * P[9] + P[10] * P[10] + P[11] * P[11];
      double ca, cb;
      rodrigues_coefficients(d[3] * d[3] + d[4] * d[4] + d[5] * d[5], &ca, &cb);
      const double Wx[9] = {0.0, -d[5], d[4], d[5], 0.0, -d[3], -d[4], d[3], 0.0};
      double E[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double w2 = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) w2 += Wx[3 * r + k] * Wx[3 * k + c];
          E[3 * r + c] = (r == c ? 1.0 : 0.0) + ca * Wx[3 * r + c] + cb * w2;
        }
      double* T = s_try + 12 * (nfix + tid);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = E[3 * r] * P[c] + E[3 * r + 1] * P[3 + c] + E[3 * r + 2] * P[6 + c];
        T[9 + r] = E[3 * r] * P[9] + E[3 * r + 1] * P[10] + E[3 * r + 2] * P[11] + d[r];
      }
    }
    for (int i = tid; i < L; i += BA_T) {
      double* d = wlm + (size_t)BA_LM_D * i;
      double rhs[3] = {d[6], d[7], d[8]};
      const int e = lm_start[i + 1];
      for (int o = lm_start[i]; o < e; ++o) {
        const int s = obs_slot[o];
        if (s < nfix) continue;
        const double* w = wobs + (size_t)BA_OBS_D * o + 21;
        const double* dp = s_b + 6 * (s - nfix);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          double t = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) t += w[3 * r + m] * dp[r];
          rhs[m] -= t;
        }
      }
      const double dl0 = d[9] * rhs[0] + d[10] * rhs[1] + d[11] * rhs[2];
      const double dl1 = d[10] * rhs[0] + d[12] * rhs[1] + d[13] * rhs[2];
      const double dl2 = d[11] * rhs[0] + d[13] * rhs[1] + d[14] * rhs[2];
      const double X0 = X[3 * i], X1 = X[3 * i + 1], X2 = X[3 * i + 2];
      d[15] = X0 + dl0;
      d[16] = X1 + dl1;
      d[17] = X2 + dl2;
      nrm[0] += dl0 * dl0 + dl1 * dl1 + dl2 * dl2;
      nrm[1] += X0 * X0 + X1 * X1 + X2 * X2;
    }
    block_sums<2>(nrm, s_red);                    // (its barriers also publish s_try and the trial landmarks)
    if (sqrt(nrm[0]) <= a.step_tol * (1.0 + sqrt(nrm[1]))) {
      status = 0;                                 // a step this small is not taken (nor counted)
      break;
    }
    ++trials;
    // ---- evaluate the trial point ----
    double ev2[2];
    {
      // (the trial landmarks are read through a stride-BA_LM_D view: same loop as eval_partial)
      double c = 0.0, back = 0.0;
      for (int i = tid; i < L; i += BA_T) {
        const double* d = wlm + (size_t)BA_LM_D * i + 15;
        const double X0 = d[0], X1 = d[1], X2 = d[2];
        const int e = lm_start[i + 1];
        for (int o = lm_start[i]; o < e; ++o) {
          const double* P = s_try + 12 * obs_slot[o];
          const double px = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[9];
          const double py = P[3] * X0 + P[4] * X1 + P[5] * X2 + P[10];
          const double pz = P[6] * X0 + P[7] * X1 + P[8] * X2 + P[11];
          if (!(pz > 0.0)) back += 1.0;
          const double iz = 1.0 / pz;
          const double eu = obs_xy[2 * o] - (cam.fx * px * iz + cam.cx);
          const double ev = obs_xy[2 * o + 1] - (cam.fy * py * iz + cam.cy);
          const double r2 = eu * eu + ev * ev;
          double rho = r2;
          if (huber > 0.0) {
            const double r = sqrt(r2);
            if (r > huber) rho = 2.0 * huber * r - huber * huber;
          }
          c += rho;
        }
      }
      ev2[0] = c;
      ev2[1] = back;
    }
    block_sums<2>(ev2, s_red);
    if (ev2[1] == 0.0 && ev2[0] <= cost) {
      if (tid < 12 * W) s_pose[tid] = s_try[tid];
      for (int i = tid; i < L; i += BA_T) {
        const double* d = wlm + (size_t)BA_LM_D * i + 15;
        X[3 * i] = d[0];
        X[3 * i + 1] = d[1];
        X[3 * i + 2] = d[2];
      }
      cost = ev2[0];
      ++it;
      lam = fmax(lam / 10.0, BA_LAMBDA_MIN);
      need_lin = true;
      __syncthreads();
    } else {
      lam *= 10.0;
    }
  }
  // (the landmarks are in place since the last accepted step; the fixed slots are written back as they were read)
  if (tid < 12 * W) poses[tid] = s_pose[tid];
  if (tid == 0) {
    res->status = status;
    res->iterations = it;
    res->trials = trials;
    res->n_obs = M;
    res->cost0 = cost0;
    res->cost = cost;
    res->lambda = lam;
  }
}

// ---- the window of W observation records ----

constexpr int WB_T = 256;
struct wb_records {
  const vo_track::word* rec[VO_WINDOW_WMAX];     // oldest first
};

// match[r * W + s] = the first row of record s that carries the id of row r of the newest record, -1 when none
__global__ __launch_bounds__(WB_T) void window_match_kernel(wb_records R, int W, int cap, int* __restrict__ match) {
  const int r = blockIdx.x * WB_T + threadIdx.x, s = blockIdx.y;
  const int n_new = vo_track::rows(R.rec[W - 1], cap);
  if (r >= n_new) return;
  if (s == W - 1) {
    match[(size_t)r * W + s] = r;
    return;
  }
  const int id = vo_track::row_id(vo_track::row(R.rec[W - 1], r));
  const int n = vo_track::rows(R.rec[s], cap);
  int found = -1;
  for (int k = 0; k < n; ++k) {
    if (vo_track::row_id(vo_track::row(R.rec[s], k)) == id) {
      found = k;
      break;
    }
  }
  match[(size_t)r * W + s] = found;
}

// One workgroup: the join (window_join_device.h) over the match table, and the window's head {L, M, flags, 0}.
__global__ __launch_bounds__(BA_T) void window_build_kernel(wb_records R, int W, int cap, int L_cap, int M_cap,
                                                            const int* __restrict__ match, int32_t* __restrict__ head,
                                                            int32_t* __restrict__ lm_start, int32_t* __restrict__ obs_slot,
                                                            double* __restrict__ obs_xy, double* __restrict__ X,
                                                            int32_t* __restrict__ lm_id) {
  __shared__ vo_window_lds<BA_T> s_win;
  vo_window_emit<BA_T>(
      s_win, W, cap, L_cap, M_cap, [&](int s) { return R.rec[s]; }, [&](int s, int, int r) { return match[(size_t)r * W + s]; },
      lm_id, X, nullptr, lm_start, obs_slot, obs_xy, nullptr);
  if (threadIdx.x == 0) {
    head[0] = s_win.tot[0];
    head[1] = s_win.tot[1];
    head[2] = s_win.tot[2];
    head[3] = 0;
  }
}

int resolve_params(vo_ctx* ctx, const vo_ba_params* prm, ba_args* a) {
  vo_ba_params p;
  memset(&p, 0, sizeof(p));
  if (prm) p = *prm;
  vo_lm_params lm;
  VO_TRY(vo_resolve_lm_params(ctx, "window_ba", p.max_iter, p.max_trials, p.huber_px, p.lambda0, p.step_tol, &lm));
  a->max_iter = lm.max_iter;
  a->max_trials = lm.max_trials;
  a->huber = lm.huber;
  a->lambda0 = lm.lambda0;
  a->step_tol = lm.step_tol;
  VO_REQUIRE(ctx, p.n_fixed >= 0, "window_ba: n_fixed must be 0 (default 2) or the number of held slots, got %d", p.n_fixed);
  a->n_fixed = p.n_fixed ? p.n_fixed : 2;
  return VO_OK;
}

}  // namespace

extern "C" {

size_t vo_window_ba_workspace_bytes(int S, int W, int L_cap, int M_cap) {
  if (S < 1 || W < 2 || W > VO_WINDOW_WMAX || L_cap < 1 || M_cap < 1) return 0;
  return (size_t)S * window_doubles(L_cap, M_cap) * sizeof(double);
}

int vo_window_ba_dev(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* d_counts, const double* d_K, double* d_poses,
                     double* d_X, const int32_t* d_lm_start, const int32_t* d_obs_slot, const double* d_obs_xy,
                     const vo_ba_params* prm, vo_ba_result* d_results) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_counts && d_K && d_poses && d_X && d_lm_start && d_obs_slot && d_obs_xy && d_results, "window_ba: null pointer");
  VO_TRY(vo_check_window_shape(ctx, "window_ba", S, W, L_cap, M_cap));
  ba_args a;
  VO_TRY(resolve_params(ctx, prm, &a));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  VO_TRY(vo_ensure(ctx, ctx->ba_work, vo_window_ba_workspace_bytes(S, W, L_cap, M_cap)));
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
  a.work = (double*)ctx->ba_work.p;
  a.res = d_results;
  {
    vo_prof_scope ps(ctx, VO_K_WINDOW_BA);
    hipLaunchKernelGGL(window_ba_kernel, dim3(S), dim3(BA_T), 0, ctx->stream, a);
  }
  return vo_check_launch(ctx, "window_ba_kernel");
}

int vo_window_ba(vo_ctx* ctx, int S, int W, int L_cap, int M_cap, const int32_t* counts, const double* K, double* poses, double* X,
                 const int32_t* lm_start, const int32_t* obs_slot, const double* obs_xy, const vo_ba_params* prm,
                 vo_ba_result* results) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, counts && K && poses && X && lm_start && obs_slot && obs_xy && results, "window_ba: null pointer");
  VO_TRY(vo_check_window_shape(ctx, "window_ba", S, W, L_cap, M_cap));
  const size_t s = (size_t)S;
  const size_t bytes[8] = {s * 16,           s * 72,        s * W * 96,        s * L_cap * 24, s * ((size_t)L_cap + 1) * 4,
                           s * M_cap * 4,    s * M_cap * 16, s * sizeof(vo_ba_result)};
  const void* src[7] = {counts, K, poses, X, lm_start, obs_slot, obs_xy};
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  for (int k = 0; k < 8; ++k) VO_TRY(vo_ensure(ctx, ctx->scratch[k], bytes[k]));
  for (int k = 0; k < 7; ++k) VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch[k].p, src[k], bytes[k], hipMemcpyHostToDevice, st));
  vo_buf* b = ctx->scratch;
  VO_TRY(vo_window_ba_dev(ctx, S, W, L_cap, M_cap, (const int32_t*)b[0].p, (const double*)b[1].p, (double*)b[2].p, (double*)b[3].p,
                          (const int32_t*)b[4].p, (const int32_t*)b[5].p, (const double*)b[6].p, prm, (vo_ba_result*)b[7].p));
  VO_HIP_TRY(ctx, hipMemcpyAsync(poses, b[2].p, bytes[2], hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(X, b[3].p, bytes[3], hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(results, b[7].p, bytes[7], hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_window_from_tracks_dev(vo_ctx* ctx, int W, const void* const* d_records, int cap, int L_cap, int M_cap, int32_t* d_head,
                              int32_t* d_lm_start, int32_t* d_obs_slot, double* d_obs_xy, double* d_X, int32_t* d_lm_id) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_records && d_head && d_lm_start && d_obs_slot && d_obs_xy && d_X && d_lm_id, "window_from_tracks: null pointer");
  VO_TRY(vo_check_window_shape(ctx, "window_from_tracks", 1, W, L_cap, M_cap));
  VO_REQUIRE(ctx, cap >= 1 && cap <= (1 << 20), "window_from_tracks: cap must be 1 .. 1048576 rows, got %d", cap);
  wb_records R;
  for (int s = 0; s < VO_WINDOW_WMAX; ++s) R.rec[s] = nullptr;
  for (int s = 0; s < W; ++s) {
    VO_REQUIRE(ctx, d_records[s] && ((uintptr_t)d_records[s] & 15) == 0, "window_from_tracks: record %d is null or not 16-byte aligned", s);
    R.rec[s] = (const unsigned long long*)d_records[s];
  }
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  VO_TRY(vo_ensure(ctx, ctx->ba_match, (size_t)cap * W * sizeof(int)));
  hipStream_t st = ctx->stream;
  {
    vo_prof_scope ps(ctx, VO_K_WINDOW_BUILD);
    hipLaunchKernelGGL(window_match_kernel, dim3(vo_cdiv(cap, WB_T), W), dim3(WB_T), 0, st, R, W, cap, (int*)ctx->ba_match.p);
  }
  VO_TRY(vo_check_launch(ctx, "window_match_kernel"));
  {
    vo_prof_scope ps(ctx, VO_K_WINDOW_BUILD);
    hipLaunchKernelGGL(window_build_kernel, dim3(1), dim3(BA_T), 0, st, R, W, cap, L_cap, M_cap, (const int*)ctx->ba_match.p, d_head,
                       d_lm_start, d_obs_slot, d_obs_xy, d_X, d_lm_id);
  }
  return vo_check_launch(ctx, "window_build_kernel");
}

}  // extern "C"
