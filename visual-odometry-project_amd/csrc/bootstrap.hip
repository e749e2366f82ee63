// Two-view bootstrap (reference: src/vo/landmarks/triangulation.py:110-350, src/vo/helpers.py:31-54), the step
// before the per-frame loop (src/main.py:204-230), as four kernels:
//
//   f8_hyp_kernel      one lane per RANSAC sample of 8 correspondences: Kronecker rows (triangulation.py:203-205), the
//                      null vector of the 8x9 system (np.linalg.svd(Q)[2][-1], :209-212) by a one-sided (Hestenes) Jacobi
//                      iteration on its columns -- the sample's rows in registers, the accumulated rotations in LDS --
//                      and the rank-2 projection (:214-217: the smallest singular triplet of the 3x3 removed)
//   f_score_kernel     every hypothesis against every correspondence: algebraic error (p2^T F p1)^2 (:140-145) or the
//                      squared distance to the epipolar lines in both images; strict `<` threshold; counts + mask rows
//   f8_fit_kernel      the 8-point fit over ALL (masked) correspondences (RANSAC's closing model_fn(population[inliers]),
//                      src/vo/algorithms/ransac.py:123-127; _find_fundamental_matrix :165-222): Hartley normalisation,
//                      the 9x9 normal matrix by a workgroup reduction and ALL its eigenvectors V by Jacobi; where its
//                      eigenvalues show that squaring Q's conditioning cost accuracy (lambda8 < 1e-5 lambda1: small
//                      baselines, near-planar scenes), a second pass over the points forms the normal matrix of Q V --
//                      nearly diagonal and graded -- whose smallest eigenvector by Jacobi with a per-pair relative test
//                      corrects V's; rank 2.  Pinned to 50-digit values at sigma8 / sigma1 of Q down to
//                      1e-5 (tests/test_gpu_twoview_reference.py)
//   relative_pose_kernel  E = K2^T F K1, its SVD (3x3 Jacobi), the four [R | +-T] (:245-277), the four cheirality
//                      votes over the inliers by DLT (:313-332), the winner's triangulation of all points (:334-350)
//
// fp64 throughout, no FMA contraction.  Parity: tests/golden/bootstrap.npz (the reference's own NumPy route) -- F up to
// scale / sign, the RANSAC trace's inlier mask exactly, M, landmarks to 1e-9 / 1e-6.
#include "dlt_device.h"
#include "fscore_device.h"
#include "rng_device.h"
#include "state_device.h"
#include "vo_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int HB = 64;        // hypotheses (lanes) per workgroup of f8_hyp_kernel

// ---- 3x3 symmetric eigenproblem in registers (cyclic Jacobi, unrolled): A -> diagonal, V its eigenvectors (columns) ----
template <int P, int Q>
__device__ __forceinline__ void sym3_rotate(double (&A)[3][3], double (&V)[3][3]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  constexpr int R = 3 - P - Q;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ void sym3_eig(double (&A)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-34 * dia || off == 0.0) break;
    sym3_rotate<0, 1>(A, V);
    sym3_rotate<0, 2>(A, V);
    sym3_rotate<1, 2>(A, V);
  }
}

// F (row-major 3x3) -> F with its smallest singular value set to zero (triangulation.py:214-217):
// F' = F - (F v3) v3^T with v3 the eigenvector of F^T F to its smallest eigenvalue
__device__ __forceinline__ void rank2(double* F) {
  double G[3][3], V[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) G[a][b] = F[a] * F[b] + F[3 + a] * F[3 + b] + F[6 + a] * F[6 + b];
  sym3_eig(G, V);
  int m = 0;
  if (G[1][1] < G[m][m]) m = 1;
  if (G[2][2] < G[m][m]) m = 2;
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = m == 0 ? V[k][0] : (m == 1 ? V[k][1] : V[k][2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double fv = F[3 * r] * v[0] + F[3 * r + 1] * v[1] + F[3 * r + 2] * v[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) F[3 * r + c] = F[3 * r + c] - fv * v[c];
  }
}

// Hartley normalisation of n points given their sums (helpers.py:31-54): s = sqrt(2) / sqrt(mean |p - mu|^2)
struct hartley {
  double s, tx, ty;        // x' = s x + tx, y' = s y + ty
};

// T2^T F T1 for T = [[s, 0, tx], [0, s, ty], [0, 0, 1]]
__device__ __forceinline__ void denormalise(double* F, const hartley& h1, const hartley& h2) {
  double A[9];             // F T1
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    A[3 * r] = F[3 * r] * h1.s;
    A[3 * r + 1] = F[3 * r + 1] * h1.s;
    A[3 * r + 2] = F[3 * r] * h1.tx + F[3 * r + 1] * h1.ty + F[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[c] = h2.s * A[c];
    F[3 + c] = h2.s * A[3 + c];
    F[6 + c] = h2.tx * A[c] + h2.ty * A[3 + c] + A[6 + c];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// one lane = one sample of 8 correspondences (idx, each within the population) -> F (9 doubles, row-major) at Fh
__device__ __forceinline__ void f8_solve(const double* __restrict__ p1, const double* __restrict__ p2, const int (&idx)[8],
                                         int normalize, double (*s_V)[HB], int lane, double* __restrict__ Fh) {
  double x1[8], y1[8], x2[8], y2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = idx[k];
    x1[k] = p1[2 * i];
    y1[k] = p1[2 * i + 1];
    x2[k] = p2[2 * i];
    y2[k] = p2[2 * i + 1];
  }
  hartley h1 = {1.0, 0.0, 0.0}, h2 = {1.0, 0.0, 0.0};
  if (normalize) {
    auto fit = [](const double* x, const double* y) {
      double mx = 0.0, my = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        mx += x[k];
        my += y[k];
      }
      mx = mx / 8.0;
      my = my / 8.0;
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) v += (x[k] - mx) * (x[k] - mx) + (y[k] - my) * (y[k] - my);
      const double s = sqrt(2.0) / sqrt(v / 8.0);
      hartley r = {s, -s * mx, -s * my};
      return r;
    };
    h1 = fit(x1, y1);
    h2 = fit(x2, y2);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      x1[k] = h1.s * x1[k] + h1.tx;
      y1[k] = h1.s * y1[k] + h1.ty;
      x2[k] = h2.s * x2[k] + h2.tx;
      y2[k] = h2.s * y2[k] + h2.ty;
    }
  }
  // Q[k] = kron(p1_k, p2_k): entry 3a + b = p1[a] p2[b]
  double Q[8][9];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double a[3] = {x1[k], y1[k], 1.0}, b[3] = {x2[k], y2[k], 1.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Q[k][3 * i + j] = a[i] * b[j];
  }
#pragma unroll
  for (int e = 0; e < 81; ++e) s_V[e][lane] = (e / 9 == e % 9) ? 1.0 : 0.0;
  // one-sided Jacobi: rotate column pairs until mutually orthogonal; the 8x9 system has a null space, whose
  // direction ends up in the column of (near-)zero norm
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool any = false;
#pragma unroll
    for (int P = 0; P < 8; ++P) {
#pragma unroll
      for (int Qc = P + 1; Qc < 9; ++Qc) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          alpha += Q[r][P] * Q[r][P];
          beta += Q[r][Qc] * Q[r][Qc];
          gamma += Q[r][P] * Q[r][Qc];
        }
        if (gamma == 0.0 || gamma * gamma <= 1e-30 * (alpha * beta)) continue;
        any = true;
        const double d = beta - alpha, g = 2.0 * gamma;
        const double w = fabs(d) + sqrt(d * d + g * g);
        const double rn = sqrt(w * w + g * g);
        const double c = w / rn;
        const double sm = fabs(g) / rn;
        const double s = (d == 0.0 || (d > 0.0) == (g > 0.0)) ? sm : -sm;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const double ap = Q[r][P], aq = Q[r][Qc];
          Q[r][P] = c * ap - s * aq;
          Q[r][Qc] = s * ap + c * aq;
        }
#pragma unroll
        for (int r = 0; r < 9; ++r) {
          const double vp = s_V[9 * r + P][lane], vq = s_V[9 * r + Qc][lane];
          s_V[9 * r + P][lane] = c * vp - s * vq;
          s_V[9 * r + Qc][lane] = s * vp + c * vq;
        }
      }
    }
    if (!any) break;
  }
  int m = 0;
  double best = 0.0;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    double nrm = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) nrm += Q[r][c] * Q[r][c];
    if (c == 0 || nrm < best) {
      best = nrm;
      m = c;
    }
  }
  // F = Vh[-1].reshape(3, 3).T (stacked column-wise, triangulation.py:212): F[b][a] = f[3a + b]
  double F[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) F[3 * b + a] = s_V[9 * (3 * a + b) + m][lane];
  rank2(F);
  if (normalize) denormalise(F, h1, h2);
#pragma unroll
  for (int k = 0; k < 9; ++k) Fh[k] = F[k];
}

__global__ __launch_bounds__(HB) void f8_hyp_kernel(const double* __restrict__ p1, const double* __restrict__ p2, int N,
                                                    const int* __restrict__ samples, int Hyp, int normalize,
                                                    double* __restrict__ Fout) {
  __shared__ double s_V[81][HB];            // accumulated rotations, [entry][lane]
  const int lane = threadIdx.x;
  const int h = blockIdx.x * HB + lane;
  if (h >= Hyp) return;
  int idx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) idx[k] = min(max(samples[8 * h + k], 0), N - 1);
  f8_solve(p1, p2, idx, normalize, s_V, lane, Fout + (size_t)9 * h);
}

using vo_fscore::f_score_body;       // fscore_device.h: f_error and the workgroup's walk over the correspondences

__global__ __launch_bounds__(256) void f_score_kernel(const double* __restrict__ p1, const double* __restrict__ p2, int N,
                                                      const double* __restrict__ Fs, int kind, double thr,
                                                      int* __restrict__ counts, unsigned long long* __restrict__ masks,
                                                      int words) {
  __shared__ int s_cnt[4];
  f_score_body(p1, p2, N, Fs, kind, thr, counts, masks, words, s_cnt);
}

// ---------------------------------------------------------------------------------------------------------------
// 9x9 symmetric cyclic Jacobi in LDS (one work item): A -> diagonal, V its eigenvectors (columns).  graded == false:
// the sweeps end once off <= 1e-34 dia.  graded == true, for a nearly diagonal matrix whose diagonal spans many orders:
// a pair is left alone once apq^2 <= 1e-32 app aqq and the sweeps end when none was rotated -- the global test stops
// while the small diagonal entries are still coupled to each other.
template <bool graded>
__device__ void sym9_jacobi(double* A /*81*/, double* V /*81*/) {
  for (int e = 0; e < 81; ++e) V[e] = (e / 9 == e % 9) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    if (!graded) {
      double off = 0.0, dia = 0.0;
      for (int r = 0; r < 9; ++r)
        for (int c = 0; c < 9; ++c) {
          const double v = A[9 * r + c];
          if (r == c) dia += v * v;
          else off += v * v;
        }
      if (off == 0.0 || off <= 1e-34 * dia) break;
    }
    bool any = false;
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double apq = A[9 * p + q];
        if (apq == 0.0) continue;
        if (graded && apq * apq <= 1e-32 * (A[9 * p + p] * A[9 * q + q])) continue;
        any = true;
        const double theta = (A[9 * q + q] - A[9 * p + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 9; ++k) {
          if (k == p || k == q) continue;
          const double akp = A[9 * k + p], akq = A[9 * k + q];
          const double np_ = c * akp - s * akq, nq = s * akp + c * akq;
          A[9 * k + p] = A[9 * p + k] = np_;
          A[9 * k + q] = A[9 * q + k] = nq;
        }
        A[9 * p + p] = A[9 * p + p] - t * apq;
        A[9 * q + q] = A[9 * q + q] + t * apq;
        A[9 * p + q] = A[9 * q + p] = 0.0;
        for (int k = 0; k < 9; ++k) {
          const double vp = V[9 * k + p], vq = V[9 * k + q];
          V[9 * k + p] = c * vp - s * vq;
          V[9 * k + q] = s * vp + c * vq;
        }
      }
    if (graded && !any) break;
  }
}

__device__ __forceinline__ double block_sum(double v, double* s_red /*[4]*/, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// the 8-point fit over the points whose mask byte is set (all if mask == NULL); one workgroup
// lambda8 / lambda1 of Q^T Q below which the null vector is refined (sigma8 / sigma1 < 3.2e-3).  The one-pass vector was
// measured at up to 6e-18 lambda1 / lambda8 from the 50-digit one: above the threshold it is good to 6e-13.
constexpr double F8_SECOND_PASS = 1e-5;
struct f8_fit_lds {
  double red[4], A[81], V[81], W[81], f[9];
  int second;          // the first pass's eigenvalues ask for the second
};

__device__ __forceinline__ void f8_fit_body(const double* __restrict__ p1, const double* __restrict__ p2, int N,
                                            const uint8_t* __restrict__ mask, int normalize, double* __restrict__ Fout,
                                            int* __restrict__ n_used, f8_fit_lds& lds) {
  double *s_red = lds.red, *s_A = lds.A, *s_V = lds.V, *s_W = lds.W, *s_f = lds.f;
  const int tid = threadIdx.x;
  hartley h1 = {1.0, 0.0, 0.0}, h2 = {1.0, 0.0, 0.0};
  double cnt = 0.0;
  for (int i = tid; i < N; i += 256) cnt += (!mask || mask[i]) ? 1.0 : 0.0;
  const double n = block_sum(cnt, s_red, tid);
  if (normalize) {
    double sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0;
    for (int i = tid; i < N; i += 256)
      if (!mask || mask[i]) {
        sx1 += p1[2 * i];
        sy1 += p1[2 * i + 1];
        sx2 += p2[2 * i];
        sy2 += p2[2 * i + 1];
      }
    const double mx1 = block_sum(sx1, s_red, tid) / n, my1 = block_sum(sy1, s_red, tid) / n;
    const double mx2 = block_sum(sx2, s_red, tid) / n, my2 = block_sum(sy2, s_red, tid) / n;
    double v1 = 0, v2 = 0;
    for (int i = tid; i < N; i += 256)
      if (!mask || mask[i]) {
        const double a = p1[2 * i] - mx1, b = p1[2 * i + 1] - my1, c = p2[2 * i] - mx2, d = p2[2 * i + 1] - my2;
        v1 += a * a + b * b;
        v2 += c * c + d * d;
      }
    const double s1 = sqrt(2.0) / sqrt(block_sum(v1, s_red, tid) / n), s2 = sqrt(2.0) / sqrt(block_sum(v2, s_red, tid) / n);
    h1 = {s1, -s1 * mx1, -s1 * my1};
    h2 = {s2, -s2 * mx2, -s2 * my2};
  }
  // Up to two passes over the points.  The first forms Q^T Q (45 sums) and takes ALL its eigenvectors V by Jacobi: forming
  // the product squares Q's conditioning, so the smallest of them is only good to about eps (sigma1 / sigma8)^2 -- measured
  // 2e-18 lambda1 / lambda8 against 50-digit values.  Where lambda8 >= F8_SECOND_PASS lambda1 that is the answer.  Else the second
  // forms the same 45 sums of q' = V^T q: its columns are orthogonal up to that error, so the matrix is nearly diagonal
  // with the squared singular values on its diagonal, each small entry computed from small terms.  Its eigenvector f' to
  // the smallest diagonal entry (graded Jacobi) is a small correction of a unit vector, and V f' is the null vector to the
  // accuracy of a one-sided Jacobi iteration on Q itself.
  double acc[45];
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (int i = tid; i < N; i += 256) {
      if (mask && !mask[i]) continue;
      const double a[3] = {h1.s * p1[2 * i] + h1.tx, h1.s * p1[2 * i + 1] + h1.ty, 1.0};
      const double b[3] = {h2.s * p2[2 * i] + h2.tx, h2.s * p2[2 * i + 1] + h2.ty, 1.0};
      double q[9];
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) q[3 * u + v] = a[u] * b[v];
      if (pass == 1) {
        double qr[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          double d = 0.0;
#pragma unroll
          for (int k = 0; k < 9; ++k) d += s_V[9 * k + j] * q[k];
          qr[j] = d;
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) q[j] = qr[j];
      }
      int k = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = r; c < 9; ++c) acc[k++] += q[r] * q[c];
    }
    {
      int k = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = r; c < 9; ++c) {
          const double v = block_sum(acc[k++], s_red, tid);
          if (tid == 0) s_A[9 * r + c] = s_A[9 * c + r] = v;
        }
    }
    __syncthreads();
    if (pass == 0) {
      if (tid == 0) {
        sym9_jacobi<false>(s_A, s_V);
        int m = 0;
        for (int c = 1; c < 9; ++c)
          if (s_A[9 * c + c] < s_A[9 * m + m]) m = c;
        double l1 = s_A[9 * m + m], l8 = 0.0;       // the largest eigenvalue and the second smallest
        bool have = false;
        for (int c = 0; c < 9; ++c) {
          if (c == m) continue;
          const double l = s_A[9 * c + c];
          if (l > l1) l1 = l;
          if (!have || l < l8) l8 = l;
          have = true;
        }
        for (int k = 0; k < 9; ++k) s_f[k] = s_V[9 * k + m];
        lds.second = !(l8 >= F8_SECOND_PASS * l1);  // (not finite: the second pass, which hands the NaN on)
      }
      __syncthreads();
      if (!lds.second) break;                       // uniform: every work item reads the same word
    }
  }
  if (tid == 0) {
    if (lds.second) {
      sym9_jacobi<true>(s_A, s_W);
      int m = 0;
      for (int c = 1; c < 9; ++c)
        if (s_A[9 * c + c] < s_A[9 * m + m]) m = c;
      for (int k = 0; k < 9; ++k) {
        double d = 0.0;
        for (int j = 0; j < 9; ++j) d += s_V[9 * k + j] * s_W[9 * j + m];
        s_f[k] = d;
      }
    }
    double F[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) F[3 * b + a] = s_f[3 * a + b];
    rank2(F);
    if (normalize) denormalise(F, h1, h2);
#pragma unroll
    for (int k = 0; k < 9; ++k) Fout[k] = F[k];
    if (n_used) *n_used = (int)n;
  }
}

__global__ __launch_bounds__(256) void f8_fit_kernel(const double* __restrict__ p1, const double* __restrict__ p2, int N,
                                                     const uint8_t* __restrict__ mask, int normalize,
                                                     double* __restrict__ Fout, int* __restrict__ n_used) {
  __shared__ f8_fit_lds lds;
  f8_fit_body(p1, p2, N, mask, normalize, Fout, n_used, lds);
}

// ---------------------------------------------------------------------------------------------------------------
// E -> the four [R | +-T] (triangulation.py:245-277).  U, Vh of E's SVD from the eigenvectors of E^T E; the four
// candidates are the same set whatever signs an SVD routine picks, their ORDER may differ from LAPACK's.
__device__ void decompose_essential(const double* E, double* M4 /*4 x 12*/) {
  double G[3][3], V[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) G[a][b] = E[a] * E[b] + E[3 + a] * E[3 + b] + E[6 + a] * E[6 + b];
  sym3_eig(G, V);
  // order the eigenvalues descending: i0 >= i1 >= i2
  int i0 = 0, i2 = 0;
  double ev[3] = {G[0][0], G[1][1], G[2][2]};
  for (int k = 1; k < 3; ++k) {
    if (ev[k] > ev[i0]) i0 = k;
    if (ev[k] < ev[i2]) i2 = k;
  }
  if (i0 == i2) {            // all equal
    i0 = 0;
    i2 = 2;
  }
  const int i1 = 3 - i0 - i2;
  auto col = [&](int c, double* v) {
    for (int k = 0; k < 3; ++k) v[k] = c == 0 ? V[k][0] : (c == 1 ? V[k][1] : V[k][2]);
  };
  double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
  col(i0, v1);
  col(i1, v2);
  // v3 = v1 x v2 (a right-handed V; E's third singular value is ~0, its direction is the cross product's)
  v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
  v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
  v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
  auto unit_Ev = [&](const double* v, double* u) {
    for (int r = 0; r < 3; ++r) u[r] = E[3 * r] * v[0] + E[3 * r + 1] * v[1] + E[3 * r + 2] * v[2];
    const double n = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int r = 0; r < 3; ++r) u[r] = u[r] / n;
  };
  unit_Ev(v1, u1);
  unit_Ev(v2, u2);
  // u2 made orthogonal to u1 (they are to rounding), u3 = u1 x u2
  {
    const double d = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
    for (int r = 0; r < 3; ++r) u2[r] = u2[r] - d * u1[r];
    const double n = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    for (int r = 0; r < 3; ++r) u2[r] = u2[r] / n;
  }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  // R0 = U W Vh = u2 v1^T - u1 v2^T + u3 v3^T;  R1 = U W^T Vh = -u2 v1^T + u1 v2^T + u3 v3^T.  U and V are both
  // right-handed here, so both have determinant +1 (the reference negates the ones that come out with -1).
  for (int j = 0; j < 2; ++j) {
    const double sg = j == 0 ? 1.0 : -1.0;
    for (int i = 0; i < 2; ++i) {
      double* M = M4 + 12 * (2 * i + j);
      const double st = i == 0 ? 1.0 : -1.0;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M[4 * r + c] = sg * (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
        M[4 * r + 3] = st * u3[r];
      }
    }
  }
}

__global__ void essential_decompose_kernel(const double* __restrict__ E, double* __restrict__ M4) {
  if (threadIdx.x == 0 && blockIdx.x == 0) decompose_essential(E, M4);
}

// one workgroup: E from F, the four candidates, the cheirality votes over the inliers, the final triangulation
struct relative_pose_lds {
  double M4[48];
  int votes[4];
  int best;
};
struct cam_pair {            // the two intrinsic matrices, wherever they live (launch arguments / the device camera table)
  const double *K1, *K2;
};

__device__ __forceinline__ void relative_pose_body(const double* __restrict__ x1, const double* __restrict__ x2, int N,
                                                   const uint8_t* __restrict__ inl, const double* __restrict__ F,
                                                   const cam_pair cams, double* __restrict__ Mout, double* __restrict__ X,
                                                   uint8_t* __restrict__ mask_out, double* __restrict__ M4out,
                                                   relative_pose_lds& lds) {
  double* s_M4 = lds.M4;
  int* s_votes = lds.votes;
  int& s_best = lds.best;
  const int tid = threadIdx.x;
  if (tid == 0) {
    // E = K2^T F K1 (triangulation.py:238-243)
    double A[9], E[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) A[3 * r + c] = F[3 * r] * cams.K1[c] + F[3 * r + 1] * cams.K1[3 + c] + F[3 * r + 2] * cams.K1[6 + c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) E[3 * r + c] = cams.K2[r] * A[c] + cams.K2[3 + r] * A[3 + c] + cams.K2[6 + r] * A[6 + c];
    decompose_essential(E, s_M4);
    for (int m = 0; m < 4; ++m) s_votes[m] = 0;
  }
  __syncthreads();
  if (M4out && tid < 48) M4out[tid] = s_M4[tid];
  double C1[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) C1[4 * r + c] = cams.K1[3 * r + c];     // K1 [I | 0]
    C1[4 * r + 3] = 0.0;
  }
  auto project2 = [&](const double* M, double* C2) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) C2[4 * r + c] = cams.K2[3 * r] * M[c] + cams.K2[3 * r + 1] * M[4 + c] + cams.K2[3 * r + 2] * M[8 + c];
  };
  for (int m = 0; m < 4; ++m) {
    double M[12], C2[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = s_M4[12 * m + k];
    project2(M, C2);
    int votes = 0;
    for (int i = tid; i < N; i += 256) {
      if (inl && !inl[i]) continue;
      double P[3];
      vo_dlt::triangulate_point(C1, x1[2 * i], x1[2 * i + 1], C2, x2[2 * i], x2[2 * i + 1], P);
      const double z2 = M[8] * P[0] + M[9] * P[1] + M[10] * P[2] + M[11];
      votes += (P[2] >= 0.0 && z2 >= 0.0) ? 1 : 0;
    }
    const unsigned long long dummy = 0ull;
    (void)dummy;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) votes += __shfl_xor(votes, off);
    if ((tid & 63) == 0 && votes) atomicAdd(&s_votes[m], votes);
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int m = 1; m < 4; ++m)
      if (s_votes[m] > s_votes[best]) best = m;        // strict `>`: the first of equals (triangulation.py:326)
    s_best = best;
  }
  __syncthreads();
  double M[12], C2[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) M[k] = s_M4[12 * s_best + k];
  project2(M, C2);
  if (tid < 12) Mout[tid] = M[tid];
  for (int i = tid; i < N; i += 256) {
    double P[3];
    vo_dlt::triangulate_point(C1, x1[2 * i], x1[2 * i + 1], C2, x2[2 * i], x2[2 * i + 1], P);
    X[3 * i] = P[0];
    X[3 * i + 1] = P[1];
    X[3 * i + 2] = P[2];
    if (mask_out) {
      const double z2 = M[8] * P[0] + M[9] * P[1] + M[10] * P[2] + M[11];
      mask_out[i] = ((!inl || inl[i]) && P[2] >= 0.0 && z2 >= 0.0) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(256) void relative_pose_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                            int N, const uint8_t* __restrict__ inl, const double* __restrict__ F,
                                                            vo_cam2 cams, double* __restrict__ Mout, double* __restrict__ X,
                                                            uint8_t* __restrict__ mask_out, double* __restrict__ M4out) {
  __shared__ relative_pose_lds lds;
  const cam_pair c = {cams.K1, cams.K2};
  relative_pose_body(x1, x2, N, inl, F, c, Mout, X, mask_out, M4out, lds);
}


// ---------------------------------------------------------------------------------------------------------------
// The 8-point RANSAC loop (src/vo/algorithms/ransac.py:90-121, s = 8) without a host turn: the generator's outputs are
// made on the device, every sample is derived from them where it is solved, and one wavefront per lane replays the
// sequential accept / adapt rule over the batch's inlier counts.  blockIdx.y (the replay and the fit: blockIdx.x) is the
// lane; a lane whose status is not "wants a batch" leaves every kernel at once.
constexpr int F8_BATCH = 2048;                                // samples per batch
constexpr int F8_RAWS = F8_BATCH * vo_rng::CHOICE8_RAWS;     // generator outputs per batch

// The words [first, first + count) of lane q's 32-bit stream (first = its batch number * per_batch) into out + q *
// out_stride.  One work item per 64-bit output: it jumps ahead by its own index, applies XSL-RR and writes the low, then
// the high half -- the order vo_rng_raw32 produces; a buffered half comes first.
__global__ __launch_bounds__(256) void pcg64_fill_kernel(const vo_f8_ctl* __restrict__ ctls, uint32_t* __restrict__ out,
                                                         size_t out_stride, int count, int per_batch) {
  const vo_f8_ctl* ctl = ctls + blockIdx.y;
  if (ctl->status != VO_F8_RUN) return;
  const vo_pcg64 g = ctl->rng;
  uint32_t* o = out + (size_t)blockIdx.y * out_stride;
  const uint64_t first = (uint64_t)ctl->batch * (uint64_t)per_batch, end = first + (uint64_t)count;
  const uint64_t off = g.has_uint32 ? 1u : 0u;
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t == 0 && off && first == 0 && count > 0) o[0] = g.uinteger;
  const uint64_t j = (first > off ? (first - off) >> 1 : 0) + t;       // this work item's 64-bit output
  const uint64_t p = 2 * j + off;                                       // the stream position of its low half
  if (p >= end || p + 1 < first) return;
  const uint64_t v = vo_rng::pcg_output(vo_rng::pcg_advance(vo_rng::make128(g.state_hi, g.state_lo),
                                                            vo_rng::make128(g.inc_hi, g.inc_lo), j + 1));
  if (p >= first) o[p - first] = (uint32_t)v;
  if (p + 1 < end) o[p + 1 - first] = (uint32_t)(v >> 32);
}

// the population of every lane: the host's, or the count a kernel left in device memory (never above the capacity)
__global__ void f8_init_kernel(vo_f8_ctl* __restrict__ ctls, int L, const int32_t* __restrict__ d_n, int n_stride, int n_cap) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= L) return;
  int n = ctls[q].n;
  if (n < 0) n = d_n[(size_t)q * n_stride];
  n = min(n, n_cap);
  ctls[q].n = n;
  // 8 correspondences: the first Floyd draw has range 0 and consumes no output -- the host sampler's case
  if (n < 8) ctls[q].status = VO_F8_FAILED;
  else if (n == 8) ctls[q].status = VO_F8_HOST;
}

// f8_hyp_kernel with the sample derived from the generator outputs 15 h .. 15 h + 14 of the lane's batch and the
// population read from the lane's control block; risky[h] = 1: one of its draws could have been rejected
__global__ __launch_bounds__(HB) void f8_hyp_raw_kernel(const double* __restrict__ p1, const double* __restrict__ p2,
                                                        vo_f8_lanes ln, const vo_f8_ctl* __restrict__ ctls,
                                                        const uint32_t* __restrict__ raws, int normalize,
                                                        double* __restrict__ Fout, uint8_t* __restrict__ risky) {
  __shared__ double s_V[81][HB];
  const int q = blockIdx.y, lane = threadIdx.x;
  if (ctls[q].status != VO_F8_RUN) return;
  const int n = ctls[q].n;                   // >= 9 (f8_init_kernel)
  const int h = blockIdx.x * HB + lane;      // the grid is F8_BATCH / HB workgroups: every h is a sample of the batch
  const uint32_t* rw = raws + (size_t)q * F8_RAWS + (size_t)vo_rng::CHOICE8_RAWS * h;
  uint32_t raw[vo_rng::CHOICE8_RAWS];
#pragma unroll
  for (int k = 0; k < vo_rng::CHOICE8_RAWS; ++k) raw[k] = rw[k];
  int idx[8];
  const bool r = vo_rng::choice8_from_raw(raw, (uint32_t)n, idx);
#pragma unroll
  for (int k = 0; k < 8; ++k) idx[k] = min(max(idx[k], 0), n - 1);      // (they are: a bounded draw is below its upper end)
  risky[(size_t)q * F8_BATCH + h] = r ? 1 : 0;
  f8_solve(p1 + (size_t)q * ln.pts, p2 + (size_t)q * ln.pts, idx, normalize, s_V, lane,
           Fout + ((size_t)q * F8_BATCH + h) * 9);
}

// f_score_kernel for the lanes' batches: grid (F8_BATCH, L); mask rows of `words` words (the capacity's)
__global__ __launch_bounds__(256) void f_score_lanes_kernel(const double* __restrict__ p1, const double* __restrict__ p2,
                                                            vo_f8_lanes ln, const vo_f8_ctl* __restrict__ ctls,
                                                            const double* __restrict__ Fs, int kind, double thr,
                                                            int* __restrict__ counts, unsigned long long* __restrict__ masks,
                                                            int words) {
  __shared__ int s_cnt[4];
  const int q = blockIdx.y;
  if (ctls[q].status != VO_F8_RUN) return;
  f_score_body(p1 + (size_t)q * ln.pts, p2 + (size_t)q * ln.pts, ctls[q].n, Fs + (size_t)q * F8_BATCH * 9, kind, thr,
               counts + (size_t)q * F8_BATCH, masks + (size_t)q * F8_BATCH * words, words, s_cnt);
}

// ONE WAVE per lane walks the batch's counts through ransac.py:90-121 (every sample has a model): 64 samples per round;
// the first sample from `cur` on whose count beats the running best is accepted (strict `>`), the bound adapts through
// the threshold table (host libm: the bound is the host's exactly), and the loop ends where the `while` test first fails.
// Leaves the loop's state in the control block, the status word, and -- when the best so far lives in this batch -- its
// mask row as the bytes the closing fit reads.
__global__ __launch_bounds__(64) void f8_replay_kernel(vo_f8_ctl* __restrict__ ctls, vo_f8_lanes ln,
                                                       const int* __restrict__ counts_all, const uint8_t* __restrict__ risky_all,
                                                       const unsigned long long* __restrict__ masks_all, int words,
                                                       const double* __restrict__ table, int table_len, long long max_it,
                                                       uint8_t* __restrict__ inl_all) {
  const int q = blockIdx.x, lane = threadIdx.x;
  vo_f8_ctl* ctl = ctls + q;
  if (ctl->status != VO_F8_RUN) return;
  const int* counts = counts_all + (size_t)q * F8_BATCH;
  const uint8_t* risky = risky_all + (size_t)q * F8_BATCH;
  const int N = ctl->n;
  long long n_it = ctl->n_it, n = ctl->n_done;
  double orat = ctl->orat;
  int best = ctl->best_count, best_idx = -1, consumed = -1;
  bool risky_seen = false;
  for (int base = 0; base < F8_BATCH && consumed < 0; base += 64) {
    const int c = counts[base + lane];
    const unsigned long long rmask = __ballot(risky[base + lane] != 0);
    const long long n_here = n + lane;                       // iterations counted before this lane's draw
    int cur = 0;
    for (int guard = 0; guard <= 64; ++guard) {              // (at most 64 accepts per round)
      const unsigned long long ge = cur >= 64 ? 0ull : ~((1ull << cur) - 1ull);
      const unsigned long long smask = __ballot(n_here >= n_it) & ge;    // the `while` test fails before this draw
      const unsigned long long emask = __ballot(c > best) & ge;
      const int sp = smask ? __ffsll((long long)smask) - 1 : 64;
      const int ep = emask ? __ffsll((long long)emask) - 1 : 64;
      if (sp <= ep && sp < 64) {
        consumed = base + sp;
        n += sp;
        risky_seen |= (rmask & ((1ull << sp) - 1ull)) != 0ull;
        break;
      }
      if (ep == 64) {
        n += 64;
        risky_seen |= rmask != 0ull;
        break;
      }
      best = __shfl(c, ep);
      best_idx = base + ep;
      double o = 1.0 - (double)best / (double)N;             // ransac.py:113-120
      o = fmin(fmax(o, 0.01), 0.99);
      orat = o;
      n_it = vo_state_dev::table_lookup_wave(table, table_len, max_it, o, lane);
      cur = ep + 1;
    }
  }
  bool more = false;
  if (consumed < 0) {
    if (n >= n_it) consumed = F8_BATCH;                      // the loop ends exactly behind the batch's last sample
    else more = true;
  }
  if (risky_seen) {                                          // the stream position departs from 15 per sample: the host's case
    if (lane == 0) ctl->status = VO_F8_HOST;
    return;
  }
  if (best_idx >= 0) {
    const unsigned long long* row = masks_all + ((size_t)q * F8_BATCH + best_idx) * words;
    uint8_t* inl = inl_all + (size_t)q * ln.inl;
    for (int i = lane; i < N; i += 64) inl[i] = (uint8_t)((row[i >> 6] >> (i & 63)) & 1ull);
  }
  if (lane == 0) {
    const int batch = ctl->batch;
    ctl->n_it = n_it;
    ctl->orat = orat;
    ctl->n_done = n;
    ctl->best_count = best;
    if (best_idx >= 0) ctl->best_idx = batch * F8_BATCH + best_idx;
    ctl->consumed += more ? F8_BATCH : consumed;
    ctl->batch = batch + 1;
    if (!more) ctl->status = best >= 8 ? VO_F8_DONE : VO_F8_FAILED;
  }
}

__global__ __launch_bounds__(256) void f8_unpack_mask_kernel(const unsigned long long* __restrict__ row, int n,
                                                             uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) mask[i] = (uint8_t)((row[i >> 6] >> (i & 63)) & 1ull);
}

// f8_fit_kernel over every finished lane's inliers: grid L
__global__ __launch_bounds__(256) void f8_fit_lanes_kernel(const double* __restrict__ p1, const double* __restrict__ p2,
                                                           vo_f8_lanes ln, const vo_f8_ctl* __restrict__ ctls,
                                                           const uint8_t* __restrict__ inl, int normalize,
                                                           double* __restrict__ Fout) {
  __shared__ f8_fit_lds lds;
  const int q = blockIdx.x;
  if (ctls[q].status != VO_F8_DONE) return;
  f8_fit_body(p1 + (size_t)q * ln.pts, p2 + (size_t)q * ln.pts, ctls[q].n, inl + (size_t)q * ln.inl, normalize,
              Fout + (size_t)q * ln.F, nullptr, lds);
}

// relative_pose_kernel for every finished lane: grid L; lane q's camera is entry seq[q] of the device camera table
// (K the first nine doubles of every `cam_stride`), both views through it
__global__ __launch_bounds__(256) void relative_pose_lanes_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                                  vo_f8_lanes ln, const vo_f8_ctl* __restrict__ ctls,
                                                                  const uint8_t* __restrict__ inl, const double* __restrict__ F,
                                                                  const double* __restrict__ cam, size_t cam_stride,
                                                                  const int32_t* __restrict__ seq, double* __restrict__ Mout,
                                                                  double* __restrict__ X, size_t X_stride,
                                                                  uint8_t* __restrict__ mask_out) {
  __shared__ relative_pose_lds lds;
  const int q = blockIdx.x;
  if (ctls[q].status != VO_F8_DONE) return;
  const double* K = cam + (size_t)seq[q] * cam_stride;
  const cam_pair c = {K, K};
  relative_pose_body(x1 + (size_t)q * ln.pts, x2 + (size_t)q * ln.pts, ctls[q].n, inl + (size_t)q * ln.inl, F + (size_t)q * ln.F, c,
                     Mout + (size_t)q * ln.F, X + (size_t)q * X_stride, mask_out + (size_t)q * ln.inl, nullptr, lds);
}

}  // namespace

// ---- device-resident forms (vo_internal.h): points, masks and results in HBM; the host-pointer entry points below upload,
// call these and download ----

int vo_fundamental_hypotheses_dev(vo_ctx* ctx, const double* d_p1, const double* d_p2, int N, const int32_t* samples, int Hyp,
                                  int normalize_samples, int error_kind, double threshold, int32_t* d_samples, double* d_F,
                                  int32_t* d_counts, uint64_t* d_masks, int32_t* counts) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_p1 && d_p2 && samples && d_samples && d_F && d_counts && counts, "fundamental_hypotheses: null pointer");
  VO_REQUIRE(ctx, N >= 8 && Hyp >= 1 && Hyp <= (1 << 20), "fundamental_hypotheses: need N >= 8, 1 <= Hyp <= 2^20");
  VO_REQUIRE(ctx, error_kind == 0 || error_kind == 1, "fundamental_hypotheses: error_kind must be 0 or 1");
  for (size_t k = 0; k < (size_t)8 * Hyp; ++k)
    VO_REQUIRE(ctx, samples[k] >= 0 && samples[k] < N, "fundamental_hypotheses: sample index %d out of range", (int)samples[k]);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int words = vo_cdiv(N, 64);
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(d_samples, samples, (size_t)Hyp * 32, hipMemcpyHostToDevice, st));
  {
    vo_prof_scope prof(ctx, VO_K_TWOVIEW_HYP);
    hipLaunchKernelGGL(f8_hyp_kernel, dim3(vo_cdiv(Hyp, HB)), dim3(HB), 0, st, d_p1, d_p2, N, (const int*)d_samples, Hyp,
                       normalize_samples, d_F);
  }
  VO_TRY(vo_check_launch(ctx, "f8_hyp_kernel"));
  {
    vo_prof_scope prof(ctx, VO_K_TWOVIEW_SCORE);
    hipLaunchKernelGGL(f_score_kernel, dim3(Hyp), dim3(256), 0, st, d_p1, d_p2, N, (const double*)d_F, error_kind, threshold,
                       (int*)d_counts, (unsigned long long*)d_masks, words);
  }
  VO_TRY(vo_check_launch(ctx, "f_score_kernel"));
  VO_HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, (size_t)Hyp * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->bytes_h2d += (int64_t)Hyp * 32;
  ctx->bytes_d2h += (int64_t)Hyp * 4;
  return VO_OK;
}

int vo_fundamental_fit_dev(vo_ctx* ctx, const double* d_p1, const double* d_p2, int N, const uint8_t* d_mask, int normalize,
                           double* d_F, int32_t* d_n_used) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_p1 && d_p2 && d_F, "fundamental_fit: null pointer");
  VO_REQUIRE(ctx, N >= 8, "fundamental_fit: the 8-point algorithm needs 8 correspondences");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(f8_fit_kernel, dim3(1), dim3(256), 0, ctx->stream, d_p1, d_p2, N, d_mask, normalize, d_F, (int*)d_n_used);
  return vo_check_launch(ctx, "f8_fit_kernel");
}

int vo_relative_pose_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, int N, const uint8_t* d_inliers, const double* K1,
                         const double* K2, const double* d_F, double* d_M, double* d_X, uint8_t* d_mask_out, double* d_M4) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_x1 && d_x2 && K1 && K2 && d_F && d_M && d_X, "relative_pose: null pointer");
  VO_REQUIRE(ctx, N >= 1, "relative_pose: no correspondences");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_cam2 cams;
  memcpy(cams.K1, K1, 72);
  memcpy(cams.K2, K2, 72);
  hipLaunchKernelGGL(relative_pose_kernel, dim3(1), dim3(256), 0, ctx->stream, d_x1, d_x2, N, d_inliers, d_F, cams, d_M, d_X,
                     d_mask_out, d_M4);
  return vo_check_launch(ctx, "relative_pose_kernel");
}

// ---- the 8-point RANSAC loop ----

// the threshold table of vo_ransac_build_table(confidence, 8, ...) in device memory: rebuilt when the confidence changes or
// the budget outgrows it
static int f8_table(vo_ctx* ctx, double confidence, int64_t max_it, int* table_len) {
  const int want = (int)max_it + 1;
  const int have = (int)ctx->f8_table_host.size() - 1;
  if (have < want || ctx->f8_table_conf != confidence) {
    ctx->f8_table_host.assign((size_t)want + 1, 0.0);
    vo_ransac_build_table(confidence, 8, want, ctx->f8_table_host.data());
    ctx->f8_table_conf = confidence;
    const size_t bytes = ctx->f8_table_host.size() * 8;
    VO_TRY(vo_ensure(ctx, ctx->f8_table, bytes));
    VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->f8_table.p, ctx->f8_table_host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->bytes_h2d += (int64_t)bytes;
  }
  *table_len = (int)ctx->f8_table_host.size() - 1;
  return VO_OK;
}

static int64_t f8_first_bound(const vo_f8_params& prm) {
  int64_t k0 = vo_ransac_num_iterations(prm.confidence, prm.outlier_ratio, 8);
  if (k0 < 0 || k0 > ((int64_t)1 << 62)) k0 = (int64_t)1 << 62;
  return (prm.max_iterations >= 0 && prm.max_iterations < k0) ? prm.max_iterations : k0;
}

// One lane's loop from its start by the sequential sampler on the host (vo_rng_choice), hypotheses and counts on the
// device, the rule by vo_ransac_replay: the route of a lane the device cannot finish alone.  Lane q's workspace blocks.
static int f8_host_loop(vo_ctx* ctx, const double* d_p1, const double* d_p2, int n, const vo_f8_params& prm, vo_pcg64* gen,
                        int q, int words_cap, uint8_t* d_inl, vo_f8_result* r) {
  hipStream_t st = ctx->stream;
  VO_TRY(vo_ensure(ctx, ctx->f8_samples, (size_t)F8_BATCH * 32));
  double* d_F = (double*)ctx->f8_F.p + (size_t)q * F8_BATCH * 9;
  int32_t* d_counts = (int32_t*)ctx->f8_counts.p + (size_t)q * F8_BATCH;
  uint64_t* d_masks = (uint64_t*)ctx->f8_masks.p + (size_t)q * F8_BATCH * words_cap;
  const int words = vo_cdiv(n, 64);
  vo_ransac_state rs;
  rs.outlier_ratio = prm.outlier_ratio;
  rs.confidence = prm.confidence;
  rs.max_iterations = prm.max_iterations;
  rs.s = 8;
  rs.adaptive = 1;
  rs.n_iterations = f8_first_bound(prm);
  std::vector<int32_t> samples((size_t)F8_BATCH * 8), counts((size_t)F8_BATCH);
  const std::vector<uint8_t> valid((size_t)F8_BATCH, 1);
  int64_t n_done = 0, total = 0;
  int32_t best_count = -1, best_idx = -1;
  int finished = 0;
  for (int batch = 0; !finished; ++batch) {
    vo_pcg64 spec = *gen;                // speculative copy: the generator moves by what the rule consumed
    if (vo_rng_choice(&spec, n, 8, F8_BATCH, samples.data()) != VO_OK)
      return vo_set_error(ctx, VO_EINVAL, "fundamental_ransac: cannot draw 8 of %d", n);
    VO_TRY(vo_fundamental_hypotheses_dev(ctx, d_p1, d_p2, n, samples.data(), F8_BATCH, prm.normalize_samples, prm.error_kind,
                                         prm.threshold, (int32_t*)ctx->f8_samples.p, d_F, d_counts, d_masks, counts.data()));
    const int32_t before = best_idx;
    int consumed = 0;
    if (vo_ransac_replay(&rs, valid.data(), counts.data(), F8_BATCH, n, &n_done, &best_count, &best_idx, batch * F8_BATCH,
                         &consumed, &finished) != VO_OK)
      return vo_set_error(ctx, VO_EINVAL, "fundamental_ransac: vo_ransac_replay failed");
    if (best_idx != before) {
      const int row = best_idx - batch * F8_BATCH;         // 0 .. F8_BATCH - 1: an index of this batch
      hipLaunchKernelGGL(f8_unpack_mask_kernel, dim3(vo_cdiv(n, 256)), dim3(256), 0, st,
                         (const unsigned long long*)d_masks + (size_t)row * words, n, d_inl);
      VO_TRY(vo_check_launch(ctx, "f8_unpack_mask_kernel"));
    }
    vo_rng_choice(gen, n, 8, consumed, samples.data());
    total += consumed;
  }
  r->n = n;
  r->iterations = n_done;
  r->best_count = best_count;
  r->consumed = (int32_t)total;
  r->finished_by_host = 1;
  r->status = (best_idx >= 0 && best_count >= 8) ? VO_F8_DONE : VO_F8_FAILED;
  return VO_OK;
}

int vo_fundamental_ransac_dev(vo_ctx* ctx, const double* d_p1, const double* d_p2, int n_cap, const int32_t* d_n,
                              const int32_t* n_host, const vo_f8_params& prm, vo_pcg64* rngs, uint8_t* d_inl, double* d_F,
                              const vo_f8_lanes* lanes, vo_f8_result* res) {
  if (!ctx) return VO_EINVAL;
  vo_f8_lanes ln;
  if (lanes) ln = *lanes;
  const int L = ln.L;
  VO_REQUIRE(ctx, d_p1 && d_p2 && (d_n || n_host) && rngs && d_inl && d_F && res, "fundamental_ransac: null pointer");
  VO_REQUIRE(ctx, L >= 1 && L <= 1024 && n_cap >= 1, "fundamental_ransac: need 1 <= lanes <= 1024 and a capacity");
  VO_REQUIRE(ctx, L == 1 || (ln.pts >= (size_t)2 * n_cap && ln.inl >= (size_t)n_cap && ln.F >= 9 && (!d_n || ln.n >= 1)),
             "fundamental_ransac: the lanes' blocks overlap");
  VO_REQUIRE(ctx, prm.error_kind == 0 || prm.error_kind == 1, "fundamental_ransac: error_kind must be 0 or 1");
  VO_REQUIRE(ctx, prm.outlier_ratio > 0.0 && prm.outlier_ratio < 1.0 && prm.confidence > 0.0 && prm.confidence < 1.0,
             "fundamental_ransac: outlier ratio and confidence must be inside (0, 1)");
  VO_REQUIRE(ctx, prm.max_iterations != 0, "fundamental_ransac: a budget of 0 iterations");
  for (int q = 0; q < L && !d_n; ++q)
    VO_REQUIRE(ctx, n_host[q] >= 0 && n_host[q] <= n_cap, "fundamental_ransac: %d correspondences, the capacity is %d",
               (int)n_host[q], n_cap);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // a budget the table does not hold (unbounded, or above 65536): the host's loop from the start
  const bool on_device = prm.max_iterations >= 1 && prm.max_iterations <= 65536;
  const int words = vo_cdiv(n_cap, 64);
  VO_TRY(vo_ensure(ctx, ctx->f8_ctl, (size_t)L * sizeof(vo_f8_ctl)));
  VO_TRY(vo_ensure(ctx, ctx->f8_raws, (size_t)L * F8_RAWS * 4));
  VO_TRY(vo_ensure(ctx, ctx->f8_F, (size_t)L * F8_BATCH * 72));
  VO_TRY(vo_ensure(ctx, ctx->f8_counts, (size_t)L * F8_BATCH * 4));
  VO_TRY(vo_ensure(ctx, ctx->f8_risky, (size_t)L * F8_BATCH));
  VO_TRY(vo_ensure(ctx, ctx->f8_masks, (size_t)L * F8_BATCH * words * 8));
  int table_len = 0;
  if (on_device) VO_TRY(f8_table(ctx, prm.confidence, prm.max_iterations, &table_len));
  vo_f8_ctl* d_ctl = (vo_f8_ctl*)ctx->f8_ctl.p;
  std::vector<vo_f8_ctl> h((size_t)L);
  for (int q = 0; q < L; ++q) {
    vo_f8_ctl& c = h[(size_t)q];
    memset(&c, 0, sizeof(c));
    c.rng = rngs[q];
    c.n = d_n ? -1 : n_host[q];
    c.status = on_device ? VO_F8_RUN : VO_F8_HOST;
    c.best_count = -1;
    c.best_idx = -1;
    c.n_it = f8_first_bound(prm);
    c.orat = prm.outlier_ratio;
  }
  const size_t ctl_bytes = (size_t)L * sizeof(vo_f8_ctl);
  VO_HIP_TRY(ctx, hipMemcpyAsync(d_ctl, h.data(), ctl_bytes, hipMemcpyHostToDevice, st));
  ctx->bytes_h2d += (int64_t)ctl_bytes;
  hipLaunchKernelGGL(f8_init_kernel, dim3(vo_cdiv(L, 64)), dim3(64), 0, st, d_ctl, L, d_n, ln.n, n_cap);
  VO_TRY(vo_check_launch(ctx, "f8_init_kernel"));
  // every batch moves a running lane 2048 iterations on, so the budget bounds the number of batches
  const int max_batches = on_device ? (int)(prm.max_iterations / F8_BATCH) + 1 : 0;
  bool any = on_device;                  // some lane wants a batch (before the first read-back: every lane may)
  for (int batch = 0;; ++batch) {
    if (any) {
      VO_REQUIRE(ctx, batch < max_batches, "fundamental_ransac: the loop did not end within its budget");
      hipLaunchKernelGGL(pcg64_fill_kernel, dim3(vo_cdiv(F8_RAWS / 2 + 2, 256), L), dim3(256), 0, st, (const vo_f8_ctl*)d_ctl,
                         (uint32_t*)ctx->f8_raws.p, (size_t)F8_RAWS, F8_RAWS, F8_RAWS);
      VO_TRY(vo_check_launch(ctx, "pcg64_fill_kernel"));
      hipLaunchKernelGGL(f8_hyp_raw_kernel, dim3(F8_BATCH / HB, L), dim3(HB), 0, st, d_p1, d_p2, ln, (const vo_f8_ctl*)d_ctl,
                         (const uint32_t*)ctx->f8_raws.p, prm.normalize_samples, (double*)ctx->f8_F.p, (uint8_t*)ctx->f8_risky.p);
      VO_TRY(vo_check_launch(ctx, "f8_hyp_raw_kernel"));
      hipLaunchKernelGGL(f_score_lanes_kernel, dim3(F8_BATCH, L), dim3(256), 0, st, d_p1, d_p2, ln, (const vo_f8_ctl*)d_ctl,
                         (const double*)ctx->f8_F.p, prm.error_kind, prm.threshold, (int*)ctx->f8_counts.p,
                         (unsigned long long*)ctx->f8_masks.p, words);
      VO_TRY(vo_check_launch(ctx, "f_score_lanes_kernel"));
      hipLaunchKernelGGL(f8_replay_kernel, dim3(L), dim3(64), 0, st, d_ctl, ln, (const int*)ctx->f8_counts.p,
                         (const uint8_t*)ctx->f8_risky.p, (const unsigned long long*)ctx->f8_masks.p, words,
                         (const double*)ctx->f8_table.p, table_len, (long long)prm.max_iterations, d_inl);
      VO_TRY(vo_check_launch(ctx, "f8_replay_kernel"));
    }
    // the lanes' control blocks (status words and the loop's scalars; never the counts)
    VO_HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_ctl, ctl_bytes, hipMemcpyDeviceToHost, st));
    VO_HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->bytes_d2h += (int64_t)ctl_bytes;
    if (!any) break;
    any = false;
    for (int q = 0; q < L; ++q) any |= h[(size_t)q].status == VO_F8_RUN;
    if (!any) break;
  }
  for (int q = 0; q < L; ++q) {
    vo_f8_ctl& c = h[(size_t)q];
    vo_f8_result& r = res[q];
    memset(&r, 0, sizeof(r));
    if (c.status == VO_F8_HOST) {
      VO_TRY(f8_host_loop(ctx, d_p1 + (size_t)q * ln.pts, d_p2 + (size_t)q * ln.pts, c.n, prm, &rngs[q], q, words,
                          d_inl + (size_t)q * ln.inl, &r));
      c.status = r.status;
      VO_HIP_TRY(ctx, hipMemcpyAsync(&d_ctl[q].status, &c.status, 4, hipMemcpyHostToDevice, st));
      ctx->bytes_h2d += 4;
      continue;
    }
    r.status = c.status;
    r.n = c.n;
    r.best_count = c.best_count;
    r.consumed = c.consumed;
    r.iterations = c.n_done;
    vo_rng::pcg_skip_words(&rngs[q], (uint64_t)vo_rng::CHOICE8_RAWS * (uint64_t)c.consumed);
  }
  hipLaunchKernelGGL(f8_fit_lanes_kernel, dim3(L), dim3(256), 0, st, d_p1, d_p2, ln, (const vo_f8_ctl*)d_ctl,
                     (const uint8_t*)d_inl, prm.normalize_samples, d_F);
  VO_TRY(vo_check_launch(ctx, "f8_fit_lanes_kernel"));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));      // (the status words uploaded above come from this frame's stack)
  return VO_OK;
}

int vo_relative_pose_lanes_dev(vo_ctx* ctx, const double* d_x1, const double* d_x2, const vo_f8_lanes& ln, const uint8_t* d_inl,
                               const double* d_F, const double* d_cam, size_t cam_stride, const int32_t* d_seq, double* d_M,
                               double* d_X, size_t X_stride, uint8_t* d_mask_out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, d_x1 && d_x2 && d_inl && d_F && d_cam && d_seq && d_M && d_X && d_mask_out && ln.L >= 1 && ctx->f8_ctl.p,
             "relative_pose_lanes: null pointer");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(relative_pose_lanes_kernel, dim3(ln.L), dim3(256), 0, ctx->stream, d_x1, d_x2, ln,
                     (const vo_f8_ctl*)ctx->f8_ctl.p, d_inl, d_F, d_cam, cam_stride, d_seq, d_M, d_X, X_stride, d_mask_out);
  return vo_check_launch(ctx, "relative_pose_lanes_kernel");
}

extern "C" {

int vo_fundamental_hypotheses(vo_ctx* ctx, const double* p1, const double* p2, int N, const int32_t* samples, int Hyp,
                              int normalize_samples, int error_kind, double threshold, double* F, int32_t* counts,
                              uint64_t* masks) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, p1 && p2 && samples && F && counts, "fundamental_hypotheses: null pointer");
  VO_REQUIRE(ctx, N >= 8 && Hyp >= 1 && Hyp <= (1 << 20), "fundamental_hypotheses: need N >= 8, 1 <= Hyp <= 2^20");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int words = vo_cdiv(N, 64);
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[2], (size_t)Hyp * 32));
  VO_TRY(vo_ensure(ctx, s[3], (size_t)Hyp * 72));
  VO_TRY(vo_ensure(ctx, s[4], (size_t)Hyp * 4));
  VO_TRY(vo_ensure(ctx, s[5], (size_t)Hyp * words * 8));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, p1, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, p2, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_TRY(vo_fundamental_hypotheses_dev(ctx, (const double*)s[0].p, (const double*)s[1].p, N, samples, Hyp, normalize_samples,
                                       error_kind, threshold, (int32_t*)s[2].p, (double*)s[3].p, (int32_t*)s[4].p,
                                       masks ? (uint64_t*)s[5].p : nullptr, counts));
  VO_HIP_TRY(ctx, hipMemcpyAsync(F, s[3].p, (size_t)Hyp * 72, hipMemcpyDeviceToHost, st));
  if (masks) VO_HIP_TRY(ctx, hipMemcpyAsync(masks, s[5].p, (size_t)Hyp * words * 8, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_fundamental_fit(vo_ctx* ctx, const double* p1, const double* p2, int N, const uint8_t* mask, int normalize,
                       double* F) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, p1 && p2 && F, "fundamental_fit: null pointer");
  VO_REQUIRE(ctx, N >= 8, "fundamental_fit: the 8-point algorithm needs 8 correspondences");
  if (mask) {
    int n = 0;
    for (int i = 0; i < N; ++i) n += mask[i] ? 1 : 0;
    VO_REQUIRE(ctx, n >= 8, "fundamental_fit: only %d correspondences are selected", n);
  }
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[2], (size_t)N));
  VO_TRY(vo_ensure(ctx, s[3], 128));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, p1, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, p2, (size_t)N * 16, hipMemcpyHostToDevice, st));
  if (mask) VO_HIP_TRY(ctx, hipMemcpyAsync(s[2].p, mask, (size_t)N, hipMemcpyHostToDevice, st));
  VO_TRY(vo_fundamental_fit_dev(ctx, (const double*)s[0].p, (const double*)s[1].p, N, mask ? (const uint8_t*)s[2].p : nullptr,
                                normalize, (double*)s[3].p, nullptr));
  VO_HIP_TRY(ctx, hipMemcpyAsync(F, s[3].p, 72, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_essential_decompose(vo_ctx* ctx, const double* E, double* M4) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, E && M4, "essential_decompose: null pointer");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], 512));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, E, 72, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(essential_decompose_kernel, dim3(1), dim3(64), 0, st, (const double*)s[0].p, (double*)s[0].p + 16);
  VO_TRY(vo_check_launch(ctx, "essential_decompose_kernel"));
  VO_HIP_TRY(ctx, hipMemcpyAsync(M4, (double*)s[0].p + 16, 48 * 8, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_relative_pose(vo_ctx* ctx, const double* x1, const double* x2, int N, const uint8_t* inliers, const double* K1,
                     const double* K2, const double* F, double* M, double* X, uint8_t* mask_out, double* M4) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, x1 && x2 && K1 && K2 && F && M && X, "relative_pose: null pointer");
  VO_REQUIRE(ctx, N >= 1, "relative_pose: no correspondences");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[2], (size_t)N));
  VO_TRY(vo_ensure(ctx, s[3], 1024));
  VO_TRY(vo_ensure(ctx, s[4], (size_t)N * 24));
  VO_TRY(vo_ensure(ctx, s[5], (size_t)N));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, x1, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, x2, (size_t)N * 16, hipMemcpyHostToDevice, st));
  if (inliers) VO_HIP_TRY(ctx, hipMemcpyAsync(s[2].p, inliers, (size_t)N, hipMemcpyHostToDevice, st));
  double* dF = (double*)s[3].p;
  VO_HIP_TRY(ctx, hipMemcpyAsync(dF, F, 72, hipMemcpyHostToDevice, st));
  VO_TRY(vo_relative_pose_dev(ctx, (const double*)s[0].p, (const double*)s[1].p, N, inliers ? (const uint8_t*)s[2].p : nullptr,
                              K1, K2, dF, dF + 16, (double*)s[4].p, (uint8_t*)s[5].p, dF + 32));
  VO_HIP_TRY(ctx, hipMemcpyAsync(M, dF + 16, 96, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(X, s[4].p, (size_t)N * 24, hipMemcpyDeviceToHost, st));
  if (mask_out) VO_HIP_TRY(ctx, hipMemcpyAsync(mask_out, s[5].p, (size_t)N, hipMemcpyDeviceToHost, st));
  if (M4) VO_HIP_TRY(ctx, hipMemcpyAsync(M4, dF + 32, 48 * 8, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_fundamental_ransac(vo_ctx* ctx, const double* p1, const double* p2, int N, int normalize_samples, int error_kind,
                          double threshold, double outlier_ratio, double confidence, int64_t max_iterations, vo_pcg64* rng,
                          double* F, uint8_t* inlier_mask, int64_t* iterations, int32_t* best_count, int32_t* finished_by_host) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, p1 && p2 && rng && F && inlier_mask, "fundamental_ransac: null pointer");
  VO_REQUIRE(ctx, N >= 8, "fundamental_ransac: the 8-point algorithm needs 8 correspondences");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, s[2], (size_t)N));
  VO_TRY(vo_ensure(ctx, s[3], 128));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, p1, (size_t)N * 16, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, p2, (size_t)N * 16, hipMemcpyHostToDevice, st));
  vo_f8_params prm;
  prm.normalize_samples = normalize_samples ? 1 : 0;
  prm.error_kind = error_kind;
  prm.threshold = threshold;
  prm.outlier_ratio = outlier_ratio;
  prm.confidence = confidence;
  prm.max_iterations = max_iterations;
  const int32_t n = N;
  vo_f8_result r;
  VO_TRY(vo_fundamental_ransac_dev(ctx, (const double*)s[0].p, (const double*)s[1].p, N, nullptr, &n, prm, rng,
                                   (uint8_t*)s[2].p, (double*)s[3].p, nullptr, &r));
  if (iterations) *iterations = r.iterations;
  if (best_count) *best_count = r.best_count;
  if (finished_by_host) *finished_by_host = r.finished_by_host;
  if (r.status != VO_F8_DONE)
    return vo_set_error(ctx, VO_ETRACKING, "fundamental_ransac: no model with 8 inliers among %d correspondences (best: %d)", N,
                        (int)r.best_count);
  VO_HIP_TRY(ctx, hipMemcpyAsync(F, s[3].p, 72, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(inlier_mask, s[2].p, (size_t)N, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_rng_raw32_device(vo_ctx* ctx, vo_pcg64* rng, int count, uint32_t* out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, rng && out && count >= 0 && count <= (1 << 24), "rng_raw32_device: need a state and 0 <= count <= 2^24");
  if (count == 0) return VO_OK;
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  VO_TRY(vo_ensure(ctx, ctx->f8_ctl, sizeof(vo_f8_ctl)));
  VO_TRY(vo_ensure(ctx, ctx->f8_raws, (size_t)count * 4));
  hipStream_t st = ctx->stream;
  vo_f8_ctl c;
  memset(&c, 0, sizeof(c));
  c.rng = *rng;
  c.status = VO_F8_RUN;
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->f8_ctl.p, &c, sizeof(c), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pcg64_fill_kernel, dim3(vo_cdiv(count / 2 + 2, 256), 1), dim3(256), 0, st, (const vo_f8_ctl*)ctx->f8_ctl.p,
                     (uint32_t*)ctx->f8_raws.p, (size_t)0, count, 0);
  VO_TRY(vo_check_launch(ctx, "pcg64_fill_kernel"));
  VO_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->f8_raws.p, (size_t)count * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  vo_rng::pcg_skip_words(rng, (uint64_t)count);
  return VO_OK;
}

}  // extern "C"
