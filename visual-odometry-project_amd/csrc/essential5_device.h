// The five-point essential-matrix solver of one RANSAC sample (include/vo_hip.h, "calibrated two-view bootstrap"; Nister
// 2004), one work item per sample.  Every stage is the one tests/essential5_reference.py defines in NumPy:
//
//   null space   Householder QR of the transposed 5x9 system (rows kron(x^1, x^2), triangulation.py:203-205); the last four
//                columns of the orthogonal factor are X, Y, Z, W with E = x X + y Y + z Z + W, E[b][a] = e[3a + b]
//   constraints  det E = 0 and 2 E E^T E - tr(E E^T) E = 0 over the 20 monomials of (x, y, z), Nister's column order
//   eliminate    Gauss-Jordan with partial pivoting on the 10x20 matrix, which lives in the work item's `work` block
//   polynomial   rows e..j give B(z) (x, y, 1)^T = 0; det B(z), degree 10
//   roots        isolated between the roots of the derivative (from the ninth derivative down, inside the Cauchy bound),
//                E5_ISO_STEPS bisection steps on a derivative, E5_BIS_STEPS + E5_NEWTON_STEPS safeguarded Newton steps on
//                the polynomial: fixed counts, so a sample's result is a function of the sample alone
//   back-subst.  (x, y, 1) from the cross product of the two rows of B(z) with the largest third component
//   output       unit Frobenius norm, the entry of largest magnitude positive (the first in row-major order on ties),
//                ascending z; a non-finite candidate is dropped
//
// A sample has no solution (n_sol = 0) when a Householder column norm falls below E5_RANK_TOL of the largest (the null space
// is not four-dimensional: a repeated correspondence), when an elimination pivot falls below E5_PIVOT_TOL of the matrix's
// largest entry, or when the leading coefficient falls below E5_LEAD_TOL of the largest coefficient.
//
// `work` holds E5_WORK doubles per work item, element e at work[e * STRIDE] (LDS, [element][lane]); the matrix first, the
// polynomial, the level's derivative and the two root lists afterwards.  fp64, no contraction.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define E5_HD __host__ __device__ __forceinline__
#else
#define E5_HD inline
#endif

#pragma clang fp contract(off)

namespace vo_e5 {

constexpr int E5_WORK = 200;
constexpr double E5_RANK_TOL = 1e-10;
constexpr double E5_PIVOT_TOL = 1e-12;
constexpr double E5_LEAD_TOL = 1e-13;
constexpr int E5_ISO_STEPS = 40;
constexpr int E5_BIS_STEPS = 64;
constexpr int E5_NEWTON_STEPS = 4;

// monomials over (x, y, z, 1) = (0, 1, 2, 3): the pair (a <= b) -> 0..9; the sorted triple -> Nister's column
E5_HD constexpr int pair_index(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * 4 - lo * (lo - 1) / 2 + (hi - lo);
}
E5_HD constexpr int pair_lo(int p) { return p < 4 ? 0 : (p < 7 ? 1 : (p < 9 ? 2 : 3)); }
E5_HD constexpr int pair_hi(int p) { return p < 4 ? p : (p < 7 ? p - 3 : (p < 9 ? p - 5 : 3)); }
E5_HD constexpr int triple_column(int a, int b, int c) {          // a <= b <= c
  const int key = 16 * a + 4 * b + c;
  return key == 0 ? 0 : key == 21 ? 1 : key == 1 ? 2 : key == 5 ? 3 : key == 2 ? 4 : key == 3 ? 5 : key == 22 ? 6
       : key == 23 ? 7 : key == 6 ? 8 : key == 7 ? 9 : key == 10 ? 10 : key == 11 ? 11 : key == 15 ? 12 : key == 26 ? 13
       : key == 27 ? 14 : key == 31 ? 15 : key == 42 ? 16 : key == 43 ? 17 : key == 47 ? 18 : 19;
}
E5_HD constexpr int mono_column(int p, int c) {                    // pair p times variable c
  const int a = pair_lo(p), b = pair_hi(p);
  return c <= a ? triple_column(c, a, b) : (c <= b ? triple_column(a, c, b) : triple_column(a, b, c));
}

E5_HD void mul11(const double* p, const double* q, double* out /*10*/) {
#pragma unroll
  for (int k = 0; k < 10; ++k) out[k] = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) out[pair_index(a, b)] += p[a] * q[b];
}

E5_HD void mul21(const double* p, const double* q, double* out /*20*/) {
#pragma unroll
  for (int k = 0; k < 20; ++k) out[k] = 0.0;
#pragma unroll
  for (int a = 0; a < 10; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) out[mono_column(a, b)] += p[a] * q[b];
}

// stage 2: the null-space basis (4 x 9) of the sample's 5x9 system; false when it is not four-dimensional
E5_HD bool null_space(const double (&h1)[5][3], const double (&h2)[5][3], double (&basis)[4][9]) {
  double A[9][5];
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) A[3 * a + b][k] = h1[k][a] * h2[k][b];
  double vv[5], dmin = 0.0, dmax = 0.0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) s += A[r][k] * A[r][k];
    const double nrm = sqrt(s);
    if (!(nrm > 0.0) || !(nrm < INFINITY)) ok = false;
    dmin = (k == 0 || nrm < dmin) ? nrm : dmin;
    dmax = (k == 0 || nrm > dmax) ? nrm : dmax;
    const double alpha = A[k][k] >= 0.0 ? -nrm : nrm;
    A[k][k] = A[k][k] - alpha;                          // v = x - alpha e_k, kept in the column
    double w = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) w += A[r][k] * A[r][k];
    vv[k] = w;
#pragma unroll
    for (int c = k + 1; c < 5; ++c) {
      double d = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) d += A[r][k] * A[r][c];
      const double f = 2.0 * d / w;
#pragma unroll
      for (int r = k; r < 9; ++r) A[r][c] = A[r][c] - f * A[r][k];
    }
  }
  if (!ok || !(dmin > E5_RANK_TOL * dmax)) return false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double b[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) b[r] = r == 5 + j ? 1.0 : 0.0;
#pragma unroll
    for (int k = 4; k >= 0; --k) {
      double d = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) d += A[r][k] * b[r];
      const double f = 2.0 * d / vv[k];
#pragma unroll
      for (int r = k; r < 9; ++r) b[r] = b[r] - f * A[r][k];
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) basis[j][r] = b[r];
  }
  return true;
}

// stage 3: the 10x20 matrix into work (row r, column c at work[(20 r + c) STRIDE])
template <int STRIDE>
E5_HD void constraint_matrix(const double (&basis)[4][9], double* work) {
  double Ep[3][3][4];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) Ep[r][c][v] = basis[v][3 * c + r];
  {
    double row[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) row[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {                       // cofactors of row 0: columns (c0, c1) of rows 1, 2
      const int c0 = j == 0 ? 1 : 0, c1 = j == 2 ? 1 : 2;
      double m0[10], m1[10], t[20];
      mul11(Ep[1][c0], Ep[2][c1], m0);
      mul11(Ep[1][c1], Ep[2][c0], m1);
#pragma unroll
      for (int k = 0; k < 10; ++k) m0[k] = m0[k] - m1[k];
      mul21(m0, Ep[0][j], t);
#pragma unroll
      for (int k = 0; k < 20; ++k) row[k] = j == 1 ? row[k] - t[k] : row[k] + t[k];
    }
#pragma unroll
    for (int k = 0; k < 20; ++k) work[k * STRIDE] = row[k];
  }
  double L[3][3][10];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      double a[10], b[10], c[10];
      mul11(Ep[i][0], Ep[j][0], a);
      mul11(Ep[i][1], Ep[j][1], b);
      mul11(Ep[i][2], Ep[j][2], c);
#pragma unroll
      for (int k = 0; k < 10; ++k) L[i][j][k] = (a[k] + b[k]) + c[k];
    }
  double t[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) t[k] = (L[0][0][k] + L[1][1][k]) + L[2][2][k];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        const double g2 = 2.0 * L[i][j][k];
        L[i][j][k] = i == j ? g2 - t[k] : g2;
        if (i != j) L[j][i][k] = g2;
      }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double a[20], b[20], c[20];
      mul21(L[i][0], Ep[0][j], a);
      mul21(L[i][1], Ep[1][j], b);
      mul21(L[i][2], Ep[2][j], c);
#pragma unroll
      for (int k = 0; k < 20; ++k) work[(20 * (1 + 3 * i + j) + k) * STRIDE] = (a[k] + b[k]) + c[k];
    }
}

// stage 4: Gauss-Jordan on the first ten columns, partial pivoting
template <int STRIDE>
E5_HD bool eliminate(double* work) {
  double big = 0.0;
  for (int e = 0; e < 200; ++e) {
    const double v = fabs(work[e * STRIDE]);
    big = (v > big || v != v) ? v : big;               // (a NaN sticks)
  }
  if (!(big > 0.0) || !(big < INFINITY)) return false;
  for (int c = 0; c < 10; ++c) {
    int p = c;
    double best = fabs(work[(20 * c + c) * STRIDE]);
    for (int r = c + 1; r < 10; ++r) {
      const double v = fabs(work[(20 * r + c) * STRIDE]);
      if (v > best) {
        best = v;
        p = r;
      }
    }
    if (!(best > E5_PIVOT_TOL * big)) return false;
    if (p != c)
      for (int k = c; k < 20; ++k) {
        const double a = work[(20 * c + k) * STRIDE];
        work[(20 * c + k) * STRIDE] = work[(20 * p + k) * STRIDE];
        work[(20 * p + k) * STRIDE] = a;
      }
    const double piv = work[(20 * c + c) * STRIDE];
    for (int k = c; k < 20; ++k) work[(20 * c + k) * STRIDE] = work[(20 * c + k) * STRIDE] / piv;
    for (int r = 0; r < 10; ++r) {
      if (r == c) continue;
      const double f = work[(20 * r + c) * STRIDE];
      for (int k = c; k < 20; ++k)
        work[(20 * r + k) * STRIDE] = work[(20 * r + k) * STRIDE] - f * work[(20 * c + k) * STRIDE];
    }
  }
  return true;
}

// stage 5: B (entries 0, 1: degree 3; entry 2: degree 4; ascending powers) and det B(z)
template <int STRIDE>
E5_HD void b_matrix(const double* work, double (&B)[3][3][5]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double e[10], f[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      e[k] = work[(20 * (4 + 2 * i) + 10 + k) * STRIDE];
      f[k] = work[(20 * (5 + 2 * i) + 10 + k) * STRIDE];
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int o = 3 * v;
      B[i][v][0] = e[o + 2];
      B[i][v][1] = e[o + 1] - f[o + 2];
      B[i][v][2] = e[o] - f[o + 1];
      B[i][v][3] = -f[o];
      B[i][v][4] = 0.0;
    }
    B[i][2][0] = e[9];
    B[i][2][1] = e[8] - f[9];
    B[i][2][2] = e[7] - f[8];
    B[i][2][3] = e[6] - f[7];
    B[i][2][4] = -f[6];
  }
}

template <int NP, int NQ, int NO>
E5_HD void pmul(const double* p, const double* q, double* out) {
#pragma unroll
  for (int k = 0; k < NO; ++k) out[k] = 0.0;
#pragma unroll
  for (int a = 0; a < NP; ++a)
#pragma unroll
    for (int b = 0; b < NQ; ++b) out[a + b] += p[a] * q[b];
}

E5_HD void det_polynomial(const double (&B)[3][3][5], double (&c)[11]) {
  double acc[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) acc[k] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {                          // along the third column: minors of the rows (r0, r1)
    const int r0 = i == 0 ? 1 : 0, r1 = i == 2 ? 1 : 2;
    double m0[7], m1[7], t[11];
    pmul<4, 4, 7>(B[r0][0], B[r1][1], m0);
    pmul<4, 4, 7>(B[r0][1], B[r1][0], m1);
#pragma unroll
    for (int k = 0; k < 7; ++k) m0[k] = m0[k] - m1[k];
    pmul<5, 7, 11>(B[i][2], m0, t);
#pragma unroll
    for (int k = 0; k < 11; ++k) acc[k] = i == 1 ? acc[k] - t[k] : acc[k] + t[k];
  }
#pragma unroll
  for (int k = 0; k < 11; ++k) c[k] = acc[k];
}

template <int STRIDE>
E5_HD double horner(const double* q, int n, double z) {
  double v = q[n * STRIDE];
  for (int k = n - 1; k >= 0; --k) v = v * z + q[k * STRIDE];
  return v;
}

// stage 6: the real roots, ascending, into roots[k * STRIDE]; work slots: c at 0, q at 11, the lists at 22 and 33
template <int STRIDE>
E5_HD int real_roots(const double (&c_in)[11], double* work, double** roots_out) {
  double* c = work;
  double* q = work + 11 * STRIDE;
  double* ra = work + 22 * STRIDE;
  double* rb = work + 33 * STRIDE;
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    const double v = fabs(c_in[k]);
    m = (v > m || v != v) ? v : m;
  }
  if (!(m > 0.0) || !(m < INFINITY)) return -1;
#pragma unroll
  for (int k = 0; k < 11; ++k) c[k * STRIDE] = c_in[k] / m;
  const double lead = c_in[10] / m;
  if (!(fabs(lead) > E5_LEAD_TOL)) return -1;
  double bound = 0.0;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const double v = fabs((c_in[k] / m) / lead);
    bound = v > bound ? v : bound;
  }
  bound = 1.0 + bound;
  if (!(bound < INFINITY)) return -1;
  int count = 0;                                         // roots of the level above, in ra
  for (int level = 9; level >= 0; --level) {
    const int n = 10 - level;
    for (int i = 0; i <= n; ++i) {
      double f = 1.0;
      for (int j = 0; j < level; ++j) f = f * (double)(i + level - j);
      q[i * STRIDE] = c[(i + level) * STRIDE] * f;
    }
    const int steps = level == 0 ? E5_BIS_STEPS : E5_ISO_STEPS;
    int found = 0;
    double lo0 = -bound;
    bool slo0 = horner<STRIDE>(q, n, lo0) < 0.0;
    for (int s = 0; s <= count; ++s) {
      const double hi0 = s < count ? ra[s * STRIDE] : bound;
      const bool shi0 = horner<STRIDE>(q, n, hi0) < 0.0;
      if (slo0 != shi0) {
        double lo = lo0, hi = hi0;
        for (int it = 0; it < steps; ++it) {
          const double mid = 0.5 * (lo + hi);
          if ((horner<STRIDE>(q, n, mid) < 0.0) == slo0) lo = mid;
          else hi = mid;
        }
        double z = 0.5 * (lo + hi);
        if (level == 0) {
          for (int it = 0; it < E5_NEWTON_STEPS; ++it) {
            double v = q[n * STRIDE], d = 0.0;
            for (int k = n - 1; k >= 0; --k) {
              d = d * z + v;
              v = v * z + q[k * STRIDE];
            }
            const double zn = d != 0.0 ? z - v / d : z;
            if (zn >= lo && zn <= hi) z = zn;
          }
        }
        rb[found * STRIDE] = z;
        ++found;
      }
      lo0 = hi0;
      slo0 = shi0;
    }
    double* t = ra;
    ra = rb;
    rb = t;
    count = found;
  }
  *roots_out = ra;
  return count;
}

// stages 7 and 8 for one root: E (row-major) into out[9]; false when it is not finite
E5_HD bool back_substitute(const double (&B)[3][3][5], const double (&basis)[4][9], double z, double* out) {
  double Bz[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      double s = B[i][v][4];
#pragma unroll
      for (int k = 3; k >= 0; --k) s = s * z + B[i][v][k];
      Bz[i][v] = s;
    }
  double bu = 0.0, bv = 0.0, bw = 0.0;
#pragma unroll
  for (int pr = 0; pr < 3; ++pr) {
    const int r0 = pr == 2 ? 1 : 0, r1 = pr == 0 ? 1 : 2;
    const double u = Bz[r0][1] * Bz[r1][2] - Bz[r0][2] * Bz[r1][1];
    const double v = Bz[r0][2] * Bz[r1][0] - Bz[r0][0] * Bz[r1][2];
    const double w = Bz[r0][0] * Bz[r1][1] - Bz[r0][1] * Bz[r1][0];
    if (pr == 0 || fabs(w) > fabs(bw)) {
      bu = u;
      bv = v;
      bw = w;
    }
  }
  if (!(fabs(bw) > 0.0)) return false;
  const double x = bu / bw, y = bv / bw;
  double e[9], s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    e[k] = ((x * basis[0][k] + y * basis[1][k]) + z * basis[2][k]) + basis[3][k];
    s += e[k] * e[k];
  }
  const double nrm = sqrt(s);
  if (!(nrm > 0.0) || !(nrm < INFINITY)) return false;
  double E[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[3 * r + c] = e[3 * c + r] / nrm;
  double big = E[0];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (fabs(E[k]) > fabs(big)) big = E[k];
    if (!(fabs(E[k]) < INFINITY)) finite = false;
  }
  if (!finite) return false;
  const double sg = big < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = sg * E[k];
  return true;
}

// one sample: normalised points in, n_sol out, E[10][9] (row-major; rows beyond n_sol zero) at Eout
template <int STRIDE>
E5_HD int solve(const double (&h1)[5][3], const double (&h2)[5][3], double* work, double* Eout) {
  for (int k = 0; k < 90; ++k) Eout[k] = 0.0;
  double basis[4][9];
  if (!null_space(h1, h2, basis)) return 0;
  constraint_matrix<STRIDE>(basis, work);
  if (!eliminate<STRIDE>(work)) return 0;
  double B[3][3][5], c[11];
  b_matrix<STRIDE>(work, B);
  det_polynomial(B, c);
  double* roots = nullptr;
  const int nr = real_roots<STRIDE>(c, work, &roots);
  int n = 0;
  for (int k = 0; k < nr; ++k)
    if (back_substitute(B, basis, roots[k * STRIDE], Eout + 9 * n)) ++n;
  return n;
}

}  // namespace vo_e5
