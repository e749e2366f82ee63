// The scorer of a fundamental matrix against every correspondence, shared by the 8-point hypotheses (bootstrap.hip) and the
// five-point hypotheses (essential5.hip): one arithmetic, one operation order, strict `<`, ballot words to counts and mask rows.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace vo_fscore {

// error of one correspondence under F.  kind 0: (p2^T F p1)^2 in NumPy's order ((p2^T F) p1, triangulation.py:140-145);
// kind 1: max of the squared distances to the epipolar lines in both images
__device__ __forceinline__ double f_error(const double* F, double x1, double y1, double x2, double y2, int kind) {
  if (kind == 0) {
    const double t0 = x2 * F[0] + y2 * F[3] + F[6];
    const double t1 = x2 * F[1] + y2 * F[4] + F[7];
    const double t2 = x2 * F[2] + y2 * F[5] + F[8];
    const double r = t0 * x1 + t1 * y1 + t2;
    return r * r;
  }
  const double l2x = F[0] * x1 + F[1] * y1 + F[2], l2y = F[3] * x1 + F[4] * y1 + F[5], l2z = F[6] * x1 + F[7] * y1 + F[8];
  const double l1x = F[0] * x2 + F[3] * y2 + F[6], l1y = F[1] * x2 + F[4] * y2 + F[7];
  const double e = x2 * l2x + y2 * l2y + l2z;
  const double num = e * e;
  const double d2 = num / (l2x * l2x + l2y * l2y), d1 = num / (l1x * l1x + l1y * l1y);
  return d1 > d2 ? d1 : d2;                  // (np.maximum)
}

// grid.x = hypothesis; one workgroup walks the correspondences: count + mask row (words 64-bit words per row)
__device__ __forceinline__ void f_score_body(const double* __restrict__ p1, const double* __restrict__ p2, int N,
                                             const double* __restrict__ Fs, int kind, double thr, int* __restrict__ counts,
                                             unsigned long long* __restrict__ masks, int words, int* s_cnt /*[4]*/) {
  const int h = blockIdx.x, tid = threadIdx.x;
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = Fs[(size_t)9 * h + k];
  int cnt = 0;
  for (int base = 0; base < N; base += 256) {
    const int i = base + tid;
    bool in = false;
    if (i < N) in = f_error(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1], kind) < thr;
    const unsigned long long b = __ballot(in);
    if ((tid & 63) == 0) {
      if (masks && (base + tid) / 64 < words) masks[(size_t)h * words + (base + tid) / 64] = b;
      cnt += __popcll(b);
    }
  }
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) counts[h] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

}  // namespace vo_fscore
