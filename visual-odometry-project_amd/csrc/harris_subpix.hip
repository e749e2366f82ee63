// Harris corners with sub-pixel refinement for gfx950: the second branch of KLTTracker.find_corners.
//
// Reference call site: src/vo/features/klt.py:99-112
//   dst = cv2.cornerHarris(img, 2, 3, 0.04); dst = cv2.dilate(dst, None)
//   ret, dst = cv2.threshold(dst, 0.01 * dst.max(), 255, 0)
//   ret, labels, stats, centroids = cv2.connectedComponentsWithStats(np.uint8(dst))
//   points = cv2.cornerSubPix(img, np.float32(centroids), (5, 5), (-1, -1), (EPS | MAX_ITER, 100, 0.001))
// The definition is restated in tests/harris_subpix_oracle.py.  S images of one size per set of launches (the image is the
// grid's extra dimension), a kernel boundary between the stages:
//   response   Harris map (Sobel and box sums as integers, the formula in double) + one maximum per image
//   init       per 2x2 block: dilate + threshold of its pixels (a 4-bit code), union-find parent = itself when any is set
//   merge      union with the already-scanned neighbour blocks (left, up-left, up, up-right); a root is the smallest
//              block index of its component, i.e. its first 2x2 block in row-major block order -- OpenCV's label order
//   flatten    parent = root; a flag at every root
//   scan       exclusive sum of the flags over all images (rocPRIM): label = rank of the root + 1
//   stats      per-label area and coordinate sums as 64-bit integers, summed in LDS before the global atomics
//   subpix     one wavefront per row (background included): centroid, then cornerSubPix's iteration
#include <cfloat>
#include <cmath>

#include "vo_internal.h"

#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int GX = 64, GY = 16, GT = 256;     // response tiles
constexpr int BT = 256;                        // block kernels
constexpr int HS_WIN_MAX = 15;                 // cornerSubPix half-window at most
constexpr int HS_BUF_MAX = (2 * HS_WIN_MAX + 3) * (2 * HS_WIN_MAX + 3);
constexpr int HT = 512;                        // stats: LDS table slots per workgroup (>= 2 x the labels it can see)

struct hs_weights {                            // cornerSubPix's window weights, mask[i][j] = vy[i] * ex[j] (float)
  float vy[2 * HS_WIN_MAX + 1];
  float ex[2 * HS_WIN_MAX + 1];
};

__device__ __forceinline__ int refl(int c, int n) {
  if (n == 1) return 0;
  while (c < 0 || c >= n) c = c < 0 ? -c : 2 * (n - 1) - c;
  return c;
}

__device__ __forceinline__ unsigned float_key(float f) {   // monotone float -> unsigned (0 is below every float)
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// cornerHarris(img, block, 3, k) for one 64 x 16 tile; grid.z = image
__global__ __launch_bounds__(GT) void hs_response_kernel(const uint8_t* __restrict__ imgs, size_t img_stride, int H, int W,
                                                         int block, float s2, double k, float* __restrict__ resp,
                                                         unsigned* __restrict__ max_key) {
  extern __shared__ __align__(16) int s_g[];                 // gradient region, packed (gx | gy << 16)
  __shared__ unsigned s_max;
  const int r0 = block / 2;
  const int RW = GX + block - 1, RH = GY + block - 1;
  int* s_hxx = s_g + RW * RH;                                // horizontal sums: RH x GX
  int* s_hxy = s_hxx + RH * GX;
  int* s_hyy = s_hxy + RH * GX;
  const int tid = threadIdx.x, z = blockIdx.z;
  const uint8_t* img = imgs + (size_t)z * img_stride;
  float* out = resp + (size_t)z * H * W;
  const int x0 = blockIdx.x * GX, y0 = blockIdx.y * GY;
  if (tid == 0) s_max = 0;
  for (int i = tid; i < RW * RH; i += GT) {
    const int ly = i / RW, lx = i - ly * RW;
    const int y = refl(y0 + ly - r0, H), x = refl(x0 + lx - r0, W);   // box border: reflect the product image
    const int ym = refl(y - 1, H), yp = refl(y + 1, H), xm = refl(x - 1, W), xp = refl(x + 1, W);
    const uint8_t* rm = img + (size_t)ym * W;
    const uint8_t* rc = img + (size_t)y * W;
    const uint8_t* rp = img + (size_t)yp * W;
    const int p00 = rm[xm], p01 = rm[x], p02 = rm[xp], p10 = rc[xm], p12 = rc[xp], p20 = rp[xm], p21 = rp[x],
              p22 = rp[xp];
    const int gx = (p02 - p00) + 2 * (p12 - p10) + (p22 - p20);
    const int gy = (p20 - p00) + 2 * (p21 - p01) + (p22 - p02);
    s_g[i] = (gx & 0xffff) | (gy << 16);
  }
  __syncthreads();
  for (int i = tid; i < RH * GX; i += GT) {
    const int ly = i / GX, lx = i - ly * GX;
    const int* g = s_g + ly * RW + lx;
    int sxx = 0, sxy = 0, syy = 0;                           // |g| <= 1020, block <= 31: below 2^31
    for (int q = 0; q < block; ++q) {
      const int v = g[q];
      const int a = (int)(short)(v & 0xffff), b = v >> 16;
      sxx += a * a;
      sxy += a * b;
      syy += b * b;
    }
    s_hxx[i] = sxx;
    s_hxy[i] = sxy;
    s_hyy[i] = syy;
  }
  __syncthreads();
  const int lx = tid & (GX - 1);
  unsigned local = 0;
  for (int ly = tid / GX; ly < GY; ly += GT / GX) {
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    long long sxx = 0, sxy = 0, syy = 0;
    for (int q = 0; q < block; ++q) {
      const int j = (ly + q) * GX + lx;
      sxx += s_hxx[j];
      sxy += s_hxy[j];
      syy += s_hyy[j];
    }
    const float a = (float)sxx * s2, b = (float)sxy * s2, c = (float)syy * s2;
    const double A = a, B = b, C = c;
    const float r = (float)(A * C - B * B - k * (A + C) * (A + C));
    out[(size_t)y * W + x] = r;
    local = max(local, float_key(r));
  }
  if (local) atomicMax(&s_max, local);
  __syncthreads();
  if (tid == 0 && s_max) atomicMax(max_key + z, s_max);
}

// One work item per 2x2 block: dilate + threshold of its (up to) four pixels -> code (bit 0 top-left, 1 top-right,
// 2 bottom-left, 3 bottom-right), parent = itself when any is foreground, else -1; clears the image's stats rows.
__global__ __launch_bounds__(BT) void hs_init_kernel(const float* __restrict__ resp, int H, int W, int BW, int nb,
                                                     const unsigned* __restrict__ max_key, double rel,
                                                     uint8_t* __restrict__ code, int* __restrict__ parent,
                                                     unsigned long long* __restrict__ stats) {
  const int b = blockIdx.x * BT + threadIdx.x, z = blockIdx.y;
  if (b >= nb) return;
  const float* R = resp + (size_t)z * H * W;
  const float t = (float)(rel * (double)key_float(max_key[z]));
  const int by = b / BW, bx = b - by * BW;
  float m[4][4];                                             // rows 2by-1 .. 2by+2, columns 2bx-1 .. 2bx+2
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = 2 * by - 1 + j, x = 2 * bx - 1 + i;
      m[j][i] = (y >= 0 && y < H && x >= 0 && x < W) ? R[(size_t)y * W + x] : -INFINITY;
    }
  unsigned c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dy = q >> 1, dx = q & 1;
    if (2 * by + dy >= H || 2 * bx + dx >= W) continue;
    float d = -INFINITY;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) d = fmaxf(d, m[dy + j][dx + i]);
    if (d > t) c |= 1u << q;
  }
  const size_t o = (size_t)z * nb + b;
  code[o] = (uint8_t)c;
  parent[o] = c ? b : -1;
  unsigned long long* st = stats + ((size_t)z * (nb + 1) + b + 1) * 3;
  st[0] = st[1] = st[2] = 0ull;
  if (b == 0) stats[(size_t)z * (nb + 1) * 3] = stats[(size_t)z * (nb + 1) * 3 + 1] = stats[(size_t)z * (nb + 1) * 3 + 2] = 0ull;
}

// (agent-scope loads: parents are lowered by other workgroups' atomics during the merge)
__device__ __forceinline__ int hs_find(int* P, int x, int bound) {
  for (int n = 0; n < bound; ++n) {
    const int p = __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
  return x;
}

// Parents only decrease, so every retry lowers a or b: the loop ends within 2 nb rounds (the bound is a guard).
__device__ __forceinline__ void hs_union(int* P, int a, int b, int nb, unsigned* fault) {
  for (int n = 0; n < 2 * nb + 2; ++n) {
    a = hs_find(P, a, nb);
    b = hs_find(P, b, nb);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(P + hi, lo);
    if (old == hi) return;
    if (a > b) a = old; else b = old;
  }
  atomicOr(fault, 1u);
}

__global__ __launch_bounds__(BT) void hs_merge_kernel(const uint8_t* __restrict__ code, int* __restrict__ parent, int BW,
                                                      int nb, unsigned* __restrict__ fault) {
  const int b = blockIdx.x * BT + threadIdx.x, z = blockIdx.y;
  if (b >= nb) return;
  const uint8_t* C = code + (size_t)z * nb;
  int* P = parent + (size_t)z * nb;
  const unsigned c = C[b];
  if (!c) return;
  const int by = b / BW, bx = b - by * BW;
  if (bx > 0 && (c & 5u) && (C[b - 1] & 10u)) hs_union(P, b, b - 1, nb, fault);                  // left
  if (by > 0) {
    if ((c & 3u) && (C[b - BW] & 12u)) hs_union(P, b, b - BW, nb, fault);                        // up
    if (bx > 0 && (c & 1u) && (C[b - BW - 1] & 8u)) hs_union(P, b, b - BW - 1, nb, fault);      // up-left
    if (bx + 1 < BW && (c & 2u) && (C[b - BW + 1] & 4u)) hs_union(P, b, b - BW + 1, nb, fault); // up-right
  }
}

// parent = root; flags[z * nb + b] = 1 at every root (flags[S * nb] is the scan's closing zero)
__global__ __launch_bounds__(BT) void hs_flatten_kernel(int* __restrict__ parent, int nb, int S, int* __restrict__ flags) {
  const int b = blockIdx.x * BT + threadIdx.x, z = blockIdx.y;
  if (b >= nb) return;
  int* P = parent + (size_t)z * nb;
  int f = 0;
  const int p = P[b];
  if (p >= 0) {
    int r = p;
    for (int n = 0; n < nb && P[r] != r; ++n) r = P[r];
    P[b] = r;
    f = r == b;
  }
  flags[(size_t)z * nb + b] = f;
  if (z == S - 1 && b == nb - 1) flags[(size_t)S * nb] = 0;
}

// Labels and per-label sums: one work item per 2x2 block (its foreground pixels share one label).  Foreground sums meet in
// an LDS table keyed by label; the background's in a workgroup sum; then one set of 64-bit global atomics per entry.
__global__ __launch_bounds__(BT) void hs_stats_kernel(const uint8_t* __restrict__ code, const int* __restrict__ parent,
                                                      const int* __restrict__ scan, int H, int W, int BW, int nb,
                                                      int32_t* __restrict__ labels, unsigned long long* __restrict__ stats,
                                                      int32_t* __restrict__ n_out) {
  __shared__ int s_key[HT];
  __shared__ unsigned long long s_val[HT][3];
  __shared__ unsigned long long s_bg[3];
  const int tid = threadIdx.x, z = blockIdx.y;
  const int b = blockIdx.x * BT + tid;
  for (int i = tid; i < HT; i += BT) {
    s_key[i] = 0;
    s_val[i][0] = s_val[i][1] = s_val[i][2] = 0ull;
  }
  if (tid < 3) s_bg[tid] = 0ull;
  __syncthreads();
  const int* Sc = scan + (size_t)z * nb;
  const int base = Sc[0];
  unsigned bg_a = 0, bg_x = 0, bg_y = 0;                       // <= 4 pixels of one block: small
  if (b < nb) {
    const unsigned c = code[(size_t)z * nb + b];
    const int lab = c ? Sc[parent[(size_t)z * nb + b]] - base + 1 : 0;
    const int by = b / BW, bx = b - by * BW;
    unsigned fa = 0, fx = 0, fy = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int y = 2 * by + (q >> 1), x = 2 * bx + (q & 1);
      if (y >= H || x >= W) continue;
      const bool on = (c >> q) & 1u;
      if (on) {
        ++fa; fx += x; fy += y;
      } else {
        ++bg_a; bg_x += x; bg_y += y;
      }
      if (labels) labels[(size_t)z * H * W + (size_t)y * W + x] = on ? lab : 0;
    }
    if (fa) {
      int h = (int)(((unsigned)lab * 2654435761u) >> 23) & (HT - 1);
      for (int n = 0; n < HT; ++n, h = (h + 1) & (HT - 1)) {
        const int old = atomicCAS(&s_key[h], 0, lab);
        if (old == 0 || old == lab) {
          atomicAdd(&s_val[h][0], (unsigned long long)fa);
          atomicAdd(&s_val[h][1], (unsigned long long)fx);
          atomicAdd(&s_val[h][2], (unsigned long long)fy);
          break;
        }
      }
    }
    if (b == 0) n_out[z] = scan[(size_t)(z + 1) * nb] - base + 1;
  }
  // background: wave sums (64 blocks x 4 pixels x x < 65536: below 2^32), then LDS
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    bg_a += __shfl_xor(bg_a, off);
    bg_x += __shfl_xor(bg_x, off);
    bg_y += __shfl_xor(bg_y, off);
  }
  if ((tid & 63) == 0 && bg_a) {
    atomicAdd(&s_bg[0], (unsigned long long)bg_a);
    atomicAdd(&s_bg[1], (unsigned long long)bg_x);
    atomicAdd(&s_bg[2], (unsigned long long)bg_y);
  }
  __syncthreads();
  unsigned long long* St = stats + (size_t)z * (nb + 1) * 3;
  for (int i = tid; i < HT; i += BT) {
    const int lab = s_key[i];
    if (lab) {
      atomicAdd(St + (size_t)lab * 3 + 0, s_val[i][0]);
      atomicAdd(St + (size_t)lab * 3 + 1, s_val[i][1]);
      atomicAdd(St + (size_t)lab * 3 + 2, s_val[i][2]);
    }
  }
  if (tid == 0 && s_bg[0]) {
    atomicAdd(St + 0, s_bg[0]);
    atomicAdd(St + 1, s_bg[1]);
    atomicAdd(St + 2, s_bg[2]);
  }
}

__device__ __forceinline__ double wave_sum(double v) {       // every lane ends with the same value (+ commutes)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// cornerSubPix, one wavefront (= workgroup) per row, rows walked with the grid's stride; grid.y = image
__global__ __launch_bounds__(64) void hs_subpix_kernel(const uint8_t* __restrict__ imgs, size_t img_stride, int H, int W,
                                                       int nb, const unsigned long long* __restrict__ stats,
                                                       const int32_t* __restrict__ n_rows, int ww, int wh, int max_iter,
                                                       double eps2, hs_weights wt, float* __restrict__ xy,
                                                       size_t xy_stride, double* __restrict__ cen) {
  __shared__ float buf[HS_BUF_MAX];
  __shared__ float s_m[(2 * HS_WIN_MAX + 1) * (2 * HS_WIN_MAX + 1)];
  const int lane = threadIdx.x, z = blockIdx.y;
  const uint8_t* img = imgs + (size_t)z * img_stride;
  const int BW2 = 2 * ww + 3, BH2 = 2 * wh + 3, MW = 2 * ww + 1, MN = (2 * wh + 1) * (2 * ww + 1);
  for (int e = lane; e < MN; e += 64) {
    const int i = e / MW, j = e - i * MW;
    s_m[e] = wt.vy[i] * wt.ex[j];
  }
  const int n = n_rows[z];
  for (int row = blockIdx.x; row < n; row += gridDim.x) {
    const unsigned long long* st = stats + ((size_t)z * (nb + 1) + row) * 3;
    const double area = (double)st[0];
    const double cxd = (double)st[1] / area, cyd = (double)st[2] / area;   // empty background: 0 / 0 = NaN
    if (cen && lane == 0) {
      cen[((size_t)z * xy_stride + row) * 2] = cxd;
      cen[((size_t)z * xy_stride + row) * 2 + 1] = cyd;
    }
    const float tx = (float)cxd, ty = (float)cyd;
    float cx = tx, cy = ty;
    if (!(isnan(cx) || isnan(cy))) {
      int iter = 0;
      double err = 0.0;
      do {
        // getRectSubPix(img, (BW2, BH2), (cx, cy), CV_32F)
        const float ccx = cx - (float)(BW2 - 1) * 0.5f, ccy = cy - (float)(BH2 - 1) * 0.5f;
        const int ipx = (int)floorf(ccx), ipy = (int)floorf(ccy);
        const float a = ccx - (float)ipx, b = ccy - (float)ipy;
        __syncthreads();                                         // the previous iteration's reads of buf are done
        if (ipx >= 0 && ipx + BW2 < W && ipy >= 0 && ipy + BH2 < H) {
          const float ac = fmaxf(a, 0.0001f);
          const float b1 = 1.f - b, b2 = b, a12 = ac * b1, a22 = ac * b2;
          const double sd = (1. - ac) / ac;
          for (int e = lane; e < BW2 * BH2; e += 64) {
            const int i = e / BW2, j = e - i * BW2;
            const uint8_t* r0 = img + (size_t)(ipy + i) * W + ipx;
            const uint8_t* r1 = r0 + W;
            const float t = a12 * (float)r0[j + 1] + a22 * (float)r1[j + 1];
            float prev;
            if (j == 0) {
              prev = (1.f - ac) * (b1 * (float)r0[0] + b2 * (float)r1[0]);
            } else {
              const float tp = a12 * (float)r0[j] + a22 * (float)r1[j];
              prev = (float)((double)tp * sd);
            }
            buf[e] = prev + t;
          }
        } else {
          const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b;
          for (int e = lane; e < BW2 * BH2; e += 64) {
            const int i = e / BW2, j = e - i * BW2;
            const int x0 = min(max(ipx + j, 0), W - 1), x1 = min(max(ipx + j + 1, 0), W - 1);
            const int y0 = min(max(ipy + i, 0), H - 1), y1 = min(max(ipy + i + 1, 0), H - 1);
            const uint8_t* r0 = img + (size_t)y0 * W;
            const uint8_t* r1 = img + (size_t)y1 * W;
            buf[e] = (float)r0[x0] * a11 + (float)r0[x1] * a12 + (float)r1[x0] * a21 + (float)r1[x1] * a22;
          }
        }
        __syncthreads();
        double sa = 0, sb = 0, sc = 0, s1 = 0, s2 = 0;
        for (int e = lane; e < MN; e += 64) {
          const int i = e / MW, j = e - i * MW;
          const float* p = buf + (i + 1) * BW2 + (j + 1);
          const double m = s_m[e];
          const double tgx = p[1] - p[-1];
          const double tgy = p[BW2] - p[-BW2];
          const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
          const double px = j - ww, py = i - wh;
          sa += gxx;
          sb += gxy;
          sc += gyy;
          s1 += gxx * px + gxy * py;
          s2 += gxy * px + gyy * py;
        }
        sa = wave_sum(sa);
        sb = wave_sum(sb);
        sc = wave_sum(sc);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const double det = sa * sc - sb * sb;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
        const double scale = 1.0 / det;
        const float nx = (float)(cx + sc * scale * s1 - sb * scale * s2);
        const float ny = (float)(cy - sb * scale * s1 + sa * scale * s2);
        const float dx = nx - cx, dy = ny - cy;
        err = dx * dx + dy * dy;
        cx = nx;
        cy = ny;
        if (cx < 0 || cx >= W || cy < 0 || cy >= H) break;
      } while (++iter < max_iter && err > eps2);
      if (fabsf(cx - tx) > ww || fabsf(cy - ty) > wh) {
        cx = tx;
        cy = ty;
      }
    }
    if (lane == 0) {
      xy[((size_t)z * xy_stride + row) * 2] = cx;
      xy[((size_t)z * xy_stride + row) * 2 + 1] = cy;
    }
  }
}

hs_weights hs_make_weights(int ww, int wh) {       // as tests/harris_subpix_oracle.subpix_mask
  hs_weights w;
  memset(&w, 0, sizeof(w));
  for (int i = 0; i < 2 * wh + 1; ++i) {
    const float y = (float)(i - wh) / (float)wh;
    w.vy[i] = (float)std::exp(-(double)(y * y));
  }
  for (int j = 0; j < 2 * ww + 1; ++j) {
    const float x = (float)(j - ww) / (float)ww;
    w.ex[j] = (float)std::exp(-(double)(x * x));
  }
  return w;
}

int hs_check(vo_ctx* ctx, int S, int H, int W, int block, int ksize, int win_w, int win_h, int max_iter, double eps) {
  VO_REQUIRE(ctx, ksize == 3, "harris_subpix: ksize %d is not supported (3 only)", ksize);
  VO_REQUIRE(ctx, block >= 1 && block <= 31, "harris_subpix: blockSize must be in 1..31, got %d", block);
  VO_REQUIRE(ctx, win_w >= 1 && win_w <= HS_WIN_MAX && win_h >= 1 && win_h <= HS_WIN_MAX,
             "harris_subpix: window half-sizes must be in 1..%d, got (%d, %d)", HS_WIN_MAX, win_w, win_h);
  VO_REQUIRE(ctx, S >= 1 && S <= 65535, "harris_subpix: S must be in 1..65535, got %d", S);
  VO_REQUIRE(ctx, W >= 2 * win_w + 5 && H >= 2 * win_h + 5,
             "harris_subpix: a %dx%d image is below the window's minimum %dx%d", H, W, 2 * win_h + 5, 2 * win_w + 5);
  VO_REQUIRE(ctx, W < 65536 && H < 65536 && (long long)H * W <= (1ll << 30), "harris_subpix: image %dx%d too large", H, W);
  VO_REQUIRE(ctx, max_iter >= 1 && max_iter <= 100, "harris_subpix: max_iter must be in 1..100, got %d", max_iter);
  VO_REQUIRE(ctx, eps >= 0 && std::isfinite(eps), "harris_subpix: eps must be finite and >= 0");
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_harris_subpix_capacity(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return ((H + 1) / 2) * ((W + 1) / 2) + 1;
}

int vo_harris_subpix_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, int block,
                               int ksize, double k, double rel, int win_w, int win_h, int max_iter, double eps,
                               float* d_xy, size_t xy_stride, int32_t* d_n, float* d_response, int32_t* d_labels,
                               double* d_centroids) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(hs_check(ctx, S, H, W, block, ksize, win_w, win_h, max_iter, eps));
  VO_REQUIRE(ctx, d_imgs && d_xy && d_n, "harris_subpix: null pointer");
  VO_REQUIRE(ctx, std::isfinite(k) && std::isfinite(rel), "harris_subpix: k and rel must be finite");
  const int BW = (W + 1) / 2, BH = (H + 1) / 2, nb = BW * BH;
  const size_t px = (size_t)H * W, Sz = (size_t)S, cap = (size_t)nb + 1;
  VO_REQUIRE(ctx, img_stride >= px, "harris_subpix: img_stride %zu below H*W", img_stride);
  VO_REQUIRE(ctx, xy_stride >= cap, "harris_subpix: xy_stride %zu below the capacity %zu", xy_stride, cap);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  const size_t n_flags = Sz * nb + 1;
  size_t scan_tmp = 0;
  VO_HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, scan_tmp, (const int*)nullptr, (int*)nullptr, 0, n_flags,
                                          rocprim::plus<int>(), st));
  // scratch 11: response (when the caller does not take it); 12: parent | flags | scan | code; 13: stats;
  // 14: [max key S | fault]; 15: scan temporary
  const size_t o_flags = ((Sz * nb * 4) + 255) & ~size_t(255);
  const size_t o_scan = o_flags + ((n_flags * 4 + 255) & ~size_t(255));
  const size_t o_code = o_scan + ((n_flags * 4 + 255) & ~size_t(255));
  if (!d_response) VO_TRY(vo_ensure(ctx, s[11], Sz * px * 4));
  VO_TRY(vo_ensure(ctx, s[12], o_code + Sz * nb));
  VO_TRY(vo_ensure(ctx, s[13], Sz * cap * 24));
  VO_TRY(vo_ensure(ctx, s[14], (Sz + 1) * 4));
  VO_TRY(vo_ensure(ctx, s[15], scan_tmp + 256));
  float* resp = d_response ? d_response : (float*)s[11].p;
  char* w = (char*)s[12].p;
  int* parent = (int*)w;
  int* flags = (int*)(w + o_flags);
  int* scan = (int*)(w + o_scan);
  uint8_t* code = (uint8_t*)(w + o_code);
  unsigned long long* stats = (unsigned long long*)s[13].p;
  unsigned* ctl = (unsigned*)s[14].p;
  VO_HIP_TRY(ctx, hipMemsetAsync(ctl, 0, (Sz + 1) * 4, st));
  const double scale = 1.0 / (4.0 * block * 255.0);
  const int RW = GX + block - 1, RH = GY + block - 1;
  const size_t lds = ((size_t)RW * RH + (size_t)3 * RH * GX) * 4;
  hipLaunchKernelGGL(hs_response_kernel, dim3(vo_cdiv(W, GX), vo_cdiv(H, GY), S), dim3(GT), lds, st, d_imgs, img_stride, H,
                     W, block, (float)(scale * scale), k, resp, ctl);
  VO_TRY(vo_check_launch(ctx, "hs_response_kernel"));
  const dim3 gb(vo_cdiv(nb, BT), S);
  hipLaunchKernelGGL(hs_init_kernel, gb, dim3(BT), 0, st, (const float*)resp, H, W, BW, nb, (const unsigned*)ctl, rel, code,
                     parent, stats);
  VO_TRY(vo_check_launch(ctx, "hs_init_kernel"));
  hipLaunchKernelGGL(hs_merge_kernel, gb, dim3(BT), 0, st, (const uint8_t*)code, parent, BW, nb, ctl + S);
  VO_TRY(vo_check_launch(ctx, "hs_merge_kernel"));
  hipLaunchKernelGGL(hs_flatten_kernel, gb, dim3(BT), 0, st, parent, nb, S, flags);
  VO_TRY(vo_check_launch(ctx, "hs_flatten_kernel"));
  VO_HIP_TRY(ctx, rocprim::exclusive_scan(s[15].p, scan_tmp, (const int*)flags, scan, 0, n_flags, rocprim::plus<int>(),
                                          st));
  hipLaunchKernelGGL(hs_stats_kernel, gb, dim3(BT), 0, st, (const uint8_t*)code, (const int*)parent, (const int*)scan, H, W,
                     BW, nb, d_labels, stats, d_n);
  VO_TRY(vo_check_launch(ctx, "hs_stats_kernel"));
  const int rows_wg = (int)std::min<size_t>(cap, 8192);   // (2048: 187 us for 19.5k rows at 1376x1241)
  hipLaunchKernelGGL(hs_subpix_kernel, dim3(rows_wg, S), dim3(64), 0, st, d_imgs, img_stride, H, W, nb,
                     (const unsigned long long*)stats, (const int32_t*)d_n, win_w, win_h, max_iter, eps * eps,
                     hs_make_weights(win_w, win_h), d_xy, xy_stride, d_centroids);
  VO_TRY(vo_check_launch(ctx, "hs_subpix_kernel"));
  return VO_OK;
}

int vo_harris_subpix_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, int block, int ksize, double k, double rel,
                           int win_w, int win_h, int max_iter, double eps, float* xy, int32_t* n, float* response,
                           int32_t* labels, double* centroids) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(hs_check(ctx, S, H, W, block, ksize, win_w, win_h, max_iter, eps));
  VO_REQUIRE(ctx, imgs && xy && n, "harris_subpix: null pointer");
  for (int q = 0; q < S; ++q) n[q] = 0;
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)H * W, Sz = (size_t)S, cap = (size_t)vo_harris_subpix_capacity(H, W);
  // ctx->img: the images; ctx->img2: [n S | xy S x cap x 2 | centroids S x cap x 2 (when asked) | response | labels]
  const size_t o_xy = (Sz * 4 + 255) & ~size_t(255);
  const size_t o_cen = o_xy + ((Sz * cap * 8 + 255) & ~size_t(255));
  const size_t o_resp = o_cen + (centroids ? ((Sz * cap * 16 + 255) & ~size_t(255)) : 0);
  const size_t o_lab = o_resp + (response ? ((Sz * px * 4 + 255) & ~size_t(255)) : 0);
  const size_t total = o_lab + (labels ? Sz * px * 4 : 0);
  VO_TRY(vo_ensure(ctx, ctx->img, Sz * px));
  VO_TRY(vo_ensure(ctx, ctx->img2, total));
  VO_TRY(vo_ensure_pinned(ctx, Sz * px));
  memcpy(ctx->h_pin, imgs, Sz * px);
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, ctx->h_pin, Sz * px, hipMemcpyHostToDevice, st));
  char* d = (char*)ctx->img2.p;
  VO_TRY(vo_harris_subpix_batch_dev(ctx, (const uint8_t*)ctx->img.p, px, S, H, W, block, ksize, k, rel, win_w, win_h,
                                    max_iter, eps, (float*)(d + o_xy), cap, (int32_t*)d, response ? (float*)(d + o_resp) : nullptr,
                                    labels ? (int32_t*)(d + o_lab) : nullptr, centroids ? (double*)(d + o_cen) : nullptr));
  unsigned fault = 0;
  VO_HIP_TRY(ctx, hipMemcpyAsync(n, d, Sz * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(&fault, (const unsigned*)ctx->scratch[14].p + S, 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  if (fault) {
    for (int q = 0; q < S; ++q) n[q] = 0;
    return vo_set_error(ctx, VO_ECAPACITY, "harris_subpix: union-find did not settle within its bound");
  }
  for (int q = 0; q < S; ++q) {
    const size_t nq = (size_t)n[q];
    VO_HIP_TRY(ctx, hipMemcpyAsync(xy + q * cap * 2, d + o_xy + q * cap * 8, nq * 8, hipMemcpyDeviceToHost, st));
    if (centroids)
      VO_HIP_TRY(ctx, hipMemcpyAsync(centroids + q * cap * 2, d + o_cen + q * cap * 16, nq * 16, hipMemcpyDeviceToHost, st));
  }
  if (response) VO_HIP_TRY(ctx, hipMemcpyAsync(response, d + o_resp, Sz * px * 4, hipMemcpyDeviceToHost, st));
  if (labels) VO_HIP_TRY(ctx, hipMemcpyAsync(labels, d + o_lab, Sz * px * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_harris_subpix_corners(vo_ctx* ctx, const uint8_t* img, int H, int W, int block, int ksize, double k, double rel,
                             int win_w, int win_h, int max_iter, double eps, float* xy, int32_t* n, float* response,
                             int32_t* labels, double* centroids) {
  return vo_harris_subpix_batch(ctx, img, 1, H, W, block, ksize, k, rel, win_w, win_h, max_iter, eps, xy, n, response,
                                labels, centroids);
}

}  // extern "C"
