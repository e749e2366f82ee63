// Frame ingest: what a frame goes through between a camera's buffer and a frame slot -- the grey conversion of a
// three-channel image [ref: the cvtColor call sites, src/vo/features/klt.py:58-62, harris.py:41-48] and the lens
// undistortion the reference's Camera declares and leaves empty [ref: src/vo/sensors/camera.py:38-54].  Both are defined
// in integers / float64 so that the device and tests/frame_ingest_oracle.py agree bit for bit:
//   grey       g = (1868 B + 9617 G + 4899 R + 8192) >> 14, channel order B, G, R
//   undistort  for output pixel (u, v): the five-coefficient model (k1, k2, p1, p2, k3) maps the ideal point to the
//              distorted image, the source position is rounded to 1/32 pixel (ties to even) and the four neighbours are
//              blended with integer weights that sum to 1024; a neighbour outside the image counts as 0.
// The map is computed per output pixel (about 40 float64 operations): no per-lane table to keep or to invalidate.
#include <algorithm>
#include <cmath>

#include "vo_internal.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ unsigned gray_of(unsigned b, unsigned g, unsigned r) {
  return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

// A stream: n pixels, 3n bytes in, n bytes out.  `head` = the pixels in front of the first 4-byte boundary of `out`
// (0..3); the caller places the input so that in + 3 * head is 4-byte aligned too (vo_ingest_head).  Work item t of the
// first `groups` takes pixels head + 4t .. head + 4t + 3: three dword loads, one dword store.  The head and the tail
// (at most 3 + 3 pixels) go one pixel per work item.
__global__ __launch_bounds__(256) void ingest_gray_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, size_t n,
                                                          unsigned head, size_t groups) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < groups) {
    const size_t p = head + 4 * t;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(in + 3 * p);
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];     // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
    const unsigned g0 = gray_of(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
    const unsigned g1 = gray_of(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
    const unsigned g2 = gray_of((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
    const unsigned g3 = gray_of((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
    *reinterpret_cast<uint32_t*>(out + p) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    return;
  }
  const size_t j = t - groups, body_end = head + 4 * groups;
  if (j >= head + (n - body_end)) return;
  const size_t p = j < head ? j : body_end + (j - head);
  out[p] = (uint8_t)gray_of(in[3 * p], in[3 * p + 1], in[3 * p + 2]);
}

// One output pixel per work item; CH = 1: `in` is a grey image, CH = 3: a B, G, R image whose taps are converted as
// they are read (the same bytes undistort(gray(img)) gives: the grey value is a function of the pixel alone).
// Neighbouring work items read neighbouring source pixels: the gather is served by the caches.
template <int CH>
__global__ __launch_bounds__(256) void ingest_undistort_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H,
                                                               int W, vo_undist q) {
  const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
  if (u >= W || v >= H) return;
  const double x = ((double)u - q.cx) / q.fx, y = ((double)v - q.cy) / q.fy;
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = (2.0 * x) * y;
  const double kr = 1.0 + ((q.k3 * r2 + q.k2) * r2 + q.k1) * r2;
  const double xd = (x * kr + q.p1 * _2xy) + q.p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + q.p1 * (r2 + 2.0 * y2)) + q.p2 * _2xy;
  const double us = q.fxr * xd + q.cxr, vs = q.fyr * yd + q.cyr;
  const double lim = 16777216.0;                            // 2^24 (fmin / fmax: a NaN becomes a bound)
  const int ix = (int)rint(fmin(fmax(us * 32.0, -lim), lim)), iy = (int)rint(fmin(fmax(vs * 32.0, -lim), lim));
  const int x0 = ix >> 5, fx5 = ix & 31, y0 = iy >> 5, fy5 = iy & 31;
  auto tap = [&](int xx, int yy) -> int {
    if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) return 0;
    const uint8_t* s = in + ((size_t)yy * W + xx) * CH;
    if (CH == 1) return s[0];
    return (int)gray_of(s[0], s[1], s[2]);
  };
  const int p00 = tap(x0, y0), p10 = tap(x0 + 1, y0), p01 = tap(x0, y0 + 1), p11 = tap(x0 + 1, y0 + 1);
  const int acc = (32 - fx5) * (32 - fy5) * p00 + fx5 * (32 - fy5) * p10 + (32 - fx5) * fy5 * p01 + fx5 * fy5 * p11 + 512;
  out[(size_t)v * W + u] = (uint8_t)(acc >> 10);
}

bool all_finite(const double* a, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

}  // namespace

int vo_undist_make(vo_ctx* ctx, const char* who, const double* K, const double* dist, const double* K_raw, vo_undist* out) {
  VO_REQUIRE(ctx, K && out, "%s: bad arguments", who);
  if (!K_raw) K_raw = K;
  const double zero[5] = {0, 0, 0, 0, 0};
  if (!dist) dist = zero;
  VO_REQUIRE(ctx, all_finite(K, 9) && all_finite(K_raw, 9) && all_finite(dist, 5),
             "%s: non-finite intrinsics or distortion coefficients", who);
  VO_REQUIRE(ctx, K[0] != 0.0 && K[4] != 0.0, "%s: singular intrinsics", who);
  *out = vo_undist{K[0], K[4], K[2], K[5], K_raw[0], K_raw[4], K_raw[2], K_raw[5], dist[0], dist[1], dist[2], dist[3], dist[4]};
  return VO_OK;
}

int vo_ingest_dev(vo_ctx* ctx, hipStream_t st, const uint8_t* d_in, int channels, int H, int W, const vo_undist* und,
                  uint8_t* d_out) {
  VO_REQUIRE(ctx, d_in && d_out && H > 0 && W > 0 && (channels == 1 || channels == 3) && (channels == 3 || und),
             "ingest: bad arguments");
  if (und) {
    const dim3 grid((unsigned)vo_cdiv(W, 64), (unsigned)vo_cdiv(H, 4)), block(64, 4);
    if (channels == 3) hipLaunchKernelGGL(ingest_undistort_kernel<3>, grid, block, 0, st, d_in, d_out, H, W, *und);
    else hipLaunchKernelGGL(ingest_undistort_kernel<1>, grid, block, 0, st, d_in, d_out, H, W, *und);
    return vo_check_launch(ctx, "ingest_undistort");
  }
  const size_t n = (size_t)H * W;
  const unsigned head = (unsigned)std::min<size_t>(vo_ingest_head(d_out), n);
  VO_REQUIRE(ctx, ((uintptr_t)d_in + 3 * (uintptr_t)head) % 4 == 0, "ingest: the input is not placed for dword loads");
  const size_t groups = (n - head) / 4, items = groups + head + (n - head - 4 * groups);
  hipLaunchKernelGGL(ingest_gray_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d_in, d_out, n, head, groups);
  return vo_check_launch(ctx, "ingest_gray");
}

extern "C" {

// cv2.cvtColor(img, COLOR_BGR2GRAY) of the reference's call sites [ref: src/vo/features/klt.py:58-62, harris.py:41-48]
int vo_gray_from_bgr(vo_ctx* ctx, const uint8_t* bgr, int H, int W, uint8_t* gray) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, bgr && gray && H > 0 && W > 0, "gray_from_bgr: bad arguments");
  const size_t px = (size_t)H * W;
  VO_TRY(vo_ensure(ctx, ctx->img, 3 * px));
  VO_TRY(vo_ensure(ctx, ctx->img2, px));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, bgr, 3 * px, hipMemcpyHostToDevice, ctx->stream));
  VO_TRY(vo_ingest_dev(ctx, ctx->stream, (const uint8_t*)ctx->img.p, 3, H, W, nullptr, (uint8_t*)ctx->img2.p));
  VO_HIP_TRY(ctx, hipMemcpyAsync(gray, ctx->img2.p, px, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VO_OK;
}

// Camera.undistort [ref: src/vo/sensors/camera.py:47-54, a stub there]
int vo_undistort_image(vo_ctx* ctx, const uint8_t* img, int H, int W, const double* K, const double* dist, const double* K_raw,
                       uint8_t* out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, img && out && H > 0 && W > 0, "undistort_image: bad arguments");
  vo_undist und;
  VO_TRY(vo_undist_make(ctx, "undistort_image", K, dist, K_raw, &und));
  const size_t px = (size_t)H * W;
  VO_TRY(vo_ensure(ctx, ctx->img, px));
  VO_TRY(vo_ensure(ctx, ctx->img2, px));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, img, px, hipMemcpyHostToDevice, ctx->stream));
  VO_TRY(vo_ingest_dev(ctx, ctx->stream, (const uint8_t*)ctx->img.p, 1, H, W, &und, (uint8_t*)ctx->img2.p));
  VO_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->img2.p, px, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VO_OK;
}

}  // extern "C"
