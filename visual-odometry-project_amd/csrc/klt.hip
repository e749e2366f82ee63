// Pyramidal Lucas-Kanade tracking for gfx950 (the pyramid it reads is built by pyramid.hip).
//
// Reference call site: src/vo/features/klt.py:233-249
//   cv2.calcOpticalFlowPyrLK(prev, next, prevPts, None, winSize=(17,17), maxLevel=2,
//                            criteria=(EPS|COUNT, 10, 0.03))          (klt.py:29-33)
// The arithmetic (Bouguet's pyramidal LK as OpenCV implements it) is restated in
// oracle/csrc/klt.c; this file is the device version of the same definition:
//   Scharr    (3,10,3) int16 derivatives, reflect-101 inside the image, 0 outside
//   bilinear  14-bit fixed-point weights, template kept at 5 extra bits
//   solve     2x2 normal equations in float32 (sums are exact integers converted
//             once), <= max_iter steps, |d|^2 <= eps^2 and ping-pong stops
// Two kernels: klt_track_kernel, one wavefront per keypoint (the 64 lanes share the window pixels, patch data in LDS,
// window sums reduced across the wave), and klt_track16_kernel, one lane per window row (windows 15, 17 and 21).  They
// differ in how lanes hold the window; which points a launch tracks (klt_points) and every rule of the level loop
// (klt_level_entry ... klt_write) are functions both call.  Every lane carries the (uniform) 2x2 solve.
#include <type_traits>
#include "pyramid_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_WIN = 31;
constexpr int W_BITS = 14;
constexpr float FLT_SCALE = 1.f / (float)(1 << 20);

// Sum over the 64 lanes of a wave with DPP row operations (no LDS traffic), result in
// every lane.  Steps: within quads, within half rows, within rows of 16, then the two
// row broadcasts that gfx9 provides for wave64.
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);   // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);   // row_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast15 into rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);   // row_bcast31 into rows 2, 3
  return __builtin_amdgcn_readlane(v, 63);
}

// exact 64-bit sum of per-lane 32-bit partials: two 16-bit limbs, each summed in 32 bits
__device__ __forceinline__ long long wave_sum(int v) {
  const int lo = wave_sum_i32(v & 0xffff);
  const int hi = wave_sum_i32(v >> 16);
  return (long long)hi * 65536LL + (long long)lo;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ __forceinline__ void bilinear_weights(float a, float b, int& w00, int& w01, int& w10, int& w11) {
  w00 = (int)rintf((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
  w01 = (int)rintf(a * (1.f - b) * (float)(1 << W_BITS));
  w10 = (int)rintf((1.f - a) * b * (float)(1 << W_BITS));
  w11 = (1 << W_BITS) - w00 - w01 - w10;
}

// stage the (n x n) block of image pixels whose top-left is (x0, y0) into LDS, reflect-101.
// Loads go out in batches of 8 per lane before any is written to LDS (one memory round
// trip per batch instead of one per byte).
__device__ __forceinline__ void stage_region(const uint8_t* __restrict__ img, int pitch, int H, int W, int x0, int y0,
                                             int n, uint8_t* s, int lane) {
  const bool inside = x0 >= 0 && y0 >= 0 && x0 + n <= W && y0 + n <= H;
  const int total = n * n;
  for (int b0 = 0; b0 < total; b0 += 8 * 64) {
    uint8_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = b0 + k * 64 + lane;
      const int ii = i < total ? i : total - 1;
      const int ly = ii / n, lx = ii - ly * n;
      const int gy = inside ? y0 + ly : reflect101(y0 + ly, H);
      const int gx = inside ? x0 + lx : reflect101(x0 + lx, W);
      v[k] = img[(size_t)gy * pitch + gx];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = b0 + k * 64 + lane;
      if (i < total) s[i] = v[k];
    }
  }
}

constexpr int KLT_MARGIN = 4;   // pixels of slack staged around the search window
constexpr int KLT_WAVES = 4;    // keypoints (waves) per workgroup

// Orders LDS traffic between the lanes of ONE wave (each wave owns a private LDS slice, and
// waves of a workgroup run different trip counts, so a workgroup barrier must not be used).
// The LDS executes a wave's instructions in order; only the compiler has to be held back.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- forward-backward check (vo_hip.h, "pyramidal KLT": vo_klt_track_fb) ----
// What a lane group keeps of a point between the two passes of an FB kernel.
template <bool FB>
struct klt_fb_keep {};
template <>
struct klt_fb_keep<true> {
  float p0x, p0y;        // where the point started (prev_xy, or the detector's keypoint as float32)
  float nx, ny, err;     // the forward pass's result
  bool ok = false;       // ... and status; false until the forward pass has been closed by klt_fb_turn
};
__device__ __forceinline__ bool klt_fb_turn(klt_fb_keep<false>&, bool&, float&, float&, float&, float&, bool&, float&) { return false; }
// After the forward pass (back is false): closes it and sets the second one up, p0 <- the forward result, back <- true.
// false: the second pass has run, or the point sits it out
__device__ __forceinline__ bool klt_fb_turn(klt_fb_keep<true>& k, bool& back, float& p0x, float& p0y, float& nx, float& ny,
                                            bool& ok, float& e_out) {
  if (back) return false;
  k.p0x = p0x;
  k.p0y = p0y;
  k.nx = nx;
  k.ny = ny;
  k.err = e_out;
  k.ok = ok;
  if (!ok) return false;
  p0x = nx;
  p0y = ny;
  nx = 0.f;
  ny = 0.f;
  e_out = 0.f;
  back = true;
  return true;
}
__device__ __forceinline__ void klt_fb_write(const klt_fb_keep<false>&, float, float, bool, float, int, float*, uint8_t*, float*,
                                             float*) {}
// (bx, by, ok_b): the backward pass's result; a point whose forward pass failed never ran it (k.ok is false)
__device__ __forceinline__ void klt_fb_write(const klt_fb_keep<true>& k, float bx, float by, bool ok_b, float thr2, int i,
                                             float* __restrict__ next_xy, uint8_t* __restrict__ status,
                                             float* __restrict__ err, float* __restrict__ fb) {
  const bool both = k.ok && ok_b;
  const float dx = bx - k.p0x, dy = by - k.p0y;
  const float d2 = both ? dx * dx + dy * dy : __builtin_inff();     // (fp contract is off: two products, one sum)
  next_xy[2 * i] = k.nx;
  next_xy[2 * i + 1] = k.ny;
  err[i] = k.err;
  fb[i] = d2;
  status[i] = (both && d2 <= thr2) ? 1 : 0;                          // a tie is kept
}

// ---- which points a launch tracks ----
// The kernel's arrays moved to the sequence of blockIdx.y (vo_klt_batch), the keypoint count N as the device knows it
// (d_n, vo_klt_source) and the time stamp.  Leaves pyr_off, the sequence's offset into both pyramid buffers, and n_own:
// points 0 .. n_own-1 start from prev_xy, the rest from the detector's keypoints.
// (the kernel argument P is left untouched, hence pyr_off: written to, P would be copied to scratch -- one copy per lane
//  -- for the run-time level index; measured as 14 MB of scratch traffic per launch)
template <bool FB>
__device__ __forceinline__ void klt_points(const float* __restrict__& prev_xy, int& N, const int* __restrict__ d_n,
                                           vo_klt_source& src, const vo_klt_batch& B, float* __restrict__& next_xy,
                                           uint8_t* __restrict__& status, float* __restrict__& err, float* __restrict__& fb,
                                           size_t& pyr_off, int& n_own) {
  pyr_off = 0;
  if (blockIdx.y != 0) {                               // several sequences per launch: grid.y = sequence
    const size_t q = blockIdx.y;
    pyr_off = q * B.pyr;
    prev_xy += q * B.xy;
    next_xy += q * B.xy;
    status += q * B.out;
    err += q * B.out;
    if (FB) fb += q * B.out;
    if (src.n) {
      src.n = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(src.n) + q * B.ctl);
      src.num_features = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(src.num_features) + q * B.ctl);
      src.det_kp += q * B.det;
      if (src.ts) src.ts = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(src.ts) + q * B.ctl);
      if (src.det_go) src.det_go += q;
      if (src.n_det_dev) src.n_det_dev += q;
    }
  }
  if (d_n) N = min(N, *d_n);                           // keypoint count read on the device (frame pipeline)
  n_own = N;
  if (src.ts && blockIdx.x == 0 && threadIdx.x == 0) *src.ts = wall_clock64();
  if (src.n) {
    n_own = *src.n;
    const bool redetect = (double)n_own < (double)*src.num_features * src.frac && (!src.det_go || *src.det_go != 0);
    N = min(N, n_own + (redetect ? (src.n_det_dev ? max(*src.n_det_dev, 0) : src.n_det) : 0));
  }
}

// where point i starts: prev_xy, or the detector's keypoint as float32
__device__ __forceinline__ float2 klt_point_start(const float* __restrict__ prev_xy, const vo_klt_source& src, int n_own, int i) {
  if (i >= n_own) return make_float2((float)src.det_kp[2 * (i - n_own)], (float)src.det_kp[2 * (i - n_own) + 1]);
  return make_float2(prev_xy[2 * i], prev_xy[2 * i + 1]);
}

// ---- the tracker's rules, each stated once for both kernels ----
// The kernels differ in how lanes hold the window (LDS template and wave sums; register rows and DPP row sums) and keep
// their level loops written out; every decision of the loop is one of these functions.

// corner (x, y) of a window -> the pixel it falls in and the bilinear weights; false (the position rule): the window lies
// wholly outside the W x H level
__device__ __forceinline__ bool klt_window_at(float x, float y, int win, int W, int H, int& ix, int& iy, int& w00, int& w01,
                                              int& w10, int& w11) {
  ix = (int)floorf(x);
  iy = (int)floorf(y);
  if (ix < -win || ix >= W || iy < -win || iy >= H) return false;
  bilinear_weights(x - (float)ix, y - (float)iy, w00, w01, w10, w11);
  return true;
}

// corner of the template window of p0 at a level
__device__ __forceinline__ void klt_template_corner(int level, float p0x, float p0y, float half, float& px, float& py) {
  const float sc = (float)(1. / (double)(1 << level));
  px = p0x * sc - half;
  py = p0y * sc - half;
}

// Entry of a level: the starting guess (n <- q: p0 scaled at the top level, twice the level above's result below it; q is
// left as the search window's corner), the template window's corner pixel and weights.  false: the level is skipped.
__device__ __forceinline__ bool klt_level_entry(int level, int n_levels, float p0x, float p0y, float half, int win, int W, int H,
                                                float& nx, float& ny, float& qx, float& qy, int& ipx, int& ipy, int& w00,
                                                int& w01, int& w10, int& w11, bool& ok, float& e_out) {
  float px, py;
  klt_template_corner(level, p0x, p0y, half, px, py);
  if (level == n_levels - 1) {
    const float sc = (float)(1. / (double)(1 << level));
    qx = p0x * sc;
    qy = p0y * sc;
  } else {
    qx = nx * 2.f;
    qy = ny * 2.f;
  }
  nx = qx;
  ny = qy;
  qx -= half;
  qy -= half;
  if (klt_window_at(px, py, win, W, H, ipx, ipy, w00, w01, w10, w11)) return true;
  if (level == 0) {
    ok = false;
    e_out = 0.f;
  }
  return false;
}

// the solve test; D <- 1 / det.  false: the level is skipped
__device__ __forceinline__ bool klt_solve(float A11, float A12, float A22, int ww, float min_eig_thr, int level, float& D, bool& ok) {
  D = A11 * A22 - A12 * A12;
  const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * ww);
  if (minEig < min_eig_thr || D < 1.1920929e-07f) {
    if (level == 0) ok = false;
    return false;
  }
  D = 1.f / D;
  return true;
}

// one Newton update from the mismatch (fb1, fb2) of iteration j, with both stops; true: the iteration ends
__device__ __forceinline__ bool klt_newton_update(float A11, float A12, float A22, float D, float fb1, float fb2, int j, double eps2,
                                                  float half, float& qx, float& qy, float& nx, float& ny, float& pdx, float& pdy) {
  const float ddx = (A12 * fb2 - A22 * fb1) * D;
  const float ddy = (A12 * fb1 - A11 * fb2) * D;
  qx += ddx;
  qy += ddy;
  nx = qx + half;
  ny = qy + half;
  if ((double)ddx * (double)ddx + (double)ddy * (double)ddy <= eps2) return true;
  if (j > 0 && fabsf(ddx + pdx) < 0.01f && fabsf(ddy + pdy) < 0.01f) {
    nx -= ddx * 0.5f;
    ny -= ddy * 0.5f;
    return true;
  }
  pdx = ddx;
  pdy = ddy;
  return false;
}

// the restage test: the search region of `next` is staged with KLT_MARGIN pixels of slack and staged again only when
// the (n1 x n1 block of the) window at (ix, iy) walks out of it; true: (rx0, ry0) is the corner to stage
__device__ __forceinline__ bool klt_restage(bool& staged, int ix, int iy, int n1, int RS, int& rx0, int& ry0) {
  if (staged && ix >= rx0 && iy >= ry0 && ix + n1 <= rx0 + RS && iy + n1 <= ry0 + RS) return false;
  rx0 = ix - KLT_MARGIN;
  ry0 = iy - KLT_MARGIN;
  staged = true;
  return true;
}

// the writer lane's stores
template <bool FB>
__device__ __forceinline__ void klt_write(const klt_fb_keep<FB>& fwd, float nx, float ny, bool ok, float e_out, float fb_thr2, int i,
                                          float* __restrict__ next_xy, uint8_t* __restrict__ status, float* __restrict__ err,
                                          float* __restrict__ fb) {
  if (FB) {
    klt_fb_write(fwd, nx, ny, ok, fb_thr2, i, next_xy, status, err, fb);
  } else {
    next_xy[2 * i] = nx;
    next_xy[2 * i + 1] = ny;
    status[i] = ok ? 1 : 0;
    err[i] = e_out;
  }
}

// ---- one wavefront per keypoint, any window from 3 to MAX_WIN ----
// WIN_T > 0: window side known at compile time (index arithmetic folds, loops unroll)
// FB: the forward-backward variant (vo_klt_track_fb).  The wave that tracked a point forward keeps p0 and its result in
// registers, runs the level loop a second time with the two pyramids exchanged, starting from the forward result, and
// writes the squared round-trip distance and the combined status.  With FB = false the second pass does not exist and
// fb_thr2 and fb are not read.
template <int WIN_T, bool FB = false>
__global__ __launch_bounds__(64 * KLT_WAVES) void klt_track_kernel(pyr_t P, const float* __restrict__ prev_xy, int N, const int* __restrict__ d_n, vo_klt_source src, vo_klt_batch B, int win_arg,
                                                       int max_iter, double eps2, float min_eig_thr,
                                                       float* __restrict__ next_xy, uint8_t* __restrict__ status,
                                                       float* __restrict__ err, int lds_per_wave, float fb_thr2,
                                                       float* __restrict__ fb) {
  extern __shared__ __align__(16) unsigned char smem_all[];
  const int i = blockIdx.x * KLT_WAVES + (threadIdx.x >> 6);
  size_t pyr_off;
  int n_own;
  klt_points<FB>(prev_xy, N, d_n, src, B, next_xy, status, err, fb, pyr_off, n_own);
  if (i >= N) return;                                  // whole wave leaves together
  unsigned char* smem = smem_all + (size_t)(threadIdx.x >> 6) * lds_per_wave;
  const int lane = threadIdx.x & 63;
  const int win = WIN_T > 0 ? WIN_T : win_arg;
  const int ww = win * win;
  const int n1 = win + 1, n3 = win + 3;
  const int RS = n1 + 2 * KLT_MARGIN;             // side of the staged search region
  // LDS: region bytes (max(n3*n3, RS*RS)) | derivatives int (n1*n1, dx | dy << 16) | template shorts (3 * ww)
  uint8_t* s_reg = smem;
  int* s_der = reinterpret_cast<int*>(smem + ((max(n3 * n3, RS * RS) + 15) & ~15));
  short4* s_tpl = reinterpret_cast<short4*>(s_der + n1 * n1 + ((n1 * n1) & 1));   // 8-byte aligned

  const float half = (float)(win - 1) * 0.5f;
  const float2 p0 = klt_point_start(prev_xy, src, n_own, i);
  float p0x = p0.x, p0y = p0.y;
  bool ok = true;
  float e_out = 0.f;
  float nx = 0.f, ny = 0.f;
  klt_fb_keep<FB> fwd;                                 // (empty without FB)
  bool back = false;                                   // FB: the second pass (next -> prev) is running

second_pass:
  for (int level = P.n_levels - 1; level >= 0; --level) {
    const uint8_t* I = (FB && back ? P.next[level] : P.prev[level]) + pyr_off;
    const uint8_t* J = (FB && back ? P.prev[level] : P.next[level]) + pyr_off;
    const int H = P.H[level], W = P.W[level], pitch = P.pitch[level];
    float qx, qy;
    int ipx, ipy, w00, w01, w10, w11;
    if (!klt_level_entry(level, P.n_levels, p0x, p0y, half, win, W, H, nx, ny, qx, qy, ipx, ipy, w00, w01, w10, w11, ok, e_out))
      continue;

    // ---- template: image block, Scharr derivatives, interpolated patch ----
    wave_sync();
    stage_region(I, pitch, H, W, ipx - 1, ipy - 1, n3, s_reg, lane);
    wave_sync();
    for (int k = lane; k < n1 * n1; k += 64) {
      const int ly = k / n1, lx = k - ly * n1;
      const int gy = ipy + ly, gx = ipx + lx;
      int dx = 0, dy = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const uint8_t* r0 = s_reg + ly * n3 + lx;
        const uint8_t* r1 = r0 + n3;
        const uint8_t* r2 = r1 + n3;
        const int t0 = (r0[0] + r2[0]) * 3 + r1[0] * 10;
        const int t2 = (r0[2] + r2[2]) * 3 + r1[2] * 10;
        const int d0 = r2[0] - r0[0], d1 = r2[1] - r0[1], d2 = r2[2] - r0[2];
        dx = t2 - t0;
        dy = (d2 + d0) * 3 + d1 * 10;
      }
      s_der[k] = (dx & 0xffff) | (dy << 16);
    }
    wave_sync();
    int a11 = 0, a12 = 0, a22 = 0;   // per-lane partial sums stay below 2^31 for win <= 31
    for (int k = lane; k < ww; k += 64) {
      const int y = k / win, x = k - y * win;
      const uint8_t* r = s_reg + (y + 1) * n3 + (x + 1);
      const int ival = descale(r[0] * w00 + r[1] * w01 + r[n3] * w10 + r[n3 + 1] * w11, W_BITS - 5);
      const int* d = s_der + y * n1 + x;
      const int v00 = d[0], v01 = d[1], v10 = d[n1], v11 = d[n1 + 1];
      const int ix = descale((int)(short)(v00 & 0xffff) * w00 + (int)(short)(v01 & 0xffff) * w01 +
                                 (int)(short)(v10 & 0xffff) * w10 + (int)(short)(v11 & 0xffff) * w11,
                             W_BITS);
      const int iy = descale((v00 >> 16) * w00 + (v01 >> 16) * w01 + (v10 >> 16) * w10 + (v11 >> 16) * w11, W_BITS);
      s_tpl[k] = make_short4((short)ival, (short)ix, (short)iy, 0);
      a11 += ix * ix;
      a12 += ix * iy;
      a22 += iy * iy;
    }
    const float A11 = (float)wave_sum(a11) * FLT_SCALE;
    const float A12 = (float)wave_sum(a12) * FLT_SCALE;
    const float A22 = (float)wave_sum(a22) * FLT_SCALE;
    float D;
    if (!klt_solve(A11, A12, A22, ww, min_eig_thr, level, D, ok)) continue;
    float pdx = 0.f, pdy = 0.f;
    int rx0 = 0, ry0 = 0;
    bool staged = false;
    auto stage_search = [&](int ix, int iy) {
      if (klt_restage(staged, ix, iy, n1, RS, rx0, ry0)) {
        wave_sync();
        stage_region(J, pitch, H, W, rx0, ry0, RS, s_reg, lane);
        wave_sync();
      }
    };
    for (int j = 0; j < max_iter; ++j) {
      int iqx, iqy;
      if (!klt_window_at(qx, qy, win, W, H, iqx, iqy, w00, w01, w10, w11)) {
        if (level == 0) ok = false;
        break;
      }
      stage_search(iqx, iqy);
      const uint8_t* base = s_reg + (iqy - ry0) * RS + (iqx - rx0);
      int b1 = 0, b2 = 0;
#pragma unroll
      for (int k = lane; k < ww; k += 64) {
        const int y = k / win, x = k - y * win;
        const uint8_t* r = base + y * RS + x;
        const int jv = descale(r[0] * w00 + r[1] * w01 + r[RS] * w10 + r[RS + 1] * w11, W_BITS - 5);
        const short4 t = s_tpl[k];
        const int diff = jv - t.x;
        b1 += diff * t.y;
        b2 += diff * t.z;
      }
      const float fb1 = (float)wave_sum(b1) * FLT_SCALE;
      const float fb2 = (float)wave_sum(b2) * FLT_SCALE;
      if (klt_newton_update(A11, A12, A22, D, fb1, fb2, j, eps2, half, qx, qy, nx, ny, pdx, pdy)) break;
    }
    if (ok && level == 0) {
      int iex, iey;
      if (!klt_window_at(nx - half, ny - half, win, W, H, iex, iey, w00, w01, w10, w11)) {
        ok = false;
        continue;
      }
      stage_search(iex, iey);
      const uint8_t* base = s_reg + (iey - ry0) * RS + (iex - rx0);
      int sabs = 0;
      for (int k = lane; k < ww; k += 64) {
        const int y = k / win, x = k - y * win;
        const uint8_t* r = base + y * RS + x;
        const int jv = descale(r[0] * w00 + r[1] * w01 + r[RS] * w10 + r[RS + 1] * w11, W_BITS - 5);
        const int diff = jv - s_tpl[k].x;
        sabs += diff < 0 ? -diff : diff;
      }
      e_out = (float)wave_sum(sabs) / (float)(32 * ww);
    }
  }
  if constexpr (FB) {                                  // once more, next -> prev, from the forward result as stored
    if (klt_fb_turn(fwd, back, p0x, p0y, nx, ny, ok, e_out)) goto second_pass;
  }
  if (lane == 0) klt_write<FB>(fwd, nx, ny, ok, e_out, fb_thr2, i, next_xy, status, err, fb);
}


// ---------------------------------------------------------------------------------
// Windows of 15, 17 and 21: one lane per window row -- 16 lanes (a DPP row, four keypoints per
// wave) for 15x15, 32 lanes (two keypoints per wave) for the larger ones
// ---------------------------------------------------------------------------------
// The wave layout spends most of its issue slots on work that is uniform per keypoint
// (window position, bilinear weights, the 2x2 solve, the reduction tree), replicated over the
// 64 lanes of a wave and paid once per keypoint.  Here a keypoint owns 16 lanes: lane r holds
// window row r -- the 16 source bytes of the row come from LDS in one read, the template row
// (patch value, Ix, Iy for 15 pixels) stays in registers for all iterations, the derivative
// row below is fetched from the neighbouring lane with a DPP row shift, and the window sums
// are four DPP adds inside the row.  The uniform work is now shared by four keypoints.
// Same arithmetic, in the same order per keypoint, as the wave layout (integer sums are
// exact, so their order is free).
typedef short v2i16 __attribute__((ext_vector_type(2)));
typedef unsigned u32_any __attribute__((aligned(1)));
typedef unsigned short u16_any __attribute__((aligned(1)));

// geometry of the row kernel for a WIN x WIN window
template <int WIN>
struct klt_rows {
  static constexpr int n1 = WIN + 1, n3 = WIN + 3;          // derivative rows / rows of the template block
  static constexpr int RS = n1 + 2 * KLT_MARGIN;            // side of the staged search region
  static constexpr int PITCH = (RS + 7) & ~7;               // LDS bytes per staged row
  static constexpr int SLICE = PITCH * RS;                  // LDS bytes per keypoint
  static constexpr int WA = (n3 + 3) / 4, WB = (n1 + 3) / 4;   // words per template-block row / search row
  static_assert(WIN + 5 <= PYR_PAD, "the staged blocks must stay inside the pyramid's border");
};

__device__ __forceinline__ int row_sum_i32(int v) {   // sum over the 16 lanes of a row, in all of them
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);   // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);   // row_mirror
  return v;
}
// sum over the LPK (16 or 32) lanes of a keypoint, in all of them
template <int LPK>
__device__ __forceinline__ int kp_sum_i32(int v) {
  v = row_sum_i32(v);
  if (LPK == 32) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast15: rows 1, 3 += rows 0, 2
    const int lo = __builtin_amdgcn_readlane(v, 31), hi = __builtin_amdgcn_readlane(v, 63);
    v = (threadIdx.x & 32) ? hi : lo;
  }
  return v;
}
// exact sum of per-lane 32-bit partials (two 16-bit limbs), as a double (|sum| < 2^53)
template <int LPK>
__device__ __forceinline__ double kp_sum_exact(int v) {
  const int lo = kp_sum_i32<LPK>(v & 0xffff);
  const int hi = kp_sum_i32<LPK>(v >> 16);
  return (double)hi * 65536.0 + (double)lo;
}

__device__ __forceinline__ int byte_at(const unsigned* w, int c) { return (int)((w[c >> 2] >> ((c & 3) * 8)) & 0xffu); }
// (byte c) | (byte c+1) << 16 of a little-endian word array
__device__ __forceinline__ unsigned pair_at(const unsigned* w, int c) {
  const int k = c >> 2, b = c & 3;
  const unsigned sel = (unsigned)b | 0x0c00u | ((unsigned)(b + 1) << 16) | 0x0c000000u;
  return __builtin_amdgcn_perm(b == 3 ? w[k + 1] : 0u, w[k], sel);   // byte index 4 = first byte of the next word
}
__device__ __forceinline__ int sdot2(unsigned a, unsigned b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, a), __builtin_bit_cast(v2i16, b), c, false);
}

// NB (16, 18 or 22) bytes from a byte-aligned LDS address into words.  The pieces behind the first
// 16 bytes are volatile on purpose: left to itself the compiler pairs the tails of two rows into one
// ds_read2_b32, which ignores the low address bits and returns the wrong bytes for a misaligned base.
template <int NB>
__device__ __forceinline__ void load_row_bytes(const uint8_t* p, unsigned* w) {
  __builtin_memcpy(w, p, 16);
  if (NB >= 20) {
    w[4] = *reinterpret_cast<const volatile u32_any*>(p + 16);
    w[5] = NB >= 22 ? (unsigned)*reinterpret_cast<const volatile u16_any*>(p + 20) : 0u;
  } else {
    w[4] = NB >= 18 ? (unsigned)*reinterpret_cast<const volatile u16_any*>(p + 16) : 0u;
    w[5] = 0u;
  }
}

// rows [0, NR) x bytes [0, NC) of the image block whose top-left pixel is (x0, y0) -> s, pitch
// PITCH; lane r takes rows r, r + LPK, ...  The block may hang over the image by up to WIN + 4
// pixels: the level is stored with PYR_PAD pixels of reflected border.
// The two halves are separate so that a block can be requested long before it is needed (the template
// block of the next level while this level iterates, the search region while the template is built).
template <int NC, int NR, int LPK>
struct staged_block {
  static constexpr int PASSES = (NR + LPK - 1) / LPK, WORDS = (NC + 3) / 4;
  unsigned v[PASSES][WORDS];
};
template <int NC, int NR, int LPK>
__device__ __forceinline__ void stage_load(const uint8_t* __restrict__ img, int pitch, int x0, int y0, int r,
                                           staged_block<NC, NR, LPK>& b) {
#pragma unroll
  for (int pass = 0; pass < b.PASSES; ++pass) {
    const int row = r + LPK * pass;
    const bool on = row < NR;
    const uint8_t* src = img + (ptrdiff_t)(y0 + (on ? row : 0)) * pitch + x0;
#pragma unroll
    for (int k = 0; k < NC / 4; ++k) b.v[pass][k] = *(const u32_any*)(src + 4 * k);
    if (NC & 2) b.v[pass][NC / 4] = *(const u16_any*)(src + (NC & ~3));
  }
}
template <int NC, int NR, int LPK, int PITCH>
__device__ __forceinline__ void stage_store(const staged_block<NC, NR, LPK>& b, uint8_t* s, int r) {
#pragma unroll
  for (int pass = 0; pass < b.PASSES; ++pass) {
    const int row = r + LPK * pass;
    if (row < NR) {
      unsigned* d = reinterpret_cast<unsigned*>(s + row * PITCH);
#pragma unroll
      for (int k = 0; k < b.WORDS; ++k) d[k] = b.v[pass][k];
    }
  }
}

template <int NC, int NR, int LPK, int PITCH>
__device__ __forceinline__ void stage16(const uint8_t* __restrict__ img, int pitch, int x0, int y0, uint8_t* s, int r) {
  staged_block<NC, NR, LPK> b;
  stage_load<NC, NR, LPK>(img, pitch, x0, y0, r, b);
  stage_store<NC, NR, LPK, PITCH>(b, s, r);
}

template <int WIN, int LPK, bool FB = false>
__global__ __launch_bounds__(64) void klt_track16_kernel(pyr_t P, const float* __restrict__ prev_xy, int N, const int* __restrict__ d_n, vo_klt_source src, vo_klt_batch B, int max_iter,
                                                         double eps2, float min_eig_thr, float* __restrict__ next_xy,
                                                         uint8_t* __restrict__ status, float* __restrict__ err,
                                                         float fb_thr2, float* __restrict__ fb) {
  typedef klt_rows<WIN> G;
  constexpr int win = WIN, ww = WIN * WIN, RS = G::RS, n1 = G::n1, n3 = G::n3, K16_PITCH = G::PITCH;
  constexpr int KPW = 64 / LPK;                        // keypoints per wave
  static_assert(n1 <= LPK, "one lane per derivative row");
  __shared__ __align__(16) uint8_t smem[KPW * G::SLICE + 16];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * KPW + lane / LPK;
  size_t pyr_off;
  int n_own;
  klt_points<FB>(prev_xy, N, d_n, src, B, next_xy, status, err, fb, pyr_off, n_own);
  if (i >= N) return;                                  // all lanes of a keypoint leave together
  const int r = lane & (LPK - 1);                      // window row of this lane (row WIN only feeds row WIN-1's derivatives)
  uint8_t* s_reg = smem + (lane / LPK) * G::SLICE;
  const int live = r < win ? 1 : 0;
  const int rr = r < win ? r : win - 1;                // row whose pixels this lane reads in the search loop
  const int rd = r < n1 ? r : n1 - 1;                  // derivative row of this lane (lanes past it idle along)

  const float half = (float)(win - 1) * 0.5f;
  const float2 p0 = klt_point_start(prev_xy, src, n_own, i);
  float p0x = p0.x, p0y = p0.y;
  bool ok = true;
  float e_out = 0.f;
  float nx = 0.f, ny = 0.f;
  klt_fb_keep<FB> fwd;                                 // (empty without FB)
  bool back = false;                                   // FB: the second pass (next -> prev) is running

  // Template blocks depend on the previous keypoint only, so the block of level l - 1 is requested
  // while level l is being worked on (tplI holds the block of the level about to start).
  staged_block<n3, n3, LPK> tplI;
  auto request_template = [&](int level) {
    float px, py;
    klt_template_corner(level, p0x, p0y, half, px, py);
    int ipx = (int)floorf(px), ipy = (int)floorf(py);
    ipx = min(max(ipx, -win), P.W[level] - 1);       // (a level whose block would leave the border is skipped below)
    ipy = min(max(ipy, -win), P.H[level] - 1);
    stage_load<n3, n3, LPK>((FB && back ? P.next[level] : P.prev[level]) + pyr_off, P.pitch[level], ipx - 1, ipy - 1, r, tplI);
  };
second_pass:
  request_template(P.n_levels - 1);

  for (int level = P.n_levels - 1; level >= 0; --level) {
    const uint8_t* J = (FB && back ? P.prev[level] : P.next[level]) + pyr_off;
    const int H = P.H[level], W = P.W[level], pitch = P.pitch[level];
    const staged_block<n3, n3, LPK> curI = tplI;
    if (level > 0) request_template(level - 1);
    float qx, qy;
    int ipx, ipy, w00, w01, w10, w11;
    if (!klt_level_entry(level, P.n_levels, p0x, p0y, half, win, W, H, nx, ny, qx, qy, ipx, ipy, w00, w01, w10, w11, ok, e_out))
      continue;
    // (w11 = 2^14 - w00 - w01 - w10 can come out as -1: the packed weights are signed 16-bit halves)
    unsigned wa = ((unsigned)w00 & 0xffffu) | ((unsigned)w01 << 16), wb = ((unsigned)w10 & 0xffffu) | ((unsigned)w11 << 16);

    // the search region around the starting guess is requested now and lands while the template is built
    int rx0, ry0;
    const bool first_in = klt_window_at(qx, qy, win, W, H, rx0, ry0, w00, w01, w10, w11);
    rx0 -= KLT_MARGIN;
    ry0 -= KLT_MARGIN;
    staged_block<RS, RS, LPK> regJ;
    stage_load<RS, RS, LPK>(J, pitch, first_in ? rx0 : 0, first_in ? ry0 : 0, r, regJ);

    // ---- template: image block, Scharr derivatives, interpolated patch (all in registers) ----
    wave_sync();
    stage_store<n3, n3, LPK, K16_PITCH>(curI, s_reg, r);
    wave_sync();
    int tI[win], tX[win], tY[win];
    int a11 = 0, a12 = 0, a22 = 0;   // per-lane partial sums stay below 2^31
    {
      unsigned A0[G::WA], A1[G::WA], A2[G::WA];   // block rows r, r+1, r+2 (n3 bytes each): the rows around derivative row r
      {
        const unsigned* q0 = reinterpret_cast<const unsigned*>(s_reg + rd * K16_PITCH);
#pragma unroll
        for (int k = 0; k < G::WA; ++k) {
          A0[k] = q0[k];
          A1[k] = q0[k + K16_PITCH / 4];
          A2[k] = q0[k + 2 * (K16_PITCH / 4)];
        }
      }
      int cs[n3], cd[n3];             // per column: 3 (a0 + a2) + 10 a1, a2 - a0
#pragma unroll
      for (int c = 0; c < n3; ++c) {
        const int b0 = byte_at(A0, c), b1 = byte_at(A1, c), b2 = byte_at(A2, c);
        cs[c] = (b0 + b2) * 3 + b1 * 10;
        cd[c] = b2 - b0;
      }
      const int gy = ipy + rd;
      const bool row_in = gy >= 0 && gy < H;
      unsigned der[n1], dern[n1];     // (dx & 0xffff) | dy << 16 of derivative rows r and r + 1
#pragma unroll
      for (int x = 0; x < n1; ++x) {
        const int gx = ipx + x;
        int dx = cs[x + 2] - cs[x];
        int dy = (cd[x + 2] + cd[x]) * 3 + cd[x + 1] * 10;
        if (!(row_in && gx >= 0 && gx < W)) {
          dx = 0;
          dy = 0;
        }
        der[x] = ((unsigned)dx & 0xffffu) | ((unsigned)dy << 16);
      }
#pragma unroll
      for (int x = 0; x < n1; ++x)   // lane r reads lane r + 1: row_shl:1 inside a DPP row, wave_shl:1 across the two rows of a keypoint
        dern[x] = LPK == 16 ? (unsigned)__builtin_amdgcn_update_dpp(0, (int)der[x], 0x101, 0xF, 0xF, true)
                            : (unsigned)__builtin_amdgcn_update_dpp(0, (int)der[x], 0x130, 0xF, 0xF, true);
#pragma unroll
      for (int x = 0; x < win; ++x) {
        const int ival = sdot2(pair_at(A1, x + 1), wa, sdot2(pair_at(A2, x + 1), wb, 1 << (W_BITS - 5 - 1))) >> (W_BITS - 5);
        const unsigned dxa = __builtin_amdgcn_perm(der[x + 1], der[x], 0x05040100u);
        const unsigned dya = __builtin_amdgcn_perm(der[x + 1], der[x], 0x07060302u);
        const unsigned dxb = __builtin_amdgcn_perm(dern[x + 1], dern[x], 0x05040100u);
        const unsigned dyb = __builtin_amdgcn_perm(dern[x + 1], dern[x], 0x07060302u);
        const int ix = live * (sdot2(dxa, wa, sdot2(dxb, wb, 1 << (W_BITS - 1))) >> W_BITS);
        const int iy = live * (sdot2(dya, wa, sdot2(dyb, wb, 1 << (W_BITS - 1))) >> W_BITS);
        tI[x] = ival;
        tX[x] = ix;
        tY[x] = iy;
        a11 += ix * ix;
        a12 += ix * iy;
        a22 += iy * iy;
      }
    }
    const float A11 = (float)kp_sum_exact<LPK>(a11) * FLT_SCALE;
    const float A12 = (float)kp_sum_exact<LPK>(a12) * FLT_SCALE;
    const float A22 = (float)kp_sum_exact<LPK>(a22) * FLT_SCALE;
    float D;
    if (!klt_solve(A11, A12, A22, ww, min_eig_thr, level, D, ok)) continue;
    float pdx = 0.f, pdy = 0.f;
    // search region of `next`: the block requested above, if the starting guess lies in the level
    bool staged = false;
    if (first_in) {
      wave_sync();
      stage_store<RS, RS, LPK, K16_PITCH>(regJ, s_reg, r);
      wave_sync();
      staged = true;
    }
    // this lane's two rows of the window at (ix, iy), with the weights packed
    auto window_rows = [&](int ix, int iy, unsigned* B0, unsigned* B1) {
      wa = ((unsigned)w00 & 0xffffu) | ((unsigned)w01 << 16);
      wb = ((unsigned)w10 & 0xffffu) | ((unsigned)w11 << 16);
      if (klt_restage(staged, ix, iy, n1, RS, rx0, ry0)) {
        wave_sync();
        stage16<RS, RS, LPK, K16_PITCH>(J, pitch, rx0, ry0, s_reg, r);
        wave_sync();
      }
      const uint8_t* base = s_reg + (iy - ry0 + rr) * K16_PITCH + (ix - rx0);
      load_row_bytes<n1>(base, B0);
      load_row_bytes<n1>(base + K16_PITCH, B1);
    };
    for (int j = 0; j < max_iter; ++j) {
      int iqx, iqy;
      if (!klt_window_at(qx, qy, win, W, H, iqx, iqy, w00, w01, w10, w11)) {
        if (level == 0) ok = false;
        break;
      }
      unsigned B0[6], B1[6];
      window_rows(iqx, iqy, B0, B1);
      int b1 = 0, b2 = 0;
#pragma unroll
      for (int x = 0; x < win; ++x) {
        const int jv = sdot2(pair_at(B0, x), wa, sdot2(pair_at(B1, x), wb, 1 << (W_BITS - 5 - 1))) >> (W_BITS - 5);
        const int diff = jv - tI[x];
        b1 += diff * tX[x];
        b2 += diff * tY[x];
      }
      const float fb1 = (float)kp_sum_exact<LPK>(b1) * FLT_SCALE;
      const float fb2 = (float)kp_sum_exact<LPK>(b2) * FLT_SCALE;
      if (klt_newton_update(A11, A12, A22, D, fb1, fb2, j, eps2, half, qx, qy, nx, ny, pdx, pdy)) break;
    }
    if (ok && level == 0) {
      int iex, iey;
      if (!klt_window_at(nx - half, ny - half, win, W, H, iex, iey, w00, w01, w10, w11)) {
        ok = false;
        continue;
      }
      unsigned B0[6], B1[6];
      window_rows(iex, iey, B0, B1);
      int sabs = 0;
#pragma unroll
      for (int x = 0; x < win; ++x) {
        const int jv = sdot2(pair_at(B0, x), wa, sdot2(pair_at(B1, x), wb, 1 << (W_BITS - 5 - 1))) >> (W_BITS - 5);
        const int diff = jv - tI[x];
        sabs += diff < 0 ? -diff : diff;
      }
      e_out = (float)kp_sum_i32<LPK>(live * sabs) / (float)(32 * ww);
    }
  }
  // FB: once more, next -> prev, from the forward result as stored.  A lane group whose forward pass failed goes straight
  // on to the kernel's end and waits there while its wave-mates run the pass: the LDS slices are per group, wave_sync()
  // holds back the compiler only, and the window sums stay inside a group's lanes.
  if constexpr (FB) {
    if (klt_fb_turn(fwd, back, p0x, p0y, nx, ny, ok, e_out)) goto second_pass;
  }
  if (r == 0) klt_write<FB>(fwd, nx, ny, ok, e_out, fb_thr2, i, next_xy, status, err, fb);
}

size_t klt_lds_bytes(int win) {
  const int n1 = win + 1, n3 = win + 3, RS = n1 + 2 * KLT_MARGIN;
  const int reg = n3 * n3 > RS * RS ? n3 * n3 : RS * RS;
  return (size_t)((reg + 15) & ~15) + (size_t)(n1 * n1 + 1) * 4 + (size_t)win * win * 8;
}

// ---- the launch ----
// Windows with a row kernel and their lanes per keypoint; a launch tracks 64 / lanes keypoints per workgroup.
// Window 15 has 16 lanes per keypoint (four per wave).  32 lanes per keypoint (two per wave, the upper half of each group
// idle in the row loops, the 18 rows of the template block in one pass instead of two) measured slower: round 3, step
// 87.6 -> 91.3 us at one sequence, the kernel 199 -> 351 us at 16.  17 is the reference's default window (klt.py:29).
struct klt_row_window {
  int win, lanes;
};
constexpr klt_row_window KLT_ROW_WINDOWS[] = {{15, 16}, {17, 32}, {21, 32}};
constexpr int KLT_N_ROW_WINDOWS = (int)(sizeof(KLT_ROW_WINDOWS) / sizeof(KLT_ROW_WINDOWS[0]));

// f(std::integral_constant<int, k>) for the table entry k of `win`; false: the window has none
template <int K = 0, class F>
bool klt_for_row_window(int win, F&& f) {
  if constexpr (K < KLT_N_ROW_WINDOWS) {
    if (win != KLT_ROW_WINDOWS[K].win) return klt_for_row_window<K + 1>(win, f);
    f(std::integral_constant<int, K>());
    return true;
  } else {
    return false;
  }
}
// f(std::bool_constant<FB>): the plain instantiation or the forward-backward one of the same template
template <class F>
void klt_for_fb(bool with_fb, F&& f) {
  if (with_fb) f(std::true_type());
  else f(std::false_type());
}

}  // namespace

extern "C" {

int vo_klt_track_dev(vo_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_prev_pyr, const uint8_t* d_next,
                     const uint8_t* d_next_pyr, int H, int W, int n_levels, const float* d_prev_xy, int N, int win,
                     int max_iter, double eps, double min_eig, float* d_next_xy, uint8_t* d_status, float* d_err) {
  return vo_klt_track_ndev(ctx, d_prev, d_prev_pyr, d_next, d_next_pyr, H, W, n_levels, d_prev_xy, N, nullptr, win,
                           max_iter, eps, min_eig, d_next_xy, d_status, d_err);
}

// fb_max > 0 (+inf allowed); anything else, NaN included, is refused before a byte is written
static bool klt_fb_max_ok(double fb_max) { return fb_max > 0.0; }

int vo_klt_track_fb_dev(vo_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_prev_pyr, const uint8_t* d_next,
                        const uint8_t* d_next_pyr, int H, int W, int n_levels, const float* d_prev_xy, int N, int win,
                        int max_iter, double eps, double min_eig, double fb_max, float* d_next_xy, uint8_t* d_status,
                        float* d_err, float* d_fb) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, klt_fb_max_ok(fb_max), "klt_track_fb: fb_max must be > 0 pixels (+inf allowed), got %g", fb_max);
  VO_REQUIRE(ctx, N <= 0 || d_fb, "klt_track_fb: null pointer");
  return vo_klt_track_ndev(ctx, d_prev, d_prev_pyr, d_next, d_next_pyr, H, W, n_levels, d_prev_xy, N, nullptr, win,
                           max_iter, eps, min_eig, d_next_xy, d_status, d_err, nullptr, nullptr, fb_max, d_fb);
}

}  // extern "C"

// Pipeline-internal form: at most N keypoints, the actual count is read from *d_n when the kernel runs.
int vo_klt_track_ndev(vo_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_prev_pyr, const uint8_t* d_next,
                      const uint8_t* d_next_pyr, int H, int W, int n_levels, const float* d_prev_xy, int N,
                      const int32_t* d_n, int win, int max_iter, double eps, double min_eig, float* d_next_xy,
                      uint8_t* d_status, float* d_err, const vo_klt_source* src_in, const vo_klt_batch* batch, double fb_max,
                      float* d_fb) {
  if (!ctx) return VO_EINVAL;
  const bool with_fb = d_fb != nullptr;                // the forward-backward launch (fb_max = 0, d_fb = null: the plain one)
  VO_REQUIRE(ctx, !with_fb || fb_max > 0.0, "klt_track_fb: fb_max must be > 0 pixels (+inf allowed), got %g", fb_max);
  VO_REQUIRE(ctx, with_fb || fb_max == 0.0, "klt_track_fb: fb_max without an fb array");
  const float thr2 = with_fb ? (float)(fb_max * fb_max) : 0.f;
  const vo_klt_source src = src_in ? *src_in : vo_klt_source();
  const vo_klt_batch B = batch ? *batch : vo_klt_batch();
  const int S = B.S > 0 ? B.S : 1;
  VO_REQUIRE(ctx, N >= 0, "klt_track: bad N");
  if (N == 0) return VO_OK;
  VO_REQUIRE(ctx, d_prev && d_next && d_prev_xy && d_next_xy && d_status && d_err, "klt_track: null pointer");
  VO_REQUIRE(ctx, n_levels >= 1 && n_levels <= MAX_LEVELS, "klt_track: n_levels must be in 1..%d", MAX_LEVELS);
  VO_REQUIRE(ctx, d_prev_pyr && d_next_pyr, "klt_track: pyramid buffers missing");
  VO_REQUIRE(ctx, win >= 3 && win <= MAX_WIN, "klt_track: window must be in 3..%d", MAX_WIN);
  VO_REQUIRE(ctx, H > 0 && W > 0, "klt_track: bad image size");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  pyr_t P;
  memset(&P, 0, sizeof(P));
  P.n_levels = n_levels;
  {
    // every level, level 0 included, is read from the bordered copies vo_pyramid_build_dev made
    size_t off = 0;
    int h = H, w = W;
    for (int l = 0; l < n_levels; ++l) {
      P.H[l] = h;
      P.W[l] = w;
      P.pitch[l] = pyr_pitch(w);
      const size_t origin = off + (size_t)PYR_PAD * P.pitch[l] + PYR_PAD;
      P.prev[l] = d_prev_pyr + origin;
      P.next[l] = d_next_pyr + origin;
      off += pyr_level_bytes(h, w);
      h = (h + 1) / 2;
      w = (w + 1) / 2;
    }
  }
  if (max_iter < 0) max_iter = 0;
  if (max_iter > 100) max_iter = 100;
  if (eps < 0) eps = 0;
  if (eps > 10) eps = 10;
  {
    vo_prof_scope ps(ctx, VO_K_KLT_TRACK);
    const int lds_wave = (int)((klt_lds_bytes(win) + 15) & ~size_t(15));
    const size_t lds = (size_t)lds_wave * KLT_WAVES;
    hipStream_t st = ctx->stream;
    const float me = (float)min_eig;
    const dim3 kgrid(vo_cdiv(N, KLT_WAVES), S), kblock(64 * KLT_WAVES);
    // (thr2 = 0 and d_fb = null without the check: the plain launch as it always was)
    klt_for_fb(with_fb, [&](auto fb_flag) {
      constexpr bool FB = decltype(fb_flag)::value;
      const bool rows = klt_for_row_window(win, [&](auto k) {
        constexpr klt_row_window R = KLT_ROW_WINDOWS[decltype(k)::value];
        vo_launch_stop(ctx, klt_track16_kernel<R.win, R.lanes, FB>, dim3(vo_cdiv(N, 64 / R.lanes), S), dim3(64), 0, st, P, d_prev_xy,
                       N, d_n, src, B, max_iter, eps * eps, me, d_next_xy, d_status, d_err, thr2, d_fb);
      });
      if (!rows)
        vo_launch_stop(ctx, klt_track_kernel<0, FB>, kgrid, kblock, lds, st, P, d_prev_xy, N, d_n, src, B, win, max_iter, eps * eps,
                       me, d_next_xy, d_status, d_err, lds_wave, thr2, d_fb);
    });
  }
  return vo_check_launch(ctx, "klt_track_kernel");
}

extern "C" {

// fb == null: the plain tracker; otherwise the forward-backward one with fb_max
static int klt_track_host(vo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int H, int W, const float* prev_xy, int N,
                          int win, int max_level, int max_iter, double eps, double min_eig, double fb_max, float* next_xy,
                          uint8_t* status, float* err, float* fb) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, N >= 0, "klt_track: bad N");
  if (N == 0) return VO_OK;
  VO_REQUIRE(ctx, prev && next && prev_xy && next_xy && status && err, "klt_track: null pointer");
  VO_REQUIRE(ctx, H > 0 && W > 0 && max_level >= 0, "klt_track: bad arguments");
  VO_REQUIRE(ctx, win >= 3 && win <= MAX_WIN, "klt_track: window must be in 3..%d", MAX_WIN);
  const int nl = vo_klt_num_levels(H, W, win, max_level);
  const size_t px = (size_t)H * W, pb = vo_pyramid_bytes(H, W, nl);
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, ctx->img, px));
  VO_TRY(vo_ensure(ctx, ctx->img2, px));
  VO_TRY(vo_ensure(ctx, s[8], pb));
  VO_TRY(vo_ensure(ctx, s[9], pb));
  VO_TRY(vo_ensure(ctx, s[10], (size_t)N * 8));
  VO_TRY(vo_ensure(ctx, s[11], (size_t)N * 8));
  VO_TRY(vo_ensure(ctx, s[12], (size_t)N));
  VO_TRY(vo_ensure(ctx, s[13], (size_t)N * 4));
  if (fb) VO_TRY(vo_ensure(ctx, s[14], (size_t)N * 4));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, prev, px, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img2.p, next, px, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[10].p, prev_xy, (size_t)N * 8, hipMemcpyHostToDevice, st));
  VO_TRY(vo_pyramid_build_dev(ctx, (const uint8_t*)ctx->img.p, H, W, nl, (uint8_t*)s[8].p));
  VO_TRY(vo_pyramid_build_dev(ctx, (const uint8_t*)ctx->img2.p, H, W, nl, (uint8_t*)s[9].p));
  VO_TRY(vo_klt_track_ndev(ctx, (const uint8_t*)ctx->img.p, (const uint8_t*)s[8].p, (const uint8_t*)ctx->img2.p,
                           (const uint8_t*)s[9].p, H, W, nl, (const float*)s[10].p, N, nullptr, win, max_iter, eps, min_eig,
                           (float*)s[11].p, (uint8_t*)s[12].p, (float*)s[13].p, nullptr, nullptr, fb ? fb_max : 0.0,
                           fb ? (float*)s[14].p : nullptr));
  VO_HIP_TRY(ctx, hipMemcpyAsync(next_xy, s[11].p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(status, s[12].p, (size_t)N, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(err, s[13].p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  if (fb) VO_HIP_TRY(ctx, hipMemcpyAsync(fb, s[14].p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_klt_track(vo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int H, int W, const float* prev_xy, int N,
                 int win, int max_level, int max_iter, double eps, double min_eig, float* next_xy, uint8_t* status,
                 float* err) {
  return klt_track_host(ctx, prev, next, H, W, prev_xy, N, win, max_level, max_iter, eps, min_eig, 0.0, next_xy, status, err,
                        nullptr);
}

int vo_klt_track_fb(vo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int H, int W, const float* prev_xy, int N,
                    int win, int max_level, int max_iter, double eps, double min_eig, double fb_max, float* next_xy,
                    uint8_t* status, float* err, float* fb) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, klt_fb_max_ok(fb_max), "klt_track_fb: fb_max must be > 0 pixels (+inf allowed), got %g", fb_max);
  VO_REQUIRE(ctx, N <= 0 || fb, "klt_track_fb: null pointer");
  return klt_track_host(ctx, prev, next, H, W, prev_xy, N, win, max_level, max_iter, eps, min_eig, fb_max, next_xy, status,
                        err, fb);
}

}  // extern "C"
