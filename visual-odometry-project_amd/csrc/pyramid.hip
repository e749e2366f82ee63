// Image pyramid for the pyramidal Lucas-Kanade tracker (klt.hip), for gfx950.
//
// The arithmetic is restated in oracle/csrc/klt.c; this file is the device version of the same definition:
//   pyrDown   5-tap [1 4 6 4 1] separable, reflect-101, (sum + 128) >> 8
// Every level is stored with its reflected border (pyramid_device.h).
#include "pyramid_device.h"

#pragma clang fp contract(off)

namespace {

// One thread per pixel of the padded destination level: the border pixels take the value of
// the interior pixel they mirror.  src points at the interior origin of the level above.
__global__ __launch_bounds__(256) void pyr_down_kernel(const uint8_t* __restrict__ src, int spitch, int H, int W,
                                                       uint8_t* __restrict__ dst, int dpitch, int Hd, int Wd,
                                                       size_t seq_stride) {
  src += (size_t)blockIdx.z * seq_stride;          // several sequences per launch: both levels live in the
  dst += (size_t)blockIdx.z * seq_stride;          // sequence's pyramid buffer
  const int xp = blockIdx.x * 64 + (threadIdx.x & 63);
  const int yp = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (xp >= Wd + 2 * PYR_PAD || yp >= Hd + 2 * PYR_PAD) return;
  const int x = reflect101(xp - PYR_PAD, Wd), y = reflect101(yp - PYR_PAD, Hd);
  int xs[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) xs[i] = reflect101(2 * x + i - 2, W);
  int sum = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uint8_t* row = src + (size_t)reflect101(2 * y + j - 2, H) * spitch;
    const int r = row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]];
    const int wj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
    sum += wj * r;
  }
  dst[(size_t)yp * dpitch + xp] = (uint8_t)((sum + 128) >> 8);
}

// level 0: the frame itself with its reflected border
__global__ __launch_bounds__(256) void pad_reflect_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                          uint8_t* __restrict__ dst, int dpitch, size_t img_stride,
                                                          size_t pyr_stride) {
  src += (size_t)blockIdx.z * img_stride;
  dst += (size_t)blockIdx.z * pyr_stride;
  const int xp = blockIdx.x * 64 + (threadIdx.x & 63);
  const int yp = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (xp >= W + 2 * PYR_PAD || yp >= H + 2 * PYR_PAD) return;
  dst[(size_t)yp * dpitch + xp] = src[(size_t)reflect101(yp - PYR_PAD, H) * W + reflect101(xp - PYR_PAD, W)];
}

// v = interior pixel (x, y) of a W x H level -> its place in the bordered buffer and every border
// place that mirrors onto it (one reflection: needs min(W, H) > PYR_PAD)
__device__ __forceinline__ void store_with_mirrors(uint8_t* __restrict__ dst, int pitch, int H, int W, int x, int y,
                                                   uint8_t v, bool skip_own = false) {
  int xs[3], ys[3];
  int nx = 1, ny = 1;
  xs[0] = x + PYR_PAD;
  ys[0] = y + PYR_PAD;
  if (x >= 1 && x <= PYR_PAD) xs[nx++] = PYR_PAD - x;
  if (x >= W - 1 - PYR_PAD && x <= W - 2) xs[nx++] = PYR_PAD + 2 * (W - 1) - x;
  if (y >= 1 && y <= PYR_PAD) ys[ny++] = PYR_PAD - y;
  if (y >= H - 1 - PYR_PAD && y <= H - 2) ys[ny++] = PYR_PAD + 2 * (H - 1) - y;
  for (int j = 0; j < ny; ++j)
    for (int i = (j == 0 && skip_own) ? 1 : 0; i < nx; ++i) dst[(size_t)ys[j] * pitch + xs[i]] = v;
}

// 5x5 [1 4 6 4 1]^2 tap at (2x, 2y) of an unbordered W x H image, reflect-101
__device__ __forceinline__ int pyr_tap(const uint8_t* __restrict__ src, int pitch, int H, int W, int x, int y) {
  int xs[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) xs[i] = reflect101(2 * x + i - 2, W);
  int sum = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uint8_t* row = src + (size_t)reflect101(2 * y + j - 2, H) * pitch;
    const int r = row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]];
    const int wj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
    sum += wj * r;
  }
  return (sum + 128) >> 8;
}

// Levels 0, 1 and 2 of the bordered pyramid in ONE launch (three dependent launches were
// 22 us of the step's critical path).  No workgroup waits for another:
//   * the first nB workgroups each produce a 16x16 tile of level 2 from a 35x35 patch of level 1
//     that they compute for themselves in LDS (straight from the frame);
//   * the others produce level 1 (one pixel per thread) and copy the 2x2 frame pixels under it
//     into the bordered level 0.
// Border pixels are written by the thread that owns the interior pixel they mirror.
__global__ __launch_bounds__(256) void pyramid3_kernel(const uint8_t* __restrict__ src, int H0, int W0,
                                                       uint8_t* __restrict__ d0, int p0, uint8_t* __restrict__ d1,
                                                       int p1, int H1, int W1, uint8_t* __restrict__ d2, int p2,
                                                       int H2, int W2, int nB, int tiles2_x, int blocks1_x,
                                                       size_t img_stride, size_t pyr_stride) {
  src += (size_t)blockIdx.y * img_stride;            // several sequences per launch: grid.y = sequence
  d0 += (size_t)blockIdx.y * pyr_stride;
  d1 += (size_t)blockIdx.y * pyr_stride;
  d2 += (size_t)blockIdx.y * pyr_stride;
  __shared__ uint8_t s_l0[73 * 76];   // frame patch under the level-1 patch
  __shared__ uint8_t s_l1[35 * 36];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nB) {
    const int tx = (int)blockIdx.x % tiles2_x, ty = (int)blockIdx.x / tiles2_x;
    const int x2a = tx * 16, y2a = ty * 16;
    // Level-1 patch entry (ly, lx) stands for level-1 coordinate (2 y2a - 2 + ly, 2 x2a - 2 + lx),
    // reflected into level 1 where that falls outside.  For every level-2 pixel this tile stores
    // the reflected coordinates stay inside [lo, hi], so the frame pixels under them are one
    // contiguous patch (reflected at the frame's own edges), staged once.
    const int ax = 2 * x2a - 2, ay = 2 * y2a - 2;
    const int lox = max(ax, 0), hix = min(ax + 34, W1 - 1);
    const int loy = max(ay, 0), hiy = min(ay + 34, H1 - 1);
    const int fx0 = 2 * lox - 2, fy0 = 2 * loy - 2;             // frame coordinate of s_l0[0][0]
    const int fw = 2 * (hix - lox) + 5, fh = 2 * (hiy - loy) + 5;
    {
      // all loads of the patch go out before the first byte is stored (one round trip, not 21)
      constexpr int PER = (73 * 73 + 255) / 256;
      uint8_t v[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int i = tid + k * 256;
        const int ly = i / fw, lx = i - ly * fw;
        int gx = fx0 + lx, gy = fy0 + ly;                       // at most 2 pixels outside: one reflection
        gx = gx < 0 ? -gx : (gx >= W0 ? 2 * (W0 - 1) - gx : gx);
        gy = gy < 0 ? -gy : (gy >= H0 ? 2 * (H0 - 1) - gy : gy);
        gx = min(max(gx, 0), W0 - 1);
        gy = min(max(gy, 0), H0 - 1);                           // (entries past fw * fh: any valid address)
        v[k] = src[(size_t)gy * W0 + gx];
      }
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int i = tid + k * 256;
        const int ly = i / fw, lx = i - ly * fw;
        if (i < fw * fh) s_l0[ly * 76 + lx] = v[k];
      }
    }
    __syncthreads();
    for (int i = tid; i < 35 * 35; i += 256) {
      const int ly = i / 35, lx = i - ly * 35;
      int x1 = reflect101(ax + lx, W1), y1 = reflect101(ay + ly, H1);
      x1 = min(max(x1, lox), hix);                              // (only entries no stored pixel uses are clamped)
      y1 = min(max(y1, loy), hiy);
      const uint8_t* q = s_l0 + (2 * (y1 - loy)) * 76 + 2 * (x1 - lox);
      int sum = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const uint8_t* row = q + j * 76;
        const int r = row[0] + 4 * row[1] + 6 * row[2] + 4 * row[3] + row[4];
        const int wj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
        sum += wj * r;
      }
      s_l1[ly * 36 + lx] = (uint8_t)((sum + 128) >> 8);
    }
    __syncthreads();
    const int lx = tid & 15, ly = tid >> 4;
    const int x2 = x2a + lx, y2 = y2a + ly;
    if (x2 < W2 && y2 < H2) {
      int sum = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const uint8_t* row = s_l1 + (2 * ly + j) * 36 + 2 * lx;
        const int r = row[0] + 4 * row[1] + 6 * row[2] + 4 * row[3] + row[4];
        const int wj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
        sum += wj * r;
      }
      store_with_mirrors(d2, p2, H2, W2, x2, y2, (uint8_t)((sum + 128) >> 8));
    }
    return;
  }
  // level 1: a 32x8 tile per workgroup from a 67x19 frame patch staged once; the patch's centre
  // is also what goes into the bordered level 0
  const int blk = (int)blockIdx.x - nB;
  const int x1a = (blk % blocks1_x) * 32, y1a = (blk / blocks1_x) * 8;
  const int fx0 = 2 * x1a - 2, fy0 = 2 * y1a - 2;
  {
    constexpr int PER = (67 * 19 + 255) / 256;
    uint8_t v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      const int ly = i / 67, lx = i - ly * 67;
      int gx = fx0 + lx, gy = fy0 + ly;
      gx = gx < 0 ? -gx : (gx >= W0 ? 2 * (W0 - 1) - gx : gx);     // at most 2 pixels outside (tiles that stick out
      gy = gy < 0 ? -gy : (gy >= H0 ? 2 * (H0 - 1) - gy : gy);     //  further only feed pixels that are not stored)
      gx = min(max(gx, 0), W0 - 1);
      gy = min(max(gy, 0), H0 - 1);
      v[k] = src[(size_t)gy * W0 + gx];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      const int ly = i / 67, lx = i - ly * 67;
      if (i < 67 * 19) s_l0[ly * 76 + lx] = v[k];
    }
  }
  __syncthreads();
  const int lx = tid & 31, ly = tid >> 5;
  const int x1 = x1a + lx, y1 = y1a + ly;
  if (x1 >= W1 || y1 >= H1) return;
  {
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint8_t* row = s_l0 + (2 * ly + j) * 76 + 2 * lx;
      const int r = row[0] + 4 * row[1] + 6 * row[2] + 4 * row[3] + row[4];
      const int wj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
      sum += wj * r;
    }
    store_with_mirrors(d1, p1, H1, W1, x1, y1, (uint8_t)((sum + 128) >> 8));
  }
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int x0 = 2 * x1, y0 = 2 * y1 + dy;
    if (y0 >= H0) continue;
    const uint8_t v0 = s_l0[(2 * ly + 2 + dy) * 76 + 2 * lx + 2], v1 = s_l0[(2 * ly + 2 + dy) * 76 + 2 * lx + 3];
    uint8_t* own = d0 + (size_t)(y0 + PYR_PAD) * p0 + (x0 + PYR_PAD);       // even offset: one 16-bit store for the pair
    if (x0 + 1 < W0) *reinterpret_cast<unsigned short*>(own) = (unsigned short)(v0 | (v1 << 8));
    else *own = v0;
    store_with_mirrors(d0, p0, H0, W0, x0, y0, v0, true);                    // border copies only
    if (x0 + 1 < W0) store_with_mirrors(d0, p0, H0, W0, x0 + 1, y0, v1, true);
  }
}

// ---- the same three levels, word-wide: one workgroup per 64x32 tile of level 1 ----
// pyramid3_kernel moves single bytes (global loads, LDS, stores) and spends a workgroup per 16x16 tile of level
// 2 on a 35x35 level-1 patch of its own: 20 us per frame however many frames a launch holds.  Here a workgroup
//   A  stages the frame patch under its level-1 tile + the 2-pixel ring level 2 needs (144 x 75 bytes) as aligned
//      dwords, every load issued before the first LDS store; out-of-frame bytes are reflected while staging;
//   B  copies the patch's centre into the bordered level 0 (dword stores);
//   C  makes the 68x36 level-1 region, two neighbours per work item from three dwords per patch row, into LDS;
//   D  stores its 64x32 centre to level 1 (dwords) and E makes the 32x16 tile of level 2 from the region.
// Border pixels are written by the owner of the interior pixel they mirror (edge tiles only).
// Needs W % 4 == 0 and a 4-byte aligned frame (the host picks the byte kernel otherwise).
// Tile size: 64x32 when a launch holds several frames (less halo work per pixel), 32x16 for a single frame (four
// times the workgroups, each a third of the latency: the launch is on the tracker's critical path then).

// seven bytes starting at byte 2 of dword a: two neighbouring 5-tap row sums
__device__ __forceinline__ void tap_pair(unsigned a, unsigned b, unsigned c, int& ra, int& rb) {
  // (1, 4, 6, 4) . four bytes is one v_dot4_u32_u8, the fifth tap its addend: five instructions for the pair
  ra = (int)__builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(b, a, 2), 0x04060401u, (b >> 16) & 255u, false);
  rb = (int)__builtin_amdgcn_udot4(b, 0x04060401u, c & 255u, false);
}

__device__ __forceinline__ int reflect_once(int c, int n) {
  c = c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c);
  return min(max(c, 0), n - 1);
}

template <int PT_X, int PT_Y>
__global__ __launch_bounds__(256) void pyramid3_tiled_kernel(const uint8_t* __restrict__ src, int H0, int W0,
                                                             uint8_t* __restrict__ d0, int p0, uint8_t* __restrict__ d1,
                                                             int p1, int H1, int W1, uint8_t* __restrict__ d2, int p2,
                                                             int H2, int W2, int tiles_x, size_t img_stride,
                                                             size_t pyr_stride) {
  constexpr int PT_RX = PT_X + 4, PT_RY = PT_Y + 4;   // level-1 region (ring of 2)
  constexpr int PT_FD = (2 * PT_X + 16) / 4;          // frame patch: dwords per row (virtual columns 2 x1a - 8 ..)
  constexpr int PT_FR = 2 * PT_Y + 11;                // frame patch rows (virtual rows 2 y1a - 6 ..)
  constexpr int PT_L1P = PT_RX + 4;                   // level-1 region pitch in bytes; entry lx sits at byte lx + 2
  static_assert(PT_X % 4 == 0 && PT_Y % 2 == 0, "tile: whole dwords per row, whole level-2 rows");
  src += (size_t)blockIdx.y * img_stride;
  d0 += (size_t)blockIdx.y * pyr_stride;
  d1 += (size_t)blockIdx.y * pyr_stride;
  d2 += (size_t)blockIdx.y * pyr_stride;
  __shared__ unsigned s_f[PT_FR * PT_FD];
  __shared__ __attribute__((aligned(4))) uint8_t s_l1[PT_RY * PT_L1P];
  const int tid = threadIdx.x;
  const int tile = (int)vo_xcd_tile(blockIdx.x, gridDim.x);
  const int x1a = (tile % tiles_x) * PT_X, y1a = (tile / tiles_x) * PT_Y;
  const int gx0 = 2 * x1a - 8, gy0 = 2 * y1a - 6;
  // ---- A: frame patch ----
  {
    constexpr int PER = (PT_FR * PT_FD + 255) / 256;
    unsigned v[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      const int r = i / PT_FD, d = i - r * PT_FD;
      const int gy = reflect_once(gy0 + r, H0);
      const int gx = gx0 + 4 * d;
      const uint8_t* row = src + (size_t)gy * W0;
      if (gx >= 0 && gx + 3 < W0) {
        v[k] = *reinterpret_cast<const unsigned*>(row + gx);
      } else {
        unsigned w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= (unsigned)row[reflect_once(gx + b, W0)] << (8 * b);
        v[k] = w;
      }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      if (i < PT_FR * PT_FD) s_f[i] = v[k];
    }
  }
  __syncthreads();
  // ---- B: level 0 = the patch's centre (rows 6 .., dwords 2 ..) ----
  {
    const bool edge0 = 2 * x1a <= PYR_PAD || 2 * x1a + 2 * PT_X >= W0 - 1 - PYR_PAD || 2 * y1a <= PYR_PAD ||
                       2 * y1a + 2 * PT_Y >= H0 - 1 - PYR_PAD;
    for (int i = tid; i < 2 * PT_Y * (2 * PT_X / 4); i += 256) {
      const int r = i / (2 * PT_X / 4), d = i - r * (2 * PT_X / 4);
      const int y0 = 2 * y1a + r, x0 = 2 * x1a + 4 * d;
      if (y0 >= H0 || x0 >= W0) continue;                       // (W0 % 4 == 0: a dword is inside or outside)
      const unsigned w = s_f[(r + 6) * PT_FD + d + 2];
      *reinterpret_cast<unsigned*>(d0 + (size_t)(y0 + PYR_PAD) * p0 + x0 + PYR_PAD) = w;
      if (edge0) {
#pragma unroll
        for (int b = 0; b < 4; ++b) store_with_mirrors(d0, p0, H0, W0, x0 + b, y0, (uint8_t)(w >> (8 * b)), true);
      }
    }
  }
  // ---- C: level-1 region ----
  {
    const int lox = max(x1a - 2, 0), hix = min(x1a + PT_X + 1, W1 - 1);
    const int loy = max(y1a - 2, 0), hiy = min(y1a + PT_Y + 1, H1 - 1);
    const bool plain_x = x1a - 2 >= 0 && x1a + PT_X + 1 < W1;   // no reflection along x: neighbours are neighbours
    for (int i = tid; i < PT_RY * (PT_RX / 2); i += 256) {
      const int ly = i / (PT_RX / 2), j = i - ly * (PT_RX / 2);
      int yr = reflect101(y1a - 2 + ly, H1);
      yr = min(max(yr, loy), hiy);                              // (only entries no stored pixel uses are clamped)
      const unsigned* prow = s_f + (2 * (yr - y1a) + 4) * PT_FD;
      int sa = 0, sb = 0;
      if (plain_x) {
#pragma unroll
        for (int jj = 0; jj < 5; ++jj) {
          const unsigned* q = prow + jj * PT_FD + j;
          int ra, rb;
          tap_pair(q[0], q[1], q[2], ra, rb);
          const int wj = (jj == 0 || jj == 4) ? 1 : ((jj == 2) ? 6 : 4);
          sa += wj * ra;
          sb += wj * rb;
        }
      } else {
        const uint8_t* pb = reinterpret_cast<const uint8_t*>(prow);
        int xa = reflect101(x1a - 2 + 2 * j, W1), xb = reflect101(x1a - 1 + 2 * j, W1);
        xa = min(max(xa, lox), hix);
        xb = min(max(xb, lox), hix);
        const uint8_t* qa = pb + 2 * (xa - x1a) + 6;
        const uint8_t* qb = pb + 2 * (xb - x1a) + 6;
#pragma unroll
        for (int jj = 0; jj < 5; ++jj) {
          const uint8_t* ra = qa + jj * PT_FD * 4;
          const uint8_t* rb = qb + jj * PT_FD * 4;
          const int wj = (jj == 0 || jj == 4) ? 1 : ((jj == 2) ? 6 : 4);
          sa += wj * (ra[0] + 4 * ra[1] + 6 * ra[2] + 4 * ra[3] + ra[4]);
          sb += wj * (rb[0] + 4 * rb[1] + 6 * rb[2] + 4 * rb[3] + rb[4]);
        }
      }
      const unsigned va = (unsigned)((sa + 128) >> 8), vb = (unsigned)((sb + 128) >> 8);
      *reinterpret_cast<unsigned short*>(s_l1 + ly * PT_L1P + 2 + 2 * j) = (unsigned short)(va | (vb << 8));
    }
  }
  __syncthreads();
  // ---- D: level 1 = the region's centre (entries 2 .., bytes 4 ..) ----
  {
    const bool edge1 = x1a <= PYR_PAD || x1a + PT_X >= W1 - 1 - PYR_PAD || y1a <= PYR_PAD || y1a + PT_Y >= H1 - 1 - PYR_PAD;
    for (int i = tid; i < PT_Y * (PT_X / 4); i += 256) {
      const int r = i / (PT_X / 4), d = i - r * (PT_X / 4);
      const int y1 = y1a + r, x1 = x1a + 4 * d;
      if (y1 >= H1 || x1 >= W1) continue;
      const unsigned w = *reinterpret_cast<const unsigned*>(s_l1 + (r + 2) * PT_L1P + 4 + 4 * d);
      uint8_t* own = d1 + (size_t)(y1 + PYR_PAD) * p1 + x1 + PYR_PAD;
      if (x1 + 3 < W1) {
        *reinterpret_cast<unsigned*>(own) = w;
      } else {
        for (int b = 0; x1 + b < W1; ++b) own[b] = (uint8_t)(w >> (8 * b));
      }
      if (edge1) {
        for (int b = 0; b < 4 && x1 + b < W1; ++b) store_with_mirrors(d1, p1, H1, W1, x1 + b, y1, (uint8_t)(w >> (8 * b)), true);
      }
    }
  }
  // ---- E: level 2 from the region: pixel (x1a / 2 + lx, y1a / 2 + ly) taps region entries 2 lx .. 2 lx + 4 ----
  for (int i = tid; i < (PT_Y / 2) * (PT_X / 4); i += 256) {
    const int ly = i / (PT_X / 4), j = i - ly * (PT_X / 4);
    const int x2 = x1a / 2 + 2 * j, y2 = y1a / 2 + ly;
    if (x2 < W2 && y2 < H2) {
      int sa = 0, sb = 0;
#pragma unroll
      for (int jj = 0; jj < 5; ++jj) {
        const unsigned* q = reinterpret_cast<const unsigned*>(s_l1 + (2 * ly + jj) * PT_L1P) + j;
        int ra, rb;
        tap_pair(q[0], q[1], q[2], ra, rb);
        const int wj = (jj == 0 || jj == 4) ? 1 : ((jj == 2) ? 6 : 4);
        sa += wj * ra;
        sb += wj * rb;
      }
      store_with_mirrors(d2, p2, H2, W2, x2, y2, (uint8_t)((sa + 128) >> 8));
      if (x2 + 1 < W2) store_with_mirrors(d2, p2, H2, W2, x2 + 1, y2, (uint8_t)((sb + 128) >> 8));
    }
  }
}

}  // namespace

extern "C" {

int vo_klt_num_levels(int H, int W, int win, int max_level) {
  // levels OpenCV's pyramid builder keeps: stop when the next level is not larger than the window
  int levels = 1, h = H, w = W;
  for (int l = 0; l < max_level && levels < MAX_LEVELS; ++l) {
    h = (h + 1) / 2;
    w = (w + 1) / 2;
    if (w <= win || h <= win) break;
    ++levels;
  }
  return levels;
}

size_t vo_pyramid_bytes(int H, int W, int n_levels) {
  size_t total = 0;
  int h = H, w = W;
  for (int l = 0; l < n_levels; ++l) {
    total += pyr_level_bytes(h, w);
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  return total ? total : 256;
}

// d_pyr receives levels 0 .. n_levels-1 back to back, each with its reflected border (see pyr_t)
int vo_pyramid_build_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, int n_levels, uint8_t* d_pyr) {
  return vo_pyramid_build_batch_dev(ctx, d_img, 0, 1, H, W, n_levels, d_pyr, 0);
}

}  // extern "C"

// S frames (d_img + s * img_stride) -> S pyramids (d_pyr + s * pyr_stride), every launch once for all sequences
int vo_pyramid_build_batch_dev(vo_ctx* ctx, const uint8_t* d_img, size_t img_stride, int S, int H, int W, int n_levels,
                               uint8_t* d_pyr, size_t pyr_stride) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, S >= 1 && S <= 65535, "pyramid_build: bad sequence count");
  VO_REQUIRE(ctx, d_img && d_pyr, "pyramid_build: null pointer");
  VO_REQUIRE(ctx, H > 0 && W > 0 && n_levels >= 1 && n_levels <= MAX_LEVELS, "pyramid_build: bad arguments");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int h1 = (H + 1) / 2, w1 = (W + 1) / 2, h2 = (h1 + 1) / 2, w2 = (w1 + 1) / 2;
  int first_plain = 1;              // first level the per-level kernel still has to make
  const uint8_t* src = d_img;       // interior origin and pitch of the level above it
  int spitch = W, h = H, w = W;
  uint8_t* dst = d_pyr + pyr_level_bytes(H, W);
  if (n_levels >= 3 && h2 > PYR_PAD && w2 > PYR_PAD) {
    // levels 0..2 in one launch
    uint8_t* d1 = dst;
    uint8_t* d2 = d1 + pyr_level_bytes(h1, w1);
    if (W % 4 == 0 && ((uintptr_t)d_img & 3) == 0 && (img_stride & 3) == 0 && (pyr_stride & 3) == 0 && ((uintptr_t)d_pyr & 3) == 0) {
      vo_prof_scope ps(ctx, VO_K_PYR_DOWN);
      static const int forced = getenv("VO_PYR_TILE") ? atoi(getenv("VO_PYR_TILE")) : 0;     // tests: 64 / 32
      if (forced == 64 || (forced != 32 && (long)S * vo_cdiv(w1, 64) * vo_cdiv(h1, 32) >= 1024)) {
        const int tiles_x = vo_cdiv(w1, 64);
        hipLaunchKernelGGL((pyramid3_tiled_kernel<64, 32>), dim3(tiles_x * vo_cdiv(h1, 32), S), dim3(256), 0, ctx->stream,
                           d_img, H, W, d_pyr, pyr_pitch(W), d1, pyr_pitch(w1), h1, w1, d2, pyr_pitch(w2), h2, w2, tiles_x,
                           img_stride, pyr_stride);
      } else {
        const int tiles_x = vo_cdiv(w1, 32);
        hipLaunchKernelGGL((pyramid3_tiled_kernel<32, 16>), dim3(tiles_x * vo_cdiv(h1, 16), S), dim3(256), 0, ctx->stream,
                           d_img, H, W, d_pyr, pyr_pitch(W), d1, pyr_pitch(w1), h1, w1, d2, pyr_pitch(w2), h2, w2, tiles_x,
                           img_stride, pyr_stride);
      }
    } else {
      const int tiles2_x = vo_cdiv(w2, 16), nB = tiles2_x * vo_cdiv(h2, 16);
      const int blocks1_x = vo_cdiv(w1, 32), nA = blocks1_x * vo_cdiv(h1, 8);
      vo_prof_scope ps(ctx, VO_K_PYR_DOWN);
      hipLaunchKernelGGL(pyramid3_kernel, dim3(nB + nA, S), dim3(256), 0, ctx->stream, d_img, H, W, d_pyr, pyr_pitch(W), d1,
                         pyr_pitch(w1), h1, w1, d2, pyr_pitch(w2), h2, w2, nB, tiles2_x, blocks1_x, img_stride, pyr_stride);
    }
    VO_TRY(vo_check_launch(ctx, "pyramid3_kernel"));
    first_plain = 3;
    src = d2 + (size_t)PYR_PAD * pyr_pitch(w2) + PYR_PAD;
    spitch = pyr_pitch(w2);
    dst = d2 + pyr_level_bytes(h2, w2);
    h = h2;
    w = w2;
  } else {
    vo_prof_scope ps(ctx, VO_K_PYR_DOWN);
    hipLaunchKernelGGL(pad_reflect_kernel, dim3(vo_cdiv(W + 2 * PYR_PAD, 64), vo_cdiv(H + 2 * PYR_PAD, 4), S), dim3(256), 0,
                       ctx->stream, d_img, H, W, d_pyr, pyr_pitch(W), img_stride, pyr_stride);
    // (the next level reads the bordered copy of level 0, which lives in the sequence's pyramid buffer like every
    //  other level: same pixels as the frame, one stride for source and destination)
    src = d_pyr + (size_t)PYR_PAD * pyr_pitch(W) + PYR_PAD;
    spitch = pyr_pitch(W);
  }
  VO_TRY(vo_check_launch(ctx, "pad_reflect_kernel"));
  for (int l = first_plain; l < n_levels; ++l) {
    const int hd = (h + 1) / 2, wd = (w + 1) / 2;
    const int dpitch = pyr_pitch(wd);
    {
      vo_prof_scope ps(ctx, VO_K_PYR_DOWN);
      hipLaunchKernelGGL(pyr_down_kernel, dim3(vo_cdiv(wd + 2 * PYR_PAD, 64), vo_cdiv(hd + 2 * PYR_PAD, 4), S), dim3(256), 0,
                         ctx->stream, src, spitch, h, w, dst, dpitch, hd, wd, pyr_stride);
    }
    VO_TRY(vo_check_launch(ctx, "pyr_down_kernel"));
    src = dst + (size_t)PYR_PAD * dpitch + PYR_PAD;
    spitch = dpitch;
    dst += pyr_level_bytes(hd, wd);
    h = hd;
    w = wd;
  }
  return VO_OK;
}

extern "C" {

int vo_pyr_down(vo_ctx* ctx, const uint8_t* img, int H, int W, uint8_t* out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, img && out && H > 0 && W > 0, "pyr_down: bad arguments");
  const size_t px = (size_t)H * W;
  const int hd = (H + 1) / 2, wd = (W + 1) / 2;
  VO_TRY(vo_ensure(ctx, ctx->img, px));
  VO_TRY(vo_ensure(ctx, ctx->scratch[8], vo_pyramid_bytes(H, W, 2)));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, img, px, hipMemcpyHostToDevice, ctx->stream));
  VO_TRY(vo_pyramid_build_dev(ctx, (const uint8_t*)ctx->img.p, H, W, 2, (uint8_t*)ctx->scratch[8].p));
  {
    const uint8_t* l1 = (const uint8_t*)ctx->scratch[8].p + pyr_level_bytes(H, W);
    const int pitch = pyr_pitch(wd);
    VO_HIP_TRY(ctx, hipMemcpy2DAsync(out, (size_t)wd, l1 + (size_t)PYR_PAD * pitch + PYR_PAD, (size_t)pitch, (size_t)wd,
                                     (size_t)hd, hipMemcpyDeviceToHost, ctx->stream));
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VO_OK;
}

}  // extern "C"
