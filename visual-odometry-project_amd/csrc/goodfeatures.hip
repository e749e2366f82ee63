// Shi-Tomasi corner detection ("good features to track") for gfx950.
//
// Reference call site: src/vo/features/klt.py:98
//   cv2.goodFeaturesToTrack(img, mask=mask, maxCorners=500, qualityLevel=0.01,
//                           minDistance=8, blockSize=7)                  (klt.py:24-26)
// The definition (restated in oracle/csrc/goodfeatures.c): min-eigenvalue map of the
// block x block structure tensor of 3x3 Sobel gradients (reflect-101 borders, exact
// integer sums scaled once), quality threshold against the masked maximum, 3x3 local
// maxima, descending order, greedy minimum-distance selection.
// Everything on the device, as a fixed sequence of launches for S images of one size: eigenvalue map and masked maximum,
// thresholded local maxima -> candidate keys (value | address), descending radix sort (rocPRIM), then the greedy
// minimum-distance rule.  The rule's recursion -- a candidate is accepted when every earlier candidate within minDistance
// is rejected, rejected when one of them is accepted -- is run over all candidates at once, one launch per round, through
// a cell grid (cell side = minDistance, as OpenCV keeps it); an image the rounds cannot take is walked by one workgroup in
// blocks of 512 candidates instead.  The one-image host call is the S = 1 case with one difference: it reads the
// candidate count back and sorts exactly that many keys device-wide, where the batched forms sort capacity-sized segments
// without a host turn (the stages and their callers are at the end of the file).
#include <algorithm>
#include <cmath>

#include <cstring>

#include "vo_internal.h"

#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int GX = 64, GY = 16, GT = 256;

__device__ __forceinline__ int refl(int c, int n) {
  if (n == 1) return 0;
  while (c < 0 || c >= n) c = c < 0 ? -c : 2 * (n - 1) - c;
  return c;
}

__device__ __forceinline__ unsigned float_key(float f) {   // monotone float -> unsigned
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// (one 64 x 16 tile of one image: the body of min_eig_batch_kernel)
__device__ __forceinline__ void min_eig_tile(const uint8_t* __restrict__ img, int H, int W, int block, float s2,
                                             const uint8_t* __restrict__ mask, float* __restrict__ eig,
                                             unsigned* __restrict__ max_key) {
  extern __shared__ __align__(16) int s_g[];                 // gradient region, packed (gx | gy << 16)
  __shared__ unsigned s_max;
  const int r0 = block / 2;
  const int RW = GX + block - 1, RH = GY + block - 1;
  int* s_hxx = s_g + RW * RH;                                // horizontal sums: RH x GX
  int* s_hxy = s_hxx + RH * GX;
  int* s_hyy = s_hxy + RH * GX;
  const int tid = threadIdx.x;
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
    int sxx = 0, sxy = 0, syy = 0;
    for (int k = 0; k < block; ++k) {
      const int v = g[k];
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
    for (int k = 0; k < block; ++k) {
      const int j = (ly + k) * GX + lx;
      sxx += s_hxx[j];
      sxy += s_hxy[j];
      syy += s_hyy[j];
    }
    const float a = (float)sxx * s2 * 0.5f, b = (float)sxy * s2, c = (float)syy * s2 * 0.5f;
    const float e = (a + c) - sqrtf((a - c) * (a - c) + b * b);
    eig[(size_t)y * W + x] = e;
    if (!mask || mask[(size_t)y * W + x]) local = max(local, float_key(e));
  }
  if (local) atomicMax(&s_max, local);
  __syncthreads();
  if (tid == 0 && s_max) atomicMax(max_key, s_max);
}

__device__ __forceinline__ void corner_candidates_tile(const float* __restrict__ eig, int H, int W,
                                                       const uint8_t* __restrict__ mask,
                                                       const unsigned* __restrict__ max_key, double quality,
                                                       unsigned long long* __restrict__ keys,
                                                       unsigned* __restrict__ count, unsigned cap) {
  // A 64 x 16 tile per workgroup, four rows per work item; the tile's maxima are collected in LDS and appended with ONE
  // reservation (one returning atomic per maximum -- or per wave -- on the one counter: ~27k / ~16k of them at 1376x1241,
  // and the launch waited for the counter 97 % of its 94 us).
  __shared__ unsigned long long s_keys[GX * GY / 4 + 64];        // (3x3 maxima: at most one per 2x2 block, ties aside)
  __shared__ unsigned s_n, s_base;
  const unsigned mk = *max_key;
  if (mk == 0) return;                                           // empty mask
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const float thr = (float)((double)key_float(mk) * quality);
  const int x = blockIdx.x * GX + (threadIdx.x & (GX - 1));
#pragma unroll
  for (int k = 0; k < GY / (GT / GX); ++k) {
    const int y = blockIdx.y * GY + k * (GT / GX) + threadIdx.x / GX;
    bool take = x >= 1 && y >= 1 && x < W - 1 && y < H - 1;
    float v = 0.f;
    if (take) {
      v = eig[(size_t)y * W + x];
      take = v > thr && v != 0.f && (!mask || mask[(size_t)y * W + x]);
    }
    if (take) {
      float m = 0.f;
#pragma unroll
      for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
          float q = eig[(size_t)(y + j) * W + (x + i)];
          q = q > thr ? q : 0.f;
          m = q > m ? q : m;
        }
      take = v == m;
    }
    if (take) {
      // descending order of the key = descending value, ties: higher address first (positive floats order like their bits)
      const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(y * W + x);
      const unsigned slot = atomicAdd(&s_n, 1u);
      if (slot < (unsigned)(GX * GY / 4 + 64)) {
        s_keys[slot] = key;
      } else {                                                   // (a plateau: more maxima than one per 2x2 block)
        const unsigned pos = atomicAdd(count, 1u);
        if (pos < cap) keys[pos] = key;
      }
    }
  }
  __syncthreads();
  const unsigned n = min(s_n, (unsigned)(GX * GY / 4 + 64));
  if (threadIdx.x == 0 && n) s_base = atomicAdd(count, n);
  __syncthreads();
  for (unsigned i = threadIdx.x; i < n; i += GT) {
    const unsigned pos = s_base + i;
    if (pos < cap) keys[pos] = s_keys[i];
  }
}

// The greedy rule over the sorted candidates, one workgroup.  Cell grid in global memory: per cell a count and up to
// GRID_SLOTS accepted corners (x | y << 16); accepted corners are >= minDistance apart, so a cell of that side holds
// at most four -- more than GRID_SLOTS raises the fault word and the image fails (VO_ECAPACITY in the host forms).
constexpr int GF_T = 512, GF_NB = 24, GRID_SLOTS = 8;
enum { GF_UNDECIDED = 0, GF_ACCEPTED = 1, GF_REJECTED = 2 };

__device__ __forceinline__ void greedy_distance_walk(const unsigned long long* __restrict__ keys, unsigned nc, int W,
                                                     int cell, int gw, int gh, double md2, int max_corners,
                                                     unsigned* __restrict__ cell_cnt, unsigned* __restrict__ cell_pts,
                                                     float* __restrict__ xy,
                                                     unsigned* __restrict__ ctl /* [2] n_out, [3] fault */) {
  __shared__ int s_xy[GF_T];
  __shared__ unsigned char s_state[GF_T];
  __shared__ unsigned short s_nb[GF_T][GF_NB];
  __shared__ int s_scan[GF_T];
  __shared__ int s_open, s_total;
  const int t = threadIdx.x;
  int n_acc = 0;
  const int limit = max_corners > 0 ? max_corners : 0x7fffffff;
  for (unsigned base = 0; base < nc && n_acc < limit; base += GF_T) {
    const unsigned k = base + t;
    const bool valid = k < nc;
    int x = 0, y = 0, state = GF_REJECTED;
    if (valid) {
      const unsigned id = (unsigned)(keys[k] & 0xffffffffull);
      y = (int)(id / (unsigned)W);
      x = (int)(id - (unsigned)y * (unsigned)W);
      state = GF_UNDECIDED;
      // accepted corners of earlier blocks, through the grid
      const int cx = x / cell, cy = y / cell;
      for (int yy = max(0, cy - 1); yy <= min(gh - 1, cy + 1) && state == GF_UNDECIDED; ++yy)
        for (int xx = max(0, cx - 1); xx <= min(gw - 1, cx + 1) && state == GF_UNDECIDED; ++xx) {
          // (agent-scope loads: the grid is written by this workgroup's earlier blocks, past the CU's L1)
          const unsigned c = (unsigned)yy * gw + xx;
          const unsigned m = min(__hip_atomic_load(&cell_cnt[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (unsigned)GRID_SLOTS);
          for (unsigned j = 0; j < m; ++j) {
            const unsigned pt = __hip_atomic_load(&cell_pts[c * GRID_SLOTS + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double dx = x - (int)(pt & 0xffffu), dy = y - (int)(pt >> 16);
            if (dx * dx + dy * dy < md2) state = GF_REJECTED;
          }
        }
    }
    s_xy[t] = x | (y << 16);
    s_state[t] = (unsigned char)state;
    __syncthreads();
    // earlier candidates of this block within minDistance (rejected ones can be left out: they decide nothing)
    // (only corners in the 3x3 cells around the candidate count, as in the grid walk above and in OpenCV)
    const int mcx = x / cell, mcy = y / cell;
    int nnb = 0;
    if (state == GF_UNDECIDED) {
      for (int q = 0; q < t; ++q) {
        if (s_state[q] == GF_REJECTED) continue;
        const int pq = s_xy[q];
        const int qx = pq & 0xffff, qy = pq >> 16;
        const double dx = x - qx, dy = y - qy;
        if (dx * dx + dy * dy < md2 && abs(qx / cell - mcx) <= 1 && abs(qy / cell - mcy) <= 1) {
          if (nnb < GF_NB) s_nb[t][nnb] = (unsigned short)q;
          ++nnb;
        }
      }
    }
    __syncthreads();
    for (;;) {
      if (t == 0) s_open = 0;
      __syncthreads();
      int next = state;
      if (state == GF_UNDECIDED) {
        bool any_acc = false, any_und = false;
        if (nnb <= GF_NB) {
          for (int j = 0; j < nnb; ++j) {
            const int st = s_state[s_nb[t][j]];
            any_acc |= st == GF_ACCEPTED;
            any_und |= st == GF_UNDECIDED;
          }
        } else {                                     // (more neighbours than the list holds: scan the block)
          for (int q = 0; q < t; ++q) {
            const int st = s_state[q];
            if (st == GF_REJECTED) continue;
            const int pq = s_xy[q];
            const int qx = pq & 0xffff, qy = pq >> 16;
            const double dx = x - qx, dy = y - qy;
            if (dx * dx + dy * dy < md2 && abs(qx / cell - mcx) <= 1 && abs(qy / cell - mcy) <= 1) {
              any_acc |= st == GF_ACCEPTED;
              any_und |= st == GF_UNDECIDED;
            }
          }
        }
        if (any_acc) next = GF_REJECTED;
        else if (!any_und) next = GF_ACCEPTED;
        else atomicOr(&s_open, 1);
      }
      __syncthreads();                               // all reads of this sweep are done
      state = next;
      s_state[t] = (unsigned char)state;
      __syncthreads();
      if (s_open == 0) break;
      __syncthreads();
    }
    // rank of the accepted among the accepted (priority order), output, grid insertion
    const int acc = state == GF_ACCEPTED ? 1 : 0;
    s_scan[t] = acc;
    __syncthreads();
    for (int off = 1; off < GF_T; off <<= 1) {
      const int add = t >= off ? s_scan[t - off] : 0;
      __syncthreads();
      s_scan[t] += add;
      __syncthreads();
    }
    if (t == GF_T - 1) s_total = s_scan[t];
    const int rank = n_acc + s_scan[t] - acc;
    if (acc && rank < limit) {
      xy[2 * rank] = (float)x;
      xy[2 * rank + 1] = (float)y;
      const unsigned c = (unsigned)(y / cell) * gw + (x / cell);
      const unsigned slot = atomicAdd(&cell_cnt[c], 1u);
      if (slot < (unsigned)GRID_SLOTS)
        __hip_atomic_store(&cell_pts[c * GRID_SLOTS + slot], (unsigned)x | ((unsigned)y << 16), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      else ctl[3] = 1u;
    }
    __threadfence();
    __syncthreads();
    n_acc = min(n_acc + s_total, limit);
    __syncthreads();
  }
  if (t == 0) ctl[2] = (unsigned)n_acc;
}

// The same rule over all candidates at once (the gfb_* kernels below): a candidate is accepted as soon as every earlier
// (higher-priority) candidate within minDistance is rejected, rejected as soon as one of them is accepted -- the
// sequential walk decides exactly that, and decisions never change, so a candidate may read any mix of its neighbours'
// old and new states.  The walk above takes 40 blocks of 14 us for the 20-30 thousand candidates of a 1376x1241 frame,
// this ~15 rounds of a few microseconds.  GC_T work items per workgroup and at most GC_WG workgroups per image (more
// candidates: the walk), GC_NB listed neighbours per candidate, GC_CCAP candidates per cell (more: the walk).
constexpr int GC_T = 512, GC_WG = 256, GC_NB = 24, GC_CCAP = 32;

// ---- S images per set of launches -----------------------------------------------------------------------------------------
// Every stage has the image as a grid dimension and leaves its counts on the device; the rounds of the minimum-distance
// rule are launches, so no workgroup ever waits for another and nothing depends on which workgroups are resident.  Per
// image a control block of GB_CTL words (256 bytes: the images' counters never share a cache line):
//   [GB_MAX] masked maximum (key)   [GB_NC] candidates sorted   [GB_N] corners   [GB_FAULT] bit 0: GRID_SLOTS overflowed
//   in the walk, bit 8: more local maxima than the candidate capacity   [GB_PATH] 0 rounds, 1 walk, 2 take-sorted
//   [GB_ROUNDS] round launches that still found the image open   [GB_WALK] the rounds path hands the image to the walk
//   [GB_OPEN + r] candidates were undecided before round r (r = the call's rounds: after the last one)   [GB_COUNT] local maxima
// GB_R = 24 round launches: about 15 settle a 1376x1241 frame (above); an image still open after them is finished by
// the walk, so the number decides speed only.
constexpr int GB_CTL = 64, GB_R = 24;
enum { GB_MAX = 0, GB_NC = 1, GB_N = 2, GB_FAULT = 3, GB_PATH = 4, GB_ROUNDS = 5, GB_WALK = 6, GB_OPEN = 8 /* .. 8 + GB_R */,
       GB_COUNT = 40 };
static_assert(GB_OPEN + GB_R < GB_COUNT && GB_COUNT < GB_CTL, "control block layout");
static_assert(GB_R == VO_GFB_ROUNDS && GC_WG * GC_T == VO_GFB_CANDIDATES, "vo_internal.h names the ABI call's values");

struct gfb_dims {
  int H, W, cell, gw, gh, ccap;     // ccap: candidates a cell holds on the rounds path, min(GC_CCAP, cell * cell)
  unsigned cap, lim;                // candidate capacity per image; candidates the rounds path holds per image
  int rounds;                       // round launches of this call (<= GB_R)
  size_t px, cells;
};

__global__ __launch_bounds__(GT) void min_eig_batch_kernel(const uint8_t* __restrict__ imgs, size_t img_stride, gfb_dims g,
                                                           int block, float s2, const uint8_t* __restrict__ masks,
                                                           size_t mask_stride, float* __restrict__ eig,
                                                           unsigned* __restrict__ ctl, const int* __restrict__ go) {
  const size_t q = blockIdx.z;
  if (go && !go[q]) return;          // (gated out: no map, no maximum -- and no candidates below)
  min_eig_tile(imgs + q * img_stride, g.H, g.W, block, s2, masks ? masks + q * mask_stride : nullptr, eig + q * g.px,
               ctl + q * GB_CTL + GB_MAX);
}

__global__ __launch_bounds__(GT) void corner_candidates_batch_kernel(const float* __restrict__ eig, gfb_dims g,
                                                                     const uint8_t* __restrict__ masks, size_t mask_stride,
                                                                     double quality, unsigned long long* __restrict__ keys,
                                                                     unsigned* __restrict__ ctl, const int* __restrict__ go) {
  const size_t q = blockIdx.z;
  if (go && !go[q]) return;          // (its count of local maxima stays 0: every later stage falls through)
  corner_candidates_tile(eig + q * g.px, g.H, g.W, masks ? masks + q * mask_stride : nullptr, ctl + q * GB_CTL + GB_MAX,
                         quality, keys + q * g.cap, ctl + q * GB_CTL + GB_COUNT, g.cap);
}

// the sort's segment bounds and the path of every image, from its count of local maxima
__global__ __launch_bounds__(256) void gfb_segments_kernel(int S, gfb_dims g, int take_sorted, unsigned* __restrict__ ctl,
                                                           unsigned* __restrict__ seg) {
  for (int q = threadIdx.x; q < S; q += 256) {
    unsigned* c = ctl + (size_t)q * GB_CTL;
    const unsigned cnt = c[GB_COUNT];
    const bool over = cnt > g.cap;        // (ties count as maxima: plateaus can exceed one maximum per 2x2 block)
    const unsigned nc = over ? 0u : cnt;
    seg[q] = (unsigned)q * g.cap;
    seg[S + q] = (unsigned)q * g.cap + nc;
    c[GB_NC] = nc;
    if (over) c[GB_FAULT] = 0x100u;
    const unsigned path = take_sorted ? 2u : (nc > g.lim ? 1u : 0u);
    c[GB_PATH] = path;
    c[GB_OPEN] = (path == 0u && nc > 0u) ? 1u : 0u;
  }
}

__device__ __forceinline__ void gfb_key_xy(unsigned long long key, int W, int& x, int& y) {
  const unsigned id = (unsigned)(key & 0xffffffffull);
  y = (int)(id / (unsigned)W);
  x = (int)(id - (unsigned)y * (unsigned)W);
}

// every earlier candidate within minDistance in the 3x3 cells around candidate k
template <class V>
__device__ __forceinline__ void gfb_neighbours(const unsigned long long* __restrict__ keys, unsigned k, int x, int y,
                                               const gfb_dims& g, double md2, const unsigned* __restrict__ cell_cnt,
                                               const unsigned* __restrict__ cell_items, V&& visit) {
  const int cx = x / g.cell, cy = y / g.cell;
  for (int yy = max(0, cy - 1); yy <= min(g.gh - 1, cy + 1); ++yy)
    for (int xx = max(0, cx - 1); xx <= min(g.gw - 1, cx + 1); ++xx) {
      const size_t c = (size_t)yy * g.gw + xx;
      const unsigned m = min(cell_cnt[c], (unsigned)g.ccap);
      for (unsigned j = 0; j < m; ++j) {
        const unsigned o = cell_items[c * g.ccap + j];
        if (o >= k) continue;
        int qx, qy;
        gfb_key_xy(keys[o], g.W, qx, qy);
        const double dx = x - qx, dy = y - qy;
        if (dx * dx + dy * dy < md2) visit(o);
      }
    }
}

// prep: every candidate of a rounds-path image enters the cell grid; a cell that does not hold its candidates hands the
// image to the walk
__global__ __launch_bounds__(GC_T) void gfb_prep_kernel(const unsigned long long* __restrict__ keys, gfb_dims g,
                                                        unsigned* __restrict__ cell_cnt, unsigned* __restrict__ cell_items,
                                                        unsigned* __restrict__ state, unsigned* __restrict__ ctl) {
  const size_t q = blockIdx.y;
  unsigned* c = ctl + q * GB_CTL;
  if (c[GB_PATH] != 0u) return;
  const unsigned k = blockIdx.x * GC_T + threadIdx.x;
  if (k >= c[GB_NC]) return;
  int x, y;
  gfb_key_xy(keys[q * g.cap + k], g.W, x, y);
  const size_t cl = q * g.cells + (size_t)(y / g.cell) * g.gw + (x / g.cell);
  const unsigned slot = atomicAdd(&cell_cnt[cl], 1u);
  if (slot < (unsigned)g.ccap) cell_items[cl * g.ccap + slot] = k;
  else __hip_atomic_store(&c[GB_WALK], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  state[q * g.lim + k] = GF_UNDECIDED;
}

// lists: a candidate's earlier neighbours (up to GC_NB; more: the cells are walked again in every round); their number
// rides in the state word above the two state bits
__global__ __launch_bounds__(GC_T) void gfb_lists_kernel(const unsigned long long* __restrict__ keys, gfb_dims g, double md2,
                                                         const unsigned* __restrict__ cell_cnt,
                                                         const unsigned* __restrict__ cell_items,
                                                         unsigned* __restrict__ state, unsigned* __restrict__ nb,
                                                         const unsigned* __restrict__ ctl) {
  const size_t q = blockIdx.y;
  const unsigned* c = ctl + q * GB_CTL;
  if (c[GB_PATH] != 0u || c[GB_WALK] != 0u) return;
  const unsigned k = blockIdx.x * GC_T + threadIdx.x;
  if (k >= c[GB_NC]) return;
  keys += q * g.cap;
  int x, y;
  gfb_key_xy(keys[k], g.W, x, y);
  unsigned* mine = nb + (q * g.lim + k) * GC_NB;
  unsigned nnb = 0;
  gfb_neighbours(keys, k, x, y, g, md2, cell_cnt + q * g.cells, cell_items + q * g.cells * g.ccap, [&](unsigned o) {
    if (nnb < (unsigned)GC_NB) mine[nnb] = o;
    ++nnb;
  });
  state[q * g.lim + k] = (unsigned)GF_UNDECIDED | (nnb << 2);
}

// one round: accepted as soon as every earlier neighbour is rejected, rejected as soon as one is accepted.  Decisions
// never change, so a neighbour's state may be this round's or the last one's; an image without an open candidate (the
// flag the round before left) costs its workgroups one load.
__global__ __launch_bounds__(GC_T) void gfb_round_kernel(const unsigned long long* __restrict__ keys, gfb_dims g, double md2,
                                                         int round, const unsigned* __restrict__ cell_cnt,
                                                         const unsigned* __restrict__ cell_items,
                                                         unsigned* __restrict__ state, const unsigned* __restrict__ nb,
                                                         unsigned* __restrict__ ctl) {
  __shared__ unsigned s_open;
  const size_t q = blockIdx.y;
  unsigned* c = ctl + q * GB_CTL;
  if (c[GB_PATH] != 0u || c[GB_WALK] != 0u || c[GB_OPEN + round] == 0u) return;
  const unsigned nc = c[GB_NC];
  if (blockIdx.x * GC_T >= nc) return;
  const int t = threadIdx.x;
  const unsigned k = blockIdx.x * GC_T + t;
  if (t == 0) {
    s_open = 0;
    if (blockIdx.x == 0) c[GB_ROUNDS] = (unsigned)round + 1u;
  }
  __syncthreads();
  keys += q * g.cap;
  state += q * g.lim;
  if (k < nc) {
    const unsigned w = state[k];          // (own word: written by this work item only)
    if ((w & 3u) == GF_UNDECIDED) {
      const unsigned nnb = w >> 2;
      bool any_acc = false, any_und = false;
      auto look = [&](unsigned o) {
        const unsigned so = __hip_atomic_load(&state[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 3u;
        any_acc |= so == GF_ACCEPTED;
        any_und |= so == GF_UNDECIDED;
      };
      if (nnb <= (unsigned)GC_NB) {
        const unsigned* mine = nb + (q * g.lim + k) * GC_NB;
        for (unsigned j = 0; j < nnb; ++j) look(mine[j]);
      } else {
        int x, y;
        gfb_key_xy(keys[k], g.W, x, y);
        gfb_neighbours(keys, k, x, y, g, md2, cell_cnt + q * g.cells, cell_items + q * g.cells * g.ccap, look);
      }
      unsigned st = GF_UNDECIDED;
      if (any_acc) st = GF_REJECTED;
      else if (!any_und) st = GF_ACCEPTED;
      if (st != GF_UNDECIDED) __hip_atomic_store(&state[k], st | (nnb << 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else s_open = 1;
    }
  }
  __syncthreads();
  if (t == 0 && s_open) __hip_atomic_store(&c[GB_OPEN + round + 1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the walk finishes an image the rounds could not take (path 1), handed over by prep (a crowded cell) or still open
// after the call's last round
__device__ __forceinline__ bool gfb_walked(const unsigned* __restrict__ c, int rounds) {
  const unsigned path = c[GB_PATH];
  return path == 1u || (path == 0u && (c[GB_WALK] != 0u || c[GB_OPEN + rounds] != 0u));
}

// an image the rounds did not finish (or could not take): the one-workgroup walk, into the staging rows
__global__ __launch_bounds__(GF_T) void greedy_distance_batch_kernel(const unsigned long long* __restrict__ keys, gfb_dims g,
                                                                     double md2, int max_corners,
                                                                     unsigned* __restrict__ cell_cnt,
                                                                     unsigned* __restrict__ cell_pts,
                                                                     float* __restrict__ xy, size_t xy_rows,
                                                                     unsigned* __restrict__ ctl) {
  const size_t q = blockIdx.x;
  unsigned* c = ctl + q * GB_CTL;
  if (!gfb_walked(c, g.rounds)) return;
  greedy_distance_walk(keys + q * g.cap, c[GB_NC], g.W, g.cell, g.gw, g.gh, md2, max_corners, cell_cnt + q * g.cells,
                       cell_pts + q * g.cells * GRID_SLOTS, xy + q * xy_rows * 2, c);
}

// One workgroup per image: the accepted candidates in priority order, the first max_corners of them (ballot + prefix as
// in boot_gather_kernel); the take-sorted path's corners; a walked image's rows from the staging buffer unless the walk
// failed; and the image's count, fault word and path record.  Nothing of an image that failed is written.
__global__ __launch_bounds__(GC_T) void gfb_emit_kernel(const unsigned long long* __restrict__ keys, gfb_dims g,
                                                        int max_corners, const unsigned* __restrict__ state,
                                                        const float* __restrict__ walk_xy, size_t walk_rows,
                                                        const unsigned* __restrict__ ctl, float* __restrict__ xy,
                                                        size_t xy_stride, int32_t* __restrict__ d_n,
                                                        int32_t* __restrict__ d_over, int32_t* __restrict__ d_info) {
  __shared__ unsigned s_cnt[GC_T / 64];
  const size_t q = blockIdx.x;
  const unsigned* c = ctl + q * GB_CTL;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const unsigned nc = c[GB_NC], path = gfb_walked(c, g.rounds) ? 1u : c[GB_PATH], fault = c[GB_FAULT];
  const unsigned limit = max_corners > 0 ? (unsigned)max_corners : 0xffffffffu;
  const int over = (fault & 0x100u) ? 1 : ((fault & 1u) ? 2 : 0);
  keys += q * g.cap;
  state += q * g.lim;
  xy += q * xy_stride * 2;
  unsigned n = 0;
  if (over) {
    n = 0;
  } else if (path == 2u) {
    n = min(nc, limit);
    for (unsigned k = t; k < n; k += GC_T) {
      int x, y;
      gfb_key_xy(keys[k], g.W, x, y);
      xy[2 * k] = (float)x;
      xy[2 * k + 1] = (float)y;
    }
  } else if (path == 1u) {
    n = c[GB_N];
    const float* src = walk_xy + q * walk_rows * 2;
    for (unsigned i = t; i < 2 * n; i += GC_T) xy[i] = src[i];
  } else {
    unsigned base = 0;
    for (unsigned k0 = 0; k0 < nc && base < limit; k0 += GC_T) {
      const unsigned k = k0 + t;
      const bool acc = k < nc && (state[k] & 3u) == GF_ACCEPTED;
      const unsigned long long bal = __ballot(acc);
      if (lane == 0) s_cnt[wv] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < GC_T / 64; ++w) {
        if (w < wv) before += s_cnt[w];
        total += s_cnt[w];
      }
      const unsigned rank = base + before;
      if (acc && rank < limit) {
        int x, y;
        gfb_key_xy(keys[k], g.W, x, y);
        xy[2 * rank] = (float)x;
        xy[2 * rank + 1] = (float)y;
      }
      base += total;
      __syncthreads();
    }
    n = min(base, limit);
  }
  if (t == 0) {
    d_n[q] = (int32_t)n;
    if (d_over) d_over[q] = over;
    if (d_info) {
      d_info[4 * q] = (int32_t)(over == 1 ? c[GB_COUNT] : nc);
      d_info[4 * q + 1] = (int32_t)path;
      d_info[4 * q + 2] = (int32_t)c[GB_ROUNDS];
      d_info[4 * q + 3] = 0;
    }
  }
}

// no partitioning of the segments by length: that step reads its counts back on the host
typedef rocprim::segmented_radix_sort_config<8, rocprim::kernel_config<256, 16>> gfb_sort_config;

// ---- one call, in stages -------------------------------------------------------------------------------------------------
// plan (checks, sizes, workspace, memsets), front (map + maximum, candidates, segment bounds and paths), the sort, back
// (prep, lists, the rounds, the walk of flagged images, emit), all on ctx->stream.  Only growing the context's workspace,
// on the first call of a size, waits.  Workspace per image, linear in S; at 1376 x 1241 with minDistance 8 (26 832 cells),
// max_corners 2000:
//   eigenvalue map 6 830 464 B, candidate keys and their sorted copy 2 x 3 415 744 B, the sort's own copy 3 415 744 B,
//   neighbour lists 131 072 x 24 x 4 = 12 582 912 B, state words 524 288 B, cell candidates 26 832 x 32 x 4 = 3 434 496 B,
//   cell counts (rounds + walk) 214 656 B, the walk's cells 858 624 B and staging rows 16 000 B, control block 256 B
//   = 34 708 928 B, about 33.1 MiB per image.
struct gfb_call {
  // the arguments of vo_good_features_batch_gated_dev, in its order
  const uint8_t* d_imgs;
  size_t img_stride;
  int S, H, W;
  const uint8_t* d_masks;
  size_t mask_stride;
  int max_corners;
  double quality, min_dist;
  int block;
  float* d_xy;
  size_t xy_stride;
  int32_t *d_n, *d_over, *d_info;
  int n_rounds, cand_limit;
  const int* d_go;
  // what plan makes of them
  gfb_dims g;
  bool rounds;                      // min_dist >= 1: the rule runs; below, the corners are the sorted list's head
  size_t out_cap, sort_tmp;
};

size_t min_eig_lds(int block) {
  const int RW = GX + block - 1, RH = GY + block - 1;
  return ((size_t)RW * RH + (size_t)3 * RH * GX) * 4;
}

int gfb_check(vo_ctx* ctx, const char* who, int S, int H, int W, double quality, double min_dist, int block) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, H > 0 && W > 0, "%s: bad arguments", who);
  VO_REQUIRE(ctx, S >= 1 && S <= 65535, "%s: S must be in 1..65535", who);
  VO_REQUIRE(ctx, block >= 1 && block <= 31, "%s: blockSize must be in 1..31", who);
  VO_REQUIRE(ctx, quality > 0 && min_dist >= 0, "%s: bad quality / minDistance", who);
  VO_REQUIRE(ctx, W < 65536 && H < 65536, "%s: image side must be below 65536", who);
  const size_t cap = ((size_t)H * W + 3) / 4 + 64;                // 3x3 maxima: at most one per 2x2 block
  VO_REQUIRE(ctx, (size_t)S * cap < 0xffffffffull, "%s: %d images of %d x %d exceed the sort's 32-bit offsets", who, S, H, W);
  return VO_OK;
}

// host_sort: the workspace of a device-wide sort of one image's keys (gfb_sort_counted) in place of the segmented one's
int gfb_plan(vo_ctx* ctx, const char* who, gfb_call& c, bool host_sort) {
  VO_REQUIRE(ctx, c.n_rounds >= 0 && c.n_rounds <= GB_R && c.cand_limit >= 1 && c.cand_limit <= GC_WG * GC_T,
             "%s: rounds must be in 0..%d, the candidate limit in 1..%d", who, GB_R, GC_WG * GC_T);
  VO_REQUIRE(ctx, c.d_imgs && c.d_xy && c.d_n && c.H > 0 && c.W > 0, "%s: bad arguments", who);
  VO_TRY(gfb_check(ctx, who, c.S, c.H, c.W, c.quality, c.min_dist, c.block));
  const size_t px = (size_t)c.H * c.W, Sz = (size_t)c.S;
  VO_REQUIRE(ctx, c.img_stride >= px && (!c.d_masks || c.mask_stride >= px), "%s: image / mask stride below H*W", who);
  const size_t cap = (px + 3) / 4 + 64;                          // 3x3 maxima: at most one per 2x2 block
  c.out_cap = c.max_corners > 0 ? (size_t)c.max_corners : cap;
  VO_REQUIRE(ctx, c.xy_stride >= c.out_cap, "%s: xy_stride %zu is below the capacity %zu", who, c.xy_stride, c.out_cap);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  gfb_dims& g = c.g;
  g.H = c.H;
  g.W = c.W;
  g.cell = std::max(1, (int)std::lround(c.min_dist));
  g.gw = (c.W + g.cell - 1) / g.cell;
  g.gh = (c.H + g.cell - 1) / g.cell;
  g.ccap = (int)std::min<long long>(GC_CCAP, (long long)g.cell * g.cell);
  g.cap = (unsigned)cap;
  g.lim = (unsigned)std::min<size_t>((size_t)c.cand_limit, cap);
  g.rounds = c.n_rounds;
  g.px = px;
  g.cells = (size_t)g.gw * g.gh;
  c.rounds = c.min_dist >= 1;
  c.sort_tmp = 0;
  if (host_sort)
    VO_HIP_TRY(ctx, rocprim::radix_sort_keys_desc(nullptr, c.sort_tmp, (unsigned long long*)nullptr,
                                                  (unsigned long long*)nullptr, cap, 0, 64, st));
  else
    VO_HIP_TRY(ctx, rocprim::segmented_radix_sort_keys_desc<gfb_sort_config>(
                        nullptr, c.sort_tmp, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned)(Sz * cap),
                        (unsigned)c.S, (unsigned*)nullptr, (unsigned*)nullptr, 0, 64, st));
  VO_TRY(vo_ensure(ctx, s[0], Sz * px * 4));
  VO_TRY(vo_ensure(ctx, s[1], Sz * GB_CTL * 4));
  VO_TRY(vo_ensure(ctx, s[2], Sz * cap * 8));
  VO_TRY(vo_ensure(ctx, s[3], Sz * cap * 8));
  VO_TRY(vo_ensure(ctx, s[4], c.sort_tmp + 256));
  VO_TRY(vo_ensure(ctx, s[11], Sz * 2 * 4));
  if (c.rounds) {
    VO_TRY(vo_ensure(ctx, s[5], Sz * g.cells * 4 * 2));
    VO_TRY(vo_ensure(ctx, s[6], Sz * g.cells * GRID_SLOTS * 4));
    VO_TRY(vo_ensure(ctx, s[7], Sz * c.out_cap * 8));
    VO_TRY(vo_ensure(ctx, s[8], Sz * g.cells * g.ccap * 4));
    VO_TRY(vo_ensure(ctx, s[9], Sz * g.lim * 4));
    VO_TRY(vo_ensure(ctx, s[10], Sz * g.lim * GC_NB * 4));
    VO_HIP_TRY(ctx, hipMemsetAsync(s[5].p, 0, Sz * g.cells * 4 * 2, st));
  }
  VO_HIP_TRY(ctx, hipMemsetAsync(s[1].p, 0, Sz * GB_CTL * 4, st));
  return VO_OK;
}

int gfb_front(vo_ctx* ctx, const gfb_call& c) {
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  unsigned* d_ctl = (unsigned*)s[1].p;
  const double scale = 1.0 / (4.0 * c.block * 255.0);
  const dim3 tiles(vo_cdiv(c.W, GX), vo_cdiv(c.H, GY), c.S);
  hipLaunchKernelGGL(min_eig_batch_kernel, tiles, dim3(GT), min_eig_lds(c.block), st, c.d_imgs, c.img_stride, c.g, c.block,
                     (float)(scale * scale), c.d_masks, c.mask_stride, (float*)s[0].p, d_ctl, c.d_go);
  VO_TRY(vo_check_launch(ctx, "min_eig_batch_kernel"));
  hipLaunchKernelGGL(corner_candidates_batch_kernel, tiles, dim3(GT), 0, st, (const float*)s[0].p, c.g, c.d_masks,
                     c.mask_stride, c.quality, (unsigned long long*)s[2].p, d_ctl, c.d_go);
  VO_TRY(vo_check_launch(ctx, "corner_candidates_batch_kernel"));
  hipLaunchKernelGGL(gfb_segments_kernel, dim3(1), dim3(256), 0, st, c.S, c.g, c.rounds ? 0 : 1, d_ctl, (unsigned*)s[11].p);
  VO_TRY(vo_check_launch(ctx, "gfb_segments_kernel"));
  return VO_OK;
}

// capacity-sized segments, one per image, bounded on the device: no host turn
int gfb_sort_segments(vo_ctx* ctx, const gfb_call& c) {
  vo_buf* s = ctx->scratch;
  size_t sort_tmp = c.sort_tmp;
  unsigned* d_seg = (unsigned*)s[11].p;
  VO_HIP_TRY(ctx, rocprim::segmented_radix_sort_keys_desc<gfb_sort_config>(
                      s[4].p, sort_tmp, (unsigned long long*)s[2].p, (unsigned long long*)s[3].p,
                      (unsigned)((size_t)c.S * c.g.cap), (unsigned)c.S, d_seg, d_seg + c.S, 0, 64, ctx->stream));
  return VO_OK;
}

// one image (plan's host_sort): its candidate count comes back -- the segments kernel has turned an overflow of the
// capacity into no candidates and the fault bit -- and exactly that many keys are sorted device-wide; at 1376 x 1241
// that sort takes 36 us where the one-segment sort above takes 426 us, which the host turn buys
int gfb_sort_counted(vo_ctx* ctx, const gfb_call& c) {
  vo_buf* s = ctx->scratch;
  hipStream_t st = ctx->stream;
  size_t sort_tmp = c.sort_tmp;
  unsigned nc = 0;
  VO_HIP_TRY(ctx, hipMemcpyAsync(&nc, (const unsigned*)s[1].p + GB_NC, 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->bytes_d2h += 4;
  if (nc > 0)
    VO_HIP_TRY(ctx, rocprim::radix_sort_keys_desc(s[4].p, sort_tmp, (unsigned long long*)s[2].p, (unsigned long long*)s[3].p,
                                                  (size_t)nc, 0, 64, st));
  return VO_OK;
}

int gfb_back(vo_ctx* ctx, const gfb_call& c) {
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  const gfb_dims& g = c.g;
  const size_t Sz = (size_t)c.S;
  unsigned* d_ctl = (unsigned*)s[1].p;
  const unsigned long long* d_sorted = (const unsigned long long*)s[3].p;
  if (c.rounds) {
    const double md2 = c.min_dist * c.min_dist;
    unsigned* cell_cnt = (unsigned*)s[5].p;
    unsigned* walk_cnt = cell_cnt + Sz * g.cells;
    const dim3 grid(vo_cdiv((int)g.lim, GC_T), c.S);
    hipLaunchKernelGGL(gfb_prep_kernel, grid, dim3(GC_T), 0, st, d_sorted, g, cell_cnt, (unsigned*)s[8].p, (unsigned*)s[9].p,
                       d_ctl);
    VO_TRY(vo_check_launch(ctx, "gfb_prep_kernel"));
    hipLaunchKernelGGL(gfb_lists_kernel, grid, dim3(GC_T), 0, st, d_sorted, g, md2, (const unsigned*)cell_cnt,
                       (const unsigned*)s[8].p, (unsigned*)s[9].p, (unsigned*)s[10].p, (const unsigned*)d_ctl);
    VO_TRY(vo_check_launch(ctx, "gfb_lists_kernel"));
    for (int r = 0; r < c.n_rounds; ++r)
      hipLaunchKernelGGL(gfb_round_kernel, grid, dim3(GC_T), 0, st, d_sorted, g, md2, r, (const unsigned*)cell_cnt,
                         (const unsigned*)s[8].p, (unsigned*)s[9].p, (const unsigned*)s[10].p, d_ctl);
    VO_TRY(vo_check_launch(ctx, "gfb_round_kernel"));
    hipLaunchKernelGGL(greedy_distance_batch_kernel, dim3(c.S), dim3(GF_T), 0, st, d_sorted, g, md2, c.max_corners, walk_cnt,
                       (unsigned*)s[6].p, (float*)s[7].p, c.out_cap, d_ctl);
    VO_TRY(vo_check_launch(ctx, "greedy_distance_batch_kernel"));
  }
  hipLaunchKernelGGL(gfb_emit_kernel, dim3(c.S), dim3(GC_T), 0, st, d_sorted, g, c.max_corners, (const unsigned*)s[9].p,
                     (const float*)s[7].p, c.out_cap, (const unsigned*)d_ctl, c.d_xy, c.xy_stride, c.d_n, c.d_over, c.d_info);
  VO_TRY(vo_check_launch(ctx, "gfb_emit_kernel"));
  return VO_OK;
}

// Both host forms: the S images (and masks) up, the stages on the context's own buffers, counts and corners down.
// host_sort (S = 1, vo_good_features): gfb_sort_counted for the sort, and the one-image call's error texts.
int gfb_host(vo_ctx* ctx, const char* who, bool host_sort, const uint8_t* imgs, const uint8_t* masks, int S, int H, int W,
             int max_corners, double quality, double min_dist, int block, float* xy, int32_t* n_out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, imgs && xy && n_out && H > 0 && W > 0 && S >= 1, "%s: bad arguments", who);
  for (int q = 0; q < S; ++q) n_out[q] = 0;
  const size_t rows = (size_t)vo_good_features_capacity(H, W, max_corners);
  VO_REQUIRE(ctx, rows > 0, "%s: image too large", who);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)H * W, Sz = (size_t)S;
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, ctx->img, Sz * px));
  if (masks) VO_TRY(vo_ensure(ctx, ctx->img2, Sz * px));
  VO_TRY(vo_ensure(ctx, s[12], Sz * rows * 8));
  VO_TRY(vo_ensure(ctx, s[13], Sz * 2 * 4));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, imgs, Sz * px, hipMemcpyHostToDevice, st));
  if (masks) VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img2.p, masks, Sz * px, hipMemcpyHostToDevice, st));
  ctx->bytes_h2d += (int64_t)(Sz * px * (masks ? 2 : 1));
  int32_t* d_cnt = (int32_t*)s[13].p;
  gfb_call c = {(const uint8_t*)ctx->img.p, px, S, H, W, masks ? (const uint8_t*)ctx->img2.p : nullptr, px, max_corners,
                quality, min_dist, block, (float*)s[12].p, rows, d_cnt, d_cnt + S, nullptr, GB_R, GC_WG * GC_T, nullptr};
  VO_TRY(gfb_plan(ctx, who, c, host_sort));
  VO_TRY(gfb_front(ctx, c));
  VO_TRY(host_sort ? gfb_sort_counted(ctx, c) : gfb_sort_segments(ctx, c));
  VO_TRY(gfb_back(ctx, c));
  std::vector<int32_t> cnt(Sz * 2);
  VO_HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_cnt, Sz * 8, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->bytes_d2h += (int64_t)(Sz * 8);
  for (int q = 0; q < S; ++q) {
    const int over = cnt[Sz + q];
    if (over && host_sort)
      return over == 1 ? vo_set_error(ctx, VO_ECAPACITY, "good_features: the local maxima exceed the candidate capacity %u", c.g.cap)
                       : vo_set_error(ctx, VO_ECAPACITY, "good_features: more than %d corners in one grid cell", GRID_SLOTS);
    if (over == 1)
      return vo_set_error(ctx, VO_ECAPACITY, "good_features_batch: the local maxima of image %d exceed the candidate capacity", q);
    if (over)
      return vo_set_error(ctx, VO_ECAPACITY, "good_features_batch: image %d has more than %d corners in one grid cell", q, GRID_SLOTS);
  }
  // a corner limit: the S blocks in one download (rows behind an image's count are workspace); every corner: the blocks
  // hold the candidate capacity, so each image's corners alone
  size_t total = 0;
  for (int q = 0; q < S; ++q) {
    n_out[q] = cnt[q];
    total += (size_t)cnt[q];
  }
  if (total == 0) return VO_OK;
  if (max_corners > 0) {
    VO_HIP_TRY(ctx, hipMemcpyAsync(xy, s[12].p, Sz * rows * 8, hipMemcpyDeviceToHost, st));
    ctx->bytes_d2h += (int64_t)(Sz * rows * 8);
  } else {
    for (int q = 0; q < S; ++q)
      if (cnt[q] > 0)
        VO_HIP_TRY(ctx, hipMemcpyAsync(xy + (size_t)q * rows * 2, (const float*)s[12].p + (size_t)q * rows * 2, (size_t)cnt[q] * 8,
                                       hipMemcpyDeviceToHost, st));
    ctx->bytes_d2h += (int64_t)(total * 8);
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

}  // namespace

// (vo_internal.h) the argument checks of the batched forms alone
int vo_good_features_batch_check(vo_ctx* ctx, int S, int H, int W, double quality, double min_dist, int block) {
  return gfb_check(ctx, "good_features_batch", S, H, W, quality, min_dist, block);
}

// (vo_internal.h) the device form every other one goes through: plan, front, the segmented sort, back -- nothing is read
// back and nothing waits.  d_go gates images out; n_rounds and cand_limit are what the tests use to send images through
// the hand-over from unfinished rounds to the walk and through the walk of a long list.
int vo_good_features_batch_gated_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                                     const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality,
                                     double min_dist, int block, float* d_xy, size_t xy_stride, int32_t* d_n, int32_t* d_over,
                                     int32_t* d_info, int n_rounds, int cand_limit, const int* d_go) {
  if (!ctx) return VO_EINVAL;
  gfb_call c = {d_imgs, img_stride, S, H, W, d_masks, mask_stride, max_corners, quality, min_dist, block, d_xy, xy_stride,
                d_n, d_over, d_info, n_rounds, cand_limit, d_go};
  VO_TRY(gfb_plan(ctx, "good_features_batch", c, false));
  VO_TRY(gfb_front(ctx, c));
  VO_TRY(gfb_sort_segments(ctx, c));
  return gfb_back(ctx, c);
}

extern "C" {

int vo_good_features_capacity(int H, int W, int max_corners) {
  if (H <= 0 || W <= 0) return 0;
  if (max_corners > 0) return max_corners;
  const size_t cap = ((size_t)H * W + 3) / 4 + 64;
  return cap > 0x7fffffffull ? 0 : (int)cap;
}

int vo_good_features_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                               const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality, double min_dist,
                               int block, float* d_xy, size_t xy_stride, int32_t* d_n, int32_t* d_over, int32_t* d_info) {
  return vo_good_features_batch_rounds_dev(ctx, d_imgs, img_stride, S, H, W, d_masks, mask_stride, max_corners, quality, min_dist,
                                           block, d_xy, xy_stride, d_n, d_over, d_info, GB_R, GC_WG * GC_T);
}

// (vo_internal.h) the same with the number of round launches and the rounds path's candidate limit given
int vo_good_features_batch_rounds_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W,
                                      const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality,
                                      double min_dist, int block, float* d_xy, size_t xy_stride, int32_t* d_n, int32_t* d_over,
                                      int32_t* d_info, int n_rounds, int cand_limit) {
  return vo_good_features_batch_gated_dev(ctx, d_imgs, img_stride, S, H, W, d_masks, mask_stride, max_corners, quality, min_dist,
                                          block, d_xy, xy_stride, d_n, d_over, d_info, n_rounds, cand_limit, nullptr);
}

int vo_good_features_batch(vo_ctx* ctx, const uint8_t* imgs, const uint8_t* masks, int S, int H, int W, int max_corners,
                           double quality, double min_dist, int block, float* xy, int32_t* n_out) {
  return gfb_host(ctx, "good_features_batch", false, imgs, masks, S, H, W, max_corners, quality, min_dist, block, xy, n_out);
}

int vo_good_features(vo_ctx* ctx, const uint8_t* img, int H, int W, const uint8_t* mask, int max_corners,
                     double quality, double min_dist, int block, float* xy, int32_t* n_out) {
  return gfb_host(ctx, "good_features", true, img, mask, 1, H, W, max_corners, quality, min_dist, block, xy, n_out);
}

int vo_min_eigen_map(vo_ctx* ctx, const uint8_t* img, int H, int W, int block, float* eig) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, img && eig && H > 0 && W > 0, "min_eigen_map: bad arguments");
  VO_REQUIRE(ctx, block >= 1 && block <= 31, "min_eigen_map: blockSize must be in 1..31");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)H * W;
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, ctx->img, px));
  VO_TRY(vo_ensure(ctx, s[0], px * 4));
  VO_TRY(vo_ensure(ctx, s[1], GB_CTL * 4));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, img, px, hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemsetAsync(s[1].p, 0, GB_CTL * 4, st));
  gfb_dims g = {};                   // (the map kernel reads H, W and px alone)
  g.H = H;
  g.W = W;
  g.px = px;
  const double scale = 1.0 / (4.0 * block * 255.0);
  hipLaunchKernelGGL(min_eig_batch_kernel, dim3(vo_cdiv(W, GX), vo_cdiv(H, GY), 1), dim3(GT), min_eig_lds(block), st,
                     (const uint8_t*)ctx->img.p, px, g, block, (float)(scale * scale), (const uint8_t*)nullptr, (size_t)0,
                     (float*)s[0].p, (unsigned*)s[1].p, (const int*)nullptr);
  VO_TRY(vo_check_launch(ctx, "min_eig_batch_kernel"));
  VO_HIP_TRY(ctx, hipMemcpyAsync(eig, s[0].p, px * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

}  // extern "C"
