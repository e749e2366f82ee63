// FAST-9 corners on the 16-pixel circle of radius 3, with a 3 x 3 suppression and a cut to the N strongest, for gfx950.
// The definition is the project's own (include/vo_hip.h, "FAST-9 corners"; tests/fast_reference.py states it in NumPy):
// bytes, int32 differences, an 8-bit score, a total order (score descending, index ascending).  Everything in this file
// is integer arithmetic, so device and definition agree bit for bit on every input, with no margins.
//
// S images of one size go through one fixed sequence of launches (image q is blockIdx.z); the one-image calls are S = 1:
//   fast_score_kernel    a 64 x 16 tile with its halo of 3 in LDS -> the score map (bytes)
//   fast_nms_kernel      the score map with a halo of 1 -> the survivor map (score where the corner survives, else 0) and
//                        a 255-bin histogram of the survivors' scores: per workgroup in LDS, then atomics nobody waits
//                        for, into one of sixteen copies
//   fast_rows_kernel     per image row: survivors above the cutting score, survivors at it
//   fast_select_kernel   a wave per row: the selected survivors go to their place in a list that is in index order
//   fast_order_kernel    an entry's row: the histogram's count of higher scores plus the equal scores before it in the
//                        list; keypoints, scores and counts are written
// The histogram tells the cutting score c (the lowest score taken) and how many survivors of score c are taken before
// anything is ordered; every stage that needs them sums the copies and scans the 255 bins again (fast_cut) instead of
// waiting for a launch that would.  The survivors of score c are taken in index order: a row's place among them is a sum
// over the rows before it.  No list of all survivors exists, so nothing has a capacity; there is no returning atomic,
// no workgroup waits for another, and a stage boundary is a launch boundary.
#include "vo_internal.h"

namespace {

constexpr int FX = 64, FY = 16, FT = 256;      // the tile of the two map kernels: 64 x 16 pixels, four rows a work item
constexpr int FROW = 72;                       // bytes between the rows of a tile in LDS (64 + 2 * 3, rounded up to dwords)
constexpr int F_COPIES = 16;                   // copies of an image's histogram: a workgroup adds to copy (its id mod 16)
constexpr int F_CTL = 256 * F_COPIES;          // words of an image's control block (16 KiB: lines of its own): the histograms
constexpr int F_ROWS = FT / 64;                // image rows per workgroup of the row kernels: a wave each

// s(p) where p is a corner, 0 where it is not; c points at the centre byte inside a tile whose rows are FROW apart.
// The score is computed as it is defined and compared with the threshold afterwards, on one path for every pixel:
//   max_k min_{j<9} (c_{k+j} - I) = (max_k min_{j<9} c_{k+j}) - I,  max_k min_{j<9} (I - c_{k+j}) = I - (min_k max_{j<9} c_{k+j}),
// and the sixteen minima (maxima) of nine contiguous circle pixels are minima of three minima of three: 2 x 32
// three-operand instructions, then two reductions over sixteen.  DESIGN.md 3.10 has the two shapes built before this one
// (bit masks per lane with the exact score for the lanes that pass; lane masks per wave on the scalar unit).
__device__ __forceinline__ int fast_score_at(const uint8_t* __restrict__ c, int t) {
  constexpr int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  constexpr int DY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
  const int I = c[0];
  int v[16], lo3[16], hi3[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = c[DY[i] * FROW + DX[i]];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    lo3[i] = min(min(v[i], v[(i + 1) & 15]), v[(i + 2) & 15]);
    hi3[i] = max(max(v[i], v[(i + 1) & 15]), v[(i + 2) & 15]);
  }
  int darkest_of_brightest = -1, brightest_of_darkest = 256;     // max_k min9, min_k max9
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    darkest_of_brightest = max(darkest_of_brightest, min(min(lo3[i], lo3[(i + 3) & 15]), lo3[(i + 6) & 15]));
    brightest_of_darkest = min(brightest_of_darkest, max(max(hi3[i], hi3[(i + 3) & 15]), hi3[(i + 6) & 15]));
  }
  const int s = max(darkest_of_brightest - I, I - brightest_of_darkest);
  return s > t ? s : 0;
}

struct fast_tile {
  int x0, y0;
};
// (vo_xcd_tile: the tiles one L2 serves are whole bands of the image)
__device__ __forceinline__ fast_tile fast_tile_of(int tiles_x, int n_tiles) {
  const unsigned t = vo_xcd_tile(blockIdx.x, (unsigned)n_tiles);
  return {(int)(t % (unsigned)tiles_x) * FX, (int)(t / (unsigned)tiles_x) * FY};
}

__global__ __launch_bounds__(FT) void fast_score_kernel(const uint8_t* __restrict__ imgs, size_t img_stride, int H, int W,
                                                        int tiles_x, int n_tiles, int thr, uint8_t* __restrict__ score,
                                                        size_t px) {
  __shared__ __attribute__((aligned(16))) uint8_t s_px[(FY + 6) * FROW];
  const int tid = threadIdx.x;
  const fast_tile tl = fast_tile_of(tiles_x, n_tiles);
  const uint8_t* img = imgs + blockIdx.z * img_stride;
  for (int i = tid; i < (FY + 6) * (FX + 6); i += FT) {
    const int r = i / (FX + 6), c = i - r * (FX + 6);
    const int y = tl.y0 - 3 + r, x = tl.x0 - 3 + c;
    s_px[r * FROW + c] = (y >= 0 && y < H && x >= 0 && x < W) ? img[(size_t)y * W + x] : (uint8_t)0;
  }
  __syncthreads();
  const int lx = tid & (FX - 1), x = tl.x0 + lx;
  if (x >= W) return;
  uint8_t* out = score + blockIdx.z * px;
#pragma unroll
  for (int k = 0; k < FY / (FT / FX); ++k) {
    const int ly = k * (FT / FX) + tid / FX, y = tl.y0 + ly;
    if (y >= H) break;
    int s = 0;
    if (x >= 3 && x < W - 3 && y >= 3 && y < H - 3) s = fast_score_at(s_px + (ly + 3) * FROW + lx + 3, thr);
    out[(size_t)y * W + x] = (uint8_t)s;
  }
}

// A corner survives when no neighbour beats it.  The four neighbours of lower index (the row above, the pixel to the
// left) beat it with a score at least its own, the four of higher index with a greater one; a neighbour outside the
// image, like one that is no corner, has score 0 and beats nothing (a corner's score is at least 1).
__global__ __launch_bounds__(FT) void fast_nms_kernel(const uint8_t* __restrict__ score, size_t px, int H, int W, int tiles_x,
                                                      int n_tiles, int nonmax, uint8_t* __restrict__ surv,
                                                      unsigned* __restrict__ ctl) {
  __shared__ __attribute__((aligned(16))) uint8_t s_s[(FY + 2) * FROW];
  __shared__ unsigned s_hist[256];
  const int tid = threadIdx.x;
  const fast_tile tl = fast_tile_of(tiles_x, n_tiles);
  const uint8_t* in = score + blockIdx.z * px;
  s_hist[tid] = 0;
  for (int i = tid; i < (FY + 2) * (FX + 2); i += FT) {
    const int r = i / (FX + 2), c = i - r * (FX + 2);
    const int y = tl.y0 - 1 + r, x = tl.x0 - 1 + c;
    s_s[r * FROW + c] = (y >= 0 && y < H && x >= 0 && x < W) ? in[(size_t)y * W + x] : (uint8_t)0;
  }
  __syncthreads();
  const int lx = tid & (FX - 1), x = tl.x0 + lx;
  uint8_t* out = surv + blockIdx.z * px;
  if (x < W) {
#pragma unroll
    for (int k = 0; k < FY / (FT / FX); ++k) {
      const int ly = k * (FT / FX) + tid / FX, y = tl.y0 + ly;
      if (y >= H) break;
      const uint8_t* p = s_s + (ly + 1) * FROW + lx + 1;
      const int s = p[0];
      bool keep = s > 0;
      if (keep && nonmax) {
        const int before = max(max((int)p[-FROW - 1], (int)p[-FROW]), max((int)p[-FROW + 1], (int)p[-1]));
        const int after = max(max((int)p[1], (int)p[FROW - 1]), max((int)p[FROW], (int)p[FROW + 1]));
        keep = before < s && after <= s;
      }
      out[(size_t)y * W + x] = keep ? (uint8_t)s : (uint8_t)0;
      if (keep) atomicAdd(&s_hist[s], 1u);
    }
  }
  __syncthreads();
  // (nobody waits for the result; sixteen copies, because all of a frame's tiles adding into one copy -- a few dozen hot
  // scores -- queued at those addresses for most of the kernel's time: DESIGN.md 3.10)
  if (s_hist[tid]) atomicAdd(&ctl[(size_t)blockIdx.z * F_CTL + (blockIdx.x % F_COPIES) * 256 + tid], s_hist[tid]);
}

// The cut of one image from its histogram, by a workgroup of 256: total survivors, n = min(N, total), the cutting score
// c -- the one score with (survivors above c) < n <= (survivors at or above c) -- and k, how many of score c are taken.
// No survivors: c = 256, which no byte reaches, and k = 0.  Ends with every work item past its last barrier and leaves
// s_scan[t] = the survivors of score t or more.
struct fast_cut_t {
  int c, k, n, total;
};
__device__ __forceinline__ fast_cut_t fast_cut(const unsigned* __restrict__ hist, int N, unsigned (&s_scan)[256]) {
  __shared__ int s_ck[2];
  const int tid = threadIdx.x;
  unsigned h = 0;
  if (tid) {                                                     // (score 0 is "no corner": never counted)
#pragma unroll
    for (int r = 0; r < F_COPIES; ++r) h += hist[r * 256 + tid];
  }
  s_scan[tid] = h;
  if (tid == 0) {
    s_ck[0] = 256;
    s_ck[1] = 0;
  }
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {                      // s_scan[t] = survivors of score >= t
    const unsigned add = tid + off < 256 ? s_scan[tid + off] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  const unsigned incl = s_scan[tid], total = s_scan[0];
  const unsigned n = min((unsigned)N, total);
  if (h > 0 && incl - h < n && n <= incl) {                      // (exactly one score when n > 0)
    s_ck[0] = tid;
    s_ck[1] = (int)(n - (incl - h));
  }
  __syncthreads();
  return {s_ck[0], s_ck[1], (int)n, (int)total};
}

__global__ __launch_bounds__(FT) void fast_rows_kernel(const uint8_t* __restrict__ surv, size_t px, int H, int W, int N,
                                                       const unsigned* __restrict__ ctl, uint2* __restrict__ rows) {
  __shared__ unsigned s_scan[256];
  const fast_cut_t cut = fast_cut(ctl + (size_t)blockIdx.z * F_CTL, N, s_scan);
  const int lane = threadIdx.x & 63, y = blockIdx.x * F_ROWS + (threadIdx.x >> 6);
  if (y >= H) return;
  const uint8_t* row = surv + blockIdx.z * px + (size_t)y * W;
  unsigned above = 0, at = 0;
  for (int xb = lane; xb < W; xb += 4 * 64) {                    // (four loads in flight)
    int v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = xb + 64 * u < W ? row[xb + 64 * u] : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      above += v[u] > cut.c ? 1u : 0u;
      at += v[u] == cut.c ? 1u : 0u;                             // (c >= 1 or c = 256: a 0 is never at the cut)
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    above += __shfl_xor(above, off);
    at += __shfl_xor(at, off);
  }
  if (lane == 0) rows[(size_t)blockIdx.z * H + y] = make_uint2(above, at);
}

// Row y's selected survivors are all of its survivors above c and those of score c whose rank among the image's
// survivors of score c, in index order, is below k.  With A and T the survivors above / at c in the rows before y, the
// rows before y have selected A + min(k, T): that is where row y's begin in the list, which so comes out in index order.
__global__ __launch_bounds__(FT) void fast_select_kernel(const uint8_t* __restrict__ surv, size_t px, int H, int W, int N,
                                                         const unsigned* __restrict__ ctl, const uint2* __restrict__ rows,
                                                         unsigned* __restrict__ sel_idx, uint8_t* __restrict__ sel_score,
                                                         int N4) {
  __shared__ unsigned s_part[F_ROWS][2];
  __shared__ unsigned s_scan[256];
  const fast_cut_t cut = fast_cut(ctl + (size_t)blockIdx.z * F_CTL, N, s_scan);
  if (cut.n == 0) return;                                        // (uniform over the workgroup)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int y0 = blockIdx.x * F_ROWS;
  const uint2* rw = rows + (size_t)blockIdx.z * H;
  unsigned A = 0, T = 0;
  for (int y = tid; y < y0; y += FT) {
    const uint2 r = rw[y];
    A += r.x;
    T += r.y;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    A += __shfl_xor(A, off);
    T += __shfl_xor(T, off);
  }
  if (lane == 0) {
    s_part[wv][0] = A;
    s_part[wv][1] = T;
  }
  __syncthreads();
  A = T = 0;
#pragma unroll
  for (int w = 0; w < F_ROWS; ++w) {
    A += s_part[w][0];
    T += s_part[w][1];
  }
  const int y = y0 + wv;
  if (y >= H) return;
  for (int yy = y0; yy < y; ++yy) {
    A += rw[yy].x;
    T += rw[yy].y;
  }
  const uint2 mine = rw[y];
  if (mine.x == 0 && mine.y == 0) return;
  const unsigned k = (unsigned)cut.k;
  unsigned base = A + min(k, T);
  const uint8_t* row = surv + blockIdx.z * px + (size_t)y * W;
  unsigned* out_idx = sel_idx + (size_t)blockIdx.z * N;
  uint8_t* out_score = sel_score + (size_t)blockIdx.z * N4;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int xq = 0; xq < W; xq += 4 * 64) {                       // (four loads in flight; a chunk past the row holds zeros)
    int vq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) vq[u] = xq + 64 * u + lane < W ? row[xq + 64 * u + lane] : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int x = xq + 64 * u + lane, v = vq[u];
      const bool at = v == cut.c;                                  // (c >= 1 here: a 0 is never at the cut)
      const unsigned long long b_at = __ballot(at);
      const bool sel = v > cut.c || (at && T + (unsigned)__popcll(b_at & below) < k);
      const unsigned long long b_sel = __ballot(sel);
      const unsigned pos = base + (unsigned)__popcll(b_sel & below);
      if (sel && pos < (unsigned)N) {                              // (pos < n by the counts above; the test keeps the stores in bounds)
        out_idx[pos] = (unsigned)((size_t)y * W + x);
        out_score[pos] = (uint8_t)v;
      }
      base += (unsigned)__popcll(b_sel);
      T += (unsigned)__popcll(b_at);
    }
  }
}

// The selected survivors are listed in index order, so entry i's row in the order (score descending, index ascending) is
// the survivors of higher score -- all of them selected, and counted by the histogram -- plus the entries before i of
// the same score.  A workgroup of 256 entries counts the scores of the entries before its first in an LDS histogram and
// compares its own 256 score bytes among themselves, four per word.  (The first shape ranked 64-bit keys
// (255 - score) << 32 | index against all n keys, the second compared every earlier score byte: 32 us and 11 us at
// n = 2000, a few waves each alone on its SIMD walking the whole list.)
__device__ __forceinline__ unsigned fast_zero_bytes(unsigned x) {
  const unsigned t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;             // bit 7 of a byte: its low seven bits are not all 0
  return (unsigned)__popc(~(t | x | 0x7f7f7f7fu));
}

constexpr int F_NMAX = 16384;
__global__ __launch_bounds__(FT) void fast_order_kernel(const unsigned* __restrict__ sel_idx, const uint8_t* __restrict__ sel_score,
                                                        int N, int N4, int W, const unsigned* __restrict__ ctl,
                                                        double* __restrict__ kp_xy, size_t xy_stride,
                                                        uint8_t* __restrict__ kp_score, int32_t* __restrict__ d_n,
                                                        int32_t* __restrict__ d_total) {
  __shared__ unsigned s_scan[256], s_before[256];
  __shared__ unsigned s_sc[FT / 4];
  const int tid = threadIdx.x;
  s_before[tid] = 0;                                             // (fast_cut's barriers come before the first add)
  const fast_cut_t cut = fast_cut(ctl + (size_t)blockIdx.z * F_CTL, N, s_scan);
  const int n = cut.n;
  if (blockIdx.x == 0 && tid == 0) {
    d_n[blockIdx.z] = n;
    if (d_total) d_total[blockIdx.z] = cut.total;
  }
  const int first = blockIdx.x * FT;
  if (first >= n) return;                                        // (uniform over the workgroup)
  const unsigned* sc = reinterpret_cast<const unsigned*>(sel_score + (size_t)blockIdx.z * N4);
  for (int w = tid; w < first / 4; w += FT) {
    const unsigned q = sc[w];
    atomicAdd(&s_before[q & 0xffu], 1u);
    atomicAdd(&s_before[(q >> 8) & 0xffu], 1u);
    atomicAdd(&s_before[(q >> 16) & 0xffu], 1u);
    atomicAdd(&s_before[q >> 24], 1u);
  }
  const int own = min(n - first, FT);                            // (bytes at and past n in the last word are never looked at)
  if (tid < (own + 3) / 4) s_sc[tid] = sc[first / 4 + tid];
  __syncthreads();
  if (tid >= own) return;
  const int i = first + tid;
  const unsigned s = (s_sc[tid >> 2] >> (8 * (tid & 3))) & 0xffu, pat = s * 0x01010101u;
  unsigned same = s_before[s];
  for (int w = 0; w < (tid >> 2); ++w) same += fast_zero_bytes(s_sc[w] ^ pat);
  if (tid & 3) same += fast_zero_bytes((s_sc[tid >> 2] ^ pat) | (0xffffffffu << (8 * (tid & 3))));
  const unsigned rank = (s < 255u ? s_scan[s + 1] : 0u) + same;
  if (rank < (unsigned)n) {
    const unsigned idx = sel_idx[(size_t)blockIdx.z * N + i];
    const unsigned y = idx / (unsigned)W, x = idx - y * (unsigned)W;
    double* o = kp_xy + ((size_t)blockIdx.z * xy_stride + rank) * 2;
    o[0] = (double)x;
    o[1] = (double)y;
    if (kp_score) kp_score[(size_t)blockIdx.z * xy_stride + rank] = (uint8_t)s;
  }
}

// ---- host side ----
struct fast_call {                 // the arguments of vo_fast_keypoints_batch_dev, in its order
  const uint8_t* d_imgs;
  size_t img_stride;
  int S, H, W, threshold, nonmax, N;
  double* d_kp_xy;
  size_t xy_stride;
  uint8_t* d_kp_score;
  int32_t *d_n, *d_total;
};

int fast_check_image(vo_ctx* ctx, const char* who, int S, int H, int W, int threshold) {
  VO_REQUIRE(ctx, H >= 1 && W >= 1, "%s: bad image size %d x %d", who, H, W);
  VO_REQUIRE(ctx, (size_t)H * W < 0x80000000ull, "%s: %d x %d pixels exceed the 31-bit index", who, H, W);
  VO_REQUIRE(ctx, threshold >= 0 && threshold <= 254, "%s: threshold = %d, must be 0 .. 254", who, threshold);
  VO_REQUIRE(ctx, S >= 1 && S <= 65535, "%s: S = %d, must be 1 .. 65535", who, S);
  return VO_OK;
}

int fast_check_cut(vo_ctx* ctx, const char* who, int nonmax, int N) {
  VO_REQUIRE(ctx, nonmax == 0 || nonmax == 1, "%s: nonmax = %d, must be 0 or 1", who, nonmax);
  VO_REQUIRE(ctx, N >= 1 && N <= F_NMAX, "%s: N = %d, must be 1 .. %d", who, N, F_NMAX);
  return VO_OK;
}

// the score maps of S images into scratch[0]
int fast_score_stage(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, int threshold) {
  const size_t px = (size_t)H * W;
  VO_TRY(vo_ensure(ctx, ctx->scratch[0], (size_t)S * px));
  const int tiles_x = vo_cdiv(W, FX), n_tiles = tiles_x * vo_cdiv(H, FY);
  hipLaunchKernelGGL(fast_score_kernel, dim3(n_tiles, 1, S), dim3(FT), 0, ctx->stream, d_imgs, img_stride, H, W, tiles_x,
                     n_tiles, threshold, (uint8_t*)ctx->scratch[0].p, px);
  return vo_check_launch(ctx, "fast_score_kernel");
}

int fast_run(vo_ctx* ctx, const char* who, const fast_call& c) {
  VO_REQUIRE(ctx, c.d_imgs && c.d_kp_xy && c.d_n, "%s: null pointer", who);
  VO_TRY(fast_check_image(ctx, who, c.S, c.H, c.W, c.threshold));
  VO_TRY(fast_check_cut(ctx, who, c.nonmax, c.N));
  const size_t px = (size_t)c.H * c.W, Sz = (size_t)c.S;
  VO_REQUIRE(ctx, c.img_stride >= px, "%s: img_stride %zu is below H * W = %zu", who, c.img_stride, px);
  VO_REQUIRE(ctx, c.xy_stride >= (size_t)c.N, "%s: xy_stride %zu is below N = %d", who, c.xy_stride, c.N);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[1], Sz * F_CTL * 4));
  VO_TRY(vo_ensure(ctx, s[2], Sz * px));
  VO_TRY(vo_ensure(ctx, s[3], Sz * c.H * sizeof(uint2)));
  const int N4 = (c.N + 3) & ~3;                                 // (an image's score bytes start on a word)
  VO_TRY(vo_ensure(ctx, s[4], Sz * c.N * 4));
  VO_TRY(vo_ensure(ctx, s[5], Sz * N4));
  unsigned* d_ctl = (unsigned*)s[1].p;
  VO_HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, Sz * F_CTL * 4, st));
  VO_TRY(fast_score_stage(ctx, c.d_imgs, c.img_stride, c.S, c.H, c.W, c.threshold));
  const int tiles_x = vo_cdiv(c.W, FX), n_tiles = tiles_x * vo_cdiv(c.H, FY);
  hipLaunchKernelGGL(fast_nms_kernel, dim3(n_tiles, 1, c.S), dim3(FT), 0, st, (const uint8_t*)s[0].p, px, c.H, c.W, tiles_x,
                     n_tiles, c.nonmax, (uint8_t*)s[2].p, d_ctl);
  VO_TRY(vo_check_launch(ctx, "fast_nms_kernel"));
  const dim3 by_rows(vo_cdiv(c.H, F_ROWS), 1, c.S);
  hipLaunchKernelGGL(fast_rows_kernel, by_rows, dim3(FT), 0, st, (const uint8_t*)s[2].p, px, c.H, c.W, c.N,
                     (const unsigned*)d_ctl, (uint2*)s[3].p);
  VO_TRY(vo_check_launch(ctx, "fast_rows_kernel"));
  hipLaunchKernelGGL(fast_select_kernel, by_rows, dim3(FT), 0, st, (const uint8_t*)s[2].p, px, c.H, c.W, c.N,
                     (const unsigned*)d_ctl, (const uint2*)s[3].p, (unsigned*)s[4].p, (uint8_t*)s[5].p, N4);
  VO_TRY(vo_check_launch(ctx, "fast_select_kernel"));
  hipLaunchKernelGGL(fast_order_kernel, dim3(vo_cdiv(c.N, FT), 1, c.S), dim3(FT), 0, st, (const unsigned*)s[4].p,
                     (const uint8_t*)s[5].p, c.N, N4, c.W, (const unsigned*)d_ctl, c.d_kp_xy, c.xy_stride, c.d_kp_score, c.d_n, c.d_total);
  return vo_check_launch(ctx, "fast_order_kernel");
}

// Both host forms: the S images up, the stages on the context's own buffers, the counts and each image's n rows down.
int fast_host(vo_ctx* ctx, const char* who, const uint8_t* imgs, int S, int H, int W, int threshold, int nonmax, int N,
              double* kp_xy, uint8_t* kp_score, int32_t* n_out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, imgs && kp_xy && n_out, "%s: null pointer", who);
  VO_TRY(fast_check_image(ctx, who, S, H, W, threshold));
  VO_TRY(fast_check_cut(ctx, who, nonmax, N));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)H * W, Sz = (size_t)S, rows = (size_t)N;
  hipStream_t st = ctx->stream;
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, ctx->img, Sz * px));
  VO_TRY(vo_ensure(ctx, s[12], Sz * rows * 16));
  VO_TRY(vo_ensure(ctx, s[13], Sz * rows));
  VO_TRY(vo_ensure(ctx, s[14], Sz * 4));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, imgs, Sz * px, hipMemcpyHostToDevice, st));
  const fast_call c = {(const uint8_t*)ctx->img.p, px, S, H, W, threshold, nonmax, N, (double*)s[12].p, rows,
                       (uint8_t*)s[13].p, (int32_t*)s[14].p, nullptr};
  VO_TRY(fast_run(ctx, who, c));
  VO_HIP_TRY(ctx, hipMemcpyAsync(n_out, s[14].p, Sz * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int q = 0; q < S; ++q) {
    const size_t n = (size_t)n_out[q];
    if (n == 0) continue;
    VO_HIP_TRY(ctx, hipMemcpyAsync(kp_xy + (size_t)q * rows * 2, (const double*)s[12].p + (size_t)q * rows * 2, n * 16,
                                   hipMemcpyDeviceToHost, st));
    if (kp_score)
      VO_HIP_TRY(ctx, hipMemcpyAsync(kp_score + (size_t)q * rows, (const uint8_t*)s[13].p + (size_t)q * rows, n,
                                     hipMemcpyDeviceToHost, st));
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

}  // namespace

extern "C" {

int vo_fast_score(vo_ctx* ctx, const uint8_t* img, int H, int W, int threshold, uint8_t* score) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, img && score, "fast_score: null pointer");
  VO_TRY(fast_check_image(ctx, "fast_score", 1, H, W, threshold));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)H * W;
  VO_TRY(vo_ensure(ctx, ctx->img, px));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, img, px, hipMemcpyHostToDevice, ctx->stream));
  VO_TRY(fast_score_stage(ctx, (const uint8_t*)ctx->img.p, px, 1, H, W, threshold));
  VO_HIP_TRY(ctx, hipMemcpyAsync(score, ctx->scratch[0].p, px, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VO_OK;
}

int vo_fast_keypoints(vo_ctx* ctx, const uint8_t* img, int H, int W, int threshold, int nonmax, int N, double* kp_xy,
                      uint8_t* kp_score, int32_t* n) {
  return fast_host(ctx, "fast_keypoints", img, 1, H, W, threshold, nonmax, N, kp_xy, kp_score, n);
}

int vo_fast_keypoints_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, int threshold, int nonmax, int N,
                            double* kp_xy, uint8_t* kp_score, int32_t* n) {
  return fast_host(ctx, "fast_keypoints_batch", imgs, S, H, W, threshold, nonmax, N, kp_xy, kp_score, n);
}

int vo_fast_keypoints_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, int threshold,
                                int nonmax, int N, double* d_kp_xy, size_t xy_stride, uint8_t* d_kp_score, int32_t* d_n,
                                int32_t* d_total) {
  if (!ctx) return VO_EINVAL;
  const fast_call c = {d_imgs, img_stride, S, H, W, threshold, nonmax, N, d_kp_xy, xy_stride, d_kp_score, d_n, d_total};
  return fast_run(ctx, "fast_keypoints_batch_dev", c);
}

}  // extern "C"
