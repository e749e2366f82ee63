// BRIEF-256 binary descriptors with an optional 30-bin orientation, and a Hamming 2-nearest-neighbour matcher with the
// ratio / distance / first-come rule, for gfx950.  The definition is the project's own (include/vo_hip.h, "BRIEF-256";
// tests/brief_reference.py states it in NumPy): box sums of bytes, `<` on integers, integer moments, integer
// distances -- device and definition agree bit for bit on every input, with no margins.
//
// Floating point appears in exactly the two places the definition puts it: the centre floor(x + 0.5) of a float64
// keypoint (with its range test, which also refuses NaN and infinities), and the ratio test's one float64 multiply.
// Everything else in this file is integer arithmetic.  No grid barrier, no spin-wait, no workgroup waits for another.
#include <climits>

#include "vo_internal.h"
#include "brief_pattern.h"

namespace {

// ---- the pattern (tools/make_brief_pattern.py): 30 rotations x 256 tests x (ax, ay, bx, by) ----
constexpr int BR_BINS = VO_BRIEF_BINS, BR_PAIRS = VO_BRIEF_PAIRS;
static_assert(BR_BINS == 30 && BR_PAIRS == 256, "the kernels are written for 30 bins of 256 tests");
__device__ __attribute__((aligned(4))) const int8_t d_pattern[BR_BINS * BR_PAIRS * 4] = VO_BRIEF_PATTERN_INIT;
__constant__ int c_cos[BR_BINS] = VO_BRIEF_COS_INIT;
__constant__ int c_sin[BR_BINS] = VO_BRIEF_SIN_INIT;
const int8_t h_pattern[BR_BINS * BR_PAIRS * 4] = VO_BRIEF_PATTERN_INIT;

// ---- describe: one wave per keypoint, four keypoints per workgroup ----
constexpr int BR_T = 256, BR_WAVES = BR_T / 64;
constexpr int BR_REACH = 16;                 // rotated offsets stay within 14 (the generator asserts it), the 5 x 5 box adds 2
constexpr int BR_WIN = 2 * BR_REACH + 1;     // 33 x 33 bytes of the zero-padded image
constexpr int BR_ROW = 36;                   // bytes between the window's rows in LDS: every row starts on a dword
constexpr int BR_DISC = 15;                  // radius of the orientation moments

// S of the window offset (ox, oy) from the centre, |ox|, |oy| <= 14: five rows of five bytes.  A row's five bytes start at
// column c0 = ox + 14 (0 .. 28) and lie in the two dwords from c0 & ~3 on (the second ends at byte 35 at most: inside the
// row's stride, and what it holds past column 32 is shifted out); four of them are summed by one byte dot product.
__device__ __forceinline__ unsigned box_sum(const uint8_t* win, int ox, int oy) {
  const int c0 = ox + BR_REACH - 2, r0 = oy + BR_REACH - 2;
  const unsigned* row = reinterpret_cast<const unsigned*>(win + r0 * BR_ROW + (c0 & ~3));
  const int sh = 8 * (c0 & 3);
  unsigned s = 0;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const unsigned long long v = (((unsigned long long)row[dy * (BR_ROW / 4) + 1] << 32) | row[dy * (BR_ROW / 4)]) >> sh;
    s = __builtin_amdgcn_udot4((unsigned)v, 0x01010101u, s + ((unsigned)(v >> 32) & 0xffu), false);
  }
  return s;
}

// The window goes to LDS with the zero padding applied on load, so a keypoint near or beyond the border needs no other
// path: a centre whose window misses the image reads zeros, gives box sums of 0, no bit set and bin 0 -- which is what
// the definition asks for outside [-16, W + 16) x [-16, H + 16).  A centre the range test refuses (and a wave past N) is
// moved to (-64, -64), where the window lies outside every image; that keeps every wave on one path to the barrier.
// blockIdx.y = image: its bytes at img + y * img_stride, its keypoints at kp_xy + y * xy_stride * 2, its descriptors at
// desc + y * desc_stride (bytes), its bins at bin + y * xy_stride.  d_n (nullable): the images' row counts, in device
// memory -- image y describes rows 0 .. min(max(d_n[y], 0), N) - 1, and a workgroup whose four rows all lie beyond that
// leaves before it loads anything (the whole workgroup takes the branch: nobody is left at the barrier).
__global__ __launch_bounds__(BR_T) void brief_describe_kernel(const uint8_t* __restrict__ img, size_t img_stride, int H, int W,
                                                              const double* __restrict__ kp_xy, size_t xy_stride,
                                                              const int* __restrict__ d_n, int N, int oriented,
                                                              uint8_t* __restrict__ desc, size_t desc_stride,
                                                              uint8_t* __restrict__ bin) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[BR_WAVES][BR_WIN * BR_ROW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (d_n) N = min(max(d_n[blockIdx.y], 0), N);
  if ((int)(blockIdx.x * BR_WAVES) >= N) return;
  if (blockIdx.y) {
    img += blockIdx.y * img_stride;
    kp_xy += blockIdx.y * xy_stride * 2;
    desc += blockIdx.y * desc_stride;
    if (bin) bin += blockIdx.y * xy_stride;
  }
  const int n = blockIdx.x * BR_WAVES + wv;
  int cx = -4 * BR_REACH, cy = -4 * BR_REACH;
  if (n < N) {
    const double fx = floor(kp_xy[2 * (size_t)n] + 0.5), fy = floor(kp_xy[2 * (size_t)n + 1] + 0.5);
    if (fx >= (double)-BR_REACH && fx < (double)W + BR_REACH && fy >= (double)-BR_REACH && fy < (double)H + BR_REACH) {
      cx = (int)fx;
      cy = (int)fy;
    }
  }
  // the tests of bin 0 are known before the window is: their table rows are on their way while it loads
  const char4* tab = reinterpret_cast<const char4*>(d_pattern);
  char4 p[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = tab[j * 64 + lane];
  uint8_t* win = s_win[wv];
  for (int i = lane; i < BR_WIN * BR_WIN; i += 64) {
    const int r = i / BR_WIN, c = i - r * BR_WIN;
    const int yy = cy - BR_REACH + r, xx = cx - BR_REACH + c;
    win[r * BR_ROW + c] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? img[(size_t)yy * W + xx] : (uint8_t)0;
  }
  __syncthreads();
  int k = 0;
  if (oriented) {
    // m10 = sum dx I, m01 = sum dy I over the disc of radius 15 on the raw window: |m| <= 255 * 15 * 709 < 2^31
    int m10 = 0, m01 = 0;
    constexpr int DW = 2 * BR_DISC + 1;
    for (int i = lane; i < DW * DW; i += 64) {
      const int r = i / DW, c = i - r * DW;
      const int dy = r - BR_DISC, dx = c - BR_DISC;
      if (dx * dx + dy * dy <= BR_DISC * BR_DISC) {
        const int v = win[(r + BR_REACH - BR_DISC) * BR_ROW + c + BR_REACH - BR_DISC];
        m10 += dx * v;
        m01 += dy * v;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      m10 += __shfl_xor(m10, off);
      m01 += __shfl_xor(m01, off);
    }
    // every lane takes the same 30-way argmax; a strict `>` leaves ties with the lowest bin (a flat patch: bin 0)
    long long top = LLONG_MIN;
    for (int b = 0; b < BR_BINS; ++b) {
      const long long v = (long long)m10 * c_cos[b] + (long long)m01 * c_sin[b];
      if (v > top) {
        top = v;
        k = b;
      }
    }
    if (k != 0) {                                          // (uniform over the wave)
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = tab[k * BR_PAIRS + j * 64 + lane];
    }
  }
  // lane l evaluates tests l, 64 + l, 128 + l, 192 + l, each box sum (at most 25 * 255 = 6375) straight from the window:
  // 512 of the 841 sums a table would hold are read at all.  Four wave ballots are the 256 bits, least significant first.
  unsigned long long bits[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned sa = box_sum(win, (signed char)p[j].x, (signed char)p[j].y);
    const unsigned sb = box_sum(win, (signed char)p[j].z, (signed char)p[j].w);
    bits[j] = __ballot(sa < sb);
  }
  if (n < N) {
    if (lane < 32) {
      const int j = lane >> 3;
      const unsigned long long w = j == 0 ? bits[0] : j == 1 ? bits[1] : j == 2 ? bits[2] : bits[3];
      desc[(size_t)n * 32 + lane] = (uint8_t)(w >> (8 * (lane & 7)));
    }
    if (lane == 0 && bin) bin[n] = (uint8_t)k;
  }
}

// ---- Hamming 2-NN ----
// A workgroup owns 8 queries; its 256 threads are 8 queries x 32 slices of the train set (thread = query + 8 * slice).
// The query row stays in registers; slice s takes train rows s, s + 32, ... and reads them where they lie: the eight
// slices of a wave read eight neighbouring rows (256 contiguous bytes at 32 bytes a row), the eight queries of a slice
// share one address, and the loads of several rows are in flight at once.  (Staging tiles of 256 rows through LDS was
// built first and measured: 25.9 us at 2000 x 2000 x 32 bytes, most of it the two barriers per tile with the next tile's
// loads behind them.  DESIGN.md 3.9.)  Each thread keeps its two smallest keys (distance << 32 | train index); the slices
// of a query meet by wave shuffles, the four waves in LDS.  The key is a total order on the train rows of a query (no two
// rows share an index), so the two smallest keys of the whole set are the two smallest of the union of any partial lists
// that each hold their own two smallest: the result depends neither on how rows are dealt to the slices nor on the order
// of the merge.
constexpr int HM_T = 256, HM_Q = 8, HM_SL = HM_T / HM_Q;

__device__ __forceinline__ void key_insert(unsigned long long& k0, unsigned long long& k1, unsigned long long k) {
  const unsigned long long lo = k < k0 ? k : k0, hi = k < k0 ? k0 : k;
  k0 = lo;
  k1 = hi < k1 ? hi : k1;
}

// WP: words of a row held in registers, 8 for rows up to 32 bytes, 16 above; the words past the row's own are zero.
// VEC: rows are exactly WP words and start on 16-byte boundaries, so a row is WP / 4 loads of four words.
// The sequences of a batch: where they lie and where their counts are (all strides 0 and no counts: one set, nq x nt)
struct hamming_batch {
  const int *d_nq = nullptr, *d_nt = nullptr;     // sequence z: d_nq[z * nq_stride] queries of the nq launched, likewise nt
  int nq_stride = 0, nt_stride = 0;
  size_t q_stride = 0, t_stride = 0;              // words between two sequences' first rows
};

// blockIdx.y = sequence: its lists at best / dist + y * 2 * nq.  A count is clamped to 0 .. the launched size; rows at and
// beyond it are neither read nor written, and a workgroup whose eight queries all lie beyond it leaves at once.
template <int WP, bool VEC>
__global__ __launch_bounds__(HM_T) void hamming_knn2_kernel(const unsigned* __restrict__ q, int nq, const unsigned* __restrict__ t,
                                                            int nt, int words, int* __restrict__ best, int* __restrict__ dist,
                                                            const hamming_batch hb) {
  __shared__ unsigned long long s_k[HM_Q][HM_T / 64][2];
  const int tid = threadIdx.x, qi = tid & (HM_Q - 1), sl = tid / HM_Q;
  const int q0 = blockIdx.x * HM_Q;
  {
    const size_t z = blockIdx.y;
    best += z * 2 * (size_t)nq;
    dist += z * 2 * (size_t)nq;
    q += z * hb.q_stride;
    t += z * hb.t_stride;
    if (hb.d_nq) nq = min(max(hb.d_nq[z * hb.nq_stride], 0), nq);
    if (hb.d_nt) nt = min(max(hb.d_nt[z * hb.nt_stride], 0), nt);
  }
  if (q0 >= nq) return;
  auto load_row = [&](const unsigned* __restrict__ base, size_t row, unsigned (&out)[WP]) {
    if constexpr (VEC) {
      const uint4* p = reinterpret_cast<const uint4*>(base + row * WP);
#pragma unroll
      for (int v = 0; v < WP / 4; ++v) {
        const uint4 x = p[v];
        out[4 * v] = x.x;
        out[4 * v + 1] = x.y;
        out[4 * v + 2] = x.z;
        out[4 * v + 3] = x.w;
      }
    } else {
#pragma unroll
      for (int w = 0; w < WP; ++w) out[w] = w < words ? base[row * words + w] : 0u;
    }
  };
  unsigned qw[WP];
  load_row(q, (size_t)min(q0 + qi, nq - 1), qw);           // (a thread past the last query works on a copy of it and writes nothing)
  unsigned long long k0 = ~0ull, k1 = ~0ull;
#pragma unroll 4
  for (int j = sl; j < nt; j += HM_SL) {
    unsigned tw[WP];
    load_row(t, (size_t)j, tw);
    unsigned d = 0;
#pragma unroll
    for (int w = 0; w < WP; ++w) d += (unsigned)__popc(qw[w] ^ tw[w]);
    key_insert(k0, k1, ((unsigned long long)d << 32) | (unsigned)j);
  }
  // the slices of a query inside a wave are HM_Q lanes apart
#pragma unroll
  for (int off = HM_Q; off < 64; off <<= 1) {
    const unsigned long long b0 = __shfl_xor(k0, off), b1 = __shfl_xor(k1, off);
    key_insert(k0, k1, b0);
    key_insert(k0, k1, b1);
  }
  if ((tid & 63) < HM_Q) {
    s_k[qi][tid >> 6][0] = k0;
    s_k[qi][tid >> 6][1] = k1;
  }
  __syncthreads();
  if (tid < HM_Q && q0 + tid < nq) {
    unsigned long long a0 = ~0ull, a1 = ~0ull;
    for (int s = 0; s < HM_T / 64; ++s) {
      key_insert(a0, a1, s_k[tid][s][0]);
      key_insert(a0, a1, s_k[tid][s][1]);
    }
    const int row = q0 + tid;
    best[2 * (size_t)row] = a0 == ~0ull ? -1 : (int)(a0 & 0xffffffffu);
    best[2 * (size_t)row + 1] = a1 == ~0ull ? -1 : (int)(a1 & 0xffffffffu);
    dist[2 * (size_t)row] = a0 == ~0ull ? 0 : (int)(a0 >> 32);
    dist[2 * (size_t)row + 1] = a1 == ~0ull ? 0 : (int)(a1 >> 32);
  }
}

// The pair list.  Query i passes when both neighbours exist, float64(d1) < ratio * float64(d2) (one IEEE multiply, strict)
// and d1 <= max_dist (max_dist >= 0).  A train row goes to the lowest query that passes with it (atomicMin, its returned
// value unused), and the pairs come out in query order through an ordered compaction, 1024 queries per round.  One
// workgroup per sequence (blockIdx.x): lists at best / dist + x * 2 * nq, owner table at owner + x * nt, pairs at
// pairs + x * 2 * nq, count in n_pairs[x]; the counts as in hamming_knn2_kernel.  The workgroup presets its own owner
// entries (above every query) before it contests them, so no launch in front of it has to.  match.hip's
// ratio_unique_kernel is the same rule on float32 square roots of float64 distances; integer distances and the
// distance limit need their own test, so the pass is written here.
constexpr int HR_T = 1024;
__global__ __launch_bounds__(HR_T) void hamming_ratio_unique_kernel(const int* __restrict__ best, const int* __restrict__ dist,
                                                                   int nq, int nt, double ratio, int max_dist,
                                                                   int* __restrict__ owner, int* __restrict__ pairs,
                                                                   int* __restrict__ n_pairs, const hamming_batch hb) {
  __shared__ int s_scan[HR_T];
  __shared__ int s_base;
  const int tid = threadIdx.x;
  {
    const size_t z = blockIdx.x;
    best += z * 2 * (size_t)nq;
    dist += z * 2 * (size_t)nq;
    pairs += z * 2 * (size_t)nq;
    owner += z * (size_t)nt;
    n_pairs += z;
    if (hb.d_nq) nq = min(max(hb.d_nq[z * hb.nq_stride], 0), nq);
    if (hb.d_nt) nt = min(max(hb.d_nt[z * hb.nt_stride], 0), nt);
  }
  if (nt < 2) nq = 0;                                     // (a pair needs both neighbours; the lists may not have been written)
  auto passes = [&](int i) -> bool {
    const int b0 = best[2 * (size_t)i], b1 = best[2 * (size_t)i + 1];
    if (b0 < 0 || b1 < 0) return false;
    const int d1 = dist[2 * (size_t)i], d2 = dist[2 * (size_t)i + 1];
    return (double)d1 < ratio * (double)d2 && (max_dist < 0 || d1 <= max_dist);
  };
  if (nq > 0)
    for (int j = tid; j < nt; j += HR_T) __hip_atomic_store(&owner[j], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) s_base = 0;
  __threadfence();
  __syncthreads();
  for (int i = tid; i < nq; i += HR_T)
    if (passes(i)) atomicMin(&owner[best[2 * (size_t)i]], i);
  __threadfence();
  __syncthreads();
  for (int base = 0; base < nq; base += HR_T) {
    const int i = base + tid;
    int keep = 0, b0 = -1;
    if (i < nq && passes(i)) {
      b0 = best[2 * (size_t)i];
      keep = __hip_atomic_load(&owner[b0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i ? 1 : 0;
    }
    s_scan[tid] = keep;
    __syncthreads();
    for (int off = 1; off < HR_T; off <<= 1) {
      const int add = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    const int pos = s_base + s_scan[tid] - keep;
    if (keep) {
      pairs[2 * (size_t)pos] = i;
      pairs[2 * (size_t)pos + 1] = b0;
    }
    __syncthreads();
    if (tid == HR_T - 1) s_base += s_scan[tid];
    __syncthreads();
  }
  if (tid == 0) *n_pairs = s_base;
}

bool row_bytes_ok(int row_bytes) { return row_bytes >= 4 && row_bytes <= 64 && (row_bytes & 3) == 0; }

int describe_check(vo_ctx* ctx, const void* img, int H, int W, const void* kp, int N, int oriented, const void* desc) {
  VO_REQUIRE(ctx, img && kp && desc, "brief_describe: null pointer");
  VO_REQUIRE(ctx, H > 0 && W > 0, "brief_describe: bad image size %d x %d", H, W);
  VO_REQUIRE(ctx, N >= 1 && N <= 16384, "brief_describe: N = %d, must be 1 .. 16384", N);
  VO_REQUIRE(ctx, oriented == 0 || oriented == 1, "brief_describe: oriented = %d, must be 0 or 1", oriented);
  return VO_OK;
}

int hamming_check(vo_ctx* ctx, const char* who, int nq, int nt, int row_bytes) {
  VO_REQUIRE(ctx, row_bytes_ok(row_bytes), "%s: row_bytes = %d, must be a multiple of 4 in 4 .. 64", who, row_bytes);
  VO_REQUIRE(ctx, nq >= 0 && nt >= 0, "%s: bad counts nq = %d, nt = %d", who, nq, nt);
  return VO_OK;
}

// the 2-NN lists of S sequences (hb: where they lie; S = 1 with an empty hb: one set of nq x nt rows)
int knn2_launch(vo_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int S, int row_bytes, int32_t* d_best,
                int32_t* d_dist, const hamming_batch& hb) {
  const int words = row_bytes / 4;
  // whole rows of 32 or 64 bytes on 16-byte boundaries are read four words at a time; every other shape word by word
  const bool vec = (words == 8 || words == 16) && (((uintptr_t)d_q | (uintptr_t)d_t) & 15) == 0 && ((hb.q_stride | hb.t_stride) & 3) == 0;
  const dim3 grid(vo_cdiv(nq, HM_Q), S), block(HM_T);
  const unsigned *uq = (const unsigned*)d_q, *ut = (const unsigned*)d_t;
  {
    vo_prof_scope ps(ctx, VO_K_HAMMING_KNN2);
    if (vec && words == 8)
      hipLaunchKernelGGL((hamming_knn2_kernel<8, true>), grid, block, 0, ctx->stream, uq, nq, ut, nt, words, (int*)d_best, (int*)d_dist, hb);
    else if (vec)
      hipLaunchKernelGGL((hamming_knn2_kernel<16, true>), grid, block, 0, ctx->stream, uq, nq, ut, nt, words, (int*)d_best, (int*)d_dist, hb);
    else if (words <= 8)
      hipLaunchKernelGGL((hamming_knn2_kernel<8, false>), grid, block, 0, ctx->stream, uq, nq, ut, nt, words, (int*)d_best, (int*)d_dist, hb);
    else
      hipLaunchKernelGGL((hamming_knn2_kernel<16, false>), grid, block, 0, ctx->stream, uq, nq, ut, nt, words, (int*)d_best, (int*)d_dist, hb);
  }
  return vo_check_launch(ctx, "hamming_knn2_kernel");
}

// the rows go up to scratch[0] / scratch[1], the lists are left in scratch[2] (best) and scratch[3] (dist); nq, nt >= 1
int hamming_host(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int row_bytes) {
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  VO_TRY(vo_ensure(ctx, s[0], (size_t)nq * row_bytes));
  VO_TRY(vo_ensure(ctx, s[1], (size_t)nt * row_bytes));
  VO_TRY(vo_ensure(ctx, s[2], (size_t)nq * 8));
  VO_TRY(vo_ensure(ctx, s[3], (size_t)nq * 8));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[0].p, q, (size_t)nq * row_bytes, hipMemcpyHostToDevice, ctx->stream));
  VO_HIP_TRY(ctx, hipMemcpyAsync(s[1].p, t, (size_t)nt * row_bytes, hipMemcpyHostToDevice, ctx->stream));
  return vo_hamming_knn2_dev(ctx, (const uint8_t*)s[0].p, nq, (const uint8_t*)s[1].p, nt, row_bytes, (int32_t*)s[2].p,
                             (int32_t*)s[3].p);
}

}  // namespace

extern "C" {

int vo_brief_pattern(int8_t* out) {
  if (!out) return VO_EINVAL;
  memcpy(out, h_pattern, sizeof(h_pattern));
  return VO_OK;
}

int vo_brief_describe_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, const double* d_kp_xy,
                                size_t xy_stride, const int32_t* d_n, int N, int oriented, uint8_t* d_desc, size_t desc_stride,
                                uint8_t* d_bin) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(describe_check(ctx, d_imgs, H, W, d_kp_xy, N, oriented, d_desc));
  VO_REQUIRE(ctx, d_n, "brief_describe_batch_dev: null pointer");
  VO_REQUIRE(ctx, S >= 1 && S <= 65535, "brief_describe_batch_dev: S = %d, must be 1 .. 65535", S);
  VO_REQUIRE(ctx, img_stride >= (size_t)H * W, "brief_describe_batch_dev: img_stride %zu is below H * W = %zu", img_stride,
             (size_t)H * W);
  VO_REQUIRE(ctx, xy_stride >= (size_t)N, "brief_describe_batch_dev: xy_stride %zu is below N = %d", xy_stride, N);
  VO_REQUIRE(ctx, desc_stride >= (size_t)N * 32, "brief_describe_batch_dev: desc_stride %zu is below 32 N = %zu", desc_stride,
             (size_t)N * 32);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  {
    vo_prof_scope ps(ctx, VO_K_BRIEF_DESCRIBE);
    hipLaunchKernelGGL(brief_describe_kernel, dim3(vo_cdiv(N, BR_WAVES), S), dim3(BR_T), 0, ctx->stream, d_imgs, img_stride, H, W,
                       d_kp_xy, xy_stride, (const int*)d_n, N, oriented, d_desc, desc_stride, d_bin);
  }
  return vo_check_launch(ctx, "brief_describe_kernel");
}

// (the batch kernel with one image and every row: no count is read)
int vo_brief_describe_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, const double* d_kp_xy, int N, int oriented,
                          uint8_t* d_desc, uint8_t* d_bin) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(describe_check(ctx, d_img, H, W, d_kp_xy, N, oriented, d_desc));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  {
    vo_prof_scope ps(ctx, VO_K_BRIEF_DESCRIBE);
    hipLaunchKernelGGL(brief_describe_kernel, dim3(vo_cdiv(N, BR_WAVES)), dim3(BR_T), 0, ctx->stream, d_img, (size_t)0, H, W,
                       d_kp_xy, (size_t)0, (const int*)nullptr, N, oriented, d_desc, (size_t)0, d_bin);
  }
  return vo_check_launch(ctx, "brief_describe_kernel");
}

int vo_brief_describe(vo_ctx* ctx, const uint8_t* img, int H, int W, const double* kp_xy, int N, int oriented, uint8_t* desc,
                      uint8_t* bin) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(describe_check(ctx, img, H, W, kp_xy, N, oriented, desc));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)H * W;
  VO_TRY(vo_ensure(ctx, ctx->img, n));
  VO_TRY(vo_ensure(ctx, ctx->kp, (size_t)N * 16));
  VO_TRY(vo_ensure(ctx, ctx->desc, (size_t)N * 33));           // descriptors, then bins
  uint8_t* d_desc = (uint8_t*)ctx->desc.p;
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->img.p, img, n, hipMemcpyHostToDevice, ctx->stream));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ctx->kp.p, kp_xy, (size_t)N * 16, hipMemcpyHostToDevice, ctx->stream));
  VO_TRY(vo_brief_describe_dev(ctx, (const uint8_t*)ctx->img.p, H, W, (const double*)ctx->kp.p, N, oriented, d_desc,
                               d_desc + (size_t)N * 32));
  VO_HIP_TRY(ctx, hipMemcpyAsync(desc, d_desc, (size_t)N * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (bin) VO_HIP_TRY(ctx, hipMemcpyAsync(bin, d_desc + (size_t)N * 32, (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VO_OK;
}

int vo_hamming_knn2_dev(vo_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int row_bytes, int32_t* d_best,
                        int32_t* d_dist) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(hamming_check(ctx, "hamming_knn2_dev", nq, nt, row_bytes));
  VO_REQUIRE(ctx, nq >= 1, "hamming_knn2_dev: no queries");
  VO_REQUIRE(ctx, d_q && d_best && d_dist && (d_t || nt == 0), "hamming_knn2_dev: null pointer");
  VO_REQUIRE(ctx, ((uintptr_t)d_q & 3) == 0 && ((uintptr_t)d_t & 3) == 0, "hamming_knn2_dev: rows must start on a 4-byte boundary");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return knn2_launch(ctx, d_q, nq, d_t, nt, 1, row_bytes, d_best, d_dist, hamming_batch());
}

int vo_match_hamming_batch_dev(vo_ctx* ctx, const uint8_t* d_q, size_t q_stride, const int32_t* d_nq, int nq_stride, int cap_q,
                               const uint8_t* d_t, size_t t_stride, const int32_t* d_nt, int nt_stride, int cap_t, int S,
                               int row_bytes, double ratio, int max_dist, int32_t* d_pairs, int32_t* d_npairs) {
  if (!ctx) return VO_EINVAL;
  const char* who = "match_hamming_batch_dev";
  VO_REQUIRE(ctx, row_bytes_ok(row_bytes), "%s: row_bytes = %d, must be a multiple of 4 in 4 .. 64", who, row_bytes);
  VO_REQUIRE(ctx, d_q && d_nq && d_t && d_nt && d_pairs && d_npairs, "%s: null pointer", who);
  VO_REQUIRE(ctx, cap_q >= 1 && cap_t >= 1 && cap_q <= (1 << 24) && cap_t <= (1 << 24), "%s: bad capacities cap_q = %d, cap_t = %d",
             who, cap_q, cap_t);
  VO_REQUIRE(ctx, S >= 1 && S <= 65535, "%s: S = %d, must be 1 .. 65535", who, S);
  VO_REQUIRE(ctx, ratio == ratio, "%s: ratio is not a number", who);
  VO_REQUIRE(ctx, ((uintptr_t)d_q & 3) == 0 && ((uintptr_t)d_t & 3) == 0 && (q_stride & 3) == 0 && (t_stride & 3) == 0,
             "%s: rows must start on a 4-byte boundary", who);
  VO_REQUIRE(ctx, S == 1 || (q_stride >= (size_t)cap_q * row_bytes && t_stride >= (size_t)cap_t * row_bytes),
             "%s: per-sequence blocks overlap", who);
  VO_REQUIRE(ctx, S == 1 || (nq_stride != 0 && nt_stride != 0), "%s: the sequences share a count", who);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_buf* s = ctx->scratch;
  const size_t Sz = (size_t)S;
  VO_TRY(vo_ensure(ctx, s[10], Sz * cap_q * 8));          // best
  VO_TRY(vo_ensure(ctx, s[11], Sz * cap_q * 8));          // dist
  VO_TRY(vo_ensure(ctx, s[12], Sz * cap_t * 4));          // owner of every train row, per sequence
  hamming_batch hb;
  hb.d_nq = (const int*)d_nq;
  hb.d_nt = (const int*)d_nt;
  hb.nq_stride = nq_stride;
  hb.nt_stride = nt_stride;
  hb.q_stride = q_stride / 4;
  hb.t_stride = t_stride / 4;
  VO_TRY(knn2_launch(ctx, d_q, cap_q, d_t, cap_t, S, row_bytes, (int32_t*)s[10].p, (int32_t*)s[11].p, hb));
  hipLaunchKernelGGL(hamming_ratio_unique_kernel, dim3(S), dim3(HR_T), 0, ctx->stream, (const int*)s[10].p, (const int*)s[11].p,
                     cap_q, cap_t, ratio, max_dist, (int*)s[12].p, (int*)d_pairs, (int*)d_npairs, hb);
  return vo_check_launch(ctx, "hamming_ratio_unique_kernel");
}

int vo_match_hamming_knn2(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int row_bytes, int32_t* best,
                          int32_t* dist) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(hamming_check(ctx, "match_hamming_knn2", nq, nt, row_bytes));
  VO_REQUIRE(ctx, nq == 0 || (best && dist), "match_hamming_knn2: null pointer");
  if (nq == 0) return VO_OK;
  if (nt == 0) {                                          // no neighbour at all: no kernel runs
    for (int i = 0; i < 2 * nq; ++i) {
      best[i] = -1;
      dist[i] = 0;
    }
    return VO_OK;
  }
  VO_REQUIRE(ctx, q && t, "match_hamming_knn2: null pointer");
  VO_TRY(hamming_host(ctx, q, nq, t, nt, row_bytes));
  VO_HIP_TRY(ctx, hipMemcpyAsync(best, ctx->scratch[2].p, (size_t)nq * 8, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipMemcpyAsync(dist, ctx->scratch[3].p, (size_t)nq * 8, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return VO_OK;
}

int vo_match_hamming_ratio(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int row_bytes, double ratio,
                           int max_dist, int32_t* pairs, int32_t* n_pairs) {
  if (!ctx) return VO_EINVAL;
  VO_TRY(hamming_check(ctx, "match_hamming_ratio", nq, nt, row_bytes));
  VO_REQUIRE(ctx, ratio == ratio, "match_hamming_ratio: ratio is not a number");
  VO_REQUIRE(ctx, pairs && n_pairs, "match_hamming_ratio: null pointer");
  *n_pairs = 0;
  if (nq == 0 || nt < 2) return VO_OK;                    // (a pair needs both neighbours)
  VO_REQUIRE(ctx, q && t, "match_hamming_ratio: null pointer");
  VO_TRY(hamming_host(ctx, q, nq, t, nt, row_bytes));
  vo_buf* s = ctx->scratch;
  hipStream_t st = ctx->stream;
  VO_TRY(vo_ensure(ctx, s[7], (size_t)nt * 4));           // owner of every train row
  VO_TRY(vo_ensure(ctx, s[8], (size_t)nq * 8 + 8));       // pairs, then their number
  int* d_pairs = (int*)s[8].p;
  int* d_n = d_pairs + (size_t)nq * 2;
  hipLaunchKernelGGL(hamming_ratio_unique_kernel, dim3(1), dim3(HR_T), 0, st, (const int*)s[2].p, (const int*)s[3].p, nq, nt,
                     ratio, max_dist, (int*)s[7].p, d_pairs, d_n, hamming_batch());
  VO_TRY(vo_check_launch(ctx, "hamming_ratio_unique_kernel"));
  int n = 0;
  VO_HIP_TRY(ctx, hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  if (n > 0) {
    VO_HIP_TRY(ctx, hipMemcpyAsync(pairs, d_pairs, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  *n_pairs = n;
  return VO_OK;
}

}  // extern "C"
