// Structure refinement inside the frame loop (vo_hip.h, "Structure loop"): the last W observation records of every lane stay
// in a ring on the device, and one call per collected step queues record, window join, refinement and write-back on the
// pipeline's main stream.  The host never waits and reads nothing back; one further step may be in flight.
//
// Launches of one post (the lane is a grid dimension of every one of them; no grid barrier, no spin-wait, no floating-point
// atomics -- the integer atomics are the table's compare-and-swap / minimum and two counters):
//   copy               the post's per-lane words (activity, feature count, records since the reset, refined pose) from a
//                      pinned ring of four slots into HBM
//   memset             the id table of the ring slot the record goes to
//   sl_record_kernel   (cap / 256, S)  the record, through export_tracks_kernel's writers, into the lane's ring slot; the pose
//                      into the pose ring; every row's id into the slot's table
//   sl_join_kernel     (S) x 1024      header check, poses in age order, then the join: the rows of the newest record probe
//                      the W - 1 older tables, a workgroup scan gives every landmark its place, and the window is written
//   window_structure_kernel, window_structure_summary_kernel   vo_window_structure_dev, unchanged
//   sl_writeback_kernel (cap / 256, S) the entry's summary; with feedback the features that still carry the window's input
//   copy, event        the S entries into the pinned result ring
//
// The id table.  Ids are unique per lane between hand-overs, so a record is a map id -> row.  Each (ring slot, lane) has an
// open-addressing table of T >= 2 cap 64-bit words, (id << 32) | row, empty = all ones (no row index is 2^32 - 1).  A row is
// inserted at the first word from hash(id) on that is empty (compare-and-swap) or carries its id (atomicMin: the smaller
// row wins, "the first row carrying the id" whatever order the threads arrive in).  At most cap < T / 2 words are taken, so
// a probe sequence always ends at an empty word.  A collision -- two ids with one hash -- only lengthens the probe: the
// lookup compares the whole id, never the hash, so it returns exactly the first row of the record that carries the id or
// "none", which is what window_match_kernel's linear scan returns.  Which word an id ends up in depends on the order of
// arrival; what a lookup returns does not.
//
// The join is window_build_kernel's: both run vo_window_emit (window_join_device.h), this one with the tables as its finder,
// so the same prefix is kept and the same flag names what cut it.
//
// Stream edges.  Everything above is enqueued on the main stream by one host thread, in this order, behind the main-stream
// chain of the step in flight (k + 1) and in front of the chain of whatever is submitted next (k + 2): regroup(k + 2), the
// first kernel that reads `land` of the features step k + 1 left, runs behind the write-back.  The tracker stream of step
// k + 2 starts on evRegroup(k + 1), possibly before the write-back: it reads keypoints (vo_feat.kp), images and pyramids
// (klt.hip takes no landmark pointer); the detection and upload streams read images only.  So `land` is the only array the
// write-back writes and no kernel of another stream reads it.  The record kernel reads the features of step k, which step
// k + 1 only reads and which only step k + 2 overwrites -- the condition vo_pipeline_export_tracks_post_seq has.
//
// A step that faults (the sticky word of vo_seq_ctl; a logical flag) leaves its lane to the host path.  The write-back
// returns on that word like every kernel behind the step, and vo_pipeline_collect_all calls vo_structure_loop_requeue behind
// recover_step / continue_step and in front of the chains it enqueues again: the write-back runs once more for that lane
// alone, on the redone step's features, and the lane's entry is copied again.
#include <algorithm>

#include "pipeline.h"
#include "window_join_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int SL_T = 256;                  // threads per workgroup of the per-row kernels
constexpr int SL_JOIN_T = 1024;            // threads of the join's one workgroup per lane
constexpr int SL_PARAM_RING = 4;           // pinned slots of the per-post lane words
constexpr int SL_RESULT_RING = 64;         // posts whose entries stay readable
constexpr unsigned long long SL_EMPTY = ~0ull;

struct sl_lane {                           // what the host knows about a lane at a post
  int32_t active;                          // 0: idle, no record
  int32_t n;                               // the step's feature count (vo_step_result.n_tracked, clamped to the capacity)
  int32_t count;                           // records posted since the last reset, this one included
  int32_t reserved;
  double pose[12];                         // R_refined row-major, t_refined
};

struct sl_args {
  int S, W, cap, L_cap, M_cap, ring;       // ring: the slot this post's record goes to; age s is slot (ring + 1 + s) % W
  int logT;                                // table words per (slot, lane): 1 << logT
  size_t rec_words;                        // 8-byte words per record
  const sl_lane* lane;                     // [S]
  unsigned long long* rec;                 // [S][W][rec_words]
  unsigned long long* tab;                 // [W][S][1 << logT]
  double* pose_ring;                       // [S][W][12]
  const vo_cam* cams;                      // [S]
  const vo_seq_ctl* ctl;                   // [S]
  // the window, vo_window_structure_dev's arrays
  int32_t* head;                           // [S][4]
  double* K;                               // [S][9]
  double* poses;                           // [S][W][12]
  double* X;                               // [S][L_cap][3]
  double* X0;                              // [S][L_cap][3]   the window's input
  int32_t* lm_start;                       // [S][L_cap + 1]
  int32_t* obs_slot;                       // [S][M_cap]
  double* obs_xy;                          // [S][M_cap][2]
  int32_t* lm_id;                          // [S][L_cap]
  int32_t* lm_of_row;                      // [S][cap]        row of the newest record -> its landmark, -1: none
  vo_structure_result* res;                // [S][L_cap]
  vo_structure_summary* sum;               // [S]
  vo_structure_loop_entry* entry;          // [S]
};

__device__ __forceinline__ unsigned long long* sl_rec(const sl_args& a, size_t q, int slot) {
  return a.rec + (q * (size_t)a.W + (size_t)slot) * a.rec_words;
}

__device__ __forceinline__ unsigned long long* sl_tab(const sl_args& a, size_t q, int slot) {
  return a.tab + (((size_t)slot * (size_t)a.S + q) << a.logT);
}

__device__ __forceinline__ unsigned sl_hash(int id, int logT) { return ((unsigned)id * 2654435761u) >> (32 - logT); }

__device__ __forceinline__ void sl_insert(unsigned long long* tab, int logT, int id, int row) {
  const unsigned mask = (1u << logT) - 1u;
  const unsigned long long mine = ((unsigned long long)(unsigned)id << 32) | (unsigned long long)(unsigned)row;
  unsigned h = sl_hash(id, logT);
  for (unsigned k = 0; k <= mask; ++k, h = (h + 1u) & mask) {
    unsigned long long cur = tab[h];
    if (cur == SL_EMPTY) {
      cur = atomicCAS(&tab[h], SL_EMPTY, mine);
      if (cur == SL_EMPTY) return;
    }
    if ((unsigned)(cur >> 32) == (unsigned)id) {
      atomicMin(&tab[h], mine);
      return;
    }
  }
}

// the first row that carries `id`, -1 when none does
__device__ __forceinline__ int sl_lookup(const unsigned long long* tab, int logT, int id) {
  const unsigned mask = (1u << logT) - 1u;
  unsigned h = sl_hash(id, logT);
  for (unsigned k = 0; k <= mask; ++k, h = (h + 1u) & mask) {
    const unsigned long long cur = tab[h];
    if (cur == SL_EMPTY) return -1;
    if ((unsigned)(cur >> 32) == (unsigned)id) return (int)(unsigned)cur;
  }
  return -1;
}

// The observation record of the step collected last (track_record_device.h: export_tracks_kernel's writers) into ring slot
// a.ring of lane blockIdx.y, its pose into the pose ring, its ids into the slot's table.  F: the features that step left;
// par: where its regroup left next_id / the step counter.
__global__ __launch_bounds__(SL_T) void sl_record_kernel(sl_args a, vo_feat Fall, int par) {
  const size_t q = blockIdx.y;
  if (!a.lane[q].active) return;
  const int n = a.lane[q].n;
  const vo_feat F = vo_feat_seq(Fall, q);
  const vo_seq_ctl* ctl = a.ctl + q;
  unsigned long long* rec = sl_rec(a, q, a.ring);
  const int i = blockIdx.x * SL_T + threadIdx.x;
  if (i == 0) vo_track::write_header(rec, n, ctl->id_step[par], ctl->next_id[par], (int)q);
  if (blockIdx.x == 0 && threadIdx.x < 12) a.pose_ring[(q * (size_t)a.W + (size_t)a.ring) * 12 + threadIdx.x] = a.lane[q].pose[threadIdx.x];
  if (i >= min(n, a.cap)) return;
  const int id = vo_track::write_row(rec, F, i);
  sl_insert(sl_tab(a, q, a.ring), a.logT, id, i);
}

// One workgroup per lane: the header check, the window's poses and intrinsics, and the join (window_join_device.h) with the
// older records' id tables as its finder.
__global__ __launch_bounds__(SL_JOIN_T) void sl_join_kernel(sl_args a) {
  __shared__ int s_full, s_step;
  __shared__ vo_window_lds<SL_JOIN_T> s_win;
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const sl_lane ln = a.lane[q];
  const int W = a.W;
  int32_t* const head = a.head + 4 * q;
  int32_t* const lm_start = a.lm_start + q * ((size_t)a.L_cap + 1);
  if (tid == 0) {
    // full iff W records since the reset, every step counter one above its predecessor's, no next_id below it
    // (vo/landmarks/window_ba.py, _headers): the host counts, the headers are read here
    int full = ln.active && ln.count >= W;
    int step = -1;
    if (ln.active) step = vo_track::step(sl_rec(a, q, a.ring));
    if (full) {
      int ps = 0, pn = 0;
      for (int s = 0; s < W; ++s) {
        const unsigned long long* r = sl_rec(a, q, (a.ring + 1 + s) % W);
        const int st = vo_track::step(r), nx = vo_track::next_id(r);
        if (s > 0 && (st != ps + 1 || nx < pn)) full = 0;
        ps = st;
        pn = nx;
      }
    }
    s_full = full;
    s_step = step;
  }
  if (tid < 12 * W) {
    const int s = tid / 12, k = tid - 12 * s;
    a.poses[q * (size_t)W * 12 + tid] = a.pose_ring[(q * (size_t)W + (size_t)((a.ring + 1 + s) % W)) * 12 + k];
  } else if (tid >= 256 && tid < 256 + 9) {
    a.K[q * 9 + (tid - 256)] = a.cams[q].K[tid - 256];
  }
  __syncthreads();
  const int full = s_full;
  if (full)
    vo_window_emit<SL_JOIN_T>(
        s_win, W, a.cap, a.L_cap, a.M_cap, [&](int s) { return sl_rec(a, q, (a.ring + 1 + s) % W); },
        [&](int s, int id, int) { return sl_lookup(sl_tab(a, q, (a.ring + 1 + s) % W), a.logT, id); }, a.lm_id + q * (size_t)a.L_cap,
        a.X + q * (size_t)a.L_cap * 3, a.X0 + q * (size_t)a.L_cap * 3, lm_start, a.obs_slot + q * (size_t)a.M_cap,
        a.obs_xy + q * (size_t)a.M_cap * 2, a.lm_of_row + q * (size_t)a.cap);
  if (tid == 0) {
    const int L = full ? s_win.tot[0] : 0, M = full ? s_win.tot[1] : 0, flags = full ? s_win.tot[2] : 0;
    head[0] = L;
    head[1] = M;
    head[2] = flags;
    head[3] = 0;
    if (!full) lm_start[0] = 0;
    vo_structure_loop_entry e;
    e.step = s_step;
    e.full = full;
    e.L = L;
    e.M = M;
    e.flags = flags;
    e.n_written = 0;
    e.summary.L = e.summary.n_refused = e.summary.n_kept = e.summary.max_iterations = 0;
    e.summary.cost0 = e.summary.cost = 0.0;
    a.entry[q] = e;
  }
}

__device__ __forceinline__ bool sl_same3(const double* u, const double* v) {
  return __double_as_longlong(u[0]) == __double_as_longlong(v[0]) && __double_as_longlong(u[1]) == __double_as_longlong(v[1]) &&
         __double_as_longlong(u[2]) == __double_as_longlong(v[2]);
}

// Lane q0 + blockIdx.y: the summary into the lane's entry, and (feedback) the write-back into F, the features the newest
// step left: feature i takes the refined landmark of window landmark l iff its id is lm_id[l], its state is 2, l is kept and
// moved, and its landmark is still, bit for bit, the window's input.  The id goes through the newest record's table (id ->
// row) and lm_of_row (row -> landmark): no list is scanned.  A lane whose step faulted is left alone.
__global__ __launch_bounds__(SL_T) void sl_writeback_kernel(sl_args a, vo_feat Fall, int q0, int feedback) {
  const size_t q = (size_t)q0 + blockIdx.y;
  vo_structure_loop_entry* const e = a.entry + q;
  if (blockIdx.x == 0 && threadIdx.x == 0) e->summary = a.sum[q];
  if (!feedback || !e->full || a.head[4 * q] <= 0) return;
  const vo_seq_ctl* ctl = a.ctl + q;
  if (ctl->fault) return;
  const vo_feat F = vo_feat_seq(Fall, q);
  const int i = blockIdx.x * SL_T + threadIdx.x;
  if (i >= min(ctl->n, a.cap) || F.state[i] != 2) return;
  const int id = F.ids[i].x;
  const int r = sl_lookup(sl_tab(a, q, a.ring), a.logT, id);
  if (r < 0 || r >= a.cap) return;
  const int l = a.lm_of_row[q * (size_t)a.cap + r];
  if (l < 0 || l >= a.head[4 * q] || a.lm_id[q * (size_t)a.L_cap + l] != id) return;
  if (!a.res[q * (size_t)a.L_cap + l].kept) return;
  const double* Xn = a.X + (q * (size_t)a.L_cap + l) * 3;
  const double* Xi = a.X0 + (q * (size_t)a.L_cap + l) * 3;
  if (sl_same3(Xn, Xi) || !sl_same3(F.land + 3 * (size_t)i, Xi)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) F.land[3 * (size_t)i + k] = Xn[k];
  atomicAdd(&e->n_written, 1);
}

}  // namespace

struct vo_structure_loop {
  vo_pipeline* p = nullptr;
  vo_structure_loop_config cfg;
  sl_args a;
  std::vector<void*> dev_mem;
  sl_lane* h_lane = nullptr;                       // pinned [SL_PARAM_RING][S]
  sl_lane* d_lane = nullptr;
  vo_structure_loop_entry* h_entry = nullptr;      // pinned [SL_RESULT_RING][S]
  hipEvent_t ev[SL_RESULT_RING];                   // post j's entries are in h_entry[j % SL_RESULT_RING]
  std::vector<int> count;                          // [S] records since the last reset
  std::vector<char> posted;                        // [S] the last post carried a record of the lane
  long n_posts = 0;
  long pending_k = -1;                             // the flight the last post's write-back waits behind (-1: none was in flight)
  int pending_fbuf = 0;                            // the Features buffer it writes
  size_t tab_bytes = 0;                            // one ring slot's tables, all lanes
};

namespace {

template <typename T>
int sl_alloc(vo_structure_loop* lp, T** out, size_t count) {
  const size_t bytes = std::max(count * sizeof(T), (size_t)256);
  hipError_t e = hipMalloc((void**)out, bytes);
  if (e != hipSuccess) return vo_set_error(lp->p->ctx, VO_ENOMEM, "structure_loop: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
  lp->dev_mem.push_back((void*)*out);
  return VO_OK;
}

void sl_free(vo_structure_loop* lp) {
  if (!lp) return;
  vo_pipeline* p = lp->p;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  for (void* q : lp->dev_mem) (void)hipFree(q);
  if (lp->h_lane) (void)hipHostFree(lp->h_lane);
  if (lp->h_entry) (void)hipHostFree(lp->h_entry);
  for (hipEvent_t e : lp->ev)
    if (e) (void)hipEventDestroy(e);
  if (p->sloop == lp) p->sloop = nullptr;
  delete lp;
}

int sl_launch_writeback(vo_structure_loop* lp, int q0, int Sn) {
  vo_pipeline* p = lp->p;
  vo_ctx* ctx = p->ctx;
  {
    vo_prof_scope ps(ctx, VO_K_LOOP_WRITE);
    hipLaunchKernelGGL(sl_writeback_kernel, dim3(vo_cdiv(p->cap, SL_T), Sn), dim3(SL_T), 0, ctx->stream, lp->a, p->F[lp->pending_fbuf], q0,
                       lp->cfg.feedback ? 1 : 0);
  }
  return vo_check_launch(ctx, "sl_writeback_kernel");
}

}  // namespace

void vo_structure_loop_free(vo_pipeline* p) {
  if (p && p->sloop) sl_free(p->sloop);
}

// vo_pipeline_collect_all, lane q of flight k redone through the host path or continued: the write-back of the last post,
// which that lane's fault word kept out, once more for the lane alone, and its entry copied again
int vo_structure_loop_requeue(vo_pipeline* p, int q, long k) {
  vo_structure_loop* lp = p->sloop;
  if (!lp || lp->n_posts == 0 || lp->pending_k != k || !lp->posted[q]) return VO_OK;
  vo_ctx* ctx = p->ctx;
  VO_TRY(sl_launch_writeback(lp, q, 1));
  const long j = lp->n_posts - 1;
  const int rs = (int)(j % SL_RESULT_RING);
  VO_HIP_TRY(ctx, hipMemcpyAsync(lp->h_entry + (size_t)rs * p->S + q, lp->a.entry + q, sizeof(vo_structure_loop_entry),
                                 hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_TRY(ctx, hipEventRecord(lp->ev[rs], ctx->stream));
  return VO_OK;
}

extern "C" {

int vo_structure_loop_create(vo_pipeline* p, const vo_structure_loop_config* cfg, vo_structure_loop** out) {
  if (!p || !cfg || !out) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  *out = nullptr;
  VO_REQUIRE(ctx, p->cfg.track_ids != 0, "structure_loop: the pipeline was created without track_ids");
  VO_REQUIRE(ctx, p->cfg.tracker_mode == 0, "structure_loop: tracker_mode must be 0 (klt), the pipeline runs mode %d", p->cfg.tracker_mode);
  VO_REQUIRE(ctx, cfg->window >= 2 && cfg->window <= VO_WINDOW_WMAX, "structure_loop: window must be 2 .. %d records, got %d", VO_WINDOW_WMAX, cfg->window);
  VO_REQUIRE(ctx, !p->sloop, "structure_loop: the pipeline has a structure loop already");
  const int W = cfg->window, S = p->S, cap = p->cap;
  const int L_cap = cfg->L_cap ? cfg->L_cap : cap;
  VO_REQUIRE(ctx, L_cap >= 1 && L_cap <= (1 << 20), "structure_loop: L_cap must be 0 (the feature capacity) or 1 .. 1048576 landmarks, got %d", cfg->L_cap);
  const long long M_max = (long long)L_cap * W;
  const int M_cap = cfg->M_cap ? cfg->M_cap : (int)std::min(M_max, (long long)0x7fffffff);
  VO_REQUIRE(ctx, M_cap >= 1 && (long long)M_cap <= M_max, "structure_loop: M_cap must be 0 (L_cap * window) or 1 .. L_cap * window observations, got %d",
             cfg->M_cap);
  VO_REQUIRE(ctx, cap >= 1 && cap <= (1 << 20), "structure_loop: the pipeline's feature capacity %d is beyond 1048576 rows", cap);
  vo_lm_params lm;      // (the parameters both solvers share are refused here; the rest by the first post's vo_window_structure_dev)
  VO_TRY(vo_resolve_lm_params(ctx, "window_structure", cfg->params.max_iter, cfg->params.max_trials, cfg->params.huber_px, cfg->params.lambda0,
                              cfg->params.step_tol, &lm));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_structure_loop* lp = new vo_structure_loop();
  lp->p = p;
  lp->cfg = *cfg;
  lp->cfg.L_cap = L_cap;
  lp->cfg.M_cap = M_cap;
  for (hipEvent_t& e : lp->ev) e = nullptr;
  lp->count.assign((size_t)S, 0);
  lp->posted.assign((size_t)S, 0);
  sl_args& a = lp->a;
  memset(&a, 0, sizeof(a));
  a.S = S;
  a.W = W;
  a.cap = cap;
  a.L_cap = L_cap;
  a.M_cap = M_cap;
  a.logT = 4;
  while ((1 << a.logT) < 2 * cap) ++a.logT;
  a.rec_words = vo_track::record_words(cap);
  a.cams = p->d_cams;
  a.ctl = p->d_ctl;
  const size_t s = (size_t)S;
  lp->tab_bytes = (s << a.logT) * 8;
  int rc = VO_OK;
  auto ok = [&](int r) {
    if (rc == VO_OK) rc = r;
  };
  ok(sl_alloc(lp, &a.rec, s * W * a.rec_words));
  ok(sl_alloc(lp, &a.tab, ((s * W) << a.logT)));
  ok(sl_alloc(lp, &a.pose_ring, s * W * 12));
  ok(sl_alloc(lp, &lp->d_lane, s));
  ok(sl_alloc(lp, &a.head, s * 4));
  ok(sl_alloc(lp, &a.K, s * 9));
  ok(sl_alloc(lp, &a.poses, s * W * 12));
  ok(sl_alloc(lp, &a.X, s * L_cap * 3));
  ok(sl_alloc(lp, &a.X0, s * L_cap * 3));
  ok(sl_alloc(lp, &a.lm_start, s * ((size_t)L_cap + 1)));
  ok(sl_alloc(lp, &a.obs_slot, s * M_cap));
  ok(sl_alloc(lp, &a.obs_xy, s * M_cap * 2));
  ok(sl_alloc(lp, &a.lm_id, s * L_cap));
  ok(sl_alloc(lp, &a.lm_of_row, s * cap));
  ok(sl_alloc(lp, &a.res, s * L_cap));
  ok(sl_alloc(lp, &a.sum, s));
  ok(sl_alloc(lp, &a.entry, s));
  a.lane = lp->d_lane;
  if (rc == VO_OK && hipHostMalloc((void**)&lp->h_lane, SL_PARAM_RING * s * sizeof(sl_lane), hipHostMallocDefault) != hipSuccess)
    rc = vo_set_error(ctx, VO_ENOMEM, "structure_loop: hipHostMalloc failed");
  if (rc == VO_OK && hipHostMalloc((void**)&lp->h_entry, SL_RESULT_RING * s * sizeof(vo_structure_loop_entry), hipHostMallocDefault) != hipSuccess)
    rc = vo_set_error(ctx, VO_ENOMEM, "structure_loop: hipHostMalloc failed");
  for (int k = 0; rc == VO_OK && k < SL_RESULT_RING; ++k)
    if (hipEventCreateWithFlags(&lp->ev[k], hipEventDisableTiming) != hipSuccess) rc = vo_set_error(ctx, VO_EHIP, "structure_loop: hipEventCreate failed");
  // everything a kernel may read before it was written: zero rows, zero entries, empty windows
  hipStream_t st = ctx->stream;
  if (rc == VO_OK) {
    hipError_t e = hipMemsetAsync(a.rec, 0, s * W * a.rec_words * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.tab, 0xff, lp->tab_bytes * W, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.pose_ring, 0, s * W * 96, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.head, 0, s * 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.lm_start, 0, s * ((size_t)L_cap + 1) * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.res, 0, s * L_cap * sizeof(vo_structure_result), st);
    if (e == hipSuccess) e = hipMemsetAsync(a.sum, 0, s * sizeof(vo_structure_summary), st);
    if (e == hipSuccess) e = hipMemsetAsync(a.entry, 0, s * sizeof(vo_structure_loop_entry), st);
    if (e != hipSuccess) rc = vo_set_error(ctx, VO_EHIP, "structure_loop: hipMemsetAsync failed: %s", hipGetErrorString(e));
  }
  if (rc != VO_OK) {
    sl_free(lp);
    return rc;
  }
  p->sloop = lp;
  *out = lp;
  return VO_OK;
}

int vo_structure_loop_destroy(vo_structure_loop* lp) {
  if (!lp) return VO_OK;
  sl_free(lp);
  return VO_OK;
}

int vo_structure_loop_reset_seq(vo_structure_loop* lp, int seq) {
  if (!lp) return VO_EINVAL;
  VO_REQUIRE(lp->p->ctx, seq >= 0 && seq < lp->p->S, "structure_loop_reset: bad sequence index %d", seq);
  lp->count[(size_t)seq] = 0;
  return VO_OK;
}

int vo_structure_loop_post(vo_structure_loop* lp, const vo_step_result* results) {
  if (!lp || !results) return VO_EINVAL;
  vo_pipeline* p = lp->p;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->steps_submitted - p->n_flight > 0, "structure_loop_post: no step has been collected");
  VO_REQUIRE(ctx, p->n_flight <= 1, "structure_loop_post: two steps are in flight, the features of the step collected last are being overwritten");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int S = p->S, W = lp->a.W;
  const long j = lp->n_posts;
  // the pinned slots come round after four posts, the result slots after 64: those posts are long over (a post is over when a
  // step submitted after it has been collected), so neither wait blocks in a running loop
  if (j >= SL_PARAM_RING) VO_HIP_TRY(ctx, hipEventSynchronize(lp->ev[(j - SL_PARAM_RING) % SL_RESULT_RING]));
  if (j >= SL_RESULT_RING) VO_HIP_TRY(ctx, hipEventSynchronize(lp->ev[j % SL_RESULT_RING]));
  sl_lane* hl = lp->h_lane + (size_t)(j % SL_PARAM_RING) * S;
  for (int q = 0; q < S; ++q) {
    const vo_step_result& r = results[q];
    const bool active = !p->idle[q] && r.n_features_in != -1;
    lp->count[q] = active ? lp->count[q] + 1 : 0;
    lp->posted[q] = active ? 1 : 0;
    hl[q].active = active ? 1 : 0;
    hl[q].n = std::max(0, std::min((int)r.n_tracked, p->cap));
    hl[q].count = lp->count[q];
    hl[q].reserved = 0;
    memcpy(hl[q].pose, r.R_refined, 72);
    memcpy(hl[q].pose + 9, r.t_refined, 24);
  }
  sl_args& a = lp->a;
  a.ring = (int)(j % W);
  VO_HIP_TRY(ctx, hipMemcpyAsync(lp->d_lane, hl, (size_t)S * sizeof(sl_lane), hipMemcpyHostToDevice, st));
  VO_HIP_TRY(ctx, hipMemsetAsync((char*)a.tab + (size_t)a.ring * lp->tab_bytes, 0xff, lp->tab_bytes, st));
  {
    // (the features and the control-block slot of the step collected last: vo_pipeline_export_tracks_post_seq's reasoning)
    vo_prof_scope ps(ctx, VO_K_LOOP_RECORD);
    hipLaunchKernelGGL(sl_record_kernel, dim3(vo_cdiv(p->cap, SL_T), S), dim3(SL_T), 0, st, a, p->F[p->last_fbuf], (int)((p->last_k + 1) & 1));
  }
  VO_TRY(vo_check_launch(ctx, "sl_record_kernel"));
  {
    vo_prof_scope ps(ctx, VO_K_LOOP_JOIN);
    hipLaunchKernelGGL(sl_join_kernel, dim3(S), dim3(SL_JOIN_T), 0, st, a);
  }
  VO_TRY(vo_check_launch(ctx, "sl_join_kernel"));
  VO_TRY(vo_window_structure_dev(ctx, S, W, a.L_cap, a.M_cap, a.head, a.K, a.poses, a.X, a.lm_start, a.obs_slot, a.obs_xy, &lp->cfg.params,
                                 a.res, a.sum));
  // the features as the newest step leaves them: the step in flight's, or the collected step's when none is
  lp->pending_k = p->n_flight == 1 ? p->flight[0].k : -1;
  lp->pending_fbuf = p->cur;
  lp->n_posts = j + 1;
  VO_TRY(sl_launch_writeback(lp, 0, S));
  const int rs = (int)(j % SL_RESULT_RING);
  VO_HIP_TRY(ctx, hipMemcpyAsync(lp->h_entry + (size_t)rs * S, a.entry, (size_t)S * sizeof(vo_structure_loop_entry), hipMemcpyDeviceToHost, st));
  VO_HIP_TRY(ctx, hipEventRecord(lp->ev[rs], st));
  return VO_OK;
}

int vo_structure_loop_posts(vo_structure_loop* lp) { return lp ? (int)lp->n_posts : 0; }

int vo_structure_loop_poll(vo_structure_loop* lp, int post_index, int wait, vo_structure_loop_entry* entries) {
  if (!lp || !entries) return VO_EINVAL;
  vo_ctx* ctx = lp->p->ctx;
  VO_REQUIRE(ctx, post_index >= 0 && post_index < lp->n_posts, "structure_loop_poll: post %d was not made (%ld so far)", post_index, lp->n_posts);
  VO_REQUIRE(ctx, post_index >= lp->n_posts - SL_RESULT_RING, "structure_loop_poll: the entries of post %d are gone, the last %d are kept", post_index,
             SL_RESULT_RING);
  const int rs = post_index % SL_RESULT_RING;
  if (wait) {
    VO_HIP_TRY(ctx, hipEventSynchronize(lp->ev[rs]));
  } else {
    const hipError_t e = hipEventQuery(lp->ev[rs]);
    if (e == hipErrorNotReady) return 1;
    VO_HIP_TRY(ctx, e);
  }
  memcpy(entries, lp->h_entry + (size_t)rs * lp->p->S, (size_t)lp->p->S * sizeof(vo_structure_loop_entry));
  return VO_OK;
}

int vo_structure_loop_download_seq(vo_structure_loop* lp, int seq, int32_t* head, double* poses, int32_t* lm_start, int32_t* obs_slot,
                                   double* obs_xy, double* X_in, int32_t* lm_id, double* X, vo_structure_result* results,
                                   vo_structure_summary* summary, vo_structure_loop_entry* entry) {
  if (!lp) return VO_EINVAL;
  vo_pipeline* p = lp->p;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "structure_loop_download: bad sequence index %d", seq);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const sl_args& a = lp->a;
  const size_t q = (size_t)seq, L = (size_t)a.L_cap, M = (size_t)a.M_cap;
  auto get = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
  VO_HIP_TRY(ctx, get(head, a.head + 4 * q, 16));
  VO_HIP_TRY(ctx, get(poses, a.poses + q * a.W * 12, (size_t)a.W * 96));
  VO_HIP_TRY(ctx, get(lm_start, a.lm_start + q * (L + 1), (L + 1) * 4));
  VO_HIP_TRY(ctx, get(obs_slot, a.obs_slot + q * M, M * 4));
  VO_HIP_TRY(ctx, get(obs_xy, a.obs_xy + q * M * 2, M * 16));
  VO_HIP_TRY(ctx, get(X_in, a.X0 + q * L * 3, L * 24));
  VO_HIP_TRY(ctx, get(lm_id, a.lm_id + q * L, L * 4));
  VO_HIP_TRY(ctx, get(X, a.X + q * L * 3, L * 24));
  VO_HIP_TRY(ctx, get(results, a.res + q * L, L * sizeof(vo_structure_result)));
  VO_HIP_TRY(ctx, get(summary, a.sum + q, sizeof(vo_structure_summary)));
  VO_HIP_TRY(ctx, get(entry, a.entry + q, sizeof(vo_structure_loop_entry)));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

}  // extern "C"
