// Device-resident per-frame loop (vo_pipeline_*): the steady state of the reference driver
// (src/main.py:248-286, KLT tracker mode) as one chain of launches per frame, with the Features /
// State / RANSAC bookkeeping living in HBM (state.hip).  See include/vo_hip.h for the stage list.
//
// Streams of one step (frame k-1 -> k):
//   main   : regroup -> hypotheses+counts -> replay+refine+candidates+landmarks+record
//   tracker: pyramid(k) -> KLT(k)           needs regroup(k-1) only: runs beside the pose estimation of step k-1
//   detect : Harris response + NMS on k -- or, vo_pipeline_config.detector = 1, the reference's own Shi-Tomasi corners and
//            their count -- (enqueued by a worker thread; consumed by the NEXT step's re-detect.
//            The reference runs its detector only when fewer than 80 % of the tracks are left, klt.py:207-230; whether
//            that will be so for frame k is known one step too late for a launch without a host turn, so the chain is
//            launched for every frame and each sequence sits it out unless its track count is within `detect_margin`
//            of the limit.  A sequence that falls through the margin in one frame finds no keypoints: fault, host path.)
// Nothing on the main stream waits for the host: counts, the generator position, the accepted pose and
// the inlier mask are words in HBM that the next kernel reads.  The host only enqueues (at most two
// steps ahead: frame buffers rotate over three slots) and reads each step's result record from mapped
// memory.  The rare step the device cannot finish alone (a bounded draw NumPy might have rejected, fewer
// than 8 landmarks, the sequential rule not done after `hyp` samples) raises a sticky fault word: every
// later kernel leaves that sequence's state untouched, and vo_pipeline_collect redoes the step with the
// sequential host sampler (recover_step) before re-enqueueing what was behind it.
//
// Several sequences per GPU (vo_pipeline_config.sequences = S): S independent streams advance in lock
// step through the SAME launches -- every per-sequence buffer is S consecutive blocks, the sequence is
// the grid's extra dimension of every kernel.  The chain is latency-bound at one sequence
// (single-workgroup kernels, 127 us per step with the chip almost empty); S sequences cost about the same
// wall time per step until the image-wide kernels fill the chip.
#include "pipeline.h"

#pragma clang fp contract(off)

namespace {

// Does sequence q need the detector on the frame being submitted?  The count that decides is known one step later;
// what is known now is the count of the frame before (or already this frame's, when the step's regroup has run) and
// how many tracks the last step lost: the detector runs when the count, extrapolated by `losses` such losses, is below
// (redetect_fraction + detect_margin) * num_features.  (Round 2: four losses and a margin of 0.02 -- the detector then ran
// on 26 % of the forward stream's frames for the 4 % that re-detect; 2.5 and 0.01: 15-18 %, still no frame caught without
// its keypoints in ~4000 sequence-steps; 2 and 0.005: 12-14 % and one such frame.)  (The fields are read while a regroup may be writing them: any
// mix of old and new values is a usable guess, and a wrong guess is caught by the step that needs the keypoints.)
// n_det: what a re-detect step appended -- the detector's fixed count, or (< 0: a detector that counts its corners) the
// count itself, which _num_features has been since (klt.py:114).
__global__ __launch_bounds__(64) void detect_decide_kernel(const vo_seq_ctl* __restrict__ ctl, int S, double limit, int n_det,
                                                           int force, int* __restrict__ go, double losses) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= S) return;
  if (ctl[q].fault & VO_FAULT_IDLE) {  // (an idle lane: vo_pipeline_set_active_seq)
    go[q] = 0;
    return;
  }
  const int n2 = ctl[q].n2;
  const int lost = max(ctl[q].n_in - (ctl[q].redetected ? (n_det < 0 ? ctl[q].num_features : n_det) : 0) - n2, 0);
  go[q] = (force || limit < 0.0 || (limit > 0.0 && (double)n2 - losses * (double)lost < (double)ctl[q].num_features * limit)) ? 1 : 0;
}

// a step whose RANSAC loop wants another batch of hypotheses (VO_FAULT_CONTINUE) goes on: the fault word is cleared and the
// population is what the step's regroup counted (a later step's regroup, enqueued behind the open step, has zeroed n_p3p)
__global__ void ctl_resume_kernel(vo_seq_ctl* __restrict__ ctl) {
  ctl->fault = 0;
  ctl->n_p3p = ctl->n_tri;
}

// SIFT tracker mode: the new frame's keypoint rows (x, y, size, angle, response, octave; float) as the float64 pairs the
// regroup takes (sift.py:18 keeps kp.pt only)
__global__ __launch_bounds__(256) void sift_kp_f64_kernel(const float* __restrict__ rows, const int* __restrict__ n, int cap,
                                                          double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(*n, cap)) return;
  out[2 * i] = (double)rows[6 * i];
  out[2 * i + 1] = (double)rows[6 * i + 1];
}

// SIFT tracker mode, every keypoint (sift_cap = -1): a frame whose SIFT lists overflowed or that has more keypoints than the
// feature capacity (vo_sift_all_batch_dev's verdict != 0: its count is 0, its rows unwritten) makes the step a capacity
// fault before the matcher -- the regroup, the descriptor gather and the pose chain leave a faulted sequence alone.  (A
// fault of an earlier step, still open, stays: this step is enqueued again when that one is done, as at the regroup.)
__global__ void sift_fit_kernel(const int32_t* __restrict__ verdict, vo_seq_ctl* __restrict__ ctl) {
  if (threadIdx.x != 0 || ctl->fault || *verdict == 0) return;
  ctl->fault = VO_FAULT_CAPACITY;
  ctl->n_in = 0;
  ctl->redetected = 0;
  ctl->few = 0;
  ctl->n_p3p = 0;
}

// ... and the descriptors of the regrouped frame: row dst of the new Features = the new keypoint src_row[dst]'s
// (blockIdx.y = sequence: ctl + y, src_row + y * cap, src + y * src_stride, dst + y * dst_stride; bytes)
__global__ __launch_bounds__(256) void desc_gather_kernel(const uint8_t* __restrict__ src, const int* __restrict__ src_row,
                                                          const vo_seq_ctl* __restrict__ ctl, int cap, uint8_t* __restrict__ dst,
                                                          int row_words, size_t src_stride, size_t dst_stride) {
  if (blockIdx.y) {
    ctl += blockIdx.y;
    src_row += (size_t)blockIdx.y * cap;
    src += blockIdx.y * src_stride;
    dst += blockIdx.y * dst_stride;
  }
  if (ctl->fault) return;
  const int w = blockIdx.x * 256 + threadIdx.x;        // one 4-byte word of one row
  const int row = w / row_words, k = w - row * row_words;
  if (row >= min(ctl->n2, cap)) return;
  reinterpret_cast<unsigned*>(dst)[(size_t)row * row_words + k] =
      reinterpret_cast<const unsigned*>(src)[(size_t)src_row[row] * row_words + k];
}

// Shi-Tomasi re-detect (vo_pipeline_config.detector = 1), the chain's last kernel: the batched detector's corners of
// sequence blockIdx.y as the float64 pairs of its keypoint slot (whole pixel positions: exact), and its count -- -1 for a
// frame whose candidate lists overflowed (verdict != 0), which the step that needs the corners turns into a capacity fault.
// A sequence that sat the detection out keeps what its slot held.
__global__ __launch_bounds__(256) void st_close_kernel(const float* __restrict__ xy, size_t xy_stride, const int32_t* __restrict__ n,
                                                       const int32_t* __restrict__ over, const int* __restrict__ go, int cap,
                                                       double* __restrict__ kp, size_t kp_stride, int32_t* __restrict__ cnt) {
  const size_t q = blockIdx.y;
  if (!go[q]) return;
  const int m = over[q] ? -1 : min(n[q], cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) {
    kp[q * kp_stride + 2 * i] = (double)xy[q * xy_stride + 2 * i];
    kp[q * kp_stride + 2 * i + 1] = (double)xy[q * xy_stride + 2 * i + 1];
  }
  if (i == 0) cnt[q] = m;
}

// the caller's context's profiling flags onto side context q (whose launches this thread makes, or an idle worker)
void copy_prof(vo_ctx* q, const vo_ctx* from) {
  q->prof_on = from->prof_on;
  q->prof_kernel = from->prof_kernel;
  q->prof_every = from->prof_every;
}

void sync_prof(vo_pipeline* p) {
  for (vo_ctx* q : {p->det, p->trk}) copy_prof(q, p->ctx);
}

}  // namespace

// A failed launch sequence: the text goes to err_buf (the worker thread's private error text -- the pipeline context's
// buffer belongs to the caller's thread) or, without one, to the pipeline context
static int launch_error(vo_pipeline* p, char* err_buf, int rc, const char* what, const char* detail) {
  if (err_buf) {
    snprintf(err_buf, 256, "%s: %s", what, detail);
    return rc;
  }
  return vo_set_error(p->ctx, rc, "%s: %s", what, detail);
}

// ---- launches; (q0, Sn): sequences q0 .. q0 + Sn - 1 (all of them, or one when a step is redone) ----

// Harris + NMS (detector 1: Shi-Tomasi corners and their count, vo_good_features_batch_gated_dev + st_close_kernel, no mask:
// klt.py:216-222) of frame slot `frame` into keypoint slot `s` on the detection stream; evDet[s] when done (err_buf: see
// launch_error).  (q0, Sn): sequences q0 .. q0 + Sn - 1 (Sn = 0: all of them); an idle sequence's detector does not run
// (detect_decide_kernel), a forced one runs and says so in d_det_go
int enqueue_detection(vo_pipeline* p, int frame, int s, bool force, char* err_buf, int q0, int Sn) {
  const vo_pipeline_config& c = p->cfg;
  if (Sn <= 0) Sn = p->S - q0;
  p->det_flip ^= 1;
  vo_ctx* det = p->det;
  double* scores = p->d_scores[p->det_flip];
  det->nms_kp_f32 = nullptr;
  int* go = p->d_det_go + (size_t)s * p->S + q0;
  bool wait_ok = hipStreamWaitEvent(det->stream, p->evImg[frame], 0) == hipSuccess;   // the frame's upload (tracker's stream)
  if (wait_ok && p->n_pinned[frame] > 0) wait_ok = hipStreamWaitEvent(det->stream, p->evUp[frame], 0) == hipSuccess;   // (pinned)
  if (!wait_ok) return launch_error(p, err_buf, VO_EHIP, "detection", "hipStreamWaitEvent failed");
  hipLaunchKernelGGL(detect_decide_kernel, dim3(vo_cdiv(Sn, 64)), dim3(64), 0, det->stream, p->d_ctl + q0, Sn, p->detect_limit,
                     c.detector == 1 ? -1 : c.n_keypoints, force ? 1 : 0, go, p->detect_losses);
  int rc = vo_check_launch(det, "detect_decide_kernel");
  if (c.detector == 1) {
    vo_prof_scope ps(det, VO_K_SHI_TOMASI_CHAIN);      // (the whole chain, executing or gated out)
    const int N = c.n_keypoints;
    float* xy = p->d_st_xy + (size_t)q0 * N * 2;
    int32_t *n = p->d_st_n + q0, *over = p->d_st_n + p->S + q0;
    if (rc == VO_OK)
      rc = vo_good_features_batch_gated_dev(det, p->img(q0, frame), p->img_stride(), Sn, c.H, c.W, nullptr, 0, N, c.st_quality,
                                            c.st_min_distance, c.st_block, xy, (size_t)N, n, over, nullptr, p->st_rounds,
                                            VO_GFB_CANDIDATES, go);
    if (rc == VO_OK) {
      hipLaunchKernelGGL(st_close_kernel, dim3(vo_cdiv(N, 256), Sn), dim3(256), 0, det->stream, (const float*)xy, (size_t)N * 2,
                         (const int32_t*)n, (const int32_t*)over, (const int*)go, N, p->kp(q0, s), p->det_stride(),
                         p->d_det_cnt + (size_t)s * p->S + q0);
      rc = vo_check_launch(det, "st_close_kernel");
    }
    if (rc == VO_OK && hipEventRecord(p->evDet[s], det->stream) != hipSuccess) rc = VO_EHIP;
    return rc != VO_OK ? launch_error(p, err_buf, rc, "detection", vo_last_error(det)) : VO_OK;
  }
  if (rc == VO_OK)
    rc = vo_harris_response_batch_dev(det, p->img(q0, frame), p->img_stride(), Sn, c.H, c.W, c.harris_patch, c.harris_kappa,
                                      scores, go);
  if (rc == VO_OK)
    rc = vo_nms_keypoints_batch_dev(det, scores, Sn, c.H, c.W, c.n_keypoints, c.nms_radius, p->kp(q0, s), p->det_stride(),
                                    go);
  if (rc == VO_OK && hipEventRecord(p->evDet[s], det->stream) != hipSuccess) rc = VO_EHIP;
  return rc != VO_OK ? launch_error(p, err_buf, rc, "detection", vo_last_error(det)) : VO_OK;
}

// (q0, Sn): sequences q0 .. q0 + Sn - 1 (Sn = 0: all of them); idle sequences are left out -- one launch per run of active ones
static int enqueue_pyramid(vo_pipeline* p, int frame, int s, int q0 = 0, int Sn = 0) {
  if (s == p->prepared_slot) p->prepared_idx = p->prepared_slot = -1;      // (whatever vo_pipeline_prepare left there goes)
  if (p->n_pinned[frame] > 0 && hipStreamWaitEvent(p->trk->stream, p->evUp[frame], 0) != hipSuccess)   // (vo_pipeline_set_frame_pinned)
    return vo_set_error(p->ctx, VO_EHIP, "pyramid: hipStreamWaitEvent failed");
  const vo_pipeline_config& c = p->cfg;
  if (Sn <= 0) Sn = p->S - q0;
  for (int a = q0; a < q0 + Sn;) {
    if (p->idle[a]) {
      ++a;
      continue;
    }
    int b = a + 1;
    while (b < q0 + Sn && !p->idle[b]) ++b;
    const int rc = vo_pyramid_build_batch_dev(p->trk, p->img(a, frame), p->img_stride(), b - a, c.H, c.W, p->n_levels,
                                              p->pyr(a, s), p->pyr_stride());
    if (rc != VO_OK) return vo_set_error(p->ctx, rc, "pyramid: %s", vo_last_error(p->trk));
    a = b;
  }
  VO_HIP_TRY(p->ctx, hipEventRecord(p->evPyr[s], p->trk->stream));
  return VO_OK;
}

// keeps sequence q's ring of generator outputs filled ahead of every step that may be in flight
static int ensure_raws(vo_pipeline* p, int q) {
  vo_ctx* ctx = p->ctx;
  const uint64_t need = (uint64_t)7 * p->cfg.hyp;
  const uint64_t pos = std::max(p->pos_known[q], p->pos_dev[q]);
  if (p->gen_upto[q] >= pos + 4 * need) return VO_OK;
  const uint64_t target = pos + 16 * need;
  const size_t m = (size_t)(target - p->gen_upto[q]);        // <= stage_cap
  if (p->raw_pending) {
    VO_HIP_TRY(ctx, hipEventSynchronize(p->evRaw));          // the staging buffer's last copy (long done)
    p->raw_pending = false;
  }
  vo_rng_raw32(&p->raw_gen[q], (int)m, p->h_stage);
  uint32_t* ring = p->d_raws + (size_t)q * p->ring_len;
  const uint32_t off = (uint32_t)(p->gen_upto[q] & (p->ring_len - 1));
  const size_t first = std::min(m, (size_t)(p->ring_len - off));
  VO_HIP_TRY(ctx, hipMemcpyAsync(ring + off, p->h_stage, first * 4, hipMemcpyHostToDevice, ctx->stream));
  if (first < m)
    VO_HIP_TRY(ctx, hipMemcpyAsync(ring, p->h_stage + first, (m - first) * 4, hipMemcpyHostToDevice, ctx->stream));
  VO_HIP_TRY(ctx, hipEventRecord(p->evRaw, ctx->stream));
  p->raw_pending = true;
  p->gen_upto[q] = target;
  return VO_OK;
}

static vo_pose_job make_pose_job(vo_pipeline* p, const vo_feat& B, int do_replay, int q0) {
  const vo_pipeline_config& c = p->cfg;
  const size_t q = (size_t)q0;
  vo_pose_job j;
  j.ctl = p->d_ctl + q;
  j.rp.valid = p->d_valid + q * c.hyp;
  j.rp.counts = p->d_counts + q * c.hyp;
  j.rp.R = p->d_R + q * c.hyp * 9;
  j.rp.t = p->d_t + q * c.hyp * 3;
  j.rp.masks = (const unsigned long long*)p->d_masks + q * c.hyp * p->words;
  j.rp.words = p->words;
  j.rp.hyp = c.hyp;
  j.rp.table = p->d_table;
  j.rp.table_len = p->table_len;
  j.rp.max_it = c.ransac_max_iterations;
  j.rp.best_mask = (unsigned long long*)p->d_best_mask + q * p->words;
  j.do_replay = do_replay;
  j.B = vo_feat_seq(B, q);
  j.cam = p->d_cams + q;
  j.bearing_thr = c.bearing_threshold;
  j.max_iter = c.refine_iters;
  j.tail = 0;
  j.res = nullptr;
  j.seq_word = nullptr;
  j.seq = 0u;
  static const int stamps = getenv("VO_POSE_STAMPS") ? 1 : 0;
  j.stamps = stamps;
  j.debug_fault_every = 0;
  return j;
}

// tracker of one step, on its own stream: it needs the previous step's regroup (the features' positions) and this
// frame's pyramid, nothing of the previous step's pose estimation, which runs beside it on the main stream
static int enqueue_tracker(vo_pipeline* p, const vo_pipeline::flight_t& f, bool with_pyramid, int q0, int Sn) {
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  const vo_feat A = vo_feat_seq(p->F[f.fcur], (size_t)q0);
  hipStream_t ts = p->trk->stream;
  if (with_pyramid) VO_TRY(enqueue_pyramid(p, f.next_idx, f.b));
  if (f.k > 0 && hipEventQuery(p->evRegroup[(f.k - 1) & 1]) != hipSuccess)
    VO_HIP_TRY(ctx, hipStreamWaitEvent(ts, p->evRegroup[(f.k - 1) & 1], 0));
  if (hipEventQuery(p->evDet[f.a]) != hipSuccess) VO_HIP_TRY(ctx, hipStreamWaitEvent(ts, p->evDet[f.a], 0));
  vo_seq_ctl* ctl = p->d_ctl + q0;
  vo_klt_source src;
  src.n = &ctl->n2;                  // (= n once the previous step has closed; known as soon as its regroup has run)
  src.num_features = &ctl->num_features;
  src.frac = c.redetect_fraction;
  src.det_kp = p->kp(q0, f.a);
  src.n_det = c.n_keypoints;
  if (p->d_det_cnt) {                // (Shi-Tomasi re-detect: the slot's corner count, and the step's _num_features word)
    src.n_det_dev = p->d_det_cnt + (size_t)f.a * p->S + q0;
    src.num_features = &ctl->nf[f.k & 1];
  }
  src.ts = &ctl->ts[0];
  src.det_go = p->d_det_go + (size_t)f.a * p->S + q0;
  vo_klt_batch kb;
  kb.S = Sn;
  kb.pyr = p->pyr_stride();
  kb.xy = (size_t)p->cap * 2;
  kb.out = (size_t)p->cap;
  kb.ctl = sizeof(vo_seq_ctl);
  kb.det = p->det_stride();
  // The tracker's and the regroup's events are the kernels' own completion signals (vo_ctx::next_stop), not markers behind
  // them: a marker between the regroup and the hypothesis kernel cost the main chain 3.7 us, the tracker started 3.4 us
  // later behind it (step 85.8 -> 84.2 us).
  p->trk->next_stop = p->evKlt[f.k & 1];
  {
    const size_t q = (size_t)q0;
    const int rc = vo_klt_track_ndev(p->trk, p->img(q0, f.prev_idx), p->pyr(q0, f.a), p->img(q0, f.next_idx), p->pyr(q0, f.b),
                                     c.H, c.W, p->n_levels, A.kp, p->cap, nullptr, c.klt_win, c.klt_max_iter, c.klt_eps,
                                     c.klt_min_eig, p->d_next + q * p->cap * 2, p->d_status + q * p->cap,
                                     p->d_err + q * p->cap, &src, &kb, p->klt_fb,
                                     p->klt_fb > 0.0 ? p->d_fb + q * p->cap : nullptr);
    if (rc != VO_OK) return vo_set_error(ctx, rc, "tracker: %s", vo_last_error(p->trk));
  }
  if (p->trk->next_stop) {             // (the launch did not take the event)
    p->trk->next_stop = nullptr;
    VO_HIP_TRY(ctx, hipEventRecord(p->evKlt[f.k & 1], ts));
  }
  return VO_OK;
}

static int enqueue_pose_half(vo_pipeline* p, const vo_pipeline::flight_t& f, int q0, int Sn, unsigned seq);

// the main-stream chain of one step (the tracker's event must have been recorded);
// first_half_only: stop behind the regroup (recover_step continues on the host)
static int enqueue_chain(vo_pipeline* p, const vo_pipeline::flight_t& f, bool first_half_only, int debug_fault_every,
                         int q0, int Sn, unsigned seq) {
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  const size_t q = (size_t)q0;
  const vo_feat A = vo_feat_seq(p->F[f.fcur], q), B = vo_feat_seq(p->F[1 - f.fcur], q);
  vo_seq_ctl* ctl = p->d_ctl + q0;
  VO_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, p->evKlt[f.k & 1], 0));
  vo_append ap;
  ap.det_kp = p->kp(q0, f.a);
  ap.det_stride = p->det_stride();
  ap.n_det = c.n_keypoints;
  ap.frac = c.redetect_fraction;
  ap.pose_mode = c.redetect_start_pose;
  ap.debug_fault_every = debug_fault_every > 0 ? debug_fault_every : 0;
  ap.det_go = p->d_det_go + (size_t)f.a * p->S + q0;
  ap.nf_par = (int)(f.k & 1);
  if (p->d_det_cnt) ap.n_det_dev = p->d_det_cnt + (size_t)f.a * p->S + q0;
  ctx->next_stop = p->evRegroup[f.k & 1];
  VO_TRY(vo_state_regroup_klt(ctx, ctl, A, B, p->d_next + q * p->cap * 2, p->d_status + q * p->cap, p->d_err + q * p->cap,
                              (float)c.klt_err_threshold, ap, p->cap, Sn));
  if (first_half_only) return VO_OK;
  return enqueue_pose_half(p, f, q0, Sn, seq);
}

// hypotheses + pose kernel of one step (the second half of its main-stream chain; also the next batch of a step whose
// RANSAC loop continues)
static int enqueue_pose_half(vo_pipeline* p, const vo_pipeline::flight_t& f, int q0, int Sn, unsigned seq) {
  vo_ctx* ctx = p->ctx;
  const int debug_pose_fault = p->pose_fault_hook && p->cfg.debug_fault_every < 0 ? -p->cfg.debug_fault_every : 0;
  const vo_pipeline_config& c = p->cfg;
  const size_t q = (size_t)q0;
  const vo_feat B = vo_feat_seq(p->F[1 - f.fcur], q);
  vo_seq_ctl* ctl = p->d_ctl + q0;
  vo_hyp_batch hb;
  hb.S = Sn;
  hb.X = (size_t)p->cap * 3;
  hb.x = (size_t)p->cap * 2;
  hb.raws = p->ring_len;
  hb.ctl = sizeof(vo_seq_ctl);
  hb.cam = reinterpret_cast<const double*>(p->d_cams + q);     // (K is the entry's first member)
  hb.cam_stride = sizeof(vo_cam) / sizeof(double);
  VO_TRY(vo_p3p_hypotheses_ring_dev(ctx, B.land, B.kp64, &ctl->n_p3p, p->cap, c.K, p->d_raws + q * p->ring_len, &ctl->raw_pos,
                                    p->ring_len - 1, c.hyp, c.p3p_thr_sq, p->d_R + q * c.hyp * 9, p->d_t + q * c.hyp * 3,
                                    p->d_valid + q * c.hyp, p->d_counts + q * c.hyp, p->d_masks + q * c.hyp * p->words,
                                    (uint32_t*)&ctl->solve_flag, (uint64_t*)&ctl->ts[2], &hb));
  // The pose kernel stops behind the refinement (walk = 0).  The feature walk (reset_outliers, bearing-angle candidates: fp64
  // arithmetic of every feature) was the last third of the pose kernel, on its ONE compute unit: 10 us; as a launch of its
  // own, cap / 256 workgroups, the step period went 93.4 -> 87.8 us.  Walk and landmark stage now run in ONE launch
  // (state_walk_landmarks_kernel), one boundary less.  (Round 2 had the pose kernel's one workgroup go on with the landmark
  // stage -- frame_pose_kernel's tail -- which was neutral at ~450 candidates per frame on a stream that never lost a track;
  // the forward stream triangulates ~1100 per frame, three rounds of DLTs for one workgroup: 50 us against 18 for the
  // launch, its boundary included; step period 152 -> 121 us.)
  vo_pose_job job = make_pose_job(p, p->F[1 - f.fcur], 1, q0);
  job.walk = 0;
  job.res = p->m_res + (size_t)f.rslot * p->S + q;
  job.seq_word = p->m_seq + (size_t)f.rslot * p->S + q;
  job.seq = seq;
  job.debug_fault_every = debug_pose_fault;
  VO_TRY(vo_frame_pose(ctx, job, Sn));
  const uint64_t* bm = p->d_best_mask + (size_t)q0 * p->words;
  return vo_state_walk_landmarks(ctx, ctl, B, bm, p->words, p->d_cams + q0, c.bearing_threshold, c.refine_iters > 0 ? 1 : 0,
                                 p->cap, p->d_pend + q * p->cap, job.res, job.seq_word, seq, Sn);
}

// ---- SIFT tracker mode ----
extern "C" int vo_sift_dev(vo_ctx* ctx, const uint8_t* d_img, int H, int W, int cap, float* d_kp, float* d_desc,
                           uint8_t* d_desc_u8, int32_t* d_n);

// detect + describe of the step's new frame on the tracker's stream (it depends on the image only): slot f.b
// (The scale space of a frame is a chain of ~60 dependent launches, most of them on images too small to fill anything:
//  consecutive frames alternate between two contexts -- the tracker's and, idle in this mode, the detection's -- each with
//  its own streams and arena, so that two frames' chains are in flight side by side.  The launches are made by the worker
//  thread; err_buf: its private error text.)
static int enqueue_sift(vo_pipeline* p, const vo_pipeline::flight_t& f, char* err_buf = nullptr) {
  vo_ctx* sc = (f.k & 1) ? p->det : p->trk;
  const vo_pipeline_config& c = p->cfg;
  int rc = VO_OK;
  if (sc != p->trk && hipStreamWaitEvent(sc->stream, p->evImg[f.next_idx], 0) != hipSuccess) rc = VO_EHIP;   // (the upload)
  if (rc == VO_OK && p->n_pinned[f.next_idx] > 0 && hipStreamWaitEvent(sc->stream, p->evUp[f.next_idx], 0) != hipSuccess) rc = VO_EHIP;
  if (rc == VO_OK && p->sift_all)
    rc = vo_sift_all_found_dev(sc, p->img(0, f.next_idx), p->img_stride(), 1, c.H, c.W, p->frame_rows,
                               p->d_skp + (size_t)f.b * p->frame_rows * 6, (size_t)p->frame_rows, nullptr, p->frame_desc(f.b, 0),
                               (size_t)p->frame_rows, p->frame_n(f.b, 0), p->d_sover + 2 * f.b, p->d_sover + 2 * f.b + 1);
  else if (rc == VO_OK)
    rc = vo_sift_dev(sc, p->img(0, f.next_idx), c.H, c.W, p->frame_rows, p->d_skp + (size_t)f.b * p->frame_rows * 6, nullptr,
                     p->frame_desc(f.b, 0), p->frame_n(f.b, 0));
  if (rc == VO_OK && hipEventRecord(p->evPyr[f.b], sc->stream) != hipSuccess) rc = VO_EHIP;
  return rc != VO_OK ? launch_error(p, err_buf, rc, "sift", vo_last_error(sc)) : VO_OK;
}

// Harris tracker mode: the new frame's N keypoints (Harris response + greedy NMS, every frame) and their raw patches as
// bytes, on the detection stream; slot f.b.  All sequences: one detection (forced) and one patch launch (grid (N, S)).
static int enqueue_harris_front(vo_pipeline* p, const vo_pipeline::flight_t& f, char* err_buf = nullptr) {
  const vo_pipeline_config& c = p->cfg;
  int rc = enqueue_detection(p, f.next_idx, f.b, true, err_buf);
  if (rc != VO_OK) return rc;
  rc = vo_patch_descriptors_u8_batch_dev(p->det, p->img(0, f.next_idx), p->img_stride(), p->S, c.H, c.W, p->kp(0, f.b),
                                         p->det_stride(), c.n_keypoints, 9, p->frame_desc(f.b, 0),
                                         (size_t)p->frame_rows * p->desc_row, p->desc_row);
  if (rc == VO_OK && hipEventRecord(p->evPyr[f.b], p->det->stream) != hipSuccess) rc = VO_EHIP;
  return rc != VO_OK ? launch_error(p, err_buf, rc, "harris front", vo_last_error(p->det)) : VO_OK;
}

// FAST + BRIEF tracker mode: the new frame's FAST-9 corners (non-maximum suppression on, the n_keypoints strongest) and their
// BRIEF-256 descriptors, on the detection stream; slot f.b.  All sequences: one detection and one describe call (the
// sequence is a grid dimension of every kernel).  The corner count of every sequence goes straight into the slot's frame
// counts, which the describe kernel, the matcher and the regroup read where they lie: nothing comes back to the host.
static int enqueue_fast_front(vo_pipeline* p, const vo_pipeline::flight_t& f, char* err_buf = nullptr) {
  const vo_pipeline_config& c = p->cfg;
  vo_ctx* det = p->det;
  const int frame = f.next_idx;
  bool wait_ok = hipStreamWaitEvent(det->stream, p->evImg[frame], 0) == hipSuccess;   // the frame's upload (tracker's stream)
  if (wait_ok && p->n_pinned[frame] > 0) wait_ok = hipStreamWaitEvent(det->stream, p->evUp[frame], 0) == hipSuccess;   // (pinned)
  if (!wait_ok) return launch_error(p, err_buf, VO_EHIP, "fast front", "hipStreamWaitEvent failed");
  int rc = vo_fast_keypoints_batch_dev(det, p->img(0, frame), p->img_stride(), p->S, c.H, c.W, p->fast_threshold, 1, c.n_keypoints,
                                       p->kp(0, f.b), p->det_stride() / 2, nullptr, p->frame_n(f.b, 0), nullptr);
  if (rc == VO_OK)
    rc = vo_brief_describe_batch_dev(det, p->img(0, frame), p->img_stride(), p->S, c.H, c.W, p->kp(0, f.b), p->det_stride() / 2,
                                     p->frame_n(f.b, 0), c.n_keypoints, p->brief_oriented, p->frame_desc(f.b, 0),
                                     (size_t)p->frame_rows * p->desc_row, nullptr);
  if (rc == VO_OK && hipEventRecord(p->evPyr[f.b], det->stream) != hipSuccess) rc = VO_EHIP;
  return rc != VO_OK ? launch_error(p, err_buf, rc, "fast front", vo_last_error(det)) : VO_OK;
}

// main-stream chain of a step in a descriptor mode: 2-NN + ratio + uniqueness against the current Features' descriptors
// (sift.py:38-54), Matches regroup from the pair list (matches.py:26-212) with the descriptors following their
// keypoints, then hypotheses and pose as in the KLT mode.  (q0, Sn): sequences q0 .. q0 + Sn - 1 (all of them, or one
// when a step is redone).  debug_fault_every: the test hook of submitted steps (0 for what the host path redoes or
// enqueues again).
static int enqueue_chain_desc(vo_pipeline* p, const vo_pipeline::flight_t& f, bool first_half_only, int debug_fault_every,
                              int q0, int Sn, unsigned seq) {
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  hipStream_t st = ctx->stream;
  const bool harris = c.tracker_mode == 2, fast = c.tracker_mode == 3;
  const size_t row = (size_t)p->desc_row, q = (size_t)q0;
  const vo_feat A = vo_feat_seq(p->F[f.fcur], q), B = vo_feat_seq(p->F[1 - f.fcur], q);
  const uint8_t* descA = p->fdesc(f.fcur, q0);
  uint8_t* descB = p->fdesc(1 - f.fcur, q0);
  const uint8_t* new_desc = p->frame_desc(f.b, q0);
  const float* skp = p->d_skp + (size_t)f.b * p->frame_rows * 6;
  int32_t* n_new = p->frame_n(f.b, q0);
  int32_t* n_pairs = p->npairs(q0);
  int32_t* pairs = p->d_pairs + q * p->cap * 2;
  int32_t* src_row = p->d_srcrow + q * p->cap;
  vo_seq_ctl* ctl = p->d_ctl + q0;
  static_assert(sizeof(vo_seq_ctl) % 4 == 0, "control blocks are read as int arrays");
  VO_HIP_TRY(ctx, hipStreamWaitEvent(st, p->evPyr[f.b], 0));
  if (p->sift_all) {            // (a frame that does not fit: the step's first kernel raises the fault, nothing else runs)
    hipLaunchKernelGGL(sift_fit_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)p->d_sover + 2 * f.b, ctl);
    VO_TRY(vo_check_launch(ctx, "sift_fit_kernel"));
  }
  const double ratio = c.match_ratio > 0.0 ? c.match_ratio : (harris ? 0.85 : 0.8);        // harris.py:255 / sift.py:49
  if (fast)           // (Hamming distances, the ratio and the distance limit: vo/features/fast.py's defaults, 0.8 and 64)
    VO_TRY(vo_match_hamming_batch_dev(ctx, descA, (size_t)p->cap * row, &ctl->n, (int)(sizeof(vo_seq_ctl) / 4), p->cap, new_desc,
                                      (size_t)p->frame_rows * row, n_new, 1, p->frame_rows, Sn, p->desc_row, ratio,
                                      p->brief_max_distance, pairs, n_pairs));
  else
    VO_TRY(vo_match_u8_batch_dev(ctx, descA, (size_t)p->cap * row, &ctl->n, (int)(sizeof(vo_seq_ctl) / 4), p->cap, new_desc,
                                 (size_t)p->frame_rows * row, n_new, 1, p->frame_rows, Sn, ratio, pairs, n_pairs, p->desc_row));
  const double* new_kp = p->d_newkp;
  vo_pairs_batch bt;
  bt.pairs = (size_t)p->cap * 2;
  bt.src_row = (size_t)p->cap;
  bt.M = 1;
  bt.n2 = 1;
  bt.debug_fault_every = debug_fault_every > 0 ? debug_fault_every : 0;
  bt.par = (int)(f.k & 1);
  if (harris || fast) {
    new_kp = p->kp(q0, f.b);           // the detector's keypoints are float64 pairs already
    bt.new_kp = p->det_stride();
  } else {
    hipLaunchKernelGGL(sift_kp_f64_kernel, dim3(vo_cdiv(p->frame_rows, 256)), dim3(256), 0, st, skp, (const int*)n_new, p->frame_rows,
                       p->d_newkp);
    VO_TRY(vo_check_launch(ctx, "sift_kp_f64_kernel"));
  }
  VO_TRY(vo_state_regroup_pairs(ctx, ctl, A, B, pairs, p->cap, new_kp, p->frame_rows, p->cap, n_pairs, n_new, src_row, Sn, &bt));
  hipLaunchKernelGGL(desc_gather_kernel, dim3(vo_cdiv(p->cap * (p->desc_row / 4), 256), Sn), dim3(256), 0, st, new_desc,
                     (const int*)src_row, (const vo_seq_ctl*)ctl, p->cap, descB, p->desc_row / 4,
                     (size_t)p->frame_rows * row, (size_t)p->cap * row);
  VO_TRY(vo_check_launch(ctx, "desc_gather_kernel"));
  VO_HIP_TRY(ctx, hipEventRecord(p->evRegroup[f.k & 1], st));
  if (first_half_only) return VO_OK;
  return enqueue_pose_half(p, f, q0, Sn, seq);
}

// Flight f once more for sequences q0 .. q0 + Sn - 1 alone, without the test hook: tracking and regroup, and the pose half
// unless first_half_only.  (The frames' pyramids, detections or fronts are done and still in their slots.)
static int enqueue_redo(vo_pipeline* p, const vo_pipeline::flight_t& f, int q0, int Sn, bool first_half_only, unsigned seq) {
  if (p->cfg.tracker_mode != 0) return enqueue_chain_desc(p, f, first_half_only, 0, q0, Sn, seq);
  VO_TRY(enqueue_tracker(p, f, false, q0, Sn));
  return enqueue_chain(p, f, first_half_only, 0, q0, Sn, seq);
}

// ---- detection worker ----
void worker_main(vo_pipeline* p) {
  (void)hipSetDevice(p->ctx->device);
  unsigned seen = 0;
  long idle = 0;
  double idle_since = 0.0;
  for (;;) {
    if (p->job_posted.load(std::memory_order_acquire) == seen) {
      if (p->quit.load(std::memory_order_acquire)) return;
      // a step is ~120 us: stay hot between the steps of a running stream, then sleep until a job is posted
      if (idle == 0) idle_since = now_s();
      if ((++idle & 63) != 0 || now_s() - idle_since < p->spin_s) {
        __builtin_ia32_pause();
      } else {
        p->worker_asleep.store(1, std::memory_order_seq_cst);
        if (p->job_posted.load(std::memory_order_seq_cst) == seen && !p->quit.load(std::memory_order_seq_cst))
          futex_wait(&p->job_posted, seen);
        p->worker_asleep.store(0, std::memory_order_seq_cst);
        idle = 0;
      }
      continue;
    }
    idle = 0;
    const vo_pipeline::flight_t j = p->jobs[seen & 3];
    const int rc = p->cfg.tracker_mode == 1   ? enqueue_sift(p, j, p->worker_err)
                   : p->cfg.tracker_mode == 2 ? enqueue_harris_front(p, j, p->worker_err)
                   : p->cfg.tracker_mode == 3 ? enqueue_fast_front(p, j, p->worker_err)
                                              : enqueue_detection(p, j.next_idx, j.b, false, p->worker_err);
    if (rc != VO_OK) p->worker_rc = rc;
    ++seen;
    p->job_done.store(seen, std::memory_order_release);
  }
}

static int worker_check(vo_pipeline* p) {
  if (p->worker_rc != VO_OK) {
    const int rc = p->worker_rc;
    p->worker_rc = VO_OK;
    return vo_set_error(p->ctx, rc, "%s", p->worker_err);
  }
  return VO_OK;
}

int worker_idle(vo_pipeline* p) {
  if (p->threads_budget < 2) return VO_OK;
  const unsigned posted = p->job_posted.load(std::memory_order_relaxed);
  wait_until(50e-6, [&] { return p->job_done.load(std::memory_order_acquire) == posted; });
  return worker_check(p);
}

int prime(vo_pipeline* p, bool wait, int q0, int Sn) {
  vo_ctx* ctx = p->ctx;
  if (p->cfg.tracker_mode != 0) {      // descriptor modes: the frame's own descriptors travel with its Features
    p->primed = true;
    return VO_OK;
  }
  VO_TRY(worker_idle(p));
  sync_prof(p);
  p->prepared_idx = p->prepared_slot = -1;           // (a hand-over or a rewind: the slots start over)
  VO_TRY(enqueue_pyramid(p, p->prev_frame, p->slot, q0, Sn));
  VO_TRY(enqueue_detection(p, p->prev_frame, p->slot, true, nullptr, q0, Sn));
  if (wait) {        // (not needed for order: the tracker sits behind the pyramid on its stream and waits for evDet)
    VO_HIP_TRY(ctx, hipStreamSynchronize(p->trk->stream));
    VO_HIP_TRY(ctx, hipStreamSynchronize(p->det->stream));
  }
  p->primed = true;
  return VO_OK;
}

extern "C" {

// The pyramid of a frame that a coming step will track INTO, built now, behind the tracker of the step submitted last (on
// the tracker's stream): the next vo_pipeline_submit whose `next_idx` is this slot finds it ready.  Without the hint a
// step's pyramid is enqueued by its own submit -- which the host makes when it has collected the step before the previous
// one -- and the tracker, which needs nothing else that late, starts behind it: 31 us after the previous regroup instead
// of ~15.  (KLT tracker mode; a no-op in the others.  A hint that turns out wrong costs one wasted pyramid.)
int vo_pipeline_prepare(vo_pipeline* p, int idx) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, idx >= 0 && idx < p->cfg.n_frames, "pipeline_prepare: bad frame slot");
  if (p->cfg.tracker_mode != 0 || !p->primed || !p->have_state) return VO_OK;
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int s = (p->slot + 1) % 3;                    // the pyramid slot the next submit gives its `next` frame
  // (that slot held the `prev` pyramid of the step before the one submitted last: its tracker is earlier on this stream)
  VO_TRY(enqueue_pyramid(p, idx, s));
  p->prepared_idx = idx;
  p->prepared_slot = s;
  return VO_OK;
}

}  // extern "C"

// Descriptor modes: enqueue the main-stream chains of the flights that do not have theirs yet (oldest first)
// (in flight order, as far as their fronts have been made -- by this thread, or by the worker: front_job = the
//  worker's job count that says so; must_reach: flights up to this index are waited for)
static int flush_desc_chains(vo_pipeline* p, int must_reach = -1) {
  while (p->desc_chains_pending > 0) {
    const int k = p->n_flight - p->desc_chains_pending;
    const vo_pipeline::flight_t& f = p->flight[k];
    if (f.front_job != 0 && (int)(p->job_done.load(std::memory_order_acquire) - f.front_job) < 0) {
      if (k > must_reach) break;
      const unsigned want = f.front_job;
      wait_until(50e-6, [&] { return (int)(p->job_done.load(std::memory_order_acquire) - want) >= 0; });
    }
    VO_TRY(worker_check(p));
    for (int q = 0; q < p->S; ++q) VO_TRY(ensure_raws(p, q));
    // (the test hook in the Harris and FAST modes only: the SIFT mode's chain never had it)
    VO_TRY(enqueue_chain_desc(p, f, false, p->cfg.tracker_mode >= 2 ? p->cfg.debug_fault_every : 0, 0, p->S, f.seq));
    --p->desc_chains_pending;
  }
  return VO_OK;
}

// hands flight f to the worker (detection of its `next` frame, or its front in a descriptor mode); returns the job's count
static unsigned post_job(vo_pipeline* p, const vo_pipeline::flight_t& f) {
  const unsigned my = p->job_posted.load(std::memory_order_relaxed);
  p->jobs[my & 3] = f;
  p->job_posted.store(my + 1, std::memory_order_seq_cst);
  if (p->worker_asleep.load(std::memory_order_seq_cst)) futex_wake(&p->job_posted);
  return my + 1;
}

extern "C" {

int vo_pipeline_submit(vo_pipeline* p, int prev_idx, int next_idx) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  VO_REQUIRE(ctx, next_idx >= 0 && next_idx < c.n_frames, "pipeline_submit: bad frame index");
  VO_REQUIRE(ctx, p->have_state && p->seeded, "pipeline_submit: call vo_pipeline_seed and vo_pipeline_set_state first");
  VO_REQUIRE(ctx, prev_idx == p->prev_frame, "pipeline_submit: prev frame %d is not the frame last submitted (%d)",
             prev_idx, p->prev_frame);
  VO_REQUIRE(ctx, p->n_flight < 2, "pipeline_submit: two steps are already in flight, collect one first");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!p->primed) VO_TRY(prime(p));
  const double t_in = now_s();
  vo_pipeline::flight_t f;
  f.prev_idx = prev_idx;
  f.next_idx = next_idx;
  f.a = p->slot;
  f.b = (p->slot + 1) % 3;
  f.fcur = p->cur;
  f.seq = ++p->seq;
  f.rslot = (int)(p->steps_submitted & 3);
  f.k = p->steps_submitted;
  // The detection of `next` (half of the step's launches, needed only by the NEXT step) goes to the worker thread;
  // this thread enqueues the pyramid, the tracker and the main-stream chain.  The tracker waits for the event behind
  // the detection of `prev`: the worker must have recorded it (it was posted a whole step ago).
  if (c.tracker_mode != 0) {
    // The frame's ~75 SIFT launches go to the worker thread; this thread first gives the flight submitted before its
    // main-stream chain (its SIFT launches are made by now), so the two threads' launches overlap across frames.
    // Two threads make the launches, a frame each: even flights' go to the worker, odd flights' are made here (each
    // thread on its own SIFT context, so that two frames' chains also run side by side on the GPU).
    if (p->threads_budget >= 2 && ((f.k & 1) == 0 || c.tracker_mode >= 2)) {      // (harris, fast: one detection context, the worker's)
      const unsigned my = p->job_posted.load(std::memory_order_relaxed);
      if ((int)(p->job_done.load(std::memory_order_acquire) - my) >= 0) sync_prof(p);   // (idle worker: its context's flags are ours)
      f.front_job = post_job(p, f);
    } else {
      copy_prof((f.k & 1) ? p->det : p->trk, ctx);          // (budget 1: both contexts are this thread's)
      if (c.tracker_mode >= 2) {
        copy_prof(p->det, ctx);
        VO_TRY(c.tracker_mode == 2 ? enqueue_harris_front(p, f) : enqueue_fast_front(p, f));
      } else {
        VO_TRY(enqueue_sift(p, f));
      }
    }
    for (int q = 0; q < p->S; ++q) p->slot_seq[(size_t)f.rslot * p->S + q] = f.seq;
    p->flight[p->n_flight++] = f;
    ++p->desc_chains_pending;
    VO_TRY(flush_desc_chains(p));
  } else {
    double tq = now_s();
    // WHEN the detection's seven launches reach the GPU matters more than who makes them.  Arriving beside the hypothesis
    // kernel -- the worker used to get them at the start of submit -- they cost that kernel 20 us (hypotheses -> pose 43 us
    // against 23.5: a chain of launches that mostly return at once still keeps the command processor busy while the
    // 144 workgroups of the hypotheses are being dispatched), 121 against 108 us per step.  So they are handed to the worker
    // behind the step's chain -- unless the detector executes on every frame (detect_margin < 0): its kernels are then real
    // work the next step's tracker waits for, and an early start pays (16 sequences: 19.2k against 17.4k frames/s).
    const bool detect_early = p->detect_limit < 0.0;
    if (p->threads_budget >= 2) {
      const unsigned my = p->job_posted.load(std::memory_order_relaxed);
      wait_until(50e-6, [&] { return (int)(p->job_done.load(std::memory_order_acquire) - my) >= 0; });
      VO_TRY(worker_check(p));
      sync_prof(p);                      // (the worker is idle: the detection context's profiling flags are ours to write)
      if (detect_early) post_job(p, f);
    } else {
      sync_prof(p);
    }
    double tn = now_s();
    p->dbg_part[0] += tn - tq;
    tq = tn;
    const bool have_pyr = p->prepared_idx == next_idx && p->prepared_slot == f.b;
    p->prepared_idx = p->prepared_slot = -1;
    VO_TRY(enqueue_tracker(p, f, !have_pyr, 0, p->S));
    tn = now_s();
    p->dbg_part[1] += tn - tq;
    tq = tn;
    for (int q = 0; q < p->S; ++q) VO_TRY(ensure_raws(p, q));
    tn = now_s();
    p->dbg_part[2] += tn - tq;
    tq = tn;
    VO_TRY(enqueue_chain(p, f, false, c.debug_fault_every, 0, p->S, f.seq));
    for (int q = 0; q < p->S; ++q) p->slot_seq[(size_t)f.rslot * p->S + q] = f.seq;
    if (p->threads_budget < 2) VO_TRY(enqueue_detection(p, f.next_idx, f.b, false));   // (needed by the NEXT step only)
    else if (!detect_early) post_job(p, f);
    p->dbg_part[3] += now_s() - tq;
    p->flight[p->n_flight++] = f;
  }
  ++p->steps_submitted;
  p->slot = f.b;
  p->cur = 1 - f.fcur;
  p->prev_frame = next_idx;
  p->dbg_submit += now_s() - t_in;
  ++p->dbg_steps;
  return VO_OK;
}

}  // extern "C"

// Waits for sequence q's record of step `seq` in slot rslot and copies it out.  The kernel writes the record,
// fences at system scope, then the sequence word; the record also carries the number at both ends and the generator
// position can only grow, so a copy taken while some of the record's lines were still on their way (seen twice in
// ~40k steps: the sequence word visible, a field behind it not yet) is recognised and taken again.
// state_device.h: seq_head = the number XOR every other dword of the record, seq_tail = the number + their record_mix sum
static void record_words(const vo_step_result* rec, unsigned seq, unsigned* head, unsigned* tail) {
  const unsigned* dw = reinterpret_cast<const unsigned*>(rec);
  unsigned x = 0u, y = 0u;
  for (size_t k = 0; k + 2 < sizeof(*rec) / 4; ++k) {
    x ^= dw[k];
    y += vo_state_dev::record_mix(dw[k], (int)k);
  }
  *head = seq ^ x;
  *tail = seq + y;
}

static bool record_fits(vo_step_result* out, unsigned seq) {
  unsigned head, tail;
  record_words(out, seq, &head, &tail);
  if (out->seq_tail != tail || out->seq_head != head) return false;
  out->seq_head = seq;           // (what the caller sees: both equal the step's number)
  out->seq_tail = seq;
  return true;
}

// The record's check as the C ABI exposes it (tests; a host that reads the mapped records itself): _seal writes the two
// closing words the way the device does, _check says whether a copy is one whole record of step `seq`.
extern "C" void vo_record_seal(vo_step_result* rec, unsigned seq) {
  if (rec) record_words(rec, seq, &rec->seq_head, &rec->seq_tail);
}

extern "C" int vo_record_check(const vo_step_result* rec, unsigned seq) {
  if (!rec) return 0;
  vo_step_result copy = *rec;
  return record_fits(&copy, seq) ? 1 : 0;
}

static int wait_record(vo_pipeline* p, int rslot, int q, unsigned seq, uint64_t floor, vo_step_result* out) {
  volatile unsigned* w = p->seq_h(rslot, q);
  const double t0 = now_s();
  long it = 0;
  bool spinning = p->spin_s > 0.0;
  for (;;) {
    if (*w == seq) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      memcpy(out, (const void*)p->res_h(rslot, q), sizeof(*out));
      if (record_fits(out, seq) && out->raw_pos >= floor) return VO_OK;
    }
    // poll for spin_s, then look every 20 us (the GPU cannot wake a host thread; a blocking stream wait would also wait
    // for the look-ahead step queued behind this one)
    if (spinning) {
      __builtin_ia32_pause();
      if ((++it & 31) == 0 && now_s() - t0 > p->spin_s) spinning = false;
      continue;
    }
    nap(20000);
    if ((++it & 0xff) == 0 && now_s() - t0 > 5.0) {
      VO_HIP_TRY(p->ctx, hipStreamSynchronize(p->ctx->stream));
      memcpy(out, (const void*)p->res_h(rslot, q), sizeof(*out));
      if (*w == seq && record_fits(out, seq)) return VO_OK;
      return vo_set_error(p->ctx, VO_EHIP, "pipeline: the GPU never published the record of step %u (sequence %d)", seq, q);
    }
  }
}

// The text of a re-detect that does not fit: n features and the detector's keypoints of the step's `prev` frame -- n_keypoints
// of them, or (Shi-Tomasi) the count the detection left in the slot; a frame whose Shi-Tomasi lists overflowed says so.
static int capacity_error(vo_pipeline* p, const vo_pipeline::flight_t& f, int q, int n) {
  vo_ctx* ctx = p->ctx;
  int32_t n_det = p->cfg.n_keypoints;
  if (p->d_det_cnt) {
    VO_HIP_TRY(ctx, mcpy(ctx->stream, &n_det, p->d_det_cnt + (size_t)f.a * p->S + q, 4, hipMemcpyDeviceToHost));
    if (n_det < 0)
      return vo_set_error(ctx, VO_ECAPACITY, "pipeline: the Shi-Tomasi candidate lists of frame %d overflowed (sequence %d)",
                          f.prev_idx, q);
  }
  return vo_set_error(ctx, VO_ECAPACITY, "pipeline: %d features + %d new keypoints exceed the capacity %d", n, n_det, p->cap);
}

// Sequence q's step of flight f raised a fault: nothing persistent of that sequence was touched, so the step is run
// again from its first main-stream kernel (for that sequence alone) with the sequential sampler and the reference's
// loop on the host (ransac.py:90-121), then handed back to the device for the refinement and the bookkeeping.
static int recover_step(vo_pipeline* p, const vo_pipeline::flight_t& f, int q, vo_step_result* out) {
  vo_ctx* ctx = p->ctx;
  const vo_pipeline_config& c = p->cfg;
  hipStream_t st = ctx->stream;
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  VO_HIP_TRY(ctx, hipStreamSynchronize(p->trk->stream));
  vo_seq_ctl* ctl = p->d_ctl + q;
  vo_seq_ctl h;
  VO_HIP_TRY(ctx, mcpy(st, &h, ctl, sizeof(h), hipMemcpyDeviceToHost));
  const int fault_reason = h.fault;
  if ((h.fault & VO_FAULT_CAPACITY) && p->sift_all) {     // (sift_fit_kernel: the frame's keypoints do not fit)
    int32_t v[2] = {0, 0};
    VO_HIP_TRY(ctx, mcpy(st, v, p->d_sover + 2 * f.b, sizeof(v), hipMemcpyDeviceToHost));
    if (v[0] == 1)
      return vo_set_error(ctx, VO_ECAPACITY, "pipeline: the SIFT candidate / keypoint lists of frame %d overflowed", f.next_idx);
    if (v[0] == 2)
      return vo_set_error(ctx, VO_ECAPACITY, "pipeline: frame %d has %d SIFT keypoints, more than the feature capacity %d",
                          f.next_idx, v[1], p->cap);
  }
  if (h.fault & VO_FAULT_CAPACITY) return capacity_error(p, f, q, h.n);
  const int zero = 0;
  VO_HIP_TRY(ctx, mcpy(st, &ctl->fault, &zero, 4, hipMemcpyHostToDevice));
  // The tracker reads its feature count from n2, which the step's own regroup has replaced by the NEW frame's count
  // when the fault came from the pose kernel (a possibly rejected draw, an unfinished loop): the tracker below would
  // redo only the first n2 features, and the rest of d_next would be whatever the next step's tracker left there --
  // the step's own values unless that one appended a detection (found by tests/pipeline_fuzz.py, now and then).
  if (c.tracker_mode == 0) VO_HIP_TRY(ctx, mcpy(st, &ctl->n2, &h.n, 4, hipMemcpyHostToDevice));
  // tracker and regroup of this sequence alone, without the forced fault.  A regroup that needs the detector's keypoints
  // of `prev` and finds that the detection was skipped (the tracks fell through the margin within one frame -- the
  // fault this step came with, or one that another fault had hidden) says so: the keypoints are made now, once more.
  for (int attempt = 0;; ++attempt) {
    if (h.fault & VO_FAULT_NO_DETECTION) {
      VO_TRY(enqueue_detection(p, f.prev_idx, f.a, true, nullptr, q, 1));
      VO_HIP_TRY(ctx, hipStreamSynchronize(p->det->stream));
    }
    VO_TRY(enqueue_redo(p, f, q, 1, true, 0u));
    VO_HIP_TRY(ctx, hipStreamSynchronize(st));
    VO_HIP_TRY(ctx, mcpy(st, &h, ctl, sizeof(h), hipMemcpyDeviceToHost));
    if (!(h.fault & VO_FAULT_NO_DETECTION) || attempt > 0) break;
    VO_HIP_TRY(ctx, mcpy(st, &ctl->fault, &zero, 4, hipMemcpyHostToDevice));
  }
  if (h.fault & VO_FAULT_CAPACITY) return capacity_error(p, f, q, h.n);
  if (h.fault & VO_FAULT_NO_DETECTION) return vo_set_error(ctx, VO_EHIP, "pipeline: the detector's keypoints are missing");
  const int n = h.n_tri;
  if (n < 4) return vo_set_error(ctx, VO_ETRACKING, "pipeline: only %d triangulated tracks survive, no pose", n);
  // (fewer than 8 landmarks is no fault here: the regroup leaves it in ctl->few, and the sequential sampler below draws from
  //  any population of 4 or more)
  const vo_feat B = vo_feat_seq(p->F[1 - f.fcur], (size_t)q);
  double* dR = p->d_R + (size_t)q * c.hyp * 9;
  double* dt = p->d_t + (size_t)q * c.hyp * 3;
  uint8_t* dvalid = p->d_valid + (size_t)q * c.hyp;
  int32_t* dcounts = p->d_counts + (size_t)q * c.hyp;
  uint64_t* dmasks = p->d_masks + (size_t)q * c.hyp * p->words;
  uint64_t* dbest = p->d_best_mask + (size_t)q * p->words;
  vo_ransac_state rs;
  // (a step that had walked some batches on the device before it met this fault is redone from its start: the fields
  //  the estimator object held then, and the host's generator, which follows closed steps only)
  rs.outlier_ratio = h.cont > 0 ? h.outlier_ratio0 : h.outlier_ratio;
  rs.confidence = c.ransac_confidence;
  rs.max_iterations = c.ransac_max_iterations;
  rs.n_iterations = h.cont > 0 ? h.n_iterations0 : h.n_iterations;
  rs.s = 4;
  rs.adaptive = 1;
  vo_pcg64 g = p->rng[q];
  std::vector<int32_t> samples((size_t)4 * c.hyp), counts(c.hyp);
  std::vector<uint8_t> valid(c.hyp);
  int64_t n_done = 0;
  int32_t best_count = -1, best_idx = -1;
  int total_consumed = 0, finished = 0, batches = 0, hyp_valid = 0;
  double best_pose[12];
  while (!finished) {
    VO_TRY(vo_rng_choice(&g, n, 4, c.hyp, samples.data()));
    VO_HIP_TRY(ctx, hipMemcpyAsync(p->d_samples, samples.data(), samples.size() * 4, hipMemcpyHostToDevice, st));
    VO_TRY(vo_p3p_hypotheses_dev(ctx, B.land, B.kp64, n, p->cams[q].K, p->d_samples, c.hyp, c.p3p_thr_sq, dR, dt, dvalid, dcounts,
                                 dmasks));
    VO_HIP_TRY(ctx, hipMemcpyAsync(valid.data(), dvalid, (size_t)c.hyp, hipMemcpyDeviceToHost, st));
    VO_HIP_TRY(ctx, hipMemcpyAsync(counts.data(), dcounts, (size_t)c.hyp * 4, hipMemcpyDeviceToHost, st));
    VO_HIP_TRY(ctx, hipStreamSynchronize(st));
    int consumed = 0;
    const int32_t before = best_idx;
    VO_TRY(vo_ransac_replay(&rs, valid.data(), counts.data(), c.hyp, n, &n_done, &best_count, &best_idx, batches * c.hyp,
                            &consumed, &finished));
    for (int i = 0; i < consumed; ++i) hyp_valid += valid[i] ? 1 : 0;
    total_consumed += consumed;
    if (best_idx != before) {
      // the winner so far lives in this batch: take its pose and mask row before the buffers are reused
      // (vo_p3p_hypotheses_dev packs mask rows with ceil(n / 64) words)
      const int local = best_idx - batches * c.hyp;
      VO_HIP_TRY(ctx, mcpy(st, best_pose, dR + (size_t)local * 9, 72, hipMemcpyDeviceToHost));
      VO_HIP_TRY(ctx, mcpy(st, best_pose + 9, dt + (size_t)local * 3, 24, hipMemcpyDeviceToHost));
      VO_HIP_TRY(ctx, mcpy(st, dbest, dmasks + (size_t)local * vo_cdiv(n, 64), (size_t)vo_cdiv(n, 64) * 8,
                           hipMemcpyDeviceToDevice));
    }
    if (++batches > 64 && !finished)
      return vo_set_error(ctx, VO_ETRACKING, "pipeline: the RANSAC rule is not done after %d samples", batches * c.hyp);
  }
  if (best_idx < 0) return vo_set_error(ctx, VO_ETRACKING, "pipeline: no hypothesis had a solution");
  // the generator moves by exactly the samples the reference loop drew; the look-ahead restarts behind it
  {
    std::vector<int32_t> tmp((size_t)4 * (total_consumed > 0 ? total_consumed : 1));
    VO_TRY(vo_rng_choice(&p->rng[q], n, 4, total_consumed, tmp.data()));
  }
  p->raw_gen[q] = p->rng[q];
  p->pos_known[q] = p->gen_upto[q];
  p->pos_dev[q] = p->gen_upto[q];
  h.fault = 0;
  h.few = 0;
  h.cont = 0;
  h.n_p3p = n;
  h.n_iterations = rs.n_iterations;
  h.outlier_ratio = rs.outlier_ratio;
  h.raw_pos = p->gen_upto[q];
  h.best_idx = best_idx;
  h.best_count = best_count;
  h.consumed = total_consumed;
  h.hyp_valid = hyp_valid;
  h.n_done = n_done;
  h.n_cand = h.n_dropped = h.n_land = h.done = 0;
  memcpy(h.best_pose, best_pose, 96);
  VO_HIP_TRY(ctx, mcpy(st, ctl, &h, sizeof(h), hipMemcpyHostToDevice));
  const unsigned seq = ++p->seq;           // the fault record carried the step's number: the new record gets its own
  p->slot_seq[(size_t)f.rslot * p->S + q] = seq;
  {
    vo_pose_job job = make_pose_job(p, p->F[1 - f.fcur], 0, q);
    job.tail = 1;
    job.res = p->m_res + (size_t)f.rslot * p->S + q;
    job.seq_word = p->m_seq + (size_t)f.rslot * p->S + q;
    job.seq = seq;
    VO_TRY(vo_frame_pose(ctx, job, 1));
  }
  VO_TRY(wait_record(p, f.rslot, q, seq, 0, out));
  out->recovered = 1;
  out->reserved = fault_reason;          // (why the step left the device-only path: VO_FAULT_* bits)
  ++p->n_recovered;
  return VO_OK;
}

// Sequence q's step of flight f is open: its RANSAC loop has walked the launch's `hyp` samples and wants more
// (VO_FAULT_CONTINUE; the loop's state is in the control block, the generator position moved on).  The next batch --
// hypotheses + pose kernel for that sequence alone -- is launched until the record is a closed step's or a real fault's.
// Nothing is recomputed and nothing comes back but the records: the loop stays on the device (ransac.py:90-121 with
// max_iterations beyond one launch, as src/main.py:194-201 configures it).
static int continue_step(vo_pipeline* p, const vo_pipeline::flight_t& f, int q, vo_step_result* out) {
  vo_ctx* ctx = p->ctx;
  for (long round = 0; out->fault == VO_FAULT_CONTINUE; ++round) {
    if (round >= (1 << 16))
      return vo_set_error(ctx, VO_ETRACKING, "pipeline: the RANSAC rule is not done after %ld batches of %d samples", round, p->cfg.hyp);
    p->pos_dev[q] = out->raw_pos;
    VO_TRY(ensure_raws(p, q));
    const unsigned seq = ++p->seq;
    p->slot_seq[(size_t)f.rslot * p->S + q] = seq;
    hipLaunchKernelGGL(ctl_resume_kernel, dim3(1), dim3(1), 0, ctx->stream, p->d_ctl + q);
    VO_TRY(vo_check_launch(ctx, "ctl_resume_kernel"));
    VO_TRY(enqueue_pose_half(p, f, q, 1, seq));
    VO_TRY(wait_record(p, f.rslot, q, seq, out->raw_pos, out));
    ++p->n_continued;
  }
  return VO_OK;
}

extern "C" {

int vo_pipeline_collect_all(vo_pipeline* p, vo_step_result* outs) {
  if (!p || !outs) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->n_flight > 0, "pipeline_collect: nothing submitted");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const vo_pipeline::flight_t f = p->flight[0];
  if (p->cfg.tracker_mode != 0) VO_TRY(flush_desc_chains(p, 0));
  {
    const double t_in = now_s();
    for (int q = 0; q < p->S; ++q)
      VO_TRY(wait_record(p, f.rslot, q, p->slot_seq[(size_t)f.rslot * p->S + q], p->idle[q] ? 0 : p->pos_known[q], &outs[q]));
    p->dbg_wait += now_s() - t_in;
  }
  for (int q = 0; q < p->S; ++q) {
    vo_step_result* out = &outs[q];
    if (p->idle[q]) {                    // an idle lane's record (vo_hip.h): nothing was done, nothing is redone
      const unsigned sh = out->seq_head, st = out->seq_tail;
      memset(out, 0, sizeof(*out));
      out->n_features_in = -1;
      out->best_index = -1;
      out->refine_iterations = -1;
      out->fault = VO_FAULT_IDLE;
      out->raw_pos = p->pos_known[q];
      out->seq_head = sh;
      out->seq_tail = st;
      continue;
    }
    const bool was_open = out->fault == VO_FAULT_CONTINUE;
    int rc = VO_OK;
    // Descriptor modes: every flight has its chain before anything is enqueued for this sequence again -- a chain enqueued
    // only behind the next batch of hypotheses (or the host path) would find the step closed and run the next step once
    // more for this sequence, from a generator position already moved on.
    if ((out->fault || was_open) && p->cfg.tracker_mode != 0) rc = flush_desc_chains(p, p->n_flight - 1);
    if (rc == VO_OK && was_open) rc = continue_step(p, f, q, out);
    if (rc != VO_OK) {
      p->n_flight = 0;
      return rc;
    }
    if (out->fault || was_open) {
      rc = out->fault ? recover_step(p, f, q, out) : VO_OK;
      // (a structure loop's write-back that this lane's fault word kept out: once more, on the redone step's features)
      if (rc == VO_OK && p->sloop) rc = vo_structure_loop_requeue(p, q, f.k);
      // steps submitted behind it saw the fault and did nothing for this sequence: their main-stream chains are
      // enqueued again for it alone (pyramids and detections are done and still in place)
      for (int k = 1; rc == VO_OK && k < p->n_flight; ++k) {
        const unsigned seq = ++p->seq;
        p->slot_seq[(size_t)p->flight[k].rslot * p->S + q] = seq;
        rc = ensure_raws(p, q);
        if (rc == VO_OK) rc = enqueue_redo(p, p->flight[k], q, 1, false, seq);
      }
      if (rc != VO_OK) {
        // the pipeline cannot go on from here: drop what was in flight so the caller can reset the state
        p->n_flight = 0;
        return rc;
      }
    }
    if (!out->recovered) {
      // the estimator's generator follows the device: 7 outputs per consumed sample
      const uint64_t delta = out->raw_pos - p->pos_known[q];
      if (delta > 0) {
        std::vector<uint32_t> tmp((size_t)delta);
        vo_rng_raw32(&p->rng[q], (int)delta, tmp.data());
      }
      p->pos_known[q] = out->raw_pos;
      p->pos_dev[q] = out->raw_pos;
    }
  }
  p->flight[0] = p->flight[1];
  --p->n_flight;
  p->last_fbuf = 1 - f.fcur;
  p->last_k = f.k;
  return VO_OK;
}

int vo_pipeline_collect(vo_pipeline* p, vo_step_result* out) {
  if (!p || !out) return VO_EINVAL;
  if (p->S == 1) return vo_pipeline_collect_all(p, out);
  std::vector<vo_step_result> all((size_t)p->S);
  VO_TRY(vo_pipeline_collect_all(p, all.data()));
  *out = all[0];
  return VO_OK;
}

int vo_pipeline_step(vo_pipeline* p, int prev_idx, int next_idx, vo_step_result* out) {
  if (!p || !out) return VO_EINVAL;
  VO_REQUIRE(p->ctx, p->n_flight == 0, "pipeline_step: %d submitted step(s) not collected", p->n_flight);
  VO_TRY(vo_pipeline_submit(p, prev_idx, next_idx));
  return vo_pipeline_collect(p, out);
}

}  // extern "C"
