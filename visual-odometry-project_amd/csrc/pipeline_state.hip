// Frame pipeline: the state it carries -- seed, hand-over, descriptors, checkpoint / rewind, lanes, read-back,
// bookkeeping and export.
#include <algorithm>

#include "pipeline.h"
#include "track_record_device.h"

#pragma clang fp contract(off)

namespace {

struct pose17 {
  double v[17];
};

// record = [T_cw 4x4 row-major | n | landmarks cap x 3]: what one rank contributes to the shared map
__global__ __launch_bounds__(256) void export_state_kernel(pose17 head, const double* __restrict__ land, int n, int cap,
                                                           double* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 17) rec[i] = head.v[i];
  const int m = min(n, cap) * 3;
  if (i < m) rec[17 + i] = land[i];
}

// The observation record of one step (track_record_device.h).  slot: where the collected step's regroup left next_id / the step counter (vo_seq_ctl.next_id).
__global__ __launch_bounds__(256) void export_tracks_kernel(vo_feat F, const vo_seq_ctl* __restrict__ ctl, int slot, int n,
                                                            int cap, int seq, unsigned long long* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) vo_track::write_header(rec, n, ctl->id_step[slot], ctl->next_id[slot], seq);
  if (i >= min(n, cap)) return;
  vo_track::write_row(rec, F, i);
}

// vo_pipeline_update_landmarks_seq: feature i of the sequence takes X[3 k ..] when its id is ids[k] (the first such k) and its
// state is 2; nothing else is written
__global__ __launch_bounds__(256) void update_landmarks_kernel(vo_feat F, const vo_seq_ctl* __restrict__ ctl, int cap, int n_list,
                                                               const int32_t* __restrict__ ids, const double* __restrict__ X) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(ctl->n, cap) || F.state[i] != 2) return;
  const int id = F.ids[i].x;
  for (int k = 0; k < n_list; ++k) {
    if (ids[k] != id) continue;
    F.land[3 * i] = X[3 * k];
    F.land[3 * i + 1] = X[3 * k + 1];
    F.land[3 * i + 2] = X[3 * k + 2];
    return;
  }
}

// vo_pipeline_rewind: the control block as it was at the checkpoint, except what lives on the reference's estimator
// object (RANSAC.n_iterations / outlier_ratio, ransac.py:47-56) and the generator position, which go on
__global__ __launch_bounds__(64) void ctl_rewind_kernel(vo_seq_ctl* __restrict__ ctl, const vo_seq_ctl* __restrict__ saved, int S,
                                                        int id_par) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= S) return;
  vo_seq_ctl c = saved[q];
  c.n_iterations = ctl[q].n_iterations;
  c.outlier_ratio = ctl[q].outlier_ratio;
  c.raw_pos = ctl[q].raw_pos;
  c.step = ctl[q].step;
  c.nf[0] = c.nf[1] = c.num_features;     // (whichever parity the next step has: vo_seq_ctl.nf)
  c.next_id[0] = c.next_id[1] = saved[q].next_id[id_par];   // (the slot the step after the checkpoint was to read)
  c.id_step[0] = c.id_step[1] = c.step;
  ctl[q] = c;
}

void expand_pose(const double* p12, double* p16) {
  memcpy(p16, p12, 96);
  if (std::isnan(p12[0])) {
    for (int k = 12; k < 16; ++k) p16[k] = NAN;     // the reference's NaN poses are NaN in all 16 entries
  } else {
    p16[12] = p16[13] = p16[14] = 0.0;
    p16[15] = 1.0;
  }
}

}  // namespace

extern "C" {

int vo_pipeline_seed(vo_pipeline* p, const vo_pcg64* rng) {
  if (!p || !rng) return VO_EINVAL;
  VO_REQUIRE(p->ctx, p->n_flight == 0, "pipeline_seed: %d submitted step(s) not collected", p->n_flight);
  p->seed_rng = *rng;
  for (int q = 0; q < p->S; ++q) {     // every sequence has its own estimator object: each starts from this state
    p->rng[q] = *rng;
    p->raw_gen[q] = *rng;
    // the device continues at the end of what has been generated so far; that look-ahead is dropped
    p->pos_known[q] = p->gen_upto[q];
    VO_HIP_TRY(p->ctx, mcpy(p->ctx->stream, &p->d_ctl[q].raw_pos, &p->gen_upto[q], 8, hipMemcpyHostToDevice));
  }
  p->seeded = true;
  return VO_OK;
}

int vo_pipeline_get_rng_seq(vo_pipeline* p, int seq, vo_pcg64* rng) {
  if (!p || !rng || seq < 0 || seq >= p->S) return VO_EINVAL;
  *rng = p->rng[seq];
  return VO_OK;
}

int vo_pipeline_get_rng(vo_pipeline* p, vo_pcg64* rng) { return vo_pipeline_get_rng_seq(p, 0, rng); }

// the arguments vo_pipeline_set_state_seq and vo_pipeline_restart_seq share (features: every per-feature array given,
// poses: the four poses given); nothing may be in flight
static int check_state_args(vo_pipeline* p, const char* who, int seq, int n, bool features, bool poses) {
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "%s: bad sequence index", who);
  VO_REQUIRE(ctx, n >= 0 && n <= p->cap, "%s: %d features exceed the capacity %d", who, n, p->cap);
  VO_REQUIRE(ctx, (n == 0 || features) && poses, "%s: null pointer", who);
  VO_REQUIRE(ctx, p->n_flight == 0, "%s: %d submitted step(s) not collected", who, p->n_flight);
  return VO_OK;
}

// Features / State of sequence seq into the current Features buffer and its control block (nothing in flight).
// keep_ransac: the RANSAC object's fields stay (a second hand-over to the same estimator), else RANSAC.__init__'s;
// raw_pos: the generator position the device continues at (NULL: where it is).  The control block starts over (fault,
// step, the VO_FAULT_IDLE bit included).
static int upload_state(vo_pipeline* p, int seq, int n, const double* kp, const uint8_t* state, const double* landmarks,
                        const double* tracks, const double* poses, const double* T_wc, const double* T_cw,
                        const double* T_wc_prev, const double* T_cw_prev, int num_features, bool keep_ransac,
                        const uint64_t* raw_pos_set) {
  vo_ctx* ctx = p->ctx;
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  const vo_feat F = vo_feat_seq(p->F[p->cur], (size_t)seq);
  std::vector<double> pose12((size_t)n * 12);
  std::vector<float> kp32((size_t)n * 2);
  std::vector<uint8_t> zeros((size_t)n, 0);
  for (int i = 0; i < 2 * n; ++i) kp32[i] = (float)kp[i];
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 12; ++k) pose12[(size_t)k * n + i] = poses[(size_t)16 * i + k];   // component-major on the device
  if (n > 0) {
    VO_HIP_TRY(ctx, mcpy(st, F.kp, kp32.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    VO_HIP_TRY(ctx, mcpy(st, F.kp64, kp, (size_t)n * 16, hipMemcpyHostToDevice));
    VO_HIP_TRY(ctx, mcpy(st, F.state, state, (size_t)n, hipMemcpyHostToDevice));
    VO_HIP_TRY(ctx, mcpy(st, F.cand, zeros.data(), (size_t)n, hipMemcpyHostToDevice));
    VO_HIP_TRY(ctx, mcpy(st, F.land, landmarks, (size_t)n * 24, hipMemcpyHostToDevice));
    VO_HIP_TRY(ctx, mcpy(st, F.track, tracks, (size_t)n * 16, hipMemcpyHostToDevice));
    for (int k = 0; k < 12; ++k)
      VO_HIP_TRY(ctx, mcpy(st, F.pose + (size_t)k * F.pitch, &pose12[(size_t)k * n], (size_t)n * 8, hipMemcpyHostToDevice));
    if (F.ids) {
      std::vector<int32_t> ids((size_t)n * 2, 0);
      for (int i = 0; i < n; ++i) ids[(size_t)2 * i] = i;
      VO_HIP_TRY(ctx, mcpy(st, F.ids, ids.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
  }
  vo_seq_ctl h;
  VO_HIP_TRY(ctx, mcpy(st, &h, p->d_ctl + seq, sizeof(h), hipMemcpyDeviceToHost));
  const uint64_t raw_pos = raw_pos_set ? *raw_pos_set : h.raw_pos;
  const int64_t n_it = h.n_iterations;
  const double orat = h.outlier_ratio;
  memset(&h, 0, sizeof(h));
  h.n = n;
  h.n2 = n;
  h.num_features = num_features;
  h.nf[0] = h.nf[1] = num_features;
  h.next_id[0] = h.next_id[1] = n;       // (track ids: 0 .. n-1 in feature order, born 0)
  h.raw_pos = raw_pos;
  if (keep_ransac) {
    h.n_iterations = n_it;
    h.outlier_ratio = orat;
  } else {
    // RANSAC.__init__ (ransac.py:47-56)
    h.outlier_ratio = p->cfg.ransac_outlier_ratio;
    const int64_t k0 = vo_ransac_num_iterations(p->cfg.ransac_confidence, p->cfg.ransac_outlier_ratio, 4);
    h.n_iterations = (p->cfg.ransac_max_iterations >= 0 && p->cfg.ransac_max_iterations < k0) ? p->cfg.ransac_max_iterations : k0;
  }
  memcpy(h.T_wc, T_wc, 96);
  memcpy(h.T_cw, T_cw, 96);
  memcpy(h.T_wc_prev, T_wc_prev, 96);
  memcpy(h.T_cw_prev, T_cw_prev, 96);
  VO_HIP_TRY(ctx, mcpy(st, p->d_ctl + seq, &h, sizeof(h), hipMemcpyHostToDevice));
  p->idle[seq] = 0;
  return VO_OK;
}

int vo_pipeline_set_state_seq(vo_pipeline* p, int seq, int idx, int n, const double* kp, const uint8_t* state,
                              const double* landmarks, const double* tracks, const double* poses, const double* T_wc,
                              const double* T_cw, const double* T_wc_prev, const double* T_cw_prev, int num_features) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, idx >= 0 && idx < p->cfg.n_frames, "pipeline_set_state: bad frame index");
  VO_TRY(check_state_args(p, "pipeline_set_state", seq, n, kp && state && landmarks && tracks && poses,
                          T_wc && T_cw && T_wc_prev && T_cw_prev));
  // the sequences step together through one frame slot: the states of one hand-over all belong to the same frame
  VO_REQUIRE(ctx, !(p->S > 1 && p->have_state && !p->primed && idx != p->prev_frame),
             "pipeline_set_state: sequence %d is handed over for frame %d, the others of this hand-over for frame %d", seq, idx,
             p->prev_frame);
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  VO_TRY(upload_state(p, seq, n, kp, state, landmarks, tracks, poses, T_wc, T_cw, T_wc_prev, T_cw_prev, num_features,
                      p->seq_state[seq] != 0, nullptr));
  // the pyramid and the detector's output of the frame the states belong to are made by the first submit
  // (for all sequences at once: they share the frame slot, the last call's idx counts)
  p->seq_state[seq] = 1;
  p->slot = 0;
  p->prev_frame = idx;
  p->have_state = true;
  p->primed = false;
  return VO_OK;
}

int vo_pipeline_set_state(vo_pipeline* p, int idx, int n, const double* kp, const uint8_t* state,
                          const double* landmarks, const double* tracks, const double* poses, const double* T_wc,
                          const double* T_cw, const double* T_wc_prev, const double* T_cw_prev, int num_features) {
  return vo_pipeline_set_state_seq(p, 0, idx, n, kp, state, landmarks, tracks, poses, T_wc, T_cw, T_wc_prev, T_cw_prev,
                                   num_features);
}

int vo_pipeline_set_descriptors(vo_pipeline* p, const float* desc, int n) {
  return vo_pipeline_set_descriptors_seq(p, 0, desc, n);
}

int vo_pipeline_set_descriptors_seq(vo_pipeline* p, int seq, const float* desc, int n) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->cfg.tracker_mode != 0, "pipeline_set_descriptors: the pipeline is not in a descriptor tracker mode");
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_set_descriptors: bad sequence index");
  VO_REQUIRE(ctx, p->have_state && p->n_flight == 0, "pipeline_set_descriptors: hand the state over first (nothing in flight)");
  VO_REQUIRE(ctx, n >= 0 && n <= p->cap && (n == 0 || desc), "pipeline_set_descriptors: bad arguments");
  const int D = p->cfg.tracker_mode == 2 ? 361 : p->cfg.tracker_mode == 3 ? 32 : 128;     // values per row handed in; rows are padded to desc_row bytes
  std::vector<uint8_t> b((size_t)n * p->desc_row, 0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < D; ++k) {
      const float v = desc[(size_t)i * D + k];
      VO_REQUIRE(ctx, v >= 0.f && v <= 255.f && v == (float)(int)v, "pipeline_set_descriptors: descriptor values must be whole numbers 0..255");
      b[(size_t)i * p->desc_row + k] = (uint8_t)v;
    }
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n > 0) VO_HIP_TRY(ctx, mcpy(ctx->stream, p->fdesc(p->cur, seq), b.data(), b.size(), hipMemcpyHostToDevice));
  return VO_OK;
}

// the inverse of vo_pipeline_set_descriptors_seq: the current Features' n rows of sequence seq as whole-number floats
int vo_pipeline_get_descriptors_seq(vo_pipeline* p, int seq, float* desc, int32_t* n_out) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->cfg.tracker_mode != 0, "pipeline_get_descriptors: the pipeline is not in a descriptor tracker mode");
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_get_descriptors: bad sequence index");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_get_descriptors: %d submitted step(s) not collected", p->n_flight);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int32_t n = 0;
  VO_HIP_TRY(ctx, mcpy(st, &n, &p->d_ctl[seq].n, 4, hipMemcpyDeviceToHost));
  n = std::max(0, std::min(n, p->cap));
  if (n_out) *n_out = n;
  if (!desc || n == 0) return VO_OK;
  const int D = p->cfg.tracker_mode == 2 ? 361 : p->cfg.tracker_mode == 3 ? 32 : 128;
  std::vector<uint8_t> b((size_t)n * p->desc_row);
  VO_HIP_TRY(ctx, mcpy(st, b.data(), p->fdesc(p->cur, seq), b.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < D; ++k) desc[(size_t)i * D + k] = (float)b[(size_t)i * p->desc_row + k];
  return VO_OK;
}

extern "C" int vo_pipeline_checkpoint(vo_pipeline* p) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->have_state, "pipeline_checkpoint: no state was handed over");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_checkpoint: %d submitted step(s) not collected", p->n_flight);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!p->d_ckpt_feat) {
    VO_TRY(dev_alloc(p, &p->d_ckpt_feat, p->feat_block));
    VO_TRY(dev_alloc(p, &p->d_ckpt_ctl, (size_t)p->S));
  }
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipMemcpyAsync(p->d_ckpt_feat, (char*)p->feat_mem + (size_t)p->cur * p->feat_block, p->feat_block,
                                 hipMemcpyDeviceToDevice, st));
  VO_HIP_TRY(ctx, hipMemcpyAsync(p->d_ckpt_ctl, p->d_ctl, (size_t)p->S * sizeof(vo_seq_ctl), hipMemcpyDeviceToDevice, st));
  if (p->cfg.tracker_mode != 0) {      // (every sequence's descriptors: S consecutive blocks)
    const size_t bytes = (size_t)p->S * p->cap * p->desc_row;
    if (!p->d_ckpt_fdesc) VO_TRY(dev_alloc(p, &p->d_ckpt_fdesc, bytes));
    VO_HIP_TRY(ctx, hipMemcpyAsync(p->d_ckpt_fdesc, p->fdesc(p->cur, 0), bytes, hipMemcpyDeviceToDevice, st));
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  p->ckpt_frame = p->prev_frame;
  p->ckpt_par = (int)(p->steps_submitted & 1);
  return VO_OK;
}

extern "C" int vo_pipeline_rewind(vo_pipeline* p) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->ckpt_frame >= 0, "pipeline_rewind: no checkpoint");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_rewind: %d submitted step(s) not collected", p->n_flight);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  VO_TRY(worker_idle(p));
  hipStream_t st = ctx->stream;
  // every step has been collected: its chain -- tracker included -- is done, nothing reads the Features any more
  VO_HIP_TRY(ctx, hipMemcpyAsync((char*)p->feat_mem + (size_t)p->cur * p->feat_block, p->d_ckpt_feat, p->feat_block,
                                 hipMemcpyDeviceToDevice, st));
  if (p->cfg.tracker_mode != 0)
    VO_HIP_TRY(ctx, hipMemcpyAsync(p->fdesc(p->cur, 0), p->d_ckpt_fdesc, (size_t)p->S * p->cap * p->desc_row,
                                   hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(ctl_rewind_kernel, dim3(vo_cdiv(p->S, 64)), dim3(64), 0, st, p->d_ctl, p->d_ckpt_ctl, p->S, p->ckpt_par);
  VO_TRY(vo_check_launch(ctx, "ctl_rewind_kernel"));
  // the next step's tracker waits for "the previous step's regroup": that event now stands for the restored state
  if (p->steps_submitted > 0) VO_HIP_TRY(ctx, hipEventRecord(p->evRegroup[(p->steps_submitted - 1) & 1], st));
  else VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  p->slot = 0;
  p->prev_frame = p->ckpt_frame;
  return prime(p, false);            // pyramid + detector of that frame, queued on their streams
}

// ---- lanes: one pipeline, many recordings (vo_hip.h, vo_pipeline_set_camera_seq / _restart_seq / _set_active_seq) ----

int vo_pipeline_set_camera_seq(vo_pipeline* p, int seq, const double* K, const double* Kinv) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S && K, "pipeline_set_camera: bad arguments");
  VO_REQUIRE(ctx, K[0] != 0.0 && K[4] != 0.0, "pipeline_set_camera: singular intrinsics");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_set_camera: %d submitted step(s) not collected", p->n_flight);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  p->cams[(size_t)seq] = make_cam(K, Kinv);
  VO_HIP_TRY(ctx, mcpy(ctx->stream, p->d_cams + seq, &p->cams[(size_t)seq], sizeof(vo_cam), hipMemcpyHostToDevice));
  return VO_OK;
}

// ---- the tracker's forward-backward check (vo_hip.h, vo_pipeline_set_klt_fb): enqueue_tracker reads klt_fb and d_fb ----

int vo_pipeline_set_klt_fb(vo_pipeline* p, double fb_max) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->cfg.tracker_mode == 0, "pipeline_set_klt_fb: KLT tracker mode only (the pipeline runs tracker_mode %d)",
             p->cfg.tracker_mode);
  VO_REQUIRE(ctx, fb_max >= 0.0, "pipeline_set_klt_fb: fb_max must be > 0 pixels (+inf allowed), or 0 for off; got %g", fb_max);
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_set_klt_fb: %d submitted step(s) not collected", p->n_flight);
  if (fb_max > 0.0 && !p->d_fb) {
    VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
    VO_TRY(dev_alloc(p, &p->d_fb, (size_t)p->S * p->cap));
  }
  p->klt_fb = fb_max;
  return VO_OK;
}

int vo_pipeline_get_klt_fb(vo_pipeline* p, double* fb_max) {
  if (!p) return VO_EINVAL;
  VO_REQUIRE(p->ctx, fb_max, "pipeline_get_klt_fb: null pointer");
  *fb_max = p->klt_fb;
  return VO_OK;
}

// ---- the FAST + BRIEF tracker mode's settings (vo_hip.h, vo_pipeline_set_fast_brief): enqueue_fast_front and the chain's
// matcher read them when a step is enqueued, so they hold from the next submit on ----

int vo_pipeline_set_fast_brief(vo_pipeline* p, int fast_threshold, int brief_oriented, int brief_max_distance) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->cfg.tracker_mode == 3, "pipeline_set_fast_brief: FAST tracker mode only (the pipeline runs tracker_mode %d)",
             p->cfg.tracker_mode);
  VO_REQUIRE(ctx, fast_threshold >= 0 && fast_threshold <= 254, "pipeline_set_fast_brief: fast_threshold = %d, must be 0 (= 20) .. 254",
             fast_threshold);
  VO_REQUIRE(ctx, brief_oriented == 0 || brief_oriented == 1, "pipeline_set_fast_brief: brief_oriented = %d, must be 0 or 1",
             brief_oriented);
  VO_REQUIRE(ctx, brief_max_distance <= 256, "pipeline_set_fast_brief: brief_max_distance = %d, must be at most 256 (0 = 64, < 0 = no limit)",
             brief_max_distance);
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_set_fast_brief: %d submitted step(s) not collected", p->n_flight);
  p->fast_threshold = fast_threshold == 0 ? 20 : fast_threshold;
  p->brief_oriented = brief_oriented;
  p->brief_max_distance = brief_max_distance == 0 ? 64 : brief_max_distance;
  return VO_OK;
}

int vo_pipeline_get_fast_brief(vo_pipeline* p, int32_t* fast_threshold, int32_t* brief_oriented, int32_t* brief_max_distance) {
  if (!p) return VO_EINVAL;
  VO_REQUIRE(p->ctx, fast_threshold && brief_oriented && brief_max_distance, "pipeline_get_fast_brief: null pointer");
  *fast_threshold = p->fast_threshold;
  *brief_oriented = p->brief_oriented;
  *brief_max_distance = p->brief_max_distance;
  return VO_OK;
}

// An idle lane's control block carries VO_FAULT_IDLE: every kernel of the main chain returns on it as on a sticky fault (the
// regroup leaves n_p3p = 0, the pose and landmark kernels write a fault record and nothing else), the detector's decision
// says no, the tracker gets n2 = 0 features, and the pyramid's launches leave the lane out.  The host neither redoes its
// steps nor moves its generator.
int vo_pipeline_set_active_seq(vo_pipeline* p, int seq, int active) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_set_active: bad sequence index");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_set_active: %d submitted step(s) not collected", p->n_flight);
  VO_REQUIRE(ctx, p->cfg.tracker_mode == 0, "pipeline_set_active: KLT tracker mode only");
  if (active) {
    VO_REQUIRE(ctx, !p->idle[seq], "pipeline_set_active: an idle lane is reactivated through vo_pipeline_restart_seq");
    return VO_OK;
  }
  if (p->idle[seq]) return VO_OK;
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  int32_t w[2];
  VO_HIP_TRY(ctx, mcpy(st, w, &p->d_ctl[seq].fault, 4, hipMemcpyDeviceToHost));
  w[0] |= VO_FAULT_IDLE;
  w[1] = 0;
  VO_HIP_TRY(ctx, mcpy(st, &p->d_ctl[seq].fault, &w[0], 4, hipMemcpyHostToDevice));
  VO_HIP_TRY(ctx, mcpy(st, &p->d_ctl[seq].n2, &w[1], 4, hipMemcpyHostToDevice));
  p->idle[seq] = 1;
  return VO_OK;
}

// A new recording for lane seq alone (main.py:168-230 per recording: a fresh RANSAC object, its own generator, the
// bootstrap's Features and poses), at frame slot idx -- the slot the next submit reads as `prev`.  The pyramid and the
// detection of that frame are made now for this sequence only; the other lanes' Features, control blocks, generators and
// pyramids are not touched.  Nothing may be in flight (the driver drains first).
int vo_pipeline_restart_seq(vo_pipeline* p, int seq, int idx, int n, const double* kp, const uint8_t* state,
                                       const double* landmarks, const double* tracks, const double* poses,
                                       const double* T_wc, const double* T_cw, const double* T_wc_prev,
                                       const double* T_cw_prev, int num_features, const vo_pcg64* rng) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_TRY(check_state_args(p, "pipeline_restart", seq, n, kp && state && landmarks && tracks && poses,
                          T_wc && T_cw && T_wc_prev && T_cw_prev));
  VO_REQUIRE(ctx, p->cfg.tracker_mode == 0, "pipeline_restart: KLT tracker mode only");
  VO_REQUIRE(ctx, p->have_state && p->seeded, "pipeline_restart: seed and hand the pipeline's states over first");
  VO_REQUIRE(ctx, idx == p->prev_frame, "pipeline_restart: frame slot %d is not the one the next step starts from (%d)", idx,
             p->prev_frame);
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the lane's generator starts over: the device continues at the end of what its ring holds, the look-ahead is dropped
  const vo_pcg64 g = rng ? *rng : p->seed_rng;
  p->rng[seq] = g;
  p->raw_gen[seq] = g;
  p->pos_known[seq] = p->gen_upto[seq];
  p->pos_dev[seq] = p->gen_upto[seq];
  VO_TRY(upload_state(p, seq, n, kp, state, landmarks, tracks, poses, T_wc, T_cw, T_wc_prev, T_cw_prev, num_features, false,
                      &p->gen_upto[seq]));
  p->seq_state[seq] = 1;
  // a prepared pyramid may hold this lane's old frame (or be read behind a pyramid rebuilt below): it goes
  p->prepared_idx = p->prepared_slot = -1;
  if (p->primed) VO_TRY(prime(p, true, seq, 1));    // (else the first submit's prime() makes every sequence's)
  return VO_OK;
}

int vo_pipeline_get_state_seq(vo_pipeline* p, int seq, int32_t* n_out, double* kp, uint8_t* state,
                              uint8_t* candidate_mask, double* landmarks, double* tracks, double* poses, double* T_wc,
                              double* T_wc_prev, vo_ransac_state* rs, int32_t* num_features) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_get_state: bad sequence index");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_get_state: %d submitted step(s) not collected", p->n_flight);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  vo_seq_ctl h;
  VO_HIP_TRY(ctx, mcpy(st, &h, p->d_ctl + seq, sizeof(h), hipMemcpyDeviceToHost));
  const int n = h.n;
  const vo_feat F = vo_feat_seq(p->F[p->cur], (size_t)seq);
  if (n_out) *n_out = n;
  if (num_features) *num_features = h.num_features;
  if (n > 0) {
    if (kp) VO_HIP_TRY(ctx, mcpy(st, kp, F.kp64, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (state) VO_HIP_TRY(ctx, mcpy(st, state, F.state, (size_t)n, hipMemcpyDeviceToHost));
    if (candidate_mask) VO_HIP_TRY(ctx, mcpy(st, candidate_mask, F.cand, (size_t)n, hipMemcpyDeviceToHost));
    if (landmarks) VO_HIP_TRY(ctx, mcpy(st, landmarks, F.land, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (tracks) VO_HIP_TRY(ctx, mcpy(st, tracks, F.track, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (poses) {
      std::vector<double> p12((size_t)n * 12);
      for (int k = 0; k < 12; ++k)
        VO_HIP_TRY(ctx, mcpy(st, &p12[(size_t)k * n], F.pose + (size_t)k * F.pitch, (size_t)n * 8, hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) {
        double row[12];
        for (int k = 0; k < 12; ++k) row[k] = p12[(size_t)k * n + i];
        expand_pose(row, poses + (size_t)16 * i);
      }
    }
  }
  if (T_wc) expand_pose(h.T_wc, T_wc);
  if (T_wc_prev) expand_pose(h.T_wc_prev, T_wc_prev);
  if (rs) {
    rs->outlier_ratio = h.outlier_ratio;
    rs->confidence = p->cfg.ransac_confidence;
    rs->max_iterations = p->cfg.ransac_max_iterations;
    rs->n_iterations = h.n_iterations;
    rs->s = 4;
    rs->adaptive = 1;
  }
  return VO_OK;
}

int vo_pipeline_get_state(vo_pipeline* p, int32_t* n_out, double* kp, uint8_t* state, uint8_t* candidate_mask,
                          double* landmarks, double* tracks, double* poses, double* T_wc, double* T_wc_prev,
                          vo_ransac_state* rs, int32_t* num_features) {
  return vo_pipeline_get_state_seq(p, 0, n_out, kp, state, candidate_mask, landmarks, tracks, poses, T_wc, T_wc_prev, rs,
                                   num_features);
}

int vo_pipeline_get_detection(vo_pipeline* p, double* kp_xy) {
  if (!p || !kp_xy) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_get_detection: %d submitted step(s) not collected", p->n_flight);
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (p->have_state && !p->primed) VO_TRY(prime(p));
  VO_HIP_TRY(ctx, hipEventSynchronize(p->evDet[p->slot]));
  {
    int ran = 0;
    VO_HIP_TRY(ctx, mcpy(ctx->stream, &ran, p->d_det_go + (size_t)p->slot * p->S, 4, hipMemcpyDeviceToHost));
    if (!ran) {                          // the frame's detection was skipped: made now (all sequences)
      VO_TRY(enqueue_detection(p, p->prev_frame, p->slot, true));
      VO_HIP_TRY(ctx, hipStreamSynchronize(p->det->stream));
    }
  }
  VO_HIP_TRY(ctx, mcpy(ctx->stream, kp_xy, p->kp(0, p->slot), (size_t)p->cfg.n_keypoints * 16, hipMemcpyDeviceToHost));
  return VO_OK;
}

int vo_pipeline_get_detection_seq(vo_pipeline* p, int seq, double* kp_xy, int32_t* n_out) {
  if (!p || !kp_xy || !n_out) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_get_detection: bad sequence index");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_get_detection: %d submitted step(s) not collected", p->n_flight);
  VO_REQUIRE(ctx, !p->idle[seq], "pipeline_get_detection: sequence %d is idle", seq);
  VO_TRY(worker_idle(p));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (p->have_state && !p->primed) VO_TRY(prime(p));
  VO_HIP_TRY(ctx, hipEventSynchronize(p->evDet[p->slot]));
  int ran = 0;
  VO_HIP_TRY(ctx, mcpy(ctx->stream, &ran, p->d_det_go + (size_t)p->slot * p->S + seq, 4, hipMemcpyDeviceToHost));
  if (!ran) {                            // the frame's detection was skipped: made now, for this sequence
    VO_TRY(enqueue_detection(p, p->prev_frame, p->slot, true, nullptr, seq, 1));
    VO_HIP_TRY(ctx, hipStreamSynchronize(p->det->stream));
  }
  int32_t n = p->cfg.n_keypoints;
  if (p->d_det_cnt) {
    VO_HIP_TRY(ctx, mcpy(ctx->stream, &n, p->d_det_cnt + (size_t)p->slot * p->S + seq, 4, hipMemcpyDeviceToHost));
    if (n < 0)
      return vo_set_error(ctx, VO_ECAPACITY, "pipeline: the Shi-Tomasi candidate lists of frame %d overflowed (sequence %d)",
                          p->prev_frame, seq);
  }
  *n_out = n;
  if (n > 0) VO_HIP_TRY(ctx, mcpy(ctx->stream, kp_xy, p->kp(seq, p->slot), (size_t)n * 16, hipMemcpyDeviceToHost));
  return VO_OK;
}

int vo_pipeline_bookkeeping(vo_pipeline* p, int phases, const double* new_kp, int n2, const int32_t* pairs, int M,
                            const double* T_wc, const double* T_cw, const uint8_t* p3p_inliers) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_bookkeeping: %d submitted step(s) not collected", p->n_flight);
  VO_REQUIRE(ctx, phases >= 1 && phases <= 3, "pipeline_bookkeeping: phases must be 1, 2 or 3");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (phases & 1) {
    VO_REQUIRE(ctx, new_kp && pairs && T_wc && T_cw && n2 >= 0 && n2 <= p->cap && M >= 0 && M <= n2,
               "pipeline_bookkeeping: bad arguments");
    for (int k = 0; k < M; ++k)
      VO_REQUIRE(ctx, pairs[2 * k] >= 0 && pairs[2 * k] < p->cap && pairs[2 * k + 1] >= 0 && pairs[2 * k + 1] < n2,
                 "pipeline_bookkeeping: pair %d = (%d, %d) is out of range", k, (int)pairs[2 * k], (int)pairs[2 * k + 1]);
    VO_HIP_TRY(ctx, hipMemcpyAsync(p->d_newkp, new_kp, (size_t)n2 * 16, hipMemcpyHostToDevice, st));
    VO_HIP_TRY(ctx, hipMemcpyAsync(p->d_pairs, pairs, (size_t)M * 8, hipMemcpyHostToDevice, st));
    vo_pairs_batch bt;                 // (track ids: the slot the next submitted step reads)
    bt.par = (int)(p->steps_submitted & 1);
    VO_TRY(vo_state_regroup_pairs(ctx, p->d_ctl, p->F[p->cur], p->F[1 - p->cur], p->d_pairs, M, p->d_newkp, n2, p->cap, nullptr,
                                  nullptr, nullptr, 1, &bt));
    VO_HIP_TRY(ctx, hipStreamSynchronize(st));
    p->cur = 1 - p->cur;
    vo_seq_ctl h;
    VO_HIP_TRY(ctx, mcpy(st, &h, p->d_ctl, sizeof(h), hipMemcpyDeviceToHost));
    memcpy(h.T_in_wc, T_wc, 96);
    memcpy(h.T_in_cw, T_cw, 96);
    h.n_cand = h.n_dropped = h.n_land = h.done = 0;
    h.next_id[bt.par] = h.next_id[bt.par ^ 1];     // (no step was submitted: the parity stays, the word moves)
    h.id_step[bt.par] = h.id_step[bt.par ^ 1];
    VO_HIP_TRY(ctx, mcpy(st, p->d_ctl, &h, sizeof(h), hipMemcpyHostToDevice));
    std::vector<uint64_t> bits((size_t)p->words, ~0ull);
    if (p3p_inliers)
      for (int i = 0; i < h.n_tri; ++i)
        if (!p3p_inliers[i]) bits[i >> 6] &= ~(1ull << (i & 63));
    VO_HIP_TRY(ctx, mcpy(st, p->d_best_mask, bits.data(), bits.size() * 8, hipMemcpyHostToDevice));
  }
  if (phases & 1)
    VO_TRY(vo_state_candidates(ctx, p->d_ctl, p->F[p->cur], p->d_best_mask, p->d_cams, p->cfg.bearing_threshold, -1, p->cap));
  if (phases & 2)
    VO_TRY(vo_state_landmarks(ctx, p->d_ctl, p->F[p->cur], p->d_cams, -1, p->cap, nullptr, nullptr, 0u));
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_pipeline_export_state_post_seq(vo_pipeline* p, int seq, const vo_step_result* r, int cap, double* d_record) {
  if (!p || !r || !d_record) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, cap >= 0 && seq >= 0 && seq < p->S, "pipeline_export_state: bad capacity or sequence index");
  pose17 h;
  for (int row = 0; row < 3; ++row) {
    for (int c = 0; c < 3; ++c) h.v[4 * row + c] = r->R_refined[3 * row + c];
    h.v[4 * row + 3] = r->t_refined[row];
  }
  h.v[12] = h.v[13] = h.v[14] = 0.0;
  h.v[15] = 1.0;
  const int n = r->best_index >= 0 ? (r->n_triangulated < cap ? r->n_triangulated : cap) : 0;
  h.v[16] = (double)n;
  // The features of the step collected last stay in their buffer until the step after next is submitted
  // (a step in flight only reads them), so the record can be queued behind whatever the main stream holds.
  const int threads = n * 3 > 17 ? n * 3 : 17;
  {
    vo_prof_scope ps(ctx, VO_K_EXPORT);
    hipLaunchKernelGGL(export_state_kernel, dim3(vo_cdiv(threads, 256)), dim3(256), 0, ctx->stream, h,
                       vo_feat_seq(p->F[p->last_fbuf], (size_t)seq).land, n, cap, d_record);
  }
  return vo_check_launch(ctx, "export_state_kernel");
}

// ---- track ids (vo_hip.h) ----

static int check_track_ids(vo_pipeline* p, const char* who, int seq, bool idle_needed) {
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, p->cfg.track_ids != 0, "%s: the pipeline was created without track_ids", who);
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "%s: bad sequence index", who);
  if (idle_needed) VO_REQUIRE(ctx, p->n_flight == 0, "%s: %d submitted step(s) not collected", who, p->n_flight);
  return VO_OK;
}

size_t vo_pipeline_tracks_record_bytes(int cap) { return 8 * vo_track::record_words(cap); }

int vo_pipeline_get_track_ids_seq(vo_pipeline* p, int seq, int32_t* ids, int32_t* born, int32_t* n_out, int32_t* next_id) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_TRY(check_track_ids(p, "pipeline_get_track_ids", seq, true));
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  vo_seq_ctl h;
  VO_HIP_TRY(ctx, mcpy(st, &h, p->d_ctl + seq, sizeof(h), hipMemcpyDeviceToHost));
  const int n = std::max(0, std::min(h.n, p->cap));
  if (n_out) *n_out = n;
  if (next_id) *next_id = h.next_id[p->steps_submitted & 1];
  if (n > 0 && (ids || born)) {
    std::vector<int32_t> b((size_t)n * 2);
    VO_HIP_TRY(ctx, mcpy(st, b.data(), vo_feat_seq(p->F[p->cur], (size_t)seq).ids, b.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
      if (ids) ids[i] = b[(size_t)2 * i];
      if (born) born[i] = b[(size_t)2 * i + 1];
    }
  }
  return VO_OK;
}

int vo_pipeline_set_track_ids_seq(vo_pipeline* p, int seq, const int32_t* ids, const int32_t* born, int n, int32_t next_id) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_TRY(check_track_ids(p, "pipeline_set_track_ids", seq, true));
  VO_REQUIRE(ctx, p->have_state, "pipeline_set_track_ids: no state was handed over");
  VO_REQUIRE(ctx, n >= 0 && (n == 0 || ids) && next_id >= 0, "pipeline_set_track_ids: bad arguments");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  vo_seq_ctl h;
  VO_HIP_TRY(ctx, mcpy(st, &h, p->d_ctl + seq, sizeof(h), hipMemcpyDeviceToHost));
  VO_REQUIRE(ctx, n == h.n, "pipeline_set_track_ids: %d ids for the sequence's %d features", n, (int)h.n);
  {
    std::vector<int32_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 0; i < n; ++i) {
      VO_REQUIRE(ctx, sorted[i] >= 0 && sorted[i] < next_id, "pipeline_set_track_ids: id %d is not in 0 .. next_id - 1 = %d",
                 (int)sorted[i], (int)next_id - 1);
      VO_REQUIRE(ctx, i == 0 || sorted[i] != sorted[i - 1], "pipeline_set_track_ids: id %d is given twice", (int)sorted[i]);
    }
  }
  const vo_feat F = vo_feat_seq(p->F[p->cur], (size_t)seq);
  if (n > 0) {
    std::vector<int32_t> b((size_t)n * 2);
    VO_HIP_TRY(ctx, mcpy(st, b.data(), F.ids, b.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
      b[(size_t)2 * i] = ids[i];
      if (born) b[(size_t)2 * i + 1] = born[i];
    }
    VO_HIP_TRY(ctx, mcpy(st, F.ids, b.data(), b.size() * 4, hipMemcpyHostToDevice));
  }
  const int32_t both[2] = {next_id, next_id};
  VO_HIP_TRY(ctx, mcpy(st, &p->d_ctl[seq].next_id[0], both, 8, hipMemcpyHostToDevice));
  return VO_OK;
}

int vo_pipeline_export_tracks_post_seq(vo_pipeline* p, int seq, const vo_step_result* r, int cap, void* d_record) {
  if (!p || !r || !d_record) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_TRY(check_track_ids(p, "pipeline_export_tracks", seq, false));
  VO_REQUIRE(ctx, cap >= 0 && ((uintptr_t)d_record & 15) == 0, "pipeline_export_tracks: bad capacity or record alignment");
  VO_REQUIRE(ctx, p->n_flight <= 1, "pipeline_export_tracks: the features of the step collected last are being overwritten");
  const int n = std::max(0, std::min((int)r->n_tracked, p->cap));
  // (the same buffer, and the same reasoning, as vo_pipeline_export_state_post_seq; the step collected last was flight
  //  last_k, so its regroup left next_id and the step counter in slot (last_k + 1) & 1, which only the step after next rewrites)
  {
    vo_prof_scope ps(ctx, VO_K_EXPORT);
    hipLaunchKernelGGL(export_tracks_kernel, dim3(vo_cdiv(std::max(std::min(n, cap), 1), 256)), dim3(256), 0, ctx->stream,
                       vo_feat_seq(p->F[p->last_fbuf], (size_t)seq), (const vo_seq_ctl*)(p->d_ctl + seq),
                       (int)((p->last_k + 1) & 1), n, cap, seq, (unsigned long long*)d_record);
  }
  return vo_check_launch(ctx, "export_tracks_kernel");
}

int vo_pipeline_update_landmarks_seq(vo_pipeline* p, int seq, int n, const int32_t* d_ids, const double* d_X) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_TRY(check_track_ids(p, "pipeline_update_landmarks", seq, true));
  VO_REQUIRE(ctx, p->have_state, "pipeline_update_landmarks: no state was handed over");
  VO_REQUIRE(ctx, n >= 0 && (n == 0 || (d_ids && d_X)), "pipeline_update_landmarks: bad arguments");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n > 0) {
    vo_prof_scope ps(ctx, VO_K_EXPORT);
    hipLaunchKernelGGL(update_landmarks_kernel, dim3(vo_cdiv(p->cap, 256)), dim3(256), 0, st, vo_feat_seq(p->F[p->cur], (size_t)seq),
                       (const vo_seq_ctl*)(p->d_ctl + seq), p->cap, n, d_ids, d_X);
    VO_TRY(vo_check_launch(ctx, "update_landmarks_kernel"));
  }
  VO_HIP_TRY(ctx, hipStreamSynchronize(st));
  return VO_OK;
}

int vo_pipeline_export_state_post(vo_pipeline* p, const vo_step_result* r, int cap, double* d_record) {
  return vo_pipeline_export_state_post_seq(p, 0, r, cap, d_record);
}

int vo_pipeline_export_state_join(vo_pipeline* p, void* consumer) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t use = consumer ? (hipStream_t)consumer : ctx->stream;
  hipStream_t st = ctx->stream;
  if (use == st) return VO_OK;
  VO_HIP_TRY(ctx, hipEventRecord(p->evB, st));
  VO_HIP_TRY(ctx, hipStreamWaitEvent(use, p->evB, 0));   // consumer: behind the records
  VO_HIP_TRY(ctx, hipEventRecord(p->evA, use));
  VO_HIP_TRY(ctx, hipStreamWaitEvent(st, p->evA, 0));    // later records: behind what the consumer holds so far
  return VO_OK;
}

}  // extern "C"
