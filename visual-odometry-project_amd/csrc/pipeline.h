// Internal to the frame pipeline (pipeline.hip, pipeline_state.hip, pipeline_step.hip): the pipeline object and the
// helpers more than one of those units uses.
#pragma once

#include <linux/futex.h>
#include <sys/prctl.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "vo_state.h"
#include "state_device.h"

struct vo_pipeline_boot;    // pipeline_bootstrap.hip: the two-view bootstrap's workspace

struct vo_pipeline {
  vo_ctx* ctx = nullptr;
  vo_ctx* det = nullptr;             // detection stream (+ the NMS workspace of all sequences)
  vo_ctx* trk = nullptr;             // tracker stream: pyramid and KLT of step k+1 run beside the pose estimation of step k
  hipEvent_t evKlt[2] = {nullptr, nullptr}, evRegroup[2] = {nullptr, nullptr};
  vo_pipeline_config cfg;
  // intrinsics per sequence (vo_pipeline_set_camera_seq; all cfg.K at create): host copy (the recovery path) and the device
  // table the kernels read entry q of
  std::vector<vo_cam> cams;
  vo_cam* d_cams = nullptr;          // [S]
  // lanes (vo_pipeline_set_active_seq / vo_pipeline_restart_seq): idle[q] = sequence q does no work and its control block
  // carries VO_FAULT_IDLE; seed_rng: the generator state of the last vo_pipeline_seed (a restarted lane's default)
  std::vector<char> idle;
  vo_pcg64 seed_rng;
  int n_levels = 1, cap = 0, words = 0, S = 1;
  size_t px = 0, pyr_bytes = 0;
  // ---- per-sequence buffers: S consecutive blocks each ----
  uint8_t* d_img = nullptr;          // [S][n_frames][px]
  uint8_t* d_pyr = nullptr;          // [S][3][pyr_bytes]      (frame count mod 3)
  double* d_kp = nullptr;            // [S][3][N * 2]          detector output per frame slot
  double* d_scores[2] = {nullptr, nullptr};   // [S][px] each, alternating between consecutive detections
  int* d_det_go = nullptr;           // [3][S]: 1 = the detector ran for that sequence on the frame in keypoint slot s
  // vo_pipeline_config.detector = 1 (Shi-Tomasi re-detect; all null otherwise): the batched detector's float corners and
  // verdicts of the detection being made (the detection stream runs one at a time), and what the closing kernel leaves
  // per keypoint slot: the corner count of every sequence (-1: its candidate lists overflowed)
  float* d_st_xy = nullptr;          // [S][N * 2]
  int32_t* d_st_n = nullptr;         // [2][S]: counts, verdicts
  int32_t* d_det_cnt = nullptr;      // [3][S]
  int st_rounds = 0;                 // round launches of the minimum-distance rule per detection (VO_ST_ROUNDS)
  double detect_limit = 0.0;         // detect when n < detect_limit * num_features (< 0: always)
  double detect_losses = 2.5;        // ... with n extrapolated by this many times the last step's loss
  hipEvent_t evPyr[3] = {nullptr, nullptr, nullptr}, evDet[3] = {nullptr, nullptr, nullptr};
  // frame upload: pinned staging per (sequence, frame slot), allocated on first use; evImg[idx]: every copy into slot idx
  // that vo_pipeline_set_frame queued (tracker's stream) is in HBM
  std::vector<uint8_t*> h_img;
  std::vector<hipEvent_t> evImg;
  // vo_pipeline_set_frame_pinned: DMA straight from the caller's pinned buffer on a stream of its own (beside the kernels,
  // not in front of the pyramid); evUp[idx]: every such copy into slot idx is in HBM.  The sequences of one slot may be
  // filled either way (a batch driver mixes them; a restart fills one sequence's frame): pinned[q * n_frames + idx] = the
  // last upload of (q, idx) was pinned, n_pinned[idx] = how many sequences of slot idx that holds for -- the pyramid and
  // the detector wait for evUp while it is > 0; plain_used[idx]: a plain upload went into slot idx (the detector waits
  // for evImg)
  hipStream_t up_stream = nullptr;
  std::vector<hipEvent_t> evUp;
  std::vector<char> pinned, plain_used;
  std::vector<int> n_pinned;
  // Frame ingest (ingest.hip; vo_pipeline_set_frame_bgr_seq / _pinned, vo_pipeline_set_distortion_seq): a frame that is not a
  // finished grey image is copied into a raw buffer and the ingest kernel writes the slot behind the copy, on the same
  // stream; evImg / evUp are recorded behind the kernel.  One raw buffer per stream (d_raw[0]: the tracker's, d_raw[1]:
  // up_stream), reused in stream order; h_bgr: the plain three-channel call's pinned staging, evBgr: its last DMA has read
  // it.  All of it is made on first use: a pipeline fed grey frames of a pinhole camera has none of it.
  struct lens_t {
    bool on = false, have_raw = false;
    double dist[5] = {0, 0, 0, 0, 0}, K_raw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  };
  std::vector<lens_t> lens;          // [S] once a lane has been given coefficients (empty: no lane has)
  uint8_t* d_raw[2] = {nullptr, nullptr};
  uint8_t* h_bgr = nullptr;
  hipEvent_t evBgr = nullptr;
  // vo_pipeline_prepare: the pyramid of frame slot prepared_idx sits in pyramid slot prepared_slot, built behind the
  // previous tracker -- the next submit whose `next` is that frame does not build it again (-1: none)
  int prepared_idx = -1, prepared_slot = -1;
  int slot = 0, det_flip = 0, prev_frame = -1;
  // Features double buffer: a step reads F[cur] (frame k-1) and writes F[1 - cur] (frame k)
  vo_feat F[2];
  void* feat_mem = nullptr;
  int cur = 0;
  vo_seq_ctl* d_ctl = nullptr;       // [S]
  float *d_next = nullptr, *d_err = nullptr;   // [S][cap * 2], [S][cap]
  uint8_t* d_status = nullptr;
  // vo_pipeline_set_klt_fb: the tracker's forward-backward check (0: off, the plain launch); d_fb [S][cap] beside d_err,
  // made when the check is first switched on
  double klt_fb = 0.0;
  float* d_fb = nullptr;
  double *d_R = nullptr, *d_t = nullptr;       // [S][hyp * 9], [S][hyp * 3]
  uint8_t* d_valid = nullptr;
  int32_t *d_counts = nullptr, *d_samples = nullptr, *d_pend = nullptr;   // d_pend: [S][cap], state_walk_landmarks_kernel's scratch
  uint64_t *d_masks = nullptr, *d_best_mask = nullptr;
  double* d_table = nullptr;
  std::vector<double> table;
  int table_len = 0;
  // generator outputs: one power-of-two ring per sequence in HBM, kept filled ahead of the device by the host
  uint32_t* d_raws = nullptr;        // [S][ring_len]
  uint32_t ring_len = 0;
  uint32_t* h_stage = nullptr;
  size_t stage_cap = 0;
  std::vector<uint64_t> gen_upto, pos_known, pos_dev;   // generated up to / the estimator's position after the last closed
                                                        // step / the device's position (ahead of it while a step continues)
  std::vector<vo_pcg64> raw_gen, rng;
  hipEvent_t evRaw = nullptr;
  bool raw_pending = false, seeded = false, have_state = false, primed = false;
  // results: records in mapped host memory, [4 slots][S]
  vo_step_result *h_res = nullptr, *m_res = nullptr;
  volatile unsigned* h_seq = nullptr;
  unsigned* m_seq = nullptr;
  unsigned seq = 0;
  // front_job (descriptor modes): the worker's job count once it has made the flight's front (0: made by the caller)
  struct flight_t { int prev_idx = 0, next_idx = 0, a = 0, b = 0, fcur = 0, rslot = 0; unsigned seq = 0; long k = 0; unsigned front_job = 0; };
  flight_t flight[2];
  int n_flight = 0;
  long steps_submitted = 0;
  std::vector<unsigned> slot_seq;    // [4][S]: the number sequence q's record in result slot r will carry
  std::vector<char> seq_state;       // [S]: a state was handed over before (the RANSAC object persists, ransac.py:47-56)
  int last_fbuf = 0;
  long last_k = 0;                   // the flight number of the step collected last (track ids: its slot of vo_seq_ctl.next_id)
  int ckpt_par = 0;                  // the parity of the step that followed the checkpoint (which next_id slot the copy's is)
  hipEvent_t evA = nullptr, evB = nullptr;
  double* d_newkp = nullptr;         // scratch of the bookkeeping entry point
  vo_pipeline_boot* boot = nullptr;  // vo_pipeline_bootstrap_seq's workspace (device memory in dev_mem; made at its first call)
  vo_structure_loop* sloop = nullptr;   // structure_loop.hip: the loop attached by vo_structure_loop_create (null: none)
  // SIFT tracker mode (vo_pipeline_config.tracker_mode = 1; src/vo/features/tracker.py:60-61, sift.py:23-56): the frame's
  // keypoints and descriptors are made by the SIFT kernels on the tracker's stream, matched against the descriptors the
  // current Features carry (bytes, regrouped with them: matches.py:51-58, 134-141) on the matrix cores, and regrouped
  // from the explicit pair list -- nothing of it leaves HBM.  One sequence per pipeline in this mode.
  // Harris tracker mode (tracker_mode = 2; tracker.py:58-59, harris.py:50-84): the same with the detector's N keypoints
  // (every frame), their 19x19 raw patches as 384-byte rows, ratio 0.85 -- for any number of sequences: the detection,
  // the patches, the matcher, the regroup and the descriptor gather take all S in one launch each (grid's extra dimension).
  // Both descriptor modes keep up to frame_rows keypoints per frame (Harris: n_keypoints; SIFT: cfg.sift_cap, or with
  // cfg.sift_cap = -1 (sift_all) every keypoint of the frame, frame_rows = feature_cap; a frame that has more, or whose
  // SIFT lists overflow, is a VO_FAULT_CAPACITY step -- d_sover says which and how many).
  // FAST + BRIEF tracker mode (tracker_mode = 3; vo/features/fast.py's FASTBRIEFDetector): the frame's FAST-9 corners -- up
  // to n_keypoints, however many the frame has: the count stays in d_frame_n -- and their BRIEF-256 descriptors (32-byte
  // rows) on the detection stream, the Hamming 2-NN with the ratio / distance / first-come rule on the main stream; the
  // regroup, the descriptor gather and everything behind them are the Harris mode's, for any number of sequences.
  int frame_rows = 0;
  bool sift_all = false;
  int desc_row = 128;                // bytes per descriptor row: 128 (SIFT), 384 (361 patch bytes, padded) or 32 (BRIEF-256)
  int fast_threshold = 20, brief_oriented = 0, brief_max_distance = 64;   // vo_pipeline_set_fast_brief (FASTBRIEFDetector's defaults)
  float* d_skp = nullptr;            // [3][frame_rows * 6]   keypoint rows of the frame in slot s (SIFT: one sequence)
  int32_t* d_sover = nullptr;        // [3][2] sift_all: the frame in slot s -- its verdict (vo_sift_all_batch_dev's d_over),
                                     //        its keypoint count (-1: list overflow)
  uint8_t* d_frame_desc = nullptr;   // [3][S][frame_rows * desc_row] the descriptors of the frame in slot s
  int32_t* d_frame_n = nullptr;      // [3][S] its keypoint count; [S]: pairs of the step being enqueued
  uint8_t* d_fdesc = nullptr;        // [2][S][cap * desc_row] descriptors of the Features buffers F[0], F[1]
  int32_t* d_srcrow = nullptr;       // [S][cap]            new keypoint behind every regrouped feature
  uint8_t* d_ckpt_fdesc = nullptr;   // [S][cap * desc_row]
  // vo_pipeline_checkpoint / _rewind: a copy of one Features buffer (all sequences) and of the control blocks
  char* d_ckpt_feat = nullptr;
  vo_seq_ctl* d_ckpt_ctl = nullptr;
  size_t feat_block = 0;             // bytes of one Features buffer (F[0] and F[1] are consecutive blocks of feat_mem)
  int ckpt_frame = -1;
  int32_t* d_pairs = nullptr;        // [cap * 2] ([S][cap * 2] in the descriptor modes)
  long n_recovered = 0, n_continued = 0;
  bool pose_fault_hook = true;       // debug_fault_every < 0 applies to submitted steps, not to what recover_step re-enqueues
  // Detection worker: a second host thread enqueues the detection of every step (6 launches) while the caller's
  // thread enqueues pyramid, tracker and the main-stream chain (6 launches): a dozen launches and half a dozen event
  // calls per step cost one thread 70-150 us on a loaded host, more than the GPU needs for the step.
  // Host threads: this pipeline's caller and (budget 2) the detection worker.  Neither spins for long: a wait first polls
  // for spin_us microseconds (a one-sequence step is ~120 us, the common waits are shorter), then blocks -- the worker on a
  // futex until a job is posted, the caller in 20 us sleeps between looks at the mapped record.  VO_HOST_THREADS_BUDGET=1:
  // no worker (the caller enqueues the detection itself, behind the step's chain) and no spinning at all -- for many ranks
  // on few cores (a job's CPU quota); VO_HOST_SPIN_US overrides the polling window.
  std::thread worker;
  std::atomic<unsigned> job_posted{0}, job_done{0};
  std::atomic<int> worker_asleep{0};
  std::atomic<bool> quit{false};
  int threads_budget = 2;
  double spin_s = 150e-6;
  vo_stream_cfg side_cfg;            // what the side contexts' streams were created with (side_pool)
  int desc_chains_pending = 0;       // descriptor modes: flights whose main-stream chain is not enqueued yet (their fronts are
                                     // being made by the worker; the chain follows at the next submit or at collect)
  flight_t jobs[4];
  int worker_rc = 0;
  char worker_err[256] = {0};
  double dbg_part[4] = {0, 0, 0, 0};   // VO_DEBUG_TIMING: submit split into worker wait / tracker / raws / chain
  double dbg_submit = 0, dbg_wait = 0;
  long dbg_steps = 0;
  // what dev_alloc / pin_alloc / make_event made: released by vo_pipeline_destroy
  std::vector<void*> dev_mem, host_mem;
  std::vector<hipEvent_t> events;

  // block q of the per-sequence arrays
  uint8_t* img(int q, int idx) const { return d_img + ((size_t)q * cfg.n_frames + idx) * px; }
  size_t img_stride() const { return (size_t)cfg.n_frames * px; }
  uint8_t* pyr(int q, int s) const { return d_pyr + ((size_t)q * 3 + s) * pyr_bytes; }
  size_t pyr_stride() const { return 3 * pyr_bytes; }
  double* kp(int q, int s) const { return d_kp + ((size_t)q * 3 + s) * cfg.n_keypoints * 2; }
  size_t det_stride() const { return (size_t)3 * cfg.n_keypoints * 2; }
  vo_step_result* res_h(int rslot, int q) const { return h_res + (size_t)rslot * S + q; }
  uint8_t* frame_desc(int s, int q) const { return d_frame_desc + ((size_t)s * S + q) * frame_rows * desc_row; }
  uint8_t* fdesc(int fb, int q) const { return d_fdesc + ((size_t)fb * S + q) * cap * desc_row; }
  int32_t* frame_n(int s, int q) const { return d_frame_n + (size_t)s * S + q; }        // keypoints of the frame in slot s
  int32_t* npairs(int q) const { return d_frame_n + (size_t)3 * S + q; }
  volatile unsigned* seq_h(int rslot, int q) const { return h_seq + (size_t)rslot * S + q; }
};

// ---- helpers shared by the pipeline's units ----

// Device and host memory, and events, made through these are the pipeline's: vo_pipeline_destroy releases them.
template <typename T>
static inline int dev_alloc(vo_pipeline* p, T** out, size_t count) {
  hipError_t e = hipMalloc((void**)out, count * sizeof(T) ? count * sizeof(T) : 256);
  if (e != hipSuccess) return vo_set_error(p->ctx, VO_ENOMEM, "hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
  p->dev_mem.push_back((void*)*out);
  return VO_OK;
}

template <typename T>
static inline int pin_alloc(vo_pipeline* p, T** out, size_t count, unsigned flags = hipHostMallocMapped | hipHostMallocCoherent) {
  hipError_t e = hipHostMalloc((void**)out, count * sizeof(T), flags);
  if (e != hipSuccess) {
    *out = nullptr;
    return vo_set_error(p->ctx, VO_ENOMEM, "hipHostMalloc failed: %s", hipGetErrorString(e));
  }
  p->host_mem.push_back((void*)*out);
  return VO_OK;
}

static inline int make_event(vo_pipeline* p, hipEvent_t* e) {
  if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return vo_set_error(p->ctx, VO_EHIP, "hipEventCreate failed");
  p->events.push_back(*e);
  return VO_OK;
}

// Blocking copies on the pipeline's own main stream: hipMemcpy would go through the null stream, one more stream
// competing for the four hardware queues the pipeline's streams are spread over.
static inline hipError_t mcpy(hipStream_t st, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

static inline double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + ts.tv_nsec * 1e-9;
}

static inline long futex_wait(std::atomic<unsigned>* a, unsigned expect) {
  return syscall(SYS_futex, reinterpret_cast<unsigned*>(a), FUTEX_WAIT_PRIVATE, expect, nullptr, nullptr, 0);
}

static inline long futex_wake(std::atomic<unsigned>* a) {
  return syscall(SYS_futex, reinterpret_cast<unsigned*>(a), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
}

// a short sleep between two looks at something another agent writes (the kernel's default timer slack would round
// 20 us up to 70: one microsecond of slack for this thread, set once)
static inline void nap(long ns) {
  static thread_local bool slack_set = false;
  if (!slack_set) {
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
    slack_set = true;
  }
  timespec ts{0, ns};
  nanosleep(&ts, nullptr);
}

// polls `done` for at most spin_s seconds, then between naps
template <typename F>
static inline void wait_until(double spin_s, F done) {
  const double t_end = now_s() + spin_s;
  for (unsigned it = 0;; ++it) {
    if (done()) return;
    if ((it & 15) != 15 || now_s() < t_end) __builtin_ia32_pause();
    else nap(5000);
  }
}

// K and its inverse: Kinv as given, or (NULL) computed as the reference's np.linalg.inv gives it for a pinhole K
static inline vo_cam make_cam(const double* K, const double* Kinv) {
  vo_cam c;
  memcpy(c.K, K, sizeof(c.K));
  if (Kinv) {
    memcpy(c.Kinv, Kinv, sizeof(c.Kinv));
  } else {
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double ki[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
    memcpy(c.Kinv, ki, sizeof(ki));
  }
  return c;
}

// ---- the step engine (pipeline_step.hip), as the other units call it ----
#define VO_PIPE_INTERNAL __attribute__((visibility("hidden")))
VO_PIPE_INTERNAL void worker_main(vo_pipeline* p);
// waits (host) until the worker has enqueued everything it was given
VO_PIPE_INTERNAL int worker_idle(vo_pipeline* p);
// pyramid and detection of the frame the handed-over states belong to, sequences q0 .. q0 + Sn - 1 (Sn = 0: all of them)
VO_PIPE_INTERNAL int prime(vo_pipeline* p, bool wait = true, int q0 = 0, int Sn = 0);
// releases p->boot (its device memory is in dev_mem)
VO_PIPE_INTERNAL void vo_pipeline_boot_free(vo_pipeline* p);
// structure_loop.hip: releases an attached loop; the write-back of the last post once more for lane q, whose step of flight
// k went through the host path or was continued (a no-op unless that post waited behind flight k)
VO_PIPE_INTERNAL void vo_structure_loop_free(vo_pipeline* p);
VO_PIPE_INTERNAL int vo_structure_loop_requeue(vo_pipeline* p, int q, long k);
VO_PIPE_INTERNAL int enqueue_detection(vo_pipeline* p, int frame, int s, bool force, char* err_buf = nullptr, int q0 = 0, int Sn = 0);
