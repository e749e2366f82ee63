// Frame pipeline (vo_pipeline_*): lifetime -- create, destroy and the side-context pool --, frame upload and the small
// getters.  The step engine is pipeline_step.hip, the handed-over state pipeline_state.hip.
#include "pipeline.h"

#pragma clang fp contract(off)

namespace {

hipError_t mset(hipStream_t st, void* dst, int v, size_t bytes) {
  hipError_t e = hipMemsetAsync(dst, v, bytes, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

uint32_t next_pow2(uint64_t v) {
  uint32_t r = 1;
  while (r < v) r <<= 1;
  return r;
}

// one Features buffer for S sequences of `cap` features: every array S * cap entries
vo_feat carve(char*& q, int cap, int S, bool ids) {
  vo_feat f;
  auto take = [&](size_t bytes) {
    void* r = q;
    q += (bytes * S + 255) & ~size_t(255);
    return r;
  };
  f.kp = (float*)take((size_t)cap * 8);
  f.kp64 = (double*)take((size_t)cap * 16);
  f.state = (uint8_t*)take((size_t)cap);
  f.cand = (uint8_t*)take((size_t)cap);
  f.land = (double*)take((size_t)cap * 24);
  f.track = (double*)take((size_t)cap * 16);
  f.pose = (double*)take((size_t)cap * 96);
  f.pitch = cap;
  f.ids = ids ? (int2*)take((size_t)cap * 8) : nullptr;     // (vo_pipeline_config.track_ids; inside the block: checkpoint,
  return f;                                                 //  rewind and the per-sequence strides cover it)
}

size_t feat_bytes(int cap, int S, bool ids) {
  char* q = nullptr;
  carve(q, cap, S, ids);
  return (size_t)(q - (char*)nullptr);
}

}  // namespace

// ---- side contexts (the tracker's and the detector's stream + workspace) are kept, not destroyed ----
// Destroying a pipeline's side streams after every pipeline and creating the next one's hung inside the runtime about once
// in 400 create / destroy cycles (tools/dev/soak_fault_timing.py with VO_DEBUG_STAGES=1: the process sat in vo_destroy of a
// side context -- hipStreamDestroy / hipFree -- with every stream idle).  A closed pipeline's side contexts go to a pool
// keyed by what their streams were created with (compute-unit mask, priority); the next pipeline with the same keys takes
// them -- streams, workspace and all.  Contexts of OTHER keys are destroyed when a pipeline is created (live CU-masked
// queues slow every other queue of the process), so at most one configuration's contexts stay alive.
// VO_SIDE_POOL=0: off.
struct side_entry {
  int device;
  vo_stream_cfg key;
  vo_ctx* c;
};
static std::mutex g_side_mu;
static std::vector<side_entry>& side_pool() {
  static std::vector<side_entry>* v = new std::vector<side_entry>();
  return *v;
}
static bool side_pool_on() {
  static const bool on = !(getenv("VO_SIDE_POOL") && getenv("VO_SIDE_POOL")[0] == '0');
  return on;
}
static bool side_pool_destroy_at_exit() {
  if (const char* e = getenv("VO_SIDE_POOL_ATEXIT")) return e[0] != '0';
  const char* pre = getenv("LD_PRELOAD");
  return (pre && strstr(pre, "rocprof")) || getenv("ROCP_TOOL_LIBRARIES") != nullptr;
}
// VO_SIDE_POOL_EVICT=0: contexts of other configurations stay alive beside the new pipeline's (a test suite that switches
// configuration from test to test and does not care about the speed of its queues: no stream is destroyed before the process ends)
static bool side_pool_evicts() {
  static const bool on = !(getenv("VO_SIDE_POOL_EVICT") && getenv("VO_SIDE_POOL_EVICT")[0] == '0');
  return on;
}
// device < 0: every context goes
static void side_evict_except(int device, const vo_stream_cfg& keep) {
  std::vector<vo_ctx*> gone;
  {
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto& v = side_pool();
    for (size_t i = 0; i < v.size();) {
      if (device < 0 || (v[i].device == device && !(v[i].key == keep))) {
        gone.push_back(v[i].c);
        v.erase(v.begin() + (long)i);
      } else {
        ++i;
      }
    }
  }
  for (vo_ctx* c : gone) vo_destroy(c);
}
static int side_take(int device, const vo_stream_cfg& key, vo_ctx** out) {
  if (side_pool_on()) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto& v = side_pool();
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i].device == device && v[i].key == key) {
        *out = v[i].c;
        v.erase(v.begin() + (long)i);
        return VO_OK;
      }
  }
  return vo_create_stream(device, nullptr, key, out);
}
static void side_give(vo_ctx* c, const vo_stream_cfg& key) {
  if (!c) return;
  if (side_pool_on() && c->own_stream) {
    c->prof_on = false;
    c->prof_kernel = -1;
    c->prof_every = 1;
    c->next_stop = nullptr;
    c->nms_kp_f32 = nullptr;
    c->err[0] = 0;
    // Under rocprofv3 what is still kept when the process ends is destroyed while the runtime is alive (streams left to the
    // runtime's own teardown crashed it there); registered on first use, i.e. after the runtime's own exit handlers.  Without
    // the profiler they are left alone: a process about to end gains nothing from a call that stalls once in a few hundred.
    // VO_SIDE_POOL_ATEXIT=1 / 0 overrides.
    static const bool at_exit = (std::atexit([] {
                                   if (side_pool_destroy_at_exit()) side_evict_except(-1, {});
                                 }),
                                 true);
    (void)at_exit;
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto& v = side_pool();
    size_t same = 0;
    for (const side_entry& e : v) same += e.device == c->device && e.key == key ? 1 : 0;
    if (same < 4) {
      v.push_back({c->device, key, c});
      return;
    }
  }
  vo_destroy(c);
}

// VO_DEBUG_STAGES=1: a line on stderr at every stage of create / destroy (which runtime call a stall sits in)
static void dbg_stage(const char* what) {
  static const bool on = getenv("VO_DEBUG_STAGES") != nullptr;
  if (on) {
    fprintf(stderr, "[stage] %s\n", what);
    fflush(stderr);
  }
}

extern "C" {

int vo_klt_num_levels(int H, int W, int win, int max_level);
size_t vo_pyramid_bytes(int H, int W, int n_levels);

void vo_pipeline_destroy(vo_pipeline* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  dbg_stage("destroy: enter");
  if (p->worker.joinable()) {          // the worker first: it enqueues on the detection stream
    p->quit.store(true, std::memory_order_seq_cst);
    futex_wake(&p->job_posted);
    p->worker.join();
  }
  dbg_stage("destroy: worker joined");
  // every stream next: nothing may still read what is freed below
  (void)hipStreamSynchronize(p->ctx->stream);
  for (vo_ctx* q : {p->det, p->trk})
    if (q) (void)hipStreamSynchronize(q->stream);
  if (p->up_stream) (void)hipStreamSynchronize(p->up_stream);
  dbg_stage("destroy: streams idle");
  vo_structure_loop_free(p);
  vo_pipeline_boot_free(p);
  for (void* q : p->dev_mem) (void)hipFree(q);
  for (void* q : p->host_mem) (void)hipHostFree(q);
  dbg_stage("destroy: memory freed");
  if (p->up_stream) (void)hipStreamDestroy(p->up_stream);
  for (hipEvent_t e : p->events) (void)hipEventDestroy(e);
  dbg_stage("destroy: events destroyed");
  if (p->det) (p->det->own_stream ? side_give(p->det, p->side_cfg) : vo_destroy(p->det));
  if (p->trk) (p->trk->own_stream ? side_give(p->trk, p->side_cfg) : vo_destroy(p->trk));
  dbg_stage("destroy: side contexts handed back");
  if (getenv("VO_DEBUG_TIMING") && p->dbg_steps > 0)
    fprintf(stderr, "[vo_pipeline] %ld steps x %d sequence(s): host %.1f us enqueueing (worker wait %.1f, tracker %.1f, raws %.1f, "
            "chain %.1f), %.1f us waiting per step; %ld finished through the host path, %ld further batches of hypotheses\n",
            p->dbg_steps, p->S, 1e6 * p->dbg_submit / p->dbg_steps, 1e6 * p->dbg_part[0] / p->dbg_steps,
            1e6 * p->dbg_part[1] / p->dbg_steps, 1e6 * p->dbg_part[2] / p->dbg_steps, 1e6 * p->dbg_part[3] / p->dbg_steps,
            1e6 * p->dbg_wait / p->dbg_steps, p->n_recovered, p->n_continued);
  delete p;
}

int vo_pipeline_create(vo_ctx* ctx, const vo_pipeline_config* cfg, vo_pipeline** out) {
  dbg_stage("create: enter");
  if (!ctx || !cfg || !out) return VO_EINVAL;
  *out = nullptr;
  VO_REQUIRE(ctx, cfg->H > 0 && cfg->W > 0 && cfg->n_frames >= 2, "pipeline: bad stream shape");
  VO_REQUIRE(ctx, cfg->n_keypoints >= 8 && cfg->n_keypoints <= 16384, "pipeline: n_keypoints must be in 8..16384");
  VO_REQUIRE(ctx, cfg->hyp >= 1 && cfg->hyp <= (1 << 20), "pipeline: hyp must be in 1..2^20");
  VO_REQUIRE(ctx, cfg->K[0] != 0.0 && cfg->K[4] != 0.0, "pipeline: singular intrinsics");
  VO_REQUIRE(ctx, cfg->refine_iters >= 0 && cfg->refine_iters <= 100, "pipeline: refine_iters must be in 0..100");
  VO_REQUIRE(ctx, cfg->sequences >= 0 && cfg->sequences <= 256, "pipeline: sequences must be in 1..256");
  VO_REQUIRE(ctx, cfg->tracker_mode >= 0 && cfg->tracker_mode <= 3,
             "pipeline: tracker_mode must be 0 (klt), 1 (sift), 2 (harris) or 3 (fast)");
  VO_REQUIRE(ctx, cfg->tracker_mode != 1 || cfg->sequences <= 1, "pipeline: the SIFT tracker mode runs one sequence per pipeline");
  VO_REQUIRE(ctx, cfg->tracker_mode != 1 || cfg->sift_cap >= -1,
             "pipeline: sift_cap must be -1 (every keypoint), 0 (n_keypoints) or 1..4000, got %d", cfg->sift_cap);
  VO_REQUIRE(ctx, cfg->detector >= 0 && cfg->detector <= 1, "pipeline: detector must be 0 (harris) or 1 (shi-tomasi), got %d",
             cfg->detector);
  VO_REQUIRE(ctx, cfg->track_ids == 0 || cfg->track_ids == 1, "pipeline: track_ids must be 0 (off) or 1 (on), got %d", cfg->track_ids);
  VO_REQUIRE(ctx, cfg->detector == 0 || cfg->tracker_mode == 0,
             "pipeline: the Shi-Tomasi detector (detector = 1) belongs to the KLT tracker mode (tracker_mode = 0)");
  if (cfg->detector == 1) {            // klt.py:24-26 where a field is 0; the rest is what the batched detector takes
    const int rc = vo_good_features_batch_check(ctx, cfg->sequences > 0 ? cfg->sequences : 1, cfg->H, cfg->W,
                                                cfg->st_quality == 0.0 ? 0.01 : cfg->st_quality,
                                                cfg->st_min_distance == 0.0 ? 8.0 : cfg->st_min_distance,
                                                cfg->st_block == 0 ? 7 : cfg->st_block);
    if (rc != VO_OK) return rc;
  }
  const int cap = cfg->feature_cap > 0 ? cfg->feature_cap : 2 * cfg->n_keypoints;
  VO_REQUIRE(ctx, cap >= cfg->n_keypoints && cap <= 32768, "pipeline: feature_cap must be in n_keypoints..32768");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  vo_pipeline* p = new (std::nothrow) vo_pipeline();
  if (!p) return VO_ENOMEM;
  p->ctx = ctx;
  p->cfg = *cfg;
  p->cap = cap;
  p->words = vo_cdiv(cap, 64);
  p->S = cfg->sequences > 0 ? cfg->sequences : 1;
  p->cfg.sequences = p->S;
  const int S = p->S;
  if (p->cfg.bearing_threshold == 0.0) p->cfg.bearing_threshold = 0.0075;    // state.py:8
  if (p->cfg.redetect_fraction == 0.0) p->cfg.redetect_fraction = 0.8;       // klt.py:212
  if (p->cfg.detect_margin == 0.0) p->cfg.detect_margin = 0.01;
  if (p->cfg.detect_losses <= 0.0) p->cfg.detect_losses = 2.5;
  if (p->cfg.st_block == 0) p->cfg.st_block = 7;                             // klt.py:24-26
  if (p->cfg.st_quality == 0.0) p->cfg.st_quality = 0.01;
  if (p->cfg.st_min_distance == 0.0) p->cfg.st_min_distance = 8.0;
  p->detect_losses = p->cfg.detect_losses;
  p->detect_limit = p->cfg.detect_margin < 0.0 ? -1.0 : p->cfg.redetect_fraction + p->cfg.detect_margin;
  if (p->cfg.debug_never_detect) p->detect_limit = 0.0;     // test hook: only forced detections (state hand-over, host path)
  {
    bool given = false;
    for (double v : cfg->Kinv) given |= v != 0.0;
    p->cams.assign((size_t)p->S, make_cam(cfg->K, given ? cfg->Kinv : nullptr));
  }
  p->idle.assign((size_t)p->S, 0);
  memset(&p->seed_rng, 0, sizeof(p->seed_rng));
  int rc = VO_OK;
  // Three streams -- main (the caller's), tracker, detection -- plus the null stream (the caller's synchronous
  // copies, torch): the runtime spreads streams over four hardware queues and kernels of one queue run in order.
  // A fifth stream shares a queue: with two detection streams the second sat on the tracker's queue and delayed
  // it every other frame (rocprofv3 trace, same queue id; 8.2k vs 5.1k frames/s run to run).  Hence the next
  // frame's pyramid on the tracker's stream, one detection stream, no hipMemcpy in here.
  // (VO_ONE_STREAM=1, measurements only: every kernel on the caller's stream, so that a kernel trace shows each
  // kernel's duration without the others running beside it)
  void* side = getenv("VO_ONE_STREAM") ? (void*)ctx->stream : nullptr;
  {
    // Tracker and detection streams keep off the first 32 compute units when the pipeline runs one or two sequences with
    // the detector gated: the next frame's pyramid (858 workgroups) reaches the GPU beside the hypothesis kernel's 144,
    // and that kernel then takes 44 us instead of 23 -- its workgroups wait for a place behind the pyramid's -- unless
    // some compute units stay out of the side streams' reach (measured: 32 of the 256 are enough, 16 are not; step period
    // 122 -> 102 us).  With many sequences, or the detector on every frame, the side streams' kernels are the throughput and
    // the mask costs more than it gives (16 sequences: -5 %).  VO_SIDE_CUS="lo-hi" overrides, "all" switches it off.
    // VO_STREAM_PRIORITY applies to the side streams as to vo_create; VO_STREAM_CUS does not.
    const char* sc = getenv("VO_SIDE_CUS");
    p->side_cfg = vo_stream_cfg_parse(sc, getenv("VO_STREAM_PRIORITY"));
    if (!sc && p->S <= 2 && p->detect_limit >= 0.0 && !side && cfg->tracker_mode == 0) {   // (KLT mode only)
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount >= 128) {
        p->side_cfg.cu_lo = 32;
        p->side_cfg.cu_hi = prop.multiProcessorCount - 1;
      }
    }
    if (!side && side_pool_evicts()) side_evict_except(ctx->device, p->side_cfg);
    for (vo_ctx** c : {&p->trk, &p->det})
      if ((side ? vo_create_stream(ctx->device, side, p->side_cfg, c) : side_take(ctx->device, p->side_cfg, c)) != VO_OK)
        rc = vo_set_error(ctx, VO_EHIP, "pipeline: cannot create the side streams");
  }
  dbg_stage("create: side streams made");
  const int N = cfg->n_keypoints, Hyp = cfg->hyp;
  const size_t px = (size_t)cfg->H * cfg->W, Sz = (size_t)S;
  p->px = px;
  p->n_levels = vo_klt_num_levels(cfg->H, cfg->W, cfg->klt_win, cfg->klt_max_level);
  p->pyr_bytes = vo_pyramid_bytes(cfg->H, cfg->W, p->n_levels);
#define PA(expr) do { if (rc == VO_OK) rc = (expr); } while (0)
  PA(dev_alloc(p, &p->d_img, Sz * cfg->n_frames * px));
  PA(dev_alloc(p, &p->d_pyr, Sz * 3 * p->pyr_bytes));
  PA(dev_alloc(p, &p->d_kp, Sz * 3 * N * 2));
  PA(dev_alloc(p, &p->d_scores[0], Sz * px));
  PA(dev_alloc(p, &p->d_scores[1], Sz * px));
  PA(dev_alloc(p, &p->d_det_go, 3 * Sz));
  if (cfg->detector == 1) {
    PA(dev_alloc(p, &p->d_st_xy, Sz * N * 2));
    PA(dev_alloc(p, &p->d_st_n, 2 * Sz));
    PA(dev_alloc(p, &p->d_det_cnt, 3 * Sz));
  }
  {
    const size_t fb = feat_bytes(cap, S, cfg->track_ids != 0);
    char* mem = nullptr;
    PA(dev_alloc(p, &mem, 2 * fb));
    p->feat_mem = mem;
    p->feat_block = fb;
    if (mem) {
      char* q = mem;
      p->F[0] = carve(q, cap, S, cfg->track_ids != 0);
      p->F[1] = carve(q, cap, S, cfg->track_ids != 0);
    }
  }
  PA(dev_alloc(p, &p->d_ctl, Sz));
  PA(dev_alloc(p, &p->d_cams, Sz));
  PA(dev_alloc(p, &p->d_next, Sz * cap * 2));
  PA(dev_alloc(p, &p->d_err, Sz * cap));
  PA(dev_alloc(p, &p->d_status, Sz * cap));
  PA(dev_alloc(p, &p->d_R, Sz * Hyp * 9));
  PA(dev_alloc(p, &p->d_t, Sz * Hyp * 3));
  PA(dev_alloc(p, &p->d_valid, Sz * Hyp));
  PA(dev_alloc(p, &p->d_counts, Sz * Hyp));
  PA(dev_alloc(p, &p->d_samples, (size_t)Hyp * 4));
  PA(dev_alloc(p, &p->d_masks, Sz * Hyp * p->words));
  PA(dev_alloc(p, &p->d_best_mask, Sz * p->words));
  PA(dev_alloc(p, &p->d_pend, Sz * cap));
  PA(dev_alloc(p, &p->d_newkp, (size_t)cap * 2));
  PA(dev_alloc(p, &p->d_pairs, (size_t)cap * 2 * (cfg->tracker_mode != 0 ? Sz : 1)));
  if (cfg->tracker_mode != 0) {
    p->desc_row = cfg->tracker_mode == 2 ? 384 : cfg->tracker_mode == 3 ? 32 : 128;
    p->sift_all = cfg->tracker_mode == 1 && cfg->sift_cap == -1;
    p->frame_rows = cfg->tracker_mode >= 2 ? cfg->n_keypoints
                  : p->sift_all          ? cap
                                         : (cfg->sift_cap > 0 ? cfg->sift_cap : cfg->n_keypoints);
    if (rc == VO_OK && !p->sift_all && (p->frame_rows > cap || p->frame_rows > 4000))
      rc = vo_set_error(ctx, VO_EINVAL, "pipeline: sift_cap %d exceeds the feature capacity %d (or 4000)", p->frame_rows, cap);
    PA(dev_alloc(p, &p->d_skp, (size_t)3 * p->frame_rows * 6));
    if (p->sift_all) PA(dev_alloc(p, &p->d_sover, (size_t)3 * 2));
    PA(dev_alloc(p, &p->d_frame_desc, 3 * Sz * p->frame_rows * p->desc_row));
    PA(dev_alloc(p, &p->d_frame_n, 4 * Sz + 4));
    PA(dev_alloc(p, &p->d_fdesc, 2 * Sz * cap * p->desc_row));
    PA(dev_alloc(p, &p->d_srcrow, Sz * cap));
    if (rc == VO_OK && (hipMemset(p->d_frame_n, 0, (4 * Sz + 4) * 4) != hipSuccess ||
                        hipMemset(p->d_fdesc, 0, 2 * Sz * cap * p->desc_row) != hipSuccess))
      rc = vo_set_error(ctx, VO_EHIP, "pipeline: hipMemset failed");
    if (rc == VO_OK && cfg->tracker_mode == 2) {          // (every frame has exactly N detector keypoints)
      const std::vector<int32_t> nn(3 * Sz, cfg->n_keypoints);
      if (hipMemcpy(p->d_frame_n, nn.data(), nn.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        rc = vo_set_error(ctx, VO_EHIP, "pipeline: hipMemcpy failed");
    }
  }
  // n_iterations as a step function of the outlier ratio (state_device.h, table_lookup): a batch of `hyp`
  // samples cannot finish a rule that needs more than `hyp` iterations, so hyp + 1 thresholds suffice
  // -- unless the loop continues over several launches (VO_FAULT_CONTINUE): then the table holds the whole budget
  //    (every bound up to max_iterations; an unbounded budget: up to 65536, beyond that the host's loop takes over)
  {
    const int64_t mi = cfg->ransac_max_iterations;
    const int64_t want = mi >= 0 ? std::min<int64_t>(mi, 65536) : 65536;
    p->table_len = (int)std::max<int64_t>(Hyp + 1, want + 1);
  }
  p->table.assign((size_t)p->table_len + 1, 0.0);
  vo_ransac_build_table(cfg->ransac_confidence, 4, p->table_len, p->table.data());
  PA(dev_alloc(p, &p->d_table, p->table.size()));
  const size_t need = (size_t)7 * Hyp;
  p->ring_len = next_pow2(32 * need);
  p->stage_cap = 16 * need;
  PA(dev_alloc(p, &p->d_raws, Sz * p->ring_len));
  PA(pin_alloc(p, &p->h_stage, p->stage_cap));
  PA(pin_alloc(p, &p->h_res, 4 * Sz));
  {
    unsigned* q = nullptr;
    PA(pin_alloc(p, &q, 4 * Sz + 16));
    if (q) memset(q, 0, (4 * Sz + 16) * sizeof(unsigned));
    p->h_seq = q;
  }
  dbg_stage("create: allocations made");
  if (rc == VO_OK && (hipHostGetDevicePointer((void**)&p->m_res, (void*)p->h_res, 0) != hipSuccess ||
                      hipHostGetDevicePointer((void**)&p->m_seq, (void*)p->h_seq, 0) != hipSuccess))
    rc = vo_set_error(ctx, VO_EHIP, "hipHostGetDevicePointer failed");
#undef PA
  if (rc == VO_OK) {
    hipEvent_t* evs[] = {&p->evPyr[0], &p->evPyr[1], &p->evPyr[2], &p->evDet[0], &p->evDet[1], &p->evDet[2],
                         &p->evRaw, &p->evA, &p->evB, &p->evKlt[0], &p->evKlt[1], &p->evRegroup[0], &p->evRegroup[1]};
    for (hipEvent_t* e : evs)
      if (rc == VO_OK) rc = make_event(p, e);
  }
  dbg_stage("create: events made");
  if (rc == VO_OK && (mcpy(ctx->stream, p->d_table, p->table.data(), p->table.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
                      mset(ctx->stream, p->d_ctl, 0, Sz * sizeof(vo_seq_ctl)) != hipSuccess ||
                      mcpy(ctx->stream, p->d_cams, p->cams.data(), Sz * sizeof(vo_cam), hipMemcpyHostToDevice) != hipSuccess))
    rc = vo_set_error(ctx, VO_EHIP, "pipeline: initial uploads failed");
  if (rc != VO_OK) {
    vo_pipeline_destroy(p);
    return rc;
  }
  dbg_stage("create: uploads made");
  p->h_img.assign(Sz * cfg->n_frames, nullptr);
  p->evImg.assign((size_t)cfg->n_frames, nullptr);
  p->evUp.assign((size_t)cfg->n_frames, nullptr);
  p->pinned.assign(Sz * cfg->n_frames, 0);
  p->plain_used.assign((size_t)cfg->n_frames, 0);
  p->n_pinned.assign((size_t)cfg->n_frames, 0);
  for (auto* v : {&p->evImg, &p->evUp})
    for (hipEvent_t& e : *v)
      if (rc == VO_OK) rc = make_event(p, &e);
  if (rc != VO_OK) {
    vo_pipeline_destroy(p);
    return rc;
  }
  p->gen_upto.assign(Sz, 0);
  p->pos_known.assign(Sz, 0);
  p->pos_dev.assign(Sz, 0);
  p->raw_gen.resize(Sz);
  p->rng.resize(Sz);
  p->slot_seq.assign(4 * Sz, 0u);
  p->seq_state.assign(Sz, 0);
  for (auto& g : p->rng) memset(&g, 0, sizeof(g));
  // First use in a fixed order -- main, tracker, detection: the runtime attaches a stream to a hardware queue when it
  // first runs, and the three streams of the frame loop should end up on three different queues.
  {
    hipStream_t order[3] = {ctx->stream, p->trk->stream, p->det->stream};
    for (hipStream_t q : order) {
      (void)hipMemsetAsync(p->d_status, 0, 4, q);
      (void)hipStreamSynchronize(q);
      dbg_stage("create: a stream ran");
    }
  }
  if (cfg->detector == 1) {
    // The Shi-Tomasi chain's workspace on the detection context, sized for all S images, before the first step: one pass of
    // the chain itself with every image gated out (no step allocates).  VO_ST_ROUNDS: round launches of the minimum-distance
    // rule per detection (measurements; results do not depend on it, an unfinished image goes to the walk).
    p->st_rounds = VO_GFB_ROUNDS;
    if (const char* e = getenv("VO_ST_ROUNDS")) p->st_rounds = std::min(VO_GFB_ROUNDS, std::max(0, atoi(e)));
    if (mset(p->det->stream, p->d_det_go, 0, 3 * Sz * sizeof(int)) != hipSuccess ||
        mset(p->det->stream, p->d_det_cnt, 0, 3 * Sz * sizeof(int32_t)) != hipSuccess)
      rc = vo_set_error(ctx, VO_EHIP, "pipeline: hipMemset failed");
    if (rc == VO_OK) {
      rc = vo_good_features_batch_gated_dev(p->det, p->img(0, 0), p->img_stride(), S, cfg->H, cfg->W, nullptr, 0, N,
                                            p->cfg.st_quality, p->cfg.st_min_distance, p->cfg.st_block, p->d_st_xy, (size_t)N,
                                            p->d_st_n, p->d_st_n + S, nullptr, p->st_rounds, VO_GFB_CANDIDATES, p->d_det_go);
      if (rc != VO_OK) vo_set_error(ctx, rc, "pipeline: %s", vo_last_error(p->det));
    }
    if (rc == VO_OK && hipStreamSynchronize(p->det->stream) != hipSuccess) rc = vo_set_error(ctx, VO_EHIP, "pipeline: the detection stream failed");
    if (rc != VO_OK) {
      vo_pipeline_destroy(p);
      return rc;
    }
  }
  if (cfg->tracker_mode == 3) {
    // The FAST workspace of the detection context and the matcher's lists and owner tables of the caller's, sized for all S
    // sequences before the first step: one pass of the front on frame slot 0 (whatever it holds) and one of the matcher
    // with every count at zero (no step allocates).  The counts the front left go back to zero.
    rc = vo_fast_keypoints_batch_dev(p->det, p->img(0, 0), p->img_stride(), S, cfg->H, cfg->W, p->fast_threshold, 1, N, p->kp(0, 0),
                                     p->det_stride() / 2, nullptr, p->frame_n(0, 0), nullptr);
    if (rc != VO_OK) vo_set_error(ctx, rc, "pipeline: %s", vo_last_error(p->det));
    if (rc == VO_OK && hipStreamSynchronize(p->det->stream) != hipSuccess) rc = vo_set_error(ctx, VO_EHIP, "pipeline: the detection stream failed");
    if (rc == VO_OK && mset(ctx->stream, p->d_frame_n, 0, (4 * Sz + 4) * 4) != hipSuccess) rc = vo_set_error(ctx, VO_EHIP, "pipeline: hipMemset failed");
    if (rc == VO_OK) {
      rc = vo_match_hamming_batch_dev(ctx, p->fdesc(0, 0), (size_t)cap * p->desc_row, &p->d_ctl->n, (int)(sizeof(vo_seq_ctl) / 4), cap,
                                      p->frame_desc(0, 0), (size_t)p->frame_rows * p->desc_row, p->frame_n(0, 0), 1, p->frame_rows, S,
                                      p->desc_row, 0.8, 64, p->d_pairs, p->npairs(0));
      if (rc != VO_OK) rc = vo_set_error(ctx, rc, "pipeline: the matcher's workspace: %s", std::string(vo_last_error(ctx)).c_str());
    }
    if (rc == VO_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = vo_set_error(ctx, VO_EHIP, "pipeline: the main stream failed");
    if (rc != VO_OK) {
      vo_pipeline_destroy(p);
      return rc;
    }
  }
  if (const char* e = getenv("VO_HOST_THREADS_BUDGET")) p->threads_budget = atoi(e) <= 1 ? 1 : 2;
  if (p->threads_budget == 1) p->spin_s = 0.0;
  if (const char* e = getenv("VO_HOST_SPIN_US")) p->spin_s = 1e-6 * (double)std::max(0, atoi(e));
  if (p->threads_budget >= 2) p->worker = std::thread(worker_main, p);
  *out = p;
  return VO_OK;
}

// The side contexts kept from closed pipelines (side_pool above) are destroyed now.  For a process that goes on WITHOUT a
// pipeline and wants its other queues at full speed (live CU-masked queues slow every queue of the process).
void vo_pipeline_release_cached(void) { side_evict_except(-1, {}); }
int vo_pipeline_release_cached_at_exit(void) { return side_pool_destroy_at_exit() ? 1 : 0; }

int vo_pipeline_feature_cap(vo_pipeline* p) { return p ? p->cap : 0; }
int vo_pipeline_sequences(vo_pipeline* p) { return p ? p->S : 0; }

int64_t vo_pipeline_ransac_bound(vo_pipeline* p, double outlier_ratio) {
  if (!p) return -1;
  return vo_ransac_table_lookup(p->table.data(), p->table_len, p->cfg.ransac_max_iterations, outlier_ratio);
}

// may frame slot idx of sequence seq be filled now?  (who: the entry point, for the error text)
static int check_frame_slot(vo_pipeline* p, const char* who, int seq, int idx, const uint8_t* img) {
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S && idx >= 0 && idx < p->cfg.n_frames && img, "%s: bad arguments", who);
  for (int k = 0; k < p->n_flight; ++k)
    VO_REQUIRE(ctx, p->flight[k].prev_idx != idx && p->flight[k].next_idx != idx, "%s: slot %d belongs to a step in flight", who,
               idx);
  // the frame submitted last is what the next step tracks FROM (and what a skipped detection is made up from) -- except
  // for an idle lane, whose frame there is the first of the recording vo_pipeline_restart_seq hands it next
  VO_REQUIRE(ctx, !(p->have_state && p->primed && idx == p->prev_frame && !p->idle[seq]),
             "%s: slot %d holds the frame the next step starts from", who, idx);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return VO_OK;
}

// One frame into slot idx of sequence seq: `channels` = 1 (grey) or 3 (B, G, R) [ref: the cvtColor call sites,
// src/vo/features/klt.py:58-62, harris.py:41-48], from the caller's pageable (plain) or pinned buffer.
//   plain:  through a pinned staging buffer -- of this (sequence, slot) for a grey image, one of its own for a
//           three-channel one --, as one DMA queued on the tracker's stream, in front of the pyramid that reads the slot;
//           the detector's stream waits for evImg.  The call does not wait for the GPU (the runtime's pageable-memory path
//           did, and drained the tracker's stream on top: 0.9 ms per frame through the Python API); the caller's buffer is
//           free on return.
//   pinned: no staging copy, and the DMA runs on a stream of its own.  The buffer must stay as it is until the upload is
//           over: vo_pipeline_frame_uploaded(idx), or the collect of a step that read the slot.
// A grey image of a lane without distortion coefficients is copied straight into the slot.  Anything else lands in the
// stream's raw buffer and the ingest kernel (ingest.hip) writes the slot behind it on the same stream; the slot's event
// is recorded behind the kernel, so whoever waits for the upload waits for the ingest.
static int upload_frame(vo_pipeline* p, const char* who, int seq, int idx, const uint8_t* src, int channels, bool from_pinned) {
  vo_ctx* ctx = p->ctx;
  VO_TRY(check_frame_slot(p, who, seq, idx, src));
  const size_t at = (size_t)seq * p->cfg.n_frames + idx, bytes = (size_t)channels * p->px;
  vo_undist und;
  const bool lens = !p->lens.empty() && p->lens[(size_t)seq].on;
  if (lens) {
    const vo_pipeline::lens_t& L = p->lens[(size_t)seq];
    VO_TRY(vo_undist_make(ctx, who, p->cams[(size_t)seq].K, L.dist, L.have_raw ? L.K_raw : nullptr, &und));
  }
  const bool direct = channels == 1 && !lens;
  if (from_pinned && !p->up_stream) VO_HIP_TRY(ctx, hipStreamCreateWithFlags(&p->up_stream, hipStreamNonBlocking));
  hipStream_t st = from_pinned ? p->up_stream : p->trk->stream;
  uint8_t* raw = nullptr;
  if (!direct) {
    uint8_t*& buf = p->d_raw[from_pinned ? 1 : 0];
    if (!buf) VO_TRY(dev_alloc(p, &buf, 3 * p->px + 4));
    // (the grey kernel's dword loads: ingest.hip, vo_ingest_head)
    raw = buf + (channels == 3 && !lens ? vo_ingest_head(p->img(seq, idx)) : 0);
  }
  if (!from_pinned) {
    if (channels == 1) {
      uint8_t*& stage = p->h_img[at];
      if (!stage) VO_TRY(pin_alloc(p, &stage, p->px, hipHostMallocDefault));
      VO_HIP_TRY(ctx, hipEventSynchronize(p->evImg[idx]));     // (the slot's previous upload has left the staging buffer)
      memcpy(stage, src, bytes);
      src = stage;
    } else {
      if (!p->h_bgr) VO_TRY(pin_alloc(p, &p->h_bgr, bytes, hipHostMallocDefault));
      if (!p->evBgr) VO_TRY(make_event(p, &p->evBgr));
      VO_HIP_TRY(ctx, hipEventSynchronize(p->evBgr));          // (its previous DMA has read it)
      memcpy(p->h_bgr, src, bytes);
      src = p->h_bgr;
    }
  }
  char& pin = p->pinned[at];
  if (from_pinned) {
    // (a slot the tracker's stream filled last: that copy is in front of everything that read the slot; a step that read it
    //  has been collected -- the check above --, so nothing on the GPU still reads what this upload overwrites)
    if (!pin && p->plain_used[idx]) VO_HIP_TRY(ctx, hipStreamWaitEvent(st, p->evImg[idx], 0));   // (an upload the plain call queued)
  } else if (pin) {
    VO_HIP_TRY(ctx, hipStreamWaitEvent(st, p->evUp[idx], 0));                                    // (this one lands after the pinned one)
  }
  VO_HIP_TRY(ctx, hipMemcpyAsync(direct ? p->img(seq, idx) : raw, src, bytes, hipMemcpyHostToDevice, st));
  if (!from_pinned && channels == 3) VO_HIP_TRY(ctx, hipEventRecord(p->evBgr, st));
  int rc = VO_OK;
  if (!direct) rc = vo_ingest_dev(ctx, st, raw, channels, p->cfg.H, p->cfg.W, lens ? &und : nullptr, p->img(seq, idx));
  // (recorded even when the launch was refused: the copy above is queued, and the events must cover it)
  VO_HIP_TRY(ctx, hipEventRecord(from_pinned ? p->evUp[idx] : p->evImg[idx], st));
  if (from_pinned && !pin) {
    pin = 1;
    ++p->n_pinned[idx];
  } else if (!from_pinned) {
    if (pin) {
      pin = 0;
      --p->n_pinned[idx];
    }
    p->plain_used[idx] = 1;
  }
  if (p->prepared_idx == idx) p->prepared_idx = p->prepared_slot = -1;
  return rc;
}

int vo_pipeline_set_frame_seq(vo_pipeline* p, int seq, int idx, const uint8_t* img) {
  return p ? upload_frame(p, "pipeline_set_frame", seq, idx, img, 1, false) : VO_EINVAL;
}

int vo_pipeline_set_frame_pinned(vo_pipeline* p, int seq, int idx, const uint8_t* pinned_img) {
  return p ? upload_frame(p, "pipeline_set_frame_pinned", seq, idx, pinned_img, 1, true) : VO_EINVAL;
}

int vo_pipeline_set_frame_bgr_seq(vo_pipeline* p, int seq, int idx, const uint8_t* bgr) {
  return p ? upload_frame(p, "pipeline_set_frame_bgr", seq, idx, bgr, 3, false) : VO_EINVAL;
}

int vo_pipeline_set_frame_bgr_pinned(vo_pipeline* p, int seq, int idx, const uint8_t* bgr_pinned) {
  return p ? upload_frame(p, "pipeline_set_frame_bgr_pinned", seq, idx, bgr_pinned, 3, true) : VO_EINVAL;
}

// Lane seq's lens from now on [ref: src/vo/sensors/camera.py:38-54: Camera takes distortion coefficients, and its two
// methods are stubs]: frames uploaded after the call are undistorted into the lane's pinhole camera K (the camera at the
// time of each upload when K_raw is NULL).  Slots already filled keep their contents.
int vo_pipeline_set_distortion_seq(vo_pipeline* p, int seq, const double* dist, const double* K_raw) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S, "pipeline_set_distortion: bad sequence index");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_set_distortion: %d submitted step(s) not collected", p->n_flight);
  vo_undist und;      // (the checks alone)
  VO_TRY(vo_undist_make(ctx, "pipeline_set_distortion", p->cams[(size_t)seq].K, dist, K_raw, &und));
  bool any = false;
  for (int i = 0; dist && i < 5; ++i) any |= dist[i] != 0.0;
  vo_pipeline::lens_t L;
  L.on = any || K_raw;
  if (L.on && dist) memcpy(L.dist, dist, sizeof(L.dist));
  if (L.on && K_raw) {
    L.have_raw = true;
    memcpy(L.K_raw, K_raw, sizeof(L.K_raw));
  }
  if (p->lens.empty()) {
    if (!L.on) return VO_OK;
    p->lens.assign((size_t)p->S, vo_pipeline::lens_t());
  }
  p->lens[(size_t)seq] = L;
  return VO_OK;
}

// what slot idx of sequence seq holds (H * W bytes), i.e. the frame as the tracker and the detector read it
int vo_pipeline_get_frame_seq(vo_pipeline* p, int seq, int idx, uint8_t* out) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, seq >= 0 && seq < p->S && idx >= 0 && idx < p->cfg.n_frames && out, "pipeline_get_frame: bad arguments");
  VO_REQUIRE(ctx, p->n_flight == 0, "pipeline_get_frame: %d submitted step(s) not collected", p->n_flight);
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  VO_HIP_TRY(ctx, hipEventSynchronize(p->evImg[idx]));
  VO_HIP_TRY(ctx, hipEventSynchronize(p->evUp[idx]));
  VO_HIP_TRY(ctx, mcpy(ctx->stream, out, p->img(seq, idx), p->px, hipMemcpyDeviceToHost));
  return VO_OK;
}

int vo_pipeline_frame_uploaded(vo_pipeline* p, int idx, int wait) {
  if (!p) return VO_EINVAL;
  vo_ctx* ctx = p->ctx;
  VO_REQUIRE(ctx, idx >= 0 && idx < p->cfg.n_frames, "pipeline_frame_uploaded: bad slot");
  if (wait) {
    VO_HIP_TRY(ctx, hipEventSynchronize(p->evUp[idx]));
    VO_HIP_TRY(ctx, hipEventSynchronize(p->evImg[idx]));
    return 1;
  }
  return hipEventQuery(p->evUp[idx]) == hipSuccess && hipEventQuery(p->evImg[idx]) == hipSuccess ? 1 : 0;
}

int vo_host_alloc(vo_ctx* ctx, size_t bytes, void** out) {
  if (!ctx) return VO_EINVAL;
  VO_REQUIRE(ctx, out && bytes > 0, "host_alloc: bad arguments");
  VO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    *out = nullptr;
    return vo_set_error(ctx, VO_ENOMEM, "hipHostMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
  }
  return VO_OK;
}

int vo_host_free(vo_ctx* ctx, void* q) {      // (ctx may be null: a buffer can outlive the context it was made with)
  if (q && hipHostFree(q) != hipSuccess) return ctx ? vo_set_error(ctx, VO_EHIP, "hipHostFree failed") : VO_EHIP;
  return VO_OK;
}

int vo_pipeline_set_frame(vo_pipeline* p, int idx, const uint8_t* img) { return vo_pipeline_set_frame_seq(p, 0, idx, img); }

// per-kernel event times accumulated over all of the pipeline's streams
int vo_pipeline_prof_read(vo_pipeline* p, int kernel_id, double* total_ms, int64_t* launches) {
  if (!p) return VO_EINVAL;
  VO_TRY(worker_idle(p));
  double sum = 0;
  int64_t n = 0;
  for (vo_ctx* q : {p->ctx, p->det, p->trk}) {
    double ms = 0;
    int64_t k = 0;
    const int rc = vo_prof_read(q, kernel_id, &ms, &k);
    if (rc != VO_OK) return q == p->ctx ? rc : vo_set_error(p->ctx, rc, "%s", vo_last_error(q));
    sum += ms;
    n += k;
  }
  if (total_ms) *total_ms = sum;
  if (launches) *launches = n;
  return VO_OK;
}

int vo_pipeline_prof_reset(vo_pipeline* p) {
  if (!p) return VO_EINVAL;
  VO_TRY(worker_idle(p));
  for (vo_ctx* q : {p->ctx, p->det, p->trk}) VO_TRY(vo_prof_reset(q));
  return VO_OK;
}

}  // extern "C"
