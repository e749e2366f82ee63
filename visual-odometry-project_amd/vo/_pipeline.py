"""Device-resident frame loop (vo_pipeline_*, include/vo_hip.h): the steady state of the reference
driver (src/main.py:248-286, KLT tracker mode) with the Features / State / RANSAC bookkeeping kept in
HBM.  The pipeline takes images only; `set_state` hands over what the bootstrap produced and
`get_state` returns the reference's Features arrays of the current frame.  With `sequences=S` the pipeline
advances S independent streams per launch (`seq=` addresses one of them, `collect_all` returns all records)."""
import ctypes as C

import numpy as np


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _as_4x4(pose):
    pose = np.asarray(pose, np.float64)
    if pose.shape == (3, 4):
        pose = np.vstack([pose, [0.0, 0.0, 0.0, 1.0]])
    return np.ascontiguousarray(pose)


DETECTORS = {"harris": 0, "shi-tomasi": 1}       # vo_pipeline_config.detector

# one row of the observation record (vo_pipeline_export_tracks_post_seq): 48 bytes
TRACK_ROW = np.dtype([("id", "<i4"), ("born", "<i4"), ("x", "<f4"), ("y", "<f4"), ("state", "<i4"), ("candidate", "<i4"),
                      ("X", "<f8"), ("Y", "<f8"), ("Z", "<f8")])
TRACK_HEADER = np.dtype([("n", "<i4"), ("step", "<i4"), ("next_id", "<i4"), ("seq", "<i4")])


class TrackRecord(np.ndarray):
    """The rows of one observation record (dtype TRACK_ROW) with the header's words as attributes: n (the step's feature
    count; len() is min(n, cap)), step (the sequence's step counter after the step), next_id, seq."""
    n = step = next_id = seq = 0

    def __array_finalize__(self, obj):
        for k in ("n", "step", "next_id", "seq"):
            setattr(self, k, getattr(obj, k, 0))

    @classmethod
    def from_bytes(cls, raw, cap):
        raw = np.ascontiguousarray(raw, np.uint8)
        head = raw[:16].view(TRACK_HEADER)[0]
        m = max(0, min(int(head["n"]), int(cap)))
        rec = raw[16:16 + 48 * m].view(TRACK_ROW).copy().view(cls)
        rec.n, rec.step, rec.next_id, rec.seq = (int(head[k]) for k in ("n", "step", "next_id", "seq"))
        return rec


class Pipeline:
    def __init__(self, ctx, H, W, n_frames, K, n_keypoints=2000, harris_patch=9, harris_kappa=0.09, nms_radius=5,
                 klt_win=15, klt_max_level=2, klt_max_iter=10, klt_eps=0.03, klt_min_eig=1e-4,
                 klt_err_threshold=100.0, hyp=1000, p3p_threshold=1.0, outlier_ratio=0.9, confidence=0.99,
                 max_iterations=1000, seed=2023, refine_iters=0, feature_cap=0, bearing_threshold=0.0075,
                 redetect_fraction=0.8, debug_fault_every=0, redetect_start_pose="identity", sequences=1,
                 detect_margin=0.01, debug_never_detect=0, detect_losses=2.5, tracker="klt", sift_cap=0, match_ratio=0.0,
                 detector="harris", st_quality=0.0, st_min_distance=0.0, st_block=0, track_ids=False,
                 fast_threshold=0, brief_oriented=False, brief_max_distance=0):
        from vo import _native
        self.ctx = ctx
        self.cfg = _native.PipelineConfig()
        c = self.cfg
        c.H, c.W, c.n_frames = H, W, n_frames
        c.n_keypoints, c.harris_patch, c.nms_radius, c.harris_kappa = n_keypoints, harris_patch, nms_radius, harris_kappa
        c.klt_win, c.klt_max_level, c.klt_max_iter, c.hyp = klt_win, klt_max_level, klt_max_iter, hyp
        c.klt_eps, c.klt_min_eig, c.klt_err_threshold = klt_eps, klt_min_eig, klt_err_threshold
        c.p3p_thr_sq = p3p_threshold
        c.ransac_outlier_ratio, c.ransac_confidence = outlier_ratio, confidence
        c.ransac_max_iterations = -1 if max_iterations is None or max_iterations == np.inf else int(max_iterations)
        c.refine_iters = int(refine_iters)
        c.feature_cap = int(feature_cap)
        c.bearing_threshold = float(bearing_threshold)
        c.redetect_fraction = float(redetect_fraction)
        c.debug_fault_every = int(debug_fault_every)
        c.redetect_start_pose = {"identity": 0, "current": 1}[redetect_start_pose]
        c.sequences = int(sequences)
        c.detect_margin = float(detect_margin)       # < 0: the detector runs on every frame
        c.debug_never_detect = int(debug_never_detect)
        c.detect_losses = float(detect_losses)
        # src/vo/features/tracker.py:54-63; "fast": the project's FAST-9 + BRIEF-256 front end (vo/features/fast.py)
        c.tracker_mode = {"klt": 0, "sift": 1, "harris": 2, "fast": 3}[tracker]
        c.sift_cap = int(sift_cap)   # SIFT mode: -1 every keypoint (<= feature_cap), 0 n_keypoints, 1..4000 the strongest
        c.match_ratio = float(match_ratio)
        # KLT mode's re-detect: "harris" (response + NMS, exactly n_keypoints) or "shi-tomasi" (the reference's
        # cv2.goodFeaturesToTrack with maxCorners = n_keypoints; st_* left at 0: klt.py:24-26's 0.01 / 8 / 7)
        c.detector = DETECTORS[detector]
        c.st_quality, c.st_min_distance, c.st_block = float(st_quality), float(st_min_distance), int(st_block)
        c.track_ids = 1 if track_ids else 0          # persistent track ids (vo_hip.h, "Track ids")
        self.track_ids = bool(track_ids)
        self.detector = detector
        self.tracker = tracker
        self.sequences = int(sequences)
        K = np.asarray(K, np.float64).reshape(3, 3)
        self.K = K
        for i, v in enumerate(K.reshape(9)):
            c.K[i] = v
        # the reference normalises keypoints with np.linalg.inv(K) (src/vo/sensors/camera.py:88)
        for i, v in enumerate(np.linalg.inv(K).reshape(9)):
            c.Kinv[i] = v
        h = C.c_void_p()
        ctx._chk(ctx._lib.vo_pipeline_create(ctx._h, C.byref(c), C.byref(h)))
        self._h = h
        self._pinned_src = {}
        ctx._pipelines.add(self)
        self.cap = ctx._lib.vo_pipeline_feature_cap(self._h)
        if tracker == "fast":
            # FASTBRIEFDetector's settings (0 / False / 0: its defaults -- threshold 20, not oriented, distance limit 64;
            # brief_max_distance < 0: no limit); ignored in the other modes.  A refused value closes the pipeline again.
            try:
                ctx._chk(ctx._lib.vo_pipeline_set_fast_brief(self._h, int(fast_threshold), 1 if brief_oriented else 0,
                                                             int(brief_max_distance)))
            except Exception:
                self.close()
                raise
        self.seed(np.random.default_rng(seed))

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_loop", None):
                self._loop.close()
            self.ctx._lib.vo_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs ----
    def set_frame(self, idx, img, seq=0, pinned=None):
        """Frame slot idx <- img: (H, W) grey or (H, W, 3) B, G, R, uint8.  The slot receives the grey image, undistorted
        when the lane has coefficients (set_distortion): a three-channel or distorted frame is converted by the ingest
        kernel behind its DMA.  pinned: img lies in Context.pinned_empty memory and is uploaded from there (no staging
        copy, DMA beside the kernels; img must stay unchanged until frame_uploaded(idx) or the collect of a step that
        read the slot); None: decided by where img lies."""
        img = _c(img, np.uint8)
        assert img.shape in ((self.cfg.H, self.cfg.W), (self.cfg.H, self.cfg.W, 3))
        lib = self.ctx._lib
        if pinned is None:
            pinned = self.ctx.is_pinned(img)
        if pinned:
            self._pinned_src[(int(seq), int(idx))] = img          # (kept alive while the DMA may read it)
            fn = lib.vo_pipeline_set_frame_pinned if img.ndim == 2 else lib.vo_pipeline_set_frame_bgr_pinned
        else:
            fn = lib.vo_pipeline_set_frame_seq if img.ndim == 2 else lib.vo_pipeline_set_frame_bgr_seq
        self.ctx._chk(fn(self._h, int(seq), int(idx), _ptr(img)))

    def set_distortion(self, seq, dist, K_raw=None):
        """Lane `seq`'s lens (vo_pipeline_set_distortion_seq; nothing in flight): dist = (k1, k2, p1, p2[, k3]) or None,
        K_raw the intrinsics of the distorted image (None: the lane's K).  Frames uploaded afterwards are undistorted
        into the lane's pinhole camera; None / all zero without K_raw switches it off."""
        from vo import _native
        d = None if dist is None else _native.distortion_coefficients(dist)
        Kr = None if K_raw is None else _c(np.asarray(K_raw, np.float64).reshape(3, 3), np.float64)
        self.ctx._chk(self.ctx._lib.vo_pipeline_set_distortion_seq(self._h, int(seq), _ptr(d), _ptr(Kr)))

    def get_frame(self, idx, seq=0):
        """What frame slot idx of lane `seq` holds, (H, W) uint8 (nothing in flight)."""
        out = np.empty((self.cfg.H, self.cfg.W), np.uint8)
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_frame_seq(self._h, int(seq), int(idx), _ptr(out)))
        return out

    def prepare(self, idx):
        """Hint: frame slot idx is the `next` of the coming submit -- its pyramid is built now, off that step's critical
        path (vo_pipeline_prepare).  Results do not depend on it."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_prepare(self._h, int(idx)))

    def set_klt_fb(self, fb_max):
        """The tracker's forward-backward check from the next step on (vo_pipeline_set_klt_fb): fb_max > 0 pixels
        (+inf allowed) switches it on, 0 off -- the state at creation.  KLT tracker mode, nothing in flight."""
        fb_max = float(fb_max)
        if not fb_max >= 0.0:
            raise ValueError("set_klt_fb: fb_max must be > 0 pixels (+inf allowed), or 0 for off; got %r" % (fb_max,))
        self.ctx._chk(self.ctx._lib.vo_pipeline_set_klt_fb(self._h, fb_max))

    @property
    def klt_fb(self):
        """The forward-backward threshold in pixels (0.0: the check is off)."""
        v = C.c_double(0.0)
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_klt_fb(self._h, C.byref(v)))
        return float(v.value)

    def frame_uploaded(self, idx, wait=False):
        rc = self.ctx._lib.vo_pipeline_frame_uploaded(self._h, int(idx), 1 if wait else 0)
        if rc < 0:
            self.ctx._chk(rc)
        return bool(rc)

    def seed(self, generator):
        """The estimator's generator (RANSAC.rng, src/vo/algorithms/ransac.py:52)."""
        from vo import _native
        pcg = _native.Pcg64.from_generator(generator)
        self.ctx._chk(self.ctx._lib.vo_pipeline_seed(self._h, C.byref(pcg)))

    def rng_state_into(self, generator, seq=0):
        """Writes the estimator generator's state after the last collected step into `generator`."""
        from vo import _native
        pcg = _native.Pcg64()
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_rng_seq(self._h, int(seq), C.byref(pcg)))
        pcg.to_generator(generator)

    def _state_args(self, features, curr_pose, prev_pose, num_features):
        n = features.length
        kp = _c(np.asarray(features.keypoints).reshape(n, 2), np.float64)
        state = _c(np.asarray(features.state).reshape(n), np.uint8)
        land = _c(np.asarray(features.landmarks).reshape(n, 3), np.float64)
        tracks = _c(np.asarray(features.tracks).reshape(n, 2), np.float64)
        poses = _c(np.asarray(features.poses).reshape(n, 16), np.float64)
        T_wc = _as_4x4(curr_pose)
        T_wc_prev = _as_4x4(prev_pose if prev_pose is not None else curr_pose)
        T_cw, T_cw_prev = _c(np.linalg.inv(T_wc), np.float64), _c(np.linalg.inv(T_wc_prev), np.float64)
        nf = int(num_features if num_features is not None else self.cfg.n_keypoints)
        keep = (kp, state, land, tracks, poses, T_wc, T_cw, T_wc_prev, T_cw_prev)     # (alive during the call)
        return keep, [n] + [_ptr(a) for a in keep] + [nf]

    def set_state(self, idx, features, curr_pose, prev_pose=None, num_features=None, seq=0):
        """Hands over `features` (a vo.primitives.Features: the current frame's, e.g. after the bootstrap) and
        State's poses (4x4 camera-to-world) for frame slot `idx`.  In the descriptor tracker modes ("sift", "harris",
        "fast") features.descriptors goes with them: n rows of 128, 361 or (fast: BRIEF-256 bytes) 32 whole numbers 0..255."""
        n = features.length
        desc = None
        if self.tracker in ("sift", "harris", "fast"):       # ("fast": n x 32 BRIEF-256 bytes)
            desc = np.asarray(features.descriptors)
            if desc.size != n * self._desc_len():            # (before anything is handed over)
                raise ValueError("set_state: %d descriptor values for %d features of %d each (tracker %r)"
                                 % (desc.size, n, self._desc_len(), self.tracker))
            desc = _c(desc.reshape(n, self._desc_len()), np.float32)
        keep, args = self._state_args(features, curr_pose, prev_pose, num_features)
        self.ctx._chk(self.ctx._lib.vo_pipeline_set_state_seq(self._h, int(seq), int(idx), *args))
        if desc is not None:
            self.ctx._chk(self.ctx._lib.vo_pipeline_set_descriptors_seq(self._h, int(seq), _ptr(desc), n))

    def _desc_len(self):
        return {"sift": 128, "fast": 32}.get(self.tracker, 361)

    # ---- lanes: many recordings through one pipeline ----
    def set_camera(self, K, seq, Kinv=None):
        """Lane `seq`'s intrinsics (vo_pipeline_set_camera_seq; nothing in flight).  Kinv: the inverse as the caller
        forms it; None = np.linalg.inv(K), as the constructor does (src/vo/sensors/camera.py:88)."""
        K = _c(np.asarray(K, np.float64).reshape(3, 3), np.float64)
        Ki = _c(np.linalg.inv(K) if Kinv is None else np.asarray(Kinv, np.float64).reshape(3, 3), np.float64)
        self.ctx._chk(self.ctx._lib.vo_pipeline_set_camera_seq(self._h, int(seq), _ptr(K), _ptr(Ki)))

    def set_active(self, seq, flag):
        """flag False: lane `seq` goes idle -- no kernel works on it, it draws nothing, its records are marked
        (StepResult.idle).  An idle lane becomes active again only through restart().  Nothing in flight."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_set_active_seq(self._h, int(seq), 1 if flag else 0))

    def restart(self, seq, idx, features, curr_pose, prev_pose=None, num_features=None, generator=None, image=None):
        """A new recording for lane `seq` alone (vo_pipeline_restart_seq; nothing in flight): its bootstrap's Features
        and poses for frame slot `idx` (the `prev` of the next submit), a fresh RANSAC object and `generator`'s state
        (None: the state the pipeline was seeded with).  image: the recording's frame for that slot; given, the lane is
        set idle and the frame uploaded first (a lane's frame in that slot can only be replaced while it is idle)."""
        from vo import _native
        if image is not None:
            self.set_active(seq, False)
            self.set_frame(idx, image, seq=seq, pinned=False)
        keep, args = self._state_args(features, curr_pose, prev_pose, num_features)
        pcg = None if generator is None else _native.Pcg64.from_generator(generator)
        self.ctx._chk(self.ctx._lib.vo_pipeline_restart_seq(self._h, int(seq), int(idx), *args,
                                                            C.byref(pcg) if pcg is not None else None))

    def bootstrap(self, idx_a, idx_b, seq=0, generator=None, max_corners=0, quality=0.0, min_distance=0.0, block=0,
                  klt_win=0, klt_max_level=None, threshold_px=0.0, outlier_ratio=0.0, confidence=0.0, max_iterations=0):
        """The two-view bootstrap of lane `seq` from frame slots idx_a, idx_b of its frame store, inside the pipeline
        (vo_pipeline_bootstrap_seq; nothing in flight): what vo.driver.bootstrap + set_state (a pipeline that is not running
        yet) or restart (a running one; generator: the lane's P3P generator, None = the state the pipeline was seeded
        with) do, without an array leaving HBM.  Parameters left at 0 / None take vo_bootstrap_params' defaults.  Returns a
        BootstrapResult; a failure (too few corners / survivors, no model) raises VoError and leaves the lane as it was."""
        from vo import _native
        prm = _native.BootstrapParams(int(max_corners), float(quality), float(min_distance), int(block), int(klt_win),
                                      -1 if klt_max_level is None else int(klt_max_level), float(threshold_px),
                                      float(outlier_ratio), float(confidence), int(max_iterations), 0)
        pcg = None if generator is None else _native.Pcg64.from_generator(generator)
        res = _native.BootstrapResult()
        self.ctx._chk(self.ctx._lib.vo_pipeline_bootstrap_seq(self._h, int(seq), int(idx_a), int(idx_b), C.byref(prm),
                                                              C.byref(pcg) if pcg is not None else None, C.byref(res)))
        return res

    def bootstrap_lanes(self, idx_a, idx_b, seqs, generators=None, max_corners=0, quality=0.0, min_distance=0.0, block=0,
                        klt_win=0, klt_max_level=None, threshold_px=0.0, outlier_ratio=0.0, confidence=0.0, max_iterations=0):
        """The two-view bootstrap of the lanes `seqs` (distinct) through one set of launches (vo_pipeline_bootstrap_lanes):
        every lane ends as bootstrap(idx_a, idx_b, seq=q, generator=generators[i], ...) would leave it.  generators: None or
        one NumPy Generator per lane.  Returns a list of BootstrapResult, one per lane, each with `.seq` and `.status` (0, or
        the VO_E* code of a lane that failed and was left as it was); raises VoError only for a refused call."""
        from vo import _native
        seqs = [int(q) for q in seqs]
        n = len(seqs)
        prm = _native.BootstrapParams(int(max_corners), float(quality), float(min_distance), int(block), int(klt_win),
                                      -1 if klt_max_level is None else int(klt_max_level), float(threshold_px),
                                      float(outlier_ratio), float(confidence), int(max_iterations), 0)
        if generators is not None and len(generators) != n:
            raise ValueError("bootstrap_lanes: %d generators for %d lanes" % (len(generators), n))
        pcgs = None if generators is None else (_native.Pcg64 * n)(*[_native.Pcg64.from_generator(g) for g in generators])
        res = (_native.BootstrapResult * max(n, 1))()
        status = (C.c_int32 * max(n, 1))()
        rc = self.ctx._lib.vo_pipeline_bootstrap_lanes(self._h, n, (C.c_int32 * max(n, 1))(*seqs), int(idx_a), int(idx_b),
                                                       C.byref(prm), pcgs, res, status)
        if rc != 0 and all(status[k] == 0 for k in range(n)):       # refused: no lane was touched
            self.ctx._chk(rc)
        out = []
        for k in range(n):
            r = _native.BootstrapResult.from_buffer_copy(res[k])
            r.seq, r.status = seqs[k], int(status[k])
            out.append(r)
        return out

    def checkpoint(self):
        """Keeps a copy of every sequence's Features / State as they are now (nothing in flight) in HBM."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_checkpoint(self._h))

    def rewind(self):
        """Puts the checkpoint back (asynchronously, nothing in flight): the next submit starts from its frame again.
        The estimator's RANSAC fields and generator go on, as they would on the reference's estimator object."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_rewind(self._h))

    # ---- outputs ----
    def get_state(self, seq=0):
        """dict with the reference's Features arrays of the current frame (shapes as in
        src/vo/primitives/features.py) plus curr_pose / prev_pose / RANSAC fields."""
        from vo import _native
        cap = self.cap
        n = C.c_int32()
        nf = C.c_int32()
        kp = np.empty((cap, 2), np.float64)
        state = np.empty(cap, np.uint8)
        cand = np.empty(cap, np.uint8)
        land = np.empty((cap, 3), np.float64)
        tracks = np.empty((cap, 2), np.float64)
        poses = np.empty((cap, 4, 4), np.float64)
        T, Tp = np.empty((4, 4)), np.empty((4, 4))
        rs = _native.RansacState()
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_state_seq(self._h, int(seq), C.byref(n), _ptr(kp), _ptr(state),
                                                              _ptr(cand), _ptr(land), _ptr(tracks), _ptr(poses),
                                                              _ptr(T), _ptr(Tp), C.byref(rs), C.byref(nf)))
        n = n.value
        return dict(n=n, keypoints=kp[:n].reshape(n, 2, 1).copy(), state=state[:n].astype(np.float64),
                    candidate_mask=cand[:n].astype(bool), landmarks=land[:n].reshape(n, 3, 1).copy(),
                    tracks=tracks[:n].reshape(n, 2, 1).copy(), poses=poses[:n].copy(), curr_pose=T, prev_pose=Tp,
                    n_iterations=int(rs.n_iterations), outlier_ratio=float(rs.outlier_ratio),
                    num_features=nf.value)

    def get_descriptors(self, seq=0):
        """The descriptors the current Features of sequence `seq` carry (descriptor tracker modes; nothing in flight):
        n x 361 (Harris), n x 128 (SIFT) or n x 32 (FAST: the BRIEF-256 bytes) float32, whole numbers, in feature order -- what set_state handed over, regrouped
        with the keypoints since."""
        n = C.c_int32()
        desc = np.empty((self.cap, self._desc_len()), np.float32)
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_descriptors_seq(self._h, int(seq), _ptr(desc), C.byref(n)))
        return desc[:n.value].copy()

    def get_features(self, seq=0):
        """The current frame's features as a vo.primitives.Features object."""
        from vo.primitives import Features
        s = self.get_state(seq)
        f = Features(keypoints=s["keypoints"], landmarks=s["landmarks"])
        f.state, f.tracks, f.poses, f.candidate_mask = s["state"], s["tracks"], s["poses"], s["candidate_mask"]
        if self.track_ids:
            f.uids = self.get_track_ids(seq)[0].astype(np.int64)
        return f

    # ---- track ids ----
    def get_track_ids(self, seq=0):
        """(ids, born, next_id) of sequence `seq`'s current features (track_ids=True; nothing in flight): two int32 arrays
        in feature order -- the track's identity and the step counter's value for the frame it was first seen on -- and the
        next id the sequence will issue."""
        ids, born = np.empty(self.cap, np.int32), np.empty(self.cap, np.int32)
        n, nxt = C.c_int32(), C.c_int32()
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_track_ids_seq(self._h, int(seq), _ptr(ids), _ptr(born), C.byref(n),
                                                                  C.byref(nxt)))
        return ids[:n.value].copy(), born[:n.value].copy(), int(nxt.value)

    def set_track_ids(self, ids, next_id, born=None, seq=0):
        """Replaces the ids of sequence `seq`'s current features (one per feature, distinct, 0 <= id < next_id) and the next
        id it issues; born: None leaves it as it is.  Nothing in flight; a refused call raises VoError and changes nothing."""
        ids = _c(np.asarray(ids).reshape(-1), np.int32)
        b = None if born is None else _c(np.asarray(born).reshape(-1), np.int32)
        if b is not None and b.shape != ids.shape:
            raise ValueError("set_track_ids: %d born values for %d ids" % (b.size, ids.size))
        self.ctx._chk(self.ctx._lib.vo_pipeline_set_track_ids_seq(self._h, int(seq), _ptr(ids), _ptr(b), ids.size,
                                                                  int(next_id)))

    def tracks_record_bytes(self, cap):
        return int(self.ctx._lib.vo_pipeline_tracks_record_bytes(int(cap)))

    def export_tracks_post(self, result, cap, d_record, seq=0):
        """Queues the observation record of the step collected last (`result`: its StepResult) of sequence `seq` on the
        pipeline's stream into device memory d_record (tracks_record_bytes(cap) bytes, 16-byte aligned); no
        synchronisation -- export_state_join orders it against a consumer."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_export_tracks_post_seq(self._h, int(seq), C.byref(result), int(cap),
                                                                       C.c_void_p(d_record)))

    def read_tracks_record(self, d_record, cap):
        """Downloads a record the pipeline's stream has written (a blocking copy on that stream, so behind the kernel that
        writes it) and returns it as a TrackRecord: a structured array of its min(n, cap) rows, the header as attributes."""
        return TrackRecord.from_bytes(self.ctx.download(d_record, (self.tracks_record_bytes(cap),), np.uint8), cap)

    def update_landmarks(self, ids, X, seq=0, n=None):
        """The features of sequence `seq` whose track id is in `ids` and whose state is 2 take the landmark of the same row
        of X; everything else stays (vo_pipeline_update_landmarks_seq; track_ids=True, nothing in flight).  ids / X: host
        arrays ((n,) and (n, 3)), or two device pointers with n given."""
        if n is not None:
            self.ctx._chk(self.ctx._lib.vo_pipeline_update_landmarks_seq(self._h, int(seq), int(n), C.c_void_p(ids),
                                                                         C.c_void_p(X)))
            return
        ids = _c(np.asarray(ids).reshape(-1), np.int32)
        X = _c(np.asarray(X, np.float64).reshape(-1, 3), np.float64)
        if len(X) != ids.size:
            raise ValueError("update_landmarks: %d landmarks for %d ids" % (len(X), ids.size))
        d_ids, d_X = self.ctx.to_device(ids), self.ctx.to_device(X)
        try:
            self.ctx._chk(self.ctx._lib.vo_pipeline_update_landmarks_seq(self._h, int(seq), ids.size, C.c_void_p(d_ids),
                                                                         C.c_void_p(d_X)))
        finally:
            self.ctx.free(d_ids)
            self.ctx.free(d_X)

    def structure_loop(self, window, L_cap=None, M_cap=None, feedback=True, **structure_params):
        """The structure refinement behind every collected step, stream-ordered (vo_hip.h, "Structure loop"; KLT tracker
        mode, track_ids=True, one loop per pipeline): returns a vo.landmarks.StructureLoop -- post(results) after every
        collect, with one further step in flight; reset(seq) at a hand-over; poll / download for what it did."""
        from vo.landmarks import StructureLoop
        self._loop = StructureLoop(self, window, L_cap=L_cap, M_cap=M_cap, feedback=feedback, **structure_params)
        return self._loop

    def get_detection(self, seq=0):
        """The detector's keypoints of the frame submitted last, sequence `seq`: (n, 2) float64 -- n_keypoints rows with
        the Harris detector, the frame's corner count with Shi-Tomasi (nothing in flight)."""
        kp = np.empty((self.cfg.n_keypoints, 2), np.float64)
        n = C.c_int32()
        self.ctx._chk(self.ctx._lib.vo_pipeline_get_detection_seq(self._h, int(seq), _ptr(kp), C.byref(n)))
        return kp[:n.value].copy()

    # ---- frames ----
    def step(self, prev_idx, next_idx):
        from vo import _native
        r = _native.StepResult()
        self.ctx._chk(self.ctx._lib.vo_pipeline_step(self._h, int(prev_idx), int(next_idx), C.byref(r)))
        return r

    def submit(self, prev_idx, next_idx):
        """Enqueue the frame's GPU work and return (at most two steps in flight)."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_submit(self._h, int(prev_idx), int(next_idx)))

    def collect(self):
        """Wait for the oldest submitted frame's result record."""
        from vo import _native
        r = _native.StepResult()
        self.ctx._chk(self.ctx._lib.vo_pipeline_collect(self._h, C.byref(r)))
        return r

    def collect_all(self):
        """Wait for the oldest submitted frame's records of all sequences (a list of StepResult)."""
        from vo import _native
        rs = (_native.StepResult * self.sequences)()
        self.ctx._chk(self.ctx._lib.vo_pipeline_collect_all(self._h, rs))
        return list(rs)

    def bookkeeping(self, phases, new_keypoints=None, pairs=None, pose_world_cam=None, p3p_inliers=None):
        """One frame's bookkeeping with the estimators' outputs given by the caller (vo_pipeline_bookkeeping)."""
        if phases & 1:
            kp = _c(np.asarray(new_keypoints).reshape(-1, 2), np.float64)
            pr = _c(np.asarray(pairs).reshape(-1, 2), np.int32)
            T_wc = _as_4x4(pose_world_cam)
            T_cw = _c(np.linalg.inv(T_wc), np.float64)
            inl = None if p3p_inliers is None else _c(np.asarray(p3p_inliers).reshape(-1), np.uint8)
            self.ctx._chk(self.ctx._lib.vo_pipeline_bookkeeping(self._h, int(phases), _ptr(kp), kp.shape[0], _ptr(pr),
                                                                pr.shape[0], _ptr(T_wc), _ptr(T_cw), _ptr(inl)))
        else:
            self.ctx._chk(self.ctx._lib.vo_pipeline_bookkeeping(self._h, int(phases), None, 0, None, 0, None, None, None))

    def ransac_bound(self, outlier_ratio):
        return int(self.ctx._lib.vo_pipeline_ransac_bound(self._h, float(outlier_ratio)))

    # ---- profiling / shared map ----
    def prof_read(self, kernel_id):
        ms, n = C.c_double(), C.c_int64()
        self.ctx._chk(self.ctx._lib.vo_pipeline_prof_read(self._h, int(kernel_id), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def prof_reset(self):
        self.ctx._chk(self.ctx._lib.vo_pipeline_prof_reset(self._h))

    def export_state_post(self, result, cap, d_record, seq=0):
        """Queues the shared-map record of the last collected step on the pipeline's stream (no synchronisation)."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_export_state_post_seq(self._h, int(seq), C.byref(result), int(cap),
                                                                      C.c_void_p(d_record)))

    def export_state_join(self, consumer_stream=None):
        """Orders the records posted so far before later work of `consumer_stream`, and later records after
        what that stream holds now."""
        self.ctx._chk(self.ctx._lib.vo_pipeline_export_state_join(self._h, C.c_void_p(consumer_stream or 0)))
