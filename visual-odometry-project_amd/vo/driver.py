"""Headless driver: the call sequence of the reference's ``main()`` (src/main.py:168-330)
without its matplotlib panes, ``time.sleep`` and dataset files.

    bootstrap on frames 0 and 2 (main.py:204-230):
        trackFeatures -> update_from_matches -> triangulate_matches -> outlier / inlier mask
        plumbing -> update_with_local_pose -> update_with_local_landmarks -> reset_outliers
    every later frame (main.py:248-286):
        trackFeatures -> estimate_pose(Features(triangulated keypoints, landmarks)) ->
        outliers[triangulate_inliers] = ~inliers -> update_from_matches ->
        update_with_world_pose -> reset_outliers -> compute_candidates ->
        triangulate_candidates -> update_with_world_landmarks

The monocular bootstrap leaves the scale free (|t| = 1 between frames 0 and 2), so the
trajectory is compared with ground truth after a single global scale fit.
"""
import time

import numpy as np

from vo.features import Tracker
from vo.landmarks import LandmarksTriangulator
from vo.pose_estimation import P3PPoseEstimator
from vo.primitives import Features, Sequence, State


def make_estimators(camera, ransac_threshold=0.25, bootstrap_method="8point"):
    """The triangulator and pose estimator as src/main.py:185-201 configures them (ransac_threshold: 0.25 px there).
    bootstrap_method: LandmarksTriangulator's `method` ("8point": the reference's route; "5point": the calibrated one)."""
    triangulator = LandmarksTriangulator(camera1=camera, camera2=camera, use_ransac=True, use_opencv=True,
                                         outlier_ratio=0.9, ransac_threshold=ransac_threshold, ransac_confidence=0.999,
                                         method=bootstrap_method)
    pose_estimator = P3PPoseEstimator(use_opencv=True, intrinsic_matrix=camera.intrinsic_matrix,
                                      inlier_threshold=1.25, outlier_ratio=0.9, confidence=0.9999,
                                      nonlinear_refinement=True)
    return triangulator, pose_estimator


def bootstrap(sequence: Sequence, tracker_mode: str = "klt", tracker_setup=None, ransac_threshold=0.25,
              bootstrap_method: str = "8point"):
    """main.py:204-230: frames 0 and 2 -> (state, tracker, triangulator, pose_estimator).  The 8-point RANSAC's
    hypotheses, counts and closing fit, the essential-matrix decomposition and the cheirality votes run on the GPU
    (csrc/bootstrap.hip); the host keeps the sequential accept rule and the bookkeeping classes.  bootstrap_method="5point":
    the relative pose starts from the five-point essential-matrix RANSAC instead (csrc/essential5.hip)."""
    camera = sequence.get_camera()
    triangulator, pose_estimator = make_estimators(camera, ransac_threshold, bootstrap_method)
    init_frame = next(sequence)
    state = State(init_frame)
    next(sequence)                                                       # frame 1 is skipped
    new_frame = next(sequence)
    if tracker_setup is not None:
        tracker_setup()
    tracker = Tracker(init_frame, mode=tracker_mode)
    matches = tracker.trackFeatures(state.curr_frame, new_frame)
    state.update_from_matches(matches)
    t0 = time.perf_counter()
    M, landmarks, inliers = triangulator.triangulate_matches(matches)
    state.bootstrap_info = {"relative_pose_seconds": time.perf_counter() - t0, "correspondences": int(len(inliers)),
                            "inliers": int(np.sum(inliers))}
    f2 = matches.frame2.features
    outliers = np.zeros(shape=(f2.length,), dtype=bool)
    outliers[f2.match_inliers] = ~inliers
    state.update_with_local_pose(M)
    inliers_mask = np.zeros_like(f2.matched_candidate_inliers).astype(bool)
    inliers_mask[f2.matched_candidate_inliers] = inliers
    state.update_with_local_landmarks(landmarks[inliers], inliers_mask)
    state.reset_outliers(outliers)
    return state, tracker, triangulator, pose_estimator


def run(sequence: Sequence, tracker_mode: str = "klt", max_frames: int = None, verbose: bool = False,
        bootstrap_method: str = "8point"):
    """The reference's loop through the drop-in classes, one call per stage (host bookkeeping, host <-> device
    copies around every kernel).  Returns dict(trajectory (n, 4, 4) camera-to-world, n_landmarks, frame_seconds)."""
    state, tracker, triangulator, pose_estimator = bootstrap(sequence, tracker_mode, bootstrap_method=bootstrap_method)
    trajectory = [np.eye(4), state.get_pose()]
    n_landmarks = [len(state.curr_frame.features.triangulated_inliers_landmarks)]
    seconds = []

    # ---- steady state ----
    for k, new_frame in enumerate(sequence):
        if max_frames is not None and k >= max_frames:
            break
        t0 = time.perf_counter()
        matches = tracker.trackFeatures(state.curr_frame, new_frame)
        f2 = matches.frame2.features
        (rmatrix, tvec), inliers = pose_estimator.estimate_pose(
            Features(keypoints=f2.triangulated_inliers_keypoints, landmarks=f2.triangulated_inliers_landmarks))
        outliers = np.zeros(shape=(f2.length,), dtype=bool)
        outliers[f2.triangulate_inliers] = ~inliers
        state.update_from_matches(matches)
        state.update_with_world_pose(np.concatenate((rmatrix, tvec), axis=1))
        state.reset_outliers(outliers)
        state.compute_candidates()
        feats = state.curr_frame.features
        assert np.sum(feats.candidate_mask) <= np.sum(feats.matched_candidate_inliers)
        if np.sum(feats.candidate_mask) > 0:
            world = triangulator.triangulate_candidates(feats, current_pose=state.get_pose())
            state.update_with_world_landmarks(world, matches.frame2.features.candidate_mask)
        seconds.append(time.perf_counter() - t0)
        trajectory.append(state.get_pose())
        n_landmarks.append(len(feats.triangulated_inliers_landmarks))
        if verbose:
            print("frame %3d: %4d keypoints, %4d landmarks, %.1f ms" % (k + 3, feats.length, n_landmarks[-1],
                                                                         seconds[-1] * 1e3))
    return dict(trajectory=np.array(trajectory), n_landmarks=np.array(n_landmarks), frame_seconds=np.array(seconds))


def _gray(image):
    from vo.features.klt import _gray as g
    return g(image)


class _TrackTap:
    """The observation records of the collected steps (Pipeline.export_tracks_post), without giving up the look-ahead: a
    record is posted right after its step's collect -- behind the step in flight on the pipeline's stream --, ordered
    before a side context's stream (export_state_join), and downloaded on that stream when the NEXT step is collected, by
    which time it has long been written.  Two device buffers per lane, used in turn."""

    def __init__(self, ctx, pipe, lanes=1):
        from vo import _native
        self.ctx, self.pipe = ctx, pipe
        self.side = _native.Context(ctx.device)          # (its own stream: a copy on the pipeline's would wait for the step in flight)
        self.nbytes = pipe.tracks_record_bytes(pipe.cap)
        self.ring = [[ctx.alloc(self.nbytes) for _ in range(lanes)] for _ in range(2)]
        self.turn = 0
        self.posted = []                                 # (device buffer, the list the record is appended to)

    def flush(self):
        from vo._pipeline import TrackRecord
        for d_rec, sink in self.posted:
            sink.append(TrackRecord.from_bytes(self.side.download(d_rec, (self.nbytes,), np.uint8), self.pipe.cap))
        self.posted = []

    def post(self, items):
        """items: (lane, the step's StepResult, the list its record goes to) of the step collected just now."""
        self.flush()
        for lane, r, sink in items:
            d_rec = self.ring[self.turn][lane]
            self.pipe.export_tracks_post(r, self.pipe.cap, d_rec, seq=lane)
            self.posted.append((d_rec, sink))
        self.pipe.export_state_join(self.side.stream)
        self.turn ^= 1

    def close(self):
        self.flush()
        for row in self.ring:
            for d in row:
                self.ctx.free(d)
        self.side.close()


class _BaTap:
    """The window bundle adjustment behind the collected steps: every lane keeps its last `window` observation records in
    device buffers of its own (posted like the tap's, behind the step in flight) and the refined poses of their frames; once
    a lane holds a full window, the windows of all such lanes go through one solver call per step
    (vo.landmarks.solve_windows).  mode "structure": the poses are held and the landmarks alone are refined
    (vo.landmarks.WindowStructureRefiner / refine_windows) -- the same records, the same builder, the same write-back."""

    def __init__(self, ctx, pipe, lanes, window, params, mode="full"):
        self.ctx, self.pipe, self.window, self.params, self.mode = ctx, pipe, int(window), params, mode
        nbytes = pipe.tracks_record_bytes(pipe.cap)
        self.ring = [[ctx.alloc(nbytes) for _ in range(self.window)] for _ in range(lanes)]
        self.turn = [0] * lanes
        self.adj = [None] * lanes

    def start(self, lane, K):
        from vo.landmarks import WindowBundleAdjuster, WindowStructureRefiner
        if self.adj[lane]:
            self.adj[lane].close()
        make = WindowStructureRefiner if self.mode == "structure" else WindowBundleAdjuster
        self.adj[lane] = make(K, window=self.window, cap=self.pipe.cap, context=self.ctx, **self.params)

    def step(self, items, feedback, results=None):
        """items: (lane, the step's StepResult, the list its `ba` entries go to) of the step collected just now."""
        from vo.landmarks import refine_windows, solve_windows
        for lane, r, _ in items:
            d_rec = self.ring[lane][self.turn[lane]]
            self.turn[lane] = (self.turn[lane] + 1) % self.window
            self.pipe.export_tracks_post(r, self.pipe.cap, d_rec, seq=lane)
            self.adj[lane].push(d_rec, np.concatenate((np.array(r.R_refined), np.array(r.t_refined))))
        if self.mode == "structure":
            for (lane, _, sink), s in zip(items, refine_windows([self.adj[lane] for lane, _, _ in items])):
                if s is None:
                    continue
                m = s.summary
                refused = int(m["n_refused"]) == s.n                       # (every landmark, or none to refuse: L = 0)
                sink.append(dict(frames=s.steps, poses=s.poses, ids=s.ids, landmarks=s.landmarks, kept=s.results["kept"].astype(bool),
                                 status=4 if refused else 0, cost0=float(m["cost0"]), cost=float(m["cost"]),
                                 iterations=int(m["max_iterations"]), n_kept=int(m["n_kept"])))
                if feedback and s.n and not refused:
                    self.pipe.update_landmarks(s.d_ids, s.d_X, seq=lane, n=s.n)      # (a landmark not kept: the bits it had)
            return
        solved = solve_windows([self.adj[lane] for lane, _, _ in items])
        for (lane, _, sink), s in zip(items, solved):
            if s is None:
                continue
            sink.append(dict(frames=s.steps, poses=s.poses, ids=s.ids, landmarks=s.landmarks, status=int(s.result["status"]),
                             cost0=float(s.result["cost0"]), cost=float(s.result["cost"]),
                             iterations=int(s.result["iterations"])))
            if feedback and s.n and int(s.result["status"]) != 4:
                self.pipe.update_landmarks(s.d_ids, s.d_X, seq=lane, n=s.n)

    def close(self):
        for a in self.adj:
            if a:
                a.close()
        for row in self.ring:
            for d in row:
                self.ctx.free(d)


class _StreamTap:
    """ba_feedback="stream": the structure refinement as stream-ordered work of the pipeline itself
    (vo.landmarks.StructureLoop).  Every collected step is posted -- record, window, refinement and write-back queue up behind
    the step in flight -- and nothing is waited for: the entries of a post are read from pinned memory at a later collect,
    when they have long landed.  download: every post is followed by a download of each lane's window (a synchronisation per
    step; for tests)."""

    def __init__(self, ctx, pipe, lanes, window, params):
        params = dict(params)
        self.download = bool(params.pop("download", False))
        self.window = int(window)
        self.loop = pipe.structure_loop(self.window, feedback=True, **params)
        self.waiting = []                                # (post index, [(lane, sink, the downloaded arrays)])

    def start(self, lane, K):
        self.loop.reset(lane)                            # (a hand-over: ids start again, a window must not span it)

    def drain(self, wait=False):
        """Appends the entries of the posts that have landed (wait: of every post) to their `ba` lists."""
        while self.waiting:
            j, items = self.waiting[0]
            entries = self.loop.poll(j, wait=wait)
            if entries is None:
                return
            self.waiting.pop(0)
            for lane, sink, extra in items:
                e = entries[lane]
                if not e["full"]:
                    continue
                m, L, step = e["summary"], int(e["L"]), int(e["step"])
                refused = int(m["n_refused"]) == L               # (every landmark, or none to refuse: L = 0)
                d = dict(frames=list(range(step - self.window + 1, step + 1)), status=4 if refused else 0, cost0=float(m["cost0"]),
                         cost=float(m["cost"]), iterations=int(m["max_iterations"]), n_kept=int(m["n_kept"]), n=L,
                         flags=int(e["flags"]), n_written=int(e["n_written"]))
                d.update(extra)
                sink.append(d)

    def step(self, items, feedback, results=None):
        """items: as _BaTap.step's; results: the records of all lanes as collect_all returned them."""
        self.drain()
        j = self.loop.post(results)
        waiting = []
        for lane, _, sink in items:
            extra = {}
            if self.download:
                w = self.loop.download(lane)
                extra = dict(poses=w.poses, ids=w.lm_id, landmarks=w.X, kept=w.results["kept"].astype(bool))
            waiting.append((lane, sink, extra))
        self.waiting.append((j, waiting))

    def close(self):
        self.drain(wait=True)
        self.loop.close()


def track_table(observations):
    """What a back end ingests from the per-step observation records (run_on_device(..., tracks=True)["observations"]):
    {id: dict(steps=(m,) int indices into `observations`, keypoints=(m, 2) float32, born=int, landmark=(3,) float64 -- the
    last one the track had, NaN if it never had one)}.  Host arithmetic."""
    table = {}
    for t, rec in enumerate(observations):
        for row in rec:
            e = table.setdefault(int(row["id"]), dict(steps=[], keypoints=[], born=int(row["born"]),
                                                       landmark=np.full(3, np.nan)))
            e["steps"].append(t)
            e["keypoints"].append((row["x"], row["y"]))
            if row["state"] == 2:
                e["landmark"] = np.array([row["X"], row["Y"], row["Z"]], np.float64)
    for e in table.values():
        e["steps"] = np.array(e["steps"], np.int64)
        e["keypoints"] = np.array(e["keypoints"], np.float32).reshape(-1, 2)
    return table


def run_on_device(sequence: Sequence, max_frames: int = None, n_keypoints: int = 2000, klt_win: int = 17,
                  klt_max_level: int = 2, hyp: int = 4000, context=None, verbose: bool = False,
                  redetect_start_pose: str = "current", bootstrap_win: int = None, bootstrap_max_level: int = None,
                  bootstrap_threshold: float = 0.25, bootstrap: str = "host", detector: str = "harris",
                  tracks: bool = False, ba_window: int = None, ba_feedback: bool = False, ba_params: dict = None,
                  bootstrap_method: str = "8point", ba_mode: str = "full", klt_fb: float = None):
    """Same loop, same bootstrap, but the steady state runs as the device-resident pipeline (vo_pipeline_*):
    after the host bootstrap the Features / State arrays are handed to the GPU once, every later frame costs one
    image upload and one call, and nothing but the pose record comes back.  KLT tracker mode with the Harris
    detector (BASELINE.json configs[1]); P3P-RANSAC as main.py:194-201 configures it (1.25 px, confidence 0.9999)
    with `hyp` hypotheses solved and scored per launch (a frame whose sequential rule needs more -- main.py allows
    10000 iterations -- gets further launches of hypotheses until the rule is done; the loop's state stays on the
    device).  redetect_start_pose: "identity" is the reference's
    update_features (klt.py:148-153: re-detected keypoints start their track at np.eye(4), so away from the origin
    they triangulate against a wrong baseline and can take the estimate with them); "current" starts them at the
    pose of the frame they were found on.
    detector: what refills the feature set -- "harris" (response + NMS, n_keypoints keypoints) or "shi-tomasi", the
    reference's cv2.goodFeaturesToTrack (klt.py:24-26, maxCorners = n_keypoints): as many corners as the frame has, and
    the re-detect limit follows that count (klt.py:114).
    bootstrap: "host" -- the bootstrap through the drop-in classes, handed over with set_state; "device" -- frames 0 and 2
    go into two slots of the frame store and the pipeline bootstraps itself from them (Pipeline.bootstrap_lanes with the
    one lane, vo_pipeline_bootstrap_lanes): same kernels, same result, no array brought back in between.
    Frames are uploaded as the sequence delivers them, grey or B, G, R; the pipeline's ingest makes them grey on the device.
    A camera with distortion_coeffs sets the lane's distortion (Pipeline.set_distortion: every frame is undistorted into
    the pinhole camera K behind its upload); one that really distorts needs bootstrap="device".
    bootstrap_method: the host route's two-view solver, LandmarksTriangulator's `method` -- "8point" (the reference's) or
    "5point" (the calibrated five-point RANSAC); the pipeline's own bootstrap is the 8-point one, so "5point" together with
    bootstrap="device" is refused.
    tracks: the pipeline keeps persistent track ids (Pipeline(track_ids=True)) and the result gains `observations`, one
    TrackRecord per step (id, born, keypoint, state, candidate, landmark of every feature; track_table() turns them into
    per-track observations) -- each posted behind its step and read back one collect later, so the look-ahead stays.
    ba_window: W (2 .. 16; needs tracks=True) -- a sliding-window bundle adjustment (vo.landmarks.WindowBundleAdjuster,
    vo_window_ba_dev) runs behind every collected step once W consecutive records exist, over the last W refined poses and
    the landmarks their records share; the result gains `ba`, one dict per solved window: frames (the records' step
    counters), poses (W, 12) world -> camera, ids, landmarks, status, cost0, cost, iterations.  The pipeline's own poses are
    never moved.  The solve is queued on the pipeline's stream and read back at once, so a collect then waits for the step
    in flight.  ba_params: WindowBundleAdjuster's n_fixed / huber_px / max_iter.  ba_feedback: the refined landmarks go
    back into the pipeline (Pipeline.update_landmarks) between steps; that needs nothing in flight, so every step is
    collected before the next is submitted: the look-ahead of one step is given up.  ba_window=None (the default): nothing
    of this exists and the loop is the one it was.
    ba_mode: "full" (the default) -- the adjustment above; "structure" -- every pose of the window is held and each landmark
    is refined on its own over the observations of its track (vo.landmarks.WindowStructureRefiner, vo_window_structure_dev):
    the cheap configuration the adjustment refuses.  ba_params then takes huber_px / max_iter / gate_px / min_parallax
    (n_fixed: ValueError), and a `ba` entry is frames, poses (as given), ids, landmarks, kept (per landmark: refined and
    through the gates; the others are the record's), status (0, or 4 when no landmark was refined: the whole window was
    refused, or it is empty, L = 0 -- as the adjustment reports an empty window), cost0, cost (sums over the landmarks not
    refused), iterations (the largest), n_kept.  ba_feedback writes back the same way.
    klt_fb: the tracker's forward-backward check in pixels (Pipeline.set_klt_fb, called once after the pipeline is made):
    a feature is kept only if tracking it back from the new frame returns to within klt_fb of where it started.  None (the
    default) makes no call: the run is the one it was.  Not > 0, or a pipeline that is not in tracker_mode "klt":
    ValueError.  The bootstrap keeps the plain tracker.
    ba_feedback="stream" (ba_mode="structure" only; ValueError otherwise, and without ba_window): the refinement and its
    write-back are stream-ordered work of the pipeline (Pipeline.structure_loop, vo_hip.h "Structure loop") -- steps are not
    drained, two stay pending as without a back end, nothing is read back, and a refined landmark reaches the features one
    step late at most, only where the feature still carries the landmark the window was built from.  A `ba` entry is then
    frames, status, cost0, cost, iterations, n_kept, n (landmarks of the window), flags, n_written (features the write-back
    wrote), taken from the entries the device leaves in pinned memory; ba_params["download"] = True adds poses, ids,
    landmarks, kept at the cost of a synchronisation per step (for tests).

    This is run_batch_on_device([sequence], lanes=1, ...)[0], the same loop (_DeviceRun) with one lane, and what comes
    with that: the lane's camera is set once more at the start (Pipeline.set_camera with the constructor's K, so the
    same values); steps are collected with collect_all (one record); the number of steps is the recording's length
    (`len(sequence)`, `increment`) capped by max_frames, and the frame size comes from _frame_shape; a recording with no
    frame after its bootstrap gets the host bootstrap and no pipeline, and its `features` are the bootstrap's own.
    frame_seconds differs from the batch driver's: it leaves out the time the sequence takes to deliver a frame
    (reading / decoding / rendering inside next() is the sequence's time, not the loop's)."""
    run = _DeviceRun([sequence], 1, max_frames, context, bootstrap, tracks,
                     (n_keypoints, klt_win, klt_max_level, bootstrap_win, bootstrap_max_level, bootstrap_threshold),
                     (n_keypoints, klt_win, klt_max_level, hyp, redetect_start_pose, detector),
                     ba_window=ba_window, ba_feedback=ba_feedback, ba_params=ba_params, bootstrap_method=bootstrap_method,
                     ba_mode=ba_mode, klt_fb=klt_fb)
    out = run.run()[0]
    out["frame_seconds"] = out["frame_seconds"] - np.array(run.read_seconds)
    if tracks:
        out.setdefault("observations", [])
    if ba_window is not None:
        out.setdefault("ba", [])
    if verbose:
        for r in out["results"]:
            print("%4d in, %4d tracked, %4d landmarks, %4d inliers, %3d candidates%s" % (
                r.n_features_in, r.n_tracked, r.n_landmarks, r.n_inliers, r.n_candidates,
                ", re-detected" if r.redetected else ""))
    return out


def _device_bootstrap(sequence, n_keypoints, klt_win, klt_max_level, bootstrap_win, bootstrap_max_level, bootstrap_threshold,
                      bootstrap_method="8point"):
    """The host bootstrap (main.py:204-230) of a recording the device-resident pipeline goes on with: (state, tracker)."""
    from vo.features.klt import KLTTracker
    saved = (dict(KLTTracker._feature_params), dict(KLTTracker._lk_params))

    def setup():
        # the bootstrap tracks Shi-Tomasi corners (the reference's find_corners, klt.py:98), as many as the
        # pipeline's detector keeps per frame
        KLTTracker._feature_params = dict(saved[0], maxCorners=n_keypoints)
        # (bootstrap_*: the two bootstrap frames are further apart than consecutive ones; on large frames the loop's own
        #  window and the reference's 0.25 px epipolar threshold can settle on a wrong model, bench.py: bootstrap_state)
        bw = bootstrap_win or klt_win
        KLTTracker._lk_params = dict(saved[1], winSize=(bw, bw),
                                     maxLevel=klt_max_level if bootstrap_max_level is None else bootstrap_max_level)

    try:
        state, tracker, _, _ = bootstrap(sequence, "klt", tracker_setup=setup, ransac_threshold=bootstrap_threshold,
                                         bootstrap_method=bootstrap_method)
    finally:
        KLTTracker._feature_params, KLTTracker._lk_params = saved
    return state, tracker


def _check_bootstrap_route(bootstrap, bootstrap_method="8point"):
    if bootstrap not in ("host", "device"):
        raise ValueError("bootstrap must be 'host' or 'device', not %r" % (bootstrap,))
    if bootstrap_method not in ("8point", "5point"):
        raise ValueError("bootstrap_method must be '8point' or '5point', not %r" % (bootstrap_method,))
    if bootstrap == "device" and bootstrap_method != "8point":
        raise ValueError("bootstrap_method=%r needs bootstrap='host': the pipeline's device bootstrap is the 8-point one"
                         % (bootstrap_method,))


def _bootstrap_frames(sequence):
    """Frames 0 and 2 of a recording as grey images (main.py:204-212: frame 1 is skipped)."""
    first = next(sequence)
    next(sequence)
    return _gray(first.image), _gray(next(sequence).image)


def _bootstrap_images(sequence):
    """Frames 0 and 2 of a recording as the sequence delivers them (grey or three-channel)."""
    first = next(sequence)
    next(sequence)
    return first.image, next(sequence).image


def _into_ring(ctx, ring, s, image):
    """image -> ring[s], a pinned buffer of its shape (made when the slot has none of that shape yet)."""
    if ring[s] is None or ring[s].shape != image.shape:
        ring[s] = ctx.pinned_empty(image.shape)
    ring[s][...] = image


def _lens_of(sequence, bootstrap):
    """The distortion coefficients of a recording's camera (None: a pinhole camera, nothing to set).  The host bootstrap
    works on the frames as delivered, so a camera that really distorts needs the device route, where the bootstrap's two
    frames go through the pipeline's ingest like every other."""
    cam = sequence.get_camera()
    dist = getattr(cam, "distortion_coeffs", None)
    if dist is not None and bootstrap != "device" and cam._distortion() is not None:
        raise ValueError("a camera with distortion coefficients needs bootstrap='device': the host bootstrap does not "
                         "undistort its frames")
    return dist


def _bootstrap_kwargs(n_keypoints, klt_win, klt_max_level, bootstrap_win, bootstrap_max_level, bootstrap_threshold):
    """Pipeline.bootstrap's parameters for what _device_bootstrap sets up on the host route."""
    return dict(max_corners=n_keypoints, klt_win=bootstrap_win or klt_win,
                klt_max_level=klt_max_level if bootstrap_max_level is None else bootstrap_max_level,
                threshold_px=bootstrap_threshold)


def _pipeline_kwargs(state, n_keypoints, klt_win, klt_max_level, hyp, redetect_start_pose, detector="harris"):
    """The pipeline's configuration for the steady state of main.py:194-201 (what run_on_device documents).  state: the
    bootstrap's State (its bearing threshold), None: State's default."""
    if state is None:
        state = State(None)
    return dict(n_keypoints=n_keypoints, klt_win=klt_win, klt_max_level=klt_max_level, hyp=hyp, p3p_threshold=1.25 ** 2,
                outlier_ratio=0.9, confidence=0.9999, max_iterations=10000, refine_iters=20,
                bearing_threshold=state._bearing_threshold, redetect_start_pose=redetect_start_pose, detector=detector)


def lane_schedule(lengths, lanes):
    """Which recording holds which lane at which step of a batch run (run_batch_on_device), host arithmetic only.

    lengths: steady-state steps of each recording (frames after its bootstrap), in queue order; lanes: pipeline
    sequences.  The first recordings take lanes 0, 1, ...; when a recording has made its last step, its lane takes the
    next recording of the queue at the following step, or goes idle when the queue is empty.  Recordings without a step
    hold no lane.  Returns dict(
        steps:   one tuple per step, entry l = (recording, its step index) held by lane l, or None (idle),
        starts:  (step, lane, recording) -- the lane starts that recording at that step (step 0: the first hand-over,
                 later ones: a restart, vo_pipeline_restart_seq),
        idles:   (step, lane) -- the lane is idle from that step on (set_active(lane, False)) until a start names it,
        lanes:   the lane count)."""
    lengths = [int(n) for n in lengths]
    lanes = int(lanes)
    if lanes < 1:
        raise ValueError("lane_schedule: need at least one lane")
    if any(n < 0 for n in lengths):
        raise ValueError("lane_schedule: negative recording length")
    queue = [r for r, n in enumerate(lengths) if n > 0]
    qi = 0
    holder, pos = [None] * lanes, [0] * lanes
    starts, idles, steps = [], [], []
    for lane in range(lanes):
        if qi < len(queue):
            holder[lane] = queue[qi]
            starts.append((0, lane, queue[qi]))
            qi += 1
        else:
            idles.append((0, lane))
    while any(h is not None for h in holder):
        t = len(steps)
        steps.append(tuple((holder[l], pos[l]) if holder[l] is not None else None for l in range(lanes)))
        for lane in range(lanes):
            if holder[lane] is None:
                continue
            pos[lane] += 1
            if pos[lane] < lengths[holder[lane]]:
                continue
            pos[lane] = 0
            if qi < len(queue):
                holder[lane] = queue[qi]
                starts.append((t + 1, lane, queue[qi]))
                qi += 1
            else:
                holder[lane] = None
                idles.append((t + 1, lane))
    # (a lane that falls idle after the last step does nothing more: only events inside the run are kept)
    idles = [(t, lane) for t, lane in idles if t < len(steps)]
    return dict(steps=steps, starts=starts, idles=idles, lanes=lanes)


def _steady_frames(sequence):
    """Frames a recording yields after its bootstrap has taken frames 0..2 (Sequence.__next__)."""
    inc = 1 if getattr(sequence, "dataset", "synthetic") == "synthetic" else int(getattr(sequence, "increment", 1))
    return len(range(3 * inc, len(sequence), inc))


def _frame_shape(sequence):
    if getattr(sequence, "dataset", None) == "synthetic":
        return (int(sequence.H), int(sequence.W))
    return tuple(_gray(sequence.get_frame(0).image).shape[:2])


class _DeviceRun:
    """The device-resident frame loop of run_batch_on_device, and of run_on_device as its one-lane case.

    Frames go through one ring of pinned buffers per lane AS DELIVERED (three channels where the sequence gives three: the
    grey conversion and the undistortion run on the device behind the DMA, csrc/ingest.hip) and are uploaded on the
    pipeline's upload stream ONE STEP AHEAD of their use (vo_pipeline_set_frame_pinned / _bgr_pinned): while step
    k -> k+1 runs, frame k+2 -- read ahead from the sequence, as a file or dataset reader can -- crosses PCIe beside it.
    One step of look-ahead on the results too: the record of step k is read back after step k+1 has been submitted.

    boot_args: _device_bootstrap's / _bootstrap_kwargs' arguments, pipe_args: _pipeline_kwargs' after the state."""
    SLOTS = 4

    def __init__(self, sequences, lanes, max_frames, context, bootstrap, tracks, boot_args, pipe_args, ba_window=None,
                 ba_feedback=False, ba_params=None, bootstrap_method="8point", ba_mode="full", klt_fb=None):
        _check_bootstrap_route(bootstrap, bootstrap_method)
        # the tracker's forward-backward check (Pipeline.set_klt_fb), set once after creation; None: no call at all
        if klt_fb is not None and not float(klt_fb) > 0.0:
            raise ValueError("klt_fb must be > 0 pixels (+inf allowed) or None, got %r" % (klt_fb,))
        self.klt_fb = None if klt_fb is None else float(klt_fb)
        self.bootstrap_method = bootstrap_method
        if ba_window is not None and not tracks:
            raise ValueError("ba_window needs tracks=True: the window is built from the observation records")
        if ba_mode not in ("full", "structure"):
            raise ValueError("ba_mode must be 'full' or 'structure', got %r" % (ba_mode,))
        # ba_feedback="stream": the write-back is stream-ordered work of the pipeline (_StreamTap); steps are not drained
        self.ba_stream = isinstance(ba_feedback, str) and ba_feedback == "stream"
        if isinstance(ba_feedback, str) and not self.ba_stream:
            raise ValueError("ba_feedback must be False, True or 'stream', got %r" % (ba_feedback,))
        if self.ba_stream and ba_window is None:
            raise ValueError("ba_feedback='stream' needs ba_window: there is no window to refine")
        if self.ba_stream and ba_mode != "structure":
            raise ValueError("ba_feedback='stream' needs ba_mode='structure', got ba_mode=%r" % (ba_mode,))
        self.ba_window, self.ba_feedback, self.ba_params = ba_window, bool(ba_feedback) and not self.ba_stream, dict(ba_params or {})
        self.ba_mode = ba_mode
        if ba_window is not None and ba_mode == "structure":
            allowed = ("huber_px", "max_iter", "gate_px", "min_parallax") + (("download",) if self.ba_stream else ())
            for k in self.ba_params:
                if k not in allowed:
                    raise ValueError("ba_mode='structure' holds every pose: ba_params takes %s, not %s" % (", ".join(allowed), k))
        self.ba = None                                   # lane -> its WindowBundleAdjuster (open_pipeline)
        self.sequences = sequences = list(sequences)
        self.on_device, self.context, self.tracks = bootstrap == "device", context, tracks
        self.boot_args, self.pipe_args = boot_args, pipe_args
        self.shapes = [_frame_shape(s) for s in sequences]
        if len(set(self.shapes)) > 1:
            raise ValueError("run_batch_on_device: the recordings' frame sizes differ (%s); one pipeline takes one H x W"
                             % sorted(set(self.shapes)))
        self.lens = [_lens_of(s, bootstrap) for s in sequences]
        self.lengths = [_steady_frames(s) for s in sequences]
        if max_frames is not None:
            self.lengths = [min(n, int(max_frames)) for n in self.lengths]
        self.lanes = int(lanes) if lanes else max(1, min(len(sequences), 16))
        plan = lane_schedule(self.lengths, self.lanes)
        self.steps = plan["steps"]
        self.first = plan["starts"][0][2] if self.steps else None       # (lane 0's recording at step 0)
        self.events = {}                                 # step -> (lane, the recording it starts, or None: it goes idle)
        for t, lane, r in plan["starts"]:
            self.events.setdefault(t, []).append((lane, r))
        for t, lane in plan["idles"]:
            self.events.setdefault(t, []).append((lane, None))
        self.boot = {}                                   # recording -> its host bootstrap (state, tracker)
        self.out = [None] * len(sequences)
        self.ctx = self.pipe = self.tap = self.ring = None
        self.pending, self.slot = [], 0                  # steps submitted and not collected; the `prev` of the next submit
        # per step of the RUN, all lanes together: the part of its wall time spent inside next(sequence).  Only run_on_device
        # reads it: with one recording on one lane the run's steps are the recording's, entry for entry of frame_seconds
        self.reading, self.read_seconds = 0.0, []

    def boot_of(self, r):
        if r not in self.boot:
            # (the default route keeps the call it always made)
            extra = {} if self.bootstrap_method == "8point" else {"bootstrap_method": self.bootstrap_method}
            self.boot[r] = _device_bootstrap(self.sequences[r], *self.boot_args, **extra)
        return self.boot[r]

    def open_result(self, r):
        state, tracker = self.boot_of(r)
        self.out[r] = dict(trajectory=[np.eye(4), state.get_pose()],
                           n_landmarks=[len(state.curr_frame.features.triangulated_inliers_landmarks)], frame_seconds=[],
                           results=[], features=state.curr_frame.features)

    def camera_of(self, r):
        return np.asarray(self.sequences[r].get_camera().intrinsic_matrix, np.float64)

    def open_pipeline(self):
        from vo import _native
        self.ctx = self.context or _native.default_context()
        state0 = None if self.on_device else self.boot_of(self.first)[0]
        H, W = self.shapes[self.first]
        self.pipe = _native.Pipeline(self.ctx, H, W, self.SLOTS, self.camera_of(self.first), sequences=self.lanes,
                                     track_ids=self.tracks, **_pipeline_kwargs(state0, *self.pipe_args))
        if self.klt_fb is not None:
            if self.pipe.tracker != "klt":
                raise ValueError("klt_fb belongs to tracker_mode 'klt', the pipeline runs %r" % (self.pipe.tracker,))
            self.pipe.set_klt_fb(self.klt_fb)
        self.tap = _TrackTap(self.ctx, self.pipe, self.lanes) if self.tracks else None
        if self.ba_window is not None and self.ba_stream:
            self.ba = _StreamTap(self.ctx, self.pipe, self.lanes, self.ba_window, self.ba_params)
        elif self.ba_window is not None:
            self.ba = _BaTap(self.ctx, self.pipe, self.lanes, self.ba_window, self.ba_params, self.ba_mode)
        self.ring = [[None] * self.SLOTS for _ in range(self.lanes)]

    def set_camera(self, lane, r):
        self.pipe.set_camera(self.camera_of(r), lane)
        # (the lens at every start: a lane that held a distorting camera's recording must lose its coefficients with it)
        if any(d is not None for d in self.lens):
            self.pipe.set_distortion(lane, self.lens[r])

    def put(self, lane, s, r):
        """Recording r's next frame -> slot s of its lane, through the lane's pinned ring."""
        t0 = time.perf_counter()
        frame = next(self.sequences[r])
        self.reading += time.perf_counter() - t0
        _into_ring(self.ctx, self.ring[lane], s, frame.image)
        self.pipe.set_frame(s, self.ring[lane][s], seq=lane, pinned=True)

    def start(self, lane, r, t):
        """Host route: the lane takes recording r from its host bootstrap (step 0: a hand-over, later: a restart)."""
        state, tracker = self.boot_of(r)
        self.open_result(r)
        frame = state.curr_frame
        self.set_camera(lane, r)
        args = (frame.features, state.curr_pose, state.prev_pose)
        nf = tracker._tracker._num_features
        if t == 0:
            self.pipe.set_frame(self.slot, _gray(frame.image), seq=lane, pinned=False)
            self.pipe.set_state(self.slot, *args, num_features=nf, seq=lane)
        else:
            self.pipe.restart(lane, self.slot, *args, num_features=nf, image=_gray(frame.image))

    def start_on_device(self, starts, t):
        """Device route: the lanes that start a recording at this step -- starts: (lane, recording) -- through ONE
        bootstrap call, from frames 0 and 2 as delivered (the pipeline's ingest makes them grey, undistorted)."""
        from vo import _native
        a = (self.slot + 1) % self.SLOTS                 # (the slot the recordings' next frames take afterwards)
        for lane, r in starts:
            img0, img2 = _bootstrap_images(self.sequences[r])
            self.set_camera(lane, r)
            if t > 0:
                self.pipe.set_active(lane, False)        # (the lane's frame in the current slot can only be replaced while idle)
            self.pipe.set_frame(a, img0, seq=lane, pinned=False)
            self.pipe.set_frame(self.slot, img2, seq=lane, pinned=False)
        results = self.pipe.bootstrap_lanes(a, self.slot, [lane for lane, _ in starts],
                                            **_bootstrap_kwargs(*self.boot_args))
        for (lane, r), res in zip(starts, results):
            if res.status != 0:
                raise _native.VoError(res.status, "the bootstrap of recording %d (lane %d) failed" % (r, lane))
            self.out[r] = dict(trajectory=[np.eye(4), self.pipe.get_state(lane)["curr_pose"]],
                               n_landmarks=[res.n_landmarks], frame_seconds=[], results=[], features=None)

    def finish(self, lane, r):
        self.out[r]["features"] = self.pipe.get_features(lane)

    def collect_one(self):
        row = self.steps[self.pending.pop(0)]
        rs = self.pipe.collect_all()
        taken = [(lane, rs[lane], self.out[e[0]]) for lane, e in enumerate(row) if e is not None]
        for lane, r, o in taken:
            o["results"].append(r)                       # (run() reads the poses and counts out of them after the loop)
        if self.tap:
            self.tap.post([(lane, r, o.setdefault("observations", [])) for lane, r, o in taken])
        if self.ba:
            self.ba.step([(lane, r, o.setdefault("ba", [])) for lane, r, o in taken],
                         feedback=self.ba_feedback and not self.pending, results=rs)

    def change(self, t):
        """Step t's events -- lanes going idle, lanes starting a recording (the host route one by one, the device route
        all of them in one call) -- with nothing in flight: drain, read what ends, then idle / start, and the first
        frame after the bootstrap of every recording that starts goes into the slot after the current one."""
        events = sorted(self.events[t])
        if t > 0:
            while self.pending:
                self.collect_one()
            if self.tap:
                self.tap.flush()                         # (a hand-over rewrites the buffers the posted records read)
            for lane, _ in events:
                prev = self.steps[t - 1][lane]
                if prev is not None:
                    self.finish(lane, prev[0])
        starts = [(lane, r) for lane, r in events if r is not None]
        if self.ba:
            for lane, r in starts:
                self.ba.start(lane, self.camera_of(r))    # (a hand-over: ids start again, a window must not span it)
        for lane, r in events:
            if r is None:
                self.pipe.set_active(lane, False)
            elif not self.on_device:
                self.start(lane, r, t)
        if self.on_device and starts:
            self.start_on_device(starts, t)
        for lane, r in starts:
            self.put(lane, (self.slot + 1) % self.SLOTS, r)

    def step(self, t):
        """Step t, slot -> slot + 1: the oldest of two pending steps is collected, the frames of step t + 1 (for lanes that
        keep their recording) go into slot + 2 -- read last by a collected step --, the step is submitted, and the pyramid
        of slot + 2 is hinted behind its tracker."""
        if t in self.events:
            self.change(t)
        t0 = time.perf_counter()
        self.reading = 0.0
        nxt, after = (self.slot + 1) % self.SLOTS, (self.slot + 2) % self.SLOTS
        while self.pending and (len(self.pending) == 2 or self.ba_feedback):
            self.collect_one()                           # (ba_feedback: nothing may be in flight when landmarks go back)
        ahead = []                                       # (lane, recording) of the lanes that keep theirs at step t + 1
        if t + 1 < len(self.steps):
            ahead = [(lane, e[0]) for lane, e in enumerate(self.steps[t + 1]) if e is not None and e[1] > 0]
        for lane, r in ahead:
            self.put(lane, after, r)
        self.pipe.submit(self.slot, nxt)
        if ahead:
            self.pipe.prepare(after)
        self.pending.append(t)
        self.slot = nxt
        seconds = time.perf_counter() - t0
        self.read_seconds.append(self.reading)
        for e in self.steps[t]:
            if e is not None:
                self.out[e[0]]["frame_seconds"].append(seconds)

    def run(self):
        for r, n in enumerate(self.lengths):             # (recordings without a steady-state step: the bootstrap is all there is)
            if n == 0:
                self.open_result(r)
        if self.steps:
            self.open_pipeline()
            for t in range(len(self.steps)):
                self.step(t)
            while self.pending:
                self.collect_one()
            for lane, e in enumerate(self.steps[-1]):
                if e is not None:
                    self.finish(lane, e[0])
            if self.tap:
                self.tap.close()
            if self.ba:
                self.ba.close()
            self.pipe.close()
        for o in self.out:
            o["trajectory"] = np.array(o["trajectory"] + [r.pose_world_cam() for r in o["results"]])
            o["n_landmarks"] = np.array(o["n_landmarks"] + [r.n_landmarks for r in o["results"]])
            o["frame_seconds"] = np.array(o["frame_seconds"])
        return self.out


def run_batch_on_device(sequences, lanes: int = None, max_frames: int = None, n_keypoints: int = 2000, klt_win: int = 17,
                        klt_max_level: int = 2, hyp: int = 4000, context=None, verbose: bool = False,
                        redetect_start_pose: str = "current", bootstrap_win: int = None, bootstrap_max_level: int = None,
                        bootstrap_threshold: float = 0.25, bootstrap: str = "host", detector: str = "harris",
                        tracks: bool = False, ba_window: int = None, ba_feedback: bool = False, ba_params: dict = None,
                        bootstrap_method: str = "8point", ba_mode: str = "full", klt_fb: float = None):
    """run_on_device for many recordings at once: one pipeline of `lanes` sequences (default: one per recording, at most
    16), every lane with its recording's camera (vo_pipeline_set_camera_seq).  Each recording is bootstrapped on the host
    (_device_bootstrap); when one ends its lane takes the next recording of the queue (vo_pipeline_restart_seq) or
    goes idle (vo_pipeline_set_active_seq) -- lane_schedule says when.  Frames go through one pinned ring per lane,
    uploaded a step ahead.  The steps in flight are drained before a lane changes recording (nothing may be in flight for
    the three calls), so each such step loses the look-ahead once.  All recordings must have the same frame size.
    A recording whose camera has distortion_coeffs sets its lane's distortion (Pipeline.set_distortion) at every start.
    bootstrap="device": a lane's recording starts from its frames 0 and 2 inside the pipeline instead: for a change of
    recording the lane goes idle, frame 0 goes into the slot after the current one and frame 2 into the current one; the
    lanes that start at the same step (all of them at step 0) then go through ONE call (Pipeline.bootstrap_lanes).  (A
    recording without a steady-state step never holds a lane: host route.)  detector: as in run_on_device, for every lane.
    tracks: as in run_on_device -- every recording's dict gains `observations`, one record per step it took (a lane's ids
    start over with every recording: each start is a hand-over).
    ba_window / ba_feedback / ba_params / ba_mode: as in run_on_device; the windows of all lanes that hold a full one go through one
    solver call per step, and a lane's window starts again with every recording.
    bootstrap_method: as in run_on_device, for every recording's host bootstrap.
    klt_fb: as in run_on_device, for every lane.

    Returns one dict per recording, in input order, with run_on_device's keys (frame_seconds: the batch's wall time of
    each step the recording took part in, the delivery of the next step's frames included).  run_on_device is this
    function with one recording and one lane; each lane computes what it computes for the lane's recording alone."""
    out = _DeviceRun(sequences, lanes, max_frames, context, bootstrap, tracks,
                     (n_keypoints, klt_win, klt_max_level, bootstrap_win, bootstrap_max_level, bootstrap_threshold),
                     (n_keypoints, klt_win, klt_max_level, hyp, redetect_start_pose, detector),
                     ba_window=ba_window, ba_feedback=ba_feedback, ba_params=ba_params, bootstrap_method=bootstrap_method,
                     ba_mode=ba_mode, klt_fb=klt_fb).run()
    if ba_window is not None:
        for o in out:
            o.setdefault("ba", [])
    if verbose:
        for o in out:
            print("%d steps, %d landmarks at the end" % (len(o["results"]), o["n_landmarks"][-1]))
    return out


def trajectory_error(result, sequence: Sequence):
    """RMS position error against the analytic ground truth after fitting the one free scale
    of the monocular bootstrap.  Trajectory index 0 is frame 0, index i >= 1 is frame i + 1."""
    traj = result["trajectory"]
    frames = [0] + list(range(2, 2 + len(traj) - 1))
    gt = np.stack([np.linalg.inv(sequence.ground_truth_pose(0)) @ sequence.ground_truth_pose(f) for f in frames])
    p, q = traj[:, :3, 3], gt[:, :3, 3]
    scale = float(np.sum(p * q) / max(np.sum(p * p), 1e-30))
    return dict(scale=scale, rms=float(np.sqrt(np.mean(np.sum((scale * p - q) ** 2, axis=1)))),
                path_length=float(np.sum(np.linalg.norm(np.diff(q, axis=0), axis=1))))


if __name__ == "__main__":
    seq = Sequence("synthetic", n_frames=30, height=480, width=640, channels=3)
    out = run(seq, "klt", verbose=True)
    print(trajectory_error(out, seq), "mean ms/frame", 1e3 * out["frame_seconds"].mean())
    seq = Sequence("synthetic", n_frames=30, height=480, width=640, channels=3)
    out = run_on_device(seq, n_keypoints=500, verbose=True)
    print(trajectory_error(out, seq), "mean ms/frame", 1e3 * out["frame_seconds"].mean())
