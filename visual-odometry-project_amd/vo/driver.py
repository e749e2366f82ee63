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


def make_estimators(camera, ransac_threshold=0.25):
    """The triangulator and pose estimator as src/main.py:185-201 configures them (ransac_threshold: 0.25 px there)."""
    triangulator = LandmarksTriangulator(camera1=camera, camera2=camera, use_ransac=True, use_opencv=True,
                                         outlier_ratio=0.9, ransac_threshold=ransac_threshold, ransac_confidence=0.999)
    pose_estimator = P3PPoseEstimator(use_opencv=True, intrinsic_matrix=camera.intrinsic_matrix,
                                      inlier_threshold=1.25, outlier_ratio=0.9, confidence=0.9999,
                                      nonlinear_refinement=True)
    return triangulator, pose_estimator


def bootstrap(sequence: Sequence, tracker_mode: str = "klt", tracker_setup=None, ransac_threshold=0.25):
    """main.py:204-230: frames 0 and 2 -> (state, tracker, triangulator, pose_estimator).  The 8-point RANSAC's
    hypotheses, counts and closing fit, the essential-matrix decomposition and the cheirality votes run on the GPU
    (csrc/bootstrap.hip); the host keeps the sequential accept rule and the bookkeeping classes."""
    camera = sequence.get_camera()
    triangulator, pose_estimator = make_estimators(camera, ransac_threshold)
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


def run(sequence: Sequence, tracker_mode: str = "klt", max_frames: int = None, verbose: bool = False):
    """The reference's loop through the drop-in classes, one call per stage (host bookkeeping, host <-> device
    copies around every kernel).  Returns dict(trajectory (n, 4, 4) camera-to-world, n_landmarks, frame_seconds)."""
    state, tracker, triangulator, pose_estimator = bootstrap(sequence, tracker_mode)
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
                  tracks: bool = False):
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
    go into two slots of the frame store and the pipeline bootstraps itself from them (Pipeline.bootstrap,
    vo_pipeline_bootstrap_seq): same kernels, same result, no array brought back in between.
    Frames are uploaded as the sequence delivers them, grey or B, G, R; the pipeline's ingest makes them grey on the device.
    A camera with distortion_coeffs sets the lane's distortion (Pipeline.set_distortion: every frame is undistorted into
    the pinhole camera K behind its upload); one that really distorts needs bootstrap="device".
    tracks: the pipeline keeps persistent track ids (Pipeline(track_ids=True)) and the result gains `observations`, one
    TrackRecord per step (id, born, keypoint, state, candidate, landmark of every feature; track_table() turns them into
    per-track observations) -- each posted behind its step and read back one collect later, so the look-ahead stays."""
    from vo import _native
    _check_bootstrap_route(bootstrap)
    ctx = context or _native.default_context()
    K = np.asarray(sequence.get_camera().intrinsic_matrix, np.float64)
    dist = _lens_of(sequence, bootstrap)
    SLOTS = 4
    if bootstrap == "device":
        img0, img = _bootstrap_images(sequence)          # (as delivered: the pipeline's ingest makes them grey, undistorted)
        H, W = img.shape[:2]
        pipe = _native.Pipeline(ctx, H, W, SLOTS, K, track_ids=tracks,
                                **_pipeline_kwargs(None, n_keypoints, klt_win, klt_max_level, hyp, redetect_start_pose, detector))
        if dist is not None:
            pipe.set_distortion(0, dist)
        pipe.set_frame(1, img0)                          # (slot 1 takes frame 3 next: the bootstrap is done with it by then)
        pipe.set_frame(0, img)
        boot = pipe.bootstrap(1, 0, **_bootstrap_kwargs(n_keypoints, klt_win, klt_max_level, bootstrap_win,
                                                        bootstrap_max_level, bootstrap_threshold))
        trajectory = [np.eye(4), pipe.get_state()["curr_pose"]]
        n_landmarks = [boot.n_landmarks]
    else:
        state, tracker = _device_bootstrap(sequence, n_keypoints, klt_win, klt_max_level, bootstrap_win, bootstrap_max_level,
                                           bootstrap_threshold)
        frame = state.curr_frame
        img = _gray(frame.image)
        H, W = img.shape
        pipe = _native.Pipeline(ctx, H, W, SLOTS, K, track_ids=tracks,
                                **_pipeline_kwargs(state, n_keypoints, klt_win, klt_max_level, hyp, redetect_start_pose, detector))
        pipe.set_frame(0, img)
        pipe.set_state(0, frame.features, state.curr_pose, state.prev_pose, num_features=tracker._tracker._num_features)
        trajectory = [np.eye(4), state.get_pose()]
        n_landmarks = [len(frame.features.triangulated_inliers_landmarks)]
    seconds, results, observations = [], [], []
    tap = _TrackTap(ctx, pipe) if tracks else None

    def collect():
        results.append(pipe.collect())
        if tap:
            tap.post([(0, results[-1], observations)])
    # Frames go through a ring of pinned buffers AS DELIVERED (three channels where the sequence gives three: the grey
    # conversion and the undistortion run on the device behind the DMA, csrc/ingest.hip) and are uploaded on the
    # pipeline's upload stream ONE STEP AHEAD of their use (vo_pipeline_set_frame_pinned / _bgr_pinned): while step
    # k -> k+1 runs, frame k+2 -- read ahead from the sequence, as a file or dataset reader can -- crosses PCIe beside it.
    # One frame of look-ahead on the results as before: the pose of frame k is read back after frame k+1 has been submitted.
    ring = [None] * SLOTS
    frames = iter(sequence)
    taken = 0

    def take():
        nonlocal taken
        if max_frames is not None and taken >= max_frames:
            return None
        f = next(frames, None)
        if f is not None:
            taken += 1
        return f

    def put(s, f):
        _into_ring(ctx, ring, s, f.image)
        pipe.set_frame(s, ring[s], pinned=True)

    slot, pending = 0, 0
    ahead = take()
    if ahead is not None:
        put(1, ahead)
    while ahead is not None:
        t0 = time.perf_counter()
        nxt = (slot + 1) % SLOTS
        if pending == 2:
            collect()
            pending -= 1
        t1 = time.perf_counter()
        ahead = take()                                   # the frame of the NEXT step: its slot was read last by a collected step
        t2 = time.perf_counter()                         # (reading / decoding / rendering the frame is the sequence's time, not the loop's)
        if ahead is not None:
            put((slot + 2) % SLOTS, ahead)
        pipe.submit(slot, nxt)
        if ahead is not None:
            pipe.prepare((slot + 2) % SLOTS)            # its pyramid too, behind this step's tracker
        pending += 1
        slot = nxt
        seconds.append(time.perf_counter() - t0 - (t2 - t1))
    while pending:
        collect()
        pending -= 1
    if tap:
        tap.close()
    for r in results:
        trajectory.append(r.pose_world_cam())
        n_landmarks.append(r.n_landmarks)
        if verbose:
            print("%4d in, %4d tracked, %4d landmarks, %4d inliers, %3d candidates%s" % (
                r.n_features_in, r.n_tracked, r.n_landmarks, r.n_inliers, r.n_candidates,
                ", re-detected" if r.redetected else ""))
    features = pipe.get_features()
    pipe.close()
    out = dict(trajectory=np.array(trajectory), n_landmarks=np.array(n_landmarks), frame_seconds=np.array(seconds),
               results=results, features=features)
    if tracks:
        out["observations"] = observations
    return out


def _device_bootstrap(sequence, n_keypoints, klt_win, klt_max_level, bootstrap_win, bootstrap_max_level, bootstrap_threshold):
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
        state, tracker, _, _ = bootstrap(sequence, "klt", tracker_setup=setup, ransac_threshold=bootstrap_threshold)
    finally:
        KLTTracker._feature_params, KLTTracker._lk_params = saved
    return state, tracker


def _check_bootstrap_route(bootstrap):
    if bootstrap not in ("host", "device"):
        raise ValueError("bootstrap must be 'host' or 'device', not %r" % (bootstrap,))


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


def run_batch_on_device(sequences, lanes: int = None, max_frames: int = None, n_keypoints: int = 2000, klt_win: int = 17,
                        klt_max_level: int = 2, hyp: int = 4000, context=None, verbose: bool = False,
                        redetect_start_pose: str = "current", bootstrap_win: int = None, bootstrap_max_level: int = None,
                        bootstrap_threshold: float = 0.25, bootstrap: str = "host", detector: str = "harris",
                        tracks: bool = False):
    """run_on_device for many recordings at once: one pipeline of `lanes` sequences (default: one per recording, at most
    16), every lane with its recording's camera (vo_pipeline_set_camera_seq).  Each recording is bootstrapped on the host
    as run_on_device does it; when one ends its lane takes the next recording of the queue (vo_pipeline_restart_seq) or
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

    Returns one dict per recording, in input order, with run_on_device's keys (frame_seconds: the batch's wall time of
    each step the recording took part in).  Each lane computes what run_on_device computes for its recording alone."""
    from vo import _native
    _check_bootstrap_route(bootstrap)
    on_device = bootstrap == "device"
    sequences = list(sequences)
    if not sequences:
        return []
    shapes = [_frame_shape(s) for s in sequences]
    if any(sh != shapes[0] for sh in shapes):
        raise ValueError("run_batch_on_device: the recordings' frame sizes differ (%s); one pipeline takes one H x W"
                         % sorted(set(shapes)))
    H, W = shapes[0]
    lengths = [_steady_frames(s) for s in sequences]
    if max_frames is not None:
        lengths = [min(n, int(max_frames)) for n in lengths]
    lanes = int(lanes) if lanes else max(1, min(len(sequences), 16))
    plan = lane_schedule(lengths, lanes)
    steps = plan["steps"]
    ctx = context or _native.default_context()
    boot = {}

    def boot_of(r):
        if r not in boot:
            boot[r] = _device_bootstrap(sequences[r], n_keypoints, klt_win, klt_max_level, bootstrap_win,
                                        bootstrap_max_level, bootstrap_threshold)
        return boot[r]

    out = [None] * len(sequences)

    def open_result(r):
        state, tracker = boot_of(r)
        out[r] = dict(trajectory=[np.eye(4), state.get_pose()],
                      n_landmarks=[len(state.curr_frame.features.triangulated_inliers_landmarks)], frame_seconds=[],
                      results=[], features=state.curr_frame.features)

    for r in range(len(sequences)):            # (recordings without a steady-state step: the bootstrap is all there is)
        if lengths[r] == 0:
            open_result(r)
    if steps:
        first = next(r for (_, _, r) in plan["starts"])
        state0 = None if on_device else boot_of(first)[0]
        K0 = np.asarray(sequences[first].get_camera().intrinsic_matrix, np.float64)
        SLOTS = 4
        pipe = _native.Pipeline(ctx, H, W, SLOTS, K0, sequences=lanes, track_ids=tracks,
                                **_pipeline_kwargs(state0, n_keypoints, klt_win, klt_max_level, hyp, redetect_start_pose,
                                                   detector))
        tap = _TrackTap(ctx, pipe, lanes) if tracks else None
        ring = [[None] * SLOTS for _ in range(lanes)]      # (frames as delivered, see run_on_device)
        lens = [_lens_of(s, bootstrap) for s in sequences]
        any_lens = any(d is not None for d in lens)

        def set_lens(lane, r):
            # (every start: a lane that held a distorting camera's recording must lose its coefficients with it)
            if any_lens:
                pipe.set_distortion(lane, lens[r])
        taken = [0] * len(sequences)

        def next_frame(r):
            taken[r] += 1
            return next(sequences[r])

        def put(lane, s, r):
            _into_ring(ctx, ring[lane], s, next_frame(r).image)
            pipe.set_frame(s, ring[lane][s], seq=lane, pinned=True)

        def start_on_device(starts, t, slot):
            """The lanes that start a recording at this step -- starts: (lane, recording) -- through ONE bootstrap call."""
            a = (slot + 1) % SLOTS                       # (the slot the recordings' next frames take afterwards)
            for lane, r in starts:
                img0, img2 = _bootstrap_images(sequences[r])
                pipe.set_camera(np.asarray(sequences[r].get_camera().intrinsic_matrix, np.float64), lane)
                set_lens(lane, r)
                if t > 0:
                    pipe.set_active(lane, False)         # (the lane's frame in the current slot can only be replaced while idle)
                pipe.set_frame(a, img0, seq=lane, pinned=False)
                pipe.set_frame(slot, img2, seq=lane, pinned=False)
            results = pipe.bootstrap_lanes(a, slot, [lane for lane, _ in starts],
                                           **_bootstrap_kwargs(n_keypoints, klt_win, klt_max_level, bootstrap_win,
                                                               bootstrap_max_level, bootstrap_threshold))
            for (lane, r), res in zip(starts, results):
                if res.status != 0:
                    raise _native.VoError(res.status, "the bootstrap of recording %d (lane %d) failed" % (r, lane))
                out[r] = dict(trajectory=[np.eye(4), pipe.get_state(lane)["curr_pose"]], n_landmarks=[res.n_landmarks],
                              frame_seconds=[], results=[], features=None)

        def start(lane, r, t, slot):
            state, tracker = boot_of(r)
            open_result(r)
            frame = state.curr_frame
            pipe.set_camera(np.asarray(sequences[r].get_camera().intrinsic_matrix, np.float64), lane)
            set_lens(lane, r)
            args = (frame.features, state.curr_pose, state.prev_pose)
            nf = tracker._tracker._num_features
            if t == 0:
                pipe.set_frame(slot, _gray(frame.image), seq=lane, pinned=False)
                pipe.set_state(slot, *args, num_features=nf, seq=lane)
            else:
                pipe.restart(lane, slot, *args, num_features=nf, image=_gray(frame.image))

        def finish(lane, r):
            out[r]["features"] = pipe.get_features(lane)

        pending = []

        def collect_one():
            t = pending.pop(0)
            rs = pipe.collect_all()
            for lane, e in enumerate(steps[t]):
                if e is not None:
                    o = out[e[0]]
                    o["results"].append(rs[lane])
                    o["trajectory"].append(rs[lane].pose_world_cam())
                    o["n_landmarks"].append(rs[lane].n_landmarks)
            if tap:
                tap.post([(lane, rs[lane], out[e[0]].setdefault("observations", []))
                          for lane, e in enumerate(steps[t]) if e is not None])

        events = {}
        for t, lane, r in plan["starts"]:
            events.setdefault(t, []).append((lane, r))
        for t, lane in plan["idles"]:
            events.setdefault(t, []).append((lane, None))
        slot = 0

        def change(t, slot):
            """Step t's events: lanes going idle, lanes starting a recording (the host route one by one, the device route
            all of them in one call)."""
            starts = [(lane, r) for lane, r in sorted(events[t]) if r is not None]
            for lane, r in sorted(events[t]):
                if r is None:
                    pipe.set_active(lane, False)
                elif not on_device:
                    start(lane, r, t, slot)
            if on_device and starts:
                start_on_device(starts, t, slot)
            return starts

        if 0 in events:
            change(0, slot)
            del events[0]
        for lane, e in enumerate(steps[0]):
            if e is not None:
                put(lane, 1, e[0])
        seconds = []
        for t, row in enumerate(steps):
            if t in events:
                # a lane changes recording: drain, read what ends, then idle / restart (nothing in flight for either)
                while pending:
                    collect_one()
                if tap:
                    tap.flush()                          # (a hand-over rewrites the buffers the posted records read)
                for lane, r in sorted(events[t]):
                    prev = steps[t - 1][lane]
                    if prev is not None:
                        finish(lane, prev[0])
                for lane, r in change(t, slot):
                    put(lane, (slot + 1) % SLOTS, r)
            t0 = time.perf_counter()
            nxt = (slot + 1) % SLOTS
            if len(pending) == 2:
                collect_one()
            ahead = False
            if t + 1 < len(steps):                       # the frames of the NEXT step, for lanes that keep their recording
                for lane, e in enumerate(steps[t + 1]):
                    if e is not None and e[1] > 0:
                        put(lane, (slot + 2) % SLOTS, e[0])
                        ahead = True
            pipe.submit(slot, nxt)
            if ahead:
                pipe.prepare((slot + 2) % SLOTS)
            pending.append(t)
            slot = nxt
            seconds.append(time.perf_counter() - t0)
            for e in row:
                if e is not None:
                    out[e[0]]["frame_seconds"].append(seconds[-1])
        while pending:
            collect_one()
        for lane, e in enumerate(steps[-1]):
            if e is not None:
                finish(lane, e[0])
        if tap:
            tap.close()
        pipe.close()
    for o in out:
        o["trajectory"] = np.array(o["trajectory"])
        o["n_landmarks"] = np.array(o["n_landmarks"])
        o["frame_seconds"] = np.array(o["frame_seconds"])
        if verbose:
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
