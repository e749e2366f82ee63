"""-m gpu: the two-view bootstrap inside the pipeline (vo_pipeline_bootstrap_seq, Pipeline.bootstrap, the drivers'
bootstrap="device").  It runs the kernels of the host route (vo.driver._device_bootstrap + set_state / restart) on the same
inputs, so everything but the 4x4 poses is compared exactly; the poses differ by construction (closed-form inverse of M
against two LAPACK inversions: at most 1.3e-15 / 5.6e-16 over 20 000 random rigid M with |t| = 1) and are held to 1e-13."""
import numpy as np
import pytest

import pipeline_bootstrap_oracle as pbo

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-13
SMALL = dict(H=480, W=640, n=500, win=17, level=2, thr=1.0)
LARGE = dict(H=1241, W=1376, n=2000, win=21, level=3, thr=1.0)       # bench.py's frame and bootstrap settings
SEEDS = (2023, 2030, 2037)


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def recording(cfg, seed, n_frames=4, intrinsics=None):
    from vo.primitives import Sequence
    return Sequence("synthetic", n_frames=n_frames, height=cfg["H"], width=cfg["W"], seed=seed, intrinsics=intrinsics)


def new_pipe(ctx, cfg, K, sequences=1, hyp=1024, **kw):
    """A pipeline as the drivers configure it (klt 17 / 2)."""
    from vo import _native, driver
    args = driver._pipeline_kwargs(None, cfg["n"], 17, 2, hyp, "current")
    args.update(kw)
    return _native.Pipeline(ctx, cfg["H"], cfg["W"], 4, K, sequences=sequences, **args)


def boot_kwargs(cfg):
    return dict(max_corners=cfg["n"], klt_win=cfg["win"], klt_max_level=cfg["level"], threshold_px=cfg["thr"])


def host_route(ctx, cfg, seq):
    """vo.driver._device_bootstrap on a recording: (state, num_features, M, RANSAC inliers, grey frame 2)."""
    from vo import driver
    from vo.landmarks import LandmarksTriangulator
    state, tracker = driver._device_bootstrap(seq, cfg["n"], 17, 2, cfg["win"], cfg["level"], cfg["thr"])
    cam = seq.get_camera()
    tri = LandmarksTriangulator(camera1=cam, camera2=cam, use_ransac=True, use_opencv=True, outlier_ratio=0.9,
                                ransac_threshold=cfg["thr"], ransac_confidence=0.999, context=ctx)
    p1 = state.prev_frame.features.keypoints.astype(np.float64)
    p2 = state.curr_frame.features.keypoints.astype(np.float64)
    F, inl = tri._find_fundamental_matrix_ransac(p1, p2)          # (deterministic: the same calls the bootstrap made)
    M = ctx.relative_pose(p1, p2, cam.intrinsic_matrix, cam.intrinsic_matrix, F, inl)[0]
    return state, tracker._tracker._num_features, M, np.asarray(inl, bool), driver._gray(state.curr_frame.image)


def host_pipe(ctx, cfg, seq, **kw):
    state, nf, M, inl, img = host_route(ctx, cfg, seq)
    pipe = new_pipe(ctx, cfg, seq.get_camera().intrinsic_matrix, **kw)
    pipe.set_frame(0, img)
    pipe.set_state(0, state.curr_frame.features, state.curr_pose, state.prev_pose, num_features=nf)
    return pipe, state, M, inl


def device_pipe(ctx, cfg, seq, **kw):
    from vo import driver
    img0, img2 = driver._bootstrap_frames(seq)
    pipe = new_pipe(ctx, cfg, seq.get_camera().intrinsic_matrix, **kw)
    pipe.set_frame(1, img0)
    pipe.set_frame(0, img2)
    return pipe, pipe.bootstrap(1, 0, **boot_kwargs(cfg))


def same_bootstrap_state(a, b, what):
    """a: the device bootstrap's get_state(), b: the host route's.  Exact but for the poses derived from inv(M)."""
    assert a["n"] == b["n"] and a["num_features"] == b["num_features"], what
    for key in ("keypoints", "state", "candidate_mask", "tracks", "landmarks", "n_iterations", "outlier_ratio", "prev_pose"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)
    d = float(np.max(np.abs(a["curr_pose"] - b["curr_pose"])))
    assert d <= POSE_TOL, (what, "curr_pose", d)
    kept = a["state"] == 2
    assert np.array_equal(a["poses"][kept], b["poses"][kept]), (what, "start poses of the triangulated features")
    if np.any(~kept):
        d = float(np.max(np.abs(a["poses"][~kept] - b["poses"][~kept])))
        assert d <= POSE_TOL, (what, "start poses of the reset features", d)


def fields(r):
    """Every integer field of a record but detector_ran: under look-ahead the detector's decision reads the feature count of
    whichever step has finished when its kernel runs (detect_margin), so it may run on a frame it could have sat out --
    tests/test_gpu_lanes.py leaves it out for the same reason; test 3 (no look-ahead) checks it."""
    return (r.n_features_in, r.redetected, r.n_tracked, r.n_triangulated, r.n_inliers, r.best_index,
            r.hyp_valid, r.ransac_iterations, r.draws_consumed, r.refine_iterations, r.n_candidates, r.n_dropped,
            r.n_landmarks, r.fault, r.recovered, r.raw_pos)


POSES = ("R", "t", "R_refined", "t_refined", "T_wc")


def close_records(got, ref, what, tol=1e-9, names=POSES):
    """Every integer field equal; the pose fields `names` within tol.  R_refined / t_refined / T_wc are the step's pose (what
    a trajectory is made of); R / t are the accepted minimal-sample hypothesis the refinement starts from."""
    assert len(got) == len(ref), what
    worst = dict.fromkeys(POSES, 0.0)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert fields(a) == fields(b), (what, "step", k, fields(a), fields(b))
        for name in POSES:
            d = float(np.max(np.abs(np.array(getattr(a, name)) - np.array(getattr(b, name)))))
            worst[name] = max(worst[name], d)
            assert name not in names or d <= tol, (what, "step", k, name, d)
    print(what, "largest pose differences:", ", ".join("%s %.3g" % kv for kv in worst.items()))


def rng_of(pipe, q=0):
    g = np.random.default_rng(0)
    pipe.rng_state_into(g, seq=q)
    return g.bit_generator.state


CASES = [(SMALL, s) for s in SEEDS] + [(LARGE, 2023)]


@pytest.mark.parametrize("cfg,seed", CASES, ids=["small-%d" % s for s in SEEDS] + ["large-2023"])
def test_equals_the_host_route(ctx, cfg, seed):
    """1. + 7.: pipe.bootstrap(1, 0) against _device_bootstrap + set_state on a second pipeline, through get_state();
    nothing sized by pixels or features crosses PCIe: one batch of 2048 samples up, its counts down, scalars."""
    ref_pipe, state, M, inl = host_pipe(ctx, cfg, recording(cfg, seed))
    pipe, res = device_pipe(ctx, cfg, recording(cfg, seed))
    a, b = pipe.get_state(), ref_pipe.get_state()
    print("%dx%d seed %d: %d corners, %d tracked, %d RANSAC inliers, %d landmarks, %d iterations, h2d %d B, d2h %d B" % (
        cfg["H"], cfg["W"], seed, res.n_corners, res.n_tracked, res.n_ransac_inliers, res.n_landmarks,
        res.ransac_iterations, res.bytes_h2d, res.bytes_d2h))
    same_bootstrap_state(a, b, (cfg["H"], seed))
    assert res.n_corners == b["num_features"] and res.n_tracked == b["n"] == res.n_features
    assert res.n_tracked == state.bootstrap_info["correspondences"]
    assert res.n_ransac_inliers == int(inl.sum())
    assert res.n_landmarks == int(np.sum(b["state"] == 2)) == state.bootstrap_info["inliers"]
    assert np.array_equal(res.relative_pose(), M)
    pbo.check_invariants(pipe.get_features(), a["curr_pose"])
    assert res.bytes_h2d <= 64 * 1024 + 4 * 1024 and res.bytes_d2h <= 8 * 1024 + 4 * 1024
    pipe.close()
    ref_pipe.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_equals_the_oracle(ctx, seed):
    """2. the small cases against tests/pipeline_bootstrap_oracle.py: counts, keypoints, state codes and the RANSAC inlier
    count / final mask exactly, M at 1e-9 and landmarks at 1e-7 (the bars the bootstrap kernels meet against their oracles)."""
    from vo import driver
    cfg = SMALL
    seq = recording(cfg, seed)
    img0, img2 = driver._bootstrap_frames(recording(cfg, seed))
    o = pbo.bootstrap(img0, img2, seq.get_camera().intrinsic_matrix, max_corners=cfg["n"], win=cfg["win"],
                      max_level=cfg["level"], threshold_px=cfg["thr"])
    pipe, res = device_pipe(ctx, cfg, seq)
    st = pipe.get_state()
    f = o["features"]
    assert (res.n_corners, res.n_tracked, res.n_ransac_inliers) == (o["n_corners"], o["n_tracked"], int(o["ransac_inliers"].sum()))
    assert res.ransac_iterations == o["iterations"]
    assert np.array_equal(st["keypoints"], np.asarray(f.keypoints).astype(np.float64))
    assert np.array_equal(st["state"], np.asarray(f.state))
    assert np.array_equal(st["state"] == 2, o["mask"])
    assert np.array_equal(st["tracks"], np.asarray(f.tracks).astype(np.float64))
    assert np.max(np.abs(res.relative_pose() - o["M"])) <= 1e-9
    kept = st["state"] == 2
    got_X, ref_X = st["landmarks"][kept], np.asarray(f.landmarks)[kept]
    excess = np.abs(got_X - ref_X) - 1e-7 * np.abs(ref_X)
    print("seed %d: M off by %.3g, landmarks by %.3g absolute (largest |X| %.3g), %.3g beyond rtol" % (
        seed, np.max(np.abs(res.relative_pose() - o["M"])), np.max(np.abs(got_X - ref_X)), np.max(np.abs(ref_X)), np.max(excess)))
    assert np.allclose(got_X, ref_X, rtol=1e-7, atol=1e-7)           # (the bar of tests/test_gpu_api.py for vo_relative_pose's X)
    assert np.max(np.abs(st["curr_pose"] - o["curr_pose"])) <= 1e-9
    pipe.close()


def test_the_pipeline_goes_on_from_it(ctx):
    """3. four steps after bootstrap against four steps of the host-bootstrapped pipeline: integer fields equal, poses
    within 1e-9; the first step shows that pyramid, detection, RANSAC fields and generator were set as by set_state."""
    from vo import driver
    cfg, seed, steps = SMALL, 2023, 4

    def frames():
        seq = recording(cfg, seed, n_frames=3 + steps)
        for _ in range(3):
            next(seq)
        return [driver._gray(next(seq).image) for _ in range(steps)]

    runs = []
    for make in (host_pipe, device_pipe):
        pipe = make(ctx, cfg, recording(cfg, seed, n_frames=3 + steps))[0]
        before = rng_of(pipe)
        recs = []
        for k, img in enumerate(frames()):
            pipe.set_frame((k + 1) % 4, img)
            recs.append(pipe.step(k % 4, (k + 1) % 4))
        runs.append((recs, before, rng_of(pipe), pipe.get_state()))
        pipe.close()
    (ref, ref_before, ref_after, ref_state), (got, got_before, got_after, got_state) = runs
    close_records(got, ref, "after the bootstrap")
    assert [r.detector_ran for r in got] == [r.detector_ran for r in ref]
    assert got[0].n_features_in == ref[0].n_features_in and got[0].detector_ran == ref[0].detector_ran
    assert got_before == ref_before and got_after == ref_after
    assert got_state["n"] == ref_state["n"] and np.array_equal(got_state["state"], ref_state["state"])
    assert np.array_equal(got_state["keypoints"], ref_state["keypoints"])


def test_lane_bootstrap_leaves_other_lanes_alone(ctx):
    """4. S = 3 with look-ahead and prepare; drain; lane 1 idle, its two frames replaced, bootstrap(seq=1) with a given
    generator.  Lanes 0 and 2 are bit-identical to the run without it; lane 1 equals a fresh one-sequence pipeline
    bootstrapped the same way."""
    from test_gpu_lanes import drive, same_records, same_state
    from pipeline_oracle import initial_features
    from vo import _native, synthetic
    H, W, N, HYP, S, F, at = 240, 320, 300, 256, 3, 5, 5
    kw = dict(n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP, p3p_threshold=1.0, max_iterations=1000, refine_iters=20)
    boot = dict(max_corners=N, klt_win=17, klt_max_level=2, threshold_px=1.0)
    streams = [synthetic.Stream(F, H, W, seed=2023 + 3 * q, start=q) for q in range(S)]
    other = synthetic.Stream(F, H, W, seed=2099, start=7)
    order = streams[0].order(10)
    pairs = list(zip(order[:-1], order[1:]))
    starts = [initial_features(streams[q], 0, N) for q in range(S)]

    def fresh():
        pipe = _native.Pipeline(ctx, H, W, F, streams[0].K, sequences=S, **kw)
        for q in range(S):
            for i in range(F):
                pipe.set_frame(i, streams[q].image(i), seq=q)
            pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
        return pipe

    base_pipe = fresh()
    base = drive(base_pipe, pairs, True, at={at: lambda: None})
    base_state = [base_pipe.get_state(seq=q) for q in range(S)]
    base_rng = [rng_of(base_pipe, q) for q in range(S)]
    base_pipe.close()

    idx = pairs[at][0]                       # the slot the step after the drain starts from
    idx_a = next(i for i in range(F) if i != idx and i != pairs[at][1])
    pipe = fresh()
    seen = {}

    def restart():
        pipe.set_active(1, False)
        for i in range(F):                   # the lane's whole frame store now holds the other recording
            pipe.set_frame(i, other.image(i), seq=1)
        pipe.set_frame(idx_a, other.image(0), seq=1)        # (frame a: any other slot; put back below)
        seen["res"] = pipe.bootstrap(idx_a, idx, seq=1, generator=np.random.default_rng(99), **boot)
        seen["state"] = pipe.get_state(seq=1)
        pipe.set_frame(idx_a, other.image(idx_a), seq=1)

    got = drive(pipe, pairs, True, at={at: restart})
    for q in (0, 2):
        same_records([g[q] for g in got], [b[q] for b in base], ("lane", q))
        same_state(pipe.get_state(seq=q), base_state[q], ("lane", q))
        assert rng_of(pipe, q) == base_rng[q]
    same_records([g[1] for g in got[:at]], [b[1] for b in base[:at]], "lane 1 before its bootstrap")
    # the reference: a one-sequence pipeline over the other recording, bootstrapped the same way at the same slots
    ref = _native.Pipeline(ctx, H, W, F, other.K, **kw)
    ref.seed(np.random.default_rng(99))
    for i in range(F):
        ref.set_frame(i, other.image(i))
    ref.set_frame(idx_a, other.image(0))
    res = ref.bootstrap(idx_a, idx, **boot)
    same_state(seen["state"], ref.get_state(), "lane 1 after its bootstrap")
    assert (res.n_corners, res.n_tracked, res.n_landmarks) == (seen["res"].n_corners, seen["res"].n_tracked, seen["res"].n_landmarks)
    assert res.n_landmarks >= 8
    ref.set_frame(idx_a, other.image(idx_a))
    ref_recs = [ref.step(a, b) for a, b in pairs[at:]]
    same_records([g[1] for g in got[at:]], ref_recs, "lane 1 after its bootstrap")
    same_state(pipe.get_state(seq=1), ref.get_state(), "lane 1")
    assert rng_of(pipe, 1) == rng_of(ref)
    ref.close()
    pipe.close()


def close_runs(got, ref, what):
    assert len(got["results"]) == len(ref["results"]), what
    # (the trajectory is made of the refined poses; the accepted P3P hypothesis of three landmarks, printed with them, is
    #  not part of it: measured up to 1.6e-9 apart on a restarted lane's third step, with every integer field equal)
    close_records(got["results"], ref["results"], what, names=("R_refined", "t_refined", "T_wc"))
    assert np.array_equal(got["n_landmarks"], ref["n_landmarks"]), what
    assert got["trajectory"].shape == ref["trajectory"].shape
    assert np.max(np.abs(got["trajectory"] - ref["trajectory"])) <= 1e-9, what
    assert got["features"].length == ref["features"].length
    assert np.array_equal(got["features"].keypoints, ref["features"].keypoints), what
    assert np.array_equal(got["features"].state, ref["features"].state), what


def test_run_on_device_with_the_device_bootstrap(ctx):
    """5a. run_on_device(bootstrap="device") against bootstrap="host": same integer results, trajectory within 1e-9."""
    from vo import driver
    kw = dict(n_keypoints=500, hyp=1024, context=ctx, bootstrap_threshold=1.0)
    ref = driver.run_on_device(recording(SMALL, 2023, n_frames=12), **kw)
    got = driver.run_on_device(recording(SMALL, 2023, n_frames=12), bootstrap="device", **kw)
    assert set(got) == set(ref)
    close_runs(got, ref, "run_on_device")


def test_batch_driver_with_the_device_bootstrap(ctx):
    """5b. run_batch_on_device(bootstrap="device"): five recordings through three lanes, two cameras (the recordings of
    test_batch_driver_equals_one_recording_at_a_time), per recording what bootstrap="host" gives."""
    from vo import driver, synthetic
    Kb = synthetic.intrinsics(480, 640).copy()
    Kb[0, 0] *= 0.92
    Kb[1, 1] *= 0.92
    Kb[0, 2] += 6.0
    Kb[1, 2] -= 4.0
    lengths = (9, 14, 6, 20, 11)

    def recordings():
        return [recording(SMALL, 2023 + 11 * i, n_frames=n + 3, intrinsics=Kb if i % 2 else None)
                for i, n in enumerate(lengths)]

    kw = dict(n_keypoints=500, hyp=1024, context=ctx, bootstrap_threshold=1.0)
    ref = driver.run_batch_on_device(recordings(), lanes=3, **kw)
    got = driver.run_batch_on_device(recordings(), lanes=3, bootstrap="device", **kw)
    assert len(got) == len(ref) == len(lengths)
    for i in range(len(lengths)):
        assert set(got[i]) == set(ref[i]), i
        assert len(got[i]["results"]) == lengths[i]
        close_runs(got[i], ref[i], ("recording", i))


def test_refusals_and_failures(ctx):
    """6. refused with a message, nothing changed: steps in flight, idx_b not the slot the next step starts from, idx_a ==
    idx_b, a sequence the pipeline does not have, a descriptor tracker mode.  Two flat images return an error and leave
    the lane's previous state readable and able to step."""
    from vo import _native, driver
    cfg, seed = SMALL, 2023
    seq = recording(cfg, seed, n_frames=6)
    frames = [driver._gray(next(seq).image) for _ in range(6)]
    pipe = new_pipe(ctx, cfg, seq.get_camera().intrinsic_matrix)
    pipe.set_frame(1, frames[0])
    pipe.set_frame(0, frames[2])
    for args, kw in (((0, 0), {}), ((1, 0), dict(seq=1)), ((1, 0), dict(seq=-1)), ((1, 7), {})):
        with pytest.raises(_native.VoError):
            pipe.bootstrap(*args, **kw)
    pipe.bootstrap(1, 0, **boot_kwargs(cfg))
    pipe.set_frame(1, frames[3])
    pipe.set_frame(2, frames[4])
    pipe.submit(0, 1)
    with pytest.raises(_native.VoError, match="not collected"):
        pipe.bootstrap(3, 1, **boot_kwargs(cfg))
    first = pipe.collect()
    with pytest.raises(_native.VoError, match="next step starts from"):
        pipe.bootstrap(3, 2, **boot_kwargs(cfg))             # (a running pipeline: idx_b must be slot 1)
    # two flat images: no corners -> an error, the lane as it was
    before, rng_before = pipe.get_state(), rng_of(pipe)
    pipe.set_frame(3, np.full((cfg["H"], cfg["W"]), 128, np.uint8))
    pipe.set_active(0, False)
    pipe.set_frame(1, np.full((cfg["H"], cfg["W"]), 128, np.uint8))
    with pytest.raises(_native.VoError) as e:
        pipe.bootstrap(3, 1, **boot_kwargs(cfg))
    assert e.value.code == -5 and "corners" in str(e.value)
    after = pipe.get_state()
    for key in ("keypoints", "state", "candidate_mask", "landmarks", "tracks", "poses", "curr_pose", "prev_pose", "n_iterations"):
        assert np.array_equal(after[key], before[key], equal_nan=True), key
    assert rng_of(pipe) == rng_before
    # ... and able to step: the lane comes back with its own frame and the state it had
    f = pipe.get_features()
    pipe.restart(0, 1, f, before["curr_pose"], before["prev_pose"], num_features=before["num_features"], image=frames[3])
    r = pipe.step(1, 2)
    assert r.fault == 0 and r.n_tracked > 0 and r.n_landmarks >= 8 and first.n_landmarks >= 8
    pipe.close()
    sift = _native.Pipeline(ctx, cfg["H"], cfg["W"], 4, seq.get_camera().intrinsic_matrix, n_keypoints=cfg["n"], tracker="harris")
    sift.set_frame(1, frames[0])
    sift.set_frame(0, frames[2])
    with pytest.raises(_native.VoError, match="KLT tracker mode"):
        sift.bootstrap(1, 0)
    sift.close()
