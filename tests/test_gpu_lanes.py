"""-m gpu: lanes -- many recordings through one pipeline (vo_pipeline_set_camera_seq / _restart_seq / _set_active_seq,
vo.driver.run_batch_on_device).  Every lane must compute exactly what a one-sequence pipeline computes for its recording
alone, and a lane's restart or idle spell must leave the other lanes' results unchanged."""
import numpy as np
import pytest

from pipeline_oracle import initial_features

pytestmark = pytest.mark.gpu

H, W, N, HYP = 240, 320, 300, 256


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def fields(r):
    return (r.n_features_in, r.redetected, r.n_tracked, r.n_triangulated, r.n_inliers, r.ransac_iterations,
            r.draws_consumed, r.n_candidates, r.n_dropped, r.n_landmarks, tuple(r.R), tuple(r.t), tuple(r.R_refined),
            tuple(r.t_refined), tuple(r.T_wc))


def camera(q):
    """Intrinsics that differ per recording in focal length and principal point."""
    from vo import synthetic
    K = synthetic.intrinsics(H, W).copy()
    K[0, 0] *= (1.0, 0.9, 1.12, 0.95)[q % 4]
    K[1, 1] *= (1.0, 0.9, 1.12, 0.97)[q % 4]
    K[0, 2] += (0.0, 7.5, -6.0, 3.0)[q % 4]
    K[1, 2] += (0.0, -5.0, 4.5, -2.0)[q % 4]
    return K


def single(ctx, stream, start_idx, feats, T, pairs, K=None, generator=None, **kw):
    """A one-sequence pipeline from (feats, T) at frame start_idx: records, final state, generator state."""
    from vo import _native
    pipe = _native.Pipeline(ctx, H, W, stream.n, stream.K if K is None else K, n_keypoints=N, klt_win=15, klt_max_level=2,
                            hyp=HYP, p3p_threshold=1.0, max_iterations=1000, refine_iters=20, **kw)
    if generator is not None:
        pipe.seed(generator)
    for i in range(stream.n):
        pipe.set_frame(i, stream.image(i))
    pipe.set_state(start_idx, feats, T, T)
    res = [pipe.step(a, b) for a, b in pairs]
    out = (res, pipe.get_state(), rng_of(pipe, 0))
    pipe.close()
    return out


def rng_of(pipe, q):
    g = np.random.default_rng(0)
    pipe.rng_state_into(g, seq=q)
    return g.bit_generator.state


def same_state(a, b, what):
    for key in ("keypoints", "state", "candidate_mask", "landmarks", "tracks", "poses", "curr_pose", "n_iterations"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def same_records(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        fa, fb = fields(a), fields(b)
        assert fa == fb, (what, "step", k, [(i, fa[i], fb[i]) for i in range(len(fa)) if fa[i] != fb[i]][:3])


def multi(ctx, streams, S, **kw):
    from vo import _native
    pipe = _native.Pipeline(ctx, H, W, streams[0].n, streams[0].K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP,
                            p3p_threshold=1.0, max_iterations=1000, refine_iters=20, sequences=S, **kw)
    for q in range(S):
        for i in range(streams[q].n):
            pipe.set_frame(i, streams[q].image(i), seq=q)
    return pipe


def drive(pipe, pairs, lookahead, at=None, prepare=True):
    """Runs the pairs; with lookahead in the driver's call order (submit, submit, prepare, collect).  at: {step: fn}
    called with nothing in flight before that step is submitted (the driver drains first).  prepare=False: no
    vo_pipeline_prepare hints (a step redone through the host path while a hint has been given re-tracks from the
    hinted frame's pyramid -- DESIGN.md 6, a gap of the frame loop this file does not cover)."""
    at = at or {}
    out, pending = [], []
    for k, (a, b) in enumerate(pairs):
        if k in at:
            while pending:
                out.append(pipe.collect_all())
                pending.pop()
            at[k]()
        if lookahead and len(pending) == 2:
            out.append(pipe.collect_all())
            pending.pop()
        pipe.submit(a, b)
        pending.append(k)
        if prepare and lookahead and k + 1 < len(pairs) and k + 1 not in at:
            pipe.prepare(pairs[k + 1][1])
        if not lookahead:
            out.append(pipe.collect_all())
            pending.pop()
    while pending:
        out.append(pipe.collect_all())
        pending.pop()
    return out


@pytest.mark.parametrize("lookahead,fault_every", [(False, 0), (True, 0), (True, 3)])
def test_per_lane_camera_equals_single_pipelines(ctx, lookahead, fault_every):
    """S = 3 recordings seen through three different cameras in one pipeline (set_camera): every lane's records, final
    Features / State and generator equal a one-sequence pipeline created with that camera -- also with steps forced
    through the host recovery path, which must use the lane's camera too."""
    from vo import synthetic
    S, F = 3, 5
    streams = [synthetic.Stream(F, H, W, seed=2023 + 5 * q, start=q, K=camera(q)) for q in range(S)]
    order = streams[0].order(9)
    pairs = list(zip(order[:-1], order[1:]))
    starts = [initial_features(streams[q], 0, N) for q in range(S)]
    kw = dict(debug_fault_every=fault_every) if fault_every else {}
    ref = [single(ctx, streams[q], 0, starts[q][0], starts[q][1], pairs, **kw) for q in range(S)]
    pipe = multi(ctx, streams, S, **kw)
    for q in range(S):
        pipe.set_camera(streams[q].K, q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    got = drive(pipe, pairs, lookahead, prepare=not fault_every)
    for q in range(S):
        same_records([g[q] for g in got], ref[q][0], ("lane", q))
        same_state(pipe.get_state(seq=q), ref[q][1], ("lane", q))
        assert rng_of(pipe, q) == ref[q][2]
    if fault_every:                  # (the host path ran on every lane, with that lane's camera: the records above are equal)
        assert all(any(g[q].recovered for g in got) for q in range(S))
    pipe.close()


def test_restart_leaves_other_lanes_alone(ctx):
    """4 lanes; lane 2 is restarted before step 5 with another recording's start state and generator (look-ahead with
    prepare, then drain and restart).  Lanes 0, 1, 3 are bit-identical to the run without the restart; lane 2 from the
    restart on equals a fresh one-sequence pipeline started from that state with that generator."""
    from vo import synthetic
    S, F, at = 4, 5, 5
    streams = [synthetic.Stream(F, H, W, seed=2023 + 3 * q, start=q) for q in range(S)]
    other = synthetic.Stream(F, H, W, seed=2099, start=7)
    order = streams[0].order(10)
    pairs = list(zip(order[:-1], order[1:]))
    starts = [initial_features(streams[q], 0, N) for q in range(S)]

    def fresh():
        pipe = multi(ctx, streams, S)
        for q in range(S):
            pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
        return pipe

    base_pipe = fresh()
    base = drive(base_pipe, pairs, True, at={at: lambda: None})
    base_state = [base_pipe.get_state(seq=q) for q in range(S)]
    base_rng = [rng_of(base_pipe, q) for q in range(S)]
    base_pipe.close()

    idx = pairs[at][0]
    f2, T2 = initial_features(other, idx, N)
    pipe = fresh()

    def restart():
        for i in range(F):
            if i != idx:
                pipe.set_frame(i, other.image(i), seq=2)
        pipe.restart(2, idx, f2, T2, T2, generator=np.random.default_rng(99), image=other.image(idx))

    got = drive(pipe, pairs, True, at={at: restart})
    for q in (0, 1, 3):
        same_records([g[q] for g in got], [b[q] for b in base], ("lane", q))
        same_state(pipe.get_state(seq=q), base_state[q], ("lane", q))
        assert rng_of(pipe, q) == base_rng[q]
    same_records([g[2] for g in got[:at]], [b[2] for b in base[:at]], "lane 2 before the restart")
    ref = single(ctx, other, idx, f2, T2, pairs[at:], generator=np.random.default_rng(99))
    same_records([g[2] for g in got[at:]], ref[0], "lane 2 after the restart")
    same_state(pipe.get_state(seq=2), ref[1], "lane 2")
    assert rng_of(pipe, 2) == ref[2]
    pipe.close()


def test_idle_lane_does_nothing_and_comes_back_through_restart(ctx):
    """Lane 1 idle for steps 3..8, restarted before step 9: lanes 0 and 2 equal the run in which lane 1 was always
    active; lane 1's records of steps 3..8 carry the idle marker and its generator does not move; after the restart (no
    generator given: the pipeline's seed) lane 1 equals a fresh pipeline started from that state."""
    from vo import synthetic
    S, F = 3, 5
    streams = [synthetic.Stream(F, H, W, seed=2030 + 3 * q, start=2 * q) for q in range(S)]
    order = streams[0].order(12)
    pairs = list(zip(order[:-1], order[1:]))
    starts = [initial_features(streams[q], 0, N) for q in range(S)]

    def fresh():
        pipe = multi(ctx, streams, S)
        for q in range(S):
            pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
        return pipe

    base_pipe = fresh()
    base = drive(base_pipe, pairs, True)
    base_state = [base_pipe.get_state(seq=q) for q in (0, 2)]
    base_pipe.close()

    idx = pairs[9][0]
    f1, T1 = initial_features(streams[1], idx, N)
    pipe = fresh()
    seen = {}

    def idle():
        seen["before"] = rng_of(pipe, 1)
        pipe.set_active(1, False)
        with pytest.raises(Exception):
            pipe.set_active(1, True)       # (an idle lane comes back through restart only)

    def restart():
        seen["after"] = rng_of(pipe, 1)
        pipe.restart(1, idx, f1, T1, T1)

    got = drive(pipe, pairs, True, at={3: idle, 9: restart})
    for q, st in zip((0, 2), base_state):
        same_records([g[q] for g in got], [b[q] for b in base], ("lane", q))
        same_state(pipe.get_state(seq=q), st, ("lane", q))
    same_records([g[1] for g in got[:3]], [b[1] for b in base[:3]], "lane 1 before idling")
    for k in range(3, 9):
        r = got[k][1]
        assert r.idle and r.n_features_in == -1 and r.fault == 256 and r.recovered == 0 and r.draws_consumed == 0, k
    assert not any(got[k][q].idle for k in range(len(pairs)) for q in (0, 2))
    assert seen["before"] == seen["after"], "an idle lane's generator moved"
    ref = single(ctx, streams[1], idx, f1, T1, pairs[9:])
    same_records([g[1] for g in got[9:]], ref[0], "lane 1 after the restart")
    same_state(pipe.get_state(seq=1), ref[1], "lane 1")
    pipe.close()


def test_mixed_pinned_and_plain_uploads_into_one_slot(ctx):
    """S = 2: lane 0's frames uploaded from pinned memory, lane 1's through the staging copy, into the same slots -- the
    records equal those of uniform uploads (the pyramid and the detector wait for both kinds of copy)."""
    from vo import synthetic
    S, F = 2, 5
    streams = [synthetic.Stream(F, H, W, seed=2040 + q, start=q) for q in range(S)]
    order = streams[0].order(8)
    pairs = list(zip(order[:-1], order[1:]))
    starts = [initial_features(streams[q], 0, N) for q in range(S)]
    runs = []
    for mixed in (False, True):
        from vo import _native
        pipe = _native.Pipeline(ctx, H, W, F, streams[0].K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP,
                                p3p_threshold=1.0, max_iterations=1000, refine_iters=20, sequences=S)
        pinned = [ctx.pinned_empty((H, W)) for _ in range(F)]
        for i in range(F):
            if mixed:
                pinned[i][...] = streams[0].image(i)
                pipe.set_frame(i, pinned[i], seq=0, pinned=True)
            else:
                pipe.set_frame(i, streams[0].image(i), seq=0, pinned=False)
            pipe.set_frame(i, streams[1].image(i), seq=1, pinned=False)
        for q in range(S):
            pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
        runs.append(drive(pipe, pairs, True))
        assert all(pipe.frame_uploaded(i) for i in range(F))
        pipe.close()
    for q in range(S):
        same_records([g[q] for g in runs[1]], [g[q] for g in runs[0]], ("lane", q))


def test_batch_driver_equals_one_recording_at_a_time(ctx):
    """run_batch_on_device: 5 recordings (9 / 14 / 6 / 20 / 11 frames after the bootstrap, two cameras) through 3 lanes
    give, recording by recording, what run_on_device gives for each alone."""
    from vo import driver
    from vo.primitives import Sequence
    from vo import synthetic
    Kb = synthetic.intrinsics(480, 640).copy()
    Kb[0, 0] *= 0.92
    Kb[1, 1] *= 0.92
    Kb[0, 2] += 6.0
    Kb[1, 2] -= 4.0
    lengths = (9, 14, 6, 20, 11)

    def recordings():
        return [Sequence("synthetic", n_frames=n + 3, height=480, width=640, seed=2023 + 11 * i,
                         intrinsics=Kb if i % 2 else None) for i, n in enumerate(lengths)]

    kw = dict(n_keypoints=500, hyp=1024, context=ctx)
    got = driver.run_batch_on_device(recordings(), lanes=3, **kw)
    assert len(got) == len(lengths)
    for i, seq in enumerate(recordings()):
        ref = driver.run_on_device(seq, **kw)
        assert set(got[i]) == set(ref), i
        assert len(got[i]["results"]) == lengths[i]
        assert np.array_equal(got[i]["trajectory"], ref["trajectory"]), i
        assert np.array_equal(got[i]["n_landmarks"], ref["n_landmarks"]), i
        same_records(got[i]["results"], ref["results"], ("recording", i))
        assert got[i]["features"].length == ref["features"].length
        assert np.array_equal(got[i]["features"].keypoints, ref["features"].keypoints), i
