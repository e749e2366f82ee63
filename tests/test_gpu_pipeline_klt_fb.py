"""-m gpu: the frame loop with the tracker's forward-backward check (vo_pipeline_set_klt_fb) against the CPU oracle of the
same loop (tests/klt_fb_oracle.py: FBOracleLoop, the plain oracle loop whose tracker makes the forward-backward call) --
240 x 320, 300 keypoints, eight steps with a re-detect among them; through the host path, with two sequences, switched off
again, refused where it does not belong, and through the drivers."""
import numpy as np
import pytest

from test_gpu_pipeline import check_state, check_step, fields, make_pipe, run_all
from test_klt_fb_host import LOOP, loop_start, oracle_loop

pytestmark = pytest.mark.gpu
P = LOOP


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def start():
    stream, feats, T = loop_start()
    order = stream.order(P["steps"])
    return stream, feats, T, list(zip(order[:-1], order[1:]))


def fb_pipe(ctx, stream, feats, T, fb_max=P["fb_max"], win=P["win"], **kw):
    pipe = make_pipe(ctx, stream, P["N"], P["hyp"], win=win, lvl=P["lvl"], redetect_start_pose=P["redetect"], **kw)
    if fb_max is not None:
        pipe.set_klt_fb(fb_max)
    pipe.set_state(0, feats, T, T)
    return pipe


def finish(pipe, q=0):
    g = np.random.default_rng(0)
    pipe.rng_state_into(g, seq=q)
    return pipe.get_state(seq=q), g.bit_generator.state


def same_state(a, b):
    for k in ("keypoints", "state", "candidate_mask", "landmarks", "tracks", "poses", "curr_pose"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.fixture(scope="module")
def blocking(ctx, start):
    """The FB loop step by step on the device: records, final state, generator."""
    stream, feats, T, pairs = start
    pipe = fb_pipe(ctx, stream, feats, T)
    res = run_all(pipe, pairs, False)
    out = (res,) + finish(pipe)
    pipe.close()
    return out


def test_fb_loop_matches_the_fb_oracle_loop(ctx, start):
    """Every integer of every step record, every carried array, the generator; poses within check_step's tolerances (those
    of tests/test_gpu_pipeline.py for the plain loop)."""
    stream, feats, T, pairs = start
    pipe = fb_pipe(ctx, stream, feats, T)
    assert pipe.klt_fb == P["fb_max"]
    orc = oracle_loop(stream, P["fb_max"])
    orc.set_state(0, feats, T, T)
    check_state(pipe.get_state(), feats, T)
    redetects = 0
    for a, b in pairs:
        ref = orc.step(b)
        r = pipe.step(a, b)
        redetects += r.redetected
        assert r.recovered == 0 and r.n_features_in == ref["n_before"] + (P["N"] if r.redetected else 0)
        check_step(r, ref, pipe, orc.rs.rng)
    assert redetects >= 1, "a re-detect was meant to run"
    assert sum(1 for n in orc.tracker._ctx.rejected if n >= 1) >= 2
    pipe.close()


def test_fb_loop_differs_from_the_plain_loop(ctx, start, blocking):
    stream, feats, T, pairs = start
    pipe = fb_pipe(ctx, stream, feats, T, fb_max=None)
    assert pipe.klt_fb == 0.0
    plain = run_all(pipe, pairs, False)
    pipe.close()
    assert plain[0].n_tracked > blocking[0][0].n_tracked, "the check drops features at the first step"


@pytest.mark.parametrize("lookahead", [False, True])
def test_fb_loop_through_the_host_path(ctx, start, blocking, lookahead):
    """debug_fault_every = 3: steps 2 and 5 leave the device-only path behind the regroup and are redone by the host path,
    which tracks through the same forward-backward launch."""
    stream, feats, T, pairs = start
    pipe = fb_pipe(ctx, stream, feats, T, debug_fault_every=3)
    got = run_all(pipe, pairs, lookahead)
    st, g = finish(pipe)
    pipe.close()
    if not lookahead:
        assert all(got[k].recovered == 1 for k in range(2, len(pairs), 3))
    else:
        # (a step that takes the host path by itself -- a re-detect whose keypoints were not made ahead of time -- has the
        #  step submitted behind it enqueued again without the hook, so the forced steps need not be 2 and 5 here)
        assert sum(r.recovered for r in got) >= 2
    for k, (a, b) in enumerate(zip(got, blocking[0])):
        assert fields(a) == fields(b), ("step", k, "recovered", a.recovered)
    same_state(st, blocking[1])
    assert g == blocking[2]


def test_lookahead_equals_blocking_steps(ctx, start, blocking):
    stream, feats, T, pairs = start
    pipe = fb_pipe(ctx, stream, feats, T)
    got = run_all(pipe, pairs, True)
    st, g = finish(pipe)
    pipe.close()
    for k, (a, b) in enumerate(zip(got, blocking[0])):
        assert fields(a) == fields(b), ("step", k)
    same_state(st, blocking[1])
    assert g == blocking[2]


def test_two_sequences_equal_each_run_alone(ctx, start, blocking):
    """sequences = 2: the stream above and another scene from another start; fb strides like err."""
    two_sequences_equal_each_run_alone(ctx, start, blocking, P["win"], P["fb_max"])


def two_sequences_equal_each_run_alone(ctx, start, blocking, win, fb_max, device_only=False, **pipe_kw):
    """blocking: (records, state, generator) of `start`'s sequence run alone at this window and threshold (None: plain).
    pipe_kw: further pipeline settings of every run; device_only: no step of any run may take the host path, and each
    sequence re-detects."""
    import copy
    from pipeline_oracle import initial_features
    from vo import _native, synthetic
    stream, feats, T, pairs = start
    other = synthetic.Stream(P["F"], P["H"], P["W"], seed=2030, start=1)
    f1, T1 = initial_features(other, 0, P["N"])
    f1 = copy.deepcopy(f1)
    alone = fb_pipe(ctx, other, f1, T1, fb_max=fb_max, win=win, **pipe_kw)
    res1 = run_all(alone, pairs, False)
    st1, g1 = finish(alone)
    alone.close()
    pipe = _native.Pipeline(ctx, P["H"], P["W"], P["F"], stream.K, n_keypoints=P["N"], klt_win=win, klt_max_level=P["lvl"],
                            hyp=P["hyp"], p3p_threshold=1.0, max_iterations=1000, refine_iters=20, sequences=2,
                            redetect_start_pose=P["redetect"], **pipe_kw)
    if fb_max is not None:
        pipe.set_klt_fb(fb_max)
    for q, (s, f, t) in enumerate(((stream, feats, T), (other, f1, T1))):
        for i in range(P["F"]):
            pipe.set_frame(i, s.image(i), seq=q)
        pipe.set_state(0, f, t, t, seq=q)
    got = []
    pipe.submit(*pairs[0])
    for k in range(len(pairs)):
        if k + 1 < len(pairs):
            pipe.submit(*pairs[k + 1])
        got.append(pipe.collect_all())
    for q, (res, st_ref, g_ref) in enumerate((blocking, (res1, st1, g1))):
        for k in range(len(pairs)):
            assert fields(got[k][q]) == fields(res[k]), ("sequence", q, "step", k)
            assert not device_only or (got[k][q].recovered == 0 and res[k].recovered == 0), ("sequence", q, "step", k)
        assert not device_only or sum(r.redetected for r in res) >= 1, ("sequence", q)
        st, g = finish(pipe, q)
        same_state(st, st_ref)
        assert g == g_ref
    pipe.close()


def test_switching_the_check_off_gives_the_pipeline_that_never_had_it(ctx, start):
    stream, feats, T, pairs = start

    def run(toggle):
        pipe = fb_pipe(ctx, stream, feats, T, fb_max=None)
        if toggle:
            pipe.set_klt_fb(2.0)
            assert pipe.klt_fb == 2.0
            pipe.set_klt_fb(0)
            assert pipe.klt_fb == 0.0
        res = run_all(pipe, pairs, True)
        out = (res,) + finish(pipe)
        pipe.close()
        return out

    never, toggled = run(False), run(True)
    for k, (a, b) in enumerate(zip(toggled[0], never[0])):
        assert fields(a) == fields(b), ("step", k)
    same_state(toggled[1], never[1])
    assert toggled[2] == never[2]


def test_setter_is_refused_where_it_does_not_belong(ctx, start):
    from vo import _native
    stream, feats, T, pairs = start
    pipe = fb_pipe(ctx, stream, feats, T, fb_max=None)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="fb_max"):
            pipe.set_klt_fb(bad)
        rc = ctx._lib.vo_pipeline_set_klt_fb(pipe._h, bad)            # (the library's own check)
        assert rc != 0
        with pytest.raises(_native.VoError, match="fb_max"):
            ctx._chk(rc)
    pipe.submit(*pairs[0])
    with pytest.raises(_native.VoError, match="not collected"):
        pipe.set_klt_fb(1.0)
    assert pipe.klt_fb == 0.0
    pipe.collect()
    pipe.set_klt_fb(1.0)
    assert pipe.klt_fb == 1.0
    pipe.close()
    for mode in ("sift", "harris"):
        other = _native.Pipeline(ctx, P["H"], P["W"], 3, stream.K, n_keypoints=P["N"], hyp=P["hyp"], tracker=mode)
        with pytest.raises(_native.VoError, match="KLT tracker mode"):
            other.set_klt_fb(1.0)
        assert other.klt_fb == 0.0                                     # (the object survives the refusal)
        other.close()


# ---- the drivers ----
# The recording and threshold are chosen so that no step of either run re-detects (480 x 640, 300 keypoints, seven steps,
# fb_max = +inf: the check drops what the backward pass loses, 2 to 8 features per step).  The driver submits a step ahead
# and gives vo_pipeline_prepare hints; a re-detect the pipeline could not predict -- the first step at 1 px drops a third
# of this recording's bootstrap features at once -- sends a step through the host path, where a pipeline that was given
# hints re-tracks from the hinted frame's pyramid (an open gap of the frame loop, with or without
# this check), so a by-hand loop without hints would not be the same computation.

STEPS, KLT_WIN, KLT_MAX_LEVEL, HYP = 7, 17, 2, 4000               # (tests/test_gpu_driver.py's settings)
DH, DW, DRIVER_FB = 480, 640, float("inf")


def recording():
    from vo.primitives import Sequence
    return Sequence("synthetic", n_frames=3 + STEPS, height=DH, width=DW)


def by_hand(ctx, fb_max):
    from vo import _native, driver
    seq = recording()
    state, tracker = driver._device_bootstrap(seq, P["N"], KLT_WIN, KLT_MAX_LEVEL, None, None, 0.25)
    frame = state.curr_frame
    K = np.asarray(seq.get_camera().intrinsic_matrix, np.float64)
    pipe = _native.Pipeline(ctx, DH, DW, 4, K, **driver._pipeline_kwargs(state, P["N"], KLT_WIN, KLT_MAX_LEVEL, HYP, "current"))
    pipe.set_klt_fb(fb_max)
    pipe.set_frame(0, driver._gray(frame.image))
    pipe.set_state(0, frame.features, state.curr_pose, state.prev_pose, num_features=tracker._tracker._num_features)
    results = []
    for k, f in enumerate(seq):
        pipe.set_frame((k + 1) % 4, f.image, pinned=False)
        results.append(pipe.step(k % 4, (k + 1) % 4))
    pipe.close()
    return dict(trajectory=np.array([np.eye(4), state.get_pose()] + [r.pose_world_cam() for r in results]), results=results)


def test_drivers_with_and_without_the_check(ctx):
    from test_gpu_lanes import same_records
    from test_gpu_window_ba import digest
    from vo import driver
    kw = dict(n_keypoints=P["N"], context=ctx)
    plain = driver.run_on_device(recording(), **kw)
    none = driver.run_on_device(recording(), klt_fb=None, **kw)
    assert digest(plain) == digest(none), "klt_fb=None makes no call: the run is the one it was"
    out = driver.run_on_device(recording(), klt_fb=DRIVER_FB, **kw)
    hand = by_hand(ctx, DRIVER_FB)
    assert len(out["results"]) == STEPS
    assert not any(r.redetected or r.recovered for r in hand["results"] + plain["results"]), "the recording was chosen for that"
    same_records(out["results"], hand["results"], "run_on_device(klt_fb) against the by-hand loop")
    assert np.array_equal(out["trajectory"], hand["trajectory"])
    assert digest(out) != digest(plain), "the check was meant to change the run"
    assert sum(r.n_tracked for r in out["results"]) < sum(r.n_tracked for r in plain["results"])
    batch = driver.run_batch_on_device([recording()], lanes=1, klt_fb=DRIVER_FB, **kw)[0]
    same_records(batch["results"], out["results"], "run_batch_on_device(klt_fb)")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="klt_fb"):
            driver.run_on_device(recording(), klt_fb=bad, **kw)
