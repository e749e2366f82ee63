"""-m gpu: the device-resident KLT loop with the Shi-Tomasi re-detect (vo_pipeline_config.detector = 1) against the CPU
oracle of the reference's KLT mode (tests/pipeline_shi_tomasi_oracle.py), frame by frame.  The tolerances are
tests/test_gpu_pipeline.py's check_step / check_state: integer results exact, R and t to 1e-9, the refined pose to 1e-7,
landmarks to 1e-6 relative."""
import types

import numpy as np
import pytest

import pipeline_shi_tomasi_oracle as sto
from test_gpu_pipeline import check_state, check_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def make_pipe(ctx, name, stream, hyp=256, detector="shi-tomasi", sequences=1, upload=True, **kw):
    from vo import _native
    _, quality, min_distance, _, _, _ = sto.CASES[name]
    _, _, n, _ = sto.SIZES.get(name, (sto.H, sto.W, sto.N, sto.STEPS))
    if detector == "shi-tomasi":
        kw.update(st_quality=quality, st_min_distance=min_distance)
    pipe = _native.Pipeline(ctx, stream.H, stream.W, stream.n, stream.K, n_keypoints=n, klt_win=sto.WIN,
                            klt_max_level=sto.LEVELS, hyp=hyp, p3p_threshold=1.0, max_iterations=1000, refine_iters=20,
                            detector=detector, sequences=sequences, **kw)
    if upload:
        for i in range(stream.n):
            pipe.set_frame(i, stream.image(i))
    return pipe


def generator_of(ref):
    """What check_step reads the oracle's generator state from."""
    return types.SimpleNamespace(bit_generator=types.SimpleNamespace(state=ref["generator"]))


def check_against(pipe, r, ref):
    assert r.redetected == ref["redetected"]
    assert r.n_features_in == ref["n_before"] + ref["appended"]
    check_step(r, ref, pipe, generator_of(ref))
    assert pipe.get_state()["num_features"] == ref["num_features"]


def run_against_oracle(ctx, name, redetect="current", hyp=256, **kw):
    stream, feats, T, pairs, refs = sto.run_case(name, redetect)
    pipe = make_pipe(ctx, name, stream, hyp=hyp, redetect_start_pose=redetect, **kw)
    pipe.set_state(0, feats, T, T)
    check_state(pipe.get_state(), feats, T)
    got = []
    for (a, b), ref in zip(pairs, refs):
        r = pipe.step(a, b)
        check_against(pipe, r, ref)
        got.append(r)
    pipe.close()
    assert sum(r.redetected for r in got) >= 1, "the re-detect branch was meant to run"
    return got, refs


@pytest.mark.parametrize("name,redetect", [("A", "current"), ("B", "current"), ("D", "current"), ("B", "identity")])
def test_loop_matches_the_oracle_of_the_reference_klt_mode(ctx, name, redetect):
    """After every step every array the reference carries, the RANSAC bookkeeping and the generator; the step that
    re-detects appends what goodFeaturesToTrack found on its frame -- the cap (A) or fewer (B, D) -- and _num_features is
    that count from then on (klt.py:114)."""
    got, refs = run_against_oracle(ctx, name, redetect)
    _, _, _, _, when, count = sto.CASES[name]
    assert got[when].redetected == 1 and got[when].n_features_in == refs[when]["n_before"] + count
    assert all(r.recovered == 0 for r in got)


def test_get_detection_is_good_features_of_the_frame(ctx):
    """Points and count of the current detection slot, on a frame the detector ran on by itself (every frame:
    detect_margin < 0) and on one it sat out (made then, for that sequence)."""
    stream, feats, T, pairs, _ = sto.run_case("B")
    _, quality, min_distance, _, _, _ = sto.CASES["B"]
    fewer = 0
    for kw in (dict(detect_margin=-1.0), dict()):
        pipe = make_pipe(ctx, "B", stream, redetect_start_pose="current", **kw)
        pipe.set_state(0, feats, T, T)
        for a, b in pairs[:3]:
            r = pipe.step(a, b)
            if kw:
                assert r.detector_ran == 1
            want = ctx.good_features(stream.image(b), None, sto.N, quality, min_distance, 7)
            got = pipe.get_detection(0)
            assert got.dtype == np.float64 and got.shape == want.shape and 0 < len(want) <= sto.N
            assert np.array_equal(got, want.astype(np.float64))
            fewer += len(want) < sto.N
        pipe.close()
    assert fewer >= 1, "a frame with fewer corners than the cap was meant to be among them"


def test_three_sequences_append_their_own_counts(ctx):
    """Cases B and C and a full start state in one pipeline, look-ahead on: each sequence equals its own one-sequence
    oracle run, with its own corner count at its own step."""
    runs = [sto.run_case("B"), sto.run_case("C"), sto.run_case("B", fraction=1.0)]
    S = len(runs)
    pairs = runs[0][3]
    pipe = make_pipe(ctx, "B", runs[0][0], sequences=S, upload=False, redetect_start_pose="current")
    for q, (stream, feats, T, _, _) in enumerate(runs):
        for i in range(stream.n):
            pipe.set_frame(i, stream.image(i), seq=q)
        pipe.set_state(0, feats, T, T, seq=q)
    got = []
    pipe.submit(*pairs[0])
    for k in range(len(pairs)):
        if k + 1 < len(pairs):
            pipe.submit(*pairs[k + 1])
        got.append(pipe.collect_all())
    appended = set()
    for q, (_, _, _, _, refs) in enumerate(runs):
        for k, ref in enumerate(refs):
            r = got[k][q]
            assert r.fault == 0 and r.redetected == ref["redetected"], (q, k)
            assert r.n_features_in == ref["n_before"] + ref["appended"], (q, k)
            assert (r.n_tracked, r.n_triangulated, r.draws_consumed, r.ransac_iterations, r.n_inliers, r.n_candidates,
                    r.n_landmarks) == (ref["n_tracked"], ref["n_tri"], ref["draws"], ref["iters"], ref["n_inliers"],
                                       ref["n_cand"], ref["n_landmarks"]), (q, k)
            assert np.allclose(np.array(r.R).reshape(3, 3), ref["R"], atol=1e-9) and np.allclose(np.array(r.t), ref["t"], atol=1e-9)
            assert np.allclose(np.array(r.R_refined).reshape(3, 3), ref["R_ref"], atol=1e-7)
            assert np.allclose(np.array(r.t_refined), ref["t_ref"], atol=1e-7)
            if r.redetected:
                appended.add(r.n_features_in - ref["n_before"])
        st = pipe.get_state(seq=q)
        check_state(st, refs[-1]["features"], refs[-1]["pose"])
        assert st["num_features"] == refs[-1]["num_features"]
        assert (st["n_iterations"], st["outlier_ratio"]) == (refs[-1]["n_iterations"], refs[-1]["outlier_ratio"])
        g = np.random.default_rng(0)
        pipe.rng_state_into(g, seq=q)
        assert g.bit_generator.state == refs[-1]["generator"]
    assert {226, 236} <= appended
    pipe.close()


def test_detection_on_every_frame_gives_the_same(ctx):
    got, _ = run_against_oracle(ctx, "B", detect_margin=-1.0)
    assert all(r.detector_ran == 1 and r.recovered == 0 for r in got)


def test_a_skipped_detection_is_made_up_through_the_host_path(ctx):
    """debug_never_detect: the step that crosses the limit finds no corners, is finished through the host path -- whose
    forced one-sequence detection goes through the same chain -- and still equals the oracle."""
    got, refs = run_against_oracle(ctx, "B", debug_never_detect=1)
    when = sto.CASES["B"][4]
    assert got[when].redetected == 1 and got[when].recovered == 1
    assert got[when].reserved & 32, "the step was meant to leave the device path for its missing detection"


def test_a_forced_fault_on_the_redetect_step(ctx):
    """debug_fault_every = 3: steps 2 and 5 take the host path; step 2 is the one that re-detects."""
    got, _ = run_against_oracle(ctx, "B", debug_fault_every=3)
    when = sto.CASES["B"][4]
    assert when == 2 and got[2].recovered == 1 and got[2].redetected == 1 and got[5].recovered == 1


def test_a_redetect_that_does_not_fit_reports_the_real_count(ctx):
    from vo import _native
    stream, feats, T, pairs, refs = sto.run_case("B")
    when, count = sto.CASES["B"][4:]
    n_before = refs[when]["n_before"]
    cap = 400
    assert max(r["n_before"] for r in refs[:when + 1]) <= cap < n_before + count
    pipe = make_pipe(ctx, "B", stream, feature_cap=cap, redetect_start_pose="current")
    pipe.set_state(0, feats, T, T)
    for a, b in pairs[:when]:
        assert pipe.step(a, b).fault == 0
    with pytest.raises(_native.VoError) as e:
        pipe.step(*pairs[when])
    assert e.value.code == _native.VO_ECAPACITY
    assert "%d features + %d new keypoints exceed the capacity %d" % (n_before, count, cap) in str(e.value)
    # the pipeline goes on from a state handed over again
    pipe.set_state(0, feats, T, T)
    r = pipe.step(*pairs[0])
    assert r.fault == 0 and r.n_tracked == refs[0]["n_tracked"] and r.n_features_in == refs[0]["n_before"]
    pipe.close()


def test_refused_configurations(ctx, monkeypatch):
    from vo import _native, _pipeline
    stream, feats, T, pairs, _ = sto.run_case("B")
    monkeypatch.setitem(_pipeline.DETECTORS, "two", 2)
    monkeypatch.setitem(_pipeline.DETECTORS, "minus", -1)
    refused = [(dict(detector="two"), "detector must be"),
               (dict(detector="minus"), "detector must be"),
               (dict(detector="shi-tomasi", tracker="harris"), "KLT tracker mode"),
               (dict(detector="shi-tomasi", st_block=32), "blockSize"),
               (dict(detector="shi-tomasi", st_quality=-0.5), "quality"),
               (dict(detector="shi-tomasi", st_min_distance=-1.0), "minDistance")]
    for kw, text in refused:
        with pytest.raises(_native.VoError) as e:
            _native.Pipeline(ctx, stream.H, stream.W, stream.n, stream.K, n_keypoints=sto.N, klt_win=sto.WIN, hyp=256, **kw)
        assert e.value.code == _native.VO_EINVAL and text in str(e.value), (kw, str(e.value))
        pipe = make_pipe(ctx, "B", stream, detector="harris")
        pipe.set_state(0, feats, T, T)
        r = pipe.step(*pairs[0])
        assert r.fault == 0 and r.n_tracked > 0
        pipe.close()


def test_loop_at_480_by_640(ctx):
    """500 keypoints at 480 x 640 (more than one workgroup of features, several tiles of the map): the re-detect comes
    at the step from frame 3 to 4 and returns the cap."""
    got, refs = run_against_oracle(ctx, "E", hyp=1000)
    when, count = sto.CASES["E"][4:]
    assert [r.redetected for r in got] == [1 if k == when else 0 for k in range(len(got))]
    assert got[when].n_features_in == refs[when]["n_before"] + count == refs[when]["n_before"] + 500
