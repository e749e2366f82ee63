"""Host side of the FAST + BRIEF tracker mode of the device-resident loop (tracker_mode = 3): the oracle subclass
(tests/pipeline_fast_oracle.py) on the two configurations the -m gpu tests run, with the conditions those tests rely on,
and every case of the batch primitives' tables (tests/fast_loop_cases.py) keeping the edge it is named for -- checked on
the definitions (tests/brief_reference.py).  No GPU."""
import functools

import numpy as np
import pytest

import brief_reference as ref
import fast_loop_cases as cases
from pipeline_fast_oracle import FastOracleLoop, initial_fast_features


@functools.lru_cache(maxsize=None)
def oracle_run(threshold, q):
    """(start count, frame counts, pair counts, step results) of sequence q's four oracle steps."""
    stream = cases.loop_streams(q + 1)[q]
    feats, T = initial_fast_features(stream, 0, cases.LOOP_N, threshold)
    orc = FastOracleLoop(stream, cases.LOOP_N, threshold=threshold)
    orc.set_state(0, feats, T, T)
    out = [orc.step(k + 1) for k in range(cases.LOOP_STEPS)]
    return feats.length, tuple(orc.fast.frame_counts), tuple(orc.fast.pair_counts), out


@pytest.mark.parametrize("threshold", cases.LOOP_THRESHOLDS)
def test_oracle_loop_runs_and_keeps_a_population(threshold):
    """Both sequences, four steps: every step has a P3P population of 8 or more (no host path for few landmarks), pairs
    every step, and the descriptors follow their keypoints (the oracle's features carry (n, 32) uint8 rows that equal the
    definition's descriptors of their keypoints on the step's frame)."""
    for q in (0, 1):
        n0, counts, pairs, out = oracle_run(threshold, q)
        assert all(r["n_tri"] >= 8 for r in out), [r["n_tri"] for r in out]
        assert all(p > 0 for p in pairs)
        assert all(r["n_tracked"] == c for r, c in zip(out, counts))
        stream = cases.loop_streams(q + 1)[q]
        f = out[-1]["features"]
        d = np.asarray(f.descriptors)
        assert d.dtype == np.uint8 and d.shape == (f.length, 32)
        assert np.array_equal(d, ref.describe(stream.image(cases.LOOP_STEPS), f.keypoints[:, :, 0], False)[0])


def test_threshold_20_fills_every_frame():
    for q in (0, 1):
        n0, counts, _, _ = oracle_run(20, q)
        assert n0 == cases.LOOP_N and counts == (cases.LOOP_N,) * cases.LOOP_STEPS


def test_threshold_170_counts_stay_below_n_and_differ():
    """What makes the per-frame, per-sequence count matter: every frame has fewer than N corners, another number on every
    frame, and the two sequences never agree."""
    runs = [oracle_run(170, q) for q in (0, 1)]
    for n0, counts, _, _ in runs:
        assert 0 < n0 < cases.LOOP_N and all(0 < c < cases.LOOP_N for c in counts)
        assert len(set(counts)) > 1
    assert runs[0][0] != runs[1][0]
    assert all(a != b for a, b in zip(runs[0][1], runs[1][1]))


def test_oriented_descriptors_differ_from_plain_ones():
    """brief_oriented is visible in the loop: on the loop's frames most keypoints leave bin 0."""
    stream = cases.loop_streams(1)[0]
    f, _ = initial_fast_features(stream, 0, cases.LOOP_N, 20, oriented=True)
    g, _ = initial_fast_features(stream, 0, cases.LOOP_N, 20)
    assert np.array_equal(f.keypoints, g.keypoints)
    assert (np.asarray(f.descriptors) != np.asarray(g.descriptors)).any(axis=1).mean() > 0.5


# ---- the batch tables ----
@pytest.mark.parametrize("name", cases.DESCRIBE_NAMES)
def test_describe_case_keeps_its_edge(name):
    c = cases.DESCRIBE_BY_NAME[name]
    S, N = c.kp.shape[:2]
    assert c.imgs.shape == (3, 40, 56) and N == 8 and S == 3
    assert c.img_stride > 40 * 56 and c.xy_stride > N and c.desc_stride > 32 * N
    eff = cases.describe_effective(c)
    assert eff == c.props["effective"]
    desc, bins = cases.describe_expected(c)
    for q in range(S):
        # rows at and beyond the count hold the sentinel, and would not if they were described
        assert (desc[q, eff[q]:] == cases.SENTINEL).all() and (bins[q, eff[q]:] == cases.SENTINEL).all()
        if eff[q] < N:
            d = ref.describe(c.imgs[q], c.kp[q, eff[q]:], c.oriented)[0]
            assert (d != cases.SENTINEL).any(axis=1).all()
        assert not (desc[q, :eff[q]] == cases.SENTINEL).all(axis=1).any()
    if name.startswith("counts_0_1_5"):
        assert c.counts == (0, 1, 5)
    if name.startswith("count_above"):
        assert c.counts[0] > N and c.counts[1] < 0
    if "valid" in c.props:
        seen = set()
        for q in range(S):
            valid = ref.centres(c.kp[q, :eff[q]], 40, 56)[2]
            assert tuple(bool(v) for v in valid) == c.props["valid"][q]
            assert not desc[q, :eff[q]][~valid].any() and not bins[q, :eff[q]][~valid].any()
            seen |= {bool(np.isfinite(k).all()) for k in c.kp[q, :eff[q]]}
        assert seen == {True, False}
        # valid centres outside the image read part of it: their descriptors are not all zero
        assert desc[0, 4].any() and desc[0, 0].any()
    if c.oriented:
        assert any(bins[q, :eff[q]].any() for q in range(S))


@pytest.mark.parametrize("name", cases.MATCH_NAMES)
def test_match_case_keeps_its_edge(name):
    c = cases.MATCH_BY_NAME[name]
    assert c.q.shape == (3, 20, 32) and c.t.shape == (3, 40, 32) and (c.cap_q, c.cap_t) == (20, 40)
    enq, ent = cases.match_effective(c)
    want = cases.match_expected(c)
    for z in range(3):
        assert len(want[z]) <= enq[z]
        if enq[z] == 0 or ent[z] < 2:
            assert len(want[z]) == 0
        assert (want[z][:, 0] < enq[z]).all() and (want[z][:, 1] < ent[z]).all()
        assert len(set(want[z][:, 1].tolist())) == len(want[z]) and (np.diff(want[z][:, 0]) > 0).all()
    assert sum(len(w) for w in want) > 0
    if name == "partial_query_groups":
        assert c.nq == (0, 9, 20) and any(n % 8 for n in enq)
    if name == "train_slices":
        assert set(c.nt) == {1, 0, 33} and cases.MATCH_BY_NAME["partial_query_groups"].nt[0] == 40
    if name == "counts_beyond_capacity_and_negative":
        assert enq == (20, 0, 17) and ent == (40, 40, 0)
    if c.props.get("beyond"):
        # a kernel that read rows beyond the counts would return other lists, in every sequence
        other = cases.match_expected(c, use_counts=False)
        assert all(not np.array_equal(a, b) for a, b in zip(want, other))
        assert any(len(b) > len(a) for a, b in zip(want, other))
    if "contested" in c.props:
        train, winners = c.props["contested"]
        assert len(set(winners)) == 3
        for z in range(3):
            assert [int(p[0]) for p in want[z] if p[1] == train] == [winners[z]]
        # sequences 0 and 2 have a second query that passes with the same row and loses it
        for z, loser in ((0, 5), (2, 4)):
            best, dist = ref.knn2(c.q[z], c.t[z])
            assert best[loser, 0] == train and dist[loser, 0] < c.ratio * dist[loser, 1] and loser not in want[z][:, 0]
    if "keeps" in c.props:
        best, dist = ref.knn2(c.q[0], c.t[0])
        assert (dist[0].tolist(), dist[1].tolist(), dist[2].tolist(), dist[3].tolist()) == ([4, 8], [3, 8], [10, 30], [11, 30])
        assert float(dist[0, 0]) == c.ratio * float(dist[0, 1]) and dist[2, 0] == c.max_dist
        assert [int(v) for v in want[0][:, 0]] == list(c.props["keeps"])
    if c.props.get("far"):
        assert c.max_dist < 0
        d = ref.hamming(c.q[0, :1], c.t[0])[0]
        assert d.min() > 64 and len(want[0]) >= 1
        assert len(ref.match(c.q[0], c.t[0], c.ratio, 64)) == 0


def test_python_pipeline_knows_the_mode():
    """Pipeline(tracker="fast") maps to tracker_mode 3 with 32 values a descriptor row (no library needed to say so)."""
    import inspect
    from vo import _pipeline
    sig = inspect.signature(_pipeline.Pipeline.__init__).parameters
    assert (sig["fast_threshold"].default, sig["brief_oriented"].default, sig["brief_max_distance"].default) == (0, False, 0)
    p = _pipeline.Pipeline.__new__(_pipeline.Pipeline)
    p.tracker = "fast"
    assert p._desc_len() == 32
    for mode, n in (("sift", 128), ("harris", 361)):
        p.tracker = mode
        assert p._desc_len() == n
    assert "fast" in (_pipeline.Pipeline.get_descriptors.__doc__ + _pipeline.Pipeline.set_state.__doc__).lower()
