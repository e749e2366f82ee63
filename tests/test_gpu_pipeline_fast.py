"""-m gpu: the FAST + BRIEF tracker mode of the device-resident loop (Pipeline(tracker="fast"), tracker_mode = 3) against
the CPU oracle of the same loop (tests/pipeline_fast_oracle.py) and, with several sequences per launch, against
one-sequence pipelines -- records, every carried array, the descriptors and the estimator generator -- through look-ahead,
the host path and checkpoint / rewind.  Threshold 170 leaves every frame with fewer corners than n_keypoints, another
number per frame and per sequence (tests/test_pipeline_fast_host.py asserts it): the counts stay on the device."""
import copy
import functools

import numpy as np
import pytest

import fast_loop_cases as cases
from pipeline_fast_oracle import FastOracleLoop, initial_fast_features
from test_gpu_harris_sequences import assert_records_equal, assert_snapshots_equal, drive, snapshot

pytestmark = pytest.mark.gpu
H, W, N, F = cases.LOOP_H, cases.LOOP_W, cases.LOOP_N, cases.LOOP_FRAMES


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def fast_pipe(ctx, H, W, F, K, N, S=1, **kw):
    from vo import _native
    return _native.Pipeline(ctx, H, W, F, K, n_keypoints=N, hyp=256, p3p_threshold=1.0, max_iterations=1000,
                            refine_iters=20, tracker="fast", sequences=S, **kw)


@functools.lru_cache(maxsize=None)
def streams_of(S, F=F, H=H, W=W):
    return cases.loop_streams(S, F, H, W)


@functools.lru_cache(maxsize=None)
def _start(q, S, threshold, oriented, F, H, W, N):
    return initial_fast_features(streams_of(S, F, H, W)[q], 0, N, threshold, oriented)


def start_state(q, S, threshold, fraction=1.0, oriented=False, F=F, H=H, W=W, N=N):
    """Sequence q's starting Features (a copy) and pose; fraction < 1: an evenly spread subset, descriptors included."""
    feats, T = _start(q, S, threshold, oriented, F, H, W, N)
    feats = copy.deepcopy(feats)
    if fraction < 1.0:
        keep = np.zeros(feats.length, dtype=bool)
        keep[np.linspace(0, feats.length - 1, int(fraction * feats.length)).astype(int)] = True
        desc = np.asarray(feats.descriptors)[keep]
        feats.mask(keep)
        feats.descriptors = desc
    return feats, T


def load(pipe, streams, starts):
    for q, stream in enumerate(streams):
        for i in range(stream.n):
            pipe.set_frame(i, stream.image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)


def against_the_oracle(ctx, threshold, steps, oriented=False):
    from test_gpu_pipeline import check_step
    stream = streams_of(1)[0]
    feats, T = start_state(0, 1, threshold, oriented=oriented)
    pipe = fast_pipe(ctx, H, W, F, stream.K, N, fast_threshold=threshold, brief_oriented=oriented)
    load(pipe, [stream], [(feats, T)])
    assert np.array_equal(pipe.get_descriptors(), np.asarray(feats.descriptors, np.float32))
    orc = FastOracleLoop(stream, N, threshold=threshold, oriented=oriented)
    orc.set_state(0, feats, T, T)
    for k in range(steps):
        ref = orc.step(k + 1)
        r = pipe.step(k, k + 1)
        print("step %d: frame corners %d, pairs %d, tracked %d / %d, triangulated %d / %d, inliers %d / %d" % (
            k, orc.fast.frame_counts[-1], orc.fast.pair_counts[-1], r.n_tracked, ref["n_tracked"], r.n_triangulated,
            ref["n_tri"], r.n_inliers, ref["n_inliers"]))
        assert r.n_triangulated >= 8
        assert r.n_tracked == orc.fast.frame_counts[-1] == len(fast_reference_keypoints(stream, k + 1, threshold))
        check_step(r, ref, pipe, orc.rs.rng, land_tol=1e-4)
        got = pipe.get_descriptors()
        want = np.asarray(ref["features"].descriptors)
        assert want.dtype == np.uint8 and np.array_equal(got, want.astype(np.float32))
    pipe.close()
    return orc


def fast_reference_keypoints(stream, idx, threshold):
    import fast_reference
    return fast_reference.keypoints(stream.image(idx), threshold, True, N)[0]


@pytest.mark.parametrize("threshold", cases.LOOP_THRESHOLDS)
def test_fast_loop_matches_the_oracle_loop(ctx, threshold):
    """One sequence, four steps: every array the loop carries after every step, the RANSAC bookkeeping and the generator
    against the oracle loop; the descriptors exactly; n_tracked is the frame's corner count (N at threshold 20, fewer and
    another number every frame at 170)."""
    orc = against_the_oracle(ctx, threshold, cases.LOOP_STEPS)
    if threshold == 170:
        assert all(c < N for c in orc.fast.frame_counts) and len(set(orc.fast.frame_counts)) > 1
    else:
        assert orc.fast.frame_counts == [N] * cases.LOOP_STEPS


def test_fast_loop_with_oriented_descriptors(ctx):
    """brief_oriented=True, two steps against the oracle loop."""
    against_the_oracle(ctx, 20, 2, oriented=True)


@pytest.mark.parametrize("lookahead,fault_every", [(False, 0), (True, 0), (False, 4), (True, 4)])
def test_fast_sequences_equal_single_sequence_pipelines(ctx, lookahead, fault_every):
    """S = 3 scenes at threshold 170 (another corner count per frame and sequence), one starting from 80 % of its features,
    through the same launches: after every step each sequence's record, carried arrays, descriptors and generator equal
    those of a one-sequence pipeline making the same calls.  fault_every = 4: every 4th step of every sequence is forced
    off the device-only path at the pair regroup and redone alone by the host path while the others go on."""
    S, thr = 3, 170
    streams = streams_of(S)
    starts = [start_state(q, S, thr, (1.0, 0.8, 1.0)[q]) for q in range(S)]
    order = streams[0].order(8)
    pairs = list(zip(order[:-1], order[1:]))
    blocking = not lookahead

    single = []
    for q in range(S):
        pipe = fast_pipe(ctx, H, W, F, streams[q].K, N, debug_fault_every=fault_every, fast_threshold=thr)
        load(pipe, [streams[q]], [starts[q]])
        snaps = []
        res = drive(pipe, pairs, lookahead, (lambda k: snaps.append(snapshot(pipe, 0))) if blocking else None)
        snaps.append(snapshot(pipe, 0))
        single.append(([r[0] for r in res], snaps))
        pipe.close()

    pipe = fast_pipe(ctx, H, W, F, streams[0].K, N, S=S, debug_fault_every=fault_every, fast_threshold=thr)
    load(pipe, streams, starts)
    for q in range(S):
        assert np.array_equal(pipe.get_descriptors(seq=q), np.asarray(starts[q][0].descriptors, np.float32))
    snaps = []
    got = drive(pipe, pairs, lookahead, (lambda k: snaps.append([snapshot(pipe, q) for q in range(S)])) if blocking else None)
    snaps.append([snapshot(pipe, q) for q in range(S)])
    assert len({got[0][q].n_tracked for q in range(S)}) > 1 and all(got[0][q].n_tracked < N for q in range(S))
    for q in range(S):
        res, ref_snaps = single[q]
        for k in range(len(pairs)):
            assert got[k][q].fault == 0
            assert_records_equal(got[k][q], res[k], ("sequence", q, "step", k))
        if fault_every and not lookahead:
            assert all(got[k][q].recovered == 1 for k in range(fault_every - 1, len(pairs), fault_every)), q
        for k, ref in enumerate(ref_snaps):
            assert_snapshots_equal(snaps[k][q], ref, ("sequence", q, "after step", k))
    if fault_every and lookahead:
        # With look-ahead the chain of step k is enqueued -- with the hook -- before step k - 1 is collected.  If step k - 1
        # of a sequence then leaves the device-only path (the host path, or a RANSAC loop that goes on over several launches
        # of 256 samples: at threshold 170 the populations are small and that is common), step k is enqueued again for that
        # sequence without the hook, as in the KLT mode.  So a forced step must have gone through the host path exactly
        # where its predecessor closed inside its first launch; the others may or may not have.
        for q in range(S):
            for k in range(fault_every - 1, len(pairs), fault_every):
                before = got[k - 1][q]
                if before.recovered == 0 and before.draws_consumed <= 256:
                    assert got[k][q].recovered == 1, (q, k)
    pipe.close()


def test_fast_sequences_one_sequence_against_the_oracle_loop(ctx):
    """Sequence 1 of an S = 2 pipeline against the oracle loop for four steps at threshold 170: the batched path is tied to
    the oracle, not only to itself."""
    from test_gpu_pipeline import check_step
    S, thr = 2, 170
    streams = streams_of(S)
    starts = [start_state(q, S, thr) for q in range(S)]
    pipe = fast_pipe(ctx, H, W, F, streams[0].K, N, S=S, fast_threshold=thr)
    load(pipe, streams, starts)
    orc = FastOracleLoop(streams[1], N, threshold=thr)
    orc.set_state(0, starts[1][0], starts[1][1], starts[1][1])

    class SequenceView:            # check_step reads sequence 0's state / generator: point it at sequence 1
        def get_state(self):
            return pipe.get_state(seq=1)

        def rng_state_into(self, g):
            pipe.rng_state_into(g, seq=1)

    for a, b in [(k, k + 1) for k in range(4)]:
        ref = orc.step(b)
        pipe.submit(a, b)
        rs = pipe.collect_all()
        r = rs[1]
        assert r.n_tracked == orc.fast.frame_counts[-1] < N and r.n_triangulated >= 8 and rs[0].n_tracked != r.n_tracked
        check_step(r, ref, SequenceView(), orc.rs.rng, land_tol=1e-4)
        assert np.array_equal(pipe.get_descriptors(seq=1), np.asarray(ref["features"].descriptors, np.float32))
    pipe.close()


def test_fast_sequences_checkpoint_and_rewind(ctx):
    """S = 2: checkpoint, three steps, rewind, the same three steps again.  Every sequence equals a one-sequence pipeline
    making the same calls (the RANSAC fields and the generator go on across a rewind)."""
    S, thr = 2, 170
    streams = streams_of(S)
    starts = [start_state(q, S, thr, (1.0, 0.85)[q]) for q in range(S)]
    pairs = [(k, k + 1) for k in range(3)]

    def run(pipe, seqs):
        pipe.checkpoint()
        out = []
        for p in range(2):
            if p:
                pipe.rewind()
            res = drive(pipe, pairs, p == 1)
            out.append((res, [snapshot(pipe, q) for q in seqs]))
        return out

    single = []
    for q in range(S):
        pipe = fast_pipe(ctx, H, W, F, streams[q].K, N, fast_threshold=thr)
        load(pipe, [streams[q]], [starts[q]])
        single.append(run(pipe, [0]))
        pipe.close()
    pipe = fast_pipe(ctx, H, W, F, streams[0].K, N, S=S, fast_threshold=thr)
    load(pipe, streams, starts)
    got = run(pipe, range(S))
    for q in range(S):
        for p in range(2):
            res, snaps = got[p]
            ref_res, ref_snaps = single[q][p]
            for k in range(len(pairs)):
                assert res[k][q].fault == 0
                assert_records_equal(res[k][q], ref_res[k][0], ("sequence", q, "pass", p, "step", k))
            assert_snapshots_equal(snaps[q], ref_snaps[0], ("sequence", q, "pass", p))
        assert got[1][0][0][q].n_features_in == got[0][0][0][q].n_features_in
    pipe.close()


def test_fast_sequences_at_configuration_size(ctx):
    """S = 2 at 1376 x 1241 with 2000 keypoints (250 query groups, 63 rounds of train slices, a 4000-row regroup), two
    steps: each sequence equals its one-sequence pipeline."""
    Hc, Wc, Nc, Fc, S = cases.CONFIG_H, cases.CONFIG_W, cases.CONFIG_N, 3, 2
    streams = streams_of(S, Fc, Hc, Wc)
    starts = [start_state(q, S, 20, (1.0, 0.9)[q], F=Fc, H=Hc, W=Wc, N=Nc) for q in range(S)]
    pairs = [(k, k + 1) for k in range(2)]
    single = []
    for q in range(S):
        pipe = fast_pipe(ctx, Hc, Wc, Fc, streams[q].K, Nc)
        load(pipe, [streams[q]], [starts[q]])
        res = drive(pipe, pairs, True)
        single.append(([r[0] for r in res], snapshot(pipe, 0)))
        pipe.close()
    pipe = fast_pipe(ctx, Hc, Wc, Fc, streams[0].K, Nc, S=S)
    load(pipe, streams, starts)
    got = drive(pipe, pairs, True)
    for q in range(S):
        for k in range(len(pairs)):
            assert got[k][q].fault == 0 and got[k][q].n_tracked > 0 and got[k][q].n_triangulated >= 8
            assert_records_equal(got[k][q], single[q][0][k], ("sequence", q, "step", k))
        assert_snapshots_equal(snapshot(pipe, q), single[q][1], ("sequence", q))
    pipe.close()


def test_fast_mode_refusals(ctx):
    """What the mode refuses, as the Harris mode does: the Shi-Tomasi detector, lanes, the bootstrap, the forward-backward
    check, the structure loop; settings out of range, with a message naming the field; descriptor rows of another width
    or values a byte cannot hold.  Refused calls change nothing: the pipeline still runs."""
    from vo import _native
    from vo._native import VoError
    Hs, Ws, Ns, Fs, S = 240, 320, 300, 3, 2
    streams = streams_of(S, Fs, Hs, Ws)
    K = streams[0].K
    with pytest.raises(VoError, match="detector"):
        fast_pipe(ctx, Hs, Ws, Fs, K, Ns, detector="shi-tomasi")
    for kw, field in ((dict(fast_threshold=255), "fast_threshold"), (dict(fast_threshold=-1), "fast_threshold"),
                      (dict(brief_max_distance=257), "brief_max_distance")):
        with pytest.raises(VoError, match=field):
            fast_pipe(ctx, Hs, Ws, Fs, K, Ns, **kw)
    # ... and ignored in the other modes
    _native.Pipeline(ctx, Hs, Ws, Fs, K, n_keypoints=Ns, tracker="harris", fast_threshold=999, brief_max_distance=999).close()
    pipe = fast_pipe(ctx, Hs, Ws, Fs, K, Ns, S=S, track_ids=True)
    with pytest.raises(VoError, match="brief_oriented"):
        ctx._chk(ctx._lib.vo_pipeline_set_fast_brief(pipe._h, 20, 2, 64))
    starts = [initial_fast_features(streams[q], 0, Ns) for q in range(S)]
    load(pipe, streams, starts)
    with pytest.raises(VoError, match="KLT tracker mode"):
        pipe.set_active(1, False)
    with pytest.raises(VoError, match="KLT tracker mode"):
        pipe.restart(1, 0, starts[1][0], starts[1][1])
    with pytest.raises(VoError, match="KLT tracker mode"):
        pipe.bootstrap(1, 0)
    with pytest.raises(VoError, match="KLT tracker mode"):
        pipe.set_klt_fb(1.0)
    with pytest.raises(VoError, match="tracker_mode"):
        pipe.structure_loop(4)
    # descriptors: 32 values a row, whole numbers 0 .. 255
    import ctypes as C
    n = starts[0][0].length
    bad = copy.deepcopy(starts[0][0])
    bad.descriptors = np.zeros((n, 361), np.uint8)
    with pytest.raises(ValueError, match="descriptor"):
        pipe.set_state(0, bad, starts[0][1], starts[0][1])
    for value in (256.0, -1.0, 0.5):
        desc = np.zeros((4, 32), np.float32)
        desc[3, 31] = value
        with pytest.raises(VoError, match="0..255"):
            ctx._chk(ctx._lib.vo_pipeline_set_descriptors_seq(pipe._h, 0, desc.ctypes.data_as(C.c_void_p), 4))
    for seq in (-1, S):
        with pytest.raises(VoError):
            pipe.get_descriptors(seq=seq)
    load(pipe, streams, starts)
    assert pipe.get_descriptors(seq=1).shape == (starts[1][0].length, 32)
    pipe.submit(0, 1)
    rs = pipe.collect_all()
    assert all(r.fault == 0 and r.n_tracked > 0 for r in rs)
    pipe.close()
