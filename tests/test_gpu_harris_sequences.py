"""-m gpu: several sequences per launch in the Harris tracker mode (vo_pipeline_config.sequences = S, tracker_mode = 2).
Every sequence of one pipeline must equal a one-sequence Harris pipeline of its own -- records, every carried array, the
descriptors the Features carry and the estimator generator -- through look-ahead, the host path, per-sequence cameras and
checkpoint / rewind; one sequence of a batched pipeline is also checked against the oracle loop."""
import copy

import numpy as np
import pytest

from pipeline_oracle import OracleLoop, initial_harris_features

pytestmark = pytest.mark.gpu

STATE_KEYS = ("keypoints", "state", "candidate_mask", "landmarks", "tracks", "poses", "curr_pose", "n_iterations")
# what may differ between two pipelines that computed the same steps: the device timestamps and the records' numbers
NOT_COMPARED = ("ts", "seq_head", "seq_tail")


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def harris_pipe(ctx, H, W, F, K, N, S=1, **kw):
    from vo import _native
    return _native.Pipeline(ctx, H, W, F, K, n_keypoints=N, hyp=256, p3p_threshold=1.0, max_iterations=1000,
                            refine_iters=20, tracker="harris", sequences=S, **kw)


def start_state(stream, N, fraction=1.0):
    feats, T = initial_harris_features(stream, 0, N)
    if fraction < 1.0:
        keep = np.zeros(feats.length, dtype=bool)
        keep[np.linspace(0, feats.length - 1, int(fraction * feats.length)).astype(int)] = True
        desc = np.asarray(feats.descriptors)[keep]
        feats = copy.deepcopy(feats)
        feats.mask(keep)
        feats.descriptors = desc
    return feats, T


def record(r):
    from vo import _native
    out = {}
    for name, _ in _native.StepResult._fields_:
        if name in NOT_COMPARED:
            continue
        v = getattr(r, name)
        out[name] = tuple(v) if hasattr(v, "__len__") else v
    return out


def assert_records_equal(got, ref, where):
    a, b = record(got), record(ref)
    diff = [(k, a[k], b[k]) for k in a if a[k] != b[k]]
    assert not diff, (where, diff[:3])


def snapshot(pipe, q):
    g = np.random.default_rng(0)
    pipe.rng_state_into(g, seq=q)
    return pipe.get_state(seq=q), pipe.get_descriptors(seq=q), g.bit_generator.state


def assert_snapshots_equal(got, ref, where):
    (st, desc, g), (st_ref, desc_ref, g_ref) = got, ref
    for key in STATE_KEYS:
        assert np.array_equal(st[key], st_ref[key], equal_nan=True), (where, key)
    assert desc.shape == desc_ref.shape and np.array_equal(desc, desc_ref), (where, "descriptors")
    assert g == g_ref, (where, "generator")


def drive(pipe, pairs, lookahead, after=None):
    """Runs `pairs` (look-ahead: one step in flight beyond the one collected); a list of collect_all() results.  after(k):
    called once step k is collected and nothing is in flight (blocking runs only)."""
    out = []
    if lookahead:
        pipe.submit(*pairs[0])
        for k in range(len(pairs)):
            if k + 1 < len(pairs):
                pipe.submit(*pairs[k + 1])
            out.append(pipe.collect_all())
    else:
        for k, (a, b) in enumerate(pairs):
            pipe.submit(a, b)
            out.append(pipe.collect_all())
            if after:
                after(k)
    return out


def scenes(S, F, H, W, **kw):
    from vo import synthetic
    return [synthetic.Stream(F, H, W, seed=2023 + 7 * q, start=q, **kw) for q in range(S)]


@pytest.mark.parametrize("lookahead,fault_every", [(False, 0), (True, 0), (False, 4), (True, 4)])
def test_harris_sequences_equal_single_sequence_pipelines(ctx, lookahead, fault_every):
    """S = 3 different scenes, one starting from a subset of its features (pair counts differ per sequence), through the
    same launches.  After every step each sequence's record, carried arrays, descriptors and generator equal those of a
    one-sequence Harris pipeline making the same calls.  fault_every = 4: every 4th step of every sequence is forced off
    the device-only path at the pair regroup and redone alone by the host path while the others go on."""
    H, W, N, F, S = 480, 640, 500, 6, 3
    streams = scenes(S, F, H, W)
    starts = [start_state(streams[q], N, (1.0, 0.8, 1.0)[q]) for q in range(S)]
    order = streams[0].order(8)
    pairs = list(zip(order[:-1], order[1:]))
    blocking = not lookahead

    single = []
    for q in range(S):
        pipe = harris_pipe(ctx, H, W, F, streams[q].K, N, debug_fault_every=fault_every)
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i))
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1])
        snaps = []
        res = drive(pipe, pairs, lookahead, (lambda k: snaps.append(snapshot(pipe, 0))) if blocking else None)
        snaps.append(snapshot(pipe, 0))
        single.append(([r[0] for r in res], snaps))
        pipe.close()

    pipe = harris_pipe(ctx, H, W, F, streams[0].K, N, S=S, debug_fault_every=fault_every)
    for q in range(S):
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    for q in range(S):
        assert np.array_equal(pipe.get_descriptors(seq=q), np.asarray(starts[q][0].descriptors, np.float32).reshape(-1, 361))
    snaps = []
    got = drive(pipe, pairs, lookahead, (lambda k: snaps.append([snapshot(pipe, q) for q in range(S)])) if blocking else None)
    snaps.append([snapshot(pipe, q) for q in range(S)])
    assert len({got[0][q].n_triangulated for q in range(S)}) > 1
    for q in range(S):
        res, ref_snaps = single[q]
        for k in range(len(pairs)):
            assert got[k][q].fault == 0 and got[k][q].n_features_in == N
            assert_records_equal(got[k][q], res[k], ("sequence", q, "step", k))
        if fault_every and not lookahead:
            assert all(got[k][q].recovered == 1 for k in range(fault_every - 1, len(pairs), fault_every)), q
        for k, ref in enumerate(ref_snaps):
            assert_snapshots_equal(snaps[k][q], ref, ("sequence", q, "after step", k))
    if fault_every:
        # (with look-ahead a forced step can be one that is enqueued again behind a step whose RANSAC loop went on over
        #  several launches -- enqueued again without the hook, as in the KLT mode; some forced steps remain)
        assert sum(got[k][q].recovered for k in range(len(pairs)) for q in range(S)) >= 2
    pipe.close()


def test_harris_sequences_per_sequence_cameras(ctx):
    """set_camera(K_q, q) on a 2-sequence Harris pipeline: each sequence equals a one-sequence pipeline built with K_q
    (its scene rendered through that camera)."""
    from vo import synthetic
    H, W, N, F, S = 480, 640, 500, 5, 2
    K0 = synthetic.intrinsics(H, W)
    K1 = K0.copy()
    K1[0, 0] *= 1.15
    K1[1, 1] *= 1.15
    K1[0, 2] += 7.0
    Ks = [K0, K1]
    streams = [synthetic.Stream(F, H, W, seed=2023 + 7 * q, start=q, K=Ks[q]) for q in range(S)]
    starts = [start_state(streams[q], N) for q in range(S)]
    pairs = [(k, k + 1) for k in range(F - 1)]
    single = []
    for q in range(S):
        pipe = harris_pipe(ctx, H, W, F, Ks[q], N)
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i))
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1])
        res = drive(pipe, pairs, True)
        single.append(([r[0] for r in res], snapshot(pipe, 0)))
        pipe.close()
    pipe = harris_pipe(ctx, H, W, F, K0, N, S=S)
    for q in range(S):
        pipe.set_camera(Ks[q], q)
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    got = drive(pipe, pairs, True)
    for q in range(S):
        for k in range(len(pairs)):
            assert got[k][q].fault == 0
            assert_records_equal(got[k][q], single[q][0][k], ("sequence", q, "step", k))
        assert_snapshots_equal(snapshot(pipe, q), single[q][1], ("sequence", q))
    pipe.close()


def test_harris_sequences_checkpoint_and_rewind(ctx):
    """S = 2: checkpoint, three steps, rewind, the same three steps again.  Every sequence equals a one-sequence Harris
    pipeline making the same calls (the RANSAC fields and the generator go on across a rewind, so the second pass is
    compared with those pipelines' second pass, not with the first)."""
    H, W, N, F, S = 480, 640, 500, 5, 2
    streams = scenes(S, F, H, W)
    starts = [start_state(streams[q], N, (1.0, 0.85)[q]) for q in range(S)]
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
        pipe = harris_pipe(ctx, H, W, F, streams[q].K, N)
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i))
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1])
        single.append(run(pipe, [0]))
        pipe.close()
    pipe = harris_pipe(ctx, H, W, F, streams[0].K, N, S=S)
    for q in range(S):
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    got = run(pipe, range(S))
    for q in range(S):
        for p in range(2):
            res, snaps = got[p]
            ref_res, ref_snaps = single[q][p]
            for k in range(len(pairs)):
                assert res[k][q].fault == 0
                assert_records_equal(res[k][q], ref_res[k][0], ("sequence", q, "pass", p, "step", k))
            assert_snapshots_equal(snaps[q], ref_snaps[0], ("sequence", q, "pass", p))
        # the second pass starts from the checkpoint again: same features, the estimator went on
        assert got[1][0][0][q].n_features_in == got[0][0][0][q].n_features_in
    pipe.close()


def test_harris_sequences_one_sequence_against_the_oracle_loop(ctx):
    """Sequence 1 of an S = 2 Harris pipeline against OracleLoop(tracker="harris") for four steps: the batched path is
    tied to the oracle, not only to itself."""
    from test_gpu_pipeline import check_step
    H, W, N, F, S = 480, 640, 500, 5, 2
    streams = scenes(S, F, H, W)
    starts = [start_state(streams[q], N) for q in range(S)]
    pipe = harris_pipe(ctx, H, W, F, streams[0].K, N, S=S)
    for q in range(S):
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    orc = OracleLoop(streams[1], N, 15, 2, refine_iters=20, tracker="harris")
    orc.set_state(0, starts[1][0], starts[1][1], starts[1][1])

    class SequenceView:            # check_step reads sequence 0's state / generator: point it at sequence 1
        def get_state(self):
            return pipe.get_state(seq=1)

        def rng_state_into(self, g):
            pipe.rng_state_into(g, seq=1)

    for a, b in [(k, k + 1) for k in range(4)]:
        ref = orc.step(b)
        pipe.submit(a, b)
        r = pipe.collect_all()[1]
        assert r.n_features_in == N and r.n_tracked == N and r.n_triangulated >= 8
        check_step(r, ref, SequenceView(), orc.rs.rng, land_tol=1e-4)
    pipe.close()


def test_harris_sequences_at_configuration_size(ctx):
    """S = 4 at 1376 x 1241 with 2000 keypoints (the matcher's real splits, a 4000-row regroup), three steps: each sequence
    equals its one-sequence pipeline."""
    H, W, N, F, S = 1241, 1376, 2000, 4, 4
    streams = scenes(S, F, H, W)
    starts = [start_state(streams[q], N, (1.0, 0.9, 1.0, 0.75)[q]) for q in range(S)]
    pairs = [(k, k + 1) for k in range(3)]
    single = []
    for q in range(S):
        pipe = harris_pipe(ctx, H, W, F, streams[q].K, N)
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i))
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1])
        res = drive(pipe, pairs, True)
        single.append(([r[0] for r in res], snapshot(pipe, 0)))
        pipe.close()
    pipe = harris_pipe(ctx, H, W, F, streams[0].K, N, S=S)
    for q in range(S):
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    got = drive(pipe, pairs, True)
    for q in range(S):
        for k in range(len(pairs)):
            assert got[k][q].fault == 0
            assert_records_equal(got[k][q], single[q][0][k], ("sequence", q, "step", k))
        assert_snapshots_equal(snapshot(pipe, q), single[q][1], ("sequence", q))
    pipe.close()


def test_harris_sequences_refusals(ctx):
    """The SIFT mode still runs one sequence per pipeline; Harris-mode lanes are not there yet; the two descriptor entry
    points refuse a sequence the pipeline does not have."""
    from vo import _native
    from vo._native import VoError
    H, W, N, F, S = 240, 320, 300, 3, 2
    streams = scenes(S, F, H, W)
    with pytest.raises(VoError, match="SIFT"):
        _native.Pipeline(ctx, H, W, F, streams[0].K, n_keypoints=N, tracker="sift", sequences=2)
    pipe = harris_pipe(ctx, H, W, F, streams[0].K, N, S=S)
    starts = [start_state(streams[q], N) for q in range(S)]
    for q in range(S):
        for i in range(F):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    with pytest.raises(VoError):
        pipe.set_active(1, False)
    with pytest.raises(VoError):
        pipe.restart(1, 0, starts[1][0], starts[1][1])
    desc = np.zeros((4, 361), np.float32)
    import ctypes as C
    for seq in (-1, S):
        with pytest.raises(VoError):
            ctx._chk(ctx._lib.vo_pipeline_set_descriptors_seq(pipe._h, seq, desc.ctypes.data_as(C.c_void_p), 4))
        with pytest.raises(VoError):
            pipe.get_descriptors(seq=seq)
    # (refused calls change nothing: the pipeline still runs)
    pipe.submit(0, 1)
    rs = pipe.collect_all()
    assert all(r.fault == 0 for r in rs)
    pipe.close()
