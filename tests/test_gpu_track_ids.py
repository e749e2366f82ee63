"""-m gpu: persistent track ids through the device-resident loop (vo_pipeline_config.track_ids; include/vo_hip.h, "Track
ids") and the per-step observation record.  After every blocking step Pipeline.get_track_ids is compared exactly with the
rule in NumPy (tests/track_ids_oracle.py) fed from the CPU oracle loop -- never from the pipeline under test -- together
with get_state's keypoints in the same order; every feature of every step is compared."""
import numpy as np
import pytest

import pipeline_shi_tomasi_oracle as sto
import track_ids_oracle as tio
from pipeline_oracle import OracleLoop, initial_features, initial_harris_features, initial_sift_features
from test_gpu_pipeline import make_pipe, start_state

pytestmark = pytest.mark.gpu

H, W, N, HYP, FRAMES = 240, 320, 300, 256, 5


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def snapshot(ref):
    """What a test compares of one oracle step, detached from the loop's live objects."""
    return dict(ids=ref["ids"], born=ref["born"], next_id=ref["next_id"], n=ref["features"].length,
                keypoints=ref["features"].keypoints.astype(np.float64).copy(), appended=ref.get("appended", 0),
                appended_dropped=ref.get("appended_dropped", 0), unmatched=ref.get("unmatched", 0))


def check_ids(pipe, ref, seq=0, where=None):
    ids, born, nxt = pipe.get_track_ids(seq)
    st = pipe.get_state(seq)
    assert st["n"] == ref["n"] == len(ids), where
    assert np.array_equal(st["keypoints"], ref["keypoints"]), where
    assert np.array_equal(ids, ref["ids"]), (where, np.flatnonzero(ids != ref["ids"])[:5])
    assert np.array_equal(born, ref["born"]), where
    assert nxt == ref["next_id"], (where, nxt, ref["next_id"])
    assert len(np.unique(ids)) == len(ids) and (ids < nxt).all() and (ids >= 0).all()


_case1 = {}


def case1():
    """Case 1's inputs and its oracle run, computed once: 240 x 320, N = 300, 8 steps of stream.order(8) from 70 % of the
    detector's keypoints, so the first step re-detects: 510 tracker inputs, three workgroups of the KLT regroup."""
    if not _case1:
        from vo import synthetic
        stream = synthetic.Stream(FRAMES, H, W)
        feats, T = start_state(stream, N, 0.7)
        order = stream.order(8)
        pairs = list(zip(order[:-1], order[1:]))
        orc = OracleLoop(stream, N, 15, 2, refine_iters=20)
        orc.set_state(0, feats, T, T)
        rec = tio.Recorder(orc)
        refs = [snapshot(rec.step(b)) for _, b in pairs]
        assert refs[0]["appended"] == N and feats.length + N == 510, "the first step was meant to re-detect"
        assert refs[0]["appended_dropped"] >= 1, "an appended keypoint was meant to be dropped in the step that appends it"
        _case1.update(stream=stream, feats=feats, T=T, pairs=pairs, refs=refs)
    return _case1


def case1_pipe(ctx, track_ids=True, **kw):
    c = case1()
    pipe = make_pipe(ctx, c["stream"], N, HYP, track_ids=track_ids, **kw)
    pipe.set_state(0, c["feats"], c["T"], c["T"])
    return pipe


def record_buffers(ctx, pipe, count):
    nbytes = pipe.tracks_record_bytes(pipe.cap)
    assert nbytes % 16 == 0
    return ctx.to_device(np.zeros(count * nbytes, np.uint8)), nbytes


def read_records(ctx, pipe, d, nbytes, count):
    pipe.export_state_join()
    ctx.sync()
    out = [pipe.read_tracks_record(d + k * nbytes, pipe.cap) for k in range(count)]
    ctx.free(d)
    return out


def record_words(rec):
    """Everything a record holds, bit for bit: the header and the rows as bytes."""
    return (rec.n, rec.step, rec.next_id, rec.seq, np.asarray(rec).tobytes())


_blocking = {}


def blocking_records(ctx):
    """Case 1 stepped blocking with the field on: every step's record, posted right after its collect; each checked
    against what get_track_ids / get_state return at that moment."""
    if not _blocking:
        c = case1()
        pipe = case1_pipe(ctx)
        d, nbytes = record_buffers(ctx, pipe, len(c["pairs"]))
        results, states = [], []
        for k, (a, b) in enumerate(c["pairs"]):
            r = pipe.step(a, b)
            pipe.export_tracks_post(r, pipe.cap, d + k * nbytes)
            results.append(r)
            states.append((pipe.get_track_ids(), pipe.get_state()))
        recs = read_records(ctx, pipe, d, nbytes, len(c["pairs"]))
        pipe.close()
        for k, (rec, ((ids, born, nxt), st)) in enumerate(zip(recs, states)):
            assert (rec.n, rec.step, rec.next_id, rec.seq) == (st["n"], k + 1, nxt, 0) and len(rec) == st["n"]
            assert np.array_equal(rec["id"], ids) and np.array_equal(rec["born"], born)
            kp = st["keypoints"][:, :, 0].astype(np.float32)
            assert np.array_equal(rec["x"].view(np.uint32), kp[:, 0].copy().view(np.uint32))
            assert np.array_equal(rec["y"].view(np.uint32), kp[:, 1].copy().view(np.uint32))
            assert np.array_equal(rec["state"], st["state"].astype(np.int32))
            assert np.array_equal(rec["candidate"], st["candidate_mask"].astype(np.int32))
            land = np.stack([rec["X"], rec["Y"], rec["Z"]], axis=1)
            tri = st["state"] == 2
            assert np.array_equal(land[tri].view(np.uint64), st["landmarks"][tri, :, 0].copy().view(np.uint64))
            assert np.isnan(land[~tri]).all()
        _blocking.update(records=recs, results=results)
    return _blocking


def test_klt_mode_with_the_harris_detector(ctx):
    """1. Survivors keep (id, born) through filter and regroup, the 300 appended keypoints of the first step are numbered
    behind next_id -- the dropped ones included -- across three workgroups of the regroup kernel."""
    c = case1()
    pipe = case1_pipe(ctx)
    ids, born, nxt = pipe.get_track_ids()
    n0 = c["feats"].length
    assert np.array_equal(ids, np.arange(n0)) and not born.any() and nxt == n0
    assert np.array_equal(pipe.get_features().uids, np.arange(n0))
    redetects = 0
    for k, ((a, b), ref) in enumerate(zip(c["pairs"], c["refs"])):
        r = pipe.step(a, b)
        assert r.fault == 0 and r.recovered == 0
        redetects += r.redetected
        assert r.n_features_in == (n0 if k == 0 else c["refs"][k - 1]["n"]) + ref["appended"]
        check_ids(pipe, ref, where=("step", k))
    assert redetects >= 1 and c["refs"][0]["next_id"] == n0 + N
    assert np.array_equal(pipe.get_features().uids, c["refs"][-1]["ids"])
    pipe.close()


@pytest.mark.parametrize("name", ["B", "D"])
def test_klt_mode_with_the_shi_tomasi_detector(ctx, name):
    """2. The appended count is what the frame has (226 / 121 corners, below the cap of 300), at the step that re-detects
    (born = 2)."""
    from test_gpu_pipeline_shi_tomasi import make_pipe as st_pipe
    stream, feats, T, loop, pairs = sto.case(name)
    when, count = sto.CASES[name][4:]
    rec = tio.Recorder(loop)
    pipe = st_pipe(ctx, name, stream, redetect_start_pose="current", track_ids=True)
    pipe.set_state(0, feats, T, T)
    for k, (a, b) in enumerate(pairs):
        ref = snapshot(rec.step(b))
        r = pipe.step(a, b)
        assert r.fault == 0
        check_ids(pipe, ref, where=(name, "step", k))
        assert ref["appended"] == (count if k == when else 0) and r.redetected == (1 if k == when else 0)
    assert count < sto.N and ref["next_id"] == feats.length + count
    assert (ref["born"] == when).sum() > 0 and set(np.unique(ref["born"])) <= {0, when}
    pipe.close()


@pytest.mark.parametrize("fault_every,lookahead", [(3, False), (-1, False), (3, True), (-3, True)])
def test_redone_steps_issue_the_same_ids(ctx, fault_every, lookahead):
    """3. A step forced off the device path -- at the regroup (> 0) or at the pose kernel (< 0: its regroup has run once
    when the host path runs it again) -- and the steps enqueued again behind it issue the ids of the run without faults."""
    c = case1()
    pipe = case1_pipe(ctx, debug_fault_every=fault_every)
    every = abs(fault_every)
    if lookahead:
        base = blocking_records(ctx)["records"]
        d, nbytes = record_buffers(ctx, pipe, len(c["pairs"]))
        got = []
        pipe.submit(*c["pairs"][0])
        for k in range(len(c["pairs"])):
            if k + 1 < len(c["pairs"]):
                pipe.submit(*c["pairs"][k + 1])
            got.append(pipe.collect())
            pipe.export_tracks_post(got[-1], pipe.cap, d + k * nbytes)
        recs = read_records(ctx, pipe, d, nbytes, len(c["pairs"]))
        for k, (rec, ref) in enumerate(zip(recs, c["refs"])):
            assert np.array_equal(rec["id"], ref["ids"]) and np.array_equal(rec["born"], ref["born"]), k
            assert rec.next_id == ref["next_id"] and rec.step == k + 1
            assert record_words(rec) == record_words(base[k]), k
        check_ids(pipe, c["refs"][-1])
    else:
        got = []
        for k, ((a, b), ref) in enumerate(zip(c["pairs"], c["refs"])):
            got.append(pipe.step(a, b))
            check_ids(pipe, ref, where=("step", k))
    for k in range(every - 1, len(c["pairs"]), every):
        assert got[k].recovered == 1, k
    pipe.close()


def test_records_posted_with_a_step_in_flight(ctx):
    """4. Every step's record, posted right after its collect while the next step is in flight, equals the blocking run's
    bit for bit: ids, born, keypoints, state, candidate, landmarks and the header."""
    c = case1()
    base = blocking_records(ctx)["records"]
    pipe = case1_pipe(ctx)
    d, nbytes = record_buffers(ctx, pipe, len(c["pairs"]))
    pipe.submit(*c["pairs"][0])
    for k in range(len(c["pairs"])):
        if k + 1 < len(c["pairs"]):
            pipe.submit(*c["pairs"][k + 1])
        r = pipe.collect()
        pipe.export_tracks_post(r, pipe.cap, d + k * nbytes)
    recs = read_records(ctx, pipe, d, nbytes, len(c["pairs"]))
    pipe.close()
    for k, (rec, ref) in enumerate(zip(recs, base)):
        assert (rec.n, rec.step, rec.next_id, rec.seq) == (ref.n, ref.step, ref.next_id, ref.seq), k
        for f in ("id", "born", "state", "candidate"):
            assert np.array_equal(rec[f], ref[f]), (k, f)
        for f in ("x", "y"):
            assert np.array_equal(rec[f].view(np.uint32), ref[f].view(np.uint32)), (k, f)
        for f in ("X", "Y", "Z"):
            assert np.array_equal(rec[f].view(np.uint64), ref[f].view(np.uint64)), (k, f)
        assert record_words(rec) == record_words(ref), k
        assert np.array_equal(rec["id"], c["refs"][k]["ids"])


def test_sequences_number_independently(ctx):
    """5. S = 3 in KLT mode, three scenes, start fractions (1.0, 0.7, 1.0): each sequence equals its own one-sequence
    pipeline after every step."""
    from vo import _native, synthetic
    S = 3
    streams = [synthetic.Stream(FRAMES, H, W, seed=2023 + 7 * q, start=q) for q in range(S)]
    starts = [start_state(streams[q], N, (1.0, 0.7, 1.0)[q]) for q in range(S)]
    order = streams[0].order(8)
    pairs = list(zip(order[:-1], order[1:]))
    single = []
    for q in range(S):
        pipe = make_pipe(ctx, streams[q], N, HYP, track_ids=True)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1])
        steps = []
        for a, b in pairs:
            pipe.step(a, b)
            ids, born, nxt = pipe.get_track_ids()
            steps.append(dict(ids=ids, born=born, next_id=nxt, n=len(ids), keypoints=pipe.get_state()["keypoints"]))
        single.append(steps)
        pipe.close()
    pipe = _native.Pipeline(ctx, H, W, FRAMES, streams[0].K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP,
                            p3p_threshold=1.0, max_iterations=1000, refine_iters=20, sequences=S, track_ids=True)
    for q in range(S):
        for i in range(FRAMES):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    for k, (a, b) in enumerate(pairs):
        pipe.submit(a, b)
        pipe.collect_all()
        for q in range(S):
            check_ids(pipe, single[q][k], seq=q, where=("sequence", q, "step", k))
    assert len({single[q][-1]["next_id"] for q in range(S)}) > 1, "the sequences' next_id values were meant to differ"
    assert single[1][0]["next_id"] == starts[1][0].length + N
    pipe.close()


_harris = {}


def stop_and_go(n_frames, height, width):
    """A camera that stands still every other frame (frames 0, 0, 1, 1, ... of the scene): a step between two equal
    images matches every keypoint (more pairs than the pair regroup has work items), the next one the stream's usual
    third of them (most new keypoints unmatched)."""
    from vo import synthetic

    class StopAndGo(synthetic.Stream):
        def _job(self, i):
            return super()._job(i // 2)

        def depth(self, i):
            return synthetic.render(self.start + i // 2, self.H, self.W, self.seed)[1]

        def T_world_cam(self, i):
            return synthetic.pose_world_cam(self.start + i // 2)

    return StopAndGo(n_frames, height, width)


def harris_case(monkeypatch, S, n_keypoints, steps):
    """The Harris-mode oracle runs at 480 x 640, computed once per (S, N): S scenes, or (S = 0) the stop-and-go stream."""
    key = (S, n_keypoints)
    if key not in _harris:
        from vo import synthetic
        F = steps + 1
        streams = ([synthetic.Stream(F, 480, 640, seed=2023 + 7 * q, start=q) for q in range(S)] if S
                   else [stop_and_go(F, 480, 640)])
        starts = [initial_harris_features(st, 0, n_keypoints) for st in streams]
        refs = []
        for q, st in enumerate(streams):
            orc = OracleLoop(st, n_keypoints, 15, 2, refine_iters=20, tracker="harris")
            orc.set_state(0, *starts[q], starts[q][1])
            rec = tio.Recorder(orc, monkeypatch)
            refs.append([snapshot(rec.step(b)) for b in range(1, F)])
        _harris[key] = (streams, starts, refs)
    return _harris[key]


@pytest.mark.parametrize("fault_every", [0, 4])
def test_harris_mode_two_sequences(ctx, monkeypatch, fault_every):
    """6. S = 2 at 480 x 640, N = 500, 5 steps against the oracle: pairs keep the old feature's (id, born), the unmatched
    new keypoints are numbered in ascending keypoint index with born = k + 1 -- also with every fourth step forced off the
    device path at the pair regroup."""
    from vo import _native
    S, n, steps = 2, 500, 5
    streams, starts, refs = harris_case(monkeypatch, S, n, steps)
    pipe = _native.Pipeline(ctx, 480, 640, steps + 1, streams[0].K, n_keypoints=n, hyp=256, p3p_threshold=1.0,
                            max_iterations=1000, refine_iters=20, tracker="harris", sequences=S, track_ids=True,
                            debug_fault_every=fault_every)
    for q in range(S):
        for i in range(steps + 1):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    for k in range(steps):
        pipe.submit(k, k + 1)
        rs = pipe.collect_all()
        for q in range(S):
            assert rs[q].recovered == (1 if fault_every and k % fault_every == fault_every - 1 else rs[q].recovered)
            check_ids(pipe, refs[q][k], seq=q, where=("sequence", q, "step", k))
            assert (refs[q][k]["born"] == k + 1).sum() == refs[q][k]["unmatched"] > 0
    assert np.array_equal(pipe.get_features(1).uids, refs[1][-1]["ids"])
    pipe.close()


def test_harris_mode_two_items_per_work_item(ctx, monkeypatch):
    """6. N = 1200 on the stop-and-go stream: the pair regroup's 1024 work items hold two pairs each on the steps between
    equal images, and two new keypoints each in the unmatched tail on the step between them."""
    from vo import _native
    n, steps = 1200, 3
    streams, starts, refs = harris_case(monkeypatch, 0, n, steps)
    pipe = _native.Pipeline(ctx, 480, 640, steps + 1, streams[0].K, n_keypoints=n, hyp=256, p3p_threshold=1.0,
                            max_iterations=1000, refine_iters=20, tracker="harris", track_ids=True)
    for i in range(steps + 1):
        pipe.set_frame(i, streams[0].image(i))
    pipe.set_state(0, starts[0][0], starts[0][1], starts[0][1])
    for k in range(steps):
        r = pipe.step(k, k + 1)
        assert r.n_features_in == n > 1024
        check_ids(pipe, refs[0][k], where=("step", k))
    assert n - refs[0][0]["unmatched"] > 1024, "two pairs per work item were meant (the camera stands still)"
    assert refs[0][1]["unmatched"] > 0 and (refs[0][1]["born"] == 2).sum() == refs[0][1]["unmatched"]
    pipe.close()


def test_sift_mode(ctx, monkeypatch):
    """7. 240 x 320, sift_cap = 300, 4 steps against the oracle."""
    from vo import _native, synthetic
    F = 5
    stream = synthetic.Stream(F, H, W)
    feats, T = initial_sift_features(stream, 0, N)
    orc = OracleLoop(stream, N, 15, 2, refine_iters=20, tracker="sift")
    orc.set_state(0, feats, T, T)
    rec = tio.Recorder(orc, monkeypatch)
    pipe = _native.Pipeline(ctx, H, W, F, stream.K, n_keypoints=N, hyp=256, p3p_threshold=1.0, max_iterations=1000,
                            refine_iters=20, tracker="sift", sift_cap=N, track_ids=True)
    for i in range(F):
        pipe.set_frame(i, stream.image(i))
    pipe.set_state(0, feats, T, T)
    for k in range(F - 1):
        ref = snapshot(rec.step(k + 1))
        pipe.step(k, k + 1)
        check_ids(pipe, ref, where=("step", k))
        assert ref["unmatched"] > 0 and (ref["born"] == k + 1).sum() == ref["unmatched"]
    pipe.close()


def test_checkpoint_and_rewind(ctx):
    """8. S = 2, KLT mode: checkpoint, three steps, rewind, the same three steps.  The ids and next_id of the second pass
    are the first pass's: the same set of ids after every step, every id on the same keypoint (the tracker does not depend
    on the pose).  Compared by id, not by row: the estimator's RANSAC fields and generator go on across a rewind, so the
    second pass resets other outliers and the regroup orders the survivors differently.  born of the tracks started in the
    second pass is three larger (the step counter is not rewound)."""
    from vo import _native, synthetic
    S = 2
    streams = [synthetic.Stream(FRAMES, H, W, seed=2023 + 7 * q, start=q) for q in range(S)]
    starts = [start_state(streams[q], N, (0.7, 1.0)[q]) for q in range(S)]
    pipe = _native.Pipeline(ctx, H, W, FRAMES, streams[0].K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP,
                            p3p_threshold=1.0, max_iterations=1000, refine_iters=20, sequences=S, track_ids=True)
    for q in range(S):
        for i in range(FRAMES):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    pipe.checkpoint()
    passes = []
    for p in range(2):
        if p:
            pipe.rewind()
            for q in range(S):
                ids, born, nxt = pipe.get_track_ids(q)
                n0 = starts[q][0].length
                assert np.array_equal(ids, np.arange(n0)) and not born.any() and nxt == n0
        steps = []
        for k in range(3):
            pipe.submit(k, k + 1)
            pipe.collect_all()
            steps.append([pipe.get_track_ids(q) + (pipe.get_state(q)["keypoints"],) for q in range(S)])
        passes.append(steps)
    started = 0
    for k in range(3):
        for q in range(S):
            (i1, b1, n1, kp1), (i2, b2, n2, kp2) = passes[0][k][q], passes[1][k][q]
            o1, o2 = np.argsort(i1), np.argsort(i2)
            assert len(np.unique(i1)) == len(i1) and len(np.unique(i2)) == len(i2)
            assert np.array_equal(i1[o1], i2[o2]) and n1 == n2, (k, q)
            assert np.array_equal(kp1[o1], kp2[o2]), (k, q)
            old = i1[o1] < starts[q][0].length
            assert np.array_equal(b1[o1][old], b2[o2][old]) and not b1[o1][old].any(), (k, q)
            assert np.array_equal(b1[o1][~old] + 3, b2[o2][~old]), (k, q)
            started += int((~old).sum())
    assert started > 0 and passes[0][0][0][2] == starts[0][0].length + N, "sequence 0 was meant to start tracks in the pass"
    pipe.close()


def test_restart_numbers_its_lane_alone(ctx):
    """9. restart_seq on lane 1 of a 2-lane pipeline: lane 1 gets 0 .. n-1, lane 0 keeps its ids."""
    from vo import _native, synthetic
    S = 2
    streams = [synthetic.Stream(FRAMES, H, W, seed=2023 + 7 * q, start=q) for q in range(S)]
    starts = [start_state(streams[q], N, 0.7) for q in range(S)]
    pipe = _native.Pipeline(ctx, H, W, FRAMES, streams[0].K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP,
                            p3p_threshold=1.0, max_iterations=1000, refine_iters=20, sequences=S, track_ids=True)
    for q in range(S):
        for i in range(FRAMES):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    for k in range(2):
        pipe.submit(k, k + 1)
        pipe.collect_all()
    before = [pipe.get_track_ids(q) for q in range(S)]
    assert before[1][2] == starts[1][0].length + N and not np.array_equal(before[1][0], np.arange(len(before[1][0])))
    f1, T1 = initial_features(streams[1], 2, N)
    pipe.restart(1, 2, f1, T1, T1)
    ids, born, nxt = pipe.get_track_ids(1)
    assert np.array_equal(ids, np.arange(f1.length)) and not born.any() and nxt == f1.length
    for a, b in zip(before[0], pipe.get_track_ids(0)):
        assert np.array_equal(a, b)
    pipe.submit(2, 3)
    rs = pipe.collect_all()
    assert rs[0].fault == 0 and rs[1].fault == 0
    ids, born, nxt = pipe.get_track_ids(1)
    assert (ids < f1.length).all() and nxt == f1.length and not born.any()      # (a lane at full count does not re-detect)
    pipe.close()


def test_bootstrap_numbers_the_features(ctx):
    """9. bootstrap_seq on a two-frame case: 0 .. n-1, born 0, next_id = n."""
    from test_gpu_pipeline_bootstrap import SMALL, device_pipe, recording
    pipe, res = device_pipe(ctx, SMALL, recording(SMALL, 2023), track_ids=True)
    ids, born, nxt = pipe.get_track_ids()
    assert res.n_features > 0 and len(ids) == res.n_features == nxt
    assert np.array_equal(ids, np.arange(nxt)) and not born.any()
    pipe.close()


def test_set_track_ids_round_trip_and_refusals(ctx):
    """9. set_track_ids: survivors keep what was set, new ids start at the next_id that was set; every refused call leaves
    a pipeline that still steps."""
    from vo import _native
    c = case1()
    pipe = case1_pipe(ctx)
    n0 = c["feats"].length
    rng = np.random.default_rng(5)
    mine = (1000 + rng.permutation(3 * n0)[:n0]).astype(np.int32)
    born = rng.integers(0, 9, n0).astype(np.int32)
    refused = [(dict(ids=mine[:-1], next_id=5000), "features"),                       # wrong n
               (dict(ids=np.concatenate((mine[:-1], mine[:1])), next_id=5000), "twice"),   # a duplicate
               (dict(ids=mine, next_id=int(mine.max())), "next_id"),                 # an id >= next_id
               (dict(ids=mine, next_id=5000, seq=1), "sequence")]                      # a bad seq
    for kw, word in refused:
        with pytest.raises(_native.VoError, match=word):
            pipe.set_track_ids(**kw)
    with pytest.raises(_native.VoError, match="sequence"):
        pipe.get_track_ids(seq=-1)
    ids, b, nxt = pipe.get_track_ids()
    assert np.array_equal(ids, np.arange(n0)) and nxt == n0, "a refused call changes nothing"
    pipe.set_track_ids(mine, 5000, born=born)
    ids, b, nxt = pipe.get_track_ids()
    assert np.array_equal(ids, mine) and np.array_equal(b, born) and nxt == 5000
    pipe.set_track_ids(mine, 5000)                      # born = None: left as it is
    assert np.array_equal(pipe.get_track_ids()[1], born)
    # the oracle's rule from what was set
    e_ids, e_born, e_next = mine, born, 5000
    prev_n = n0
    for k, (a, b_) in enumerate(c["pairs"][:2]):
        if k == 1:                                       # a call with a step in flight
            pipe.submit(a, b_)
            with pytest.raises(_native.VoError, match="not collected"):
                pipe.set_track_ids(np.arange(prev_n), prev_n)
            with pytest.raises(_native.VoError, match="not collected"):
                pipe.get_track_ids()
            r = pipe.collect()
        else:
            r = pipe.step(a, b_)
        assert r.fault == 0
        ref = c["refs"][k]
        # case 1 numbered from the hand-over: old ids < n0 map to what was set, issued ids move by 5000 - n0
        expect = np.where(ref["ids"] < n0, mine[np.minimum(ref["ids"], n0 - 1)], ref["ids"] - n0 + 5000)
        expect_born = np.where(ref["ids"] < n0, born[np.minimum(ref["ids"], n0 - 1)], ref["born"])
        ids, b, nxt = pipe.get_track_ids()
        assert np.array_equal(ids, expect) and np.array_equal(b, expect_born) and nxt == ref["next_id"] - n0 + 5000
        prev_n = len(ids)
    assert (ids >= 5000).sum() > 0 and (ids < 5000).sum() > 0
    pipe.close()


def test_off_is_off(ctx):
    """10. track_ids = 0: the four entry points refuse naming the field, uids stays None, and case 1 gives identical
    records and arrays with the field on and off."""
    from vo import _native
    from test_gpu_harris_sequences import NOT_COMPARED
    c = case1()
    runs = []
    for on in (False, True):
        # detect_margin < 0: the detector executes on every frame, so detector_ran is determined and stays in the comparison.
        # (With a margin, detect_decide_kernel predicts on the detection stream, ordered only behind the frame's upload, from
        #  control-block fields the main stream's regroup may be writing at that moment -- csrc/pipeline_step.hip -- and two
        #  runs of one pipeline need not agree in the field near the limit, blocking steps included.)
        pipe = case1_pipe(ctx, track_ids=on, detect_margin=-1.0)
        if not on:
            d = ctx.alloc(pipe.tracks_record_bytes(pipe.cap))
            for call in (lambda: pipe.get_track_ids(), lambda: pipe.set_track_ids(np.arange(c["feats"].length), 1000),
                         lambda: pipe.export_tracks_post(_native.StepResult(), pipe.cap, d)):
                with pytest.raises(_native.VoError, match="track_ids"):
                    call()
            ctx.free(d)
            assert pipe.tracks_record_bytes(10) == 16 + 480
            assert pipe.get_features().uids is None
        steps = []
        for a, b in c["pairs"]:
            r = pipe.step(a, b)
            rec = {name: (tuple(v) if hasattr(v, "__len__") else v)
                   for name, _ in _native.StepResult._fields_ if name not in NOT_COMPARED for v in [getattr(r, name)]}
            steps.append((rec, pipe.get_state()))
        runs.append(steps)
        pipe.close()
    for k, ((ra, sa), (rb, sb)) in enumerate(zip(*runs)):
        assert ra == rb, (k, [(f, ra[f], rb[f]) for f in ra if ra[f] != rb[f]][:3])
        assert set(sa) == set(sb)
        for key in sa:
            assert np.array_equal(sa[key], sb[key], equal_nan=True), (k, key)


def check_observations(out, plain):
    from vo.driver import track_table
    assert np.array_equal(out["trajectory"], plain["trajectory"])
    obs = out["observations"]
    assert len(obs) == len(out["results"]) == len(plain["results"])
    for t, (rec, r) in enumerate(zip(obs, out["results"])):
        assert rec.n == r.n_tracked == len(rec) and rec.step == t + 1
    assert np.array_equal(obs[-1]["id"], out["features"].uids)
    table = track_table(obs)
    assert sum(len(e["steps"]) for e in table.values()) == sum(len(rec) for rec in obs)
    born_later = 0
    for i, e in table.items():
        steps = e["steps"]
        assert np.array_equal(steps, np.arange(steps[0], steps[0] + len(steps))), i
        # (a track handed over, born 0, may have been lost in the first step: only those that were seen are in the table)
        assert steps[0] == e["born"], (i, steps[0], e["born"])
        born_later += e["born"] > 0
        for t, kp in zip(steps, e["keypoints"]):
            row = obs[t][obs[t]["id"] == i]
            assert len(row) == 1 and row["x"][0] == kp[0] and row["y"][0] == kp[1] and row["born"][0] == e["born"]
    return born_later


def test_run_on_device_with_tracks(ctx):
    """11. run_on_device(tracks=True): the trajectory of the run without, one record per step, and a track table whose
    every id is seen on consecutive steps from its born on."""
    from vo import driver
    from vo.primitives import Sequence

    def seq():
        return Sequence("synthetic", n_frames=12, height=240, width=320)
    plain = driver.run_on_device(seq(), n_keypoints=300, context=ctx)
    assert "observations" not in plain and plain["features"].uids is None
    out = driver.run_on_device(seq(), n_keypoints=300, context=ctx, tracks=True)
    check_observations(out, plain)


def test_run_batch_on_device_with_tracks(ctx):
    """11. The same through run_batch_on_device, two recordings on two lanes."""
    from vo import driver
    from vo.primitives import Sequence

    def seqs():
        return [Sequence("synthetic", n_frames=12 - 2 * i, height=240, width=320, seed=2023 + 11 * i) for i in range(2)]
    kw = dict(n_keypoints=300, context=ctx)
    plain = driver.run_batch_on_device(seqs(), lanes=2, **kw)
    out = driver.run_batch_on_device(seqs(), lanes=2, tracks=True, **kw)
    for i in range(2):
        check_observations(out[i], plain[i])
        alone = driver.run_on_device(seqs()[i], tracks=True, **kw)
        assert len(alone["observations"]) == len(out[i]["observations"])
        for a, b in zip(alone["observations"], out[i]["observations"]):
            # (as bytes: the rows hold NaN landmarks, which compare unequal as numbers)
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes() and (a.n, a.step, a.next_id) == (b.n, b.step, b.next_id)
