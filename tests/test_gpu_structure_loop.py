"""-m gpu: the structure loop (include/vo_hip.h, "Structure loop"; csrc/structure_loop.hip) -- the last W observation
records kept in a ring on the device, and record, join, refinement and write-back queued on the pipeline's stream by one call
per collected step, with one further step in flight.

Everything here is equality of bits.  The join against tests/test_gpu_window_ba.py's numpy_window on that module's posted
loop; the refinement against Context.window_structure on the downloaded window; the write-back's lag rule against a
synchronous run built from the existing primitives alone (Pipeline.step, export_tracks_post, WindowStructureRefiner, a NumPy
filter, Pipeline.update_landmarks); lanes against each lane alone; the driver's ba_feedback="stream" against the same
construction.  Shapes: 240 x 320, 300 keypoints, W = 3, 4, 5, at most 12 frames."""
import numpy as np
import pytest

from pipeline_oracle import initial_features
from test_gpu_pipeline import make_pipe, start_state

pytestmark = pytest.mark.gpu

H, W_IMG, N, HYP, FRAMES = 240, 320, 300, 256, 5
PRM = dict(max_iter=4, gate_px=2.0)


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def posted(ctx):
    """tests/test_gpu_window_ba.py's posted loop on this module's context (its cache holds device pointers of the context
    that built it: emptied before and after)."""
    import test_gpu_window_ba as wb
    wb._loop.clear()
    lp = wb.posted_loop(ctx)
    yield lp
    lp["pipe"].close()
    ctx.free(lp["d"][0])
    wb._loop.clear()


def lane_stream(q):
    from vo import synthetic
    return synthetic.Stream(FRAMES, H, W_IMG, seed=2023 + 7 * q, start=q)


_inputs = {}


def lane_inputs(q):
    if q not in _inputs:
        s = lane_stream(q)
        _inputs[q] = (s, start_state(s, N, 0.7))
    return _inputs[q]


def lanes_pipe(ctx, qs, **kw):
    """A pipeline of len(qs) lanes: lane i runs scene qs[i] from 70 % of the detector's keypoints (the first step re-detects);
    one lane of scene 0 is the posted loop's shape."""
    from vo import _native
    streams = [lane_inputs(q)[0] for q in qs]
    pipe = _native.Pipeline(ctx, H, W_IMG, FRAMES, streams[0].K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP, p3p_threshold=1.0,
                            max_iterations=1000, refine_iters=20, sequences=len(qs), track_ids=True, **kw)
    for i, q in enumerate(qs):
        for f in range(FRAMES):
            pipe.set_frame(f, streams[i].image(f), seq=i)
        feats, T = lane_inputs(q)[1]
        pipe.set_state(0, feats, T, T, seq=i)
    return pipe


def pairs_of(steps):
    order = lane_stream(0).order(steps)
    return list(zip(order[:-1], order[1:]))


def state_bytes(pipe, seq=0):
    st = pipe.get_state(seq)
    ids, born, nxt = pipe.get_track_ids(seq)
    return tuple(np.asarray(st[k]).tobytes() for k in sorted(st)) + (ids.tobytes(), born.tobytes(), nxt)


def result_words(r):
    return (np.array(list(r.R_refined) + list(r.t_refined) + list(r.T_wc)).tobytes(), r.n_tracked, r.n_triangulated, r.n_inliers,
            r.n_candidates, r.n_landmarks, r.draws_consumed, r.redetected)


def record_bytes(rec):
    return (rec.n, rec.step, rec.next_id, rec.seq, np.asarray(rec).tobytes())


def run_b(ctx, qs, steps=10, window=3, feedback=True, fault_every=0, loop=True, lookahead=True, before_step=None, **loop_kw):
    """submit / collect with one step in flight (lookahead=False: none); every collected step's records exported and the
    step posted to the loop.  before_step(k, pipe, sl): a hook in front of step k's submit (lookahead=False only: nothing is
    in flight there).  Returns results [step][lane], records [step][lane], entries [step] (rows per lane), the final states
    and the landmarks alone."""
    pipe = lanes_pipe(ctx, qs, debug_fault_every=fault_every)
    sl = pipe.structure_loop(window, feedback=feedback, **dict(PRM, **loop_kw)) if loop else None
    S, pairs = len(qs), pairs_of(steps)
    nbytes = pipe.tracks_record_bytes(pipe.cap)
    d = ctx.to_device(np.zeros(steps * S * nbytes, np.uint8))
    results, posts = [], []
    if lookahead:
        pipe.submit(*pairs[0])
    for k in range(steps):
        if not lookahead:
            if before_step:
                before_step(k, pipe, sl)
            pipe.submit(*pairs[k])
        elif k + 1 < steps:
            pipe.submit(*pairs[k + 1])
        rs = pipe.collect_all()
        results.append(rs)
        for q in range(S):
            pipe.export_tracks_post(rs[q], pipe.cap, d + (k * S + q) * nbytes, seq=q)
        if sl:
            posts.append(sl.post(rs))
    entries = [sl.poll(j, wait=True) for j in posts] if sl else []
    pipe.export_state_join()
    ctx.sync()
    records = [[pipe.read_tracks_record(d + (k * S + q) * nbytes, pipe.cap) for q in range(S)] for k in range(steps)]
    out = dict(results=results, records=records, entries=entries, states=[state_bytes(pipe, q) for q in range(S)],
               landmarks=[pipe.get_state(q)["landmarks"] for q in range(S)], posts=posts)
    ctx.free(d)
    pipe.close()
    return out


def numpy_writeback(pipe, pending):
    """Item 5 of the rule in NumPy on the features the pipeline holds now: the ids and landmarks to write."""
    lm_id, X_in, X_ref, kept = pending
    st = pipe.get_state()
    ids = pipe.get_track_ids()[0]
    land = st["landmarks"][:, :, 0]
    row = {int(i): j for j, i in enumerate(ids)}
    sel_ids, sel_X = [], []
    for i in range(len(lm_id)):
        j = row.get(int(lm_id[i]))
        if j is None or st["state"][j] != 2 or not kept[i] or X_ref[i].tobytes() == X_in[i].tobytes():
            continue
        if land[j].tobytes() != X_in[i].tobytes():
            continue
        sel_ids.append(int(lm_id[i]))
        sel_X.append(X_ref[i])
    return np.array(sel_ids, np.int32), np.array(sel_X, np.float64).reshape(-1, 3)


def run_a(ctx, steps=10, window=3, fault_every=0):
    """The same loop from the existing primitives, nothing in flight: per step the record is exported and
    WindowStructureRefiner refines the records through k; after step k + 1 the four conditions are applied in NumPy and the
    landmarks written through Pipeline.update_landmarks, then record k + 1 is exported."""
    from vo.landmarks import WindowStructureRefiner
    pipe = lanes_pipe(ctx, [0], debug_fault_every=fault_every)
    sr = WindowStructureRefiner(pipe.K, window=window, cap=pipe.cap, context=ctx, **PRM)
    pairs = pairs_of(steps)
    nbytes = pipe.tracks_record_bytes(pipe.cap)
    d = ctx.to_device(np.zeros(steps * nbytes, np.uint8))
    results, records, written, summaries, pending = [], [], [], [], None

    def apply():
        ids, X = numpy_writeback(pipe, pending)
        pipe.update_landmarks(ids, X)
        written.append(len(ids))

    for k, (a, b) in enumerate(pairs):
        r = pipe.step(a, b)
        results.append([r])
        if pending is not None:
            apply()
        elif k > 0:
            written.append(0)
        pipe.export_tracks_post(r, pipe.cap, d + k * nbytes)
        rec = pipe.read_tracks_record(d + k * nbytes, pipe.cap)
        records.append([rec])
        sr.push(d + k * nbytes, np.concatenate((np.array(r.R_refined), np.array(r.t_refined))))
        out = sr.solve()
        pending = None
        summaries.append(None if out is None else out.summary)
        if out is not None:
            at = {int(i): j for j, i in enumerate(rec["id"])}
            X_in = np.array([[rec[at[int(i)]][c] for c in ("X", "Y", "Z")] for i in out.ids], np.float64).reshape(-1, 3)
            pending = (out.ids, X_in, out.landmarks, out.results["kept"])
    if pending is not None:                              # (the last post finds nothing in flight: the step's own features)
        apply()
    else:
        written.append(0)
    res = dict(results=results, records=records, written=written, summaries=summaries, states=[state_bytes(pipe)],
               landmarks=[pipe.get_state()["landmarks"]])
    sr.close()
    ctx.free(d)
    pipe.close()
    return res


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def plain(ctx):
    return cached("plain", lambda: run_b(ctx, [0], loop=False))


def fed(ctx):
    return cached("fed", lambda: run_b(ctx, [0]))


def alone(ctx, q):
    return fed(ctx) if q == 0 else cached(("alone", q), lambda: run_b(ctx, [q]))


def same_runs(a, b):
    for k, (ra, rb) in enumerate(zip(a["results"], b["results"])):
        assert [result_words(r) for r in ra] == [result_words(r) for r in rb], ("step", k)
    for k, (ra, rb) in enumerate(zip(a["records"], b["records"])):
        assert [record_bytes(r) for r in ra] == [record_bytes(r) for r in rb], ("record", k)
    assert a["states"] == b["states"]


# ---- 1, 2: the join and the refinement ----

@pytest.mark.parametrize("W", [3, 5])
def test_join_equals_the_builder_and_refinement_a_standalone_call(ctx, posted, W):
    from test_gpu_window_ba import numpy_window, same_window
    lp = posted
    cap = lp["cap"]
    want = numpy_window(lp["records"][-W:], cap, cap, cap * W)
    L, M = int(want["head"][0]), int(want["head"][1])
    assert L > 20 and want["head"][2] == 0
    for L_cap, M_cap, flag in ((None, None, 0), (L - 3, None, 1), (None, M - 1, 2), (L, int(want["lm_start"][L // 2]) + 1, 2)):
        pipe = lanes_pipe(ctx, [0])
        sl = pipe.structure_loop(W, L_cap=L_cap, M_cap=M_cap, feedback=False, **PRM)
        rs = []
        for a, b in pairs_of(8):                         # (8 posts into W slots: the ring wraps)
            rs.append(pipe.step(a, b))
            sl.post(rs[-1])
        got = sl.download()
        cut = numpy_window(lp["records"][-W:], cap, L_cap or cap, M_cap or (L_cap or cap) * W)
        assert cut["head"][2] == flag and (flag == 0 or cut["head"][0] < L)
        same_window(got.window(), cut)
        assert (got.entry["step"], got.entry["full"], got.entry["L"], got.entry["M"], got.entry["flags"]) == (
            8, 1, cut["head"][0], cut["head"][1], flag)
        poses = np.stack([np.concatenate((np.array(r.R_refined), np.array(r.t_refined))) for r in rs[-W:]])
        assert got.poses.tobytes() == poses.tobytes(), "the poses of the window come from the pose ring in age order"
        # the refinement: a stand-alone call on the downloaded window
        n, m = got.L, got.M
        assert n > 20
        X, res, summ = ctx.window_structure(pipe.K[None], got.poses[None], got.X_in[None], got.lm_start[None], got.obs_slot[None],
                                            got.obs_xy[None], [[n, m]], **PRM)
        assert got.X.tobytes() == X[0, :n].tobytes() and got.results.tobytes() == res[0, :n].tobytes()
        assert got.summary.tobytes() == summ[0].tobytes() == got.entry["summary"].tobytes()
        assert summ[0]["L"] == n and summ[0]["n_kept"] > 0 and np.any(got.X != got.X_in)
        assert got.entry["n_written"] == 0, "feedback = 0 writes nothing"
        pipe.close()


# ---- 3, 4: the lag rule against the existing primitives ----

def check_lag_rule(ctx, a, b, nothing):
    same_runs(a, b)
    e = np.stack(b["entries"])[:, 0]
    assert [int(x) for x in e["n_written"]] == a["written"], "every entry's n_written is what the synchronous run wrote"
    assert [int(x) for x in e["step"]] == list(range(1, len(e) + 1))
    assert [int(x) for x in e["full"]] == [0, 0] + [1] * (len(e) - 2)
    for k, s in enumerate(a["summaries"]):
        assert (s is None) == (not e[k]["full"])
        if s is not None:
            assert e[k]["summary"].tobytes() == s.tobytes(), k
    assert any(x["full"] and x["summary"]["n_kept"] > 0 for x in e) and sum(a["written"]) > 0
    assert not np.array_equal(b["landmarks"][0], nothing["landmarks"][0], equal_nan=True), "a final landmark was meant to move"


def test_lag_rule_equals_the_synchronous_construction(ctx):
    a = cached("run_a", lambda: run_a(ctx))
    check_lag_rule(ctx, a, fed(ctx), plain(ctx))


def test_recovery_path_receives_the_pending_write_back(ctx):
    a = run_a(ctx, fault_every=3)
    b = run_b(ctx, [0], fault_every=3)
    nothing = run_b(ctx, [0], fault_every=3, loop=False)
    check_lag_rule(ctx, a, b, nothing)
    rec = [k for k, rs in enumerate(b["results"]) if rs[0].recovered == 1]
    assert rec == [2, 5, 8]
    e = np.stack(b["entries"])[:, 0]
    # post k - 1 was made with step k in flight: its write-back met the fault word and was queued again behind the host path
    assert any(e[k - 1]["full"] and e[k - 1]["n_written"] > 0 for k in rec), "a write-back was meant to be pending behind a redone step"


# ---- 5: feedback = 0 ----

def test_without_feedback_the_loop_computes_what_it_computed(ctx):
    off = run_b(ctx, [0], feedback=False)
    same_runs(off, plain(ctx))
    e = np.stack(off["entries"])[:, 0]
    assert not e["n_written"].any() and e["full"].sum() == len(e) - 2
    assert all(x["summary"]["L"] == x["L"] > 20 and x["summary"]["n_kept"] > 0 and x["summary"]["cost"] <= x["summary"]["cost0"]
               for x in e if x["full"])


# ---- 6, 7: breaks and lanes ----

def test_breaks_empty_one_lanes_window_and_leave_the_other(ctx):
    restart_at = 6
    f1, T1 = initial_features(lane_stream(1), pairs_of(10)[restart_at][0], N)

    def breaks(k, pipe, sl):
        if k == 3:
            sl.reset(1)
        if k == restart_at:
            pipe.restart(1, pairs_of(10)[k][0], f1, T1, T1)      # (a hand-over without a reset: the headers give it away)

    both = run_b(ctx, [0, 1], lookahead=False, before_step=breaks)
    e = np.stack(both["entries"])
    assert [int(x) for x in e[:, 1]["full"]] == [0, 0, 1, 0, 0, 1, 0, 0, 1, 1]
    assert [int(x) for x in e[:, 1]["step"]] == [1, 2, 3, 4, 5, 6, 1, 2, 3, 4], "a restart starts the lane's step counter again"
    assert not e[:, 1]["n_written"][[3, 4, 6, 7]].any() and not e[:, 1]["L"][[3, 4, 6, 7]].any()
    assert e[8, 1]["L"] > 0 and e[8, 1]["summary"]["n_kept"] > 0
    # lane 0 against the same scene alone, stepped the same way
    one = run_b(ctx, [0], lookahead=False)
    assert e[:, 0].tobytes() == np.stack(one["entries"])[:, 0].tobytes() and e[:, 0]["n_written"].sum() > 0
    assert both["states"][0] == one["states"][0]
    assert [result_words(rs[0]) for rs in both["results"]] == [result_words(rs[0]) for rs in one["results"]]
    assert [record_bytes(rs[0]) for rs in both["records"]] == [record_bytes(rs[0]) for rs in one["records"]]


def test_two_lanes_equal_each_lane_alone(ctx):
    both = run_b(ctx, [0, 1])
    e = np.stack(both["entries"])
    for q in range(2):
        one = alone(ctx, q)
        assert e[:, q].tobytes() == np.stack(one["entries"])[:, 0].tobytes(), q
        assert both["states"][q] == one["states"][0], q
        for k in range(10):
            assert result_words(both["results"][k][q]) == result_words(one["results"][k][0]), (q, k)
            rb, ro = both["records"][k][q], one["records"][k][0]
            assert (rb.n, rb.step, rb.next_id, np.asarray(rb).tobytes()) == (ro.n, ro.step, ro.next_id, np.asarray(ro).tobytes())
        assert e[:, q]["n_written"].sum() > 0


# ---- 8: repeat ----

def test_a_second_run_gives_identical_bits(ctx):
    first, again = fed(ctx), run_b(ctx, [0])
    same_runs(first, again)
    assert np.stack(first["entries"]).tobytes() == np.stack(again["entries"]).tobytes()


# ---- 9: the driver ----

def test_run_on_device_with_stream_feedback(ctx):
    from test_gpu_window_ba import digest
    from vo import driver
    from vo.primitives import Sequence

    def seq():
        return Sequence("synthetic", n_frames=12, height=240, width=320)
    kw = dict(n_keypoints=300, context=ctx, tracks=True, ba_window=4, ba_mode="structure")
    before = [digest(driver.run_on_device(seq(), ba_feedback=f, ba_params=PRM, **kw)) for f in (True, False)]
    out = driver.run_on_device(seq(), ba_feedback="stream", ba_params=dict(PRM, download=True), **kw)
    steps = len(out["results"])
    assert len(out["ba"]) == steps - 3 and np.isfinite(out["trajectory"]).all()
    for k, e in enumerate(out["ba"]):
        assert set(e) == {"frames", "status", "cost0", "cost", "iterations", "n_kept", "n", "flags", "n_written", "poses", "ids",
                          "landmarks", "kept"}
        assert e["frames"] == list(range(k + 1, k + 5)) and e["status"] == 0 and e["cost"] <= e["cost0"] and e["n_kept"] > 0
        assert e["n"] == len(e["ids"]) == len(e["landmarks"]) == len(e["kept"]) and e["kept"].sum() == e["n_kept"]
        rs = out["results"][k:k + 4]
        assert e["poses"].tobytes() == np.stack([np.concatenate((np.array(r.R_refined), np.array(r.t_refined))) for r in rs]).tobytes()
    assert sum(e["n_written"] for e in out["ba"]) > 0
    # the kept and moved landmarks of the last window that are still triangulated are in the features, byte for byte
    last, f = out["ba"][-1], out["features"]
    newest = out["observations"][-1]
    row = {int(i): j for j, i in enumerate(newest["id"])}
    at = {int(i): j for j, i in enumerate(f.uids)}
    checked = 0
    for i, X, kept in zip(last["ids"], last["landmarks"], last["kept"]):
        j = at.get(int(i))
        rec = np.array([newest[row[int(i)]][c] for c in ("X", "Y", "Z")])
        if kept and X.tobytes() != rec.tobytes() and j is not None and f.state[j] == 2:
            assert np.asarray(f.landmarks[j]).reshape(3).tobytes() == X.tobytes()
            checked += 1
    assert checked > 0 and checked == last["n_written"]
    # without the download the same run, the entries without the arrays
    lean = driver.run_on_device(seq(), ba_feedback="stream", ba_params=PRM, **kw)
    assert digest(lean) == digest(out) and len(lean["ba"]) == len(out["ba"])
    for a, b in zip(lean["ba"], out["ba"]):
        assert set(a) == set(b) - {"poses", "ids", "landmarks", "kept"} and all(a[k] == b[k] for k in a)
    # poses and records are those of run_b's construction for the same recording: the driver's own frame loop without a back
    # end (two steps pending), and every collected step posted by hand to a loop made by hand
    class ByHand(driver._DeviceRun):
        def open_pipeline(self):
            super().open_pipeline()
            self.sl, self.posts = self.pipe.structure_loop(4, feedback=True, **PRM), []
            inner = self.pipe.collect_all

            def collect_all():
                self.last = inner()
                return self.last
            self.pipe.collect_all = collect_all

        def collect_one(self):
            super().collect_one()
            self.posts.append(self.sl.post(self.last))
    hand = ByHand([seq()], 1, None, ctx, "host", True, (300, 17, 2, None, None, 0.25), (300, 17, 2, 4000, "current", "harris")).run()[0]
    assert digest(hand) == digest(out), "trajectory, every step's refined pose and every record"
    assert np.asarray(hand["features"].landmarks).tobytes() == np.asarray(out["features"].landmarks).tobytes()
    sync = driver.run_on_device(seq(), ba_feedback=True, ba_params=PRM, **kw)
    assert [e["frames"] for e in sync["ba"]] == [e["frames"] for e in out["ba"]]
    assert out["ba"][0]["cost0"] == sync["ba"][0]["cost0"] and out["ba"][0]["cost"] == sync["ba"][0]["cost"], (
        "the first window is built before any landmark went back: the same in both modes")
    after = [digest(driver.run_on_device(seq(), ba_feedback=f, ba_params=PRM, **kw)) for f in (True, False)]
    assert before == after, "ba_feedback=True / False are what they were"
    assert digest(out) != before[1], "the write-back reaches the poses"
    for args, word in ((dict(ba_mode="full"), "ba_mode"), (dict(ba_window=None), "ba_window")):
        with pytest.raises(ValueError, match=word):
            driver.run_on_device(seq(), ba_feedback="stream", **dict(kw, **args))


def test_run_batch_on_device_with_stream_feedback(ctx):
    """Two recordings on two lanes equal each recording alone: entries, poses and records.  (Equal lengths: a lane that
    changes its recording drains the steps in flight, and a post that finds nothing in flight writes into the step's own
    features instead of the next step's -- the rule, but not what the recording alone meets at that step.)"""
    from vo import driver
    from vo.primitives import Sequence

    def seqs():
        return [Sequence("synthetic", n_frames=11, height=240, width=320, seed=2023 + 11 * i) for i in range(2)]
    kw = dict(n_keypoints=300, context=ctx, tracks=True, ba_window=4, ba_mode="structure", ba_feedback="stream", ba_params=PRM)
    out = driver.run_batch_on_device(seqs(), lanes=2, **kw)
    for i in range(2):
        one = driver.run_on_device(seqs()[i], **kw)
        assert len(out[i]["ba"]) == len(one["ba"]) == len(out[i]["results"]) - 3
        assert out[i]["ba"] == one["ba"] and sum(e["n_written"] for e in one["ba"]) > 0
        assert [result_words(r) for r in out[i]["results"]] == [result_words(r) for r in one["results"]]
        assert [record_bytes(r)[:3] + record_bytes(r)[4:] for r in out[i]["observations"]] == [
            record_bytes(r)[:3] + record_bytes(r)[4:] for r in one["observations"]]


# ---- 10: argument errors ----

def test_argument_errors_carry_a_message(ctx):
    from vo import _native, synthetic
    stream = lane_stream(0)
    plainp = make_pipe(ctx, stream, N, HYP)
    with pytest.raises(_native.VoError, match="track_ids") as e:
        plainp.structure_loop(4)
    assert e.value.code == _native.VO_EINVAL
    plainp.close()
    har = _native.Pipeline(ctx, H, W_IMG, FRAMES, stream.K, n_keypoints=N, hyp=HYP, tracker="harris", track_ids=True)
    with pytest.raises(_native.VoError, match="tracker_mode"):
        har.structure_loop(4)
    har.close()
    pipe = lanes_pipe(ctx, [0])
    for w in (1, 17):
        with pytest.raises(_native.VoError, match="window must be"):
            pipe.structure_loop(w)
    with pytest.raises(_native.VoError, match="M_cap"):
        pipe.structure_loop(4, L_cap=10, M_cap=41)
    sl = pipe.structure_loop(4)
    with pytest.raises(_native.VoError, match="already"):
        pipe.structure_loop(4)
    with pytest.raises(_native.VoError, match="no step has been collected"):
        sl.post(_native.StepResult())
    pairs = pairs_of(3)
    pipe.submit(*pairs[0])
    r = pipe.collect()
    pipe.submit(*pairs[1])
    pipe.submit(*pairs[2])
    with pytest.raises(_native.VoError, match="two steps are in flight") as e:
        sl.post(r)
    assert e.value.code == _native.VO_EINVAL
    pipe.collect()
    j = sl.post(pipe.collect())
    assert sl.poll(j, wait=True)[0]["step"] == 3
    with pytest.raises(_native.VoError, match="was not made"):
        sl.poll(j + 1)
    with pytest.raises(_native.VoError, match="sequence"):
        sl.reset(1)
    with pytest.raises(_native.VoError, match="max_iter"):
        bad = lanes_pipe(ctx, [0])
        try:
            s2 = bad.structure_loop(4, max_iter=51)
            s2.post(bad.step(*pairs[0]))
        finally:
            bad.close()
    sl.close()
    again = pipe.structure_loop(3)                       # (a closed loop leaves the pipeline free for another)
    again.close()
    pipe.close()
