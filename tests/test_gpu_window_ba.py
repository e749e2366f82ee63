"""-m gpu: the window bundle adjustment (include/vo_hip.h, "Window bundle adjustment"; csrc/window_ba.hip) against its
float64 definition (tests/window_ba_reference.py) on the case table of tests/window_ba_cases.py, the window builder against
a NumPy join of the downloaded records, the one write into a pipeline, and the driver's `ba_window`.

Bars.  Stepwise (max_iter 2 and 4): poses and landmarks within 1e-8 (1 + |value|) -- test_refine_pose_matches_oracle's bar,
for the same cause (summation order, libm), ten times what tests/test_window_ba_host.py allows a permuted summation order
to move them -- with iterations, trials and status equal and the cost within 1e-9 relative.  Converged (max_iter 50): by cost
alone (flat directions move by 1e-6 under a permuted order while the cost holds to 1e-13): within 1e-9 of the definition's,
not above SciPy's by more than 1e-9, status 0 or 3, the iteration count within one."""
import hashlib

import numpy as np
import pytest

import window_ba_cases as wc
import window_ba_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def run(ctx, windows, n_fixed=2, huber_px=0.0, max_iter=0, **kw):
    from vo.landmarks import pack_windows
    a = pack_windows(windows)
    poses, X, res = ctx.window_ba(a["K"], a["poses"], a["X"], a["lm_start"], a["obs_slot"], a["obs_xy"], a["counts"],
                                  n_fixed=n_fixed, huber_px=huber_px, max_iter=max_iter, **kw)
    return a, poses, X, res


def run_case(ctx, name, max_iter):
    c = wc.get(name)
    _, poses, X, res = run(ctx, [c.win], c.n_fixed, c.huber_px, max_iter)
    return poses[0], X[0, :len(c.win.X)], res[0]


def close(a, b):
    return np.abs(a - b) <= 1e-8 * (1.0 + np.abs(b))


@pytest.mark.parametrize("max_iter", [2, 4])
@pytest.mark.parametrize("name", wc.SOLVED)
def test_steps_match_the_definition(ctx, name, max_iter):
    d = wc.definition(name, max_iter)
    poses, X, res = run_case(ctx, name, max_iter)
    print("%s, max_iter %d: status %d / %d, iterations %d / %d, trials %d / %d, cost %.15g / %.15g, poses off by %.3e, "
          "landmarks by %.3e" % (name, max_iter, res["status"], d.status, res["iterations"], d.iterations, res["trials"],
                                 d.trials, res["cost"], d.cost, np.abs(poses - d.poses).max(), np.abs(X - d.X).max()))
    assert (res["status"], res["iterations"], res["trials"]) == (d.status, d.iterations, d.trials)
    assert res["n_obs"] == len(wc.get(name).win.obs_slot)
    assert abs(res["cost0"] - d.cost0) <= 1e-9 * d.cost0 and abs(res["cost"] - d.cost) <= 1e-9 * d.cost
    assert abs(res["lam"] - d.lam) <= 1e-12 * d.lam
    assert close(poses, d.poses).all() and close(X, d.X).all()
    c = wc.get(name)
    assert np.array_equal(poses[:c.n_fixed], c.win.poses[:c.n_fixed]), "the held slots are bit for bit what they were"


@pytest.mark.parametrize("name", wc.SOLVED)
def test_converged_cost_matches_the_definition_and_scipy(ctx, name):
    d = wc.definition(name, 50)
    sp = wc.scipy_cost(name)
    _, _, res = run_case(ctx, name, 50)
    print("%s: status %d / %d, iterations %d / %d, cost %.15g, definition %.15g, SciPy %.15g" % (
        name, res["status"], d.status, res["iterations"], d.iterations, res["cost"], d.cost, sp))
    assert abs(res["cost"] - d.cost) <= 1e-9 * d.cost
    assert res["cost"] <= sp * (1.0 + 1e-9)
    assert res["status"] in (0, 3)
    assert abs(int(res["iterations"]) - d.iterations) <= 1


@pytest.mark.parametrize("name", wc.NOISY)
def test_noisy_windows_move_towards_the_generating_poses(ctx, name):
    c = wc.get(name)
    before = wc.pose_rms(c, c.win.poses)
    assert wc.pose_rms(c, wc.definition(name, 4).poses) < before
    poses, _, _ = run_case(ctx, name, 4)
    assert wc.pose_rms(c, poses) < before


def batch_windows():
    return [wc.empty_window(8) if n is None else wc.get(n).win for n in wc.BATCH]


def test_batch_equals_single_calls_bit_for_bit(ctx):
    wins = batch_windows()
    a, poses, X, res = run(ctx, wins, max_iter=4)
    assert [int(s) for s in res["status"]] == [1, 4, 1]
    for q, w in enumerate(wins):
        if len(w.X) == 0:
            assert np.array_equal(poses[q], w.poses) and res[q]["iterations"] == 0 and res[q]["n_obs"] == 0
            continue
        _, p1, X1, r1 = run(ctx, [w], max_iter=4)
        L = len(w.X)
        assert p1[0].tobytes() == poses[q].tobytes() and X1[0, :L].tobytes() == X[q, :L].tobytes()
        assert r1[0].tobytes() == res[q].tobytes()
        assert np.array_equal(X[q, L:], a["X"][q, L:]), "rows beyond L are not touched"


def test_a_second_run_gives_identical_bits(ctx):
    for name, max_iter in (("w8_l600", 4), ("w8_l60_outliers_huber", 50)):
        c = wc.get(name)
        first = run(ctx, [c.win], c.n_fixed, c.huber_px, max_iter)[1:]
        again = run(ctx, [c.win], c.n_fixed, c.huber_px, max_iter)[1:]
        for u, v in zip(first, again):
            assert u.tobytes() == v.tobytes()


def test_refusals_leave_every_input_bit(ctx):
    import copy
    wins = [(wc.get(n).win, 2) for n in wc.REFUSED] + [(wc.empty_window(4), 2), (wc.get("w3_l8_full").win, 3)]
    bad = copy.deepcopy(wc.get("w4_l12_missing").win)
    bad.obs_slot[3] = 9                                        # a slot outside the window
    wins.append((bad, 2))
    bad = copy.deepcopy(wc.get("w4_l12_missing").win)
    bad.lm_start[4] = bad.lm_start[5]                          # a landmark without observations
    wins.append((bad, 2))
    bad = copy.deepcopy(wc.get("w4_l12_missing").win)
    bad.poses[3, 10] = np.inf
    wins.append((bad, 2))
    for w, n_fixed in wins:
        a, poses, X, res = run(ctx, [w], n_fixed=n_fixed, max_iter=4)
        assert res[0]["status"] == 4 and res[0]["iterations"] == 0 and res[0]["trials"] == 0
        assert poses.tobytes() == a["poses"].tobytes() and X.tobytes() == a["X"].tobytes()
        assert ref.solve(w, n_fixed, 0.0, 4).status == ref.STATUS_REFUSED


def test_argument_errors_carry_a_message(ctx):
    from vo import _native
    from vo.landmarks import pack_windows
    a = pack_windows([wc.get("w4_l12_missing").win])
    args = (a["K"], a["poses"], a["X"], a["lm_start"], a["obs_slot"], a["obs_xy"], a["counts"])
    for kw, word in ((dict(max_iter=51), "max_iter"), (dict(max_trials=-1), "max_trials"), (dict(n_fixed=-1), "n_fixed"),
                     (dict(huber_px=-1.0), "huber_px"), (dict(lambda0=float("nan")), "lambda0"), (dict(step_tol=-1.0), "step_tol")):
        with pytest.raises(_native.VoError, match=word) as e:
            ctx.window_ba(*args, **kw)
        assert e.value.code == _native.VO_EINVAL
    with pytest.raises(_native.VoError, match="W must be") as e:
        ctx.window_ba(a["K"], np.zeros((1, 17, 12)), *args[2:])
    assert e.value.code == _native.VO_EINVAL
    with pytest.raises(_native.VoError, match="M_cap"):
        ctx.window_ba(a["K"], a["poses"], a["X"][:, :2], a["lm_start"][:, :3], *args[4:])      # M_cap > L_cap * W
    d = ctx.alloc(4096)
    with pytest.raises(_native.VoError, match="null pointer"):
        ctx.window_ba_dev(1, 4, 12, 40, d, d, d, d, d, d, d, None)
    with pytest.raises(_native.VoError, match="S must be"):
        ctx.window_ba_dev(0, 4, 12, 40, d, d, d, d, d, d, d, d)
    with pytest.raises(_native.VoError, match="cap must be"):
        ctx.window_from_tracks([d, d], 0, 12, 24, d, d, d, d, d, d)
    with pytest.raises(_native.VoError, match="16-byte aligned"):
        ctx.window_from_tracks([d, d + 8], 10, 12, 24, d, d, d, d, d, d)
    with pytest.raises(_native.VoError, match="W must be"):
        ctx.window_from_tracks([d], 10, 12, 12, d, d, d, d, d, d)
    ctx.free(d)
    assert ctx.window_ba_workspace_bytes(2, 8, 100, 800) > 0 and ctx.window_ba_workspace_bytes(1, 17, 100, 800) == 0


# ---- the builder ----

def numpy_window(records, cap, L_cap, M_cap):
    """vo_window_from_tracks_dev in NumPy from downloaded records (TrackRecord arrays, oldest first)."""
    recs = [r[:cap] for r in records]
    W = len(recs)
    first_row = [{} for _ in recs]
    for s, r in enumerate(recs):
        for k, i in enumerate(r["id"]):
            first_row[s].setdefault(int(i), k)
    head = [0, 0, 0, 0]
    lm_start, slot, xy, X, lm_id = [0], [], [], [], []
    for row in recs[-1]:
        if row["state"] != 2 or not np.all(np.isfinite([row["X"], row["Y"], row["Z"]])):
            continue
        seen = [s for s in range(W) if int(row["id"]) in first_row[s]]
        if len(seen) < 2:
            continue
        if len(lm_id) >= L_cap:
            head[2] |= 1
            break
        if len(slot) + len(seen) > M_cap:
            head[2] |= 2
            break
        for s in seen:
            o = recs[s][first_row[s][int(row["id"])]]
            slot.append(s)
            xy.append((np.float64(o["x"]), np.float64(o["y"])))
        lm_start.append(len(slot))
        X.append((row["X"], row["Y"], row["Z"]))
        lm_id.append(row["id"])
    head[0], head[1] = len(lm_id), len(slot)
    return dict(head=np.array(head, np.int32), lm_start=np.array(lm_start, np.int32), obs_slot=np.array(slot, np.int32),
                obs_xy=np.array(xy, np.float64).reshape(-1, 2), X=np.array(X, np.float64).reshape(-1, 3),
                lm_id=np.array(lm_id, np.int32))


def device_window(ctx, d_records, cap, L_cap, M_cap):
    sizes = dict(head=16, lm_start=4 * (L_cap + 1), obs_slot=4 * M_cap, obs_xy=16 * M_cap, X=24 * L_cap, lm_id=4 * L_cap)
    d = {k: ctx.to_device(np.full(v, 0xEE, np.uint8)) for k, v in sizes.items()}
    ctx.window_from_tracks(d_records, cap, L_cap, M_cap, d["head"], d["lm_start"], d["obs_slot"], d["obs_xy"], d["X"], d["lm_id"])
    head = ctx.download(d["head"], (4,), np.int32)
    L, M = int(head[0]), int(head[1])
    assert 0 <= L <= L_cap and 0 <= M <= M_cap
    out = dict(head=head, lm_start=ctx.download(d["lm_start"], (L_cap + 1,), np.int32)[:L + 1],
               obs_slot=ctx.download(d["obs_slot"], (M_cap,), np.int32)[:M],
               obs_xy=ctx.download(d["obs_xy"], (M_cap, 2), np.float64)[:M], X=ctx.download(d["X"], (L_cap, 3), np.float64)[:L],
               lm_id=ctx.download(d["lm_id"], (L_cap,), np.int32)[:L])
    for p in d.values():
        ctx.free(p)
    return out


def same_window(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


_loop = {}


def posted_loop(ctx):
    """test_gpu_track_ids.py's case-1 shape (240 x 320, 300 keypoints, 5 frames of synthetic.Stream walked for 8 steps from
    70 % of the detector's keypoints, so the first step re-detects) with every step's record posted; the records stay on
    the device for the module."""
    if not _loop:
        from vo import synthetic
        from test_gpu_pipeline import make_pipe, start_state
        stream = synthetic.Stream(5, 240, 320)
        feats, T = start_state(stream, 300, 0.7)
        order = stream.order(8)
        pipe = make_pipe(ctx, stream, 300, 256, track_ids=True)
        pipe.set_state(0, feats, T, T)
        nbytes = pipe.tracks_record_bytes(pipe.cap)
        d = ctx.to_device(np.zeros(8 * nbytes, np.uint8))
        results = []
        for k, (a, b) in enumerate(zip(order[:-1], order[1:])):
            r = pipe.step(a, b)
            assert r.fault == 0
            pipe.export_tracks_post(r, pipe.cap, d + k * nbytes)
            results.append(r)
        pipe.export_state_join()
        ctx.sync()
        records = [pipe.read_tracks_record(d + k * nbytes, pipe.cap) for k in range(8)]
        _loop.update(pipe=pipe, d=[d + k * nbytes for k in range(8)], records=records, results=results, cap=pipe.cap,
                     K=stream.K, order=order)
    return _loop


@pytest.mark.parametrize("W", [3, 5])
def test_builder_equals_a_numpy_join_of_the_records(ctx, W):
    lp = posted_loop(ctx)
    cap = lp["cap"]
    want = numpy_window(lp["records"][-W:], cap, cap, cap * W)
    assert want["head"][0] > 20 and want["head"][2] == 0, "the loop was meant to leave landmarks seen more than once"
    same_window(device_window(ctx, lp["d"][-W:], cap, cap, cap * W), want)
    # the capacities: the list ends at the last landmark that fits wholly, and the flag says which capacity ended it
    L, M = int(want["head"][0]), int(want["head"][1])
    for L_cap, M_cap, flag in ((L - 3, (L - 3) * W, 1), (L, M - 1, 2), (L, int(want["lm_start"][L // 2]) + 1, 2)):
        cut = numpy_window(lp["records"][-W:], cap, L_cap, M_cap)
        assert cut["head"][2] == flag and cut["head"][0] < L
        same_window(device_window(ctx, lp["d"][-W:], cap, L_cap, M_cap), cut)
    # rows beyond `cap` of a record are ignored: n > cap
    small = min(len(r) for r in lp["records"][-W:]) - 40
    assert all(r.n > small for r in lp["records"][-W:])
    same_window(device_window(ctx, lp["d"][-W:], small, cap, cap * W), numpy_window(lp["records"][-W:], small, cap, cap * W))


def test_builder_on_hand_made_records(ctx):
    from vo._pipeline import TRACK_HEADER, TRACK_ROW, TrackRecord
    nan = np.nan

    def record(step, rows, n=None):
        raw = np.zeros(16 + 48 * len(rows), np.uint8)
        raw[:16].view(TRACK_HEADER)[0] = (len(rows) if n is None else n, step, 100, 0)
        body = raw[16:].view(TRACK_ROW)
        for k, row in enumerate(rows):
            body[k] = row
        return raw

    # id, born, x, y, state, candidate, X, Y, Z
    old = record(1, [(7, 0, 1.5, 2.5, 1, 0, nan, nan, nan), (3, 0, 3.5, 4.5, 2, 0, 1.0, 1.0, 9.0), (9, 0, 5.0, 6.0, 0, 0, nan, nan, nan)])
    mid = record(2, [(3, 0, 3.25, 4.25, 2, 0, 1.0, 1.0, 9.0), (5, 1, 8.0, 9.0, 1, 0, nan, nan, nan), (7, 0, 1.25, 2.25, 1, 0, nan, nan, nan)])
    new = record(3, [(5, 1, 8.5, 9.5, 2, 0, 2.0, 2.0, 8.0),       # seen in mid only
                     (11, 2, 0.5, 0.5, 2, 0, 3.0, 3.0, 7.0),      # seen nowhere else: no landmark
                     (7, 0, 1.0, 2.0, 2, 1, 4.0, 4.0, 6.0),       # seen in all three (states 1, 1, 2)
                     (3, 0, 3.0, 4.0, 1, 0, nan, nan, nan),       # not triangulated now
                     (9, 0, 5.5, 6.5, 2, 0, 5.0, nan, 5.0)],      # a landmark that is not finite
                 n=9)                                             # n > cap: the rows beyond do not exist
    raws = [old, mid, new]
    d = [ctx.to_device(r) for r in raws]
    recs = [TrackRecord.from_bytes(r, 5) for r in raws]
    want = numpy_window(recs, 5, 4, 12)
    assert want["lm_id"].tolist() == [5, 7] and want["obs_slot"].tolist() == [1, 2, 0, 1, 2]
    assert want["obs_xy"].tolist() == [[8.0, 9.0], [8.5, 9.5], [1.5, 2.5], [1.25, 2.25], [1.0, 2.0]]
    same_window(device_window(ctx, d, 5, 4, 12), want)
    for L_cap, M_cap, flag, ids in ((1, 3, 1, [5]), (2, 4, 2, [5]), (2, 2, 2, [5])):
        cut = numpy_window(recs, 5, L_cap, M_cap)
        assert cut["head"][2] == flag and cut["lm_id"].tolist() == ids
        same_window(device_window(ctx, d, 5, L_cap, M_cap), cut)
    # cap = 2: only the first two rows of every record exist
    same_window(device_window(ctx, d, 2, 4, 12), numpy_window([TrackRecord.from_bytes(r, 2) for r in raws], 2, 4, 12))
    for p in d:
        ctx.free(p)


def long_run_records():
    """Three records (raw bytes, oldest first) whose newest has 1100 rows: more than the builder's 512 threads, so every
    thread owns a run of 3 rows (the last run is short).  The middle row of every run, row 3 k + 1, is a landmark; k decides
    where else its id is seen: k % 7 == 3 nowhere (no landmark), else k % 5 == 0 in both older records, else in the older one
    of the parity of k.  The older records are shuffled among rows of other ids, and id 1046 (k = 15, seen in both) occurs
    twice in the oldest: the first row's pixel is the observation."""
    from vo._pipeline import TRACK_HEADER, TRACK_ROW
    rng = np.random.default_rng(5)

    def record(step, rows):
        raw = np.zeros(16 + 48 * len(rows), np.uint8)
        raw[:16].view(TRACK_HEADER)[0] = (len(rows), step, 5000, 0)
        raw[16:].view(TRACK_ROW)[:] = rows
        return raw

    n = 1100
    new = np.zeros(n, TRACK_ROW)
    new["id"], new["x"], new["y"], new["state"] = 1000 + np.arange(n), np.arange(n) + 0.5, np.arange(n) * 0.25, 1
    lm = np.arange(n) % 3 == 1
    new["state"][lm] = 2
    for c, f in (("X", 1.0), ("Y", -0.5), ("Z", 0.125)):
        new[c] = np.where(lm, 4.0 + f * np.arange(n), np.nan)
    k = np.arange(n) // 3
    seen = lm & (k % 7 != 3)
    older = []
    for s in range(2):
        here = new[seen & ((k % 5 == 0) | (k % 2 == s))].copy()
        here["x"] += 0.25 * (2 - s)
        here["state"], here["X"], here["Y"], here["Z"] = 1, np.nan, np.nan, np.nan
        other = np.zeros(200 + 100 * s, TRACK_ROW)                     # ids the newest record does not carry
        other["id"], other["x"] = 9000 + np.arange(len(other)), 7.0
        rows = np.concatenate((here, other))[rng.permutation(len(here) + len(other))]
        if s == 0:
            twice = rows[rows["id"] == 1046].copy()
            twice["x"], twice["y"] = 77.0, 88.0
            rows = np.concatenate((rows, twice))                       # behind the first row that carries the id
        older.append(record(1 + s, rows))
    return older + [record(3, new)]


def test_builder_with_runs_longer_than_a_row(ctx):
    from vo._pipeline import TrackRecord
    raws = long_run_records()
    cap, W = 1100, 3
    recs = [TrackRecord.from_bytes(r, cap) for r in raws]
    assert len(recs[2]) == cap and (recs[0]["id"] == 1046).sum() == 2
    want = numpy_window(recs, cap, cap, cap * W)
    L, M = int(want["head"][0]), int(want["head"][1])
    assert L == 315 and 2 * L < M < 3 * L and want["head"][2] == 0          # 367 middle rows, 52 of them seen nowhere else
    at = want["lm_id"].tolist().index(1046)
    assert want["obs_slot"][want["lm_start"][at]:want["lm_start"][at + 1]].tolist() == [0, 1, 2]
    assert want["obs_xy"][want["lm_start"][at]].tolist() == [47.0, 11.5]        # the first row's pixel, not (77, 88)
    d = [ctx.to_device(r) for r in raws]
    same_window(device_window(ctx, d, cap, cap, cap * W), want)
    # both cuts fall on the middle row of a run far from either end of the list
    for L_cap, M_cap, flag in ((L // 2, (L // 2) * W, 1), (L, int(want["lm_start"][L // 3]) + 1, 2)):
        cut = numpy_window(recs, cap, L_cap, M_cap)
        assert cut["head"][2] == flag and 0 < cut["head"][0] < L
        same_window(device_window(ctx, d, cap, L_cap, M_cap), cut)
    for p in d:
        ctx.free(p)


def test_adjuster_solves_the_loops_window(ctx):
    """WindowBundleAdjuster on the posted loop: the window it solves is the builder's, the result the solver's on it; a
    break in the step counter drops what lies before it."""
    from vo.landmarks import WindowBundleAdjuster
    lp = posted_loop(ctx)
    W = 4
    ba = WindowBundleAdjuster(lp["K"], window=W, max_iter=4, cap=lp["cap"], context=ctx)
    assert ba.solve() is None
    poses_in = [np.concatenate((np.array(r.R_refined), np.array(r.t_refined))) for r in lp["results"]]
    for k in range(8 - W, 8):
        ba.push(lp["d"][k], poses_in[k])
    poses, ids, X, res = ba.solve()
    want = numpy_window(lp["records"][-W:], lp["cap"], lp["cap"], lp["cap"] * W)
    assert np.array_equal(ids, want["lm_id"]) and res["n_obs"] == want["head"][1]
    win = ref.window(lp["K"], np.stack(poses_in[-W:]), want["X"], want["lm_start"], want["obs_slot"], want["obs_xy"])
    d = ref.solve(win, 2, 0.0, 4)
    print("the loop's window: %d landmarks, %d observations, status %d / %d (%s), cost %.6g -> %.6g" % (
        len(ids), res["n_obs"], res["status"], d.status, ref.refusal(win, 2), res["cost0"], res["cost"]))
    assert (res["status"], res["iterations"], res["trials"]) == (d.status, d.iterations, d.trials)
    assert abs(res["cost0"] - d.cost0) <= 1e-9 * d.cost0 and abs(res["cost"] - d.cost) <= 1e-9 * d.cost and res["cost"] <= res["cost0"]
    assert close(poses, d.poses).all() and close(X, d.X).all()
    assert np.array_equal(poses[:2], np.stack(poses_in[-W:])[:2])
    ba.push(lp["d"][2], poses_in[2])                         # step 3 behind step 8: a break
    assert ba.solve() is None and len(ba.records) == 1
    ba.close()


# ---- the one write into a pipeline ----

def test_update_landmarks_changes_exactly_the_listed_ids_in_state_2(ctx):
    from vo import _native
    lp = posted_loop(ctx)
    pipe = lp["pipe"]
    ids, _, nxt = pipe.get_track_ids()
    before = pipe.get_state()
    tri = np.flatnonzero(before["state"] == 2)
    rest = np.flatnonzero(before["state"] != 2)
    assert len(tri) >= 8 and len(rest) >= 4
    listed = np.concatenate((ids[tri[::2]], ids[rest[:4]], [nxt + 5, nxt + 6])).astype(np.int32)      # state 2, others, absent
    rng = np.random.default_rng(3)
    order = rng.permutation(len(listed))
    listed = listed[order]
    newX = rng.normal(0.0, 5.0, (len(listed), 3))
    pipe.update_landmarks(listed, newX)
    after = pipe.get_state()
    assert np.array_equal(pipe.get_track_ids()[0], ids)
    expect = before["landmarks"].copy()
    for k, i in enumerate(listed):
        f = np.flatnonzero(ids == i)
        if len(f) and before["state"][f[0]] == 2:
            expect[f[0], :, 0] = newX[k]
    assert not np.array_equal(expect, before["landmarks"], equal_nan=True)
    for key in before:
        want = expect if key == "landmarks" else before[key]
        assert np.asarray(after[key]).tobytes() == np.asarray(want).tobytes(), key
    pipe.update_landmarks(np.zeros(0, np.int32), np.zeros((0, 3)))           # an empty list changes nothing
    assert np.asarray(pipe.get_state()["landmarks"]).tobytes() == expect.tobytes()
    # refused with a step in flight, with a bad sequence, and on a pipeline without track ids
    pipe.submit(lp["order"][-1], lp["order"][-2])
    with pytest.raises(_native.VoError, match="not collected"):
        pipe.update_landmarks(listed, newX)
    pipe.collect()
    with pytest.raises(_native.VoError, match="sequence"):
        pipe.update_landmarks(listed, newX, seq=1)
    from vo import synthetic
    from test_gpu_pipeline import make_pipe
    plain = make_pipe(ctx, synthetic.Stream(5, 240, 320), 300, 256)
    with pytest.raises(_native.VoError, match="track_ids"):
        plain.update_landmarks(listed, newX)
    plain.close()


# ---- the driver ----

def digest(out):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(out["trajectory"]).tobytes())
    for r in out["results"]:
        h.update(np.array(list(r.R_refined) + list(r.t_refined) + list(r.T_wc)).tobytes())
    for rec in out.get("observations", []):
        h.update(np.asarray(rec).tobytes())
        h.update(np.array([rec.n, rec.step, rec.next_id, rec.seq]).tobytes())
    return h.hexdigest()


def test_run_on_device_with_a_window(ctx):
    from vo import driver
    from vo.primitives import Sequence

    def seq():
        return Sequence("synthetic", n_frames=12, height=240, width=320)
    kw = dict(n_keypoints=300, context=ctx, tracks=True)
    plain = driver.run_on_device(seq(), **kw)
    none = driver.run_on_device(seq(), ba_window=None, **kw)
    assert "ba" not in plain and "ba" not in none and digest(plain) == digest(none)
    out = driver.run_on_device(seq(), ba_window=4, ba_params=dict(max_iter=4), **kw)
    assert digest(out) == digest(plain), "without feedback the loop computes what it computed"
    steps = len(out["results"])
    assert len(out["ba"]) == steps - 3
    print("windows: status %s, landmarks %s, cost %s" % ([e["status"] for e in out["ba"]], [len(e["ids"]) for e in out["ba"]],
                                                         ["%.4g -> %.4g" % (e["cost0"], e["cost"]) for e in out["ba"]]))
    assert sum(e["status"] != 4 and e["cost"] < e["cost0"] for e in out["ba"]) >= len(out["ba"]) // 2, "windows are solved"
    for k, e in enumerate(out["ba"]):
        assert e["frames"] == list(range(k + 1, k + 5)) and e["poses"].shape == (4, 12)
        assert e["status"] in (0, 1, 2, 3) and e["cost"] <= e["cost0"]
        newest = out["observations"][k + 3]
        assert len(e["ids"]) == len(e["landmarks"]) > 0 and np.isin(e["ids"], newest["id"]).all()
        assert np.isfinite(e["landmarks"]).all()
    fed = driver.run_on_device(seq(), ba_window=4, ba_feedback=True, ba_params=dict(max_iter=4), **kw)
    assert len(fed["ba"]) == steps - 3 and all(e["cost"] <= e["cost0"] for e in fed["ba"])
    assert np.isfinite(fed["trajectory"]).all()
    with pytest.raises(ValueError, match="tracks=True"):
        driver.run_on_device(seq(), n_keypoints=300, context=ctx, ba_window=4)


def test_run_batch_on_device_with_a_window(ctx):
    from vo import driver
    from vo.primitives import Sequence

    def seqs():
        return [Sequence("synthetic", n_frames=12 - 2 * i, height=240, width=320, seed=2023 + 11 * i) for i in range(2)]
    kw = dict(n_keypoints=300, context=ctx, tracks=True, ba_window=4, ba_params=dict(max_iter=4))
    out = driver.run_batch_on_device(seqs(), lanes=2, **kw)
    for i in range(2):
        alone = driver.run_on_device(seqs()[i], **kw)
        assert len(out[i]["ba"]) == len(alone["ba"]) == len(out[i]["results"]) - 3
        for a, b in zip(alone["ba"], out[i]["ba"]):
            assert a["frames"] == b["frames"] and np.array_equal(a["ids"], b["ids"])
            assert a["poses"].tobytes() == b["poses"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
            assert (a["status"], a["cost0"], a["cost"]) == (b["status"], b["cost0"], b["cost"])
