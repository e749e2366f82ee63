"""-m gpu: the window structure refinement (include/vo_hip.h, "Window structure refinement"; csrc/window_structure.hip)
against its float64 definition (tests/window_structure_reference.py) on the case table of tests/window_structure_cases.py,
WindowStructureRefiner on the posted loop of tests/test_gpu_window_ba.py, and the driver's ba_mode="structure".

Bars (the window bundle adjustment's against its definition): per landmark, after max_iter 2 and 4 and converged at 50,
status, iterations, trials, n_obs and kept equal -- tests/test_window_structure_host.py shows that the definition takes no
decision closer than 1e-9 relative and that a permuted summation order moves X by 2e-14 (1 + |X|) -- X within 1e-8 (1 + |v|),
cost0 and cost within 1e-9 relative, min_cos within 1e-12, the summary's counts equal and its sums within 1e-9 relative.
The noise-free copies (sc.NOISE_FREE), and they alone, get an absolute rounding allowance beside the relative cost bar
(RESIDUAL_EPS, below): their costs are rounding noise.
Largest differences measured on the MI355X, every count equal.  Noisy cases, plain relative differences:
X 2.4e-14 (1 + |X|), cost0 2.6e-14, cost 6.2e-11, min_cos 1.1e-16, the summary's sums 3.6e-14.  Noise-free copies: X 1.8e-14
(1 + |X|), min_cos 1.1e-16; cost0, cost and the summary's sums at 1.8e-5, 0.077 and 0.0067 of their allowance."""
import numpy as np
import pytest

import window_structure_cases as sc
import window_structure_reference as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def run(ctx, windows, **params):
    from vo.landmarks import pack_windows
    a = pack_windows(windows)
    X, res, summ = ctx.window_structure(a["K"], a["poses"], a["X"], a["lm_start"], a["obs_slot"], a["obs_xy"], a["counts"], **params)
    return a, X, res, summ


def run_case(ctx, name, max_iter, gate_px=0.0):
    win = sc.without_bad().win if name == "without_bad" else sc.get(name).win
    prm = sc.params("bad_landmarks" if name == "without_bad" else name, max_iter, gate_px)
    _, X, res, summ = run(ctx, [win], **prm)
    L = len(win.X)
    return X[0, :L], res[0, :L], summ[0]


# The noise-free copies alone: how far two correct evaluations of one cost may lie apart.  A residual e = x - proj(...) at
# image coordinates up to 640 px carries the rounding of about eight fp64 operations on numbers of that size, 8 * 1.1e-16 * 640
# = 6e-13 px: RESIDUAL_EPS = 1e-12.  A cost of n residuals then moves by up to 2 sum |e| eps + n eps^2 <= 2 sqrt(n cost) eps
# + n eps^2 whatever the order of its sums.  Those copies reach costs of 1e-8 .. 1e-22 px^2 per landmark, where the definition
# itself moves by 1e-8 of its cost under a permuted observation order (and at the stop the cost IS that rounding): 1e-9 of the
# cost cannot be asked there, so for them, and for them only, this absolute allowance stands beside the relative bar.
RESIDUAL_EPS = 1e-12


def rel(a, b):
    """|a - b| / |b| elementwise; 0 where both are 0, inf where only b is."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))


def over_allowance(a, b, n):
    """|a - b| over the noise-free copies' bar, 1e-9 |b| plus the rounding allowance of n residuals (<= 1: within it)."""
    a, b, n = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(n, np.float64)
    return np.abs(a - b) / (1e-9 * np.abs(b) + 2.0 * np.sqrt(n * np.abs(b)) * RESIDUAL_EPS + n * RESIDUAL_EPS ** 2)


def check_against_definition(name, d, X, res, summ, noise_free=False):
    for key in ("status", "iterations", "trials", "n_obs", "kept"):
        assert np.array_equal(res[key], getattr(d, key)), (name, key, np.flatnonzero(res[key] != getattr(d, key))[:8])
    dx = float((np.abs(X - d.X) / (1.0 + np.abs(d.X))).max()) if len(X) else 0.0
    dm = float(np.abs(res["min_cos"] - d.min_cos).max()) if len(X) else 0.0
    s = d.summary
    m = float(d.n_obs[d.status != sref.STATUS_REFUSED].sum())
    if noise_free:
        dc0, dc = (float(over_allowance(res[k], getattr(d, k), d.n_obs).max()) for k in ("cost0", "cost"))
        ds = max(float(over_allowance(summ[k], getattr(s, k), m)) for k in ("cost0", "cost"))
        print("%s (noise-free): X off by %.3e (1 + |X|), min_cos by %.3e; cost0 at %.3e, cost at %.3e, summary sums at %.3e "
              "of the allowance" % (name, dx, dm, dc0, dc, ds))
        assert dc0 <= 1.0 and dc <= 1.0 and ds <= 1.0
    else:
        dc0, dc = (float(rel(res[k], getattr(d, k)).max()) if len(X) else 0.0 for k in ("cost0", "cost"))
        ds = max(float(rel(summ[k], getattr(s, k))) for k in ("cost0", "cost"))
        print("%s: X off by %.3e (1 + |X|), cost0 by %.3e, cost by %.3e relative, min_cos by %.3e, summary sums by %.3e"
              % (name, dx, dc0, dc, dm, ds))
        assert dc0 <= 1e-9 and dc <= 1e-9 and ds <= 1e-9
    assert dx <= 1e-8 and dm <= 1e-12
    assert (summ["L"], summ["n_refused"], summ["n_kept"], summ["max_iterations"]) == (s.L, s.n_refused, s.n_kept, s.max_iterations)
    assert np.all(res["reserved"] == 0)


@pytest.mark.parametrize("max_iter", [2, 4, 50])
@pytest.mark.parametrize("name", sc.SOLVED)
def test_landmarks_match_the_definition(ctx, name, max_iter):
    d = sc.definition(name, max_iter)
    X, res, summ = run_case(ctx, name, max_iter)
    check_against_definition("%s, max_iter %d" % (name, max_iter), d, X, res, summ, noise_free=name in sc.NOISE_FREE)


@pytest.mark.parametrize("name", sc.GATED)
def test_gate_matches_the_definition(ctx, name):
    d = sc.definition(name, 50, sc.GATE_PX)
    X, res, summ = run_case(ctx, name, 50, sc.GATE_PX)
    check_against_definition("%s, gated" % name, d, X, res, summ)
    assert 0 < res["kept"].sum() < len(res)


def batch_windows():
    return [sc.empty_window(8) if n is None else sc.get(n).win for n in sc.BATCH]


def test_batch_equals_single_calls_bit_for_bit(ctx):
    wins = batch_windows()
    a, X, res, summ = run(ctx, wins, max_iter=4, gate_px=sc.GATE_PX)
    assert [int(s["L"]) for s in summ] == [len(w.X) for w in wins]
    for q, w in enumerate(wins):
        L = len(w.X)
        if L == 0:
            assert tuple(summ[q]) == (0, 0, 0, 0, 0.0, 0.0) and X[q].tobytes() == a["X"][q].tobytes()
            assert res[q].tobytes() == bytes(res[q].nbytes), "no row of an empty window is written"
            continue
        _, X1, r1, s1 = run(ctx, [w], max_iter=4, gate_px=sc.GATE_PX)
        assert X1[0, :L].tobytes() == X[q, :L].tobytes() and r1[0, :L].tobytes() == res[q, :L].tobytes()
        assert s1[0].tobytes() == summ[q].tobytes()
        assert np.array_equal(X[q, L:], a["X"][q, L:]), "rows beyond L are not touched"
        assert res[q, L:].tobytes() == bytes(res[q, L:].nbytes)


def test_a_second_run_gives_identical_bits(ctx):
    for name, max_iter in (("w8_l600", 4), ("w16_l64_missing_huber", 50)):
        first = run_case(ctx, name, max_iter)
        again = run_case(ctx, name, max_iter)
        for u, v in zip(first, again):
            assert u.tobytes() == v.tobytes()


def test_refusals_leave_every_input_bit(ctx):
    # refused landmarks among good neighbours: their bits stay, the neighbours are what they are without them
    c = sc.get("bad_landmarks")
    X, res, summ = run_case(ctx, "bad_landmarks", 50)
    assert np.flatnonzero(res["status"] == 4).tolist() == list(c.bad) and summ["n_refused"] == 3
    for i in c.bad:
        assert X[i].tobytes() == c.win.X[i].tobytes()
        assert (res[i]["iterations"], res[i]["trials"], res[i]["kept"], res[i]["cost0"], res[i]["cost"]) == (0, 0, 0, 0.0, 0.0)
    good = np.setdiff1d(np.arange(len(c.win.X)), c.bad)
    Xa, ra, sa = run_case(ctx, "without_bad", 50)
    assert Xa.tobytes() == X[good].tobytes() and ra.tobytes() == res[good].tobytes()
    assert sa["n_kept"] == summ["n_kept"]               # (the sums pair the rows differently: not compared bit for bit)
    # refused windows
    for name in sc.WINDOW_REFUSED:
        w = sc.get(name).win
        a, X, res, summ = run(ctx, [w], max_iter=4)
        assert X.tobytes() == a["X"].tobytes() and np.all(res[0]["status"] == 4) and np.all(res[0]["n_obs"] == 0)
        assert tuple(summ[0]) == (len(w.X), len(w.X), 0, 0, 0.0, 0.0)
        assert np.all(sref.solve(w, max_iter=4).status == 4)
    from vo.landmarks import pack_windows
    a = pack_windows([sc.get("w4_l12_missing").win])
    for L, M in ((13, 40), (12, 10000), (12, -1)):                         # L beyond L_cap, M beyond M_cap, M < 0
        X, res, summ = ctx.window_structure(a["K"], a["poses"], a["X"], a["lm_start"], a["obs_slot"], a["obs_xy"], [[L, M]], max_iter=4)
        assert X.tobytes() == a["X"].tobytes() and np.all(res[0]["status"] == 4) and summ[0]["n_refused"] == 12 and summ[0]["L"] == L
    # landmarks that are not kept: the 2 px gate, the parallax gate
    for name in sc.GATED:
        c = sc.get(name)
        X, res, _ = run_case(ctx, name, 50, sc.GATE_PX)
        out = res["kept"] == 0
        assert out.any() and X[out].tobytes() == c.win.X[out].tobytes()
        assert not np.any(np.all(X[~out] == c.win.X[~out], axis=1))
    c = sc.get("zero_parallax")
    X, res, _ = run_case(ctx, "zero_parallax", 50)
    assert res[c.thin]["kept"] == 0 and res[c.thin]["status"] in (0, 1) and X[c.thin].tobytes() == c.win.X[c.thin].tobytes()
    assert res["kept"].sum() == len(res) - 1


def test_argument_errors_carry_a_message(ctx):
    from vo import _native
    from vo.landmarks import pack_windows
    a = pack_windows([sc.get("w4_l12_missing").win])
    args = (a["K"], a["poses"], a["X"], a["lm_start"], a["obs_slot"], a["obs_xy"], a["counts"])
    for kw, word in ((dict(max_iter=51), "max_iter"), (dict(max_trials=-1), "max_trials"), (dict(huber_px=-1.0), "huber_px"),
                     (dict(lambda0=float("nan")), "lambda0"), (dict(step_tol=-1.0), "step_tol"), (dict(f_tol=float("inf")), "f_tol"),
                     (dict(gate_px=-2.0), "gate_px"), (dict(min_parallax=4.0), "min_parallax")):
        with pytest.raises(_native.VoError, match=word) as e:
            ctx.window_structure(*args, **kw)
        assert e.value.code == _native.VO_EINVAL
    with pytest.raises(_native.VoError, match="W must be") as e:
        ctx.window_structure(a["K"], np.zeros((1, 17, 12)), *args[2:])
    assert e.value.code == _native.VO_EINVAL
    with pytest.raises(_native.VoError, match="M_cap"):
        ctx.window_structure(a["K"], a["poses"], a["X"][:, :2], a["lm_start"][:, :3], *args[4:])      # M_cap > L_cap * W
    d = ctx.alloc(4096)
    with pytest.raises(_native.VoError, match="null pointer"):
        ctx.window_structure_dev(1, 4, 12, 40, d, d, d, d, d, d, d, d, None)
    with pytest.raises(_native.VoError, match="S must be"):
        ctx.window_structure_dev(0, 4, 12, 40, d, d, d, d, d, d, d, d, d)
    with pytest.raises(_native.VoError, match="L_cap must be"):
        ctx.window_structure_dev(1, 4, 0, 40, d, d, d, d, d, d, d, d, d)
    ctx.free(d)


# ---- the refiner on the posted loop ----

@pytest.fixture()
def loop(ctx):
    """tests/test_gpu_window_ba.py's posted loop on this module's context (its cache holds device pointers of the context
    that built it: emptied before and after)."""
    import test_gpu_window_ba as wb
    wb._loop.clear()
    lp = wb.posted_loop(ctx)
    yield lp
    lp["pipe"].close()
    ctx.free(lp["d"][0])
    wb._loop.clear()


def test_refiner_refines_the_loops_window(ctx, loop):
    """WindowStructureRefiner on the posted loop: the window it refines is the builder's, the result vo_window_structure's
    on the downloaded window; a break in the step counter drops what lies before it."""
    from test_gpu_window_ba import numpy_window
    from vo.landmarks import WindowStructureRefiner
    lp, W = loop, 4
    prm = dict(max_iter=4, gate_px=2.0, min_parallax=sc.PARALLAX)
    sr = WindowStructureRefiner(lp["K"], window=W, cap=lp["cap"], context=ctx, **prm)
    assert sr.solve() is None
    poses_in = [np.concatenate((np.array(r.R_refined), np.array(r.t_refined))) for r in lp["results"]]
    for k in range(8 - W, 8):
        sr.push(lp["d"][k], poses_in[k])
    out = sr.solve()
    want = numpy_window(lp["records"][-W:], lp["cap"], lp["cap"], lp["cap"] * W)
    L = int(want["head"][0])
    assert L > 20 and out.n == L and np.array_equal(out.ids, want["lm_id"]) and out.steps == [5, 6, 7, 8]
    assert out.poses.tobytes() == np.stack(poses_in[-W:]).tobytes(), "the poses come back as given"
    win = sref.ref.window(lp["K"], np.stack(poses_in[-W:]), want["X"], want["lm_start"], want["obs_slot"], want["obs_xy"])
    _, X, res, summ = run(ctx, [win], **prm)
    assert out.landmarks.tobytes() == X[0, :L].tobytes() and out.results.tobytes() == res[0, :L].tobytes()
    assert out.summary.tobytes() == summ[0].tobytes() and summ[0]["L"] == L
    assert np.array_equal(np.diff(want["lm_start"]), out.results["n_obs"])
    moved = np.any(out.landmarks != want["X"], axis=1)
    print("the loop's window: %d landmarks, %d kept, %d refused, %d moved, cost %.6g -> %.6g" % (
        L, summ[0]["n_kept"], summ[0]["n_refused"], moved.sum(), summ[0]["cost0"], summ[0]["cost"]))
    assert summ[0]["cost"] <= summ[0]["cost0"] and summ[0]["n_kept"] > 0
    assert not np.any(moved & (out.results["kept"] == 0)), "a landmark that is not kept is the record's"
    assert ctx.download(out.d_X, (L, 3), np.float64).tobytes() == out.landmarks.tobytes()
    assert np.array_equal(ctx.download(out.d_ids, (L,), np.int32), out.ids)
    sr.push(lp["d"][2], poses_in[2])                         # step 3 behind step 8: a break
    assert sr.solve() is None and len(sr.records) == 1
    sr.reset()
    assert sr.records == [] and sr.poses == []
    sr.close()
    with pytest.raises(ValueError, match="window must be"):
        WindowStructureRefiner(lp["K"], window=17, context=ctx)


# ---- the driver ----

def test_run_on_device_in_structure_mode(ctx):
    from test_gpu_window_ba import digest
    from vo import driver
    from vo.primitives import Sequence

    def seq():
        return Sequence("synthetic", n_frames=12, height=240, width=320)
    kw = dict(n_keypoints=300, context=ctx, tracks=True)
    prm = dict(max_iter=4, gate_px=2.0)
    plain = driver.run_on_device(seq(), **kw)
    out = driver.run_on_device(seq(), ba_window=4, ba_mode="structure", ba_params=prm, **kw)
    assert digest(out) == digest(plain), "without feedback the loop computes what it computed"
    steps = len(out["results"])
    assert len(out["ba"]) == steps - 3
    print("windows: landmarks %s, kept %s, cost %s" % ([len(e["ids"]) for e in out["ba"]], [e["n_kept"] for e in out["ba"]],
                                                       ["%.4g -> %.4g" % (e["cost0"], e["cost"]) for e in out["ba"]]))
    for k, e in enumerate(out["ba"]):
        assert set(e) == {"frames", "poses", "ids", "landmarks", "kept", "status", "cost0", "cost", "iterations", "n_kept"}
        assert e["frames"] == list(range(k + 1, k + 5)) and e["poses"].shape == (4, 12)
        assert e["status"] == 0 and e["cost"] <= e["cost0"] and e["n_kept"] > 0
        assert e["kept"].dtype == bool and e["kept"].sum() == e["n_kept"] and len(e["kept"]) == len(e["ids"]) == len(e["landmarks"])
        rs = out["results"][k:k + 4]
        assert e["poses"].tobytes() == np.stack([np.concatenate((np.array(r.R_refined), np.array(r.t_refined))) for r in rs]).tobytes()
        newest = out["observations"][k + 3]
        assert np.isin(e["ids"], newest["id"]).all() and np.isfinite(e["landmarks"]).all()
        # a landmark that is not kept is the record's own
        row = {int(i): j for j, i in enumerate(newest["id"])}
        rec = np.array([[newest[row[int(i)]][c] for c in ("X", "Y", "Z")] for i in e["ids"]])
        assert rec[~e["kept"]].tobytes() == e["landmarks"][~e["kept"]].tobytes()
    fed = driver.run_on_device(seq(), ba_window=4, ba_mode="structure", ba_feedback=True, ba_params=prm, **kw)
    assert len(fed["ba"]) == steps - 3 and all(e["cost"] <= e["cost0"] and e["n_kept"] > 0 for e in fed["ba"])
    assert np.isfinite(fed["trajectory"]).all()
    last, f = fed["ba"][-1], fed["features"]
    at = {int(i): j for j, i in enumerate(f.uids)}
    checked = 0
    for i, X, kept in zip(last["ids"], last["landmarks"], last["kept"]):
        j = at.get(int(i))
        if kept and j is not None and f.state[j] == 2:
            assert np.asarray(f.landmarks[j]).reshape(3).tobytes() == X.tobytes()
            checked += 1
    assert checked > 0, "the pipeline holds the refined landmarks after the last step"
    # ba_mode="full" is what the argument's absence is
    full = driver.run_on_device(seq(), ba_window=4, ba_mode="full", ba_params=dict(max_iter=4), **kw)
    today = driver.run_on_device(seq(), ba_window=4, ba_params=dict(max_iter=4), **kw)
    assert digest(full) == digest(today) and len(full["ba"]) == len(today["ba"])
    for a, b in zip(full["ba"], today["ba"]):
        assert set(a) == set(b) and a["poses"].tobytes() == b["poses"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
        assert (a["status"], a["cost0"], a["cost"], a["iterations"]) == (b["status"], b["cost0"], b["cost"], b["iterations"])
    with pytest.raises(ValueError, match="n_fixed"):
        driver.run_on_device(seq(), ba_window=4, ba_mode="structure", ba_params=dict(n_fixed=2), **kw)
    with pytest.raises(ValueError, match="ba_mode"):
        driver.run_on_device(seq(), ba_window=4, ba_mode="poses", **kw)


def test_run_batch_on_device_in_structure_mode(ctx):
    from vo import driver
    from vo.primitives import Sequence

    def seqs():
        return [Sequence("synthetic", n_frames=12 - 2 * i, height=240, width=320, seed=2023 + 11 * i) for i in range(2)]
    kw = dict(n_keypoints=300, context=ctx, tracks=True, ba_window=4, ba_mode="structure", ba_params=dict(max_iter=4, gate_px=2.0))
    out = driver.run_batch_on_device(seqs(), lanes=2, **kw)
    for i in range(2):
        alone = driver.run_on_device(seqs()[i], **kw)
        assert len(out[i]["ba"]) == len(alone["ba"]) == len(out[i]["results"]) - 3
        for a, b in zip(alone["ba"], out[i]["ba"]):
            assert a["frames"] == b["frames"] and np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["kept"], b["kept"])
            assert a["poses"].tobytes() == b["poses"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
            assert (a["status"], a["cost0"], a["cost"], a["iterations"], a["n_kept"]) == (
                b["status"], b["cost0"], b["cost"], b["iterations"], b["n_kept"])
