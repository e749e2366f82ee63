"""The definition of the window structure refinement (tests/window_structure_reference.py) on its case table
(tests/window_structure_cases.py), without a GPU: what the kernel is pinned to must itself be right (SciPy, the generating
landmarks), must not depend on the order its sums are formed in, and must take no decision by a hair -- the condition under
which tests/test_gpu_window_structure.py may demand equal counts of the kernel."""
import numpy as np
import pytest

import window_structure_cases as sc
import window_structure_reference as sref

NOISY_SOLVED = [n for n in sc.SOLVED if not n.endswith("_exact")]


def test_cases_keep_the_edge_they_are_named_for():
    for name, W, L in (("w2_l1", 2, 1), ("w2_l5", 2, 5), ("w16_l17_full", 16, 17), ("w16_l33_ragged", 16, 33),
                       ("w16_l64_missing_huber", 16, 64), ("l65", 5, 65), ("l129", 5, 129), ("w8_l600", 8, 600)):
        c = sc.get(name)
        assert (len(c.win.poses), len(c.win.X)) == (W, L), name
    for name in sc.SOLVED + list(sc.WINDOW_REFUSED):
        c = sc.get(name)
        assert np.array_equal(c.win.poses[np.isfinite(c.win.poses)], c.true_poses[np.isfinite(c.win.poses)]), "the poses are the generating ones"
    n = np.diff(sc.get("w16_l17_full").win.lm_start)
    assert np.all(n == 16), "every lane of a row is busy"
    n = np.diff(sc.get("w16_l33_ragged").win.lm_start)
    assert n.min() == 2 and n.max() == 16 and len(set(n)) > 8
    n = np.diff(sc.get("w16_l64_missing_huber").win.lm_start)
    assert n.min() < 16 and len(sc.get("w16_l64_missing_huber").outlier_obs) > 0 and sc.get("w16_l64_missing_huber").huber_px == 2.0
    assert np.all(np.diff(sc.get("w2_l5").win.lm_start) == 2)
    # the bad landmarks: one observation, behind the camera, a NaN observation; all the others are solved
    c = sc.get("bad_landmarks")
    d = sc.definition("bad_landmarks", 50)
    assert np.diff(c.win.lm_start)[3] == 1 and c.win.X[6, 2] < 0 and np.isnan(c.win.obs_xy[c.win.lm_start[9]:c.win.lm_start[10]]).sum() == 1
    assert np.flatnonzero(d.status == sref.STATUS_REFUSED).tolist() == list(c.bad)
    assert d.n_obs[3] == 1 and (d.summary.n_refused, d.summary.n_kept, d.summary.L) == (3, 9, 12)
    # refused windows: every landmark
    for name in sc.WINDOW_REFUSED:
        c = sc.get(name)
        d = sref.solve(c.win)
        assert sref.window_refusal(c.win) is not None and np.all(d.status == sref.STATUS_REFUSED) and d.summary.n_refused == len(c.win.X)
    assert sc.get("csr_does_not_end_at_m").win.lm_start[-1] != len(sc.get("csr_does_not_end_at_m").win.obs_slot)
    assert not np.all(np.isfinite(sc.get("non_finite_pose").win.poses))
    # zero parallax: the thin landmark converges and is not kept, every other one is
    c = sc.get("zero_parallax")
    d = sc.definition("zero_parallax", 50)
    assert np.array_equal(c.win.poses[0], c.win.poses[1]) and np.diff(c.win.lm_start)[c.thin] == 2
    assert d.min_cos[c.thin] > np.cos(sc.PARALLAX) and d.status[c.thin] in (0, 1) and d.kept[c.thin] == 0
    assert np.all(np.delete(d.kept, c.thin) == 1)
    # the noise-free copies: the observations are the exact projections
    for name in sc.NOISE_FREE:
        c = sc.get(name)
        win = sref.ref.window(c.win.K, c.win.poses, c.true_X, c.win.lm_start, c.win.obs_slot, c.win.obs_xy)
        _, e, _, _ = sref.ref.residuals(win, win.poses, win.X)
        assert np.abs(e).max() < 1e-10, name


@pytest.mark.parametrize("name", NOISY_SOLVED)
def test_converged_cost_is_scipys(name):
    """Per landmark, not more than 2e-9 relative (2 f_tol: what is left at the stop is at most the predicted decrease of
    the last solve) above SciPy's least_squares on the same objective.  The noise-free copies, whose cost at the stop is
    rounding noise around zero, are held to the generating landmarks instead (below)."""
    d = sc.definition(name, 50)
    sp = sc.scipy_costs(name)
    live = d.status != sref.STATUS_REFUSED
    assert np.all(np.isin(d.status[live], (0, 1)))
    over = (d.cost[live] - sp[live]) / sp[live]
    print("%s: the definition's converged cost above SciPy's by at most %.3g relative" % (name, over.max()))
    assert np.all(over <= 2e-9)


@pytest.mark.parametrize("name", list(sc.NOISE_FREE))
def test_noise_free_cases_reach_the_generating_landmarks(name):
    c = sc.get(name)
    d = sc.definition(name, 50)
    off = np.abs(d.X - c.true_X) / (1.0 + np.abs(c.true_X))
    print("%s: off the generating landmarks by at most %.3g (1 + |X|)" % (name, off.max()))
    assert np.all(d.status == 0) and np.all(d.kept == 1)
    assert np.all(off <= 1e-8)


@pytest.mark.parametrize("name", sc.NOISY)
def test_noisy_cases_move_towards_the_generating_landmarks(name):
    c = sc.get(name)
    d = sc.definition(name, 50)
    before, after = sc.landmark_rms(c, c.win.X), sc.landmark_rms(c, d.X)
    print("%s: RMS distance to the generating landmarks %.2f -> %.2f m" % (name, before, after))
    assert after < before


@pytest.mark.parametrize("name", sc.SOLVED)
def test_observation_order_changes_no_decision(name):
    c = sc.get(name)
    M = len(c.win.obs_slot)
    rng = np.random.default_rng(2024)
    perms = [rng.permutation(M) for _ in range(4)]
    worst = 0.0
    for max_iter in (2, 4, 50):
        d = sc.definition(name, max_iter)
        for perm in perms:
            p = sc.definition(name, max_iter, perm=perm)
            for key in ("status", "iterations", "trials", "kept", "n_obs"):
                assert np.array_equal(getattr(p, key), getattr(d, key)), (name, max_iter, key)
            worst = max(worst, float((np.abs(p.X - d.X) / (1.0 + np.abs(d.X))).max()))
    print("%s: X moves by at most %.3g (1 + |X|) under a permuted observation order" % (name, worst))
    assert worst <= 1e-9


def test_no_decision_is_taken_by_a_hair():
    """What makes exact counts a fair demand of the kernel: over every case, at max_iter 2, 4 and 50 and with the 2 px gate,
    the closest decision of the definition keeps a relative margin of at least 1e-10."""
    worst = {k: np.inf for k in sref.MARGIN_KINDS}
    for name in sc.SOLVED:
        runs = [sc.definition(name, m) for m in (2, 4, 50)]
        if name in sc.GATED:
            runs.append(sc.definition(name, 50, sc.GATE_PX))
        for d in runs:
            for k, v in d.margins.items():
                worst[k] = min(worst[k], v)
    print("closest decisions:", {k: "%.3g" % v for k, v in worst.items()})
    assert all(np.isfinite(v) for v in worst.values()), "every kind of decision was taken somewhere"
    assert min(worst.values()) >= 1e-10


@pytest.mark.parametrize("name", sc.GATED)
def test_gate_keeps_the_landmarks_without_an_outlier(name):
    c = sc.get(name)
    d = sc.definition(name, 50, sc.GATE_PX)
    lm = sref.ref.obs_landmark(c.win.lm_start)
    clean = np.ones(len(c.win.X), bool)
    clean[lm[c.outlier_obs]] = False
    print("%s: %d of %d landmarks kept at %g px" % (name, d.kept.sum(), len(d.kept), sc.GATE_PX))
    assert 0 < clean.sum() < len(clean)
    assert np.array_equal(d.kept.astype(bool), clean)
    assert d.summary.n_kept == clean.sum()


def test_refused_and_unkept_landmarks_return_their_input_bits():
    c = sc.get("bad_landmarks")
    d = sc.definition("bad_landmarks", 50)
    for i in c.bad:
        assert d.X[i].tobytes() == c.win.X[i].tobytes()
    good = np.setdiff1d(np.arange(len(c.win.X)), c.bad)
    assert not np.any(np.all(d.X[good] == c.win.X[good], axis=1)), "the neighbours move"
    alone = sc.definition("without_bad", 50)
    assert alone.X.tobytes() == d.X[good].tobytes(), "one bad landmark never touches its neighbours"
    for name in sc.WINDOW_REFUSED:
        w = sc.get(name).win
        assert sref.solve(w).X.tobytes() == w.X.tobytes()
    for name in sc.GATED:
        c = sc.get(name)
        d = sc.definition(name, 50, sc.GATE_PX)
        out = d.kept == 0
        assert out.any() and d.X[out].tobytes() == c.win.X[out].tobytes()
        assert not np.any(np.all(d.X[~out] == c.win.X[~out], axis=1))
    c = sc.get("zero_parallax")
    d = sc.definition("zero_parallax", 50)
    assert d.X[c.thin].tobytes() == c.win.X[c.thin].tobytes()
