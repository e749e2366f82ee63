"""The window bundle adjustment's definition (tests/window_ba_reference.py) and case table (tests/window_ba_cases.py), on
the host: every case keeps the edge it is named for; the definition reaches SciPy's minimum of the same objective; and what
summation order alone moves stays far below the bar the kernels are held to (tests/test_gpu_window_ba.py)."""
import numpy as np
import pytest

import window_ba_cases as wc
import window_ba_reference as ref

SPREAD_BOUND = 1e-9          # poses and landmarks under a permuted observation order, max_iter <= 4
MARGIN_BOUND = 1e-6          # the closest decision of such a run


def test_every_case_keeps_its_edge():
    full = wc.get("w3_l8_full")
    assert full.seen.shape == (8, 3) and full.seen.all()
    miss = wc.get("w4_l12_missing")
    assert miss.seen.shape == (12, 4) and not miss.seen.all() and miss.seen.sum(axis=1).min() >= 2
    rag = wc.get("w6_l40_ragged")
    assert rag.seen.shape == (40, 6) and set(rag.seen.sum(axis=1)) == set(range(2, 7))
    for name, huber in (("w8_l60_outliers_huber", 2.0), ("w8_l60_outliers_squared", 0.0)):
        c = wc.get(name)
        assert c.seen.shape == (60, 8) and c.huber_px == huber
        assert len(c.outlier_obs) == round(0.05 * len(c.win.obs_slot)) > 0
        e = ref.residuals(ref.window(c.win.K, c.true_poses, c.true_X, c.win.lm_start, c.win.obs_slot, c.win.obs_xy),
                          c.true_poses, c.true_X)[1]
        assert np.all(np.linalg.norm(e[c.outlier_obs], axis=1) > 10.0)            # gross: each axis off by 8 px or more, the noise is 0.3 px
    fo = wc.get("fixed_only_landmark")
    assert np.any(fo.seen[:, :fo.n_fixed].any(axis=1) & ~fo.seen[:, fo.n_fixed:].any(axis=1))
    thin = wc.get("three_observation_pose")
    assert 3 in thin.seen[:, thin.n_fixed:].sum(axis=0)
    assert wc.get("n_fixed_1").n_fixed == 1
    assert len(wc.get("l65").win.X) == 65 and len(wc.get("l129").win.X) == 129
    big = wc.get("w8_l600")
    assert len(big.win.X) == 600 and len(big.win.poses) == 8 and 3000 <= len(big.win.obs_slot) <= 4000
    sizes = {None if n is None else len(wc.get(n).win.X) for n in wc.BATCH}
    assert len(wc.BATCH) == 3 and None in sizes and len(sizes) == 3
    for name in wc.CASES:
        w = wc.get(name).win
        assert ref.refusal(w, wc.get(name).n_fixed) is None
        for i in range(len(w.X)):                                                  # ascending slots within a landmark
            assert np.all(np.diff(w.obs_slot[w.lm_start[i]:w.lm_start[i + 1]]) > 0)


@pytest.mark.parametrize("name", list(wc.REFUSED))
def test_refused_windows_come_back_unchanged(name):
    c = wc.get(name)
    before = (c.win.poses.copy(), c.win.X.copy())
    r = ref.solve(c.win, c.n_fixed, c.huber_px, 4)
    assert r.status == ref.STATUS_REFUSED and r.iterations == 0 and r.trials == 0
    assert np.array_equal(r.poses, before[0]) and np.array_equal(r.X, before[1], equal_nan=True)
    assert ref.solve(wc.empty_window(4)).status == ref.STATUS_REFUSED
    assert ref.solve(wc.get("w3_l8_full").win, n_fixed=3).status == ref.STATUS_REFUSED       # no free pose


@pytest.mark.parametrize("name", wc.SOLVED)
def test_definition_reaches_scipys_minimum(name):
    c = wc.get(name)
    r = wc.definition(name, 50)
    sp = wc.scipy_cost(name)
    print("%s: definition %.15g (status %d, %d iterations, %d trials), SciPy %.15g, relative difference %.3e" % (
        name, r.cost, r.status, r.iterations, r.trials, sp, (r.cost - sp) / sp))
    assert r.status in (ref.STATUS_CONVERGED, ref.STATUS_LAMBDA)
    assert r.cost <= sp * (1.0 + 1e-9)
    # the gradient at the result against the size of its terms: sum |w J^T e| over the observations, entry by entry
    lin = ref.linearise(c.win, r.poses, r.X, c.n_fixed, c.huber_px, np.arange(len(c.win.obs_slot)))
    g = max(np.abs(lin.gp[c.n_fixed:]).max(), np.abs(lin.gl).max())
    p, e, _, w = ref.residuals(c.win, r.poses, r.X, c.huber_px)
    Jp, Jl = ref.jacobians(c.win, r.poses, p)
    scale = max(np.abs(w[:, None, None] * Jp * e[:, :, None]).sum(axis=(0, 1)).max(),
                np.abs(w[:, None, None] * Jl * e[:, :, None]).sum(axis=(0, 1)).max())
    print("%s: |gradient|_inf %.3e against terms of %.3e" % (name, g, scale))
    assert g <= 1e-6 * scale


@pytest.mark.parametrize("max_iter", [2, 4])
@pytest.mark.parametrize("name", wc.SOLVED)
def test_summation_order_moves_little_and_no_decision_is_close(name, max_iter):
    c = wc.get(name)
    base = wc.definition(name, max_iter)
    assert base.status == ref.STATUS_MAX_ITER and base.iterations == max_iter
    assert base.cost <= base.cost0
    rng = np.random.default_rng(100 + max_iter)
    spread, cost_spread, margin = 0.0, 0.0, base.min_margin
    for _ in range(4):
        r = wc.definition(name, max_iter, perm=rng.permutation(len(c.win.obs_slot)))
        assert (r.status, r.iterations, r.trials) == (base.status, base.iterations, base.trials)
        spread = max(spread, np.abs(r.poses - base.poses).max(), np.abs(r.X - base.X).max())
        cost_spread = max(cost_spread, abs(r.cost - base.cost) / base.cost)
        margin = min(margin, r.min_margin)
    print("%s, max_iter %d: spread %.3e, cost spread %.3e, smallest margin %.3e" % (name, max_iter, spread, cost_spread, margin))
    assert spread <= SPREAD_BOUND
    assert margin >= MARGIN_BOUND


@pytest.mark.parametrize("name", wc.NOISY)
def test_noisy_windows_move_towards_the_generating_poses(name):
    c = wc.get(name)
    before, after = wc.pose_rms(c, c.win.poses), wc.pose_rms(c, wc.definition(name, 4).poses)
    print("%s: free poses' RMS distance from the generating ones %.4f -> %.4f" % (name, before, after))
    assert after < before
