"""The C oracle of the P3P solve (oracle/csrc/p3p.c) against solution sets from an independent solver.

tests/golden/p3p_cases.npz (tools/make_p3p_cases.py) holds, per case, every pose of the first three points computed
in mpmath at 60 digits by another elimination, ranked by the fourth point.  The oracle is the kernel's twin (same
operations, same order), so an error of the method is in both; this table is what says the answer is right."""
import os
import sys

import numpy as np
import pytest

import p3p_cases as pc
from oracle import native


@pytest.fixture(scope="module")
def tab():
    return pc.table()


@pytest.fixture(scope="module")
def solved(tab):
    """the oracle's (valid, R, t) for every case, and what pc.measure makes of them"""
    n = len(tab["n_sol"])
    valid, R, t = np.zeros(n, np.uint8), np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        got = native.p3p_solve(tab["X"][i], tab["x"][i], tab["K_table"][tab["K_index"][i]])
        if got is not None:
            valid[i], R[i], t[i] = 1, got[0], got[1]
    return valid, R, t, pc.measure(tab, valid, R, t)


def test_table_covers_its_families(tab):
    fam = tab["family"]
    assert set(fam) == set(pc.FAMILIES)
    gen = fam == "generic"
    assert gen.sum() >= 1500
    assert set(tab["n_sol"][gen]) == {0, 1, 2, 3, 4}, "every solution count occurs among the generic cases"
    assert set(tab["sub"][gen]) == {"n0", "n0.3"} and set(tab["K_index"][gen]) == {0, 1, 2}
    assert (tab["n_sol"][fam == "outlier"] == 0).any()
    subs = set(tab["sub"])
    for s in ("equi_d0", "equi_d1e-12", "equi_moved_d0", "isos_y0_h3", "repeat01", "collinear0", "fourth_is_0", "on_axis0",
              "fourth_behind", "offset1e4", "danger_cylinder", "small_dd", "equi_alt_d0", "equi_alt_d0.001"):
        assert s in subs, s
    assert os.path.getsize(pc.PATH) < 560 * 1024


def test_hypothesis_batch_equals_single_solves(tab, solved):
    """oracle_p3p_hypotheses (what the GPU tests compare the kernel with) is oracle_p3p_solve per sample"""
    valid, R, t, _ = solved
    for Kid in range(3):
        rows, K, X, x, samples = pc.pack(tab, Kid)
        Rh, th, vh, counts, _ = native.p3p_hypotheses(X, x, K, samples, 1.0)
        assert np.array_equal(vh, valid[rows]) and np.array_equal(Rh, R[rows]) and np.array_equal(th, t[rows])
        assert (counts[vh == 0] == 0).all() and (counts[vh == 1] >= 3).all()


def test_oracle_validity(tab, solved):
    """A pose exactly where the reference's solution set is not empty (but for cases marked `conditioning`: the only
    positive root double to 1e-6, which rounding may lose -- the table has none at present)."""
    pc.check_validity(tab, solved[0])


def test_oracle_backward_error(tab, solved):
    """Every returned R is a rotation to 1e-12 and the three solved points reproject within 1e-3 px: 16 times the
    worst generic case of this table (6.2e-5 px), three orders below the 1 px RANSAC threshold.

    Measured with this oracle (max-abs px over the family): generic 6.2e-5 (a 0.3 px noise case), outlier 7.3e-8,
    symmetric 7.0e-7, biquadratic 2.3e-12, rejects 1.5e-10, edges 9.8e-10.  The symmetric maximum is the Nn / Dd route
    at delta = 1e-2 (fx = 2759); every case that takes the quadratic route is below 1e-11 px.  Before the
    vanishing-denominator repair the symmetric family stood at 11.6 px (equi_d0), 22 cases above the bound."""
    worst = pc.check_backward(tab, solved[3])
    assert worst["symmetric"] <= 1e-4, "the repair of the vanishing denominator is not good enough"


def test_oracle_selection(tab, solved):
    """Well separated cases (positive v roots pairwise more than 1e-3 apart, best and second-best fourth-point errors
    more than 1e-6 px^2 apart) return the reference's best pose to 1e-6; the others some pose of the reference's set
    to 1e-4.  At most 5 % of the generic family may fall outside `well separated`."""
    pc.check_selection(tab, solved[3])


def test_oracle_picks_the_right_root_at_a_vanishing_denominator(tab, solved):
    pc.check_demanded(tab, solved[3])


def test_table_is_what_the_generator_writes(tab):
    """A stratified twentieth of the table, rebuilt from (family, k) alone, equals the committed rows to 1e-12."""
    pytest.importorskip("mpmath")
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import make_p3p_cases as gen
    assert np.array_equal(gen.KS, tab["K_table"])
    picked = 0
    for f in pc.FAMILIES:
        rows = np.flatnonzero(tab["family"] == f)
        for i in rows[len(rows) // 2 % 20::20]:
            row = gen.make_case(f, int(tab["k"][i]))
            assert row is not None and row["sub"] == tab["sub"][i] and row["K_index"] == tab["K_index"][i], pc.name(tab, i)
            assert row["n_sol"] == tab["n_sol"][i] and row["n_v"] == tab["n_v"][i], pc.name(tab, i)
            assert row["conditioning"] == tab["conditioning"][i] and row["demand_best"] == tab["demand_best"][i]
            for key in ("X", "x", "q", "t", "e4", "v"):
                assert np.allclose(row[key], tab[key][i], rtol=1e-12, atol=1e-12), (pc.name(tab, i), key)
            picked += 1
    assert picked >= len(tab["n_sol"]) // 20
