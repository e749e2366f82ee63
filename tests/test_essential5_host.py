"""The five-point case table and the float64 definition of the rule, on the CPU: the 50-digit golden is self-consistent,
every case keeps the edge it is named for, and the definition's distance to the golden sets -- the yardstick the kernel's
tolerance is derived from (tests/essential5_cases.py, DEFINITION) -- is what the case module records."""
import numpy as np
import pytest

import essential5_cases as cases
import essential5_reference as ref


@pytest.fixture(scope="module")
def tab():
    return cases.table()


@pytest.fixture(scope="module")
def solved(tab):
    """the definition on every case: [(n_sol, E, normalised points 1, 2)]"""
    out = []
    for i in range(len(tab["family"])):
        h1 = ref.normalise(ref.pinhole_inverse(tab["K1"][i]), tab["x1"][i])
        h2 = ref.normalise(ref.pinhole_inverse(tab["K2"][i]), tab["x2"][i])
        n, E, _ = ref.solve5(h1, h2)
        out.append((n, E, h1, h2))
    return out


def test_table_layout(tab):
    n = len(tab["family"])
    assert 100 <= n <= 140 and set(tab["family"]) == set(cases.FAMILIES)
    assert tab["E"].shape == (n, 10, 3, 3) and tab["E50"].shape == (n, 10, 9) and tab["x1"].shape == (n, 5, 2)
    for i in range(n):
        k = tab["n_sol"][i]
        assert np.all(tab["E"][i, k:] == 0.0) and np.all(tab["E50"][i, k:] == b"")
        assert bool(tab["separated"][i]) == (tab["family"][i] in cases.SEPARATED)


def test_golden_is_self_consistent(tab):
    """Every stored E meets the five epipolar equations and the ten constraints to 1e-40 at 50 digits, is canonical, and
    the ground truth is a member of the set."""
    import mpmath as mp
    worst = 0.0
    member = {}
    for i in range(len(tab["family"])):
        h1, h2 = cases.mp_normalise(tab["K1"][i], tab["x1"][i]), cases.mp_normalise(tab["K2"][i], tab["x2"][i])
        k = tab["n_sol"][i]
        for s in range(k):
            E = cases.mp_matrix_of(tab["E50"][i, s])
            r = max(cases.mp_residuals(E, h1, h2))
            worst = max(worst, float(r))
            assert r < mp.mpf(10) ** -40, (cases.name(tab, i), s, r)
            assert abs(mp.sqrt(sum(E[a, b] ** 2 for a in range(3) for b in range(3))) - 1) < mp.mpf(10) ** -45
            f = tab["E"][i, s].reshape(9)
            assert f[np.argmax(np.abs(f))] > 0.0
        if tab["family"][i] != "rejects":
            assert k >= 1
            d = min(np.linalg.norm(tab["E"][i, s] - tab["E_true"][i]) for s in range(k))
            member[tab["family"][i]] = max(member.get(tab["family"][i], 0.0), d)
            assert d < cases.MEMBER[bool(tab["separated"][i])], (cases.name(tab, i), d)
    print("worst 50-digit residual %.2e; ground truth to its set, per family: %s" % (
        worst, {k: "%.1e" % v for k, v in member.items()}))


def test_every_case_keeps_its_edge(tab):
    for i in range(len(tab["family"])):
        fam, sub, k = tab["family"][i], tab["sub"][i], tab["n_sol"][i]
        h1 = ref.normalise(ref.pinhole_inverse(tab["K1"][i]), tab["x1"][i])
        h2 = ref.normalise(ref.pinhole_inverse(tab["K2"][i]), tab["x2"][i])
        Et = tab["E_true"][i]
        if fam in cases.SEPARATED:
            assert tab["gap_real"][i] > cases.ROOT_GAP and tab["gap_imag"][i] > cases.ROOT_GAP, cases.name(tab, i)
        if fam == "few":
            assert k == 2
        if fam == "many":
            assert k >= 6
        if fam == "forward" or sub == "forward":             # t along the optical axis: t^T E = 0 with t = e_z
            assert np.abs(Et[2]).max() < 1e-12, cases.name(tab, i)
        if fam == "sideways":
            assert np.abs(Et[0]).max() < 1e-12, cases.name(tab, i)
        if fam == "planar":                                   # the homography of four of the points maps the fifth
            A = []
            for p, q in zip(h1[:4], h2[:4]):
                A.append(np.concatenate([np.zeros(3), -q[2] * p, q[1] * p]))
                A.append(np.concatenate([q[2] * p, np.zeros(3), -q[0] * p]))
            H = np.linalg.svd(np.array(A))[2][-1].reshape(3, 3)
            q = H @ h1[4]
            assert np.abs(q[:2] / q[2] - h2[4, :2] / h2[4, 2]).max() < 1e-9, cases.name(tab, i)
        if fam == "pixels":
            assert not np.array_equal(tab["K1"][i], np.eye(3))
        if fam == "near-rotation":                            # a rotation alone explains the bearings to 1e-3, not exactly
            u1 = h1 / np.linalg.norm(h1, axis=1, keepdims=True)
            u2 = h2 / np.linalg.norm(h2, axis=1, keepdims=True)
            U, _, Vt = np.linalg.svd(u2.T @ u1)
            Rf = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
            r = np.abs(u2 - u1 @ Rf.T).max()
            assert 1e-7 < r < 1e-3, (cases.name(tab, i), r)
        if sub == "repeated":
            assert np.array_equal(tab["x1"][i, 3], tab["x1"][i, 1]) and np.array_equal(tab["x2"][i, 3], tab["x2"][i, 1])
        if sub == "all-equal":
            assert np.all(tab["x1"][i] == tab["x1"][i, 0]) and np.all(tab["x2"][i] == tab["x2"][i, 0])
        if sub == "collinear":
            assert np.linalg.svd(h1, compute_uv=False)[-1] < 1e-12
    assert any(not np.array_equal(tab["K1"][i], tab["K2"][i]) for i in range(len(tab["family"])))


def test_definition_against_the_golden_sets(tab, solved):
    """The measured yardstick: per family the definition's worst set distance and backward figures; none exceeds what
    tests/essential5_cases.py records (the kernel's bars are 100 times those)."""
    fig = {}
    for i, (n, E, h1, h2) in enumerate(solved):
        fam, k = tab["family"][i], tab["n_sol"][i]
        f = fig.setdefault(fam, dict(set=0.0, norm=0.0, epipolar=0.0, det=0.0, trace=0.0))
        assert np.all(np.isfinite(E)) and np.all(E[n:] == 0.0)
        if fam in cases.SEPARATED:
            assert n == k, (cases.name(tab, i), n, k)
            f["set"] = max(f["set"], ref.set_distance(E[:n], tab["E"][i, :k]))
        for s in range(n):
            b = ref.backward_figures(E[s], h1, h2)
            assert b[1], cases.name(tab, i)
            for key, v in zip(("norm", "epipolar", "det", "trace"), (b[0], b[2], b[3], b[4])):
                f[key] = max(f[key], v)
    for fam in cases.FAMILIES:
        print(fam, {k: "%.2e" % v for k, v in fig[fam].items()})
        for key, v in fig[fam].items():
            rec = cases.DEFINITION[fam][key]
            if rec is not None:
                assert v <= rec, (fam, key, v, rec)
                assert fam == "rejects" or key == "norm" or v >= 0.5 * rec, (fam, key, v, rec)   # (the record is current)


def test_rejects_have_no_solution_in_the_definition(tab, solved):
    for i, (n, E, _, _) in enumerate(solved):
        if tab["family"][i] == "rejects":
            assert n == 0 and np.all(E == 0.0), cases.name(tab, i)


def test_definition_stages():
    """The stages on one generic sample: an orthonormal null space of the system, a reduced matrix with the identity in
    front, a polynomial whose roots the root finder returns in ascending order."""
    tab = cases.table()
    i = int(np.flatnonzero(tab["family"] == "generic")[0])
    h1, h2 = tab["x1"][i] @ np.eye(2, 3) + [0, 0, 1], tab["x2"][i] @ np.eye(2, 3) + [0, 0, 1]
    ok, basis = ref.null_space(h1, h2)
    assert ok and np.allclose(basis @ basis.T, np.eye(4), atol=1e-14)
    Q = np.array([np.kron(a, b) for a, b in zip(h1, h2)])
    assert np.abs(Q @ basis.T).max() < 1e-14
    M = ref.constraint_matrix(basis)
    c = np.array([0.3, -0.2, 0.7, 1.0])                      # the constraints evaluated at a point, both ways
    E = np.tensordot(c, basis, 1).reshape(3, 3).T
    mono = np.array([np.prod(c[list(m)]) for m in ref.MONOMIALS])
    G = E @ E.T
    assert np.allclose(M @ mono, np.concatenate([[np.linalg.det(E)], (2 * G @ E - np.trace(G) * E).reshape(9)]), atol=1e-13)
    ok, R = ref.eliminate(M)
    assert ok and np.allclose(R[:, :10], np.eye(10), atol=1e-12)
    poly = ref.det_polynomial(ref.b_matrix(R))
    ok, roots = ref.real_roots(poly)
    assert ok and roots == sorted(roots) and len(roots) == tab["n_sol"][i]
    want = np.roots(poly[::-1])
    want = np.sort(want[np.abs(want.imag) < 1e-9 * np.maximum(1, np.abs(want))].real)
    assert np.allclose(roots, want, rtol=1e-8)


def test_scorer_formula_and_exempt_share():
    """The seeded scoring scene stays under the exempt share with the definition's own matrices, for both error kinds; an
    absent solution counts 0."""
    x1, x2, K, _, _, _ = cases.scene(200, 7)
    samples = np.random.default_rng(8).integers(0, 200, size=(65, 5)).astype(np.int32)
    samples[3, 1] = samples[3, 0]                              # a repeated correspondence: no solution
    E, n_sol = ref.hypotheses(x1, x2, K, K, samples)
    assert n_sol[3] == 0 and n_sol.max() >= 4
    for kind, thr in ((0, cases.THRESHOLDS[0]), (1, cases.THRESHOLDS[1])):
        counts, masks, near = cases.expected_scores(E, n_sol, x1, x2, K, K, kind, thr)
        decisions = int(n_sol.sum()) * 200
        assert near.sum() <= cases.EXEMPT_SHARE * decisions, (kind, int(near.sum()), decisions)
        assert counts[3].sum() == 0 and counts.max() > 100
        for h in range(len(samples)):
            assert np.all(counts[h, n_sol[h]:] == 0)
