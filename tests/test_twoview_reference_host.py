"""The definitions of the 8-point rule and the DLT (tests/twoview_reference.py) against the 50-digit values of
tests/golden/twoview_cases.npz -- the fit under permuted point orders -- against oracle/bootstrap_np.py and
oracle/dlt_np.py, and the self-checks of the case tables (tests/twoview_cases.py).  CPU only.

This file measures the bars of tests/test_gpu_twoview_reference.py: the largest distance of the float64 definition from
the 50-digit value per group must stay below twoview_cases.DEFINITION_DISTANCE (the kernels are allowed 100 times that),
and pins the LAPACK oracles, which the older GPU tests compare the kernels with, at twoview_cases.LAPACK_DISTANCE."""
import functools

import numpy as np
import pytest

import twoview_cases as tc
import twoview_reference as tr
from oracle import bootstrap_np, dlt_np

N_PERM = 20


def orders(n):
    rng = np.random.default_rng(n)
    return [None] + [rng.permutation(n) for _ in range(N_PERM)]


def lapack_fit(a, b, normalize):
    with np.errstate(all="ignore"):
        return bootstrap_np.find_fundamental_matrix(a.reshape(-1, 2, 1), b.reshape(-1, 2, 1), is_normalized=not normalize)


def homogeneous(X):
    return np.concatenate((X, np.ones((len(X), 1))), axis=1)


@functools.lru_cache(maxsize=None)
def measured():
    """(definition, lapack): group -> quantity -> (largest distance, case)."""
    d, l = {}, {}

    def note(store, group, quantity, value, name):
        q = store.setdefault(group, {})
        q[quantity] = max(q.get(quantity, (0.0, "")), (float(value), name))

    gold = tc.golden("fit")
    for c in tc.table("fit"):
        if c.kind == "solved":
            for perm in orders(len(c.p1)):
                F, sig, n = tr.fundamental(c.p1, c.p2, c.mask, c.normalize, perm)
                note(d, c.group, "F", tc.vector_distance(F, gold[c.name].F), c.name)
            note(l, c.group, "F", tc.vector_distance(lapack_fit(c.p1[c.on], c.p2[c.on], c.normalize), gold[c.name].F), c.name)
    gold = tc.golden("hyp")
    for c in tc.table("hyp"):
        if c.kind == "solved":
            F, sig = tr.fundamental_samples(c.p1, c.p2, c.samples, c.normalize)
            for h, s in enumerate(c.samples):
                note(d, c.group, "F", tc.vector_distance(F[h], gold[c.name].F[h]), c.name)
                note(l, c.group, "F", tc.vector_distance(lapack_fit(c.p1[s], c.p2[s], c.normalize), gold[c.name].F[h]), c.name)
    gold = tc.golden("dlt")
    for c in tc.table("dlt"):
        if c.kind == "solved":
            v, X, sig = tr.dlt(c.x1, c.x2, c.C1, c.C2)
            Xl = dlt_np.linear_triangulation(c.x1, c.x2, c.C1, c.C2)
            g = gold[c.name]
            for i in range(len(v)):
                note(d, c.group, "v", tc.vector_distance(v[i], g.v[i]), c.name)
                note(l, c.group, "v", tc.vector_distance(homogeneous(Xl)[i], g.v[i]), c.name)
            if c.compare == "point":
                note(d, c.group, "X", tc.point_distance(X, g.X).max(), c.name)
                note(l, c.group, "X", tc.point_distance(Xl, g.X).max(), c.name)
    return d, l


def test_definitions_match_the_50_digit_values():
    """Per group and quantity: the largest distance is below the recorded one (which sets the kernel's bar for that group)
    and within a factor of ten of it, or below the floor.  The LAPACK oracles likewise, at their own recorded distances."""
    for what, got, recorded in (("definition", measured()[0], tc.DEFINITION_DISTANCE), ("lapack", measured()[1], tc.LAPACK_DISTANCE)):
        for g in sorted(got):
            print("%-10s %-18s" % (what, g), "  ".join("%s %.2g (%s)" % (q, *got[g][q]) for q in sorted(got[g])))
    for what, got, recorded in (("definition", measured()[0], tc.DEFINITION_DISTANCE), ("lapack", measured()[1], tc.LAPACK_DISTANCE)):
        assert sorted(got) == sorted(recorded), what
        for g in got:
            assert sorted(got[g]) == sorted(recorded[g]), (what, g)
            for q, (worst, name) in got[g].items():
                r = recorded[g][q]
                assert worst <= r, (what, g, q, worst, name)
                # (LAPACK's values depend on the library build: its record is an upper bound with room, not a measurement)
                assert what == "lapack" or r == tc.DISTANCE_FLOOR or worst >= 0.1 * r, ("the recorded distance is stale", g, q, worst)
                assert r >= tc.DISTANCE_FLOOR
    for which in ("fit", "hyp", "dlt"):
        for c in tc.table(which):
            if c.kind == "solved":
                assert c.group in tc.DEFINITION_DISTANCE, c.name
                for q in tc.DEFINITION_DISTANCE[c.group]:
                    assert tc.bar(q, c.group, which) <= tc.CAPS[which]


def test_the_definition_is_not_far_behind_lapack():
    """More than 100 times LAPACK's distance in a group would be a finding about the Jacobi rule itself."""
    d, l = measured()
    for g in d:
        for q in d[g]:
            assert d[g][q][0] <= 100.0 * max(l[g][q][0], tc.DISTANCE_FLOOR), (g, q, d[g][q], l[g][q])


def ratio(sig, k):
    return sig[..., k] / sig[..., 0]


def test_fit_cases_are_named_for():
    by, gold = {c.name: c for c in tc.table("fit")}, tc.golden("fit")
    assert [len(by["size_%d" % n].p1) for n in tc.SIZES] == list(tc.SIZES)
    for n in tc.SIZES:
        c = by["size_%d" % n]
        assert c.mask is None and c.normalize and c.on.all()
        assert np.abs(c.p1 - tc.two_views(tc.SEEDS["sizes"], n, "wide", 0.0).p1).max() > 0.05, "noisy"
    for n in tc.PRENORMALISED:
        c = by["prenormalised_%d" % n]
        assert not c.normalize and len(c.p1) == n
        for p in (c.p1, c.p2):
            assert np.abs(p.mean(axis=0)).max() < 1e-12 and abs((p * p).sum(axis=1).mean() - 2.0) < 1e-12
    for n in (300, 2500):
        c = by["mask_bytes_60pct_n%d" % n]
        assert set(np.unique(c.mask)) == {0, 1, 2, 255} and 0.55 < (c.mask != 0).mean() < 0.65 and len(c.mask) == n
    for name in ("mask_bytes_60pct_n300", "mask_bytes_60pct_n2500", "mask_only_past_256_n600", "mask_on8_n600",
                 "mask_on9_first_and_last_n600"):
        c = by[name]
        assert np.array_equal(c.mask != 0, c.on) and set(np.unique(c.mask[c.on])) <= {1, 2, 255}
        clean = tc.two_views(tc.SEEDS["masks"] + {"mask_on8_n600": 1, "mask_on9_first_and_last_n600": 2}.get(name, 0),
                             len(c.p1), "wide", 0.3)
        moved = np.sqrt(((c.p2 - clean.p2) ** 2).sum(axis=1))
        assert np.array_equal(moved == 0.0, c.on) and moved[~c.on].mean() > 20.0, "gross outliers under the zero bytes"
        # ... which the fit would notice: with them F is another matrix
        assert tc.vector_distance(tr.fundamental(c.p1, c.p2, None, True)[0], gold[name].F) > 1e-4
    c = by["mask_only_past_256_n600"]
    assert not c.mask[:256].any() and c.mask[256:].all()
    assert by["mask_on8_n600"].on.sum() == 8 and gold["mask_on8_n600"].sigma[2] < 1e-40
    c = by["mask_on9_first_and_last_n600"]
    assert c.on.sum() == 9 and c.on[0] and c.on[-1]
    # conditioning classes, from the 50-digit singular values
    for cls, (lo, hi) in tc.CLASSES.items():
        names = [c.name for c in tc.table("fit") if c.group == cls]
        assert len(names) == 4 * len(tc.CLASS_SCENES[cls])
        for name in names:
            s = gold[name].sigma
            assert lo <= s[1] / s[0] < hi, (name, s[1] / s[0])
            assert (s[2] / s[0] < 1e-15) == (by[name].expect["sigma"] == 0.0), (name, s[2] / s[0])
            assert s[2] < 0.6 * s[1], "the null space is one-dimensional"
    assert tc.CLASSES["well"][0] == tc.CLASSES["video"][1] and tc.CLASSES["video"][0] == tc.CLASSES["hard"][1]
    for c in tc.table("fit"):                                  # a lost or doubled point shows: ten orders above the bar
        if c.group in ("sizes", "masks") and c.on.sum() > 9:
            on = c.on.copy()
            on[np.flatnonzero(on)[len(on) // 3 % on.sum()]] = False
            assert tc.vector_distance(tr.fundamental(c.p1, c.p2, on, c.normalize)[0], gold[c.name].F) > 1e4 * tc.bar("F", c.group, "fit")
    # rank-deficient
    c = by["rank_all_points_identical"]
    assert (c.p1 == c.p1[0]).all() and (c.p2 == c.p2[0]).all()
    with np.errstate(all="ignore"):
        assert not np.isfinite(tr.hartley(c.p1[None])[0]).all()
    c = by["rank_two_of_eight_equal"]
    idx = np.flatnonzero(c.on)
    assert len(idx) == 8 and len(np.unique(np.concatenate((c.p1[idx], c.p2[idx]), axis=1), axis=0)) == 7
    sig = tr.fundamental(c.p1, c.p2, c.mask, True)[1]
    assert sig[7] < 1e-12 * sig[0] < 1e-12 * 1e3 * sig[6], "rank 7"


def test_hypothesis_cases_are_named_for():
    gold = tc.golden("hyp")
    seen = set()
    for c in tc.table("hyp"):
        n, hyp = len(c.p1), len(c.samples)
        assert c.samples.dtype == np.int32 and c.samples.min() >= 0 and c.samples.max() < n
        if c.kind == "solved":
            assert all(len(set(s.tolist())) == 8 for s in c.samples)
            s = gold[c.name].sigma
            lo = {"hyp_well": 1e-5, "hyp_video": 1e-6}[c.group]
            assert (ratio(s, 1) >= lo).all() and (ratio(s, 2) < 1e-40).all(), (c.name, ratio(s, 1).min())
        if "masks" not in c.name and c.kind == "solved":
            seen.add((hyp, n, c.normalize))
            assert (c.samples == 0).any() and (c.samples == n - 1).any()
            if n == 8:
                assert all(sorted(s.tolist()) == list(range(8)) for s in c.samples)
            if n > 8 and hyp > 1:
                assert not (c.samples == 0).any(axis=1).all() and not (c.samples == n - 1).any(axis=1).all()
            # pixels for the per-sample normalisation, Hartley-normalised populations otherwise
            assert (np.abs(c.p1.mean(axis=0)).max() < 1e-12) == (not c.normalize)
    assert {(h, n) for h, n, _ in seen} == {(h, n) for h in tc.HYPS for n in tc.POPULATIONS}
    for h in tc.HYPS:
        assert {z for a, _, z in seen if a == h} == {False, True}
    for n in tc.POPULATIONS:
        assert {z for _, a, z in seen if a == n} == {False, True}
    assert {c.group for c in tc.table("hyp") if c.kind == "solved"} == {"hyp_well", "hyp_video"}
    c = tc.by_name("hyp", "hyp_repeated_correspondence")
    assert len(set(c.samples[0].tolist())) == 7


def test_the_definition_reproduces_the_exact_masks():
    """The two mask cases: no 50-digit error of any hypothesis lies within half a per cent of the threshold, so the float64
    definition -- and every kernel within its bar -- takes each of the 65 x 200 decisions as the 50-digit values do."""
    gold = tc.golden("hyp")
    for kind in (0, 1):
        c = tc.by_name("hyp", "hyp65_n200_masks_kind%d" % kind)
        g = gold[c.name]
        thr = float(g.threshold)
        assert c.samples.shape == (65, 8) and len(c.p1) == 200 and c.expect["error_kind"] == kind
        flat = np.sort(g.errors.reshape(-1))
        k = np.searchsorted(flat, thr)
        assert flat[k] / flat[k - 1] >= 1.01 and abs(thr / np.sqrt(flat[k] * flat[k - 1]) - 1.0) < 1e-14
        for h in range(65):
            assert not ((g.errors[h] > thr / 1.00498) & (g.errors[h] < thr * 1.00498)).any(), h
        want = g.errors < thr
        assert 0.1 < want.mean() < 0.3 and len(set(want.sum(axis=1).tolist())) >= 15, "a threshold that separates"
        F, _ = tr.fundamental_samples(c.p1, c.p2, c.samples, c.normalize)
        for h in range(65):
            e = tr.f_errors(F[h], c.p1, c.p2, kind)
            assert np.array_equal(e < thr, want[h]), h
            sel = g.errors[h] > 1e-20
            assert np.abs(e[sel] / g.errors[h][sel] - 1.0).max() < 1e-5, h


def test_dlt_cases_are_named_for():
    by, gold = {c.name: c for c in tc.table("dlt")}, tc.golden("dlt")
    assert [len(by["shared_n%d" % n].x1) for n in tc.DLT_SIZES] == list(tc.DLT_SIZES)
    for n in tc.DLT_SIZES:
        assert by["shared_n%d" % n].C1.shape == (3, 4)
    for n in tc.DLT_PER_POINT:
        c = by["per_point_n%d" % n]
        assert c.C1.shape == (n, 3, 4) and len(np.unique(c.C1.reshape(n, 12), axis=0)) == n
        if n > 1:        # an indexing slip shows: with its neighbour's camera a point lands elsewhere
            X = tr.dlt(c.x1, c.x2, np.roll(c.C1, 1, axis=0), c.C2)[1]
            assert np.median(tc.point_distance(X, gold[c.name].X)) > 1e-3
    gap = {}
    for name in tc.PARALLAX:
        c, s = by["parallax_" + name], gold["parallax_" + name].sigma
        depth = np.sqrt((c.X_true ** 2).sum(axis=1))
        assert np.all(np.abs(c.baseline / depth / float(name) - 1.0) < 0.3)
        gap[name] = float(np.sqrt(np.median(((s[:, 2] - s[:, 3]) / s[:, 0]) ** 2)))
    print("parallax classes, median (sigma3 - sigma4) / sigma1:", gap)
    assert [name for name, _, _ in tc.PARALLAX_GAPS] == list(tc.PARALLAX)
    for k, (name, lo, hi) in enumerate(tc.PARALLAX_GAPS):
        assert lo <= gap[name] < hi, name
        assert k == 0 or hi <= tc.PARALLAX_GAPS[k - 1][1], "the classes do not overlap"
    for name, d in (("1e4", 1e4), ("1e8", 1e8)):
        c = by["far_depth_" + name]
        assert c.compare == "direction" and 0.7 * d < c.X_true[:, 2].min() and c.X_true[:, 2].max() < 1.3 * d
    assert all(c.compare == "point" for c in tc.table("dlt") if c.group != "dlt_far")
    c = by["world_offset_1e3"]
    assert 900.0 < np.sqrt((c.X_true ** 2).sum(axis=1)).min() and np.abs(c.C1[:, 3]).max() > 1e5 * np.abs(c.C1[:, :3]).min()
    scale = np.sqrt((tr.dlt_rows(c.x1, c.x2, c.C1, c.C2) ** 2).sum(axis=1))
    assert (scale[:, 3] > 3e2 * scale[:, :3].max(axis=1)).all(), "column scales"
    c = by["point_behind_both"]
    depth = lambda C, X: C[2, :3] @ X + C[2, 3]
    assert depth(c.C1, c.X_true[2]) < 0.0 and depth(c.C2, c.X_true[2]) < 0.0
    assert tc.point_distance(gold[c.name].X[2:3], c.X_true[2:3])[0] < 1e-9, "the DLT puts it back there"
    c = by["image_corners"]
    assert tuple(c.x1[0]) == (0.0, 0.0) and tuple(c.x2[1]) == tc.IMAGE
    for name in ("shared_n257", "noise_0p4_px", "per_point_n257"):
        s = gold[name].sigma
        assert (s[:, 3] / s[:, 0]).min() > 1e-9, "noise: sigma4 != 0"
    c = by["rank_same_camera_same_pixel"]
    assert np.array_equal(c.C1, c.C2) and np.array_equal(c.x1, c.x2)
    sig = tr.dlt(c.x1, c.x2, c.C1, c.C2)[2]
    assert (sig[:, 2] < 1e-12 * sig[:, 0]).all(), "a two-dimensional null space"


def test_golden_refuses_other_inputs(monkeypatch):
    c = tc.by_name("dlt", "shared_n1")
    real = tc.sha256
    monkeypatch.setattr(tc, "sha256", lambda case: "0" * 64 if case is c else real(case))
    tc.golden.cache_clear()
    try:
        with pytest.raises(AssertionError):
            tc.golden("dlt")
    finally:
        tc.golden.cache_clear()
