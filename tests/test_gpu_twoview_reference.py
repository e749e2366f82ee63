"""vo_fundamental_fit, vo_fundamental_hypotheses (csrc/bootstrap.hip) and vo_triangulate_dlt (csrc/dlt.hip) against the
rules of include/vo_hip.h: the 50-digit values of tests/golden/twoview_cases.npz on the case tables of
tests/twoview_cases.py.

Bars (twoview_cases.bar): per group of a table, 100 times the distance measured there between the float64 definition
(tests/twoview_reference.py; the fit over 21 point orders) and the 50-digit value (tests/test_twoview_reference_host.py),
never looser than what the suite held the kernels to against the LAPACK oracles: 1e-9 for the fit, 1e-7 for a hypothesis,
1e-8 for the DLT.  For the fit that is 4e-13 (sizes), 1e-13 (masks, well), 1.5e-11 (video) and 2.5e-10 (hard: a wall, where
sigma8 / sigma1 of Q is below 1e-5).  Every test prints the largest distance it saw before it asserts."""
import ctypes as C

import numpy as np
import pytest

import twoview_cases as tc
from vo import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def bits(*values):
    return b"".join(np.ascontiguousarray(v).tobytes() for v in values)


def fit(ctx, c, p1=None, p2=None, mask="case"):
    return ctx.fundamental_fit(c.p1 if p1 is None else p1, c.p2 if p2 is None else p2,
                               c.mask if isinstance(mask, str) else mask, normalize=c.normalize)


def fit_dev(ctx, c):
    """vo_fundamental_fit_dev, bound by hand: (F, n_used)."""
    fn = _native.load().vo_fundamental_fit_dev
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    d_p1, d_p2 = ctx.to_device(np.ascontiguousarray(c.p1)), ctx.to_device(np.ascontiguousarray(c.p2))
    d_m = None if c.mask is None else ctx.to_device(np.ascontiguousarray(c.mask))
    d_F, d_n = ctx.to_device(np.full(10, -7.0)), ctx.to_device(np.full(2, -7, np.int32))
    try:
        assert fn(ctx._h, d_p1, d_p2, len(c.p1), d_m, int(c.normalize), d_F, d_n) == 0
        ctx.sync()
        F, n = ctx.download(d_F, (10,), np.float64), ctx.download(d_n, (2,), np.int32)
    finally:
        for p in (d_p1, d_p2, d_F, d_n) + (() if d_m is None else (d_m,)):
            ctx.free(p)
    assert F[9] == -7.0 and n[1] == -7, "nine doubles and one count are written"
    return F[:9].reshape(3, 3), int(n[0])


@pytest.mark.parametrize("group", ["sizes", "masks", "well", "video", "hard"])
def test_fit_matches_the_50_digit_values(ctx, group):
    """Every solved case of the group; also the device-resident form, bit for bit, and its count of used points."""
    gold, worst, failed = tc.golden("fit"), (0.0, ""), []
    for c in tc.table("fit"):
        if c.group == group:
            F = fit(ctx, c)
            d = tc.vector_distance(F, gold[c.name].F)
            print("%-32s %.3g" % (c.name, d))
            worst = max(worst, (d, c.name))
            if not d <= tc.bar("F", group, "fit"):
                failed.append((c.name, d))
            Fd, n_used = fit_dev(ctx, c)
            assert bits(Fd) == bits(F) and n_used == int(c.on.sum()), c.name
    print("fit, %s: largest distance %.3g (%s), bar %.3g" % (group, *worst, tc.bar("F", group, "fit")))
    assert not failed, (tc.bar("F", group, "fit"), failed)


def test_fit_masked_off_points_cannot_leak(ctx):
    """NaN, 1e300 and inf under the off bytes change no bit of F; every non-zero byte means the same; and the mask means
    what leaving the points out means, to the bar."""
    gold = tc.golden("fit")
    for c in tc.table("fit"):
        if c.group == "masks":
            want = bits(fit(ctx, c))
            for poison in (np.nan, 1e300, np.inf):
                p1, p2 = c.p1.copy(), c.p2.copy()
                p1[~c.on], p2[~c.on] = poison, -poison
                assert bits(fit(ctx, c, p1, p2)) == want, (c.name, poison)
            for byte in (1, 255):
                assert bits(fit(ctx, c, mask=np.where(c.on, byte, 0).astype(np.uint8))) == want, (c.name, byte)
            d = tc.vector_distance(fit(ctx, c, c.p1[c.on], c.p2[c.on], mask=None), gold[c.name].F)
            assert d <= tc.bar("F", "masks", "fit"), (c.name, d)


def test_fit_rank_deficient_cases_keep_their_invariants(ctx):
    """The call returns, the count is right, and F is not finite or has no residual on an active point above what removing
    the smallest singular triplet can leave: |p2^T F p1| <= sigma3 |p1| |p2| <= |F| |p1| |p2| / sqrt(2) in the
    normalised frame (|F|^2 = sigma1^2 + sigma2^2 >= 2 sigma3^2 after the projection)."""
    for c in tc.table("fit"):
        if c.kind == "property":
            F, n_used = fit_dev(ctx, c)
            assert n_used == int(c.on.sum()), c.name
            print(c.name, "finite" if np.isfinite(F).all() else "not finite")
            if np.isfinite(F).all():
                assert not (c.p1[c.on] == c.p1[c.on][0]).all(), "a finite F from a normalisation that is not finite"
                a, b = tc.prenormalise(c.p1[c.on]), tc.prenormalise(c.p2[c.on])
                ah, bh = np.concatenate((a, np.ones((len(a), 1))), axis=1), np.concatenate((b, np.ones((len(b), 1))), axis=1)
                A1, A2 = affine(c.p1[c.on], a), affine(c.p2[c.on], b)          # pixel -> normalised, 3x3
                Fn = np.linalg.inv(A2).T @ F @ np.linalg.inv(A1)
                res = np.abs(np.einsum("ki,ij,kj->k", bh, Fn, ah))
                bound = np.sqrt((Fn * Fn).sum() / 2.0) * np.sqrt((ah * ah).sum(axis=1) * (bh * bh).sum(axis=1))
                assert (res <= bound * (1.0 + 1e-9)).all(), (c.name, res / bound)


def affine(pixels, normalised):
    """The T of x' = s x + tx, y' = s y + ty from two of the points (they are not all equal where this is called)."""
    k = int(np.argmax(np.abs(pixels[:, 0] - pixels[0, 0])))
    s = (normalised[k, 0] - normalised[0, 0]) / (pixels[k, 0] - pixels[0, 0])
    return np.array([[s, 0.0, normalised[0, 0] - s * pixels[0, 0]], [0.0, s, normalised[0, 1] - s * pixels[0, 1]], [0.0, 0.0, 1.0]])


def test_hypotheses_match_the_50_digit_values(ctx):
    """Every sample's F of every solved case; the counts are the mask rows' sums."""
    gold, worst, failed = tc.golden("hyp"), {}, []
    for c in tc.table("hyp"):
        if c.kind == "solved":
            F, counts, masks = ctx.fundamental_hypotheses(c.p1, c.p2, c.samples, 1e-4, c.normalize, 0, want_masks=True)
            assert np.array_equal(counts, masks.sum(axis=1)), c.name
            d = max(tc.vector_distance(F[h], gold[c.name].F[h]) for h in range(len(c.samples)))
            print("%-36s %.3g" % (c.name, d))
            worst[c.group] = max(worst.get(c.group, (0.0, "")), (d, c.name))
            if not d <= tc.bar("F", c.group, "hyp"):
                failed.append((c.name, d))
    for g, w in worst.items():
        print("hypotheses, %s: largest distance %.3g (%s), bar %.3g" % (g, *w, tc.bar("F", g, "hyp")))
    assert not failed, failed


@pytest.mark.parametrize("kind", [0, 1])
def test_hypothesis_counts_and_masks_exactly(ctx, kind):
    """65 hypotheses over 200 correspondences at a threshold no 50-digit error comes within half a per cent of: every
    decision is the 50-digit one, bit for bit."""
    c = tc.by_name("hyp", "hyp65_n200_masks_kind%d" % kind)
    g = tc.golden("hyp")[c.name]
    want = g.errors < float(g.threshold)
    F, counts, masks = ctx.fundamental_hypotheses(c.p1, c.p2, c.samples, float(g.threshold), c.normalize, kind, want_masks=True)
    print("decisions that differ:", int((masks != want).sum()))
    assert np.array_equal(masks, want) and np.array_equal(counts, want.sum(axis=1))


def test_hypothesis_of_a_repeated_correspondence(ctx):
    """Rank 7: F is finite or NaN; a NaN F scores no inlier, a finite one counts its mask row."""
    c = tc.by_name("hyp", "hyp_repeated_correspondence")
    for kind, thr in ((0, 1e-4), (1, 1.0)):
        F, counts, masks = ctx.fundamental_hypotheses(c.p1, c.p2, c.samples, thr, c.normalize, kind, want_masks=True)
        print("kind", kind, "finite" if np.isfinite(F).all() else "not finite", counts)
        assert np.isfinite(F[0]).all() or np.isnan(F[0]).any()
        assert counts[0] == masks[0].sum() and 0 <= counts[0] <= len(c.p1)
        if not np.isfinite(F[0]).all():
            assert counts[0] == 0


def test_dlt_matches_the_50_digit_values(ctx):
    """Every solved case: the homogeneous direction, and outside the far group the point."""
    gold, worst, failed = tc.golden("dlt"), {}, []
    for c in tc.table("dlt"):
        if c.kind == "solved":
            X, g = ctx.triangulate_dlt(c.x1, c.x2, c.C1, c.C2), gold[c.name]
            Xh = np.concatenate((X, np.ones((len(X), 1))), axis=1)
            d = {"v": max(tc.vector_distance(Xh[i], g.v[i]) for i in range(len(X)))}
            if c.compare == "point":
                d["X"] = float(tc.point_distance(X, g.X).max())
            print("%-24s" % c.name, "  ".join("%s %.3g" % kv for kv in d.items()))
            for q, v in d.items():
                worst[(c.group, q)] = max(worst.get((c.group, q), (0.0, "")), (v, c.name))
                if not v <= tc.bar(q, c.group, "dlt"):
                    failed.append((c.name, q, v, tc.bar(q, c.group, "dlt")))
    for (g, q), w in worst.items():
        print("DLT, %s %s: largest distance %.3g (%s), bar %.3g" % (g, q, *w, tc.bar(q, g, "dlt")))
    assert not failed, failed


def test_dlt_of_a_two_dimensional_null_space_returns(ctx):
    c = tc.by_name("dlt", "rank_same_camera_same_pixel")
    X = ctx.triangulate_dlt(c.x1, c.x2, c.C1, c.C2)
    print(X)
    assert X.shape == (len(c.x1), 3)
