"""The P3P case table (tests/golden/p3p_cases.npz, written by tools/make_p3p_cases.py) and the three criteria a
solver's output is held to against the table's reference solution sets.  Shared by the host tests (the C oracle)
and the GPU tests (the kernel's own output), so that the two cannot move together unnoticed."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p3p_cases.npz")
FAMILIES = ("generic", "outlier", "symmetric", "biquadratic", "rejects", "edges")

BACKWARD_PX = 1e-3        # the three solved points reproject within this (max-abs, px)
ORTHO = 1e-12             # R^T R = I and det R = +1 to this
SELECT = 1e-6             # well separated: the reference's best pose, to this
MEMBER = 1e-4             # otherwise: some pose of the reference's set, to this
ROOT_GAP = 1e-3           # well separated: positive v roots pairwise further apart than this (relative) ...
E4_GAP = 1e-6             # ... and best / second-best fourth-point errors further apart than this (px^2)
GENERIC_UNSEPARATED_MAX = 0.05

_table = None


def table():
    global _table
    if _table is None:
        z = np.load(PATH)
        _table = {k: z[k] for k in z.files}
        _table["R"] = rot_of(_table["q"]) * (np.arange(4)[None, :] < _table["n_sol"][:, None])[:, :, None, None]
        for a in _table.values():
            a.setflags(write=False)
    return _table


def rot_of(q):
    """rotations (..., 3, 3) of the unit quaternions (w, x, y, z) the table stores its poses' rotations as"""
    w, x, y, z = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def name(tab, i):
    return "%s/%s (k=%d, row %d)" % (tab["family"][i], tab["sub"][i], tab["k"][i], i)


def pack(tab, Kid):
    """All cases of one intrinsics as one hypothesis batch: (rows, K, X (4n, 3), x (4n, 2), samples (n, 4))."""
    rows = np.flatnonzero(tab["K_index"] == Kid)
    X = tab["X"][rows].reshape(-1, 3).copy()
    x = tab["x"][rows].reshape(-1, 2).copy()
    samples = np.arange(4 * len(rows), dtype=np.int32).reshape(-1, 4)
    return rows, tab["K_table"][Kid].copy(), X, x, samples


def well_separated(tab):
    n = len(tab["n_sol"])
    sep = np.ones(n, bool)
    for i in range(n):
        v = tab["v"][i, :tab["n_v"][i]]
        for a in range(len(v)):
            for b in range(a + 1, len(v)):
                if not abs(v[a] - v[b]) > ROOT_GAP * max(v[a], v[b]):
                    sep[i] = False
        if tab["n_sol"][i] >= 2 and not tab["e4"][i, 1] - tab["e4"][i, 0] > E4_GAP:
            sep[i] = False
    return sep


def measure(tab, valid, R, t):
    """Per case, for a solver's (valid, R, t) in table order: ortho (departure of R from a rotation), be (max-abs
    reprojection of the three solved points, px), best / member (distance to the reference's best pose / to the
    nearest pose of its set: max of max|dR| and |dt| / max(1, |t|)).  NaN where there is nothing to measure."""
    n = len(valid)
    out = {k: np.full(n, np.nan) for k in ("ortho", "be", "best", "member")}
    for i in np.flatnonzero(np.asarray(valid) & 1):
        K = tab["K_table"][tab["K_index"][i]]
        Ri, ti = R[i], t[i]
        out["ortho"][i] = max(np.abs(Ri @ Ri.T - np.eye(3)).max(), abs(np.linalg.det(Ri) - 1.0))
        Xc = tab["X"][i, :3] @ Ri.T + ti
        p = np.stack([Xc[:, 0] / Xc[:, 2] * K[0, 0] + K[0, 2], Xc[:, 1] / Xc[:, 2] * K[1, 1] + K[1, 2]], axis=1)
        out["be"][i] = np.abs(p - tab["x"][i, :3]).max()
        d = [max(np.abs(Ri - tab["R"][i, j]).max(),
                 np.linalg.norm(ti - tab["t"][i, j]) / max(1.0, np.linalg.norm(tab["t"][i, j])))
             for j in range(tab["n_sol"][i])]
        if d:
            out["best"][i], out["member"][i] = d[0], min(d)
    return out


def check_validity(tab, valid):
    want = tab["n_sol"] > 0
    bad = np.flatnonzero((want != ((np.asarray(valid) & 1) != 0)) & ~tab["conditioning"])
    assert bad.size == 0, "%d cases: a pose where the reference has none, or none where it has one; first: %s (reference %d)" % (
        bad.size, name(tab, bad[0]), tab["n_sol"][bad[0]])


def check_backward(tab, m):
    """-> {family: max backward error in px}"""
    ok = ~np.isnan(m["be"])
    bad = np.flatnonzero(ok & ~(m["ortho"] <= ORTHO))
    assert bad.size == 0, "R is no rotation to %g: %s (%.3g)" % (ORTHO, name(tab, bad[0]), m["ortho"][bad[0]])
    worst = {}
    for f in FAMILIES:
        sel = ok & (tab["family"] == f)
        if sel.any():
            i = np.flatnonzero(sel)[np.argmax(m["be"][sel])]
            worst[f] = float(m["be"][i])
            print("backward error, %-12s max %.3g px at %s" % (f, m["be"][i], name(tab, i)))
    bad = np.flatnonzero(ok & ~(m["be"] <= BACKWARD_PX))
    assert bad.size == 0, "%d poses reproject their own three points more than %g px off; first: %s (%.3g px)" % (
        bad.size, BACKWARD_PX, name(tab, bad[0]), m["be"][bad[0]])
    return worst


def check_selection(tab, m):
    """-> share of the generic family outside `well separated`"""
    sep = well_separated(tab)
    gen = tab["family"] == "generic"
    share = float((~sep[gen]).mean())
    print("generic cases outside 'well separated': %d of %d (%.2f %%)" % ((~sep[gen]).sum(), gen.sum(), 100 * share))
    assert share <= GENERIC_UNSEPARATED_MAX
    have = ~np.isnan(m["best"])
    print("selection: worst distance to the best pose where well separated %.3g, to the set elsewhere %.3g" % (
        np.nanmax(np.where(have & sep, m["best"], np.nan)), np.nanmax(np.where(have & ~sep, m["member"], np.nan))))
    bad = np.flatnonzero(have & sep & ~(m["best"] <= SELECT))
    assert bad.size == 0, "%d well separated cases do not return the reference's best pose; first: %s (%.3g, nearest of the set %.3g)" % (
        bad.size, name(tab, bad[0]), m["best"][bad[0]], m["member"][bad[0]])
    bad = np.flatnonzero(have & ~sep & ~(m["member"] <= MEMBER))
    assert bad.size == 0, "%d poses are no member of the reference's set; first: %s (%.3g)" % (
        bad.size, name(tab, bad[0]), m["member"][bad[0]])
    return share


def check_demanded(tab, m):
    """Rows marked `demand_best` (the equilateral sweeps, but for the three deltas at which rounding loses the double
    root) are mostly not `well separated` -- two roots v coincide or nearly so -- yet the reference's best pose is
    demanded to 1e-6: at those roots the solver's vanishing-denominator step has to pick the right one of two roots u,
    by the residual (delta = 1e-3, 1e-4), or one per copy of the double root (delta <= 1e-5), once the larger
    (equi_d*) and once the smaller (equi_alt_d*).  A step that always takes the same root, or the same root for both copies, fails here."""
    rows = np.flatnonzero(tab["demand_best"])
    assert rows.size >= 14
    assert not np.isnan(m["best"][rows]).any(), "no pose for " + name(tab, rows[np.isnan(m["best"][rows])][0])
    bad = rows[~(m["best"][rows] <= SELECT)]
    assert bad.size == 0, "%d demanded cases miss the reference's best pose; first: %s (%.3g, nearest of the set %.3g)" % (
        bad.size, name(tab, bad[0]), m["best"][bad[0]], m["member"][bad[0]])
