"""The five-point case table (tests/golden/essential5_cases.npz, written by tools/make_essential5_golden.py) and the
comparisons a solver's output is held to against its 50-digit solution sets.  Shared by the host test (the float64
definition, tests/essential5_reference.py) and the GPU test (the kernel's own output), so that the two cannot move
together unnoticed.

How the bars are set.  The float64 definition and the kernel are float64 solvers of the same conditioning; the host test
measures the definition's worst figure per family against the 50-digit sets (DEFINITION below records them), and the
kernel's bar is 100 times that figure -- two orders of magnitude cover another elimination order -- with a floor."""
import math
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "essential5_cases.npz")
SEPARATED = ("generic", "forward", "sideways", "planar", "pixels", "few", "many")      # redrawn until both gaps > ROOT_GAP
FAMILIES = SEPARATED + ("near-rotation", "rejects")
ROOT_GAP = 1e-3           # the constant of tests/p3p_cases.py
SET_FLOOR = 1e-9          # the floor of the solution-set bar
BACK_FLOOR = 1e-12        # the floor of the backward bars: 4500 ulp of a unit-norm matrix's entries
MARGIN = 100.0

# The float64 definition's worst figures per family on the CPU (tests/test_essential5_host.py measures them again on every
# run and fails when one is exceeded): the set distance to the 50-digit sets, and the backward figures
# (|norm - 1|, |x^2^T E x^1| on unit-scaled points, |det E|, ||2EE^TE - tr(EE^T)E||) over every returned matrix.
DEFINITION = {
    "generic": dict(set=1.2e-6, norm=2.3e-16, epipolar=3.7e-16, det=8.4e-8, trace=3.5e-7),
    "forward": dict(set=9.6e-9, norm=2.3e-16, epipolar=1.6e-16, det=2.7e-10, trace=1.2e-9),
    "sideways": dict(set=5.3e-11, norm=2.3e-16, epipolar=2.3e-16, det=6.4e-12, trace=5.0e-11),
    "planar": dict(set=7.4e-5, norm=2.3e-16, epipolar=1.7e-16, det=7.4e-8, trace=2.0e-6),
    "pixels": dict(set=3.2e-5, norm=2.3e-16, epipolar=1.7e-16, det=2.4e-7, trace=1.5e-6),
    "few": dict(set=4.5e-11, norm=2.3e-16, epipolar=1.2e-16, det=4.2e-12, trace=1.7e-11),
    "many": dict(set=1.3e-12, norm=2.3e-16, epipolar=2.4e-16, det=3.0e-13, trace=1.4e-12),
    # only the backward checks apply: the translation is 1e-4 of the depth and the set itself is ill-determined
    "near-rotation": dict(set=None, norm=2.3e-16, epipolar=1.7e-16, det=8.9e-4, trace=4.1e-3),
    # the definition returns no solution for any of them
    "rejects": dict(set=None, norm=0.0, epipolar=0.0, det=0.0, trace=0.0),
}
# the ground truth is a member of the 50-digit set of its float64 inputs: a coordinate is rounded by 2^-53 (1.1e-16), a
# root gap of ROOT_GAP amplifies that by at most 1 / ROOT_GAP^2 in the separated families; in near-rotation the parallax
# that determines E is 1e-4 of a coordinate, so the rounding is 1.1e-12 of it, times up to 1e4 for roots not held apart
MEMBER = {True: 1.1e-16 / ROOT_GAP ** 2, False: 1.1e-12 * 1e4}
EXEMPT_REL = 1e-9         # a scoring decision whose error lies within this (relative) of the threshold is not compared
THRESHOLDS = {0: 2e-6, 1: 1.0}          # the scoring tests' thresholds: (x^2^T E x^1)^2 of about a pixel; 1 px^2
EXEMPT_SHARE = 1e-4       # ... and at most this share of all (solution, point) decisions may be


def set_bar(family):
    return max(SET_FLOOR, MARGIN * DEFINITION[family]["set"])


def backward_bars(family):
    d = DEFINITION[family]
    return tuple(max(BACK_FLOOR, MARGIN * d[k]) for k in ("norm", "epipolar", "det", "trace"))


_table = None


def table():
    global _table
    if _table is None:
        z = np.load(PATH)
        _table = {k: z[k] for k in z.files}
        _table["family"] = np.array([f.decode() for f in _table["family"]])
        _table["sub"] = np.array([f.decode() for f in _table["sub"]])
        for a in _table.values():
            a.setflags(write=False)
    return _table


def name(tab, i):
    return "%s/%s (row %d)" % (tab["family"][i], tab["sub"][i], i)


def pack(tab, rows):
    """The cases `rows` (all of one camera pair) as one hypothesis batch: (x1 (5n, 2), x2 (5n, 2), samples (n, 5))."""
    x1 = tab["x1"][rows].reshape(-1, 2).copy()
    x2 = tab["x2"][rows].reshape(-1, 2).copy()
    return x1, x2, np.arange(5 * len(rows), dtype=np.int32).reshape(-1, 5)


def camera_groups(tab):
    """lists of rows that share (K1, K2)"""
    groups = {}
    for i in range(len(tab["family"])):
        groups.setdefault((tab["K1"][i].tobytes(), tab["K2"][i].tobytes()), []).append(i)
    return [np.array(v) for v in groups.values()]


# ---- 50 digits ----

def _mp():
    import mpmath as mp
    mp.mp.dps = max(mp.mp.dps, 50)       # (the generator works at 100)
    return mp


def mp_normalise(K, x):
    """x^ = K^-1 (x, y, 1) of float64 pixels through the EXACT inverse of the float64 pinhole K: list of [x^, y^, 1]."""
    mp = _mp()
    fx, fy, cx, cy = (mp.mpf(float(K[0][0])), mp.mpf(float(K[1][1])), mp.mpf(float(K[0][2])), mp.mpf(float(K[1][2])))
    return [[(mp.mpf(float(p[0])) - cx) / fx, (mp.mpf(float(p[1])) - cy) / fy, mp.mpf(1)] for p in x]


def mp_canonical(E):
    """unit Frobenius norm, the entry of largest magnitude positive (the first in row-major order on ties)"""
    mp = _mp()
    n = mp.sqrt(sum(E[r, c] ** 2 for r in range(3) for c in range(3)))
    E = E / n
    big = E[0, 0]
    for r in range(3):
        for c in range(3):
            if abs(E[r, c]) > abs(big):
                big = E[r, c]
    return -E if big < 0 else E


def mp_matrix_of(strings):
    """the mp.matrix of nine decimal strings (row-major)"""
    mp = _mp()
    E = mp.matrix(3, 3)
    for k in range(9):
        E[k // 3, k % 3] = mp.mpf(strings[k].decode())
    return E


def mp_residuals(E, h1, h2):
    """(max |x^2^T E x^1| over the five points, |det E|, max |2 E E^T E - tr(E E^T) E|) at 50 digits"""
    mp = _mp()
    epi = max(abs(sum(h2[k][b] * E[b, a] * h1[k][a] for a in range(3) for b in range(3))) for k in range(5))
    G = E * E.T
    C = 2 * G * E - (G[0, 0] + G[1, 1] + G[2, 2]) * E
    return epi, abs(mp.det(E)), max(abs(C[r, c]) for r in range(3) for c in range(3))


# ---- scenes of many correspondences (the scoring, loop and planar tests) ----

def kitti_camera():
    g = np.load(os.path.join(os.path.dirname(PATH), "kitti_harris.npz"))
    return np.ascontiguousarray(g["calib_P0"][:, :3], dtype=np.float64)


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(n, seed, outliers=0.3, noise_px=0.3, planar=False):
    """n correspondences of a forward-and-sideways motion through the KITTI camera (1226 x 370): (x1, x2 (n, 2), K, R, t,
    the gross-outlier flags).  planar: every point on one plane (a tilted wall ahead)."""
    rng = np.random.default_rng(seed)
    K = kitti_camera()
    R = _rodrigues(np.deg2rad(2.0) * np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1]))
    t = np.array([0.25, -0.05, -1.0])
    rays = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.24, 0.24, n), np.ones(n)], axis=1)
    if planar:
        nrm = np.array([0.3, 0.1, 1.0]) / np.linalg.norm([0.3, 0.1, 1.0])
        X = rays * (12.0 / (rays @ nrm))[:, None]
    else:
        X = rays * rng.uniform(5.0, 40.0, n)[:, None]
    x1 = X @ K.T
    x2 = (X @ R.T + t) @ K.T
    x1, x2 = x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:]
    x1 = x1 + rng.normal(0.0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0.0, noise_px, x2.shape)
    bad = rng.random(n) < outliers
    x2[bad] = np.stack([rng.uniform(0, 1226, bad.sum()), rng.uniform(0, 370, bad.sum())], axis=1)
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2), K, R, t, bad


def pose_errors(M, R, t):
    """(rotation error in degrees, cosine between the translation directions) of M = [R' | t'] against (R, t)"""
    M = np.asarray(M).reshape(3, 4)
    c = (np.trace(M[:, :3].T @ R) - 1.0) / 2.0
    tt = M[:, 3]
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(tt @ t / (np.linalg.norm(tt) * np.linalg.norm(t)))


def expected_scores(E, n_sol, x1, x2, K1, K2, kind, thr):
    """The NumPy formula on given matrices E (Hyp, 10, 3, 3): (counts (Hyp, 10), masks (Hyp, 10, N) bool, near (same shape):
    the decisions within EXEMPT_REL of the threshold)."""
    import essential5_reference as ref
    F = ref.fundamental_from_essential(E, ref.pinhole_inverse(K1), ref.pinhole_inverse(K2))
    H, N = len(E), len(x1)
    masks = np.zeros((H, 10, N), bool)
    near = np.zeros((H, 10, N), bool)
    for h in range(H):
        for s in range(int(n_sol[h])):
            e = ref.f_error(F[h, s], x1, x2, kind)
            masks[h, s] = e < thr
            near[h, s] = np.abs(e - thr) <= EXEMPT_REL * thr
    return masks.sum(axis=2).astype(np.int32), masks, near


def replay(valid, counts, n, state):
    """ransac.py:90-121 over one batch, in Python.  state: dict(n_done, n_iterations, best_count, max_iterations,
    confidence, s); returns (consumed, finished, the batch index of the model accepted last or -1)."""
    b, idx = 0, -1
    while state["n_done"] < state["n_iterations"]:
        if b >= len(valid):
            return b, False, idx
        cur = b
        b += 1
        if not valid[cur]:
            continue
        if counts[cur] > state["best_count"]:
            state["best_count"] = int(counts[cur])
            idx = cur
            o = min(max(1.0 - counts[cur] / n, 0.01), 0.99)
            k = int(math.ceil(math.log(1.0 - state["confidence"]) / math.log(1.0 - math.pow(1.0 - o, state["s"]))))
            state["n_iterations"] = min(k, state["max_iterations"])
        state["n_done"] += 1
    return b, True, idx
