"""Writes tests/golden/refine_cases.npz: the pose refinement's rule (include/vo_hip.h) evaluated with mpmath at 50 digits
on every case of tests/refine_cases.py.  Per case (rounded to double; NaN where the case's kind has none):

  sha256            of the case's input bytes -- the inputs themselves are regenerated from seeds, not stored
  cost0             the exact cost of the active points at the start (inf where a point has p_z = 0)
  step1             the pose (R row-major, t) after one exact Gauss-Newton step from the start      (solved, large)
  final, final_cost the pose the iteration ends at and its cost: Gauss-Newton from the start in 50 digits, a trial accepted
                    iff its cost does not grow, until the step is below 1e-40 (at most the case's max_iter steps where that is
                    below 20) -- the minimiser of the basin unless a trial is rejected or max_iter ends it     (solved)
  final_iterations  accepted steps of that iteration

    python tools/make_refine_golden.py            (about two minutes)"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_cases  # noqa: E402

mp.mp.dps = 50
STEP_END = mp.mpf(10) ** -40
MAX_STEPS = 400


def points(c):
    on = np.flatnonzero(c.on)
    return [tuple(mp.mpf(float(v)) for v in (*c.X[i], *c.x[i])) for i in on]


def sums(pts, K, R, t, want_system=True):
    """(A, g, cost) in 50 digits; cost = +inf when a point has p_z = 0."""
    fx, fy, cx, cy = K
    A = [[mp.mpf(0)] * 6 for _ in range(6)]
    g = [mp.mpf(0)] * 6
    cost = mp.mpf(0)
    for X, Y, Z, u, v in pts:
        px = R[0] * X + R[1] * Y + R[2] * Z + t[0]
        py = R[3] * X + R[4] * Y + R[5] * Z + t[1]
        pz = R[6] * X + R[7] * Y + R[8] * Z + t[2]
        if pz == 0:
            return None, None, mp.inf
        iz = 1 / pz
        eu = u - (fx * px * iz + cx)
        ev = v - (fy * py * iz + cy)
        cost += eu * eu + ev * ev
        if not want_system:
            continue
        a, c = fx * iz, -fx * px * iz * iz
        b, d = fy * iz, -fy * py * iz * iz
        J0 = (a, 0, c, c * py, a * pz - c * px, -a * py)
        J1 = (0, b, d, d * py - b * pz, -d * px, b * px)
        for i in range(6):
            g[i] += J0[i] * eu + J1[i] * ev
            for j in range(i, 6):
                A[i][j] += J0[i] * J0[j] + J1[i] * J1[j]
    for i in range(6):
        for j in range(i):
            A[i][j] = A[j][i]
    return A, g, cost


def increment(R, t, d):
    w = d[3:]
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    ca, cb = (mp.mpf(1), mp.mpf(1) / 2) if th == 0 else (mp.sin(th) / th, (1 - mp.cos(th)) / th ** 2)
    Wx = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = mp.eye(3) + ca * Wx + cb * (Wx * Wx)
    Rn = E * mp.matrix([R[0:3], R[3:6], R[6:9]])
    tn = E * mp.matrix(t) + mp.matrix(d[:3])
    return [Rn[i, j] for i in range(3) for j in range(3)], [tn[i] for i in range(3)]


def norm(v):
    return mp.sqrt(sum(q * q for q in v))


def run(c):
    nan12 = np.full(12, np.nan)
    out = dict(cost0=np.nan, step1=nan12, final=nan12, final_cost=np.nan, final_iterations=-1)
    pts = points(c)
    K = [mp.mpf(float(c.K[0, 0])), mp.mpf(float(c.K[1, 1])), mp.mpf(float(c.K[0, 2])), mp.mpf(float(c.K[1, 2]))]
    R = [mp.mpf(float(v)) for v in c.R0.reshape(9)]
    t = [mp.mpf(float(v)) for v in c.t0]
    solve = c.kind in ("solved", "large")
    A, g, cost = sums(pts, K, R, t, want_system=solve)
    out["cost0"] = float(cost)
    if not solve:
        return out
    max_steps = c.max_iter if c.max_iter < 20 else MAX_STEPS
    it = 0
    while True:
        d = list(mp.lu_solve(mp.matrix(A), mp.matrix(g)))
        Rn, tn = increment(R, t, d)
        if it == 0:                                   # (the single step is stored for max_iter = 0 as well)
            out["step1"] = np.array([float(v) for v in Rn + tn])
        if c.kind == "large" or it >= max_steps or norm(d) <= STEP_END * (1 + norm(tn)):
            break
        An, gn, cost_new = sums(pts, K, Rn, tn)
        if not cost_new <= cost:
            break
        R, t, A, g, cost = Rn, tn, An, gn, cost_new
        it += 1
    assert it < MAX_STEPS, c.name
    if c.kind == "solved":
        out.update(final=np.array([float(v) for v in R + t]), final_cost=float(cost), final_iterations=it)
    return out


def main():
    arrays = {}
    for c in refine_cases.table():
        if c.kind == "property":
            continue
        r = run(c)
        arrays[c.name + "/sha256"] = np.array(refine_cases.sha256(c))
        for k, v in r.items():
            arrays[c.name + "/" + k] = np.asarray(v)
        print("%-28s cost0 %.17g  final cost %.17g after %d steps" % (c.name, r["cost0"], r["final_cost"], r["final_iterations"]),
              flush=True)
    np.savez_compressed(refine_cases.GOLDEN, **arrays)
    print("wrote", refine_cases.GOLDEN, os.path.getsize(refine_cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
