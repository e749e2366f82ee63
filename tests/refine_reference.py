"""The definition the pose refinement is pinned to.  TEST INFRASTRUCTURE.

The rule of include/vo_hip.h ("pose refinement") stated in float64 NumPy, vectorised over points; both kernels of
csrc/refine.hip (tests/test_gpu_refine_reference.py, tests/test_gpu_pipeline.py) and the 50-digit values of
tests/golden/refine_cases.npz (tools/make_refine_golden.py, tests/test_refine_reference_host.py) are compared with it.

  e = x - proj(K, R X + t) over the active points (mask byte != 0)            cost = sum |e|^2
  p = R X + t, a = fx / p_z, b = fy / p_z, c = -fx p_x / p_z^2, d = -fy p_y / p_z^2
  J = [a 0 c  c p_y  a p_z - c p_x  -a p_y;  0 b d  d p_y - b p_z  -d p_x  b p_x]
  A = sum J^T J (21 sums), g = sum J^T e (6), cost (1); A d = g by Gauss-Jordan elimination without pivoting, refused on
  a pivot that is not positive; T <- [Exp(w) | v] T for d = (v, w), the series below th^2 = 1/16

Order: the start is evaluated; fewer than three active points or a start cost that is not finite end it there.  Then
`max_iter` accepted steps -> stop; solve (refused -> stop); |d| <= tol (1 + |t_trial|) -> stop, the step is not taken;
evaluation; not cost_new <= cost -> stop, the previous pose stays; accept and count; cost - cost_new <= 1e-16 cost -> stop.

refine() also returns the reason it stopped, th^2 of the first step, and the smallest relative margin of the decisions it
took (accept / reject: |cost_new - cost| / cost; the step test: | |d| - limit | / limit), and takes a permutation of the
point order in which every sum is then formed."""
import types

import numpy as np

from window_ba_reference import rodrigues_coefficients

FEW_POINTS, NOT_FINITE, MAX_ITER, PIVOT, STEP, REJECTED, COST_CLAUSE = (
    "few points", "start not finite", "max_iter", "pivot", "step", "rejected", "cost clause")
UNCHANGED = (FEW_POINTS, NOT_FINITE)      # the reasons that promise the start pose bit for bit, whatever else holds
TOL = 1e-9


def active(n, mask):
    return np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0


def point_terms(X, x, K, R, t):
    """The 28 terms of every point, (n, 28), in the kernel's order: the upper triangle of J^T J row by row with its zero
    entry (0, 1) left at column 1, J^T e, |e|^2."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        px = R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]
        py = R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]
        pz = R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2]
        iz = 1.0 / pz
        eu = x[:, 0] - (fx * px * iz + cx)
        ev = x[:, 1] - (fy * py * iz + cy)
        a, c = fx * iz, -fx * px * iz * iz
        b, d = fy * iz, -fy * py * iz * iz
        J0 = [a, None, c, c * py, a * pz - c * px, -a * py]
        J1 = [None, b, d, -b * pz + d * py, -d * px, b * px]
        T = np.zeros((len(X), 28))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                if J0[i] is not None and J0[j] is not None and J1[i] is not None and J1[j] is not None:
                    T[:, k] = J0[i] * J0[j] + J1[i] * J1[j]
                elif J0[i] is not None and J0[j] is not None:
                    T[:, k] = J0[i] * J0[j]
                elif J1[i] is not None and J1[j] is not None:
                    T[:, k] = J1[i] * J1[j]
                k += 1
        for i in range(6):
            if J0[i] is None:
                T[:, 21 + i] = J1[i] * ev
            elif J1[i] is None:
                T[:, 21 + i] = J0[i] * eu
            else:
                T[:, 21 + i] = J0[i] * eu + J1[i] * ev
        T[:, 27] = eu * eu + ev * ev
    return T


def sums(X, x, K, R, t):
    """(A (6, 6), g (6,), cost) over the points given, summed in their order (NumPy's pairwise sum)."""
    with np.errstate(all="ignore"):
        s = point_terms(X, x, K, R, t).sum(axis=0) if len(X) else np.zeros(28)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, s[21:27].copy(), float(s[27])


def solve6(A, g):
    """Gauss-Jordan elimination row by row without pivoting, as solve6_rows does it; None when a pivot is not positive."""
    M = np.concatenate((np.array(A, np.float64), np.asarray(g, np.float64).reshape(6, 1)), axis=1)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(6):
            pk = M[k].copy()
            ok = ok and bool(pk[k] > 0.0)
            for i in range(6):
                if i != k:
                    f = M[i, k] / pk[k]
                    M[i, k + 1:] = M[i, k + 1:] - f * pk[k + 1:]
                    M[i, k] = 0.0
        d = M[:, 6] / np.diag(M)
    return d if ok else None


def apply_increment(R, t, d):
    """[Exp(w) | v] T for d = (v, w); also th^2."""
    v, w = d[:3], d[3:]
    th2 = float(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    ca, cb = rodrigues_coefficients(th2)
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            w2 = 0.0 + Wx[r, 0] * Wx[0, c] + Wx[r, 1] * Wx[1, c] + Wx[r, 2] * Wx[2, c]
            E[r, c] = (1.0 if r == c else 0.0) + ca * Wx[r, c] + cb * w2
    Rn, tn = np.empty((3, 3)), np.empty(3)
    for r in range(3):
        for c in range(3):
            Rn[r, c] = E[r, 0] * R[0, c] + E[r, 1] * R[1, c] + E[r, 2] * R[2, c]
        tn[r] = E[r, 0] * t[0] + E[r, 1] * t[1] + E[r, 2] * t[2] + v[r]
    return Rn, tn, th2


def norm(v):
    s = 0.0
    for q in v:
        s = s + q * q
    return float(np.sqrt(s))


def refine(X, x, K, R0, t0, mask=None, max_iter=20, perm=None, tol=TOL):
    """Runs the rule.  Returns R, t, iterations, cost, cost0, n_active, reason, th2_first (None: no step was formed),
    min_margin, steps (|d| of every step formed)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    x = np.asarray(x, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64).reshape(3, 3)
    on = np.flatnonzero(active(len(X), mask))
    if perm is not None:
        on = np.asarray(perm)[np.isin(perm, on)]
    Xa, xa = X[on], x[on]
    R, t = np.array(R0, np.float64).reshape(3, 3), np.array(t0, np.float64).reshape(3)
    A, g, cost = sums(Xa, xa, K, R, t)
    out = types.SimpleNamespace(R=R, t=t, iterations=0, cost=cost, cost0=cost, n_active=len(on), reason=None,
                                th2_first=None, min_margin=np.inf, steps=[])
    if len(on) < 3:
        out.reason = FEW_POINTS
        return out
    if not np.isfinite(cost):
        out.reason = NOT_FINITE
        return out
    while True:
        if out.iterations >= max_iter:
            out.reason = MAX_ITER
            break
        d = solve6(A, g)
        if d is None:
            out.reason = PIVOT
            break
        with np.errstate(all="ignore"):
            Rn, tn, th2 = apply_increment(R, t, d)
            dn, limit = norm(d), tol * (1.0 + norm(tn))
        if out.th2_first is None:
            out.th2_first = th2
        out.steps.append(dn)
        if np.isfinite(dn) and np.isfinite(limit):
            out.min_margin = min(out.min_margin, abs(dn - limit) / limit)
        if dn <= limit:
            out.reason = STEP
            break
        An, gn, cost_new = sums(Xa, xa, K, Rn, tn)
        if np.isfinite(cost_new) and cost > 0.0:
            out.min_margin = min(out.min_margin, abs(cost_new - cost) / cost)
        if not cost_new <= cost:
            out.reason = REJECTED
            break
        R, t, A, g = Rn, tn, An, gn
        out.iterations += 1
        done = cost - cost_new <= 1e-16 * cost
        cost = cost_new
        if done:
            out.reason = COST_CLAUSE
            break
    out.R, out.t, out.cost = R, t, cost
    return out
