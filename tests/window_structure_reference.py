"""The definition the window structure refinement is pinned to.  TEST INFRASTRUCTURE.

The rule of include/vo_hip.h ("Window structure refinement") stated in float64 NumPy, one landmark at a time, every sum over
a landmark's observations formed one term after the other in CSR order (or in the order a permutation gives); the kernels of
csrc/window_structure.hip (tests/test_gpu_window_structure.py) and SciPy (tests/test_window_structure_host.py) are compared
with it.  The window is window_ba_reference's (K, poses (W, 12), X (L, 3), lm_start, obs_slot, obs_xy); the poses are held,
so landmark i is a least-squares problem of its own in three unknowns:

  e, rho, w, p, J_lm   as in the window bundle adjustment (window_ba_reference.residuals / jacobians)
  V = sum w J_lm^T J_lm    g = sum w J_lm^T e    cost = sum rho
  damping: diag V <- diag V (1 + lambda); Cholesky without pivoting, dX = V*^-1 g; a pivot that is not positive rejects the
  trial (counted, lambda <- 10 lambda)

Control: lambda0 = 1e-3; before every trial, in this order: `max_iter` accepted steps -> status 1, `max_trials` trials ->
status 2, lambda > 1e12 -> status 3; then the system is solved.  The step is not taken and not counted, status 0, when
|dX| <= step_tol (1 + |X|) or g . dX <= f_tol cost (the predicted first-order decrease).  Otherwise the trial is counted and
accepted iff every observation has p_z > 0 at X + dX and cost_new <= cost: lambda <- max(lambda / 10, 1e-12), else
lambda <- 10 lambda.  Refused (status 4, X bit for bit): fewer than 2 observations or more than W, slots not strictly
ascending in 0 .. W - 1, a non-finite observation or X, p_z <= 0 at the start; a window whose CSR does not end at M or
with a non-finite pose or intrinsic refuses every landmark.  min_cos: the smallest cosine between two of the landmark's
world-frame observation rays.  Kept iff status is 0 or 1, gate_px == 0 or sqrt(sum |e|^2 / n_obs) <= gate_px at the result,
and min_parallax == 0 or min_cos <= cos(min_parallax); a landmark not kept gets its input X back.

solve() also returns the smallest relative margin of the decisions it took, by kind -- "accept" (|cost_new - cost| / cost),
"step" and "decrease" (the two stop tests: |value - limit| / limit), "gate" and "parallax" (the two gates) -- and takes a
permutation of the observation order."""
import types

import numpy as np

import window_ba_reference as ref

STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_MAX_TRIALS, STATUS_LAMBDA, STATUS_REFUSED = 0, 1, 2, 3, 4
LAMBDA_MAX, LAMBDA_MIN = 1e12, 1e-12
MARGIN_KINDS = ("accept", "step", "decrease", "gate", "parallax")


def _ordered_sum(terms):
    """terms[0] + terms[1] + ... one after the other."""
    acc = np.array(terms[0], np.float64)
    for t in terms[1:]:
        acc = acc + t
    return acc


def _solve3(V, g, damp):
    """dX of (V with its diagonal times damp) dX = g by Cholesky without pivoting, or None at a pivot that is not positive."""
    v00, v01, v02, v11, v12, v22 = V[0, 0] * damp, V[0, 1], V[0, 2], V[1, 1] * damp, V[1, 2], V[2, 2] * damp
    if not v00 > 0.0:
        return None
    l00 = np.sqrt(v00)
    l10, l20 = v01 / l00, v02 / l00
    d1 = v11 - l10 * l10
    if not d1 > 0.0:
        return None
    l11 = np.sqrt(d1)
    l21 = (v12 - l20 * l10) / l11
    d2 = v22 - l20 * l20 - l21 * l21
    if not d2 > 0.0:
        return None
    l22 = np.sqrt(d2)
    y0 = g[0] / l00
    y1 = (g[1] - l10 * y0) / l11
    y2 = (g[2] - l20 * y0 - l21 * y1) / l22
    x2 = y2 / l22
    x1 = (y1 - l21 * x2) / l11
    x0 = (y0 - l10 * x1 - l20 * x2) / l00
    return np.array([x0, x1, x2])


def window_refusal(win):
    """The reason every landmark of the window is refused, or None."""
    L, M = len(win.X), len(win.obs_slot)
    if len(win.lm_start) != L + 1 or (L > 0 and win.lm_start[L] != M):
        return "the CSR does not end at M"
    if not np.all(np.isfinite(win.poses)):
        return "non-finite pose"
    if not np.all(np.isfinite([win.K[0, 0], win.K[1, 1], win.K[0, 2], win.K[1, 2]])):
        return "non-finite intrinsic"
    return None


def rays(win, slots, xy):
    """The world-frame unit rays of observations (slot, xy)."""
    fx, fy, cx, cy = win.K[0, 0], win.K[1, 1], win.K[0, 2], win.K[1, 2]
    d = np.stack(((xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy, np.ones(len(xy))), axis=1)
    R = win.poses[slots][:, :9].reshape(-1, 3, 3)
    dw = np.einsum("mji,mj->mi", R, d)
    return dw / np.sqrt(np.sum(dw * dw, axis=1))[:, None]


def solve_landmark(win, i, prm, order=None, margins=None):
    """The rule for landmark i.  prm: the resolved parameters; order: the order of its observations (indices into the
    window's arrays).  Returns X (3,), status, iterations, trials, n_obs, cost0, cost, min_cos, kept."""
    W, M = len(win.poses), len(win.obs_slot)
    X0 = win.X[i].copy()
    s, e = int(win.lm_start[i]), int(win.lm_start[i + 1])
    n = e - s
    refused = (X0, STATUS_REFUSED, 0, 0, n if 0 <= n <= W and 0 <= s and e <= M else 0, 0.0, 0.0, 0.0, 0)
    if s < 0 or e > M or n < 2 or n > W:
        return refused
    idx = np.arange(s, e) if order is None else np.asarray(order, np.int64)
    slots, xy = win.obs_slot[s:e], win.obs_xy[s:e]
    if np.any(slots < 0) or np.any(slots >= W) or np.any(np.diff(slots) <= 0):
        return refused
    if not (np.all(np.isfinite(xy)) and np.all(np.isfinite(X0))):
        return refused
    sub = types.SimpleNamespace(K=win.K, lm_start=np.array([0, n]), obs_slot=win.obs_slot[idx], obs_xy=win.obs_xy[idx])
    huber = prm.huber_px

    def evaluate(X):
        p, e2, rho, w = ref.residuals(sub, win.poses, X[None], huber)
        return p, e2, w, float(_ordered_sum(rho)), float(_ordered_sum(np.sum(e2 * e2, axis=1))), bool(np.all(p[:, 2] > 0.0))

    p, e2, w, cost, sq, front = evaluate(X0)
    if not front or not np.isfinite(cost):
        return refused
    d = rays(win, sub.obs_slot, sub.obs_xy)
    cosines = d @ d.T
    min_cos = float(np.min(cosines[~np.eye(n, dtype=bool)]))
    note = (lambda kind, m: margins.__setitem__(kind, min(margins[kind], m))) if margins is not None else (lambda kind, m: None)
    X, cost0, lam, it, trials = X0, cost, prm.lambda0, 0, 0
    lin = None
    while True:
        if it >= prm.max_iter:
            status = STATUS_MAX_ITER
            break
        if trials >= prm.max_trials:
            status = STATUS_MAX_TRIALS
            break
        if lam > LAMBDA_MAX:
            status = STATUS_LAMBDA
            break
        if lin is None:
            _, Jl = ref.jacobians(sub, win.poses, p)
            wJ = w[:, None, None] * Jl
            lin = (_ordered_sum(np.einsum("mki,mkj->mij", wJ, Jl)), _ordered_sum(np.einsum("mki,mk->mi", wJ, e2)))
        V, g = lin
        dX = _solve3(V, g, 1.0 + lam)
        if dX is None:
            trials += 1
            lam *= 10.0
            continue
        dn, limit = np.sqrt(dX @ dX), prm.step_tol * (1.0 + np.sqrt(X @ X))
        pred, floor = float(g @ dX), prm.f_tol * cost
        note("step", abs(dn - limit) / limit)
        if floor > 0.0:
            note("decrease", abs(pred - floor) / floor)
        if dn <= limit or pred <= floor:
            status = STATUS_CONVERGED
            break
        trials += 1
        p_new, e_new, w_new, cost_new, sq_new, front = evaluate(X + dX)
        if front and cost > 0.0:
            note("accept", abs(cost_new - cost) / cost)
        if front and cost_new <= cost:
            X, p, e2, w, cost, sq = X + dX, p_new, e_new, w_new, cost_new, sq_new
            it += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            lin = None
        else:
            lam *= 10.0
    kept = status in (STATUS_CONVERGED, STATUS_MAX_ITER)
    if prm.gate_px > 0.0:
        rms = np.sqrt(sq / n)
        note("gate", abs(rms - prm.gate_px) / prm.gate_px)
        kept = kept and rms <= prm.gate_px
    if prm.min_parallax > 0.0:
        limit = np.cos(prm.min_parallax)
        note("parallax", abs(min_cos - limit) / limit)
        kept = kept and min_cos <= limit
    return (X if kept else X0, status, it, trials, n, cost0, cost, min_cos, int(kept))


def resolve(huber_px=0.0, max_iter=0, max_trials=0, lambda0=0.0, step_tol=0.0, f_tol=0.0, gate_px=0.0, min_parallax=0.0):
    """vo_structure_params with its defaults filled in."""
    max_iter = max_iter or 10
    return types.SimpleNamespace(huber_px=float(huber_px), max_iter=max_iter, max_trials=max_trials or 2 * max_iter,
                                 lambda0=lambda0 or 1e-3, step_tol=step_tol or 1e-10, f_tol=f_tol or 1e-9,
                                 gate_px=float(gate_px), min_parallax=float(min_parallax))


def solve(win, perm=None, **params):
    """Runs the rule over a window.  Returns X (L, 3), the per-landmark arrays status, iterations, trials, n_obs, cost0,
    cost, min_cos, kept, the summary (L, n_refused, n_kept, max_iterations, cost0, cost), margins (by kind) and min_margin.
    perm: a permutation of 0 .. M - 1; every landmark's sums are formed over its observations in the order perm lists them."""
    prm = resolve(**params)
    L, M = len(win.X), len(win.obs_slot)
    margins = {k: np.inf for k in MARGIN_KINDS}
    rows = []
    whole = window_refusal(win)
    rank = None
    if perm is not None:
        perm = np.asarray(perm, np.int64)
        assert np.array_equal(np.sort(perm), np.arange(M))
        rank = np.empty(M, np.int64)
        rank[perm] = np.arange(M)
    for i in range(L):
        if whole is not None:
            rows.append((win.X[i].copy(), STATUS_REFUSED, 0, 0, 0, 0.0, 0.0, 0.0, 0))
            continue
        order = None
        s, e = int(win.lm_start[i]), int(win.lm_start[i + 1])
        if rank is not None and 0 <= s <= e <= M:
            own = np.arange(s, e)
            order = own[np.argsort(rank[own], kind="stable")]
        rows.append(solve_landmark(win, i, prm, order, margins))
    col = lambda k, dt: np.array([r[k] for r in rows], dt).reshape((L,) + ((3,) if k == 0 else ()))
    out = types.SimpleNamespace(X=col(0, np.float64), status=col(1, np.int32), iterations=col(2, np.int32), trials=col(3, np.int32),
                                n_obs=col(4, np.int32), cost0=col(5, np.float64), cost=col(6, np.float64),
                                min_cos=col(7, np.float64), kept=col(8, np.int32), margins=margins,
                                min_margin=min(margins.values()))
    live = out.status != STATUS_REFUSED
    out.summary = types.SimpleNamespace(L=L, n_refused=int(np.sum(~live)), n_kept=int(np.sum(out.kept)),
                                        max_iterations=int(out.iterations.max()) if L else 0,
                                        cost0=float(_ordered_sum(out.cost0[live])) if live.any() else 0.0,
                                        cost=float(_ordered_sum(out.cost[live])) if live.any() else 0.0)
    return out
