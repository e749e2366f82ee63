"""The definition the window bundle adjustment is pinned to.  TEST INFRASTRUCTURE.

The rule of include/vo_hip.h ("Window bundle adjustment") stated in float64 NumPy, vectorised over observations; the
kernels of csrc/window_ba.hip (tests/test_gpu_window_ba.py) and SciPy (tests/test_window_ba_host.py) are compared with it.

A window: K (3, 3); poses (W, 12), world -> camera, R row-major then t; X (L, 3); lm_start (L + 1,) the CSR of the
observations by landmark; obs_slot (M,) ascending within a landmark; obs_xy (M, 2).  The leading n_fixed slots are held.

  e = x - proj(K, R X + t)       rho = |e|^2, or Huber's (|e|^2 up to delta, 2 delta |e| - delta^2 above; w = min(1, delta / |e|))
  cost = sum rho
  pose increment d = (v, w) on the left: T <- [Exp(w) | v] T; landmark increment additive
  U_j = sum w Jp^T Jp   V_i = sum w Jl^T Jl   W_ij = w Jp^T Jl   g_p = sum w Jp^T e   g_l = sum w Jl^T e
  damping diag <- diag (1 + lambda) on U and V;  S = U* - sum_i W_i V_i*^-1 W_i^T,  b = g_p - sum_i W_i V_i*^-1 g_l,i
  S solved by Cholesky without pivoting, landmarks by back-substitution; a non-positive pivot rejects the trial

Control: lambda0 = 1e-3; in this order before every trial: `max_iter` accepted steps -> status 1, `max_trials` trials ->
status 2, lambda > 1e12 -> status 3; the system is solved (a non-positive pivot: the trial is counted and rejected); a step
with |delta| <= step_tol (1 + |x|) -- delta: every pose and landmark increment, x: the free poses' translations and every
landmark -- is not taken and not counted: status 0; the trial is accepted iff every observation has p_z > 0 at the trial
point and cost_new <= cost: lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.  Refused (status 4, nothing
changes): L == 0, no free pose, a landmark without observations or a slot outside 0 .. W - 1, a non-finite observation,
pose or landmark, p_z <= 0 at the start.

solve() also returns the smallest relative margin of the decisions it took (accept / reject: |cost_new - cost| / cost; the
stop test: | |delta| - limit | / limit) and the cost of every trial, and takes a permutation of the observation order in
which every sum over observations is then formed."""
import types

import numpy as np

STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_MAX_TRIALS, STATUS_LAMBDA, STATUS_REFUSED = 0, 1, 2, 3, 4
LAMBDA_MAX, LAMBDA_MIN = 1e12, 1e-12


def window(K, poses, X, lm_start, obs_slot, obs_xy):
    return types.SimpleNamespace(K=np.asarray(K, np.float64).reshape(3, 3), poses=np.array(poses, np.float64).reshape(-1, 12),
                                 X=np.array(X, np.float64).reshape(-1, 3), lm_start=np.asarray(lm_start, np.int64).reshape(-1),
                                 obs_slot=np.asarray(obs_slot, np.int64).reshape(-1),
                                 obs_xy=np.asarray(obs_xy, np.float64).reshape(-1, 2))


def obs_landmark(lm_start):
    return np.repeat(np.arange(len(lm_start) - 1), np.diff(lm_start))


def rodrigues_coefficients(th2):
    """sin(th)/th and (1 - cos th)/th^2 as csrc/refine.hip forms them: the nested series below th^2 = 1/16."""
    if th2 < 0.0625:
        sa = sb = 1.0
        ca = [1.0 / 272, 1.0 / 210, 1.0 / 156, 1.0 / 110, 1.0 / 72, 1.0 / 42, 1.0 / 20, 1.0 / 6]
        cb = [1.0 / 306, 1.0 / 240, 1.0 / 182, 1.0 / 132, 1.0 / 90, 1.0 / 56, 1.0 / 30, 1.0 / 12]
        for k in range(8):
            sa = 1.0 - th2 * ca[k] * sa
            sb = 1.0 - th2 * cb[k] * sb
        return sa, 0.5 * sb
    th = np.sqrt(th2)
    return np.sin(th) / th, (1.0 - np.cos(th)) / th2


def apply_pose_increment(pose12, d):
    """[Exp(w) | v] T for d = (v, w)."""
    v, w = d[:3], d[3:]
    a, b = rodrigues_coefficients(float(w @ w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(3) + a * Wx + b * (Wx @ Wx)
    R, t = pose12[:9].reshape(3, 3), pose12[9:]
    return np.concatenate(((E @ R).reshape(9), E @ t + v))


def residuals(win, poses, X, huber_px=0.0):
    """Per observation: camera point p (M, 3), e (M, 2), rho (M,), IRLS weight (M,)."""
    lm = obs_landmark(win.lm_start)
    P = poses[win.obs_slot]
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    p = np.einsum("mij,mj->mi", R, X[lm]) + t
    fx, fy, cx, cy = win.K[0, 0], win.K[1, 1], win.K[0, 2], win.K[1, 2]
    with np.errstate(all="ignore"):
        iz = 1.0 / p[:, 2]
        e = np.stack((win.obs_xy[:, 0] - (fx * p[:, 0] * iz + cx), win.obs_xy[:, 1] - (fy * p[:, 1] * iz + cy)), axis=1)
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        if huber_px > 0.0:
            r = np.sqrt(r2)
            big = r > huber_px
            rho = np.where(big, 2.0 * huber_px * r - huber_px * huber_px, r2)
            w = np.where(big, huber_px / np.where(big, r, 1.0), 1.0)
        else:
            rho, w = r2, np.ones_like(r2)
    return p, e, rho, w


def jacobians(win, poses, p):
    """J_pose (M, 2, 6) for d = (v, w) (csrc/refine.hip's J0 / J1) and J_lm (M, 2, 3) = (d proj / d p) R."""
    fx, fy = win.K[0, 0], win.K[1, 1]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    iz = 1.0 / pz
    a, c = fx * iz, -fx * px * iz * iz
    b, d = fy * iz, -fy * py * iz * iz
    z = np.zeros_like(a)
    Jp = np.stack((np.stack((a, z, c, c * py, a * pz - c * px, -a * py), axis=1),
                   np.stack((z, b, d, -b * pz + d * py, -d * px, b * px), axis=1)), axis=1)
    R = poses[win.obs_slot][:, :9].reshape(-1, 3, 3)
    Jl = np.stack((a[:, None] * R[:, 0] + c[:, None] * R[:, 2], b[:, None] * R[:, 1] + d[:, None] * R[:, 2]), axis=1)
    return Jp, Jl


def _cholesky(A):
    """Lower factor without pivoting, or None at the first pivot that is not positive."""
    n = len(A)
    Lm = np.zeros_like(A)
    for k in range(n):
        d = A[k, k] - Lm[k, :k] @ Lm[k, :k]
        if not d > 0.0:
            return None
        s = np.sqrt(d)
        Lm[k, k] = s
        Lm[k + 1:, k] = (A[k + 1:, k] - Lm[k + 1:, :k] @ Lm[k, :k]) / s
    return Lm


def _chol_solve(Lm, b):
    n = len(b)
    y = np.zeros(n)
    for k in range(n):
        y[k] = (b[k] - Lm[k, :k] @ y[:k]) / Lm[k, k]
    x = np.zeros(n)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - Lm[k + 1:, k] @ x[k + 1:]) / Lm[k, k]
    return x


def _inverse3_spd(V):
    """Inverses of (L, 3, 3) symmetric matrices through their Cholesky factors; ok False where a pivot is not positive."""
    with np.errstate(all="ignore"):
        d0 = V[:, 0, 0]
        l00 = np.sqrt(d0)
        l10, l20 = V[:, 1, 0] / l00, V[:, 2, 0] / l00
        d1 = V[:, 1, 1] - l10 * l10
        l11 = np.sqrt(d1)
        l21 = (V[:, 2, 1] - l20 * l10) / l11
        d2 = V[:, 2, 2] - l20 * l20 - l21 * l21
        l22 = np.sqrt(d2)
        ok = (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0)
        # M = L^-1 (lower), V^-1 = M^T M
        m00, m11, m22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
        m10 = -l10 * m00 * m11
        m21 = -l21 * m11 * m22
        m20 = -(l20 * m00 + l21 * m10) * m22
        inv = np.empty_like(V)
        inv[:, 0, 0] = m00 * m00 + m10 * m10 + m20 * m20
        inv[:, 1, 0] = inv[:, 0, 1] = m10 * m11 + m20 * m21
        inv[:, 2, 0] = inv[:, 0, 2] = m20 * m22
        inv[:, 1, 1] = m11 * m11 + m21 * m21
        inv[:, 2, 1] = inv[:, 1, 2] = m21 * m22
        inv[:, 2, 2] = m22 * m22
    return inv, bool(np.all(ok))


def refusal(win, n_fixed):
    """The reason a window is refused (status 4), or None."""
    W, L, M = len(win.poses), len(win.X), len(win.obs_slot)
    if L == 0:
        return "empty"
    if not 1 <= n_fixed < W:
        return "no free pose"
    if len(win.lm_start) != L + 1 or win.lm_start[0] != 0 or win.lm_start[-1] != M or np.any(np.diff(win.lm_start) < 1):
        return "a landmark without observations"
    if np.any(win.obs_slot < 0) or np.any(win.obs_slot >= W):
        return "slot out of range"
    if not (np.all(np.isfinite(win.obs_xy)) and np.all(np.isfinite(win.poses)) and np.all(np.isfinite(win.X))):
        return "non-finite input"
    p = residuals(win, win.poses, win.X)[0]
    if not np.all(p[:, 2] > 0.0):
        return "a point behind a camera"
    return None


def linearise(win, poses, X, n_fixed, huber_px, order):
    """The blocks at (poses, X), every sum formed in the observation order `order`."""
    W, L = len(poses), len(X)
    lm = obs_landmark(win.lm_start)
    p, e, rho, w = residuals(win, poses, X, huber_px)
    Jp, Jl = jacobians(win, poses, p)
    o = order
    U, V = np.zeros((W, 6, 6)), np.zeros((L, 3, 3))
    gp, gl = np.zeros((W, 6)), np.zeros((L, 3))
    wJp, wJl = w[:, None, None] * Jp, w[:, None, None] * Jl
    np.add.at(U, win.obs_slot[o], np.einsum("mki,mkj->mij", wJp, Jp)[o])
    np.add.at(V, lm[o], np.einsum("mki,mkj->mij", wJl, Jl)[o])
    np.add.at(gp, win.obs_slot[o], np.einsum("mki,mk->mi", wJp, e)[o])
    np.add.at(gl, lm[o], np.einsum("mki,mk->mi", wJl, e)[o])
    Wm = np.einsum("mki,mkj->mij", wJp, Jl)
    return types.SimpleNamespace(U=U, V=V, gp=gp, gl=gl, Wm=Wm, lm=lm, cost=float(np.sum(rho[o])))


def _free_pairs(win, n_fixed, order):
    """Every ordered pair (o1, o2) of observations of one landmark from free slots, in the order `order` gives o1 then o2."""
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    lm = obs_landmark(win.lm_start)
    free = np.flatnonzero(win.obs_slot >= n_fixed)
    free = free[np.argsort(rank[free], kind="stable")]
    by_lm = {}
    for o in free:
        by_lm.setdefault(int(lm[o]), []).append(int(o))
    a, b = [], []
    for o in free:
        mates = by_lm[int(lm[o])]
        a.extend([int(o)] * len(mates))
        b.extend(mates)
    return free, np.array(a, np.int64), np.array(b, np.int64)


def solve_step(win, lin, lam, n_fixed, pairs):
    """(dp (W - n_fixed, 6), dl (L, 3)) of the damped, reduced system, or None when a pivot is not positive."""
    W, L = len(lin.U), len(lin.V)
    nf = W - n_fixed
    damp = 1.0 + lam
    Vs = lin.V.copy()
    Vs[:, [0, 1, 2], [0, 1, 2]] *= damp
    Vinv, ok = _inverse3_spd(Vs)
    if not ok:
        return None
    free, pa, pb = pairs
    Y = np.einsum("mij,mjk->mik", lin.Wm, Vinv[lin.lm])
    S = np.zeros((nf, 6, nf, 6))
    for j in range(nf):
        Uj = lin.U[n_fixed + j].copy()
        Uj[np.arange(6), np.arange(6)] *= damp
        S[j, :, j, :] = Uj
    S4 = np.zeros((nf, nf, 6, 6))
    np.add.at(S4, (win.obs_slot[pa] - n_fixed, win.obs_slot[pb] - n_fixed), np.einsum("mik,mjk->mij", Y[pa], lin.Wm[pb]))
    S -= S4.transpose(0, 2, 1, 3)
    b = lin.gp[n_fixed:].copy()
    bs = np.zeros_like(b)
    np.add.at(bs, win.obs_slot[free] - n_fixed, np.einsum("mik,mk->mi", Y[free], lin.gl[lin.lm[free]]))
    b -= bs
    Lm = _cholesky(S.reshape(6 * nf, 6 * nf))
    if Lm is None:
        return None
    dp = _chol_solve(Lm, b.reshape(-1)).reshape(nf, 6)
    rhs = lin.gl.copy()
    back = np.zeros_like(rhs)
    np.add.at(back, lin.lm[free], np.einsum("mik,mi->mk", lin.Wm[free], dp[win.obs_slot[free] - n_fixed]))
    rhs -= back
    dl = np.einsum("lij,lj->li", Vinv, rhs)
    return dp, dl


def solve(win, n_fixed=2, huber_px=0.0, max_iter=10, max_trials=0, lambda0=0.0, step_tol=0.0, perm=None):
    """Runs the rule.  Returns poses, X, status, iterations, trials, n_obs, cost0, cost, lam, min_margin, trial_costs."""
    max_iter = max_iter or 10
    max_trials = max_trials or 2 * max_iter
    n_fixed = n_fixed or 2
    lam = lambda0 or 1e-3
    step_tol = step_tol or 1e-10
    M = len(win.obs_slot)
    out = types.SimpleNamespace(poses=win.poses.copy(), X=win.X.copy(), status=STATUS_REFUSED, iterations=0, trials=0, n_obs=M,
                                cost0=0.0, cost=0.0, lam=lam, min_margin=np.inf, trial_costs=[])
    if refusal(win, n_fixed) is not None:
        return out
    order = np.arange(M) if perm is None else np.asarray(perm, np.int64)
    assert np.array_equal(np.sort(order), np.arange(M))
    pairs = _free_pairs(win, n_fixed, order)
    poses, X = out.poses, out.X
    lin = linearise(win, poses, X, n_fixed, huber_px, order)
    cost = out.cost0 = lin.cost
    it = trials = 0
    while True:
        if it >= max_iter:
            status = STATUS_MAX_ITER
            break
        if trials >= max_trials:
            status = STATUS_MAX_TRIALS
            break
        if lam > LAMBDA_MAX:
            status = STATUS_LAMBDA
            break
        step = solve_step(win, lin, lam, n_fixed, pairs)
        if step is None:
            trials += 1
            out.trial_costs.append(np.nan)
            lam *= 10.0
            continue
        dp, dl = step
        dn = np.sqrt(np.sum(dp * dp) + np.sum(dl * dl))
        xn = np.sqrt(np.sum(poses[n_fixed:, 9:] ** 2) + np.sum(X * X))
        limit = step_tol * (1.0 + xn)
        out.min_margin = min(out.min_margin, abs(dn - limit) / limit)
        if dn <= limit:
            status = STATUS_CONVERGED
            break
        trials += 1
        poses_try = poses.copy()
        for j in range(len(dp)):
            poses_try[n_fixed + j] = apply_pose_increment(poses[n_fixed + j], dp[j])
        X_try = X + dl
        p, _, rho, _ = residuals(win, poses_try, X_try, huber_px)
        cost_new = float(np.sum(rho[order]))
        out.trial_costs.append(cost_new)
        front = bool(np.all(p[:, 2] > 0.0))
        if front and cost > 0.0:
            out.min_margin = min(out.min_margin, abs(cost_new - cost) / cost)
        if front and cost_new <= cost:
            poses, X, cost = poses_try, X_try, cost_new
            it += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            lin = linearise(win, poses, X, n_fixed, huber_px, order)
        else:
            lam *= 10.0
    out.poses, out.X, out.status, out.iterations, out.trials, out.cost, out.lam = poses, X, status, it, trials, cost, lam
    return out
