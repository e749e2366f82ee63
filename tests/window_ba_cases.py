"""The window bundle adjustment's case table (tests/test_window_ba_host.py, tests/test_gpu_window_ba.py): seeded synthetic
windows, small, each named for the edge it keeps.  TEST INFRASTRUCTURE.

A camera (f = 420, 640 x 480) drives forward and sideways (0.8 m and 0.35 m per frame); landmarks lie 5 .. 16 m ahead of the last pose; every
observation carries 0.3 px of noise; the start is the generating poses and landmarks perturbed (free poses by ~8 cm and
~0.6 degrees, landmarks by ~40 cm), the fixed slots exact."""
import types

import numpy as np

import window_ba_reference as ref

OUTLIER_PX = (8.0, 15.0)      # a gross outlier is off by this much along each axis (the noise: 0.3 px)
K = np.array([[420.0, 0.0, 320.0], [0.0, 420.0, 240.0], [0.0, 0.0, 1.0]])


def _true_poses(rng, W):
    poses = np.zeros((W, 12))
    for j in range(W):
        w = np.array([0.004, 0.012, -0.003]) * j + rng.normal(0.0, 0.002, 3)
        c = np.array([0.35 * j, -0.1 * j, 0.8 * j]) + rng.normal(0.0, 0.02, 3)        # camera centre in the world
        R = ref.apply_pose_increment(np.concatenate((np.eye(3).reshape(9), np.zeros(3))), np.concatenate((np.zeros(3), w)))[:9]
        R = R.reshape(3, 3)
        poses[j] = np.concatenate((R.reshape(9), -R @ c))
    return poses


def make(seed, W, L, lengths="all", n_fixed=2, huber_px=0.0, outliers=0.0, fixed_only=0, thin_pose=None):
    """lengths: "all" (every slot), "missing" (each observation dropped with probability 0.25, two kept), "ragged" (a run
    of 2 .. W consecutive slots).  fixed_only: that many landmarks seen from the fixed slots alone.  thin_pose: a free slot
    left with exactly three observations."""
    rng = np.random.default_rng(seed)
    Pt = _true_poses(rng, W)
    Xt = np.stack((rng.uniform(-3.0, 3.0, L) + 0.17 * (W - 1), rng.uniform(-2.0, 2.0, L), rng.uniform(5.0, 16.0, L) + 0.8 * (W - 1)), axis=1)
    seen = np.ones((L, W), bool)
    if lengths == "missing":
        seen = rng.uniform(size=(L, W)) >= 0.25
        seen[:, 0] = True
        seen[np.arange(L), 1 + rng.integers(0, W - 1, L)] = True
        assert not seen.all()
    elif lengths == "ragged":
        n = 2 + np.arange(L) % (W - 1)
        first = rng.integers(0, W - n + 1)
        slots = np.arange(W)[None, :]
        seen = (slots >= first[:, None]) & (slots < (first + n)[:, None])
    if fixed_only:
        seen[:fixed_only] = False
        seen[:fixed_only, :n_fixed] = True
    if thin_pose is not None:
        keep = rng.choice(L - fixed_only, 3, replace=False) + fixed_only
        col = np.zeros(L, bool)
        col[keep] = True
        seen[:, thin_pose] = col
        assert np.all(seen.sum(axis=1) >= 2)
    lm, slot = np.nonzero(seen)
    lm_start = np.concatenate(([0], np.cumsum(seen.sum(axis=1))))
    R, t = Pt[slot][:, :9].reshape(-1, 3, 3), Pt[slot][:, 9:]
    p = np.einsum("mij,mj->mi", R, Xt[lm]) + t
    assert np.all(p[:, 2] > 1.0)
    xy = np.stack((K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]), axis=1)
    xy += rng.normal(0.0, 0.3, xy.shape)
    n_out = int(round(outliers * len(xy)))
    out_idx = np.sort(rng.choice(len(xy), n_out, replace=False)) if n_out else np.zeros(0, np.int64)
    xy[out_idx] += rng.uniform(OUTLIER_PX[0], OUTLIER_PX[1], (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    P0 = Pt.copy()
    for j in range(n_fixed, W):
        P0[j] = ref.apply_pose_increment(Pt[j], np.concatenate((rng.normal(0.0, 0.08, 3), rng.normal(0.0, 0.01, 3))))
    X0 = Xt + rng.normal(0.0, 0.4, Xt.shape)
    win = ref.window(K, P0, X0, lm_start, slot, xy)
    return types.SimpleNamespace(win=win, true_poses=Pt, true_X=Xt, n_fixed=n_fixed, huber_px=huber_px, outlier_obs=out_idx,
                                 seen=seen)


def _refused(kind):
    c = make(31, 4, 12, "missing")
    if kind == "behind":
        c.win.X[5, 2] = -3.0                     # behind every camera of the window at the start
    else:
        c.win.obs_xy[7, 1] = np.nan
    return c


CASES = {
    "w3_l8_full": lambda: make(1, 3, 8),
    "w4_l12_missing": lambda: make(2, 4, 12, "missing"),
    "w6_l40_ragged": lambda: make(3, 6, 40, "ragged"),
    "w8_l60_outliers_huber": lambda: make(106, 8, 60, "missing", huber_px=2.0, outliers=0.05),
    "w8_l60_outliers_squared": lambda: make(106, 8, 60, "missing", outliers=0.05),
    "fixed_only_landmark": lambda: make(5, 4, 16, "missing", fixed_only=2),
    "three_observation_pose": lambda: make(16, 5, 20, thin_pose=3),
    "n_fixed_1": lambda: make(7, 4, 24, "missing", n_fixed=1),
    "l65": lambda: make(8, 5, 65, "ragged"),
    "l129": lambda: make(9, 5, 129, "ragged"),
    "w8_l600": lambda: make(10, 8, 600, "missing"),
}
# compared by parameters after max_iter = 2 and 4 (and by cost when converged)
SOLVED = list(CASES)
REFUSED = {"behind_camera": lambda: _refused("behind"), "nan_observation": lambda: _refused("nan")}
# noisy windows on which the adjustment must bring the free poses closer to the generating ones (not the squared loss with
# gross outliers, which it cannot; not the pose with three observations, which the noise alone moves further than the start)
NOISY = ("w4_l12_missing", "w8_l60_outliers_huber", "l65", "l129", "w8_l600")
BATCH = ("w8_l60_outliers_squared", None, "w8_l600")      # S = 3, one W: different sizes, the middle window empty

_cache = {}


def get(name):
    """The case (built once; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = (CASES.get(name) or REFUSED[name])()
    return _cache[name]


def pose_rms(case, poses):
    """RMS distance of the free poses' translations from the generating ones."""
    f = slice(case.n_fixed, None)
    return float(np.sqrt(np.mean((np.asarray(poses)[f, 9:] - case.true_poses[f, 9:]) ** 2)))


def empty_window(W):
    return ref.window(K, np.tile(np.concatenate((np.eye(3).reshape(9), np.zeros(3))), (W, 1)), np.zeros((0, 3)), [0],
                      np.zeros(0, np.int64), np.zeros((0, 2)))


_solved = {}


def definition(name, max_iter, perm=None):
    """The definition's result for a case (cached per (name, max_iter) for the natural order)."""
    c = get(name)
    if perm is not None:
        return ref.solve(c.win, c.n_fixed, c.huber_px, max_iter, perm=perm)
    if (name, max_iter) not in _solved:
        _solved[name, max_iter] = ref.solve(c.win, c.n_fixed, c.huber_px, max_iter)
    return _solved[name, max_iter]


def scipy_cost(name):
    """The cost SciPy's least_squares reaches on the same objective from the same start (tolerances 1e-15, x_scale='jac',
    analytic Jacobian), cached."""
    key = (name, "scipy")
    if key in _solved:
        return _solved[key]
    from scipy.optimize import least_squares
    from scipy.sparse import csr_matrix
    c = get(name)
    win, nf0 = c.win, c.n_fixed
    W, L, M = len(win.poses), len(win.X), len(win.obs_slot)
    nf = W - nf0
    lm = ref.obs_landmark(win.lm_start)

    def unpack(x):
        poses = win.poses.copy()
        for j in range(nf):
            poses[nf0 + j] = ref.apply_pose_increment(win.poses[nf0 + j], x[6 * j:6 * j + 6])
        return poses, win.X + x[6 * nf:].reshape(L, 3)

    def scale(e, rho):
        r2 = np.sum(e * e, axis=1)
        return np.sqrt(rho / np.where(r2 > 0.0, r2, 1.0))

    def fun(x):
        poses, X = unpack(x)
        _, e, rho, _ = ref.residuals(win, poses, X, c.huber_px)
        return (e * scale(e, rho)[:, None]).reshape(-1)

    free = win.obs_slot >= nf0
    rows = np.arange(2 * M).reshape(M, 2)

    def jac(x):
        # analytic, sparse: the definition's Jacobians are for an increment on the CURRENT pose, x_j is an increment on the
        # start pose; the 6 x 6 map between the two (G below) is taken by finite differences, which only steers the solver
        poses, X = unpack(x)
        p, e, rho, _ = ref.residuals(win, poses, X, c.huber_px)
        Jp, Jl = ref.jacobians(win, poses, p)
        s = scale(e, rho)
        # f = s(e) e, e = x - proj: d f = -(s I + e ds/de^T) J; for the squared part s = 1, for the Huber part
        # s = sqrt(2 d r - d^2) / r
        r = np.sqrt(np.sum(e * e, axis=1))
        D = -s[:, None, None] * np.eye(2)[None]
        if c.huber_px > 0.0:
            d = c.huber_px
            big = r > d
            rb = np.where(big, r, 1.0)
            sb = np.sqrt(np.maximum(2.0 * d * rb - d * d, 0.0))
            ds = np.where(big, (d / np.where(big, sb, 1.0)) / rb - sb / (rb * rb), 0.0) / rb     # (ds/dr) / r
            D = D - ds[:, None, None] * np.einsum("mi,mj->mij", e, e)
        Ap = np.einsum("mik,mkj->mij", D, Jp)
        Al = np.einsum("mik,mkj->mij", D, Jl)
        ri, ci, vi = [], [], []
        fo = np.flatnonzero(free)
        for j in range(nf):
            xj = x[6 * j:6 * j + 6]
            G = np.zeros((6, 6))
            base = ref.apply_pose_increment(win.poses[nf0 + j], xj)
            Rb, tb = base[:9].reshape(3, 3), base[9:]
            for k in range(6):
                h = np.zeros(6)
                h[k] = 1e-7
                q = ref.apply_pose_increment(win.poses[nf0 + j], xj + h)
                dR = q[:9].reshape(3, 3) @ Rb.T
                wv = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0
                G[3:, k] = wv / 1e-7
                G[:3, k] = (q[9:] - dR @ tb) / 1e-7
            sel = fo[win.obs_slot[fo] == nf0 + j]
            blk = np.einsum("mik,kj->mij", Ap[sel], G)
            ri.append(np.repeat(rows[sel].reshape(-1), 6))
            ci.append(np.tile(6 * j + np.arange(6), 2 * len(sel)))
            vi.append(blk.reshape(-1))
        ri.append(np.repeat(rows.reshape(-1), 3))
        ci.append((6 * nf + 3 * lm[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 2, 1), np.int64)).reshape(-1))
        vi.append(Al.reshape(-1))
        return csr_matrix((np.concatenate(vi), (np.concatenate(ri), np.concatenate(ci))), shape=(2 * M, 6 * nf + 3 * L))

    dense = 6 * nf + 3 * L <= 500
    r = least_squares(fun, np.zeros(6 * nf + 3 * L), jac=(lambda x: jac(x).toarray()) if dense else jac, x_scale="jac",
                      ftol=1e-15, xtol=1e-15, gtol=1e-15, method="trf", tr_solver="exact" if dense else "lsmr", max_nfev=400)
    _solved[key] = float(2.0 * r.cost)
    return _solved[key]
