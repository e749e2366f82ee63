"""The window structure refinement's case table (tests/test_window_structure_host.py, tests/test_gpu_window_structure.py):
the window bundle adjustment's seeded windows (tests/window_ba_cases.py: make) with the poses set to the generating ones, so
that the generating landmarks are reachable, each named for the edge it keeps.  TEST INFRASTRUCTURE."""
import copy
import types

import numpy as np

import window_ba_cases as wc
import window_structure_reference as sref

PARALLAX = 0.0075             # the bearing angle at which the frame loop triangulates (radians)


def make(*args, **kw):
    """window_ba_cases.make with every pose the generating one."""
    c = wc.make(*args, **kw)
    c.win.poses = c.true_poses.copy()
    return c


def noise_free(c):
    """The case with every observation the exact projection of its generating landmark."""
    c = copy.deepcopy(c)
    win = c.win
    lm = wc.ref.obs_landmark(win.lm_start)
    P = c.true_poses[win.obs_slot]
    p = np.einsum("mij,mj->mi", P[:, :9].reshape(-1, 3, 3), c.true_X[lm]) + P[:, 9:]
    K = win.K
    win.obs_xy = np.stack((K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]), axis=1)
    c.outlier_obs = np.zeros(0, np.int64)
    return c


def _bad_landmarks():
    """w4_l12_missing's seed with one single-observation landmark (3), one landmark behind the camera (6) and one NaN
    observation (in landmark 9) among good neighbours."""
    c = make(31, 4, 12, "missing")
    win = c.win
    s, e = int(win.lm_start[3]), int(win.lm_start[4])
    drop = np.arange(s + 1, e)                               # landmark 3 keeps its first observation only
    win.obs_slot, win.obs_xy = np.delete(win.obs_slot, drop), np.delete(win.obs_xy, drop, axis=0)
    win.lm_start = win.lm_start.copy()
    win.lm_start[4:] -= len(drop)
    c.seen[3, win.obs_slot[s] + 1:] = False
    win.X[6, 2] = -3.0
    win.obs_xy[int(win.lm_start[9]) + 1, 0] = np.nan
    c.bad = (3, 6, 9)
    return c


def _without(c, drop):
    """The window without the landmarks `drop`."""
    c = copy.deepcopy(c)
    win = c.win
    keep = np.array([i for i in range(len(win.X)) if i not in drop])
    sel = np.concatenate([np.arange(win.lm_start[i], win.lm_start[i + 1]) for i in keep])
    counts = np.diff(win.lm_start)[keep]
    c.win = wc.ref.window(win.K, win.poses, win.X[keep], np.concatenate(([0], np.cumsum(counts))), win.obs_slot[sel], win.obs_xy[sel])
    c.true_X, c.kept_rows = c.true_X[keep], keep
    return c


def _window_refused(kind):
    c = make(2, 4, 12, "missing")
    c.win.lm_start = c.win.lm_start.copy()
    if kind == "csr":
        c.win.lm_start[-1] -= 1                               # lm_start[L] != M
    else:
        c.win.poses[2, 4] = np.inf
    return c


def _zero_parallax():
    """make(32, 4, 12): landmark 5 is seen from slots 0 and 1 only and slot 1 is given slot 0's pose, its observations of
    every landmark recomputed for that pose (consistent): landmark 5's two rays are parallel up to the 0.3 px noise."""
    c = make(32, 4, 12)
    win = c.win
    rng = np.random.default_rng(3200)
    win.poses[1] = win.poses[0]
    c.true_poses[1] = c.true_poses[0]
    lm = wc.ref.obs_landmark(win.lm_start)
    at1 = np.flatnonzero(win.obs_slot == 1)
    R, t = win.poses[1, :9].reshape(3, 3), win.poses[1, 9:]
    p = c.true_X[lm[at1]] @ R.T + t
    K = win.K
    win.obs_xy[at1] = np.stack((K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]), axis=1)
    win.obs_xy[at1] += rng.normal(0.0, 0.3, (len(at1), 2))
    s = int(win.lm_start[5])
    drop = np.arange(s + 2, int(win.lm_start[6]))
    win.obs_slot, win.obs_xy = np.delete(win.obs_slot, drop), np.delete(win.obs_xy, drop, axis=0)
    win.lm_start = win.lm_start.copy()
    win.lm_start[6:] -= len(drop)
    c.seen[5, 2:] = False
    c.thin = 5
    c.min_parallax = PARALLAX
    return c


CASES = {
    "w3_l8_full": lambda: make(1, 3, 8),
    "w4_l12_missing": lambda: make(2, 4, 12, "missing"),
    "w6_l40_ragged": lambda: make(3, 6, 40, "ragged"),
    "w8_l60_outliers_huber": lambda: make(106, 8, 60, "missing", huber_px=2.0, outliers=0.05),
    "w8_l60_outliers_squared": lambda: make(106, 8, 60, "missing", outliers=0.05),
    "l65": lambda: make(8, 5, 65, "ragged"),
    "l129": lambda: make(9, 5, 129, "ragged"),
    "w8_l600": lambda: make(10, 8, 600, "missing"),
    # the kernel's edges: one row of one wave; a wave remainder; every lane of a row busy and a workgroup remainder; ...
    "w2_l1": lambda: make(41, 2, 1),
    "w2_l5": lambda: make(42, 2, 5),
    "w16_l17_full": lambda: make(43, 16, 17),
    "w16_l33_ragged": lambda: make(44, 16, 33, "ragged"),
    "w16_l64_missing_huber": lambda: make(45, 16, 64, "missing", huber_px=2.0, outliers=0.05),
}
SEEDS = list(CASES)[:8]                                    # the adjustment's seeds
NOISE_FREE = {name + "_exact": (lambda name=name: noise_free(get(name))) for name in list(CASES)}
CASES.update(NOISE_FREE)
CASES["bad_landmarks"] = _bad_landmarks
CASES["zero_parallax"] = _zero_parallax
SOLVED = list(CASES)                                       # compared after max_iter 2, 4 and 50
WINDOW_REFUSED = {"csr_does_not_end_at_m": lambda: _window_refused("csr"), "non_finite_pose": lambda: _window_refused("pose")}
# noisy windows on which the refinement must bring the landmarks closer to the generating ones (not the squared loss with
# gross outliers, which keeps them)
NOISY = tuple(n for n in SEEDS if n != "w8_l60_outliers_squared")
GATED = ("w8_l60_outliers_huber", "w8_l60_outliers_squared")
GATE_PX = 2.0
BATCH = ("w8_l60_outliers_squared", None, "w8_l600")       # S = 3, one W: different sizes, the middle window empty

_cache, _solved = {}, {}


def get(name):
    """The case (built once; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = (CASES.get(name) or WINDOW_REFUSED[name])()
    return _cache[name]


def without_bad():
    if "without_bad" not in _cache:
        c = get("bad_landmarks")
        _cache["without_bad"] = _without(c, c.bad)
    return _cache["without_bad"]


def params(name, max_iter=0, gate_px=0.0):
    c = get(name)
    return dict(huber_px=c.huber_px, max_iter=max_iter, gate_px=gate_px, min_parallax=getattr(c, "min_parallax", 0.0))


def definition(name, max_iter, gate_px=0.0, perm=None):
    """The definition's result for a case (cached for the natural order)."""
    if name == "without_bad":
        win, prm = without_bad().win, params("bad_landmarks", max_iter, gate_px)
    else:
        win, prm = get(name).win, params(name, max_iter, gate_px)
    if perm is not None:
        return sref.solve(win, perm=perm, **prm)
    key = (name, max_iter, gate_px)
    if key not in _solved:
        _solved[key] = sref.solve(win, **prm)
    return _solved[key]


def landmark_rms(case, X, rows=None):
    """RMS distance of the landmarks (all, or `rows`) from the generating ones."""
    d = np.asarray(X) - case.true_X
    if rows is not None:
        d = d[rows]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def scipy_costs(name):
    """Per landmark, the cost SciPy's least_squares reaches on the same objective from the same start (tolerances 1e-15,
    x_scale='jac', analytic Jacobian); NaN for a refused landmark.  Cached."""
    key = (name, "scipy")
    if key in _solved:
        return _solved[key]
    from scipy.optimize import least_squares
    c = get(name)
    win = c.win
    d = definition(name, 50)
    out = np.full(len(win.X), np.nan)
    for i in np.flatnonzero(d.status != sref.STATUS_REFUSED):
        s, e = int(win.lm_start[i]), int(win.lm_start[i + 1])
        sub = types.SimpleNamespace(K=win.K, lm_start=np.array([0, e - s]), obs_slot=win.obs_slot[s:e], obs_xy=win.obs_xy[s:e])

        def scale(e2, rho):
            r2 = np.sum(e2 * e2, axis=1)
            return np.sqrt(rho / np.where(r2 > 0.0, r2, 1.0))

        def fun(x):
            _, e2, rho, _ = wc.ref.residuals(sub, win.poses, x[None], c.huber_px)
            return (e2 * scale(e2, rho)[:, None]).reshape(-1)

        def jac(x):
            p, e2, rho, _ = wc.ref.residuals(sub, win.poses, x[None], c.huber_px)
            _, Jl = wc.ref.jacobians(sub, win.poses, p)
            sc = scale(e2, rho)
            D = -sc[:, None, None] * np.eye(2)[None]
            if c.huber_px > 0.0:                              # f = s(e) e: d f = -(s I + e ds/de^T) J (window_ba_cases.scipy_cost)
                dl = c.huber_px
                r = np.sqrt(np.sum(e2 * e2, axis=1))
                big = r > dl
                rb = np.where(big, r, 1.0)
                sb = np.sqrt(np.maximum(2.0 * dl * rb - dl * dl, 0.0))
                ds = np.where(big, (dl / np.where(big, sb, 1.0)) / rb - sb / (rb * rb), 0.0) / rb
                D = D - ds[:, None, None] * np.einsum("mi,mj->mij", e2, e2)
            return np.einsum("mik,mkj->mij", D, Jl).reshape(-1, 3)

        r = least_squares(fun, win.X[i].copy(), jac=jac, x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, method="trf",
                          max_nfev=400)
        out[i] = 2.0 * r.cost
    _solved[key] = out
    return out


def empty_window(W):
    return wc.empty_window(W)
