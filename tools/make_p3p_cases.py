#!/usr/bin/env python
"""Writes tests/golden/p3p_cases.npz: P3P cases with their solution sets from an independent solver.

    python tools/make_p3p_cases.py [--jobs 8]

CPU only; needs mpmath.  tests/test_p3p_reference_host.py regenerates a share of the table with this module and
compares, so the committed file is what this file writes.

The reference solver (ref_solutions) shares nothing with oracle/csrc/p3p.c but the statement of the problem: depth
ratios u = s2/s1, v = s3/s1 of the first three points obey two quadratics in u whose coefficients are polynomials
in v.  It works in mpmath at 60 digits, eliminates u by the resultant of the two quadratics (never through the
rational step u = Nn/Dd of the oracle), takes every root of the resultant with polyroots, and for each real v > 0
takes both roots u of the first quadratic and keeps those that also satisfy the second.  Each (u, v) gives a pose
by aligning the two point triads; the poses are ranked by the squared reprojection error of the fourth point.

Every case is built from its index alone (make_case), each family for the branch of the solver it is named after;
the builder checks on the oracle's own intermediate quantities, recomputed here in Python floats in the oracle's
operation order (oracle_quantities), that the branch is really reached.

Family `biquadratic` (depressed quartic with q == 0 exactly in double): reached by construction, not by search --
a right isosceles world triangle (d12 = d23, d12^2 / d13^2 = 1/2 exactly) whose hypotenuse ends are seen along
(2, 0, 1) and (-1/2, 0, 1), so that c13 == 0 exactly; then the odd coefficients of the quartic cancel term by term
in double.  Only intrinsics whose (pixel - c) / f comes out at exactly 2 and -1/2 take part.

Left out on purpose: the far, tiny triangle (1e-3 wide at distance 80) -- ill-conditioned beyond what fp64 can
select, no target for the solver.  No case is constructed for a leading coefficient `c4 == 0` exactly.
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "p3p_cases.npz")
SEED = 20261018
DD_REL = 1e-4          # oracle/csrc/p3p.c: P3P_DD_REL

KS = np.array([
    [[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]],
    [[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]],
    [[2759.48, 0, 1520.69], [0, 2764.16, 1006.81], [0, 0, 1]],
])

FAMILIES = ("generic", "outlier", "symmetric", "biquadratic", "rejects", "edges")


# ------------------------------------------------------------------ the reference solver
def ref_solutions(X4, x4, K, dps=60):
    """(poses, vroots): poses = [(R 3x3, t 3, e4, u, v)] as float64 sorted by e4 (the squared reprojection error of
    the fourth point, px^2), vroots = the positive real roots v of the resultant, ascending, repeated roots repeated."""
    import mpmath as mp
    mp.mp.dps = dps
    tiny = mp.mpf(10) ** -25
    F = lambda v: mp.mpf(float(v))
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    P = [mp.matrix([F(c) for c in X4[i]]) for i in range(4)]
    f = []
    for i in range(3):
        m = mp.matrix([(F(x4[i][0]) - cx) / fx, (F(x4[i][1]) - cy) / fy, 1])
        f.append(m / mp.norm(m))
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    c12, c13, c23 = dot(f[0], f[1]), dot(f[0], f[2]), dot(f[1], f[2])
    d12, d13, d23 = dot(P[0] - P[1], P[0] - P[1]), dot(P[0] - P[2], P[0] - P[2]), dot(P[1] - P[2], P[1] - P[2])
    if d12 == 0 or d13 == 0 or d23 == 0:
        return [], []

    def cross(a, b):
        return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    def frame(p1, p2, p3):
        e1 = p2 - p1
        e1 = e1 / mp.norm(e1)
        e3 = cross(e1, p3 - p1)
        if mp.norm(e3) == 0:
            return None
        e3 = e3 / mp.norm(e3)
        e2 = cross(e3, e1)
        return mp.matrix([[e1[r], e2[r], e3[r]] for r in range(3)])

    Ew = frame(P[0], P[1], P[2])
    if Ew is None:
        return [], []
    a, b = d12 / d13, d23 / d13

    def padd(p, q):
        n = max(len(p), len(q))
        return [(p[i] if i < len(p) else 0) + (q[i] if i < len(q) else 0) for i in range(n)]

    def pmul(p, q):
        r = [mp.mpf(0)] * (len(p) + len(q) - 1)
        for i, pi in enumerate(p):
            for j, qj in enumerate(q):
                r[i + j] += pi * qj
        return r

    psc = lambda p, s: [s * c for c in p]
    # E1: u^2 + A1 u + A0 = 0, E2: u^2 + B1 u + B0 = 0 (coefficients low -> high in v), qv = v^2 - 2 c13 v + 1;
    # resultant of two monic quadratics: (A0 - B0)^2 + (A1 - B1) (A1 B0 - A0 B1)
    qv = [mp.mpf(1), -2 * c13, mp.mpf(1)]
    A0, A1 = padd([mp.mpf(1)], psc(qv, -a)), [-2 * c12]
    B0, B1 = padd([0, 0, mp.mpf(1)], psc(qv, -b)), [0, -2 * c23]
    D0, D1 = padd(A0, psc(B0, -1)), padd(A1, psc(B1, -1))
    res = padd(pmul(D0, D0), pmul(D1, padd(pmul(A1, B0), psc(pmul(A0, B1), -1))))
    while len(res) > 1 and abs(res[-1]) < mp.mpf(10) ** -50:
        res.pop()
    if len(res) < 2:
        return [], []
    roots = mp.polyroots(res[::-1], maxsteps=500, extraprec=400)
    vs = sorted(mp.re(v) for v in roots if abs(mp.im(v)) <= tiny and mp.re(v) > 0)
    sols = []
    for v in vs:
        q = v * v - 2 * c13 * v + 1
        disc = c12 * c12 - (1 - a * q)
        if disc < 0:
            if disc < -tiny:
                continue
            disc = mp.mpf(0)
        for sg in (1, -1):
            u = c12 + sg * mp.sqrt(disc)
            if u <= 0:
                continue
            if abs(u * u - 2 * c23 * v * u + v * v - b * q) > mp.mpf(10) ** -20 * (1 + u * u + v * v):
                continue
            s1 = mp.sqrt(d13 / q)
            C = [s1 * f[0], u * s1 * f[1], v * s1 * f[2]]
            Ec = frame(*C)
            if Ec is None:
                continue
            R = Ec * Ew.T
            t = C[0] - R * P[0]
            Xc = R * P[3] + t
            if Xc[2] == 0:
                continue
            e = (F(x4[3][0]) - (Xc[0] / Xc[2] * fx + cx)) ** 2 + (F(x4[3][1]) - (Xc[1] / Xc[2] * fy + cy)) ** 2
            if not any(mp.norm(R - s_[0]) < mp.mpf(10) ** -12 for s_ in sols):
                sols.append((R, t, e, u, v))
    sols.sort(key=lambda s: s[2])
    poses = [(np.array([[float(R[i, j]) for j in range(3)] for i in range(3)]), np.array([float(t[i]) for i in range(3)]),
              float(e), float(u), float(v)) for R, t, e, u, v in sols]
    return poses, [float(v) for v in vs]


# ------------------------------------------------------------------ the oracle's intermediate quantities
def oracle_quantities(X4, x4, K):
    """What oracle/csrc/p3p.c computes before its roots, in Python floats (IEEE double, no contraction) and in its
    operation order: the squared distances, the cosines, the quartic, the depressed quartic's p, q, r, the norm of
    the world triad's normal; dd_rel(v) is the quantity the vanishing-denominator test looks at."""
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    f = []
    for i in range(3):
        mu, mv = (float(x4[i][0]) - cx) / fx, (float(x4[i][1]) - cy) / fy
        nrm = math.sqrt(mu * mu + mv * mv + 1.0)
        f.append((mu / nrm, mv / nrm, 1.0 / nrm))
    P = [[float(c) for c in X4[i]] for i in range(3)]
    d12s = d13s = d23s = 0.0
    for k in range(3):
        a_, b_, c_ = P[0][k] - P[1][k], P[0][k] - P[2][k], P[1][k] - P[2][k]
        d12s += a_ * a_
        d13s += b_ * b_
        d23s += c_ * c_
    out = dict(d12s=d12s, d13s=d13s, d23s=d23s, n3=None, q=None, c4=None)
    if not (d12s > 0.0 and d13s > 0.0 and d23s > 0.0):
        return out
    dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
    c12, c13, c23 = dot(f[0], f[1]), dot(f[0], f[2]), dot(f[1], f[2])
    a, b = d12s / d13s, d23s / d13s
    g = a - b
    n2, n1, n0 = 1.0 + g, -2.0 * g * c13, g - 1.0
    e1, e0 = 2.0 * c23, -2.0 * c12
    w2, w1, w0 = -a, 2.0 * a * c13, 1.0 - a
    dd2, dd1, dd0 = e1 * e1, 2.0 * e1 * e0, e0 * e0
    nd3, nd2, nd1, nd0 = n2 * e1, n2 * e0 + n1 * e1, n1 * e0 + n0 * e1, n0 * e0
    tc = 2.0 * c12
    c = [0.0] * 5
    c[4] = n2 * n2 + w2 * dd2
    c[3] = 2.0 * n2 * n1 - tc * nd3 + (w2 * dd1 + w1 * dd2)
    c[2] = (2.0 * n2 * n0 + n1 * n1) - tc * nd2 + (w2 * dd0 + w1 * dd1 + w0 * dd2)
    c[1] = 2.0 * n1 * n0 - tc * nd1 + (w1 * dd0 + w0 * dd1)
    c[0] = n0 * n0 - tc * nd0 + w0 * dd0
    def fallback(v):
        """(ua, ub, ra, rb) of the vanishing-denominator step at root v: the two roots of the first quadratic and
        what each leaves of the second"""
        qv = (v - 2.0 * c13) * v + 1.0
        disc = c12 * c12 - (1.0 - a * qv)
        if disc < 0.0:
            return None
        sq = math.sqrt(disc)
        ua, ub = c12 + sq, c12 - sq
        k1, k0 = 2.0 * c23 * v, v * v - b * qv
        return ua, ub, abs((ua - k1) * ua + k0), abs((ub - k1) * ub + k0)

    out.update(c12=c12, c13=c13, c23=c23, a=a, b=b, coef=c, c4=c[4], fallback=fallback,
               dd_rel=lambda v: abs(e1 * v + e0) / (abs(e1 * v) + abs(e0)))
    if c[4] != 0.0:
        a3, a2, a1, a0 = c[3] / c[4], c[2] / c[4], c[1] / c[4], c[0] / c[4]
        a3sq = a3 * a3
        out["p"] = a2 - 0.375 * a3sq
        out["q"] = a1 - 0.5 * a2 * a3 + 0.125 * a3sq * a3
        out["r"] = a0 - 0.25 * a1 * a3 + 0.0625 * a2 * a3sq - (3.0 / 256.0) * a3sq * a3sq
    # triad(): e1 = (P2 - P1) / |.|, e3 = e1 x (P3 - P1)
    av = [P[1][k] - P[0][k] for k in range(3)]
    bv = [P[2][k] - P[0][k] for k in range(3)]
    na = math.sqrt(av[0] * av[0] + av[1] * av[1] + av[2] * av[2])
    ev = [av[k] / na for k in range(3)]
    e3 = [ev[1] * bv[2] - ev[2] * bv[1], ev[2] * bv[0] - ev[0] * bv[2], ev[0] * bv[1] - ev[1] * bv[0]]
    out["n3"] = math.sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2])
    return out


# ------------------------------------------------------------------ scenes
def rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_of(R):
    """unit quaternion (w, x, y, z) of a rotation, largest component positive (Shepperd)"""
    t = np.trace(R)
    c = [t, R[0, 0], R[1, 1], R[2, 2]]
    i = int(np.argmax(c))
    if i == 0:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2 * R[0, 0] - t, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2 * R[1, 1] - t, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2 * R[2, 2] - t])
    return q / np.linalg.norm(q)


def rot_of(q):
    """rotations of unit quaternions (..., 4) -> (..., 3, 3)"""
    w, x, y, z = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


# the sweep deltas at which rounding loses the double root in the quartic stage (a discriminant that should be 0
# comes out negative): the solver then returns another true pose, and the best one is not demanded there
LOST_ROOT = (1e-8, 1e-10, 1e-11)
ALT_DELTAS = (0.0, 1e-3, 1e-5, 1e-7)


def demand_best(fam, sub):
    """Cases that are not `well separated` (their double root, or pair of close roots) and whose best pose is
    demanded all the same: they are what decides how the vanishing-denominator step picks among the two roots of
    the first quadratic."""
    if fam != "symmetric" or not (sub.startswith("equi_d") or sub.startswith("equi_alt_d")):
        return False
    return float(sub.split("_d")[1]) not in LOST_ROOT


def project(K, Xc):
    """pixels of camera-frame points; the depth may be negative (cv2.projectPoints forms the projection anyway)"""
    return np.stack([Xc[:, 0] / Xc[:, 2] * K[0, 0] + K[0, 2], Xc[:, 1] / Xc[:, 2] * K[1, 1] + K[1, 2]], axis=1)


def frustum_points(rng, depth, n=4):
    return np.stack([rng.uniform(-.6, .6, n) * depth, rng.uniform(-.4, .4, n) * depth, rng.uniform(.3, 1.5, n) * depth], 1)


def world_of(rng, Xc, t_scale=5.0):
    """world points of which Xc are the camera-frame images under a random pose"""
    R, t = rand_rot(rng), rng.normal(size=3) * t_scale
    return (Xc - t) @ R


def look_at(C, target, roll):
    """world->camera rotation of a camera at C whose optical axis passes through `target`"""
    z = target - C
    z /= np.linalg.norm(z)
    h = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x0 = np.cross(h, z)
    x0 /= np.linalg.norm(x0)
    y0 = np.cross(z, x0)
    x = math.cos(roll) * x0 + math.sin(roll) * y0
    y = np.cross(z, x)
    return np.stack([x, y, z])


EQUI = np.array([[1.0, 0, 0], [-.5, math.sqrt(3) / 2, 0], [-.5, -math.sqrt(3) / 2, 0], [.3, .2, .5]])
ISOS = np.array([[0.0, 1, 0], [-1.0, 0, 0], [1.0, 0, 0], [.3, .2, .5]])
RIGHT = np.array([[-1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0], [.3, -.4, .5]])       # d12 = d23, d12^2 / d13^2 = 1/2
DELTAS = [0.0] + [10.0 ** -k for k in range(1, 13)]


def _generic(k, rng):
    Kid, depth, noise = k % 3, (2.0, 10.0, 60.0)[(k // 3) % 3], (0.0, 0.3)[(k // 9) % 2]
    Xc = frustum_points(rng, depth)
    X = world_of(rng, Xc)
    x = project(KS[Kid], Xc)
    if noise:
        x = x + rng.normal(0, noise, x.shape)
    return "n%g" % noise, Kid, X, x


def _outlier(k, rng):
    _, Kid, X, x = _generic(k, rng)
    ang, r = rng.uniform(0, 2 * math.pi), rng.uniform(200, 800)
    x[k % 3] += r * np.array([math.cos(ang), math.sin(ang)])
    return "pix%d" % (k % 3), Kid, X, x


def _symmetric(k, rng):
    if k < 13:                         # the equilateral triangle from above its centroid, moved sideways by delta
        d = DELTAS[k]
        return "equi_d%g" % d, 0, EQUI.copy(), project(KS[0], EQUI + np.array([d, 0.3 * d, 4.0]))
    k -= 13
    if k < 20:                         # the same after a rigid motion of the world, other intrinsics
        d = (0.0, 1e-2, 1e-4, 1e-6, 1e-9)[k % 5]
        Kid = 1 + (k // 5) % 2
        Xc = EQUI + np.array([d, 0.3 * d, 4.0])
        return "equi_moved_d%g" % d, Kid, world_of(rng, Xc, 3.0), project(KS[Kid], Xc)
    k -= 20
    if k >= 18:
        # the equilateral sweep again, the fourth pixel taken from the OTHER pose of the (near-)double root: the three
        # points look the same, the best pose is now the one with the smaller root u of the first quadratic
        d = ALT_DELTAS[k - 18]
        x = project(KS[0], EQUI + np.array([d, 0.3 * d, 4.0]))
        poses, _ = ref_solutions(EQUI, x, KS[0])
        assert poses[0][2] < 1e-20
        j = min(range(1, len(poses)), key=lambda j: abs(poses[j][4] - poses[0][4]))
        x[3] = project(KS[0], (EQUI[3:] @ poses[j][0].T + poses[j][1]))[0]
        return "equi_alt_d%g" % d, 0, EQUI.copy(), x
    # the isosceles triangle seen from above a point of its axis
    y0, h, Kid = (0.0, 1.0 / 3.0, 0.5)[k % 3], (3.0, 4.0)[(k // 3) % 2], (k // 6) % 3
    return "isos_y%g_h%g" % (y0, h), Kid, ISOS.copy(), project(KS[Kid], ISOS + np.array([0.0, -y0, h]))


N_BIQ_TRY = 12


def _biquadratic(k, rng):
    # camera frame: P1 = s1 (2, 0, 1), P3 = s3 (-1/2, 0, 1) (perpendicular rays), |P1 - P3| = 2, P2 at distance
    # sqrt(2) from both, turned by phi about the axis P1 P3; pixels 1 and 3 are set exactly
    Kid = k % 3
    s1 = (0.5, 0.6, 0.7, 0.8)[(k // 3) % 4]
    phi = (0.4, 1.1, 2.0)[k % 3] + 0.3 * (k // 3)
    s3 = math.sqrt((4.0 - 5.0 * s1 * s1) / 1.25)
    C1, C3 = s1 * np.array([2.0, 0, 1]), s3 * np.array([-.5, 0, 1])
    ex = (C3 - C1) / 2.0
    ey = np.cross(ex, [0.0, 1.0, 0.0])
    ey /= np.linalg.norm(ey)
    ez = np.cross(ex, ey)
    ey, ez = math.cos(phi) * ey + math.sin(phi) * ez, -math.sin(phi) * ey + math.cos(phi) * ez
    Rwc = np.stack([ex, ey, ez], axis=1)                 # world axes in the camera frame
    Xc = RIGHT @ Rwc.T + (C1 + C3) / 2.0
    K = KS[Kid]
    x = project(K, Xc)
    x[0] = [K[0, 2] + 2.0 * K[0, 0], K[1, 2]]
    x[2] = [K[0, 2] - 0.5 * K[0, 0], K[1, 2]]
    return "s%g" % s1, Kid, RIGHT.copy(), x


def _rejects(k, rng):
    Kid = k % 3
    Xc = frustum_points(rng, 10.0)
    if k < 6:                          # a repeated index in the first three
        i, j = ((0, 1), (0, 2), (1, 2))[k % 3]
        Xc[j] = Xc[i]
        X = world_of(rng, Xc)
        X[j] = X[i]
        x = project(KS[Kid], Xc)
        x[j] = x[i]
        return "repeat%d%d" % (i, j), Kid, X, x
    k -= 6
    if k < 6:                          # collinear world points, exactly so in double
        base = np.array([[0.0, 0, 0], [1.0, 1, 1], [2.5, 2.5, 2.5]]) if k % 2 == 0 else np.array(
            [[-1.0, 2, 0], [0.5, 2, 0], [3.0, 2, 0]])
        X = np.vstack([base, rng.uniform(-1, 1, (1, 3))])
        R, t = rand_rot(rng), np.array([0.3, -0.2, 8.0])
        return "collinear%d" % (k % 2), Kid, X, project(KS[Kid], X @ R.T + t)
    k -= 6
    i = k % 3                          # the fourth point repeats one of the three: valid, error 0
    X = world_of(rng, Xc)
    x = project(KS[Kid], Xc)
    X[3], x[3] = X[i], x[i]
    return "fourth_is_%d" % i, Kid, X, x


def _edges(k, rng):
    Kid = k % 3
    K = KS[Kid]
    if k < 6:                          # a sampled point on the optical axis: its pixel is the principal point
        i = k % 3
        Xc = frustum_points(rng, 10.0)
        Xc[i, :2] = 0.0
        x = project(K, Xc)
        x[i] = [K[0, 2], K[1, 2]]
        return "on_axis%d" % i, Kid, world_of(rng, Xc), x
    k -= 6
    if k < 6:                          # the fourth point behind the camera
        Xc = frustum_points(rng, 10.0)
        Xc[3, 2] = -rng.uniform(1.0, 8.0)
        return "fourth_behind", Kid, world_of(rng, Xc), project(K, Xc)
    k -= 6
    if k < 6:                          # world coordinates offset by 1e4
        Xc = frustum_points(rng, 10.0)
        R = rand_rot(rng)
        t = -R @ (1e4 * np.array([1.0, -0.7, 0.4])) + rng.normal(size=3)
        return "offset1e4", Kid, (Xc - t) @ R, project(K, Xc)
    k -= 6
    if k >= 9:
        # Nn and Dd nearly vanish together without any symmetry: sample (929, 391, 513, 681) of the 1000-point scene of
        # tests/test_oracle_geometry.py (hypothesis 584 of test_p3p_hypotheses_match_oracle[1000-1000-0.0]), where
        # |Dd| is 4.7e-5 of its terms and u = Nn / Dd left the pose 3.3e-6 off the reference's
        g = np.random.default_rng(1005)
        th1, th2 = np.pi / 8, np.pi / 32
        R = np.array([[np.cos(th1), -np.sin(th1), 0], [np.sin(th1), np.cos(th1), 0], [0, 0, 1]]) @ np.array(
            [[np.cos(th2), 0, np.sin(th2)], [0, 1, 0], [-np.sin(th2), 0, np.cos(th2)]])
        Xs = g.uniform(-1, 1, size=(1000, 3))
        Xs[:, 2] = Xs[:, 2] * 5 + 10
        X = Xs[[929, 391, 513, 681]]
        xh = (X @ R.T + np.array([1.0, 1.0, -1.0])) @ KS[0].T
        return "small_dd", 0, X, xh[:, :2] / xh[:, 2:]
    # the camera centre on the danger cylinder: the circular cylinder through the three points, axis along the
    # normal of their plane.  The true pose is a double solution there, and the rounding of the pixels to double
    # either splits it into two real ones 1e-8 apart or into a complex pair -- in which case the problem as
    # stated has no solution near the true pose at all, and a solver that returns the real part (backward error
    # 1e-9 px) is as right as one that does not.  Only the first kind is a case: draw until the solution is real.
    for _ in range(64):
        X = rng.uniform(-1, 1, (4, 3)) * 2.0
        A, B, Cc = X[0], X[1], X[2]
        n = np.cross(B - A, Cc - A)
        n /= np.linalg.norm(n)
        ab, ac = B - A, Cc - A
        O = A + (np.dot(ac, ac) * np.cross(np.cross(ab, ac), ab) + np.dot(ab, ab) * np.cross(ac, np.cross(ab, ac))) / (
            2.0 * np.dot(np.cross(ab, ac), np.cross(ab, ac)))
        r = np.linalg.norm(A - O)
        ea = (A - O) / r
        eb = np.cross(n, ea)
        th, h = rng.uniform(0.3, 1.8), rng.uniform(4.0, 9.0)          # (not at a vertex: theta = 0 is A itself)
        C = O + r * (math.cos(th) * ea + math.sin(th) * eb) + h * n
        R = look_at(C, X[:3].mean(axis=0), rng.uniform(0, 2 * math.pi))
        x = project(K, (X - C) @ R.T)
        poses, _ = ref_solutions(X, x, K)
        if poses and poses[0][2] < 1e-6:
            return "danger_cylinder", Kid, X, x
    raise AssertionError("no danger-cylinder case with a real solution")


BUILDERS = {"generic": (_generic, 1500), "outlier": (_outlier, 150), "symmetric": (_symmetric, 13 + 20 + 18 + len(ALT_DELTAS)),
            "biquadratic": (_biquadratic, N_BIQ_TRY), "rejects": (_rejects, 6 + 6 + 9), "edges": (_edges, 6 + 6 + 6 + 9 + 1)}


def case_list():
    """[(family, k)] of the table, in order"""
    out = []
    for fam in FAMILIES:
        for k in range(BUILDERS[fam][1]):
            out.append((fam, k))
    return out


def make_case(fam, k):
    """One row of the table, from (family, k) alone; None where a `biquadratic` attempt misses q == 0 in double."""
    rng = np.random.default_rng([SEED, FAMILIES.index(fam), k])
    sub, Kid, X, x = BUILDERS[fam][0](k, rng)
    X, x = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(x, np.float64)
    K = KS[Kid]
    oq = oracle_quantities(X, x, K)
    if fam == "biquadratic" and oq["q"] != 0.0:
        return None
    poses, vs = ref_solutions(X, x, K)
    # --- the branch the case is there for is reached
    if fam == "biquadratic":
        assert oq["q"] == 0.0 and oq["c13"] == 0.0
    if fam == "rejects":
        if sub.startswith("repeat"):
            assert min(oq["d12s"], oq["d13s"], oq["d23s"]) == 0.0 and not poses
        elif sub.startswith("collinear"):
            assert oq["n3"] == 0.0 and not poses
        else:
            assert poses and poses[0][2] < 1e-40, "the repeated fourth point has error 0"
    if fam == "symmetric" and sub.startswith("equi"):
        d = float(sub.split("_d")[1])
        if d <= 1e-4:                  # the rational step's denominator vanishes at a root of the reference
            assert min(oq["dd_rel"](v) for v in vs) < DD_REL, sub
        if "moved" not in sub and d <= 1e-3:
            # what the step has to decide at the best pose's root: which root of the first quadratic
            ub, vb = poses[0][3:5]
            ua_, ub_, ra, rb = oq["fallback"](vb)
            assert oq["dd_rel"](vb) < DD_REL
            needs_b = abs(ub - ub_) < abs(ub - ua_)
            assert needs_b == sub.startswith("equi_alt"), sub
            if d >= 1e-4:              # the residual decides: only the root that belongs fits the second quadratic
                assert (rb if needs_b else ra) < 1e-9 and (ra if needs_b else rb) > 1e-6, (sub, ra, rb)
            else:                      # both fit to 1e-6: the parity rule decides
                assert ra < 1e-6 and rb < 1e-6, (sub, ra, rb)
    if fam == "symmetric" and sub.startswith("isos"):
        assert len(poses) == 4, (sub, len(poses))
    if fam == "edges" and sub.startswith("on_axis"):
        i = int(sub[-1])
        assert x[i][0] == K[0, 2] and x[i][1] == K[1, 2]
    if fam == "edges" and sub == "fourth_behind":
        assert poses, sub
        R, t = poses[0][:2]
        assert (R @ X[3] + t)[2] < 0.0, "the fourth point lies behind the camera of the best pose"
    if fam == "edges" and sub == "danger_cylinder":   # the double solution: two roots that rounding alone separates
        assert min(abs(vs[i + 1] - vs[i]) / vs[i] for i in range(len(vs) - 1)) < 1e-6, sub
    if fam == "edges" and sub == "small_dd":
        assert poses and min(oq["dd_rel"](v) for v in vs) < DD_REL, sub
    if fam == "edges" and sub == "offset1e4":
        assert np.abs(X).max() > 5e3
    row = dict(family=fam, sub=sub, K_index=Kid, X=X, x=x, n_sol=len(poses), R=np.zeros((4, 3, 3)), q=np.zeros((4, 4)),
               t=np.zeros((4, 3)), demand_best=demand_best(fam, sub),
               e4=np.zeros(4), n_v=len(vs), v=np.zeros(4))
    assert len(poses) <= 4 and len(vs) <= 4
    for j, (R, t, e, _, _) in enumerate(poses):
        row["R"][j], row["q"][j], row["t"][j], row["e4"][j] = R, quat_of(R), t, e
    row["v"][:len(vs)] = vs
    # its only positive root is double to within 1e-6: rounding may lose it (a discriminant that should be 0 goes
    # negative), the solver then rightly or wrongly reports no pose -- conditioning, not a defect
    row["conditioning"] = bool(len(vs) >= 2 and (max(vs) - min(vs)) <= 1e-6 * max(vs))
    return row


def _job(fk):
    return make_case(*fk)


def build_table(jobs=1):
    todo = case_list()
    if jobs > 1:
        import multiprocessing as mpc
        with mpc.Pool(jobs) as pool:
            rows = pool.map(_job, todo, chunksize=8)
    else:
        rows = [make_case(f, k) for f, k in todo]
    kept = [(fk, r) for fk, r in zip(todo, rows) if r is not None]
    rows = [r for _, r in kept]
    tab = dict(K_table=KS, family=np.array([r["family"] for r in rows]), sub=np.array([r["sub"] for r in rows]),
               k=np.array([fk[1] for fk, _ in kept], np.int32), K_index=np.array([r["K_index"] for r in rows], np.int32),
               X=np.stack([r["X"] for r in rows]), x=np.stack([r["x"] for r in rows]),
               n_sol=np.array([r["n_sol"] for r in rows], np.int32), q=np.stack([r["q"] for r in rows]),
               demand_best=np.array([r["demand_best"] for r in rows], bool),
               t=np.stack([r["t"] for r in rows]), e4=np.stack([r["e4"] for r in rows]),
               n_v=np.array([r["n_v"] for r in rows], np.int32), v=np.stack([r["v"] for r in rows]),
               conditioning=np.array([r["conditioning"] for r in rows], bool))
    return tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    tab = build_table(a.jobs)
    fam = tab["family"]
    for f in FAMILIES:
        m = fam == f
        print("%-12s %5d cases, solutions 0/1/2/3/4: %s, conditioning: %d" % (
            f, m.sum(), np.bincount(tab["n_sol"][m], minlength=5).tolist(), tab["conditioning"][m].sum()))
    if not (fam == "biquadratic").any():
        print("biquadratic: q == 0 is not reached in double; the family is dropped")
    np.savez_compressed(a.out, **tab)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    sys.exit(main())
