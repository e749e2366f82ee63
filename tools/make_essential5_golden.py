"""Writes tests/golden/essential5_cases.npz: the five-point case table with its 50-digit solution sets.

    python tools/make_essential5_golden.py

Every case is five correspondences (pixels) with two pinhole cameras.  Its complete set of real essential matrices is
computed with mpmath (100 digits of working precision, 50 kept) by a route of its own -- the null space from mpmath's QR, the ten cubic constraints by
exact polynomial arithmetic on dictionaries, the elimination by mpmath's matrix inverse, the roots of the degree-10 polynomial
by mpmath.polyroots with its error bound -- so nothing of the float64 rule (tests/essential5_reference.py) decides what
the set is.  Stored per case: the inputs, the set as decimal strings (E50) and as float64 (E), the ground-truth E, and
two separation figures: the smallest relative gap between neighbouring real roots in z and the smallest |Im| / |z| over
the complex roots.  The generator is seeded; for the families marked separated a case is redrawn until both figures
exceed ROOT_GAP, so no test has to leave a case out."""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import essential5_cases as cases  # noqa: E402
import essential5_reference as ref  # noqa: E402

mp.mp.dps = 100           # the working precision; the table keeps 50 digits of every entry
ROOT_GAP = cases.ROOT_GAP
SEED = 20041


def mp_solution_set(x1, x2, K1, K2):
    """(list of E (mp.matrix 3x3, canonical), gap between real roots, smallest relative imaginary part)"""
    h1, h2 = cases.mp_normalise(K1, x1), cases.mp_normalise(K2, x2)
    A = mp.matrix(5, 9)
    for k in range(5):
        for a in range(3):
            for b in range(3):
                A[k, 3 * a + b] = h1[k][a] * h2[k][b]
    Q, _ = mp.qr(A.T, mode="full")
    basis = [[Q[r, 5 + j] for r in range(9)] for j in range(4)]
    # E[r][c] as a linear form {monomial exponents (i, j, k): coefficient}
    var = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]

    def lin(r, c):
        return {var[v]: basis[v][3 * c + r] for v in range(4)}

    def pmul(p, q):
        out = {}
        for m1, c1 in p.items():
            for m2, c2 in q.items():
                m = (m1[0] + m2[0], m1[1] + m2[1], m1[2] + m2[2])
                out[m] = out.get(m, mp.mpf(0)) + c1 * c2
        return out

    def padd(p, q, s=1):
        out = dict(p)
        for m, c in q.items():
            out[m] = out.get(m, mp.mpf(0)) + s * c
        return out

    def pscale(p, s):
        return {m: s * c for m, c in p.items()}

    E = [[lin(r, c) for c in range(3)] for r in range(3)]
    det = padd(padd(pmul(E[0][0], padd(pmul(E[1][1], E[2][2]), pmul(E[1][2], E[2][1]), -1)),
                    pmul(E[0][1], padd(pmul(E[1][0], E[2][2]), pmul(E[1][2], E[2][0]), -1)), -1),
               pmul(E[0][2], padd(pmul(E[1][0], E[2][1]), pmul(E[1][1], E[2][0]), -1)))
    G = [[padd(padd(pmul(E[i][0], E[j][0]), pmul(E[i][1], E[j][1])), pmul(E[i][2], E[j][2])) for j in range(3)] for i in range(3)]
    tr = padd(padd(G[0][0], G[1][1]), G[2][2])
    rows = [det]
    for i in range(3):
        for j in range(3):
            acc = {}
            for k in range(3):
                L = pscale(G[i][k], 2)
                if i == k:
                    L = padd(L, tr, -1)
                acc = padd(acc, pmul(L, E[k][j]))
            rows.append(acc)
    # Nister's column order as exponent triples (x, y, z)
    cols = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
            (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
    M = mp.matrix(10, 20)
    for r in range(10):
        for c in range(20):
            M[r, c] = rows[r].get(cols[c], mp.mpf(0))
    R = mp.inverse(M[:, :10]) * M[:, 10:]                # the reduced right half
    # B(z): rows (4, 5), (6, 7), (8, 9); polynomials as ascending coefficient lists
    def zp(*c):
        return list(c)

    B = []
    for i in range(3):
        e = [R[4 + 2 * i, k] for k in range(10)]
        f = [R[5 + 2 * i, k] for k in range(10)]
        row = []
        for v in range(2):
            o = 3 * v
            row.append(zp(e[o + 2], e[o + 1] - f[o + 2], e[o] - f[o + 1], -f[o]))
        row.append(zp(e[9], e[8] - f[9], e[7] - f[8], e[6] - f[7], -f[6]))
        B.append(row)

    def zmul(p, q):
        out = [mp.mpf(0)] * (len(p) + len(q) - 1)
        for a, ca in enumerate(p):
            for b, cb in enumerate(q):
                out[a + b] += ca * cb
        return out

    def zsub(p, q):
        return [a - b for a, b in zip(p, q)]

    def zadd(p, q):
        return [a + b for a, b in zip(p, q)]

    def minor(r0, r1):
        return zsub(zmul(B[r0][0], B[r1][1]), zmul(B[r0][1], B[r1][0]))

    poly = zadd(zsub(zmul(B[0][2], minor(1, 2)), zmul(B[1][2], minor(0, 2))), zmul(B[2][2], minor(0, 1)))
    roots, err = mp.polyroots(poly[::-1], maxsteps=500, extraprec=400, error=True)
    assert err < mp.mpf(10) ** -80, err
    real, imag_sep = [], mp.inf
    for z in roots:
        if abs(mp.im(z)) <= mp.mpf(10) ** -30 * max(1, abs(z)):
            real.append(mp.re(z))
        else:
            imag_sep = min(imag_sep, abs(mp.im(z)) / abs(z))
    real.sort()
    gap = mp.inf
    for a, b in zip(real[:-1], real[1:]):
        gap = min(gap, (b - a) / max(abs(a), abs(b)))
    out = []
    for z in real:
        def ev(p):
            return mp.polyval(p[::-1], z)
        Bz = [[ev(B[i][v]) for v in range(3)] for i in range(3)]
        best = None
        for r0, r1 in ((0, 1), (0, 2), (1, 2)):
            u = Bz[r0][1] * Bz[r1][2] - Bz[r0][2] * Bz[r1][1]
            v = Bz[r0][2] * Bz[r1][0] - Bz[r0][0] * Bz[r1][2]
            w = Bz[r0][0] * Bz[r1][1] - Bz[r0][1] * Bz[r1][0]
            if best is None or abs(w) > abs(best[2]):
                best = (u, v, w)
        x, y = best[0] / best[2], best[1] / best[2]
        e = [x * basis[0][k] + y * basis[1][k] + z * basis[2][k] + basis[3][k] for k in range(9)]
        Em = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                Em[r, c] = e[3 * c + r]
        out.append(cases.mp_canonical(Em))
    return out, gap, imag_sep


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(rng, family):
    """(X (5, 3) in frame 1, R, t): x2 ~ R X + t"""
    ang = np.deg2rad(rng.uniform(1.0, 30.0))
    axis = rng.normal(size=3)
    R = rodrigues(ang * axis / np.linalg.norm(axis))
    depth = rng.uniform(2.0, 20.0, 5)
    X = np.stack([rng.uniform(-0.5, 0.5, 5) * depth, rng.uniform(-0.35, 0.35, 5) * depth, depth], axis=1)
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t)
    if family == "forward":
        R = rodrigues(np.deg2rad(rng.uniform(0.2, 3.0)) * axis / np.linalg.norm(axis))
        t = np.array([0.0, 0.0, -1.0]) * rng.uniform(0.5, 1.5)
    elif family == "sideways":
        R = rodrigues(np.deg2rad(rng.uniform(0.2, 5.0)) * axis / np.linalg.norm(axis))
        t = np.array([1.0, 0.0, 0.0]) * rng.uniform(0.3, 1.0) * (1 if rng.random() < 0.5 else -1)
    elif family == "planar":
        n = rng.normal(size=3) * np.array([0.5, 0.5, 1.0])
        n = n / np.linalg.norm(n)
        d = rng.uniform(4.0, 12.0)
        rays = np.stack([rng.uniform(-0.5, 0.5, 5), rng.uniform(-0.35, 0.35, 5), np.ones(5)], axis=1)
        X = rays * (d / (rays @ n))[:, None]               # n . X = d
        if np.any(X[:, 2] < 1.0):
            return None
    elif family == "near-rotation":
        t = t * 1e-4 * depth.mean()
    X2 = X @ R.T + t
    if np.any(X2[:, 2] < 0.5):
        return None
    return X, R, t


def project(K, X):
    p = X @ K.T
    return p[:, :2] / p[:, 2:]


def essential_of(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return ref.canonical_sign(E / np.linalg.norm(E))


def main():
    rng = np.random.default_rng(SEED)
    kitti = np.load(os.path.join(ROOT, "tests", "golden", "kitti_harris.npz"))["calib_P0"][:, :3].astype(np.float64)
    cam_a = np.array([[820.0, 0.0, 645.5], [0.0, 815.0, 360.25], [0.0, 0.0, 1.0]])
    cam_b = np.array([[530.0, 0.0, 318.0], [0.0, 540.0, 242.5], [0.0, 0.0, 1.0]])
    eye = np.eye(3)
    plan = ([("generic", "generic", eye, eye, True, None)] * 24 + [("forward", "forward", eye, eye, True, None)] * 16
            + [("sideways", "sideways", eye, eye, True, None)] * 16 + [("planar", "planar", eye, eye, True, None)] * 16
            + [("pixels", "generic", kitti, kitti, True, None)] * 4 + [("pixels", "forward", kitti, kitti, True, None)] * 4
            + [("pixels", "generic", cam_a, cam_b, True, None)] * 8
            + [("few", "generic", eye, eye, True, lambda n: n == 2)] * 6
            + [("many", "generic", eye, eye, True, lambda n: n >= 6)] * 6
            + [("near-rotation", "near-rotation", eye, eye, False, None)] * 8)
    rec = {k: [] for k in ("family", "sub", "x1", "x2", "K1", "K2", "n_sol", "E", "E50", "E_true", "gap_real", "gap_imag",
                           "separated")}

    def add(family, sub, x1, x2, K1, K2, sols, Et, gap, im, separated):
        E = np.zeros((10, 3, 3))
        E50 = np.full((10, 9), b"", dtype="S60")
        for s, Em in enumerate(sols):
            for r in range(3):
                for c in range(3):
                    E[s, r, c] = float(Em[r, c])
                    E50[s, 3 * r + c] = mp.nstr(Em[r, c], 50, strip_zeros=False).encode()
        for k, v in zip(rec, (family, sub, x1, x2, K1, K2, len(sols), E, E50, Et, float(min(gap, 1e300)), float(min(im, 1e300)),
                              separated)):
            rec[k].append(v)

    for family, kind, K1, K2, separated, want in plan:
        for attempt in range(100000):
            sc = scene(rng, kind)
            if sc is None:
                continue
            X, R, t = sc
            x1, x2 = project(K1, X), project(K2, X @ R.T + t)
            if want is not None:                             # seed search in float64 first: the count, then confirmed below
                n, _, _ = ref.solve5(ref.normalise(ref.pinhole_inverse(K1), x1), ref.normalise(ref.pinhole_inverse(K2), x2))
                if not want(n):
                    continue
            sols, gap, im = mp_solution_set(x1, x2, K1, K2)
            if want is not None and not want(len(sols)):
                continue
            if separated and not (gap > ROOT_GAP and im > ROOT_GAP):
                continue
            add(family, kind, x1, x2, K1, K2, sols, essential_of(R, t), gap, im, separated)
            break
        else:
            raise RuntimeError("no case found for " + family)
        print(family, kind, len(rec["family"]), rec["n_sol"][-1], "%.2e %.2e" % (rec["gap_real"][-1], rec["gap_imag"][-1]), flush=True)

    # rejects: a repeated correspondence, all five equal, collinear points in image 1
    for sub in ("repeated", "all-equal", "collinear"):
        for _ in range(2):
            while True:
                sc = scene(rng, "generic")
                if sc is not None:
                    break
            X, R, t = sc
            if sub == "repeated":
                X[3] = X[1]
            elif sub == "all-equal":
                X[:] = X[0]
            else:
                d = X[1] - X[0]
                for k in range(2, 5):
                    X[k] = (X[0] + rng.uniform(-1.0, 2.0) * d) * rng.uniform(0.6, 1.5)      # same image line, other depths
            x1, x2 = project(eye, X), project(eye, X @ R.T + t)
            add("rejects", sub, x1, x2, eye, eye, [], essential_of(R, t), 0.0, 0.0, False)
    out = {k: np.array(v) for k, v in rec.items()}
    out["family"] = out["family"].astype("S16")
    out["sub"] = out["sub"].astype("S16")
    path = os.path.join(ROOT, "tests", "golden", "essential5_cases.npz")
    np.savez_compressed(path, **out)
    print(len(rec["family"]), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
