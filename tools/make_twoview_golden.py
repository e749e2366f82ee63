"""Writes tests/golden/twoview_cases.npz: the 8-point rule and the DLT (include/vo_hip.h) evaluated with mpmath on every
solved case of tests/twoview_cases.py.  The null vectors are the eigenvectors of Q^T Q (A^T A) to its smallest eigenvalue
at 90 digits: forming the product costs twice the condition exponent (at most 2 x 9 digits in these tables), which leaves
the stored values good to 50 digits and more.  Per case (rounded to double):

  sha256      of the case's input bytes -- the inputs themselves are regenerated from seeds, not stored
  fit         F (3, 3) with unit Frobenius norm and its largest-magnitude entry positive; sigma = (sigma1, sigma8, sigma9) of Q
  hyp         F (Hyp, 3, 3) and sigma (Hyp, 3) likewise per sample; for the two mask cases also errors (Hyp, N) -- every
              correspondence under every sample's F, at the scale the rule leaves F with (a unit null vector) -- and the
              threshold: the geometric mean of the two adjacent sorted errors of ratio >= 1.01 nearest the errors' 20th percentile
  dlt         v (n, 4) the unit homogeneous vector, largest-magnitude entry positive; X (n, 3); sigma (n, 4) descending

    python tools/make_twoview_golden.py            (under a minute)"""
import os
import sys
import time

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import twoview_cases as tc  # noqa: E402

mp.mp.dps = 90
RATIO = mp.mpf("1.01")


def M(v):
    return mp.mpf(float(v))


def smallest(rows, k):
    """Eigen-decomposition of sum_rows r r^T (k x k): the unit eigenvector of the smallest eigenvalue, and the singular
    values of the row matrix, descending."""
    G = mp.zeros(k)
    for q in rows:
        for r in range(k):
            for c in range(r, k):
                G[r, c] += q[r] * q[c]
    for r in range(k):
        for c in range(r):
            G[r, c] = G[c, r]
    E, V = mp.eigsy(G)
    order = sorted(range(k), key=lambda i: E[i])
    v = [V[r, order[0]] for r in range(k)]
    sig = [mp.sqrt(max(E[i], mp.mpf(0))) for i in reversed(order)]
    return v, sig


def hartley(pts):
    n = len(pts)
    mx, my = sum(p[0] for p in pts) / n, sum(p[1] for p in pts) / n
    s = mp.sqrt(2) / mp.sqrt(sum((p[0] - mx) ** 2 + (p[1] - my) ** 2 for p in pts) / n)
    return s, -s * mx, -s * my


def fundamental(a, b, normalize):
    """a, b: lists of (x, y) -> F as the rule leaves it (3 x 3 nested lists) and sigma1, sigma8, sigma9 of Q."""
    h1 = h2 = (mp.mpf(1), mp.mpf(0), mp.mpf(0))
    if normalize:
        h1, h2 = hartley(a), hartley(b)
        a = [(h1[0] * x + h1[1], h1[0] * y + h1[2]) for x, y in a]
        b = [(h2[0] * x + h2[1], h2[0] * y + h2[2]) for x, y in b]
    rows = [[p[i] * q[j] for i in range(3) for j in range(3)] for p, q in
            (((x1, y1, mp.mpf(1)), (x2, y2, mp.mpf(1))) for (x1, y1), (x2, y2) in zip(a, b))]
    f, sig = smallest(rows, 9)
    F = [[f[3 * c + r] for c in range(3)] for r in range(3)]                  # F[b][a] = f[3a + b]
    v, _ = smallest(F, 3)                                                      # F^T F = sum of (rows of F)(rows of F)^T
    Fv = [sum(F[r][c] * v[c] for c in range(3)) for r in range(3)]
    F = [[F[r][c] - Fv[r] * v[c] for c in range(3)] for r in range(3)]
    if normalize:
        T1 = mp.matrix([[h1[0], 0, h1[1]], [0, h1[0], h1[2]], [0, 0, 1]])
        T2 = mp.matrix([[h2[0], 0, h2[1]], [0, h2[0], h2[2]], [0, 0, 1]])
        D = T2.T * mp.matrix(F) * T1
        F = [[D[r, c] for c in range(3)] for r in range(3)]
    return F, (sig[0], sig[7], sig[8])


def unit(values):
    """Unit norm, the largest-magnitude entry positive, as doubles."""
    n = mp.sqrt(sum(v * v for v in values))
    big = max(values, key=abs)
    return np.array([float(v / n * (-1 if big < 0 else 1)) for v in values])


def points(arr, idx):
    return [(M(arr[i, 0]), M(arr[i, 1])) for i in idx]


def f_error(F, p, q, kind):
    (x1, y1), (x2, y2) = p, q
    l2 = [F[r][0] * x1 + F[r][1] * y1 + F[r][2] for r in range(3)]
    e = x2 * l2[0] + y2 * l2[1] + l2[2]
    if kind == 0:
        return e * e
    l1 = [F[0][c] * x2 + F[1][c] * y2 + F[2][c] for c in range(2)]
    return max(e * e / (l2[0] ** 2 + l2[1] ** 2), e * e / (l1[0] ** 2 + l1[1] ** 2))


def run_fit(c):
    idx = np.flatnonzero(c.on)
    F, sig = fundamental(points(c.p1, idx), points(c.p2, idx), c.normalize)
    return dict(F=unit([F[r][k] for r in range(3) for k in range(3)]).reshape(3, 3), sigma=np.array([float(s) for s in sig]))


def run_hyp(c):
    n = len(c.p1)
    a, b = points(c.p1, range(n)), points(c.p2, range(n))
    Fs, sigs, raw = [], [], []
    for s in c.samples:
        F, sig = fundamental([a[i] for i in s], [b[i] for i in s], c.normalize)
        raw.append(F)
        Fs.append(unit([F[r][k] for r in range(3) for k in range(3)]).reshape(3, 3))
        sigs.append([float(v) for v in sig])
    out = dict(F=np.array(Fs), sigma=np.array(sigs))
    if "error_kind" in c.expect:
        kind = c.expect["error_kind"]
        err = [[f_error(F, a[i], b[i], kind) for i in range(n)] for F in raw]
        flat = sorted(e for row in err for e in row)
        nominal = flat[len(flat) // 5]
        gaps = [k for k in range(len(flat) - 1) if flat[k] > 0 and flat[k + 1] >= RATIO * flat[k]]
        k = min(gaps, key=lambda k: abs(mp.log(flat[k] * flat[k + 1]) / 2 - mp.log(nominal)))
        thr = mp.sqrt(flat[k] * flat[k + 1])
        for row in err:                                        # every hypothesis: no error within half a per cent
            assert all(e * mp.sqrt(RATIO) <= thr or e >= thr * mp.sqrt(RATIO) for e in row)
        out.update(errors=np.array([[float(e) for e in row] for row in err]), threshold=np.array(float(thr)))
    return out


def run_dlt(c):
    n = len(c.x1)
    C1 = np.broadcast_to(c.C1, (n, 3, 4))
    vs, Xs, sigs = [], [], []
    for i in range(n):
        rows = []
        for x, C in ((c.x1[i], C1[i]), (c.x2[i], c.C2)):
            u, v = M(x[0]), M(x[1])
            r = [[M(C[k, j]) for j in range(4)] for k in range(3)]
            rows.append([v * r[2][j] - r[1][j] for j in range(4)])
            rows.append([r[0][j] - u * r[2][j] for j in range(4)])
            rows.append([u * r[1][j] - v * r[0][j] for j in range(4)])
        w, sig = smallest(rows, 4)
        vs.append(unit(w))
        Xs.append([float(w[k] / w[3]) for k in range(3)])
        sigs.append([float(s) for s in sig])
    return dict(v=np.array(vs), X=np.array(Xs), sigma=np.array(sigs))


def main():
    t0 = time.time()
    arrays = {}
    for which, run in (("fit", run_fit), ("hyp", run_hyp), ("dlt", run_dlt)):
        for c in tc.table(which):
            if c.kind == "property":
                continue
            key = which + "/" + c.name + "/"
            arrays[key + "sha256"] = np.array(tc.sha256(c))
            for k, v in run(c).items():
                arrays[key + k] = np.asarray(v)
            s = arrays[key + "sigma"].reshape(-1, arrays[key + "sigma"].shape[-1])
            print("%-4s %-36s sigma ratios: second smallest %.2e  smallest %.2e   (%.0f s)" % (
                which, c.name, (s[:, -2] / s[:, 0]).min(), (s[:, -1] / s[:, 0]).max(), time.time() - t0), flush=True)
    np.savez_compressed(tc.GOLDEN, **arrays)
    print("wrote", tc.GOLDEN, os.path.getsize(tc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
