"""The float64 definition of the five-point essential-matrix rule (include/vo_hip.h, "calibrated two-view bootstrap";
csrc/essential5_device.h), stage by stage in NumPy, and the scorer's error formulas in the kernel's operation order.
TEST INFRASTRUCTURE: the kernels are compared with the 50-digit solution sets of tests/golden/essential5_cases.npz, and this
file's own distance to those sets is the yardstick their tolerance is derived from (tests/essential5_cases.py).

The rule (Nister 2004, "An efficient solution to the five-point relative pose problem"):
  1. x^ = Kinv (x, y, 1) for both images, Kinv the closed form of a pinhole K
  2. the rows kron(x^1, x^2) of the 5x9 system; Householder QR of its transpose; the last four columns of the orthogonal
     factor are the basis X, Y, Z, W of its null space, E = x X + y Y + z Z + W with E[b][a] = e[3a + b]
  3. det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10x20 matrix over the monomials MONOMIALS of (x, y, z)
  4. Gauss-Jordan elimination of its first ten columns with partial (row) pivoting
  5. rows e..j of the reduced system give B(z) (x, y, 1)^T = 0 with a 3x3 polynomial matrix B; det B is of degree 10
  6. its real roots: isolated between the real roots of its derivative (recursively, from the ninth derivative down, inside
     the Cauchy bound), a fixed number of bisection steps, then safeguarded Newton steps
  7. (x, y, 1) is the cross product of the two rows of B(z) whose third component is largest in magnitude
  8. unit Frobenius norm, the entry of largest magnitude (the first of equals) positive; ascending z
"""
import numpy as np

# the 20 monomials of degree <= 3 in Nister's column order; a monomial is a sorted triple over (x, y, z, 1) = (0, 1, 2, 3)
MONOMIALS = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
             (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3)]
PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]                     # the 10 monomials of degree <= 2
T2 = np.array([[PAIRS.index((min(a, b), max(a, b))) for b in range(4)] for a in range(4)])
T3 = np.array([[MONOMIALS.index(tuple(sorted(PAIRS[p] + (c,)))) for c in range(4)] for p in range(10)])

RANK_TOL = 1e-10        # a Householder column norm below this share of the largest: the null space is not 4-dimensional
PIVOT_TOL = 1e-12       # an elimination pivot below this share of the matrix's largest entry: no solution
LEAD_TOL = 1e-13        # a leading coefficient below this share of the largest coefficient: no solution
ISO_STEPS = 40          # bisection steps on the derivatives (isolation only)
BIS_STEPS = 64          # bisection steps on the polynomial itself
NEWTON_STEPS = 4


def pinhole_inverse(K):
    """The closed form the library passes to its kernels: K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])


def normalise(Kinv, p):
    """x^ = Kinv (x, y, 1), each row summed left to right: (n, 3)."""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    return np.stack([Kinv[r, 0] * x + Kinv[r, 1] * y + Kinv[r, 2] for r in range(3)], axis=1)


def null_space(h1, h2):
    """Stage 2: (ok, basis (4, 9)) from the normalised points of one sample ((5, 3) each)."""
    A = np.empty((9, 5))
    for k in range(5):
        for a in range(3):
            for b in range(3):
                A[3 * a + b, k] = h1[k, a] * h2[k, b]
    diag = np.empty(5)
    for k in range(5):
        s = 0.0
        for r in range(k, 9):
            s += A[r, k] * A[r, k]
        nrm = np.sqrt(s)
        diag[k] = nrm
        if not (nrm > 0.0) or not np.isfinite(nrm):
            return False, None
        alpha = -nrm if A[k, k] >= 0.0 else nrm
        A[k, k] = A[k, k] - alpha                       # v = x - alpha e_k, kept in the column
        vv = 0.0
        for r in range(k, 9):
            vv += A[r, k] * A[r, k]
        for c in range(k + 1, 5):
            d = 0.0
            for r in range(k, 9):
                d += A[r, k] * A[r, c]
            f = 2.0 * d / vv
            for r in range(k, 9):
                A[r, c] = A[r, c] - f * A[r, k]
    if not (diag.min() > RANK_TOL * diag.max()):
        return False, None
    basis = np.zeros((4, 9))
    for j in range(4):
        b = np.zeros(9)
        b[5 + j] = 1.0
        for k in range(4, -1, -1):
            vv = 0.0
            d = 0.0
            for r in range(k, 9):
                vv += A[r, k] * A[r, k]
                d += A[r, k] * b[r]
            f = 2.0 * d / vv
            for r in range(k, 9):
                b[r] = b[r] - f * A[r, k]
        basis[j] = b
    return True, basis


def constraint_matrix(basis):
    """Stage 3: the 10x20 coefficient matrix; row 0 is det E, rows 1..9 the entries of 2 E E^T E - tr(E E^T) E."""
    Ep = np.empty((3, 3, 4))                              # E[r][c] as a linear form over (x, y, z, 1)
    for r in range(3):
        for c in range(3):
            for v in range(4):
                Ep[r, c, v] = basis[v, 3 * c + r]

    def mul11(p, q):
        out = np.zeros(10)
        for a in range(4):
            for b in range(4):
                out[T2[a, b]] += p[a] * q[b]
        return out

    def mul21(p, q):
        out = np.zeros(20)
        for a in range(10):
            for b in range(4):
                out[T3[a, b]] += p[a] * q[b]
        return out

    M = np.zeros((10, 20))
    M[0] = (mul21(mul11(Ep[1, 1], Ep[2, 2]) - mul11(Ep[1, 2], Ep[2, 1]), Ep[0, 0])
            - mul21(mul11(Ep[1, 0], Ep[2, 2]) - mul11(Ep[1, 2], Ep[2, 0]), Ep[0, 1])
            + mul21(mul11(Ep[1, 0], Ep[2, 1]) - mul11(Ep[1, 1], Ep[2, 0]), Ep[0, 2]))
    G = np.empty((3, 3, 10))
    for i in range(3):
        for j in range(i, 3):
            G[i, j] = (mul11(Ep[i, 0], Ep[j, 0]) + mul11(Ep[i, 1], Ep[j, 1])) + mul11(Ep[i, 2], Ep[j, 2])
            G[j, i] = G[i, j]
    t = (G[0, 0] + G[1, 1]) + G[2, 2]
    L = 2.0 * G
    for i in range(3):
        L[i, i] = L[i, i] - t
    for i in range(3):
        for j in range(3):
            M[1 + 3 * i + j] = (mul21(L[i, 0], Ep[0, j]) + mul21(L[i, 1], Ep[1, j])) + mul21(L[i, 2], Ep[2, j])
    return M


def eliminate(M):
    """Stage 4: (ok, reduced matrix).  Partial pivoting over rows, the first ten columns to the identity."""
    M = M.copy()
    big = np.abs(M).max()
    if not np.isfinite(big) or big == 0.0:
        return False, M
    for c in range(10):
        p = c
        for r in range(c + 1, 10):
            if abs(M[r, c]) > abs(M[p, c]):
                p = r
        if not (abs(M[p, c]) > PIVOT_TOL * big):
            return False, M
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c, c:] = M[c, c:] / M[c, c]
        for r in range(10):
            if r != c:
                f = M[r, c]
                M[r, c:] = M[r, c:] - f * M[c, c:]
    return True, M


def b_matrix(R):
    """Stage 5a: B (3, 3, 5), ascending powers of z, from rows (4, 5), (6, 7), (8, 9) of the reduced matrix:
    row_e - z row_f over the columns [x z^2, x z, x, y z^2, y z, y, z^3, z^2, z, 1]."""
    B = np.zeros((3, 3, 5))
    for i in range(3):
        e, f = R[4 + 2 * i, 10:], R[5 + 2 * i, 10:]
        for v in range(2):
            o = 3 * v
            B[i, v, 0] = e[o + 2]
            B[i, v, 1] = e[o + 1] - f[o + 2]
            B[i, v, 2] = e[o] - f[o + 1]
            B[i, v, 3] = -f[o]
        B[i, 2, 0] = e[9]
        B[i, 2, 1] = e[8] - f[9]
        B[i, 2, 2] = e[7] - f[8]
        B[i, 2, 3] = e[6] - f[7]
        B[i, 2, 4] = -f[6]
    return B


def _pmul(p, q, n):
    out = np.zeros(n)
    for a in range(len(p)):
        for b in range(len(q)):
            if a + b < n:
                out[a + b] += p[a] * q[b]
    return out


def det_polynomial(B):
    """Stage 5b: det B(z), 11 coefficients in ascending powers, expanded along the third column."""
    def minor(r0, r1):
        return _pmul(B[r0, 0, :4], B[r1, 1, :4], 7) - _pmul(B[r0, 1, :4], B[r1, 0, :4], 7)
    return (_pmul(B[0, 2], minor(1, 2), 11) - _pmul(B[1, 2], minor(0, 2), 11)) + _pmul(B[2, 2], minor(0, 1), 11)


def _horner(q, n, z):
    v = q[n]
    for k in range(n - 1, -1, -1):
        v = v * z + q[k]
    return v


def real_roots(c):
    """Stage 6: (ok, ascending real roots) of the degree-10 polynomial with ascending coefficients c."""
    c = np.asarray(c, np.float64)
    m = np.abs(c).max()
    if not np.isfinite(m) or m == 0.0:
        return False, []
    c = c / m
    if not (abs(c[10]) > LEAD_TOL):
        return False, []
    bound = 0.0
    for k in range(10):
        bound = max(bound, abs(c[k] / c[10]))
    bound = 1.0 + bound
    if not np.isfinite(bound):
        return False, []
    roots = []
    for level in range(9, -1, -1):               # the level-th derivative, of degree n
        n = 10 - level
        q = np.empty(n + 1)
        for i in range(n + 1):
            f = 1.0
            for j in range(level):
                f = f * (i + level - j)
            q[i] = c[i + level] * f
        brk = [-bound] + roots + [bound]
        new = []
        steps = BIS_STEPS if level == 0 else ISO_STEPS
        for s in range(len(brk) - 1):
            lo, hi = brk[s], brk[s + 1]
            slo = _horner(q, n, lo) < 0.0
            shi = _horner(q, n, hi) < 0.0
            if slo == shi:
                continue
            for _ in range(steps):
                mid = 0.5 * (lo + hi)
                if (_horner(q, n, mid) < 0.0) == slo:
                    lo = mid
                else:
                    hi = mid
            z = 0.5 * (lo + hi)
            if level == 0:
                for _ in range(NEWTON_STEPS):
                    v = q[n]
                    d = 0.0
                    for k in range(n - 1, -1, -1):
                        d = d * z + v
                        v = v * z + q[k]
                    zn = z - v / d if d != 0.0 else z
                    if zn >= lo and zn <= hi:
                        z = zn
            new.append(z)
        roots = new
    return True, roots


def back_substitute(B, basis, z):
    """Stages 7 and 8 for one root: (ok, E (3, 3))."""
    Bz = np.empty((3, 3))
    for i in range(3):
        for v in range(3):
            Bz[i, v] = _horner(B[i, v], 4, z)
    best = None
    for (r0, r1) in ((0, 1), (0, 2), (1, 2)):
        u = Bz[r0, 1] * Bz[r1, 2] - Bz[r0, 2] * Bz[r1, 1]
        v = Bz[r0, 2] * Bz[r1, 0] - Bz[r0, 0] * Bz[r1, 2]
        w = Bz[r0, 0] * Bz[r1, 1] - Bz[r0, 1] * Bz[r1, 0]
        if best is None or abs(w) > abs(best[2]):
            best = (u, v, w)
    if not (abs(best[2]) > 0.0):
        return False, None
    x, y = best[0] / best[2], best[1] / best[2]
    e = ((x * basis[0] + y * basis[1]) + z * basis[2]) + basis[3]
    s = 0.0
    for k in range(9):
        s += e[k] * e[k]
    nrm = np.sqrt(s)
    if not np.isfinite(nrm) or not (nrm > 0.0):
        return False, None
    e = e / nrm
    E = np.empty((3, 3))                         # entry (r, c) is e[3c + r]
    for r in range(3):
        for c_ in range(3):
            E[r, c_] = e[3 * c_ + r]
    return True, canonical_sign(E)


def canonical_sign(E):
    """The entry of largest magnitude positive, the first such entry in row-major order on ties."""
    f = E.reshape(9)
    m = 0
    for k in range(1, 9):
        if abs(f[k]) > abs(f[m]):
            m = k
    return -E if f[m] < 0.0 else E


def solve5(h1, h2):
    """All real essential matrices of one sample of normalised points: (n_sol, E (10, 3, 3), z (10,))."""
    E = np.zeros((10, 3, 3))
    zs = np.zeros(10)
    ok, basis = null_space(h1, h2)
    if not ok:
        return 0, E, zs
    ok, R = eliminate(constraint_matrix(basis))
    if not ok:
        return 0, E, zs
    B = b_matrix(R)
    ok, roots = real_roots(det_polynomial(B))
    if not ok:
        return 0, E, zs
    n = 0
    for z in roots:
        ok, Ez = back_substitute(B, basis, z)
        if ok and np.all(np.isfinite(Ez)):
            E[n] = Ez
            zs[n] = z
            n += 1
    return n, E, zs


def hypotheses(x1, x2, K1, K2, samples):
    """(E (Hyp, 10, 3, 3), n_sol (Hyp,)) of pixel correspondences through pinhole cameras."""
    h1 = normalise(pinhole_inverse(K1), x1)
    h2 = normalise(pinhole_inverse(K2), x2)
    samples = np.asarray(samples).reshape(-1, 5)
    E = np.zeros((len(samples), 10, 3, 3))
    n_sol = np.zeros(len(samples), np.int32)
    for h, s in enumerate(samples):
        n_sol[h], E[h], _ = solve5(h1[s], h2[s])
    return E, n_sol


# ---- the scorer, in the operation order of f_error (csrc/fscore_device.h) ----

def fundamental_from_essential(E, K1inv, K2inv):
    """F = K2inv^T (E K1inv), every entry summed left to right; E (..., 3, 3)."""
    E = np.asarray(E, np.float64)
    A = np.empty(E.shape)
    F = np.empty(E.shape)
    for r in range(3):
        for c in range(3):
            A[..., r, c] = (E[..., r, 0] * K1inv[0, c] + E[..., r, 1] * K1inv[1, c]) + E[..., r, 2] * K1inv[2, c]
    for r in range(3):
        for c in range(3):
            F[..., r, c] = (K2inv[0, r] * A[..., 0, c] + K2inv[1, r] * A[..., 1, c]) + K2inv[2, r] * A[..., 2, c]
    return F


def f_error(F, p1, p2, kind):
    """Errors (N,) of pixel correspondences under one F (3, 3)."""
    F = np.asarray(F, np.float64).reshape(9)
    p1 = np.asarray(p1, np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(all="ignore"):
        if kind == 0:
            t0 = (x2 * F[0] + y2 * F[3]) + F[6]
            t1 = (x2 * F[1] + y2 * F[4]) + F[7]
            t2 = (x2 * F[2] + y2 * F[5]) + F[8]
            r = (t0 * x1 + t1 * y1) + t2
            return r * r
        l2x = (F[0] * x1 + F[1] * y1) + F[2]
        l2y = (F[3] * x1 + F[4] * y1) + F[5]
        l2z = (F[6] * x1 + F[7] * y1) + F[8]
        l1x = (F[0] * x2 + F[3] * y2) + F[6]
        l1y = (F[1] * x2 + F[4] * y2) + F[7]
        e = (x2 * l2x + y2 * l2y) + l2z
        num = e * e
        d2 = num / (l2x * l2x + l2y * l2y)
        d1 = num / (l1x * l1x + l1y * l1y)
        return np.where(d1 > d2, d1, d2)


# ---- comparisons ----

def set_distance(Ea, Eb):
    """Two sets of canonical unit matrices (na, 3, 3), (nb, 3, 3) of the same size matched one to one (greedy on the
    sorted pair distances): the largest Frobenius distance of a matched pair; inf when the sizes differ."""
    Ea = np.asarray(Ea, np.float64).reshape(-1, 9)
    Eb = np.asarray(Eb, np.float64).reshape(-1, 9)
    if len(Ea) != len(Eb):
        return np.inf
    if len(Ea) == 0:
        return 0.0
    D = np.minimum(np.linalg.norm(Ea[:, None] - Eb[None], axis=2), np.linalg.norm(Ea[:, None] + Eb[None], axis=2))
    worst = 0.0
    D = D.copy()
    for _ in range(len(Ea)):
        i, j = np.unravel_index(np.argmin(D), D.shape)
        worst = max(worst, D[i, j])
        D[i, :] = np.inf
        D[:, j] = np.inf
    return float(worst)


def backward_figures(E, h1, h2):
    """(|norm - 1|, sign ok, max |x^2^T E x^1| over the five unit-scaled points, |det E|, ||2EE^TE - tr(EE^T)E||)."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    u1 = h1 / np.linalg.norm(h1, axis=1, keepdims=True)
    u2 = h2 / np.linalg.norm(h2, axis=1, keepdims=True)
    epi = np.abs(np.einsum("kb,ba,ka->k", u2, E, u1)).max()
    f = E.reshape(9)
    sign_ok = bool(f[np.argmax(np.abs(f))] > 0.0)
    EEt = E @ E.T
    return (abs(np.linalg.norm(E) - 1.0), sign_ok, float(epi), abs(float(np.linalg.det(E))),
            float(np.linalg.norm(2.0 * EEt @ E - np.trace(EEt) * E)))
