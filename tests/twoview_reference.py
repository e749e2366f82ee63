"""The definitions the 8-point kernels and the DLT are pinned to.  TEST INFRASTRUCTURE.

The rules of include/vo_hip.h ("two-view bootstrap", "DLT triangulation") stated in float64 NumPy with + - * / sqrt only
(no LAPACK, no BLAS: every machine computes the same values), vectorised over samples / points.  The kernels of
csrc/bootstrap.hip and csrc/dlt.hip (tests/test_gpu_twoview_reference.py) and the 50-digit values of
tests/golden/twoview_cases.npz (tools/make_twoview_golden.py, tests/test_twoview_reference_host.py) are compared with it.

  hartley         x' = s x + tx, y' = s y + ty with s = sqrt(2) / sqrt(mean |p - mean p|^2)        (helpers.py:31-54)
  kron_rows       Q[k, 3a + b] = p1_k[a] p2_k[b] for p = (x, y, 1)                                  (triangulation.py:203-205)
  null_vector     the right singular vector of Q's smallest singular value (np.linalg.svd(Q)[2][-1], :209-212) by a
                  one-sided (Hestenes) Jacobi iteration on the columns of the WHOLE matrix Q: column pairs are rotated
                  until mutually orthogonal, the same rotations accumulate V, the column norms are the singular values.
                  Backward stable -- deliberately not the route over the normal matrix Q^T Q, whose conditioning is Q's
                  squared.
  rank2           F minus its smallest singular triplet (:214-217), the same iteration on the 3x3
  denormalise     T2^T F T1 for T = [[s, 0, tx], [0, s, ty], [0, 0, 1]]
  dlt             A = [[x1]_x C1; [x2]_x C2] (6x4, the rows of csrc/dlt_device.h), the same iteration, the column of least
                  norm, de-homogenised

A point order (`perm`) is the order in which every sum over the points is formed."""
import numpy as np

SWEEPS = 60
TOL2 = 1e-30           # a pair is left alone once gamma^2 <= TOL2 alpha beta: |cos| of the two columns below 1e-15


def jacobi_columns(A):
    """One-sided Jacobi.  A: (B, k, m), matrix b's column j in A[b, j, :].  Returns the rotated columns (mutually
    orthogonal: U Sigma, transposed), V (B, k, k) with V[b, r, j] = entry r of right singular vector j, and the squared
    column norms (B, k)."""
    A = np.array(A, np.float64)
    B, k, m = A.shape
    V = np.zeros((B, k, k))
    V[:, np.arange(k), np.arange(k)] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            rotated = False
            for p in range(k - 1):
                for q in range(p + 1, k):
                    ap, aq = A[:, p, :].copy(), A[:, q, :].copy()
                    alpha, beta, gamma = (ap * ap).sum(axis=1), (aq * aq).sum(axis=1), (ap * aq).sum(axis=1)
                    rot = ~((gamma == 0.0) | (gamma * gamma <= TOL2 * (alpha * beta)))
                    if not rot.any():
                        continue
                    rotated = True
                    d, g = beta - alpha, 2.0 * gamma
                    w = np.abs(d) + np.sqrt(d * d + g * g)
                    rn = np.sqrt(w * w + g * g)
                    sm = np.abs(g) / rn
                    c = np.where(rot, w / rn, 1.0)[:, None]
                    s = np.where(rot, np.where((d == 0.0) | ((d > 0.0) == (g > 0.0)), sm, -sm), 0.0)[:, None]
                    A[:, p, :], A[:, q, :] = c * ap - s * aq, s * ap + c * aq
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p], V[:, :, q] = c * vp - s * vq, s * vp + c * vq
            if not rotated:
                break
        return A, V, (A * A).sum(axis=2)


def _least(A, V, n2):
    """Per matrix: the right singular vector of the least column norm, that column, and the singular values descending."""
    m = np.argmin(np.where(np.isnan(n2), np.inf, n2), axis=1)
    b = np.arange(len(m))
    return V[b, :, m], A[b, m, :], -np.sort(-np.sqrt(n2), axis=1)


def hartley(points):
    """points (B, m, 2) -> s, tx, ty, each (B,).  The sums run over axis 1 in the order given."""
    m = points.shape[1]
    with np.errstate(all="ignore"):
        mx, my = points[:, :, 0].sum(axis=1) / m, points[:, :, 1].sum(axis=1) / m
        dx, dy = points[:, :, 0] - mx[:, None], points[:, :, 1] - my[:, None]
        s = np.sqrt(2.0) / np.sqrt((dx * dx + dy * dy).sum(axis=1) / m)
        return s, -s * mx, -s * my


def apply_hartley(points, h):
    s, tx, ty = h
    with np.errstate(all="ignore"):
        return np.stack((s[:, None] * points[:, :, 0] + tx[:, None], s[:, None] * points[:, :, 1] + ty[:, None]), axis=2)


def kron_rows(p1, p2):
    """p1, p2 (B, m, 2) -> Q (B, m, 9) with Q[.., 3a + b] = (x1, y1, 1)[a] (x2, y2, 1)[b]."""
    one = np.ones(p1.shape[:2])
    a, b = (p1[:, :, 0], p1[:, :, 1], one), (p2[:, :, 0], p2[:, :, 1], one)
    with np.errstate(all="ignore"):
        return np.stack([a[i] * b[j] for i in range(3) for j in range(3)], axis=2)


def null_vector(Q, perm=None):
    """Q (m, 9) [or (B, m, 9)] -> the unit right singular vector of the smallest singular value and the nine column norms,
    descending -- the singular values.  `perm`: the row order in which the column sums are formed."""
    Q = np.asarray(Q, np.float64)
    single = Q.ndim == 2
    Q = Q[None] if single else Q
    if perm is not None:
        Q = Q[:, np.asarray(perm)]
    A, V, n2 = jacobi_columns(np.transpose(Q, (0, 2, 1)))
    f, _, sig = _least(A, V, n2)
    return (f[0], sig[0]) if single else (f, sig)


def rank2(F):
    """F (B, 3, 3) minus its smallest singular triplet: F - (F v) v^T."""
    A, V, n2 = jacobi_columns(np.transpose(F, (0, 2, 1)))
    v, Fv, _ = _least(A, V, n2)
    with np.errstate(all="ignore"):
        return F - Fv[:, :, None] * v[:, None, :]


def denormalise(F, h1, h2):
    """T2^T F T1, in the kernel's order: (F T1) first."""
    (s1, tx1, ty1), (s2, tx2, ty2) = h1, h2
    with np.errstate(all="ignore"):
        A = np.empty_like(F)
        A[:, :, 0] = F[:, :, 0] * s1[:, None]
        A[:, :, 1] = F[:, :, 1] * s1[:, None]
        A[:, :, 2] = F[:, :, 0] * tx1[:, None] + F[:, :, 1] * ty1[:, None] + F[:, :, 2]
        out = np.empty_like(F)
        out[:, 0, :] = s2[:, None] * A[:, 0, :]
        out[:, 1, :] = s2[:, None] * A[:, 1, :]
        out[:, 2, :] = tx2[:, None] * A[:, 0, :] + ty2[:, None] * A[:, 1, :] + A[:, 2, :]
        return out


def fundamental_batch(a, b, normalize):
    """a, b (B, m, 2): B point sets of m correspondences -> F (B, 3, 3), singular values of Q (B, 9)."""
    if normalize:
        h1, h2 = hartley(a), hartley(b)
        a, b = apply_hartley(a, h1), apply_hartley(b, h2)
    f, sig = null_vector(kron_rows(a, b))
    F = np.transpose(f.reshape(-1, 3, 3), (0, 2, 1))            # F[b][a] = f[3a + b]
    F = rank2(F)
    return (denormalise(F, h1, h2) if normalize else F), sig


def active(n, on):
    return np.ones(n, bool) if on is None else np.asarray(on).reshape(-1) != 0


def fundamental(p1, p2, on=None, normalize=True, perm=None):
    """The 8-point fit over the active correspondences (mask byte != 0; None: all) -> F (3, 3), the nine singular values
    of Q, the active count.  `perm`: a permutation of the point order."""
    p1, p2 = np.asarray(p1, np.float64).reshape(-1, 2), np.asarray(p2, np.float64).reshape(-1, 2)
    idx = np.flatnonzero(active(len(p1), on))
    if perm is not None:
        idx = np.asarray(perm)[np.isin(perm, idx)]
    F, sig = fundamental_batch(p1[idx][None], p2[idx][None], normalize)
    return F[0], sig[0], len(idx)


def fundamental_samples(p1, p2, samples, normalize):
    """The 8-point F of every sample (Hyp, 8) of indices -> (Hyp, 3, 3), singular values (Hyp, 9)."""
    p1, p2 = np.asarray(p1, np.float64).reshape(-1, 2), np.asarray(p2, np.float64).reshape(-1, 2)
    samples = np.asarray(samples).reshape(-1, 8)
    return fundamental_batch(p1[samples], p2[samples], normalize)


def f_errors(F, p1, p2, kind):
    """Every correspondence under one F, in the operation order of csrc/fscore_device.h.  kind 0: (p2^T F p1)^2; 1: the
    larger squared distance to the epipolar lines of the two images."""
    F = np.asarray(F, np.float64).reshape(9)
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(all="ignore"):
        if kind == 0:
            t0, t1, t2 = x2 * F[0] + y2 * F[3] + F[6], x2 * F[1] + y2 * F[4] + F[7], x2 * F[2] + y2 * F[5] + F[8]
            r = t0 * x1 + t1 * y1 + t2
            return r * r
        l2x, l2y, l2z = F[0] * x1 + F[1] * y1 + F[2], F[3] * x1 + F[4] * y1 + F[5], F[6] * x1 + F[7] * y1 + F[8]
        l1x, l1y = F[0] * x2 + F[3] * y2 + F[6], F[1] * x2 + F[4] * y2 + F[7]
        e = x2 * l2x + y2 * l2y + l2z
        num = e * e
        d2, d1 = num / (l2x * l2x + l2y * l2y), num / (l1x * l1x + l1y * l1y)
        return np.where(d1 > d2, d1, d2)


def dlt_rows(x1, x2, C1, C2):
    """(n, 6, 4): the rows (0, -1, v), (1, 0, -u), (-v, u, 0) of [x]_x times each camera, as csrc/dlt_device.h forms them."""
    x1, x2 = np.asarray(x1, np.float64).reshape(-1, 2), np.asarray(x2, np.float64).reshape(-1, 2)
    n = len(x1)
    C1 = np.broadcast_to(np.asarray(C1, np.float64).reshape(-1, 3, 4), (n, 3, 4))
    C2 = np.broadcast_to(np.asarray(C2, np.float64).reshape(-1, 3, 4), (n, 3, 4))
    A = np.empty((n, 6, 4))
    with np.errstate(all="ignore"):
        for k, (x, C) in enumerate(((x1, C1), (x2, C2))):
            u, v = x[:, 0:1], x[:, 1:2]
            A[:, 3 * k] = v * C[:, 2] - C[:, 1]
            A[:, 3 * k + 1] = C[:, 0] - u * C[:, 2]
            A[:, 3 * k + 2] = u * C[:, 1] - v * C[:, 0]
    return A


def dlt(x1, x2, C1, C2):
    """Per point: the unit homogeneous vector (n, 4), the de-homogenised point (n, 3), the four singular values (n, 4)."""
    A, V, n2 = jacobi_columns(np.transpose(dlt_rows(x1, x2, C1, C2), (0, 2, 1)))
    v, _, sig = _least(A, V, n2)
    with np.errstate(all="ignore"):
        return v, v[:, :3] / v[:, 3:], sig
