"""TEST INFRASTRUCTURE.  The definition of the Shi-Tomasi detector the project restates: cv2.cornerMinEigenVal +
cv2.goodFeaturesToTrack as the reference calls them (src/vo/features/klt.py:24-26, 98), one function per stage, in exact
integers and float64.  It imports neither `oracle` nor the library: oracle/csrc/goodfeatures.c and csrc/goodfeatures.hip are
what it is compared with (tests/test_good_features_reference_host.py, tests/test_gpu_good_features_reference.py).

    sobel         gx, gy: 3x3 Sobel correlation, reflect-101 on the image              exact integers
    tensor_sums   block x block box sums of gx^2, gx gy, gy^2, window [-(block//2), block-1-block//2],
                  reflect-101 on the product images, as often as it takes                exact integers
    min_eig       the smaller eigenvalue of [[a, b/2], [b/2, c]] * 2 in the code's notation, a = s^2 Sxx / 2, b = s^2 Sxy,
                  c = s^2 Syy / 2, s = 1 / (4 block 255), without the cancellation       float64
    select        threshold, 3x3 maxima, order, minimum distance, by brute force

One documented difference from OpenCV remains: OpenCV accumulates the box sums in float32 in its own (SIMD-dependent) order;
the definition, the oracle and the kernels sum exact integers."""
import numpy as np

U = 2.0 ** -24              # float32 unit roundoff (round to nearest)
KAPPA = 10                  # rounding_bound's constant, derived in its docstring


def reflect101(i, n):
    """Index i reflected into [0, n) without repeating the edge (... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...), as often as it
    takes: the closed form of period 2(n - 1).  A side of 1 has one index."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def sobel(img):
    """(gx, gy) int64: correlation with [[-1 0 1], [-2 0 2], [-1 0 1]] and its transpose, reflect-101 border.  |g| <= 1020."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    p = img.astype(np.int64)[reflect101(np.arange(-1, H + 1), H)][:, reflect101(np.arange(-1, W + 1), W)]
    gx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    gy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    return gx, gy


def _box(prod, block):
    H, W = prod.shape
    r0 = block // 2
    ext = prod[reflect101(np.arange(-r0, H + block - 1 - r0), H)][:, reflect101(np.arange(-r0, W + block - 1 - r0), W)]
    ii = np.zeros((ext.shape[0] + 1, ext.shape[1] + 1), np.int64)
    ii[1:, 1:] = ext.cumsum(0).cumsum(1)
    return ii[block:, block:] - ii[:-block, block:] - ii[block:, :-block] + ii[:-block, :-block]


def tensor_sums(img, block):
    """(Sxx, Sxy, Syy) int64, exact.  |S| <= 31^2 1020^2 < 2^30 for block <= 31, so Sxx Syy, (Sxx - Syy)^2 + 4 Sxy^2 (below
    2^60 + 2^62) and the integral image the box is read from (below 1020^2 (H + 30)(W + 30)) stay inside int64; asserted."""
    assert 1 <= block <= 31
    gx, gy = sobel(img)
    assert (gx.shape[0] + 30) * (gx.shape[1] + 30) * 1020 ** 2 < 2 ** 62
    Sxx, Sxy, Syy = _box(gx * gx, block), _box(gx * gy, block), _box(gy * gy, block)
    assert max(int(np.abs(S).max()) for S in (Sxx, Sxy, Syy)) < 2 ** 30
    return Sxx, Sxy, Syy


def scale(block):
    return 1.0 / (4.0 * block * 255.0)


def min_eig(img, block):
    """(lambda, trace) float64.  With T = Sxx + Syy, det = Sxx Syy - Sxy^2 >= 0 (Cauchy-Schwarz; an exact integer) and
    D = sqrt((Sxx - Syy)^2 + 4 Sxy^2):  lambda = s^2 (T - D) / 2 = s^2 2 det / (T + D), the second form free of cancellation
    (relative error a few 2^-53); 0 where T = 0.  trace = s^2 T / 2 = a + c."""
    Sxx, Sxy, Syy = tensor_sums(img, block)
    T = Sxx + Syy
    det = Sxx * Syy - Sxy * Sxy
    assert det.min() >= 0
    D = np.sqrt(((Sxx - Syy) ** 2 + 4 * Sxy * Sxy).astype(np.float64))
    s2 = scale(block) ** 2
    den = T.astype(np.float64) + D
    lam = np.where(T > 0, s2 * 2.0 * det.astype(np.float64) / np.where(T > 0, den, 1.0), 0.0)
    return lam, s2 * T.astype(np.float64) / 2.0


def rounding_bound(trace):
    """First-order worst case of |float32 evaluation - lambda|, KAPPA 2^-24 trace, for the evaluation the oracle and the
    kernels share:

        s2 = (float)(s^2);  a = (float)Sxx * s2 * 0.5f;  b = (float)Sxy * s2;  c = (float)Syy * s2 * 0.5f;
        e  = (a + c) - sqrtf((a - c) * (a - c) + b * b)

    u = 2^-24, t = a + c (the trace), R = sqrt((a - c)^2 + b^2) <= t (t^2 - R^2 = 4ac - b^2 = s^4 det >= 0), every operation
    rounded to nearest, * 0.5f exact, no underflow (a >= 2^-31 where it is not 0).
      s2      its rounding is one factor (1 + d), |d| <= u, on a, b and c alike, so on e: u lambda <= 1 u t.
      a, b, c beyond that each carry two roundings, (float)S and the product: relative 2u each.
      a + c   2u a + 2u c, and the sum's own rounding u t:                                            3 u t.
      root    a - c errs by 2u a + 2u c + u |a - c| <= 2u t + u |a - c|, b by 2u |b|.  Through R's gradient
              ((a - c) / R, b / R), with |a - c| = R cos w, |b| = R sin w:
                  2u t cos w + u R cos^2 w + 2u R sin^2 w <= u t (2 cos w + 2 - cos^2 w) <= 3 u t   (largest at cos w = 1);
              the two squares and their sum put at most 2u on the radicand, u R on the root; sqrtf's own rounding u R:
                                                                                  3 u t + 2 u R <=  5 u t.
      (a + c) - root   its own rounding, u |e| <= u t:                                               1 u t.
    KAPPA = 1 + 3 + 5 + 1 = 10.  (Bounding the root's three input terms one by one, without the angle, gives 6 for the
    root and 11 in all.)  The bound is proportional to the trace, not to lambda: on an edge lambda is 0 and the float32
    value is whatever the subtraction of two numbers near t leaves."""
    return KAPPA * U * np.asarray(trace, np.float64)


def _allowed(shape, mask):
    return np.ones(shape, bool) if mask is None else np.asarray(mask) != 0


def _neighbourhood_max(t):
    """Maximum of every pixel's 3x3 neighbourhood (pixels outside count as 0; only interior pixels are asked)."""
    H, W = t.shape
    p = np.zeros((H + 2, W + 2), t.dtype)
    p[1:-1, 1:-1] = t
    m = np.zeros_like(t)
    for j in range(3):
        for i in range(3):
            m = np.maximum(m, p[j:j + H, i:i + W])
    return m


def threshold(eig_map, mask, quality):
    """quality x the maximum over the allowed pixels (None: nothing is allowed).  A float32 map: the product is made in
    float64 and rounded to float32, as OpenCV's threshold() receives it; a float64 map (the definition's): plain float64."""
    ok = _allowed(eig_map.shape, mask)
    if not ok.any():
        return None
    thr = np.float64(eig_map[ok].max()) * np.float64(quality)
    return np.float32(thr) if eig_map.dtype == np.float32 else thr


def candidates(eig_map, mask, quality):
    """(ys, xs) of the kept pixels in the rule's order: v > thr, v != 0, mask non-zero, rows 1..H-2 and columns 1..W-2, v
    equal to the maximum of its 3x3 neighbourhood of the thresholded map (values <= thr count as 0); value descending, ties by
    higher address y W + x first."""
    eig_map = np.asarray(eig_map)
    assert eig_map.dtype in (np.float32, np.float64) and eig_map.ndim == 2
    H, W = eig_map.shape
    thr = threshold(eig_map, mask, quality)
    none = np.zeros(0, np.int64)
    if thr is None or H < 3 or W < 3:
        return none, none
    t = np.where(eig_map > thr, eig_map, eig_map.dtype.type(0))
    keep = (eig_map > thr) & (eig_map != 0) & _allowed(eig_map.shape, mask) & (eig_map == _neighbourhood_max(t))
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    ys, xs = np.nonzero(keep)
    order = sorted(range(len(ys)), key=lambda k: (-float(eig_map[ys[k], xs[k]]), -(int(ys[k]) * W + int(xs[k]))))
    return ys[order].astype(np.int64), xs[order].astype(np.int64)


def select(eig_map, mask, max_corners, quality, min_distance):
    """The corners, (n, 2) float32 rows (x, y): the candidates in order, each accepted unless an accepted corner lies closer
    than min_distance (dx^2 + dy^2 < min_distance^2; the test is made only when min_distance >= 1), until max_corners are
    accepted (max_corners <= 0: no limit).  Every accepted corner is compared: no cell grid, no rounds."""
    ys, xs = candidates(eig_map, mask, quality)
    d2 = float(min_distance) * float(min_distance)
    ax, ay = [], []
    for y, x in zip(ys.tolist(), xs.tolist()):
        if max_corners > 0 and len(ax) >= max_corners:
            break
        if min_distance >= 1 and ax:
            dx, dy = np.asarray(ax) - x, np.asarray(ay) - y
            if ((dx * dx + dy * dy) < d2).any():
                continue
        ax.append(x)
        ay.append(y)
    return np.stack([np.asarray(ax, np.float32), np.asarray(ay, np.float32)], 1).reshape(-1, 2)


def tie_key(img, block):
    """(T, (Sxx - Syy)^2, Sxy^2) per pixel.  Two pixels with the same key have bit-equal float32 values in the code: a + c
    and (a - c)^2 do not change when Sxx and Syy trade places, b * b not with the sign of Sxy."""
    Sxx, Sxy, Syy = tensor_sums(img, block)
    return np.stack([Sxx + Syy, (Sxx - Syy) ** 2, Sxy * Sxy], -1)


def decided(img, mask, max_corners, quality, min_distance, block, report=None):
    """True when every decision select() makes on the definition's map comes out the same on any map within
    rounding_bound of it, so that the code's corners must equal the definition's:
      - the threshold lies in quality x [max(lambda - beta), max(lambda + beta)] over the allowed pixels, widened by one
        float32 ulp; every allowed interior pixel clears that interval by more than its beta (a pixel whose sums are all 0
        is exactly 0 in the code and never kept);
      - a pixel above the threshold either has a neighbour higher by more than the two bounds (not a maximum), or each of
        its eight neighbours is lower by more than the two bounds or an exact tie (tie_key: bit-equal values, both kept);
      - any two kept pixels differ by more than their bounds or tie exactly (then the address decides).
    Mask, interior, distance and the corner limit are exact integer decisions.  `report`, a dict, receives the margins."""
    del max_corners, min_distance
    lam, trace = min_eig(img, block)
    beta = rounding_bound(trace)
    key = tie_key(img, block)
    H, W = lam.shape
    ok = _allowed(lam.shape, mask)
    if not ok.any() or H < 3 or W < 3:
        return True
    hi = (lam + beta)[ok].max() * quality
    lo = (lam - beta)[ok].max() * quality
    ulp = float(np.spacing(np.float32(hi)))
    lo, hi = lo - ulp, hi + ulp
    inner = np.zeros(lam.shape, bool)
    inner[1:-1, 1:-1] = True
    ask = ok & inner & (trace > 0)
    above = ask & (lam - beta > hi)
    below = ask & (lam + beta < lo)
    if report is not None:
        gap = (np.where(lam >= hi, lam - hi, lo - lam) / np.where(ask, beta, 1.0))[ask]
        report["threshold_margin"] = float(gap.min()) if gap.size else np.inf      # distance to the interval / own bound
    if (ask & ~above & ~below).any():
        return False
    kept = []
    margin = np.inf
    for y, x in zip(*np.nonzero(above)):
        higher, clear = False, True
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                if i == 0 and j == 0:
                    continue
                q = (y + j, x + i)
                both = beta[y, x] + beta[q]
                if lam[q] - lam[y, x] > both:
                    higher = True
                elif np.array_equal(key[q], key[y, x]):
                    pass
                elif lam[y, x] - lam[q] > both:
                    margin = min(margin, (lam[y, x] - lam[q]) / both)
                else:
                    clear = False
        if higher:
            continue
        if not clear:
            return False
        kept.append((y, x))
    for n, p in enumerate(kept):
        for q in kept[:n]:
            if np.array_equal(key[p], key[q]):
                continue
            both = beta[p] + beta[q]
            if not abs(lam[p] - lam[q]) > both:
                return False
            margin = min(margin, abs(lam[p] - lam[q]) / both)
    if report is not None:
        report["kept"] = len(kept)
        report["order_margin"] = float(margin)        # smallest decided difference / sum of the two bounds
    return True
