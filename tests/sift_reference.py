"""The definition the SIFT oracle (oracle/csrc/sift.c) and kernels (csrc/sift.hip) are pinned to.  TEST INFRASTRUCTURE.

Lowe's SIFT as cv2.SIFT_create() (4.8.1 defaults) structures it, written from the description in the header of
oracle/csrc/sift.c and include/vo_hip.h, in real arithmetic: NumPy float64, libm exp / sin / cos, unrounded kernel weights,
NumPy's summation order.  It does not import oracle.native.  tests/test_sift_reference_host.py compares the oracle with it
stage by stage, tests/test_gpu_sift_reference.py the kernels end to end.

Conventions.  Images are (H, W) uint8, a point is (x, y), x right, y down.  The base image is the input doubled with
half-pixel-centre bilinear weights (sample (i + 0.5) / 2 - 0.5, edge-replicated) and blurred from its nominal sigma 1 to
1.6; octave o halves octave o - 1's level 3 by taking every second pixel.  A keypoint found at (c + xc, r + xr) of octave o
is reported at (c + xc, r + xr) * 2^o * 0.5: the doubling's half-pixel centres are NOT undone (cv2's enable_precise_upscale
is off by default), so a feature at p of the input is reported near p + 0.25 -- part of the definition, asserted by the
blob tests.  size = 1.6 * 2^((layer + xi) / 3) * 2^o; the angle is measured clockwise on screen from +x, in degrees.

Every discrete decision yields a margin in the unit of the compared quantity and the bound that quantity carries in a
float32 implementation (pyramid_bounds, solve bounds below).  A decision is DECIDED when margin > 2 * bound; a keypoint or a
rejected candidate is decided when every decision on its path is.  Candidates and histogram peaks that fail a comparison by
less than that are kept as undecided records, so that an implementation that lands on the other side has a counterpart.

ft = numpy.float32 runs the same statements with every intermediate rounded to float32 -- used only to measure how far
hard-binned quantities (histogram, angle, descriptor) move under rounding (HIST_TOL, ANGLE_TOL, DESC_TOL)."""
import math
import types

import numpy as np

SIGMA, NOL, NG, BORDER = 1.6, 3, 6, 5
CONTRAST_THR, EDGE_THR, MAX_STEPS = 0.04, 10.0, 5
ORI_BINS, ORI_SIG, ORI_RADIUS, ORI_PEAK = 36, 1.5, 4.5, 0.8
#: A gradient whose angle is this close to a boundary between two histogram bins is binned by rounding, not by the image
#: (whole-number images put many exactly on 45 degrees); a keypoint with more than BIN_TIE_MASS of its histogram's maximum
#: in such samples is undecided ("bin tie").  1e-3 degrees is a hundred float32 ulps of an angle.  A gradient that
#: close to a diagonal counts too: fastAtan2's two branches meet there 0.019 degrees apart, on either side of the boundary
#: between two bins (44.990 and 45.010), and rounding picks the branch.
BIN_TIE_DEG, BIN_TIE_MASS = 1e-3, 1e-4
DESC_D, DESC_N, DESC_SCL, DESC_CLAMP = 4, 8, 3.0, 0.2
U = 2.0 ** -24                       # float32 unit roundoff
F32_SLACK = 2.0 ** -20               # a handful of float32 roundings in a final formula (and the exp polynomial), relative
DOG_THRESHOLD = math.floor(0.5 * CONTRAST_THR / NOL * 255)

#: 4 x the largest distance between the float64 and the float32 run of this definition over the cases of sift_cases.py
#: (tests/test_sift_reference_host.py::test_measured_tolerances re-measures them; DESIGN.md section 2 has the table).
#: Histogram values are relative to the histogram's maximum, angles in degrees, descriptor entries in descriptor units.
HIST_TOL = 4 * 1.35e-5
ANGLE_TOL = 4 * 8.2e-5
DESC_TOL = 4 * 3.4e-3


# ---------------------------------------------------------------- atan2
def atan2_real(y, x):
    return np.mod(np.degrees(np.arctan2(y, x)), 360.0).astype(np.result_type(y, x))


def atan2_cv(y, x):
    """The polynomial of cv::fastAtan2 in the arithmetic of its arguments: degrees in [0, 360]."""
    ft = np.result_type(y, x)
    ax, ay = np.abs(x), np.abs(y)
    eps = ft.type(2.220446049250313e-16)
    swap = ax < ay
    c = np.where(swap, ax / (ay + eps), ay / (ax + eps))
    c2 = c * c
    a = (((ft.type(-2.5397272) * c2 + ft.type(8.9140005)) * c2 - ft.type(18.667446)) * c2 + ft.type(57.283627)) * c
    a = np.where(swap, 90 - a, a)
    a = np.where(x < 0, 180 - a, a)
    return np.where(y < 0, 360 - a, a).astype(ft)


ATAN2 = {"real": atan2_real, "cv": atan2_cv}


# ---------------------------------------------------------------- scale space
def reflect101(c, n):
    c = np.asarray(c, np.int64)
    if n == 1:
        return np.zeros_like(c)
    m = np.mod(c, 2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def base_image(img, ft=np.float64):
    """x2 bilinear, half-pixel centres, edge-replicated: (2H, 2W)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2

    def axis(n):
        s = (np.arange(2 * n) + 0.5) * 0.5 - 0.5
        i0 = np.floor(s).astype(np.int64)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), (s - i0).astype(ft)

    ya, yb, fy = axis(img.shape[0])
    xa, xb, fx = axis(img.shape[1])
    a = img.astype(ft)
    rows = a[:, xa] * (1 - fx) + a[:, xb] * fx
    return rows[ya] * (1 - fy)[:, None] + rows[yb] * fy[:, None]


def sigma_ladder():
    """(total sigma of level i, the increment that takes level i - 1 to it (level 0: from the base's nominal 1), taps)."""
    k = 2.0 ** (1.0 / NOL)
    total = [SIGMA * k ** i for i in range(NG)]
    inc = [math.sqrt(max(SIGMA ** 2 - 1.0, 0.01))] + [math.sqrt(total[i] ** 2 - total[i - 1] ** 2) for i in range(1, NG)]
    taps = [int(np.rint(8 * s + 1)) | 1 for s in inc]
    return total, inc, taps


def gauss_weights(sigma, taps):
    d = np.arange(taps) - taps // 2
    w = np.exp(-d * d / (2.0 * sigma * sigma))
    return w / w.sum()


def blur(img, sigma, taps):
    """Separable Gaussian of `taps` taps on the reflect-101 image, in img's arithmetic."""
    ft = img.dtype.type
    w = gauss_weights(sigma, taps).astype(ft)
    r = taps // 2
    H, W = img.shape
    xs = reflect101(np.arange(-r, W + r), W)
    ys = reflect101(np.arange(-r, H + r), H)
    p = img[:, xs]
    t = np.zeros_like(img)
    for k in range(taps):
        t = t + w[k] * p[:, k:k + W]
    p = t[ys, :]
    out = np.zeros_like(img)
    for k in range(taps):
        out = out + w[k] * p[k:k + H, :]
    return out


def num_octaves(H, W):
    """Octaves of an H x W input: cvRound(log2(min side of the doubled image) - 2), and none smaller than 2 * 5 + 3."""
    n = int(np.rint(math.log(min(2 * H, 2 * W)) / math.log(2.0) - 2))
    h, w, k = 2 * H, 2 * W, 0
    while k < n and w >= 2 * BORDER + 3 and h >= 2 * BORDER + 3:
        k, w, h = k + 1, w // 2, h // 2
    return k


def pyramid(img, ft=np.float64):
    """[(G (6, h, w), D (5, h, w)) per octave]."""
    _, inc, taps = sigma_ladder()
    out = []
    for o in range(num_octaves(*np.shape(img))):
        g = [blur(base_image(img, ft), inc[0], taps[0]) if o == 0 else out[-1][0][NOL][::2, ::2][:h // 2, :w // 2]]
        h, w = g[0].shape
        for i in range(1, NG):
            g.append(blur(g[-1], inc[i], taps[i]))
        G = np.stack(g)
        out.append((G, G[1:] - G[:-1]))
    return out


def pyramid_bounds(n_oct):
    """(eps_G[o][i], eps_D[o][i]): how far a float32 implementation's Gaussian / DoG image may be from the definition's, in
    grey levels.  A separable pass with normalised weights on values <= 255 errs by at most (taps + 1) u 255 in its sum, and
    by u 255 more for its weights' own rounding; its weights sum to one, so the error of its input passes through once.  The
    base image's three float32 lerps add 3 u 255.  Octave o + 1 starts from octave o's level 3.  eps_D = eps_G(i + 1) +
    eps_G(i) + one ulp of a value below 255."""
    _, _, taps = sigma_ladder()
    eg, ed = [], []
    for o in range(n_oct):
        e = [(3 * U * 255 if o == 0 else eg[-1][NOL]) + (2 * (taps[0] + 2) * U * 255 if o == 0 else 0.0)]
        for i in range(1, NG):
            e.append(e[-1] + 2 * (taps[i] + 2) * U * 255)
        eg.append(e)
        ed.append([e[i + 1] + e[i] + 2 * U * 255 for i in range(NG - 1)])
    return eg, ed


# ---------------------------------------------------------------- extrema and refinement
_NBR = [(dl, dy, dx) for dl in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dl, dy, dx) != (0, 0, 0)]


def candidates(D, eps_d):
    """Extrema of the 26 neighbours with |D| > threshold inside the 5-pixel border: [(layer, r, c, margin, bound)], margin
    the smallest of |D| - threshold and the 26 signed differences, bound = the eps_D of the layers involved.  Points that
    fail by less than 2 * bound are included (negative margin)."""
    out = []
    _, H, W = D.shape
    if H <= 2 * BORDER or W <= 2 * BORDER:
        return out
    for layer in range(1, NOL + 1):
        bound = max(eps_d[layer - 1:layer + 2])
        v = D[layer, BORDER:H - BORDER, BORDER:W - BORDER].astype(np.float64)
        sgn = np.where(v > 0, 1.0, -1.0)
        m = np.abs(v) - DOG_THRESHOLD
        for dl, dy, dx in _NBR:
            nb = D[layer + dl, BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx]
            m = np.minimum(m, sgn * (v - nb))
        for r, c in zip(*np.nonzero(m > -2 * bound)):
            out.append((layer, int(r) + BORDER, int(c) + BORDER, float(m[r, c]), bound))
    return out


def _derivatives(D, layer, r, c):
    ft = D.dtype.type
    img, prv, nxt = D[layer], D[layer - 1], D[layer + 1]
    g = np.array([(img[r, c + 1] - img[r, c - 1]) * ft(0.5), (img[r + 1, c] - img[r - 1, c]) * ft(0.5),
                  (nxt[r, c] - prv[r, c]) * ft(0.5)], ft)
    v2 = img[r, c] * ft(2)
    dxx, dyy, dss = img[r, c + 1] + img[r, c - 1] - v2, img[r + 1, c] + img[r - 1, c] - v2, nxt[r, c] + prv[r, c] - v2
    dxy = (img[r + 1, c + 1] - img[r + 1, c - 1] - img[r - 1, c + 1] + img[r - 1, c - 1]) * ft(0.25)
    dxs = (nxt[r, c + 1] - nxt[r, c - 1] - prv[r, c + 1] + prv[r, c - 1]) * ft(0.25)
    dys = (nxt[r + 1, c] - nxt[r - 1, c] - prv[r + 1, c] + prv[r - 1, c]) * ft(0.25)
    return g, np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], ft)


def refine(D, octave, layer, r, c, eps_d):
    """Up to five Newton steps of the quadratic fit, then the contrast and edge tests.  Returns a namespace: ok, reason,
    layer, r, c, x = (xc, xr, xi), trajectory [(layer, r, c, x)], ratio = the smallest margin / (2 * bound) on the path,
    and for an accepted point response, scl (= 1.6 * 2^((layer + xi) / 3)) with their bounds x_bound, resp_bound, scl_bound.
    First-order bound of the solve: |dx| <= |H^-1| (|dg| + |dH| |x|), |dg| <= sqrt(3) eps, |dH|_F <= sqrt(54) eps (second
    differences carry 4 eps, mixed ones eps), eps the largest eps_D of the three layers read."""
    _, H, W = D.shape
    res = types.SimpleNamespace(ok=False, reason="", trajectory=[], ratio=np.inf, why="", octave=octave)

    def decide(margin, bound, name):
        ratio = margin / (2 * bound) if bound > 0 else np.inf
        if ratio < res.ratio:
            res.ratio, res.why = ratio, name

    x = None
    for step in range(MAX_STEPS + 1):
        if step == MAX_STEPS:
            res.reason = "steps"
            return res
        eps = max(eps_d[layer - 1:layer + 2])
        g, Hm = _derivatives(D, layer, r, c)
        try:
            x = -np.linalg.solve(Hm, g)
            hinv = float(np.linalg.norm(np.linalg.inv(Hm.astype(np.float64)), 2))
        except np.linalg.LinAlgError:
            res.reason, res.ratio = "singular", 0.0
            return res
        xn = float(np.linalg.norm(x))
        xb = hinv * (math.sqrt(3) * eps + math.sqrt(54) * eps * xn) + xn * F32_SLACK * np.linalg.cond(Hm.astype(np.float64))
        res.trajectory.append((layer, r, c, x.copy()))
        ax = np.abs(x).astype(np.float64)
        if np.all(ax < 0.5):
            decide(float(np.min(0.5 - ax)), xb, "offset")
            break
        if np.any(ax > 7e8):
            res.reason = "diverged"
            return res
        # leaving the loop is decided by the largest component; each move by its distance to the next half-integer
        decide(float(np.max(ax) - 0.5), xb, "offset")
        decide(float(np.min(np.abs(ax - np.floor(ax) - 0.5))), xb, "move")
        c, r, layer = c + int(np.rint(x[0])), r + int(np.rint(x[1])), layer + int(np.rint(x[2]))
        if layer < 1 or layer > NOL or c < BORDER or c >= W - BORDER or r < BORDER or r >= H - BORDER:
            res.reason = "left"
            return res
    res.layer, res.r, res.c, res.x, res.x_bound = layer, r, c, x, xb
    gn = float(np.linalg.norm(g))
    contr = D[layer, r, c] + (g[0] * x[0] + g[1] * x[1] + g[2] * x[2]) * D.dtype.type(0.5)
    res.response = abs(float(contr)) / 255.0
    res.resp_bound = (eps + 0.5 * (math.sqrt(3) * eps * xn + gn * xb)) / 255.0 + res.response * F32_SLACK
    decide(abs(res.response * NOL - CONTRAST_THR), NOL * res.resp_bound, "contrast")
    if res.response * NOL < CONTRAST_THR:
        res.reason = "contrast"
        return res
    dxx, dyy, dxy = float(Hm[0, 0]), float(Hm[1, 1]), float(Hm[0, 1])
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    f = (EDGE_THR + 1) ** 2 * det - EDGE_THR * tr * tr
    fb = (EDGE_THR + 1) ** 2 * (4 * eps * (abs(dxx) + abs(dyy)) + 2 * eps * abs(dxy)) + 2 * EDGE_THR * abs(tr) * 8 * eps
    decide(abs(f), fb, "edge")
    if det <= 0 or f <= 0:
        res.reason = "edge"
        return res
    res.scl = SIGMA * 2.0 ** ((layer + float(x[2])) / NOL)
    res.scl_bound = res.scl * (math.log(2) / NOL * xb + F32_SLACK)
    res.ok = True
    return res


# ---------------------------------------------------------------- orientation
def _gradients(g, ys, xs):
    """dx, dy (y up) at the pixel grid ys x xs of g, and the mask of pixels with all four neighbours inside."""
    H, W = g.shape
    ok = ((ys > 0) & (ys < H - 1))[:, None] & ((xs > 0) & (xs < W - 1))[None, :]
    yc, xc = np.clip(ys, 1, max(H - 2, 1)), np.clip(xs, 1, max(W - 2, 1))
    dx = g[np.ix_(yc, xc + 1)] - g[np.ix_(yc, xc - 1)]
    dy = g[np.ix_(yc - 1, xc)] - g[np.ix_(yc + 1, xc)]
    return dx, dy, ok


def orientation_histogram(g, r, c, radius, sigma, atan2="cv", ties=None):
    """(raw, smoothed) 36-bin histograms of the gradients within `radius` of (r, c): weight exp(-(i^2 + j^2) / 2 sigma^2)
    times the magnitude, into bin rint(angle / 10); smoothed by [1 4 6 4 1] / 16, circularly."""
    ft = g.dtype.type
    off = np.arange(-radius, radius + 1)
    dx, dy, ok = _gradients(g, r + off, c + off)
    w = np.exp(((off * off)[:, None] + (off * off)[None, :]).astype(ft) * ft(-1.0 / (2.0 * sigma * sigma)))
    ori = ATAN2[atan2](dy, dx)
    mag = np.sqrt(dx * dx + dy * dy)
    b = np.mod(np.rint(ori * ft(0.1)).astype(np.int64), ORI_BINS)
    raw = np.bincount(b[ok], weights=(w * mag)[ok].astype(np.float64), minlength=ORI_BINS).astype(ft)
    sm = ((np.roll(raw, 2) + np.roll(raw, -2)) * ft(1 / 16) + (np.roll(raw, 1) + np.roll(raw, -1)) * ft(4 / 16)
          + raw * ft(6 / 16))
    if ties is not None:
        # the share of the histogram that sits within BIN_TIE_DEG of a bin boundary and lands on either side by rounding
        t = ori.astype(np.float64) * 0.1
        ax, ay = np.abs(dx).astype(np.float64), np.abs(dy).astype(np.float64)
        near = ok & ((np.abs(t - np.floor(t) - 0.5) * 10 < BIN_TIE_DEG)
                     | (np.abs(ax - ay) <= np.radians(BIN_TIE_DEG) * np.maximum(ax, ay)))
        ties.append(float((w * mag)[near].sum() / sm.max()) if sm.max() > 0 else 0.0)
    return raw, sm


def orientation_peaks(hist, tol=HIST_TOL):
    """[(bin j, angle, margin, bound)]: local maxima of the smoothed histogram that reach 0.8 of its maximum, with the
    parabola's peak as the angle (360 - 10 bin, clockwise on screen).  margin: the smallest of hist[j] - hist[j +- 1] and
    hist[j] - 0.8 max; bound = tol * max (each compared value may be off by that).  Near-peaks within 2 * bound are included."""
    hist = np.asarray(hist)
    mx = float(hist.max())
    out = []
    if not mx > 0:
        return out
    bound = tol * mx
    for j in range(ORI_BINS):
        hl, hj, hr = float(hist[j - 1]), float(hist[j]), float(hist[(j + 1) % ORI_BINS])
        margin = min(hj - hl, hj - hr, hj - ORI_PEAK * mx)
        if margin <= -2 * bound:
            continue
        den = hl - 2 * hj + hr
        b = j + (0.5 * (hl - hr) / den if den != 0 else 0.0)
        b = b + ORI_BINS if b < 0 else (b - ORI_BINS if b >= ORI_BINS else b)
        angle = 360.0 - 10.0 * b
        if abs(angle - 360.0) < 2.0 ** -23:
            angle = 0.0
        out.append((j, angle, margin, bound))
    return out


# ---------------------------------------------------------------- descriptor
def descriptor(g, pxi, pyi, ori_deg, scl, atan2="cv"):
    """4 x 4 x 8 descriptor around the integer centre (pxi, pyi) of Gaussian image g: the frame turned by ori_deg (= 360 -
    the keypoint's angle), cells 3 scl wide, trilinear binning of Gaussian-weighted gradient magnitudes.  Returns
    (unrounded, rounded): after the 0.2 clamp and the x 512 normalisation; then rint and saturation to 0..255."""
    ft = g.dtype.type
    d, n = DESC_D, DESC_N
    H, W = g.shape
    hw = ft(DESC_SCL * scl)
    radius = min(int(np.rint(float(hw) * math.sqrt(2) * (d + 1) * 0.5)), int(math.sqrt(H * H + W * W)))
    t = math.radians(ori_deg)
    cos_t, sin_t = ft(math.cos(t)) / hw, ft(math.sin(t)) / hw
    off = np.arange(-radius, radius + 1)
    i, j = off[:, None].astype(ft), off[None, :].astype(ft)
    c_rot, r_rot = j * cos_t - i * sin_t, j * sin_t + i * cos_t
    rbin, cbin = r_rot + ft(d / 2 - 0.5), c_rot + ft(d / 2 - 0.5)
    dx, dy, ok = _gradients(g, pyi + off, pxi + off)
    ok = ok & (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d)
    rbin, cbin, c_rot, r_rot, dx, dy = rbin[ok], cbin[ok], c_rot[ok], r_rot[ok], dx[ok], dy[ok]
    mag = np.sqrt(dx * dx + dy * dy) * np.exp((c_rot * c_rot + r_rot * r_rot) * ft(-1.0 / (d * d * 0.5)))
    obin = (ATAN2[atan2](dy, dx) - ft(ori_deg)) * ft(n / 360.0)
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    hist = np.zeros((d + 2, d + 2, n), np.float64)
    for a, wr in ((0, 1 - fr), (1, fr)):
        for b, wc in ((0, 1 - fc), (1, fc)):
            for e, wo in ((0, 1 - fo), (1, fo)):
                np.add.at(hist, (r0 + 1 + a, c0 + 1 + b, np.mod(o0 + e, n)), (mag * wr * wc * wo).astype(np.float64))
    raw = hist[1:d + 1, 1:d + 1, :].reshape(-1).astype(ft)
    thr = np.sqrt((raw * raw).sum()) * ft(DESC_CLAMP)
    raw = np.minimum(raw, thr)
    unrounded = raw * (ft(512) / max(np.sqrt((raw * raw).sum()), ft(2.0 ** -23)))
    return unrounded, np.clip(np.rint(unrounded), 0, 255)


# ---------------------------------------------------------------- final order, duplicates, cap
def final_order(rows):
    """Indices that sort (n, 6) rows (x, y, size, angle, response, octave) by x, y, size descending, angle, response
    descending, octave descending."""
    rows = np.asarray(rows)
    return np.lexsort((-rows[:, 5], -rows[:, 4], rows[:, 3], -rows[:, 2], rows[:, 1], rows[:, 0]))


def remove_duplicates(rows):
    """Mask over SORTED rows: a row equal to the last kept row in x, y, size and angle goes."""
    keep = np.ones(len(rows), bool)
    last = None
    for k in range(len(rows)):
        if last is not None and np.array_equal(rows[k, :4], rows[last, :4]):
            keep[k] = False
        else:
            last = k
    return keep


def cap_rows(rows, cap):
    """Mask over sorted, de-duplicated rows: the `cap` strongest by response stay, ties at the cap-th response going to
    the earliest rows; order unchanged."""
    n = len(rows)
    if n <= cap:
        return np.ones(n, bool)
    resp = np.asarray(rows)[:, 4]
    thr = np.sort(resp)[::-1][cap - 1]
    keep = resp > thr
    ties = np.nonzero(resp == thr)[0][:cap - int(keep.sum())]
    keep[ties] = True
    return keep


def finish(rows, cap=None):
    """Indices into `rows` of the keypoints returned, in the order returned."""
    rows = np.asarray(rows).reshape(-1, 6)
    idx = final_order(rows)
    idx = idx[remove_duplicates(rows[idx])]
    return idx if cap is None else idx[cap_rows(rows[idx], cap)]


# ---------------------------------------------------------------- the whole
def detect(img, atan2="cv", ft=np.float64, descriptors=True, pyr=None):
    """Namespace: pyramid, eps_g, eps_d, keypoints, rejected.  A keypoint record (one per candidate and histogram peak)
    has octave, layer, r, c, x = (xc, xr, xi), bin, xy, size, angle, response, hist (smoothed), ori_radius, desc_radius,
    desc_raw, desc, their bounds xy_bound, size_bound, resp_bound, ratio (the smallest margin / (2 bound) on its path), why (that
    decision's name), decided (ratio > 1) and accepted (the definition itself returns it: an undecided record kept only as a
    counterpart has accepted = False); `rows` holds the float32 (x, y, size,
    angle, response, octave - 1) rows of all of them in detection order."""
    img = np.ascontiguousarray(img, np.uint8)
    pyr = pyramid(img, ft) if pyr is None else pyr
    eps_g, eps_d = pyramid_bounds(len(pyr))
    out = types.SimpleNamespace(pyramid=pyr, eps_g=eps_g, eps_d=eps_d, keypoints=[], rejected=[])
    for o, (G, D) in enumerate(pyr):
        for layer, r, c, margin, bound in candidates(D, eps_d[o]):
            res = refine(D, o, layer, r, c, eps_d[o])
            res.start = (layer, r, c)
            if margin / (2 * bound) < res.ratio:
                res.ratio, res.why = margin / (2 * bound), "extremum"
            res.decided, res.accepted = res.ratio > 1, margin >= 0
            if not res.ok:
                out.rejected.append(res)
                continue
            xo = res.c + float(res.x[0]), res.r + float(res.x[1])
            rr, dr = ORI_RADIUS * res.scl, DESC_SCL * res.scl * math.sqrt(2) * (DESC_D + 1) * 0.5
            ratio, why = min((res.ratio, res.why),
                             (abs(rr - math.floor(rr) - 0.5) / (2 * ORI_RADIUS * res.scl_bound), "ori_radius"),
                             (abs(dr - math.floor(dr) - 0.5) / (2 * dr / res.scl * res.scl_bound), "desc_radius"))
            ties = []
            raw, hist = orientation_histogram(G[res.layer], res.r, res.c, int(np.rint(rr)), ORI_SIG * res.scl, atan2, ties)
            if ties[0] > BIN_TIE_MASS:
                ratio, why = min((ratio, why), (BIN_TIE_MASS / ties[0], "bin tie"))
            for j, angle, pm, pb in orientation_peaks(hist):
                k = types.SimpleNamespace(octave=o, layer=res.layer, r=res.r, c=res.c, x=res.x, bin=j, start=res.start,
                                          trajectory=res.trajectory, hist=hist, hist_raw=raw, scl=res.scl,
                                          ori_radius=int(np.rint(rr)), desc_radius=int(np.rint(dr)))
                k.xy = (xo[0] * 2.0 ** o * 0.5, xo[1] * 2.0 ** o * 0.5)
                k.xy_bound = res.x_bound * 2.0 ** o * 0.5 + max(k.xy) * F32_SLACK
                k.size, k.size_bound = res.scl * 2.0 ** o, res.scl_bound * 2.0 ** o
                k.response, k.resp_bound = res.response, res.resp_bound
                k.angle = angle
                k.ratio, k.why = min((ratio, why), (pm / (2 * pb), "peak"))
                hl, hj, hr = hist[j - 1], hist[j], hist[(j + 1) % ORI_BINS]
                k.accepted = bool(margin >= 0 and hj > hl and hj > hr and hj >= ORI_PEAK * hist.max())
                k.decided = k.ratio > 1
                if descriptors:
                    ori = 360.0 - angle
                    k.desc_raw, k.desc = descriptor(G[res.layer], int(np.rint(xo[0])), int(np.rint(xo[1])),
                                                    0.0 if abs(ori - 360.0) < 2.0 ** -23 else ori, res.scl, atan2)
                out.keypoints.append(k)
    out.rows = np.array([[k.xy[0], k.xy[1], k.size, k.angle, k.response, k.octave - 1] for k in out.keypoints],
                        np.float32).reshape(-1, 6)
    return out
