"""The definition the Lucas-Kanade tracker and its pyramid are pinned to.  TEST INFRASTRUCTURE.

cv2.calcOpticalFlowPyrLK as the header of oracle/csrc/klt.c describes it, stated in real arithmetic (float64 NumPy,
vectorised over points) with none of klt.c's fixed-point steps: no 14-bit weights, no 5-bit patch, no integer Scharr, no
float32 solve, no stopping rules.  It does not import oracle.native.  The oracle (tests/test_klt_reference_host.py) and the
kernels (tests/test_gpu_klt_reference.py) are compared with it; quantisation_bound() says how far their fixed point may be
from it.

Conventions: a point is (x, y); images are (H, W) uint8; the win x win window of a point p has its samples at
p - (win - 1) / 2 + (i, j), i, j = 0 .. win - 1.  Pixels outside the image are the reflect-101 image; the derivative is the
Scharr (3, 10, 3) derivative of the reflect-101 image at pixels inside the image and ZERO at pixels outside it; both are
read between pixels with bilinear weights.

  T   = bilinear I                      g = bilinear Scharr(I) / 32   (grey levels per pixel: 32 = (3 + 10 + 3) * 2)
  G   = sum g g^T                       lambda = lambda_min(G) * 1024 * 2^-20 / win^2   (the unit min_eig is compared in)
  d   = J(q + .) - T                    b = sum d g
  delta = -G^-1 b                       e = mean |d|

Position rule: a window whose first sample is x0 = p - (win - 1) / 2 is read only when -win <= floor(x0) <= W - 1 (and the
same along y); it flips at x0 = -win and x0 = W.  A level whose template window fails the rule, whose lambda is below min_eig
or whose det(G) in the kernel's unit, det(G) * 2^-20, is below FLT_EPSILON is skipped: the point passes through it unchanged,
and is lost only when the level is level 0.  An iterate or the final point failing the rule at level 0 loses the point."""
import types

import numpy as np

#: What one interpolated image sample of the kernel may be off by, in grey levels: the patch keeps 5 fractional bits (half a
#: unit of 2^-5), and each of the four bilinear weights is rounded to 2^-14 (error 2^-15 each, on pixels up to 255).
EPS_SAMPLE = 2.0 ** -6 + 4 * 255 * 2.0 ** -15
#: The same for a derivative sample, in grey levels per pixel: the interpolated Scharr value is rounded to a whole number
#: (2^-1 Scharr units = 2^-1 / 32), and the weight term grows by the Scharr gain 32 and shrinks by it again in g's unit.
EPS_GRAD = 2.0 ** -1 / 32 + 4 * 255 * 2.0 ** -15
FLT_EPSILON = 2.0 ** -23
LAMBDA_SCALE = 1024 * 2.0 ** -20          # lambda_min(G) / win^2 times this is what min_eig is compared with
POSITION_MARGIN = 1e-3                    # a window-position test this close to flipping is undecided


def reflect101(c, n):
    """Index c of the reflect-101 extension of an axis of n pixels (gfedcb|abcdefgh|gfedcba), by the periodic formula:
    any distance outside, any n >= 1."""
    c = np.asarray(c, np.int64)
    if n == 1:
        return np.zeros_like(c)
    period = 2 * (n - 1)
    m = np.mod(c, period)
    return np.where(m < n, m, period - m)


def pad_reflect101(img, pad):
    H, W = img.shape
    return img[np.ix_(reflect101(np.arange(-pad, H + pad), H), reflect101(np.arange(-pad, W + pad), W))]


def pyr_down(img):
    """cv2.pyrDown: [1 4 6 4 1] x [1 4 6 4 1] at the even pixels of the reflect-101 image, (s + 128) >> 8.  Exact integers."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    k = np.array([1, 4, 6, 4, 1], np.int64)
    taps = np.arange(-2, 3)
    ys = reflect101(2 * np.arange((H + 1) // 2)[:, None] + taps, H)          # (Hd, 5)
    xs = reflect101(2 * np.arange((W + 1) // 2)[:, None] + taps, W)          # (Wd, 5)
    rows = (img.astype(np.int64)[:, xs] * k).sum(axis=2)                     # (H, Wd)
    s = (rows[ys, :] * k[None, :, None]).sum(axis=1)                         # (Hd, Wd)
    return ((s + 128) >> 8).astype(np.uint8)


def num_levels(H, W, win, max_level):
    """Levels the pyramid builder keeps: it stops before a level that is not larger than the window on both sides."""
    levels = 1
    for _ in range(max_level):
        H, W = (H + 1) // 2, (W + 1) // 2
        if W <= win or H <= win:
            break
        levels += 1
    return levels


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1]))
    return out


class Level:
    """One pyramid level prepared for window reads: the reflect-101 image and the zero-outside Scharr derivatives, all
    with win + 2 pixels of border (the position rule keeps every read inside it)."""

    def __init__(self, img, win):
        f = np.asarray(img).astype(np.float64)
        self.H, self.W = f.shape
        self.win, self.pad = win, win + 2
        e = pad_reflect101(f, 1)
        gx = 3 * (e[:-2, 2:] - e[:-2, :-2]) + 10 * (e[1:-1, 2:] - e[1:-1, :-2]) + 3 * (e[2:, 2:] - e[2:, :-2])
        gy = 3 * (e[2:, :-2] - e[:-2, :-2]) + 10 * (e[2:, 1:-1] - e[:-2, 1:-1]) + 3 * (e[2:, 2:] - e[:-2, 2:])
        self.pitch = self.W + 2 * self.pad
        self.I = pad_reflect101(f, self.pad).ravel()
        self.gx = np.pad(gx / 32.0, self.pad).ravel()
        self.gy = np.pad(gy / 32.0, self.pad).ravel()

    def position_ok(self, x0):
        ix, iy = np.floor(x0[:, 0]), np.floor(x0[:, 1])
        return (ix >= -self.win) & (ix <= self.W - 1) & (iy >= -self.win) & (iy <= self.H - 1)

    def position_margin(self, x0):
        """Distance of a window's first sample from the nearest place where the position rule flips."""
        m = np.minimum(np.abs(x0[:, 0] + self.win), np.abs(x0[:, 0] - self.W))
        return np.minimum(m, np.minimum(np.abs(x0[:, 1] + self.win), np.abs(x0[:, 1] - self.H)))

    def window(self, x0, planes):
        """Bilinear reads of `planes` over the win x win windows whose first samples are x0 (N, 2); (N, win, win) each.
        Windows that fail the position rule are read at the nearest place that passes it (the caller discards them)."""
        x = np.clip(x0[:, 0], -self.win, self.W - 2.0 ** -20)
        y = np.clip(x0[:, 1], -self.win, self.H - 2.0 ** -20)
        ix, iy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
        a, b = (x - ix)[:, None, None], (y - iy)[:, None, None]
        o = np.arange(self.win)
        at = ((iy + self.pad)[:, None, None] + o[None, :, None]) * self.pitch + (ix + self.pad)[:, None, None] + o[None, None, :]
        w00, w01, w10, w11 = (1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b
        return [w00 * f[at] + w01 * f[at + 1] + w10 * f[at + self.pitch] + w11 * f[at + self.pitch + 1] for f in planes]


def _template(LI, p):
    win = LI.win
    T, gx, gy = LI.window(p - (win - 1) / 2.0, (LI.I, LI.gx, LI.gy))
    t = types.SimpleNamespace(win=win, T=T, gx=gx, gy=gy)
    t.G11, t.G12, t.G22 = (gx * gx).sum(axis=(1, 2)), (gx * gy).sum(axis=(1, 2)), (gy * gy).sum(axis=(1, 2))
    t.lam_min = 0.5 * (t.G11 + t.G22 - np.sqrt((t.G11 - t.G22) ** 2 + 4 * t.G12 ** 2))
    t.lam = t.lam_min * LAMBDA_SCALE / (win * win)
    t.det = (t.G11 * t.G22 - t.G12 ** 2) * LAMBDA_SCALE ** 2            # det of the kernel's 2^-20-scaled matrix
    return t


def _take(t, idx):
    return types.SimpleNamespace(win=t.win, **{k: v[idx] for k, v in vars(t).items() if k != "win"})


def _residual(LJ, t, q):
    """The step state of template t (N points) against image J at q: adds d, b1/b2, delta and e."""
    s = types.SimpleNamespace(**vars(t))
    x0 = q - (t.win - 1) / 2.0
    Jv, = LJ.window(x0, (LJ.I,))
    s.d = Jv - t.T
    s.b1, s.b2 = (s.d * t.gx).sum(axis=(1, 2)), (s.d * t.gy).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        det = t.G11 * t.G22 - t.G12 ** 2
        s.delta = np.stack([(t.G12 * s.b2 - t.G22 * s.b1) / det, (t.G12 * s.b1 - t.G11 * s.b2) / det], axis=1)
    s.delta[~np.isfinite(s.delta).all(axis=1)] = 0.0
    s.e = np.abs(s.d).mean(axis=(1, 2))
    s.LJ, s.x0 = LJ, x0
    return s


def lk_step_state(I, J, p, q, win):
    """One level's Lucas-Kanade step for points p (N, 2) of image I sought at q (N, 2) in image J: T, gx, gy (N, win, win),
    G11/G12/G22, lam_min = lambda_min(G), lam (min_eig's unit), det (FLT_EPSILON's unit), d, b1/b2, delta (N, 2), e."""
    p, q = np.asarray(p, np.float64).reshape(-1, 2), np.asarray(q, np.float64).reshape(-1, 2)
    return _residual(Level(J, win), _template(Level(I, win), p), q)


def step_gain(s):
    """||d(q + delta)/dq||_2 per point: how much of an offset of the start survives one step.  The bilinear interpolant is
    differentiable inside a pixel cell: dJ/dx = (1 - b)(J01 - J00) + b (J11 - J10), and every sample of a window shares the
    cell offsets; d delta/dq = -G^-1 sum g (grad J)^T."""
    LJ = s.LJ
    h = 1e-6          # one-sided difference inside the cell (towards the cell's middle): exact for a bilinear surface
    fx, fy = s.x0[:, 0] - np.floor(s.x0[:, 0]), s.x0[:, 1] - np.floor(s.x0[:, 1])
    sx, sy = np.where(fx < 0.5, h, -h), np.where(fy < 0.5, h, -h)
    J0, = LJ.window(s.x0, (LJ.I,))
    Jx, = LJ.window(s.x0 + np.stack([sx, 0 * sx], axis=1), (LJ.I,))
    Jy, = LJ.window(s.x0 + np.stack([0 * sy, sy], axis=1), (LJ.I,))
    dJx, dJy = (Jx - J0) / sx[:, None, None], (Jy - J0) / sy[:, None, None]
    M = np.empty((len(fx), 2, 2))
    M[:, 0, 0], M[:, 0, 1] = (s.gx * dJx).sum(axis=(1, 2)), (s.gx * dJy).sum(axis=(1, 2))
    M[:, 1, 0], M[:, 1, 1] = (s.gy * dJx).sum(axis=(1, 2)), (s.gy * dJy).sum(axis=(1, 2))
    G = np.empty_like(M)
    G[:, 0, 0], G[:, 0, 1], G[:, 1, 0], G[:, 1, 1] = s.G11, s.G12, s.G12, s.G22
    ok = s.lam_min > 0
    out = np.full(len(fx), np.inf)
    if ok.any():
        out[ok] = np.linalg.norm(np.eye(2) - np.linalg.solve(G[ok], M[ok]), ord=2, axis=(1, 2))
    return out


def quantisation_bound(s):
    """Per point, how far one step of the kernel's fixed point may land from the definition's step, to first order (px).

    The kernel computes the same sums from rounded samples.  Write d', g' for its residual and derivative samples in the
    definition's units:
      |d' - d| <= eps_I = EPS_SAMPLE   (5-bit patch: 2^-6; 14-bit weights: 4 * 255 * 2^-15)
      |g' - g| <= eps_g = EPS_GRAD     (whole-number Scharr: 2^-1 / 32; weights: 4 * 255 * 2^-15) per component
    With b = sum d g and G = sum g g^T:
      |db_x| <= sum |g_x| * eps_I + sum |d| * eps_g          (and the same for y; ||db|| is the length of the two)
      ||dG|| <= sum (|dg| |g| + |g| |dg|) <= 2 sqrt(2) eps_g * sum |g|       (|dg| <= sqrt(2) eps_g: both components)
    and delta = -G^-1 b moves by  -G^-1 db + G^-1 dG G^-1 b = -G^-1 db - G^-1 dG delta, hence
      |d delta| <= ||G^-1|| * (sum |g| eps_I + sum |d| eps_g) + ||G^-1|| * ||dG|| * |delta|,   ||G^-1|| = 1 / lambda_min(G).
    Terms of second order in eps are dropped (the tests allow twice the bound for them).

    Not counted: the window sums are exact integers in the kernel; their one conversion to float32 and the float32 2x2
    solve are relative errors near 2^-24, and the float32 coordinate arithmetic (p / 2^l - half, q + delta, q + half) is a
    few units in the last place of a coordinate, about 1e-5 px: three to four orders below the terms above.

    eps_I is charged once per residual.  d' = J' - T' is made of two rounded samples, each within eps_I, so a strict worst
    case would charge 2 eps_I; the weight term in eps_I is already a worst case over pixel values (four pixels spanning
    0 .. 255 under every sample, where real neighbours differ by tens), which covers that several times over, and the
    measured shares say so: a few percent of the bound for one step, about the whole tolerance eps + 2 * bound only at a
    fixed point whose step contracts slowly (step_gain near 0.8: a fixed point moves by up to 1 / (1 - gain) times what
    a step moves)."""
    sgx, sgy = np.abs(s.gx).sum(axis=(1, 2)), np.abs(s.gy).sum(axis=(1, 2))
    sd = np.abs(s.d).sum(axis=(1, 2))
    db = np.hypot(sgx * EPS_SAMPLE + sd * EPS_GRAD, sgy * EPS_SAMPLE + sd * EPS_GRAD)
    dG = 2 * np.sqrt(2.0) * EPS_GRAD * np.hypot(s.gx, s.gy).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(s.lam_min > 0, 1.0 / s.lam_min, np.inf)
        bound = inv * db + inv * dG * np.hypot(s.delta[:, 0], s.delta[:, 1])
    return np.where(np.isfinite(bound), bound, np.inf)


def track(prev, nxt, pts, win, max_level, iters, min_eig=1e-4):
    """The pyramid loop with `iters` full Newton steps per level: no eps stop, no ping-pong stop, no quantisation.  (A point
    whose step has fallen below 1e-13 px is not stepped further: the steps left would not move it.)

    Returns a namespace, N points and L = num_levels(...) levels:
      q (N, 2)        the tracked point at level 0
      lam, det (L, N) lambda and det(G) of each level's template in the units of min_eig / FLT_EPSILON; nan where the
                      template window fails the position rule
      x0 (L, N, 2)    first sample of each level's template window;  template_ok (L, N) the position rule on it,
                      template_margin (L, N) its distance from flipping
      used (L, N)     the level was tracked on (not skipped)
      last_step (N)   length of the last step taken at level 0 (nan if none);  steps (iters, N) the length of every step
                      taken at level 0 (nan where none was)
      bound (N)       quantisation_bound at q on level 0;  gain (N) step_gain there
      chain (N)       first-order bound on |kernel - q| when the kernel, too, takes exactly `iters` = 1 step per level:
                      chain_top = bound_top, chain_l = bound_l + gain_l * 2 chain_(l+1)  -- the start of level l is twice the
                      point of level l + 1, so it inherits twice its error, of which the step keeps the share step_gain; a
                      skipped level only doubles it.  With one level it is quantisation_bound itself.
      e (N)           mean |J - T| at q, level 0
      iter_margin (N) smallest position_margin of any iterate or of the final point at level 0
      lost (N)        an iterate or the final point failed the position rule at level 0
      walked (N)      an iterate failed the position rule at some level: the kernel's own path decides what happens next, so
                      the point is frozen there and left undecided"""
    pts = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 2)
    N = len(pts)
    H, W = np.asarray(prev).shape
    L = num_levels(H, W, win, max_level)
    pI, pJ = pyramid(prev, L), pyramid(nxt, L)
    half = (win - 1) / 2.0
    r = types.SimpleNamespace(levels=L, win=win)
    r.lam, r.det = np.full((L, N), np.nan), np.full((L, N), np.nan)
    r.x0, r.template_ok, r.used = np.zeros((L, N, 2)), np.zeros((L, N), bool), np.zeros((L, N), bool)
    r.last_step, r.bound, r.gain, r.e = np.full(N, np.nan), np.full(N, np.inf), np.full(N, np.inf), np.zeros(N)
    r.chain, r.template_margin = np.zeros(N), np.zeros((L, N))
    r.steps = np.full((iters, N), np.nan)
    r.iter_margin = np.full(N, np.inf)
    r.lost, r.walked = np.zeros(N, bool), np.zeros(N, bool)
    q = None
    for l in range(L - 1, -1, -1):
        LI, LJ = Level(pI[l], win), Level(pJ[l], win)
        p = pts / 2.0 ** l
        q = p.copy() if l == L - 1 else 2.0 * q
        r.chain *= 2.0
        r.x0[l] = p - half
        r.template_ok[l] = LI.position_ok(r.x0[l])
        r.template_margin[l] = LI.position_margin(r.x0[l])
        t = _template(LI, p)
        r.lam[l] = np.where(r.template_ok[l], t.lam, np.nan)
        r.det[l] = np.where(r.template_ok[l], t.det, np.nan)
        r.used[l] = r.template_ok[l] & (t.lam >= min_eig) & (t.det >= FLT_EPSILON) & ~r.walked
        active = r.used[l].copy()
        for j in range(iters):
            idx = np.flatnonzero(active)
            if not len(idx):
                break
            x0 = q[idx] - half
            ok = LJ.position_ok(x0)
            if l == 0:
                r.iter_margin[idx] = np.minimum(r.iter_margin[idx], LJ.position_margin(x0))
                r.lost[idx[~ok]] = True
            r.walked[idx[~ok]] = True
            active[idx[~ok]] = False
            idx = idx[ok]
            s = _residual(LJ, _take(t, idx), q[idx])
            if iters == 1:
                r.chain[idx] = quantisation_bound(s) + step_gain(s) * r.chain[idx]
            q[idx] += s.delta
            step = np.hypot(s.delta[:, 0], s.delta[:, 1])
            if l == 0:
                r.last_step[idx] = step
                r.steps[j, idx] = step
            active[idx[step < 1e-13]] = False
        if l == 0:
            x0 = q - half
            fin = r.used[0] & ~r.lost
            r.iter_margin[fin] = np.minimum(r.iter_margin[fin], LJ.position_margin(x0[fin]))
            r.lost |= fin & ~LJ.position_ok(x0)
            idx = np.flatnonzero(r.used[0])
            if len(idx):
                s = _residual(LJ, _take(t, idx), q[idx])
                r.e[idx], r.bound[idx], r.gain[idx] = s.e, quantisation_bound(s), step_gain(s)
    r.q = q
    return r


def verdict(r, min_eig=1e-4, position_tol=0.0):
    """(status, decided) of a track() result.  status: the level-0 template window passes the position rule, lambda >=
    min_eig and det >= FLT_EPSILON there, and no iterate nor the final point failed the rule at level 0 -- a level above
    that was skipped does not lose the point.  A point is undecided when, at some level, lambda is within a factor 2 of
    min_eig (or det of FLT_EPSILON), or the template's position test is within POSITION_MARGIN of flipping; when an iterate's
    or the final point's position test is within POSITION_MARGIN + position_tol of flipping (position_tol: how far the
    kernel's iterates may be from the definition's, per point or one number); or when the definition walked out of the
    image."""
    status = r.used[0] & ~r.lost
    decided = ~r.walked
    for l in range(r.levels):
        m = r.template_ok[l]
        with np.errstate(invalid="ignore"):
            near = m & (((r.lam[l] > min_eig / 2) & (r.lam[l] < min_eig * 2)) |
                        ((r.det[l] > FLT_EPSILON / 2) & (r.det[l] < FLT_EPSILON * 2)))
        decided &= ~near & (r.template_margin[l] > POSITION_MARGIN)
    decided &= ~(r.used[0] & (r.iter_margin <= POSITION_MARGIN + position_tol))
    return status, decided


def err_at(prev, nxt, pts, out, win):
    """e = mean |J(out + .) - T(pts + .)| at level 0, for the points the caller gives (N, 2 each)."""
    s = lk_step_state(prev, nxt, np.asarray(pts, np.float64), np.asarray(out, np.float64), win)
    return s.e
