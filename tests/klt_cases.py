"""The case table of the Lucas-Kanade tracker's tests.  tests/test_klt_reference_host.py runs every case through the oracle
(oracle/csrc/klt.c) and tests/test_gpu_klt_reference.py through the kernels of csrc/klt.hip and csrc/pyramid.hip; both compare the result with the
float64 definition of tests/klt_reference.py by the checks at the end of this file, and the GPU file also with the oracle bit
for bit.

CASES: (name, prev, nxt, pts, win, max_level, max_iter, eps, min_eig).  DOCS[name] names the edge a case exists for and
GUARDS[name]() asserts that the edge is still there (the host file calls every guard).  Images are at most 132 x 136 and a
case has about 600 points, among them points up to win / 2 outside every edge.

Textures.  shift_image is the suite's smooth texture: its gradient is a few grey levels per pixel, which leaves one step of
the kernel's fixed point a quantisation bound of 0.3 px and more.  dot_image (blurred random dots, gradients of tens of grey
levels per pixel) brings the bound to about 0.02 px: the cases whose name ends in _dots are the ones in which a few percent
of bias cannot hide (a Sobel in place of the Scharr derivative fails 47 checks, all of them on these cases).  wave_image
has texture in every 3 x 3 window (windows of 3 to 5), two_contrast_image two separate modes of the min-eigenvalue
(min_eig 1e-2).  Every case's inputs were chosen so that the definition alone decides at least 90 %
of its points (CAP); a case that could not meet that got other inputs, not a looser cap."""
import collections
import functools

import numpy as np

import klt_reference as ref
from test_oracle_geometry import shift_image

#: shapes at which pyrDown must equal the definition: sides of 1 and 2, both sides of the 32-pixel border, odd sizes
PYR_SHAPES = [(1, 1), (1, 7), (2, 2), (3, 5), (2, 9), (32, 32), (33, 34), (31, 40), (37, 51)]

Case = collections.namedtuple("Case", "name prev nxt pts win max_level max_iter eps min_eig")
CASES, DOCS, GUARDS = [], {}, {}
DEFAULT = (10, 0.03)          # the reference call site's criteria
TIGHT = (30, 1e-3)
# keypoints the last wave of a launch holds (0: it is full), per (window, N): both kernels get 1, and win 15 also 2 and 3
REMAINDER = {(15, 1): 1, (15, 2): 2, (15, 3): 3, (15, 5): 1, (15, 7): 3, (15, 601): 1,
             (17, 1): 1, (17, 2): 0, (17, 3): 1, (17, 5): 1, (17, 7): 1, (17, 601): 1}
SPECIALISED = {15: 4, 17: 2, 21: 2}       # window -> keypoints per wave of klt_track16_kernel; every other window: generic
MAX_WIN, PYR_PAD = 31, 32
CAP = 0.10                    # share of a case's points that may stay undecided or unconverged


@functools.lru_cache(maxsize=None)
def dot_image(h, w, seed, dx, dy, sigma=1.0, density=0.06):
    """Gaussian dots (sigma px) at random places, `density` per pixel, and the same dots moved by (dx, dy): rendered
    analytically, so the flow is exact up to the rounding to bytes."""
    rng = np.random.default_rng(seed)
    n = int(h * w * density)
    cy, cx, amp = rng.uniform(-5, h + 5, n), rng.uniform(-5, w + 5, n), rng.uniform(0.4, 1.0, n)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def render(ox, oy):
        img = np.zeros((h, w))
        for k in range(n):
            y0, y1 = int(max(0, cy[k] + oy - 4 * sigma)), int(min(h, cy[k] + oy + 4 * sigma + 1))
            x0, x1 = int(max(0, cx[k] + ox - 4 * sigma)), int(min(w, cx[k] + ox + 4 * sigma + 1))
            if y0 < y1 and x0 < x1:
                img[y0:y1, x0:x1] += amp[k] * np.exp(-((yy[y0:y1, x0:x1] - cy[k] - oy) ** 2 +
                                                       (xx[y0:y1, x0:x1] - cx[k] - ox) ** 2) / (2 * sigma ** 2))
        return np.clip(np.rint(img / 1.6 * 255), 0, 255).astype(np.uint8)
    a, b = render(0.0, 0.0), render(dx, dy)
    a.flags.writeable = b.flags.writeable = False
    return a, b


@functools.lru_cache(maxsize=None)
def wave_image(h, w, seed, dx, dy, fmin=0.3, fmax=0.9, n=12):
    """n plane waves of random direction, fmin .. fmax rad/px, and the same waves moved by (dx, dy): texture in every 3 x 3
    window (the dots leave flat gaps that windows of 3 to 5 pixels fall into)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b = np.zeros((h, w)), np.zeros((h, w))
    for _ in range(n):
        f, th, ph = rng.uniform(fmin, fmax), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        fx, fy = f * np.cos(th), f * np.sin(th)
        a += np.sin(fx * xx + fy * yy + ph)
        b += np.sin(fx * (xx - dx) + fy * (yy - dy) + ph)
    scale = 127.5 / (3.2 * np.sqrt(n / 2))
    a, b = (np.clip(np.rint(127.5 + scale * v), 0, 255).astype(np.uint8) for v in (a, b))
    a.flags.writeable = b.flags.writeable = False
    return a, b


@functools.lru_cache(maxsize=None)
def two_contrast_image(h, w, seed, dx, dy, split, low):
    """Dense dots whose columns from `split` on are dimmed to the share `low`: the min-eigenvalue has two separate modes."""
    a, b = dot_image(h, w, seed, dx, dy, 1.2, 0.12)
    gain = np.where(np.arange(w)[None, :] < split, 1.0, low)
    a, b = (np.rint(v * gain).astype(np.uint8) for v in (a, b))
    a.flags.writeable = b.flags.writeable = False
    return a, b


@functools.lru_cache(maxsize=None)
def smooth_image(h, w, seed, dx, dy):
    a, b = shift_image(h, w, seed, dx, dy)
    a.flags.writeable = b.flags.writeable = False
    return a, b


def scatter(seed, n, shape, win, outside=0.12):
    """n points: the share `outside` of them in the band of win / 2 around the image, uniform over the band, the others
    uniform over the image (its edge pixels included: most of their windows' pixels are reflected ones)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    pts = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], axis=1)
    for i in range(int(round(outside * n))):
        while 0 <= pts[i, 0] <= W - 1 and 0 <= pts[i, 1] <= H - 1:
            pts[i] = rng.uniform(-win / 2, W - 1 + win / 2), rng.uniform(-win / 2, H - 1 + win / 2)
    return rng.permutation(pts).astype(np.float32)


def interior(seed, n, shape, win):
    rng = np.random.default_rng(seed)
    H, W = shape
    return np.stack([rng.uniform(win, W - 1 - win, n), rng.uniform(win, H - 1 - win, n)], axis=1).astype(np.float32)


def level_shape(shape, l):
    H, W = shape
    for _ in range(l):
        H, W = (H + 1) // 2, (W + 1) // 2
    return H, W


def crossing_rows(shape, win, level, steps=None, places=(-1, 1), across=6):
    """Points whose template window, at pyramid level `level`, steps by 0.25 px across the places where the position rule
    flips: first sample x0 = p / 2^level - (win - 1) / 2 from c - 2 to c + 2 for c = -win and c = W (so floor(x0) takes
    -win - 2 .. -win + 1 and W - 2 .. W + 1), the other coordinate at six places inside the image; and the same along y."""
    H, W = level_shape(shape, level)
    half = (win - 1) / 2.0
    steps = np.arange(-2.0, 2.0 + 1e-9, 0.25) if steps is None else steps
    pts = []
    for axis, (n_along, n_across) in enumerate(((W, H), (H, W))):
        for c in [(-win, n_along)[k > 0] for k in places]:
            for t in np.linspace(0.2 * n_across, 0.8 * n_across, across) + 0.37:
                for s in steps:
                    p = [c + s + half, t]
                    pts.append(p if axis == 0 else p[::-1])
    return (np.array(pts) * 2.0 ** level).astype(np.float32)


def add(name, doc, images, pts, win, max_level=2, criteria=DEFAULT, min_eig=1e-4, guard=None):
    assert name not in DOCS, name
    prev, nxt = images
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    pts.flags.writeable = False
    CASES.append(Case(name, prev, nxt, pts, win, max_level, criteria[0], criteria[1], min_eig))
    DOCS[name] = doc
    GUARDS[name] = guard if guard is not None else (lambda: None)


def levels_of(c):
    return ref.num_levels(c.prev.shape[0], c.prev.shape[1], c.win, c.max_level)


def _outside_guard(name):
    """Every scatter case: points beyond each of the four edges, and points inside."""
    def g():
        c = BY_NAME[name]
        H, W = c.prev.shape
        x, y = c.pts[:, 0], c.pts[:, 1]
        assert (x < 0).any() and (x > W - 1).any() and (y < 0).any() and (y > H - 1).any() and ((x > 0) & (x < W - 1)).any()
    return g


def iter0_guard(name):
    """max_iter 0: the definition leaves every point where it was, and keeps some points and loses others."""
    c = BY_NAME[name]
    r, st, decided = compared(name)[:3]
    assert c.max_iter == 0 and np.array_equal(r.q, c.pts.astype(np.float64))
    assert (st & decided).sum() >= 400 and (~st & decided).sum() >= 5


def stop_guard(name):
    """Which stop ends the iteration, from the definition's own steps at level 0.  eps > 0: for nine points in ten the step
    falls below eps / 2 at least two steps before the count runs out (the eps stop, not the count).  eps = 0: the eps stop
    cannot fire on a non-zero step, and nine points in ten have a step below the ping-pong stop's 0.01 px within the count."""
    c = BY_NAME[name]
    r = reference(name)
    used = r.used[0] & ~r.walked
    with np.errstate(invalid="ignore"):
        small = r.steps[:c.max_iter - 2] < (c.eps / 2 if c.eps > 0 else 0.01)
    assert (c.eps == 0) == name.startswith("eps0_") and used.sum() >= 500
    assert small.any(axis=0)[used].mean() >= 0.9


def _both(*guards):
    def g():
        for f in guards:
            f()
    return g


def _build():
    S = (96, 128)
    smooth = smooth_image(96, 128, 8, 1.3, -0.7)
    dots = dot_image(96, 128, 5, 1.7, -1.1)
    dots_slow = dot_image(96, 128, 6, 0.3, -0.2, 1.5)       # small windows: wider dots, a small motion

    # ---- window and dispatch ----
    for win in (15, 17, 21, 9, 16, 20, 31):
        kind = "the specialised kernel klt_track16_kernel<%d>" % win if win in SPECIALISED else "the generic kernel"
        extra = {16: ", an even window", 20: ", an even window", 31: ", the largest window (MAX_WIN)"}.get(win, "")
        for tex, images, crit in (("smooth", smooth, DEFAULT), ("dots", dots, TIGHT)):
            if (win, tex) == (9, "smooth"):
                continue          # (10.2 % of its points stay unconverged or undecided: over the cap; win 9 keeps the dots)
            name = "win%d_%s" % (win, tex)

            def g(win=win, name=name):
                # (which kernel a window gets and MAX_WIN are read from csrc/klt.hip, PYR_PAD from csrc/pyramid_device.h, by
                #  the host file's test_constants_are_the_kernels)
                assert 3 <= win <= MAX_WIN
                # 96 x 128 with three levels: level 2 is 24 x 32, a side <= PYR_PAD, so the bordered builder takes the
                # per-level kernels and their border reflects more than once
                if levels_of(BY_NAME[name]) == 3:
                    assert min(level_shape(S, 2)) <= PYR_PAD
            add(name, "win %d: %s%s; %s texture, 96 x 128, level 2 is 24 x 32 (tiled builder not taken)" % (win, kind, extra, tex),
                images, scatter(100 + win, 600, S, win), win, 2, crit, guard=_both(g, _outside_guard(name)))
    waves = wave_image(96, 128, 6, 0.3, -0.2)
    for win, max_level in ((3, 0), (4, 0), (5, 2)):
        name = "win%d_waves" % win

        def g(win=win):
            assert win not in SPECIALISED and win >= 3                         # 3 is the smallest window the entry accepts
        add(name, "win %d: the generic kernel at its smallest windows (3 is the minimum, 4 even); plane waves moved by "
            "(0.3, -0.2), max_level %d (a 3 x 3 window finds no fixed point on the coarse levels of any texture tried)" % (win, max_level),
            waves, scatter(100 + win, 600, S, win), win, max_level, TIGHT, guard=_both(g, _outside_guard(name)))

    # ---- N: launch remainders ----
    for win in (15, 17):
        per_wave = SPECIALISED[win]
        for n in (1, 2, 3, 5, 7, 601):
            name = "win%d_n%d_dots" % (win, n)

            def g(n=n, win=win, per_wave=per_wave, name=name):
                assert len(BY_NAME[name].pts) == n and n % per_wave == REMAINDER[win, n]
            pts = interior(200 + n, n, S, win) if n < 600 else scatter(200 + n, n, S, win)
            add(name, "win %d, N = %d: %d keypoints per wave, the last wave is %s" %
                (win, n, per_wave, "partly empty" if n % per_wave else "full"), dots, pts, win, 2, TIGHT, guard=g)

    # ---- levels ----
    def levels_guard(name, want, extra=None):
        def g():
            c = BY_NAME[name]
            assert levels_of(c) == want
            assert extra is None or extra(c)
        return g
    add("levels1_win15_smooth", "max_level 0: one level, the top level is level 0", smooth, scatter(301, 600, S, 15), 15, 0, DEFAULT,
        guard=levels_guard("levels1_win15_smooth", 1))
    add("levels4_win9_dots", "max_level 3, win 9: four levels, the top one 12 x 16", dots, scatter(302, 600, S, 9), 9, 3, TIGHT,
        guard=levels_guard("levels4_win9_dots", 4, lambda c: level_shape(S, 3) == (12, 16)))
    add("levels_stop_win9_dots", "max_level 7 on 96 x 128, win 9: the builder's stop decides (level 4 would be 6 x 8 <= win)", dots,
        scatter(303, 600, S, 9), 9, 7, TIGHT,
        guard=levels_guard("levels_stop_win9_dots", 4, lambda c: c.max_level + 1 > 4 and min(level_shape(S, 4)) <= c.win))
    big = dot_image(132, 136, 7, 1.7, -1.1)
    for win in (17, 9):
        name = "tiled_132x136_win%d_dots" % win

        def g(name=name):
            c = BY_NAME[name]
            h2, w2 = level_shape(c.prev.shape, 2)
            assert levels_of(c) == 3 and (h2, w2) == (33, 34) and h2 > PYR_PAD and w2 > PYR_PAD and c.prev.shape[1] % 4 == 0
        add(name, "132 x 136 with three levels: level 2 is 33 x 34, both sides > 32, the one-launch tiled builder is taken",
            big, scatter(310 + win, 600, (132, 136), win), win, 2, TIGHT, guard=_both(g, _outside_guard(name)))
    odd = dot_image(97, 131, 8, 1.7, -1.1)
    for win in (15, 17):
        name = "odd_97x131_win%d_dots" % win

        def g(name=name):
            c = BY_NAME[name]
            assert c.prev.shape[1] % 4 != 0 and c.prev.shape[0] % 2 == 1 and levels_of(c) == 3
        add(name, "97 x 131: a width that is no multiple of 4 (pitch padding, byte builder), odd sides at every level", odd,
            scatter(320 + win, 600, (97, 131), win), win, 2, TIGHT, guard=_both(g, _outside_guard(name)))
    tiny = dot_image(20, 24, 9, 0.4, 0.3)
    for win in (21, 31):
        name = "tiny_20x24_win%d_dots" % win

        def g(name=name):
            c = BY_NAME[name]
            assert max(c.prev.shape) < c.win + 4 and levels_of(c) == 1
        add(name, "20 x 24 with win %d: the image is smaller than the window, every window reads reflected pixels" % win, tiny,
            scatter(330 + win, 600, (20, 24), win), win, 2, TIGHT, guard=_both(g, _outside_guard(name)))

    # ---- criteria ----
    add("iter0_win17_dots", "max_iter 0: no step; every point comes back where it was, with that place's status and err", dots,
        scatter(401, 600, S, 17), 17, 2, (0, 0.03), guard=lambda: iter0_guard("iter0_win17_dots"))
    add("iter0_win9_dots", "max_iter 0 on the generic kernel", dots, scatter(402, 600, S, 9), 9, 2, (0, 0.03),
        guard=lambda: iter0_guard("iter0_win9_dots"))
    for name, win, max_level, images, want in (("iter1_levels1_win17_dots", 17, 0, dots, 1), ("iter1_levels3_win15_dots", 15, 2, dots, 3),
                                               ("iter1_levels3_win17_dots", 17, 2, dots, 3), ("iter1_levels4_win9_dots", 9, 3, dots, 4),
                                               ("iter1_levels5_win5_dots", 5, 7, dots_slow, 5), ("iter1_levels3_win3_waves", 3, 2, waves, 3),
                                               ("iter1_levels3_win4_waves", 4, 2, waves, 3)):
        add(name, "max_iter 1, eps 0 through %d level(s): exactly one Newton step per level" % want, images,
            scatter(410 + win + want, 600, S, win), win, max_level, (1, 0.0), guard=levels_guard(name, want))
    add("eps0_win15_dots", "eps 0 with max_iter 30: only the ping-pong stop, a zero step or the count end the iteration", dots,
        scatter(420, 600, S, 15), 15, 2, (30, 0.0), guard=lambda: stop_guard("eps0_win15_dots"))
    add("eps0_win16_dots", "eps 0 with max_iter 30 on the generic kernel", dots, scatter(421, 600, S, 16), 16, 2, (30, 0.0),
        guard=lambda: stop_guard("eps0_win16_dots"))
    add("eps003_iter30_win21_dots", "eps 0.03 with max_iter 30: the eps stop, never the count", dots, scatter(422, 600, S, 21), 21, 2, (30, 0.03),
        guard=lambda: stop_guard("eps003_iter30_win21_dots"))
    add("default_win17_dots", "the call site's own criteria (10, 0.03), win 17, on the sharp texture: the eps stop within the count", dots,
        scatter(423, 600, S, 17), 17, 2, DEFAULT, guard=lambda: stop_guard("default_win17_dots"))
    dim = two_contrast_image(96, 128, 11, 0.3, -0.2, 96, 0.08)
    for name, win, images in (("mineig1e-2_win9_dim", 9, dim), ("mineig1e-2_win17_dim", 17, dim), ("mineig1e-2_win5_dim", 5, dim)):
        def g(name=name):
            c = BY_NAME[name]
            lam = reference(name).lam[0]
            with np.errstate(invalid="ignore"):
                assert ((lam > 2e-4) & (lam < 5e-3)).sum() >= 60, "too few points between the default threshold and this one"
                assert (lam > 2e-2).sum() >= 300
        add(name, "min_eig 1e-2 on one level: the dimmed quarter's lambda lies between the default 1e-4 and this threshold (lost), the "
            "rest's well above it", images, scatter(430 + win, 600, S, win), win, 0, TIGHT, min_eig=1e-2, guard=g)

    # ---- points ----
    for name, win, offs in (("integer_win15_dots", 15, 0.0), ("integer_win9_dots", 9, 0.0), ("halfinteger_win17_dots", 17, 0.5),
                            ("halfinteger_win16_dots", 16, 0.5)):
        def g(name=name, offs=offs):
            c = BY_NAME[name]
            x0 = c.pts.astype(np.float64) - (c.win - 1) / 2.0
            frac = x0 - np.floor(x0)
            assert np.all((frac == 0.0) | (frac == 0.5)) and (frac == 0.0).all() == ((c.win % 2 == 1) == (offs == 0.0))
        add(name, "%s coordinates: the template's bilinear weights are exactly %s" %
            ("whole-number" if offs == 0.0 else "half-integer", "1, 0, 0, 0" if (win % 2 == 1) == (offs == 0.0) else "a half or a quarter"),
            dots, np.floor(scatter(440 + win, 600, S, win)) + offs, win, 2, TIGHT, guard=g)
    for win in (15, 17, 9):
        for level in (0, 2):
            name = "rows_level%d_win%d_dots" % (level, win)

            def g(name=name, level=level):
                c = BY_NAME[name]
                assert levels_of(c) == 3
                H, W = level_shape(c.prev.shape, level)
                x0 = c.pts.astype(np.float64) / 2.0 ** level - (c.win - 1) / 2.0
                for axis, n in ((0, W), (1, H)):
                    f = np.floor(x0[:, axis])
                    for v in (-c.win - 1, -c.win, n - 1, n):
                        assert (f == v).any(), "no window with floor(x0) = %d" % v
                    assert (x0[:, axis] == -c.win).any() and (x0[:, axis] == n).any()
            # (what the rows can show of the low end is bit equality between kernel and oracle: a template window with
            #  floor(x0) = -win has one column inside the image, column 0, whose reflect-101 x-derivative is zero, so
            #  lambda is zero and the point is lost whether the rule reads < -win or <= -win)
            add(name, "rows stepped by 0.25 px across the four places where floor(p - half) crosses -win - 1 | -win and "
                "W - 1 | W (and H) at level %d: %s" % (level, "the top level; one step per level, so a skipped top level shows in the "
                                                        "returned point" if level else "both frames the same, so no step moves a point and "
                                                        "status is the position rule and lambda alone"),
                (dots[0], dots[0]) if level == 0 else dots, crossing_rows(S, win, level), win, 2, TIGHT if level == 0 else (1, 0.0), guard=g)

    # ---- search windows that end on the last place the position rule allows ----
    # A window there is 0.2 .. 0.8 px from leaving, and a Newton step that overshoots leaves: of points aimed at that place
    # about one in ten is tracked to it by the definition without an iterate outside.  So candidates are tried on the
    # definition alone (never on the oracle or a kernel), 2000 per edge, and the ones it decides are kept (at most 25), with
    # four it does not.
    for side, move in (("low", -2.5), ("high", 2.5)):
        images = dot_image(96, 128, 5, move, move)
        for win in (15, 9):
            name = "search_edge_%s_win%d_dots" % (side, win)
            rng = np.random.default_rng(500 + win + (side == "high"))
            pts = [interior(510 + win, 520, S, win)]
            for axis, n in ((0, S[1]), (1, S[0])):
                edge = -win if side == "low" else n - 1
                cand = np.empty((2000, 2))
                cand[:, axis] = rng.uniform(0.2, 0.8, 2000) + edge - move + (win - 1) / 2.0     # the final window starts at edge + 0.2 .. 0.8
                cand[:, 1 - axis] = rng.uniform(win, S[axis] - 1 - win, 2000)
                cand = cand.astype(np.float32)
                r = ref.track(images[0], images[1], cand, win, 0, 40)
                tol = TIGHT[1] + 2 * r.bound
                st, decided = ref.verdict(r, 1e-4, np.where(np.isfinite(tol), tol, 1e9))
                good = st & decided & (r.last_step < 1e-6) & (np.floor(r.q[:, axis] - (win - 1) / 2.0) == edge)
                pts += [cand[good][:25], cand[~good][:4]]

            def g(name=name, side=side):
                c = BY_NAME[name]
                r, st, decided = compared(name)[:3]
                x0 = r.q - (c.win - 1) / 2.0
                found = 0
                for axis, n in ((0, c.prev.shape[1]), (1, c.prev.shape[0])):
                    at_edge = np.floor(x0[:, axis]) == (-c.win if side == "low" else n - 1)
                    started_inside = np.floor(r.x0[0, :, axis]) != np.floor(x0[:, axis])
                    found += (st & decided & at_edge & started_inside).sum()
                # (along y and at the high edge the definition decides few of them: 25 + 8, 19 + 3, 1 + 0 and 13 + 2 points)
                assert found >= 1, "no tracked, decided point ends at the edge"
            add(name, "one level, dots moving by (%g, %g): points whose search window walks 2.5 px to the %s place the position "
                "rule allows an iterate and the final point, floor(q - half) = %s, along x and along y -- a rule off by one "
                "there loses them" % (move, move, "first" if side == "low" else "last", "-win" if side == "low" else "W - 1 (H - 1)"),
                images, np.concatenate(pts), win, 0, TIGHT, guard=g)

_build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


# ---------------- the definition's answers: computed once per case, shared, read-only ----------------
def mode_of(c):
    return "zero" if c.max_iter == 0 else "chain" if c.max_iter == 1 else "fixed"


@functools.lru_cache(maxsize=None)
def reference(name):
    """klt_reference.track for the case: no step (max_iter 0), one step per level (max_iter 1), else the fixed point (40
    full steps per level)."""
    c = BY_NAME[name]
    iters = {"zero": 0, "chain": 1, "fixed": 40}[mode_of(c)]
    return ref.track(c.prev, c.nxt, c.pts, c.win, c.max_level, iters, c.min_eig)


@functools.lru_cache(maxsize=None)
def one_step_reference(name):
    """The case's images, points and window with max_level = 0, max_iter = 1, eps = 0."""
    c = BY_NAME[name]
    return ref.track(c.prev, c.nxt, c.pts, c.win, 0, 1, c.min_eig)


def one_step_args(c):
    return dict(win=c.win, max_level=0, max_iter=1, eps=0.0, min_eig=c.min_eig)


def case_args(c):
    return dict(win=c.win, max_level=c.max_level, max_iter=c.max_iter, eps=c.eps, min_eig=c.min_eig)


def compared(name, one_step=False):
    """From the definition alone: (track result, status, decided, converged, tol) of the case.  `decided` leaves out, besides
    what klt_reference.verdict leaves out, the points that the definition tracks on level 0 without settling (its last step
    is not below 1e-6): an iteration that does not settle says nothing about where, or whether, the tracker's ends.
    tol is the distance allowed between the
    tracker's point and the definition's:
      one step / chain   twice track().chain: the quantisation bound, carried from level to level, doubled for the second
                         order -- with one level, 2 * quantisation_bound
      fixed point        eps + 2 * bound at the definition's point: the tracker stopped after a step <= eps, or at the
                         ping-pong midpoint, which lies closer; applied where the definition's own last step is < 1e-6.
                         With eps = 0 that is 2 * bound: only the ping-pong stop, a zero step or the count end the tracker
    and also what the tracker's iterates may differ by when their position tests are judged."""
    c = BY_NAME[name]
    r = one_step_reference(name) if one_step else reference(name)
    mode = "chain" if one_step else mode_of(c)
    if mode == "zero":
        tol = np.zeros(len(c.pts))
    elif mode == "chain":
        tol = 2 * r.chain
    else:
        tol = c.eps + 2 * r.bound
    status, decided = ref.verdict(r, c.min_eig, np.where(np.isfinite(tol), tol, 1e9))
    with np.errstate(invalid="ignore"):
        converged = r.last_step < 1e-6 if mode == "fixed" else np.ones(len(c.pts), bool)
    decided = decided & (converged | ~r.used[0])
    return r, status, decided, converged, tol


def cap_share(name, one_step=False):
    """Share of the case's points that no check against the definition reaches: undecided, or tracked but unconverged."""
    r, status, decided, converged, tol = compared(name, one_step)
    return 1.0 - float(np.mean(decided))


ERR_TOL = 2 * ref.EPS_SAMPLE


def check(name, out, status, err, one_step=False, figures=None):
    """The checks against the definition for a tracker's (out, status, err) of the case (or of its one-step form): every one
    is made, then the failures are raised together.  figures: a dict that receives the measured distances (for reports);
    nothing in it is a tolerance."""
    c = BY_NAME[name]
    r, st_ref, decided, converged, tol = compared(name, one_step)
    mode = "chain" if one_step else mode_of(c)
    status, out, err = np.asarray(status).astype(bool), np.asarray(out), np.asarray(err)
    failures = []
    # status: equal for every decided point
    bad = decided & (status != st_ref)
    if bad.any():
        failures.append("status differs from the definition's at decided points %s" % np.flatnonzero(bad)[:10])
    if mode == "zero" and not np.array_equal(out, c.pts):
        failures.append("max_iter 0 moved a point")
    # the point: where the definition decides and, for the fixed point, both track it.  With a fixed number of steps the
    # point is compared even where it is lost: the tracker returns how far it came.
    m = decided & ((status & st_ref) if mode == "fixed" else np.isfinite(tol))
    if m.any():
        dist = np.hypot(*(out.astype(np.float64)[m] - r.q[m]).T)
        over = dist > tol[m]
        if figures is not None:
            base = r.chain[m] if mode == "chain" else r.bound[m]
            frac = dist[base > 0] / base[base > 0]
            figures.update(n=int(m.sum()), max_px=float(dist.max()), p99_px=float(np.percentile(dist, 99)), median_bound=float(np.median(base)))
            if frac.size:
                figures.update(max_frac=float(frac.max()), p99_frac=float(np.percentile(frac, 99)))
        if over.any():
            k = np.flatnonzero(m)[over][np.argmax(dist[over] / tol[m][over])]
            failures.append("%d point(s) farther from the definition than allowed, worst: point %d at %.4g px against %.4g (bound %.4g, "
                            "step gain %.3g)" % (over.sum(), k, np.hypot(*(out[k] - r.q[k])), tol[k], r.bound[k], r.gain[k]))
    # err: the definition's e at the point the tracker returned
    k = np.flatnonzero(status & st_ref & decided)
    if len(k):
        de = np.abs(err.astype(np.float64)[k] - ref.err_at(c.prev, c.nxt, c.pts[k], out[k], c.win))
        if figures is not None:
            figures["max_err"] = float(de.max())
        if de.max() > ERR_TOL:
            failures.append("err is %.4g grey levels from the definition's (allowed %.4g)" % (de.max(), ERR_TOL))
    assert not failures, "%s%s: %s" % (name, " (one step)" if one_step else "", "; ".join(failures))
