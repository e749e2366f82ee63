"""The case table of the forward-backward check's tests (include/vo_hip.h, "pyramidal KLT": vo_klt_track_fb).
tests/test_klt_fb_host.py calls every guard on the CPU oracle (tests/klt_fb_oracle.py); tests/test_gpu_klt_fb.py runs every
case, and every case of tests/klt_cases.py at fb_max = 1, through the kernels and compares bit for bit.

CASES: (name, prev, nxt, pts, win, max_level, max_iter, eps, min_eig, fb_max).  DOCS[name] names what a case exists for,
GUARDS[name]() asserts on the oracle that it is still there.  Images are at most 132 x 136, a case has at most ~600 points."""
import collections
import functools

import numpy as np

import klt_cases as kc
import klt_fb_oracle as fbo
from oracle import native

Case = collections.namedtuple("Case", "name prev nxt pts win max_level max_iter eps min_eig fb_max")
CASES, DOCS, GUARDS = [], {}, {}
ERR_THRESHOLD = 100.0         # KLTTracker._error_threshold, the existing filter's other half


def add(name, doc, images, pts, win, max_level=2, criteria=kc.TIGHT, min_eig=1e-4, fb_max=1.0, guard=None):
    assert name not in DOCS, name
    prev, nxt = images
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    pts.flags.writeable = False
    CASES.append(Case(name, prev, nxt, pts, win, max_level, criteria[0], criteria[1], min_eig, float(fb_max)))
    DOCS[name] = doc
    GUARDS[name] = guard if guard is not None else (lambda: None)


def case_args(c):
    return dict(win=c.win, max_level=c.max_level, max_iter=c.max_iter, eps=c.eps, min_eig=c.min_eig)


def from_klt_case(c, fb_max=1.0):
    """A case of tests/klt_cases.py with a threshold."""
    return Case(c.name, c.prev, c.nxt, c.pts, c.win, c.max_level, c.max_iter, c.eps, c.min_eig, float(fb_max))


# ---------------- the oracle's answers: computed once per case, shared, read-only ----------------
def _frozen(arrays):
    for a in arrays:
        a.flags.writeable = False
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def _expected(key):
    c = _LOOKUP[key]
    return _frozen(fbo.fb_track(c.prev, c.nxt, c.pts, fb_max=c.fb_max, **case_args(c)))


def expected(c):
    """(next_xy, status, err, fb) of the rule for the case, from the oracle.  (Case names are unique across this table and
    tests/klt_cases.py, so name and threshold identify the inputs.)"""
    key = (c.name, c.fb_max)
    _LOOKUP[key] = c
    return _expected(key)


@functools.lru_cache(maxsize=None)
def _passes(key):
    c = _LOOKUP[key]
    kw = case_args(c)
    nxy, sf, err = native.klt_track(c.prev, c.nxt, c.pts, **kw)
    sf = sf.astype(bool)
    back, sb = np.zeros_like(nxy), np.zeros(len(sf), bool)
    if sf.any():
        b, s, _ = native.klt_track(c.nxt, c.prev, np.ascontiguousarray(nxy[sf]), **kw)
        back[sf], sb[sf] = b, s.astype(bool)
    return _frozen([nxy, sf, err, back, sb])


def passes(c):
    """The two plain oracle calls of the case: (next_xy, status_f, err, back_xy, status_b), status as bool."""
    key = ("passes", c.name)
    _LOOKUP[key] = c
    return _passes(key)


_LOOKUP = {}


# ---------------- occluder: the experiment the check exists for ----------------
OCC_SHAPE, OCC_SHIFT, OCC_ROWS, OCC_COLS = (120, 132), (2.3, -1.6), (30, 80), (40, 100)


@functools.lru_cache(maxsize=None)
def occluder_images():
    """A dot_image pair moved by OCC_SHIFT; rows 30-80 and columns 40-100 of the new frame are another texture.  (Seeds:
    of nine pairs tried on the oracle, eight meet the guard's counts at every window and one leaves window 21 with 7
    caught points; this is one of the eight.)"""
    a, b = kc.dot_image(OCC_SHAPE[0], OCC_SHAPE[1], 7, OCC_SHIFT[0], OCC_SHIFT[1])
    other = kc.dot_image(OCC_SHAPE[0], OCC_SHAPE[1], 8, 0.0, 0.0)[0]
    b = b.copy()
    b[OCC_ROWS[0]:OCC_ROWS[1], OCC_COLS[0]:OCC_COLS[1]] = other[OCC_ROWS[0]:OCC_ROWS[1], OCC_COLS[0]:OCC_COLS[1]]
    b.flags.writeable = False
    return a, b


def occluder_regions(c):
    """(occluded, well outside): points whose place in the new frame lies inside the replaced block, and points whose
    window and search stay a window's width away from it."""
    x, y = c.pts[:, 0] + OCC_SHIFT[0], c.pts[:, 1] + OCC_SHIFT[1]
    inside = (x >= OCC_COLS[0]) & (x < OCC_COLS[1]) & (y >= OCC_ROWS[0]) & (y < OCC_ROWS[1])
    m = c.win
    near = (x >= OCC_COLS[0] - m) & (x < OCC_COLS[1] + m) & (y >= OCC_ROWS[0] - m) & (y < OCC_ROWS[1] + m)
    return inside, ~near


def _occluder_guard(name):
    def g():
        c = BY_NAME[name]
        nxy, st, err, fb = expected(c)
        _, sf, _, _, _ = passes(c)
        inside, outside = occluder_regions(c)
        old_filter = sf & (err < ERR_THRESHOLD)
        caught = inside & old_filter & (st == 0)
        assert caught.sum() >= 20, "only %d occluded points pass the old filter and are rejected at 1 px" % caught.sum()
        fwd_out = outside & sf
        kept = (st[fwd_out] == 1).mean()
        assert kept >= 0.85, "only %.1f %% of the forward-passing points outside keep status 1" % (100 * kept)
    return g


# ---------------- mixed waves ----------------
def _mixed_guard(name):
    def g():
        c = BY_NAME[name]
        per_wave = kc.SPECIALISED[c.win]
        sf = passes(c)[1]
        n = len(sf) // per_wave * per_wave
        waves = sf[:n].reshape(-1, per_wave)
        mixed = waves.any(axis=1) & ~waves.all(axis=1)
        assert mixed.sum() >= 1, "no wave holds a forward failure beside a success"
    return g


def _build():
    rng = np.random.default_rng(77)
    occ = occluder_images()
    occ_pts = np.stack([rng.uniform(0, OCC_SHAPE[1] - 1, 400), rng.uniform(0, OCC_SHAPE[0] - 1, 400)], axis=1)
    for win in (15, 17, 21, 9):
        name = "occluder_w%d" % win
        add(name, "win %d: a dot texture moved by (2.3, -1.6) with a block of the new frame replaced by another texture -- tracks "
            "that slid onto the occluder pass status & err < 100 and fail the round trip" % win, occ, occ_pts, win, 2, kc.TIGHT,
            guard=_occluder_guard(name))

    S = (96, 128)
    dots = kc.dot_image(96, 128, 5, 1.7, -1.1)

    # ---- tie: thr2 == fb[j] exactly keeps j; one float32 step lower rejects j and nothing else ----
    tie_pts = kc.interior(901, 200, S, 17)
    probe = Case("tie_probe", dots[0], dots[1], tie_pts, 17, 2, kc.TIGHT[0], kc.TIGHT[1], 1e-4, float("inf"))
    fb = fbo.fb_track(probe.prev, probe.nxt, probe.pts, fb_max=np.inf, **case_args(probe))[3]
    tie = {}
    for j in np.argsort(fb):
        lo = np.nextafter(fb[j], np.float32(0))
        f_at, f_lo = float(np.sqrt(np.float64(fb[j]))), float(np.sqrt(np.float64(lo)))
        if (np.isfinite(fb[j]) and fb[j] > 0 and lo > 0 and np.float32(f_at * f_at) == fb[j] and np.float32(f_lo * f_lo) == lo
                and (fb == fb[j]).sum() == 1 and (fb < fb[j]).sum() >= 20 and (fb > fb[j]).sum() >= 20):
            tie = dict(j=int(j), at=f_at, lo=f_lo)
            break
    TIE.update(tie)

    def tie_guard():
        assert TIE, "no point whose fb is the float32 square of a double"
        j = TIE["j"]
        at, lo = BY_NAME["tie"], BY_NAME["tie_below"]
        fb_at, fb_lo = expected(at)[3], expected(lo)[3]
        assert np.float32(at.fb_max * at.fb_max) == fb_at[j] and at.fb_max == float(np.sqrt(np.float64(fb_at[j])))
        assert np.float32(lo.fb_max * lo.fb_max) == np.nextafter(fb_at[j], np.float32(0))
        st_at, st_lo = expected(at)[1], expected(lo)[1]
        assert st_at[j] == 1 and st_lo[j] == 0
        assert np.array_equal(np.delete(st_at, j), np.delete(st_lo, j)) and np.array_equal(fb_at.view(np.uint32), fb_lo.view(np.uint32))
    add("tie", "fb_max = sqrt(double(fb[j])): thr2 equals fb[j] exactly and the tie is kept", dots, tie_pts, 17, 2, kc.TIGHT,
        fb_max=TIE.get("at", 1.0), guard=tie_guard)
    add("tie_below", "thr2 one float32 step below fb[j]: point j is rejected and no other point changes", dots, tie_pts, 17, 2,
        kc.TIGHT, fb_max=TIE.get("lo", 1.0), guard=tie_guard)

    # ---- back_out: the forward result lies within win / 2 of a border and the backward pass loses the point ----
    # the new frame is flat in a band along its left and top edges: a template taken there has no texture (the backward
    # pass's min-eigenvalue test fails) while the forward pass, whose template is the old frame's, still returns a point
    flat = dots[1].copy()
    flat[:, :14] = 90
    flat[:14, :] = 90
    flat.flags.writeable = False
    for win in (15, 9):
        name = "back_out_w%d" % win
        r2 = np.random.default_rng(910 + win)
        edge = np.concatenate([np.stack([r2.uniform(0, 9, 150), r2.uniform(0, S[0] - 1, 150)], axis=1),
                               np.stack([r2.uniform(0, S[1] - 1, 150), r2.uniform(0, 9, 150)], axis=1),
                               kc.interior(911, 100, S, win)])

        def g(name=name):
            c = BY_NAME[name]
            nxy, sf, err, back, sb = passes(c)
            H, W = c.prev.shape
            h = c.win / 2.0
            near = (nxy[:, 0] < h) | (nxy[:, 1] < h) | (nxy[:, 0] > W - 1 - h) | (nxy[:, 1] > H - 1 - h)
            lost = sf & ~sb & near
            assert lost.sum() >= 5, "only %d points end near a border and are lost on the way back" % lost.sum()
            assert np.all(np.isposinf(expected(c)[3][lost])) and np.all(expected(c)[1][lost] == 0)
        add(name, "win %d: the new frame is flat along two edges -- points tracked into the band come back with status_b = 0 and "
            "fb = +inf" % win, (dots[0], flat), r2.permutation(edge), win, 2, kc.DEFAULT, guard=g)

    # ---- fwd_fail_mixed: lane groups of one wave that mix forward failures with successes ----
    for win in (15, 17, 21):
        name = "fwd_fail_mixed_w%d" % win
        add(name, "win %d: %d keypoints per wave, out-of-image points of klt_cases.scatter among them -- a group whose forward pass "
            "failed sits out the second pass beside wave-mates that run it" % (win, kc.SPECIALISED[win]), dots,
            kc.scatter(920 + win, 403, S, win, outside=0.3), win, 2, kc.TIGHT, guard=_mixed_guard(name))

    # ---- remainders and levels: the inputs of klt_cases ----
    for win in (15, 17):
        for n in (1, 2, 3, 5, 7):
            src = kc.BY_NAME["win%d_n%d_dots" % (win, n)]
            name = "fb_win%d_n%d" % (win, n)

            def g(name=name, win=win, n=n):
                assert len(BY_NAME[name].pts) == n and n % kc.SPECIALISED[win] == kc.REMAINDER[win, n]
            add(name, "win %d, N = %d: the last wave is partly empty (%d of %d keypoints)" % (win, n, kc.REMAINDER[win, n],
                                                                                              kc.SPECIALISED[win]),
                (src.prev, src.nxt), src.pts, win, src.max_level, (src.max_iter, src.eps), guard=g)
    for src_name, want in (("levels4_win9_dots", 4), ("levels1_win15_smooth", 1)):
        src = kc.BY_NAME[src_name]
        name = "fb_" + src_name

        def g(name=name, want=want):
            c = BY_NAME[name]
            assert native.klt_num_levels(c.prev.shape[0], c.prev.shape[1], c.win, c.max_level) == want
        add(name, "%d level(s): both passes run the same level loop" % want, (src.prev, src.nxt), src.pts, src.win, src.max_level,
            (src.max_iter, src.eps), guard=g)

    # ---- inf ----
    def inf_guard():
        c = BY_NAME["inf"]
        nxy, sf, err, back, sb = passes(c)
        st, fb = expected(c)[1], expected(c)[3]
        assert np.array_equal(st.astype(bool), sf & sb) and (sf & sb).sum() >= 100 and (sf & ~sb).sum() >= 1 and (~sf).sum() >= 1
        assert np.all(np.isfinite(fb[sf & sb])) and (fb[sf & sb] > 1.0).sum() >= 10       # (points 1 px would reject are kept)
    add("inf", "fb_max = +inf: the status is status_f & status_b, whatever the distance -- and a point either pass lost stays lost "
        "although its fb = +inf is not above the threshold", occ, kc.scatter(930, 400, OCC_SHAPE, 15), 15, 2, kc.TIGHT,
        fb_max=float("inf"), guard=inf_guard)


TIE = {}
BY_NAME = {}
_build()
BY_NAME.update({c.name: c for c in CASES})
NAMES = [c.name for c in CASES]
