"""-m gpu: the P3P hypothesis kernels against the case table with reference solution sets
(tests/golden/p3p_cases.npz), bit for bit against the C oracle, and at the edges of their launch shapes.

The table's cases of one intrinsics go into one call of vo_p3p_hypotheses: X holds the 4 points of every case,
sample i is (4i, 4i+1, 4i+2, 4i+3).  The kernel's output is held to the oracle's bits (the header of p3p.hip
promises them) and, on its own, to the three criteria of test_p3p_reference_host.py -- so a change that moves
oracle and kernel together in a wrong direction still fails here."""
import numpy as np
import pytest

import p3p_cases as pc
from oracle import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tab():
    return pc.table()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def first_difference(names, got, ref, label):
    """None, or a description of the first hypothesis whose outputs differ and the first output that does, in the
    order the kernels produce them: valid flag, R, t (solve kernel), count, mask (score kernel)"""
    for h in range(len(got[0])):
        for nm, g, r in zip(names, got, ref):
            same = np.array_equal(bits(g[h]), bits(r[h])) if g.dtype == np.float64 else np.array_equal(g[h], r[h])
            if not same:
                return "%s: %s differs (kernel %s, oracle %s)" % (label(h), nm, np.asarray(g[h]).ravel()[:9], np.asarray(r[h]).ravel()[:9])
    return None


@pytest.fixture(scope="module")
def solved(ctx, tab):
    """kernel and oracle on the whole table, one call per intrinsics; outputs in table order"""
    n = len(tab["n_sol"])
    out = {"rows": []}
    for who in ("gpu", "cpu"):
        out[who] = dict(valid=np.zeros(n, np.uint8), R=np.zeros((n, 3, 3)), t=np.zeros((n, 3)), counts=np.zeros(n, np.int32),
                        masks=[None] * n)
    for Kid in range(3):
        rows, K, X, x, samples = pc.pack(tab, Kid)
        assert len(rows) <= 1100 and len(X) == 4 * len(rows)
        for who, fn in (("gpu", ctx.p3p_hypotheses), ("cpu", native.p3p_hypotheses)):
            R, t, v, c, m = fn(X, x, K, samples, 1.0, want_masks=True)
            o = out[who]
            o["valid"][rows], o["R"][rows], o["t"][rows], o["counts"][rows] = v, R, t, c
            for j, i in enumerate(rows):
                o["masks"][i] = np.asarray(m[j]).astype(bool)
    out["measure"] = pc.measure(tab, out["gpu"]["valid"], out["gpu"]["R"], out["gpu"]["t"])
    return out


def test_table_bit_identical_to_oracle(tab, solved):
    g, c = solved["gpu"], solved["cpu"]
    keys = ("valid", "R", "t", "counts")
    d = first_difference(keys, [g[k] for k in keys], [c[k] for k in keys], lambda h: pc.name(tab, h))
    assert d is None, d
    for i in range(len(g["masks"])):
        assert np.array_equal(g["masks"][i], c["masks"][i]), "mask row of " + pc.name(tab, i)


def test_kernel_validity(tab, solved):
    pc.check_validity(tab, solved["gpu"]["valid"])


def test_kernel_backward_error(tab, solved):
    """As test_oracle_backward_error, on the kernel's own poses: rotations to 1e-12, the three solved points within
    1e-3 px, the symmetric family within 1e-4 px."""
    worst = pc.check_backward(tab, solved["measure"])
    assert worst["symmetric"] <= 1e-4


def test_kernel_selection(tab, solved):
    pc.check_selection(tab, solved["measure"])


def test_kernel_picks_the_right_root_at_a_vanishing_denominator(tab, solved):
    pc.check_demanded(tab, solved["measure"])


# ---------------- launch-shape edges ----------------
def generic_subset(tab, cases=64):
    rows = np.flatnonzero((tab["family"] == "generic") & (tab["K_index"] == 0))[:cases]
    return tab["K_table"][0].copy(), tab["X"][rows].reshape(-1, 3).copy(), tab["x"][rows].reshape(-1, 2).copy()


@pytest.mark.parametrize("hyp", [1, 3, 15, 16, 17, 1003])
def test_hypothesis_count_edges(ctx, tab, hyp):
    """16 hypotheses (quads of lanes) fill a 64-lane block of the solve kernel: a partial block, a full one, one
    hypothesis more, many blocks with a partial last one."""
    K, X, x = generic_subset(tab)
    case = np.arange(hyp) * 7 % 64
    samples = (4 * case[:, None] + np.arange(4)[None, :]).astype(np.int32)
    keys = ("valid", "R", "t", "counts", "masks")
    Rg, tg, vg, cg, mg = ctx.p3p_hypotheses(X, x, K, samples, 1.0, want_masks=True)
    Rr, tr, vr, cr, mr = native.p3p_hypotheses(X, x, K, samples, 1.0, want_masks=True)
    d = first_difference(keys, (vg, Rg, tg, cg, mg), (vr, Rr, tr, cr, mr.astype(bool)), lambda h: "hypothesis %d" % h)
    assert d is None, d
    assert vg[0] == 1 and (cg[vg == 1] >= 3).all(), "a pose counts at least its own three points"


@pytest.fixture(scope="module")
def one_pose_scene():
    """257 points seen noise-free from one pose, and five samples of it"""
    rng = np.random.default_rng(77)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
    Xc = np.stack([rng.uniform(-4, 4, 257), rng.uniform(-2, 2, 257), rng.uniform(4, 20, 257)], axis=1)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, a, b, c = q
    R = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                  [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                  [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])
    t = np.array([0.5, -1.0, 2.0])
    X = (Xc - t) @ R
    x = np.stack([Xc[:, 0] / Xc[:, 2] * K[0, 0] + K[0, 2], Xc[:, 1] / Xc[:, 2] * K[1, 1] + K[1, 2]], axis=1)
    return K, X, x


@pytest.mark.parametrize("n", [4, 63, 64, 65, 257])
def test_population_edges_and_mask_stride(ctx, one_pose_scene, n):
    """The score kernel walks the population 256 at a time and writes ceil(n / 64) mask words per hypothesis: one
    word not full, exactly full, one bit into the next, and one point past the first 256.  Once with every point an
    inlier of the sampled pose (threshold 1 px^2 on noise-free data), once with none (threshold 0: the comparison is
    strict).  Counts and masks against the oracle, and straight from the device buffers, whose every other byte
    must keep its sentinel."""
    K, X, x = one_pose_scene
    X, x = X[:n].copy(), x[:n].copy()
    samples = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [n - 1, 0, n - 2, 1], [2, n - 1, 1, 0]], np.int32)
    hyp, words = len(samples), (n + 63) // 64
    d_X, d_x, d_s = ctx.to_device(X), ctx.to_device(x), ctx.to_device(samples)
    for thr, every in ((1.0, True), (0.0, False)):
        Rr, tr, vr, cr, mr = native.p3p_hypotheses(X, x, K, samples, thr, want_masks=True)
        assert vr.all(), "every sample of a noise-free scene yields a pose"
        assert (cr == (n if every else 0)).all()
        Rg, tg, vg, cg, mg = ctx.p3p_hypotheses(X, x, K, samples, thr, want_masks=True)
        assert np.array_equal(vg, vr) and np.array_equal(bits(Rg), bits(Rr)) and np.array_equal(bits(tg), bits(tr))
        assert np.array_equal(cg, cr) and np.array_equal(mg, mr.astype(bool))
        # the device form, every output buffer one row longer than needed and filled with a sentinel
        S8, S64 = 0xA5, np.uint64(0xA5A5A5A5A5A5A5A5)
        d_R = ctx.to_device(np.full((hyp + 1) * 72, S8, np.uint8))
        d_t = ctx.to_device(np.full((hyp + 1) * 24, S8, np.uint8))
        d_v = ctx.to_device(np.full(hyp + 8, S8, np.uint8))
        d_c = ctx.to_device(np.full((hyp + 1) * 4, S8, np.uint8))
        d_m = ctx.to_device(np.full((hyp + 1) * words, S64, np.uint64))
        ctx.p3p_hypotheses_dev(d_X, d_x, n, K, d_s, hyp, thr, d_R, d_t, d_v, d_c, d_m)
        ctx.sync()
        gR = ctx.download(d_R, ((hyp + 1) * 72,), np.uint8)
        gt = ctx.download(d_t, ((hyp + 1) * 24,), np.uint8)
        gv = ctx.download(d_v, (hyp + 8,), np.uint8)
        gc = ctx.download(d_c, ((hyp + 1) * 4,), np.uint8)
        gm = ctx.download(d_m, ((hyp + 1) * words,), np.uint64)
        for p in (d_R, d_t, d_v, d_c, d_m):
            ctx.free(p)
        assert np.array_equal(gR[:hyp * 72].view(np.uint64), bits(Rr).ravel()) and (gR[hyp * 72:] == S8).all()
        assert np.array_equal(gt[:hyp * 24].view(np.uint64), bits(tr).ravel()) and (gt[hyp * 24:] == S8).all()
        assert np.array_equal(gv[:hyp], vr) and (gv[hyp:] == S8).all()
        assert np.array_equal(gc[:hyp * 4].view(np.int32), cr) and (gc[hyp * 4:] == S8).all()
        want = np.zeros((hyp, words * 64), np.uint8)
        want[:, :n] = mr                                     # bits past n in the last word: zero
        want = np.packbits(want, axis=1, bitorder="little").view(np.uint64).reshape(hyp, words)
        assert np.array_equal(gm[:hyp * words].reshape(hyp, words), want), "mask rows: stride ceil(n / 64) words"
        assert (gm[hyp * words:] == S64).all()
    for p in (d_X, d_x, d_s):
        ctx.free(p)


# ---------------- reprojection edges ----------------
@pytest.mark.parametrize("n", [1, 257])
def test_reproj_depth_and_threshold_edges(ctx, n):
    """vo_reproj_inliers against oracle_reproj_errors on the bit patterns (infinities count): camera-frame depths of
    exactly 0 (the projection divides by 1 instead), -3 (behind the camera, still projected), 1e-300 and 1e300, and
    thresholds on either side of an error that is exactly 25 (dx = 3, dy = 4 on the optical axis; the comparison is
    strict).  One point per call, and one more than a 256-thread block."""
    K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])
    R, t = np.eye(3), np.zeros(3)
    rng = np.random.default_rng(5)
    special = np.array([[0.7, -0.4, 0.0], [0.7, -0.4, -3.0], [0.7, -0.4, 1e-300], [0.7, -0.4, 1e300], [0.0, 0.0, 1e-300],
                        [0.0, 0.0, 2.0]])
    pix = np.array([[300.0, 250.0]] * 5 + [[323.0, 244.0]])
    thrs = (25.0, np.nextafter(25.0, 0.0), np.nextafter(25.0, np.inf), 0.0, np.inf)
    if n == 1:
        sets = [(special[i:i + 1], pix[i:i + 1]) for i in range(len(special))]
    else:
        Xr = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(1, 30, n)], axis=1)
        xr = np.stack([Xr[:, 0] / Xr[:, 2] * 500 + 320, Xr[:, 1] / Xr[:, 2] * 500 + 240], axis=1) + rng.normal(0, 2, (n, 2))
        at = np.array([0, 63, 64, 255, 256, 100])            # block and wave boundaries
        Xr[at], xr[at] = special, pix
        sets = [(Xr, xr)]
    for X, x in sets:
        ref = native.reproj_errors(X, x, K, R, t)
        assert not np.isnan(ref).any()
        for thr in thrs:
            mask, err = ctx.reproj_inliers(X, x, K, R, t, thr, want_err=True)
            assert np.array_equal(bits(err), bits(ref)), "squared reprojection errors not bit-identical"
            assert np.array_equal(mask, ref < thr)
    e = native.reproj_errors(special[5:], pix[5:], K, R, t)[0]
    assert e == 25.0, "the threshold case is exactly representable"
    assert np.isinf(native.reproj_errors(special[2:3], pix[2:3], K, R, t)[0])
