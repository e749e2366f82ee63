"""The SIFT oracle (oracle/csrc/sift.c) against the float64 definition of tests/sift_reference.py, on the CPU: its
polynomials against libm, its scale space, keypoints and histograms stage by stage, its final rows end to end, analytic
ground truth (Gaussian blobs, one dominant gradient direction, transposition) on the definition and on the oracle, and the
final order, duplicate rule and cap on hand-made rows.  tests/test_gpu_sift_reference.py runs the end-to-end and analytic
checks on the kernels.

Figures measured here (CPU), see DESIGN.md section 2, "SIFT definition":
  sift_atan2 against atan2: ATAN2_ERR_DEG at most (the fit error of fastAtan2's polynomial plus float32 rounding), for
    vectors longer than 1e-6; shorter ones fall towards 0 / 90 / 180 / 270 (the 2.2e-16 added to the denominator)
  sift_exp against exp, relative: EXP_ERR_REL on [-8, 0], where every weight above 3e-4 lies; EXP_ERR_REL_87 on [-87, 0]
    (the argument x log2(e) is rounded to float32: 6e-8 |x|); exactly 0 below -87
  the descriptor's sin / cos against libm: SINCOS_ERR absolute
  float64 against float32 run of the definition: histogram 1.34e-5 of its maximum, angle 8.1e-5 degrees, descriptor 3.3e-3"""
import math

import numpy as np
import pytest

import sift_cases as sc
import sift_reference as ref
from oracle import native

#: the measured maxima of measure_polynomials(); each is asserted at 1.5 x (these are properties of fixed polynomials)
ATAN2_ERR_DEG, EXP_ERR_REL, EXP_ERR_REL_87, SINCOS_ERR = 0.0096, 5.1e-7, 3.9e-6, 4.7e-7
#: how far the definition itself (so anything within its bounds) is from the closed forms, measured on BLOBS: the position
#: bias of the doubling is 0.25 px, size / s tends to 2 * 2^(-1/6) from below as the sampling gets finer
BLOB_BIAS, BLOB_BIAS_TOL = 0.25, 0.04                # the definition: 0.231 ... 0.283
SIZE_RATIO = 2.0 * 2.0 ** (-1.0 / 6.0)
#: the definition: 1.742 .. 1.747, 1.750 .. 1.759, 1.763 .. 1.772, 1.776 .. 1.777, 1.7785 .. 1.7786 of 1.7818
SIZE_RATIO_BELOW = {3.0: 0.05, 4.5: 0.04, 6.0: 0.025, 8.0: 0.008, 9.0: 0.005}
#: the definition's own angle on the patterns of sift_cases.oriented is within 6.9 degrees of phi (10-degree bins and a
#: window centred on a whole pixel); a wrong sign or axis is off by 60 degrees or more on 30 / 100 / 200 / 310
ORIENTATION_TOL_DEG = 9.0


def measure_polynomials():
    xs = np.concatenate([np.linspace(-3, 3, 61), [1e-38, -1e-38, 1e-30, 1e30, -1e30, 255.0, -255.0, 0.0]]).astype(np.float32)
    Y, X = np.meshgrid(xs, xs, indexing="ij")
    Y, X = Y.ravel(), X.ravel()
    keep = np.maximum(np.abs(X), np.abs(Y)) > 1e-6
    got = native.sift_atan2(Y, X).astype(np.float64)
    want = np.mod(np.degrees(np.arctan2(Y.astype(np.float64), X.astype(np.float64))), 360.0)
    atan = float(np.max(np.abs((got - want + 180.0) % 360.0 - 180.0)[keep]))
    x = np.concatenate([np.linspace(-87, 0, 4001), -np.logspace(-8, 1.9, 400)]).astype(np.float32)
    rel = np.abs(native.sift_exp(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1)
    e = float(rel[x >= -8].max()), float(rel.max())
    deg = np.concatenate([np.linspace(0, 360, 2881)[:-1], [90.0, 270.0, 89.99999, 90.00001, 269.99997, 270.00003]]).astype(np.float32)
    s_c = native.sift_sincos(deg).astype(np.float64)
    rad = np.radians(deg.astype(np.float64))
    sc_err = float(max(np.abs(s_c[:, 0] - np.sin(rad)).max(), np.abs(s_c[:, 1] - np.cos(rad)).max()))
    return atan, e, sc_err


# ---------------------------------------------------------------- polynomials
def test_polynomials_against_libm():
    atan, e, s_c = measure_polynomials()
    print("atan2 %.3g deg, exp %.3g / %.3g relative, sin/cos %.3g" % (atan, e[0], e[1], s_c))
    assert atan <= 1.5 * ATAN2_ERR_DEG and s_c <= 1.5 * SINCOS_ERR
    assert e[0] <= 1.5 * EXP_ERR_REL and e[1] <= 1.5 * EXP_ERR_REL_87
    tiny = native.sift_atan2(np.float32([1e-38, 1e-30, -1e-38]), np.float32([1e-38, 1e-30, 1e-38]))
    assert np.all((tiny < 1e-9) | (tiny == 360)), "a vector far below 2.2e-16 has angle 0: its magnitude, the weight, is 0 too"
    assert float(native.sift_atan2(0.0, 0.0)[0]) == 0.0
    assert np.all(native.sift_exp([-87.5, -100.0, -1e30]) == 0) and float(native.sift_exp([0.0])[0]) == 1.0
    for y, x, want in ((0, 1, 0), (1, 0, 90), (0, -1, 180), (-1, 0, 270), (1e30, 1e-30, 90), (-1e-30, -1e30, 180)):
        assert abs(float(native.sift_atan2(y, x)[0]) - want) <= 1.5 * ATAN2_ERR_DEG, (y, x)


def test_definitions_cv_atan2_is_the_oracles_polynomial_and_near_the_real_one():
    rng = np.random.default_rng(0)
    y, x = rng.normal(size=4000), rng.normal(size=4000)
    y[:8], x[:8] = (0, 1, 0, -1, 1, -1, 1, -1), (1, 0, -1, 0, 1, 1, -1, -1)
    cv, real = ref.atan2_cv(y, x), ref.atan2_real(y, x)
    assert np.max(np.abs((cv - real + 180) % 360 - 180)) <= 1.5 * ATAN2_ERR_DEG
    got = native.sift_atan2(y.astype(np.float32), x.astype(np.float32)).astype(np.float64)
    cv32 = ref.atan2_cv(y.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64))
    assert np.max(np.abs((got - cv32 + 180) % 360 - 180)) <= 64 * 360 * ref.U


# ---------------------------------------------------------------- the definition's own stages
def test_sigma_ladder_taps_and_octaves():
    total, inc, taps = ref.sigma_ladder()
    assert np.allclose(total, [1.6 * 2 ** (i / 3) for i in range(6)]) and total[3] == pytest.approx(3.2)
    assert inc[0] == pytest.approx(math.sqrt(1.6 ** 2 - 1))
    for i in range(1, 6):
        assert inc[i] ** 2 + total[i - 1] ** 2 == pytest.approx(total[i] ** 2)
    assert taps == [11, 11, 13, 17, 21, 27]
    assert [ref.num_octaves(h, w) for h, w in ((6, 6), (7, 7), (12, 40), (16, 16), (14, 200), (97, 131), (64, 128))] == \
        [0, 1, 1, 2, 2, 4, 4]
    assert ref.DOG_THRESHOLD == 1


def test_base_image_and_blur_closed_forms():
    img = np.arange(12, dtype=np.uint8).reshape(3, 4) * 10
    b = ref.base_image(img)
    assert b.shape == (6, 8) and b[0, 0] == 0 and b[0, 1] == 2.5 and b[0, 2] == 7.5 and b[1, 0] == 10 and b[-1, -1] == 110
    ramp = np.tile(np.arange(40.0), (9, 1))
    out = ref.blur(ramp, 1.5, 13)
    assert np.allclose(out[:, 6:-6], ramp[:, 6:-6]) and np.allclose(ref.blur(np.full((5, 7), 3.0), 2.0, 17), 3.0)
    eg, ed = ref.pyramid_bounds(2)
    assert eg[0][0] == pytest.approx((3 + 2 * 13) * 255 * 2.0 ** -24) and eg[1][0] == eg[0][3]
    assert ed[0][0] == pytest.approx(eg[0][0] + eg[0][1] + 2 * 255 * 2.0 ** -24)


def test_measured_tolerances():
    """HIST_TOL, ANGLE_TOL, DESC_TOL are 4 x the largest float64 - float32 distance of the definition over the cases."""
    m = sc.measure_rounding()
    print({k: v for k, v in m.items()})
    for name, tol in (("hist", ref.HIST_TOL), ("angle", ref.ANGLE_TOL), ("desc", ref.DESC_TOL)):
        assert 4 * m["all"][name] <= tol <= 8 * m["all"][name], (name, m["all"][name], tol)


def test_cases_reach_the_edges_they_are_named_for():
    d = {n: sc.definition(n) for n in sc.NAMES}
    assert not d["below6x6"].pyramid and not d["flat40x40"].keypoints and len(d["smallest7x7"].pyramid) == 1
    assert len(d["oneoctave12x40"].pyramid) == 1 and len(d["strip14x200"].pyramid) == 2 and len(d["strip16x200"].pyramid) == 2
    every = [k for r in d.values() for k in r.keypoints if k.accepted]
    moved = [k for k in every if len(k.trajectory) > 1]
    assert any(t[0][0] != k.layer for k in moved for t in [k.trajectory]), "no refinement crosses a layer"
    assert any(r.reason == "left" and r.accepted for x in d.values() for r in x.rejected), "no refinement leaves the border"
    assert any(r.reason == "contrast" for x in d.values() for r in x.rejected) and any(r.reason == "edge" for x in d.values() for r in x.rejected)
    b = d["borders64x64"]
    H, W = 128, 128
    clip = {"left": False, "right": False, "top": False, "bottom": False, "corner": False}
    for k in b.keypoints:
        if k.octave == 0 and k.accepted:
            lo_x, hi_x, lo_y, hi_y = k.c - k.desc_radius < 1, k.c + k.desc_radius > W - 2, k.r - k.desc_radius < 1, k.r + k.desc_radius > H - 2
            clip["left"] |= lo_x
            clip["right"] |= hi_x
            clip["top"] |= lo_y
            clip["bottom"] |= hi_y
            clip["corner"] |= (lo_x or hi_x) and (lo_y or hi_y)
    assert all(clip.values()), clip
    assert any(k.octave == 0 and ref.BORDER in (k.c, k.r) for k in b.keypoints if k.accepted), "no keypoint on the 5-pixel border"
    ck = [k for k in d["checker48x48"].keypoints if k.accepted]
    assert max(sum(1 for q in ck if (q.octave, q.layer, q.r, q.c) == (k.octave, k.layer, k.r, k.c)) for k in ck) >= 2, \
        "no position with several orientation peaks"
    assert any(len([k for k in r.keypoints if k.accepted]) > len(sc.unique_keypoints(r)) for r in d.values()), \
        "no two candidates refine to one keypoint (exact duplicates)"
    tw = native.sift(sc.BY_NAME["twins64x128"].img)[0]
    assert sc.tied_cap(tw) is not None, "the twin patterns have no tied responses"


# ---------------------------------------------------------------- the oracle, stage by stage and end to end
def _stages(img):
    out, o = [], 0
    while True:
        out.append(native.sift_stages(img, o))
        if out[-1] is None:
            return out
        o += 1


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_stages_match_definition(name):
    c = sc.BY_NAME[name]
    fig = {}
    try:
        sc.check_stages(c, sc.definition(name), _stages(c.img), fig)
    finally:
        print(name, {k: round(float(v), 3) for k, v in fig.items()})


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_rows_match_definition(name):
    c = sc.BY_NAME[name]
    kp, desc = native.sift(c.img)
    fig = {}
    try:
        sc.check_rows(sc.definition(name), kp, desc, fig, name)
    finally:
        print(name, {k: round(float(v), 3) for k, v in fig.items()})
    for cap in {1, sc.tied_cap(kp) or 2, len(kp) + 3}:
        sc.check_cap(kp, native.sift(c.img, cap=cap)[0], cap)


# ---------------------------------------------------------------- analytic ground truth
def strongest(d):
    return max(sc.unique_keypoints(d), key=lambda k: k.response)


def check_blob(blob, kp, figures=None):
    """The strongest row of an implementation on a blob image: at the centre + 0.25 px, size / s the definition's, both
    within twice the definition's bounds; and within the stated distance of the closed forms."""
    _, _, cx, cy, s = blob
    k = strongest(sc.definition_of(("blob",) + blob))
    q = kp[int(np.argmax(kp[:, 4]))].astype(np.float64)
    assert abs(q[0] - k.xy[0]) <= 2 * k.xy_bound and abs(q[1] - k.xy[1]) <= 2 * k.xy_bound and abs(q[2] - k.size) <= 2 * k.size_bound
    for v in (q[0] - cx, q[1] - cy):
        assert abs(v - BLOB_BIAS) <= BLOB_BIAS_TOL, (blob, q)
    assert SIZE_RATIO - SIZE_RATIO_BELOW[s] <= q[2] / s <= SIZE_RATIO, (blob, q[2] / s)
    if figures is not None:
        figures[blob] = (q[0] - cx, q[1] - cy, q[2] / s)


@pytest.mark.parametrize("blob", sc.BLOBS, ids=lambda b: "s%g@%g,%g" % (b[4], b[2], b[3]))
def test_blob_position_bias_and_size(blob):
    d = sc.definition_of(("blob",) + blob)
    k = strongest(d)
    rows = np.array([[k.xy[0], k.xy[1], k.size, k.angle, k.response, k.octave - 1]])
    fig = {}
    check_blob(blob, rows, fig)                                   # the definition against the closed forms
    check_blob(blob, native.sift(sc.image_of(("blob",) + blob))[0], fig)
    print(blob, fig, "layer + xi %.3f radii %d %d" % (k.layer + k.x[2], k.ori_radius, k.desc_radius))
    if blob[4] == 8.0:
        assert k.layer + k.x[2] > 3.3 and (k.ori_radius, k.desc_radius) == (16, 38), "the largest radii are not reached"


def check_orientation(phi, kp):
    near = kp[np.argmin(np.abs(kp[:, 0] - 33.25) + np.abs(kp[:, 1] - 30.25))]
    assert abs(near[0] - 33.25) < 1 and abs(near[1] - 30.25) < 1, near
    here = kp[(np.abs(kp[:, 0] - near[0]) < 1e-3) & (np.abs(kp[:, 1] - near[1]) < 1e-3)]
    assert len(here) == 1, "one dominant direction, %d keypoints" % len(here)
    assert sc.angle_diff(float(near[3]), phi) <= ORIENTATION_TOL_DEG, (phi, near[3])
    return float(near[3])


@pytest.mark.parametrize("phi", sc.ORIENTATIONS)
def test_orientation_is_clockwise_on_screen_from_x(phi):
    d = sc.definition_of(("ori", phi))
    a = check_orientation(phi, d.rows[[i for i, k in enumerate(d.keypoints) if k.accepted]].astype(np.float64))
    b = check_orientation(phi, native.sift(sc.image_of(("ori", phi)))[0])
    print(phi, a, b)


def check_transposition(name, kp, desc, kp_t, desc_t, figures=None):
    """Rows of an image and of its transpose: every keypoint the definition decides in both has its mirror image -- (y, x),
    same size and response within twice the bounds, angle 90 - angle, descriptor permuted."""
    d, dt = sc.definition(name), sc.definition_of(("T", name))
    mirror = {(k.octave, k.layer, k.c, k.r): k for k in sc.unique_keypoints(dt)}
    n = 0
    for k in sc.unique_keypoints(d):
        m = mirror.get((k.octave, k.layer, k.r, k.c))
        if m is None or not (k.decided and m.decided):
            continue
        rows = [q for q in range(len(kp)) if kp[q, 5] == k.octave - 1 and abs(kp[q, 0] - k.xy[0]) <= 2 * k.xy_bound
                and abs(kp[q, 1] - k.xy[1]) <= 2 * k.xy_bound and sc.angle_diff(kp[q, 3], k.angle) <= ref.ANGLE_TOL]
        assert len(rows) == 1
        q = rows[0]
        hits = [p for p in range(len(kp_t)) if kp_t[p, 5] == kp[q, 5]
                and abs(kp_t[p, 0] - kp[q, 1]) <= 2 * (k.xy_bound + m.xy_bound) and abs(kp_t[p, 1] - kp[q, 0]) <= 2 * (k.xy_bound + m.xy_bound)
                and abs(kp_t[p, 2] - kp[q, 2]) <= 2 * (k.size_bound + m.size_bound)
                and sc.angle_diff(float(kp_t[p, 3]), 90.0 - float(kp[q, 3])) <= 2 * ref.ANGLE_TOL]
        assert len(hits) == 1, (name, kp[q], len(hits))
        diff = np.abs(sc.transpose_descriptor(desc[q]) - desc_t[hits[0]]).max()
        assert diff <= 1 + 2 * ref.DESC_TOL, (name, kp[q], diff)          # two roundings of entries 2 DESC_TOL apart
        n += 1
    if figures is not None:
        figures[name] = n
    return n


TRANSPOSED = ["blocks65x33", "strip16x200", "oneoctave12x40", "blocks64x64"]


@pytest.mark.parametrize("name", TRANSPOSED)
def test_transposition(name):
    d, dt = sc.definition(name), sc.definition_of(("T", name))
    rows = lambda r: (r.rows.astype(np.float64), np.array([k.desc for k in r.keypoints]).reshape(-1, 128))
    a = [k.accepted for k in d.keypoints]
    b = [k.accepted for k in dt.keypoints]
    n = check_transposition(name, rows(d)[0][a], rows(d)[1][a], rows(dt)[0][b], rows(dt)[1][b])
    assert n >= 3, "too few keypoints decided in both images: %d" % n
    c = sc.BY_NAME[name]
    assert check_transposition(name, *native.sift(c.img), *native.sift(sc.image_of(("T", name)))) == n


# ---------------------------------------------------------------- final order, duplicates, cap
ROWS = np.array([
    # x, y, size, angle, response, octave
    [5.0, 9.0, 2.0, 10.0, 0.05, 0], [5.0, 3.0, 2.0, 10.0, 0.05, 0], [4.0, 9.0, 2.0, 10.0, 0.05, 0],      # x, then y
    [5.0, 3.0, 4.0, 10.0, 0.05, 1], [5.0, 3.0, 2.0, 5.0, 0.05, 0],                                      # size desc, then angle
    [5.0, 3.0, 2.0, 5.0, 0.09, 0], [5.0, 3.0, 2.0, 5.0, 0.09, 2], [5.0, 3.0, 2.0, 5.0, 0.01, 0],         # duplicates of the last
    [7.0, 1.0, 3.0, 0.0, 0.05, 0], [7.0, 1.0, 3.0, 359.9, 0.05, 0], [8.0, 1.0, 3.0, 0.0, 0.02, -1],
    [9.0, 1.0, 3.0, 0.0, 0.05, 0], [9.5, 1.0, 3.0, 0.0, 0.05, 1], [9.75, 1.0, 3.0, 0.0, 0.3, 1]], np.float32)


def test_final_order_duplicates_and_cap_on_hand_made_rows():
    order = ref.finish(ROWS)
    assert list(order) == [2, 3, 6, 1, 0, 8, 9, 10, 11, 12, 13]
    # [5, 3, 2, 5]: the row with the largest response and then the largest octave stays, its duplicates go
    for cap in (1000, len(order), 7, 6, 5, 4, 3, 2, 1):
        want = ref.finish(ROWS, cap)
        assert list(native.sift_finish(ROWS, cap)) == list(want), cap
        assert len(want) == min(cap, len(order))
    # five rows tie at response 0.05 after the three stronger ones: a cap inside the run keeps the first of them in order
    assert list(ref.finish(ROWS, 5)) == [2, 3, 6, 1, 13]
    rng = np.random.default_rng(5)
    for _ in range(20):
        r = np.round(rng.uniform(0, 3, size=(60, 6)), 0).astype(np.float32)
        for cap in (1, 7, 30, 100):
            assert list(native.sift_finish(r, cap)) == list(ref.finish(r, cap))
