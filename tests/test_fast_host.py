"""CPU checks of the FAST-9 definition (tests/fast_reference.py) and its case table (tests/fast_cases.py): the vectorised
definition against a plain per-pixel loop on every case, every case against the properties it is named for, the C ABI's
declarations, the tracker mode, and the match quality of FAST-9 + BRIEF-256 on the reference's KITTI frames 0 and 2."""
import os
import re

import numpy as np
import pytest

import brief_cases
import brief_reference as bref
import fast_cases as cases
import fast_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule, pixel by pixel ----
def slow_score_map(img, t, literal_only):
    """The rule as the header words it.  Every pixel gets the literal test "nine contiguous circle pixels all brighter
    than I + t, or all darker than I - t"; the max-min formula is evaluated at every pixel too unless literal_only (the
    large images), where it is evaluated at the corners the literal test finds."""
    H, W = img.shape
    rows = img.tolist()
    out = np.zeros((H, W), np.uint8)
    for y in range(3, H - 3):
        for x in range(3, W - 3):
            centre = rows[y][x]
            c = [rows[y + dy][x + dx] for dx, dy in ref.CIRCLE]
            brighter = "".join("1" if v > centre + t else "0" for v in c)
            darker = "".join("1" if v < centre - t else "0" for v in c)
            corner = "1" * 9 in brighter + brighter[:8] or "1" * 9 in darker + darker[:8]
            if literal_only and not corner:
                continue
            s = -256
            for k in range(16):
                w = [c[(k + j) % 16] for j in range(9)]
                s = max(s, min(w) - centre, centre - max(w))
            assert (s > t) == corner, (x, y, s)
            if corner:
                out[y, x] = s
    return out


def slow_survivors(score, nonmax):
    H, W = score.shape
    out = np.zeros_like(score)
    for y, x in zip(*np.nonzero(score)):
        s, keep = int(score[y, x]), True
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if (dx or dy) and 0 <= yy < H and 0 <= xx < W and nonmax:
                    q = int(score[yy, xx])
                    if q > s or (q == s and yy * W + xx < y * W + x):
                        keep = False
        if keep:
            out[y, x] = s
    return out


def slow_keypoints(surv, N):
    W = surv.shape[1]
    keys = sorted((-int(surv[y, x]), int(y) * W + int(x)) for y, x in zip(*np.nonzero(surv)))
    take = keys[:N]
    kp = np.array([(i % W, i // W) for _, i in take], np.float64).reshape(-1, 2)
    return kp, np.array([-s for s, _ in take], np.uint8), len(keys)


@pytest.mark.parametrize("name", cases.NAMES)
def test_definition_equals_the_per_pixel_loop_and_the_case_keeps_its_props(name):
    c, props = cases.BY_NAME[name], cases.PROPS[name]
    H, W = c.img.shape
    score = ref.score_map(c.img, c.threshold)
    assert score.dtype == np.uint8 and score.shape == (H, W)
    assert np.array_equal(score, slow_score_map(c.img, c.threshold, literal_only=H * W > 20000)), name
    border = np.ones((H, W), bool)
    border[3:max(H - 3, 3), 3:max(W - 3, 3)] = False
    assert not score[border].any()
    assert not np.any((score > 0) & (score <= c.threshold))
    got = {}
    for nonmax in (0, 1):
        surv = ref.survivor_map(score, nonmax)
        assert np.array_equal(surv, slow_survivors(score, nonmax)), (name, nonmax)
        kp, sc, total = ref.keypoints(c.img, c.threshold, nonmax, c.N)
        skp, ssc, stotal = slow_keypoints(surv, c.N)
        assert kp.dtype == np.float64 and kp.shape == (min(c.N, total), 2) and sc.dtype == np.uint8
        assert np.array_equal(kp, skp) and np.array_equal(sc, ssc) and total == stotal, (name, nonmax)
        got[nonmax] = (surv, kp, sc, total)
    surv, kp, sc, total = got[1]
    # two survivors are never adjacent, so they fit the bound the header states
    ys, xs = np.nonzero(surv)
    if len(ys) > 1:
        order = np.lexsort((xs, ys))
        pts = set(zip(xs[order].tolist(), ys[order].tolist()))
        assert not any((x + dx, y + dy) in pts for x, y in pts for dx, dy in ((1, 0), (-1, 1), (0, 1), (1, 1)))
    assert total <= -(-max(H - 6, 0) // 2) * -(-max(W - 6, 0) // 2)
    assert got[0][3] == np.count_nonzero(score)
    for (x, y), s in props.get("score_at", ()):
        assert score[y, x] == s, (name, x, y, int(score[y, x]))
    if "corners" in props:
        assert np.count_nonzero(score) == props["corners"], (name, np.count_nonzero(score))
    for (x, y), alive in props.get("survive_at", ()):
        assert score[y, x] > 0 and (surv[y, x] > 0) == alive, (name, x, y)
    if "survivors" in props:
        assert total == props["survivors"], (name, total)
    if "n" in props:
        assert len(kp) == props["n"], (name, len(kp))
    if "one_score" in props:
        assert total > 0 and set(surv[surv > 0].tolist()) == {props["one_score"]}, name
    if props.get("cut_in_class"):
        ordered = np.sort(surv[surv > 0])[::-1]
        assert total > c.N and ordered[c.N - 1] == ordered[c.N], name
    if "min_total" in props:
        assert got[0][3] >= props["min_total"][0] and total >= props["min_total"][1], (name, got[0][3], total)


def test_cases_cover_the_list():
    names = set(cases.NAMES)
    tw, th = cases.TILE_W, cases.TILE_H
    assert {"tiles_%dx%d" % (H, W) for H in (th - 1, th, th + 1, 2 * th + 1) for W in (tw - 1, tw, tw + 1, 2 * tw + 1)} <= names
    assert {"no_interior_6x40", "no_interior_40x6", "one_candidate_7x7", "two_candidates_7x8", "strip_9x150", "arc_9_brighter",
            "arc_8_brighter", "arc_9_darker", "arc_16_of_16", "difference_equals_threshold", "difference_threshold_plus_1",
            "score_255", "score_1_at_threshold_0", "threshold_254", "corners_at_3_3_and_opposite", "plateaus_across_tile_seams",
            "equal_scores_lower_index_wins", "plateau_a_a_a", "suppressed_corner_still_suppresses", "n_above_survivors", "n_1",
            "cut_inside_a_class", "one_score_survivors_far_above_n", "noise_70x131", "largest_n_16384"} <= names
    assert {"arc_wraps_from_%d" % s for s in (12, 13, 14, 15)} <= names
    # the tile shape the table is built around is the kernels'
    src = open(os.path.join(ROOT, "visual-odometry-project_amd", "csrc", "fast.hip")).read()
    m = re.search(r"constexpr int FX = (\d+), FY = (\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (tw, th)
    big = cases.BY_NAME["largest_n_16384"]
    assert big.img.shape == (480, 640) == max((c.img.shape for c in cases.CASES), key=lambda s: s[0] * s[1])
    assert big.N == ref.MAX_KEYPOINTS
    assert sorted(len(lanes) for _, lanes, _, _ in cases.BATCH)[-1] == 5 and {1, 2, 5} <= {len(b[1]) for b in cases.BATCH}
    for _, lanes, t, N in cases.BATCH:
        assert len({cases.BY_NAME[n].img.shape for n in lanes}) == 1
    s5 = [b for b in cases.BATCH if len(b[1]) == 5][0]
    totals = [ref.keypoints(cases.BY_NAME[n].img, s5[2], True, s5[3])[2] for n in s5[1]]
    assert totals[1] == 0 and totals[0] > s5[3] and totals[2] > s5[3]           # a flat image between two busy ones


# ---- ABI, classes ----
def test_header_declares_the_fast_entry_points():
    from vo import _native
    header = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", text))
    new = {"vo_fast_score", "vo_fast_keypoints", "vo_fast_keypoints_batch", "vo_fast_keypoints_batch_dev"}
    assert new <= names and new <= set(_native._SIGS)
    ids = dict(re.findall(r"\b(VO_K_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert int(ids["VO_K_COUNT"]) == _native.K_COUNT == 38                      # the new kernels take no profiling id
    import ctypes
    lib = ctypes.CDLL(_native.lib_path())
    assert all(hasattr(lib, n) for n in new)
    # a call without a context is refused before anything touches a device
    assert lib.vo_fast_score(None, None, 8, 8, 20, None) == _native.VO_EINVAL
    assert lib.vo_fast_keypoints(None, None, 8, 8, 20, 1, 10, None, None, None) == _native.VO_EINVAL


def test_tracker_knows_the_fast_mode():
    from vo.features import BRIEFDetector, FASTBRIEFDetector, tracker
    assert tracker._TRACKERS["fast"] == (FASTBRIEFDetector, "get_brief_matches")
    assert issubclass(FASTBRIEFDetector, BRIEFDetector)
    d = FASTBRIEFDetector()
    assert (d._detector, d._threshold, d._num_keypoints, d._oriented, d._match_ratio, d._max_distance) == (
        "fast", 20, 1000, False, 0.8, 64)
    for name in ("extractDescriptors", "matchDescriptor", "get_brief_matches"):
        assert getattr(FASTBRIEFDetector, name) is getattr(BRIEFDetector, name)
    FASTBRIEFDetector._num_keypoints_override = 300
    try:
        assert FASTBRIEFDetector(num_keypoints=50)._num_keypoints == 300
        assert BRIEFDetector(num_keypoints=50)._num_keypoints == 50            # (the override is the class's own)
    finally:
        FASTBRIEFDetector._num_keypoints_override = None
    with pytest.raises(ValueError):
        BRIEFDetector(detector="fast")


# ---- match quality on the reference's KITTI frames 0 and 2 ----
def test_match_quality_on_kitti_fast_keypoints():
    """The definition's 1000 strongest FAST-9 survivors per frame at threshold 20 (FASTBRIEFDetector's defaults) on frames
    0 and 2, BRIEF-256 at its defaults (not oriented, ratio 0.8, max_distance 64); pairs whose Sampson distance to the
    ground-truth epipolar geometry is under 2 px, as tests/test_brief_host.py measures the patch route (569 pairs,
    96.84 %) and BRIEF on Harris keypoints (577 pairs, 97.75 %).  Measured here on the CPU: 570 pairs, 96.67 % under 2 px;
    the cut falls at scores 37 and 38, so every threshold up to 36 gives the same keypoints."""
    from oracle import harris_np, native
    img0, img2, _, F = brief_cases.kitti_pair()
    hk = [harris_np.nms_keypoints_fast(harris_np.harris_scores(img, 9, 0.09), 1000, 5)[:, :, 0] for img in (img0, img2)]
    patches = [harris_np.patch_descriptors(img, k.reshape(-1, 2, 1), 9).reshape(len(k), -1).astype(np.float32)
               for img, k in zip((img0, img2), hk)]
    pp = native.match_knn2_ratio(patches[0], patches[1], 0.85)[0]
    found = [ref.keypoints(img, 20, True, 1000) for img in (img0, img2)]
    kp = [f[0] for f in found]
    assert all(len(k) == 1000 for k in kp)
    desc = [bref.describe(img, k, False)[0] for img, k in zip((img0, img2), kp)]
    bp = bref.match(desc[0], desc[1], 0.8, 64)
    share = float(np.mean(brief_cases.sampson_px(F, kp[0][bp[:, 0]], kp[1][bp[:, 1]]) < 2.0))
    print("patch route: %d pairs; FAST-9 + BRIEF-256: %d pairs, %.4f under 2 px; cutting scores %s, survivors %s" % (
        len(pp), len(bp), share, [int(f[1][-1]) for f in found], [f[2] for f in found]))
    assert share >= 0.95
    assert 2 * len(bp) >= len(pp)
