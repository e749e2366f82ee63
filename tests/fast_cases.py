"""The case table of the FAST-9 tests.  tests/test_gpu_fast.py runs every case on the device against
tests/fast_reference.py, with nonmax 0 and 1; tests/test_fast_host.py checks on the CPU that the reference agrees with a
plain per-pixel loop on every case and that every case still has the edge its PROPS promise.

CASES: (name, img (H, W) uint8, threshold, N).  PROPS[name] (all exact, all optional):
  score_at     ((x, y), s) pairs: the score map there (0: not a corner)
  corners      the number of corners in the map
  survive_at   ((x, y), bool) pairs: whether that corner survives the suppression
  survivors    the survivors with nonmax = 1
  n            the keypoints with nonmax = 1
  one_score    every survivor (nonmax = 1) has this score
  cut_in_class the N-th and (N+1)-th survivors (nonmax = 1) share a score: the cut is decided by index
  min_total    at least this many survivors with nonmax = 0 and with nonmax = 1 (a pair)
BATCH: (name, [case names of one shape], threshold, N): lanes of one batched call.
The kernels' tile is TILE_W x TILE_H pixels (csrc/fast.hip: FX x FY); the shapes below sit at one tile - 1, + 0, + 1 and at
two tiles + 1 in both directions.  All inputs come from seeded generators."""
import collections

import numpy as np

import fast_reference as ref

TILE_W, TILE_H = 64, 16
FastCase = collections.namedtuple("FastCase", "name img threshold N")
CASES, PROPS = [], {}
BATCH = []
GROUND = 100


def _add(name, img, threshold, N, **props):
    assert name not in PROPS, name
    img = np.ascontiguousarray(img, np.uint8)
    img.flags.writeable = False
    CASES.append(FastCase(name, img, int(threshold), int(N)))
    PROPS[name] = props


def noise(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W)).astype(np.uint8)


def steps(seed, H, W, levels=4, step=60):
    """Few grey levels: whole classes of equal scores."""
    return (np.random.default_rng(seed).integers(0, levels, size=(H, W)) * step).astype(np.uint8)


def flat(H, W, v=GROUND):
    return np.full((H, W), v, np.uint8)


def plant(img, x, y, centre, circle):
    """The centre byte and the sixteen circle bytes (c_0 .. c_15; None: left as it is) of pixel (x, y)."""
    img[y, x] = centre
    for (dx, dy), v in zip(ref.CIRCLE, circle):
        if v is not None:
            img[y + dy, x + dx] = v
    return img


def arc(start, length, v, rest=None):
    out = [rest] * 16
    for j in range(length):
        out[(start + j) % 16] = v
    return out


def _build_shapes():
    for H, W in ((6, 40), (40, 6)):
        _add("no_interior_%dx%d" % (H, W), noise(H * W, H, W), 5, 50, corners=0, survivors=0, n=0)
    img = plant(flat(7, 7, 200), 3, 3, 0, [200] * 16)
    _add("one_candidate_7x7", img, 20, 50, score_at=[((3, 3), 200)], corners=1, survivors=1, n=1)
    img = plant(flat(7, 8, 200), 4, 3, 10, [200] * 16)
    _add("two_candidates_7x8", img, 20, 50, score_at=[((3, 3), 0), ((4, 3), 190)], corners=1, n=1)
    _add("strip_9x150", steps(3, 9, 150), 5, 50, min_total=(40, 20))
    _add("strip_150x9", steps(4, 150, 9), 5, 50, min_total=(40, 20))
    for H in (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1):
        for W in (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1):
            _add("tiles_%dx%d" % (H, W), steps(H * 1000 + W, H, W), 5, 40, min_total=(60, 20))


def _build_arcs():
    t = 20

    def one(name, centre, circle, threshold, want, ground=GROUND, **props):
        img = plant(flat(24, 30, ground), 12, 11, centre, circle)
        _add(name, img, threshold, 50, score_at=[((12, 11), want)], **props)

    one("arc_9_brighter", GROUND, arc(3, 9, GROUND + 50), t, 50)
    one("arc_8_brighter", GROUND, arc(3, 8, GROUND + 50), t, 0)
    one("arc_9_darker", GROUND, arc(5, 9, GROUND - 50), t, 50)
    one("arc_8_darker", GROUND, arc(5, 8, GROUND - 50), t, 0)
    for s in (12, 13, 14, 15):
        one("arc_wraps_from_%d" % s, GROUND, arc(s, 9, GROUND + 40 + s), t, 40 + s)
        one("arc_of_8_wraps_from_%d" % s, GROUND, arc(s, 8, GROUND + 40 + s), t, 0)
    one("arc_16_of_16", GROUND, [GROUND + 33] * 16, t, 33)
    one("difference_equals_threshold", GROUND, arc(0, 9, GROUND + t), t, 0, corners=0)
    one("difference_threshold_plus_1", GROUND, arc(0, 9, GROUND + t + 1), t, t + 1)
    one("darker_equals_threshold", GROUND, arc(7, 9, GROUND - t), t, 0, corners=0)
    one("darker_threshold_plus_1", GROUND, arc(7, 9, GROUND - t - 1), t, t + 1)
    one("score_255", 0, [255] * 16, t, 255, ground=255)
    one("score_1_at_threshold_0", GROUND, arc(2, 9, GROUND + 1), 0, 1)
    one("threshold_254", 0, [255] * 16, 254, 255, ground=255, corners=1)
    one("threshold_254_difference_254", 1, [255] * 16, 254, 0, ground=255, corners=0)
    # Nine brighter and nine darker pixels cannot share a circle of sixteen, so no pixel has both arcs qualify at once.
    # What the two sides can do together: a qualifying bright arc whose complement is darker by more (the score is the
    # qualifying side's, 30, not 70), ...
    one("bright_arc_qualifies_dark_side_larger", GROUND, arc(0, 9, GROUND + 30, GROUND - 70), t, 30)
    one("dark_arc_qualifies_bright_side_larger", GROUND, arc(11, 9, GROUND - 25, GROUND + 90), t, 25)
    # ... and an arc of ten with unequal differences: two windows of nine qualify, with minima 30 and 45
    c = arc(2, 10, GROUND + 60)
    c[2], c[11] = GROUND + 30, GROUND + 45
    one("windows_with_different_minima", GROUND, c, t, 45)
    c = arc(9, 10, GROUND - 60)                              # (c_9 .. c_15, c_0 .. c_2)
    c[9], c[2] = GROUND - 30, GROUND - 45
    one("dark_windows_with_different_minima", GROUND, c, t, 45)


def _dark(img, pts, v=0):
    for x, y in pts:
        img[y, x] = v
    return img


def _build_border_and_seams():
    H, W = 20, 26
    img = _dark(flat(H, W, 200), [(3, 3), (W - 4, H - 4)])
    # ... on a ground that would make corners of the border of 3 if the rule were applied there with any padding
    img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = 0
    _add("corners_at_3_3_and_opposite", img, 20, 50, score_at=[((3, 3), 200), ((W - 4, H - 4), 200), ((2, 3), 0), ((3, 2), 0),
                                                                ((W - 3, H - 4), 0), ((W - 4, H - 3), 0)], n=2)
    # 2 x 2 blocks of equal scores across every seam of 2 x 2 tiles and across the corner where four tiles meet
    H, W = 2 * TILE_H + 8, 2 * TILE_W + 8
    sx, sy = TILE_W, TILE_H
    blocks = [(sx - 1, 6), (sx - 1, sy + 9), (10, sy - 1), (sx + 30, sy - 1), (sx - 1, sy - 1)]
    img = flat(H, W, 200)
    at, sv = [], []
    for bx, by in blocks:
        four = [(bx, by), (bx + 1, by), (bx, by + 1), (bx + 1, by + 1)]
        _dark(img, four)
        at += [(p, 200) for p in four]
        sv += [(four[0], True)] + [(p, False) for p in four[1:]]
    _add("plateaus_across_tile_seams", img, 20, 50, score_at=at, survive_at=sv, corners=20, survivors=5, n=5, one_score=200)
    # different scores on the two sides of each seam: the survivor is on the far side
    img = flat(H, W, 200)
    _dark(img, [(sx - 1, 8), (10, sy - 1), (sx - 1, sy - 1)], 90)
    _dark(img, [(sx, 8), (10, sy), (sx, sy)], 50)
    _add("stronger_corner_beyond_the_seam", img, 20, 50,
         score_at=[((sx - 1, 8), 110), ((sx, 8), 150), ((10, sy - 1), 110), ((10, sy), 150), ((sx - 1, sy - 1), 110), ((sx, sy), 150)],
         survive_at=[((sx - 1, 8), False), ((sx, 8), True), ((10, sy - 1), False), ((10, sy), True), ((sx - 1, sy - 1), False),
                     ((sx, sy), True)], corners=6, survivors=3, n=3)


def _build_suppression():
    H, W = 24, 60
    img = flat(H, W, 200)
    pairs = {"left_right": [(8, 6), (9, 6)], "up_down": [(20, 6), (20, 7)], "diagonal": [(30, 6), (31, 7)],
             "anti_diagonal": [(41, 6), (40, 7)]}
    at, sv = [], []
    for pts in pairs.values():
        _dark(img, pts)
        at += [(p, 200) for p in pts]
        sv += [(pts[0], True), (pts[1], False)]                # pts[0] has the lower index
    _add("equal_scores_lower_index_wins", img, 20, 50, score_at=at, survive_at=sv, corners=8, survivors=4, n=4)
    img = _dark(flat(H, W, 200), [(10, 10), (11, 10), (12, 10)])
    _add("plateau_a_a_a", img, 20, 50, score_at=[((10, 10), 200), ((11, 10), 200), ((12, 10), 200)],
         survive_at=[((10, 10), True), ((11, 10), False), ((12, 10), False)], corners=3, survivors=1, n=1)
    # scores 100, 150, 200 in a row: the middle one is suppressed by the right one and still suppresses the left one (a
    # greedy walk from the strongest would keep the left one)
    img = flat(H, W, 200)
    img[10, 10], img[10, 11], img[10, 12] = 100, 50, 0
    _add("suppressed_corner_still_suppresses", img, 20, 50, score_at=[((10, 10), 100), ((11, 10), 150), ((12, 10), 200)],
         survive_at=[((10, 10), False), ((11, 10), False), ((12, 10), True)], corners=3, survivors=1, n=1)


def _build_selection():
    _add("n_above_survivors", steps(11, 40, 50), 5, 2000, min_total=(100, 50))
    _add("n_1", steps(12, 40, 50), 5, 1, n=1)
    _add("cut_inside_a_class", steps(13, 40, 90), 5, 30, cut_in_class=True)
    _add("one_score_survivors_far_above_n", steps(14, 70, 131, levels=3, step=100), 5, 50, one_score=100, cut_in_class=True,
         min_total=(700, 400))                                   # (761 corners, 479 survivors, all of score 100)
    _add("steps_70x131", steps(15, 70, 131), 5, 50, cut_in_class=True, min_total=(1000, 300))
    _add("noise_70x131", noise(16, 70, 131), 5, 50, min_total=(1000, 500))
    _add("largest_n_16384", noise(17, 480, 640), 5, 16384, min_total=(30000, 16385))
    _add("largest_blocky_n_1000", np.kron(steps(18, 120, 160), np.ones((4, 4), np.uint8)), 20, 1000, min_total=(1000, 1000))


def _build_batch():
    a, b, f = steps(21, 40, 70), noise(22, 40, 70), flat(40, 70)
    _add("lane_steps_40x70", a, 5, 60, min_total=(100, 61))
    _add("lane_noise_40x70", b, 5, 60, min_total=(100, 61))
    _add("lane_flat_40x70", f, 5, 60, corners=0, survivors=0, n=0)
    _add("lane_plateau_40x70", _dark(flat(40, 70, 200), [(63, 15), (64, 15), (63, 16), (64, 16), (5, 5)]), 5, 60, survivors=2, n=2)
    _add("lane_sparse_40x70", _dark(flat(40, 70, 180), [(9, 9), (30, 20), (66, 36)], 7), 5, 60, survivors=3, n=3)
    BATCH.append(("s1", ["lane_noise_40x70"], 5, 60))
    BATCH.append(("s2", ["lane_steps_40x70", "lane_plateau_40x70"], 5, 60))
    BATCH.append(("s5_flat_between_busy", ["lane_steps_40x70", "lane_flat_40x70", "lane_noise_40x70", "lane_sparse_40x70",
                                           "lane_plateau_40x70"], 5, 60))
    BATCH.append(("s2_n_1", ["lane_noise_40x70", "lane_steps_40x70"], 30, 1))


_build_shapes()
_build_arcs()
_build_border_and_seams()
_build_suppression()
_build_selection()
_build_batch()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
