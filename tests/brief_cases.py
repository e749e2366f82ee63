"""The case tables of the BRIEF-256 / Hamming tests.  tests/test_gpu_brief.py runs every case on the device against
tests/brief_reference.py; tests/test_brief_host.py checks on the CPU that the reference agrees with a second, per-pixel
statement on every case and that every case still has the edge its PROPS promise.

DESCRIBE: (name, img (H, W) uint8, kp (N, 2) float64); every case is run with oriented 0 and 1.  DESCRIBE_PROPS[name]:
  valid       the exact mask of keypoints whose centre is valid (the others: all-zero descriptor, bin 0)
  zero_bits   every descriptor is all zero (both oriented values)
  bin         the bin every keypoint must have when oriented
  bin_shift   (i, j, allowed): bin[j] - bin[i] mod 30 lies in `allowed`
  ties        at least this share of the unoriented tests of valid keypoints are exact ties S(a) == S(b)
  s_max       the largest box sum the case reaches
  centres     the exact integer centres of the valid keypoints, in order
MATCH: (name, q (nq, B) uint8, t (nt, B) uint8, ratio, max_dist).  MATCH_PROPS[name]:
  ties        groups of identical train rows that are the exact nearest of some query: its two neighbours are the
              group's two lowest indices at one distance
  equidistant the tied rows differ, they are only equally far
  first       (best, dist) of query 0
  n_pairs / pairs   the exact pair count / list
  seam        the pair list has queries on both sides of index 1024 and a train row two queries ask for across it
All inputs come from seeded generators."""
import collections

import numpy as np

import brief_reference as ref

DescribeCase = collections.namedtuple("DescribeCase", "name img kp")
MatchCase = collections.namedtuple("MatchCase", "name q t ratio max_dist")
DESCRIBE, DESCRIBE_PROPS = [], {}
MATCH, MATCH_PROPS = [], {}


def texture(seed, H, W):
    """Random bytes smoothed a little: box sums that differ, gradients in every direction."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H + 2, W + 2)).astype(np.int64)
    sm = (a[:-2, :-2] + a[:-2, 2:] + a[2:, :-2] + a[2:, 2:] + 2 * (a[1:-1, :-2] + a[1:-1, 2:] + a[:-2, 1:-1] + a[2:, 1:-1])
          + 4 * a[1:-1, 1:-1]) // 16
    big = np.kron(rng.integers(0, 256, size=(H // 8 + 1, W // 8 + 1)), np.ones((8, 8), np.int64))[:H, :W]
    return ((sm + big) // 2).astype(np.uint8)


def _dadd(name, img, kp, **props):
    assert name not in DESCRIBE_PROPS, name
    img = np.ascontiguousarray(img, np.uint8)
    kp = np.ascontiguousarray(np.asarray(kp, np.float64).reshape(-1, 2))
    img.flags.writeable = kp.flags.writeable = False
    DESCRIBE.append(DescribeCase(name, img, kp))
    DESCRIBE_PROPS[name] = props


def _build_describe():
    H, W = 40, 48
    img = texture(1, H, W)
    _dadd("corners", img, [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)], valid=[True] * 4)
    H, W = 64, 80
    img = texture(2, H, W)
    kp = []
    for d in (0, 1, 15, 16, 17):
        kp += [(d, H // 2), (W - 1 - d, H // 2), (W // 2, d), (W // 2, H - 1 - d), (d, d), (W - 1 - d, H - 1 - d)]
    _dadd("borders_and_inside", img, kp, valid=[True] * len(kp))
    kp = []
    for d in (1, 8, 15, 16):
        kp += [(-d, 20), (W - 1 + d, 20), (30, -d), (30, H - 1 + d), (-d, -d), (W - 1 + d, H - 1 + d)]
    _dadd("outside_by_up_to_16", img, kp, valid=[True] * len(kp))
    kp = [(-17, 20), (W + 16, 20), (30, -17), (30, H + 16), (-17, -17), (W + 16, H + 16), (-1000, 5), (5, 1e6), (1e300, 5),
          (5, -1e300), (3e9, 3e9), (-3e9, 7), (20, 20)]
    _dadd("beyond_the_window", img, kp, valid=[False] * 12 + [True])
    half = [(10.5, 20.5), (-0.5, 20), (-1.5, 20), (0.49999999999999994, 20), (-16.5, 20), (-17.5, 20), (W + 15.5, 20),
            (W + 15.499, 20), (20, -0.5), (20, -16.5), (20, -17.5), (20, H + 15.5), (10.49999, 20.49999), (-0.50000001, 20)]
    _dadd("halves", img, half,
          valid=[True, True, True, True, True, False, False, True, True, True, False, False, True, True],
          centres=[(11, 21), (0, 20), (-1, 20), (1, 20), (-16, 20), (W + 15, 20), (20, 0), (20, -16), (10, 20), (-1, 20)])
    nan, inf = float("nan"), float("inf")
    _dadd("non_finite", img, [(nan, 20), (20, nan), (nan, nan), (inf, 20), (20, inf), (-inf, 20), (20, -inf), (inf, -inf), (20, 20)],
          valid=[False] * 8 + [True])
    interior = [(x, y) for x in (16, 23.4, 31) for y in (16, 24.6, 31)]
    _dadd("flat", np.full((48, 48), 77, np.uint8), interior, valid=[True] * 9, zero_bits=True, bin=[0] * 9)
    _dadd("all_zero", np.zeros((40, 48), np.uint8), [(0, 0), (24, 20), (47, 39), (-16, -16)], valid=[True] * 4, zero_bits=True,
          bin=[0] * 4)
    sat = [(x, y) for x in (0, 5, 24, 47) for y in (0, 20, 39)]
    _dadd("saturated", np.full((40, 48), 255, np.uint8), sat, valid=[True] * len(sat), s_max=6375)
    rng = np.random.default_rng(3)
    two = np.kron(rng.integers(0, 2, size=(8, 10)) * 200, np.ones((8, 8), np.int64))
    kp = np.stack([rng.uniform(0, 80, size=24), rng.uniform(0, 64, size=24)], axis=1)
    _dadd("two_valued_ties", two, kp, valid=[True] * 24, ties=0.2)
    # ---- orientation ----
    _, C, Sn = ref.tables()
    y, x = np.mgrid[0:65, 0:65] - 32
    for k in range(30):
        ramp = 128 + np.floor((x * int(C[k]) + y * int(Sn[k])) * 2 / 16384.0 + 0.5).astype(np.int64)
        assert ramp.min() >= 0 and ramp.max() <= 255
        _dadd("ramp_bin_%d" % k, ramp, [(32, 32), (30.2, 33.7)], valid=[True] * 2, bin=[k] * 2)
    # a ramp along +y has m10 = 0 exactly (the disc and the image are symmetric in x): bins 7 and 8 (84 and 96 degrees)
    # score m01 * 16294 both, the lower wins; along -y bins 22 and 23 tie
    assert Sn[7] == Sn[8] and Sn[22] == Sn[23] and C[7] == -C[8]
    _dadd("ramp_between_bins_7_8", (128 + 2 * y), [(32, 32), (29, 35)], valid=[True] * 2, bin=[7, 7])
    _dadd("ramp_between_bins_22_23", (128 - 2 * y), [(32, 32), (29, 35)], valid=[True] * 2, bin=[22, 22])
    # an image and its quarter turn (clockwise on the screen = +90 degrees with y down): a pixel at (dx, dy) from the
    # centre moves to (-dy, dx), so (m10, m01) -> (-m01, m10) exactly.  With C[k + 15] = -C[k], Sn[k + 15] = -Sn[k],
    # C[15 - k] = -C[k], Sn[15 - k] = Sn[k] the 30 directions are symmetric under half turns and reflections but a
    # quarter turn is 7.5 bins: the bin moves by 7 or 8.
    assert all(C[(k + 15) % 30] == -C[k] and Sn[(k + 15) % 30] == -Sn[k] for k in range(30))
    assert all(C[(15 - k) % 30] == -C[k] and Sn[(15 - k) % 30] == Sn[k] for k in range(30))
    A = texture(4, 65, 65)
    B = np.rot90(A, -1)
    _dadd("quarter_turn", np.concatenate([A, B], axis=1), [(32, 32), (65 + 32, 32)], valid=[True] * 2, bin_shift=(0, 1, (7, 8)))
    # ---- workgroup and launch remainders ----
    big = texture(5, 96, 128)
    for n in (1, 3, 4, 5, 63, 64, 65, 257):
        rng = np.random.default_rng(100 + n)
        kp = np.stack([rng.uniform(-20, 148, size=n), rng.uniform(-20, 116, size=n)], axis=1)
        _dadd("n_%d" % n, big, kp)


def _madd(name, q, t, ratio=0.8, max_dist=-1, **props):
    assert name not in MATCH_PROPS, name
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    q.flags.writeable = t.flags.writeable = False
    MATCH.append(MatchCase(name, q, t, float(ratio), int(max_dist)))
    MATCH_PROPS[name] = props


def flip(rows, rng, n_bits):
    """Copies of the rows with n_bits random (not necessarily distinct) bits flipped."""
    out = rows.copy()
    B = rows.shape[1]
    for r in range(len(out)):
        for pos in rng.integers(0, 8 * B, size=n_bits):
            out[r, pos // 8] ^= np.uint8(1 << (pos % 8))
    return out


def with_bits(base, bits):
    out = base.copy()
    for pos in bits:
        out[pos // 8] ^= np.uint8(1 << (pos % 8))
    return out


# identical train rows (the kernel deals row j to slice j % 32, eight slices to a wave, four waves to a workgroup): in
# neighbouring slices (3, 4), on both sides of a wave (7, 8: slices 0..7 are wave 0), in the last and the first slice
# (31, 32), twice in one slice (5, 37; 64, 288, 512: the merge inside a thread), across a multiple of the workgroup's
# 256 threads (255, 256), and a pair whose higher row belongs to the lower slice (200 is slice 8, 289 slice 1:
# a merge that visits the slices in order must still put row 200 first)
GROUPS = ((3, 4), (7, 8), (31, 32), (5, 37), (255, 256), (64, 288, 512), (200, 289))
ROW_BYTES = (4, 32, 64)
NQ = (1, 63, 64, 65, 130)
NT = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)


def grid_rows(seed, nq, nt, B):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=(nt, B)).astype(np.uint8)
    used = []
    if B >= 32:                                            # (4-byte rows tie all the time anyway)
        for g in GROUPS:
            if g[-1] < nt:
                t[list(g[1:])] = t[g[0]]
                used.append(g)
    if nt == 0:
        return rng.integers(0, 256, size=(nq, B)).astype(np.uint8), t, []
    q = flip(t[rng.integers(0, nt, size=nq)], rng, max(1, B // 4))
    planted = []
    for i, g in enumerate(used):                           # queries 1, 2, ... : exact copies of the groups' rows
        if 1 + i < nq - 1:
            q[1 + i] = t[g[0]]
            planted.append(g)
    if nq > 1:
        q[nq - 1] = q[0]                                   # the last query wants what query 0 wants
    return q, t, planted


def _build_match():
    for B in ROW_BYTES:
        for nq in NQ:
            for nt in NT:
                q, t, planted = grid_rows(1000 * B + 10 * nt + nq, nq, nt, B)
                _madd("grid_B%d_nq%d_nt%d" % (B, nq, nt), q, t, 0.8, -1, ties=planted)
    for B in ROW_BYTES:
        rng = np.random.default_rng(B)
        base = rng.integers(0, 256, size=B).astype(np.uint8)
        # equidistant but different: every train row one (different) bit away; rows 0 and 1 win at distance 1
        t = np.stack([with_bits(base, [(7 * j) % (8 * B)]) for j in range(20)])
        _madd("equidistant_B%d" % B, base[None], t, 0.8, -1, ties=[tuple(range(20))], equidistant=1, first=((0, 1), (1, 1)), n_pairs=0)
        zeros, ones = np.zeros(B, np.uint8), np.full(B, 255, np.uint8)
        _madd("zeros_and_ones_B%d" % B, np.stack([zeros, ones]), np.stack([ones, zeros]), 0.8, -1,
              first=((1, 0), (0, 8 * B)), pairs=[(0, 1), (1, 0)])
        # strict ratio: d1 = 2, d2 = 4 at ratio 0.5 gives no pair; d1 = 1 does
        t = np.stack([with_bits(base, [0, 9]), with_bits(base, [1, 2, 3, 4])])
        _madd("ratio_on_boundary_B%d" % B, base[None], t, 0.5, -1, first=((0, 1), (2, 4)), n_pairs=0)
        t = np.stack([with_bits(base, [0]), with_bits(base, [1, 2, 3, 4])])
        _madd("ratio_inside_B%d" % B, base[None], t, 0.5, -1, first=((0, 1), (1, 4)), n_pairs=1)
        # the distance limit: d1 = 5, d2 = 20
        t = np.stack([with_bits(base, range(10, 30)), with_bits(base, [0, 1, 2, 3, 4])])
        _madd("max_dist_equal_B%d" % B, base[None], t, 0.8, 5, first=((1, 0), (5, 20)), n_pairs=1)
        _madd("max_dist_below_B%d" % B, base[None], t, 0.8, 4, first=((1, 0), (5, 20)), n_pairs=0)
        _madd("second_absent_B%d" % B, base[None], t[:1], 0.8, -1, first=((0, -1), (20, 0)), n_pairs=0)
    # 1100 queries: the ordered compaction's second round; queries 1000 and 1060 both want train row 500
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, size=(1100, 32)).astype(np.uint8)
    q = flip(t[np.concatenate([rng.integers(0, 1000, size=1000), 1000 + np.arange(100)])], rng, 6)
    q[1000] = flip(t[500:501], rng, 3)[0]
    q[1060] = t[500]
    nearest = ref.knn2(q, t)[0][:, 0]
    for i in np.nonzero(nearest == 500)[0]:                # nobody else may want row 500
        if i in (1000, 1060):
            continue
        q[i] = flip(t[501:502], rng, 6)[0]
    _madd("queries_1100_seam", q, t, 0.8, 64, seam=(1000, 1060, 500))


_build_describe()
_build_match()
DESCRIBE_BY_NAME = {c.name: c for c in DESCRIBE}
MATCH_BY_NAME = {c.name: c for c in MATCH}
DESCRIBE_NAMES = [c.name for c in DESCRIBE]
MATCH_NAMES = [c.name for c in MATCH]


# ---- match quality on the reference's KITTI frames 0 and 2 ----
def kitti_pair():
    """(image0, image2, K, F): the frames, the camera and the ground-truth fundamental matrix x2^T F x1 = 0 from rows 0
    and 2 of poses/05.txt (camera-to-world)."""
    import os
    G = os.path.join(os.path.dirname(__file__), "golden")
    g = dict(np.load(os.path.join(G, "kitti_harris.npz")))
    g.update(np.load(os.path.join(G, "kitti_frames.npz")))
    K = g["calib_P0"][:, :3]

    def pose(k):
        M = np.eye(4)
        M[:3] = g["poses05_head"][k]
        return M
    rel = np.linalg.inv(pose(0)) @ pose(2)                 # X0 = R X2 + t
    R2, t2 = rel[:3, :3].T, -rel[:3, :3].T @ rel[:3, 3]    # X2 = R2 X0 + t2
    tx = np.array([[0, -t2[2], t2[1]], [t2[2], 0, -t2[0]], [-t2[1], t2[0], 0]])
    Ki = np.linalg.inv(K)
    return g["image0"], g["image2"], K, Ki.T @ tx @ R2 @ Ki


def sampson_px(F, p1, p2):
    """The Sampson distance in pixels of the correspondences p1 -> p2 ((n, 2) each) to x2^T F x1 = 0."""
    x1, x2 = np.c_[p1, np.ones(len(p1))], np.c_[p2, np.ones(len(p2))]
    Fx1, Ftx2 = x1 @ F.T, x2 @ F
    num = np.sum(x2 * Fx1, axis=1) ** 2
    return np.sqrt(num / (Fx1[:, 0] ** 2 + Fx1[:, 1] ** 2 + Ftx2[:, 0] ** 2 + Ftx2[:, 1] ** 2))
