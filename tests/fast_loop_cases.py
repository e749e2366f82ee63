"""Case tables of the two batch primitives the FAST + BRIEF tracker mode is made of (vo_brief_describe_batch_dev,
vo_match_hamming_batch_dev) and the stream configurations of its loop tests.  Shared by tests/test_pipeline_fast_host.py
(every case keeps the edge it is named for, on the definitions) and the -m gpu tests (the kernels against the definitions,
bit for bit).  The expected values come from tests/brief_reference.py alone."""
import collections

import numpy as np

import brief_reference as ref

SENTINEL = 0xA5             # what the outputs are pre-filled with: a row nobody may write still holds it
PAIR_SENTINEL = -77

# ---- the loop's configurations (tests/test_pipeline_fast_host.py asserts what the GPU tests rely on) ----
LOOP_H, LOOP_W, LOOP_N, LOOP_FRAMES, LOOP_STEPS = 480, 640, 500, 5, 4
LOOP_THRESHOLDS = (20, 170)        # 20: every frame has N corners; 170: every frame fewer, another count per frame and sequence
CONFIG_H, CONFIG_W, CONFIG_N = 1241, 1376, 2000


def loop_streams(S, F=LOOP_FRAMES, H=LOOP_H, W=LOOP_W):
    from vo import synthetic
    return [synthetic.Stream(F, H, W, seed=2023 + 7 * q, start=q) for q in range(S)]


# ---- describe ----
DescribeCase = collections.namedtuple(
    "DescribeCase", "name imgs kp counts N oriented img_stride xy_stride desc_stride props")
D_H, D_W, D_S, D_N = 40, 56, 3, 8
DESCRIBE = []


def _texture(seed, H, W):
    """Random bytes smoothed a little: box sums that differ, gradients in every direction."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H + 2, W + 2)).astype(np.int64)
    b = sum(a[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) // 9
    return b.astype(np.uint8)


def _interior(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(17, D_W - 18, n), rng.uniform(17, D_H - 18, n)], axis=1)


def _dadd(name, kp, counts, oriented, **props):
    imgs = np.stack([_texture(100 + 10 * len(DESCRIBE) + q, D_H, D_W) for q in range(D_S)])
    kp = np.ascontiguousarray(kp, np.float64).reshape(D_S, D_N, 2)
    imgs.flags.writeable = kp.flags.writeable = False
    # strides beyond the blocks' own sizes (and not a multiple of anything the kernels vectorise by)
    DESCRIBE.append(DescribeCase(name, imgs, kp, tuple(int(c) for c in counts), D_N, bool(oriented), D_H * D_W + 37, D_N + 3,
                                 32 * D_N + 40, props))


def _build_describe():
    base = np.stack([_interior(q, D_N) for q in range(D_S)])
    for oriented in (False, True):
        tag = "_oriented" if oriented else ""
        # every row beyond a count is a describable interior keypoint: written, it would not look like the sentinel
        _dadd("counts_0_1_5" + tag, base, (0, 1, 5), oriented, effective=(0, 1, 5))
        _dadd("count_above_n_and_negative" + tag, base, (D_N + 5, -3, D_N), oriented, effective=(D_N, 0, D_N))
        # on the border, beyond it (inside and outside the range [-16, W + 16) of a centre), non-finite
        kp = base.copy()
        kp[0, :6] = [(0, 0), (D_W - 1, D_H - 1), (-0.5, 12.0), (D_W - 0.51, 3.2), (-8.49, 20.0), (D_W + 15.49, D_H + 15.49)]
        kp[1, :5] = [(-16.51, 20.0), (D_W + 15.5, 5.0), (7.0, D_H + 15.5), (-1e300, 3.0), (1e9, 1e9)]
        kp[2, :4] = [(np.nan, 5.0), (5.0, np.inf), (-np.inf, np.nan), (20.0, 20.0)]
        _dadd("border_and_nonfinite" + tag, kp, (6, 5, 4), oriented, effective=(6, 5, 4),
              valid=((True,) * 6, (False,) * 5, (False, False, False, True)))


_build_describe()
DESCRIBE_BY_NAME = {c.name: c for c in DESCRIBE}
DESCRIBE_NAMES = [c.name for c in DESCRIBE]


def describe_effective(case):
    return tuple(min(max(c, 0), case.N) for c in case.counts)


def describe_expected(case):
    """(desc (S, N, 32), bins (S, N)) uint8: the definition's rows below each image's count, SENTINEL at and beyond it."""
    desc = np.full((D_S, case.N, 32), SENTINEL, np.uint8)
    bins = np.full((D_S, case.N), SENTINEL, np.uint8)
    for q, n in enumerate(describe_effective(case)):
        if n:
            d, b = ref.describe(case.imgs[q], case.kp[q, :n], case.oriented)
            desc[q, :n], bins[q, :n] = d, b
    return desc, bins


# ---- matcher ----
MatchCase = collections.namedtuple("MatchCase", "name q t nq nt cap_q cap_t ratio max_dist props")
M_S, M_CAPQ, M_CAPT, M_B = 3, 20, 40, 32
MATCH = []


def with_bits(base, bits):
    out = np.array(base, np.uint8)
    for pos in bits:
        out[pos // 8] ^= np.uint8(1 << (pos % 8))
    return out


def _random_rows(seed):
    """Rows some 128 bits from one another: nothing passes a ratio test unless a case plants it."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=(M_S, M_CAPQ, M_B)).astype(np.uint8),
            rng.integers(0, 256, size=(M_S, M_CAPT, M_B)).astype(np.uint8))


def plant(q, t, z, qi, ta, tb, d1, d2):
    """Sequence z: train row tb = train row ta with d2 - d1 bits flipped, query qi = train row ta with d1 other bits
    flipped: its neighbours are (ta, d1) and (tb, d2) as long as d2 stays well below 100."""
    t[z, tb] = with_bits(t[z, ta], range(128, 128 + d2 - d1))
    q[z, qi] = with_bits(t[z, ta], range(0, d1))


def _madd(name, q, t, nq, nt, ratio=0.8, max_dist=-1, **props):
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    q.flags.writeable = t.flags.writeable = False
    MATCH.append(MatchCase(name, q, t, tuple(nq), tuple(nt), M_CAPQ, M_CAPT, float(ratio), int(max_dist), props))


def _build_match():
    # counts that leave a partial group of eight queries, train counts across the 32 slices
    for name, nq, nt, seed in (("partial_query_groups", (0, 9, 20), (40, 33, 40), 1), ("train_slices", (9, 20, 20), (1, 0, 33), 2),
                               ("counts_beyond_capacity_and_negative", (M_CAPQ + 7, -2, 17), (M_CAPT + 9, 40, -1), 3)):
        q, t = _random_rows(seed)
        for z in range(M_S):
            for k, qi in enumerate((0, 3, 8, 12, 19)):
                plant(q, t, z, qi, 2 * k, 2 * k + 1, 3 + k, 40 + k)
            plant(q, t, z, 5, 32, 38, 2, 30)               # (train rows of the second round of slices)
        _madd(name, q, t, nq, nt)
    # rows beyond a count that equal a query: a train row read beyond nt is a neighbour at distance 0 and replaces the
    # pair's train index; a query read beyond nq is one pair more, with a train row nobody else asks for
    q, t = _random_rows(4)
    nq, nt = (9, 12, 20), (33, 20, 10)
    for z in range(M_S):
        plant(q, t, z, 1, 0, 1, 5, 40)
        plant(q, t, z, 6, 4, 5, 7, 50)
        if nq[z] < M_CAPQ:
            plant(q, t, z, nq[z], 8, 9, 1, 30)             # the first query beyond the count
        t[z, nt[z]] = q[z, 1]                              # the first train row beyond the count
        t[z, M_CAPT - 1] = q[z, 6]                         # the last row of the block
    _madd("rows_beyond_counts_equal_a_query", q, t, nq, nt, beyond=True)
    # one train index contested in two sequences: in sequence 0 by queries 2 and 5 (2 wins), in sequence 1 by query 3
    # alone, in sequence 2 by queries 4 and 1 (1 wins) -- under one shared owner table query 2 or 1 would own all three
    q, t = _random_rows(5)
    for z, (first, second) in enumerate(((2, 5), (3, None), (1, 4))):
        plant(q, t, z, first, 7, 11, 4, 40)
        if second is not None:
            q[z, second] = with_bits(t[z, 7], range(60, 63))          # (nearer than the winner: the order decides, not d1)
    _madd("train_index_contested_in_two_sequences", q, t, (20, 20, 20), (40, 40, 40), contested=(7, (2, 3, 1)))
    # exact ties: ratio 0.5 with (d1, d2) = (4, 8) fails, (3, 8) passes; max_dist 10 with d1 = 10 passes, 11 fails
    q, t = _random_rows(6)
    for z in range(M_S):
        plant(q, t, z, 0, 0, 1, 4, 8)
        plant(q, t, z, 1, 2, 3, 3, 8)
        plant(q, t, z, 2, 4, 5, 10, 30)
        plant(q, t, z, 3, 6, 7, 11, 30)
    _madd("ties_at_ratio_and_max_dist", q, t, (20, 9, 4), (40, 33, 8), ratio=0.5, max_dist=10, keeps=(1, 2), drops=(0, 3))
    # no distance limit: pairs far above any limit a default would set
    q, t = _random_rows(7)
    for z in range(M_S):
        plant(q, t, z, 0, 0, 1, 70, 99)
        plant(q, t, z, 9, 2, 3, 66, 95)
    _madd("no_distance_limit", q, t, (20, 10, 1), (40, 40, 40), ratio=0.8, max_dist=-1, far=True)


_build_match()
MATCH_BY_NAME = {c.name: c for c in MATCH}
MATCH_NAMES = [c.name for c in MATCH]


def match_effective(case):
    return (tuple(min(max(n, 0), case.cap_q) for n in case.nq), tuple(min(max(n, 0), case.cap_t) for n in case.nt))


def match_expected(case, use_counts=True):
    """Per sequence the (n, 2) int64 pair list of the definition on the rows below the counts (use_counts = False: on
    every row of the blocks, what a kernel that ignored the counts would see)."""
    enq, ent = match_effective(case)
    out = []
    for z in range(M_S):
        nq, nt = (enq[z], ent[z]) if use_counts else (case.cap_q, case.cap_t)
        pairs = ref.match(case.q[z, :nq], case.t[z, :nt], case.ratio, case.max_dist) if nq and nt else []
        out.append(np.asarray(pairs, np.int64).reshape(-1, 2))
    return out
