"""The case table of the descriptor matcher's tests: tests/test_gpu_matcher.py runs every case on the device (all three
kernels of csrc/match.hip: matrix cores, packed byte dot product, float), tests/test_matcher_host.py checks on the CPU that the
oracle (oracle/csrc/match.c) agrees with an independent NumPy statement on every case and that every case still has the
edge its name promises.

CASES: (name, q, t, ratio, expected_path) with q (nq, D) and t (nt, D) float32; expected_path is the kernel that must
produce the result: 0 float, 1 byte dot, 2 matrix cores.  PROPS[name] holds what the case claims about itself:
  ties     groups of identical train rows that each are the exact nearest of some query: that query's two neighbours are
           the group's two lowest indices at one distance (a name with "tie" has at least one)
  n_pairs  the exact number of pairs, where the case is built for it (a name with "nopair" has none)
  seam     the pair list has queries on both sides of index 1024 (the ordered compaction's second block)
  equidistant  the tied train rows are not identical, only equally far from their query
All inputs come from seeded generators; nothing is larger than 1100 x 1100 x 384."""
import collections
import functools

import numpy as np

from oracle import native

FLOAT, BYTE_DOT, MFMA = 0, 1, 2
Case = collections.namedtuple("Case", "name q t ratio path")
CASES = []
PROPS = {}

# identical train rows: in neighbouring lanes / the two lane halves (3, 4), across a tile of 32 (31, 32), across the four
# waves' 128 rows -- with 257 or 288 train rows also the edge between two splits -- (127, 128), three of a kind, and a pair
# whose higher row belongs to the lower thread of the byte-dot and float kernels (300 = 256 + 44 against 200): a merge that
# visits the threads in order must still put row 200 first
THREADS = ((3, 4), (31, 32), (127, 128), (5, 130, 250), (200, 300))
# train rows j and j + 256 belong to one thread of the byte-dot and float kernels
SAME_THREAD = ((7, 263), (0, 256, 512))


def same_thread(nt):
    return SAME_THREAD if nt > 512 else ((0, 256),)

MFMA_NT = (1, 2, 31, 32, 33, 127, 128, 129, 256, 257, 288, 512)
MFMA_NQ = (1, 31, 32, 33, 70)
DOT_D = (1, 3, 4, 5, 16, 127, 129, 360, 362)
DOT_NQ = (1, 7, 8, 9, 20)
DOT_NT = (2, 255, 256, 257, 513)


def _add(name, q, t, ratio, path, **props):
    assert name not in PROPS, name
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    q.flags.writeable = t.flags.writeable = False
    if props.get("ties"):
        assert "tie" in name, name
    if props.get("n_pairs") == 0 or t.shape[0] < 2:
        assert "nopair" in name, name
    CASES.append(Case(name, q, t, float(ratio), path))
    PROPS[name] = props


def _plant(t, nq, q, groups, bump):
    """Copies the first row of every group that fits over its other rows, and gives queries 1, 2, ... the planted rows:
    an exact copy (distance 0 to the whole group) and, while queries last, one changed by `bump` (one non-zero distance
    to the whole group).  The last query is left alone.  Returns the groups that received their exact copy."""
    nt = t.shape[0]
    fit = [g for g in groups if g[-1] < nt]
    for g in fit:
        t[list(g[1:])] = t[g[0]]
    k, used = 1, []
    for g in fit:
        if k >= nq - 1:
            break
        q[k] = t[g[0]]
        used.append(g)
        k += 1
        if k < nq - 1:
            q[k] = bump(t[g[0]])
            k += 1
    return used, k


def byte_rows(seed, nq, nt, D, groups=()):
    """Whole numbers in 0..255.  Query 0 is a noisy copy of train row 1 (no group holds it) and passes the ratio test when
    there are two train rows; the last query repeats it and loses the row to it; in between the planted queries, noisy
    copies of random train rows and, every seventh, an unrelated one.  Below D = 16 random rows collide, so nothing is
    planted and train row 1 is set apart instead: all zeros among rows of 100..255."""
    rng = np.random.default_rng(seed)
    small = D < 16
    t = rng.integers(100 if small else 0, 256, size=(nt, D)).astype(np.float64)
    if small and nt > 1:
        t[1] = 0
    src = rng.integers(0, nt, size=nq)
    q = np.clip(t[src] + rng.integers(-12, 13, size=(nq, D)), 0, 255)
    if nt > 1:
        q[0] = rng.integers(0, 4, size=D) if small else np.clip(t[1] + rng.integers(-5, 6, size=D), 0, 255)

    def bump(row):
        out = row.copy()
        out[:3] += np.where(row[:3] < 128, 1, -1)
        return out
    used, k = _plant(t, nq, q, () if small else groups, bump)
    for i in range(k, nq - 1):
        if i % 7 == 6:
            q[i] = rng.integers(0, 256, size=D)
    if nq > 1:
        q[nq - 1] = q[0]
    return q, t, used


def float_rows(seed, nq, nt, D, groups=(), scale=1.0):
    rng = np.random.default_rng(seed)
    t = (rng.normal(size=(nt, D)) * scale).astype(np.float32)
    src = rng.integers(0, nt, size=nq)
    q = (t[src] + rng.normal(scale=0.05 * scale, size=(nq, D))).astype(np.float32)
    if nt > 1:
        q[0] = t[1] + np.float32(0.01 * scale)

    def bump(row):
        out = row.copy()
        out[0] += np.float32(0.25 * scale)
        return out
    used, k = _plant(t, nq, q, groups, bump)
    if nq > 1:
        q[nq - 1] = q[0]
    return q, t, used


def _label(used, nt):
    return ("_tie" if used else "") + ("_nopair" if nt < 2 else "")


def _build():
    # ---- matrix cores: D = 128 and D = 361 (padded to 384), 1 / 2 / 4 splits of the train set ----
    for D in (128, 361):
        for nt in MFMA_NT:
            for nq in MFMA_NQ:
                q, t, used = byte_rows(1000 * D + 10 * nt + nq, nq, nt, D, THREADS)
                _add("mfma_D%d_nq%d_nt%d%s" % (D, nq, nt, _label(used, nt)), q, t, 0.8 if D == 128 else 0.85, MFMA, ties=used)
    # the suite's earlier byte shapes: three for the matrix cores, one (a single train row) for the byte dot product
    for nq, nt, D, ratio in ((300, 280, 361, 0.85), (500, 700, 128, 0.8), (5, 3, 128, 0.8), (40, 1, 16, 0.9)):
        rng = np.random.default_rng(nq + D)
        t = rng.integers(0, 256, size=(nt, D)).astype(np.float32)
        q = np.clip(t[rng.integers(0, nt, size=nq)] + rng.integers(-12, 13, size=(nq, D)), 0, 255).astype(np.float32)
        q[::7] = rng.integers(0, 256, size=q[::7].shape)
        q[1] = q[0]
        if D == 16:
            _add("dot_earlier_40x1x16_nopair", q, t, ratio, BYTE_DOT, n_pairs=0)
        else:
            _add("mfma_earlier_%dx%dx%d" % (nq, nt, D), q, t, ratio, MFMA)
    # the largest distance: an all-0 row against an all-255 row
    for D in (128, 361):
        t = np.stack([np.zeros(D), np.full(D, 255.0)])
        _add("mfma_D%d_extremes" % D, t[::-1], t, 0.8, MFMA, n_pairs=2, d2_max=D * 255.0 * 255.0)
    # D = 361: rows equal but for the last real element; train row j holds 6 j there (the last one 255)
    t = np.tile(np.random.default_rng(361).integers(0, 256, size=361).astype(np.float64), (40, 1))
    t[:, 360] = 6 * np.arange(40)
    t[39, 360] = 255
    q = np.tile(t[0], (33, 1))
    q[:, 360] = [254] + [6 * j + 3 for j in range(31)] + [1]          # next to row 39; midway between rows j, j + 1; next to row 0
    _add("mfma_D361_last_element_tie", q, t, 0.85, MFMA, ties=[(j, j + 1) for j in range(31)], n_pairs=2, equidistant=1)

    # ---- packed byte dot product: every other length ----
    shapes = [(nq, nt, DOT_D[(5 * a + b) % len(DOT_D)]) for a, nq in enumerate(DOT_NQ) for b, nt in enumerate(DOT_NT)]
    shapes += [(nq, nt, D) for D in DOT_D for nq, nt in ((20, 513), (9, 257))]
    for nq, nt, D in sorted(set(shapes)):
        q, t, used = byte_rows(7000 * D + 10 * nt + nq, nq, nt, D, THREADS + same_thread(nt))
        _add("dot_D%d_nq%d_nt%d%s" % (D, nq, nt, _label(used, nt)), q, t, 0.8, BYTE_DOT, ties=used)
    q, t, used = byte_rows(77, 20, 513, 129, SAME_THREAD + THREADS)       # (the one-thread groups get their queries first)
    _add("dot_D129_same_thread_tie", q, t, 0.8, BYTE_DOT, ties=used)

    # ---- float ----
    for i, nt in enumerate(MFMA_NT + (513,)):
        nq = MFMA_NQ[i % len(MFMA_NQ)] if nt != 513 else 20
        q, t, used = float_rows(500 + nt, nq, nt, 32, THREADS + same_thread(nt))
        _add("float_D32_nq%d_nt%d%s" % (nq, nt, _label(used, nt)), q, t, 0.8, FLOAT, ties=used)
    q, t, used = float_rows(78, 20, 513, 32, SAME_THREAD + THREADS)
    _add("float_D32_same_thread_tie", q, t, 0.8, FLOAT, ties=used)
    rng = np.random.default_rng(3)                                        # the suite's earlier float shape
    t = rng.normal(size=(150, 32)).astype(np.float32)
    _add("float_earlier_120x150x32", (t[rng.integers(0, 150, size=120)] + rng.normal(scale=0.05, size=(120, 32))), t, 0.8, FLOAT)
    # byte data with exactly one value that is no byte: the byte kernel's result must be thrown away
    for D in (128, 361):
        for v in (0.5, 256.0, -1.0, 255.5):
            for where in ("q_first", "t_last"):
                q, t, used = byte_rows(int(D + 8 * v), 33, 320, D, THREADS)
                if where == "q_first":
                    q[0, 0] = v
                else:
                    t[-1, -1] = v
                _add("float_spoiled_D%d_%s_%s_tie" % (D, where, v), q, t, 0.8, FLOAT, ties=used, spoiled=1)
    # ... in a length the byte-dot kernel would take, and byte values in a length whose distances pass 2^31
    q, t, used = byte_rows(91, 9, 257, 16, THREADS)
    q[8, 15] = 0.5
    _add("float_spoiled_D16_q_last_tie", q, t, 0.8, FLOAT, ties=used, spoiled=1)
    rng = np.random.default_rng(92)
    t = rng.integers(0, 256, size=(3, 33100))
    _add("float_bytes_too_long", np.clip(t[[1, 2]] + rng.integers(-3, 4, size=(2, 33100)), 0, 255), t, 0.8, FLOAT)
    # ... and -0.0, which is a byte: both byte kernels keep their result
    for D, path, name in ((128, MFMA, "mfma"), (16, BYTE_DOT, "dot")):
        q, t, used = byte_rows(93 + D, 9, 40, D, THREADS)
        q, t = q.astype(np.float32), t.astype(np.float32)
        q[0, 0] = t[0, 0] = 0.0
        q[q == 0], t[t == 0] = -0.0, -0.0
        _add("%s_D%d_negative_zero_tie" % (name, D), q, t, 0.8, path, ties=used, negative_zero=1)
    for scale, label in ((1e18, "1e18"), (1e-18, "1e-18")):
        q, t, used = float_rows(94, 33, 320, 8, THREADS, scale=scale)
        _add("float_D8_scale_%s_tie" % label, q, t, 0.8, FLOAT, ties=used)
    q, t, used = float_rows(95, 33, 300, 8, THREADS[:4])
    t = t.copy()
    t[::2] *= np.float32(1e18)
    t[1::2] *= np.float32(1e-18)
    for g in THREADS[:4]:
        t[list(g[1:])] = t[g[0]]
    q = q.copy()
    q[0] = t[1] * np.float32(1.5)
    q[1:9:2] = t[[g[0] for g in THREADS[:4]]]
    q[2:9:2] = t[[g[0] for g in THREADS[:4]]] * np.float32(1.25)
    q[9:32] = t[np.arange(9, 32) * 7] * np.float32(0.75)
    q[32] = q[0]
    _add("float_D8_scales_mixed_tie", q, t, 0.8, FLOAT, ties=list(THREADS[:4]))

    # ---- the ratio test's boundary: float32(sqrt(d0)) < ratio * float32(sqrt(d1)), strictly ----
    for D, path, name, unit, shift in ((16, BYTE_DOT, "dot", 1.0, 0.0), (128, MFMA, "mfma", 1.0, 0.0), (16, FLOAT, "float", 0.5, 0.25)):
        base = np.random.default_rng(96 + D).integers(10, 200, size=D).astype(np.float64)

        def rows(*offsets):
            out = np.tile(base, (len(offsets), 1))
            for r, off in enumerate(offsets):
                out[r, :len(off)] += np.array(off, np.float64)
            return out * unit + shift
        u2 = unit * unit
        # d^2 = 4 and 16: 2 == 0.5 * 4, rejected; 4 and 17: kept; equal distances at ratio 1: rejected
        _add("%s_ratio_half_on_boundary_nopair" % name, rows(()), rows((2,), (0, 4)), 0.5, path, n_pairs=0, d2=(4 * u2, 16 * u2))
        _add("%s_ratio_half_inside" % name, rows(()), rows((2,), (0, 4, 1)), 0.5, path, n_pairs=1, d2=(4 * u2, 17 * u2))
        _add("%s_ratio_one_equal_tie_nopair" % name, rows(()), rows((3,), (0, 3)), 1.0, path, n_pairs=0, d2=(9 * u2, 9 * u2),
             ties=[(0, 1)], equidistant=1)
        _add("%s_ratio_one_inside" % name, rows(()), rows((3,), (0, 3, 1)), 1.0, path, n_pairs=1, d2=(9 * u2, 10 * u2))
        _add("%s_second_absent_nopair" % name, rows((), (1,)), rows((2,)), 0.8, path, n_pairs=0, d2=(4 * u2, 0.0))

    # ---- uniqueness: the lowest query that passes the ratio test with a train row takes it ----
    for D, path, name in ((16, BYTE_DOT, "dot"), (128, MFMA, "mfma"), (16, FLOAT, "float")):
        rng = np.random.default_rng(97 + D)
        t = rng.integers(0, 256, size=(40, D)).astype(np.float64)
        q = np.clip(t[[9, 9, 9, 4, 9, 4, 20]] + rng.integers(-3, 4, size=(7, D)), 0, 255)
        if path == FLOAT:
            q, t = q + 0.5, t + 0.25
        _add("%s_contested_train_rows" % name, q, t, 0.8, path, n_pairs=3, pairs=[(0, 9), (3, 4), (6, 20)])
    # ... and 1100 queries: the ordered compaction's second block of 1024, pairs kept on both sides of the seam
    for D, nt, path, name in ((128, 1100, MFMA, "mfma"), (361, 1100, MFMA, "mfma"), (20, 600, BYTE_DOT, "dot"), (8, 300, FLOAT, "float")):
        rng = np.random.default_rng(98 + D)
        # (the last 100 queries copy train rows that none of the first 1000 copies)
        src = np.concatenate([rng.integers(0, nt - 100, size=1000), nt - 100 + np.arange(100)])
        if path == FLOAT:
            t = rng.normal(size=(nt, D))
            q = t[src] + rng.normal(scale=0.02, size=(1100, D))
        else:
            t = rng.integers(0, 256, size=(nt, D)).astype(np.float64)
            q = np.clip(t[src] + rng.integers(-6, 7, size=(1100, D)), 0, 255)
        _add("%s_D%d_1100_queries_seam" % (name, D), q, t, 0.8, path, seam=1)


_build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(pairs, best, d2) of oracle/csrc/match.c for a case: computed once, shared, read-only."""
    c = BY_NAME[name]
    out = native.match_knn2_ratio(c.q, c.t, c.ratio)
    for a in out:
        a.flags.writeable = False
    return out


def is_byte_data(c):
    """Every value a whole number in 0..255 (what the byte kernels can hold; -0.0 is one)."""
    return all(bool(np.all((a >= 0) & (a <= 255) & (a == np.floor(a)))) for a in (c.q, c.t))


# ---- the frame pipeline's batch form (vo_knn2_u8_batch_dev / vo_match_u8_batch_dev) ----
BATCH_CAP_Q, BATCH_CAP_T, BATCH_S = 1100, 544, 3
BATCH_COUNTS = ((1100, 544), (33, 257), (70, 1))          # (queries, train rows) of the three sequences
BATCH_EMPTY = ((0, 40), (40, 0), (33, 257))               # the second launch on the same context
BATCH_RATIO = {128: 0.8, 384: 0.85}


def batch_inputs(row_bytes):
    """(q, t): uint8 arrays (S, rows, row_bytes) with rows = the capacity + 3 (so the strides exceed capacity x row_bytes).
    Train rows hold planted ties; every query is a noisy copy of a train row.  Rows past any count the tests use are filled
    by batch_blocks with copies of the queries."""
    rng = np.random.default_rng(row_bytes)
    q = np.zeros((BATCH_S, BATCH_CAP_Q + 3, row_bytes), np.uint8)
    t = rng.integers(0, 256, size=(BATCH_S, BATCH_CAP_T + 3, row_bytes)).astype(np.uint8)
    for z in range(BATCH_S):
        for g in THREADS + ((256, 310),):
            t[z, list(g[1:])] = t[z, g[0]]
        src = rng.integers(0, BATCH_CAP_T, size=q.shape[1])
        src[:8] = (0, 3, 31, 127, 5, 256, 1, 2)
        q[z] = np.clip(t[z, src].astype(np.int64) + rng.integers(-6, 7, size=q[z].shape), 0, 255)
        q[z, 1:6] = t[z, [3, 31, 127, 5, 256]]
    return q, t


def batch_blocks(q, t, counts):
    """The arrays as the device sees them for `counts`: sequence z's rows past its counts are exact copies of its first
    queries -- a kernel that reads past a count finds neighbours at distance 0 there (train side) or writes lists nobody
    asked for (query side)."""
    q, t = q.copy(), t.copy()
    for z, (nq, nt) in enumerate(counts):
        fill = q[z, :max(nq, 1)]
        t[z, nt:] = fill[np.arange(t.shape[1] - nt) % len(fill)]
        q[z, nq:] = fill[np.arange(q.shape[1] - nq) % len(fill)]
    return q, t


def batch_oracle(q, t, counts, ratio):
    """Per sequence (pairs, best, d2) of the oracle on the first (nq, nt) rows only; an empty side gives no pairs and
    best = -1, d2 = 0.0."""
    out = []
    for z, (nq, nt) in enumerate(counts):
        if nq == 0 or nt == 0:
            out.append((np.zeros((0, 2), np.int64), np.full((nq, 2), -1, np.int32), np.zeros((nq, 2))))
            continue
        pairs, best, d2 = native.match_knn2_ratio(q[z, :nq].astype(np.float32), t[z, :nt].astype(np.float32), ratio)
        out.append((pairs, best[:nq], d2[:nq]))
    return out
