"""-m gpu: the three 2-NN kernels of csrc/match.hip (matrix cores, packed byte dot product, float) and the ratio /
uniqueness filter against the oracle (oracle/csrc/match.c), bit for bit: both neighbours and both squared distances of
every query, the pair list, and which kernel produced them -- on every case of tests/matcher_cases.py (what each case is
for, and that it still is, is checked on the CPU by tests/test_matcher_host.py).  Then the frame pipeline's batch form on
device buffers of this test's own, and what the calls leave behind in the context."""
import numpy as np
import pytest

import matcher_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    return a.dtype == np.float64 and b.dtype == np.float64 and a.shape == b.shape and np.array_equal(
        np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_parametrization_reaches_all_three_kernels():
    for path in (cases.FLOAT, cases.BYTE_DOT, cases.MFMA):
        assert sum(c.path == path for c in cases.CASES) >= 10, path


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_equals_the_oracle(ctx, name):
    c = cases.BY_NAME[name]
    pairs, best, d2 = cases.oracle(name)
    got_best, got_d2, path = ctx.match_knn2(c.q, c.t)
    assert path == c.path and ctx.match_last_path() == c.path
    assert got_best.dtype == np.int32 and np.array_equal(got_best, best)
    assert same_bits(got_d2, d2)
    # (a call of the other kind in between: the getter must report the ratio call's own choice)
    other = cases.BY_NAME["float_D32_nq1_nt1_nopair" if c.path != cases.FLOAT else "dot_D16_nq20_nt513_tie"]
    assert ctx.match_knn2(other.q, other.t)[2] == other.path != c.path
    got = ctx.match_knn2_ratio(c.q, c.t, c.ratio)
    assert ctx.match_last_path() == c.path
    assert got.dtype == np.int64 and np.array_equal(got, pairs)
    assert len(set(got[:, 1])) == len(got)


def test_empty_sides(ctx):
    t = cases.BY_NAME["float_earlier_120x150x32"].t
    assert ctx.match_knn2_ratio(np.zeros((0, 8), np.float32), t[:, :8], 0.8).shape == (0, 2)
    assert ctx.match_knn2_ratio(t[:, :8], np.zeros((0, 8), np.float32), 0.8).shape == (0, 2)
    best, d2, path = ctx.match_knn2(np.zeros((0, 8), np.float32), t[:, :8])
    assert best.shape == (0, 2) and d2.shape == (0, 2) and path == -1 and ctx.match_last_path() == -1
    best, d2, path = ctx.match_knn2(t[:5, :8], np.zeros((0, 8), np.float32))
    assert np.all(best == -1) and best.shape == (5, 2) and same_bits(d2, np.zeros((5, 2))) and path == -1
    from vo import _native
    n = _native.C.c_int32(7)
    pairs = np.zeros((4, 2), np.int32)
    ctx._chk(ctx._lib.vo_match_knn2_ratio(ctx._h, None, 0, None, 0, 8, 0.8, _native._ptr(pairs), _native.C.byref(n)))
    assert n.value == 0 and ctx.match_last_path() == -1


# ---- the batch form: counts on the device, capacities above them, strides, one sequence per blockIdx.z ----

def run_batch(ctx, row_bytes, qb, tb, counts):
    """Both batch entries on fresh device buffers: (best, d2, pairs, n_pairs) as downloaded, every output preset to -7."""
    S, cq, ct = cases.BATCH_S, cases.BATCH_CAP_Q, cases.BATCH_CAP_T
    ctl = np.full((S, 6), 12345, np.int32)                   # sequence z: its query count in word 0, its train count in word 3
    ctl[:, 0], ctl[:, 3] = [c[0] for c in counts], [c[1] for c in counts]
    bufs = [ctx.to_device(a) for a in (qb, tb, ctl, np.full((S, cq, 2), -7, np.int32), np.full((S, cq, 2), -7.0),
                                       np.full((S, cq, 2), -7, np.int32), np.full(S, -7, np.int32))]
    d_q, d_t, d_ctl, d_best, d_d2, d_pairs, d_n = bufs
    q_stride, t_stride = qb.shape[1] * row_bytes, tb.shape[1] * row_bytes
    assert q_stride > cq * row_bytes and t_stride > ct * row_bytes
    try:
        ctx.knn2_u8_batch_dev(d_q, q_stride, d_ctl, 6, cq, d_t, t_stride, d_ctl + 12, 6, ct, S, row_bytes, d_best, d_d2)
        ctx.match_u8_batch_dev(d_q, q_stride, d_ctl, 6, cq, d_t, t_stride, d_ctl + 12, 6, ct, S, cases.BATCH_RATIO[row_bytes],
                               d_pairs, d_n, row_bytes)
        ctx.sync()
        return (ctx.download(d_best, (S, cq, 2), np.int32), ctx.download(d_d2, (S, cq, 2), np.float64),
                ctx.download(d_pairs, (S, cq, 2), np.int32), ctx.download(d_n, (S,), np.int32))
    finally:
        for p in bufs:
            ctx.free(p)


def check_batch(got, ref, counts):
    best, d2, pairs, n_pairs = got
    for z, (nq, nt) in enumerate(counts):
        ref_pairs, ref_best, ref_d2 = ref[z]
        if nt == 0:                                          # the documented fill: no neighbour, distance 0.0
            assert np.all(ref_best == -1) and not ref_d2.any()
        if nq == 0 or nt == 0:
            assert n_pairs[z] == 0
        assert np.array_equal(best[z, :nq], ref_best), z
        assert same_bits(d2[z, :nq], ref_d2), z
        assert np.all(best[z, nq:] == -7) and np.all(d2[z, nq:] == -7.0), z       # rows past the count are nobody's
        assert n_pairs[z] == len(ref_pairs), z
        assert np.array_equal(pairs[z, :n_pairs[z]], ref_pairs), z
        assert np.all(pairs[z, n_pairs[z]:] == -7), z


@pytest.mark.parametrize("row_bytes", [128, 384])
def test_batch_form_equals_the_oracle_per_sequence(ctx, row_bytes):
    q, t = cases.batch_inputs(row_bytes)
    for counts in (cases.BATCH_COUNTS, cases.BATCH_EMPTY):
        qb, tb = cases.batch_blocks(q, t, counts)
        ref = cases.batch_oracle(qb, tb, counts, cases.BATCH_RATIO[row_bytes])
        check_batch(run_batch(ctx, row_bytes, qb, tb, counts), ref, counts)


# ---- what a call leaves behind: arrival counters at zero, the partial lists reusable ----

def test_calls_leave_the_context_ready_for_the_next(ctx):
    by = {(c.q.shape, c.t.shape): c for c in cases.CASES if c.name.startswith("mfma_D128_nq70_")}
    four, one = by[((70, 128), (512, 128))], by[((70, 128), (129, 128))]
    two = cases.BY_NAME["mfma_earlier_300x280x361"]
    flt = cases.BY_NAME["float_spoiled_D128_t_last_0.5_tie"]

    def both(c):
        best, d2, path = ctx.match_knn2(c.q, c.t)
        return best, d2, path, ctx.match_knn2_ratio(c.q, c.t, c.ratio)

    def check(c, got):
        pairs, best, d2 = cases.oracle(c.name)
        assert np.array_equal(got[0], best) and same_bits(got[1], d2) and got[2] == c.path and np.array_equal(got[3], pairs)
    first = both(four)
    check(four, first)
    check(one, both(one))
    check(flt, both(flt))
    check(two, both(two))
    q, t = cases.batch_inputs(128)
    qb, tb = cases.batch_blocks(q, t, cases.BATCH_COUNTS)
    check_batch(run_batch(ctx, 128, qb, tb, cases.BATCH_COUNTS), cases.batch_oracle(qb, tb, cases.BATCH_COUNTS, 0.8),
                cases.BATCH_COUNTS)
    again = both(four)
    check(four, again)
    assert np.array_equal(again[0], first[0]) and same_bits(again[1], first[1]) and np.array_equal(again[3], first[3])
