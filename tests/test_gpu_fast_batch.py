"""-m gpu: the two batch primitives of the FAST + BRIEF tracker mode (vo_brief_describe_batch_dev,
vo_match_hamming_batch_dev) against the definition (tests/brief_reference.py), bit for bit, on the case tables of
tests/fast_loop_cases.py: counts in device memory, blocks further apart than their sizes, outputs pre-filled with a
sentinel that every row nobody may write must still hold."""
import numpy as np
import pytest

import brief_reference as ref
import fast_loop_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


class Dev:
    """Device buffers freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, arr):
        p = self.ctx.to_device(arr)
        self.ptrs.append(p)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.free(p)


def blocks(rows, stride, fill, dtype):
    """rows (S, ...) laid out as S blocks `stride` items of dtype apart, the gaps holding `fill`."""
    S = rows.shape[0]
    flat = rows.reshape(S, -1)
    out = np.full((S, stride), fill, dtype)
    out[:, :flat.shape[1]] = flat
    return out


@pytest.mark.parametrize("name", cases.DESCRIBE_NAMES)
def test_describe_batch_equals_the_definition(ctx, name):
    c = cases.DESCRIBE_BY_NAME[name]
    S, N = c.kp.shape[:2]
    H, W = c.imgs.shape[1:]
    want_desc, want_bins = cases.describe_expected(c)
    with Dev(ctx) as d:
        d_img = d.put(blocks(c.imgs, c.img_stride, 255, np.uint8))
        d_kp = d.put(blocks(c.kp, 2 * c.xy_stride, 20.0, np.float64))
        d_n = d.put(np.asarray(c.counts, np.int32))
        d_desc = d.put(np.full((S, c.desc_stride), cases.SENTINEL, np.uint8))
        d_bin = d.put(np.full((S, c.xy_stride), cases.SENTINEL, np.uint8))
        ctx.brief_describe_batch_dev(d_img, c.img_stride, S, H, W, d_kp, c.xy_stride, d_n, N, c.oriented, d_desc,
                                     c.desc_stride, d_bin)
        ctx.sync()
        got_desc = ctx.download(d_desc, (S, c.desc_stride), np.uint8)
        got_bins = ctx.download(d_bin, (S, c.xy_stride), np.uint8)
        # without the bins: the same descriptors
        d_desc2 = d.put(np.full((S, c.desc_stride), cases.SENTINEL, np.uint8))
        ctx.brief_describe_batch_dev(d_img, c.img_stride, S, H, W, d_kp, c.xy_stride, d_n, N, c.oriented, d_desc2, c.desc_stride)
        ctx.sync()
        assert np.array_equal(ctx.download(d_desc2, (S, c.desc_stride), np.uint8), got_desc)
    assert np.array_equal(got_desc[:, :32 * N].reshape(S, N, 32), want_desc)
    assert (got_desc[:, 32 * N:] == cases.SENTINEL).all()
    assert np.array_equal(got_bins[:, :N], want_bins) and (got_bins[:, N:] == cases.SENTINEL).all()


def match_batch(ctx, c, q_gap=64, t_gap=96):
    """(pairs (S, cap_q, 2), n (S,)) of one vo_match_hamming_batch_dev call on case c, d_pairs pre-filled with
    PAIR_SENTINEL; the counts lie 3 (queries) and 2 (train rows) ints apart, as fields of a structure would."""
    S, B = c.q.shape[0], c.q.shape[2]
    q_stride, t_stride = c.cap_q * B + q_gap, c.cap_t * B + t_gap
    nq = np.full((S, 3), -99, np.int32)
    nt = np.full((S, 2), -99, np.int32)
    nq[:, 0], nt[:, 0] = c.nq, c.nt
    with Dev(ctx) as d:
        d_q = d.put(blocks(c.q, q_stride, 0, np.uint8))
        d_t = d.put(blocks(c.t, t_stride, 0, np.uint8))
        d_nq, d_nt = d.put(nq), d.put(nt)
        d_pairs = d.put(np.full((S, c.cap_q, 2), cases.PAIR_SENTINEL, np.int32))
        d_np = d.put(np.full(S, cases.PAIR_SENTINEL, np.int32))
        ctx.match_hamming_batch_dev(d_q, q_stride, d_nq, 3, c.cap_q, d_t, t_stride, d_nt, 2, c.cap_t, S, B, c.ratio,
                                    c.max_dist, d_pairs, d_np)
        ctx.sync()
        return ctx.download(d_pairs, (S, c.cap_q, 2), np.int32), ctx.download(d_np, (S,), np.int32)


@pytest.mark.parametrize("name", cases.MATCH_NAMES)
def test_match_batch_equals_the_definition(ctx, name):
    c = cases.MATCH_BY_NAME[name]
    want = cases.match_expected(c)
    pairs, n = match_batch(ctx, c)
    for z, w in enumerate(want):
        assert n[z] == len(w), (z, n[z], len(w))
        assert np.array_equal(pairs[z, :len(w)], w), z
        assert (pairs[z, len(w):] == cases.PAIR_SENTINEL).all(), z          # rows beyond the count are not written
    # ... and, called twice, the same again (the owner tables of the first call are nobody's business in the second)
    pairs2, n2 = match_batch(ctx, c)
    assert np.array_equal(n, n2) and np.array_equal(pairs, pairs2)


@pytest.mark.parametrize("name", ["partial_query_groups", "ties_at_ratio_and_max_dist"])
def test_unaligned_rows_take_the_word_path(ctx, name):
    """Blocks 4 but not 16 bytes apart: the rows are read word by word, with the same result."""
    c = cases.MATCH_BY_NAME[name]
    want = cases.match_expected(c)
    pairs, n = match_batch(ctx, c, q_gap=4, t_gap=12)
    for z, w in enumerate(want):
        assert n[z] == len(w) and np.array_equal(pairs[z, :len(w)], w), z


def test_one_image_entry_points_equal_the_batch_of_one(ctx):
    """vo_brief_describe_dev / vo_match_hamming_ratio and the batch entry points with S = 1: the same bytes."""
    c = cases.DESCRIBE_BY_NAME["border_and_nonfinite_oriented"]
    H, W = c.imgs.shape[1:]
    img, kp = c.imgs[0], np.ascontiguousarray(c.kp[0])
    N = len(kp)
    with Dev(ctx) as d:
        d_img, d_kp, d_n = d.put(img), d.put(kp), d.put(np.asarray([N], np.int32))
        outs = [d.put(np.full(N * 33, cases.SENTINEL, np.uint8)) for _ in range(2)]
        ctx.brief_describe_dev(d_img, H, W, d_kp, N, 1, outs[0], outs[0] + 32 * N)
        ctx.brief_describe_batch_dev(d_img, H * W, 1, H, W, d_kp, N, d_n, N, 1, outs[1], 32 * N, outs[1] + 32 * N)
        ctx.sync()
        a, b = (ctx.download(p, (N * 33,), np.uint8) for p in outs)
    want_desc, want_bins = ref.describe(img, kp, True)
    assert np.array_equal(a, b)
    assert np.array_equal(a[:32 * N].reshape(N, 32), want_desc) and np.array_equal(a[32 * N:], want_bins)
    m = cases.MATCH_BY_NAME["train_index_contested_in_two_sequences"]
    pairs, n = match_batch(ctx, m)
    for z in range(m.q.shape[0]):
        one = ctx.match_hamming_ratio(m.q[z], m.t[z], m.ratio, m.max_dist)
        assert np.array_equal(one, pairs[z, :n[z]])


def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx):
    from vo._native import VoError
    c = cases.DESCRIBE_BY_NAME["counts_0_1_5"]
    S, N = c.kp.shape[:2]
    H, W = c.imgs.shape[1:]
    m = cases.MATCH_BY_NAME["partial_query_groups"]
    with Dev(ctx) as d:
        buf = d.put(np.zeros(1 << 16, np.uint8))
        ok_d = dict(d_imgs=buf, img_stride=c.img_stride, S=S, H=H, W=W, d_kp_xy=buf, xy_stride=c.xy_stride, d_n=buf, N=N, oriented=0,
                    d_desc=buf, desc_stride=c.desc_stride)
        for bad in (dict(S=0), dict(N=0), dict(N=16385), dict(img_stride=H * W - 1), dict(xy_stride=N - 1), dict(desc_stride=32 * N - 1),
                    dict(d_n=None), dict(d_desc=None), dict(H=0)):
            with pytest.raises(VoError):
                ctx.brief_describe_batch_dev(**{**ok_d, **bad})
        ok_m = dict(d_q=buf, q_stride=20 * 32, d_nq=buf, nq_stride=1, cap_q=20, d_t=buf, t_stride=40 * 32, d_nt=buf, nt_stride=1, cap_t=40,
                    S=3, row_bytes=32, ratio=0.8, max_dist=64, d_pairs=buf, d_npairs=buf)
        for bad in (dict(row_bytes=30), dict(row_bytes=68), dict(S=0), dict(cap_q=0), dict(cap_t=0), dict(q_stride=20 * 32 - 4),
                    dict(t_stride=40 * 32 + 2), dict(nq_stride=0), dict(ratio=float("nan")), dict(d_pairs=None), dict(d_nt=None),
                    dict(d_q=buf + 2)):
            with pytest.raises(VoError):
                ctx.match_hamming_batch_dev(**{**ok_m, **bad})
    # (refused calls change nothing: the context still computes)
    pairs, n = match_batch(ctx, m)
    assert [int(v) for v in n] == [len(w) for w in cases.match_expected(m)]
