"""-m gpu: csrc/brief.hip through the C ABI against the definition (tests/brief_reference.py), bit for bit on every case
of tests/brief_cases.py: descriptors and bins for both `oriented` values, the device-pointer form, the pattern table, the
Hamming 2-NN lists, the pair list, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import brief_cases as cases
import brief_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    yield _native.default_context()


@pytest.mark.parametrize("name", cases.DESCRIBE_NAMES)
def test_describe_equals_the_definition(ctx, name):
    c = cases.DESCRIBE_BY_NAME[name]
    for oriented in (0, 1):
        want_d, want_b = ref.describe(c.img, c.kp, oriented)
        desc, bins = ctx.brief_describe(c.img, c.kp, oriented=oriented, want_bins=True)
        assert desc.dtype == np.uint8 and desc.shape == (len(c.kp), 32) and bins.shape == (len(c.kp),)
        assert np.array_equal(bins, want_b), (name, oriented)
        assert np.array_equal(desc, want_d), (name, oriented)
        again = ctx.brief_describe(c.img, c.kp, oriented=oriented)              # a second run, no bins asked for
        assert np.array_equal(again, desc)


@pytest.mark.parametrize("name", ["borders_and_inside", "beyond_the_window", "quarter_turn", "n_65", "n_257"])
def test_describe_dev_form_equals_the_host_form(ctx, name):
    c = cases.DESCRIBE_BY_NAME[name]
    H, W = c.img.shape
    n = len(c.kp)
    d_img, d_kp = ctx.to_device(c.img), ctx.to_device(c.kp)
    d_desc, d_bin = ctx.to_device(np.full((n, 32), 0xA5, np.uint8)), ctx.to_device(np.full(n, 0xA5, np.uint8))
    try:
        for oriented in (0, 1):
            host_d, host_b = ctx.brief_describe(c.img, c.kp, oriented=oriented, want_bins=True)
            ctx.brief_describe_dev(d_img, H, W, d_kp, n, oriented, d_desc, d_bin)
            ctx.sync()
            assert np.array_equal(ctx.download(d_desc, (n, 32), np.uint8), host_d)
            assert np.array_equal(ctx.download(d_bin, (n,), np.uint8), host_b)
        ctx.upload(d_bin, np.full(n, 0xA5, np.uint8))
        ctx.brief_describe_dev(d_img, H, W, d_kp, n, 1, d_desc, None)           # no bins wanted: none written
        ctx.sync()
        assert np.array_equal(ctx.download(d_desc, (n, 32), np.uint8), host_d)
        assert np.all(ctx.download(d_bin, (n,), np.uint8) == 0xA5)
    finally:
        for p in (d_img, d_kp, d_desc, d_bin):
            ctx.free(p)


def test_pattern_is_the_generators(ctx):
    table = ctx.brief_pattern()
    assert table.dtype == np.int8 and np.array_equal(table, ref.tables()[0])


@pytest.mark.parametrize("name", cases.MATCH_NAMES)
def test_hamming_lists_and_pairs_equal_the_definition(ctx, name):
    c = cases.MATCH_BY_NAME[name]
    want_best, want_dist = ref.knn2(c.q, c.t)
    best, dist = ctx.match_hamming_knn2(c.q, c.t)
    assert best.dtype == np.int32 and dist.dtype == np.int32
    assert np.array_equal(dist, want_dist), name
    assert np.array_equal(best, want_best), name
    pairs = ctx.match_hamming_ratio(c.q, c.t, c.ratio, c.max_dist)
    want = ref.ratio_pairs(want_best, want_dist, c.ratio, c.max_dist)
    assert pairs.shape == want.shape and np.array_equal(pairs, want), name


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("name", ["grid_B4_nq65_nt513", "grid_B32_nq130_nt513", "grid_B64_nq63_nt257", "grid_B32_nq1_nt0"])
def test_hamming_dev_form_equals_the_definition(ctx, name, offset):
    """Device pointers; offset 4: rows that start on a 4-byte boundary only (32- and 64-byte rows then take the kernel that
    loads word by word, as every other length does)."""
    c = cases.MATCH_BY_NAME[name]
    nq, nt, B = len(c.q), len(c.t), c.q.shape[1]
    d_q, d_t = ctx.alloc(c.q.nbytes + 16), ctx.alloc(c.t.nbytes + 16)
    d_best, d_dist = ctx.to_device(np.full((nq, 2), 77, np.int32)), ctx.to_device(np.full((nq, 2), 77, np.int32))
    try:
        ctx.upload(d_q + offset, c.q)
        if nt:
            ctx.upload(d_t + offset, c.t)
        ctx.hamming_knn2_dev(d_q + offset, nq, d_t + offset, nt, B, d_best, d_dist)
        ctx.sync()
        best, dist = ref.knn2(c.q, c.t)
        assert np.array_equal(ctx.download(d_best, (nq, 2), np.int32), best)
        assert np.array_equal(ctx.download(d_dist, (nq, 2), np.int32), dist)
        with pytest.raises(Exception, match="4-byte"):
            ctx.hamming_knn2_dev(d_q + 2, nq, d_t, nt, B, d_best, d_dist)
    finally:
        for p in (d_q, d_t, d_best, d_dist):
            ctx.free(p)


def test_bad_arguments_are_refused_and_write_nothing(ctx):
    from vo import _native
    lib, h = ctx._lib, ctx._h
    img = cases.DESCRIBE_BY_NAME["corners"].img
    H, W = img.shape
    kp = np.tile(np.array([[10.0, 10.0]]), (16385, 1))
    desc, bins = np.full((16385, 32), 0x5A, np.uint8), np.full(16385, 0x5A, np.uint8)
    p = _native._ptr
    for n, image, oriented in ((0, img, 0), (16385, img, 0), (-1, img, 0), (4, None, 0), (4, img, 2)):
        rc = lib.vo_brief_describe(h, p(image), H, W, p(kp), n, oriented, p(desc), p(bins))
        assert rc == _native.VO_EINVAL and b"brief_describe" in lib.vo_last_error(h), (n, oriented)
        assert np.all(desc == 0x5A) and np.all(bins == 0x5A)
    assert lib.vo_brief_describe(h, p(img), 0, W, p(kp), 4, 0, p(desc), p(bins)) == _native.VO_EINVAL
    assert lib.vo_brief_describe(h, p(img), H, W, None, 4, 0, p(desc), p(bins)) == _native.VO_EINVAL
    assert lib.vo_brief_describe(h, p(img), H, W, p(kp), 4, 0, None, p(bins)) == _native.VO_EINVAL
    assert lib.vo_brief_describe_dev(h, None, H, W, None, 4, 0, None, None) == _native.VO_EINVAL
    assert np.all(desc == 0x5A) and np.all(bins == 0x5A)
    assert lib.vo_brief_pattern(None) == _native.VO_EINVAL
    q = np.zeros((4, 68), np.uint8)
    best, dist = np.full((4, 2), 99, np.int32), np.full((4, 2), 99, np.int32)
    pairs, npairs = np.full((4, 2), 99, np.int32), C.c_int32(99)
    for B in (0, 3, 68, 6, -4):
        assert lib.vo_match_hamming_knn2(h, p(q), 4, p(q), 4, B, p(best), p(dist)) == _native.VO_EINVAL
        assert b"row_bytes" in lib.vo_last_error(h)
        assert lib.vo_hamming_knn2_dev(h, None, 4, None, 4, B, None, None) == _native.VO_EINVAL
        assert lib.vo_match_hamming_ratio(h, p(q), 4, p(q), 4, B, 0.8, -1, p(pairs), C.byref(npairs)) == _native.VO_EINVAL
        assert np.all(best == 99) and np.all(dist == 99) and np.all(pairs == 99) and npairs.value == 99
    assert lib.vo_match_hamming_knn2(h, p(q), -1, p(q), 4, 32, p(best), p(dist)) == _native.VO_EINVAL
    assert lib.vo_match_hamming_knn2(h, None, 4, p(q), 4, 32, p(best), p(dist)) == _native.VO_EINVAL
    assert lib.vo_match_hamming_ratio(h, p(q), 4, p(q), 4, 32, float("nan"), -1, p(pairs), C.byref(npairs)) == _native.VO_EINVAL
    assert np.all(best == 99) and np.all(dist == 99) and np.all(pairs == 99) and npairs.value == 99
    with pytest.raises(_native.VoError, match="row_bytes"):
        ctx.match_hamming_knn2(np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8))
    # empty sides, as match_knn2_ratio has them
    assert ctx.match_hamming_ratio(np.zeros((0, 32), np.uint8), np.zeros((5, 32), np.uint8), 0.8).shape == (0, 2)
    assert ctx.match_hamming_ratio(np.zeros((5, 32), np.uint8), np.zeros((0, 32), np.uint8), 0.8).shape == (0, 2)
    best, dist = ctx.match_hamming_knn2(np.zeros((3, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert np.all(best == -1) and np.all(dist == 0) and best.shape == (3, 2)
    assert ctx.match_hamming_knn2(np.zeros((0, 32), np.uint8), np.zeros((3, 32), np.uint8))[0].shape == (0, 2)
