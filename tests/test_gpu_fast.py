"""-m gpu: csrc/fast.hip through the C ABI against the definition (tests/fast_reference.py), bit for bit on every case of
tests/fast_cases.py: the score map, keypoints / scores / n / total for both `nonmax` values through the host and the
device-pointer forms, the batch forms against one-image calls, what the _dev form leaves untouched, its hand-over to
vo_brief_describe_dev without a host turn, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import brief_reference as bref
import fast_cases as cases
import fast_reference as ref

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    yield _native.default_context()


_want = {}


def want(name, threshold, nonmax, N):
    key = (name, threshold, int(nonmax), N)
    if key not in _want:
        _want[key] = ref.keypoints(cases.BY_NAME[name].img, threshold, nonmax, N)
    return _want[key]


def run_dev(ctx, imgs, threshold, nonmax, N, img_pad=0, xy_pad=0, scores=True, total=True):
    """vo_fast_keypoints_batch_dev on freshly filled buffers; returns the raw (S, xy_stride, 2) float64 block, the
    (S, xy_stride) score block or None, n (S,) and total (S,) or None -- everything the call could have written."""
    S, (H, W) = len(imgs), imgs[0].shape
    img_stride, xy_stride = H * W + img_pad, N + xy_pad
    block = np.full((S, img_stride), 0x3C, np.uint8)
    for q, im in enumerate(imgs):
        block[q, :H * W] = im.reshape(-1)
    d_img = ctx.to_device(block)
    d_kp = ctx.to_device(np.full(S * xy_stride * 16, FILL, np.uint8))
    d_sc = ctx.to_device(np.full(S * xy_stride, FILL, np.uint8))
    d_n = ctx.to_device(np.full(S * 4, FILL, np.uint8))
    d_tot = ctx.to_device(np.full(S * 4, FILL, np.uint8))
    try:
        ctx.fast_keypoints_batch_dev(d_img, img_stride, S, H, W, d_kp, xy_stride, d_n, threshold, N, nonmax,
                                     d_kp_score=d_sc if scores else None, d_total=d_tot if total else None)
        ctx.sync()
        return (ctx.download(d_kp, (S, xy_stride, 2), np.float64), ctx.download(d_sc, (S, xy_stride), np.uint8),
                ctx.download(d_n, (S,), np.int32), ctx.download(d_tot, (S,), np.int32))
    finally:
        for p in (d_img, d_kp, d_sc, d_n, d_tot):
            ctx.free(p)


def check_dev(out, names, threshold, nonmax, N, scores=True, total=True):
    kp, sc, n, tot = out
    fill_f64 = np.frombuffer(bytes([FILL]) * 8, np.float64)[0]
    for q, name in enumerate(names):
        wkp, wsc, wtot = want(name, threshold, nonmax, N)
        assert n[q] == len(wkp), (name, nonmax, int(n[q]), len(wkp))
        assert np.array_equal(kp[q, :n[q]], wkp), (name, nonmax)
        assert np.all(kp[q, n[q]:].view(np.uint64) == fill_f64.view(np.uint64)), (name, "rows at and beyond n were written")
        if scores:
            assert np.array_equal(sc[q, :n[q]], wsc), (name, nonmax)
            assert np.all(sc[q, n[q]:] == FILL)
        else:
            assert np.all(sc == FILL)
        if total:
            assert tot[q] == wtot, (name, nonmax, int(tot[q]), wtot)
        else:
            assert np.all(tot.view(np.uint8) == FILL)


@pytest.mark.parametrize("name", cases.NAMES)
def test_score_map_equals_the_definition(ctx, name):
    c = cases.BY_NAME[name]
    got = ctx.fast_score(c.img, c.threshold)
    assert got.dtype == np.uint8 and got.shape == c.img.shape
    assert np.array_equal(got, ref.score_map(c.img, c.threshold)), name


@pytest.mark.parametrize("name", cases.NAMES)
def test_keypoints_equal_the_definition(ctx, name):
    c = cases.BY_NAME[name]
    for nonmax in (0, 1):
        wkp, wsc, _ = want(name, c.threshold, nonmax, c.N)
        kp, sc = ctx.fast_keypoints(c.img, c.threshold, c.N, nonmax=bool(nonmax), want_scores=True)
        assert kp.dtype == np.float64 and sc.dtype == np.uint8
        assert kp.shape == wkp.shape and np.array_equal(kp, wkp), (name, nonmax)
        assert np.array_equal(sc, wsc), (name, nonmax)
        assert np.array_equal(ctx.fast_keypoints(c.img, c.threshold, c.N, nonmax=bool(nonmax)), wkp)     # no scores asked for
        out = run_dev(ctx, [c.img], c.threshold, nonmax, c.N)
        check_dev(out, [name], c.threshold, nonmax, c.N)
        again = run_dev(ctx, [c.img], c.threshold, nonmax, c.N)                # a second run: the same bytes
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out, again)), (name, nonmax)


@pytest.mark.parametrize("batch", [b[0] for b in cases.BATCH])
def test_batch_forms_equal_one_image_calls(ctx, batch):
    _, names, threshold, N = [b for b in cases.BATCH if b[0] == batch][0]
    imgs = [cases.BY_NAME[n].img for n in names]
    for nonmax in (0, 1):
        single = [ctx.fast_keypoints(im, threshold, N, nonmax=bool(nonmax), want_scores=True) for im in imgs]
        for q, name in enumerate(names):
            wkp, wsc, _ = want(name, threshold, nonmax, N)
            assert np.array_equal(single[q][0], wkp) and np.array_equal(single[q][1], wsc), (name, nonmax)
        for form in (imgs, np.stack(imgs)):
            both = ctx.fast_keypoints_batch(form, threshold, N, nonmax=bool(nonmax), want_scores=True)
            assert len(both) == len(imgs)
            for (kp, sc), (skp, ssc) in zip(both, single):
                assert kp.shape == skp.shape and np.array_equal(kp, skp) and np.array_equal(sc, ssc), (batch, nonmax)
        plain = ctx.fast_keypoints_batch(imgs, threshold, N, nonmax=bool(nonmax))
        assert all(np.array_equal(a, b[0]) for a, b in zip(plain, single))
        # the device form: padded strides, and the nullable outputs absent
        check_dev(run_dev(ctx, imgs, threshold, nonmax, N, img_pad=37, xy_pad=5), names, threshold, nonmax, N)
        check_dev(run_dev(ctx, imgs, threshold, nonmax, N, img_pad=1, xy_pad=3, scores=False, total=False), names, threshold,
                  nonmax, N, scores=False, total=False)


def test_dev_output_feeds_brief_describe_dev_without_a_host_turn(ctx):
    name, N = "steps_70x131", 50
    c = cases.BY_NAME[name]
    H, W = c.img.shape
    wkp, _, wtot = want(name, c.threshold, 1, N)
    assert len(wkp) == N < wtot                                  # n = N is known beforehand: the describe call needs no count
    d_img = ctx.to_device(c.img)
    d_kp, d_n = ctx.to_device(np.full((N, 2), -1.0)), ctx.to_device(np.zeros(1, np.int32))
    d_desc = ctx.to_device(np.full((N, 32), FILL, np.uint8))
    try:
        ctx.fast_keypoints_batch_dev(d_img, H * W, 1, H, W, d_kp, N, d_n, c.threshold, N, True)
        ctx.brief_describe_dev(d_img, H, W, d_kp, N, 0, d_desc)
        ctx.sync()
        assert ctx.download(d_n, (1,), np.int32)[0] == N
        assert np.array_equal(ctx.download(d_desc, (N, 32), np.uint8), bref.describe(c.img, wkp, False)[0])
    finally:
        for p in (d_img, d_kp, d_n, d_desc):
            ctx.free(p)


def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx):
    from vo import _native
    lib, h, p = ctx._lib, ctx._h, _native._ptr
    c = cases.BY_NAME["lane_sparse_40x70"]
    img = np.ascontiguousarray(c.img)
    H, W = img.shape
    wkp, wsc, _ = want(c.name, 5, 1, 60)
    wmap = ref.score_map(img, 5)
    kp, sc, n = np.full((70, 2), 7.5), np.full(70, 0x5A, np.uint8), C.c_int32(-3)
    smap = np.full((H, W), 0x5A, np.uint8)

    def good():
        assert np.array_equal(ctx.fast_keypoints(img, 5, 60), wkp)
        assert np.array_equal(ctx.fast_score(img, 5), wmap)

    def untouched():
        assert np.all(kp == 7.5) and np.all(sc == 0x5A) and n.value == -3 and np.all(smap == 0x5A)

    one = [  # (img, H, W, threshold, nonmax, N, kp, n)
        (None, H, W, 5, 1, 60, kp, n), (img, H, W, 5, 1, 60, None, n), (img, H, W, 5, 1, 60, kp, None), (img, 0, W, 5, 1, 60, kp, n),
        (img, H, 0, 5, 1, 60, kp, n), (img, -1, W, 5, 1, 60, kp, n), (img, H, W, -1, 1, 60, kp, n), (img, H, W, 255, 1, 60, kp, n),
        (img, H, W, 5, 2, 60, kp, n), (img, H, W, 5, 1, 0, kp, n), (img, H, W, 5, 1, 16385, kp, n)]
    for a in one:
        rc = lib.vo_fast_keypoints(h, p(a[0]), a[1], a[2], a[3], a[4], a[5], p(a[6]), p(sc), C.byref(a[7]) if a[7] is not None else None)
        assert rc == _native.VO_EINVAL and b"fast_keypoints" in lib.vo_last_error(h), a[1:6]
        untouched()
        good()
    for a in ((None, H, W, 5, smap), (img, H, W, 5, None), (img, 0, W, 5, smap), (img, H, W, 255, smap), (img, H, W, -1, smap)):
        assert lib.vo_fast_score(h, p(a[0]), a[1], a[2], a[3], p(a[4])) == _native.VO_EINVAL
        assert b"fast_score" in lib.vo_last_error(h)
        untouched()
        good()
    ns = np.full(2, -3, np.int32)
    for S in (0, -1):
        assert lib.vo_fast_keypoints_batch(h, p(img), S, H, W, 5, 1, 60, p(kp), p(sc), p(ns)) == _native.VO_EINVAL
        assert b"fast_keypoints_batch" in lib.vo_last_error(h) and np.all(ns == -3)
        untouched()
        good()
    # the device form: strides below what the call needs, S, null pointers
    d_img, d_kp, d_n = ctx.to_device(img), ctx.to_device(np.full((60, 2), 7.5)), ctx.to_device(np.full(1, -3, np.int32))
    try:
        vp = C.c_void_p
        dev = [  # (d_imgs, img_stride, S, N, d_kp, xy_stride, d_n)
            (d_img, H * W - 1, 1, 60, d_kp, 60, d_n), (d_img, H * W, 1, 60, d_kp, 59, d_n), (d_img, H * W, 0, 60, d_kp, 60, d_n),
            (None, H * W, 1, 60, d_kp, 60, d_n), (d_img, H * W, 1, 60, None, 60, d_n), (d_img, H * W, 1, 60, d_kp, 60, None),
            (d_img, H * W, 1, 16385, d_kp, 16385, d_n)]
        for a in dev:
            rc = lib.vo_fast_keypoints_batch_dev(h, vp(a[0]), a[1], a[2], H, W, 5, 1, a[3], vp(a[4]), a[5], None, vp(a[6]), None)
            assert rc == _native.VO_EINVAL and b"fast_keypoints_batch_dev" in lib.vo_last_error(h), a[1:4]
            ctx.sync()
            assert np.all(ctx.download(d_kp, (60, 2), np.float64) == 7.5) and ctx.download(d_n, (1,), np.int32)[0] == -3
            good()
        with pytest.raises(_native.VoError, match="xy_stride"):
            ctx.fast_keypoints_batch_dev(d_img, H * W, 1, H, W, d_kp, 10, d_n, 5, 60, True)
        ctx.fast_keypoints_batch_dev(d_img, H * W, 1, H, W, d_kp, 60, d_n, 5, 60, True)
        ctx.sync()
        assert ctx.download(d_n, (1,), np.int32)[0] == len(wkp)
        assert np.array_equal(ctx.download(d_kp, (60, 2), np.float64)[:len(wkp)], wkp)
    finally:
        for q in (d_img, d_kp, d_n):
            ctx.free(q)
    with pytest.raises(_native.VoError, match="threshold"):
        ctx.fast_keypoints(img, 300, 60)
    with pytest.raises(_native.VoError, match="N ="):
        ctx.fast_keypoints_batch([img, img], 5, 0)
    good()
