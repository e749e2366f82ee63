"""-m gpu: batched Shi-Tomasi (vo_good_features_batch_dev / vo_good_features_batch, Context.good_features_batch) against
the CPU oracle image by image and against the one-image call.  Every comparison is np.array_equal: image q's corners are
those of the one-image definition, bit for bit and in order, whichever path -- parallel rounds, the one-workgroup walk, the
sorted list's head -- the device chose for it (d_info).  The images' preconditions are checked on the CPU in
tests/test_good_features_batch_host.py."""
import numpy as np
import pytest

import good_features_batch_cases as cases
from oracle import native

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def oracle_each(imgs, masks, n, quality, min_dist, block):
    masks = masks or [None] * len(imgs)
    return [native.good_features(img, m, n, quality, min_dist, block) for img, m in zip(imgs, masks)]


def same_lists(got, ref, what=""):
    assert len(got) == len(ref), what
    for q, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == np.float32 and g.shape == r.shape, (what, q, g.shape, r.shape)
        assert np.array_equal(g, r), (what, q)


def rounds_dev(ctx, rounds, cand_limit):
    """The library's internal form of the batched call with the number of round launches and the rounds path's candidate
    limit given (csrc/vo_internal.h: vo_good_features_batch_rounds_dev), as a stand-in for Context.good_features_batch_dev."""
    import ctypes as C
    fn = ctx._lib.vo_good_features_batch_rounds_dev
    fn.restype = C.c_int
    vp, i, d, sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    fn.argtypes = [vp, vp, sz, i, i, i, vp, sz, i, d, d, i, vp, sz, vp, vp, vp, i, i]

    def call(d_imgs, img_stride, S, H, W, d_xy, xy_stride, d_n, d_masks, mask_stride, n, quality, min_dist, block, d_over, d_info):
        ctx._chk(fn(ctx._h, d_imgs, img_stride, S, H, W, d_masks or None, mask_stride, n, quality, min_dist, block, d_xy,
                    xy_stride, d_n, d_over, d_info, rounds, cand_limit))
    return call


def batch_dev(ctx, imgs, masks, n, quality, min_dist, block, xy_stride=None, S=None, call=None):
    """The device form on buffers of this test's own: (corner lists, d_n, d_over, d_info)."""
    call = call or ctx.good_features_batch_dev
    imgs = np.ascontiguousarray(np.stack(imgs), np.uint8)
    S_real, H, W = imgs.shape
    S = S_real if S is None else S
    rows = ctx.good_features_capacity(H, W, n)
    stride = rows if xy_stride is None else xy_stride
    held = []

    def dev(arr):
        held.append(ctx.to_device(arr))
        return held[-1]
    try:
        d_imgs = dev(imgs)
        d_masks = 0
        if masks is not None:
            full = np.full((H, W), 255, np.uint8)
            d_masks = dev(np.stack([full if m is None else m for m in masks]).astype(np.uint8))
        sentinel = np.full((S_real, max(stride, 1), 2), -7.0, np.float32)
        d_xy, d_n = dev(sentinel), dev(np.full(S_real, -1, np.int32))
        d_over, d_info = dev(np.full(S_real, -1, np.int32)), dev(np.full((S_real, 4), -1, np.int32))
        call(d_imgs, H * W, S, H, W, d_xy, stride, d_n, d_masks, H * W, n, quality, min_dist, block, d_over, d_info)
        ctx.sync()
        xy = ctx.download(d_xy, sentinel.shape, np.float32)
        cnt = ctx.download(d_n, (S_real,), np.int32)
        over = ctx.download(d_over, (S_real,), np.int32)
        info = ctx.download(d_info, (S_real, 4), np.int32)
    finally:
        for p in held:
            ctx.free(p)
    for q in range(S_real):               # nothing behind an image's count is written
        assert np.all(xy[q, max(cnt[q], 0):] == -7.0), q
    return [xy[q, : cnt[q]].copy() for q in range(S_real)], cnt, over, info


def test_five_images_equal_the_oracle_and_take_the_rounds_path(ctx):
    """1. + 6. S = 5 at 480 x 640 with the defaults, the flat image among them: corners and counts are the oracle's; the
    ordinary images went through the rounds (path 0, at least one round), none was handed to the walk."""
    imgs = cases.ordinary_images()
    ref = oracle_each(imgs, None, *cases.DEFAULTS)
    same_lists(ctx.good_features_batch(imgs, None, *cases.DEFAULTS), ref, "host form")
    got, cnt, over, info = batch_dev(ctx, imgs, None, *cases.DEFAULTS)
    same_lists(got, ref, "device form")
    print("candidates / path / rounds:", info[:, :3].tolist())
    assert cnt.tolist() == [len(r) for r in ref] and cnt[2] == 0 and np.all(over == 0)
    for q in range(5):
        take = cases.local_maxima(imgs[q], None, cases.DEFAULTS[1], cases.DEFAULTS[3])
        assert info[q, 0] == take.sum(), q
        assert info[q, 1] == 0, (q, info[q].tolist())
        assert (info[q, 2] >= 1) if q != 2 else (info[q, 2] == 0), (q, info[q].tolist())
        assert info[q, 3] == 0


def test_batch_equals_the_one_image_call(ctx):
    """2. the same batch through Context.good_features one by one; both are the oracle's (the one-image call runs the batched
    stages, so it is no independent witness)."""
    imgs = cases.ordinary_images()
    one = [ctx.good_features(img, None, *cases.DEFAULTS) for img in imgs]
    ref = oracle_each(imgs, None, *cases.DEFAULTS)
    same_lists(one, ref, "one by one against the oracle")
    same_lists(ctx.good_features_batch(imgs, None, *cases.DEFAULTS), ref, "the batch against the oracle")
    same_lists(ctx.good_features_batch(imgs, None, *cases.DEFAULTS), one)
    same_lists(ctx.good_features_batch(np.stack(imgs), None, *cases.DEFAULTS), one, "a 3-D array")


@pytest.mark.parametrize("shape,seed", [((120, 160), 1), ((240, 320), 2), ((97, 131), 3), ((480, 640), 11)])
def test_one_image_batch_equals_good_features(ctx, shape, seed):
    """3. S = 1 is vo_good_features (sizes that are not multiples of the tiles included)."""
    from scenarios import synthetic_image
    img = synthetic_image(shape[0], shape[1], seed, block=9)
    for params in (cases.DEFAULTS, cases.MASKED, cases.CROWDED):
        got = ctx.good_features_batch([img], None, *params)
        assert len(got) == 1
        assert np.array_equal(got[0], ctx.good_features(img, None, *params)), params
        assert np.array_equal(got[0], native.good_features(img, None, *params)), params


def test_masks_are_per_image(ctx):
    """4. some images masked, some not, with the one-image test's (50, 0.05, 5, 5)."""
    imgs, masks = cases.ordinary_images(), cases.masks_for()
    ref = oracle_each(imgs, masks, *cases.MASKED)
    same_lists(ctx.good_features_batch(imgs, masks, *cases.MASKED), ref, "host form")
    got, cnt, over, info = batch_dev(ctx, imgs, masks, *cases.MASKED)
    same_lists(got, ref, "device form")
    assert np.all(got[0][:, 0] < cases.SMALL[1] // 2) and np.all(got[3][:, 1] >= cases.SMALL[0] // 2)
    assert np.all(over == 0)
    # an all-zero mask for one image: no corner there, the others as before
    empty = [None, np.zeros(cases.SMALL, np.uint8), None, None, None]
    got = ctx.good_features_batch(imgs, empty, *cases.MASKED)
    assert len(got[1]) == 0
    same_lists([got[0]] + got[2:], oracle_each([imgs[0]] + imgs[2:], None, *cases.MASKED), "beside an empty mask")


def test_crowded_cells_go_to_the_walk(ctx):
    """5. every corner at min_distance 40: the crowded images are finished by the one-workgroup walk (path 1), the flat one is
    not; all equal the oracle."""
    imgs = cases.ordinary_images()
    ref = oracle_each(imgs, None, *cases.CROWDED)
    same_lists(ctx.good_features_batch(imgs, None, *cases.CROWDED), ref, "host form")
    got, cnt, over, info = batch_dev(ctx, imgs, None, *cases.CROWDED)
    same_lists(got, ref, "device form")
    print("candidates / path / rounds:", info[:, :3].tolist())
    assert [int(p) for p in info[:, 1]] == [1, 1, 0, 1, 1] and np.all(over == 0)


@pytest.mark.parametrize("rounds", [0, 1, 3])
@pytest.mark.parametrize("params", [cases.DEFAULTS, (0, 0.01, 8, 7)], ids=["500", "all"])
def test_images_still_open_after_the_last_round_go_to_the_walk(ctx, rounds, params):
    """The third way to the walk: fewer round launches than the images need (rounds that read only the states of the round
    before need 8 or 9 for them) leave candidates open beside decided ones; the walk starts over on its own cell counts and staging rows
    and gives the oracle's corners.  The flat image has nothing open and stays on the rounds path."""
    imgs = cases.ordinary_images()
    ref = oracle_each(imgs, None, *params)
    got, cnt, over, info = batch_dev(ctx, imgs, None, *params, call=rounds_dev(ctx, rounds, 131072))
    print("rounds %d: candidates / path / rounds used: %s" % (rounds, info[:, :3].tolist()))
    same_lists(got, ref, rounds)
    assert np.all(over == 0) and info[2, 1] == 0 and info[2, 2] == 0
    for q in (0, 1, 3, 4):
        # (how far a round gets depends on the order its workgroups ran in: an image may be finished by fewer rounds than the
        #  synchronous count; without any round it cannot be)
        assert (info[q, 1] == 1 and info[q, 2] == rounds) or (rounds > 0 and info[q, 1] == 0 and 1 <= info[q, 2] <= rounds), info[q]
    same_lists(batch_dev(ctx, imgs, None, *params)[0], ref, "the full count of rounds afterwards")


def test_more_candidates_than_the_rounds_path_holds_go_to_the_walk(ctx):
    """The second way to the walk, with the limit lowered from 131 072 to 5 200 candidates: of the ordinary images (5 082 to
    5 254 candidates, tests/test_good_features_batch_host.py) some are above it and are walked, some below and go through
    the rounds, in one call."""
    imgs = cases.ordinary_images()
    ref = oracle_each(imgs, None, *cases.DEFAULTS)
    got, cnt, over, info = batch_dev(ctx, imgs, None, *cases.DEFAULTS, call=rounds_dev(ctx, 24, 5200))
    print("candidates / path / rounds used:", info[:, :3].tolist())
    same_lists(got, ref)
    assert [int(p) for p in info[:, 1]] == [1 if c > 5200 else 0 for c in info[:, 0]]
    assert sorted(set(int(p) for p in info[:, 1])) == [0, 1] and np.all(over == 0)
    for bad in ((25, 131072), (-1, 131072), (24, 0), (24, 131073)):
        from vo import _native
        with pytest.raises(_native.VoError) as e:
            batch_dev(ctx, imgs[:1], None, *cases.DEFAULTS, call=rounds_dev(ctx, *bad))
        assert e.value.code == EINVAL, bad


def test_no_minimum_distance_takes_the_sorted_list(ctx):
    """7. min_distance 0: path 2, with and without a corner limit."""
    imgs = cases.ordinary_images()
    for n in (300, 0):
        ref = oracle_each(imgs, None, n, 0.01, 0, 7)
        got, cnt, over, info = batch_dev(ctx, imgs, None, n, 0.01, 0, 7)
        same_lists(got, ref, n)
        assert np.all(info[:, 1] == 2) and np.all(over == 0)
        same_lists(ctx.good_features_batch(imgs, None, n, 0.01, 0, 7), ref, ("host form", n))


@pytest.mark.parametrize("n,quality,min_dist,block", cases.CONFIG_SETS)
def test_four_images_at_configuration_size(ctx, n, quality, min_dist, block):
    """8. S = 4 at 1376 x 1241 with the one-image test's parameter sets."""
    imgs = cases.config_images()
    ref = oracle_each(imgs, None, n, quality, min_dist, block)
    assert all(len(r) > 400 for r in ref)
    got, cnt, over, info = batch_dev(ctx, imgs, None, n, quality, min_dist, block)
    print("candidates / path / rounds:", info[:, :3].tolist())
    same_lists(got, ref)
    assert np.all(over == 0)
    if (n, quality, min_dist, block) == cases.CONFIG_SETS[0]:
        assert np.all(info[:, 1] == 0) and np.all(info[:, 2] >= 1)


def test_workspace_is_reused_across_sizes(ctx):
    """9. two batched calls with different S and sizes on one context, then a one-image call: all still equal."""
    from scenarios import synthetic_image
    big = cases.ordinary_images()
    small = [synthetic_image(97, 131, s, block=9) for s in (5, 6, 7)]
    same_lists(ctx.good_features_batch(small, None, *cases.DEFAULTS), oracle_each(small, None, *cases.DEFAULTS), "small")
    same_lists(ctx.good_features_batch(big, None, *cases.DEFAULTS), oracle_each(big, None, *cases.DEFAULTS), "big")
    same_lists(ctx.good_features_batch(small[:2], None, *cases.CROWDED), oracle_each(small[:2], None, *cases.CROWDED), "again")
    assert np.array_equal(ctx.good_features(big[0], None, *cases.DEFAULTS), native.good_features(big[0], None, *cases.DEFAULTS))
    assert np.array_equal(ctx.good_features(small[0], None, 0, 0.01, 40, 7), native.good_features(small[0], None, 0, 0.01, 40, 7))
    same_lists(ctx.good_features_batch(big[:2], None, *cases.DEFAULTS), oracle_each(big[:2], None, *cases.DEFAULTS), "after")


def test_refused_calls_leave_the_context_usable(ctx):
    """10. S < 1, xy_stride below the capacity, block outside 1..31, quality <= 0: VO_EINVAL each, and the next call works."""
    from vo import _native
    imgs = cases.ordinary_images()[:2]
    ref = oracle_each(imgs, None, *cases.DEFAULTS)
    n, quality, min_dist, block = cases.DEFAULTS
    for kw in (dict(S=0), dict(S=-3), dict(xy_stride=n - 1), dict(block=0), dict(block=32), dict(quality=0.0),
               dict(quality=-0.5)):
        args = dict(n=n, quality=quality, min_dist=min_dist, block=block, xy_stride=None, S=None)
        args.update(kw)
        with pytest.raises(_native.VoError) as e:
            batch_dev(ctx, imgs, None, args["n"], args["quality"], args["min_dist"], args["block"], args["xy_stride"], args["S"])
        assert e.value.code == EINVAL, (kw, e.value.code)
        same_lists(batch_dev(ctx, imgs, None, *cases.DEFAULTS)[0], ref, kw)
    with pytest.raises(_native.VoError) as e:                # every corner: the capacity is the candidate capacity
        batch_dev(ctx, imgs, None, 0, quality, min_dist, block, xy_stride=cases.candidate_capacity(cases.SMALL) - 1)
    assert e.value.code == EINVAL
    for bad in (dict(block_size=0), dict(block_size=32), dict(quality=0.0)):
        with pytest.raises(_native.VoError) as e:
            ctx.good_features_batch(imgs, None, **bad)
        assert e.value.code == EINVAL, bad
    same_lists(ctx.good_features_batch(imgs, None, *cases.DEFAULTS), ref, "host form after refusals")


def test_an_image_beyond_the_candidate_capacity_fails_alone(ctx):
    """11. plateau ties (a period-3 texture under block_size 3: every interior pixel is a local maximum) exceed the candidate
    capacity of image 1: d_over 1, d_n 0, nothing of it written; its neighbours are the oracle's; the host form names it."""
    from scenarios import synthetic_image
    from vo import _native
    shape = (96, 128)
    imgs = [synthetic_image(shape[0], shape[1], 31, block=9), cases.plateau_image(shape), synthetic_image(shape[0], shape[1], 32, block=9)]
    got, cnt, over, info = batch_dev(ctx, imgs, None, *cases.PLATEAU)
    print("counts %s over %s info %s" % (cnt.tolist(), over.tolist(), info.tolist()))
    assert over.tolist() == [0, 1, 0] and cnt[1] == 0 and len(got[1]) == 0
    assert info[1, 0] > cases.candidate_capacity(shape)
    for q in (0, 2):
        assert np.array_equal(got[q], native.good_features(imgs[q], None, *cases.PLATEAU)), q
    with pytest.raises(_native.VoError, match="image 1") as e:
        ctx.good_features_batch(imgs, None, *cases.PLATEAU)
    assert e.value.code == ECAPACITY
    same_lists(ctx.good_features_batch([imgs[0], imgs[2]], None, *cases.PLATEAU),
               oracle_each([imgs[0], imgs[2]], None, *cases.PLATEAU), "after the failure")


# ---- the one-image call: the batched stages at S = 1 behind a device-wide sort of exactly the candidates the host read
# back, which no batched call reaches (the cases' counts are checked on the CPU in tests/test_good_features_batch_host.py) ----

def test_one_image_call_with_nothing_to_sort(ctx):
    """No candidate at all -- a flat image, an all-zero mask -- skips the sort: no corners, and the next call is the oracle's."""
    from scenarios import synthetic_image
    img = synthetic_image(120, 160, 1, block=9)
    for got in (ctx.good_features(cases.flat_image((96, 128)), None, *cases.DEFAULTS),
                ctx.good_features(img, np.zeros((120, 160), np.uint8), *cases.MASKED)):
        assert got.shape == (0, 2) and got.dtype == np.float32
    assert np.array_equal(ctx.good_features(img, None, *cases.DEFAULTS), native.good_features(img, None, *cases.DEFAULTS))


def test_one_image_call_over_several_workgroups_with_a_remainder(ctx):
    """1 235 candidates: three workgroups of 512 per round, the last with 211."""
    from scenarios import synthetic_image
    img = synthetic_image(240, 320, 2, block=9)
    ref = native.good_features(img, None, *cases.DEFAULTS)
    got = ctx.good_features(img, None, *cases.DEFAULTS)
    assert got.dtype == np.float32 and got.shape == ref.shape == (493, 2)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("shape,seed,params", [
    ((120, 160), 1, cases.CROWDED),          # 33 candidates in the fullest cell: prep hands the image to the walk
    ((97, 131), 3, cases.CROWDED),           # 29: it stays on the rounds
    ((120, 160), 1, (30, 0.01, 0, 7)),       # no minimum distance: the sorted list's head, cut at 30 ...
    ((120, 160), 1, (0, 0.01, 0, 7)),        # ... and whole
], ids=["walk", "rounds", "sorted-30", "sorted-all"])
def test_one_image_call_takes_every_path(ctx, shape, seed, params):
    from scenarios import synthetic_image
    img = synthetic_image(shape[0], shape[1], seed, block=9)
    ref = native.good_features(img, None, *params)
    got = ctx.good_features(img, None, *params)
    assert got.dtype == np.float32 and got.shape == ref.shape and len(ref) > 0
    assert np.array_equal(got, ref)


def test_one_image_call_beyond_the_candidate_capacity(ctx):
    """The plateau image's 11 318 maxima against a capacity of 3 136: VO_ECAPACITY in the one-image call's words, and the
    context works on."""
    from scenarios import synthetic_image
    from vo import _native
    with pytest.raises(_native.VoError) as e:
        ctx.good_features(cases.plateau_image((96, 128)), None, *cases.PLATEAU)
    assert e.value.code == ECAPACITY
    assert str(e.value).startswith("VO_ECAPACITY (-4): good_features: "), str(e.value)      # (code name, code, the library's text)
    img = synthetic_image(96, 128, 31, block=9)
    assert np.array_equal(ctx.good_features(img, None, *cases.PLATEAU), native.good_features(img, None, *cases.PLATEAU))
