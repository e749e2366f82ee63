"""-m gpu: the Shi-Tomasi kernels of csrc/goodfeatures.hip (min_eig_batch_kernel, corner_candidates_batch_kernel and the
selection stages behind Context.min_eigen_map, Context.good_features, good_features_batch and good_features_batch_dev) against
the definition of tests/good_features_reference.py, directly, on every case of tests/good_features_cases.py -- and,
separately, against the oracle bit for bit.  tests/test_good_features_reference_host.py runs the same checks on the oracle
and asserts each case's edge.  No image is larger than 64 x 80."""
import numpy as np
import pytest

import good_features_cases as gc
import good_features_reference as ref
from oracle import native
from test_gpu_good_features_batch import batch_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name,img,blocks", gc.map_cases(), ids=[c[0] for c in gc.map_cases()])
def test_kernel_map_is_within_the_rounding_bound_and_equals_the_oracle(ctx, name, img, blocks):
    """Images narrower and lower than the 64 x 16 tile and than the box (refl() passing both edges repeatedly), one row and one
    column into the next tiles, blocks 1 to 31 odd and even, gradients of +-1020 in the packed halves."""
    shares = {}
    for block in blocks:
        got = ctx.min_eigen_map(img, block)
        shares[block] = round(gc.check_map(got, img, block), 2)
        assert np.array_equal(got, native.min_eigen_map(img, block)), ("kernel and oracle maps differ in bits", block)
    print("%s: largest |kernel - lambda| / (2^-24 trace) per block (bound %d): %s" % (name, ref.KAPPA, shares))


@pytest.mark.parametrize("shape", gc.SHAPES + ("smallest",), ids=lambda s: s if isinstance(s, str) else gc.name_of(s))
def test_kernel_corners_are_the_rule_on_its_own_map(ctx, shape):
    """Shapes x blocks x parameters x masks: the corners are select() on the map the same min_eig_batch_kernel wrote --
    images without an interior, one candidate cell (min_distance 200), cells of side 1, no minimum distance, empty masks."""
    img = gc.smallest_with_a_corner() if shape == "smallest" else gc.shape_image(shape)
    calls = gc.run_select_table(str(shape), img, {b: ctx.min_eigen_map(img, b) for b in gc.BLOCKS}, ctx.good_features)
    print(shape, calls, "calls")


def test_kernel_corners_on_the_extremes(ctx):
    """The checkers, ramps and the flat image.  Plateaus of tied maxima (the 3 x 3 checker under most blocks, a ramp's
    rounding noise under wide ones) hold more local maxima than the candidate capacity H W / 4 + 64: those calls are refused
    with VO_ECAPACITY as include/vo_hip.h says, exactly those, and the context works on."""
    from vo import _native
    refused = answered = 0
    for name, img in gc.EXTREMES.items():
        cap = ctx.good_features_capacity(img.shape[0], img.shape[1], 0)
        assert cap == (img.size + 3) // 4 + 64
        for block in gc.EXTREME_BLOCKS:
            eig = ctx.min_eigen_map(img, block)
            for params in ((0, 0.01, 0), (0, 0.01, 2.5), (7, 0.5, 8)):
                if len(ref.candidates(eig, None, params[1])[0]) > cap:
                    with pytest.raises(_native.VoError) as e:
                        ctx.good_features(img, None, *params, block)
                    assert e.value.code == -4, (name, block, params)
                    refused += 1
                else:
                    gc.corners_equal_rule(ctx.good_features, eig, img, None, *params, block, (name, block, params))
                    answered += 1
    print("extremes: %d calls answered, %d refused for capacity" % (answered, refused))
    assert refused > 0 and answered > refused


@pytest.mark.parametrize("name", [s.name for s in gc.SCENES])
def test_kernel_corners_equal_the_definition_on_decided_scenes(ctx, name):
    """The corners of the definition's own float64 map, in order, four-way ties included; decided() is asserted, not used as
    a filter."""
    s = gc.SCENE_BY_NAME[name]
    assert ref.decided(s.img, s.mask, *s.params), "the case is not decided: it proves nothing"
    want = ref.select(ref.min_eig(s.img, s.params[3])[0], s.mask, *s.params[:3])
    got = ctx.good_features(s.img, s.mask, *s.params)
    assert len(want) > 0 and got.dtype == np.float32
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(got, native.good_features(s.img, s.mask, *s.params))
    if name in gc.TIE_DISTANCE:
        assert got.tolist() == [list(map(float, p)) for p in gc.TIE_DISTANCE[name]]


@pytest.mark.parametrize("batch", gc.BATCHES, ids=lambda b: b[1].name)
def test_batch_of_flat_decided_and_tie_images(ctx, batch):
    """S = 3 at 41 x 41 through both batched forms: image q's corners are the one-image call's and the definition's, bits and
    order; the flat image has none; with min_distance below 1 every image takes the sorted list's head (path 2), else not."""
    imgs, masks, params = [s.img for s in batch], [s.mask for s in batch], batch[0].params
    want = []
    for s in batch:
        assert ref.decided(s.img, s.mask, *s.params)
        want.append(ref.select(ref.min_eig(s.img, params[3])[0], s.mask, *params[:3]))
    assert [len(w) for w in want] == [0, 8, 4]
    one = [ctx.good_features(s.img, s.mask, *params) for s in batch]
    host = ctx.good_features_batch(imgs, masks, *params)
    dev, cnt, over, info = batch_dev(ctx, imgs, masks, *params)
    for q in range(3):
        for what, got in (("one image", one[q]), ("host form", host[q]), ("device form", dev[q])):
            assert got.dtype == np.float32 and np.array_equal(got, want[q]), (what, q, got.tolist(), want[q].tolist())
    assert cnt.tolist() == [0, 8, 4] and np.all(over == 0)
    assert np.all(info[:, 1] == 2) if params[2] < 1 else np.all(info[:, 1] != 2), info.tolist()
