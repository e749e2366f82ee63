"""CPU: the C ABI of batched Shi-Tomasi (vo_good_features_capacity / _batch_dev / _batch) -- declared in include/vo_hip.h,
exported by the built library, bound in vo/_native.py with the declaration's argument types -- Context.good_features_batch's
argument checks before any library call, and the preconditions of the images tests/test_gpu_good_features_batch.py and
tests/test_gpu_bootstrap_lanes_corners.py run on the device (computed with the CPU oracle), so that "both paths ran" there
is a statement about the inputs and not an accident."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import good_features_batch_cases as cases
from oracle import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vo_hip.h")
SYMBOLS = {
    "vo_good_features_capacity": "int vo_good_features_capacity(int H, int W, int max_corners);",
    "vo_good_features_batch_dev": "int vo_good_features_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, "
                                  "int H, int W, const uint8_t* d_masks, size_t mask_stride, int max_corners, double quality, "
                                  "double min_dist, int block, float* d_xy, size_t xy_stride, int32_t* d_n, int32_t* d_over, "
                                  "int32_t* d_info);",
    "vo_good_features_batch": "int vo_good_features_batch(vo_ctx* ctx, const uint8_t* imgs, const uint8_t* masks, int S, int H, "
                              "int W, int max_corners, double quality, double min_dist, int block, float* xy, int32_t* n);",
}
_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
ARGS = {
    "vo_good_features_capacity": [_i, _i, _i],
    "vo_good_features_batch_dev": [_vp, _vp, _sz, _i, _i, _i, _vp, _sz, _i, _d, _d, _i, _vp, _sz, _vp, _vp, _vp],
    "vo_good_features_batch": [_vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _i, _vp, _vp],
}


def _declaration(text, name):
    """The declaration of `name` in the header with comments removed and whitespace squashed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"int\s+%s\s*\([^;]*\)\s*;" % name, text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(0)).replace("( ", "(").replace(" )", ")").replace(" ,", ",").strip()


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_declared_in_the_header(name):
    assert _declaration(open(HEADER).read(), name) == SYMBOLS[name]


def test_header_cites_the_reference_call_site():
    text = open(HEADER).read()
    i = text.index("int vo_good_features_batch_dev(")
    section = text.rindex("/* ---- ", 0, i)
    assert "Shi-Tomasi" in text[section:section + 80]
    assert "klt.py:98" in text[section:i]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_exported_by_the_library(name):
    from vo import _native
    path = _native.lib_path()
    if not os.path.exists(path):
        pytest.fail("libvo_hip.so is not built: %s" % path)
    lib = C.CDLL(path)
    assert getattr(lib, name, None) is not None, name       # (dlsym: the dynamic symbol table has it)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_bound_with_the_declared_argument_types(name):
    from vo import _native
    res, args = _native._SIGS[name]
    assert res is C.c_int and args == ARGS[name]
    fn = getattr(_native.load(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGS[name]


def test_capacity_is_the_one_image_rule():
    """max_corners rows, or the candidate capacity H*W/4 + 64 when every corner is kept (no GPU needed: host arithmetic)."""
    from vo import _native
    lib = _native.load()
    assert lib.vo_good_features_capacity(480, 640, 500) == 500
    assert lib.vo_good_features_capacity(480, 640, 0) == cases.candidate_capacity((480, 640))
    assert lib.vo_good_features_capacity(1241, 1376, -1) == cases.candidate_capacity((1241, 1376))
    assert lib.vo_good_features_capacity(97, 131, 0) == (97 * 131 + 3) // 4 + 64
    assert lib.vo_good_features_capacity(0, 640, 0) == 0


class _StubLib:
    def __init__(self):
        self.calls = []

    def vo_good_features_capacity(self, H, W, n):
        self.calls.append("vo_good_features_capacity")
        return n if n > 0 else (H * W + 3) // 4 + 64

    def vo_good_features_batch(self, h, imgs, masks, S, H, W, n, q, md, block, xy, cnt):
        self.calls.append(("vo_good_features_batch", S, H, W, n, masks is not None))
        return 0


def _stub_context():
    from vo import _native
    ctx = _native.Context.__new__(_native.Context)
    ctx._lib, ctx._h = _StubLib(), None
    return ctx


@pytest.mark.parametrize("images,masks", [
    ([np.zeros((32, 40), np.uint8), np.zeros((32, 41), np.uint8)], None),
    ([np.zeros((32, 40, 1), np.uint8)] * 2, None),
    ([], None),
    ([np.zeros((32, 40), np.uint8)] * 2, [None]),
    ([np.zeros((32, 40), np.uint8)] * 2, [None, np.zeros((32, 41), np.uint8)]),
])
def test_good_features_batch_refuses_before_any_library_call(images, masks):
    ctx = _stub_context()
    with pytest.raises(ValueError):
        ctx.good_features_batch(images, masks)
    assert ctx._lib.calls == []


def test_good_features_batch_passes_the_batch_in_one_call():
    ctx = _stub_context()
    out = ctx.good_features_batch(np.zeros((3, 32, 40), np.uint8), max_corners=50)
    assert ctx._lib.calls == ["vo_good_features_capacity", ("vo_good_features_batch", 3, 32, 40, 50, False)]
    assert len(out) == 3 and all(a.shape == (0, 2) and a.dtype == np.float32 for a in out)
    ctx = _stub_context()
    ctx.good_features_batch([np.zeros((32, 40), np.uint8)] * 2, [None, np.ones((32, 40), np.uint8)], max_corners=0)
    assert ctx._lib.calls[-1] == ("vo_good_features_batch", 2, 32, 40, 0, True)
    ctx = _stub_context()
    ctx.good_features_batch([np.zeros((32, 40), np.uint8)] * 2, [None, None])      # no mask at all: none is passed
    assert ctx._lib.calls[-1] == ("vo_good_features_batch", 2, 32, 40, 500, False)


# ---- the GPU tests' images are what they claim ----

def test_ordinary_images_have_no_crowded_cell_and_the_flat_one_no_corner():
    n, quality, min_dist, block = cases.DEFAULTS
    imgs = cases.ordinary_images()
    assert len(imgs) == 5 and all(a.shape == cases.SMALL for a in imgs)
    for q, img in enumerate(imgs):
        take = cases.local_maxima(img, None, quality, block)
        corners = native.good_features(img, None, n, quality, min_dist, block)
        print("image %d: %d candidates, at most %d per cell, %d corners" % (
            q, int(take.sum()), cases.max_per_cell(take, min_dist), len(corners)))
        if q == 2:
            assert len(corners) == 0 and take.sum() == 0
            continue
        assert 0 < cases.max_per_cell(take, min_dist) <= cases.CELL_LIST
        assert take.sum() <= 131072                       # (the rounds path's candidate limit)
        assert len(corners) >= 8
    assert len({a.tobytes() for a in imgs}) == 5


def test_masked_images_keep_candidates_inside_their_masks():
    n, quality, min_dist, block = cases.MASKED
    for q, (img, mask) in enumerate(zip(cases.ordinary_images(), cases.masks_for())):
        corners = native.good_features(img, mask, n, quality, min_dist, block)
        if q == 2:
            assert len(corners) == 0
            continue
        assert len(corners) >= 8
        if mask is not None:
            assert np.all(mask[corners[:, 1].astype(int), corners[:, 0].astype(int)] != 0)
            assert not np.array_equal(corners, native.good_features(img, None, n, quality, min_dist, block))


def test_crowded_case_has_a_cell_beyond_the_cell_lists():
    n, quality, min_dist, block = cases.CROWDED
    imgs = cases.ordinary_images()
    crowded = [cases.max_per_cell(cases.local_maxima(img, None, quality, block), min_dist) for img in imgs]
    print("candidates in the fullest cell of side %d: %s" % (min_dist, crowded))
    assert all(c > cases.CELL_LIST for q, c in enumerate(crowded) if q != 2) and crowded[2] == 0


def test_configuration_images_are_ordinary_at_the_bootstraps_parameters():
    n, quality, min_dist, block = cases.CONFIG_SETS[0]
    for img in cases.config_images():
        take = cases.local_maxima(img, None, quality, block)
        assert cases.max_per_cell(take, min_dist) <= cases.CELL_LIST and 0 < take.sum() <= 131072
        assert len(native.good_features(img, None, n, quality, min_dist, block)) > 400


def test_rounds_of_the_batched_call_cover_the_test_images():
    """The rule as rounds, each reading only the round before (the most rounds the device can need), gives the oracle's corners
    and settles the ordinary images and a configuration frame inside the batched call's round launches -- what the GPU
    test's "path 0" for them rests on.  The counts are printed: DESIGN 3.6 quotes them."""
    todo = [("480x640 image %d" % q, img, cases.DEFAULTS) for q, img in enumerate(cases.ordinary_images())]
    todo += [("480x640 image %d, every corner" % q, img, (0, 0.01, 8, 7)) for q, img in enumerate(cases.ordinary_images()[:2])]
    todo.append(("1376x1241 image 0", cases.config_images()[0], cases.CONFIG_SETS[0]))
    for name, img, params in todo:
        rounds, candidates, corners = cases.synchronous_rounds(img, None, *params)
        print("%s %s: %d candidates settle in %d synchronous rounds" % (name, params, candidates, rounds))
        assert np.array_equal(corners, native.good_features(img, None, *params)), name
        assert rounds <= cases.ROUNDS, (name, rounds)


def test_plateau_image_exceeds_the_candidate_capacity():
    n, quality, min_dist, block = cases.PLATEAU
    img = cases.plateau_image()
    take = cases.local_maxima(img, None, quality, block)
    print("plateau: %d local maxima, capacity %d" % (int(take.sum()), cases.candidate_capacity(img.shape)))
    assert take.sum() > cases.candidate_capacity(img.shape)


def test_one_image_call_cases_are_what_they_claim():
    """The images of the GPU tests of the one-image call (the sort the host sizes): nothing to sort, a candidate count that
    is no multiple of a workgroup, a cell on either side of the cell lists' length, the sorted list's head."""
    from scenarios import synthetic_image
    img = synthetic_image(120, 160, 1, block=9)
    n, quality, min_dist, block = cases.DEFAULTS
    flat = cases.flat_image((96, 128))
    assert cases.local_maxima(flat, None, quality, block).sum() == 0 and len(native.good_features(flat, None, *cases.DEFAULTS)) == 0
    empty = np.zeros((120, 160), np.uint8)
    assert cases.local_maxima(img, empty, cases.MASKED[1], cases.MASKED[3]).sum() == 0
    assert len(native.good_features(img, empty, *cases.MASKED)) == 0
    mid = synthetic_image(240, 320, 2, block=9)
    assert cases.local_maxima(mid, None, quality, block).sum() == 1235 == 2 * 512 + 211
    assert len(native.good_features(mid, None, *cases.DEFAULTS)) == 493
    n, quality, min_dist, block = cases.CROWDED
    small = synthetic_image(97, 131, 3, block=9)
    assert cases.max_per_cell(cases.local_maxima(img, None, quality, block), min_dist) == 33 > cases.CELL_LIST
    assert cases.max_per_cell(cases.local_maxima(small, None, quality, block), min_dist) == 29 <= cases.CELL_LIST
    assert len(native.good_features(img, None, *cases.CROWDED)) == 9 and len(native.good_features(small, None, *cases.CROWDED)) == 8
    assert len(native.good_features(img, None, 30, 0.01, 0, 7)) == 30 and len(native.good_features(img, None, 0, 0.01, 0, 7)) == 310
    plateau = cases.plateau_image((96, 128))
    assert cases.local_maxima(plateau, None, cases.PLATEAU[1], cases.PLATEAU[3]).sum() == 11318
    assert cases.candidate_capacity((96, 128)) == 3136


def test_bootstrap_frames_yield_eight_corners():
    """Frame a of every lane of the 4-lane bootstrap test: at least 8 corners, and four different scenes."""
    from test_gpu_pipeline_bootstrap import SMALL, boot_kwargs
    from test_gpu_pipeline_bootstrap_lanes import lane_data
    data = lane_data(SMALL, 4)
    counts = [len(native.good_features(d["img0"], None, boot_kwargs(SMALL)["max_corners"], 0.01, 8, 7)) for d in data]
    print("corners on frame a:", counts)
    assert all(c >= 8 for c in counts)
    assert len({d["img0"].tobytes() for d in data}) == 4
