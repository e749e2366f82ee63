"""CPU: Harris corners with sub-pixel refinement (klt.py:99-112) -- the C ABI (declared in include/vo_hip.h, exported by
the built library, bound in vo/_native.py with the argument types of the declaration), the oracle's label order and
sub-pixel step on hand-made inputs, Context.harris_subpix_corners_batch's refusal of mixed shapes, and
KLTTracker.find_corners(use_goodFeaturesToTrack=False) with a stub context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import harris_subpix_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vo_hip.h")
SYMBOLS = {
    "vo_harris_subpix_capacity": "int vo_harris_subpix_capacity(int H, int W);",
    "vo_harris_subpix_batch_dev": "int vo_harris_subpix_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, "
                                  "int S, int H, int W, int block, int ksize, double k, double rel, int win_w, int win_h, "
                                  "int max_iter, double eps, float* d_xy, size_t xy_stride, int32_t* d_n, "
                                  "float* d_response, int32_t* d_labels, double* d_centroids);",
    "vo_harris_subpix_batch": "int vo_harris_subpix_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, "
                              "int block, int ksize, double k, double rel, int win_w, int win_h, int max_iter, double eps, "
                              "float* xy, int32_t* n, float* response, int32_t* labels, double* centroids);",
    "vo_harris_subpix_corners": "int vo_harris_subpix_corners(vo_ctx* ctx, const uint8_t* img, int H, int W, int block, "
                                "int ksize, double k, double rel, int win_w, int win_h, int max_iter, double eps, "
                                "float* xy, int32_t* n, float* response, int32_t* labels, double* centroids);",
}
_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
ARGS = {
    "vo_harris_subpix_capacity": [_i, _i],
    "vo_harris_subpix_batch_dev": [_vp, _vp, _sz, _i, _i, _i, _i, _i, _d, _d, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp,
                                   _vp],
    "vo_harris_subpix_batch": [_vp, _vp, _i, _i, _i, _i, _i, _d, _d, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp],
    "vo_harris_subpix_corners": [_vp, _vp, _i, _i, _i, _i, _d, _d, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp],
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


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_header_cites_the_reference_call_site(name):
    text = open(HEADER).read()
    i = text.index("int %s(" % name)
    j = text.rfind("*/", 0, i)
    k = text.rfind("/*", 0, j)
    assert "src/vo/features/klt.py:99-112" in text[k:j]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_exported_by_the_library(name):
    from vo import _native
    path = _native.lib_path()
    if not os.path.exists(path):
        pytest.fail("libvo_hip.so is not built: %s" % path)
    lib = C.CDLL(path)
    assert getattr(lib, name, None) is not None, name


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_bound_with_the_declared_argument_types(name):
    from vo import _native
    res, args = _native._SIGS[name]
    assert res is C.c_int and args == ARGS[name]
    lib = _native.load()
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGS[name]


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (370, 1226), (1241, 1376)])
def test_capacity_is_the_block_count_plus_the_background(H, W):
    from vo import _native
    assert _native.load().vo_harris_subpix_capacity(H, W) == orc.capacity(H, W) == -(-H // 2) * -(-W // 2) + 1


# ---- the oracle's label order --------------------------------------------------------------------------------------

def _mask(H, W, pixels):
    m = np.zeros((H, W), bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def test_labels_follow_the_first_2x2_block_not_the_raster():
    # A's first pixel is (row 1, col 0): block (0, 0); B's is (row 0, col 5): block (0, 2) -- A comes first although
    # B's pixel comes first in raster order
    fg = _mask(6, 8, [(1, 0), (0, 5)])
    lab, rows = orc.label_blocks(fg)
    assert rows == 3 and lab[1, 0] == 1 and lab[0, 5] == 2
    # the same within one block row: (row 1, col 2) is block (0, 1), before (row 0, col 4), block (0, 2)
    fg = _mask(4, 8, [(1, 2), (0, 4)])
    lab, _ = orc.label_blocks(fg)
    assert lab[1, 2] == 1 and lab[0, 4] == 2


def test_diagonal_contacts_are_joined():
    fg = _mask(8, 8, [(0, 0), (1, 1), (2, 2), (3, 3), (3, 5), (2, 6), (1, 7)])
    lab, rows = orc.label_blocks(fg)
    assert rows == 3
    assert len({lab[y, x] for y, x in [(0, 0), (1, 1), (2, 2), (3, 3)]}) == 1
    assert lab[3, 5] == lab[2, 6] == lab[1, 7] != lab[0, 0]
    # the second's first block is (0, 3) (pixel (1, 7)), after the first's (0, 0)
    assert lab[0, 0] == 1 and lab[1, 7] == 2


def test_odd_sizes():
    fg = _mask(5, 7, [(4, 6), (4, 0), (0, 6)])
    lab, rows = orc.label_blocks(fg)
    assert rows == 4
    # blocks: (0, 6) -> block (0, 3); (4, 0) -> (2, 0); (4, 6) -> (2, 3)
    assert (lab[0, 6], lab[4, 0], lab[4, 6]) == (1, 2, 3)
    cen = orc.centroids(lab, rows)
    assert np.array_equal(cen[1:], [[6, 0], [0, 4], [6, 4]])


def test_u_shape_whose_arms_meet_late():
    H, W = 12, 12
    fg = np.zeros((H, W), bool)
    fg[2:10, 2] = True          # left arm
    fg[2:10, 8] = True          # right arm
    fg[9, 2:9] = True           # the bottom joins them
    fg[0, 5] = True             # a dot whose block (0, 2) comes between the arms' first blocks (1, 1) and (1, 4)
    lab, rows = orc.label_blocks(fg)
    assert rows == 3
    assert lab[0, 5] == 1 and lab[2, 2] == lab[2, 8] == lab[9, 5] == 2


def test_background_row_and_centroids():
    fg = _mask(4, 4, [(0, 0), (0, 1)])
    lab, rows = orc.label_blocks(fg)
    cen = orc.centroids(lab, rows)
    ys, xs = np.nonzero(~fg)
    assert np.array_equal(cen[0], [xs.mean(), ys.mean()]) and np.array_equal(cen[1], [0.5, 0.0])
    lab, rows = orc.label_blocks(np.ones((3, 3), bool))
    cen = orc.centroids(lab, rows)
    assert rows == 2 and np.isnan(cen[0]).all() and np.array_equal(cen[1], [1.0, 1.0])


# ---- the oracle's sub-pixel step ------------------------------------------------------------------------------------

def _smooth_corner(H, W, cx, cy, s=1.5):
    """A smooth checkerboard corner (an X-junction) at (cx, cy): its gradient field is symmetric about that point."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.clip(np.rint(128 + 100 * np.tanh((x - cx) / s) * np.tanh((y - cy) / s)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("cx,cy", [(20.3, 18.6), (24.75, 21.2)])
@pytest.mark.parametrize("off", [(-1.4, 1.1), (2.0, -1.6)])
def test_subpix_converges_to_a_smooth_corner(cx, cy, off):
    img = _smooth_corner(48, 52, cx, cy)
    out = orc.corner_subpix(img, np.array([[cx + off[0], cy + off[1]]], np.float32))
    assert np.abs(out[0] - [cx, cy]).max() < 0.05


def test_flat_window_leaves_the_point():
    img = np.full((40, 40), 90, np.uint8)
    p = np.array([[17.25, 22.5]], np.float32)
    assert np.array_equal(orc.corner_subpix(img, p), p)


def test_a_point_that_walks_away_returns_to_its_start():
    # an X-junction at (30, 20): from 6 px away the solve still finds it, a move beyond win = 5, so the start is kept;
    # from 4.5 px away the move is allowed
    img = _smooth_corner(40, 60, 30.0, 20.0, 2.0)
    p = np.array([[24.0, 20.0]], np.float32)
    out, raw = orc.corner_subpix(img, p, win=(5, 5), want_raw=True)
    assert abs(raw[0, 0] - 30.0) < 0.05 and np.array_equal(out, p)
    out = orc.corner_subpix(img, np.array([[25.5, 20.0]], np.float32), win=(5, 5))
    assert abs(out[0, 0] - 30.0) < 0.05


def test_subpix_refuses_images_below_the_window():
    with pytest.raises(ValueError):
        orc.corner_subpix(np.zeros((14, 40), np.uint8), np.zeros((1, 2), np.float32), win=(5, 5))


# ---- Python surface -------------------------------------------------------------------------------------------------

class _StubLib:
    def __init__(self):
        self.calls = []

    def vo_harris_subpix_capacity(self, H, W):
        return orc.capacity(H, W)

    def vo_harris_subpix_batch(self, *a):
        self.calls.append(("vo_harris_subpix_batch",) + tuple(a[2:5]))
        return 0


def _stub_context():
    from vo import _native
    ctx = _native.Context.__new__(_native.Context)
    ctx._lib, ctx._h = _StubLib(), None
    return ctx


@pytest.mark.parametrize("images", [
    [np.zeros((32, 40), np.uint8), np.zeros((32, 41), np.uint8)],
    [np.zeros((32, 40), np.uint8), np.zeros((32, 40, 1), np.uint8)],
    [],
])
def test_batch_refuses_mixed_shapes_before_any_library_call(images):
    ctx = _stub_context()
    with pytest.raises(ValueError):
        ctx.harris_subpix_corners_batch(images)
    assert ctx._lib.calls == []


def test_criteria_resolve_as_cornersubpix_does():
    from vo import _native
    f = _native.Context._subpix_criteria
    assert f((3, 100, 0.001)) == (100, 0.001)
    assert f((1, 30, 0.5)) == (30, 0.0)           # COUNT only: no epsilon
    assert f((2, 7, 0.01)) == (100, 0.01)         # EPS only: 100 iterations
    assert f((3, 0, 0.01)) == (1, 0.01) and f((3, 500, 0.01)) == (100, 0.01)


class _StubContext:
    def __init__(self, n=7):
        self.calls = []
        self.n = n

    def good_features(self, img, mask, *a):
        return np.zeros((3, 2), np.float32)

    def harris_subpix_corners(self, img, **kw):
        self.calls.append((img.shape, img.dtype, kw))
        return np.arange(self.n * 2, dtype=np.float32).reshape(self.n, 2)


def test_find_corners_runs_the_harris_subpix_branch():
    from vo.features.klt import KLTTracker
    from vo.primitives import Frame
    ctx = _StubContext(7)
    frame = Frame(np.zeros((30, 40, 3), np.uint8))
    tracker = KLTTracker(frame, context=ctx)
    assert tracker._num_features == 3                         # the default branch ran in the constructor
    pts = tracker.find_corners(frame, mask=np.zeros((30, 40), np.uint8), use_goodFeaturesToTrack=False)
    assert pts.shape == (7, 2, 1) and pts.dtype == np.float32
    assert np.array_equal(pts[:, :, 0], np.arange(14, dtype=np.float32).reshape(7, 2))
    assert tracker._num_features == 7
    (shape, dtype, kw), = ctx.calls
    assert shape == (30, 40) and dtype == np.uint8           # the grey image; the mask is not passed on
    assert kw == dict(block_size=2, ksize=3, k=0.04, rel_threshold=0.01, win=(5, 5), criteria=(3, 100, 0.001))
    assert KLTTracker._harris_subpix_params == kw
