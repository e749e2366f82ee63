"""GPU: Harris corners with sub-pixel refinement (vo_harris_subpix_*, klt.py:99-112) against the NumPy oracle
(tests/harris_subpix_oracle.py).  Response, labels, row count and centroids are bit-exact; refined corners differ only by
the order of the double sums of cornerSubPix's normal equations."""
import os

import numpy as np
import pytest

import harris_subpix_oracle as orc
from scenarios import synthetic_image

pytestmark = pytest.mark.gpu

TOL, TIGHT = 2e-3, 1e-4


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kitti():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_frames.npz"))
    return {k: g[k] for k in sorted(g.files)}


def _big():
    return synthetic_image(1241, 1376, 11)


def _edge_rows(ref, img, win, tol=TOL):
    """Rows whose oracle outcome sits within `tol` of a decision edge: the revert-to-start bound (the point before that
    rule, against the start) or the image border (where the solve stops)."""
    H, W = img.shape
    start = ref["centroids"].astype(np.float32).astype(np.float64)
    raw = ref["raw"].astype(np.float64)
    d = np.abs(raw - start)
    near_bound = (np.abs(d[:, 0] - win[0]) < tol) | (np.abs(d[:, 1] - win[1]) < tol)
    near_border = (np.abs(raw[:, 0]) < tol) | (np.abs(raw[:, 0] - W) < tol) | (np.abs(raw[:, 1]) < tol) | (
        np.abs(raw[:, 1] - H) < tol)
    return near_bound | near_border


def _check_points(got, ref, img, win=(5, 5)):
    """The tolerance rule; returns the number of decision-edge rows."""
    exp = ref["xy"]
    assert got.shape == exp.shape and got.dtype == np.float32
    nan_g, nan_e = np.isnan(got), np.isnan(exp)
    assert np.array_equal(nan_g, nan_e)
    ok = ~nan_e.any(axis=1)
    diff = np.abs(got[ok].astype(np.float64) - exp[ok]).max(axis=1) if ok.any() else np.zeros(0)
    edge = _edge_rows(ref, img, win)[ok]
    bad = (diff > TOL) & ~edge
    assert not bad.any(), "rows %s differ by %s" % (np.nonzero(bad)[0][:10], diff[bad][:10])
    if diff.size:
        assert np.mean(diff <= TIGHT) >= 0.99, "only %.4f of rows within %g" % (np.mean(diff <= TIGHT), TIGHT)
    return int(edge.sum())


def _check_stages(img, got, st, ref):
    assert np.array_equal(st["response"], ref["response"]), "response differs"
    assert np.array_equal(st["labels"] > 0, ref["fg"]), "foreground differs"
    assert np.array_equal(st["labels"], ref["labels"]), "labels differ"
    assert got.shape[0] == ref["rows"]
    assert np.array_equal(st["centroids"], ref["centroids"], equal_nan=True), "centroids differ"


@pytest.mark.parametrize("shape,seed", [((64, 80), 1), ((241, 319), 2), ((480, 640), 3)])
def test_stages_and_points_equal_the_oracle_synthetic(ctx, shape, seed):
    img = synthetic_image(shape[0], shape[1], seed)
    got, st = ctx.harris_subpix_corners(img, stages=True)
    ref = orc.harris_subpix(img)
    _check_stages(img, got, st, ref)
    n_edge = _check_points(got, ref, img)
    print("%s: %d rows, %d at a decision edge" % (shape, got.shape[0], n_edge))


def test_stages_and_points_equal_the_oracle_kitti(ctx, kitti):
    for name, img in kitti.items():
        got, st = ctx.harris_subpix_corners(img, stages=True)
        ref = orc.harris_subpix(img)
        _check_stages(img, got, st, ref)
        n_edge = _check_points(got, ref, img)
        print("%s %s: %d rows, %d at a decision edge" % (name, img.shape, got.shape[0], n_edge))


def test_stages_and_points_equal_the_oracle_configuration_size(ctx):
    img = _big()
    got, st = ctx.harris_subpix_corners(img, stages=True)
    ref = orc.harris_subpix(img)
    _check_stages(img, got, st, ref)
    n_edge = _check_points(got, ref, img)
    print("1241x1376: %d rows, %d at a decision edge" % (got.shape[0], n_edge))


@pytest.mark.parametrize("S", [1, 4, 16])
def test_batch_equals_single_calls_with_padded_strides(ctx, S):
    H, W = 183, 245
    imgs = np.stack([synthetic_image(H, W, 100 + q) for q in range(S)])
    singles = [ctx.harris_subpix_corners(imgs[q], stages=True) for q in range(S)]
    host = ctx.harris_subpix_corners_batch(imgs, stages=True)
    for (p, st), (bp, bst) in zip(singles, host):
        assert np.array_equal(p, bp, equal_nan=True)
        for key in ("response", "labels", "centroids"):
            assert np.array_equal(st[key], bst[key], equal_nan=True), key
    # the device form with padded strides
    cap = ctx.harris_subpix_capacity(H, W)
    img_stride, xy_stride = H * W + 173, cap + 9
    buf = np.zeros((S, img_stride), np.uint8)
    buf[:, : H * W] = imgs.reshape(S, -1)
    d_img = ctx.to_device(buf)
    d_xy = ctx.alloc(S * xy_stride * 8)
    d_n = ctx.alloc(S * 4)
    d_resp, d_lab, d_cen = ctx.alloc(S * H * W * 4), ctx.alloc(S * H * W * 4), ctx.alloc(S * xy_stride * 16)
    try:
        ctx.harris_subpix_batch_dev(d_img, img_stride, S, H, W, d_xy, xy_stride, d_n, d_response=d_resp, d_labels=d_lab,
                                    d_centroids=d_cen)
        ctx.sync()
        n = ctx.download(d_n, (S,), np.int32)
        xy = ctx.download(d_xy, (S, xy_stride, 2), np.float32)
        resp = ctx.download(d_resp, (S, H, W), np.float32)
        lab = ctx.download(d_lab, (S, H, W), np.int32)
        cen = ctx.download(d_cen, (S, xy_stride, 2), np.float64)
    finally:
        for p in (d_img, d_xy, d_n, d_resp, d_lab, d_cen):
            ctx.free(p)
    for q, (p, st) in enumerate(singles):
        assert n[q] == p.shape[0]
        assert np.array_equal(xy[q, : n[q]], p, equal_nan=True)
        assert np.array_equal(resp[q], st["response"]) and np.array_equal(lab[q], st["labels"])
        assert np.array_equal(cen[q, : n[q]], st["centroids"], equal_nan=True)


def test_non_reference_parameters(ctx):
    img = synthetic_image(200, 260, 21)
    kw = dict(block_size=3, k=0.06, rel_threshold=0.05, win=(3, 4), criteria=(1, 30, 0.5))
    got, st = ctx.harris_subpix_corners(img, stages=True, **kw)
    ref = orc.harris_subpix(img, block=3, k=0.06, rel=0.05, win=(3, 4), max_iter=30, eps=0.0)
    _check_stages(img, got, st, ref)
    _check_points(got, ref, img, win=(3, 4))


def test_flat_image_gives_the_background_row_unchanged(ctx):
    H, W = 37, 50
    got, st = ctx.harris_subpix_corners(np.full((H, W), 77, np.uint8), stages=True)
    assert got.shape == (1, 2)
    assert np.array_equal(got[0], np.array([(W - 1) / 2, (H - 1) / 2], np.float32))
    assert not st["labels"].any() and not st["response"].any()


def test_refusals_leave_the_context_usable(ctx):
    from vo import _native
    img = synthetic_image(64, 64, 5)
    good = ctx.harris_subpix_corners(img)
    for kw in (dict(ksize=5), dict(block_size=0)):
        with pytest.raises(_native.VoError):
            ctx.harris_subpix_corners(img, **kw)
        assert np.array_equal(ctx.harris_subpix_corners(img), good, equal_nan=True)
    with pytest.raises(_native.VoError):
        ctx.harris_subpix_corners(img[:14, :40])                  # below 2 * 5 + 5 rows
    assert np.array_equal(ctx.harris_subpix_corners(img), good, equal_nan=True)
    H, W = img.shape
    d_img = ctx.to_device(img)
    d_xy, d_n = ctx.alloc(ctx.harris_subpix_capacity(H, W) * 8), ctx.alloc(4)
    try:
        with pytest.raises(_native.VoError):
            ctx.harris_subpix_batch_dev(d_img, H * W, 0, H, W, d_xy, ctx.harris_subpix_capacity(H, W), d_n)
    finally:
        for p in (d_img, d_xy, d_n):
            ctx.free(p)
    assert np.array_equal(ctx.harris_subpix_corners(img), good, equal_nan=True)


def test_find_corners_branch_on_a_kitti_frame(ctx, kitti):
    from vo.features.klt import KLTTracker
    from vo.primitives import Frame
    img = next(iter(kitti.values()))
    frame = Frame(img)
    tracker = KLTTracker(frame, context=ctx)
    pts = tracker.find_corners(frame, use_goodFeaturesToTrack=False)
    ref = orc.harris_subpix(img)
    assert pts.shape == (ref["rows"], 2, 1) and pts.dtype == np.float32
    assert tracker._num_features == ref["rows"]
    _check_points(pts[:, :, 0], ref, img)
