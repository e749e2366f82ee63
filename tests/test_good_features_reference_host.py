"""The oracle's Shi-Tomasi detector (oracle/csrc/goodfeatures.c) against the definition of tests/good_features_reference.py on
the cases of tests/good_features_cases.py; no GPU.  The kernels equal the oracle bit for bit (the GPU tests assert it), so a
mistake the two share -- a Sobel tap, the scale, an even box's anchor, a border rule, the side of a comparison -- shows only
here and in tests/test_gpu_good_features_reference.py, which runs the same checks on the kernels."""
import numpy as np
import pytest

import good_features_cases as gc
import good_features_reference as ref
from oracle import native

MAP = native.min_eigen_map              # (what the checks run on: a mutated copy of the oracle must fail them)
CORNERS = native.good_features


# ---- the definition against plainer statements of itself ---------------------------------------------------------------------
def test_reflect101_is_numpys_reflect():
    for n in (1, 2, 3, 5, 9):
        i = np.arange(-40, 40 + n)
        want = np.pad(np.arange(n), 40, mode="reflect") if n > 1 else np.zeros(len(i), np.int64)
        assert np.array_equal(ref.reflect101(i, n), want), n


@pytest.mark.parametrize("shape,block", [((1, 1), 3), ((2, 5), 4), ((5, 4), 7), ((6, 7), 2), ((7, 6), 31), ((9, 8), 1)])
def test_sums_are_the_plain_double_loop(shape, block):
    """Sobel by its nine taps and the box by its block^2 terms, borders by np.pad's reflect (reflect-101, repeated)."""
    img = gc.texture(shape, 5)
    H, W = shape
    pad = (lambda a, n: np.pad(a, n, mode="reflect")) if min(shape) > 1 else None
    if pad is None:                                                        # (NumPy refuses to reflect a side of 1)
        pad = lambda a, n: a[ref.reflect101(np.arange(-n, H + n), H)][:, ref.reflect101(np.arange(-n, W + n), W)]
    p = pad(img.astype(np.int64), 1)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    gx, gy = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    for y in range(H):
        for x in range(W):
            gx[y, x] = (p[y:y + 3, x:x + 3] * kx).sum()
            gy[y, x] = (p[y:y + 3, x:x + 3] * kx.T).sum()
    assert np.array_equal(ref.sobel(img)[0], gx) and np.array_equal(ref.sobel(img)[1], gy)
    r0 = block // 2
    for got, prod in zip(ref.tensor_sums(img, block), (gx * gx, gx * gy, gy * gy)):
        e = pad(prod, block)
        for y in range(H):
            for x in range(W):                                             # window [-(block//2), block-1-block//2]
                assert got[y, x] == e[y + block - r0:y + 2 * block - r0, x + block - r0:x + 2 * block - r0].sum()


def test_min_eig_is_the_smaller_eigenvalue():
    """Against LAPACK on s^2 [[Sxx, Sxy], [Sxy, Syy]] = [[2a, b], [b, 2c]] in the code's notation, whose smaller eigenvalue is
    (a + c) - sqrt((a - c)^2 + b^2); LAPACK's own error is relative to the trace, not to lambda."""
    img = gc.shape_image((33, 47))
    for block in (1, 3, 8):
        Sxx, Sxy, Syy = ref.tensor_sums(img, block)
        lam, trace = ref.min_eig(img, block)
        s2 = ref.scale(block) ** 2
        M = np.stack([np.stack([Sxx, Sxy], -1), np.stack([Sxy, Syy], -1)], -2).astype(np.float64) * s2
        assert np.allclose(trace, (M[..., 0, 0] + M[..., 1, 1]) / 2, rtol=1e-15, atol=0)
        assert np.all(np.abs(np.linalg.eigvalsh(M)[..., 0] - lam) <= 1e-14 * trace + 1e-300)
        assert np.all(lam >= 0) and np.all(lam <= trace)


def test_select_on_hand_made_maps():
    """The rule's sides, one at a time, on maps small enough to read."""
    z = np.zeros((5, 7), np.float32)
    m = z.copy()
    m[2, 2], m[2, 4] = 4, 2
    assert ref.select(m, None, 0, 0.5, 0).tolist() == [[2, 2]]                     # 2 is not > 0.5 * 4
    assert ref.select(m, None, 0, 0.49, 0).tolist() == [[2, 2], [4, 2]]
    assert ref.select(m, None, 0, 0.49, 2).tolist() == [[2, 2], [4, 2]]            # distance 2 is not < 2
    assert ref.select(m, None, 0, 0.49, 2.01).tolist() == [[2, 2]]
    assert ref.select(m, None, 1, 0.49, 0).tolist() == [[2, 2]] and ref.select(m, None, -1, 0.49, 0).shape == (2, 2)
    m[2, 4] = 4
    assert ref.select(m, None, 0, 0.5, 0).tolist() == [[4, 2], [2, 2]]             # a tie: the higher address first
    m[2, 3] = 4
    assert ref.select(m, None, 0, 0.5, 0.99).tolist() == [[4, 2], [3, 2], [2, 2]]  # a plateau: all kept; below 1 no test
    assert ref.select(m, None, 0, 0.5, 1).tolist() == [[4, 2], [3, 2], [2, 2]] and ref.select(m, None, 0, 0.5, 1.01).tolist() == [[4, 2], [2, 2]]
    b = z.copy()
    b[0, 3], b[2, 3], b[3, 6] = 9, 1, 5                                              # border pixels: in the maximum, never kept
    assert ref.select(b, None, 0, 0.1, 0).tolist() == [[3, 2]] and ref.select(b, None, 0, 0.12, 0).tolist() == []
    mask = np.ones((5, 7), np.uint8)
    mask[0, 3] = 0
    assert ref.select(b, mask, 0, 0.19, 0).tolist() == [[3, 2]] and ref.select(b, mask, 0, 0.2, 0).tolist() == []
    b[1, 3] = 3                                  # a forbidden neighbour still counts in the 3 x 3 maximum
    mask[1, 3] = 0
    assert ref.select(b, mask, 0, 0.01, 0).tolist() == []
    assert ref.select(b.astype(np.float64), mask * 0, 0, 0.01, 0).shape == (0, 2)
    # the threshold's rounding: float32 of the float64 product
    t = z.copy()
    t[2, 2], t[2, 5] = np.float32(1) + np.float32(2.0 ** -23), np.float32(0.1)
    assert ref.threshold(t, None, 0.1) == np.float32(np.float64(t[2, 2]) * 0.1) and ref.threshold(t.astype(np.float64), None, 0.1) == np.float64(t[2, 2]) * 0.1


# ---- the map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,img,blocks", gc.map_cases(), ids=[c[0] for c in gc.map_cases()])
def test_oracle_map_is_within_the_rounding_bound(name, img, blocks):
    """|oracle - lambda| <= KAPPA 2^-24 trace at every pixel, exactly 0 where the sums are 0; and the oracle's bits are the
    float32 formula on the definition's sums, so the bound's premises (one conversion, one product, * 0.5, the five
    operations of the root form) are the code's."""
    shares = {}
    for block in blocks:
        got = MAP(img, block)
        shares[block] = round(gc.check_map(got, img, block), 2)
        assert np.array_equal(got, gc.float32_formula(img, block)), block
    print("%s: largest |oracle - lambda| / (2^-24 trace) per block (bound %d): %s" % (name, ref.KAPPA, shares))


def test_extremes_are_what_they_claim():
    """A period-1 checker has no Sobel response at all; 3 x 3 cells of 0 / 255 reach +-1020 in both gradients; a ramp is rank
    one away from borders and clipping (lambda = 0 exactly while the trace is not: the code's value there is rounding alone,
    and not always 0); a flat image is 0."""
    for name in ("checker1_20x21", "flat_20x20"):
        gx, gy = ref.sobel(gc.EXTREMES[name])
        assert not gx.any() and not gy.any()
        for block in gc.EXTREME_BLOCKS:
            assert not MAP(gc.EXTREMES[name], block).any()
            assert CORNERS(gc.EXTREMES[name], None, 0, 0.01, 0, block).shape == (0, 2)
    gx, gy = ref.sobel(gc.EXTREMES["checker3_24x27"])
    assert {int(gx.min()), int(gx.max()), int(gy.min()), int(gy.max())} == {-1020, 1020}
    noise = 0
    for name, img in gc.EXTREMES.items():
        if name.startswith("ramp"):
            for block in gc.EXTREME_BLOCKS[:-1]:
                lam, trace = ref.min_eig(img, block)
                inner = gc.ramp_interior(img, block)
                assert inner.sum() > 100 and np.all(lam[inner] == 0) and np.all(trace[inner] > 0)
                noise += int(np.count_nonzero(MAP(img, block)[inner]))
    assert noise > 0


# ---- the selection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gc.SHAPES + ("smallest",), ids=lambda s: s if isinstance(s, str) else gc.name_of(s))
def test_oracle_corners_are_the_rule_on_its_own_map(shape):
    img = gc.smallest_with_a_corner() if shape == "smallest" else gc.shape_image(shape)
    calls = gc.run_select_table(str(shape), img, {b: MAP(img, b) for b in gc.BLOCKS}, CORNERS)
    print(shape, calls, "calls")


def test_oracle_corners_on_the_extremes():
    for name, img in gc.EXTREMES.items():
        for block in gc.EXTREME_BLOCKS:
            for params in ((0, 0.01, 0), (0, 0.01, 2.5), (7, 0.5, 8)):
                gc.corners_equal_rule(CORNERS, MAP(img, block), img, None, *params, block, (name, block, params))


# ---- decided scenes and ties: the corners of the definition's own map ------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in gc.SCENES])
def test_oracle_corners_equal_the_definition_on_decided_scenes(name):
    s = gc.SCENE_BY_NAME[name]
    report = {}
    assert ref.decided(s.img, s.mask, *s.params, report=report), "the case is not decided: it proves nothing"
    lam, trace = ref.min_eig(s.img, s.params[3])
    want = ref.select(lam, s.mask, *s.params[:3])
    got = CORNERS(s.img, s.mask, *s.params)
    print(name, "corners", len(want), "kept", report["kept"], "smallest distance to the threshold / bound %.0f" % report["threshold_margin"],
          "smallest ordering difference / bounds %.0f" % report["order_margin"])
    assert len(want) > 0 and got.dtype == np.float32
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("block", gc.TIE_BLOCKS)
def test_four_way_tie_comes_back_by_address(block):
    """The centred square's four corner maxima: one value (bit-equal in the oracle's map), mirror images of each other,
    returned bottom-right, bottom-left, top-right, top-left."""
    img = gc.tie_image()
    got = CORNERS(img, None, *gc.TIE_PARAMS, block)
    assert got.shape == (4, 2)
    x0, y0 = (int(v) for v in got[3])
    far = gc.TIE_SIDE - 1
    assert x0 == y0 and got.tolist() == [[far - x0, far - y0], [x0, far - y0], [far - x0, y0], [x0, y0]]
    if block == 3:
        assert got.tolist() == [list(map(float, p)) for p in gc.TIE_BLOCK3]
    key = ref.tie_key(img, block)
    m = MAP(img, block)
    assert len({tuple(key[int(y), int(x)]) for x, y in got}) == 1 and len({m[int(y), int(x)].tobytes() for x, y in got}) == 1
    for name, want in gc.TIE_DISTANCE.items():
        s = gc.SCENE_BY_NAME[name]
        assert CORNERS(s.img, None, *s.params).tolist() == [list(map(float, p)) for p in want], name


# ---- metamorphic, bit for bit on the map -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 65), (33, 47), (5, 9), (20, 20), (3, 64)], ids=gc.name_of)
def test_map_under_transposition_inversion_and_mirrors(shape):
    """Transposition trades Sxx and Syy, inversion negates both gradients, a mirror negates one: a + c, (a - c)^2 and b * b
    keep their bits.  An odd box is its own mirror image; an even box [-(b/2), b/2 - 1] mirrors into [-(b/2 - 1), b/2], the
    box of the next pixel, wherever neither box reaches the border."""
    img = gc.shape_image(shape)
    H, W = shape
    for block in gc.BLOCKS:
        m = MAP(img, block)
        assert np.array_equal(MAP(np.ascontiguousarray(img.T), block), m.T), ("transposed", block)
        assert np.array_equal(MAP(255 - img, block), m), ("inverted", block)
        mx = MAP(np.ascontiguousarray(img[:, ::-1]), block)[:, ::-1]
        my = MAP(np.ascontiguousarray(img[::-1]), block)[::-1]
        if block % 2:
            assert np.array_equal(mx, m) and np.array_equal(my, m), ("mirrored", block)
        else:
            if W > 2 * block + 1:
                assert np.array_equal(mx[:, block:W - block - 1], m[:, block + 1:W - block]), ("mirrored in x", block)
            if H > 2 * block + 1:
                assert np.array_equal(my[block:H - block - 1], m[block + 1:H - block]), ("mirrored in y", block)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_cases_reach_the_edges_they_are_named_for():
    # blocks wider than the image, boxes that reflect more than once
    assert max(gc.BLOCKS) == 31 and any(max(s) < 31 for s in gc.SHAPES) and (5, 9) in gc.SHAPES and (20, 20) in gc.SHAPES
    rows = np.arange(-(31 // 2), 5 + 31 // 2)                           # a 31-wide box on 5 rows passes both edges repeatedly
    assert np.count_nonzero(np.diff(np.sign(np.diff(ref.reflect101(rows, 5))))) >= 8
    # no interior / one interior pixel / one tile / one row and column into the next tiles
    assert all(min(s) < 3 for s in gc.NO_INTERIOR) and (3, 3) in gc.SHAPES
    assert gc.TILE in gc.SHAPES and (gc.TILE[0] + 1, gc.TILE[1] + 1) in gc.SHAPES
    # a gradient of +-1020, the packed halves' full range
    gx, gy = ref.sobel(gc.EXTREMES["checker3_24x27"])
    assert gx.min() == gy.min() == -1020 and gx.max() == gy.max() == 1020
    # an exact four-way tie
    for block in gc.TIE_BLOCKS:
        key = ref.tie_key(gc.tie_image(), block)
        got = CORNERS(gc.tie_image(), None, *gc.TIE_PARAMS, block)
        assert len(got) == 4 and len({tuple(key[int(y), int(x)]) for x, y in got}) == 1
    # a corner at no more than 8 x 8
    small = gc.smallest_with_a_corner()
    assert max(small.shape) <= 8 and len(CORNERS(small, None, *gc.SMALLEST_PARAMS)) > 0
    assert ref.decided(small, None, *gc.SMALLEST_PARAMS)
    # a masked-out maximum larger than the masked one, and corners that only the masked threshold lets through
    lower = 0
    for shape in gc.SHAPES[len(gc.NO_INTERIOR):]:
        img = gc.shape_image(shape)
        for block in gc.SELECT_BLOCKS:
            mask = gc.make_mask("no_max", img, block)
            if not mask.any():                                        # (3 x 3: the forbidden 3 x 3 is the image)
                continue
            m = MAP(img, block)
            assert m[mask != 0].max() < m.max(), (shape, block)
            thr_all = ref.threshold(m, None, 0.5)
            ys, xs = ref.candidates(m, mask, 0.5)                     # (kept under the masked threshold ...)
            lower += int(np.count_nonzero(m[ys, xs] <= thr_all))      # (... but not above the whole image's)
    assert lower > 0
    s = gc.SCENE_BY_NAME["squares64x80_b5_masked_q05"]
    m = MAP(s.img, s.params[3])
    assert m[s.mask != 0].max() < 0.75 * m.max()
    with_mask, without = (ref.select(m, k, *s.params[:3]).tolist() for k in (s.mask, None))
    assert len(with_mask) == 8 and [21, 51] in with_mask and [21, 51] not in without       # (a corner of the square of 160)
    # settings: both sides of min_distance 1, a distance larger than every image, quality 1
    assert {0, 0.5, 1, 200} <= set(gc.MIN_DISTANCES) and 1.0 in gc.QUALITIES and max(max(s) for s in gc.SHAPES) < 200
    # candidates exactly min_distance apart, so `<` against `<=` decides
    hits = 0
    for shape in ((17, 65), (33, 47), (20, 20), (16, 64)):
        img = gc.shape_image(shape)
        for block in gc.SELECT_BLOCKS:
            ys, xs = ref.candidates(MAP(img, block), None, gc.BASE[1])
            d2 = (ys[:, None] - ys[None]) ** 2 + (xs[:, None] - xs[None]) ** 2
            hits += int(np.count_nonzero(np.triu(d2 == 64, 1)))
    assert hits > 0
