"""The cases of the Shi-Tomasi definition tests (tests/test_good_features_reference_host.py on the oracle,
tests/test_gpu_good_features_reference.py on the kernels): small images, each named for the edge it keeps, all from seeds or
formulas.  Nothing here imports `oracle` or the library; what an image claims is asserted on the definition
(tests/good_features_reference.py) where it is built, and on the oracle in the host file's
test_cases_reach_the_edges_they_are_named_for."""
import functools
from collections import namedtuple

import numpy as np

import good_features_reference as ref

BLOCKS = (1, 2, 3, 4, 6, 7, 8, 15, 16, 30, 31)
# no interior pixel (no corner, whatever the map) ... one interior pixel ... one row / column of them ... exactly one 64 x 16
# tile of the map kernel ... one row and one column into the next tiles ... narrower than blocks 7 to 31 (5 x 9: a 31-wide box
# reflects eight times) ... an ordinary odd size
NO_INTERIOR = ((1, 1), (1, 7), (7, 1), (2, 2), (2, 9))
SHAPES = NO_INTERIOR + ((3, 3), (3, 64), (64, 3), (16, 64), (17, 65), (5, 9), (20, 20), (33, 47))
TILE = (16, 64)             # GY x GX of csrc/goodfeatures.hip


def name_of(shape):
    return "%dx%d" % tuple(shape)


def texture(shape, seed):
    """4 x 4 cells of random grey with +-6 of noise: strong corners at the cells' crossings, weak gradients everywhere else."""
    H, W = shape
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 256, size=(-(-H // 4), -(-W // 4)))
    img = np.kron(cells, np.ones((4, 4), np.int64))[:H, :W] + rng.integers(-6, 7, size=shape)
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shape_image(shape):
    return texture(shape, 1000 * shape[0] + shape[1])


SMALLEST_PARAMS = (0, 0.01, 1.0, 3)          # max_corners, quality, min_distance, block


@functools.lru_cache(maxsize=None)
def smallest_with_a_corner():
    """The smallest texture (by area, then height; sides 3..8; seeds 0..31) on which the definition returns a corner and
    every decision is decided, so the code must return it too."""
    shapes = sorted(((h, w) for h in range(3, 9) for w in range(3, 9)), key=lambda s: (s[0] * s[1], s[0]))
    for shape in shapes:
        for seed in range(32):
            img = texture(shape, seed)
            if len(ref.select(ref.min_eig(img, SMALLEST_PARAMS[3])[0], None, *SMALLEST_PARAMS[:3])) > 0 and \
                    ref.decided(img, None, *SMALLEST_PARAMS):
                return img
    raise AssertionError("no texture of at most 8 x 8 returns a corner")


def map_cases():
    """(name, image, blocks) of every image whose map is compared with the definition."""
    out = [(name_of(s), shape_image(s), BLOCKS) for s in SHAPES]
    out.append(("smallest", smallest_with_a_corner(), BLOCKS))
    out += [(n, img, EXTREME_BLOCKS) for n, img in EXTREMES.items()]
    out += [(n, img, (2, 3, 4, 5, 6, 7)) for n, img in SCENE_IMAGES.items()]
    return out


def check_map(got, img, block):
    """The checks every float32 map goes through, the oracle's and the kernels': within rounding_bound of the definition at
    every pixel, exactly 0 where the sums are 0.  Returns the largest |got - lambda| in units of 2^-24 trace (KAPPA is the
    bound)."""
    lam, trace = ref.min_eig(img, block)
    assert got.dtype == np.float32 and got.shape == lam.shape
    err = np.abs(got.astype(np.float64) - lam)
    assert np.all(got[trace == 0] == 0), "a pixel whose sums are 0 is not exactly 0"
    assert np.all(err <= ref.rounding_bound(trace)), "map outside the rounding bound: %g of it at %s" % (
        float(np.max(err[trace > 0] / ref.rounding_bound(trace[trace > 0]))), np.unravel_index(int(np.argmax(err)), err.shape))
    return float(np.max(err[trace > 0] / (ref.U * trace[trace > 0]))) if (trace > 0).any() else 0.0


def float32_formula(img, block):
    """The float32 evaluation rounding_bound is derived for, on the definition's exact sums, operation by operation (NumPy's
    float32 arithmetic is IEEE round-to-nearest without contraction): what the oracle and the kernels return, bit for bit."""
    Sxx, Sxy, Syy = ref.tensor_sums(img, block)
    s2 = np.float32(ref.scale(block) * ref.scale(block))
    half = np.float32(0.5)
    a, b, c = Sxx.astype(np.float32) * s2 * half, Sxy.astype(np.float32) * s2, Syy.astype(np.float32) * s2 * half
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


# ---- extremes --------------------------------------------------------------------------------------------------------------
def checker(shape, cell):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return ((((y // cell) + (x // cell)) & 1) * 255).astype(np.uint8)


def ramp(shape, a, b, offset=0):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return np.clip(a * x + b * y + offset, 0, 255).astype(np.uint8)


def flat(shape, value=128):
    return np.full(shape, value, np.uint8)


EXTREME_BLOCKS = (1, 2, 3, 7, 8, 31)
EXTREMES = {
    "checker1_20x21": checker((20, 21), 1),          # period 1: every Sobel response is 0, lambda = 0 exactly
    "checker3_24x27": checker((24, 27), 3),          # 3 x 3 cells of 0 / 255: gradients of +-1020
    "ramp_x3_33x47": ramp((33, 47), 3, 0),           # rank one away from the borders: lambda = 0, the code's value rounding
    "ramp_y2_33x47": ramp((33, 47), 0, 2, 7),
    "ramp_2x1y_33x47": ramp((33, 47), 2, 1, 30),
    "ramp_5x-3y_33x47": ramp((33, 47), 5, -3, 96),   # clipped at 0 and at 255 along two diagonals
    "flat_20x20": flat((20, 20)),
}


def ramp_interior(img, block):
    """Pixels of a ramp whose box, widened by the Sobel ring, touches neither the border nor a clipped pixel."""
    H, W = img.shape
    r = block // 2 + 1
    sat = (img == 0) | (img == 255)
    ok = np.zeros(img.shape, bool)
    for y in range(r, H - r):
        for x in range(r, W - r):
            ok[y, x] = not sat[y - r:y + r + 1, x - r:x + r + 1].any()
    return ok


# ---- analytic ties ---------------------------------------------------------------------------------------------------------
def square_image(shape, squares, background):
    """squares: (top, left, side, grey)."""
    img = np.full(shape, background, np.uint8)
    for top, left, side, grey in squares:
        img[top:top + side, left:left + side] = grey
    return img


TIE_SIDE, TIE_AT, TIE_SQUARE = 41, 12, 17
TIE_PARAMS = (500, 0.01, 8)                   # the call site's


def tie_image():
    """A 17-pixel square centred in 41 x 41: the image is its own mirror image in x, in y and across the diagonals, so the
    maxima at its four corners have the same (T, (Sxx - Syy)^2, Sxy^2) for every odd block."""
    return square_image((TIE_SIDE, TIE_SIDE), [(TIE_AT, TIE_AT, TIE_SQUARE, 220)], 40)


TIE_BLOCKS = (3, 5, 7)
TIE_BLOCK3 = [(28, 28), (12, 28), (28, 12), (12, 12)]     # (x, y): bottom-right, bottom-left, top-right, top-left


# ---- decided scenes --------------------------------------------------------------------------------------------------------
Scene = namedtuple("Scene", "name img mask params")       # params: max_corners, quality, min_distance, block


def _scene_images():
    four = [(8, 8, 14, 250), (10, 40, 21, 200), (36, 6, 17, 160), (40, 52, 12, 120)]
    three = [(5, 6, 11, 20), (7, 27, 15, 90), (27, 9, 9, 140)]              # dark squares on a bright ground
    small = [(4, 5, 9, 250), (6, 24, 12, 190), (24, 8, 11, 140)]
    return {"squares64x80": square_image((64, 80), four, 30), "dark40x48": square_image((40, 48), three, 230),
            "tie41x41": tie_image(), "squares41x41": square_image((TIE_SIDE, TIE_SIDE), small, 30)}


SCENE_IMAGES = _scene_images()
_TIE = SCENE_IMAGES["tie41x41"]


def _scenes():
    a, b = SCENE_IMAGES["squares64x80"], SCENE_IMAGES["dark40x48"]
    m = np.full((64, 80), 255, np.uint8)
    m[:32, :36] = 0                                      # the strongest square masked out
    return [Scene("squares64x80_b5", a, None, (500, 0.01, 8, 5)),
            Scene("squares64x80_b3_d0", a, None, (0, 0.01, 0, 3)),
            Scene("squares64x80_b7_first5", a, None, (5, 0.01, 8, 7)),
            Scene("squares64x80_b5_masked", a, m, (500, 0.01, 8, 5)),
            # lambda goes with the contrast squared, 220^2 : 170^2 : 130^2 : 90^2: half the allowed maximum keeps the squares
            # of 200 and 160, half the image's maximum would keep the one of 200 alone
            Scene("squares64x80_b5_masked_q05", a, m, (500, 0.5, 8, 5)),
            Scene("squares64x80_b4", a, None, (500, 0.05, 7.5, 4)),
            Scene("dark40x48_b3", b, None, (500, 0.01, 2.5, 3)),
            Scene("dark40x48_b6_q05", b, None, (0, 0.5, 1, 6))]


SCENES = _scenes() + [Scene("tie41x41_b%d" % b, _TIE, None, TIE_PARAMS + (b,)) for b in TIE_BLOCKS]
# the block-3 corners are 16 apart along the sides and 16 sqrt 2 = 22.6 across: at min_distance 16 the `<` keeps all four, at
# 16.5 the first and the one across from it
SCENES += [Scene("tie41x41_b3_d16", _TIE, None, (500, 0.01, 16, 3)), Scene("tie41x41_b3_d16.5", _TIE, None, (500, 0.01, 16.5, 3))]
TIE_DISTANCE = {"tie41x41_b3_d16": TIE_BLOCK3, "tie41x41_b3_d16.5": [TIE_BLOCK3[0], TIE_BLOCK3[3]]}


# ---- one batch: a flat image, a decided scene under a mask of its own, the tie image -- all 41 x 41 -------------------------
def batch_scenes(params):
    """Three Scenes of one size and one parameter set, in the order the GPU tests batch them."""
    img = SCENE_IMAGES["squares41x41"]
    m = np.full((TIE_SIDE, TIE_SIDE), 1, np.uint8)
    m[:18, :18] = 0                                     # the strongest square masked out, the allowed value 1
    tag = "_d%g_b%d" % (params[2], params[3])
    return [Scene("batch_flat41x41" + tag, flat((TIE_SIDE, TIE_SIDE)), None, params), Scene("batch_squares41x41" + tag, img, m, params),
            Scene("batch_tie41x41" + tag, _TIE, None, params)]


BATCHES = [batch_scenes((500, 0.01, 8, 5)), batch_scenes((0, 0.05, 0.5, 3))]      # the second: min_distance < 1, path 2
SCENES += [s for b in BATCHES for s in b if "flat" not in s.name]
SCENE_BY_NAME = {s.name: s for s in SCENES}


# ---- parameters and masks, on the small shapes -----------------------------------------------------------------------------
BASE = (0, 0.01, 2.5)                          # max_corners, quality, min_distance
QUALITIES = (1e-3, 0.01, 0.5, 1.0)             # at 1.0 nothing passes `>`
MIN_DISTANCES = (0, 0.5, 1, 1.4, 2.5, 7.5, 8, 8.5, 200)      # below 1: no test; 200: larger than every image, one corner
MASKS = ("zero", "one", "border", "ones", "no_max")
SELECT_BLOCKS = (2, 3, 7)                      # every setting runs with these; BASE alone with every block


def make_mask(kind, img, block):
    """zero: nothing allowed.  one: one allowed pixel, the centre.  border: only the first and last row, where a maximum
    exists but no candidate.  ones: value 1 for 255, the left third forbidden.  no_max: the definition's largest value and
    the 3 x 3 around it forbidden, so the threshold follows the largest allowed one."""
    H, W = img.shape
    m = np.zeros((H, W), np.uint8)
    if kind == "one":
        m[H // 2, W // 2] = 255
    elif kind == "border":
        m[0, :] = m[-1, :] = 255
    elif kind == "ones":
        m[:, W // 3:] = 1
    elif kind == "no_max":
        lam = ref.min_eig(img, block)[0]
        y, x = np.unravel_index(int(np.argmax(lam)), lam.shape)
        m[:] = 255
        m[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 0
    else:
        assert kind == "zero"
    return m


Setting = namedtuple("Setting", "name mask max_corners quality min_distance")


def settings():
    """Every (mask kind or None, max_corners, quality, min_distance) besides BASE; max_corners is set by the tests from the
    number of corners the unlimited call returns (corner_limits)."""
    out = [Setting("q%g" % q, None, BASE[0], q, BASE[2]) for q in QUALITIES if q != BASE[1]]
    out += [Setting("d%g" % d, None, BASE[0], BASE[1], d) for d in MIN_DISTANCES if d != BASE[2]]
    out += [Setting("mask_" + k, k, *BASE) for k in MASKS]
    out.append(Setting("mask_no_max_q0.5", "no_max", BASE[0], 0.5, BASE[2]))      # corners between the two thresholds
    return out


def corner_limits(n_all):
    """max_corners beside 0: one, exactly the number available, more."""
    return sorted({1, max(n_all, 1), n_all + 3})


def select_table(shape):
    """(block, Setting) of one shape: BASE with every block, every other setting with SELECT_BLOCKS."""
    base = Setting("base", None, *BASE)
    return [(b, base) for b in BLOCKS] + [(b, s) for b in SELECT_BLOCKS for s in settings()]


# ---- the selection check both test files run, on the oracle and on the kernels -----------------------------------------------
def corners_equal_rule(corners, eig_map, img, mask, max_corners, quality, min_distance, block, what):
    """corners(img, mask, max_corners, quality, min_distance, block) must be select() on eig_map, the map of the same code."""
    got = corners(img, mask, max_corners, quality, min_distance, block)
    want = ref.select(eig_map, mask, max_corners, quality, min_distance)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), (what, got.tolist(), want.tolist())
    return got


def run_select_table(name, img, maps, corners):
    """Every (block, setting) of the image, and max_corners 1 / exactly the number available / more."""
    calls = 0
    for block, s in select_table(img.shape):
        mask = None if s.mask is None else make_mask(s.mask, img, block)
        got = corners_equal_rule(corners, maps[block], img, mask, s.max_corners, s.quality, s.min_distance, block, (name, block, s))
        calls += 1
        if s.name == "base" and block in SELECT_BLOCKS:
            for limit in corner_limits(len(got)):
                cut = corners_equal_rule(corners, maps[block], img, None, limit, s.quality, s.min_distance, block, (name, block, limit))
                assert np.array_equal(cut, got[:limit])
                calls += 1
        if s.quality == 1.0 or s.name in ("mask_zero", "mask_border") or img.shape in NO_INTERIOR:
            assert len(got) == 0, (name, block, s)
        if s.name == "mask_one" or s.min_distance == 200:
            assert len(got) <= 1
    return calls
