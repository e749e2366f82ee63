"""The image recipes of the batched Shi-Tomasi tests (tests/test_gpu_good_features_batch.py runs them on the device,
tests/test_good_features_batch_host.py checks on the CPU that they are what they claim), and the thresholded 3x3 local
maxima of the definition (oracle/csrc/goodfeatures.c) restated over oracle.native.min_eigen_map."""
import numpy as np

from oracle import native
from scenarios import synthetic_image

DEFAULTS = (500, 0.01, 8, 7)            # max_corners, quality, min_distance, block_size (klt.py:24-26)
MASKED = (50, 0.05, 5, 5)               # the one-image test's masked call
CROWDED = (0, 0.01, 40, 7)              # cells of side 40: more candidates per cell than the rounds path's lists hold
CELL_LIST = 32                          # candidates a cell holds on the rounds path (GC_CCAP in csrc/goodfeatures.hip)
ROUNDS = 24                             # round launches of the batched call (GB_R in csrc/goodfeatures.hip)
SMALL = (480, 640)
CONFIG = (1241, 1376)
# test_good_features_at_configuration_size's parameter sets
CONFIG_SETS = [(2000, 0.01, 8, 7), (500, 0.01, 7.5, 7), (0, 0.02, 12, 5), (3000, 0.01, 0, 7), (100000, 0.001, 3, 3)]


def flat_image(shape=SMALL):
    return np.full(shape, 128, np.uint8)


def ordinary_images(shape=SMALL):
    """Four textured images (different seeds) and a flat one, in the order the tests batch them: the flat one is third."""
    H, W = shape
    imgs = [synthetic_image(H, W, seed, block=9) for seed in (11, 12, 13, 14)]
    imgs.insert(2, flat_image(shape))
    return imgs


def half_mask(shape, side):
    m = np.zeros(shape, np.uint8)
    if side == "left":
        m[:, : shape[1] // 2] = 255
    else:
        m[shape[0] // 2:, :] = 255
    return m


def masks_for(shape=SMALL):
    """Per image of ordinary_images: left half, none, none, lower half, none."""
    return [half_mask(shape, "left"), None, None, half_mask(shape, "lower"), None]


def config_images():
    H, W = CONFIG
    return [synthetic_image(H, W, seed, block=9) for seed in (17, 18, 19, 20)]


def plateau_image(shape=(96, 128)):
    """A texture of period 3 in both directions.  With block_size 3 every window of the structure tensor covers exactly one
    period, so the (exact-integer) sums and with them the eigenvalue are one constant over the interior: every interior
    pixel ties with its eight neighbours and counts as a local maximum -- about H*W of them, against a capacity of
    H*W/4 + 64."""
    tile = np.array([[10, 200, 60], [120, 30, 250], [220, 90, 5]], np.uint8)
    H, W = shape
    return np.tile(tile, (-(-H // 3), -(-W // 3)))[:H, :W].copy()


PLATEAU = (100, 0.01, 8, 3)


def candidate_capacity(shape):
    return (shape[0] * shape[1] + 3) // 4 + 64


def local_maxima(img, mask, quality, block):
    """Boolean map of the candidates: interior pixels above the threshold (float32 of masked maximum x quality), non-zero,
    allowed by the mask, equal to the maximum of their thresholded 3x3 neighbourhood."""
    eig = native.min_eigen_map(img, block)
    allowed = np.ones(eig.shape, bool) if mask is None else np.asarray(mask) != 0
    if not allowed.any():
        return np.zeros(eig.shape, bool)
    thr = np.float32(np.float64(eig[allowed].max()) * quality)
    t = np.where(eig > thr, eig, np.float32(0))
    p = np.pad(t, 1)
    H, W = eig.shape
    m = np.zeros_like(t)
    for j in range(3):
        for i in range(3):
            m = np.maximum(m, p[j:j + H, i:i + W])
    take = (eig > thr) & (eig != 0) & allowed & (eig == m)
    take[0, :] = take[-1, :] = False
    take[:, 0] = take[:, -1] = False
    return take


def max_per_cell(take, min_distance):
    """The largest number of candidates in one cell of the minimum-distance grid (cell side = round(min_distance))."""
    cell = max(1, int(np.floor(min_distance + 0.5)))
    ys, xs = np.nonzero(take)
    if len(ys) == 0:
        return 0
    gw = -(-take.shape[1] // cell)
    return int(np.bincount((ys // cell) * gw + xs // cell).max())


def synchronous_rounds(img, mask, max_corners, quality, min_distance, block):
    """The minimum-distance rule as the batched call's rounds apply it, with every round reading only the states the round
    before left (on the device a round may also see decisions of its own round, so it needs at most as many): a candidate
    is accepted once every earlier candidate within min_distance in the 3x3 cells around it is rejected, rejected once one
    is accepted.  Returns (rounds until nothing is open, candidates, corners as the first max_corners accepted)."""
    take = local_maxima(img, mask, quality, block)
    eig = native.min_eigen_map(img, block)
    ys, xs = np.nonzero(take)
    addr = ys.astype(np.int64) * img.shape[1] + xs
    order = np.lexsort((-addr, -eig[ys, xs].view(np.uint32).astype(np.int64)))      # value, then address, descending
    ys, xs = ys[order], xs[order]
    cell = max(1, int(np.floor(min_distance + 0.5)))
    grid = {}
    for k in range(len(xs)):
        grid.setdefault((xs[k] // cell, ys[k] // cell), []).append(k)
    earlier = []
    for k in range(len(xs)):
        x, y = int(xs[k]), int(ys[k])
        near = [o for cy in range(y // cell - 1, y // cell + 2) for cx in range(x // cell - 1, x // cell + 2)
                for o in grid.get((cx, cy), ()) if o < k and (x - xs[o]) ** 2 + (y - ys[o]) ** 2 < min_distance * min_distance]
        earlier.append(np.array(near, np.int64))
    state = np.zeros(len(xs), np.int8)              # 0 undecided, 1 accepted, 2 rejected
    rounds = 0
    while (state == 0).any():
        new = state.copy()
        for k in np.flatnonzero(state == 0):
            st = state[earlier[k]]
            if (st == 1).any():
                new[k] = 2
            elif not (st == 0).any():
                new[k] = 1
        state = new
        rounds += 1
    acc = np.flatnonzero(state == 1)
    if max_corners > 0:
        acc = acc[:max_corners]
    return rounds, len(xs), np.stack([xs[acc], ys[acc]], 1).astype(np.float32).reshape(-1, 2)
