"""The definition of the project's FAST-9 corner detector (include/vo_hip.h, "FAST-9 corners"), vectorised in NumPy.
Everything is integer arithmetic: csrc/fast.hip is held to this bit for bit on every input (tests/test_gpu_fast.py), and
tests/test_fast_host.py checks it against a plain per-pixel loop on every case of tests/fast_cases.py."""
import numpy as np

# radius 3, sixteen offsets (dx, dy), clockwise from the top
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0),
          (-3, -1), (-2, -2), (-1, -3))
MAX_KEYPOINTS = 16384


def score_map(img, threshold):
    """(H, W) uint8: s(p) where s(p) > threshold, 0 elsewhere and on the border of 3."""
    assert 0 <= threshold <= 254
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    if H < 7 or W < 7:
        return out
    a = img.astype(np.int32)
    centre = a[3:H - 3, 3:W - 3]
    d = np.stack([a[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - centre for dx, dy in CIRCLE])
    best = np.full(centre.shape, -256, np.int32)
    for k in range(16):
        arc = d[[(k + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    out[3:H - 3, 3:W - 3] = np.where(best > threshold, best, 0)
    return out


def survivor_map(score, nonmax):
    """(H, W) uint8: the score where the corner survives, 0 elsewhere.  nonmax: a corner survives iff none of its eight
    neighbours has a higher score, or the same score and a lower index y W + x."""
    score = np.asarray(score)
    if not nonmax:
        return score.copy()
    H, W = score.shape
    s = score.astype(np.int32)
    pad = np.zeros((H + 2, W + 2), np.int32)
    pad[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            nb = pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
            lower = dy < 0 or (dy == 0 and dx < 0)
            keep &= ~((nb > s) | ((nb == s) & lower))
    return np.where(keep, score, 0).astype(np.uint8)


def keypoints(img, threshold=20, nonmax=True, N=1000):
    """(kp (n, 2) float64 (x, y), scores (n,) uint8, total): the n = min(N, total) survivors first in the order (score
    descending, index ascending); total: the survivors before the cut."""
    assert 1 <= N <= MAX_KEYPOINTS
    surv = survivor_map(score_map(img, threshold), nonmax)
    W = surv.shape[1]
    idx = np.flatnonzero(surv)
    sc = surv.reshape(-1)[idx]
    order = np.lexsort((idx, -sc.astype(np.int64)))[:N]
    idx, sc = idx[order], sc[order]
    kp = np.stack([idx % W, idx // W], axis=1).astype(np.float64).reshape(-1, 2)
    return kp, sc.astype(np.uint8), int(np.count_nonzero(surv))
