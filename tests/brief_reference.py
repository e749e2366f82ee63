"""The BRIEF-256 descriptor, its orientation bin and the Hamming 2-NN matcher as NumPy states them: the definition
include/vo_hip.h gives in words, which csrc/brief.hip is held to bit for bit (tests/test_gpu_brief.py) and which
tests/test_brief_host.py checks against a second, per-pixel statement.  Everything is integer arithmetic except the two
places the definition names: the centre floor(x + 0.5) in float64 and the ratio test's one float64 multiply.

The sampling pattern comes from the generator (tools/make_brief_pattern.py), not from the header the kernels compile in:
test_brief_host.py checks that the two are the same table."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACH = 16            # rotated offsets stay within radius 14, the box adds 2
DISC = 15             # radius of the orientation moments
PAD = 2 * REACH + 1   # a valid centre lies in [-16, W + 16): every pixel it reads lies in [-32, W + 32)


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_brief_pattern", os.path.join(ROOT, "tools", "make_brief_pattern.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def tables():
    """(table (30, 256, 4) int8 rows (ax, ay, bx, by), C (30,) int32, Sn (30,) int32), read-only."""
    out = generator().tables()
    for a in out:
        a.flags.writeable = False
    return out


def centres(kp_xy, H, W):
    """(cx, cy, valid): int64 centres floor(x + 0.5), floor(y + 0.5) in float64; valid where both coordinates are finite and
    the centre lies in [-16, W + 16) x [-16, H + 16).  Invalid centres are returned as 0."""
    kp = np.asarray(kp_xy, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(kp + 0.5)
        valid = np.isfinite(kp).all(axis=1) & (f[:, 0] >= -REACH) & (f[:, 0] < W + REACH) & (f[:, 1] >= -REACH) & (f[:, 1] < H + REACH)
    f = np.where(valid[:, None], f, 0.0).astype(np.int64)
    return f[:, 0], f[:, 1], valid


def padded(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    return np.pad(img.astype(np.int64), PAD)


def box_sums(P):
    """S of the padded image: S[y, x] = the sum over the 5 x 5 box centred there (zero beyond the padding)."""
    Q = np.pad(P, 2)
    I = np.zeros((Q.shape[0] + 1, Q.shape[1] + 1), np.int64)
    I[1:, 1:] = Q.cumsum(0).cumsum(1)
    h, w = P.shape
    return I[5:5 + h, 5:5 + w] - I[:h, 5:5 + w] - I[5:5 + h, :w] + I[:h, :w]


def moments(img, kp_xy):
    """(m10, m01) int64 per keypoint: sums of dx I and dy I over dx^2 + dy^2 <= 15^2, image zero outside; 0 where the
    centre is not valid."""
    H, W = img.shape
    cx, cy, valid = centres(kp_xy, H, W)
    P = padded(img)
    d = np.arange(-DISC, DISC + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    inside = (dx * dx + dy * dy) <= DISC * DISC
    patch = P[(cy[:, None, None] + dy + PAD), (cx[:, None, None] + dx + PAD)] * inside
    m10 = (patch * dx).sum(axis=(1, 2)) * valid
    m01 = (patch * dy).sum(axis=(1, 2)) * valid
    return m10, m01


def bins(img, kp_xy):
    """The orientation bin of every keypoint: argmax_k (m10 C[k] + m01 Sn[k]) in int64, ties to the lowest k."""
    _, C, Sn = tables()
    m10, m01 = moments(img, kp_xy)
    val = m10[:, None] * C.astype(np.int64) + m01[:, None] * Sn.astype(np.int64)
    return np.argmax(val, axis=1).astype(np.uint8)         # (the first maximum)


def sample_values(img, kp_xy, oriented):
    """(sa, sb, k, valid): the two box sums of every test (N, 256), the bins, the valid centres."""
    H, W = img.shape
    table = tables()[0]
    cx, cy, valid = centres(kp_xy, H, W)
    k = bins(img, kp_xy) if oriented else np.zeros(len(cx), np.uint8)
    S = box_sums(padded(img))
    tab = table[k].astype(np.int64)                          # (N, 256, 4)
    sa = S[cy[:, None] + tab[:, :, 1] + PAD, cx[:, None] + tab[:, :, 0] + PAD]
    sb = S[cy[:, None] + tab[:, :, 3] + PAD, cx[:, None] + tab[:, :, 2] + PAD]
    return sa, sb, k, valid


def describe(img, kp_xy, oriented=False):
    """(desc (N, 32) uint8, bin (N,) uint8): bit i = S(c + a_i) < S(c + b_i), stored in byte i // 8 at position i % 8."""
    sa, sb, k, valid = sample_values(img, kp_xy, oriented)
    bits = (sa < sb) & valid[:, None]
    return np.packbits(bits, axis=1, bitorder="little"), np.where(valid, k, 0).astype(np.uint8)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(q, t):
    """(nq, nt) int64 distances of uint8 rows."""
    q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
    out = np.zeros((q.shape[0], t.shape[0]), np.int64)
    for b in range(q.shape[1]):
        out += _POP[q[:, b, None] ^ t[None, :, b]]
    return out


def knn2(q, t):
    """(best (nq, 2) int32, dist (nq, 2) int32): the two train rows smallest under (distance, index); -1 / 0 where absent."""
    nq, nt = len(q), len(t)
    best = np.full((nq, 2), -1, np.int32)
    dist = np.zeros((nq, 2), np.int32)
    if nq == 0 or nt == 0:
        return best, dist
    d = hamming(q, t)
    order = np.argsort(d * (1 << 32) + np.arange(nt), axis=1, kind="stable")[:, :2]
    n = order.shape[1]
    best[:, :n] = order
    dist[:, :n] = np.take_along_axis(d, order, axis=1)
    return best, dist


def ratio_pairs(best, dist, ratio, max_dist=-1):
    """Queries in order; (q, best) iff both neighbours exist, float64(d1) < ratio * float64(d2), d1 <= max_dist when
    max_dist >= 0, and no earlier query took `best`."""
    ratio = np.float64(ratio)
    passes = (best[:, 0] >= 0) & (best[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64))
    if max_dist >= 0:
        passes &= dist[:, 0] <= max_dist
    idx = np.nonzero(passes)[0]
    _, first = np.unique(best[idx, 0], return_index=True)
    keep = np.sort(idx[first])
    return np.stack([keep, best[keep, 0]], axis=1).astype(np.int64).reshape(-1, 2)


def match(q, t, ratio, max_dist=-1):
    return ratio_pairs(*knn2(q, t), ratio, max_dist)
