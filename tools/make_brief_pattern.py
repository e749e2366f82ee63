"""Draws the BRIEF-256 sampling pattern and writes the table the kernels compile in
(visual-odometry-project_amd/csrc/brief_pattern.h: data only).

    python tools/make_brief_pattern.py            # rewrite the header
    python tools/make_brief_pattern.py --check    # exit 1 if the committed header differs

The definition (include/vo_hip.h, "BRIEF-256"; tests/brief_reference.py states it in NumPy):
  * 256 pairs (a_i, b_i) of integer offsets (x, y), drawn in order by np.random.default_rng(SEED) from an isotropic
    Gaussian with sigma = 13 / 2, each coordinate rounded half away from zero.  A draw is rejected when
      - a or b lies outside the disc of radius 13,
      - a == b, or the pair (a, b) was drawn before,
      - some rotation of a or b by a multiple of 12 degrees has a coordinate within MARGIN_DRAW of a rounding boundary
        (60 degrees turns (3, 0) into (1.5, 2.598...): such offsets are left out, so that no table entry depends on the
        last bit of a cosine),
      - some rotation maps a and b to one offset (that bit would be 0 on every image).
  * table k (k = 0 .. 29) rotates every offset by 12 k degrees, (x, y) -> (x cos - y sin, x sin + y cos) in float64, and
    rounds half away from zero.  Table 0 is the drawn pattern.
  * C[k] = round(16384 cos(2 pi k / 30)), Sn[k] = round(16384 sin(2 pi k / 30)): the orientation bins' directions.
The asserts below hold the table to that without a libm: no rotated coordinate (and no 16384 cos / sin) lies within 1e-9 of
a rounding boundary, and every rotated offset stays within radius 14 -- with the 5 x 5 box (2) the reach is 16 pixels.
"""
import argparse
import os
import sys

import numpy as np

SEED = 256
N_PAIRS = 256
N_BINS = 30
RADIUS = 13
SIGMA = RADIUS / 2.0
ROT_RADIUS = 14
MARGIN_DRAW = 1e-6          # rejection while drawing
MARGIN_ASSERT = 1e-9        # what the finished table is held to
SCALE = 16384

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "visual-odometry-project_amd", "csrc", "brief_pattern.h")


def round_half_away(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def boundary_distance(v):
    """Distance of every value to the nearest rounding boundary (an integer + 1/2)."""
    v = np.abs(np.asarray(v, np.float64))
    return np.abs(v - np.floor(v) - 0.5)


def rotations(p):
    """(N_BINS, ..., 2) float64: the offsets p (..., 2) rotated by 12 k degrees."""
    p = np.asarray(p, np.float64)
    ang = 2.0 * np.pi * np.arange(N_BINS) / N_BINS
    c, s = np.cos(ang), np.sin(ang)
    shape = (N_BINS,) + (1,) * (p.ndim - 1)
    c, s = c.reshape(shape), s.reshape(shape)
    return np.stack([p[..., 0] * c - p[..., 1] * s, p[..., 0] * s + p[..., 1] * c], axis=-1)


def draw_pattern(seed=SEED):
    """(256, 4) int64 rows (ax, ay, bx, by)."""
    rng = np.random.default_rng(seed)
    rows, seen = [], set()
    while len(rows) < N_PAIRS:
        v = round_half_away(rng.normal(0.0, SIGMA, size=4))
        a, b = v[:2], v[2:]
        if a @ a > RADIUS * RADIUS or b @ b > RADIUS * RADIUS:
            continue
        key = tuple(int(x) for x in v)
        if key[:2] == key[2:] or key in seen:
            continue
        rot = rotations(v.reshape(2, 2))                     # (30, 2, 2)
        if np.any(boundary_distance(rot) < MARGIN_DRAW):
            continue
        r = round_half_away(rot)
        if np.any(np.all(r[:, 0] == r[:, 1], axis=-1)):
            continue
        seen.add(key)
        rows.append(key)
    return np.array(rows, np.int64)


def rotated_tables(pattern):
    """(30, 256, 4) int8 from the (256, 4) pattern, with the asserts of the definition."""
    pts = pattern.reshape(N_PAIRS, 2, 2)
    rot = rotations(pts)                                     # (30, 256, 2, 2)
    assert boundary_distance(rot).min() >= MARGIN_ASSERT, "a rotated coordinate sits on a rounding boundary"
    r = round_half_away(rot)
    assert np.array_equal(r[0], pts), "table 0 is the pattern itself"
    assert int((r ** 2).sum(axis=-1).max()) <= ROT_RADIUS * ROT_RADIUS, "a rotated offset leaves radius 14"
    assert int((pts ** 2).sum(axis=-1).max()) <= RADIUS * RADIUS
    assert not np.any(np.all(r[:, :, 0] == r[:, :, 1], axis=-1)), "a rotated pair collapsed"
    assert len({tuple(row) for row in pattern.tolist()}) == N_PAIRS, "a pair appears twice"
    return r.reshape(N_BINS, N_PAIRS, 4).astype(np.int8)


def direction_tables():
    """(C, Sn): int32 arrays of 30."""
    ang = 2.0 * np.pi * np.arange(N_BINS) / N_BINS
    c, s = SCALE * np.cos(ang), SCALE * np.sin(ang)
    for v in (c, s):
        # (16384 cos(0) = 16384.0 and friends are whole numbers: far from a boundary)
        assert boundary_distance(v).min() >= MARGIN_ASSERT, "a direction sits on a rounding boundary"
    return round_half_away(c).astype(np.int32), round_half_away(s).astype(np.int32)


def tables(seed=SEED):
    pattern = draw_pattern(seed)
    C, Sn = direction_tables()
    return rotated_tables(pattern), C, Sn


def header_text(table, C, Sn):
    out = ["/* Generated by tools/make_brief_pattern.py (seed %d): data only, do not edit.  The BRIEF-256 sampling pattern" % SEED,
           " * in its 30 rotations (12 degrees apart), rows (ax, ay, bx, by), and the 30 bin directions scaled by 16384.",
           " * The definition is in include/vo_hip.h. */",
           "#ifndef VO_BRIEF_PATTERN_H",
           "#define VO_BRIEF_PATTERN_H",
           "#define VO_BRIEF_SEED %d" % SEED,
           "#define VO_BRIEF_BINS %d" % N_BINS,
           "#define VO_BRIEF_PAIRS %d" % N_PAIRS,
           "#define VO_BRIEF_COS_INIT { %s }" % ", ".join(str(int(v)) for v in C),
           "#define VO_BRIEF_SIN_INIT { %s }" % ", ".join(str(int(v)) for v in Sn),
           "#define VO_BRIEF_PATTERN_INIT { \\"]
    for k in range(N_BINS):
        flat = table[k].reshape(-1)
        for i in range(0, flat.size, 32):
            out.append("  %s, \\" % ", ".join("%d" % v for v in flat[i:i + 32]))
    out[-1] = out[-1][:-3] + " \\"
    out += ["}", "#endif", ""]
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed header instead of writing it")
    args = ap.parse_args(argv)
    text = header_text(*tables())
    if args.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("brief_pattern.h", "is up to date" if same else "DIFFERS from the generator")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main())
