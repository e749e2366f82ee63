"""The images the SIFT oracle and kernels are compared with the definition of tests/sift_reference.py on, and the
comparisons themselves, shared by tests/test_sift_reference_host.py (oracle) and tests/test_gpu_sift_reference.py (kernels).
TEST INFRASTRUCTURE.

The images are the smallest at which the kernels can go wrong: on and off the tiles of blur2d_rb_kernel (32 x 64),
blur2d_kernel (64 x 32) and extrema_kernel (64 x 16), odd sizes whose halves truncate at every octave, the smallest images
with and without an octave, a strip, windows clipped by every border, the 5-pixel border itself, and flat / saturated /
repeated textures.  The kernels refuse H or W below 16 (include/vo_hip.h); cases smaller than that are host only."""
import functools
import types

import numpy as np

import sift_reference as ref
from scenarios import synthetic_image
from test_oracle_geometry import shift_image

SHARE_COMPARED = 0.8


def ellipses(H, W, specs, bg=20.0):
    """Gaussian blobs (cx, cy, std, aspect, angle, amplitude) on a flat background, rounded to uint8."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.full((H, W), bg)
    for cx, cy, s, asp, th, amp in specs:
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        a += amp * np.exp(-(u * u / (2 * (s * asp) ** 2) + v * v / (2 * s * s)))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def blob_field(H, W, seed, pitch=22, s=(1.3, 3.2), amp=225):
    rng = np.random.default_rng(seed)
    specs = [(x + rng.uniform(-2, 2), y + rng.uniform(-2, 2), rng.uniform(*s), 1.5, rng.uniform(0, np.pi), amp)
             for y in range(pitch // 2, H - 4, pitch) for x in range(pitch // 2, W - 4, pitch)]
    return ellipses(H, W, specs)


def gaussian_blob(H, W, cx, cy, s, amp=200.0, bg=30.0):
    """An isotropic blob whose camera image has std s: rendered with variance s^2 - 0.25 (the 0.5 px nominal blur of the
    input, which the base image's sigma 1 = 2 * 0.5 assumes), amplitude scaled to keep its integral."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    v = s * s - 0.25
    a = bg + amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * v))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def oriented(H, W, cx, cy, phi_deg, s=3.0, amp=40.0):
    """An isotropic blob (the keypoint) on a smooth step that rises along phi, measured clockwise on screen from +x: 7 grey
    levels per pixel at the blob, odd about it (so it adds no difference of Gaussians there) and far stronger than the
    blob's own gradients, which are symmetric about phi anyway once the step's is added."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    phi = np.radians(phi_deg)
    t = (xx - cx) * np.cos(phi) + (yy - cy) * np.sin(phi)
    a = 118 + 84 * np.tanh(t / 12.0) + amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def checker(H, W, sq):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy // sq + xx // sq) % 2) * 255).astype(np.uint8)


def twins(H=64, W=128, shift=64):
    """One compact pattern twice, `shift` pixels apart (a multiple of every octave's step): bit-identical neighbourhoods,
    so tied responses, sizes and angles at positions `shift` apart."""
    a = ellipses(H, shift, [(20, 22, 2.0, 1.5, 0.5, 220), (42, 40, 2.8, 1.4, 2.0, 200), (24, 46, 1.6, 1.6, 1.1, 215)])
    return np.concatenate([a, a], axis=1)[:, :W]


def _border_blobs(H=64, W=64):
    e = 3.3
    specs = [(e, 30.2, 1.6, 1.5, 0.4, 225), (W - 1 - e, 22.4, 1.6, 1.5, 1.3, 225), (28.3, e, 1.6, 1.5, 2.2, 225),
             (36.6, H - 1 - e, 1.6, 1.5, 2.9, 225), (e, e, 1.6, 1.5, 0.8, 225), (W - 1 - e, H - 1 - e, 2.4, 1.4, 2.0, 225),
             (2.25, 48.0, 1.4, 1.4, 0.3, 225), (44.0, 2.25, 1.4, 1.4, 1.9, 225), (32, 32, 3.0, 1.5, 0.7, 225)]
    return ellipses(H, W, specs)


def _case(name, img, note=""):
    img = np.ascontiguousarray(img, np.uint8)
    return types.SimpleNamespace(name=name, img=img, note=note, gpu=min(img.shape) >= 16)


CASES = [
    _case("blocks64x64", synthetic_image(64, 64, 3, block=6, noise=0.0), "one tile of each blur kernel"),
    _case("blocks65x33", synthetic_image(65, 33, 5, block=7, noise=2.0), "one past the tiles"),
    _case("smooth97x131", shift_image(97, 131, 8, 0.0, 0.0)[0], "odd halves at every octave; smooth texture"),
    _case("blobs33x130", blob_field(33, 130, 4), "wide, several extrema tiles"),
    _case("blobs51x77", blob_field(51, 77, 7), "odd halves: 102 51 25 12, 154 77 38 19"),
    _case("borders64x64", _border_blobs(), "windows clipped by each border and two corners; the 5-pixel border"),
    _case("strip16x200", blob_field(16, 200, 2, pitch=16, s=(1.2, 1.8)), "octave count set by the short side"),
    _case("strip14x200", blob_field(14, 200, 3, pitch=14, s=(1.2, 1.6)), "the same below the kernels' smallest height"),
    _case("smallest16x16", ellipses(16, 16, [(7.3, 8.1, 1.5, 1.4, 0.6, 225)]), "the kernels' smallest image"),
    _case("oneoctave12x40", ellipses(12, 40, [(6.2, 5.8, 1.3, 1.3, 0.4, 225), (20.5, 6.1, 1.4, 1.4, 1.7, 225)]), "one octave"),
    _case("smallest7x7", ellipses(7, 7, [(3.2, 3.1, 1.2, 1.2, 0.3, 225)]), "the smallest image with an octave"),
    _case("below6x6", ellipses(6, 6, [(3, 3, 1.2, 1.2, 0.3, 225)]), "no octave: zero keypoints, no error"),
    _case("flat40x40", np.full((40, 40), 128, np.uint8), "flat"),
    _case("checker48x48", checker(48, 48, 8), "saturated 0 / 255; corners with several orientation peaks"),
    _case("twins64x128", twins(), "one pattern twice: tied responses"),
    _case("faint40x72", ellipses(40, 72, [(12 + 16 * i, 20, 2.0, 1.3, 0.5 * i, 10.0 + 1.5 * i) for i in range(4)]),
          "extrema with |D| between the threshold floor(1.7) = 1 and 1.7: candidates that the contrast test then rejects"),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
GPU_NAMES = [c.name for c in CASES if c.gpu]

#: analytic blobs (H, W, cx, cy, std): whole and fractional centres; std 9 puts layer + xi above 3.3 -- the largest
#: orientation and descriptor radii the defaults can produce
BLOBS = [(96, 112, 40.0, 44.0, 3.0), (96, 112, 40.3, 44.6, 3.0), (96, 112, 52.0, 47.0, 4.5), (96, 112, 52.7, 47.2, 4.5),
         (96, 112, 50.0, 48.0, 6.0), (96, 112, 50.4, 48.8, 6.0), (96, 112, 56.0, 48.0, 9.0), (96, 112, 55.6, 47.3, 9.0),
         (96, 112, 56.0, 48.0, 8.0), (96, 112, 55.6, 47.3, 8.0)]
ORIENTATIONS = [30.0, 100.0, 200.0, 310.0, 0.0, 90.0, 180.0, 270.0]


@functools.lru_cache(maxsize=None)
def definition(name, atan2="cv"):
    """The definition's run on a case, computed once and shared."""
    return ref.detect(BY_NAME[name].img, atan2=atan2)


@functools.lru_cache(maxsize=None)
def definition_of(key):
    """The same for the analytic images: key = ("blob", H, W, cx, cy, s), ("ori", phi) or ("T", case name)."""
    return ref.detect(image_of(key))


def image_of(key):
    if key[0] == "blob":
        return gaussian_blob(*key[1:])
    if key[0] == "ori":
        return oriented(64, 72, 33.0, 30.0, key[1])
    if key[0] == "T":
        return np.ascontiguousarray(BY_NAME[key[1]].img.T)
    raise KeyError(key)


# ---------------------------------------------------------------- comparisons
def angle_diff(a, b):
    return abs((a - b + 180.0) % 360.0 - 180.0)


def desc_distance(k, desc_row):
    """How far a rounded, saturated descriptor row is from the definition's unrounded entries, beyond the half unit of
    rounding: entries the definition has above 255 must come back as 255, none may be negative."""
    want = np.clip(np.asarray(k.desc_raw, np.float64), 0, 255)
    return float(np.max(np.abs(np.asarray(desc_row, np.float64) - want)) - 0.5)


def unique_keypoints(d):
    """The keypoints the definition returns: accepted records, one per final (octave, layer, position, bin) -- two
    candidates that refine to the same point give equal rows, which the duplicate rule merges."""
    seen, out = set(), []
    for k in d.keypoints:
        key = (k.octave, k.layer, k.r, k.c, k.bin)
        if k.accepted and key not in seen:
            seen.add(key)
            out.append(k)
    return out


def check_stages(c, d, stages, figures=None):
    """One case's oracle stages (oracle.native.sift_stages per octave, None past the last) against the definition run d:
    Gaussian and DoG images within eps_G / eps_D; the number of extrema beyond the threshold between the definition's
    decided and all candidates; each accepted oracle keypoint has the definition's record of the same
    (octave, layer, position, bin); every decided keypoint of the definition is there exactly once; on those with the same
    path, offset, size and response within twice their bounds, the smoothed histogram within HIST_TOL of its maximum and
    the angle within ANGLE_TOL.  Returns the share of the definition's keypoints compared."""
    fig = figures if figures is not None else {}
    for key in ("G", "D", "offset", "size", "response", "hist", "angle"):
        fig.setdefault(key, 0.0)
    assert len(stages) == len(d.pyramid) + 1 and stages[-1] is None, "octave count"
    records = {}
    for k in d.keypoints:
        records.setdefault((k.octave, k.layer, k.r, k.c, k.bin), k)
    found = {}
    for o, (G, D, kp, hist, n_ext) in enumerate(stages[:-1]):
        Gd, Dd = d.pyramid[o]
        cand = ref.candidates(Dd, d.eps_d[o])
        sure = sum(1 for q in cand if q[3] > 2 * q[4])
        assert sure <= n_ext <= len(cand), "%s octave %d: %d extrema, the definition %d to %d" % (c.name, o, n_ext, sure, len(cand))
        fig["extrema"] = fig.get("extrema", 0) + n_ext
        fig["extrema decided"] = fig.get("extrema decided", 0) + sure
        assert G.shape == Gd.shape, "octave %d size" % o
        for i in range(ref.NG):
            fig["G"] = max(fig["G"], float(np.abs(G[i] - Gd[i]).max() / d.eps_g[o][i]))
        for i in range(ref.NG - 1):
            fig["D"] = max(fig["D"], float(np.abs(D[i] - Dd[i]).max() / d.eps_d[o][i]))
        assert fig["G"] <= 1 and fig["D"] <= 1, "%s octave %d: pyramid off by %.3g / %.3g of its bound" % (c.name, o, fig["G"], fig["D"])
        for q, h in zip(kp, hist):
            key = tuple(int(v) for v in q[[0, 1, 2, 3, 7]])
            k = records.get(key)
            assert k is not None, "%s: oracle keypoint %s has no counterpart in the definition" % (c.name, key)
            if key in found:                 # the same point reached from a second candidate: an exact duplicate
                continue
            step = 2.0 ** o * 0.5
            share = {"offset": float(np.abs(q[[6, 5, 4]] - k.x).max() / (2 * k.xy_bound / step)),
                     "size": abs(q[9] * 0.5 - k.size) / (2 * k.size_bound),
                     "response": abs(q[10] - k.response) / (2 * k.resp_bound)}
            if int(q[11]) == k.ori_radius:
                share["hist"] = float(np.abs(h - k.hist).max() / k.hist.max() / ref.HIST_TOL)
                share["angle"] = angle_diff(float(q[8]), k.angle) / ref.ANGLE_TOL
            else:
                assert not k.decided, "%s: orientation radius %d, definition %d" % (c.name, q[11], k.ori_radius)
            if k.why == "bin tie":           # which bin its tied gradients fall into is rounding: the rest is compared
                share.pop("hist", None), share.pop("angle", None)
            for name, v in share.items():
                fig[name] = max(fig[name], float(v))
                assert v <= 1 or not k.decided, "%s %s: %s off by %.3g of its bound" % (c.name, key, name, v)
            found[key] = 1 if all(v <= 1 for v in share.values()) else -1
    uniq = unique_keypoints(d)
    for k in uniq:
        if k.decided:
            assert found.get((k.octave, k.layer, k.r, k.c, k.bin)) == 1, \
                "%s: decided keypoint octave %d layer %d (%d, %d) bin %d missing" % (c.name, k.octave, k.layer, k.c, k.r, k.bin)
    compared = sum(found.get((k.octave, k.layer, k.r, k.c, k.bin)) == 1 for k in uniq)
    fig["keypoints"], fig["decided"], fig["compared"] = len(uniq), sum(k.decided for k in uniq), compared
    share = compared / len(uniq) if uniq else 1.0
    assert share >= SHARE_COMPARED, "%s: only %d of %d keypoints compared" % (c.name, compared, len(uniq))
    return share


def check_rows(d, kp, desc, figures=None, what="rows"):
    """The end-to-end comparison of final rows (kp (n, 6), desc (n, 128)) with a definition run d:
      - the rows are in the definition's final order and hold no duplicate;
      - every decided keypoint of the definition is found exactly once: same octave, x, y, size and response within twice
        their bounds, angle within ANGLE_TOL, descriptor within 0.5 + DESC_TOL;
      - every row has a counterpart among the definition's records, decided or not (within 1.5 octave pixels);
      - at least SHARE_COMPARED of the keypoints the definition returns are compared in that way.
    Returns the share compared."""
    kp = np.asarray(kp, np.float64).reshape(-1, 6)
    assert np.array_equal(ref.finish(kp.astype(np.float32)), np.arange(len(kp))), "%s: not in the final order" % what
    fig = figures if figures is not None else {}
    for key in ("xy", "size", "response", "angle", "desc"):
        fig.setdefault(key, 0.0)
    used = np.zeros(len(kp), bool)
    accepted = unique_keypoints(d)
    compared = 0
    for k in sorted(accepted, key=lambda k: not k.decided):
        hits = []
        for q in np.nonzero(kp[:, 5] == k.octave - 1)[0]:
            share = {"xy": max(abs(kp[q, 0] - k.xy[0]), abs(kp[q, 1] - k.xy[1])) / (2 * k.xy_bound),
                     "size": abs(kp[q, 2] - k.size) / (2 * k.size_bound),
                     "response": abs(kp[q, 4] - k.response) / (2 * k.resp_bound),
                     "angle": angle_diff(kp[q, 3], k.angle) / ref.ANGLE_TOL,
                     "desc": desc_distance(k, desc[q]) / ref.DESC_TOL}
            if all(v <= 1 for v in share.values()):
                hits.append((q, share))
        if k.decided:
            assert len(hits) == 1, ("%s: decided keypoint octave %d layer %d (%d, %d) bin %d found %d times"
                                    % (what, k.octave, k.layer, k.c, k.r, k.bin, len(hits)))
        if len(hits) == 1:
            compared += 1
            used[hits[0][0]] = True
            for key, v in hits[0][1].items():
                fig[key] = max(fig[key], float(v))
    for q in np.nonzero(~used)[0]:
        step = 2.0 ** (kp[q, 5] + 1) * 0.5
        near = [k for k in d.keypoints if k.octave - 1 == kp[q, 5]
                and max(abs(kp[q, 0] - k.xy[0]), abs(kp[q, 1] - k.xy[1])) <= 1.5 * step + 2 * k.xy_bound]
        near += [r for r in d.rejected if not r.decided and r.octave - 1 == kp[q, 5]
                 and max(abs(kp[q, 0] / step - r.trajectory[-1][2]), abs(kp[q, 1] / step - r.trajectory[-1][1])) <= 2.5]
        assert near, "%s: row %d %s has no counterpart in the definition" % (what, q, kp[q])
    fig["keypoints"], fig["decided"], fig["compared"] = len(accepted), sum(k.decided for k in accepted), compared
    share = compared / len(accepted) if accepted else 1.0
    assert share >= SHARE_COMPARED, "%s: only %d of %d keypoints compared" % (what, compared, len(accepted))
    if not accepted:
        assert len(kp) == 0 or not used.all()
    return share


def check_cap(kp_all, kp_capped, cap):
    """A capped run against the definition's cap rule applied to the uncapped rows of the same implementation."""
    kp_all = np.asarray(kp_all, np.float32).reshape(-1, 6)
    want = kp_all[ref.finish(kp_all, cap)]
    assert np.array_equal(np.asarray(kp_capped, np.float32).reshape(-1, 6), want), "cap %d: not the definition's choice" % cap


def tied_cap(kp_all):
    """A cap that falls inside a run of tied responses, or None."""
    resp = np.sort(np.asarray(kp_all)[:, 4])[::-1]
    for i in range(len(resp) - 1):
        if resp[i] == resp[i + 1]:
            return i + 1
    return None


def transpose_descriptor(desc):
    """The descriptor of the transposed image's keypoint from the original's: the frame's row axis flips and angles run
    the other way -- entry (i, j, k) comes from (3 - i, j, (8 - k) mod 8)."""
    d = np.asarray(desc).reshape(-1, 4, 4, 8)
    return d[:, ::-1, :, (8 - np.arange(8)) % 8].reshape(np.shape(desc))


@functools.lru_cache(maxsize=None)
def measure_rounding():
    """The largest distance between the float64 and the float32 run of the definition, per case and over all of them, on
    keypoints both runs reach by the same path (octave, layer, position, histogram bin, both radii) and that have no gradient on a boundary between histogram bins ("bin tie"): smoothed histogram
    value relative to the histogram's maximum, angle in degrees, unrounded descriptor entry."""
    out = {}
    for c in CASES:
        a = definition(c.name)
        b = ref.detect(c.img, ft=np.float32)
        other = {(k.octave, k.layer, k.r, k.c, k.bin, k.ori_radius, k.desc_radius): k for k in b.keypoints}
        fig = {"hist": 0.0, "angle": 0.0, "desc": 0.0, "n": 0}
        for k in a.keypoints:
            m = other.get((k.octave, k.layer, k.r, k.c, k.bin, k.ori_radius, k.desc_radius))
            if m is None or not k.accepted or k.why == "bin tie":
                continue
            fig["n"] += 1
            fig["hist"] = max(fig["hist"], float(np.abs(k.hist - m.hist).max() / k.hist.max()))
            fig["angle"] = max(fig["angle"], angle_diff(k.angle, m.angle))
            fig["desc"] = max(fig["desc"], float(np.abs(k.desc_raw - m.desc_raw).max()))
        out[c.name] = fig
    out["all"] = {q: max(f[q] for f in out.values()) for q in ("hist", "angle", "desc")}
    return out
