"""CPU: the forward-backward check of the tracker (include/vo_hip.h, "pyramidal KLT": vo_klt_track_fb) -- every case of
tests/klt_fb_cases.py still holds the edge it exists for (on the oracle), the composed oracle returns the forward call's
arrays untouched, KLTTracker makes the call only when asked to, the C ABI is declared, exported and bound, and the oracle
loop the GPU test compares with really differs from the plain one."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import klt_fb_cases as fc
import klt_fb_oracle as fbo
from oracle import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the loop of tests/test_gpu_pipeline_klt_fb.py: stream, start and threshold (a test parameter, not a default)
LOOP = dict(H=240, W=320, N=300, hyp=256, F=6, steps=8, frac=0.83, win=15, lvl=2, fb_max=1.0, redetect="current")


@pytest.mark.parametrize("name", fc.NAMES)
def test_case_keeps_its_edge(name):
    fc.GUARDS[name]()
    assert fc.DOCS[name]
    c = fc.BY_NAME[name]
    assert max(c.prev.shape) <= 136 and len(c.pts) <= 620 and c.prev.shape == c.nxt.shape


@pytest.mark.parametrize("name", fc.NAMES)
def test_fb_track_returns_the_forward_call_bit_for_bit(name):
    c = fc.BY_NAME[name]
    nxy, st, err, fb = fc.expected(c)
    f_xy, f_st, f_err = native.klt_track(c.prev, c.nxt, c.pts, **fc.case_args(c))
    assert np.array_equal(nxy.view(np.uint32), f_xy.view(np.uint32)) and np.array_equal(err.view(np.uint32), f_err.view(np.uint32))
    assert not np.any(st.astype(bool) & ~f_st.astype(bool)), "the check only ever removes points"
    assert np.all(np.isposinf(fb[f_st == 0])) and fb.dtype == np.float32 and st.dtype == np.uint8
    keep = np.isfinite(fb)
    assert np.array_equal(st[keep] == 1, fb[keep] <= np.float32(c.fb_max * c.fb_max))


def test_rule_arithmetic_is_float32_in_the_stated_order():
    pts = np.array([[10.25, 20.5], [0.1, 0.2], [5.0, 5.0], [1.0, 1.0]], np.float32)
    back = np.array([[10.75, 20.0], [0.1000001, 0.2], [np.float32(5.0) + np.float32(1e-3), 5.0], [2.0, 1.0]], np.float32)
    st, fb = fbo.compare(pts, back, [1, 1, 1, 0], [1, 1, 1, 1], np.float32(0.5))
    dx, dy = back[:, 0] - pts[:, 0], back[:, 1] - pts[:, 1]
    want = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
    assert np.array_equal(fb[:3].view(np.uint32), want[:3].view(np.uint32)) and np.isposinf(fb[3])
    assert st.tolist() == [1, 1, 1, 0] and fb[0] == np.float32(0.5)          # (0.25 + 0.25: the tie is kept)
    assert fbo.compare(pts, back, [1, 1, 1, 0], [1, 1, 1, 1], np.nextafter(np.float32(0.5), np.float32(0)))[0].tolist() == [0, 1, 1, 0]
    assert fbo.compare(pts, back, [1, 1, 1, 0], [1, 1, 1, 1], np.float32(np.inf))[0].tolist() == [1, 1, 1, 0]
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            fbo.check_fb_max(bad)
    assert fbo.check_fb_max(float("inf")) == np.float32(np.inf) and fbo.check_fb_max(3.0) == np.float32(9.0)


# ---- KLTTracker on the oracle context ----

class CountingContext(fbo.FBOracleContext):
    def __init__(self):
        super().__init__()
        self.calls = []

    def klt_track(self, *a, **kw):
        self.calls.append(("klt_track", a, kw))
        return super().klt_track(*a, **kw)

    def klt_track_fb(self, *a, **kw):
        self.calls.append(("klt_track_fb", a, kw))
        return super().klt_track_fb(*a, **kw)


def _tracker_pair(fb_threshold):
    from pipeline_oracle import make_tracker
    from vo import synthetic
    from vo.primitives import Frame
    from vo.sensors import Camera
    stream = synthetic.Stream(2, 120, 160)
    cam = Camera(intrinsic_matrix=stream.K)
    f0, f1 = (Frame(stream.image(i), sensor=cam, intrinsics=stream.K) for i in (0, 1))
    trk = make_tracker(f0, 150, 15, 2)
    trk._ctx = CountingContext()
    if fb_threshold is not None:
        trk._fb_threshold = fb_threshold
    kp = f0.features.keypoints.copy()
    matches = trk.track_features(f0, f1)
    return stream, trk, kp, matches


def test_tracker_without_threshold_makes_todays_call():
    from vo.features.klt import KLTTracker
    assert KLTTracker._fb_threshold is None and KLTTracker._error_threshold == 100
    stream, trk, kp, matches = _tracker_pair(None)
    calls = trk._ctx.calls
    assert [c[0] for c in calls] == ["klt_track"] and trk._ctx.fb_calls == 0
    name, a, kw = calls[0]
    assert len(a) == 3 and kw == dict(win=15, max_level=2, max_iter=10, eps=0.03)        # (the call as it always was)
    nxy, st, err = native.klt_track(stream.image(0), stream.image(1), kp.reshape(-1, 2).astype(np.float32), win=15, max_level=2,
                                    max_iter=10, eps=0.03)
    keep = st.astype(bool) & (err < 100)
    assert np.array_equal(matches.frame2.features.keypoints[:, :, 0], nxy[keep])


def test_tracker_with_threshold_keeps_the_rules_status():
    stream, trk, kp, matches = _tracker_pair(1.0)
    assert [c[0] for c in trk._ctx.calls] == ["klt_track_fb"] and trk._ctx.calls[0][2]["fb_max"] == 1.0
    nxy, st, err, fb = fbo.fb_track(stream.image(0), stream.image(1), kp.reshape(-1, 2).astype(np.float32), 15, 2, 10, 0.03, 1e-4, 1.0)
    keep = st.astype(bool) & (err < 100)
    assert np.array_equal(matches.frame2.features.keypoints[:, :, 0], nxy[keep])
    assert np.array_equal(matches.frame1.features.keypoints[:, :, 0], kp.reshape(-1, 2)[keep])
    assert trk._ctx.rejected[0] >= 1 and keep.sum() >= 20, "the pair was meant to lose points to the check, and keep some"


# ---- C ABI, ctypes table, Python surface ----

NAMES = {"vo_klt_track_fb": 17, "vo_klt_track_fb_dev": 19, "vo_pipeline_set_klt_fb": 2, "vo_pipeline_get_klt_fb": 2}


def test_abi_is_declared_exported_and_bound():
    from vo import _native
    from vo._pipeline import Pipeline
    doc = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = _native.load()
    for name, n_args in NAMES.items():
        declared = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        res, args = _native._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(declared.split(",")) == n_args, name
        assert hasattr(lib, name), name
    fb = re.search(r"\bint\s+vo_klt_track_fb\s*\(([^;]*)\)", text).group(1)
    plain = re.search(r"\bint\s+vo_klt_track\s*\(([^;]*)\)", text).group(1)
    strip = lambda s: [re.sub(r"\s+", " ", p).strip() for p in s.split(",")]
    assert strip(fb) == strip(plain)[:12] + ["double fb_max"] + strip(plain)[12:] + ["float* fb"]
    assert _native._SIGS["vo_klt_track_fb"][1][12] is ctypes.c_double and _native._SIGS["vo_klt_track_fb_dev"][1][14] is ctypes.c_double
    # the rule stands under "pyramidal KLT", and the bootstrap's exemption is stated
    sect = doc[doc.index("---- pyramidal KLT"):doc.index("---- DLT triangulation")]
    for phrase in ("fb_max > 0", "status_f & status_b & (fb[i] <= thr2)", "A tie is kept", "+inf where status_f = 0 or status_b = 0",
                   "product formed in double", "bootstrap"):
        assert phrase in sect, phrase
    assert "vo_pipeline_config" in doc and "klt_fb" not in doc[doc.index("typedef struct vo_pipeline_config"):doc.index("} vo_pipeline_config;")]
    assert all(callable(getattr(_native.Context, k)) for k in ("klt_track_fb", "klt_track_fb_dev"))
    assert callable(Pipeline.set_klt_fb) and isinstance(Pipeline.klt_fb, property)


class FakeLib:
    def __init__(self):
        self.calls, self.value = [], 0.0

    def vo_pipeline_set_klt_fb(self, h, v):
        self.calls.append(v)
        self.value = v
        return 0

    def vo_pipeline_get_klt_fb(self, h, ref):
        ref._obj.value = self.value
        return 0


def test_pipeline_setter_checks_its_argument_before_the_library():
    from vo._pipeline import Pipeline
    lib = FakeLib()
    errors = []
    pipe = object.__new__(Pipeline)
    pipe._h = None
    pipe.ctx = types.SimpleNamespace(_lib=lib, _chk=lambda rc: errors.append(rc) if rc else None)
    for bad in (-1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="fb_max"):
            pipe.set_klt_fb(bad)
    with pytest.raises((TypeError, ValueError)):
        pipe.set_klt_fb(None)
    assert lib.calls == []
    pipe.set_klt_fb(1.5)
    assert pipe.klt_fb == 1.5
    pipe.set_klt_fb(float("inf"))
    pipe.set_klt_fb(0)
    assert lib.calls == [1.5, float("inf"), 0.0] and pipe.klt_fb == 0.0 and not errors and isinstance(lib.calls[2], float)


def test_drivers_take_klt_fb_and_refuse_bad_values():
    import inspect
    from vo import driver
    for fn in (driver.run_on_device, driver.run_batch_on_device):
        assert inspect.signature(fn).parameters["klt_fb"].default is None
    from vo.primitives import Sequence
    seq = Sequence("synthetic", n_frames=4, height=120, width=160)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="klt_fb"):
            driver.run_on_device(seq, klt_fb=bad)            # (refused before anything is built)


# ---- the loop guard ----

OTHER_WINDOWS = (9, 17, 21)          # the generic kernel and the two other row kernels (LOOP's 15 is the third)


def loop_start():
    """Stream, thinned start features and start pose of the loop; the same for every window (the start does not track)."""
    import copy
    from pipeline_oracle import initial_features
    from vo import synthetic
    p = LOOP
    stream = synthetic.Stream(p["F"], p["H"], p["W"])
    feats, T = initial_features(stream, 0, p["N"])
    keep = np.zeros(feats.length, dtype=bool)
    keep[np.linspace(0, feats.length - 1, int(p["frac"] * feats.length)).astype(int)] = True
    feats = copy.deepcopy(feats)
    feats.mask(keep)
    return stream, feats, T


def oracle_loop(stream, fb_max, seed=2023, win=LOOP["win"]):
    from pipeline_oracle import OracleLoop
    p = dict(LOOP, win=win)
    kw = dict(refine_iters=20, redetect_start_pose=p["redetect"], seed=seed)
    if fb_max is None:
        return OracleLoop(stream, p["N"], p["win"], p["lvl"], **kw)
    return fbo.FBOracleLoop(stream, p["N"], p["win"], p["lvl"], fb_max=fb_max, **kw)


@pytest.mark.parametrize("fb_max", [None, LOOP["fb_max"]], ids=["plain", "fb"])
@pytest.mark.parametrize("win", OTHER_WINDOWS)
def test_oracle_loops_redetect_at_the_other_windows(win, fb_max):
    """What tests/test_gpu_pipeline_klt_windows.py needs of the reference alone: at windows 9, 17 and 21 the loop's tracked
    count rises in at least one step, which only a re-detect does (measured: one such step plain, two with the check, at
    every window)."""
    stream, feats, T = loop_start()
    orc = oracle_loop(stream, fb_max, win=win)
    assert orc.cfg["win"] == win and LOOP["win"] == 15
    orc.set_state(0, feats, T, T)
    counts = [orc.step(b)["n_tracked"] for b in stream.order(LOOP["steps"])[1:]]
    rises = sum(1 for a, b in zip(counts[:-1], counts[1:]) if b > a)
    print("window", win, "fb" if fb_max else "plain", counts, "rises", rises)
    assert rises >= 1, counts


def test_fb_oracle_loop_drops_features_the_plain_loop_keeps():
    """On the stream and threshold of the GPU loop test: in at least two steps the check drops a feature that
    status & err < 100 keeps, a re-detect among the steps; and the two loops' feature counts differ."""
    stream, feats, T = loop_start()
    order = stream.order(LOOP["steps"])
    plain, fb = oracle_loop(stream, None), oracle_loop(stream, LOOP["fb_max"])
    counts = []
    for orc in (plain, fb):
        orc.set_state(0, feats, T, T)
        counts.append([orc.step(b)["n_tracked"] for b in order[1:]])
    ctx = fb.tracker._ctx
    assert isinstance(ctx, fbo.FBOracleContext) and fb.tracker._fb_threshold == LOOP["fb_max"]
    assert ctx.fb_calls == len(order) - 1 == LOOP["steps"]
    assert sum(1 for r in ctx.rejected if r >= 1) >= 2, ctx.rejected
    assert counts[0][0] > counts[1][0], "the first step already differs"
    assert counts[0] != counts[1]
    assert any(b > a for a, b in zip(counts[1][:-1], counts[1][1:])), "a re-detect was meant to run in the FB loop"
