"""CPU oracle of the device-resident frame loop with the Shi-Tomasi re-detect (vo_pipeline_config.detector = 1): the
reference's KLT mode as it is (src/vo/features/klt.py:207-230 refills with cv2.goodFeaturesToTrack and sets
_num_features to the count it got, klt.py:114).  tests/pipeline_oracle.py's OracleLoop, unchanged, around the product's
KLTTracker shell with _detector = "shi-tomasi", whose corners come from oracle/csrc/goodfeatures.c.

The cases (CASES) are the smallest that separate "the detector returned its cap" from "it returned fewer, a different
count per sequence": 240 x 320, six frames, 300 keypoints at most, a start state below the detector's count.

TEST INFRASTRUCTURE ONLY: nothing here touches the GPU."""
import numpy as np

from oracle import native
from pipeline_oracle import OracleContext, OracleLoop, initial_features

N, WIN, LEVELS, FRAMES, H, W, STEPS = 300, 15, 2, 6, 240, 320, 7

# name: (Stream keywords, qualityLevel, minDistance, start fraction, the step that re-detects (index into the order's
#        pairs), corners appended = _num_features afterwards)
CASES = {
    "A": (dict(), 0.01, 8, 0.83, 2, 300),
    "B": (dict(), 0.01, 14, 0.83, 2, 226),
    "C": (dict(seed=2030, start=1), 0.01, 14, 0.83, 2, 236),
    "D": (dict(), 0.01, 20, 0.83, 2, 121),
    "E": (dict(), 0.01, 8, 0.83, 3, 500),          # at 480 x 640 with 500 keypoints (SIZES), five steps
}
SIZES = {"E": (480, 640, 500, 5)}                  # (H, W, N, steps) where they are not the module's


class ShiTomasiContext(OracleContext):
    """OracleContext plus the call KLTTracker.find_corners makes for Shi-Tomasi corners; remembers what it returned."""

    def __init__(self):
        self.calls, self.last = 0, None

    def good_features(self, img, mask=None, max_corners=500, quality=0.01, min_distance=8, block_size=7):
        self.calls += 1
        self.last = native.good_features(img, mask, max_corners, quality, min_distance, block_size)
        return self.last


def make_tracker(frame, n_keypoints, win, max_level, redetect_start_pose, quality, min_distance, block):
    from vo.features.klt import KLTTracker, TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS

    class OracleShiTomasiKLT(KLTTracker):
        _detector = "shi-tomasi"
        _feature_params = dict(maxCorners=n_keypoints, qualityLevel=quality, minDistance=min_distance, blockSize=block)
        _lk_params = dict(winSize=(win, win), maxLevel=max_level,
                          criteria=(TERM_CRITERIA_EPS | TERM_CRITERIA_COUNT, 10, 0.03))
        current_pose = None

        def update_features(self, new_keypoints):       # (as pipeline_oracle.make_tracker's: redetect_start_pose)
            feats = super().update_features(new_keypoints)
            if redetect_start_pose == "current" and len(new_keypoints) > 0:
                poses = feats.poses.copy()
                poses[-len(new_keypoints):] = self.current_pose
                feats.poses = poses
            return feats

    return OracleShiTomasiKLT(frame, context=ShiTomasiContext())


class ShiTomasiLoop(OracleLoop):
    def __init__(self, stream, n_keypoints, win, max_level, quality=0.01, min_distance=8, block=7, **kw):
        super().__init__(stream, n_keypoints, win, max_level, **kw)
        self.st = dict(quality=quality, min_distance=min_distance, block=block)

    def set_state(self, idx, features, curr_pose, prev_pose):
        import copy
        from vo.primitives import State
        f = self.frame(idx, copy.deepcopy(features))
        self.state = State(f, bearing_threshold=self.cfg["bearing"])
        self.state.curr_pose = np.array(curr_pose, np.float64)
        self.state.prev_pose = np.array(prev_pose, np.float64)
        self.state.prev_frame = f
        self.tracker = make_tracker(self.frame(idx), self.cfg["N"], self.cfg["win"], self.cfg["lvl"], self.cfg["redetect"],
                                    **self.st)
        self.tracker._num_features = self.cfg["N"]      # (what Pipeline.set_state hands over by default)

    def step(self, next_idx):
        """OracleLoop.step's dict plus redetected, appended (corners the step's re-detect found; 0 without one),
        detection (those corners, (n, 2) float32, or None) and num_features (_num_features after the step)."""
        ctx = self.tracker._ctx
        calls = ctx.calls
        ref = super().step(next_idx)
        ref["redetected"] = int(ctx.calls > calls)
        ref["detection"] = ctx.last if ref["redetected"] else None
        ref["appended"] = len(ctx.last) if ref["redetected"] else 0
        ref["num_features"] = self.tracker._num_features
        return ref


def start_state(stream, n_keypoints, fraction=1.0):
    """initial_features of frame 0, evenly subsampled to `fraction` (tests/test_gpu_pipeline.py's start_state)."""
    import copy
    feats, T = initial_features(stream, 0, n_keypoints)
    if fraction < 1.0:
        keep = np.zeros(feats.length, dtype=bool)
        keep[np.linspace(0, feats.length - 1, int(fraction * feats.length)).astype(int)] = True
        feats = copy.deepcopy(feats)
        feats.mask(keep)
    return feats, T


def case(name, redetect_start_pose="current", fraction=None, **loop_kw):
    """(stream, start features, start pose, loop ready at frame 0, the frame pairs of stream.order(STEPS)) of one of CASES."""
    from vo import synthetic
    skw, quality, min_distance, frac, _, _ = CASES[name]
    h, w, n, steps = SIZES.get(name, (H, W, N, STEPS))
    stream = synthetic.Stream(FRAMES, h, w, **skw)
    feats, T = start_state(stream, n, frac if fraction is None else fraction)
    loop = ShiTomasiLoop(stream, n, WIN, LEVELS, quality=quality, min_distance=min_distance, refine_iters=20,
                         redetect_start_pose=redetect_start_pose, **loop_kw)
    loop.set_state(0, feats, T, T)
    order = stream.order(steps)
    return stream, feats, T, loop, list(zip(order[:-1], order[1:]))


_runs = {}


def run_case(name, redetect_start_pose="current", fraction=None):
    """The whole oracle run of a case, computed once per process and shared (read-only) by the tests that compare
    against it: (stream, start features, start pose, pairs, [the dict of every step])."""
    key = (name, redetect_start_pose, fraction)
    if key not in _runs:
        stream, feats, T, loop, pairs = case(name, redetect_start_pose, fraction)
        refs = []
        import copy
        for _, b in pairs:
            ref = loop.step(b)
            ref["generator"] = loop.rs.rng.bit_generator.state
            ref["features"] = copy.deepcopy(ref["features"])
            refs.append(ref)
        _runs[key] = (stream, feats, T, pairs, refs)
    return _runs[key]
