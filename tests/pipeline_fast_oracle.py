"""CPU oracle of the device-resident frame loop in the FAST + BRIEF tracker mode (tracker_mode = 3): tests/pipeline_oracle.py's
OracleLoop with its tracker replaced by the definitions of the two primitives -- tests/fast_reference.py (FAST-9 corners)
and tests/brief_reference.py (BRIEF-256, Hamming 2-NN with the ratio / distance / first-come rule).  OracleLoop.step calls
`self.tracker.track_features(curr_frame, new)` in its default branch; the subclass installs an object with that method, so
no line of the step is restated here.

TEST INFRASTRUCTURE ONLY: nothing here touches the GPU."""
import numpy as np

import brief_reference
import fast_reference
from pipeline_oracle import OracleLoop

DEFAULT_THRESHOLD, DEFAULT_RATIO, DEFAULT_MAX_DISTANCE = 20, 0.8, 64      # vo/features/fast.py: FASTBRIEFDetector


class FastBriefTracker:
    """What vo/features/fast.py's FASTBRIEFDetector does for a frame pair whose first frame has its features, on the
    definitions: detect (non-maximum suppression on, the N strongest) and describe the new frame, match the current
    descriptors (queries) against the new ones (train rows)."""
    current_pose = None                # (OracleLoop.step sets it for the KLT shell; unused here)

    def __init__(self, n_keypoints, threshold, oriented, ratio, max_distance):
        self.N, self.threshold, self.oriented = int(n_keypoints), int(threshold), bool(oriented)
        self.ratio, self.max_distance = float(ratio), int(max_distance)
        self.frame_counts, self.pair_counts = [], []

    def detect_describe(self, img):
        kp = fast_reference.keypoints(img, self.threshold, True, self.N)[0]
        desc = brief_reference.describe(img, kp, self.oriented)[0]
        return kp, desc

    def track_features(self, curr_frame, new_frame):
        from vo.primitives import Features, Matches
        kp, desc = self.detect_describe(np.asarray(new_frame.image))
        new_frame.features = Features(kp.reshape(-1, 2, 1))
        new_frame.features.descriptors = desc
        d1 = np.asarray(curr_frame.features.descriptors, np.uint8).reshape(curr_frame.features.length, 32)
        pairs = np.asarray(brief_reference.match(d1, desc, self.ratio, self.max_distance), np.int64).reshape(-1, 2)
        self.frame_counts.append(len(kp))
        self.pair_counts.append(len(pairs))
        return Matches(curr_frame, new_frame, pairs if len(pairs) > 0 else np.empty((0, 2), dtype=int))


class FastOracleLoop(OracleLoop):
    """OracleLoop(tracker="fast"): threshold / oriented / max_distance as Pipeline(tracker="fast", fast_threshold=,
    brief_oriented=, brief_max_distance=) takes them once their zeros are resolved (20, False, 64; max_distance < 0: no
    limit)."""

    def __init__(self, stream, n_keypoints, threshold=DEFAULT_THRESHOLD, oriented=False, match_ratio=DEFAULT_RATIO,
                 max_distance=DEFAULT_MAX_DISTANCE, **kw):
        super().__init__(stream, n_keypoints, 15, 2, tracker="fast", match_ratio=match_ratio, **kw)
        self.fast = FastBriefTracker(n_keypoints, threshold, oriented, match_ratio, max_distance)

    def set_state(self, idx, features, curr_pose, prev_pose):
        # (the base class builds a KLT shell around the frame unless the mode is a descriptor mode it knows)
        self.tracker_mode = "harris"
        try:
            super().set_state(idx, features, curr_pose, prev_pose)
        finally:
            self.tracker_mode = "fast"
        self.tracker = self.fast


def initial_fast_features(stream, idx, n_keypoints, threshold=DEFAULT_THRESHOLD, oriented=False):
    """Starting state for the FAST tracker mode, built as pipeline_oracle.initial_features is: the frame's FAST keypoints
    (whole pixels), the first two thirds triangulated from the stream's analytic depth, the rest matched tracks that start
    here, with their BRIEF descriptors ((n, 32) uint8)."""
    from vo.primitives import Features
    K = stream.K
    img = stream.image(idx)
    kp = fast_reference.keypoints(img, threshold, True, n_keypoints)[0].reshape(-1, 2, 1)
    f = Features(keypoints=kp)
    n = f.length
    T = stream.T_world_cam(idx)
    z = stream.depth(idx)[kp[:, 1, 0].astype(int), kp[:, 0, 0].astype(int)].astype(np.float64)
    xc = (kp[:, 0, 0] - K[0, 2]) / K[0, 0] * z
    yc = (kp[:, 1, 0] - K[1, 2]) / K[1, 1] * z
    land = np.stack([T[r, 0] * xc + T[r, 1] * yc + T[r, 2] * z + T[r, 3] for r in range(3)], axis=1)
    n_tri = (2 * n) // 3
    # group order as Matches leaves it: triangulated first, then matched
    f.state = np.concatenate([2 * np.ones(n_tri), np.ones(n - n_tri)])
    f.landmarks[:n_tri] = land[:n_tri].reshape(-1, 3, 1)
    f.tracks = np.concatenate([np.full((n_tri, 2, 1), np.nan), kp[n_tri:]])
    f.poses = np.concatenate([np.full((n_tri, 4, 4), np.nan), np.stack([T] * (n - n_tri))])
    f.descriptors = brief_reference.describe(img, kp[:, :, 0], oriented)[0]
    return f, T
