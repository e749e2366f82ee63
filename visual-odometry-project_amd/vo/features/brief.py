"""Corners + BRIEF-256 binary descriptors + Hamming matching.  The reference has no binary descriptor: this is the
project's own ORB-style front end beside its Harris-patch and SIFT routes, with the same detect-if-missing flow as
HarrisCornerDetector.featureMatcher.  Detection (vo_harris_keypoints or vo_good_features), description
(vo_brief_describe) and the 2-NN search with the ratio / distance / first-come rule (vo_match_hamming_ratio) are HIP
kernels; the definition of the descriptor is in include/vo_hip.h."""
import numpy as np

from vo import _native
from vo.features.harris import _gray
from vo.primitives import Features, Frame, Matches


class BRIEFDetector:
    # Tracker(frame, mode="brief") constructs the detector with its defaults; a caller that wants another count there
    # sets this before (as HarrisCornerDetector._num_keypoints_override)
    _num_keypoints_override = None

    def __init__(self, frame: Frame = None, detector: str = "harris", num_keypoints: int = 1000, oriented: bool = False,
                 match_ratio: float = 0.8, max_distance: int = 64, context=None):
        if detector not in ("harris", "shi_tomasi"):
            raise ValueError("detector must be 'harris' or 'shi_tomasi', not %r" % (detector,))
        self._frame1 = frame
        self._frame2 = frame
        self._detector = detector
        self._num_keypoints = type(self)._num_keypoints_override or num_keypoints
        self._oriented = bool(oriented)
        self._match_ratio = float(match_ratio)
        self._max_distance = int(max_distance)
        self._ctx = context

    def _context(self):
        if self._ctx is None:
            self._ctx = _native.default_context()
        return self._ctx

    def get_brief_matches(self, curr_frame: Frame, new_frame: Frame) -> Matches:
        """Detect + describe on the new frame (and on the current one if it has no features yet), then match."""
        self._frame1, self._frame2 = curr_frame, new_frame
        self._frame1.image = _gray(self._frame1.image)
        self._frame2.image = _gray(self._frame2.image)
        if self._frame1.features is None:
            self._frame1 = self.extractDescriptors(self.extractKeypoints(self._frame1))
        self._frame2 = self.extractDescriptors(self.extractKeypoints(self._frame2))
        return self.matchDescriptor(self._frame1, self._frame2)

    def extractKeypoints(self, frame: Frame) -> Frame:
        """The num_keypoints strongest Harris corners under greedy NMS (HarrisCornerDetector's defaults), or up to that
        many Shi-Tomasi corners (KLTTracker's detector: quality 0.01, minimum distance 8, block 7)."""
        img = _gray(frame.image)
        if self._detector == "harris":
            kp = self._context().harris_keypoints(img, 9, 0.09, self._num_keypoints, 5)
        else:
            kp = self._context().good_features(img, None, self._num_keypoints, 0.01, 8, 7).astype(np.float64)
        assert frame.features is None, "Frame already has features"
        frame.features = Features(kp.reshape(-1, 2, 1))
        return frame

    def extractDescriptors(self, frame: Frame) -> Frame:
        """(N, 32, 1) uint8: one BRIEF-256 descriptor per keypoint, rows index-aligned with the keypoints."""
        kp = frame.features.keypoints
        if kp.shape[0] == 0:
            desc = np.empty((0, 32), np.uint8)
        else:
            desc = self._context().brief_describe(_gray(frame.image), kp[:, :, 0], oriented=self._oriented)
        frame.features.descriptors = desc.reshape(kp.shape[0], 32, 1)
        return frame

    def matchDescriptor(self, frame1: Frame, frame2: Frame) -> Matches:
        """Hamming 2-NN + ratio + distance limit + first-come uniqueness."""
        d1, d2 = frame1.features.descriptors, frame2.features.descriptors
        pairs = self._context().match_hamming_ratio(d1.reshape(len(d1), -1), d2.reshape(len(d2), -1), self._match_ratio,
                                                    self._max_distance)
        m = pairs if len(pairs) > 0 else np.empty(shape=(0, 2), dtype=int)
        return Matches(frame1, frame2, m)
