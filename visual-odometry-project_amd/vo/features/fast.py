"""FAST-9 corners + BRIEF-256 + Hamming matching: BRIEFDetector with the segment-test detector of csrc/fast.hip in front
(vo_fast_keypoints: integer scores, 3 x 3 suppression, the num_keypoints strongest).  The reference has no such detector;
the definition is in include/vo_hip.h.  Describing and matching are BRIEFDetector's, unchanged."""
from vo.features.brief import BRIEFDetector
from vo.features.harris import _gray
from vo.primitives import Features, Frame


class FASTBRIEFDetector(BRIEFDetector):
    _num_keypoints_override = None

    def __init__(self, frame: Frame = None, threshold: int = 20, num_keypoints: int = 1000, oriented: bool = False,
                 match_ratio: float = 0.8, max_distance: int = 64, context=None):
        super().__init__(frame, "harris", num_keypoints, oriented, match_ratio, max_distance, context)
        self._detector = "fast"
        self._threshold = int(threshold)

    def extractKeypoints(self, frame: Frame) -> Frame:
        """Up to num_keypoints FAST-9 corners: the strongest survivors of the 3 x 3 suppression, (score descending, index
        ascending)."""
        kp = self._context().fast_keypoints(_gray(frame.image), self._threshold, self._num_keypoints, nonmax=True)
        assert frame.features is None, "Frame already has features"
        frame.features = Features(kp.reshape(-1, 2, 1))
        return frame
