"""-m gpu: the BRIEF front end through the drop-in classes.  BRIEFDetector.get_brief_matches against the definition
composed on the CPU from the same keypoints, the Tracker's dispatch, and the class driver on the reference's six KITTI
frames under the bars the klt / harris / sift modes meet in tests/test_gpu_kitti.py.

The driver's defaults come from the CPU figures of tests/test_brief_host.py (1000 Harris keypoints, not oriented, ratio
0.8, max_distance 64: 577 pairs on frames 0 and 2, 97.75 % within 2 px of the ground-truth epipolar geometry, against 569
pairs and 96.84 % for the patch route that passes the same bars).  The rest of the class driver (8-point RANSAC, P3P,
refinement, DLT) runs on the device only, so the chain cannot be composed on the CPU: the bars are first met here."""
import numpy as np
import pytest

import brief_reference as ref
from kitti_fixture import make_kitti_dir
from test_gpu_kitti import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    yield _native.default_context()


@pytest.fixture(scope="module")
def frames():
    from vo import synthetic
    stream = synthetic.Stream(2, 240, 320)
    return stream.image(0), stream.image(1)


@pytest.mark.parametrize("detector,oriented", [("harris", False), ("harris", True), ("shi_tomasi", False)])
def test_get_brief_matches_equals_the_definition(ctx, frames, detector, oriented):
    from vo.features import BRIEFDetector
    from vo.primitives import Frame, Matches
    a, b = frames
    det = BRIEFDetector(detector=detector, num_keypoints=300, oriented=oriented, match_ratio=0.85, max_distance=70, context=ctx)
    # the same keypoints, described and matched by the definition
    fa, fb = det.extractKeypoints(Frame(a.copy())), det.extractKeypoints(Frame(b.copy()))
    ka, kb = fa.features.keypoints.copy(), fb.features.keypoints.copy()
    assert ka.shape[1:] == (2, 1) and ka.dtype == np.float64 and 30 < len(ka) <= 300
    da, db = ref.describe(a, ka[:, :, 0], oriented)[0], ref.describe(b, kb[:, :, 0], oriented)[0]
    pairs = ref.match(da, db, 0.85, 70)
    assert len(pairs) > 30
    got = det.extractDescriptors(fa).features.descriptors
    assert got.shape == (len(ka), 32, 1) and got.dtype == np.uint8 and np.array_equal(got[:, :, 0], da)
    # ... and the whole flow on fresh frames: detect-if-missing, describe, match, regroup
    f1, f2 = Frame(a.copy()), Frame(b.copy())
    m = det.get_brief_matches(f1, f2)
    assert isinstance(m, Matches)
    n = len(pairs)
    assert int((m.frame2.features.state >= 1).sum()) == n
    assert np.array_equal(m.frame1.features.keypoints[:n], ka[pairs[:, 0]])
    assert np.array_equal(m.frame2.features.keypoints[:n], kb[pairs[:, 1]])
    assert np.array_equal(m.frame1.features.descriptors[:n, :, 0], da[pairs[:, 0]])
    assert np.array_equal(m.frame2.features.descriptors[:n, :, 0], db[pairs[:, 1]])
    assert m.frame2.features.descriptors.dtype == np.uint8 and m.frame2.features.descriptors.shape == (len(kb), 32, 1)
    # a current frame that already has features is not detected again
    f3 = Frame(b.copy())
    m2 = det.get_brief_matches(m.frame1, f3)
    assert np.array_equal(np.sort(m2.frame1.features.keypoints[:, :, 0], axis=0), np.sort(ka[:, :, 0], axis=0))


def test_tracker_dispatches_to_brief(ctx, frames):
    from vo.features import BRIEFDetector, Tracker
    from vo.primitives import Frame, Matches
    a, b = frames
    t = Tracker(Frame(a.copy()), mode="brief")
    assert isinstance(t._tracker, BRIEFDetector)
    m = t.trackFeatures(Frame(a.copy()), Frame(b.copy()))
    assert isinstance(m, Matches)
    want = BRIEFDetector(context=ctx).get_brief_matches(Frame(a.copy()), Frame(b.copy()))
    assert np.array_equal(m.frame2.features.keypoints, want.frame2.features.keypoints)
    assert np.array_equal(m.frame2.features.state, want.frame2.features.state)
    assert int((m.frame2.features.state >= 1).sum()) > 30


def test_class_driver_on_the_reference_kitti_frames_brief(tmp_path):
    """The reference's call order with tracker_mode="brief": rotation < 1 degree, direction cosine > 0.99 on every frame."""
    from vo import driver
    from vo.primitives import Sequence
    make_kitti_dir(str(tmp_path), frames=range(6))
    seq = Sequence("kitti", path=str(tmp_path))
    out = driver.run(seq, tracker_mode="brief")
    check(out, seq, "run[brief]")
