"""-m gpu: the FAST-9 + BRIEF-256 front end through the drop-in classes.  FASTBRIEFDetector.get_brief_matches against the
definition composed on the CPU (tests/fast_reference.py, tests/brief_reference.py), the Tracker's dispatch, and the class
driver on the reference's six KITTI frames under the bars the other modes meet in tests/test_gpu_kitti.py.

The driver's defaults come from the CPU figures of tests/test_fast_host.py (the 1000 strongest FAST-9 survivors at
threshold 20, BRIEF-256 not oriented, ratio 0.8, max_distance 64: 570 pairs on frames 0 and 2, 96.67 % within 2 px of the
ground-truth epipolar geometry, against 569 pairs and 96.84 % for the patch route that passes the same bars).  The rest
of the class driver (8-point RANSAC, P3P, refinement, DLT) runs on the device only, so the chain cannot be composed on the
CPU: the bars are first met here."""
import numpy as np
import pytest

import brief_reference as bref
import fast_reference as ref
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


def test_get_brief_matches_equals_the_definition(ctx, frames):
    from vo.features import FASTBRIEFDetector
    from vo.primitives import Frame, Matches
    a, b = frames
    det = FASTBRIEFDetector(num_keypoints=300, match_ratio=0.85, max_distance=70, context=ctx)
    ka, kb = ref.keypoints(a, 20, True, 300)[0], ref.keypoints(b, 20, True, 300)[0]
    da, db = bref.describe(a, ka, False)[0], bref.describe(b, kb, False)[0]
    pairs = bref.match(da, db, 0.85, 70)
    print("definition: %d and %d keypoints, %d pairs" % (len(ka), len(kb), len(pairs)))
    assert len(ka) == len(kb) == 300 and len(pairs) > 30
    fa = det.extractKeypoints(Frame(a.copy()))
    assert fa.features.keypoints.shape == (300, 2, 1) and fa.features.keypoints.dtype == np.float64
    assert np.array_equal(fa.features.keypoints[:, :, 0], ka)
    m = det.get_brief_matches(Frame(a.copy()), Frame(b.copy()))
    assert isinstance(m, Matches)
    n = len(pairs)
    assert int((m.frame2.features.state >= 1).sum()) == n
    assert np.array_equal(m.frame1.features.keypoints[:n, :, 0], ka[pairs[:, 0]])
    assert np.array_equal(m.frame2.features.keypoints[:n, :, 0], kb[pairs[:, 1]])
    assert np.array_equal(m.frame1.features.descriptors[:n, :, 0], da[pairs[:, 0]])
    assert np.array_equal(m.frame2.features.descriptors[:n, :, 0], db[pairs[:, 1]])
    assert m.frame2.features.descriptors.dtype == np.uint8 and m.frame2.features.descriptors.shape == (300, 32, 1)


def test_tracker_dispatches_to_fast(ctx, frames):
    from vo.features import FASTBRIEFDetector, Tracker
    from vo.primitives import Frame, Matches
    a, b = frames
    t = Tracker(Frame(a.copy()), mode="fast")
    assert isinstance(t._tracker, FASTBRIEFDetector)
    m = t.trackFeatures(Frame(a.copy()), Frame(b.copy()))
    assert isinstance(m, Matches)
    want = FASTBRIEFDetector(context=ctx).get_brief_matches(Frame(a.copy()), Frame(b.copy()))
    assert np.array_equal(m.frame2.features.keypoints, want.frame2.features.keypoints)
    assert np.array_equal(m.frame2.features.state, want.frame2.features.state)
    assert int((m.frame2.features.state >= 1).sum()) > 30


def test_class_driver_on_the_reference_kitti_frames_fast(tmp_path):
    """The reference's call order with tracker_mode="fast": rotation < 1 degree, direction cosine > 0.99 on every frame."""
    from vo import driver
    from vo.primitives import Sequence
    make_kitti_dir(str(tmp_path), frames=range(6))
    seq = Sequence("kitti", path=str(tmp_path))
    out = driver.run(seq, tracker_mode="fast")
    check(out, seq, "run[fast]")
