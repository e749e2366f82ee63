"""-m gpu: vo.driver.run_on_device -- the batch driver's loop with one lane (pinned ring, uploads a step ahead, two steps
in flight) -- against a plain loop that has none of it: the same host bootstrap, then one unpinned upload and one
blocking Pipeline.step per frame.  The recording and settings are those of test_gpu_track_ids.py's driver test with 3 + 7
frames: seven steps are the fewest at which the four slots wrap and two steps are in flight at the drain."""
import numpy as np
import pytest

from test_gpu_lanes import same_records

pytestmark = pytest.mark.gpu

H, W, N, STEPS = 240, 320, 300, 7
KLT_WIN, KLT_MAX_LEVEL, HYP = 17, 2, 4000                  # (run_on_device's defaults)


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def recording():
    from vo.primitives import Sequence
    return Sequence("synthetic", n_frames=3 + STEPS, height=H, width=W)


@pytest.fixture(scope="module")
def full(ctx):
    from vo import driver
    return driver.run_on_device(recording(), n_keypoints=N, context=ctx)


def plain_loop(ctx):
    from vo import _native, driver
    seq = recording()
    state, tracker = driver._device_bootstrap(seq, N, KLT_WIN, KLT_MAX_LEVEL, None, None, 0.25)
    frame = state.curr_frame
    K = np.asarray(seq.get_camera().intrinsic_matrix, np.float64)
    pipe = _native.Pipeline(ctx, H, W, 4, K, **driver._pipeline_kwargs(state, N, KLT_WIN, KLT_MAX_LEVEL, HYP, "current"))
    pipe.set_frame(0, driver._gray(frame.image))
    pipe.set_state(0, frame.features, state.curr_pose, state.prev_pose, num_features=tracker._tracker._num_features)
    results = []
    for k, f in enumerate(seq):
        pipe.set_frame((k + 1) % 4, f.image, pinned=False)
        results.append(pipe.step(k % 4, (k + 1) % 4))
    features = pipe.get_features()
    pipe.close()
    return dict(trajectory=np.array([np.eye(4), state.get_pose()] + [r.pose_world_cam() for r in results]),
                n_landmarks=np.array([len(frame.features.triangulated_inliers_landmarks)] + [r.n_landmarks for r in results]),
                results=results, features=features)


def test_run_on_device_equals_a_plain_loop(ctx, full):
    ref = plain_loop(ctx)
    assert len(full["results"]) == len(ref["results"]) == STEPS == len(full["frame_seconds"])
    same_records(full["results"], ref["results"], "run_on_device against the plain loop")
    assert all(r.fault == 0 for r in full["results"]) and full["results"][-1].n_tracked > 0
    assert np.array_equal(full["trajectory"], ref["trajectory"])
    assert np.array_equal(full["n_landmarks"], ref["n_landmarks"])
    assert full["features"].length == ref["features"].length > 0
    assert np.array_equal(full["features"].keypoints, ref["features"].keypoints)


def test_max_frames_gives_the_first_steps_of_the_full_run(ctx, full):
    from vo import driver
    out = driver.run_on_device(recording(), n_keypoints=N, context=ctx, max_frames=5)
    assert len(out["results"]) == 5 and len(out["frame_seconds"]) == 5
    same_records(out["results"], full["results"][:5], "max_frames=5")
    assert out["trajectory"].shape == (7, 4, 4)              # (the identity, the bootstrap's pose and five steps')
    assert np.array_equal(out["trajectory"], full["trajectory"][:7])
    assert np.array_equal(out["n_landmarks"], full["n_landmarks"][:6])
