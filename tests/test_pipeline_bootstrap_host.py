"""Host tests (-m "not gpu") of the pipeline's two-view bootstrap: the CPU oracle (tests/pipeline_bootstrap_oracle.py) on
synthetic streams, the binding's structures, and the drivers' bootstrap= argument."""
import ctypes as C

import numpy as np
import pytest

import pipeline_bootstrap_oracle as pbo

H, W, CORNERS = 480, 640, 500


@pytest.mark.parametrize("seed", [2023, 2030, 2037])
def test_oracle_bootstrap_recovers_the_streams_relative_pose(seed):
    """Frames 0 and 2, 500 corners, 17x17 / max level 2, 1 px: rotation within 1 degree and translation-direction cosine
    >= 0.99 of the stream's analytic relative pose (the bars of tests/test_gpu_kitti.py), at least 8 landmarks, and the
    end state of the bootstrap's mask plumbing."""
    from vo import synthetic
    stream = synthetic.Stream(4, H, W, seed=seed)
    o = pbo.bootstrap(stream.image(0), stream.image(2), stream.K, max_corners=CORNERS, win=17, max_level=2, threshold_px=1.0)
    ang, cos = pbo.pose_errors(o["M"], stream.T_world_cam(0), stream.T_world_cam(2))
    f = o["features"]
    n_land = int(np.sum(np.asarray(f.state) == 2))
    print("seed %d: %d corners, %d tracked, %d RANSAC inliers, %d landmarks, %.3f deg, cos %.6f" % (
        seed, o["n_corners"], o["n_tracked"], int(o["ransac_inliers"].sum()), n_land, ang, cos))
    assert ang < 1.0 and cos >= 0.99
    assert n_land >= 8
    assert f.length == o["n_tracked"] and o["num_features"] == o["n_corners"]
    assert abs(np.linalg.norm(o["M"][:, 3]) - 1.0) < 1e-12
    pbo.check_invariants(f, o["curr_pose"])
    # the landmarks are the winner's triangulation of the masked correspondences, in the world frame (= camera a's)
    st = np.asarray(f.state)
    assert np.array_equal(st == 2, o["mask"])
    assert np.array_equal(np.asarray(f.landmarks)[st == 2], o["X"][o["mask"]])
    assert np.array_equal(o["prev_pose"], np.eye(4))


def test_binding_structures_and_default_generator():
    """vo_bootstrap_params / vo_bootstrap_result as ctypes lays them out (natural alignment, the C compiler's), and the
    generator the bootstrap's RANSAC starts from equals np.random.default_rng(2023)."""
    from vo import _native
    assert C.sizeof(_native.BootstrapParams) == 72
    assert _native.BootstrapParams.threshold_px.offset == 40 and _native.BootstrapParams.max_iterations.offset == 64
    assert C.sizeof(_native.BootstrapResult) == 32 + 96 + 16
    assert _native.BootstrapResult.M.offset == 32
    lib = _native.load()
    got = _native.Pcg64()
    lib.vo_bootstrap_default_rng(C.byref(got))
    ref = _native.Pcg64.from_generator(np.random.default_rng(2023))
    for name, _ in _native.Pcg64._fields_:
        assert getattr(got, name) == getattr(ref, name), name
    assert hasattr(_native.Pipeline, "bootstrap")


def test_drivers_refuse_an_unknown_bootstrap_route():
    from vo import driver
    with pytest.raises(ValueError):
        driver.run_on_device(None, bootstrap="gpu")
    with pytest.raises(ValueError):
        driver.run_batch_on_device([None], bootstrap="gpu")
    kw = driver._bootstrap_kwargs(2000, 15, 2, 21, 3, 1.0)
    assert kw == dict(max_corners=2000, klt_win=21, klt_max_level=3, threshold_px=1.0)
    assert driver._bootstrap_kwargs(500, 17, 2, None, None, 0.25) == dict(max_corners=500, klt_win=17, klt_max_level=2,
                                                                         threshold_px=0.25)
