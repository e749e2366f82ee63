"""Frame ingest without a GPU: the NumPy oracle (tests/frame_ingest_oracle.py) against the cases whose result is known in
closed form, and Camera.distort_points (plain NumPy) against the oracle."""
import numpy as np
import pytest

import frame_ingest_oracle as fio

KITTI_K = np.array([[7.188560000000e+02, 0.0, 6.071928000000e+02], [0.0, 7.188560000000e+02, 1.852157000000e+02],
                    [0.0, 0.0, 1.0]])


def camera_matrix(H, W):
    return np.array([[0.9 * W, 0.0, W / 2 - 0.37], [0.0, 0.9 * W, H / 2 + 0.21], [0.0, 0.0, 1.0]])


def test_oracle_grey_is_the_package_formula():
    from vo.features.klt import _gray
    rng = np.random.default_rng(1)
    for shape in ((1, 1), (37, 53), (120, 160)):
        img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        assert np.array_equal(fio.gray_from_bgr(img), _gray(img))
    for lo in (0, 255):
        for ch in range(4):                      # every channel at one extreme, the others at the other; and all equal
            img = np.full((5, 7, 3), lo, np.uint8)
            if ch < 3:
                img[..., ch] = 255 - lo
            assert np.array_equal(fio.gray_from_bgr(img), _gray(img))
    assert fio.gray_from_bgr(np.full((2, 2, 3), 255, np.uint8)).min() == 255       # (the weights sum to 2^14)
    assert fio.gray_from_bgr(np.zeros((2, 2, 3), np.uint8)).max() == 0


@pytest.mark.parametrize("H,W,K", [(61, 83, None), (240, 320, None), (1241, 1376, None), (376, 1241, KITTI_K)])
def test_zero_coefficients_return_the_input(H, W, K):
    K = camera_matrix(H, W) if K is None else K
    img = np.random.default_rng(H).integers(0, 256, (H, W), dtype=np.uint8)
    for dist in (None, np.zeros(4), np.zeros(5)):
        assert np.array_equal(fio.undistort_image(img, K, dist), img)
    assert fio.taps_outside(H, W, K, None) > 0.0        # (the last row and column: their right / lower taps have weight 0)


@pytest.mark.parametrize("H,W", [(61, 83), (240, 320)])
def test_half_pixel_shift_in_closed_form(H, W):
    """K_raw = K with cx + 3.5: every source position is u + 3.5 exactly, the weights are 512 / 512 / 0 / 0."""
    K = camera_matrix(H, W)
    Kr = K.copy()
    Kr[0, 2] += 3.5
    img = np.random.default_rng(W).integers(0, 256, (H, W), dtype=np.uint8)
    out = fio.undistort_image(img, K, None, Kr)
    assert np.array_equal(out, shifted_expectation(img))


def shifted_expectation(img):
    H, W = img.shape
    a = img.astype(np.int64)
    exp = np.zeros((H, W), np.int64)
    exp[:, :W - 4] = (a[:, 3:W - 1] + a[:, 4:] + 1) >> 1
    exp[:, W - 4] = (a[:, W - 1] + 1) >> 1              # (column W - 4 reads W - 1 and the zero border)
    return exp.astype(np.uint8)


def test_shift_expectation_is_the_issue_statement():
    """out[:, u] = (img[:, u + 3] + img[:, u + 4] + 1) >> 1 for u < W - 4, zeros from column W - 3 on."""
    img = np.random.default_rng(3).integers(0, 256, (9, 20), dtype=np.uint8)
    exp = shifted_expectation(img)
    for u in range(20 - 4):
        assert np.array_equal(exp[:, u], ((img[:, u + 3].astype(int) + img[:, u + 4] + 1) >> 1).astype(np.uint8))
    assert not exp[:, 20 - 3:].any()


def test_distort_points_against_the_oracle_and_a_closed_form():
    from vo.sensors import Camera
    K = camera_matrix(240, 320)
    rng = np.random.default_rng(7)
    pts = np.stack((rng.uniform(0, 320, 200), rng.uniform(0, 240, 200)), axis=1)[:, :, None]
    for dist in ((-0.3, 0.1, 0.0, 0.0, 0.0), (0.2, 0.0, 0.01, -0.005, 0.05), (0.1, -0.02, 0.003, 0.004)):
        got = Camera(K, np.array(dist)).distort_points(pts)
        assert got.shape == (200, 2, 1)
        assert np.max(np.abs(got - fio.distort_points(pts, K, dist))) <= 1e-12
    # k1 alone: the point at normalised (0.5, 0) moves to 0.5 * (1 + 0.25 * k1)
    k1 = -0.2
    p = np.array([[[K[0, 2] + 0.5 * K[0, 0]], [K[1, 2]]]])
    got = Camera(K, np.array([k1, 0, 0, 0])).distort_points(p)
    assert abs(got[0, 0, 0] - (K[0, 2] + K[0, 0] * 0.5 * (1 + 0.25 * k1))) <= 1e-12 and abs(got[0, 1, 0] - K[1, 2]) <= 1e-12
    # no coefficients: the points themselves
    assert Camera(K).distort_points(pts) is pts
    assert Camera(K).undistort(pts) is pts                   # (a pinhole camera returns the image, no device involved)


def test_more_than_five_coefficients_are_refused():
    from vo.sensors import Camera
    K = camera_matrix(240, 320)
    pts = np.zeros((1, 2, 1))
    with pytest.raises(ValueError, match="k1, k2, p1, p2, k3"):
        Camera(K, np.array([0.1, 0, 0, 0, 0, 0.2])).distort_points(pts)
    with pytest.raises(ValueError, match="k1, k2, p1, p2, k3"):
        Camera(K, np.array([0.1, 0, 0, 0, 0, 0.2])).undistort(np.zeros((4, 4), np.uint8))
    from vo import _native
    with pytest.raises(ValueError, match="k1, k2, p1, p2, k3"):
        _native.distortion_coefficients(np.zeros(8))
    assert np.array_equal(_native.distortion_coefficients((1.0, 2.0, 3.0, 4.0)), [1.0, 2.0, 3.0, 4.0, 0.0])


def test_border_coverage_of_the_gpu_cases():
    """The coefficient sets of tests/test_gpu_frame_ingest.py do what that file says: the barrel set keeps every tap
    inside, the mixed set sends 11-13 % of the pixels over the border."""
    for H, W in ((61, 83), (240, 320)):
        K = camera_matrix(H, W)
        assert fio.taps_outside(H, W, K, (-0.3, 0.1, 0, 0, 0)) == 0.0
        assert 0.11 <= fio.taps_outside(H, W, K, (0.2, 0, 0.01, -0.005, 0.05)) <= 0.13


def test_distorted_view_round_trip():
    """The test input builder: undistorting the distorted view of a smooth scene gives the scene back (to resampling
    error) away from the border."""
    H, W = 120, 160
    K = camera_matrix(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    scene = (127 + 60 * np.sin(xx / 9.0) + 50 * np.cos(yy / 7.0)).astype(np.uint8)
    dist = (-0.05, 0.01, 0.001, -0.001, 0.0)
    back = fio.undistort_image(fio.distorted_view(scene, K, dist), K, dist)
    assert np.max(np.abs(back[8:-8, 8:-8].astype(int) - scene[8:-8, 8:-8])) <= 3
