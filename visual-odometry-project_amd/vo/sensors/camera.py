"""Pinhole camera (reference: src/vo/sensors/camera.py)."""
import numpy as np

from vo.helpers import to_cartesian_coordinates, to_homogeneous_coordinates


class Camera:
    """Intrinsics K plus an optional world->camera pose (R, t)."""

    def __init__(self, intrinsic_matrix: np.ndarray, distortion_coeffs: np.ndarray = None,
                 R: np.ndarray = None, t: np.ndarray = None):
        self.intrinsic_matrix = intrinsic_matrix
        self.distortion_coeffs = distortion_coeffs
        self.R = R
        self.t = t

    def _require_pose(self):
        assert self.R is not None and self.t is not None, "Camera pose not set"

    @property
    def projection_matrix(self) -> np.ndarray:
        """K [R | t] (camera.py:30-36)."""
        self._require_pose()
        return self.intrinsic_matrix @ np.hstack((self.R, self.t))

    @property
    def c_T_w(self) -> np.ndarray:
        """4x4 world->camera transform (camera.py:94-100)."""
        self._require_pose()
        return np.vstack((np.hstack((self.R, self.t)), [0, 0, 0, 1]))

    def _distortion(self):
        """(k1, k2, p1, p2, k3), or None for a pinhole camera (no coefficients, or all zero)."""
        if self.distortion_coeffs is None:
            return None
        from vo._native import distortion_coefficients
        d = distortion_coefficients(self.distortion_coeffs)
        return d if np.any(d != 0.0) else None

    def distort_points(self, points: np.ndarray) -> np.ndarray:
        """(N, 2, 1) ideal pixels -> (N, 2, 1) pixels of the distorted image, by the forward model
        (k1, k2, p1, p2, k3) with the same intrinsics on both sides (camera.py:38-45 declares it and leaves it empty)."""
        d = self._distortion()
        if d is None:
            return points
        k1, k2, p1, p2, k3 = (float(v) for v in d)
        K = np.asarray(self.intrinsic_matrix, np.float64)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        pts = np.asarray(points, np.float64)
        x, y = (pts[:, 0, 0] - cx) / fx, (pts[:, 1, 0] - cy) / fy
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, (2 * x) * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)
        yd = (y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy
        return np.stack((fx * xd + cx, fy * yd + cy), axis=1)[:, :, np.newaxis]

    def undistort(self, image: np.ndarray, context=None) -> np.ndarray:
        """The image of the pinhole camera K from one of this (distorted) camera, on the device (vo_undistort_image;
        camera.py:47-54 declares it and leaves it empty): (H, W) uint8, or (H, W, C) channel by channel."""
        d = self._distortion()
        if d is None:
            return image
        from vo import _native
        ctx = context or _native.default_context()
        image = np.asarray(image)
        if image.ndim == 2:
            return ctx.undistort_image(image, self.intrinsic_matrix, d)
        return np.stack([ctx.undistort_image(image[..., c], self.intrinsic_matrix, d) for c in range(image.shape[2])], axis=2)

    def project_points_world_frame(self, points_3d: np.ndarray) -> np.ndarray:
        """(N, 3, 1) world points -> (N, 2, 1) pixels (camera.py:56-65)."""
        self._require_pose()
        return self.project_points_camera_frame(self.R[np.newaxis] @ points_3d + self.t)

    def project_points_camera_frame(self, points_3d: np.ndarray) -> np.ndarray:
        """(N, 3, 1) camera-frame points -> (N, 2, 1) pixels (camera.py:67-78)."""
        return to_cartesian_coordinates(self.intrinsic_matrix[np.newaxis] @ points_3d)

    def to_normalized_image_coordinates(self, points_2d: np.ndarray) -> np.ndarray:
        """(N, 2, 1) pixels -> (N, 3, 1) bearing vectors with unit z (camera.py:80-92)."""
        rays = np.linalg.inv(self.intrinsic_matrix) @ to_homogeneous_coordinates(points_2d)
        assert np.allclose(rays[:, -1], 1), "Normalization not successful"
        return rays
