"""NumPy oracle of the frame ingest (csrc/ingest.hip; include/vo_hip.h, "frame ingest"): the grey conversion of a B, G, R
image and the lens undistortion, as the header defines them -- integers for the pixels, float64 in a fixed operation order
for the map (NumPy rounds every elementwise operation on its own: no fused multiply-add), so the device must give the same
bytes.  The reference has nothing to compare with (src/vo/sensors/camera.py:38-54 are stubs) and OpenCV is not a
dependency: parity with cv2.undistort is not claimed (unpinned).

TEST INFRASTRUCTURE ONLY: nothing here touches the GPU."""
import numpy as np

LIMIT = float(2 ** 24)


def gray_from_bgr(bgr):
    """(H, W, 3) uint8, channels B, G, R -> (H, W) uint8."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def coefficients(dist):
    """(k1, k2, p1, p2, k3) as floats; None: zeros; four coefficients: k3 = 0."""
    d = np.zeros(5) if dist is None else np.asarray(dist, np.float64).reshape(-1)
    if d.size not in (4, 5):
        raise ValueError("the model is (k1, k2, p1, p2[, k3]), got %d coefficients" % d.size)
    return [float(v) for v in np.concatenate((d, np.zeros(5 - d.size)))]


def forward_model(x, y, dist):
    """Normalised ideal coordinates -> normalised distorted coordinates (float64 arrays, the header's operation order)."""
    k1, k2, p1, p2, k3 = coefficients(dist)
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, (2 * x) * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2 * x2)
    yd = (y * kr + p1 * (r2 + 2 * y2)) + p2 * _2xy
    return xd, yd


def source_positions(H, W, K, dist, K_raw=None):
    """For every output pixel the position in the distorted image, in 1/32 pixels: (ix, iy) int64 arrays (H, W)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Kr = K if K_raw is None else np.asarray(K_raw, np.float64).reshape(3, 3)
    u, v = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    x = np.broadcast_to((u - K[0, 2]) / K[0, 0], (H, W))
    y = np.broadcast_to((v - K[1, 2]) / K[1, 1], (H, W))
    xd, yd = forward_model(x, y, dist)
    us, vs = Kr[0, 0] * xd + Kr[0, 2], Kr[1, 1] * yd + Kr[1, 2]

    def fixed(a):          # (fmax / fmin: a NaN becomes a bound, as in C; rint: ties to even)
        return np.rint(np.fmin(np.fmax(a * 32, -LIMIT), LIMIT)).astype(np.int64)

    return fixed(us), fixed(vs)


def undistort_image(img, K, dist, K_raw=None):
    """(H, W) uint8 of the distorted camera (K_raw, dist) -> (H, W) uint8 of the pinhole camera K."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    ix, iy = source_positions(H, W, K, dist, K_raw)
    x0, fx, y0, fy = ix >> 5, ix & 31, iy >> 5, iy & 31
    src = img.astype(np.int64)

    def tap(xx, yy):       # (a tap outside the image counts as 0)
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)

    acc = ((32 - fx) * (32 - fy) * tap(x0, y0) + fx * (32 - fy) * tap(x0 + 1, y0)
           + (32 - fx) * fy * tap(x0, y0 + 1) + fx * fy * tap(x0 + 1, y0 + 1) + 512)
    return (acc >> 10).astype(np.uint8)


def taps_outside(H, W, K, dist, K_raw=None):
    """The share of output pixels with at least one of the four taps outside the image."""
    ix, iy = source_positions(H, W, K, dist, K_raw)
    x0, y0 = ix >> 5, iy >> 5
    return float(np.mean((x0 < 0) | (x0 + 1 >= W) | (y0 < 0) | (y0 + 1 >= H)))


def ingest(img, K, dist, K_raw=None):
    """What a frame slot receives: undistort(gray(img)); a grey image skips the conversion, no coefficients (None) and no
    K_raw skip the undistortion."""
    img = np.asarray(img)
    g = gray_from_bgr(img) if img.ndim == 3 else img
    if K_raw is None and (dist is None or not np.any(np.asarray(dist, np.float64) != 0.0)):
        return g
    return undistort_image(g, K, dist, K_raw)


def distort_points(points, K, dist):
    """(N, 2, 1) ideal pixels -> (N, 2, 1) pixels of the distorted image, the same intrinsics on both sides."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    p = np.asarray(points, np.float64)
    xd, yd = forward_model((p[:, 0, 0] - K[0, 2]) / K[0, 0], (p[:, 1, 0] - K[1, 2]) / K[1, 1], dist)
    return np.stack((K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]), axis=1)[:, :, None]


def distorted_view(scene, K, dist, iterations=8):
    """A test input, not part of the definition: roughly what the distorted camera (K, dist) sees where the pinhole camera
    K sees `scene` ((H, W) uint8), so that undistorting it gives the scene back up to resampling blur.  The model is
    inverted by fixed-point iteration and the scene sampled bilinearly (float, edge-clamped)."""
    k1, k2, p1, p2, k3 = coefficients(dist)
    K = np.asarray(K, np.float64).reshape(3, 3)
    H, W = scene.shape
    xd = np.broadcast_to((np.arange(W)[None, :] - K[0, 2]) / K[0, 0], (H, W))
    yd = np.broadcast_to((np.arange(H)[:, None] - K[1, 2]) / K[1, 1], (H, W))
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / kr, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / kr
    u = np.clip(K[0, 0] * x + K[0, 2], 0, W - 1)
    v = np.clip(K[1, 1] * y + K[1, 2], 0, H - 1)
    u0, v0 = np.minimum(u.astype(np.int64), W - 2), np.minimum(v.astype(np.int64), H - 2)
    a, b = u - u0, v - v0
    s = scene.astype(np.float64)
    out = ((1 - a) * (1 - b) * s[v0, u0] + a * (1 - b) * s[v0, u0 + 1] + (1 - a) * b * s[v0 + 1, u0] + a * b * s[v0 + 1, u0 + 1])
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def bgr_of(scene):
    """A three-channel test frame whose channels differ (B, G, R = the scene scaled by 1.0 / 0.9 / 0.8): a swapped channel
    order changes its grey value."""
    s = scene.astype(np.float64)
    return np.stack([np.rint(s * f).astype(np.uint8) for f in (1.0, 0.9, 0.8)], axis=2)
