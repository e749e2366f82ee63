"""CPU oracle: Harris corners with sub-pixel refinement (the second branch of KLTTracker.find_corners).
TEST INFRASTRUCTURE -- never imported by the product.

Reference call site: src/vo/features/klt.py:99-112
    dst = cv2.cornerHarris(img, 2, 3, 0.04)
    dst = cv2.dilate(dst, None)
    ret, dst = cv2.threshold(dst, 0.01 * dst.max(), 255, 0)
    ret, labels, stats, centroids = cv2.connectedComponentsWithStats(np.uint8(dst))
    points = cv2.cornerSubPix(img, np.float32(centroids), (5, 5), (-1, -1),
                              (EPS | MAX_ITER, 100, 0.001))
PARITY UNPINNED against OpenCV (opencv-python==4.8.1.78 is absent; the reference has no test for it).  Restated:
  response   3x3 Sobel as integers (reflect-101), block x block box sums Sxx, Sxy, Syy as exact integers (anchor block/2,
             reflect-101), a = (float)Sxx * s2 (s2 = (float)(scale^2), scale = 1 / (4 * block * 255)), likewise b, c;
             R = (float)(A*C - B*B - k*(A+C)*(A+C)) in double, left to right
  dilate     3x3 maximum of the in-image neighbourhood
  threshold  foreground iff dilated > (float)(rel * (double)max(dilated))
  labels     8-connectivity, background 0; components numbered in the order of their first 2x2 block (rows 2i..2i+1 x
             columns 2j..2j+1, row-major block order), as OpenCV's block-based labelling leaves them
  centroids  exact integer sums of x and y over the area, in double; row 0 is the background (NaN when it is empty)
  subpix     cornerSubPix on np.float32(centroids), every row: Gaussian window weights, getRectSubPix samples (OpenCV's
             8u->32f recurrence inside the image, clamped bilinear elsewhere), double sums, 2x2 solve per iteration
Three places where this may depart from OpenCV: the box sums are exact integers (OpenCV sums float32 products), the
Harris formula is evaluated in double (as OpenCV's vectorised calcHarris does), and the label order is the block order.
"""
import numpy as np

DBL_EPS = np.finfo(np.float64).eps


def capacity(H, W):
    """Rows of the result at most: one per 2x2 block plus the background."""
    return ((H + 1) // 2) * ((W + 1) // 2) + 1


def _sobel(img):
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    H, W = img.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) - s(-1, -1)) + 2 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    gy = (s(1, -1) - s(-1, -1)) + 2 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return gx, gy


def _box(v, block):
    H, W = v.shape
    r0 = block // 2
    r1 = block - 1 - r0
    p = np.pad(v, ((r0, r1), (r0, r1)), mode="reflect")
    out = np.zeros_like(v)
    for j in range(block):
        for i in range(block):
            out += p[j:j + H, i:i + W]
    return out


def harris_response(img, block=2, ksize=3, k=0.04):
    """cornerHarris(img, block, 3, k) as restated: (H, W) float32."""
    if ksize != 3:
        raise ValueError("only ksize 3 is restated")
    gx, gy = _sobel(np.asarray(img, np.uint8))
    sxx, sxy, syy = _box(gx * gx, block), _box(gx * gy, block), _box(gy * gy, block)
    scale = 1.0 / (4.0 * block * 255.0)
    s2 = np.float32(scale * scale)
    a = sxx.astype(np.float32) * s2
    b = sxy.astype(np.float32) * s2
    c = syy.astype(np.float32) * s2
    A, B, C = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    return (A * C - B * B - k * (A + C) * (A + C)).astype(np.float32)


def foreground(resp, rel=0.01):
    """dilate (3x3, in-image part) then threshold against rel * max: (H, W) bool."""
    p = np.pad(resp, 1, mode="constant", constant_values=-np.inf)
    H, W = resp.shape
    d = p[1:1 + H, 1:1 + W].copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            np.maximum(d, p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], out=d)
    t = np.float32(rel * float(d.max()))
    return d > t


def label_blocks(fg):
    """8-connected components numbered by their first 2x2 block: (labels (H, W) int32, rows = components + 1)."""
    from scipy import ndimage
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    if n == 0:
        return np.zeros((H, W), np.int32), 1
    ys, xs = np.nonzero(fg)
    key = (ys // 2) * ((W + 1) // 2) + xs // 2
    first = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, lab[ys, xs], key)
    order = np.argsort(first[1:], kind="stable")            # scipy's label l -> position in block order
    new = np.zeros(n + 1, np.int32)
    new[order + 1] = np.arange(1, n + 1, dtype=np.int32)
    return new[lab].astype(np.int32), n + 1


def centroids(labels, rows):
    """(rows, 2) float64 (x, y): exact integer sums over the area; the background row is NaN when it is empty."""
    H, W = labels.shape
    l = labels.ravel()
    ys, xs = np.divmod(np.arange(H * W, dtype=np.int64), W)
    area = np.bincount(l, minlength=rows).astype(np.int64)
    sx = np.bincount(l, weights=xs, minlength=rows)          # integers below 2^53: exact in double
    sy = np.bincount(l, weights=ys, minlength=rows)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([sx / area, sy / area], axis=1)


def subpix_mask(win_w, win_h):
    """cornerSubPix's window weights: (2 win_h + 1, 2 win_w + 1) float32, mask[i][j] = (float)(vy_i * ex_j)."""
    y = ((np.arange(2 * win_h + 1) - win_h).astype(np.float32) / np.float32(win_h)).astype(np.float32)
    x = ((np.arange(2 * win_w + 1) - win_w).astype(np.float32) / np.float32(win_w)).astype(np.float32)
    vy = np.exp(-(y * y).astype(np.float64)).astype(np.float32)
    ex = np.exp(-(x * x).astype(np.float64)).astype(np.float32)
    return (vy[:, None] * ex[None, :]).astype(np.float32)


def rect_subpix(img, cx, cy, bw, bh):
    """getRectSubPix(img (uint8), (bw, bh), (cx, cy), CV_32F) for m centres at once: (m, bh, bw) float32."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    f32 = np.float32
    cx = np.asarray(cx, f32) - f32((bw - 1) * 0.5)
    cy = np.asarray(cy, f32) - f32((bh - 1) * 0.5)
    ipx, ipy = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    a = (cx - ipx.astype(f32)).astype(f32)
    b = (cy - ipy.astype(f32)).astype(f32)
    m = cx.shape[0]
    out = np.empty((m, bh, bw), f32)
    I = img.astype(f32)
    jj = np.arange(bw)[None, None, :]
    ii = np.arange(bh)[None, :, None]
    inner = (ipx >= 0) & (ipx + bw < W) & (ipy >= 0) & (ipy + bh < H)
    if inner.any():
        k = np.nonzero(inner)[0]
        ac = np.maximum(a[k], f32(1e-4))
        b1, b2 = (f32(1) - b[k]).astype(f32), b[k]
        a12, a22 = (ac * b1).astype(f32), (ac * b2).astype(f32)
        s = (1.0 - ac.astype(np.float64)) / ac.astype(np.float64)
        r0 = (ipy[k][:, None, None] + ii)
        c0 = (ipx[k][:, None, None] + jj)
        t = (a12[:, None, None] * I[r0, c0 + 1] + a22[:, None, None] * I[r0 + 1, c0 + 1]).astype(f32)
        first = ((f32(1) - ac)[:, None] * (b1[:, None] * I[r0[:, :, 0], c0[:, :, 0]]
                                          + b2[:, None] * I[r0[:, :, 0] + 1, c0[:, :, 0]])).astype(f32)
        prev = np.empty_like(t)
        prev[:, :, 0] = first
        prev[:, :, 1:] = (t[:, :, :-1].astype(np.float64) * s[:, None, None]).astype(f32)
        out[k] = (prev + t).astype(f32)
    if (~inner).any():
        k = np.nonzero(~inner)[0]
        ak, bk = a[k][:, None, None], b[k][:, None, None]
        a11 = ((f32(1) - ak) * (f32(1) - bk)).astype(f32)
        a12 = (ak * (f32(1) - bk)).astype(f32)
        a21 = ((f32(1) - ak) * bk).astype(f32)
        a22 = (ak * bk).astype(f32)
        x0 = np.clip(ipx[k][:, None, None] + jj, 0, W - 1)
        x1 = np.clip(ipx[k][:, None, None] + jj + 1, 0, W - 1)
        y0 = np.clip(ipy[k][:, None, None] + ii, 0, H - 1)
        y1 = np.clip(ipy[k][:, None, None] + ii + 1, 0, H - 1)
        v = I[y0, x0] * a11
        v = (v + I[y0, x1] * a12).astype(f32)
        v = (v + I[y1, x0] * a21).astype(f32)
        out[k] = (v + I[y1, x1] * a22).astype(f32)
    return out


def corner_subpix(img, pts, win=(5, 5), max_iter=100, eps=0.001, want_raw=False):
    """cornerSubPix(img, pts, win, (-1, -1), criteria) as restated, every point in lock step: (m, 2) float32.
    max_iter: the criteria's count (clamped to 1..100); eps: its epsilon (compared squared, as OpenCV does).
    want_raw: also return where each point ended before the revert-to-start rule."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    ww, wh = int(win[0]), int(win[1])
    if W < 2 * ww + 5 or H < 2 * wh + 5:
        raise ValueError("image smaller than the window allows")
    max_iter = min(max(int(max_iter), 1), 100)
    eps2 = float(eps) * float(eps)
    mask = subpix_mask(ww, wh).astype(np.float64)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    cT = pts.copy()
    cI = pts.copy()
    active = np.isfinite(cI).all(axis=1)
    py = (np.arange(2 * wh + 1) - wh).astype(np.float64)[:, None]
    px = (np.arange(2 * ww + 1) - ww).astype(np.float64)[None, :]
    it = 0
    while active.any():
        k = np.nonzero(active)[0]
        buf = rect_subpix(img, cI[k, 0], cI[k, 1], 2 * ww + 3, 2 * wh + 3)
        tgx = (buf[:, 1:-1, 2:] - buf[:, 1:-1, :-2]).astype(np.float64)
        tgy = (buf[:, 2:, 1:-1] - buf[:, :-2, 1:-1]).astype(np.float64)
        gxx, gxy, gyy = tgx * tgx * mask, tgx * tgy * mask, tgy * tgy * mask
        a, b, c = gxx.sum(axis=(1, 2)), gxy.sum(axis=(1, 2)), gyy.sum(axis=(1, 2))
        bb1 = (gxx * px + gxy * py).sum(axis=(1, 2))
        bb2 = (gxy * px + gyy * py).sum(axis=(1, 2))
        det = a * c - b * b
        go = ~(np.abs(det) <= DBL_EPS * DBL_EPS)
        active[k[~go]] = False
        k, a, b, c, bb1, bb2, det = k[go], a[go], b[go], c[go], bb1[go], bb2[go], det[go]
        scale = 1.0 / det
        x, y = cI[k, 0], cI[k, 1]
        nx = (x.astype(np.float64) + c * scale * bb1 - b * scale * bb2).astype(np.float32)
        ny = (y.astype(np.float64) - b * scale * bb1 + a * scale * bb2).astype(np.float32)
        dx, dy = (nx - x).astype(np.float32), (ny - y).astype(np.float32)
        err = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32).astype(np.float64)
        cI[k, 0], cI[k, 1] = nx, ny
        out = (nx < 0) | (nx >= W) | (ny < 0) | (ny >= H)
        it += 1
        cont = ~out & (it < max_iter) & (err > eps2)
        active[k[~cont]] = False
    far = (np.abs(cI[:, 0] - cT[:, 0]) > np.float32(ww)) | (np.abs(cI[:, 1] - cT[:, 1]) > np.float32(wh))
    raw = cI.copy()
    cI[far] = cT[far]
    return (cI, raw) if want_raw else cI


def harris_subpix(img, block=2, ksize=3, k=0.04, rel=0.01, win=(5, 5), max_iter=100, eps=0.001):
    """The whole branch: dict of the stages (response, fg, labels, rows, centroids), the refined points `xy` and where
    they ended before the revert-to-start rule (`raw`)."""
    img = np.asarray(img, np.uint8)
    resp = harris_response(img, block, ksize, k)
    fg = foreground(resp, rel)
    labels, rows = label_blocks(fg)
    cen = centroids(labels, rows)
    xy, raw = corner_subpix(img, cen.astype(np.float32), win, max_iter, eps, want_raw=True)
    return dict(response=resp, fg=fg, labels=labels, rows=rows, centroids=cen, xy=xy, raw=raw)
