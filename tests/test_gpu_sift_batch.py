"""-m gpu: batched SIFT (vo_sift_batch / vo_sift_batch_dev, Context.sift_batch).  S images of one size go through one set
of launches; every image's keypoints and descriptors must equal those of the one-image entry points on that image alone,
bit for bit -- whatever the batch holds (a flat image with no keypoints, an image twice), whatever the cap, at
configuration size, with padded strides, after the batch grows and shrinks on one context, and after refused calls."""
import ctypes as C

import numpy as np
import pytest

from oracle import native
from scenarios import synthetic_image
from test_oracle_geometry import shift_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)          # (a context of its own: the batch buffers go when the module is done)
    yield c
    c.close()


def frames(S, H, W, seed=0):
    """S distinct textured frames: smooth shifted scenes and block images alternately."""
    out = []
    for q in range(S):
        if q % 2 == 0:
            out.append(shift_image(H, W, 21 + seed + q, 0.7 * q, -0.4 * q)[0])
        else:
            out.append(synthetic_image(H, W, 5 + seed + q, block=14, noise=3.0))
    return [np.ascontiguousarray(a, np.uint8) for a in out]


def assert_equal_per_image(got, want, what):
    assert len(got) == len(want)
    for q, ((kg, dg), (kw, dw)) in enumerate(zip(got, want)):
        assert kg.shape == kw.shape, "%s: image %d has %d keypoints, the one-image call %d" % (what, q, len(kg), len(kw))
        assert np.array_equal(kg.view(np.uint32), kw.view(np.uint32)), "%s: image %d keypoints differ" % (what, q)
        assert np.array_equal(dg.view(np.uint32), dw.view(np.uint32)), "%s: image %d descriptors differ" % (what, q)


def test_batch_of_six_with_a_flat_and_a_repeated_image(ctx):
    H, W = 240, 320
    imgs = frames(4, H, W)
    imgs = imgs[:2] + [np.full((H, W), 128, np.uint8)] + imgs[2:] + [imgs[1].copy()]
    assert len(imgs) == 6
    for cap in (300, None):
        got = ctx.sift_batch(imgs, cap=cap)
        want = [ctx.sift(im, cap=cap) for im in imgs]
        assert_equal_per_image(got, want, "cap=%s" % cap)
        assert len(got[2][0]) == 0, "the flat image has no keypoints"
        assert all(len(got[q][0]) > 20 for q in (0, 1, 3, 4, 5))
        assert np.array_equal(got[1][0], got[5][0]) and np.array_equal(got[1][1], got[5][1])
        kr, dr = native.sift(imgs[0], cap=cap) if cap else native.sift(imgs[0])
        assert np.array_equal(got[0][0], kr) and np.array_equal(got[0][1], dr), "image 0 differs from the oracle"
    # an (S, H, W) array is the same batch
    assert_equal_per_image(ctx.sift_batch(np.stack(imgs), cap=300), ctx.sift_batch(imgs, cap=300), "array input")


def test_configuration_size(ctx):
    """Four 1376x1241 frames of the synthetic stream: candidate lists of thousands of entries, caps in FIN_MAX's range."""
    from vo import synthetic
    s = synthetic.Stream(4, 1241, 1376)
    imgs = [s.image(i) for i in range(4)]
    for cap in (2000, None):
        got = ctx.sift_batch(imgs, cap=cap)
        want = [ctx.sift(im, cap=cap) for im in imgs]
        assert_equal_per_image(got, want, "1376x1241 cap=%s" % cap)
        assert all(len(k) == 2000 for k, _ in got) if cap else all(len(k) > 5000 for k, _ in got)


def _batch_dev(ctx, d_imgs, img_stride, S, H, W, cap, d_kp, kp_stride, d_desc, d_u8, desc_stride, d_n, d_over):
    ctx._chk(ctx._lib.vo_sift_batch_dev(ctx._h, d_imgs, img_stride, S, H, W, cap, d_kp, kp_stride, d_desc, d_u8,
                                        desc_stride, d_n, d_over))


def _one_dev(ctx, img, cap):
    """vo_sift_dev on one image: (kp, desc float, desc bytes) with the count's rows."""
    H, W = img.shape
    d_img, d_kp, d_desc, d_u8, d_n = (ctx.alloc(img.nbytes), ctx.alloc(cap * 24), ctx.alloc(cap * 512), ctx.alloc(cap * 128),
                                      ctx.alloc(4))
    ctx.upload(d_img, img)
    ctx._chk(ctx._lib.vo_sift_dev(ctx._h, d_img, H, W, cap, d_kp, d_desc, d_u8, d_n))
    ctx.sync()
    n = int(ctx.download(d_n, (1,), np.int32)[0])
    out = (ctx.download(d_kp, (cap, 6), np.float32)[:n], ctx.download(d_desc, (cap, 128), np.float32)[:n],
           ctx.download(d_u8, (cap, 128), np.uint8)[:n])
    for p in (d_img, d_kp, d_desc, d_u8, d_n):
        ctx.free(p)
    return out


SENT_F = np.float32(-7777.5)
SENT_B = np.uint8(0xA5)
SENT_I = np.int32(-99)


class _DevBatch:
    """Device buffers of a padded batch: images at img_stride bytes, outputs at kp_stride / desc_stride rows, every
    byte the library must not write holding a sentinel."""

    def __init__(self, ctx, imgs, cap, pad_img=1000, pad_kp=7, pad_desc=5):
        self.ctx, self.cap = ctx, cap
        self.S = len(imgs)
        self.H, self.W = imgs[0].shape
        self.img_stride = self.H * self.W + pad_img
        self.kp_stride, self.desc_stride = cap + pad_kp, cap + pad_desc
        host = np.full((self.S, self.img_stride), 255, np.uint8)
        for q, im in enumerate(imgs):
            host[q, : self.H * self.W] = im.reshape(-1)
        self.d_imgs = ctx.to_device(host)
        self.d_kp = ctx.alloc(self.S * self.kp_stride * 24)
        self.d_desc = ctx.alloc(self.S * self.desc_stride * 512)
        self.d_u8 = ctx.alloc(self.S * self.desc_stride * 128)
        self.d_n = ctx.alloc(self.S * 4)
        self.d_over = ctx.alloc(self.S * 4)
        self.reset()

    def reset(self):
        c, S = self.ctx, self.S
        c.upload(self.d_kp, np.full((S, self.kp_stride, 6), SENT_F, np.float32))
        c.upload(self.d_desc, np.full((S, self.desc_stride, 128), SENT_F, np.float32))
        c.upload(self.d_u8, np.full((S, self.desc_stride, 128), SENT_B, np.uint8))
        c.upload(self.d_n, np.full(S, SENT_I, np.int32))
        c.upload(self.d_over, np.full(S, SENT_I, np.int32))

    def run(self, desc=True, u8=True, over=True, **kw):
        a = dict(d_imgs=self.d_imgs, img_stride=self.img_stride, S=self.S, H=self.H, W=self.W, cap=self.cap, d_kp=self.d_kp,
                 kp_stride=self.kp_stride, d_desc=self.d_desc if desc else None, d_u8=self.d_u8 if u8 else None,
                 desc_stride=self.desc_stride, d_n=self.d_n, d_over=self.d_over if over else None)
        a.update(kw)
        _batch_dev(self.ctx, **a)
        self.ctx.sync()

    def read(self):
        c, S = self.ctx, self.S
        return (c.download(self.d_kp, (S, self.kp_stride, 6), np.float32),
                c.download(self.d_desc, (S, self.desc_stride, 128), np.float32),
                c.download(self.d_u8, (S, self.desc_stride, 128), np.uint8),
                c.download(self.d_n, (S,), np.int32), c.download(self.d_over, (S,), np.int32))

    def free(self):
        for p in (self.d_imgs, self.d_kp, self.d_desc, self.d_u8, self.d_n, self.d_over):
            self.ctx.free(p)


def test_device_entry_with_padded_strides(ctx):
    H, W, cap = 240, 320, 200
    imgs = frames(3, H, W, seed=3)
    ref = [_one_dev(ctx, im, cap) for im in imgs]
    b = _DevBatch(ctx, imgs, cap)
    try:
        for desc, u8 in ((True, False), (False, True), (True, True)):
            b.reset()
            b.run(desc=desc, u8=u8)
            kp, df, db, n, over = b.read()
            assert np.array_equal(over, np.zeros(b.S, np.int32))
            for q in range(b.S):
                k = int(n[q])
                assert k == len(ref[q][0]) and k > 20
                assert np.array_equal(kp[q, :k].view(np.uint32), ref[q][0].view(np.uint32)), "image %d keypoints" % q
                assert np.all(kp[q, k:] == SENT_F), "image %d: keypoint rows past the count / padding written" % q
                if desc:
                    assert np.array_equal(df[q, :k].view(np.uint32), ref[q][1].view(np.uint32)), "image %d descriptors" % q
                    assert np.all(df[q, k:] == SENT_F), "image %d: descriptor padding written" % q
                else:
                    assert np.all(df[q] == SENT_F), "d_desc = NULL but written"
                if u8:
                    assert np.array_equal(db[q, :k], ref[q][2]), "image %d byte descriptors" % q
                    assert np.all(db[q, k:] == SENT_B), "image %d: byte descriptor padding written" % q
                else:
                    assert np.all(db[q] == SENT_B), "d_desc_u8 = NULL but written"
        # d_over may be NULL
        b.reset()
        b.run(over=False)
        kp, _, _, n, over = b.read()
        assert np.all(over == SENT_I) and [int(v) for v in n] == [len(r[0]) for r in ref]
    finally:
        b.free()


def test_sixteen_then_two_then_one_on_one_context(ctx):
    H, W, cap = 480, 640, 500
    imgs = frames(16, H, W, seed=11)
    want = [ctx.sift(im, cap=cap) for im in imgs]
    assert_equal_per_image(ctx.sift_batch(imgs, cap=cap), want, "S=16")
    assert_equal_per_image(ctx.sift_batch(imgs[5:7], cap=cap), want[5:7], "S=2 after S=16")
    k, d = ctx.sift(imgs[9], cap=cap)
    assert np.array_equal(k, want[9][0]) and np.array_equal(d, want[9][1]), "one image after the batches"


def test_refusals_leave_the_context_usable(ctx):
    from vo._native import VoError
    H, W, cap = 240, 320, 150
    imgs = frames(2, H, W, seed=7)
    ref = [_one_dev(ctx, im, cap) for im in imgs]
    b = _DevBatch(ctx, imgs, cap)
    try:
        bad = [dict(S=0), dict(cap=0), dict(cap=4001), dict(img_stride=H * W - 1), dict(kp_stride=cap - 1),
               dict(desc_stride=cap - 1), dict(d_n=None), dict(H=15), dict(d_kp=None), dict(d_imgs=None)]
        for kw in bad:
            with pytest.raises(VoError):
                b.run(**kw)
            b.reset()
            b.run()
            kp, df, db, n, over = b.read()
            assert np.array_equal(over, [0, 0])
            for q in range(2):
                k = int(n[q])
                assert k == len(ref[q][0]), kw
                assert np.array_equal(kp[q, :k], ref[q][0]) and np.array_equal(df[q, :k], ref[q][1]), kw
    finally:
        b.free()
    # the host entry refuses S < 1 and null pointers as well
    n = np.zeros(1, np.int32)
    kp, desc = np.empty((cap, 6), np.float32), np.empty((cap, 128), np.float32)
    img = imgs[0]
    for args in ((img, 0, H, W), (None, 1, H, W), (img, 1, 8, W)):
        with pytest.raises(VoError):
            p = None if args[0] is None else args[0].ctypes.data_as(C.c_void_p)
            ctx._chk(ctx._lib.vo_sift_batch(ctx._h, p, args[1], args[2], args[3], cap, kp.ctypes.data_as(C.c_void_p),
                                            desc.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p)))
    k, d = ctx.sift_batch([img], cap=cap)[0]
    assert np.array_equal(k, ref[0][0]) and np.array_equal(d, ref[0][1])
