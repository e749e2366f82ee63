"""-m gpu: every SIFT keypoint with the final order made on the device (vo_sift_all_batch_dev) and the SIFT tracker mode
that keeps every keypoint of each frame (sift_cap = -1), as the reference's cv2.SIFT_create() (nfeatures = 0) does.

Image q of a batch must equal vo_sift(cap <= 0) on that image alone -- the device's described rows ordered on the host --
bit for bit: small frames, a flat frame, a repeated frame, padded strides, and 1376x1241 frames whose counts exceed one
4096-row sort tile.  An image with more keypoints than `rows` is reported (d_over = 2) and left unwritten.  The device
loop with sift_cap = -1 must equal the oracle loop that keeps every keypoint; a frame that does not fit the feature
capacity fails its step with VO_ECAPACITY."""
import numpy as np
import pytest

from pipeline_oracle import OracleLoop, initial_sift_features
from test_gpu_pipeline import check_step, run_all
from test_gpu_sift_batch import frames

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-7777.5)
SENT_B = np.uint8(0xA5)
SENT_I = np.int32(-99)
VO_ECAPACITY = -4


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)          # (a context of its own: the batch buffers go when the module is done)
    yield c
    c.close()


class _AllBatch:
    """Device buffers of a padded batch for vo_sift_all_batch_dev: images at img_stride bytes, outputs at kp_stride /
    desc_stride rows, every byte the library must not write holding a sentinel."""

    def __init__(self, ctx, imgs, rows, pad_img=0, pad_kp=0, pad_desc=0):
        self.ctx, self.rows = ctx, rows
        self.S = len(imgs)
        self.H, self.W = imgs[0].shape
        self.img_stride = self.H * self.W + pad_img
        self.kp_stride, self.desc_stride = rows + pad_kp, rows + pad_desc
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
        a = dict(d_imgs=self.d_imgs, img_stride=self.img_stride, S=self.S, H=self.H, W=self.W, rows=self.rows,
                 d_kp=self.d_kp, kp_stride=self.kp_stride, d_desc=self.d_desc if desc else None,
                 d_desc_u8=self.d_u8 if u8 else None, desc_stride=self.desc_stride, d_n=self.d_n,
                 d_over=self.d_over if over else None)
        a.update(kw)
        self.ctx.sift_all_batch_dev(**a)
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


def _check(b, want, desc=True, u8=True, over=True):
    """Image q of the batch equals want[q] = Context.sift(image, cap=None); nothing past its count is written."""
    kp, df, db, n, ov = b.read()
    if over:
        assert np.array_equal(ov, np.zeros(b.S, np.int32)), ov
    else:
        assert np.all(ov == SENT_I), "d_over = NULL but written"
    for q, (kw, dw) in enumerate(want):
        k = int(n[q])
        assert k == len(kw), "image %d: %d keypoints, vo_sift(cap <= 0) %d" % (q, k, len(kw))
        assert np.array_equal(kp[q, :k].view(np.uint32), kw.view(np.uint32)), "image %d keypoints differ" % q
        assert np.all(kp[q, k:] == SENT_F), "image %d: keypoint rows past the count / padding written" % q
        if desc:
            assert np.array_equal(df[q, :k].view(np.uint32), dw.view(np.uint32)), "image %d descriptors differ" % q
            assert np.all(df[q, k:] == SENT_F), "image %d: descriptor rows past the count / padding written" % q
        else:
            assert np.all(df[q] == SENT_F), "d_desc = NULL but written"
        if u8:
            assert np.array_equal(db[q, :k], dw.astype(np.uint8)), "image %d byte descriptors differ" % q
            assert np.all(db[q, k:] == SENT_B), "image %d: byte descriptor rows past the count / padding written" % q
        else:
            assert np.all(db[q] == SENT_B), "d_desc_u8 = NULL but written"
    return n


def test_small_frames_flat_and_repeated_image(ctx):
    H, W = 240, 320
    a, c = frames(2, H, W, seed=5)
    imgs = [a, np.full((H, W), 128, np.uint8), c, a.copy()]
    want = [ctx.sift(im, cap=None) for im in imgs]
    rows = max(len(k) for k, _ in want) + 3
    b = _AllBatch(ctx, imgs, rows)
    try:
        b.run()
        n = _check(b, want)
        assert n[1] == 0, "the flat image has no keypoints"
        assert n[0] > 20 and n[2] > 20 and n[0] == n[3]
    finally:
        b.free()
    for im, w in zip(imgs, want):                        # S = 1
        b = _AllBatch(ctx, [im], rows)
        try:
            b.run()
            _check(b, [w])
        finally:
            b.free()


def test_padded_strides_and_either_descriptor_output(ctx):
    H, W = 480, 640
    imgs = frames(3, H, W, seed=3)
    want = [ctx.sift(im, cap=None) for im in imgs]
    rows = max(len(k) for k, _ in want) + 10
    b = _AllBatch(ctx, imgs, rows, pad_img=1000, pad_kp=7, pad_desc=5)
    try:
        for desc, u8, over in ((True, True, True), (True, False, True), (False, True, True), (True, True, False)):
            b.reset()
            b.run(desc=desc, u8=u8, over=over)
            _check(b, want, desc=desc, u8=u8, over=over)
    finally:
        b.free()


def test_configuration_size_beyond_one_sort_tile(ctx):
    """Four 1376x1241 frames of the synthetic stream: ~9k keypoints each, more than one 4096-row tile -- the merge passes
    decide the order."""
    from vo import synthetic
    s = synthetic.Stream(4, 1241, 1376)
    imgs = [s.image(i) for i in range(4)]
    want = [ctx.sift(im, cap=None) for im in imgs]
    assert all(len(k) > 4096 for k, _ in want), [len(k) for k, _ in want]
    b = _AllBatch(ctx, imgs, 16384, pad_img=64, pad_kp=3, pad_desc=9)
    try:
        b.run()
        n = _check(b, want)
        assert all(int(v) > 4096 for v in n)
    finally:
        b.free()
    b = _AllBatch(ctx, imgs[2:3], ctx._lib.vo_sift_capacity(1241, 1376))       # rows = the list capacity, S = 1
    try:
        b.run(desc=False)
        _check(b, want[2:3], desc=False)
    finally:
        b.free()


def test_rows_below_an_images_count(ctx):
    """The image with more keypoints than `rows`: d_over = 2, d_n = 0, nothing written; the others as usual."""
    H, W = 480, 640
    imgs = frames(3, H, W, seed=13)
    want = [ctx.sift(im, cap=None) for im in imgs]
    counts = [len(k) for k, _ in want]
    big = int(np.argmax(counts))
    rows = sorted(counts)[-2]                            # (the largest count exceeds it, the others fit exactly or below)
    assert counts[big] > rows
    b = _AllBatch(ctx, imgs, rows, pad_kp=2, pad_desc=2)
    try:
        b.run()
        kp, df, db, n, ov = b.read()
        assert ov[big] == 2 and n[big] == 0
        assert np.all(kp[big] == SENT_F) and np.all(df[big] == SENT_F) and np.all(db[big] == SENT_B)
        for q in range(3):
            if q == big:
                continue
            k = int(n[q])
            assert ov[q] == 0 and k == counts[q]
            assert np.array_equal(kp[q, :k].view(np.uint32), want[q][0].view(np.uint32))
            assert np.array_equal(df[q, :k].view(np.uint32), want[q][1].view(np.uint32))
            assert np.all(kp[q, k:] == SENT_F) and np.all(df[q, k:] == SENT_F) and np.all(db[q, k:] == SENT_B)
    finally:
        b.free()


def test_refusals_leave_the_context_usable(ctx):
    from vo._native import VoError
    H, W = 240, 320
    imgs = frames(2, H, W, seed=7)
    want = [ctx.sift(im, cap=None) for im in imgs]
    rows = max(len(k) for k, _ in want) + 1
    cap = ctx._lib.vo_sift_capacity(H, W)
    b = _AllBatch(ctx, imgs, rows)
    try:
        bad = [dict(S=0), dict(rows=0), dict(rows=cap + 1, kp_stride=cap + 1, desc_stride=cap + 1),
               dict(img_stride=H * W - 1), dict(kp_stride=rows - 1), dict(desc_stride=rows - 1), dict(d_n=None),
               dict(d_kp=None), dict(d_imgs=None), dict(d_desc=None, d_desc_u8=None), dict(H=15)]
        for kw in bad:
            with pytest.raises(VoError):
                b.run(**kw)
            b.reset()
            b.run()
            _check(b, want)
    finally:
        b.free()


# ---- the SIFT tracker mode with every keypoint (sift_cap = -1) ----

def _sift_all_pipe(ctx, stream, F, N, cap):
    from vo import _native
    return _native.Pipeline(ctx, stream.H, stream.W, F, stream.K, n_keypoints=N, feature_cap=cap, hyp=256,
                            p3p_threshold=1.0, max_iterations=1000, refine_iters=20, tracker="sift", sift_cap=-1)


def _stream(F, H, W):
    from vo import synthetic
    return synthetic.Stream(F, H, W)


@pytest.mark.parametrize("H,W,F,N,lookahead", [(480, 640, 5, 8192, False), (480, 640, 5, 8192, True),
                                               (1241, 1376, 4, 16384, False)])
def test_every_keypoint_loop_matches_oracle_loop(ctx, H, W, F, N, lookahead):
    """Tracker(mode="sift") with the reference's own settings: every keypoint of each frame (sift_cap = -1, the feature
    capacity N above every frame's count) against the oracle loop that keeps up to N (so keeps them all)."""
    stream = _stream(F, H, W)
    feats, T = initial_sift_features(stream, 0, N)
    pipe = _sift_all_pipe(ctx, stream, F, N, N)
    try:
        for i in range(F):
            pipe.set_frame(i, stream.image(i))
        pipe.set_state(0, feats, T, T)
        orc = OracleLoop(stream, N, 15, 2, refine_iters=20, tracker="sift")
        orc.set_state(0, feats, T, T)
        pairs = [(k, k + 1) for k in range(F - 1)]
        if lookahead:
            refs, news = [], []
            for _, b in pairs:
                refs.append(orc.step(b))
                news.append(orc.n_new)
            rs = run_all(pipe, pairs, True)
            for r, ref, n_new in zip(rs, refs, news):
                assert r.fault == 0 and r.n_features_in == n_new
                assert (r.n_tracked, r.n_triangulated, r.n_inliers, r.draws_consumed, r.ransac_iterations, r.n_candidates,
                        r.n_landmarks) == (ref["n_tracked"], ref["n_tri"], ref["n_inliers"], ref["draws"], ref["iters"],
                                           ref["n_cand"], ref["n_landmarks"])
            check_step(rs[-1], refs[-1], pipe, orc.rs.rng, land_tol=1e-4)
        else:
            for a, b in pairs:
                ref = orc.step(b)
                r = pipe.step(a, b)
                assert orc.n_new < N, "the oracle must keep every keypoint"
                assert r.n_features_in == orc.n_new and r.n_triangulated >= 8
                if H > 1000:
                    assert orc.n_new > 4096, "configuration-size frames take more than one sort tile"
                check_step(r, ref, pipe, orc.rs.rng, land_tol=1e-4)
    finally:
        pipe.close()


@pytest.mark.parametrize("lookahead", [False, True])
def test_frame_beyond_the_feature_capacity_is_a_capacity_error(ctx, lookahead):
    """feature_cap below a frame's keypoint count: collect raises VO_ECAPACITY naming the count and the capacity --
    no record with a truncated list -- and the pipeline closes cleanly."""
    from vo._native import VoError
    H, W, F, N, cap = 480, 640, 3, 400, 800
    stream = _stream(F, H, W)
    n1 = len(ctx.sift(stream.image(1), cap=None)[0])
    assert n1 > cap, "frame 1 must have more keypoints than the capacity"
    feats, T = initial_sift_features(stream, 0, N)
    pipe = _sift_all_pipe(ctx, stream, F, N, cap)
    try:
        for i in range(F):
            pipe.set_frame(i, stream.image(i))
        pipe.set_state(0, feats, T, T)
        with pytest.raises(VoError) as e:
            if lookahead:
                pipe.submit(0, 1)
                pipe.submit(1, 2)
                pipe.collect()
            else:
                pipe.step(0, 1)
        assert e.value.code == VO_ECAPACITY
        assert ("%d SIFT keypoints" % n1) in str(e.value) and ("capacity %d" % cap) in str(e.value), str(e.value)
    finally:
        pipe.close()


def test_sift_cap_below_minus_one_is_refused(ctx):
    from vo import _native
    from vo._native import VoError
    stream = _stream(3, 240, 320)
    with pytest.raises(VoError):
        _native.Pipeline(ctx, 240, 320, 3, stream.K, n_keypoints=300, tracker="sift", sift_cap=-2)
