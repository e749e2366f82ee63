"""-m gpu: frame ingest on the device (csrc/ingest.hip) -- three-channel frames and lens undistortion between the caller's
buffer and a frame slot.  The arithmetic is defined in integers and ordered float64 (include/vo_hip.h, "frame ingest"), so
every comparison with tests/frame_ingest_oracle.py is exact: a slot holds the oracle's undistort(gray(img)), and a
pipeline fed raw frames computes what a pipeline fed the oracle-ingested frames computes."""
import numpy as np
import pytest

import frame_ingest_oracle as fio
from pipeline_oracle import initial_features

pytestmark = pytest.mark.gpu

H, W, N, HYP, F = 240, 320, 300, 256, 5
LANE_DIST = (None, (-0.05, 0.01, 0.001, -0.001, 0.0))          # lane 0: a pinhole camera, lane 1: a lens
BARREL, MIXED = (-0.3, 0.1, 0.0, 0.0, 0.0), (0.2, 0.0, 0.01, -0.005, 0.05)


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def camera_matrix(h, w):
    return np.array([[0.9 * w, 0.0, w / 2 - 0.37], [0.0, 0.9 * w, h / 2 + 0.21], [0.0, 0.0, 1.0]])


# ---- 1. grey ----

@pytest.mark.parametrize("h,w", [(1, 1), (37, 53), (240, 320), (1241, 1376)])
def test_grey_equals_the_oracle(ctx, h, w):
    """Random bytes and planes of 0 and 255 (every channel alone at an extreme); 37 x 53 and 1 x 1 leave a tail of fewer
    than four pixels."""
    rng = np.random.default_rng(h * 7 + w)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]
    for lo in (0, 255):
        for ch in range(3):
            im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            im[..., ch] = lo
            imgs.append(im)
        imgs.append(np.full((h, w, 3), lo, np.uint8))
    if h > 1000:                                           # (the large shape: random bytes and the two full planes)
        imgs = [imgs[0], imgs[4], imgs[8]]
    for k, im in enumerate(imgs):
        got = ctx.gray_from_bgr(im)
        assert got.shape == (h, w) and got.dtype == np.uint8
        assert np.array_equal(got, fio.gray_from_bgr(im)), ("image", k)


# ---- 2. undistort ----

def shifted_expectation(img):
    """K_raw = K with cx + 3.5: out[:, u] = (img[:, u + 3] + img[:, u + 4] + 1) >> 1, the zero border from column W on."""
    a = np.concatenate((img.astype(np.int64), np.zeros((img.shape[0], 5), np.int64)), axis=1)
    w = img.shape[1]
    return ((a[:, 3:w + 3] + a[:, 4:w + 4] + 1) >> 1).astype(np.uint8)


@pytest.mark.parametrize("h,w", [(61, 83), (240, 320)])
def test_undistort_equals_the_oracle(ctx, h, w):
    K = camera_matrix(h, w)
    img = np.random.default_rng(w).integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(ctx.undistort_image(img, K, np.zeros(5)), img), "zero coefficients"
    assert np.array_equal(ctx.undistort_image(img, K, np.zeros(4)), img), "four zero coefficients"
    assert fio.taps_outside(h, w, K, BARREL) == 0.0 and 0.11 <= fio.taps_outside(h, w, K, MIXED) <= 0.13
    for dist in (BARREL, MIXED, MIXED[:4]):
        got = ctx.undistort_image(img, K, dist)
        assert np.array_equal(got, fio.undistort_image(img, K, dist)), dist
    Kr = K.copy()
    Kr[0, 2] += 3.5
    got = ctx.undistort_image(img, K, None, K_raw=Kr)
    assert np.array_equal(got, shifted_expectation(img))
    assert not got[:, w - 3:].any()
    assert np.array_equal(got, fio.undistort_image(img, K, None, Kr))
    Kr[1, 1] *= 1.07                                       # (another camera behind the lens: K_raw and coefficients together)
    Kr[1, 2] -= 2.25
    assert np.array_equal(ctx.undistort_image(img, K, MIXED, K_raw=Kr), fio.undistort_image(img, K, MIXED, Kr))


def test_camera_undistort_runs_on_the_device(ctx):
    from vo.sensors import Camera
    K = camera_matrix(61, 83)
    img = np.random.default_rng(5).integers(0, 256, (61, 83, 3), dtype=np.uint8)
    cam = Camera(K, np.array(MIXED))
    assert np.array_equal(cam.undistort(img[..., 0], context=ctx), fio.undistort_image(img[..., 0], K, MIXED))
    got = cam.undistort(img, context=ctx)
    assert got.shape == img.shape
    for c in range(3):
        assert np.array_equal(got[..., c], fio.undistort_image(img[..., c], K, MIXED))


# ---- 3 / 4. the pipeline's slots and its loop ----

class Lanes:
    """Two recordings of F frames: what each lane's camera delivers (raw: B, G, R, lane 1 through its lens) and what the
    oracle makes of it (grey: what the slot must hold).  Computed once for the module."""

    def __init__(self):
        from vo import synthetic
        self.streams = [synthetic.Stream(F, H, W, seed=2023 + 5 * q, start=q) for q in range(2)]
        self.K = self.streams[0].K
        self.raw, self.grey, self._starts = [], [], None
        for q, s in enumerate(self.streams):
            scenes = [s.image(i) for i in range(F)]
            views = scenes if LANE_DIST[q] is None else [fio.distorted_view(im, self.K, LANE_DIST[q]) for im in scenes]
            self.raw.append([fio.bgr_of(v) for v in views])
            self.grey.append([fio.ingest(r, self.K, LANE_DIST[q]) for r in self.raw[q]])
        for a in self.raw + self.grey:
            for im in a:
                im.flags.writeable = False

    def starts(self):
        """(features, pose) of frame 0 per lane, found on the ingested frames."""
        if self._starts is None:
            self._starts = [initial_features(self.ingested_stream(q), 0, N) for q in range(2)]
        return self._starts

    def ingested_stream(self, q):
        """Lane q as pipeline_oracle.initial_features wants it: the ingested frames, the scene's depth and poses."""
        lanes, base = self, self.streams[q]

        class View:
            K, n = base.K, F
            image = staticmethod(lambda i: lanes.grey[q][i])
            depth, T_world_cam, order = base.depth, base.T_world_cam, base.order

        return View()


@pytest.fixture(scope="module")
def lanes():
    return Lanes()


def new_pipe(ctx, K, **kw):
    from vo import _native
    return _native.Pipeline(ctx, H, W, F, K, n_keypoints=N, klt_win=15, klt_max_level=2, hyp=HYP, p3p_threshold=1.0,
                            max_iterations=1000, refine_iters=20, sequences=2, **kw)


def fill(ctx, pipe, frames, pinned):
    """frames[q][i] -> slot i of lane q, every lane of a slot by the same route.  Returns what must stay alive."""
    keep = []
    for i in range(F):
        for q in range(2):
            im = frames[q][i]
            if pinned:
                buf = ctx.pinned_empty(im.shape)
                buf[...] = im
                keep.append(buf)
                im = buf
            pipe.set_frame(i, im, seq=q, pinned=pinned)
    return keep


@pytest.mark.parametrize("pinned", [False, True], ids=["plain", "pinned"])
def test_slots_hold_the_ingested_frames(ctx, lanes, pinned):
    """B, G, R frames whose channels differ, lane 1 behind a lens: every slot holds undistort(gray(img)) of the oracle.
    Then the grey entry points on the same lanes: lane 1's grey frames are undistorted too, lane 0's are copied."""
    pipe = new_pipe(ctx, lanes.K)
    pipe.set_distortion(1, LANE_DIST[1])
    keep = fill(ctx, pipe, lanes.raw, pinned)
    for i in range(F):
        for q in range(2):
            assert np.array_equal(pipe.get_frame(i, seq=q), lanes.grey[q][i]), ("slot", i, "lane", q)
    assert not np.array_equal(lanes.grey[0][0], fio.gray_from_bgr(lanes.raw[0][0][..., ::-1]))     # (the channel order shows)
    grey_in = [[fio.gray_from_bgr(im)[::-1].copy() for im in lanes.raw[q]] for q in range(2)]     # (upside down: new bytes)
    keep += fill(ctx, pipe, grey_in, pinned)
    for i in range(F):
        for q in range(2):
            assert np.array_equal(pipe.get_frame(i, seq=q), fio.ingest(grey_in[q][i], lanes.K, LANE_DIST[q])), (i, q)
    # the lens goes: frames uploaded afterwards are copied, slots already filled keep their contents
    pipe.set_distortion(1, None)
    before = pipe.get_frame(1, seq=1)
    pipe.set_frame(0, grey_in[1][0], seq=1, pinned=False)
    assert np.array_equal(pipe.get_frame(0, seq=1), grey_in[1][0]) and np.array_equal(pipe.get_frame(1, seq=1), before)
    pipe.close()
    del keep


RECORD_FIELDS = ("R", "t", "n_tracked", "n_inliers", "best_index", "hyp_valid", "ransac_iterations", "draws_consumed",
                 "refine_iterations", "R_refined", "t_refined", "refine_cost", "n_features_in", "redetected",
                 "n_triangulated", "n_candidates", "n_dropped", "n_landmarks", "fault", "recovered", "detector_ran",
                 "reserved", "raw_pos", "T_wc")
STATE_KEYS = ("n", "keypoints", "state", "candidate_mask", "landmarks", "tracks", "poses", "curr_pose", "prev_pose",
              "n_iterations", "outlier_ratio", "num_features")


def differing(a, b, skip=()):
    """The names of the record fields (all but ts, seq_head, seq_tail, and `skip`) in which two StepResults differ."""
    from vo import _native
    assert set(RECORD_FIELDS) | {"ts", "seq_head", "seq_tail"} == {name for name, _ in _native.StepResult._fields_}
    return [(name, np.array(getattr(a, name)).tolist(), np.array(getattr(b, name)).tolist()) for name in RECORD_FIELDS
            if name not in skip and not np.array_equal(np.array(getattr(a, name)), np.array(getattr(b, name)), equal_nan=True)]


# detector_ran says whether the detector EXECUTED on the step's `prev` frame.  With a re-detect margin (the default) that
# is a prediction made on the detection stream from the track count of whichever step has finished by then: under
# look-ahead two runs of one pipeline on the same frames may differ in it near the limit, and nothing else depends on it
# (tests/test_gpu_lanes.py and tests/test_gpu_pipeline_bootstrap.py leave it out of their look-ahead
# comparisons for that reason).  With detect_margin < 0 the detector executes on every frame and the field is determined.
SCHEDULING = ("detector_ran",)


def rng_of(pipe, q):
    g = np.random.default_rng(0)
    pipe.rng_state_into(g, seq=q)
    return g.bit_generator.state


def run_loop(pipe, starts, pairs):
    """Four steps in the drivers' call order: two in flight, the next frame's pyramid hinted."""
    for q in range(2):
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    out, pending = [], 0
    for k, (a, b) in enumerate(pairs):
        if pending == 2:
            out.append(pipe.collect_all())
            pending -= 1
        pipe.submit(a, b)
        pending += 1
        if k + 1 < len(pairs):
            pipe.prepare(pairs[k + 1][1])
    while pending:
        out.append(pipe.collect_all())
        pending -= 1
    return out


@pytest.mark.parametrize("every_frame", [True, False], ids=["detector-every-frame", "detector-gated"])
def test_loop_on_raw_frames_equals_loop_on_ingested_frames(ctx, lanes, every_frame):
    """The pipeline fed B, G, R frames (lane 1 with coefficients) against a pipeline fed the oracle's grey frames and no
    coefficients, four steps with look-ahead: no step faults; the carried arrays and the generators are equal; and
      detector-every-frame (detect_margin < 0: the detector reads every ingested frame): EVERY record field but ts,
        seq_head, seq_tail is equal;
      detector-gated (the default margin; lane 1 comes within a few features of the limit at step 3): every one of those
        fields but detector_ran, which two runs of ONE pipeline on the same bytes need not agree in (SCHEDULING above)."""
    kw = dict(detect_margin=-1.0) if every_frame else {}
    skip = () if every_frame else SCHEDULING
    starts = lanes.starts()
    order = lanes.streams[0].order(4)
    pairs = list(zip(order[:-1], order[1:]))
    runs = []
    for frames, dist in ((lanes.raw, LANE_DIST[1]), (lanes.grey, None)):
        pipe = new_pipe(ctx, lanes.K, **kw)
        pipe.set_distortion(1, dist)
        keep = fill(ctx, pipe, frames, pinned=True)
        recs = run_loop(pipe, starts, pairs)
        runs.append((recs, [pipe.get_state(seq=q) for q in range(2)], [rng_of(pipe, q) for q in range(2)]))
        pipe.close()
        del keep
    (got, got_state, got_rng), (ref, ref_state, ref_rng) = runs
    assert len(got) == len(ref) == 4
    for k in range(4):
        for q in range(2):
            print("step", k, "lane", q, "fault", got[k][q].fault, ref[k][q].fault, "tracked", got[k][q].n_tracked,
                  "inliers", got[k][q].n_inliers)
            assert got[k][q].fault == 0 and ref[k][q].fault == 0, (k, q)
            assert not differing(got[k][q], ref[k][q], skip), (k, q, differing(got[k][q], ref[k][q], skip)[:3])
            if every_frame:
                assert got[k][q].detector_ran == 1
    for q in range(2):
        for key in STATE_KEYS:
            assert np.array_equal(got_state[q][key], ref_state[q][key], equal_nan=True), (q, key)
        assert got_rng[q] == ref_rng[q]
        assert got[-1][q].n_tracked > 0 and got[-1][q].n_landmarks >= 8


# ---- 5. the drivers ----

DRIVER_SHAPE = (480, 640)
_frames = {}


class Recording:
    """A Sequence whose camera has a lens and delivers B, G, R (ingested = False), or the same recording after the oracle's
    ingest, grey and from a pinhole camera (ingested = True)."""

    def __init__(self, seed, n_frames, dist, ingested):
        from vo.primitives import Sequence
        from vo.sensors import Camera
        self._base = Sequence("synthetic", n_frames=n_frames, height=DRIVER_SHAPE[0], width=DRIVER_SHAPE[1], seed=seed)
        self._dist, self._ingested, self._seed = dist, ingested, seed
        self._K = np.asarray(self._base.get_camera().intrinsic_matrix, np.float64)
        self._cam = Camera(self._K, None if ingested or dist is None else np.array(dist))

    def _deliver(self, frame):
        key = (self._seed, frame.frame_id)
        if key not in _frames:
            view = frame.image if self._dist is None else fio.distorted_view(frame.image, self._K, self._dist)
            raw = fio.bgr_of(view)
            _frames[key] = (raw, fio.ingest(raw, self._K, self._dist))
        frame.image = _frames[key][1 if self._ingested else 0]
        return frame

    def get_camera(self):
        return self._cam

    def get_frame(self, idx):
        return self._deliver(self._base.get_frame(idx))

    def __iter__(self):
        return self

    def __next__(self):
        return self._deliver(next(self._base))

    def __len__(self):
        return len(self._base)

    def __getattr__(self, name):                 # (dataset, H, W, increment, ground_truth_pose)
        return getattr(self._base, name)


def same_runs(got, ref, what):
    """Every record field but ts, seq_head, seq_tail and detector_ran (the drivers run with look-ahead and the default
    re-detect margin: SCHEDULING above), the trajectory and the final features: equal exactly."""
    assert set(got) == set(ref), what
    assert len(got["results"]) == len(ref["results"]) > 0, what
    for k, (a, b) in enumerate(zip(got["results"], ref["results"])):
        assert not differing(a, b, SCHEDULING), (what, "step", k, differing(a, b, SCHEDULING)[:3])
    assert np.array_equal(got["n_landmarks"], ref["n_landmarks"]), what
    assert np.array_equal(got["trajectory"], ref["trajectory"]), what
    assert got["features"].length == ref["features"].length > 0, what
    assert np.array_equal(got["features"].keypoints, ref["features"].keypoints), what
    assert np.array_equal(got["features"].state, ref["features"].state), what


DRIVER_KW = dict(n_keypoints=500, hyp=1024, bootstrap_threshold=1.0, bootstrap="device")


def test_run_on_device_takes_a_lens_camera(ctx):
    """run_on_device(bootstrap="device") on B, G, R frames of a camera with coefficients against the same driver on the
    pre-ingested grey recording of a pinhole camera: every record and the trajectory are equal exactly."""
    from vo import driver
    dist = LANE_DIST[1]
    got = driver.run_on_device(Recording(2023, 9, dist, False), context=ctx, **DRIVER_KW)
    ref = driver.run_on_device(Recording(2023, 9, dist, True), context=ctx, **DRIVER_KW)
    same_runs(got, ref, "run_on_device")
    assert all(r.fault == 0 for r in got["results"])
    with pytest.raises(ValueError, match="bootstrap='device'"):       # (the host bootstrap does not undistort)
        driver.run_on_device(Recording(2023, 9, dist, False), context=ctx, n_keypoints=500, hyp=1024)


def test_run_batch_on_device_takes_a_lens_per_lane(ctx):
    """Three recordings through two lanes: two cameras with different coefficients, then a pinhole camera on a lane that
    held a lens before (its coefficients must go with the recording).  Per recording what the driver gives for the
    pre-ingested grey recordings."""
    from vo import driver
    specs = [(2023, 8, LANE_DIST[1]), (2034, 6, (0.04, -0.01, -0.001, 0.0015, 0.002)), (2045, 6, None)]
    got = driver.run_batch_on_device([Recording(s, n, d, False) for s, n, d in specs], lanes=2, context=ctx, **DRIVER_KW)
    ref = driver.run_batch_on_device([Recording(s, n, d, True) for s, n, d in specs], lanes=2, context=ctx, **DRIVER_KW)
    assert len(got) == len(ref) == 3
    for i, (s, n, d) in enumerate(specs):
        assert len(got[i]["results"]) == n - 3
        same_runs(got[i], ref[i], ("recording", i))


# ---- 6. refusals ----

def test_refusals_leave_the_pipeline_running(ctx, lanes):
    from vo import _native
    K = lanes.K
    with pytest.raises(_native.VoError, match="non-finite"):
        ctx.undistort_image(lanes.grey[0][0], K, (np.nan, 0, 0, 0, 0))
    Kbad = K.copy()
    Kbad[0, 2] = np.inf
    with pytest.raises(_native.VoError, match="non-finite"):
        ctx.undistort_image(lanes.grey[0][0], K, BARREL, K_raw=Kbad)
    pipe = new_pipe(ctx, K)
    pipe.set_distortion(1, LANE_DIST[1])
    fill(ctx, pipe, lanes.raw, pinned=False)
    starts = lanes.starts()
    for q in range(2):
        pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q)
    for bad in ((0.1, np.nan, 0, 0, 0), (np.inf, 0, 0, 0, 0)):
        with pytest.raises(_native.VoError, match="non-finite"):
            pipe.set_distortion(1, bad)
    with pytest.raises(_native.VoError, match="non-finite"):
        pipe.set_distortion(1, BARREL, K_raw=Kbad)
    for seq in (-1, 2):
        with pytest.raises(_native.VoError):
            pipe.set_distortion(seq, BARREL)
        with pytest.raises(_native.VoError):
            pipe.get_frame(0, seq=seq)
        with pytest.raises(_native.VoError):
            pipe.set_frame(2, lanes.raw[0][2], seq=seq, pinned=False)
    with pytest.raises(_native.VoError):
        pipe.get_frame(F, seq=0)
    with pytest.raises(ValueError, match="k1, k2, p1, p2, k3"):
        pipe.set_distortion(1, np.zeros(6))
    pipe.submit(0, 1)
    with pytest.raises(_native.VoError, match="not collected"):
        pipe.set_distortion(1, BARREL)
    with pytest.raises(_native.VoError, match="not collected"):
        pipe.get_frame(2, seq=0)
    with pytest.raises(_native.VoError, match="step in flight"):
        pipe.set_frame(1, lanes.raw[0][1], seq=0, pinned=False)
    first = pipe.collect_all()
    with pytest.raises(_native.VoError, match="next step starts from"):
        pipe.set_frame(1, lanes.raw[0][1], seq=0, pinned=False)          # (a B, G, R upload into the slot step 2 starts from)
    # none of it changed the lanes: lane 1 still has its lens, and the pipeline goes on
    assert np.array_equal(pipe.get_frame(2, seq=1), lanes.grey[1][2])
    pipe.set_frame(3, lanes.raw[1][3], seq=1, pinned=False)
    assert np.array_equal(pipe.get_frame(3, seq=1), lanes.grey[1][3])
    second = pipe.step(1, 2)
    assert all(r.fault == 0 for r in first) and second.fault == 0 and second.n_tracked > 0
    pipe.close()
