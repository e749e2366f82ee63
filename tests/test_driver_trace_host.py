"""CPU: the order of pipeline calls the device-resident drivers make (vo.driver.run_on_device, run_batch_on_device),
recorded by a stub Pipeline -- the four-slot pinned ring, the frame of step k + 2 uploaded before step k -> k + 1 is
submitted, its pyramid hinted behind that submit, a collect whenever two steps are pending, the drain at the end.  The
expected traces were recorded from the two separate loops the driver had before run_on_device became the one-lane case
of the batch driver; the one-lane trace may differ from the old run_on_device's in the three ways as_one_lane() spells
out, the batch trace in none."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

K = np.array([[8.0, 0.0, 4.0], [0.0, 8.0, 4.0], [0.0, 0.0, 1.0]])
BOOT_POSE = np.array([[1.0, 0, 0, 0.5], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0], [0, 0, 0, 1.0]])
STEP_POSE = np.array([[1.0, 0, 0, 2.0], [0, 1.0, 0, 0], [0, 0, 1.0, 3.0], [0, 0, 0, 1.0]])


class Recording:
    """A scripted recording of 8 x 8 grey frames; frame i is filled with 16 * tag + i, which is how a trace names it.
    reads: the frames next() has delivered so far.  delay: seconds next() takes to deliver one."""

    def __init__(self, n_frames, tag=0, delay=0.0):
        self.n_frames, self.tag, self.delay, self.idx, self.reads = n_frames, tag, delay, 0, []

    def get_camera(self):
        return SimpleNamespace(intrinsic_matrix=K)

    def get_frame(self, idx):
        return SimpleNamespace(image=np.full((8, 8), 16 * self.tag + idx, np.uint8), frame_id=idx)

    def __len__(self):
        return self.n_frames

    def __iter__(self):
        return self

    def __next__(self):
        if self.idx >= self.n_frames:
            raise StopIteration
        if self.delay:
            time.sleep(self.delay)
        self.reads.append(self.idx)
        self.idx += 1
        return self.get_frame(self.idx - 1)


class _Pinned(np.ndarray):
    pass


class _StubContext:
    def __init__(self):
        self.calls, self.pipelines = [], 0

    def pinned_empty(self, shape, dtype=np.uint8):
        return np.empty(shape, dtype).view(_Pinned)


class _StubPipeline:
    """Records every call with the arguments that say where a frame or a state goes; a frame is named by its fill value."""

    def __init__(self, ctx, H, W, n_frames, K, sequences=1, track_ids=False, **kw):
        assert (H, W, n_frames) == (8, 8, 4)
        ctx.pipelines += 1
        self.calls, self.sequences = ctx.calls, sequences

    def _result(self):
        return SimpleNamespace(n_landmarks=7, n_features_in=9, n_tracked=8, n_inliers=6, n_candidates=1, redetected=0,
                               pose_world_cam=lambda: STEP_POSE)

    def set_camera(self, K, seq, Kinv=None):
        self.calls.append(("set_camera", seq))

    def set_distortion(self, seq, dist, K_raw=None):
        self.calls.append(("set_distortion", seq))

    def set_frame(self, idx, img, seq=0, pinned=None):
        assert img.shape == (8, 8) and (img == img[0, 0]).all()
        if pinned is None:                                   # (Pipeline.set_frame: decided by where img lies)
            pinned = isinstance(img, _Pinned)
        assert pinned == isinstance(img, _Pinned)
        self.calls.append(("set_frame", idx, seq, "pinned" if pinned else "plain", int(img[0, 0])))

    def set_state(self, idx, features, curr_pose, prev_pose=None, num_features=None, seq=0):
        self.calls.append(("set_state", idx, seq))

    def restart(self, seq, idx, features, curr_pose, prev_pose=None, num_features=None, generator=None, image=None):
        self.calls.append(("restart", seq, idx, int(image[0, 0])))

    def set_active(self, seq, flag):
        self.calls.append(("set_active", seq, flag))

    def bootstrap(self, idx_a, idx_b, **kw):
        self.calls.append(("bootstrap", idx_a, idx_b))
        return SimpleNamespace(n_landmarks=5, status=0)

    def bootstrap_lanes(self, idx_a, idx_b, seqs, **kw):
        self.calls.append(("bootstrap_lanes", idx_a, idx_b, list(seqs)))
        return [SimpleNamespace(n_landmarks=5, status=0, seq=q) for q in seqs]

    def submit(self, prev_idx, next_idx):
        self.calls.append(("submit", prev_idx, next_idx))

    def prepare(self, idx):
        self.calls.append(("prepare", idx))

    def collect(self):
        self.calls.append(("collect",))
        return self._result()

    def collect_all(self):
        self.calls.append(("collect_all",))
        return [self._result() for _ in range(self.sequences)]

    def get_features(self, seq=0):
        self.calls.append(("get_features", seq))
        return ("features of lane", seq)

    def get_state(self, seq=0):
        self.calls.append(("get_state", seq))
        return dict(curr_pose=BOOT_POSE)

    def close(self):
        self.calls.append(("close",))


def _scripted_bootstrap(sequence, *args):
    """What vo.driver._device_bootstrap hands on: frames 0..2 taken from the recording, the state of frame 2."""
    next(sequence)
    next(sequence)
    frame = next(sequence)
    features = SimpleNamespace(length=6, triangulated_inliers_landmarks=np.zeros((5, 3, 1)))
    state = SimpleNamespace(curr_frame=SimpleNamespace(image=frame.image, features=features), curr_pose=BOOT_POSE,
                            prev_pose=np.eye(4), get_pose=lambda: BOOT_POSE, _bearing_threshold=0.0075)
    return state, SimpleNamespace(_tracker=SimpleNamespace(_num_features=6))


@pytest.fixture
def ctx(monkeypatch):
    from vo import _native, driver
    monkeypatch.setattr(_native, "Pipeline", _StubPipeline)
    monkeypatch.setattr(driver, "_device_bootstrap", _scripted_bootstrap)
    return _StubContext()


def as_one_lane(old):
    """The trace of the former run_on_device loop -> the trace of the batch driver with one lane: the lane's camera is set
    once more at the start, steps are collected with collect_all, the device route bootstraps through bootstrap_lanes."""
    new = [("set_camera", 0)]
    for call in old:
        if call == ("collect",):
            call = ("collect_all",)
        elif call[0] == "bootstrap":
            call = ("bootstrap_lanes", call[1], call[2], [0])
        new.append(call)
    return new


# run_on_device(Recording(10)) as the former loop made its calls: 7 steady-state frames (3 .. 9), so the four slots wrap
OLD_ONE_HOST = [
    ("set_frame", 0, 0, "plain", 2), ("set_state", 0, 0), ("set_frame", 1, 0, "pinned", 3),
    ("set_frame", 2, 0, "pinned", 4), ("submit", 0, 1), ("prepare", 2), ("set_frame", 3, 0, "pinned", 5),
    ("submit", 1, 2), ("prepare", 3), ("collect",), ("set_frame", 0, 0, "pinned", 6), ("submit", 2, 3),
    ("prepare", 0), ("collect",), ("set_frame", 1, 0, "pinned", 7), ("submit", 3, 0), ("prepare", 1), ("collect",),
    ("set_frame", 2, 0, "pinned", 8), ("submit", 0, 1), ("prepare", 2), ("collect",),
    ("set_frame", 3, 0, "pinned", 9), ("submit", 1, 2), ("prepare", 3), ("collect",), ("submit", 2, 3), ("collect",),
    ("collect",), ("get_features", 0), ("close",),
]
OLD_ONE_DEVICE = [
    ("set_frame", 1, 0, "plain", 0), ("set_frame", 0, 0, "plain", 2), ("bootstrap", 1, 0), ("get_state", 0),
    ("set_frame", 1, 0, "pinned", 3), ("set_frame", 2, 0, "pinned", 4), ("submit", 0, 1), ("prepare", 2),
    ("set_frame", 3, 0, "pinned", 5), ("submit", 1, 2), ("prepare", 3), ("collect",),
    ("set_frame", 0, 0, "pinned", 6), ("submit", 2, 3), ("prepare", 0), ("collect",),
    ("set_frame", 1, 0, "pinned", 7), ("submit", 3, 0), ("prepare", 1), ("collect",),
    ("set_frame", 2, 0, "pinned", 8), ("submit", 0, 1), ("prepare", 2), ("collect",),
    ("set_frame", 3, 0, "pinned", 9), ("submit", 1, 2), ("prepare", 3), ("collect",), ("submit", 2, 3), ("collect",),
    ("collect",), ("get_features", 0), ("close",),
]
# run_batch_on_device of three recordings with 3, 5 and 2 steps through 2 lanes, before the loop became a class
BATCH_HOST = [
    ("set_camera", 0), ("set_frame", 0, 0, "plain", 2), ("set_state", 0, 0), ("set_camera", 1),
    ("set_frame", 0, 1, "plain", 18), ("set_state", 0, 1), ("set_frame", 1, 0, "pinned", 3),
    ("set_frame", 1, 1, "pinned", 19), ("set_frame", 2, 0, "pinned", 4), ("set_frame", 2, 1, "pinned", 20),
    ("submit", 0, 1), ("prepare", 2), ("set_frame", 3, 0, "pinned", 5), ("set_frame", 3, 1, "pinned", 21),
    ("submit", 1, 2), ("prepare", 3), ("collect_all",), ("set_frame", 0, 1, "pinned", 22), ("submit", 2, 3),
    ("prepare", 0), ("collect_all",), ("collect_all",), ("get_features", 0), ("set_camera", 0), ("restart", 0, 3, 34),
    ("set_frame", 0, 0, "pinned", 35), ("set_frame", 1, 0, "pinned", 36), ("set_frame", 1, 1, "pinned", 23),
    ("submit", 3, 0), ("prepare", 1), ("submit", 0, 1), ("collect_all",), ("collect_all",), ("get_features", 0),
    ("get_features", 1), ("close",),
]
BATCH_DEVICE = [
    ("set_camera", 0), ("set_frame", 1, 0, "plain", 0), ("set_frame", 0, 0, "plain", 2), ("set_camera", 1),
    ("set_frame", 1, 1, "plain", 16), ("set_frame", 0, 1, "plain", 18), ("bootstrap_lanes", 1, 0, [0, 1]),
    ("get_state", 0), ("get_state", 1), ("set_frame", 1, 0, "pinned", 3), ("set_frame", 1, 1, "pinned", 19),
    ("set_frame", 2, 0, "pinned", 4), ("set_frame", 2, 1, "pinned", 20), ("submit", 0, 1), ("prepare", 2),
    ("set_frame", 3, 0, "pinned", 5), ("set_frame", 3, 1, "pinned", 21), ("submit", 1, 2), ("prepare", 3),
    ("collect_all",), ("set_frame", 0, 1, "pinned", 22), ("submit", 2, 3), ("prepare", 0), ("collect_all",),
    ("collect_all",), ("get_features", 0), ("set_camera", 0), ("set_active", 0, False),
    ("set_frame", 0, 0, "plain", 32), ("set_frame", 3, 0, "plain", 34), ("bootstrap_lanes", 0, 3, [0]),
    ("get_state", 0), ("set_frame", 0, 0, "pinned", 35), ("set_frame", 1, 0, "pinned", 36),
    ("set_frame", 1, 1, "pinned", 23), ("submit", 3, 0), ("prepare", 1), ("submit", 0, 1), ("collect_all",),
    ("collect_all",), ("get_features", 0), ("get_features", 1), ("close",),
]


def loop_of(trace):
    """The part of a one-lane trace from the first pinned upload on."""
    first = next(i for i, c in enumerate(trace) if c[0] == "set_frame" and c[3] == "pinned")
    return trace[:first], trace[first:]


def check_one_lane_protocol(trace, steps, first_frame=3):
    """The look-ahead protocol on a one-lane trace, rule by rule (the literal traces pin the same thing call by call)."""
    head, loop = loop_of(trace)
    assert not any(c[0] in ("submit", "prepare", "collect_all", "collect") for c in head)
    assert loop[0] == ("set_frame", 1, 0, "pinned", first_frame)         # the frame of step 0 -> 1, before the loop
    pos, pending, slot = 1, 0, 0
    for k in range(steps):
        if pending == 2:                                     # a collect exactly when two steps are pending
            assert loop[pos] == ("collect_all",)
            pos, pending = pos + 1, pending - 1
        ahead = k + 1 < steps
        if ahead:                                            # the frame of step k + 1 -> k + 2, before this submit
            assert loop[pos] == ("set_frame", (slot + 2) % 4, 0, "pinned", first_frame + k + 1)
            pos += 1
        assert loop[pos] == ("submit", slot, (slot + 1) % 4)
        pos += 1
        if ahead:                                            # its pyramid behind that submit, only when a frame was put
            assert loop[pos] == ("prepare", (slot + 2) % 4)
            pos += 1
        pending, slot = pending + 1, (slot + 1) % 4
    assert loop[pos:] == [("collect_all",)] * min(steps, 2) + [("get_features", 0), ("close",)]


def test_one_recording_host_route(ctx):
    from vo import driver
    rec = Recording(10)
    out = driver.run_on_device(rec, context=ctx)
    assert ctx.calls == as_one_lane(OLD_ONE_HOST)
    check_one_lane_protocol(ctx.calls, 7)
    assert loop_of(ctx.calls)[0] == [("set_camera", 0), ("set_frame", 0, 0, "plain", 2), ("set_state", 0, 0)]
    assert ctx.pipelines == 1 and rec.reads == list(range(10))
    assert sorted(out) == ["features", "frame_seconds", "n_landmarks", "results", "trajectory"]
    assert out["trajectory"].shape == (9, 4, 4) and np.array_equal(out["trajectory"][0], np.eye(4))
    assert np.array_equal(out["trajectory"][1], BOOT_POSE) and np.array_equal(out["trajectory"][-1], STEP_POSE)
    assert out["n_landmarks"].tolist() == [5] + [7] * 7 and len(out["results"]) == 7 and len(out["frame_seconds"]) == 7
    assert out["features"] == ("features of lane", 0)


def test_one_recording_device_route(ctx):
    """Frame 0 goes into slot 1 and frame 2 into slot 0, both unpinned, before the single bootstrap_lanes(1, 0, [0])."""
    from vo import driver
    out = driver.run_on_device(Recording(10), context=ctx, bootstrap="device")
    assert ctx.calls == as_one_lane(OLD_ONE_DEVICE)
    check_one_lane_protocol(ctx.calls, 7)
    assert loop_of(ctx.calls)[0] == [("set_camera", 0), ("set_frame", 1, 0, "plain", 0), ("set_frame", 0, 0, "plain", 2),
                                     ("bootstrap_lanes", 1, 0, [0]), ("get_state", 0)]
    assert sum(c[0] == "bootstrap_lanes" for c in ctx.calls) == 1
    assert np.array_equal(out["trajectory"][1], BOOT_POSE) and out["n_landmarks"].tolist() == [5] + [7] * 7


def test_max_frames_stops_the_reads(ctx):
    from vo import driver
    rec = Recording(10)
    out = driver.run_on_device(rec, context=ctx, max_frames=5)
    check_one_lane_protocol(ctx.calls, 5)
    assert sum(c[0] == "submit" for c in ctx.calls) == 5 and len(out["results"]) == 5
    assert rec.reads == list(range(8))                       # frames 8 and 9 are never read from the sequence


def test_recording_without_a_steady_state_frame(ctx):
    """Frames 0..2 only: the batch driver's rule -- the host bootstrap is all there is, no pipeline is made."""
    from vo import driver
    for route in ("host", "device"):
        out = driver.run_on_device(Recording(3), context=ctx, bootstrap=route)
        assert ctx.pipelines == 0 and ctx.calls == []
        assert out["trajectory"].shape == (2, 4, 4) and np.array_equal(out["trajectory"][1], BOOT_POSE)
        assert out["n_landmarks"].tolist() == [5] and out["features"].length == 6
        assert out["results"] == [] and len(out["frame_seconds"]) == 0


def test_frame_seconds_with_and_without_delivery(ctx):
    """A recording that takes 20 ms to deliver a frame: run_on_device's frame_seconds leave the delivery out, the batch
    driver's are the wall time of the step -- which reads the frame of the NEXT step, so every step but the last one."""
    from vo import driver
    alone = driver.run_on_device(Recording(7, delay=0.02), context=ctx)
    assert len(alone["frame_seconds"]) == 4 and (alone["frame_seconds"] >= 0.0).all()
    assert (alone["frame_seconds"] < 0.010).all(), alone["frame_seconds"]
    batch = driver.run_batch_on_device([Recording(7, delay=0.02)], lanes=1, context=ctx)[0]
    assert len(batch["frame_seconds"]) == 4
    assert (batch["frame_seconds"][:-1] >= 0.020).all(), batch["frame_seconds"]


@pytest.mark.parametrize("route,expected", [("host", BATCH_HOST), ("device", BATCH_DEVICE)])
def test_three_recordings_through_two_lanes(ctx, route, expected):
    from vo import driver
    recs = [Recording(3 + n, tag=i) for i, n in enumerate((3, 5, 2))]
    out = driver.run_batch_on_device(recs, lanes=2, context=ctx, bootstrap=route)
    assert ctx.calls == expected
    assert [len(o["results"]) for o in out] == [3, 5, 2] and ctx.pipelines == 1
    assert all(rec.reads == list(range(rec.n_frames)) for rec in recs)
