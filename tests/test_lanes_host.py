"""CPU: the host side of lanes -- vo.driver.lane_schedule (which recording holds which lane at which step) and what
run_batch_on_device refuses before it touches a GPU."""
import pytest


def check(plan, lengths):
    """Every recording with steps runs them in order, on one lane, without a gap; a lane holds one recording at a time."""
    steps = plan["steps"]
    seen = {}
    for t, row in enumerate(steps):
        assert len(row) == plan["lanes"]
        for lane, e in enumerate(row):
            if e is None:
                continue
            r, j = e
            seen.setdefault(r, []).append((t, lane, j))
    for r, n in enumerate(lengths):
        got = seen.get(r, [])
        assert len(got) == n, r
        if n:
            t0, lane, _ = got[0]
            assert [x[2] for x in got] == list(range(n)), r
            assert all(x[1] == lane for x in got) and [x[0] for x in got] == list(range(t0, t0 + n)), r
            assert (t0, lane, r) in plan["starts"]
    assert len(plan["starts"]) == sum(1 for n in lengths if n > 0)


def test_uneven_lengths_fill_freed_lanes_in_queue_order():
    from vo.driver import lane_schedule
    lengths = [9, 14, 6, 20, 11]
    plan = lane_schedule(lengths, 3)
    check(plan, lengths)
    assert plan["starts"] == [(0, 0, 0), (0, 1, 1), (0, 2, 2), (6, 2, 3), (9, 0, 4)]
    # recording 1 ends after step 13, recording 4 after step 19, recording 3 after step 25
    assert plan["idles"] == [(14, 1), (20, 0)]
    assert len(plan["steps"]) == 26
    assert plan["steps"][6] == ((0, 6), (1, 6), (3, 0))
    assert plan["steps"][25] == (None, None, (3, 19))


def test_more_lanes_than_recordings():
    from vo.driver import lane_schedule
    plan = lane_schedule([3, 5], 4)
    check(plan, [3, 5])
    assert plan["starts"] == [(0, 0, 0), (0, 1, 1)]
    assert plan["idles"] == [(0, 2), (0, 3), (3, 0)]
    assert plan["steps"][0] == ((0, 0), (1, 0), None, None)
    assert plan["steps"][4] == (None, (1, 4), None, None)


def test_empty_recordings_hold_no_lane():
    from vo.driver import lane_schedule
    lengths = [0, 4, 0, 2, 0]
    plan = lane_schedule(lengths, 1)
    check(plan, lengths)
    assert plan["starts"] == [(0, 0, 1), (4, 0, 3)]
    assert plan["idles"] == []
    assert lane_schedule([0, 0], 2) == dict(steps=[], starts=[], idles=[], lanes=2)
    assert lane_schedule([], 1)["steps"] == []


def test_bad_arguments():
    from vo.driver import lane_schedule
    with pytest.raises(ValueError):
        lane_schedule([3], 0)
    with pytest.raises(ValueError):
        lane_schedule([3, -1], 2)


def test_batch_driver_refuses_mixed_frame_sizes():
    from vo import driver
    from vo.primitives import Sequence
    seqs = [Sequence("synthetic", n_frames=8, height=240, width=320), Sequence("synthetic", n_frames=8, height=480, width=640)]
    with pytest.raises(ValueError):
        driver.run_batch_on_device(seqs, lanes=2)


def test_synthetic_camera_is_optional():
    """render / Stream / Sequence take a camera K; the default is intrinsics(H, W), and a given K changes the image."""
    import numpy as np
    from vo import synthetic
    from vo.primitives import Sequence
    H, W = 48, 64
    K = synthetic.intrinsics(H, W)
    a = synthetic.render(3, H, W, want_depth=False)[0]
    assert np.array_equal(a, synthetic.render(3, H, W, want_depth=False, K=K)[0])
    K2 = K.copy()
    K2[0, 0] *= 0.8
    b = synthetic.render(3, H, W, want_depth=False, K=K2)
    assert np.array_equal(b[3], K2) and not np.array_equal(a, b[0])
    assert np.array_equal(synthetic.Stream(5, H, W, K=K2).image(3), b[0])
    assert np.array_equal(synthetic.Stream(5, H, W).image(3), a)
    s = Sequence("synthetic", n_frames=5, height=H, width=W, intrinsics=K2)
    assert np.array_equal(s.get_camera().intrinsic_matrix, K2)
    assert np.array_equal(s.get_frame(3).image, b[0])
