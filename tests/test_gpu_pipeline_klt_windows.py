"""-m gpu: the frame loop of tests/test_gpu_pipeline_klt_fb.py at the tracker's other windows -- 9 (the generic kernel,
klt_track_kernel), 17 and 21 (the other two row kernels, klt_track16_kernel) -- plain and with the forward-backward check,
against the CPU oracle of the same loop; and two sequences through the generic kernel.  Both kernels take their points
from one prologue in csrc/klt.hip (klt_points, klt_point_start): the device-side count, vo_klt_source's re-detect rule
and the detector's keypoints as start points.  Every run here re-detects at least once and never leaves the device path,
so that branch runs in every instantiation; tests/test_klt_fb_host.py holds the oracle loops to the same condition."""
import pytest

from test_gpu_pipeline import check_state, check_step, run_all
from test_gpu_pipeline_klt_fb import fb_pipe, finish, two_sequences_equal_each_run_alone
from test_klt_fb_host import LOOP, OTHER_WINDOWS, loop_start, oracle_loop

pytestmark = pytest.mark.gpu
P = LOOP
FORMS = pytest.mark.parametrize("fb_max", [None, P["fb_max"]], ids=["plain", "fb"])


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


EVERY_FRAME = dict(detect_margin=-1.0)         # the detector runs on every frame (test_loop_matches_the_oracle_loop)


def start():
    stream, feats, T = loop_start()
    order = stream.order(P["steps"])
    return stream, feats, T, list(zip(order[:-1], order[1:]))


@FORMS
@pytest.mark.parametrize("win", OTHER_WINDOWS)
def test_loop_matches_the_oracle_loop(ctx, win, fb_max):
    """Every integer of every step record, every carried array, the generator; poses within check_step's tolerances.

    detect_margin < 0: the detector runs on every frame.  Whether it runs is otherwise a guess made one step early from the
    last step's loss (csrc/pipeline_step.hip, detect_decide_kernel); these loops lose up to 110 of 249 features in their
    first step, the guess misses, and the re-detect step is finished by the host path (VO_FAULT_NO_DETECTION) -- measured
    with the default margin at 9-fb, 17-fb, 21-plain and 21-fb, on this tree and on the one before it alike, with the same
    counts in every record.  The margin changes no result, only which frames have keypoints ready."""
    stream, feats, T, pairs = start()
    pipe = fb_pipe(ctx, stream, feats, T, fb_max=fb_max, win=win, **EVERY_FRAME)
    assert pipe.klt_fb == (fb_max or 0.0)
    orc = oracle_loop(stream, fb_max, win=win)
    orc.set_state(0, feats, T, T)
    check_state(pipe.get_state(), feats, T)
    redetects = 0
    for a, b in pairs:
        ref = orc.step(b)
        r = pipe.step(a, b)
        redetects += r.redetected
        assert r.recovered == 0 and r.n_features_in == ref["n_before"] + (P["N"] if r.redetected else 0)
        check_step(r, ref, pipe, orc.rs.rng)
    assert redetects >= 1, "a re-detect was meant to run"
    pipe.close()


@FORMS
def test_two_sequences_through_the_generic_kernel(ctx, fb_max):
    """Window 9, sequences = 2: grid.y != 0 together with vo_klt_source in klt_track_kernel; records, states and
    generators equal each sequence run alone.  The detector runs on every frame here too, and no step of any run --
    alone or in the pair -- leaves the device path, so the re-detect's det_kp branch runs at grid.y = 1 in the kernel."""
    win = 9
    stream, feats, T, pairs = begin = start()
    pipe = fb_pipe(ctx, stream, feats, T, fb_max=fb_max, win=win, **EVERY_FRAME)
    res = run_all(pipe, pairs, False)
    blocking = (res,) + finish(pipe)
    pipe.close()
    assert sum(r.redetected for r in res) >= 1 and not any(r.recovered for r in res)
    two_sequences_equal_each_run_alone(ctx, begin, blocking, win, fb_max, device_only=True, **EVERY_FRAME)
