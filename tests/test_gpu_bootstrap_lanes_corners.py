"""-m gpu: vo_pipeline_bootstrap_lanes' first stage is one batched Shi-Tomasi call (vo_good_features_batch_dev) over the
named lanes' frame-a images.  Four different scenes in one L = 4 call: every lane's corner count is the oracle's for its
own frame, the lanes end as the one-lane call leaves them, and the call moves fewer bytes to the host than before the
batched stage existed (no read-back of candidate or corner counts: they reach the host with the result's download).

The file's name puts it behind tests/test_gpu_pipeline_bootstrap_lanes.py, whose helpers it imports."""
import numpy as np
import pytest

from oracle import native
from test_gpu_pipeline_bootstrap import SMALL, boot_kwargs
from test_gpu_pipeline_bootstrap_lanes import boot, lane_data, lanes_pipe, same_everything, same_results

pytestmark = pytest.mark.gpu

# bytes_d2h per lane of this file's 4-lane call (second call on a pipeline) measured on the commit before this stage was
# batched, and by tools/dev/pipeline_bootstrap.py --lanes 4 at 1376x1241 there: 384 = the result's F, M and counts (272) + the
# RANSAC loop's control block (88) + Shi-Tomasi's candidate count (8) and corner count + fault word (16).  The batched stage
# reads nothing back: the last 24 are gone, no part of them left (measured: 360).
PARENT_D2H_PER_LANE = 384
SHI_TOMASI_READ_BACKS = 24


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def test_four_scenes_in_one_call(ctx):
    cfg, S = SMALL, 4
    data = lane_data(cfg, S)
    assert len({d["img0"].tobytes() for d in data}) == S
    pipe, single = lanes_pipe(ctx, cfg, data), lanes_pipe(ctx, cfg, data)
    res = boot(pipe, "lanes", [tuple(range(S))], 1, 0, cfg)
    res1 = boot(single, "single", [tuple(range(S))], 1, 0, cfg)
    for q in range(S):
        ref = native.good_features(data[q]["img0"], None, boot_kwargs(cfg)["max_corners"], 0.01, 8, 7)
        assert res[q].status == 0, (q, res[q].status)
        assert res[q].n_corners == len(ref), (q, res[q].n_corners, len(ref))
        same_results(res[q], res1[q], ("lane", q))
        same_everything(pipe.get_state(seq=q), single.get_state(seq=q), ("lane", q))
    again = pipe.bootstrap_lanes(1, 0, list(range(S)), **boot_kwargs(cfg))       # (workspaces and the threshold table are up)
    print("bytes per lane down: first call %d, second %d (before: %d)" % (res[0].bytes_d2h, again[0].bytes_d2h, PARENT_D2H_PER_LANE))
    for r in again:
        assert r.status == 0
        assert r.bytes_d2h < PARENT_D2H_PER_LANE, r.bytes_d2h
        assert r.bytes_d2h == PARENT_D2H_PER_LANE - SHI_TOMASI_READ_BACKS, r.bytes_d2h
    pipe.close()
    single.close()


def test_a_lane_without_corners_fails_alone(ctx):
    """A flat frame a among four lanes: that lane is VO_ETRACKING with 0 corners reported, the others have their oracle
    counts and go through."""
    cfg, S = SMALL, 4
    data = [dict(d) for d in lane_data(cfg, S)]
    data[1]["img0"] = np.full((cfg["H"], cfg["W"]), 128, np.uint8)
    pipe = lanes_pipe(ctx, cfg, data)
    res = {r.seq: r for r in pipe.bootstrap_lanes(1, 0, list(range(S)), **boot_kwargs(cfg))}
    assert res[1].status == -5 and res[1].n_corners == 0
    for q in (0, 2, 3):
        ref = native.good_features(data[q]["img0"], None, boot_kwargs(cfg)["max_corners"], 0.01, 8, 7)
        assert res[q].status == 0 and res[q].n_corners == len(ref), q
    pipe.close()
