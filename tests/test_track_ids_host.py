"""Track ids without a GPU: the rule (tests/track_ids_oracle.py) on hand-made cases, vo.driver.track_table on scripted
records, and the entry points in the header, the library and the binding."""
import ctypes
import os
import re

import numpy as np

import track_ids_oracle as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vo_pipeline_get_track_ids_seq", "vo_pipeline_set_track_ids_seq", "vo_pipeline_export_tracks_post_seq",
                "vo_pipeline_tracks_record_bytes")


def test_entry_points_are_declared_exported_and_bound():
    from vo import _native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_native.lib_path())
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _native._SIGS, name
    # the field sits in what was padding between sift_cap and match_ratio: no other field moves, the size stays
    assert re.search(r"int32_t\s+sift_cap\s*;\s*int32_t\s+track_ids\s*;\s*double\s+match_ratio\s*;", header)
    P = _native.PipelineConfig
    assert (P.track_ids.offset, P.match_ratio.offset) == (P.sift_cap.offset + 4, P.sift_cap.offset + 8)
    assert ctypes.sizeof(P) == P.st_min_distance.offset + 8 and P().track_ids == 0
    lib.vo_pipeline_tracks_record_bytes.restype = ctypes.c_size_t
    assert [lib.vo_pipeline_tracks_record_bytes(c) for c in (0, 1, 4000)] == [16, 64, 16 + 48 * 4000]
    from vo._pipeline import TRACK_HEADER, TRACK_ROW
    assert TRACK_HEADER.itemsize == 16 and TRACK_ROW.itemsize == 48 and TRACK_ROW.fields["X"][1] == 24


def test_handover_numbers_the_features_in_order():
    ids, born, nxt = tio.handover(5)
    assert ids.tolist() == [0, 1, 2, 3, 4] and born.tolist() == [0] * 5 and nxt == 5
    ids, born, nxt = tio.handover(0)
    assert len(ids) == 0 and nxt == 0


def klt_start():
    # ids deliberately not in order; states: two of every group
    ids = np.array([10, 4, 7, 1, 9, 3], np.int32)
    born = np.array([0, 0, 2, 2, 1, 5], np.int32)
    state = np.array([2, 1, 0, 2, 0, 1])
    return ids, born, state


def test_klt_rule_a_drop_in_every_group():
    ids, born, state = klt_start()
    keep = np.array([1, 0, 1, 0, 0, 1], bool)                   # one of every group dropped
    i2, b2, nxt = tio.klt_step(ids, born, 20, 6, state, 0, keep)
    assert i2.tolist() == [10, 3, 7] and b2.tolist() == [0, 5, 2] and nxt == 20
    # everything kept: [triangulated | matched | newly matched], each in feature order
    i2, b2, nxt = tio.klt_step(ids, born, 20, 6, state, 0, np.ones(6, bool))
    assert i2.tolist() == [10, 1, 4, 3, 7, 9] and b2.tolist() == [0, 2, 0, 5, 2, 1]


def test_klt_rule_appends():
    ids, born, state = klt_start()
    # an append of 0 keypoints (a Shi-Tomasi frame without corners): nothing issued
    i2, b2, nxt = tio.klt_step(ids, born, 20, 6, state, 0, np.ones(6, bool))
    assert nxt == 20 and 20 not in i2
    # three appended, the middle one dropped: its id is used up; appended ones are newly matched, behind the old ones
    keep = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1], bool)
    i2, b2, nxt = tio.klt_step(ids, born, 20, 6, state, 3, keep)
    assert i2.tolist() == [10, 1, 4, 3, 7, 9, 20, 22] and b2.tolist() == [0, 2, 0, 5, 2, 1, 6, 6] and nxt == 23
    # all appended dropped: the ids are burnt and next_id still moves
    keep = np.array([1, 1, 1, 1, 1, 1, 0, 0, 0], bool)
    i2, b2, nxt = tio.klt_step(ids, born, 20, 6, state, 3, keep)
    assert i2.tolist() == [10, 1, 4, 3, 7, 9] and nxt == 23
    # nothing survives at all
    i2, b2, nxt = tio.klt_step(ids, born, 20, 6, state, 2, np.zeros(8, bool))
    assert len(i2) == 0 and len(b2) == 0 and nxt == 22


def test_pairs_rule():
    ids, born, state = klt_start()
    # pairs in the matcher's order; old features 1 (matched), 2 and 4 (unmatched before), 0 (triangulated); 3 and 5 are lost
    pairs = np.array([[4, 0], [1, 5], [0, 2], [2, 3]])
    i2, b2, nxt = tio.pairs_step(ids, born, 20, 6, state, pairs, 7)
    # [triangulated: 0 | matched: 1 | newly matched: 4, 2 in pair order | unmatched new keypoints 1, 4, 6]
    assert i2.tolist() == [10, 4, 9, 7, 20, 21, 22] and b2.tolist() == [0, 0, 1, 2, 7, 7, 7] and nxt == 23
    # a drop in every group is what the missing old features 3 (triangulated), 5 (matched) and -- here -- 4 are
    i2, b2, nxt = tio.pairs_step(ids, born, 20, 6, state, pairs[1:], 7)
    assert i2.tolist() == [10, 4, 7, 20, 21, 22, 23] and nxt == 24
    # every new keypoint matched: nothing issued (an "append" of 0)
    i2, b2, nxt = tio.pairs_step(ids, born, 20, 6, state, np.array([[0, 1], [1, 0]]), 2)
    assert i2.tolist() == [10, 4] and nxt == 20
    # no pairs at all: every track ends, every new keypoint starts one
    i2, b2, nxt = tio.pairs_step(ids, born, 20, 6, state, np.empty((0, 2), int), 3)
    assert i2.tolist() == [20, 21, 22] and b2.tolist() == [7, 7, 7] and nxt == 23
    # no pairs and no keypoints
    i2, b2, nxt = tio.pairs_step(ids, born, 20, 6, state, np.empty((0, 2), int), 0)
    assert len(i2) == 0 and nxt == 20


def record(rows, step, next_id):
    from vo._pipeline import TRACK_HEADER, TRACK_ROW, TrackRecord
    body = np.zeros(len(rows), TRACK_ROW)
    for k, (i, born, x, y, state, land) in enumerate(rows):
        body[k] = (i, born, x, y, state, 0) + tuple(land)
    head = np.zeros(1, TRACK_HEADER)
    head[0] = (len(rows), step, next_id, 0)
    return TrackRecord.from_bytes(np.concatenate((head.view(np.uint8), body.view(np.uint8))), len(rows))


def test_track_record_and_track_table():
    from vo.driver import track_table
    nan3 = (np.nan,) * 3
    obs = [record([(0, 0, 1.0, 2.0, 2, (1, 2, 3)), (1, 0, 5.0, 6.0, 1, nan3)], 1, 2),
           record([(0, 0, 1.5, 2.5, 2, (1, 2, 4)), (1, 0, 5.5, 6.5, 0, nan3), (2, 1, 9.0, 9.0, 1, nan3)], 2, 3),
           record([(2, 1, 9.5, 9.5, 2, (7, 8, 9)), (0, 0, 2.0, 3.0, 0, nan3)], 3, 3)]
    assert (obs[1].n, obs[1].step, obs[1].next_id, obs[1].seq) == (3, 2, 3, 0) and len(obs[1]) == 3
    assert obs[0]["id"].tolist() == [0, 1] and obs[0]["X"][0] == 1.0 and np.isnan(obs[0]["Z"][1])
    t = track_table(obs)
    assert sorted(t) == [0, 1, 2]
    assert t[0]["steps"].tolist() == [0, 1, 2] and t[1]["steps"].tolist() == [0, 1] and t[2]["steps"].tolist() == [1, 2]
    assert t[0]["born"] == 0 and t[2]["born"] == 1
    assert t[0]["keypoints"].dtype == np.float32 and t[0]["keypoints"].tolist() == [[1.0, 2.0], [1.5, 2.5], [2.0, 3.0]]
    assert t[0]["landmark"].tolist() == [1.0, 2.0, 4.0]              # the last one it had (reset at step 2: kept)
    assert np.isnan(t[1]["landmark"]).all() and t[2]["landmark"].tolist() == [7.0, 8.0, 9.0]
    # a record cut by its capacity: n says how many there were
    cut = record([(0, 0, 1.0, 2.0, 2, (1, 2, 3))], 1, 2)
    raw = np.concatenate((np.array([5, 1, 9, 3], np.int32).view(np.uint8), np.asarray(cut).view(np.uint8)))
    from vo._pipeline import TrackRecord
    r = TrackRecord.from_bytes(raw, 1)
    assert (r.n, r.next_id, r.seq, len(r)) == (5, 9, 3, 1)
    assert track_table([]) == {}
