"""The track-id rule of include/vo_hip.h ("Track ids") in NumPy, and a recorder that feeds it from the oracle loop.

Each feature carries (id, born); the sequence carries next_id.  A hand-over numbers the features 0 .. n-1, born 0.  A KLT
step appends the re-detected keypoints with ids next_id .., born k, then filters and regroups; a descriptor step keeps
the pair's old feature's (id, born) and numbers the unmatched new keypoints next_id .., born k + 1.

The recorder wraps tests/pipeline_oracle.OracleLoop FROM THE OUTSIDE: in KLT mode the tracker shell's klt_track and
find_corners (status, err, appended count), in the descriptor modes pipeline_oracle.native.match_knn2_ratio (the pair
list); the old state codes are read from the oracle's Features before the step.  The ids it predicts therefore come from
the images through the oracle, never from the pipeline under test.

TEST INFRASTRUCTURE ONLY: nothing here touches the GPU."""
import numpy as np

import pipeline_oracle


def group_of(state):
    """Matches' groups (matches.py:26-212): 0 triangulated, 1 matched before, 2 newly matched."""
    state = np.asarray(state)
    return np.where(state == 2, 0, np.where(state == 1, 1, 2))


def handover(n):
    return np.arange(n, dtype=np.int32), np.zeros(n, np.int32), int(n)


def klt_step(ids, born, next_id, k, old_state, appended, keep):
    """ids, born, next_id before step k; old_state: the n old features' state codes; appended: keypoints the re-detect
    appended (0: none); keep: the filter's verdict over the n + appended tracker inputs.  Returns the new triple."""
    ids = np.concatenate((ids, next_id + np.arange(appended))).astype(np.int32)
    born = np.concatenate((born, np.full(appended, k))).astype(np.int32)
    g = group_of(np.concatenate((np.asarray(old_state), np.zeros(appended))))
    keep = np.asarray(keep, bool).reshape(-1)
    assert len(keep) == len(ids) == len(g)
    order = np.concatenate([np.flatnonzero(keep & (g == q)) for q in range(3)]).astype(int)
    return ids[order], born[order], int(next_id + appended)


def pairs_step(ids, born, next_id, k, old_state, pairs, n_new):
    """pairs: (M, 2) rows (old feature, new keypoint) in the matcher's order; n_new: keypoints of the new frame."""
    pairs = np.asarray(pairs, int).reshape(-1, 2)
    g = group_of(np.asarray(old_state)[pairs[:, 0]])
    src = np.concatenate([pairs[g == q, 0] for q in range(3)]).astype(int)
    unmatched = np.setdiff1d(np.arange(n_new), pairs[:, 1])            # ascending (np.delete(arange, matched))
    new_ids = np.concatenate((ids[src], next_id + np.arange(len(unmatched)))).astype(np.int32)
    new_born = np.concatenate((born[src], np.full(len(unmatched), k + 1))).astype(np.int32)
    return new_ids, new_born, int(next_id + len(unmatched))


class Recorder:
    """loop: an OracleLoop (or a subclass) whose state has been set.  step(next_idx) runs the loop's step and returns its
    dict plus ids / born / next_id after the step and, for the test's own assertions, appended (KLT: keypoints the step
    appended), appended_dropped (how many of those the filter dropped), unmatched (descriptor modes)."""

    def __init__(self, loop, monkeypatch=None):
        self.loop = loop
        self.seen = {}
        if loop.tracker_mode in ("sift", "harris"):
            assert monkeypatch is not None, "the descriptor modes' pair list is captured with monkeypatch"
            inner = pipeline_oracle.native.match_knn2_ratio

            def match(*a, **kw):
                out = inner(*a, **kw)
                self.seen["pairs"] = np.asarray(out[0]).reshape(-1, 2).copy()
                return out
            monkeypatch.setattr(pipeline_oracle.native, "match_knn2_ratio", match)
        else:
            self._wrap(loop.tracker)
        self.restart()

    def _wrap(self, tracker):
        ctx = tracker._context()
        klt, corners = ctx.klt_track, tracker.find_corners

        def klt_track(*a, **kw):
            out = klt(*a, **kw)
            self.seen["status"], self.seen["err"] = np.asarray(out[1]).copy(), np.asarray(out[2]).copy()
            return out

        def find_corners(*a, **kw):
            pts = corners(*a, **kw)
            self.seen["appended"] = int(len(pts))
            return pts
        ctx.klt_track = klt_track
        tracker.find_corners = find_corners
        self.err_threshold = tracker._error_threshold

    def restart(self, k=0):
        """A hand-over: the loop's current features are numbered 0 .. n-1."""
        self.ids, self.born, self.next_id = handover(self.loop.state.curr_frame.features.length)
        self.k = k

    def set(self, ids, born, next_id):
        self.ids, self.born, self.next_id = np.asarray(ids, np.int32).copy(), np.asarray(born, np.int32).copy(), int(next_id)

    def step(self, next_idx):
        old_state = np.asarray(self.loop.state.curr_frame.features.state).copy()
        assert len(old_state) == len(self.ids)
        self.seen.clear()
        ref = self.loop.step(next_idx)
        if self.loop.tracker_mode in ("sift", "harris"):
            pairs = self.seen["pairs"]
            self.ids, self.born, self.next_id = pairs_step(self.ids, self.born, self.next_id, self.k, old_state, pairs,
                                                           self.loop.n_new)
            ref["unmatched"] = self.loop.n_new - len(pairs)
        else:
            appended = self.seen.get("appended", 0)
            keep = self.seen["status"].reshape(-1).astype(bool) & (self.seen["err"].reshape(-1) < self.err_threshold)
            ref["appended"] = appended
            ref["appended_dropped"] = int((~keep[len(old_state):]).sum())
            self.ids, self.born, self.next_id = klt_step(self.ids, self.born, self.next_id, self.k, old_state, appended, keep)
        self.k += 1
        assert len(self.ids) == ref["features"].length and len(np.unique(self.ids)) == len(self.ids)
        ref["ids"], ref["born"], ref["next_id"] = self.ids.copy(), self.born.copy(), self.next_id
        return ref
