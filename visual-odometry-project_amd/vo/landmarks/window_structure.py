"""Structure-only refinement of the last `window` frames' landmarks over the device pipeline's observation records
(include/vo_hip.h, "Window structure refinement"; csrc/window_structure.hip): the poses stay as the per-frame refinement left
them, every landmark of the window is re-triangulated over all the observations of its track.

    sr = WindowStructureRefiner(K, window=8, gate_px=2.0, min_parallax=0.0075)
    ...after every collected step:  pipe.export_tracks_post(r, pipe.cap, d_rec, seq); sr.push(d_rec, pose_of(r))
    out = sr.solve()       # None until `window` consecutive records are held

Records are handled as WindowBundleAdjuster handles them (a full window only, never across a hand-over), the window is joined
on the device by the same builder and refined there; the landmarks, their per-landmark results and the summary come back."""
import types

import numpy as np

from .window_ba import _WindowHolder, _full_windows, _join_windows


class WindowStructureRefiner(_WindowHolder):
    """The last `window` observation records of one sequence and the poses of their frames; solve() refines the landmarks.

    K: the sequence's intrinsics.  huber_px, max_iter, gate_px, min_parallax: vo_structure_params (0 = its default).  cap:
    the capacity the records were exported with (Pipeline.cap); L_cap: landmarks a window may hold (default: cap).  Records
    are device pointers the caller keeps alive while they are among the last `window` pushed."""

    def __init__(self, K, window=8, huber_px=0.0, max_iter=0, gate_px=0.0, min_parallax=0.0, cap=None, L_cap=None, context=None):
        super().__init__(K, window, cap, L_cap, context)
        self.params = dict(huber_px=float(huber_px), max_iter=int(max_iter), gate_px=float(gate_px), min_parallax=float(min_parallax))

    def solve(self):
        """The window held, refined: a namespace with poses (W, 12) as given, ids (L,), landmarks (L, 3), results (L,)
        STRUCTURE_RESULT rows, summary (a STRUCTURE_SUMMARY row), steps, flags and d_ids / d_X / n (the landmarks still on
        the device, for Pipeline.update_landmarks); None when fewer than `window` consecutive records are held."""
        return refine_windows([self])[0]


def refine_windows(refiners):
    """The windows of several refiners (same context, window length, capacities and parameters: the lanes of one pipeline)
    through ONE call of vo_window_structure_dev.  Returns a list with, per refiner, None (no full window) or the namespace
    WindowStructureRefiner.solve describes (d_ids / d_X are valid until the first refiner's next solve)."""
    from vo import _native
    out = [None] * len(refiners)
    ready = _full_windows(refiners)
    if not ready:
        return out
    first = ready[0][1]
    ctx = first.ctx
    ar, S, W, L_cap, M_cap = _join_windows(ready, "WindowStructureRefiner", summary=_native.STRUCTURE_SUMMARY.itemsize,
                                           res=lambda W, L_cap, M_cap: _native.STRUCTURE_RESULT.itemsize * L_cap)
    ctx.window_structure_dev(S, W, L_cap, M_cap, ar.d["head"], ar.d["K"], ar.d["poses"], ar.d["X"], ar.d["lm_start"],
                             ar.d["obs_slot"], ar.d["obs_xy"], ar.d["res"], ar.d["summary"], **first.params)
    head = ctx.download(ar.d["head"], (S, 4), np.int32)
    summary = ctx.download(ar.d["summary"], (S,), _native.STRUCTURE_SUMMARY)
    for q, (k, a, steps) in enumerate(ready):
        L = int(head[q, 0])
        ids = ctx.download(ar.at("lm_id", q), (L,), np.int32) if L else np.zeros(0, np.int32)
        X = ctx.download(ar.at("X", q), (L, 3), np.float64) if L else np.zeros((0, 3))
        res = ctx.download(ar.at("res", q), (L,), _native.STRUCTURE_RESULT) if L else np.zeros(0, _native.STRUCTURE_RESULT)
        out[k] = types.SimpleNamespace(poses=np.stack(a.poses), ids=ids, landmarks=X, results=res, summary=summary[q], steps=steps,
                                       flags=int(head[q, 2]), d_ids=ar.at("lm_id", q), d_X=ar.at("X", q), n=L)
    return out
