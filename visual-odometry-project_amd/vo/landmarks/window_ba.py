"""Sliding-window bundle adjustment over the device pipeline's observation records (include/vo_hip.h, "Window bundle
adjustment"; csrc/window_ba.hip).  The reference has no back end; this is what `driver.track_table` was waiting for.

    ba = WindowBundleAdjuster(K, window=6)
    ...after every collected step:  pipe.export_tracks_post(r, pipe.cap, d_rec, seq); ba.push(d_rec, pose_of(r))
    out = ba.solve()       # None until `window` consecutive records are held

The records stay in device memory: the window is joined there (Context.window_from_tracks), solved there
(Context.window_ba_dev), and only the refined poses, the landmark ids / coordinates and the result come back."""
import types

import numpy as np


def pack_windows(windows, W=None):
    """Host windows -> the strided arrays Context.window_ba takes.  windows: objects with poses (W, 12), X (L, 3),
    lm_start (L + 1,), obs_slot (M,), obs_xy (M, 2), K (3, 3); all with the same W.  Returns a dict of its arguments."""
    W = W or len(windows[0].poses)
    L_cap = max(1, max(len(w.X) for w in windows))
    M_cap = max(1, max(len(w.obs_slot) for w in windows))
    S = len(windows)
    out = dict(K=np.zeros((S, 3, 3)), poses=np.zeros((S, W, 12)), X=np.zeros((S, L_cap, 3)),
               lm_start=np.zeros((S, L_cap + 1), np.int32), obs_slot=np.zeros((S, M_cap), np.int32),
               obs_xy=np.zeros((S, M_cap, 2)), counts=np.zeros((S, 2), np.int32))
    for q, w in enumerate(windows):
        L, M = len(w.X), len(w.obs_slot)
        if len(w.poses) != W:
            raise ValueError("pack_windows: window %d has %d slots, the batch %d" % (q, len(w.poses), W))
        out["K"][q], out["poses"][q], out["counts"][q] = w.K, w.poses, (L, M)
        out["X"][q, :L], out["lm_start"][q, :L + 1] = w.X, w.lm_start
        out["obs_slot"][q, :M], out["obs_xy"][q, :M] = w.obs_slot, w.obs_xy
    return out


def pose_cw12(pose):
    """A world -> camera pose as 12 doubles (R row-major, then t) from (12,), (3, 4) or (4, 4)."""
    p = np.asarray(pose, np.float64)
    if p.size == 12 and p.ndim == 1:
        return p.copy()
    p = p.reshape(-1, 4)[:3]
    return np.concatenate((p[:, :3].reshape(9), p[:, 3]))


class _Arena:
    """Device arrays of S windows (W slots, L_cap landmarks, M_cap observations each)."""

    def __init__(self, ctx, S, W, L_cap, M_cap, **more):
        self.ctx, self.shape = ctx, (S, W, L_cap, M_cap)
        sizes = dict(head=16, K=72, poses=96 * W, X=24 * L_cap, lm_start=4 * (L_cap + 1), obs_slot=4 * M_cap,
                     obs_xy=16 * M_cap, lm_id=4 * L_cap, res=40)
        sizes.update(more)            # (bytes per window of a further array, or another size for one of these)
        self.stride = sizes
        self.d = {k: ctx.alloc(S * v) for k, v in sizes.items()}

    def at(self, name, q):
        return self.d[name] + q * self.stride[name]

    def close(self):
        for p in self.d.values():
            self.ctx.free(p)
        self.d = {}


class _WindowHolder:
    """The last `window` observation records of one sequence (device pointers the caller keeps alive while they are among
    them) and the poses of their frames.  cap: the capacity the records were exported with (Pipeline.cap); L_cap: landmarks
    a window may hold (default: cap)."""

    def __init__(self, K, window, cap, L_cap, context):
        from vo import _native
        if not 2 <= int(window) <= 16:
            raise ValueError("%s: window must be 2 .. 16 frames, got %r" % (type(self).__name__, window))
        self.ctx = context or _native.default_context()
        self.K = np.asarray(K, np.float64).reshape(3, 3).copy()
        self.window = int(window)
        self.cap, self.L_cap = cap, L_cap
        self.records, self.poses = [], []
        self._arena = None

    def reset(self):
        """Forgets the window (a hand-over: ids start again and a window must not span it)."""
        self.records, self.poses = [], []

    def push(self, d_record, pose_cw):
        """The record of the next step (device pointer) and that frame's world -> camera pose."""
        self.records = (self.records + [int(d_record)])[-self.window:]
        self.poses = (self.poses + [pose_cw12(pose_cw)])[-self.window:]

    def close(self):
        if self._arena:
            self._arena.close()
            self._arena = None


class WindowBundleAdjuster(_WindowHolder):
    """The last `window` observation records of one sequence and the poses of their frames; solve() adjusts them.

    K: the sequence's intrinsics.  n_fixed, huber_px, max_iter: vo_ba_params (0 = its default).  cap: the capacity the
    records were exported with (Pipeline.cap); L_cap: landmarks a window may hold (default: cap).  Records are device
    pointers the caller keeps alive while they are among the last `window` pushed."""

    def __init__(self, K, window=8, n_fixed=2, huber_px=0.0, max_iter=0, cap=None, L_cap=None, context=None):
        super().__init__(K, window, cap, L_cap, context)
        if not 1 <= int(n_fixed) < int(window):
            raise ValueError("WindowBundleAdjuster: n_fixed must be 1 .. window - 1, got %r" % (n_fixed,))
        self.params = dict(n_fixed=int(n_fixed), huber_px=float(huber_px), max_iter=int(max_iter))

    def solve(self):
        """(poses (W, 12), ids (L,), landmarks (L, 3), result) of the window held, or None when fewer than `window`
        consecutive records are."""
        r = solve_windows([self])[0]
        return None if r is None else (r.poses, r.ids, r.landmarks, r.result)


def _headers(adj):
    """(step, next_id) of the records held; drops what lies before a break (a step that does not follow the previous one,
    a next_id that decreases) and returns the steps left."""
    from vo._pipeline import TRACK_HEADER
    heads = [adj.ctx.download(d, (1,), TRACK_HEADER)[0] for d in adj.records]
    keep = 0
    for k in range(1, len(heads)):
        if int(heads[k]["step"]) != int(heads[k - 1]["step"]) + 1 or int(heads[k]["next_id"]) < int(heads[k - 1]["next_id"]):
            keep = k
    if keep:
        adj.records, adj.poses = adj.records[keep:], adj.poses[keep:]
    return [int(h["step"]) for h in heads[keep:]]


def _full_windows(holders):
    """(index, holder, steps) of the holders that hold a full window of consecutive records."""
    ready = []
    for k, a in enumerate(holders):
        if len(a.records) == a.window:
            steps = _headers(a)
            if len(a.records) == a.window:
                ready.append((k, a, steps))
    return ready


def _join_windows(ready, who, **more):
    """The windows of `ready` (_full_windows) joined on the device into the first holder's arena, K and the poses uploaded.
    more: further arrays of the arena (name -> bytes per window, or a function of (W, L_cap, M_cap))."""
    first = ready[0][1]
    ctx, W = first.ctx, first.window
    cap = first.cap
    if cap is None:
        raise ValueError("%s: cap (the records' capacity) was not given" % who)
    L_cap = first.L_cap or cap
    M_cap = L_cap * W
    S = len(ready)
    if first._arena is None or first._arena.shape != (S, W, L_cap, M_cap):
        if first._arena:
            first._arena.close()
        first._arena = _Arena(ctx, S, W, L_cap, M_cap, **{k: v(W, L_cap, M_cap) if callable(v) else v for k, v in more.items()})
    ar = first._arena
    ctx.upload(ar.d["K"], np.stack([a.K for _, a, _ in ready]))
    ctx.upload(ar.d["poses"], np.stack([np.stack(a.poses) for _, a, _ in ready]))
    for q, (_, a, _) in enumerate(ready):
        ctx.window_from_tracks(a.records, cap, L_cap, M_cap, ar.at("head", q), ar.at("lm_start", q), ar.at("obs_slot", q),
                               ar.at("obs_xy", q), ar.at("X", q), ar.at("lm_id", q))
    return ar, S, W, L_cap, M_cap


def solve_windows(adjusters):
    """The windows of several adjusters (same context, window length, capacities and parameters: the lanes of one pipeline)
    through ONE solver call.  Returns a list with, per adjuster, None (no full window) or a namespace: poses (W, 12), ids
    (L,), landmarks (L, 3), result (a BA_RESULT row), steps (the records' step counters), flags (the builder's), and
    d_ids / d_X / n: the refined landmarks still on the device (valid until the first adjuster's next solve)."""
    from vo import _native
    out = [None] * len(adjusters)
    ready = _full_windows(adjusters)
    if not ready:
        return out
    first = ready[0][1]
    ctx = first.ctx
    ar, S, W, L_cap, M_cap = _join_windows(ready, "WindowBundleAdjuster")
    ctx.window_ba_dev(S, W, L_cap, M_cap, ar.d["head"], ar.d["K"], ar.d["poses"], ar.d["X"], ar.d["lm_start"],
                      ar.d["obs_slot"], ar.d["obs_xy"], ar.d["res"], **first.params)
    head = ctx.download(ar.d["head"], (S, 4), np.int32)
    res = ctx.download(ar.d["res"], (S,), _native.BA_RESULT)
    poses = ctx.download(ar.d["poses"], (S, W, 12), np.float64)
    for q, (k, a, steps) in enumerate(ready):
        L = int(head[q, 0])
        ids = ctx.download(ar.at("lm_id", q), (L,), np.int32) if L else np.zeros(0, np.int32)
        X = ctx.download(ar.at("X", q), (L, 3), np.float64) if L else np.zeros((0, 3))
        out[k] = types.SimpleNamespace(poses=poses[q], ids=ids, landmarks=X, result=res[q], steps=steps, flags=int(head[q, 2]),
                                       d_ids=ar.at("lm_id", q), d_X=ar.at("X", q), n=L)
    return out
