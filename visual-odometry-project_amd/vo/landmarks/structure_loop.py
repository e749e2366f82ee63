"""The structure refinement inside the device-resident frame loop (include/vo_hip.h, "Structure loop";
csrc/structure_loop.hip): the last `window` observation records of every lane stay in a ring on the device, and one call per
collected step queues record, window join, refinement and write-back on the pipeline's stream.

    loop = pipe.structure_loop(window=8, gate_px=2.0)
    pipe.submit(a, b)
    ...   rs = pipe.collect_all(); j = loop.post(rs); pipe.submit(b, c)       # one step stays in flight
    entries = loop.poll(j)          # None until a step submitted after the post has been collected (or wait=True)

Nothing is read back unless asked for: poll returns the entries (dtype STRUCTURE_LOOP_ENTRY, one per lane) the device copied
into pinned memory, download synchronises and returns a lane's last window."""
import ctypes as C
import types

import numpy as np


def ring_slots(n_posts, window):
    """Ring slots of the last `window` records, oldest first, after n_posts posts (post j goes to slot j % window)."""
    return [(n_posts - window + s) % window for s in range(window)]


def ring_full(headers, window):
    """The rule of vo_structure_loop_post's item 2 on the (step, next_id) headers posted since the last reset, oldest first:
    full iff `window` of them exist and, among the last `window`, every step follows its predecessor by one and no next_id
    decreases."""
    if len(headers) < window:
        return False
    last = headers[-window:]
    return all(int(b[0]) == int(a[0]) + 1 and int(b[1]) >= int(a[1]) for a, b in zip(last[:-1], last[1:]))


class StructureLoop:
    """vo_structure_loop of one Pipeline (Pipeline.structure_loop makes it).  window: W records; L_cap / M_cap: the window's
    capacities (None: the feature capacity, L_cap * W); feedback: refined landmarks go back into the features, one step
    late at most; structure_params: vo_structure_params' huber_px, max_iter, max_trials, lambda0, step_tol, f_tol, gate_px,
    min_parallax."""

    def __init__(self, pipe, window, L_cap=None, M_cap=None, feedback=True, **structure_params):
        from vo import _native
        self.pipe, self.ctx = pipe, pipe.ctx
        self.window = int(window)
        self.L_cap = int(L_cap) if L_cap else pipe.cap
        self.M_cap = int(M_cap) if M_cap else self.L_cap * self.window
        self.feedback = bool(feedback)
        cfg = _native.StructureLoopConfig(self.window, int(L_cap or 0), int(M_cap or 0), 1 if feedback else 0,
                                          _native.structure_params(**structure_params))
        h = C.c_void_p()
        self.ctx._chk(self.ctx._lib.vo_structure_loop_create(pipe._h, C.byref(cfg), C.byref(h)))
        self._h = h
        self.n_posts = 0

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.pipe, "_h", None):           # (a closed pipeline has released its loop)
                self.ctx._lib.vo_structure_loop_destroy(self._h)
            self._h = None
            if getattr(self.pipe, "_loop", None) is self:
                self.pipe._loop = None

    def post(self, results):
        """Queues the record, the window, the refinement and the write-back of the step collected last; results: what
        collect_all returned (or one StepResult of a one-lane pipeline).  Never waits.  Returns the post's index."""
        from vo import _native
        if isinstance(results, _native.StepResult):
            results = [results]
        if len(results) != self.pipe.sequences:
            raise ValueError("StructureLoop.post: %d results for %d lanes" % (len(results), self.pipe.sequences))
        rs = (_native.StepResult * len(results))(*results)
        self.ctx._chk(self.ctx._lib.vo_structure_loop_post(self._h, rs))
        self.n_posts += 1
        return self.n_posts - 1

    def reset(self, seq=0):
        """Forgets lane `seq`'s window (a hand-over: ids start again)."""
        self.ctx._chk(self.ctx._lib.vo_structure_loop_reset_seq(self._h, int(seq)))

    def poll(self, index, wait=False):
        """The entries of post `index` (one STRUCTURE_LOOP_ENTRY row per lane), or None while they are on their way
        (wait=False).  wait=True blocks on the post's event."""
        from vo import _native
        out = np.zeros(self.pipe.sequences, _native.STRUCTURE_LOOP_ENTRY)
        rc = self.ctx._lib.vo_structure_loop_poll(self._h, int(index), 1 if wait else 0, out.ctypes.data_as(C.c_void_p))
        if rc == 1:
            return None
        self.ctx._chk(rc)
        return out

    def download(self, seq=0):
        """Lane `seq`'s last window and its refinement (synchronises): a namespace with head (4,), poses (W, 12), lm_start
        (L + 1,), obs_slot (M,), obs_xy (M, 2), X_in (L, 3), lm_id (L,), X (L, 3), results (L,) STRUCTURE_RESULT rows,
        summary, entry, and window(): the six arrays of the join as tests/test_gpu_window_ba.py's numpy_window names them."""
        from vo import _native
        W, Lc, Mc = self.window, self.L_cap, self.M_cap
        a = dict(head=np.zeros(4, np.int32), poses=np.zeros((W, 12)), lm_start=np.zeros(Lc + 1, np.int32),
                 obs_slot=np.zeros(Mc, np.int32), obs_xy=np.zeros((Mc, 2)), X_in=np.zeros((Lc, 3)), lm_id=np.zeros(Lc, np.int32),
                 X=np.zeros((Lc, 3)), results=np.zeros(Lc, _native.STRUCTURE_RESULT), summary=np.zeros(1, _native.STRUCTURE_SUMMARY),
                 entry=np.zeros(1, _native.STRUCTURE_LOOP_ENTRY))
        self.ctx._chk(self.ctx._lib.vo_structure_loop_download_seq(self._h, int(seq), *[v.ctypes.data_as(C.c_void_p) for v in a.values()]))
        L, M = int(a["head"][0]), int(a["head"][1])
        out = types.SimpleNamespace(head=a["head"], poses=a["poses"], lm_start=a["lm_start"][:L + 1].copy(), obs_slot=a["obs_slot"][:M].copy(),
                                    obs_xy=a["obs_xy"][:M].copy(), X_in=a["X_in"][:L].copy(), lm_id=a["lm_id"][:L].copy(),
                                    X=a["X"][:L].copy(), results=a["results"][:L].copy(), summary=a["summary"][0], entry=a["entry"][0],
                                    L=L, M=M)
        out.window = lambda: dict(head=out.head, lm_start=out.lm_start, obs_slot=out.obs_slot, obs_xy=out.obs_xy, X=out.X_in,
                                  lm_id=out.lm_id)
        return out
