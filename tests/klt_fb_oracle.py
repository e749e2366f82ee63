"""CPU oracle of the tracker's forward-backward check (include/vo_hip.h, "pyramidal KLT": vo_klt_track_fb), composed from
the unchanged tracker oracle (oracle/csrc/klt.c through oracle.native.klt_track) called twice and the rule in NumPy float32:

  1. forward   (next_xy, status_f, err) = klt_track(prev, nxt, pts);
  2. backward  only for status_f = 1: klt_track(nxt, prev, next_xy as stored) -> (back_xy, status_b);
  3. distance  fb = dx*dx + dy*dy in float32 (two products, one sum), +inf where either status is 0;
  4. status    status_f & status_b & (fb <= float32(fb_max * fb_max)), the product formed in double; a tie is kept.

TEST INFRASTRUCTURE ONLY: nothing here touches the GPU."""
import numpy as np

from oracle import native
from pipeline_oracle import OracleContext, OracleLoop


def check_fb_max(fb_max):
    if not float(fb_max) > 0.0:
        raise ValueError("fb_max must be > 0 pixels (+inf allowed), got %r" % (fb_max,))
    return np.float32(float(fb_max) * float(fb_max))


def compare(pts, back_xy, status_f, status_b, thr2):
    """Rule items 3 and 4 from two tracker results: (status, fb).  back_xy: one row per point (any value where the
    backward pass did not run)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    back_xy = np.asarray(back_xy, np.float32).reshape(-1, 2)
    both = np.asarray(status_f).astype(bool) & np.asarray(status_b).astype(bool)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (back_xy[:, 0] - pts[:, 0]).astype(np.float32)
        dy = (back_xy[:, 1] - pts[:, 1]).astype(np.float32)
        d2 = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
    fb = np.where(both, d2, np.float32(np.inf)).astype(np.float32)
    status = (both & (fb <= np.float32(thr2))).astype(np.uint8)
    return status, fb


def fb_track(prev, nxt, pts, win=17, max_level=2, max_iter=10, eps=0.03, min_eig=1e-4, fb_max=1.0, thr2=None, track=None):
    """(next_xy, status, err, fb) of the rule.  thr2: the float32 threshold itself instead of fb_max.  track: the tracker
    to compose from (default: the CPU oracle), called as track(prev, nxt, pts, win=, max_level=, max_iter=, eps=, min_eig=)."""
    return fb_track_full(prev, nxt, pts, win, max_level, max_iter, eps, min_eig, fb_max, thr2, track)[:4]


def fb_track_full(prev, nxt, pts, win=17, max_level=2, max_iter=10, eps=0.03, min_eig=1e-4, fb_max=1.0, thr2=None, track=None):
    """fb_track's four arrays, then status_f, status_b (bool) and back_xy."""
    track = native.klt_track if track is None else track
    thr2 = check_fb_max(fb_max) if thr2 is None else np.float32(thr2)
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    kw = dict(win=win, max_level=max_level, max_iter=max_iter, eps=eps, min_eig=min_eig)
    next_xy, status_f, err = track(prev, nxt, pts, **kw)
    next_xy = np.asarray(next_xy, np.float32).reshape(-1, 2)
    fwd = np.asarray(status_f).reshape(-1).astype(bool)
    back_xy = np.zeros_like(next_xy)
    status_b = np.zeros(len(pts), bool)
    if fwd.any():
        b_xy, b_st, _ = track(nxt, prev, np.ascontiguousarray(next_xy[fwd]), **kw)
        back_xy[fwd] = np.asarray(b_xy, np.float32).reshape(-1, 2)
        status_b[fwd] = np.asarray(b_st).reshape(-1).astype(bool)
    status, fb = compare(pts, back_xy, fwd, status_b, thr2)
    return next_xy, status, np.asarray(err, np.float32).reshape(-1), fb, fwd, status_b, back_xy


class FBOracleContext(OracleContext):
    """OracleContext with the forward-backward call of vo._native.Context."""

    def __init__(self):
        self.fb_calls = 0
        self.rejected = []        # per call: points the existing filter (status_f & err < 100) keeps and the check drops

    def klt_track_fb(self, prev, nxt, prev_xy, win=17, max_level=2, max_iter=10, eps=0.03, min_eig=1e-4, fb_max=1.0):
        self.fb_calls += 1
        nxy, st, err, fb, sf = fb_track_full(prev, nxt, prev_xy, win, max_level, max_iter, eps, min_eig, fb_max)[:5]
        self.rejected.append(int((sf & (err < 100) & (st == 0)).sum()))
        return nxy, st, err, fb


class FBOracleLoop(OracleLoop):
    """OracleLoop whose tracker makes the forward-backward call: the device loop with Pipeline.set_klt_fb(fb_max)."""

    def __init__(self, *args, fb_max=1.0, **kwargs):
        super().__init__(*args, **kwargs)
        self.fb_max = fb_max

    def set_state(self, idx, features, curr_pose, prev_pose):
        super().set_state(idx, features, curr_pose, prev_pose)
        self.tracker._ctx = FBOracleContext()
        self.tracker._fb_threshold = self.fb_max
