"""CPU: the structure loop's C ABI (include/vo_hip.h, "Structure loop") is declared, exported and bound, and the ring rule
the device applies -- post j goes to slot j % W, age s of the window is slot (n_posts - W + s) % W, and the window is full
iff W records were posted since the reset, every step counter follows its predecessor by one and no next_id decreases --
is, on hand-made header sequences, what vo.landmarks.window_ba._headers / _full_windows decide for the same pushes."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vo_structure_loop_create", "vo_structure_loop_post", "vo_structure_loop_posts", "vo_structure_loop_reset_seq",
         "vo_structure_loop_poll", "vo_structure_loop_download_seq", "vo_structure_loop_destroy")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_hip.h")).read(), flags=re.S)


def test_header_declares_every_entry_point():
    text = header_text()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert "vo_structure_loop* loop" in m.group(1) or name == "vo_structure_loop_create"
    assert re.search(r"typedef struct vo_structure_loop_config\s*\{[^}]*window;[^}]*L_cap, M_cap;[^}]*feedback;[^}]*vo_structure_params params;",
                     text)
    assert re.search(r"typedef struct vo_structure_loop_entry\s*\{[^}]*step;[^}]*full;[^}]*L, M, flags;[^}]*n_written;[^}]*"
                     r"vo_structure_summary summary;", text)
    doc = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    assert "Structure loop" in doc and "bit for bit the window's input" in doc


def test_binding_table_lists_every_entry_point():
    import ctypes
    from vo import _native
    text = header_text()
    lib = ctypes.CDLL(_native.lib_path())
    for name in NAMES:
        assert name in _native._SIGS, name
        assert hasattr(lib, name), name
        res, args = _native._SIGS[name]
        declared = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        assert res is ctypes.c_int and len(args) == len(declared.split(",")), name
    # the entry and the configuration as the C structs lay them out
    assert _native.STRUCTURE_LOOP_ENTRY.itemsize == 24 + _native.STRUCTURE_SUMMARY.itemsize == 56
    assert _native.STRUCTURE_LOOP_ENTRY.fields["summary"][1] == 24
    assert ctypes.sizeof(_native.StructureLoopConfig) == 16 + ctypes.sizeof(_native.StructureParams)
    from vo.landmarks import StructureLoop
    from vo._pipeline import Pipeline
    assert callable(Pipeline.structure_loop) and all(hasattr(StructureLoop, k) for k in ("post", "reset", "poll", "download", "close"))


# ---- the ring rule against _headers ----

class FakeContext:
    """Context.download for record "pointers" that are indices into a list of headers."""

    def __init__(self):
        self.heads = []

    def put(self, step, next_id):
        self.heads.append((step, next_id))
        return len(self.heads) - 1

    def download(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        out[0]["step"], out[0]["next_id"] = self.heads[int(d)]
        return out


class NumpyRing:
    """The loop's ring of one lane as the device keeps it: W slots, post j into slot j % W; the host counts the records since
    the reset, the headers decide the rest."""

    def __init__(self, W):
        self.W, self.slots, self.n_posts, self.count = W, [None] * W, 0, 0

    def reset(self):
        self.count = 0

    def post(self, header):
        from vo.landmarks import ring_slots
        self.slots[self.n_posts % self.W] = header
        self.n_posts += 1
        self.count += 1
        if self.count < self.W:
            return False, None
        window = [self.slots[s] for s in ring_slots(self.n_posts, self.W)]
        ok = all(b[0] == a[0] + 1 and b[1] >= a[1] for a, b in zip(window[:-1], window[1:]))
        return ok, window


def holder_decides(W, ctx, holder, header):
    """WindowStructureRefiner's bookkeeping (push, then _full_windows) for one more record: (full, the window's steps)."""
    from vo.landmarks.window_ba import _full_windows
    d = ctx.put(*header)
    holder.records = (holder.records + [d])[-W:]
    holder.poses = (holder.poses + [None])[-W:]
    ready = _full_windows([holder])
    return (True, ready[0][2]) if ready else (False, None)


CLEAN = [(k, 10 + 3 * k) for k in range(1, 12)]
SEQUENCES = {
    "clean": (CLEAN, ()),
    "wrap": ([(k, 100) for k in range(5, 5 + 23)], ()),
    "step_does_not_follow": (CLEAN[:5] + [(9, 40), (10, 41), (11, 45), (12, 45), (13, 46), (14, 50), (15, 50)], ()),
    "step_repeats": (CLEAN[:4] + [CLEAN[3]] + [(k, 60) for k in range(5, 12)], ()),
    "next_id_decreases": ([(1, 50), (2, 55), (3, 60), (4, 20), (5, 22), (6, 22), (7, 30), (8, 31), (9, 31), (10, 40)], ()),
    "reset": (CLEAN, (5,)),                     # (a reset in front of these posts; steps go on: only the count says so)
    "restart_without_reset": (CLEAN[:6] + [(1, 8), (2, 9), (3, 9), (4, 12), (5, 12), (6, 13)], ()),
}


@pytest.mark.parametrize("W", [2, 3, 4, 5])
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_ring_rule_is_the_refiners(name, W):
    from vo.landmarks import ring_full
    headers, resets = SEQUENCES[name]
    ctx = FakeContext()
    holder = types.SimpleNamespace(ctx=ctx, window=W, records=[], poses=[])
    ring = NumpyRing(W)
    since, n_full = [], 0
    for j, h in enumerate(headers):
        if j in resets:
            ring.reset()
            holder.records, holder.poses = [], []       # (WindowStructureRefiner.reset)
            since = []
        since.append(h)
        want_full, want_steps = holder_decides(W, ctx, holder, h)
        got_full, window = ring.post(h)
        assert got_full == want_full == ring_full(since, W), (name, W, j)
        if got_full:
            assert [s for s, _ in window] == want_steps == [h[0] - W + 1 + k for k in range(W)]
            n_full += 1
    assert n_full > 0, "the sequence was meant to hold full windows"
    if name != "clean" and name != "wrap":
        assert n_full < len(headers) - W + 1, "and a break"


def test_ring_slots_are_age_ordered():
    from vo.landmarks import ring_slots
    for W in (2, 3, 5, 16):
        for n in range(W, 4 * W + 3):
            slots = ring_slots(n, W)
            assert sorted(slots) == list(range(W))
            assert slots[-1] == (n - 1) % W and slots[0] == n % W          # newest = the last post's, oldest = the next to go
            assert [(s - slots[0]) % W for s in slots] == list(range(W))


def test_driver_refuses_stream_feedback_without_its_mode():
    from vo import driver
    from vo.primitives import Sequence
    seq = Sequence("synthetic", n_frames=6, height=240, width=320)
    with pytest.raises(ValueError, match="ba_mode"):
        driver._DeviceRun([seq], 1, None, None, "host", True, (), (), ba_window=4, ba_feedback="stream", ba_mode="full")
    with pytest.raises(ValueError, match="ba_window"):
        driver._DeviceRun([seq], 1, None, None, "host", True, (), (), ba_feedback="stream", ba_mode="structure")
    with pytest.raises(ValueError, match="ba_feedback"):
        driver._DeviceRun([seq], 1, None, None, "host", True, (), (), ba_window=4, ba_feedback="later", ba_mode="structure")
