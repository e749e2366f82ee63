"""CPU: the C ABI of the per-sequence descriptor entry points (Harris tracker mode with several sequences) -- declared in
include/vo_hip.h, exported by the built library, bound in vo/_native.py with the argument types of the declaration."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vo_hip.h")
SYMBOLS = {
    "vo_pipeline_set_descriptors_seq": "int vo_pipeline_set_descriptors_seq(vo_pipeline* p, int seq, const float* desc, int n);",
    "vo_pipeline_get_descriptors_seq": "int vo_pipeline_get_descriptors_seq(vo_pipeline* p, int seq, float* desc, int32_t* n_out);",
}


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_declared_in_the_header(name):
    text = _squash(open(HEADER).read())
    assert _squash(SYMBOLS[name]) in text


def test_header_says_harris_mode_takes_any_number_of_sequences():
    text = _squash(open(HEADER).read())
    assert "KLT and Harris tracker modes: any S; SIFT tracker mode: one." in text


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_exported_by_the_library(name):
    from vo import _native
    path = _native.lib_path()
    if not os.path.exists(path):
        pytest.fail("libvo_hip.so is not built: %s" % path)
    lib = C.CDLL(path)
    assert getattr(lib, name, None) is not None, name       # (dlsym: the dynamic symbol table has it)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_bound_with_the_declared_argument_types(name):
    from vo import _native
    res, args = _native._SIGS[name]
    assert res is C.c_int
    # (vo_pipeline*, int seq, float* desc, int n) / (vo_pipeline*, int seq, float* desc, int32_t* n_out)
    want = [C.c_void_p, C.c_int, C.c_void_p, C.c_int if name.startswith("vo_pipeline_set") else C.c_void_p]
    assert args == want
    lib = _native.load()
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == want


def test_pipeline_wrapper_sends_descriptors_to_the_sequence_it_is_given():
    """Pipeline.set_state(..., seq=q) in a descriptor mode calls the _seq entry with q; get_descriptors(seq=q) reads q's."""
    import numpy as np
    from vo._pipeline import Pipeline

    calls = []

    class Lib:
        def vo_pipeline_set_state_seq(self, h, seq, idx, *args):
            calls.append(("state", seq, idx))
            return 0

        def vo_pipeline_set_descriptors_seq(self, h, seq, ptr, n):
            calls.append(("desc", seq, n))
            return 0

        def vo_pipeline_get_descriptors_seq(self, h, seq, ptr, n_out):
            calls.append(("get", seq))
            n_out._obj.value = 0 if ptr is None else 1
            return 0

    class Ctx:
        _lib = Lib()

        def _chk(self, rc):
            assert rc == 0

    class Feats:
        length = 3
        keypoints = np.zeros((3, 2, 1))
        state = np.zeros(3)
        landmarks = np.zeros((3, 3, 1))
        tracks = np.zeros((3, 2, 1))
        poses = np.zeros((3, 4, 4))
        descriptors = np.arange(3 * 361, dtype=np.float64).reshape(3, 361, 1) % 256

    p = Pipeline.__new__(Pipeline)
    p.ctx, p._h, p.tracker, p.cap = Ctx(), None, "harris", 8

    class Cfg:
        n_keypoints = 3
    p.cfg = Cfg()
    p.set_state(0, Feats(), np.eye(4), seq=2)
    assert calls == [("state", 2, 0), ("desc", 2, 3)]
    d = p.get_descriptors(seq=1)
    assert calls[-1] == ("get", 1) and d.shape == (1, 361) and d.dtype == np.float32
    p._h = None                        # (nothing to destroy)
