"""CPU: the C ABI of batched SIFT (vo_sift_batch_dev / vo_sift_batch) -- declared in include/vo_hip.h, exported by the
built library, bound in vo/_native.py with the argument types of the declaration -- and Context.sift_batch's refusal of
images of different shapes before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vo_hip.h")
SYMBOLS = {
    "vo_sift_batch_dev": "int vo_sift_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, "
                         "int cap, float* d_kp, size_t kp_stride, float* d_desc, uint8_t* d_desc_u8, size_t desc_stride, "
                         "int32_t* d_n, int32_t* d_over);",
    "vo_sift_batch": "int vo_sift_batch(vo_ctx* ctx, const uint8_t* imgs, int S, int H, int W, int cap, float* kp, "
                     "float* desc, int32_t* n);",
}
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
ARGS = {
    "vo_sift_batch_dev": [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _sz, _vp, _vp],
    "vo_sift_batch": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
}


def _declaration(text, name):
    """The declaration of `name` in the header with comments removed and whitespace squashed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"int\s+%s\s*\([^;]*\)\s*;" % name, text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(0)).replace("( ", "(").replace(" )", ")").replace(" ,", ",").strip()


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_declared_in_the_header(name):
    assert _declaration(open(HEADER).read(), name) == SYMBOLS[name]


def test_header_cites_the_reference_call_site():
    text = open(HEADER).read()
    i = text.index("int vo_sift_batch_dev(")
    assert "src/vo/features/sift.py:10,17" in text[max(0, i - 1500):i]


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
    assert res is C.c_int and args == ARGS[name]
    lib = _native.load()
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGS[name]


class _StubLib:
    """Records every call; answers vo_sift_capacity and vo_sift_batch like the library would for no keypoints."""

    def __init__(self):
        self.calls = []

    def vo_sift_capacity(self, H, W):
        self.calls.append("vo_sift_capacity")
        return 65536

    def vo_sift_batch(self, h, imgs, S, H, W, cap, kp, desc, n):
        self.calls.append(("vo_sift_batch", S, H, W, cap))
        return 0


def _stub_context():
    from vo import _native
    ctx = _native.Context.__new__(_native.Context)
    ctx._lib, ctx._h = _StubLib(), None
    return ctx


@pytest.mark.parametrize("images", [
    [np.zeros((32, 40), np.uint8), np.zeros((32, 41), np.uint8)],
    [np.zeros((32, 40), np.uint8), np.zeros((33, 40), np.uint8), np.zeros((32, 40), np.uint8)],
    [np.zeros((32, 40), np.uint8), np.zeros((32, 40, 1), np.uint8)],
    [],
])
def test_sift_batch_refuses_mixed_shapes_before_any_library_call(images):
    ctx = _stub_context()
    with pytest.raises(ValueError):
        ctx.sift_batch(images, cap=100)
    assert ctx._lib.calls == []


def test_sift_batch_passes_the_batch_in_one_call():
    ctx = _stub_context()
    out = ctx.sift_batch(np.zeros((3, 32, 40), np.uint8), cap=50)
    assert ctx._lib.calls == [("vo_sift_batch", 3, 32, 40, 50)]
    assert len(out) == 3 and all(k.shape == (0, 6) and d.shape == (0, 128) for k, d in out)
    ctx = _stub_context()
    out = ctx.sift_batch([np.zeros((32, 40), np.uint8)] * 2)
    assert ctx._lib.calls == ["vo_sift_capacity", ("vo_sift_batch", 2, 32, 40, 0)] and len(out) == 2
