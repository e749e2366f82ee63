"""CPU: the C ABI of uncapped device SIFT (vo_sift_all_batch_dev) -- declared in include/vo_hip.h with the reference's call
site, exported by the built library, bound in vo/_native.py with the argument types of the declaration -- and the
pipeline configuration's documented sift_cap = -1."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vo_hip.h")
NAME = "vo_sift_all_batch_dev"
DECL = ("int vo_sift_all_batch_dev(vo_ctx* ctx, const uint8_t* d_imgs, size_t img_stride, int S, int H, int W, int rows, "
        "float* d_kp, size_t kp_stride, float* d_desc, uint8_t* d_desc_u8, size_t desc_stride, int32_t* d_n, "
        "int32_t* d_over);")
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
ARGS = [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _sz, _vp, _vp]


def _declaration(text, name):
    """The declaration of `name` in the header with comments removed and whitespace squashed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"int\s+%s\s*\([^;]*\)\s*;" % name, text)
    assert m, name
    return re.sub(r"\s+", " ", m.group(0)).replace("( ", "(").replace(" )", ")").replace(" ,", ",").strip()


def test_declared_in_the_header():
    assert _declaration(open(HEADER).read(), NAME) == DECL


def test_header_cites_the_reference_call_site():
    text = open(HEADER).read()
    i = text.index("int %s(" % NAME)
    comment = text[text.rindex("/*", 0, i):i]
    assert "src/vo/features/sift.py:10,17" in comment


def test_sift_cap_minus_one_is_documented():
    text = open(HEADER).read()
    i = text.index("int32_t sift_cap;")
    assert "-1 = every keypoint" in text[i:i + 600]


def test_exported_by_the_library():
    from vo import _native
    path = _native.lib_path()
    if not os.path.exists(path):
        pytest.fail("libvo_hip.so is not built: %s" % path)
    lib = C.CDLL(path)
    assert getattr(lib, NAME, None) is not None       # (dlsym: the dynamic symbol table has it)


def test_bound_with_the_declared_argument_types():
    from vo import _native
    res, args = _native._SIGS[NAME]
    assert res is C.c_int and args == ARGS
    fn = getattr(_native.load(), NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGS


class _StubLib:
    """Records the call of vo_sift_all_batch_dev and answers VO_OK."""

    def __init__(self):
        self.calls = []

    def vo_sift_all_batch_dev(self, *a):
        self.calls.append(a)
        return 0


def test_context_method_passes_every_argument_through():
    from vo import _native
    ctx = _native.Context.__new__(_native.Context)      # (no device: the library is a stub)
    ctx._lib, ctx._h = _StubLib(), C.c_void_p(7)
    ctx.sift_all_batch_dev(1000, 5000, 3, 40, 50, 700, 2000, 710, 3000, None, 705, 4000, d_over=None)
    (a,) = ctx._lib.calls
    assert a[0] is ctx._h
    assert [x.value if isinstance(x, C.c_void_p) else x for x in a[1:]] == [1000, 5000, 3, 40, 50, 700, 2000, 710, 3000,
                                                                            None, 705, 4000, None]
