"""-m gpu: the forward-backward variants of the Lucas-Kanade kernels (csrc/klt.hip: klt_track16_kernel<15,16,true>,
<17,32,true>, <21,32,true> and klt_track_kernel<0,true>) against the rule of include/vo_hip.h ("pyramidal KLT",
vo_klt_track_fb) as tests/klt_fb_oracle.py composes it from the unchanged tracker oracle: bit for bit, on every case of
tests/klt_fb_cases.py and on every case of tests/klt_cases.py at fb_max = 1."""
import numpy as np
import pytest

import klt_cases as kc
import klt_fb_cases as fc
import klt_fb_oracle as fbo
from oracle import native

pytestmark = pytest.mark.gpu

ALL = [(c.name, c) for c in fc.CASES] + [("klt:" + c.name, fc.from_klt_case(c, 1.0)) for c in kc.CASES]
IDS = [n for n, _ in ALL]
BY_ID = dict(ALL)
# the device-pointer form, the composition and the repeat: every new case, and one klt_cases case per kernel and builder
SUBSET = [n for n in IDS if not n.startswith("klt:")] + ["klt:win15_dots", "klt:win17_smooth", "klt:win21_dots", "klt:win9_dots",
                                                         "klt:win31_dots", "klt:tiled_132x136_win17_dots",
                                                         "klt:odd_97x131_win15_dots", "klt:tiny_20x24_win21_dots"]


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


def assert_bits(got, want, what):
    (go, gs, ge, gf), (wo, ws, we, wf) = got, want
    assert np.array_equal(gs, ws), "%s: status differs at %s" % (what, np.flatnonzero(gs != ws)[:10])
    assert np.array_equal(go.view(np.uint32), wo.view(np.uint32)), "%s: next_xy not bit-identical" % what
    assert np.array_equal(ge.view(np.uint32), we.view(np.uint32)), "%s: err not bit-identical" % what
    assert np.array_equal(gf.view(np.uint32), wf.view(np.uint32)), "%s: fb not bit-identical at %s" % (
        what, np.flatnonzero(gf.view(np.uint32) != wf.view(np.uint32))[:10])


def run_fb(ctx, c):
    return ctx.klt_track_fb(c.prev, c.nxt, c.pts, fb_max=c.fb_max, **fc.case_args(c))


@pytest.mark.parametrize("name", IDS)
def test_fb_kernel_equals_rule(ctx, name):
    c = BY_ID[name]
    assert_bits(run_fb(ctx, c), fc.expected(c), name)


def run_fb_dev(ctx, c):
    """vo_klt_track_fb_dev on pyramids built by vo_pyramid_build_dev."""
    H, W = c.prev.shape
    n = len(c.pts)
    nl = ctx.klt_num_levels(H, W, c.win, c.max_level)
    nbytes = ctx.pyramid_bytes(H, W, nl)
    bufs = dict(prev=ctx.to_device(np.ascontiguousarray(c.prev)), nxt=ctx.to_device(np.ascontiguousarray(c.nxt)),
                pp=ctx.to_device(np.zeros(nbytes, np.uint8)), pn=ctx.to_device(np.zeros(nbytes, np.uint8)),
                xy=ctx.to_device(np.ascontiguousarray(c.pts)), out=ctx.to_device(np.zeros((n, 2), np.float32)),
                st=ctx.to_device(np.zeros(n, np.uint8)), err=ctx.to_device(np.zeros(n, np.float32)),
                fb=ctx.to_device(np.zeros(n, np.float32)))
    try:
        ctx.pyramid_build_dev(bufs["prev"], H, W, nl, bufs["pp"])
        ctx.pyramid_build_dev(bufs["nxt"], H, W, nl, bufs["pn"])
        ctx.klt_track_fb_dev(bufs["prev"], bufs["pp"], bufs["nxt"], bufs["pn"], H, W, nl, bufs["xy"], n, c.win, c.max_iter, c.eps,
                             c.min_eig, c.fb_max, bufs["out"], bufs["st"], bufs["err"], bufs["fb"])
        ctx.sync()
        return (ctx.download(bufs["out"], (n, 2), np.float32), ctx.download(bufs["st"], (n,), np.uint8),
                ctx.download(bufs["err"], (n,), np.float32), ctx.download(bufs["fb"], (n,), np.float32))
    finally:
        for b in bufs.values():
            ctx.free(b)


@pytest.mark.parametrize("name", SUBSET)
def test_fb_dev_form_equals_rule(ctx, name):
    c = BY_ID[name]
    assert_bits(run_fb_dev(ctx, c), fc.expected(c), name + " (_dev)")


@pytest.mark.parametrize("name", SUBSET)
def test_fb_equals_two_plain_calls_and_is_repeatable(ctx, name):
    """The fused launch against the kernels' own two vo_klt_track calls plus the NumPy compare, and a second run."""
    c = BY_ID[name]
    got = run_fb(ctx, c)
    composed = fbo.fb_track(c.prev, c.nxt, c.pts, fb_max=c.fb_max, track=ctx.klt_track, **fc.case_args(c))
    assert_bits(got, composed, name + " (two vo_klt_track calls)")
    assert_bits(run_fb(ctx, c), got, name + " (second run)")


@pytest.mark.parametrize("name", SUBSET)
def test_plain_tracker_still_equals_oracle(ctx, name):
    """The plain instantiations share the templates with the forward-backward ones: same inputs, plain call, oracle."""
    c = BY_ID[name]
    ro, rs, re = native.klt_track(c.prev, c.nxt, c.pts, **fc.case_args(c))
    go, gs, ge = ctx.klt_track(c.prev, c.nxt, c.pts, **fc.case_args(c))
    assert np.array_equal(gs, rs) and np.array_equal(go.view(np.uint32), ro.view(np.uint32))
    assert np.array_equal(ge.view(np.uint32), re.view(np.uint32))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("-inf")], ids=["zero", "negative", "nan", "minus_inf"])
def test_bad_fb_max_is_refused_and_writes_nothing(ctx, bad):
    from vo import _native
    c = fc.BY_NAME["fb_win15_n7"]
    lib, n = ctx._lib, len(c.pts)
    H, W = c.prev.shape
    prev, nxt, pts = (np.ascontiguousarray(a) for a in (c.prev, c.nxt, c.pts))
    out, st, err, fb = (np.full((n, 2), 7.5, np.float32), np.full(n, 9, np.uint8), np.full(n, 7.5, np.float32),
                        np.full(n, 7.5, np.float32))
    rc = lib.vo_klt_track_fb(ctx._h, _native._ptr(prev), _native._ptr(nxt), H, W, _native._ptr(pts), n, c.win, c.max_level,
                             c.max_iter, c.eps, c.min_eig, bad, _native._ptr(out), _native._ptr(st), _native._ptr(err),
                             _native._ptr(fb))
    assert rc != 0
    with pytest.raises(Exception, match="fb_max"):
        ctx._chk(rc)
    assert np.all(out == 7.5) and np.all(st == 9) and np.all(err == 7.5) and np.all(fb == 7.5)
    with pytest.raises(Exception, match="fb_max"):
        ctx.klt_track_fb(c.prev, c.nxt, c.pts, fb_max=bad, **fc.case_args(c))
    # the device form: refused before a launch
    d = ctx.to_device(np.full(n, 7.5, np.float32))
    try:
        with pytest.raises(Exception, match="fb_max"):
            ctx.klt_track_fb_dev(d, d, d, d, H, W, 1, d, n, c.win, c.max_iter, c.eps, c.min_eig, bad, d, d, d, d)
        ctx.sync()
        assert np.all(ctx.download(d, (n,), np.float32) == 7.5)
    finally:
        ctx.free(d)
