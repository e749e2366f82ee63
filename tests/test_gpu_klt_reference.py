"""-m gpu: the Lucas-Kanade kernels of csrc/klt.hip (klt_track16_kernel<15,16>, <17,32>, <21,32> and the generic
klt_track_kernel<0>) and the pyramid builders of csrc/pyramid.hip against the float64 definition of tests/klt_reference.py, directly, on every
case of tests/klt_cases.py -- and, separately, against the oracle bit for bit.  tests/test_klt_reference_host.py runs the same
checks on the oracle and asserts each case's edge and the 10 % cap."""
import os
import subprocess
import sys

import numpy as np
import pytest

import klt_cases as kc
import klt_reference as ref
from oracle import native
from test_gpu_geometry import run_pyramid_case

pytestmark = pytest.mark.gpu
PYRAMID_SHAPES = [(20, 24), (24, 32), (32, 32), (33, 34), (96, 128), (132, 136)]
MAX_LEVELS = 8          # what vo_pyramid_build_dev accepts


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("shape", kc.PYR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pyr_down_kernel_equals_definition(ctx, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for img in (rng.integers(0, 256, size=shape).astype(np.uint8), np.full(shape, 255, np.uint8)):
        assert np.array_equal(ctx.pyr_down(img), ref.pyr_down(img))


@pytest.mark.parametrize("shape", PYRAMID_SHAPES, ids=lambda s: "%dx%d" % s)
def test_bordered_pyramid_equals_definition(ctx, shape):
    """Every level count the builder accepts, down to levels of 1 x 1: two levels and fewer go through the per-level kernels,
    three and more through the one-launch builder when level 2 has both sides > 32 (132 x 136: 33 x 34), else not (96 x 128:
    24 x 32); the 32-pixel border of a level with a side <= 32 mirrors more than once."""
    for levels in range(1, MAX_LEVELS + 1):
        run_pyramid_case(ctx, shape, levels)


def test_bordered_pyramid_large_tiles_equals_definition():
    """The same shapes through the 64x32-tile variant (VO_PYR_TILE is read once per process: own process)."""
    code = ("import sys; sys.path[:0] = %r; import test_gpu_geometry as t; from vo import _native; c = _native.Context(0); "
            "[t.run_pyramid_case(c, s, n) for s in %r for n in range(1, %d)]; c.close(); print('ok')"
            % ([p for p in sys.path if p], PYRAMID_SHAPES, MAX_LEVELS + 1))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VO_PYR_TILE="64"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("name", kc.NAMES)
def test_kernel_equals_oracle(ctx, name):
    c = kc.BY_NAME[name]
    for args in (kc.case_args(c), kc.one_step_args(c)):
        ro, rs, re = native.klt_track(c.prev, c.nxt, c.pts, **args)
        go, gs, ge = ctx.klt_track(c.prev, c.nxt, c.pts, **args)
        assert np.array_equal(gs, rs), "status flags differ"
        assert np.array_equal(go, ro), "tracked points not bit-identical to the oracle"
        assert np.array_equal(ge, re), "error measures not bit-identical"


@pytest.mark.parametrize("name", kc.NAMES)
def test_kernel_one_step_matches_definition(ctx, name):
    """max_level 0, max_iter 1, eps 0: out - pts is one Newton step, within twice the quantisation bound per point."""
    c = kc.BY_NAME[name]
    fig = {}
    try:
        kc.check(name, *ctx.klt_track(c.prev, c.nxt, c.pts, **kc.one_step_args(c)), one_step=True, figures=fig)
    finally:
        print("one-step", name, c.win, fig)


@pytest.mark.parametrize("name", kc.NAMES)
def test_kernel_matches_definition(ctx, name):
    """The case as it stands: the fixed point within eps + twice the bound, the one-step chain through the pyramid, or
    max_iter 0; status at every decided point; err at the returned point."""
    c = kc.BY_NAME[name]
    fig = {}
    try:
        kc.check(name, *ctx.klt_track(c.prev, c.nxt, c.pts, **kc.case_args(c)), figures=fig)
    finally:
        print(kc.mode_of(c), name, c.win, fig)
