"""-m gpu: the SIFT kernels of csrc/sift.hip (through Context.sift) against the float64 definition of
tests/sift_reference.py, directly and not via the oracle, on every case of tests/sift_cases.py the kernels accept (H, W >= 16):
the end-to-end keypoint-set comparison with the tolerances of the host tests, the blob and orientation ground truths,
transposition, and capped runs against the definition's cap rule.  One case goes through sift_batch and one through
sift_all_batch_dev, which the other suites pin to vo_sift bit for bit.  tests/test_sift_reference_host.py runs the same
checks on the oracle, and the oracle's stages one by one."""
import numpy as np
import pytest

import sift_cases as sc
from test_gpu_sift_all import _AllBatch
from test_sift_reference_host import TRANSPOSED, check_blob, check_orientation, check_transposition

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sc.GPU_NAMES)
def test_kernel_rows_match_definition(ctx, name):
    c = sc.BY_NAME[name]
    kp, desc = ctx.sift(c.img)
    fig = {}
    try:
        sc.check_rows(sc.definition(name), kp, desc, fig, name)
    finally:
        print(name, {k: round(float(v), 3) for k, v in fig.items()})


@pytest.mark.parametrize("name", ["twins64x128", "checker48x48", "blocks64x64", "smallest16x16"])
def test_capped_runs_follow_the_definitions_cap_rule(ctx, name):
    """cap = 1, a cap inside a run of tied responses (the twin patterns and the checker have them) and a cap above the
    count, against the rule applied to the kernels' own uncapped rows."""
    c = sc.BY_NAME[name]
    kp, _ = ctx.sift(c.img)
    tied = sc.tied_cap(kp)
    if name in ("twins64x128", "checker48x48"):
        assert tied is not None, "no tied responses"
    for cap in sorted({1, tied or 2, len(kp) + 3}):
        sc.check_cap(kp, ctx.sift(c.img, cap=cap)[0], cap)


@pytest.mark.parametrize("blob", sc.BLOBS, ids=lambda b: "s%g@%g,%g" % (b[4], b[2], b[3]))
def test_blob_position_bias_and_size(ctx, blob):
    fig = {}
    check_blob(blob, ctx.sift(sc.image_of(("blob",) + blob))[0], fig)
    print(fig)


@pytest.mark.parametrize("phi", sc.ORIENTATIONS)
def test_orientation_is_clockwise_on_screen_from_x(ctx, phi):
    print(phi, check_orientation(phi, ctx.sift(sc.image_of(("ori", phi)))[0]))


@pytest.mark.parametrize("name", [n for n in TRANSPOSED if sc.BY_NAME[n].gpu])
def test_transposition(ctx, name):
    n = check_transposition(name, *ctx.sift(sc.BY_NAME[name].img), *ctx.sift(sc.image_of(("T", name))))
    assert n >= 3


def test_sift_batch_matches_definition(ctx):
    names = ["blocks64x64", "borders64x64"]
    for name, (kp, desc) in zip(names, ctx.sift_batch([sc.BY_NAME[n].img for n in names])):
        sc.check_rows(sc.definition(name), kp, desc, None, "sift_batch " + name)


def test_sift_all_batch_dev_matches_definition(ctx):
    names = ["blobs51x77"]
    b = _AllBatch(ctx, [sc.BY_NAME[n].img for n in names], 256, pad_img=3, pad_kp=1, pad_desc=2)
    try:
        b.run()
        kp, df, db, n, ov = b.read()
        for q, name in enumerate(names):
            assert ov[q] == 0
            sc.check_rows(sc.definition(name), kp[q, :n[q]], df[q, :n[q]], None, "sift_all_batch_dev " + name)
            assert np.array_equal(db[q, :n[q]], df[q, :n[q]].astype(np.uint8))
    finally:
        b.free()
