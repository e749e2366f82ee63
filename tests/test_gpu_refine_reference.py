"""vo_refine_pose / vo_refine_pose_dev (csrc/refine.hip) against the rule of include/vo_hip.h: the 50-digit values of
tests/golden/refine_cases.npz and the float64 definition tests/refine_reference.py, on the case table
tests/refine_cases.py.

Bars (refine_cases.bar): per group of the table, 100 times the distance measured there between the float64 definition,
over 21 point orders, and the 50-digit value (tests/test_refine_reference_host.py), never looser than 1e-8 -- for the
size cases: start cost 1.2e-12, one-step pose 4e-13, final cost 1.6e-11, final pose 1e-8 against the 50-digit end (the
step the rule leaves untaken is part of it) and 9e-13 against the definition's own final pose.  A lost or doubled point
moves a start cost of the size cases by 1e-6 at least.  Every test prints the largest distance it saw."""
import numpy as np
import pytest

import refine_cases as rc
import refine_reference as rr
from vo import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def gpu(ctx, c, max_iter=None, X=None, x=None, mask="case"):
    R, t, it, cost = ctx.refine_pose(c.X if X is None else X, c.x if x is None else x, c.K, c.R0, c.t0,
                                     inlier_mask=c.mask if isinstance(mask, str) else mask,
                                     max_iter=c.max_iter if max_iter is None else max_iter)
    return np.concatenate((R.reshape(9), t)), it, cost


def definition(c, max_iter=None):
    return rr.refine(c.X, c.x, c.K, c.R0, c.t0, c.mask, c.max_iter if max_iter is None else max_iter)


def start12(c):
    return np.concatenate((c.R0.reshape(9), c.t0))


def bits(*values):
    return b"".join(np.ascontiguousarray(v, np.float64).tobytes() for v in values)


def n_active(c):
    return int(rr.active(len(c.X), c.mask).sum())


def test_start_cost_of_every_size_and_mask(ctx):
    """(a) max_iter = 0: the cost is the 50-digit start cost, the pose the start bit for bit."""
    gold, worst = rc.golden(), (0.0, "")
    for c in rc.table():
        if c.group in ("sizes", "masks"):
            pose, it, cost = gpu(ctx, c, max_iter=0)
            d = rc.cost_distance(cost, gold[c.name].cost0, n_active(c))
            worst = max(worst, (d, c.name))
            assert d <= rc.bar("cost0", c.group), (c.name, cost, gold[c.name].cost0)
            assert it == 0 and bits(pose) == bits(start12(c)), c.name
    print("start cost: largest distance %.3g (%s)" % worst)


def test_one_step(ctx):
    """(b) max_iter = 1: the pose is the 50-digit Gauss-Newton step wherever the rule accepts it."""
    gold, worst, n = rc.golden(), (0.0, ""), 0
    for c in rc.table():
        if c.kind in ("solved", "large") and definition(c, 1).iterations == 1:
            pose, it, cost = gpu(ctx, c, max_iter=1)
            d = rc.pose_distance(pose, gold[c.name].step1)
            worst, n = max(worst, (d, c.name)), n + 1
            assert it == 1 and d <= rc.bar("step1", c.group), (c.name, it, d)
    assert n >= 40
    print("one step: largest distance %.3g (%s)" % worst)


def test_final_pose_cost_and_iterations(ctx):
    """(c) the case's max_iter (20 but for the max_iter cases): pose and cost against the 50-digit iteration's end -- the
    minimiser, or where a rejected trial or max_iter ends it -- and, where every decision of the definition is wide, its
    iteration count and its own final pose.  A stop by the 1e-16 clause lies on a valley floor whose consecutive iterates
    are further apart than any bar: there the cost is held to the 50-digit value, the count to the definition's +- 1, and
    the pose to the definition's iterate of the kernel's own count."""
    gold = rc.golden()
    worst = dict(final=(0.0, ""), final_cost=(0.0, ""), final_order=(0.0, ""))
    for c in rc.table():
        if c.kind not in ("solved", "large"):
            continue
        pose, it, cost = gpu(ctx, c)
        ref = definition(c)
        wide = c.name not in rc.narrow_margin_cases()
        assert wide == (ref.min_margin >= rc.DECISION_MARGIN), c.name
        if wide:
            d = rc.pose_distance(pose, np.concatenate((ref.R.reshape(9), ref.t)))
            worst["final_order"] = max(worst["final_order"], (d, c.name))
            assert it == ref.iterations, (c.name, it, ref.iterations, ref.reason)
            assert d <= rc.bar("final_order", c.group), (c.name, d)
        else:       # the count may differ by the one step rounding decides; the pose is the definition's iterate of that count
            assert abs(it - ref.iterations) <= 1, (c.name, it, ref.iterations)
            at = definition(c, max_iter=it)
            if at.iterations == it:
                d = rc.pose_distance(pose, np.concatenate((at.R.reshape(9), at.t)))
                worst["final_order"] = max(worst["final_order"], (d, c.name))
                assert d <= rc.bar("final_order", c.group), (c.name, d)
        if c.kind == "solved":
            g = gold[c.name]
            d = rc.cost_distance(cost, g.final_cost, n_active(c))
            worst["final_cost"] = max(worst["final_cost"], (d, c.name))
            assert d <= rc.bar("final_cost", c.group), (c.name, cost, g.final_cost)
            if ref.reason != rr.COST_CLAUSE:
                d = rc.pose_distance(pose, g.final)
                worst["final"] = max(worst["final"], (d, c.name))
                assert d <= rc.bar("final", c.group), (c.name, d)
    for q, w in worst.items():
        print("%s: largest distance %.3g (%s)" % (q, *w))


def test_invariants_on_every_case(ctx):
    """(d) finite or the start; R orthonormal or R0; the cost does not rise; and the returned cost is the cost of the
    returned pose, recomputed in extended precision -- a rejected trial leaking into either output fails this."""
    worst = (0.0, "")
    for c in rc.table():
        pose, it, cost = gpu(ctx, c)
        _, _, cost0 = gpu(ctx, c, max_iter=0)
        same = bits(pose) == bits(start12(c))
        assert same or (np.isfinite(pose).all() and np.isfinite(cost)), c.name
        assert same or it >= 1, c.name
        R = pose[:9].reshape(3, 3)
        assert same or np.abs(R @ R.T - np.eye(3)).max() <= 1e-12, c.name
        assert cost <= cost0 or (same and bits(cost) == bits(cost0)), (c.name, cost, cost0)
        if np.isfinite(cost):
            d = rc.cost_distance(cost, rc.cost_extended(c, R, pose[9:]), n_active(c))
            worst = max(worst, (d, c.name))
            assert d <= rc.bar("final_cost", c.group), (c.name, d)
    print("returned cost against the cost of the returned pose: largest distance %.3g (%s)" % worst)


def test_pose_stays_where_the_rule_says_so(ctx):
    """(e) fewer than three active points, the all-off mask, N = 0, a start cost that is not finite, and a first pivot
    that is exactly zero: the start pose bit for bit, no iterations, the start's cost."""
    gold, n = rc.golden(), 0
    for c in rc.table():
        if c.kind == "unchanged":
            pose, it, cost = gpu(ctx, c)
            assert it == 0 and bits(pose) == bits(start12(c)), (c.name, it)
            assert rc.cost_distance(cost, gold[c.name].cost0, n_active(c)) <= rc.bar("cost0", c.group), (c.name, cost)
            n += 1
    assert n >= 17
    assert gold["geom_pz_zero_at_start"].cost0 == np.inf and gold["mask_on0_seed0"].cost0 == 0.0
    c = rc.by_name("size_6")
    pose, it, cost = gpu(ctx, c, X=np.zeros((0, 3)), x=np.zeros((0, 2)))
    assert it == 0 and bits(pose) == bits(start12(c)) and bits(cost) == bits(0.0)
    for k in (1, 2):                 # unmasked, too
        pose, it, cost = gpu(ctx, c, X=c.X[:k], x=c.x[:k])
        assert it == 0 and bits(pose) == bits(start12(c))
        assert rc.cost_distance(cost, rr.sums(c.X[:k], c.x[:k], c.K, c.R0, c.t0)[2], k) <= rc.bar("cost0", c.group)


def test_masked_off_points_cannot_leak(ctx):
    """(f) NaN, +-1e300 and +-inf under the off bytes change no bit of any output; every non-zero byte means the same."""
    for name in ("mask_bytes_60pct_n300", "mask_bytes_60pct_n2500", "mask_only_past_2048_n2600", "mask_last_plus_two_n2100",
                 "mask_on0_seed0", "mask_on1_seed0", "mask_on2_seed0", "mask_on3_seed0", "mask_bytes_60pct_n10000"):
        c = rc.by_name(name)
        for max_iter in (0, 20):
            want = bits(*gpu(ctx, c, max_iter=max_iter))
            off = c.mask == 0
            for poison in (np.nan, 1e300, -1e300, np.inf, -np.inf):
                X, x = c.X.copy(), c.x.copy()
                X[off], x[off] = poison, poison
                assert bits(*gpu(ctx, c, max_iter=max_iter, X=X, x=x)) == want, (name, poison)
                X, x = c.X.copy(), c.x.copy()
                X[off, 2], x[off, 0] = poison, -poison          # one coordinate only
                assert bits(*gpu(ctx, c, max_iter=max_iter, X=X, x=x)) == want, (name, poison)
            for byte in (1, 2, 255):
                m = np.where(off, 0, byte).astype(np.uint8)
                assert bits(*gpu(ctx, c, max_iter=max_iter, mask=m)) == want, (name, byte)
            on = np.flatnonzero(~off)              # and the mask means what leaving the points out means, to the bars
            if max_iter == 0 and len(on):
                _, _, cost = gpu(ctx, c, max_iter=0, X=c.X[on], x=c.x[on], mask=None)
                assert rc.cost_distance(cost, rc.golden()[name].cost0, len(on)) <= rc.bar("cost0", c.group)


def dev_call(ctx, c, max_iter):
    d_X, d_x, d_Rt = ctx.to_device(c.X), ctx.to_device(c.x), ctx.to_device(start12(c))
    d_m = None if c.mask is None else ctx.to_device(c.mask)
    d_out = ctx.to_device(np.full(16, -7.0))
    try:
        ctx.refine_pose_dev(d_X, d_x, len(c.X), c.K, d_m, d_Rt, max_iter, d_out)
        ctx.sync()
        out = ctx.download(d_out, (16,), np.float64)
    finally:
        for p in (d_X, d_x, d_Rt, d_out) + (() if d_m is None else (d_m,)):
            ctx.free(p)
    assert bits(out[14:]) == bits(np.full(2, -7.0)), "14 doubles are written"
    return out[:12], int(out[12]), out[13]


def test_repeatable_bit_for_bit(ctx):
    """(g) the same call twice; the host-pointer form against the _dev form; a small call after the 10000-point masked one
    on the same context against a fresh context; a permuted point order stays within the bars."""
    gold = rc.golden()
    for name in ("size_65", "size_2049", "mask_bytes_60pct_n2500", "rot_first_step_0.8", "stop_rejected_c", "mask_on2_seed3"):
        c = rc.by_name(name)
        first = gpu(ctx, c)
        assert bits(*gpu(ctx, c)) == bits(*first), name
        pose, it, cost = dev_call(ctx, c, c.max_iter)
        assert bits(pose, it, cost) == bits(*first), name
    small, big = rc.by_name("size_63"), rc.by_name("mask_bytes_60pct_n10000")
    gpu(ctx, big)
    after = gpu(ctx, small)
    fresh = _native.Context(0)
    try:
        assert bits(*gpu(fresh, small)) == bits(*after)
    finally:
        fresh.close()
    rng = np.random.default_rng(5)
    for name in ("size_2561", "mask_bytes_60pct_n2500", "size_513"):
        c = rc.by_name(name)
        perm = rng.permutation(len(c.X))
        mask = None if c.mask is None else c.mask[perm]
        _, it0, cost0 = gpu(ctx, c, max_iter=0, X=c.X[perm], x=c.x[perm], mask=mask)
        assert rc.cost_distance(cost0, gold[name].cost0, n_active(c)) <= rc.bar("cost0", c.group)
        pose, it, cost = gpu(ctx, c, X=c.X[perm], x=c.x[perm], mask=mask)
        assert rc.pose_distance(pose, gold[name].final) <= rc.bar("final", c.group) and it == gpu(ctx, c)[1]
        assert rc.cost_distance(cost, gold[name].final_cost, n_active(c)) <= rc.bar("final_cost", c.group)


def test_refusals_leave_the_context_usable(ctx):
    """(h) max_iter of 101 and of -1, fx == 0 and fy == 0 are refused; the next call computes what it did before."""
    c = rc.by_name("size_64")
    want = bits(*gpu(ctx, c))
    for max_iter in (101, -1):
        with pytest.raises(_native.VoError):
            gpu(ctx, c, max_iter=max_iter)
        assert bits(*gpu(ctx, c)) == want
    for entry in ((0, 0), (1, 1)):
        K = c.K.copy()
        K[entry] = 0.0
        with pytest.raises(_native.VoError):
            ctx.refine_pose(c.X, c.x, K, c.R0, c.t0)
        assert bits(*gpu(ctx, c)) == want
