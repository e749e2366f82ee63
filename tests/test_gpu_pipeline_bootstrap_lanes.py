"""-m gpu: the 8-point RANSAC loop on the device (vo_rng_raw32_device, vo_fundamental_ransac) against NumPy's stream and
against the route composed from vo_rng_choice + vo_fundamental_hypotheses + vo_ransac_replay + vo_fundamental_fit, and
several lanes per bootstrap call (vo_pipeline_bootstrap_lanes) against the one-lane call lane by lane.  The same kernels
run either way, so results are compared exactly.

The file's name puts it behind tests/test_gpu_lanes.py and tests/test_gpu_pipeline.py on purpose.  Observed, cause not
established: with this file collected in front of them, test_per_lane_camera_equals_single_pipelines[True-0] (look-ahead
with prepare hints) differed at one step (lane 2, step 4: 519 features tracked against 528) in two runs of the whole suite,
while this file and that one alone, in that order, passed, as did every pairing with one more file.  Suspected: DESIGN.md 6,
item 6 -- a step finished by the host path under a hint re-tracks from the hinted frame's pyramid, and whether a step
needs the host path under look-ahead depends on the timing of the detector's decision, which the pipelines created
earlier in the process shift."""
import numpy as np
import pytest

from test_bootstrap_sampler_host import marked_draws, numpy_choice_model, raw_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo import _native
    c = _native.Context(0)
    yield c
    c.close()


# ---- 3. the fill kernel against NumPy's stream ----

@pytest.mark.parametrize("seed", [2023, 1, 7, 123456789])
@pytest.mark.parametrize("count", [30720, 4097, 1])
@pytest.mark.parametrize("buffered", [False, True])
def test_fill_kernel_equals_numpy_stream(ctx, seed, count, buffered):
    from vo import _native
    gen = np.random.Generator(np.random.PCG64(seed))
    if buffered:
        gen.integers(0, 10)                       # leaves the high half of an output buffered
        assert gen.bit_generator.state["has_uint32"] == 1
    state = gen.bit_generator.state
    pcg = _native.Pcg64.from_generator(gen)
    got = ctx.rng_raw32_device(pcg, count)
    # NumPy's own words: the buffered half, then every 64-bit output low half, high half
    twin = np.random.PCG64()
    twin.state = state
    raws = twin.random_raw(count // 2 + 2)
    words = np.empty(2 * raws.size, np.uint32)
    words[0::2] = (raws & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    words[1::2] = (raws >> np.uint64(32)).astype(np.uint32)
    if buffered:
        words = np.concatenate([[np.uint32(state["uinteger"])], words])
    assert np.array_equal(got, words[:count])
    # the state handed back: NumPy's after the same number of 32-bit draws
    for _ in range(count):
        gen.bit_generator.ctypes.next_uint32(gen.bit_generator.ctypes.state)
    after = np.random.default_rng(0)
    pcg.to_generator(after)
    a, b = after.bit_generator.state, gen.bit_generator.state
    assert a["state"] == b["state"] and a["has_uint32"] == b["has_uint32"]
    assert a["has_uint32"] == 0 or a["uinteger"] == b["uinteger"]
    # ... and the next words of both agree
    assert np.array_equal(ctx.rng_raw32_device(pcg, 5),
                          [gen.bit_generator.ctypes.next_uint32(gen.bit_generator.ctypes.state) for _ in range(5)])


# ---- 4. the loop against the composed route ----

def two_views(n, inlier_fraction, seed):
    """n correspondences of a synthetic two-view geometry in pixels; all but inlier_fraction of them scattered."""
    rng = np.random.default_rng(seed)
    K = np.array([[700.0, 0, 320.0], [0, 700.0, 240.0], [0, 0, 1.0]])
    X = rng.uniform([-4, -3, 4], [4, 3, 12], (n, 3))
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.5, 0.05, 0.1])

    def project(P):
        p = P @ K.T
        return p[:, :2] / p[:, 2:]
    p1, p2 = project(X), project(X @ R.T + t)
    p2 += rng.normal(0, 0.05, p2.shape)
    out = rng.random(n) >= inlier_fraction
    p2[out] = rng.uniform([0, 0], [640, 480], (int(out.sum()), 2))
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2)


def composed_route(ctx, p1, p2, threshold, normalize, kind, gen, max_iterations, outlier_ratio=0.9, confidence=0.999):
    """LandmarksTriangulator._ransac_fundamental with the generator given: (F, inliers, iterations)."""
    from vo.algorithms.ransac import RANSAC
    n = p1.shape[0]
    ransac = RANSAC(s_points=8, population=np.arange(n), model_fn=None, error_fn=None, inlier_threshold=threshold,
                    outlier_ratio=outlier_ratio, confidence=confidence, max_iterations=max_iterations)
    ransac.rng = gen

    def batch_fn(samples):
        F, counts, masks = ctx.fundamental_hypotheses(p1, p2, samples, threshold, normalize, kind, want_masks="packed")
        return np.ones(len(samples), np.uint8), counts, lambda b: (F[b], ctx.unpack_mask(masks[b], n))

    _, inliers, iterations = ransac.find_best_model_batched(n, batch_fn, batch_size=2048)
    return ctx.fundamental_fit(p1, p2, inliers, normalize=normalize), inliers, iterations


def both_routes(ctx, p1, p2, threshold, normalize, kind, seed, max_iterations):
    ref_gen, gen = np.random.default_rng(seed), np.random.default_rng(seed)
    F_ref, inl_ref, it_ref = composed_route(ctx, p1, p2, threshold, normalize, kind, ref_gen, max_iterations)
    F, inl, info = ctx.fundamental_ransac(p1, p2, threshold, gen, normalize_samples=normalize, error_kind=kind,
                                          max_iterations=max_iterations)
    print("N %d kind %d budget %s: %d iterations, %d inliers, finished_by_host %d" % (
        p1.shape[0], kind, max_iterations, info["iterations"], info["best_count"], info["finished_by_host"]))
    assert np.array_equal(inl, inl_ref)
    assert info["iterations"] == it_ref and info["best_count"] == int(inl_ref.sum())
    assert np.array_equal(F, F_ref)
    assert gen.bit_generator.state == ref_gen.bit_generator.state
    return info, it_ref


KINDS = [(True, 1, 1.0), (False, 0, None)]         # (normalise every sample, error kind, threshold)


def scaled(p1, p2, normalize, thr):
    if normalize:
        return p1, p2, thr
    c = np.array([320.0, 240.0])                    # the algebraic error on points of order 1
    return (p1 - c) / 400.0, (p2 - c) / 400.0, 1e-5


@pytest.mark.parametrize("normalize,kind,thr", KINDS, ids=["epipolar", "algebraic"])
@pytest.mark.parametrize("n", [9, 200, 2000])
def test_loop_equals_the_composed_route(ctx, n, normalize, kind, thr):
    p1, p2, thr = scaled(*two_views(n, 1.0 if n == 9 else 0.6, 100 + n), normalize, thr)
    info, _ = both_routes(ctx, p1, p2, thr, normalize, kind, 2023 if n != 200 else 7, 2000)
    marks = marked_draws(raw_words(2023 if n != 200 else 7, 15 * 2048), n, 2048).any(axis=1)
    assert info["finished_by_host"] == int(marks[:info["iterations"]].any())


def test_a_budget_of_several_batches(ctx):
    """10 000 iterations on data with so few inliers that the bound never falls below the budget: over five batches."""
    p1, p2 = two_views(600, 0.12, 5)
    info, it_ref = both_routes(ctx, p1, p2, 0.05, True, 1, 11, 10000)
    assert it_ref > 4 * 2048, "the case is not what it claims: the loop ended after %d iterations" % it_ref
    marks = marked_draws(raw_words(11, 15 * it_ref), 600, it_ref).any(axis=1)
    assert info["finished_by_host"] == int(marks.any())


def test_eight_correspondences_go_to_the_host_sampler(ctx):
    p1, p2 = two_views(8, 1.0, 3)
    info, _ = both_routes(ctx, p1, p2, 1.0, True, 1, 2023, 2000)
    assert info["finished_by_host"] == 1


def test_unbounded_budget_goes_to_the_host_sampler(ctx):
    p1, p2 = two_views(300, 0.7, 4)
    info, _ = both_routes(ctx, p1, p2, 1.0, True, 1, 2023, np.inf)
    assert info["finished_by_host"] == 1


@pytest.mark.parametrize("n,mark,rejected", [(3922, 18, True), (2215, 801, True), (2911, 412, False)])
def test_marked_draw_inside_the_consumed_prefix(ctx, n, mark, rejected):
    """default_rng(2023) on low-inlier data (the whole budget consumed): the marked sample is inside the prefix, the host
    sampler finishes the loop, the results are the composed route's."""
    p1, p2 = two_views(n, 0.12, 9)
    info, it_ref = both_routes(ctx, p1, p2, 0.05, True, 1, 2023, 2000)
    marks = np.flatnonzero(marked_draws(raw_words(2023, 15 * 2048), n, 2048).any(axis=1))
    assert marks[0] == mark
    words, pos = raw_words(2023, 15 * (mark + 2)), 15 * mark       # (no mark before it: the stream stands at 15 per sample)
    assert (numpy_choice_model(words, pos, n)[1] - pos != 15) == rejected
    assert it_ref > mark, "the case is not what it claims: the loop ended after %d iterations, the mark is at %d" % (it_ref, mark)
    assert info["finished_by_host"] == 1


def test_marked_draw_behind_the_loops_end(ctx):
    """N = 2215 with so many inliers that the loop ends before sample 801: the device finishes it."""
    p1, p2 = two_views(2215, 0.8, 9)
    info, it_ref = both_routes(ctx, p1, p2, 1.0, True, 1, 2023, 2000)
    assert it_ref <= 801, "the case is not what it claims: the loop ended after %d iterations" % it_ref
    assert info["finished_by_host"] == 0


# ---- 5. - 9. several lanes per bootstrap call ----

from test_gpu_pipeline_bootstrap import (LARGE, SMALL, boot_kwargs, close_records, close_runs, new_pipe, recording,  # noqa: E402
                                         rng_of)

ETRACKING = -5
_DATA = {}


def lane_data(cfg, S, steps=4, first_seed=2023):
    """Per lane: camera, the two bootstrap frames and `steps` following frames of its own recording (two cameras)."""
    from vo import driver, synthetic
    key = (cfg["H"], S, steps, first_seed)
    if key not in _DATA:
        Kb = synthetic.intrinsics(cfg["H"], cfg["W"]).copy()
        Kb[0, 0] *= 0.92
        Kb[1, 1] *= 0.92
        Kb[0, 2] += 6.0
        Kb[1, 2] -= 4.0
        lanes = []
        for q in range(S):
            seq = recording(cfg, first_seed + 7 * q, n_frames=3 + steps, intrinsics=Kb if q % 2 else None)
            img0, img2 = driver._bootstrap_frames(seq)
            rest = [driver._gray(next(seq).image) for _ in range(steps)]
            lanes.append(dict(K=np.asarray(seq.get_camera().intrinsic_matrix, np.float64), img0=img0, img2=img2, rest=rest))
        _DATA[key] = lanes
    return _DATA[key]


def lanes_pipe(ctx, cfg, data):
    """A pipeline of len(data) lanes, every lane with its camera, frame 0 in slot 1 and frame 2 in slot 0."""
    pipe = new_pipe(ctx, cfg, data[0]["K"], sequences=len(data))
    for q, d in enumerate(data):
        pipe.set_camera(d["K"], q)
        pipe.set_frame(1, d["img0"], seq=q)
        pipe.set_frame(0, d["img2"], seq=q)
    return pipe


def boot(pipe, how, groups, a, b, cfg, generators=None):
    """how = "lanes": one bootstrap_lanes call per group; "single": Pipeline.bootstrap lane by lane, in the same order.
    Returns {lane: BootstrapResult} (status set either way)."""
    from vo import _native
    out = {}
    for group in groups:
        gens = None if generators is None else [np.random.default_rng(generators + q) for q in group]
        if how == "lanes":
            for r in pipe.bootstrap_lanes(a, b, list(group), generators=gens, **boot_kwargs(cfg)):
                out[r.seq] = r
        else:
            for k, q in enumerate(group):
                try:
                    out[q] = pipe.bootstrap(a, b, seq=q, generator=None if gens is None else gens[k], **boot_kwargs(cfg))
                except _native.VoError as e:
                    out[q] = _native.BootstrapResult()
                    out[q].status = e.code
    return out


def same_everything(a, b, what):
    """Two get_state() dicts equal in every field (the same kernels ran: the poses too)."""
    assert set(a) == set(b), what
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


RESULT_FIELDS = ("n_corners", "n_tracked", "n_ransac_inliers", "n_landmarks", "n_features", "reserved", "ransac_iterations")


def same_results(a, b, what):
    assert a.status == b.status, (what, a.status, b.status)
    if a.status != 0:
        return
    for name in RESULT_FIELDS:
        assert getattr(a, name) == getattr(b, name), (what, name, getattr(a, name), getattr(b, name))
    assert np.array_equal(a.relative_pose(), b.relative_pose()), what


def step_all(pipe, data, k, a, b, lanes=None):
    """Frame rest[k] of every lane (of `lanes`) into slot b, then one step of the whole pipeline."""
    for q, d in enumerate(data):
        if lanes is None or q in lanes:
            pipe.set_frame(b, d["rest"][k], seq=q)
    pipe.submit(a, b)
    return pipe.collect_all()


def per_lane(records, q):
    return [r[q] for r in records]


GROUPINGS = {"all": lambda S: [tuple(range(S))],
             "subset": lambda S: [(0, 2, 3), tuple(q for q in range(S) if q not in (0, 2, 3))],
             "one": lambda S: [(2,)] + [(q,) for q in range(S) if q != 2]}


@pytest.mark.parametrize("grouping", ["all", "subset", "one"])
@pytest.mark.parametrize("cfg,S", [(SMALL, 4), (SMALL, 16), (LARGE, 4)], ids=["small-4", "small-16", "large-4"])
def test_lanes_equal_the_one_lane_call(ctx, cfg, S, grouping):
    """5. bootstrap_lanes over all lanes / a non-consecutive subset and then the rest / one lane at a time, against
    Pipeline.bootstrap(seq=q) lane by lane on a second pipeline fed the same frames: state, results, generators equal; then
    four steps of both."""
    data = lane_data(cfg, S)
    groups = GROUPINGS[grouping](S)
    generators = 50 if grouping == "all" else None
    runs = []
    for how in ("lanes", "single"):
        pipe = lanes_pipe(ctx, cfg, data)
        res = boot(pipe, how, groups, 1, 0, cfg, generators)
        states = [pipe.get_state(seq=q) for q in range(S)]
        rngs = [rng_of(pipe, q) for q in range(S)]
        recs = [step_all(pipe, data, k, k % 4, (k + 1) % 4) for k in range(4)]
        runs.append((res, states, rngs, recs, [pipe.get_state(seq=q) for q in range(S)], [rng_of(pipe, q) for q in range(S)]))
        pipe.close()
    (res, states, rngs, recs, end, end_rng), (res1, states1, rngs1, recs1, end1, end_rng1) = runs
    for q in range(S):
        assert res[q].status == 0 and res[q].n_landmarks >= 8, (q, res[q].status)
        same_results(res[q], res1[q], ("lane", q))
        same_everything(states[q], states1[q], ("lane", q))
        assert rngs[q] == rngs1[q], q
        close_records(per_lane(recs, q), per_lane(recs1, q), ("lane", q))
        assert end_rng[q] == end_rng1[q], q
        assert end[q]["n"] == end1[q]["n"] and np.array_equal(end[q]["state"], end1[q]["state"])
    print("%s %dx%d, %d lanes: %s" % (grouping, cfg["H"], cfg["W"], S,
                                     ", ".join("%d/%d/%d" % (res[q].n_corners, res[q].n_tracked, res[q].n_landmarks) for q in range(S))))


def restart_scenario(ctx, how, restart_lanes, flat=()):
    """A running 4-lane pipeline: hand-over of all lanes, two steps, then `restart_lanes` go idle, get the two frames of
    another recording (lanes in `flat`: two flat frames) and restart -- in one call or one call each -- while the others go
    on; two more steps.  A lane that failed is then restarted with the state it had and steps on."""
    cfg, S = SMALL, 4
    data, other = lane_data(cfg, S), lane_data(cfg, S, first_seed=2100)
    grey = np.full((cfg["H"], cfg["W"]), 128, np.uint8)
    pipe = lanes_pipe(ctx, cfg, data)
    first = boot(pipe, how, [tuple(range(S))], 1, 0, cfg)
    recs = [step_all(pipe, data, 0, 0, 1), step_all(pipe, data, 1, 1, 2)]
    before = {q: (pipe.get_state(seq=q), rng_of(pipe, q), pipe.get_features(q)) for q in restart_lanes}
    for q in restart_lanes:
        pipe.set_active(q, False)
        pipe.set_camera(other[q]["K"], q)
        pipe.set_frame(3, grey if q in flat else other[q]["img0"], seq=q)
        pipe.set_frame(2, grey if q in flat else other[q]["img2"], seq=q)
    second = boot(pipe, how, [tuple(restart_lanes)], 3, 2, cfg, generators=99)
    after = {q: (pipe.get_state(seq=q), rng_of(pipe, q)) for q in range(S)}
    for q in flat:                       # the failed lane: as it was; it comes back with its own frame and state
        assert second[q].status == ETRACKING, second[q].status
        same_everything(after[q][0], before[q][0], ("failed lane", q))
        assert after[q][1] == before[q][1]
        st = before[q][0]
        pipe.set_camera(data[q]["K"], q)
        pipe.restart(q, 2, before[q][2], st["curr_pose"], st["prev_pose"], num_features=st["num_features"],
                     image=data[q]["rest"][1])
    for k, (a, b) in ((2, (2, 3)), (3, (3, 0))):
        for q in range(S):
            src = other if (q in restart_lanes and q not in flat) else data
            pipe.set_frame(b, src[q]["rest"][k - 2 if src is other else k], seq=q)
        pipe.submit(a, b)
        recs.append(pipe.collect_all())
    end = [(pipe.get_state(seq=q), rng_of(pipe, q)) for q in range(S)]
    return pipe, first, second, recs, after, end


@pytest.mark.parametrize("restart_lanes,flat", [((0, 3), ()), ((0, 2, 3), (2,))], ids=["two-restart", "one-of-three-fails"])
def test_restart_in_one_call_on_a_running_pipeline(ctx, restart_lanes, flat):
    """6. + 7. lanes restarted in one call while the others go on equal the same run with one call per lane; a lane with two
    flat frames among them fails alone (VO_ETRACKING), keeps its state and generator, and can be restarted and stepped."""
    pipe, first, second, recs, after, end = restart_scenario(ctx, "lanes", restart_lanes, flat)
    pipe1, first1, second1, recs1, after1, end1 = restart_scenario(ctx, "single", restart_lanes, flat)
    for q in range(4):
        same_results(first[q], first1[q], ("hand-over", q))
        if q in restart_lanes:
            same_results(second[q], second1[q], ("restart", q))
            assert second[q].status == (ETRACKING if q in flat else 0)
        same_everything(after[q][0], after1[q][0], ("after the restart", q))
        assert after[q][1] == after1[q][1]
        close_records(per_lane(recs, q), per_lane(recs1, q), ("lane", q))
        same_everything(end[q][0], end1[q][0], ("at the end", q))
        assert end[q][1] == end1[q][1]
        assert recs[-1][q].fault == 0 and recs[-1][q].n_tracked > 0, q
    pipe.close()
    pipe1.close()


def test_refused_calls_change_nothing(ctx):
    """7. a lane twice, a lane out of range, steps in flight, a descriptor tracker mode: a message, nothing changed, the
    pipeline still steps."""
    from vo import _native
    cfg, S = SMALL, 4
    data = lane_data(cfg, S)
    pipe = lanes_pipe(ctx, cfg, data)
    for seqs, text in (((0, 2, 0), "named twice"), ((0, 4), "bad sequence index"), ((-1,), "bad sequence index"), ((), "no lane"),
                       ((0, 1, 2, 3, 1), "lanes named")):
        with pytest.raises(_native.VoError, match=text):
            pipe.bootstrap_lanes(1, 0, list(seqs), **boot_kwargs(cfg))
    res = pipe.bootstrap_lanes(1, 0, [0, 1, 2, 3], **boot_kwargs(cfg))
    assert all(r.status == 0 for r in res)
    recs = [step_all(pipe, data, 0, 0, 1)]
    for q, d in enumerate(data):
        pipe.set_frame(2, d["rest"][1], seq=q)
    before = [(pipe.get_state(seq=q), rng_of(pipe, q)) for q in range(S)]
    with pytest.raises(_native.VoError, match="named twice"):
        pipe.bootstrap_lanes(3, 1, [1, 1], **boot_kwargs(cfg))
    pipe.submit(1, 2)
    with pytest.raises(_native.VoError, match="not collected"):
        pipe.bootstrap_lanes(3, 2, [0, 1], **boot_kwargs(cfg))
    recs.append(pipe.collect_all())
    with pytest.raises(_native.VoError, match="next step starts from"):
        pipe.bootstrap_lanes(3, 1, [0, 1], **boot_kwargs(cfg))
    ref = lanes_pipe(ctx, cfg, data)
    ref.bootstrap_lanes(1, 0, [0, 1, 2, 3], **boot_kwargs(cfg))
    ref_recs = [step_all(ref, data, 0, 0, 1), step_all(ref, data, 1, 1, 2)]
    for q in range(S):
        close_records(per_lane(recs, q), per_lane(ref_recs, q), ("lane", q), tol=0.0)
        same_everything(pipe.get_state(seq=q), ref.get_state(seq=q), ("lane", q))
    assert len(before) == S
    recs.append(step_all(pipe, data, 2, 2, 3))
    assert all(r.fault == 0 and r.n_tracked > 0 for r in recs[-1])
    pipe.close()
    ref.close()
    harris = _native.Pipeline(ctx, cfg["H"], cfg["W"], 4, data[0]["K"], n_keypoints=cfg["n"], tracker="harris", sequences=2)
    with pytest.raises(_native.VoError, match="KLT tracker mode"):
        harris.bootstrap_lanes(1, 0, [0, 1])
    harris.close()


def test_later_calls_move_scalars_only(ctx):
    """8. from the second call with the same parameters on: at most 1 KiB up and 1 KiB down per lane (uploaded samples would
    be 64 KiB)."""
    cfg, S = SMALL, 4
    data = lane_data(cfg, S)
    pipe = lanes_pipe(ctx, cfg, data)
    first = pipe.bootstrap_lanes(1, 0, list(range(S)), **boot_kwargs(cfg))
    second = pipe.bootstrap_lanes(1, 0, list(range(S)), **boot_kwargs(cfg))
    third = pipe.bootstrap(1, 0, seq=2, **boot_kwargs(cfg))
    print("bytes per lane up / down: first call %d / %d, second %d / %d, a one-lane call %d / %d" % (
        first[0].bytes_h2d, first[0].bytes_d2h, second[0].bytes_h2d, second[0].bytes_d2h, third.bytes_h2d, third.bytes_d2h))
    for r in second + [third]:
        assert r.status == 0
        assert r.bytes_h2d <= 1024 and r.bytes_d2h <= 1024, (r.bytes_h2d, r.bytes_d2h)
    for a, b in zip(first, second):
        same_results(a, b, "the same call twice")
    pipe.close()


def test_batch_driver_starts_its_lanes_in_one_call(ctx, monkeypatch):
    """9. run_batch_on_device(bootstrap="device"): one bootstrap_lanes call for the lanes of step 0 (and one per later step
    at which recordings start), per recording what bootstrap="host" returns."""
    from vo import _native, driver
    lengths = (9, 14, 6, 20, 11)
    calls = []
    inner = _native.Pipeline.bootstrap_lanes

    def counted(self, idx_a, idx_b, seqs, *args, **kw):
        calls.append(list(seqs))
        return inner(self, idx_a, idx_b, seqs, *args, **kw)

    monkeypatch.setattr(_native.Pipeline, "bootstrap_lanes", counted)

    def recordings():
        return [recording(SMALL, 2023 + 11 * i, n_frames=n + 3) for i, n in enumerate(lengths)]

    kw = dict(n_keypoints=500, hyp=1024, context=ctx, bootstrap_threshold=1.0)
    ref = driver.run_batch_on_device(recordings(), lanes=3, **kw)
    assert calls == []
    got = driver.run_batch_on_device(recordings(), lanes=3, bootstrap="device", **kw)
    print("bootstrap_lanes calls:", calls)
    assert calls[0] == [0, 1, 2]
    assert sum(len(c) for c in calls) == len(lengths)
    for i in range(len(lengths)):
        assert len(got[i]["results"]) == lengths[i]
        close_runs(got[i], ref[i], ("recording", i))
