"""Timings of the track ids (vo_pipeline_config.track_ids) on the stream bench.py times: the resident 1376 x 1241 forward
stream, look-ahead, seams included.  Three modes:

  (default) one process: the one-sequence and the 16-sequence loop with the field off and on, legs alternating, --repeats
    times each -- frames/s and the step period (records' device clock, regroup start to regroup start), and a digest of
    the records (off and on must agree: the ids change nothing else) -- then the export kernel's time at cap 4000
    (Pipeline.export_tracks_post behind every collected step, HIP events around each launch).
  --parent ROOT   field off against another checkout of the project (the commit before, built there): the one-sequence
    loop in one fresh process per leg, legs alternating between the two trees; the digests must agree.
  --sequences / --steps / --warmup / --repeats size the legs.

    python3 tools/dev/track_ids.py [--repeats 3] [--steps 1500] [--warmup 200] [--parent ROOT]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EXPORT_CAP = 4000
K_EXPORT = 26                # VO_K_EXPORT (vo_hip.h)


def use_tree(root):
    for p in (os.path.join(root, "tests"), os.path.join(root, "visual-odometry-project_amd"), root):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)


def setup(S):
    """bench.py's resident streams and bootstraps for S sequences (its own scene for one, its 16-sequence leg's scenes
    otherwise) and a context on a stream of its own, as bench.py makes them."""
    import numpy as np
    import torch
    import bench
    from vo import _native, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("track_ids: no GPU (there is no CPU path to time)")
    seeds = [2023] if S == 1 else [3023 + q for q in range(S)]
    streams = [synthetic.Stream(bench.N_FRAMES, bench.H, bench.W, seed=s) for s in seeds]
    jobs = [(i, bench.H, bench.W, s) for s in seeds for i in range(bench.N_FRAMES)]
    imgs = synthetic.render_images(jobs, min(16, bench.RENDER_WORKERS))
    for q, st in enumerate(streams):
        for i in range(bench.N_FRAMES):
            st._img[i] = imgs[q * bench.N_FRAMES + i]
    comp = torch.cuda.Stream()
    ctx = _native.Context(0, stream=comp.cuda_stream)
    _native.set_default_context(ctx)
    states = [bench.bootstrap_state(st) for st in streams]
    return dict(np=np, bench=bench, native=_native, ctx=ctx, comp=comp, streams=streams, states=states, S=S)


def pipeline(env, track_ids):
    """bench.make_pipeline with the field (not passed at all when off: another checkout's Pipeline may not know it)."""
    bench, streams, states, S = env["bench"], env["streams"], env["states"], env["S"]
    kw = dict(track_ids=True) if track_ids else {}
    pipe = env["native"].Pipeline(env["ctx"], bench.H, bench.W, bench.N_FRAMES, streams[0].K, n_keypoints=bench.N_KP,
                                  klt_win=bench.WIN, klt_max_level=bench.MAX_LEVEL, hyp=bench.HYP_LAUNCH, p3p_threshold=1.0,
                                  outlier_ratio=0.9, confidence=0.99, max_iterations=bench.HYP, refine_iters=bench.REFINE_ITERS,
                                  redetect_start_pose=bench.REDETECT_POSE, sequences=S, detect_margin=bench.DETECT_MARGIN, **kw)
    for q in range(S):
        for i in range(bench.N_FRAMES):
            pipe.set_frame(i, streams[q].image(i), seq=q)
        pipe.set_state(bench.PASS_START, states[q].curr_frame.features, states[q].curr_pose, states[q].prev_pose,
                       num_features=bench.N_KP, seq=q)
    pipe.checkpoint()
    return pipe


def timed(env, pipe, warm, steps, on_step=None):
    np, bench, ctx, S = env["np"], env["bench"], env["ctx"], env["S"]
    w = bench.Walker(pipe, bench.N_FRAMES)
    recs = []

    def each(b, rs):
        recs.append(rs)
        if on_step:
            on_step(rs)
    w.run(warm)
    ctx.sync()
    t0 = time.perf_counter()
    w.run(steps, on_step=each)
    ctx.sync()
    dt = time.perf_counter() - t0
    d = np.diff(np.array([rs[0].ts[1] for rs in recs], dtype=np.float64) * 1e-2)
    ok = (d > 0) & (d < 20 * np.median(d))
    h = hashlib.sha256(repr([(r.n_tracked, r.n_inliers, r.n_landmarks, r.draws_consumed, tuple(r.T_wc))
                             for rs in recs for r in rs]).encode())
    return dict(frames_per_s=round(S * steps / dt, 1), step_period_us=round(float(np.median(d[ok])), 1),
                host_path=int(sum(r.recovered for rs in recs for r in rs)), digest=h.hexdigest()[:12])


def summary(rows):
    return {m: dict(frames_per_s_median=statistics.median(r["frames_per_s"] for r in rs),
                    step_period_us_median=statistics.median(r["step_period_us"] for r in rs),
                    frames_per_s=[r["frames_per_s"] for r in rs], step_period_us=[r["step_period_us"] for r in rs],
                    digests=sorted({r["digest"] for r in rs})) for m, rs in rows.items()}


def off_and_on(a):
    use_tree(HERE)
    out = {}
    for S in a.sequences:
        env = setup(S)
        steps = a.steps if S == 1 else max(2 * (env["bench"].N_FRAMES - 1 - env["bench"].PASS_START), a.steps // 8)
        warm = a.warmup if S == 1 else 30
        rows = {"off": [], "on": []}
        for _ in range(a.repeats):
            for mode in rows:
                pipe = pipeline(env, mode == "on")
                rows[mode].append(timed(env, pipe, warm, steps))
                pipe.close()
                print(S, mode, rows[mode][-1], flush=True)
        out["sequences_%d" % S] = summary(rows)
        if S == 1:                       # the export kernel, behind every collected step of the same loop
            ctx = env["ctx"]
            pipe = pipeline(env, True)
            d_rec = ctx.alloc(pipe.tracks_record_bytes(EXPORT_CAP))
            ctx.prof_enable(K_EXPORT)
            pipe.prof_reset()
            seen = []

            def post(rs):
                pipe.export_tracks_post(rs[0], EXPORT_CAP, d_rec)
                seen.append(min(rs[0].n_tracked, EXPORT_CAP))
            timed(env, pipe, 20, min(a.steps, 400), on_step=post)
            ms, n = pipe.prof_read(K_EXPORT)
            ctx.prof_disable()
            ctx.free(d_rec)
            pipe.close()
            out["export_kernel"] = dict(cap=EXPORT_CAP, launches=int(n), us_mean=round(1e3 * ms / max(n, 1), 2),
                                        rows_median=int(statistics.median(seen)),
                                        bytes_written_median=16 + 48 * int(statistics.median(seen)))
        env["ctx"].close()
    print(json.dumps(out), flush=True)


def leg(a):
    """One field-off run of the one-sequence loop in this process, on the tree a.root."""
    use_tree(a.root)
    os.chdir(a.root)
    env = setup(1)
    pipe = pipeline(env, False)
    print(json.dumps(timed(env, pipe, a.warmup, a.steps)), flush=True)
    pipe.close()
    env["ctx"].close()


def against_parent(a):
    legs = [("this", HERE), ("parent", os.path.abspath(a.parent))]
    rows = {name: [] for name, _ in legs}
    for _ in range(a.repeats):
        for name, root in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--root", root, "--steps", str(a.steps), "--warmup",
                   str(a.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                raise SystemExit("leg %s failed (%d):\n%s" % (name, res.returncode, res.stderr[-2000:]))
            rows[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(name, rows[name][-1], flush=True)
    print(json.dumps(summary(rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(a)
    elif a.parent:
        against_parent(a)
    else:
        off_and_on(a)


if __name__ == "__main__":
    main()
