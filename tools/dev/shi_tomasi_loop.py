"""The device-resident KLT loop on bench.py's forward stream with the Shi-Tomasi re-detect (vo_pipeline_config.detector = 1)
beside the Harris one (detector = 0), in one process, legs alternating:

  per detector and sequence count (default 1 and 16), --repeats legs of --warmup + --steps steps each (look-ahead, seams
  included, as bench.py's timed leg):
    frames/s and ms per step (wall clock around the leg);
    the step period from the records' device clock stamps (regroup start to regroup start, 100 MHz ticks): the median
      over all steps, over the steps whose `prev` frame the detector executed on (detector_ran), and over the others;
    how often the detector executed, how often a step re-detected, what it appended, steps finished by the host path.
  detector = 1 only, from device events around the whole chain (VO_K_SHI_TOMASI_CHAIN, every launch of it bracketed on the
  detection stream; the bracket itself costs two event records, so these legs are not the timed ones):
    the chain's duration gated out for every sequence (debug_never_detect, and a re-detect limit no stream reaches, so
      that no step asks the host path for a detection) and executing for every sequence (detect_margin < 0).
  VO_ST_ROUNDS=<n> (before the process starts) changes the round launches of the minimum-distance rule: run once per value
  for the A/B.

    python3 tools/dev/shi_tomasi_loop.py [--sequences 1 16] [--steps 1500] [--warmup 200] [--repeats 3] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "visual-odometry-project_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chain-steps", type=int, default=60)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from vo import _native, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("shi_tomasi_loop: no GPU (there is no CPU path to time)")
    S_max = max(a.sequences)
    streams = [synthetic.Stream(bench.N_FRAMES, bench.H, bench.W, seed=2023 + q) for q in range(S_max)]
    jobs = [(st.start + i, bench.H, bench.W, st.seed) for st in streams for i in range(bench.N_FRAMES)]
    for (st, i), im in zip([(st, i) for st in streams for i in range(bench.N_FRAMES)],
                           synthetic.render_images(jobs, min(16, bench.RENDER_WORKERS))):
        st._img[i] = im
    torch.cuda.synchronize()
    comp = torch.cuda.Stream()
    ctx = _native.Context(0, stream=comp.cuda_stream)
    _native.set_default_context(ctx)
    states = [bench.bootstrap_state(st) for st in streams]

    def make(S, detector, **kw):
        kw.setdefault("detect_margin", bench.DETECT_MARGIN)
        pipe = _native.Pipeline(ctx, bench.H, bench.W, bench.N_FRAMES, streams[0].K, n_keypoints=bench.N_KP, klt_win=bench.WIN,
                                klt_max_level=bench.MAX_LEVEL, hyp=bench.HYP_LAUNCH, p3p_threshold=1.0, outlier_ratio=0.9,
                                confidence=0.99, max_iterations=bench.HYP, refine_iters=bench.REFINE_ITERS,
                                redetect_start_pose=bench.REDETECT_POSE, sequences=S, detector=detector, **kw)
        for q in range(S):
            for i in range(bench.N_FRAMES):
                pipe.set_frame(i, streams[q].image(i), seq=q)
            pipe.set_state(bench.PASS_START, states[q].curr_frame.features, states[q].curr_pose, states[q].prev_pose,
                           num_features=bench.N_KP, seq=q)
        pipe.checkpoint()
        return pipe

    def leg(w, S, warm, steps):
        recs = []
        w.run(warm)
        ctx.sync()
        t0 = time.perf_counter()
        w.run(steps, on_step=lambda b, rs: recs.append(rs))
        ctx.sync()
        dt = time.perf_counter() - t0
        # the step period on the device: sequence 0's regroup start, step to step (seams left out: a rewind lies between)
        t = np.array([rs[0].ts[1] for rs in recs], dtype=np.float64) * 1e-2
        d = np.diff(t)
        ran = np.array([max(r.detector_ran for r in rs) for rs in recs][1:], dtype=bool)
        ok = (d > 0) & (d < 20 * np.median(d))
        flat = [r for rs in recs for r in rs]
        med = lambda v: round(float(np.median(v)), 1) if len(v) else None
        return dict(frames_per_s=round(S * steps / dt, 1), ms_per_step=round(dt / steps * 1e3, 4),
                    step_period_us=med(d[ok]), step_period_us_detector_executed=med(d[ok & ran]),
                    step_period_us_detector_gated=med(d[ok & ~ran]),
                    detector_executed_fraction=round(float(np.mean([r.detector_ran for r in flat])), 4),
                    redetect_fraction=round(float(np.mean([r.redetected for r in flat])), 4),
                    features_in_median=med([r.n_features_in for r in flat]),
                    host_path_steps=int(sum(r.recovered for r in flat)))

    out = []
    for S in a.sequences:
        pipes = {d: make(S, d) for d in ("harris", "shi-tomasi")}
        walkers = {d: bench.Walker(pipe, bench.N_FRAMES) for d, pipe in pipes.items()}     # (one per pipeline: it knows the frame)
        rows = {d: [] for d in pipes}
        for _ in range(a.repeats):
            for d, w in walkers.items():
                rows[d].append(leg(w, S, a.warmup, a.steps))
        for pipe in pipes.values():
            pipe.close()
        row = dict(S=S, st_rounds=os.environ.get("VO_ST_ROUNDS", "24"))
        for d, legs in rows.items():
            fps = [r["frames_per_s"] for r in legs]
            row[d] = dict(frames_per_s=fps, frames_per_s_median=statistics.median(fps),
                          spread_pct=round(100.0 * (max(fps) - min(fps)) / statistics.median(fps), 2), legs=legs)
        # the chain alone: gated out everywhere / executing everywhere
        chain = {}
        for name, kw in (("gated_out", dict(debug_never_detect=1, redetect_fraction=0.01)), ("executing", dict(detect_margin=-1.0))):
            pipe = make(S, "shi-tomasi", **kw)
            w = bench.Walker(pipe, bench.N_FRAMES)
            w.run(30)
            ctx.sync()
            ctx.prof_enable(_native.K_SHI_TOMASI_CHAIN)
            pipe.prof_reset()
            # (inside one pass: a seam's rewind forces a detection, which executes whatever the gate says)
            w.run(min(a.chain_steps, bench.N_FRAMES - 1 - bench.PASS_START - 30 - 2))
            ctx.sync()
            ms, n = pipe.prof_read(_native.K_SHI_TOMASI_CHAIN)
            ctx.prof_disable()
            chain[name] = dict(chain_us=round(1e3 * ms / max(n, 1), 1), chains=n)
            pipe.close()
        row["shi_tomasi_chain"] = chain
        out.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
