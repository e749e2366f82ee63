"""Harris tracker mode with several sequences per launch: frames/s (all sequences) and ms per step at S = 1, 4, 16 on the
cfg-2 stream (1376 x 1241, 2000 keypoints, bench.py's harris hypotheses / iteration budget), frames resident, look-ahead
on, a warm-up, then a timed window of at least a second (host clock after a synchronise).  Sequence q walks the scene from
frame q on (one rendered stream shared by all); at the end of the resident frames the pass starts again from the
checkpoint (vo_pipeline_rewind), as bench.py's walker does.

    python3 tools/dev/harris_sequences.py [--sequences 1 4 16] [--frames 40] [--min-seconds 1.0] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "visual-odometry-project_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W, N, HYP = 1241, 1376, 2000, 1000
HYP_LAUNCH = HYP + HYP // 8 + 24          # bench.py's launch size for a budget of HYP iterations
START = 0


def run(ctx, frames, starts, S, F, warm, min_s):
    from vo import _native
    pipe = _native.Pipeline(ctx, H, W, F, frames[0][1], n_keypoints=N, hyp=HYP_LAUNCH, p3p_threshold=1.0, outlier_ratio=0.9,
                            confidence=0.99, max_iterations=HYP, refine_iters=20, tracker="harris", sequences=S)
    for q in range(S):
        for i in range(F):
            pipe.set_frame(i, frames[q + i][0], seq=q)
        pipe.set_state(START, starts[q][0], starts[q][1], starts[q][1], seq=q, num_features=N)
    pipe.checkpoint()
    state = {"b": START, "inflight": 0}

    def steps(n):
        done = 0
        while done < n:
            a = state["b"]
            if a + 1 >= F:                     # the seam: drain, rewind to the checkpoint
                while state["inflight"]:
                    pipe.collect_all()
                    state["inflight"] -= 1
                    done += 1
                pipe.rewind()
                state["b"] = START
                continue
            pipe.submit(a, a + 1)
            state["b"] = a + 1
            state["inflight"] += 1
            if state["inflight"] == 2:
                rs = pipe.collect_all()
                assert all(r.fault == 0 for r in rs), [r.fault for r in rs]
                state["inflight"] -= 1
                done += 1
        return done

    steps(warm)
    n = 16
    while True:
        ctx.sync()
        t0 = time.perf_counter()
        k = steps(n)
        while state["inflight"]:
            pipe.collect_all()
            state["inflight"] -= 1
            k += 1
        ctx.sync()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            break
        n = int(n * max(2.0, 1.2 * min_s / max(dt, 1e-3)))
    pipe.close()
    return {"sequences": S, "steps": k, "seconds": round(dt, 4), "frames_per_s": round(k * S / dt, 1),
            "ms_per_step": round(dt / k * 1e3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--frames", type=int, default=40, help="resident frames per sequence")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from vo import _native, synthetic
    from pipeline_oracle import initial_harris_features
    S_max, F = max(args.sequences), args.frames
    stream = synthetic.Stream(F + S_max - 1, H, W).prefetch(workers=min(12, max(1, (os.cpu_count() or 2) - 2)))
    frames = [(stream.image(i), stream.K) for i in range(F + S_max - 1)]
    starts = []
    for q in range(S_max):
        sq = synthetic.Stream(F, H, W, start=q)
        sq._img = {i: stream.image(q + i) for i in range(F)}
        starts.append(initial_harris_features(sq, START, N))
    ctx = _native.Context(0)
    out = []
    for S in args.sequences:
        r = run(ctx, frames, starts, S, F, args.warmup, args.min_seconds)
        out.append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
