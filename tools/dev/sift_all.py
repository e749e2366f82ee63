"""Every SIFT keypoint on the device (vo_sift_all_batch_dev) on the cfg-3 frame size (1376 x 1241, ~9k keypoints per frame,
frames in device memory), against the other ways of making the same or a capped result:
  (a) all      one vo_sift_all_batch_dev call on S images (rows = 16384, byte descriptors): the order on the device;
  (b) host     vo_sift_batch(cap = 0) on the same S images: the described rows copied to the host and ordered there (host
               images in, host arrays out: its upload and the rows' download are part of it);
  (c) capped   one vo_sift_batch_dev call at cap 2000 (the capped device path, for scale).
Then the device loop of the cfg-3 stream in the SIFT tracker mode (look-ahead on, frames resident, bench.py's hypotheses
budget) at sift_cap = 2000 and at sift_cap = -1 (every keypoint, feature_cap = 16384): frames/s.  Per case a warm-up,
then a timed window of at least --min-seconds (host clock between two synchronisations); the image cases run --repeats
times interleaved, the median is reported with the spread.

    python3 tools/dev/sift_all.py [--sequences 1 4 16] [--repeats 3] [--min-seconds 1.0] [--json OUT]
    python3 tools/dev/sift_all.py --trace S [--iters 20]    # case (a) only, untimed: for a rocprofv3 --kernel-trace run
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

H, W, ROWS, CAP = 1241, 1376, 16384, 2000
HYP = 1000
HYP_LAUNCH = HYP + HYP // 8 + 24          # bench.py's launch size for a budget of HYP iterations


class Ctx:
    """A context with S frames resident and its own output buffers (byte descriptors, as the pipeline asks for)."""

    def __init__(self, frames):
        import numpy as np
        from vo import _native
        self.c = _native.Context(0)
        self.frames = frames
        self.S = len(frames)
        self.d_imgs = self.c.to_device(np.stack(frames))
        self.d_kp = self.c.alloc(self.S * ROWS * 24)
        self.d_u8 = self.c.alloc(self.S * ROWS * 128)
        self.d_n = self.c.alloc(self.S * 4)
        self.d_over = self.c.alloc(self.S * 4)

    def all(self, S):
        self.c.sift_all_batch_dev(self.d_imgs, H * W, S, H, W, ROWS, self.d_kp, ROWS, None, self.d_u8, ROWS, self.d_n,
                                  self.d_over)

    def host(self, S):
        self.c.sift_batch(self.frames[:S], cap=None)

    def capped(self, S):
        c = self.c
        c._chk(c._lib.vo_sift_batch_dev(c._h, self.d_imgs, H * W, S, H, W, CAP, self.d_kp, ROWS, None, self.d_u8, ROWS,
                                        self.d_n, self.d_over))

    def check(self, S):
        import numpy as np
        self.c.sync()
        over = self.c.download(self.d_over, (S,), np.int32)
        n = self.c.download(self.d_n, (S,), np.int32)
        assert not over.any() and (n > 4096).all(), (over, n)
        return [int(v) for v in n]

    def close(self):
        self.c.close()


def timed(step, sync, per_step, warm, min_s):
    for _ in range(warm):
        step()
    sync()
    k = 2
    while True:
        sync()
        t0 = time.perf_counter()
        for _ in range(k):
            step()
        sync()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return k * per_step / dt
        k = int(k * max(2.0, 1.2 * min_s / max(dt, 1e-3)))


def loop(ctx, stream, F, sift_cap, warm, min_s):
    """frames/s of the device loop in the SIFT tracker mode over the F resident frames, pass after pass (rewind at the
    seam, as bench.py's walker); also the median keypoints per frame and the steps the host path finished."""
    import numpy as np
    from pipeline_oracle import initial_sift_features
    from vo import _native
    n_kp = CAP if sift_cap > 0 else ROWS
    feats, T = initial_sift_features(stream, 0, n_kp)
    pipe = _native.Pipeline(ctx, H, W, F, stream.K, n_keypoints=n_kp, feature_cap=(0 if sift_cap > 0 else ROWS),
                            hyp=HYP_LAUNCH, p3p_threshold=1.0, outlier_ratio=0.9, confidence=0.99, max_iterations=HYP,
                            refine_iters=20, tracker="sift", sift_cap=sift_cap)
    for i in range(F):
        pipe.set_frame(i, stream.image(i))
    pipe.set_state(0, feats, T, T, num_features=n_kp)
    pipe.checkpoint()
    st = {"b": 0, "inflight": 0, "n_in": [], "rec": 0}

    def collect():
        r = pipe.collect()
        st["inflight"] -= 1
        st["n_in"].append(r.n_features_in)
        st["rec"] += int(r.recovered)

    def steps(n):
        done = 0
        while done < n:
            a = st["b"]
            if a + 1 >= F:                     # the seam: drain, rewind to the checkpoint
                while st["inflight"]:
                    collect()
                    done += 1
                pipe.rewind()
                st["b"] = 0
                continue
            pipe.submit(a, a + 1)
            st["b"] = a + 1
            st["inflight"] += 1
            if st["inflight"] == 2:
                collect()
                done += 1
        return done

    steps(warm)
    k = 8
    while True:
        ctx.sync()
        t0 = time.perf_counter()
        n = steps(k)
        ctx.sync()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            break
        k = int(k * max(2.0, 1.2 * min_s / max(dt, 1e-3)))
    while st["inflight"]:
        collect()
    pipe.close()
    return {"sift_cap": sift_cap, "frames_per_s": round(n / dt, 1), "ms_per_step": round(dt / n * 1e3, 3),
            "median_keypoints_per_frame": int(np.median(st["n_in"])), "steps_finished_by_host_path": st["rec"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=20, help="resident frames of the loop")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--trace", type=int, default=0, help="run case (a) at this S only, --iters times, untimed")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from vo import synthetic
    S_max = args.trace or max(args.sequences)
    stream = synthetic.Stream(max(S_max, args.frames), H, W).prefetch(workers=min(12, max(1, (os.cpu_count() or 2) - 2)))
    frames = [stream.image(i) for i in range(S_max)]
    if args.trace:
        a = Ctx(frames)
        for _ in range(args.iters):
            a.all(args.trace)
        a.check(args.trace)
        a.close()
        return
    a = Ctx(frames)
    cases = {"all": a.all, "host": a.host, "capped": a.capped}
    res = {(S, k): [] for S in args.sequences for k in cases}
    counts = {}
    for r in range(args.repeats):
        for S in args.sequences:
            for k, fn in cases.items():
                res[(S, k)].append(timed(lambda: fn(S), a.c.sync, S, args.warmup, args.min_seconds))
                if k == "all":
                    counts[S] = a.check(S)
    out = []
    for S in args.sequences:
        row = {"S": S, "keypoints": counts[S]}
        for k in cases:
            v = res[(S, k)]
            row[k + "_images_per_s"] = round(statistics.median(v), 1)
            row[k + "_runs"] = [round(x, 1) for x in v]
        row["all_over_host"] = round(row["all_images_per_s"] / row["host_images_per_s"], 3)
        out.append(row)
        print(json.dumps(row), flush=True)
    if not args.no_loop:
        for cap in (CAP, -1):
            row = loop(a.c, stream, args.frames, cap, 10, max(2.0, args.min_seconds))
            out.append(row)
            print(json.dumps(row), flush=True)
    a.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
