"""Measurements of the FAST + BRIEF tracker mode of the device-resident loop (tracker_mode = 3), all on one
tree, at 1376 x 1241 with 2000 keypoints and bench.py's harris hypotheses / iteration budget.

loop     the step period of the "fast" mode beside the "harris" and "klt" modes at S = 1 and S = 16: frames resident,
         look-ahead on, the pass starting again from the checkpoint at the end of the resident frames.  A window is K steps
         between two synchronises (host clock), K sized so that it lasts at least --window seconds; the configurations
         alternate, --windows windows each (every pipeline stays alive in between); medians with min - max.
front    the new pieces, each as back-to-back calls between two synchronises on the shapes of the loop: FAST, describe, both
         (the new front), and the Hamming matcher beside the matrix-core byte matcher of the Harris mode, 2000 queries
         against 2000 train rows, S = 1 and S = 16.  (The Harris front's own figures are in DESIGN.md 3.9 / 3.10.)
profile  a fixed number of calls of the new front and matcher and nothing else: the program of a kernel-trace run
         (rocprofv3 --kernel-trace --stats -- python3 tools/dev/fast_loop.py --parts profile), for the per-kernel split.
driver   the class driver's frame rate with tracker_mode "fast" (driver.run: every array through the host).

    python3 tools/dev/fast_loop.py [--parts loop,front,driver] [--sequences 1 16] [--window 0.5] [--windows 5] [--json OUT]
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

H, W, N, HYP = 1241, 1376, 2000, 1000
HYP_LAUNCH = HYP + HYP // 8 + 24          # bench.py's launch size for a budget of HYP iterations
MODES = ("fast", "harris", "klt")


def start_features(ctx, stream, idx, mode):
    """The starting state of pipeline_oracle.initial_features for the mode's own keypoints, made with the device
    primitives (equal to the oracles' bit for bit, and quicker at this size): two thirds triangulated from the analytic
    depth, the rest tracks that start here, and the mode's descriptors."""
    import numpy as np
    from vo.primitives import Features
    img, K = stream.image(idx), stream.K
    if mode == "fast":
        kp = ctx.fast_keypoints(img, 20, N, nonmax=True)
    else:
        kp = ctx.harris_keypoints(img, 9, 0.09, N, 5)
    kp = np.asarray(kp, np.float64).reshape(-1, 2, 1)
    if mode == "klt":
        kp = kp.astype(np.float32)
    f = Features(keypoints=kp)
    n = f.length
    T = stream.T_world_cam(idx)
    z = stream.depth(idx)[kp[:, 1, 0].astype(int), kp[:, 0, 0].astype(int)].astype(np.float64)
    xc = (kp[:, 0, 0].astype(np.float64) - K[0, 2]) / K[0, 0] * z
    yc = (kp[:, 1, 0].astype(np.float64) - K[1, 2]) / K[1, 1] * z
    land = np.stack([T[r, 0] * xc + T[r, 1] * yc + T[r, 2] * z + T[r, 3] for r in range(3)], axis=1)
    n_tri = (2 * n) // 3
    f.state = np.concatenate([2 * np.ones(n_tri), np.ones(n - n_tri)])
    f.landmarks[:n_tri] = land[:n_tri].reshape(-1, 3, 1)
    f.tracks = np.concatenate([np.full((n_tri, 2, 1), np.nan), kp[n_tri:].astype(np.float64)])
    f.poses = np.concatenate([np.full((n_tri, 4, 4), np.nan), np.stack([T] * (n - n_tri))])
    if mode == "fast":
        f.descriptors = ctx.brief_describe(img, kp[:, :, 0])
    elif mode == "harris":
        f.descriptors = ctx.patch_descriptors(img, kp[:, :, 0], 9)
    return f, T


class Walker:
    """One pipeline walking its resident frames with one step of look-ahead, back to the checkpoint at the end."""

    def __init__(self, ctx, mode, S, frames, K, starts, F):
        from vo import _native
        self.S, self.F, self.mode = S, F, mode
        self.pipe = _native.Pipeline(ctx, H, W, F, K, n_keypoints=N, hyp=HYP_LAUNCH, p3p_threshold=1.0, outlier_ratio=0.9,
                                     confidence=0.99, max_iterations=HYP, refine_iters=20, tracker=mode, sequences=S)
        for q in range(S):
            for i in range(F):
                self.pipe.set_frame(i, frames[q + i], seq=q)
            self.pipe.set_state(0, starts[q][0], starts[q][1], starts[q][1], seq=q, num_features=N)
        self.pipe.checkpoint()
        self.b, self.inflight, self.faults, self.recovered, self.tracked = 0, 0, 0, 0, []

    def _collect(self):
        rs = self.pipe.collect_all()
        self.inflight -= 1
        self.faults += sum(1 for r in rs if r.fault)
        self.recovered += sum(r.recovered for r in rs)
        self.tracked.append(rs[0].n_tracked)

    def steps(self, n):
        done = 0
        while done < n:
            if self.b + 1 >= self.F:              # the seam: drain, rewind to the checkpoint
                while self.inflight:
                    self._collect()
                    done += 1
                self.pipe.rewind()
                self.b = 0
                continue
            self.pipe.submit(self.b, self.b + 1)
            self.b += 1
            self.inflight += 1
            if self.inflight == 2:
                self._collect()
                done += 1
        while self.inflight:
            self._collect()
            done += 1
        return done


def part_loop(a, out):
    from vo import _native, synthetic
    S_max, F = max(a.sequences), a.frames
    stream = synthetic.Stream(F + S_max - 1, H, W).prefetch(workers=min(12, max(1, (os.cpu_count() or 2) - 2)))
    frames = [stream.image(i) for i in range(F + S_max - 1)]
    ctx = _native.Context(0)
    starts = {m: [] for m in MODES}
    for q in range(S_max):
        sq = synthetic.Stream(F, H, W, start=q)
        sq._img = {i: frames[q + i] for i in range(F)}
        for m in MODES:
            starts[m].append(start_features(ctx, sq, 0, m))
    walkers = {}
    for S in a.sequences:
        for m in MODES:
            walkers["%s_S%d" % (m, S)] = Walker(ctx, m, S, frames, stream.K, starts[m], F)

    def window(w, k):
        ctx.sync()
        t0 = time.perf_counter()
        n = w.steps(k)
        ctx.sync()
        return (time.perf_counter() - t0) / n

    k = {}
    for name, w in walkers.items():                           # warm up, and size the windows
        window(w, a.warmup)
        k[name] = max(a.warmup, int(a.window / window(w, a.warmup)) + 1)
    xs = {name: [] for name in walkers}
    for _ in range(a.windows):
        for name, w in walkers.items():                       # (the configurations alternate)
            xs[name].append(1e6 * window(w, k[name]))
    for name, v in xs.items():
        w = walkers[name]
        med = statistics.median(v)
        out["loop_" + name] = dict(us_per_step_median=round(med, 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                                   frames_per_s=round(1e6 * w.S / med, 1), steps_per_window=k[name], windows=len(v),
                                   faults=w.faults, host_path_steps=w.recovered,
                                   tracked_median=int(statistics.median(w.tracked)))
    for w in walkers.values():
        w.pipe.close()
    ctx.close()


class FrontRig:
    """S frames on the device with the buffers of both fronts and both matchers, laid out as the pipeline lays them."""

    def __init__(self, S):
        import numpy as np
        from vo import _native, synthetic
        self.np, self.S = np, S
        self.ctx = ctx = _native.Context(0)
        img = synthetic.Stream(2, H, W)
        a, b = img.image(0), img.image(1)
        self.d_imgs = ctx.to_device(np.stack([np.roll(b, (7 * q, 13 * q), axis=(0, 1)) for q in range(S)]))
        self.d_kp, self.d_n = ctx.alloc(S * N * 16), ctx.to_device(np.full(S, N, np.int32))
        self.d_brief = ctx.alloc(S * N * 32)
        tp = np.zeros((N, 384), np.uint8)                     # the byte matcher's train rows: frame b's patches
        tp[:, :361] = ctx.patch_descriptors(b, ctx.harris_keypoints(b, 9, 0.09, N, 5), 9).astype(np.uint8)
        self.d_patch = ctx.to_device(np.stack([tp] * S))
        self.d_pairs, self.d_np = ctx.alloc(S * N * 8), ctx.alloc(S * 4)
        # the query side: frame a's descriptors of both kinds, the same for every sequence
        kf = ctx.fast_keypoints(a, 20, N, nonmax=True)
        kh = ctx.harris_keypoints(a, 9, 0.09, N, 5)
        qb = np.zeros((N, 32), np.uint8)
        qb[:len(kf)] = ctx.brief_describe(a, kf)
        qp = np.zeros((N, 384), np.uint8)
        qp[:, :361] = ctx.patch_descriptors(a, kh, 9).astype(np.uint8)
        self.d_qb, self.d_qp = ctx.to_device(np.stack([qb] * S)), ctx.to_device(np.stack([qp] * S))
        self.d_nq = ctx.to_device(np.full(S, N, np.int32))
        self.ptrs = [self.d_imgs, self.d_kp, self.d_n, self.d_brief, self.d_patch, self.d_pairs, self.d_np,
                     self.d_qb, self.d_qp, self.d_nq]

    def fast(self):
        self.ctx.fast_keypoints_batch_dev(self.d_imgs, H * W, self.S, H, W, self.d_kp, N, self.d_n, 20, N, True)

    def describe(self):
        self.ctx.brief_describe_batch_dev(self.d_imgs, H * W, self.S, H, W, self.d_kp, N, self.d_n, N, False, self.d_brief, N * 32)

    def fast_front(self):
        self.fast()
        self.describe()

    def hamming(self):
        self.ctx.match_hamming_batch_dev(self.d_qb, N * 32, self.d_nq, 1, N, self.d_brief, N * 32, self.d_n, 1, N, self.S, 32, 0.8, 64,
                                         self.d_pairs, self.d_np)

    def u8(self):
        self.ctx.match_u8_batch_dev(self.d_qp, N * 384, self.d_nq, 1, N, self.d_patch, N * 384, self.d_nq, 1, N, self.S, 0.85,
                                    self.d_pairs, self.d_np, 384)

    def configs(self):
        return dict(fast_detect=self.fast, brief_describe=self.describe, fast_front=self.fast_front, hamming_match=self.hamming,
                    u8_match=self.u8)

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ctx.close()


def call_window(ctx, call, k):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        call()
    ctx.sync()
    return (time.perf_counter() - t0) / k


def part_front(a, out):
    for S in a.sequences:
        rig = FrontRig(S)
        np, ctx = rig.np, rig.ctx
        rig.fast_front()
        rig.hamming()
        ctx.sync()
        out["front_S%d_counts" % S] = dict(corners=ctx.download(rig.d_n, (S,), np.int32).tolist()[:4],
                                           pairs=ctx.download(rig.d_np, (S,), np.int32).tolist()[:4])
        cfg = rig.configs()
        k = {}
        for name, call in cfg.items():
            call_window(ctx, call, 10)
            k[name] = max(10, int(a.window / 2 / call_window(ctx, call, 20)) + 1)
        xs = {name: [] for name in cfg}
        for _ in range(a.windows):
            for name, call in cfg.items():
                xs[name].append(1e6 * call_window(ctx, call, k[name]))
        for name, v in xs.items():
            out["front_S%d_%s" % (S, name)] = dict(us_median=round(statistics.median(v), 2), us_min=round(min(v), 2),
                                                   us_max=round(max(v), 2), calls_per_window=k[name], windows=len(v))
        rig.close()


def part_profile(a, out):
    for S in a.sequences:
        rig = FrontRig(S)
        for _ in range(a.profile_calls):
            rig.fast_front()
            rig.hamming()
        rig.ctx.sync()
        out["profiled_S%d" % S] = a.profile_calls
        rig.close()


def part_driver(a, out):
    import numpy as np
    from vo import driver
    from vo.features import FASTBRIEFDetector
    from vo.primitives import Sequence
    FASTBRIEFDetector._num_keypoints_override = N
    seq = Sequence("synthetic", n_frames=a.driver_frames, height=H, width=W, channels=1)
    run = driver.run(seq, "fast")
    s = np.asarray(run["frame_seconds"])[1:]                  # (the first frame pays the allocations)
    out["driver_fast"] = dict(frames=len(s), ms_median=round(1e3 * float(np.median(s)), 2),
                              fps=round(1.0 / float(np.median(s)), 1), landmarks_last=int(run["n_landmarks"][-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="loop,front,driver")
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--frames", type=int, default=24, help="resident frames per sequence")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--profile-calls", type=int, default=50)
    ap.add_argument("--driver-frames", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    class Report(dict):
        def __setitem__(self, k, v):
            print(k, v, flush=True)
            dict.__setitem__(self, k, v)
    out = Report()
    for part in a.parts.split(","):
        dict(loop=part_loop, front=part_front, profile=part_profile, driver=part_driver)[part](a, out)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
