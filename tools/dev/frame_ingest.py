"""Timings of the frame ingest (csrc/ingest.hip) at bench.py's frame size, 1376 x 1241.  Three modes:

  (default) the driver rate: vo.driver.run_on_device(bootstrap="device") on a three-channel recording, one fresh process per
    leg, legs alternating between this tree, the same recording behind a lens (coefficients set: the undistortion runs) and,
    with --parent ROOT, another checkout of the project (the commit before the ingest, built there) -- frames/s of the loop
    (the driver's frame_seconds: reading the frame is the sequence's time, not the loop's), first --skip steps left out, and
    a digest of the trajectory and the records' integer fields (this tree and the parent must agree: same grey formula).
  --kernels   every ingest kernel --reps times, for `rocprofv3 --kernel-trace --stats -- python tools/dev/frame_ingest.py
    --kernels`: grey (3 + 1 bytes per pixel), undistort of a grey image (1 + 1), undistort of a B, G, R image in one kernel
    (3 + 1), the last through the pipeline's pinned upload.  Prints the algorithmic bytes to divide by the trace's times.
  --beside    the step period (records' device clock, regroup start to regroup start) and frames/s of bench.py's resident
    loop with nothing uploaded, with one grey frame per step uploaded from pinned memory (a copy, no kernel), with one grey
    frame per step behind a lens (the same copy + the undistort kernel on the upload stream, beside the step) and with one
    B, G, R frame per step behind a lens (three times the copy + the kernel).  The uploaded frame is the one the slot holds
    already (K_raw = K, zero coefficients: the identity), 48 steps ahead of its use.

    python3 tools/dev/frame_ingest.py [--frames 80] [--repeats 3] [--parent ROOT] | --kernels [--reps 50] | --beside
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LENS = (-0.05, 0.01, 0.001, -0.001, 0.0)
H, W = 1241, 1376            # bench.py's frame


def use_tree(root):
    for p in (os.path.join(root, "tests"), os.path.join(root, "visual-odometry-project_amd"), root):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)


class Recording:
    """Grey frames held in memory, delivered with three channels (as cv2.imread delivers a grey PNG)."""

    dataset, increment = "frames", 1

    def __init__(self, frames, K, dist):
        from vo.sensors import Camera
        import numpy as np
        self.frames, self.idx = [np.repeat(f[:, :, None], 3, axis=2) for f in frames], 0
        self.camera = Camera(K, None if dist is None else np.array(dist))

    def get_camera(self):
        return self.camera

    def __len__(self):
        return len(self.frames)

    def __iter__(self):
        return self

    def __next__(self):
        from vo.primitives import Frame
        if self.idx >= len(self.frames):
            raise StopIteration
        f = Frame(self.frames[self.idx], sensor=self.camera, intrinsics=self.camera.intrinsic_matrix)
        f.frame_id = self.idx
        self.idx += 1
        return f


def leg(a):
    """One run of the driver in this process, on the tree a.root."""
    use_tree(a.root)
    import numpy as np
    from vo import driver, synthetic
    frames = np.load(a.leg)
    K = synthetic.intrinsics(*frames.shape[1:])
    rec = Recording(list(frames), K, LENS if a.lens else None)
    out = driver.run_on_device(rec, n_keypoints=2000, bootstrap="device", bootstrap_win=21, bootstrap_max_level=3,
                               bootstrap_threshold=1.0)
    sec = out["frame_seconds"][a.skip:]
    h = hashlib.sha256(np.ascontiguousarray(out["trajectory"]).tobytes())
    for r in out["results"]:
        h.update(repr((r.n_tracked, r.n_inliers, r.n_landmarks, r.draws_consumed, r.fault)).encode())
    print(json.dumps(dict(steps=len(sec), frames_per_s=round(len(sec) / float(np.sum(sec)), 1),
                          us_per_step_median=round(1e6 * float(np.median(sec)), 1), digest=h.hexdigest()[:16],
                          faults=int(sum(r.fault != 0 for r in out["results"])))), flush=True)


def driver_rate(a):
    use_tree(HERE)
    import numpy as np
    from vo import synthetic
    tmp = tempfile.mkdtemp(prefix="frame_ingest_")
    path = os.path.join(tmp, "frames.npy")
    jobs = [(i, H, W, 2023) for i in range(a.frames)]
    np.save(path, np.stack(synthetic.render_images(jobs, 12)))
    legs = [("this", HERE, False), ("this_lens", HERE, True)] + ([("parent", os.path.abspath(a.parent), False)] if a.parent else [])
    rows = {name: [] for name, _, _ in legs}
    for _ in range(a.repeats):
        for name, root, lens in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", path, "--root", root, "--skip", str(a.skip)]
            res = subprocess.run(cmd + (["--lens"] if lens else []), capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit("leg %s failed (%d):\n%s" % (name, res.returncode, res.stderr[-2000:]))
            rows[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(name, rows[name][-1], flush=True)
    os.remove(path)
    os.rmdir(tmp)
    out = {}
    for name, rs in rows.items():
        fps = [r["frames_per_s"] for r in rs]
        out[name] = dict(frames_per_s=fps, median=statistics.median(fps),
                         spread_pct=round(100.0 * (max(fps) - min(fps)) / statistics.median(fps), 2),
                         digests=sorted({r["digest"] for r in rs}), faults=sum(r["faults"] for r in rs))
    print(json.dumps(out), flush=True)


def kernels(a):
    use_tree(HERE)
    import numpy as np
    from vo import _native, synthetic
    rng = np.random.default_rng(1)
    bgr, grey = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    K = synthetic.intrinsics(H, W)
    ctx = _native.Context(0)
    pipe = _native.Pipeline(ctx, H, W, 4, K, n_keypoints=2000)
    pipe.set_distortion(0, LENS)
    pin = ctx.pinned_empty((H, W, 3))
    pin[...] = bgr
    for _ in range(a.reps):
        ctx.gray_from_bgr(bgr)
        ctx.undistort_image(grey, K, LENS)
        pipe.set_frame(1, pin, pinned=True)
        pipe.frame_uploaded(1, wait=True)
    pipe.close()
    ctx.close()
    px = H * W
    print(json.dumps(dict(pixels=px, reps=a.reps, bytes=dict(ingest_gray_kernel=4 * px, ingest_undistort_kernel_1=2 * px,
                                                              ingest_undistort_kernel_3=4 * px))), flush=True)


def beside(a):
    use_tree(HERE)
    import numpy as np
    import torch
    import bench
    from vo import _native, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("frame_ingest: no GPU (there is no CPU path to time)")
    st = synthetic.Stream(bench.N_FRAMES, bench.H, bench.W, seed=2023)
    jobs = [(i, bench.H, bench.W, st.seed) for i in range(bench.N_FRAMES)]
    for i, im in enumerate(synthetic.render_images(jobs, min(16, bench.RENDER_WORKERS))):
        st._img[i] = im
    comp = torch.cuda.Stream()
    ctx = _native.Context(0, stream=comp.cuda_stream)
    _native.set_default_context(ctx)
    state = bench.bootstrap_state(st)
    pipe = _native.Pipeline(ctx, bench.H, bench.W, bench.N_FRAMES, st.K, n_keypoints=bench.N_KP, klt_win=bench.WIN,
                            klt_max_level=bench.MAX_LEVEL, hyp=bench.HYP_LAUNCH, p3p_threshold=1.0, outlier_ratio=0.9,
                            confidence=0.99, max_iterations=bench.HYP, refine_iters=bench.REFINE_ITERS,
                            redetect_start_pose=bench.REDETECT_POSE, detect_margin=bench.DETECT_MARGIN)
    for i in range(bench.N_FRAMES):
        pipe.set_frame(i, st.image(i))
    pipe.set_state(bench.PASS_START, state.curr_frame.features, state.curr_pose, state.prev_pose, num_features=bench.N_KP)
    pipe.checkpoint()
    pin1 = [ctx.pinned_empty((bench.H, bench.W)) for _ in range(bench.N_FRAMES)]
    pin3 = [ctx.pinned_empty((bench.H, bench.W, 3)) for _ in range(bench.N_FRAMES)]
    for i in range(bench.N_FRAMES):
        pin1[i][...] = st.image(i)
        pin3[i][...] = st.image(i)[:, :, None]
    span = bench.N_FRAMES - bench.PASS_START
    w = bench.Walker(pipe, bench.N_FRAMES)

    def run(mode, warm, steps):
        pipe.set_distortion(0, None, K_raw=st.K if mode.endswith("_lens") else None)
        recs = []

        def on_step(b, rs):
            recs.append(rs[0])
            s = bench.PASS_START + (b - bench.PASS_START + 48) % span
            if mode != "none" and s != bench.PASS_START:           # (the checkpoint's frame stays)
                pipe.set_frame(s, pin1[s] if mode.startswith("grey") else pin3[s], pinned=True)

        w.run(warm, on_step=on_step)
        ctx.sync()
        del recs[:]
        t0 = time.perf_counter()
        w.run(steps, on_step=on_step)
        ctx.sync()
        dt = time.perf_counter() - t0
        d = np.diff(np.array([r.ts[1] for r in recs], dtype=np.float64) * 1e-2)
        ok = (d > 0) & (d < 20 * np.median(d))
        h = hashlib.sha256(repr([(r.n_tracked, r.n_inliers, r.n_landmarks, tuple(r.T_wc)) for r in recs[-50:]]).encode())
        return dict(frames_per_s=round(steps / dt, 1), step_period_us=round(float(np.median(d[ok])), 1),
                    faults=int(sum(r.fault != 0 for r in recs)), digest=h.hexdigest()[:12])

    rows = {m: [] for m in ("none", "grey", "grey_lens", "bgr_lens")}
    for _ in range(a.repeats):
        for m in rows:
            rows[m].append(run(m, a.warmup, a.steps))
            print(m, rows[m][-1], flush=True)
    pipe.close()
    ctx.close()
    print(json.dumps({m: dict(frames_per_s_median=statistics.median(r["frames_per_s"] for r in rs),
                              step_period_us_median=statistics.median(r["step_period_us"] for r in rs),
                              frames_per_s=[r["frames_per_s"] for r in rs], step_period_us=[r["step_period_us"] for r in rs])
                      for m, rs in rows.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", type=int, default=10)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--beside", action="store_true")
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--lens", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(a)
    elif a.kernels:
        kernels(a)
    elif a.beside:
        beside(a)
    else:
        driver_rate(a)


if __name__ == "__main__":
    main()
