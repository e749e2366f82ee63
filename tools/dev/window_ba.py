"""Device time of the window bundle adjustment (vo_window_ba_dev) and of the window builder (vo_window_from_tracks_dev):
HIP events around each launch (the library's own brackets, Context.prof_enable), median and spread over --repeats calls,
inputs uploaded afresh before every solve (it works in place).

Windows, all W = 8:
  stream    the last window the configuration stream produces -- bench.py's driver leg: 1376 x 1241 synthetic frames,
            2000 keypoints, the device loop with tracks=True for --frames frames; the window is rebuilt from the records the
            run returned, uploaded again, joined by the builder (timed) and solved (timed) with max_iter 10, squared loss
            and Huber 2 px
  smallest  the case table's smallest W = 8 window (tests/window_ba_cases.py: 60 landmarks)
each at S = 1 and S = 16 (the same window in every lane: one workgroup per window, so S = 16 is sixteen workgroups).

    python3 tools/dev/window_ba.py [--frames 14] [--repeats 20] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "visual-odometry-project_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W_IMG, N_KP, WINDOW = 1241, 1376, 2000, 8
K_WINDOW_BA, K_WINDOW_BUILD = 28, 29          # VO_K_WINDOW_BA, VO_K_WINDOW_BUILD (vo_hip.h)


def record_bytes(rec, cap):
    """A TrackRecord back as the bytes the pipeline wrote, padded to the capacity's size."""
    import numpy as np
    from vo._pipeline import TRACK_HEADER
    raw = np.zeros(16 + 48 * cap, np.uint8)
    raw[:16].view(TRACK_HEADER)[0] = (rec.n, rec.step, rec.next_id, rec.seq)
    body = np.asarray(rec).tobytes()
    raw[16:16 + len(body)] = np.frombuffer(body, np.uint8)
    return raw


def timed(ctx, kernel, call, before, repeats, warmup=2):
    """Median / min / max device milliseconds per call of `call` (all its launches of `kernel` summed)."""
    ms = []
    for k in range(warmup + repeats):
        before()
        ctx.sync()
        ctx.prof_reset()
        call()
        ctx.sync()
        if k >= warmup:
            ms.append(ctx.prof_read(kernel)[0])
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import window_ba_cases as wc
    from vo import _native, driver
    from vo.landmarks import pack_windows
    from vo.primitives import Sequence
    ctx = _native.Context(0)
    out = {"window": WINDOW, "repeats": a.repeats}

    # ---- the configuration stream's last window ----
    seq = Sequence("synthetic", n_frames=a.frames, height=H, width=W_IMG, channels=1)
    run = driver.run_on_device(seq, n_keypoints=N_KP, klt_win=15, klt_max_level=2, hyp=4000, context=ctx, bootstrap_win=21,
                               bootstrap_max_level=3, bootstrap_threshold=1.0, tracks=True)
    recs = run["observations"][-WINDOW:]
    poses = np.stack([np.concatenate((np.array(r.R_refined), np.array(r.t_refined))) for r in run["results"][-WINDOW:]])
    cap = max(len(r) for r in recs)
    d_recs = [ctx.to_device(record_bytes(r, cap)) for r in recs]
    L_cap, M_cap = cap, cap * WINDOW
    sizes = dict(head=16, lm_start=4 * (L_cap + 1), obs_slot=4 * M_cap, obs_xy=16 * M_cap, X=24 * L_cap, lm_id=4 * L_cap)
    d = {k: ctx.alloc(v) for k, v in sizes.items()}

    def build():
        ctx.window_from_tracks(d_recs, cap, L_cap, M_cap, d["head"], d["lm_start"], d["obs_slot"], d["obs_xy"], d["X"], d["lm_id"])
    ctx.prof_enable(-1)
    out["build_stream_window"] = timed(ctx, K_WINDOW_BUILD, build, lambda: None, a.repeats)
    head = ctx.download(d["head"], (4,), np.int32)
    L, M = int(head[0]), int(head[1])
    import window_ba_reference as ref
    K = np.asarray(seq.get_camera().intrinsic_matrix, np.float64)
    stream_win = ref.window(K, poses, ctx.download(d["X"], (L_cap, 3), np.float64)[:L],
                            ctx.download(d["lm_start"], (L_cap + 1,), np.int32)[:L + 1],
                            ctx.download(d["obs_slot"], (M_cap,), np.int32)[:M], ctx.download(d["obs_xy"], (M_cap, 2), np.float64)[:M])
    out["stream_window"] = dict(landmarks=L, observations=M, record_rows=cap, flags=int(head[2]))

    # ---- the solver ----
    small = wc.get("w8_l60_outliers_squared").win
    for label, win in (("stream", stream_win), ("smallest", small)):
        for huber in (0.0, 2.0):
            for S in (1, 16):
                arr = pack_windows([win] * S)
                Lc, Mc = arr["X"].shape[1], arr["obs_slot"].shape[1]
                cnt = np.zeros((S, 4), np.int32)
                cnt[:, :2] = arr["counts"]
                dd = dict(counts=ctx.to_device(cnt), K=ctx.to_device(arr["K"]), poses=ctx.to_device(arr["poses"]),
                          X=ctx.to_device(arr["X"]), lm_start=ctx.to_device(arr["lm_start"]), obs_slot=ctx.to_device(arr["obs_slot"]),
                          obs_xy=ctx.to_device(arr["obs_xy"]), res=ctx.alloc(40 * S))

                def reset():
                    ctx.upload(dd["poses"], arr["poses"])
                    ctx.upload(dd["X"], arr["X"])

                def solve():
                    ctx.window_ba_dev(S, WINDOW, Lc, Mc, dd["counts"], dd["K"], dd["poses"], dd["X"], dd["lm_start"], dd["obs_slot"],
                                      dd["obs_xy"], dd["res"], huber_px=huber, max_iter=10)
                t = timed(ctx, K_WINDOW_BA, solve, reset, a.repeats)
                res = ctx.download(dd["res"], (S,), _native.BA_RESULT)[0]
                t.update(landmarks=len(win.X), observations=len(win.obs_slot), status=int(res["status"]),
                         iterations=int(res["iterations"]), trials=int(res["trials"]), cost0=float(res["cost0"]),
                         cost=float(res["cost"]))
                if res["trials"] > 0:
                    t["ms_per_trial"] = round(t["median_ms"] / int(res["trials"]), 4)
                out["solve_%s_huber%g_S%d" % (label, huber, S)] = t
                for p in dd.values():
                    ctx.free(p)
    for k, v in out.items():
        print(k, v)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
