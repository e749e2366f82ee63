"""Batched Shi-Tomasi (vo_good_features_batch_dev) at the configuration frame size, 1376 x 1241, 2000 corners, defaults
otherwise, for S = 1, 4, 16 distinct synthetic frames, in one process, alternating:
  batch_dev  one vo_good_features_batch_dev call, frames and corners resident in device memory (nothing crosses PCIe)
  batch      one vo_good_features_batch call (frames up, corners down)
  one_each   S vo_good_features calls (frames up, one count read-back that sizes the sort, counts and corners down, each)
Times are device events on the context's stream (a stream of torch's, handed to the context) around each case, read after
a synchronise; per case --warmup untimed calls, then --repeats timed ones: median and spread.  batch against one_each is
the like-for-like pair (both move the frames and the corners); batch_dev is what a device-resident caller pays.
Also prints, per image, what d_info recorded: candidates, path, round launches used.

    python3 tools/dev/good_features_batch.py [--sequences 1 4 16] [--repeats 20] [--json OUT]
    python3 tools/dev/good_features_batch.py --trace 16 [--iters 10]   # batch_dev only, untimed: for rocprofv3 --kernel-trace
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

H, W, N, QUALITY, MIN_DIST, BLOCK = 1241, 1376, 2000, 0.01, 8, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scenarios import synthetic_image
    from vo import _native
    if not torch.cuda.is_available():
        raise SystemExit("good_features_batch: no GPU (there is no CPU path to time)")
    S_max = a.trace or max(a.sequences)
    frames = np.stack([synthetic_image(H, W, 17 + q, block=9) for q in range(S_max)])
    stream = torch.cuda.Stream()
    ctx = _native.Context(0, stream=stream.cuda_stream)
    rows = ctx.good_features_capacity(H, W, N)
    d_imgs = ctx.to_device(frames)
    d_xy, d_n = ctx.alloc(S_max * rows * 8), ctx.alloc(S_max * 4)
    d_over, d_info = ctx.alloc(S_max * 4), ctx.alloc(S_max * 16)

    def batch_dev(S):
        ctx.good_features_batch_dev(d_imgs, H * W, S, H, W, d_xy, rows, d_n, None, 0, N, QUALITY, MIN_DIST, BLOCK, d_over, d_info)

    def batch(S):
        return ctx.good_features_batch(frames[:S], None, N, QUALITY, MIN_DIST, BLOCK)

    def one_each(S):
        return [ctx.good_features(frames[q], None, N, QUALITY, MIN_DIST, BLOCK) for q in range(S)]

    if a.trace:
        for _ in range(a.iters):
            batch_dev(a.trace)
        ctx.sync()
        print("batch_dev calls", a.iters, "S", a.trace)
        ctx.close()
        return
    cases = dict(batch_dev=batch_dev, batch=batch, one_each=one_each)
    out = []
    for S in a.sequences:
        got, ref = batch(S), one_each(S)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref)), "the batch differs from the one-image calls"
        batch_dev(S)
        ctx.sync()
        info = ctx.download(d_info, (S, 4), np.int32)
        cnt = ctx.download(d_n, (S,), np.int32)
        assert cnt.tolist() == [len(r) for r in ref] and not ctx.download(d_over, (S,), np.int32).any()
        for fn in cases.values():
            for _ in range(a.warmup):
                fn(S)
        ctx.sync()
        ms = {k: [] for k in cases}
        for _ in range(a.repeats):
            for k, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(S)
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        row = dict(S=S, corners=cnt.tolist(), candidates=info[:, 0].tolist(), path=info[:, 1].tolist(), rounds=info[:, 2].tolist())
        for k, v in ms.items():
            v = sorted(v)
            row[k] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))
        row["batch_over_one_each"] = round(row["batch"]["median_ms"] / row["one_each"]["median_ms"], 3)
        row["batch_dev_ms_per_image"] = round(row["batch_dev"]["median_ms"] / S, 4)
        out.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
