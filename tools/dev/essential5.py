"""Device time of the five-point hypotheses and their scoring (vo_essential_hypotheses) beside the 8-point ones
(vo_fundamental_hypotheses) on the same inputs, and the whole RANSAC calls on the loop test's scene.

  kernels   2048 samples x 2000 correspondences at 1376 x 1241 geometry (the synthetic stream's camera, a forward motion,
            0.3 px noise, 30 % gross outliers): HIP events around each launch (the library's own brackets,
            Context.prof_enable; VO_K_TWOVIEW_HYP / VO_K_TWOVIEW_SCORE), median of --repeats calls; per sample and, for the
            five-point kernels, per solution (every real root is a solution that is scored)
  loops     Context.essential_ransac against Context.fundamental_ransac on tests/essential5_cases.py's scene(200, 21), the
            same generator, threshold and budget: host wall time of the whole call, median of --repeats

    python3 tools/dev/essential5.py [--repeats 20] [--json OUT]
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

H, W, N, HYP = 1241, 1376, 2000, 2048


def big_scene(K, seed=5):
    import numpy as np
    import essential5_cases as cases
    rng = np.random.default_rng(seed)
    R = cases._rodrigues(np.deg2rad(1.5) * np.array([0.1, 1.0, 0.05]) / np.linalg.norm([0.1, 1.0, 0.05]))
    t = np.array([0.1, -0.02, -1.0])
    rays = np.stack([rng.uniform(-0.6, 0.6, N), rng.uniform(-0.55, 0.55, N), np.ones(N)], axis=1)
    X = rays * rng.uniform(5.0, 40.0, N)[:, None]
    x1, x2 = X @ K.T, (X @ R.T + t) @ K.T
    x1, x2 = x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:]
    x1 += rng.normal(0, 0.3, x1.shape)
    x2 += rng.normal(0, 0.3, x2.shape)
    bad = rng.random(N) < 0.3
    x2[bad] = np.stack([rng.uniform(0, W, bad.sum()), rng.uniform(0, H, bad.sum())], axis=1)
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2)


def stats(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import essential5_cases as cases
    from vo import _native, synthetic
    ctx = _native.Context(0)
    K = np.ascontiguousarray(synthetic.Stream(3, H, W).K, dtype=np.float64)
    x1, x2 = big_scene(K)
    s5 = _native.rng_choice(_native.Pcg64.from_generator(np.random.default_rng(2023)), N, 5, HYP)
    s8 = _native.rng_choice(_native.Pcg64.from_generator(np.random.default_rng(2023)), N, 8, HYP)
    out = {"N": N, "Hyp": HYP, "repeats": a.repeats}
    ctx.prof_enable()

    def kernels(call):
        hyp, score = [], []
        for k in range(2 + a.repeats):
            ctx.sync()
            ctx.prof_reset()
            r = call()
            ctx.sync()
            if k >= 2:
                hyp.append(ctx.prof_read(_native.K_TWOVIEW_HYP)[0])
                score.append(ctx.prof_read(_native.K_TWOVIEW_SCORE)[0])
        return r, stats(hyp), stats(score)

    r5, h5, sc5 = kernels(lambda: ctx.essential_hypotheses(x1, x2, K, K, s5, 1.0, error_kind=1, want_masks="packed"))
    r8, h8, sc8 = kernels(lambda: ctx.fundamental_hypotheses(x1, x2, s8, 1.0, True, 1, want_masks="packed"))
    n_sol = int(r5[1].sum())
    out["five_point"] = dict(hyp_ms=h5, score_ms=sc5, solutions=n_sol, samples_with_solution=int((r5[1] > 0).sum()),
                             hyp_us_per_sample=round(1e3 * h5["median"] / HYP, 4),
                             score_us_per_solution=round(1e3 * sc5["median"] / max(n_sol, 1), 5),
                             score_us_per_sample=round(1e3 * sc5["median"] / HYP, 4))
    out["eight_point"] = dict(hyp_ms=h8, score_ms=sc8, hyp_us_per_sample=round(1e3 * h8["median"] / HYP, 4),
                              score_us_per_sample=round(1e3 * sc8["median"] / HYP, 4))
    ctx.prof_disable()

    lx1, lx2, LK, _, _, _ = cases.scene(200, 21)

    def wall(call):
        ms = []
        for k in range(2 + a.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            r = call()
            ctx.sync()
            if k >= 2:
                ms.append(1e3 * (time.perf_counter() - t0))
        return r, stats(ms)

    r, w5 = wall(lambda: ctx.essential_ransac(lx1, lx2, LK, LK, 0.81, np.random.default_rng(2023), max_iterations=2000))
    out["essential_ransac"] = dict(wall_ms=w5, iterations=r[2]["iterations"], best_count=r[2]["best_count"])
    r, w8 = wall(lambda: ctx.fundamental_ransac(lx1, lx2, 0.81, np.random.default_rng(2023), normalize_samples=True,
                                                error_kind=1, max_iterations=2000))
    out["fundamental_ransac"] = dict(wall_ms=w8, iterations=r[2]["iterations"], best_count=r[2]["best_count"],
                                     finished_by_host=r[2]["finished_by_host"])
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
