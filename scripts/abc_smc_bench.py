"""ABC-SMC on MI355X against the rejection sampler at the same final threshold, one JSON line.

Workload: the reference's ABC setting -- the abc_noisy_150 observations (tests/golden/abc_golden.npz, T = 15), priors
beta, gamma ~ U[0, 5], a schedule ending at threshold 80.  Reports trials and wall time per generation, trials/s,
the total trials per accepted sample next to the rejection sampler's (epipf_abc at the final threshold), and the wall
time of an epipf_abc_smc_weights call (copies in and out included) at N = N_prev in {1024, 16384, 65536}.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stochastic-epidemic-modelling_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[400.0, 250.0, 150.0, 100.0, 80.0])
    ap.add_argument("--kernel-scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0)
    args = ap.parse_args()
    from epipf.abc import abc_smc
    from epipf.engine import get_engine
    Y = np.load(os.path.join(REPO, "tests", "golden", "abc_golden.npz"))["abc_noisy_150/Y"]
    pr = {"beta": [0.0, 5.0], "gamma": [0.0, 5.0]}
    n = args.samples
    kw = dict(kernel_scale=args.kernel_scale, key=2024, batch=args.batch)
    abc_smc(Y, n, args.thresholds, pr, run_index=999, **kw)                        # warm-up
    eng = get_engine("sir", 1, 1, 1, 1)
    runs = []
    for r in range(args.runs):
        t0 = time.perf_counter()
        res = abc_smc(Y, n, args.thresholds, pr, run_index=r, **kw)
        wall = time.perf_counter() - t0
        runs.append(dict(wall_s=wall, total_trials=res["total_trials"], ess=res["ess"],
                         generations=[dict(threshold=g["threshold"], trials=g["trials"], seconds=g["seconds"])
                                      for g in res["generations"]]))
    rej = []
    for r in range(args.runs):
        t0 = time.perf_counter()
        _, _, trials, acc = eng.abc(Y, n, args.thresholds[-1], pr, 2024, 100 + r, batch=args.batch)
        assert acc == n
        rej.append(dict(wall_s=time.perf_counter() - t0, trials=trials))
    weights = []
    rng = np.random.RandomState(1)
    for m in (1024, 16384, 65536):
        prev = rng.uniform(0.0, 5.0, (m, 2))
        w = np.full(m, 1.0 / m)
        hw = np.array([0.5, 0.5])
        theta = prev + hw * rng.uniform(-1.0, 1.0, (m, 2))
        eng.abc_smc_weights(theta, prev, w, hw)
        best = np.inf
        for _ in range(3):
            t0 = time.perf_counter()
            eng.abc_smc_weights(theta, prev, w, hw)
            best = min(best, time.perf_counter() - t0)
        weights.append(dict(n=m, n_prev=m, call_ms=best * 1e3, pairs_per_s=m * m / best))
    smc_trials = float(np.mean([r["total_trials"] for r in runs]))
    smc_wall = float(np.mean([r["wall_s"] for r in runs]))
    rej_trials = float(np.mean([r["trials"] for r in rej]))
    rej_wall = float(np.mean([r["wall_s"] for r in rej]))
    print(json.dumps({
        "metric": "abc_smc_trials_per_accepted_sample", "value": smc_trials / n, "unit": "trials/sample",
        "higher_is_better": False,
        "workload": "abc_smc(abc_noisy_150 T=15, n=%d, thresholds=%s, kernel_scale=%g, U[0,5]^2 priors)"
                    % (n, args.thresholds, args.kernel_scale),
        "rejection_trials_per_accepted_sample": rej_trials / n, "trial_saving": rej_trials / smc_trials,
        "smc_wall_s": smc_wall, "rejection_wall_s": rej_wall, "smc_trials_per_s": smc_trials / smc_wall,
        "rejection_trials_per_s": rej_trials / rej_wall, "runs": runs, "rejection_runs": rej,
        "weight_kernel": weights,
    }))


if __name__ == "__main__":
    main()
