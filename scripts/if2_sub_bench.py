"""Iterated filtering of the subgroup models (Engine.if2_subgroups) against the plain filter on the
same build.

    python scripts/if2_sub_bench.py --out profiles/if2_sub_bench.json

Workload: BASELINE config 5's shape (benchmark_dataset(5): SIR_SUBGROUPS, G = 2, N = 10^4, T = 14), --searches (64)
searches of --iterations (5) iterations, every swarm starting at the config's theta with half-widths of 2 % of it (no
cooling: the cost does not depend on it).  Yardsticks, in the same process: Engine.run of the same number of chains at
that theta on the one-lane layout (set_lanes(1), the layout the IF2 kernels use) and on the engine's default layout.
G = 3 and G = 4 run on synthetic data of the same N and T: an epidemic simulated day by day on the device
(Engine.simulate) with beta = 4 on the diagonal and 1 beside it, gamma = 1, thinned with p = 0.1.  Each timed run is one
synchronous call, median of --reps after --warmup, spread = (max - min) / median.  Printed: ms per iteration,
particle-steps/s, and the quotients.  No ratio is fixed in advance; nothing here is traced or profiled."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stochastic-epidemic-modelling_amd"))


def timed(fn, reps, warmup):
    out, ts = None, []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if r >= warmup:
            ts.append(dt)
    med = statistics.median(ts)
    return out, dict(seconds=ts, median_s=med, spread=(max(ts) - min(ts)) / med)


def synthetic(G, N, T):
    """(Y [T, 3G], meta) of G groups at config 5's N and T."""
    from epipf.engine import Engine
    npop = [2030 + 500 * g for g in range(G)]
    mu = [30 + 5 * g for g in range(G)]
    beta = np.where(np.eye(G, dtype=bool), 4.0, 1.0)
    eng = Engine("sir_subgroups", G, 64, T, 1)
    x = np.zeros((1, 3 * G), dtype=np.int32)
    for g in range(G):
        x[0, 3 * g], x[0, 3 * g + 1] = npop[g] - mu[g], mu[g]
    rows = [x[0].copy()]
    for p in range(1, T):
        x, _ = eng.simulate(x, (beta, 1.0), 1.0, key=5, filter_index=0, step=p)
        rows.append(x[0].copy())
    eng.close()
    Y = np.random.RandomState(5).binomial(np.array(rows), 0.1).astype(np.float64)
    return Y, dict(model="sir_subgroups", n_population=npop, mu=mu, theta=list(beta.reshape(-1)) + [1.0], probs=0.1, N=N)


def measure(Y, meta, G, S, M, reps, warmup):
    from epipf.engine import Engine
    N, T = meta["N"], Y.shape[0]
    theta = np.asarray(meta["theta"], dtype=np.float64)
    eng = Engine(meta["model"], G, N, T, S)
    eng.set_observations(Y)
    eng.set_population(meta["n_population"], meta["mu"])
    keys = np.arange(S) + 1
    swarm = np.tile(theta, (S, N, 1))
    hw = np.tile(0.02 * theta, (M, 1))
    (_, _, _, done, st), t_if2 = timed(lambda: eng.if2_subgroups(swarm, hw, meta["probs"], keys, 0), reps, warmup)
    assert np.all(st == 0) and np.all(done == M), (st, done)
    thetas = np.tile(theta, (S, 1))
    eng.set_lanes(1)
    (_, rst), t_one = timed(lambda: eng.run(thetas, meta["probs"], keys, 0), reps, warmup)
    assert np.all(rst == 0), rst
    one_lane = eng.stats()["last_lanes"]
    eng.set_lanes(0)
    (_, rst), t_def = timed(lambda: eng.run(thetas, meta["probs"], keys, 0), reps, warmup)
    assert np.all(rst == 0), rst
    s = eng.stats()
    eng.close()
    steps = S * N * T
    per_iter = t_if2["median_s"] / M
    return {"G": G, "N": N, "T": T, "if2": t_if2, "filter_one_lane": t_one, "filter_default": t_def,
            "filter_one_lane_lanes": int(one_lane), "filter_default_lanes": int(s["last_lanes"]),
            "filter_default_fused": int(s["last_fused"]),
            "if2_ms_per_iteration": 1e3 * per_iter, "if2_particle_steps_per_s": steps / per_iter,
            "filter_one_lane_ms": 1e3 * t_one["median_s"], "filter_default_ms": 1e3 * t_def["median_s"],
            "iteration_over_filter_one_lane": per_iter / t_one["median_s"],
            "iteration_over_filter_default": per_iter / t_def["median_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--searches", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--groups", default="2,3,4", help="G = 2 is config 5; 3 and 4 are synthetic")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from epipf import _lib
    from epipf.datasets import benchmark_dataset
    Y5, meta5 = benchmark_dataset(5)
    doc = {"build_id": _lib.build_id(), "config": 5, "searches": args.searches, "iterations": args.iterations,
           "half_width_fraction": 0.02, "reps": args.reps, "warmup": args.warmup, "sir_iteration_over_filter": 1.36,
           "results": []}
    for G in [int(g) for g in args.groups.split(",")]:
        Y, meta = (Y5, meta5) if G == 2 else synthetic(G, meta5["N"], Y5.shape[0])
        try:
            r = measure(Y, meta, G, args.searches, args.iterations, args.reps, args.warmup)
        except AssertionError as e:                      # a search or a filter died on this data: nothing to time
            r = {"G": G, "not_measured": f"status / iterations_done {e}"}
        r["data"] = "benchmark_dataset(5)" if G == 2 else "synthetic (see the module docstring)"
        doc["results"].append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, sort_keys=True, indent=1) + "\n")


if __name__ == "__main__":
    main()
