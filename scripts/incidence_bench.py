"""The incidence filter on the device (Engine.run_incidence) beside the state filter (Engine.run) on the
same build in the same process.

    python scripts/incidence_bench.py --out profiles/incidence_bench.json

Workload: BASELINE config 2's shape (SIR, N = 10^4, population 10^4, --chains (64) chains at the config's theta, every
chain under its own key), D = 198 days so that both filters run T = 200 rows.  The reports are the day-to-day flows of
one epidemic simulated on the device at the config's theta from (9980, 20, 0) (Engine.simulate, key 1, step p), thinned by
RandomState(1).binomial(flows, probs).  Protocol: a host clock around each synchronous call, the median of --reps (5)
after --warmup (1), spread = (max - min) / median.
  state filter            Engine.run on the config's observations
  one column              Engine.run_incidence on the infections alone
  two columns             on infections and removals
  weekly, cumulated       7-day totals of both columns on every seventh day, cumulate=True
The ratios to the state filter are recorded, not asserted."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stochastic-epidemic-modelling_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from smooth_bench import timed  # noqa: E402


def reports(eng, theta, probs, days):
    x = np.array([[9980, 20, 0]], dtype=np.int32)
    rows = [x[0].copy()]
    for p in range(1, days + 1):
        x, _ = eng.simulate(x, theta, 1.0, key=1, filter_index=0, step=p)
        rows.append(x[0].copy())
    X = np.array(rows, dtype=np.int64)
    flows = np.stack([X[:-1, 0] - X[1:, 0], X[1:, 2] - X[:-1, 2]], axis=1)
    rs = np.random.RandomState(1)
    daily = rs.binomial(flows, probs).astype(np.float64)
    weeks = days // 7
    weekly = np.full((days, 2), np.nan)
    weekly[6:7 * weeks:7] = rs.binomial(flows[:7 * weeks].reshape(weeks, 7, 2).sum(axis=1), probs)
    return daily, weekly


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--days", type=int, default=198, help="D (a rehearsal: fewer)")
    ap.add_argument("--particles", type=int, default=0, help="override N (a rehearsal; 0: the config's)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from epipf import _lib
    from epipf.datasets import benchmark_dataset
    from epipf.engine import Engine
    Y, meta = benchmark_dataset(2)
    D = args.days
    T = D + 2
    Y = Y[:T]
    N, S = args.particles or meta["N"], args.chains
    theta = np.tile(np.asarray(meta["theta"], dtype=np.float64), (S, 1))
    eng = Engine(meta["model"], 1, N, T, S)
    eng.set_observations(Y)
    eng.set_population(meta["n_population"], meta["mu"])
    daily, weekly = reports(eng, meta["theta"], meta["probs"], D)
    one = daily.copy()
    one[:, 1] = np.nan
    keys = np.arange(S, dtype=np.uint64) + 1
    doc = {"build_id": _lib.build_id(), "config": 2, "N": N, "T": T, "D": D, "chains": S, "reps": args.reps,
           "warmup": args.warmup, "reports_total": daily.sum(axis=0).tolist()}
    (lz, st), doc["state_filter"] = timed(lambda: eng.run(theta, meta["probs"], keys, 0), args.reps, args.warmup)
    doc["state_filter"]["ok_chains"] = int((st == 0).sum())
    base = doc["state_filter"]["median_s"]
    for name, counts, cum in (("one_column", one, False), ("two_columns", daily, False), ("weekly_cumulated", weekly, True)):
        (lz, st), r = timed(lambda: eng.run_incidence(theta, meta["probs"], keys, 0, counts, cumulate=cum), args.reps,
                            args.warmup)
        r["ok_chains"] = int((st == 0).sum())
        r["loglik_chain0"] = float(lz[0, -1])
        r["over_state_filter"] = r["median_s"] / base
        r["particle_steps_per_s"] = S * N * T / r["median_s"]
        doc[name] = r
    eng.close()
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, sort_keys=True) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
