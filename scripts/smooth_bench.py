"""The particle smoother on the device (Engine.smooth: a backward pass over the history resident in HBM) against the
route there was before it: Engine.history() to the host, then the numpy restatement (epipf.smooth_history,
backend="numpy").

    python scripts/smooth_bench.py --out profiles/smooth_bench.json

Workload: BASELINE config 2 (benchmark_dataset(2): SIR, N = 10^4, T = 200, population 10^4), one chain and --chains
(256) chains, every chain at the config's theta with its own key.  Device route: Engine.smooth with three quantiles
and with quantiles=None; each timed run is one synchronous call, median of --reps after --warmup, spread =
(max - min) / median.  Host route: the history copy and the numpy backend are timed separately.  At one chain both run
--reps times.  At --chains chains the copy (8 GB at 256) runs --host-reps times and the numpy backend on --host-subset
chains, scaled by chains / subset (it is a loop over chains); the quotient says which parts were scaled.  The device's
results are checked against the host's on the chains the host computed.  Also recorded: the per-day lineage counts of
chain 0 under both lineages.  No ratio is fixed in advance."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stochastic-epidemic-modelling_amd"))

QS = (0.05, 0.5, 0.95)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-subset", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from epipf import _lib, smooth_history
    from epipf.datasets import benchmark_dataset
    from epipf.engine import Engine
    Y, meta = benchmark_dataset(2)
    N, T = meta["N"], Y.shape[0]
    bins = int(meta["n_population"]) + 1
    doc = {"build_id": _lib.build_id(), "config": 2, "N": N, "T": T, "bins": bins, "quantiles": list(QS),
           "reps": args.reps, "warmup": args.warmup, "runs": {}}
    for chains in (1, args.chains):
        eng = Engine(meta["model"], 1, N, T, chains)
        eng.set_observations(Y)
        eng.set_population(meta["n_population"], meta["mu"])
        th = np.repeat(np.asarray(meta["theta"], dtype=np.float64)[None], chains, 0)
        lz, st = eng.run(th, meta["probs"], np.arange(chains) + 1, 0)
        assert np.all(st == 0), st
        run = {"chains": chains, "history_bytes": int(chains) * T * N * 4 * (eng.C + 1)}
        dev_q, run["device_quantiles"] = timed(lambda: eng.smooth(chains, quantiles=QS), args.reps, args.warmup)
        dev_m, run["device_mean_only"] = timed(lambda: eng.smooth(chains, quantiles=None), args.reps, args.warmup)
        _, run["device_reference_lineage"] = timed(lambda: eng.smooth(chains, quantiles=QS, lineage="reference"),
                                                   args.reps, args.warmup)
        _, run["device_predictive"] = timed(lambda: eng.smooth(chains, quantiles=QS, kind="predictive"),
                                            args.reps, args.warmup)
        assert np.array_equal(dev_q.sums, dev_m.sums) and np.array_equal(dev_q.lineages, dev_m.lineages)
        one = chains == 1
        (hid, anc), run["host_copy"] = timed(lambda: eng.history(chains), args.reps if one else args.host_reps,
                                             1 if not one else args.warmup)
        sub = chains if one else min(args.host_subset, chains)
        host, hn = timed(lambda: smooth_history(hid[:sub], anc[:sub], quantiles=QS, bins=bins, backend="numpy"),
                         args.reps if one else args.host_reps, 1)
        for f in ("sums", "quantiles", "lineages"):
            assert np.array_equal(getattr(host, f), getattr(dev_q, f)[:sub]), f
        hn["chains_computed"] = sub
        hn["scaled_median_s"] = hn["median_s"] * chains / sub
        run["host_numpy"] = hn
        run["host_route_s"] = run["host_copy"]["median_s"] + hn["scaled_median_s"]
        run["host_over_device_quantiles"] = run["host_route_s"] / run["device_quantiles"]["median_s"]
        run["copy_alone_over_device_quantiles"] = run["host_copy"]["median_s"] / run["device_quantiles"]["median_s"]
        if one:
            ref = eng.smooth(1, quantiles=None, lineage="reference")
            doc["lineages_chain0"] = {"genealogy": dev_q.lineages[0].tolist(), "reference": ref.lineages[0].tolist()}
        doc["runs"][str(chains)] = run
        del hid, anc
        eng.close()
    print(json.dumps({k: v for k, v in doc.items() if k != "lineages_chain0"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, sort_keys=True) + "\n")    # one line: the lists of times and lineages are long


if __name__ == "__main__":
    main()
