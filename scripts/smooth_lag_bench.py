"""The fixed-lag particle smoother on the device (Engine.smooth(lag=L): one backward window per (chain, day) over the
history resident in HBM) beside the smoother and the predictive cloud, and against the route there was before it:
Engine.history() to the host, then the numpy restatement (epipf.smooth_history, backend="numpy", lag=L).

    python scripts/smooth_lag_bench.py --out profiles/smooth_lag_bench.json

Workload and protocol are scripts/smooth_bench.py's: BASELINE config 2 (SIR, N = 10^4, T = 200, population 10^4), one
chain and --chains (256) chains, every chain at the config's theta with its own key; each timed run is one synchronous
call, median of --reps after --warmup, spread = (max - min) / median.  Device: lag in --lags (1, 10, 30) with three
quantiles and with quantiles=None, then kind="smoothing" and kind="predictive" in the same process.  Host route: the
history copy and the numpy backend are timed separately, per lag; at --chains chains the copy runs --host-reps times
and the numpy backend on --host-subset chains, scaled by chains / subset (it is a loop over chains) and labelled as
scaled.  The device's results are checked against the host's on the chains the host computed.  Also recorded: chain
0's lineage counts per day for every lag and for the smoother.  No time is fixed in advance."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stochastic-epidemic-modelling_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from smooth_bench import QS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--lags", type=int, nargs="+", default=[1, 10, 30])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-subset", type=int, default=4)
    ap.add_argument("--days", type=int, default=0, help="keep only the first DAYS days (a rehearsal; 0: all)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from epipf import _lib, smooth_history
    from epipf.datasets import benchmark_dataset
    from epipf.engine import Engine
    Y, meta = benchmark_dataset(2)
    if args.days:
        Y = Y[:args.days]
    N, T = meta["N"], Y.shape[0]
    bins = int(meta["n_population"]) + 1
    doc = {"build_id": _lib.build_id(), "config": 2, "N": N, "T": T, "bins": bins, "quantiles": list(QS),
           "lags": args.lags, "reps": args.reps, "warmup": args.warmup, "runs": {}, "lineages_chain0": {}}
    for chains in (1, args.chains):
        eng = Engine(meta["model"], 1, N, T, chains)
        eng.set_observations(Y)
        eng.set_population(meta["n_population"], meta["mu"])
        th = np.repeat(np.asarray(meta["theta"], dtype=np.float64)[None], chains, 0)
        lz, st = eng.run(th, meta["probs"], np.arange(chains) + 1, 0)
        assert np.all(st == 0), st
        one = chains == 1
        run = {"chains": chains, "history_bytes": int(chains) * T * N * 4 * (eng.C + 1), "lag": {}}
        _, run["device_smoothing"] = timed(lambda: eng.smooth(chains, quantiles=QS), args.reps, args.warmup)
        _, run["device_predictive"] = timed(lambda: eng.smooth(chains, quantiles=QS, kind="predictive"), args.reps,
                                            args.warmup)
        (hid, anc), run["host_copy"] = timed(lambda: eng.history(chains), args.reps if one else args.host_reps,
                                             1 if not one else args.warmup)
        sub = chains if one else min(args.host_subset, chains)
        for L in args.lags:
            r = {}
            dev_q, r["device_quantiles"] = timed(lambda: eng.smooth(chains, quantiles=QS, lag=L), args.reps, args.warmup)
            dev_m, r["device_mean_only"] = timed(lambda: eng.smooth(chains, quantiles=None, lag=L), args.reps,
                                                 args.warmup)
            assert np.array_equal(dev_q.sums, dev_m.sums) and np.array_equal(dev_q.lineages, dev_m.lineages)
            host, hn = timed(lambda: smooth_history(hid[:sub], anc[:sub], quantiles=QS, bins=bins, backend="numpy", lag=L),
                             args.reps if one else args.host_reps, 1)
            for f in ("sums", "quantiles", "lineages"):
                assert np.array_equal(getattr(host, f), getattr(dev_q, f)[:sub]), (L, f)
            hn["chains_computed"] = sub
            hn["scaled"] = sub != chains
            hn["scaled_median_s"] = hn["median_s"] * chains / sub
            r["host_numpy"] = hn
            r["host_route_s"] = run["host_copy"]["median_s"] + hn["scaled_median_s"]
            r["host_over_device_quantiles"] = r["host_route_s"] / r["device_quantiles"]["median_s"]
            r["copy_alone_over_device_quantiles"] = run["host_copy"]["median_s"] / r["device_quantiles"]["median_s"]
            run["lag"][str(L)] = r
            if one:
                doc["lineages_chain0"][str(L)] = dev_q.lineages[0].tolist()
        if one:
            doc["lineages_chain0"]["smoothing"] = eng.smooth(1, quantiles=None).lineages[0].tolist()
        doc["runs"][str(chains)] = run
        del hid, anc
        eng.close()
    print(json.dumps({k: v for k, v in doc.items() if k != "lineages_chain0"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, sort_keys=True) + "\n")    # one line: the lists of times and lineages are long
    return 0


if __name__ == "__main__":
    sys.exit(main())
