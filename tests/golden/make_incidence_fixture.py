"""Writes tests/golden/incidence_small.npz: the reported case counts of the incidence tests (data only).

Every series is the true day-to-day flows of a simulated epidemic of 300 people, thinned by a binomial with p = 0.5:
  sir      [24, 2]  infections, removals of the SIR epidemic X in if2_sir_small.npz (make_if2_fixture.py), rng 7
  seir     [24, 3]  exposures, onsets, removals of a SEIR epidemic from (295, 0, 5, 0) at theta (0.9, 0.6, 0.3),
                    simulated day by day with the project's CPU oracle (key 99, filter index 0, step p), rng 9
  weekly   [21, 2]  7-day sums of the SIR flows, reported on days 7, 14, 21 (NaN elsewhere), rng 8
  threeday [12, 2]  3-day sums of the SIR flows, reported on days 3, 6, 9, 12 (NaN elsewhere), rng 10
Run from the repository root:
    python tests/golden/make_incidence_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import oracle  # noqa: E402

SEIR_THETA = (0.9, 0.6, 0.3)
P = 0.5


def sir_flows(X):
    return np.stack([X[:-1, 0] - X[1:, 0], X[1:, 2] - X[:-1, 2]], axis=1)


def seir_flows(X):
    return np.stack([X[:-1, 0] - X[1:, 0], (X[1:, 2] + X[1:, 3]) - (X[:-1, 2] + X[:-1, 3]), X[1:, 3] - X[:-1, 3]],
                    axis=1)


def blocks(flows, width, days, seed):
    """width-day sums of the first `days` rows, thinned, on the last day of each block; NaN elsewhere."""
    sums = flows[:days].reshape(days // width, width, -1).sum(axis=1)
    out = np.full((days, flows.shape[1]), np.nan)
    out[width - 1::width] = np.random.default_rng(seed).binomial(sums, P)
    return out


def main():
    z = np.load(os.path.join(HERE, "if2_sir_small.npz"))
    X = z["X"].astype(np.int64)
    fs = sir_flows(X)
    assert fs.shape == (24, 2) and (fs >= 0).all()
    sir = np.random.default_rng(7).binomial(fs, P).astype(np.float64)
    x = np.array([[295, 0, 5, 0]], dtype=np.int32)
    rows = [x[0].copy()]
    for p in range(1, 25):
        x, _ = oracle.simulate("seir", x, SEIR_THETA, 1.0, 99, 0, p)
        rows.append(x[0].copy())
    X4 = np.array(rows, dtype=np.int64)
    fe = seir_flows(X4)
    assert fe.shape == (24, 3) and (fe >= 0).all()
    seir = np.random.default_rng(9).binomial(fe, P).astype(np.float64)
    np.savez(os.path.join(HERE, "incidence_small.npz"), sir=sir, seir=seir, weekly=blocks(fs, 7, 21, 8),
             threeday=blocks(fs, 3, 12, 10), sir_flows=fs, seir_flows=fe, seir_states=X4, seir_theta=np.array(SEIR_THETA),
             theta=z["theta"], population=np.array(300.0), mu=np.array(5.0), probs=np.array(P))
    print("wrote incidence_small.npz: sir", sir.sum(axis=0), "seir", seir.sum(axis=0))


if __name__ == "__main__":
    main()
