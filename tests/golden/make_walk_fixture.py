"""Writes tests/golden/walk_sir_step.npz: the SIR data set of the time-varying-rates tests (data only).

An epidemic of 300 people (5 infected at day 0) simulated day by day with the project's CPU oracle, in which the
transmission rate steps down mid-series: beta = 0.6 on days 1..11, beta = 0.05 on days 12..29, gamma = 0.2 throughout;
observed through a binomial with p = 0.5.  Run from the repository root:
    python tests/golden/make_walk_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import oracle  # noqa: E402

T, STEP_DAY = 30, 12
BETA_EARLY, BETA_LATE, GAMMA = 0.6, 0.05, 0.2


def main():
    beta = np.where(np.arange(T) < STEP_DAY, BETA_EARLY, BETA_LATE)
    x = np.array([[295, 5, 0]], dtype=np.int32)
    rows = [x[0].copy()]
    for p in range(1, T):
        x, _ = oracle.simulate("sir", x, (float(beta[p]), GAMMA), 1.0, 2013, 0, p)
        rows.append(x[0].copy())
    X = np.array(rows, dtype=np.int64)
    Y = np.random.default_rng(13).binomial(X, 0.5).astype(np.float64)
    np.savez(os.path.join(HERE, "walk_sir_step.npz"), X=X, Y=Y, beta=beta, gamma=np.array(GAMMA),
             step_day=np.array(STEP_DAY), population=np.array(300.0), mu=np.array(5.0), probs=np.array(0.5))
    print("wrote walk_sir_step.npz:", Y.shape, "I =", X[:, 1].tolist())


if __name__ == "__main__":
    main()
