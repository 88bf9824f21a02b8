"""Writes tests/golden/if2_sir_small.npz: the small SIR data set of the iterated-filtering tests (data only).

An epidemic of 300 people (5 infected at day 0) simulated day by day with the project's CPU oracle at the true
theta = (0.8, 0.3), observed through a binomial with p = 0.5.  Run from the repository root:
    python tests/golden/make_if2_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import oracle  # noqa: E402

TRUE_THETA = (0.8, 0.3)
EXPECTED_I = [5, 7, 9, 16, 19, 22, 43, 61, 70, 81, 92, 90, 84, 71, 61, 55, 42, 36, 29, 22, 19, 18, 18, 13, 8]


def main():
    x = np.array([[295, 5, 0]], dtype=np.int32)
    rows = [x[0].copy()]
    for p in range(1, 25):
        x, _ = oracle.simulate("sir", x, TRUE_THETA, 1.0, 99, 0, p)
        rows.append(x[0].copy())
    X = np.array(rows, dtype=np.int64)
    assert X[:, 1].tolist() == EXPECTED_I, X[:, 1].tolist()
    Y = np.random.default_rng(5).binomial(X, 0.5).astype(np.float64)
    np.savez(os.path.join(HERE, "if2_sir_small.npz"), X=X, Y=Y, theta=np.array(TRUE_THETA), population=np.array(300.0),
             mu=np.array(5.0), probs=np.array(0.5))
    print("wrote if2_sir_small.npz:", Y.shape, "I =", X[:, 1].tolist())


if __name__ == "__main__":
    main()
