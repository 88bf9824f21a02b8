"""Writes tests/golden/if2_sub_small.npz: the small subgroup data sets of the iterated-filtering tests (data only).

For G = 2, 3, 4: an epidemic of a few hundred people in G groups simulated day by day for 20 days with the project's CPU
oracle ("sir_subgroups", key 99, filter index 0, day p at step p) at the true theta, observed through a binomial with
p = 0.5.  Stored per G as g<G>_X, g<G>_Y [20, 3G], g<G>_theta (beta row-major, then gamma), g<G>_population, g<G>_mu,
and probs.  The sir_subgroups2 tests observe the sums of Y's columns over the groups.  Run from the repository root:
    python tests/golden/make_if2_sub_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import oracle  # noqa: E402

DAYS = 20
GAMMA = 0.35
SETS = {
    2: dict(beta=[[1.2, 0.3], [0.3, 0.9]], population=(120, 180), infected=(3, 4)),
    3: dict(beta=[[1.3, 0.3, 0.2], [0.3, 1.1, 0.3], [0.2, 0.3, 1.2]], population=(100, 120, 140), infected=(3, 3, 4)),
    4: dict(beta=[[1.2, 0.3, 0.2, 0.1], [0.3, 1.1, 0.3, 0.2], [0.2, 0.3, 1.3, 0.3], [0.1, 0.2, 0.3, 1.1]],
            population=(90, 100, 110, 120), infected=(3, 3, 3, 4)),
}
# the simulated infected per day, one list per group
EXPECTED_I = {
    2: [[3, 3, 3, 8, 7, 10, 17, 19, 28, 33, 27, 21, 15, 15, 12, 8, 4, 4, 5, 4],
        [4, 5, 6, 11, 11, 13, 19, 33, 38, 45, 43, 42, 38, 28, 21, 15, 15, 12, 10, 8]],
    3: [[3, 4, 6, 12, 11, 11, 12, 12, 13, 17, 16, 12, 10, 11, 8, 3, 1, 1, 3, 5],
        [3, 4, 4, 11, 13, 16, 14, 14, 13, 16, 21, 20, 15, 12, 12, 8, 6, 8, 6, 6],
        [4, 6, 6, 9, 11, 14, 22, 32, 32, 32, 26, 22, 15, 10, 7, 4, 3, 5, 4, 5]],
    4: [[3, 4, 4, 2, 2, 0, 2, 6, 6, 7, 7, 4, 4, 5, 1, 2, 1, 1, 2, 3],
        [3, 4, 8, 9, 5, 5, 5, 5, 8, 8, 13, 13, 9, 5, 3, 4, 2, 2, 3, 2],
        [3, 4, 4, 6, 8, 8, 12, 10, 7, 9, 5, 6, 2, 4, 4, 2, 2, 4, 6, 6],
        [4, 5, 7, 8, 10, 9, 8, 8, 8, 6, 5, 5, 2, 2, 1, 2, 0, 0, 0, 2]],
}


def epidemic(G):
    s = SETS[G]
    x = np.zeros((1, 3 * G), dtype=np.int32)
    for g in range(G):
        x[0, 3 * g] = s["population"][g] - s["infected"][g]
        x[0, 3 * g + 1] = s["infected"][g]
    rows = [x[0].copy()]
    for p in range(1, DAYS):
        x, _ = oracle.simulate("sir_subgroups", x, (np.array(s["beta"]), GAMMA), 1.0, 99, 0, p)
        rows.append(x[0].copy())
    return np.array(rows, dtype=np.int64)


def main():
    out = dict(probs=np.array(0.5))
    for G, s in SETS.items():
        X = epidemic(G)
        got = [X[:, 3 * g + 1].tolist() for g in range(G)]
        assert got == EXPECTED_I[G], (G, got)
        Y = np.random.default_rng(5 + G).binomial(X, 0.5).astype(np.float64)
        out.update({f"g{G}_X": X, f"g{G}_Y": Y, f"g{G}_theta": np.append(np.array(s["beta"]).reshape(-1), GAMMA),
                    f"g{G}_population": np.array(s["population"], dtype=np.float64),
                    f"g{G}_mu": np.array(s["infected"], dtype=np.float64)})
        print(f"G = {G}: I =", got)
    np.savez(os.path.join(HERE, "if2_sub_small.npz"), **out)
    print("wrote if2_sub_small.npz")


if __name__ == "__main__":
    main()
