"""Generate tests/golden/wide_groups_golden.npz: the UNMODIFIED reference particle filter at G = 5, 6 and 8 groups,
driven by the keyed-stream shim of make_golden.py (same shim, same conventions, same record layout as its filter
cases).  Runs only in the build container (the reference is never shipped).

    python tests/golden/make_golden_wide.py [--reference /root/reference]

Cases (all N = 48, T = 5, npop = 300 and mu = 6 per group, beta = RandomState(100 + G).uniform(0.5, 3, (G, G)),
gamma = 0.7, probs = 0.1, key 900 + G, filter index 0):
    G = 6  SIR_SUBGROUPS   Y = tile(Y0, (1, G))
    G = 5  SIR_SUBGROUPS2  Y = Y0 * G
    G = 8  SIR_SUBGROUPS   Y = tile(Y0, (1, G))
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import S, check_numpy_identities, install_shim, save  # noqa: E402

Y0 = np.array([[28, 1, 0], [26, 2, 1], [22, 4, 3], [17, 6, 6], [12, 7, 10]], dtype=np.float64)
CASES = [(6, "SIR_SUBGROUPS"), (5, "SIR_SUBGROUPS2"), (8, "SIR_SUBGROUPS")]
N, GAMMA, PROBS = 48, 0.7, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import matplotlib
    matplotlib.use("Agg")
    import gillespie_algo as ga
    import pmcmc as pm

    check_numpy_identities()
    pf = install_shim(pm, ga)
    out = {}
    for G, model in CASES:
        beta = np.random.RandomState(100 + G).uniform(0.5, 3.0, (G, G))
        Y = np.tile(Y0, (1, G)) if model == "SIR_SUBGROUPS" else Y0 * G
        npop, mu = np.full(G, 300.0), np.full(G, 6.0)
        S.key = 900 + G
        S.next_f = 0
        t0 = time.time()
        z, hid, anc = pf(Y, getattr(pm.ModelType, model), (beta, GAMMA), False, PROBS, N, npop, mu, 1)
        dt = time.time() - t0
        assert z is not None, f"G={G} {model}: the reference filter degenerated"
        assert np.array_equal(hid, np.round(hid)) and np.array_equal(anc, np.round(anc))
        out[f"wide_{model.lower()}_g{G}"] = dict(
            Y=Y, model=model, obs=False, probs=PROBS, N=N, npop=npop, mu=mu, key=900 + G, f=0, seconds=dt,
            beta=beta, gamma=GAMMA, status=0, zetas=z, hidden=hid.astype(np.int32), ancestry=anc.astype(np.int32))
        print(f"wide G={G} {model}: {dt:.1f}s", flush=True)
    save(out, os.path.join(HERE, "wide_groups_golden.npz"))


if __name__ == "__main__":
    main()
