"""The inputs of the incidence tests (a helper, no test itself): tests/test_incidence_restatement.py pins on the CPU what
each case contains, tests/test_gpu_incidence.py runs the same inputs on the device against the restatement
(tests/incidence_restatement.py).  A restated pass is computed once per process and shared."""
import os

import numpy as np

import incidence_restatement as ir
from conftest import GOLDEN

KEY, F = 11, 3
N, D = 65, 12
NPOP, MU = 300.0, 5.0
THETA = {"sir": (0.8, 0.3), "seir": (0.9, 0.6, 0.3)}
PROBS = {False: 0.5, True: 0.2}                         # binomial p / normal noise ratio
COLUMNS = {"sir": [(0,), (1,), (0, 1)], "seir": [(0,), (1,), (2,), (0, 1, 2)]}
# the batch of three chains: theta, probs, key (the second dies at its step 3, the others are untouched)
BATCH = [((0.8, 0.3), 0.5, 11), ((0.05, 0.3), 0.4, 1), ((1.6, 0.3), 0.6, 2)]

_FX = {}
_PASSES = {}


def fixture():
    if not _FX:
        z = np.load(os.path.join(GOLDEN, "incidence_small.npz"))
        _FX.update({k: z[k] for k in z.files})
    return _FX


def only(counts, cols):
    """counts with every column outside cols unreported."""
    out = np.full(counts.shape, np.nan)
    out[:, list(cols)] = counts[:, list(cols)]
    return out


def daily(model, observations, cols, days=D):
    """The first `days` daily reports of the model: thinned counts for the binomial model, the true flows for the
    normal one."""
    fx = fixture()
    src = fx[model + "_flows"].astype(np.float64) if observations else fx[model]
    return only(src[:days], cols)


def mixed():
    """Infections daily, removals every third day as 3-day totals (for cumulate=True)."""
    fx = fixture()
    out = fx["threeday"].copy()
    out[:, 0] = fx["sir"][:D, 0]
    return out


def restate(counts, model, theta, observations, probs, n=N, key=KEY, f=F, cumulate=False):
    """incidence_restatement.one_pass at population 300, mu 5, cached on its arguments."""
    counts = np.asarray(counts, dtype=np.float64)
    k = (counts.tobytes(), counts.shape, model, tuple(theta), bool(observations), float(probs), int(n), int(key), int(f),
         bool(cumulate))
    if k not in _PASSES:
        _PASSES[k] = ir.one_pass(counts, model, theta, observations, probs, n, NPOP, MU, key, f, cumulate=cumulate)
    return _PASSES[k]


# ------------------------------------------------------------------------------------------- the pinned MH run
# 20 iterations of two chains at N = 65, D = 12 on the daily SIR reports.  The seed is pinned so that every decision
# has |log u - (lz_new - lz_old)| > 1e-6 (tests/test_incidence_host.py checks that condition on the input): the device
# and the restatement agree on log_zetas to rtol 1e-9 only, which then cannot flip an acceptance.
MCMC = dict(parameters=(0.8, 0.3), h=0.03, iters=20, chains=2, seed=5, filter_index_start=7)


def mcmc_run(**kw):
    import epipf
    args = dict(MCMC)
    args.update(kw)
    return epipf.incidence_mcmc(daily("sir", False, (0, 1)), "sir", args.pop("parameters"), args.pop("h"),
                                flows=("infections", "removals"), probs=0.5, n_particles=N, n_population=NPOP, mu=MU,
                                **args)
