"""The inputs of the negative-binomial tests (a helper, no test itself): tests/test_negbin_restatement.py pins on the CPU
what each case contains, tests/test_gpu_negbin.py runs the same inputs on the device against the restatements
(tests/negbin_restatement.py, tests/walk_negbin_restatement.py).  A restated pass is computed once per process and
shared."""
import os

import numpy as np

import incidence_cases as ic
import negbin_restatement as nr
import walk_negbin_restatement as wnr
from conftest import GOLDEN

KEY, F = ic.KEY, ic.F
N, D = ic.N, ic.D
NPOP, MU = ic.NPOP, ic.MU
THETA, COLUMNS = ic.THETA, ic.COLUMNS
RHO, KAPPA = 0.5, 2.0
SERIES = {"sir": "over", "seir": "over_seir"}
# the batch of three chains: theta, probs, dispersion, key.  The second dies at its step 3 by construction: its mean is
# 0, day 1 reports (0, 0) and day 2 reports (2, 3)
BATCH = [((0.8, 0.3), 0.5, 2.0, 11), ((0.8, 0.3), 0.0, 0.7, 1), ((1.6, 0.3), 0.6, 50.0, 2)]
SIZES = [(n, d) for n in (1, 63, 64, 65, 200) for d in (1, 2, 10)]
RW = {"sir": (0.05, 0.0), "seir": (0.05, 0.0, 0.02)}

_FX = {}
_PASSES = {}


def fixture():
    if not _FX:
        z = np.load(os.path.join(GOLDEN, "negbin_small.npz"))
        _FX.update({k: z[k] for k in z.files})
    return _FX


def daily(model, cols, days=D):
    """The first `days` overdispersed daily reports of the model, the columns outside cols unreported."""
    return ic.only(fixture()[SERIES[model]][:days], cols)


def mixed():
    """Infections daily, removals every third day as 3-day totals (for cumulate=True)."""
    out = fixture()["over_threeday"].copy()
    out[:, 0] = fixture()["over"][:D, 0]
    return out


def restate(counts, model, theta, probs=RHO, kappa=KAPPA, n=N, key=KEY, f=F, cumulate=False):
    """negbin_restatement.one_pass at population 300, mu 5, cached on its arguments."""
    counts = np.asarray(counts, dtype=np.float64)
    k = ("pass", counts.tobytes(), counts.shape, model, tuple(theta), float(probs), float(kappa), int(n), int(key), int(f),
         bool(cumulate))
    if k not in _PASSES:
        _PASSES[k] = nr.one_pass(counts, model, theta, probs, kappa, n, NPOP, MU, key, f, cumulate=cumulate)
    return _PASSES[k]


def restate_walk(counts, model, rw, probs=RHO, kappa=KAPPA, n=N, key=KEY, f=F, cumulate=False):
    """walk_negbin_restatement.one_pass from every particle at THETA[model], cached on its arguments."""
    counts = np.asarray(counts, dtype=np.float64)
    k = ("walk", counts.tobytes(), counts.shape, model, tuple(rw), float(probs), float(kappa), int(n), int(key), int(f),
         bool(cumulate))
    if k not in _PASSES:
        start = np.broadcast_to(np.array(THETA[model]), (n, len(THETA[model])))
        _PASSES[k] = wnr.one_pass(counts, model, start, rw, probs, kappa, NPOP, MU, key, f, cumulate=cumulate)
    return _PASSES[k]


# ------------------------------------------------------------------------------------------- the pinned MH run
# 20 iterations of two chains at N = 65, D = 12 on the overdispersed daily SIR reports, the dispersion estimated as the
# third parameter.  The seed is pinned so that every decision has |log u - (lz_new - lz_old)| > 1e-6
# (tests/test_negbin_host.py checks that condition on the input), as incidence_cases.MCMC's is.
MCMC = dict(parameters=(0.8, 0.3, 2.0), h=0.03, iters=20, chains=2, seed=5, filter_index_start=7)
MCMC_SIGMA = np.diag([1.0, 1.0, 400.0])                  # the dispersion walks in steps of ~3.5: both ends of (0, 1e6]


def mcmc_run(**kw):
    import epipf
    args = dict(MCMC)
    args.update(kw)
    return epipf.incidence_mcmc(daily("sir", (0, 1)), "sir", args.pop("parameters"), args.pop("h"), sigma=MCMC_SIGMA,
                                flows=("infections", "removals"), probs=RHO, n_particles=N, n_population=NPOP, mu=MU,
                                dispersion="estimate", **args)
