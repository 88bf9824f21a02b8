"""Inputs shared by the tests of the random-walk filter on incidence (a helper, no test itself): the "does it work"
configuration on the step fixture (tests/golden/walk_sir_step.npz: beta steps from 0.6 to 0.05 on day 12, 300 people)
with its recorded numbers, and the small cases the device is compared with the restatement on.  A restated pass is
computed once per process and shared, never modified."""
import functools
import os

import numpy as np

import incidence_cases as ic
import walk_cases as wc
import walk_incidence_restatement as wir
from conftest import GOLDEN

# ---------------------------------------------------------------------------------------------- does it work
START, RW, N_WORK, LAG_WORK, F_WORK, PROBS_WORK = wc.START, wc.RW, wc.N_WORK, wc.LAG_WORK, wc.F_WORK, 0.5
KEYS = wc.KEYS
COLUMNS_WORK = {"both": (0, 1), "infections": (0,)}
# Measured on the CPU restatement at N = 200, lag 5, probs 0.5, filter index 0.  gap: the smoothed median
# of beta_t averaged over rows 2..11 minus rows 17..29 (walk_cases.EARLY / LATE); gain: log_zetas[-1] with rw = (0.1, 0)
# minus the same run with rw = (0, 0).
#   key   gap, both columns   gain, both columns                   gap, infections alone   gain, infections alone
#   1     0.4927              +inf (fixed rates degenerate)        0.4474                  39.36
#   2     0.4144              56.64                                0.4789                  25.55
#   3     0.4492              41.75                                0.4111                  23.23
#   4     0.4338              38.67                                0.4338                  25.51
# The tests assert half the smallest finite value per column.
GAP_BOUND = {"both": 0.207, "infections": 0.205}
GAIN_BOUND = {"both": 19.3, "infections": 11.6}
GAPS = {"both": (0.4927, 0.4144, 0.4492, 0.4338), "infections": (0.4474, 0.4789, 0.4111, 0.4338)}
GAINS = {"both": (np.inf, 56.64, 41.75, 38.67), "infections": (39.36, 25.55, 23.23, 25.51)}
# The smoothed-mean true infections at lag 5 from infections alone: mean absolute error per day against the true daily
# flows, beside the raw reports' 3.76 (the thinned counts against the same flows).
#   key   error    margin (3.7586 - error)   smoothed total (true 219, reported 110)
#   1     1.1012   2.657                     225.9
#   2     0.8472   2.911                     231.5
#   3     1.0364   2.722                     227.1
#   4     0.9574   2.801                     224.5
# The tests require half the smallest margin.
RAW_ERROR = 3.7586
ERRORS = (1.1012, 0.8472, 1.0364, 0.9574)
MARGIN_BOUND = 2.657 / 2


@functools.lru_cache(maxsize=None)
def work():
    """The step fixture's true daily flows [29, 2] (infections S' - S, removals R - R' of its states X) and their
    reports, thinned once at 0.5."""
    fx = wc.load_fixture()
    X = np.load(os.path.join(GOLDEN, "walk_sir_step.npz"))["X"]
    flows = np.stack([X[:-1, 0] - X[1:, 0], X[1:, 2] - X[:-1, 2]], axis=1)
    counts = np.random.default_rng(14).binomial(flows, 0.5).astype(np.float64)
    return dict(flows=flows, counts=counts, npop=fx["npop"], mu=fx["mu"])


def work_counts(which):
    """The reports [29, 2] with the columns outside `which` unreported."""
    return ic.only(work()["counts"], COLUMNS_WORK[which])


@functools.lru_cache(maxsize=None)
def restated(which, key, walking):
    """The restatement's pass on the step fixture's reports under `key`, with the walk's half-widths or none."""
    w = work()
    hw = RW if walking else (0.0, 0.0)
    return wir.one_pass(work_counts(which), "sir", np.tile(START, (N_WORK, 1)), hw, False, PROBS_WORK, w["npop"], w["mu"],
                        key, F_WORK)


def infection_error(mean_infections):
    """Mean absolute error per day of smoothed-mean infections [D + 2] (rows 1..D the days) against the true flows."""
    return float(np.abs(np.asarray(mean_infections)[1:-1] - work()["flows"][:, 0]).mean())


# ---------------------------------------------------------------------------------------------- the small cases
KEY, F, N, D = ic.KEY, ic.F, ic.N, ic.D
NPOP, MU = ic.NPOP, ic.MU
THETA, PROBS, COLUMNS = ic.THETA, ic.PROBS, ic.COLUMNS
HW = {"sir": (0.1, 0.05), "seir": (0.1, 0.08, 0.05)}
# the batch of three chains: start, half-widths, probs, key.  The second keeps its rates (rw = 0), so it is
# incidence_cases.BATCH's second chain bit for bit and dies at its step 3 as that one does.
BATCH = [((0.8, 0.3), (0.1, 0.05), 0.5, 11), ((0.05, 0.3), (0.0, 0.0), 0.4, 1), ((1.6, 0.3), (0.3, 0.0), 0.6, 2)]

_PASSES = {}


def swarm(theta, n=N):
    return np.tile(np.asarray(theta, dtype=np.float64), (n, 1))


def restate(counts, model, theta, hw, observations, probs, n=N, key=KEY, f=F, cumulate=False):
    """walk_incidence_restatement.one_pass from `theta` tiled over n particles at population 300, mu 5, cached."""
    counts = np.asarray(counts, dtype=np.float64)
    k = (counts.tobytes(), counts.shape, model, tuple(theta), tuple(hw), bool(observations), float(probs), int(n),
         int(key), int(f), bool(cumulate))
    if k not in _PASSES:
        _PASSES[k] = wir.one_pass(counts, model, swarm(theta, n), hw, observations, probs, NPOP, MU, key, f,
                                  cumulate=cumulate)
    return _PASSES[k]
