"""numpy restatement of the random-walk filter on incidence as DESIGN.md §20 defines it (a helper for the tests, no test
itself): the composition of tests/incidence_restatement.py (the T = D + 2 rows, the flows, the accumulator, the product
weight) with tests/if2_restatement.py's perturb (theta per particle, jittered at every step and kept).  Everything else
is the CPU oracle's, as in the two restatements it composes, and the order of a step is the incidence pass's: sum,
resample (the chain may die here), log_zeta, theta, SSA, flows, weight.  The smoothed true flows are restated from a
pass's own history with epipf.incidence.true_flows and epipf.smoothing's numpy reduction."""
import numpy as np

import if2_restatement as rs
import incidence_restatement as ir
import oracle
import philox
from epipf import _lib, incidence, smoothing

DEGENERATE = 1
MID = {"sir": _lib.SIR, "seir": _lib.SEIR}


def one_pass(counts, model, theta, hw, observations, probs, npop, mu, key, f, cumulate=False):
    """One pass on counts [D, F] from the swarm theta [N, d] with half-widths hw [d].  Returns dict(status, theta_hist
    [T, N, d] (NaN from the dying step on), hidden [T, N, C], ancestry [T, N], log_zetas [T], step (the dying step, or
    None), acc [T, N, F] (the accumulators the weights saw; row T - 1 is not formed))."""
    Y = ir.padded(counts, model)
    T, nf = Y.shape
    rep = ~np.isnan(Y)
    theta = np.asarray(theta, dtype=np.float64)
    hw = np.asarray(hw, dtype=np.float64)
    N, d = theta.shape
    C = ir.C[model]
    first = oracle.particle_filter(np.zeros((1, C)), model, tuple(theta[0]), False, 0.0, N, npop, mu, key=key,
                                   filter_index=f)
    hidden = np.zeros((T, N, C), dtype=np.int32)
    anc = np.zeros((T, N), dtype=np.int32)
    accs = np.zeros((T, N, nf), dtype=np.int64)
    hist = np.full((T, N, d), np.nan)
    lz = np.zeros(T)
    hidden[0] = first["hidden"][0]

    def jitter(th, p):
        t = th + hw * (2.0 * rs.perturb_uniforms(key, f, p, N, d) - 1.0)
        return np.where(t < 0.0, -t, t)

    hist[0] = jitter(theta, 0)
    w = np.ones(N)                                       # row 0 is never reported
    status, step = 0, None
    for p in range(1, T):
        sw = 0.0
        for v in w:                                      # the sequential sum, pmcmc.py:183
            sw = sw + v
        a = oracle.resample(w, philox.resample_uniforms(key, f, p, N))
        if a is None:
            status, step = DEGENERATE, p
            lz[p:] = -np.inf
            break
        with np.errstate(divide="ignore", invalid="ignore"):
            lz[p] = lz[p - 1] + oracle.log_batch(np.array([sw / float(N)]))[0]
        anc[p] = a
        hist[p] = jitter(hist[p - 1][a], p)
        for j in range(N):
            rows = np.zeros((j + 1, C), dtype=np.int32)  # rows before j hold no infection: they draw nothing
            rows[j] = hidden[p - 1, a[j]]
            hidden[p, j] = oracle.simulate(model, rows, tuple(hist[p, j]), 1.0, key, f, p)[0][j]
        if p + 1 == T:
            break
        acc = ir.flows(model, hidden[p - 1][a], hidden[p])
        if cumulate:
            acc = acc + np.where(rep[p - 1][None, :], 0, accs[p - 1][a])
        accs[p] = acc
        w = ir.weights(Y[p], acc, observations, probs)
    return dict(status=status, theta_hist=hist, hidden=hidden, ancestry=anc, log_zetas=lz, step=step, acc=accs)


def true_flows(model, hidden, ancestry):
    """flow [T, N, F] int64 of one pass, row by row with incidence_restatement.flows (row 0 zeros)."""
    T, N = ancestry.shape
    out = np.zeros((T, N, ir.F[model]), dtype=np.int64)
    for p in range(1, T):
        out[p] = ir.flows(model, hidden[p - 1][ancestry[p]], hidden[p])
    return out


def smoothed_flows(model, hidden, ancestry, lag, q, bins):
    """(sums [T, F], quantiles [Q, T, F] or None, lineages [T]) of one pass's true flows under the genealogy's
    multiplicities at `lag` (None: the full smoother)."""
    flow = true_flows(model, hidden, ancestry)
    np.testing.assert_array_equal(flow, incidence.true_flows(MID[model], hidden, ancestry))
    q = None if q is None else np.asarray(q, dtype=np.float64)
    return smoothing._smooth_numpy(flow, np.asarray(ancestry, dtype=np.int64), 1, False, q, bins, lag=lag)
