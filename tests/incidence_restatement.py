"""numpy restatement of the incidence filter as DESIGN.md §19 defines it (a helper for the tests, no test itself).

What is new is restated here in numpy: the T = D + 2 rows, the flows as differences of a particle's parent and new
state, the accumulator since a column's previous report, and the product weight over the reported columns.  Everything
else is the CPU oracle's: the initial states are oracle.particle_filter's on one row, a column's factor is
oracle.binom_pmf / norm_pdf, the weights are summed sequentially, the logarithm is oracle.log_batch, the ancestors are
oracle.resample on the filter's resampling uniforms (oracle/philox.py), and particle j's day is oracle.simulate on row j
(the counter's particle word is the row index)."""
import numpy as np

import oracle
import philox

F = {"sir": 2, "seir": 3}
C = {"sir": 3, "seir": 4}
DEGENERATE = 1


def flows(model, parent, new):
    """[N, F] int64 from parent and new states [N, C]."""
    parent, new = np.asarray(parent, dtype=np.int64), np.asarray(new, dtype=np.int64)
    if model == "sir":
        return np.stack([parent[:, 0] - new[:, 0], new[:, 2] - parent[:, 2]], axis=1)
    return np.stack([parent[:, 0] - new[:, 0], (new[:, 2] + new[:, 3]) - (parent[:, 2] + parent[:, 3]),
                     new[:, 3] - parent[:, 3]], axis=1)


def padded(counts, model):
    """Y [D + 2, F]: rows 0 and D + 1 all NaN, rows 1..D the counts."""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, F[model])
    Y = np.full((counts.shape[0] + 2, F[model]), np.nan)
    Y[1:-1] = counts
    return Y


def weights(yrow, acc, observations, probs):
    """The product over the reported columns, in column order from 1.0."""
    n = acc.shape[0]
    w = np.ones(n)
    for k in range(acc.shape[1]):
        if np.isnan(yrow[k]):
            continue
        if observations:
            fac = oracle.norm_pdf(np.full(n, yrow[k]), acc[:, k].astype(float), np.full(n, probs))
        else:
            fac = oracle.binom_pmf(np.full(n, yrow[k]), acc[:, k].astype(float), np.full(n, probs))
        w = w * fac
    return w


def one_pass(counts, model, theta, observations, probs, N, npop, mu, key, f, cumulate=False):
    """One filter on counts [D, F].  Returns dict(status, hidden [T, N, C], ancestry [T, N], log_zetas [T], step (the
    dying step, or None), acc [T, N, F] (the accumulators the weights saw; row T - 1 is not formed))."""
    Y = padded(counts, model)
    T, nf = Y.shape
    rep = ~np.isnan(Y)
    first = oracle.particle_filter(np.zeros((1, C[model])), model, tuple(theta), False, 0.0, N, npop, mu, key=key,
                                   filter_index=f)
    hidden = np.zeros((T, N, C[model]), dtype=np.int32)
    anc = np.zeros((T, N), dtype=np.int32)
    accs = np.zeros((T, N, nf), dtype=np.int64)
    lz = np.zeros(T)
    hidden[0] = first["hidden"][0]
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
        for j in range(N):
            rows = np.zeros((j + 1, C[model]), dtype=np.int32)   # rows before j hold no infection: they draw nothing
            rows[j] = hidden[p - 1, a[j]]
            hidden[p, j] = oracle.simulate(model, rows, tuple(theta), 1.0, key, f, p)[0][j]
        if p + 1 == T:
            break
        acc = flows(model, hidden[p - 1][a], hidden[p])
        if cumulate:
            acc = acc + np.where(rep[p - 1][None, :], 0, accs[p - 1][a])
        accs[p] = acc
        w = weights(Y[p], acc, observations, probs)
    return dict(status=status, hidden=hidden, ancestry=anc, log_zetas=lz, step=step, acc=accs)


def loglik(r):
    return r["log_zetas"][-1] if r["status"] == 0 else -np.inf
