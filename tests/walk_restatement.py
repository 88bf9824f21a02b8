"""numpy restatement of the random-walk filter and a brute-force reduction of its parameter history, as DESIGN.md §18
defines them (a helper for the tests, no test itself).

The pass is §17's one_pass at M = 1, m = 0 with the whole theta history kept; it is restated here with its own loop
over if2_restatement.perturb_uniforms / weights and the CPU oracle, so that tests/test_walk_restatement.py can compare
the two.  The reduction uses no multiplicity recursion: every particle of day e(p) is walked back to day p one ancestor
at a time, and the N values found there go through np.quantile(..., method="inverted_cdf"), an exact sum and np.unique.
The exact sum is kept as a Fraction (the number math.fsum would round), so that the reference of the mean carries no
rounding of its own."""
import math
from fractions import Fraction

import numpy as np

import if2_restatement as rs
import oracle
import philox

DEGENERATE = 1


def one_pass(Y, model, theta, hw, observations, probs, npop, mu, key, f):
    """The pass at filter index f from the swarm theta [N, d] with half-widths hw [d].  Returns dict(status, theta_hist
    [T, N, d] (NaN from the dying step on), hidden [T, N, C], ancestry [T, N], log_zetas [T])."""
    Y = np.asarray(Y, dtype=np.float64)
    T = Y.shape[0]
    theta = np.asarray(theta, dtype=np.float64)
    hw = np.asarray(hw, dtype=np.float64)
    N, d = theta.shape
    first = oracle.particle_filter(Y[:1], model, tuple(theta[0]), observations, probs, N, npop, mu, key=key, filter_index=f)
    C = first["hidden"].shape[2]
    hidden = np.zeros((T, N, C), dtype=np.int32)
    anc = np.zeros((T, N), dtype=np.int32)
    hist = np.full((T, N, d), np.nan)
    lz = np.zeros(T)
    hidden[0] = first["hidden"][0]

    def jitter(th, p):
        t = th + hw * (2.0 * rs.perturb_uniforms(key, f, p, N, d) - 1.0)
        return np.where(t < 0.0, -t, t)

    hist[0] = jitter(theta, 0)
    status = 0
    for p in range(1, T):
        w = rs.weights(model, hidden[p - 1], Y[p - 1], observations, probs)
        sw = 0.0
        for v in w:                                      # the sequential sum, pmcmc.py:183
            sw = sw + v
        with np.errstate(divide="ignore", invalid="ignore"):
            lz[p] = lz[p - 1] + oracle.log_batch(np.array([sw / float(N)]))[0]
        a = oracle.resample(w, philox.resample_uniforms(key, f, p, N))
        if a is None:
            status = DEGENERATE
            lz[p:] = -np.inf
            break
        anc[p] = a
        hist[p] = jitter(hist[p - 1][a], p)
        for j in range(N):
            rows = np.zeros((j + 1, C), dtype=np.int32)  # rows before j hold no infection: they draw nothing
            rows[j] = hidden[p - 1, a[j]]
            out, _ = oracle.simulate(model, rows, tuple(hist[p, j]), 1.0, key, f, p)
            hidden[p, j] = out[j]
    return dict(status=status, theta_hist=hist, hidden=hidden, ancestry=anc, log_zetas=lz)


def quantities(theta, hidden, pop):
    """v [N, d + 1] of one day, one IEEE operation per numpy call: v_c = theta_c + 0.0; R = (theta_0 * S) / (theta_{d-1}
    * P) + 0.0, +inf where the denominator is 0.0."""
    theta = np.asarray(theta, dtype=np.float64)
    N, d = theta.shape
    v = np.empty((N, d + 1))
    v[:, :d] = np.add(theta, 0.0)
    den = np.multiply(theta[:, d - 1], np.float64(pop))
    num = np.multiply(theta[:, 0], hidden[:, 0].astype(np.float64))
    zero = den == 0.0
    v[:, d] = np.inf
    v[~zero, d] = np.add(np.divide(num[~zero], den[~zero]), 0.0)
    return v


def exact_sum(col):
    """The exact sum of float64 values as a Fraction: every float is an integer over a power of two."""
    tot, scale = 0, 2 ** 1074
    for x in col.tolist():
        n, den = x.as_integer_ratio()
        tot += n * (scale // den)
    return Fraction(tot, scale)


def rank_of(q, N):
    return max(int(np.ceil(np.float64(q) * np.float64(N))), 1)


def inverted_cdf(vals, q):
    """np.quantile(vals, q, method="inverted_cdf").  numpy's implementation interpolates between neighbours with weight 0
    or 1, which turns an infinite neighbour into NaN; with an infinite value present the same element is taken from the
    sorted values at the rule's rank max(ceil(q n), 1) instead."""
    vals = np.asarray(vals, dtype=np.float64)
    if np.all(np.isfinite(vals)):
        return np.float64(np.quantile(vals, q, method="inverted_cdf"))
    return np.sort(vals)[rank_of(q, vals.size) - 1]


def brute_force(hidden, ancestry, theta, pop, shift, lag, q):
    """(exact_mean [T, V] of Fractions (the exact sum over N), or math.inf where a value is infinite; quantiles
    [Q, T, V]; lineages [T]) of one chain's hidden [T, N, C], ancestry [T, N], theta [T, N, d]; lag None is the full
    smoother."""
    T, N = ancestry.shape
    V = theta.shape[2] + 1
    q = [] if q is None else list(q)
    mean = np.empty((T, V), dtype=object)
    qs = np.empty((len(q), T, V))
    lin = np.empty(T, dtype=np.int32)
    for p in range(T):
        e = T - 1 if lag is None else min(p + int(lag), T - 1)
        idx = np.arange(N)
        for day in range(e - 1, p - 1, -1):              # a day-(day + 1) particle's place on `day`
            idx = ancestry[day + shift][idx]
        lin[p] = np.unique(idx).size
        v = quantities(theta[p], hidden[p], pop)[idx]
        for k in range(V):
            col = v[:, k]
            mean[p, k] = math.inf if np.isinf(col).any() else exact_sum(col) / N
            for i, qi in enumerate(q):
                qs[i, p, k] = inverted_cdf(col, qi)
    return mean, qs, lin


def assert_mean_close(got, exact, N):
    """|computed - exact| <= (N + 1) 2^-53 exact + 2^-1074, in exact rational arithmetic.  A mean of N non-negative terms
    summed in any order in float64 rounds once per product m v, once per addition (at most N - 1) and once in the
    division by N: (N + 1) 2^-53 relative to first order.  2^-1074 is one spacing of the subnormal range, which the
    division's rounding can reach when the mean is subnormal.  An infinite mean must be infinite."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    exact = np.asarray(exact, dtype=object).reshape(-1)
    assert got.size == exact.size
    for g, e in zip(got, exact):
        if e == math.inf:
            assert g == math.inf, (g, e)
            continue
        assert math.isfinite(g), (g, float(e))
        err = abs(Fraction(float(g)) - e)
        assert err <= Fraction(N + 1, 2 ** 53) * e + Fraction(1, 2 ** 1074), (float(g), float(e), float(err))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)
