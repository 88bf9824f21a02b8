"""Time-varying rates: a filter in which the rates follow a random walk, and smoothed daily beta, gamma and R_t with
credible bands (epipf_walk_filter and epipf_walk_smooth, csrc/epipf_walk.hip).

Every other tool of the package holds the rates constant over the series.  Here each particle carries its own theta,
jittered uniformly by +-rw at every step and reflected at 0 (the perturbation of iterated filtering, `epipf.if2`, at one
iteration), and resampling selects parameters with the states: the bootstrap filter of the model "theta follows a
reflected random walk" (Dureau, Kalogeropoulos, Baguelin 2013).  Every day's parameters are kept, and the smoother's
backward window reduces them:

    res = epipf.walk_filter(Y, ModelType.SIR, start=[1.2, 0.5], rw=[0.05, 0.0], lag=10, n_particles=1000,
                            n_population=300, mu=5, probs=.5)
    res.theta_quantiles[res.best, 1, :, 0]                 # the smoothed median of beta_t
    res.rt_mean[res.best]                                  # R_t = beta_t S_t / (gamma_t P)

The quantities of particle i on day p, from theta_p[i] (d components) and its state (S = compartment 0):

    v_c = theta_p[i][c] + 0.0                              c < d   (+ 0.0 turns -0.0 into +0.0)
    v_d = R = (theta_p[i][0] * float(S)) / (theta_p[i][d-1] * P) + 0.0,   +inf where the denominator is 0.0

With m[p][i] the fixed-lag multiplicities of `epipf.smoothing` (lag L >= 0 from day e(p) = min(p + L, T-1); lag=None or
L >= T-1: the full genealogy smoother; L = 0: the particle cloud) under `lineage`:

    lineages[p]          = #{i : m[p][i] > 0}
    mean[p][k]           = sum_i m[p][i] v_k[i] / N        over the i with m > 0
    quantile q of (p, k) = the smallest v_k[i] with sum_{i' : v_k[i'] <= v_k[i]} m[p][i'] >= max(ceil(q N), 1)
                           = np.quantile(np.repeat(v, m), q, method="inverted_cdf"): an element of the input

`rw` may differ between the chains of a call, so the step width can be chosen by likelihood: `loglik` [S] estimates each
chain's random-walk model likelihood and `best` is its argmax.  An rw entry of 0 keeps that component constant bit for
bit.  Scope: SIR and SEIR.

Random numbers: key = the module stream (`epipf.seed_stream`), chain s under chain_key(key, s), all at one filter index
taken from the stream's counter.
"""
import numpy as np

from . import _lib
from . import engine as _engine
from . import smoothing
from .pmcmc import _STREAM, _check_Y, _population, _take_filter_index, chain_key

DIMS = {_lib.SIR: 2, _lib.SEIR: 3}


def quantities(theta, hidden, population_total):
    """v [..., N, d + 1] float64 of the definition above from theta [..., N, d] and hidden [..., N, C]."""
    theta = np.asarray(theta, dtype=np.float64)
    S = np.asarray(hidden)[..., 0].astype(np.float64)
    d = theta.shape[-1]
    v = np.empty(theta.shape[:-1] + (d + 1,), dtype=np.float64)
    v[..., :d] = theta + 0.0
    den = theta[..., d - 1] * np.float64(population_total)
    num = theta[..., 0] * S
    with np.errstate(divide="ignore", invalid="ignore"):
        v[..., d] = np.where(den == 0.0, np.inf, num / den + 0.0)
    return v


def _reduce_numpy(hid, anc, theta, pop, shift, lag, q):
    """The host restatement for one chain: (mean [T, V], quantiles [Q, T, V] or None, lineages [T])."""
    T, N = anc.shape
    m = smoothing.lag_multiplicities(anc, shift, T - 1 if lag is None else min(int(lag), T - 1))
    v = quantities(theta, hid, pop)
    V = v.shape[-1]
    mean = np.empty((T, V))
    qs = None if q is None else np.empty((q.size, T, V))
    ranks = None if q is None else [max(int(np.ceil(qi * np.float64(N))), 1) for qi in q]
    for p in range(T):
        live = m[p] > 0
        w = m[p, live]
        for k in range(V):
            x = v[p, live, k]
            mean[p, k] = np.sum(w * x) / float(N)
            if q is not None:
                order = np.argsort(x, kind="stable")
                cum = np.cumsum(w[order])
                for i, r in enumerate(ranks):
                    qs[i, p, k] = x[order[np.searchsorted(cum, r, side="left")]]
    return mean, qs, np.count_nonzero(m, axis=1).astype(np.int32)


def smooth_history(hidden, ancestry, theta, population_total, *, lag=10, quantiles=smoothing.DEFAULT_QUANTILES,
                   lineage="genealogy", device=None):
    """The reduction on histories from anywhere: hidden [T, N, C], ancestry [T, N], theta [T, N, d] (or a batch with a
    leading axis).  Returns (mean [T, d + 1], quantiles [Q, T, d + 1] or None, lineages [T]); the last column is R_t.
    device=None computes on the host in numpy; an integer runs epipf_walk_smooth_history on that device."""
    lin, _, q = smoothing.check_options(lineage, "smoothing", quantiles)
    lag = smoothing.check_lag(lag, "smoothing")
    hid, anc, th = np.asarray(hidden), np.asarray(ancestry), np.asarray(theta, dtype=np.float64)
    batch = hid.ndim == 4
    if not batch:
        hid, anc, th = hid[None], anc[None], th[None]
    if hid.ndim != 4 or anc.shape != hid.shape[:3] or th.ndim != 4 or th.shape[:3] != hid.shape[:3]:
        raise ValueError("hidden [T, N, C], ancestry [T, N] and theta [T, N, d] (or batches of them) must agree")
    n, T, N, C = hid.shape
    if min(n, T, N, C, th.shape[3]) < 1:
        raise ValueError("n, T, N, C and d must be >= 1")
    if not (np.all(np.isfinite(th)) and np.all(th >= 0.0)):
        raise ValueError("theta must be finite and >= 0")
    if not (np.isfinite(population_total) and population_total > 0):
        raise ValueError("population_total must be finite and > 0")
    hid = np.rint(hid).astype(np.int64)
    anc = np.rint(anc).astype(np.int64)
    if hid.min() < 0 or hid.max() > 2**31 - 1:
        raise ValueError("counts must be non-negative int32 values")
    if anc.min() < 0 or anc.max() >= N:
        raise ValueError("ancestors must lie in [0, N)")
    if device is None:
        parts = [_reduce_numpy(hid[i], anc[i], th[i], population_total, lin, lag, q) for i in range(n)]
        mean = np.stack([a for a, _, _ in parts])
        qs = None if q is None else np.stack([b for _, b, _ in parts])
        lineages = np.stack([c for _, _, c in parts])
    else:
        eng = _engine.get_engine(_lib.SIR, 1, 1, 1, 1, device)
        mean, qs, lineages = eng.walk_smooth_history(hid.astype(np.int32), anc.astype(np.int32), th, population_total,
                                                     lin, q, lag=lag)
    if not batch:
        return mean[0], None if qs is None else qs[0], lineages[0]
    return mean, qs, lineages


class WalkResult:
    """loglik [S]: the random-walk model's log-likelihood estimate of each chain (-inf where degenerate); log_zetas
    [S, T]; status [S] (STATUS_*); theta_mean [S, T, d] and theta_quantiles [S, Q, T, d] (None without quantiles): the
    smoothed parameters per day; rt_mean [S, T] and rt_quantiles [S, Q, T]: R_t; lineages [S, T]; states: the
    `Smoothed` compartments of the same run under the same lineage and lag (Engine.smooth); best: the argmax of loglik
    over the chains whose status is OK, or None when there is none.  Rows of chains that are not OK are NaN.
    incidence: None after walk_filter; after `epipf.walk_incidence_filter` the `Smoothed` true flows per day under the
    same lag (Engine.incidence_smooth), or None under lineage="reference"."""

    def __init__(self, log_zetas, status, mean, quant, lineages, states, incidence=None):
        d = mean.shape[-1] - 1
        self.log_zetas, self.status, self.lineages, self.states = log_zetas, status, lineages, states
        self.incidence = incidence
        ok = status == _lib.STATUS_OK
        self.loglik = np.where(ok, log_zetas[:, -1], -np.inf)
        self.theta_mean, self.rt_mean = mean[..., :d], mean[..., d]
        self.theta_quantiles = None if quant is None else quant[..., :d]
        self.rt_quantiles = None if quant is None else quant[..., d]
        self.best = int(np.argmax(np.where(ok, self.loglik, -np.inf))) if ok.any() else None


def walk_filter(Y, type_model, start, rw, *, lag=10, quantiles=smoothing.DEFAULT_QUANTILES, lineage="genealogy",
                n_particles=1000, n_population=4820, mu=20, observations=False, probs=.1, chains=1, key=None, device=0):
    """Run `chains` random-walk filters and smooth their parameter histories on the device (the module's docstring).
    `start` is [d] (every particle starts there), [N, d] or [chains, N, d] (a prior sample of theta_0); `rw` is [d] or
    [chains, d] (>= 0).  lag=None is the full smoother.  Returns WalkResult."""
    mid = _engine.model_id(type_model)
    if mid not in DIMS:
        raise ValueError("walk_filter covers the SIR and SEIR models; the subgroup models are out of its scope")
    d = DIMS[mid]
    S, N = int(chains), int(n_particles)
    if S < 1 or N < 1:
        raise ValueError("chains and n_particles must be >= 1")
    smoothing.check_options(lineage, "smoothing", quantiles)
    lag = smoothing.check_lag(lag, "smoothing")
    start = np.asarray(start, dtype=np.float64)
    if start.shape not in ((d,), (N, d), (S, N, d)):
        raise ValueError(f"start must be [{d}], [{N}, {d}] or [{S}, {N}, {d}], got {start.shape}")
    rw = np.asarray(rw, dtype=np.float64)
    if rw.shape not in ((d,), (S, d)):
        raise ValueError(f"rw must be [{d}] or [{S}, {d}], got {rw.shape}")
    if not (np.all(np.isfinite(rw)) and np.all(rw >= 0.0) and np.all(np.isfinite(start)) and np.all(start >= 0.0)):
        raise ValueError("rw and start must be finite and >= 0")
    swarm = np.ascontiguousarray(np.broadcast_to(start, (S, N, d)))
    hw = np.ascontiguousarray(np.broadcast_to(rw, (S, d)))
    Y = _check_Y(mid, 1, Y)
    npop, mus = _population(mid, 1, n_population, mu)
    k = _STREAM.key if key is None else int(key)
    f = _take_filter_index()
    keys = np.array([chain_key(k, s) for s in range(S)], dtype=np.uint64)
    eng = _engine.get_engine(mid, 1, N, Y.shape[0], S, device)
    eng.set_observations(Y)
    eng.set_population(npop, mus)
    lz, st = eng.walk_filter(swarm, hw, probs, keys, f, observations=observations)
    mean, quant, lineages = eng.walk_smooth(S, quantiles=quantiles, lineage=lineage, lag=lag)
    states = eng.smooth(S, quantiles=quantiles, lineage=lineage, kind="smoothing", lag=lag)
    return WalkResult(lz, st, mean, quant, lineages, states)
