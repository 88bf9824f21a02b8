"""R_t from case counts: the random-walk filter weighted by reported incidence, with smoothed daily beta, gamma, R_t and
true incidence (epipf_incidence_walk and epipf_incidence_smooth, csrc/epipf_walk_incidence.hip).

`epipf.walk_filter` estimates time-varying rates, but from observed compartments; `epipf.incidence_filter` takes what
surveillance delivers, but holds the rates constant.  This is their union: every particle carries its own theta,
jittered uniformly by +-rw at every step and reflected at 0 (`epipf.walk`), and is weighted by the reports of its flows
(`epipf.incidence`: `cases`, `flows`, `probs`, `cumulate` and the T = D + 2 rows are defined there):

    res = epipf.walk_incidence_filter(cases, ModelType.SIR, start=[0.3, 0.2], rw=[0.1, 0.0], flows=("infections",),
                                      probs=0.5, lag=5, n_particles=1000, n_population=300, mu=5)
    res.rt_quantiles[res.best]                             # R_t with its credible band, [Q, D + 2]
    res.incidence.mean[res.best, 1:-1, 0]                  # smoothed true infections per day

The result is `epipf.walk`'s WalkResult over the D + 2 rows (theta, R_t, lineages and states, smoothed under `lineage`
and `lag`), with one more attribute: `incidence`, the `Smoothed` true flows per day in the model's flow columns under
the same lag.  A flow is defined by a particle's true parent, so it is reduced under the genealogy's multiplicities;
lineage="reference" leaves `incidence` None.  With cumulate=True the flows are still each day's own.

Random numbers: `epipf.walk`'s (the resampling uniforms, the jitter's domain 7 and the SSA's: no stream of its own).
Scope: SIR and SEIR.
"""
import numpy as np

from . import engine as _engine
from . import smoothing
from .incidence import _check_dispersion, _check_probs, _check_ratio, _model, counts_matrix
from .pmcmc import _STREAM, _population, _take_filter_index, chain_key
from .walk import DIMS, WalkResult


def walk_incidence_filter(cases, type_model, start, rw, flows=("infections",), *, observations=False, probs=.5,
                          cumulate=False, lag=10, quantiles=smoothing.DEFAULT_QUANTILES, lineage="genealogy",
                          n_particles=1000, n_population=4820, mu=20, chains=1, key=None, device=0, dispersion=None):
    """Run `chains` random-walk filters on the reports and smooth their parameter histories, states and true flows on
    the device (the module's docstring).  `start` is [d] (every particle starts there), [N, d] or [chains, N, d]; `rw`
    is [d] or [chains, d] (>= 0); `probs` is a scalar or one per chain, and so is `dispersion` (None: the binomial or
    normal model; else negative-binomial reports, `epipf.incidence`; not with observations=True).  lag=None is the full smoother.  Returns
    WalkResult with `incidence`."""
    mid = _model(type_model)
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
    extra = {}
    if dispersion is not None:
        extra["dispersion"] = _check_dispersion(dispersion, observations, S)
    counts = counts_matrix(cases, mid, flows, observations)
    pr = _check_probs(probs, observations) if dispersion is None else _check_ratio(probs)
    if pr.shape not in ((), (S,)):
        raise ValueError(f"probs must be a scalar or [{S}], got {pr.shape}")
    npop, mus = _population(mid, 1, n_population, mu)
    k = _STREAM.key if key is None else int(key)
    f = _take_filter_index()
    keys = np.array([chain_key(k, s) for s in range(S)], dtype=np.uint64)
    eng = _engine.get_engine(mid, 1, N, counts.shape[0] + 2, S, device)
    eng.set_population(npop, mus)
    lz, st = eng.walk_incidence(swarm, hw, np.broadcast_to(pr, (S,)), keys, f, counts, observations=observations,
                                cumulate=cumulate, **extra)
    mean, quant, lineages = eng.walk_smooth(S, quantiles=quantiles, lineage=lineage, lag=lag)
    states = eng.smooth(S, quantiles=quantiles, lineage=lineage, kind="smoothing", lag=lag)
    true_flows = eng.incidence_smooth(S, quantiles=quantiles, lag=lag) if lineage == "genealogy" else None
    return WalkResult(lz, st, mean, quant, lineages, states, true_flows)
