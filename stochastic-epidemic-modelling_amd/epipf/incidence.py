"""Incidence observations: the particle filter and PMCMC on reported case counts (epipf_run_incidence,
csrc/epipf_incidence.hip).

The reference's observation models see the compartments themselves, (S, I, R) on every day.  A surveillance system
delivers something else: new cases per day or per week, sometimes removals as well, with gaps, and a report after a gap
covers everything since the previous one.  Here the filter is weighted by such reports:

    res = epipf.incidence_filter(cases, ModelType.SIR, [0.8, 0.3], flows=("infections",), probs=0.5,
                                 n_particles=1000, n_population=300, mu=5)
    res.loglik                                             # log-likelihood of every report, per chain

`cases` is [D] or [D, len(flows)], one row per day d = 1..D counting what was reported for the interval (d-1, d]; NaN
means "not reported" (a day without a report is a row of NaN).  `flows` names the columns:

    SIR    "infections" = S' - S    "removals" = R - R'
    SEIR   "exposures"  = S' - S    "onsets"   = (I + R) - (I' + R')    "removals" = R - R'

with x' a particle's parent state and x its new one ("infections" is accepted for SEIR's first column too).  Columns
that are not named are never observed.  The pass runs over T = D + 2 rows: row 0 is the initial draw, rows 1..D are the
days, and row D + 1 is resampled on day D's weights and propagated once more, so that `log_zetas[:, D + 1]` is the
likelihood of every report and trajectories and smoothed states see the last one.  With rep[p][k] = "column k of day p
is reported":

    acc_p[j][k] = flow_p[j][k] + (cumulate and not rep[p-1][k] ? acc_{p-1}[a_p[j]][k] : 0),   acc_0 = 0
    w_p[j]      = product over the reported k, in column order from 1.0, of
                  observations=False: the binomial pmf of the report out of acc_p[j][k] at `probs`
                  observations=True:  the normal pdf of the report at mean acc_p[j][k], sd probs acc_p[j][k] + 1e-4

                  dispersion=k:       the negative-binomial pmf of the report at mean probs acc_p[j][k] and variance
                                      mean + mean^2 / k: overdispersed reports, and a report may
                                      exceed the particle's flow; probs is then a mean ratio and may exceed 1

cumulate=False: a report counts that day alone and unreported days are simply unobserved; cumulate=True: a report counts
everything since that column's previous report (weekly totals).  The product is the likelihood of independent reports.
Resampling, random numbers, the SSA and the degeneracy rule are the filter's.  Scope: SIR and SEIR.

`incidence_mcmc` is a lockstep random-walk Metropolis-Hastings sampler on that likelihood, one batched filter call per
iteration for all chains.
"""
import numpy as np

from . import _lib
from . import engine as _engine
from . import smoothing
from .pmcmc import (_STREAM, ChainResult, _population, _take_filter_index, chain_key, legacy_randint, mvn_apply,
                    mvn_factor)

FLOWS = {_lib.SIR: ("infections", "removals"), _lib.SEIR: ("exposures", "onsets", "removals")}
ALIASES = {_lib.SIR: {}, _lib.SEIR: {"infections": "exposures"}}
DIMS = {_lib.SIR: 2, _lib.SEIR: 3}


def _model(type_model):
    mid = _engine.model_id(type_model)
    if mid not in FLOWS:
        raise ValueError("incidence observations cover the SIR and SEIR models; the subgroup models are out of their scope")
    return mid


def counts_matrix(cases, mid, flows, observations=False):
    """`cases` [D] or [D, len(flows)] mapped into the model's F columns: [D, F] float64, NaN where nothing is reported."""
    names = FLOWS[mid]
    if isinstance(flows, str):
        flows = (flows,)
    flows = tuple(flows)
    if not flows:
        raise ValueError("flows must name at least one column")
    cols = []
    for f in flows:
        f = ALIASES[mid].get(f, f)
        if f not in names:
            raise ValueError(f"unknown flow {f!r}: this model has {names}")
        if names.index(f) in cols:
            raise ValueError(f"flow {f!r} is named twice")
        cols.append(names.index(f))
    cases = np.asarray(cases, dtype=np.float64)
    if cases.ndim == 1:
        cases = cases[:, None]
    if cases.ndim != 2 or cases.shape[1] != len(cols):
        raise ValueError(f"cases must be [D] or [D, {len(cols)}] for flows {flows}, got {cases.shape}")
    if cases.shape[0] < 1:
        raise ValueError("cases needs at least one day")
    seen = cases[~np.isnan(cases)]
    if np.isinf(seen).any() or (seen < 0).any():
        raise ValueError("reports must be finite and >= 0 (NaN: not reported)")
    if not observations and (seen != np.floor(seen)).any():
        raise ValueError("the binomial model needs integer reports")
    out = np.full((cases.shape[0], len(names)), np.nan)
    out[:, cols] = cases
    return out


def _check_probs(p, observations):
    p = np.asarray(p, dtype=np.float64)
    if not (np.all(np.isfinite(p)) and np.all(p >= 0.0) and (observations or np.all(p <= 1.0))):
        raise ValueError("probs must be finite and >= 0" if observations else "probs must lie in [0, 1]")
    return p


MAX_DISPERSION = 1e6


def _check_dispersion(dispersion, observations, n=None):
    """The negative-binomial dispersion as a float64 array, each entry in (0, 1e6]; with n, a scalar or
    [n] broadcast to [n]."""
    if n is None:
        if observations:
            raise ValueError("dispersion is the negative-binomial model's: it does not go with observations=True")
        k = np.asarray(dispersion, dtype=np.float64)
    else:
        k = _engine.dispersion_vector(dispersion, n, observations)
    if not (np.all(np.isfinite(k)) and np.all(k > 0.0)):
        raise ValueError("dispersion must be finite and > 0")
    if np.any(k > MAX_DISPERSION):
        raise ValueError("dispersion must be <= 1e6: the Poisson limit beyond it is out of scope")
    return k


def _check_ratio(p):
    """probs under a dispersion: a mean ratio, finite and >= 0."""
    p = np.asarray(p, dtype=np.float64)
    if not (np.all(np.isfinite(p)) and np.all(p >= 0.0)):
        raise ValueError("probs must be finite and >= 0")
    return p


def true_flows(mid, hidden, ancestry):
    """flow [..., T, N, F] int64 of histories hidden [..., T, N, C], ancestry [..., T, N]: the flows above between each
    particle's parent hidden[p-1][ancestry[p][i]] and its own state hidden[p][i]; row 0 is zeros.  What
    Engine.incidence_smooth reduces, restated on the host."""
    hid, anc = np.asarray(hidden, dtype=np.int64), np.asarray(ancestry, dtype=np.int64)
    new = hid[..., 1:, :, :]
    par = np.take_along_axis(hid[..., :-1, :, :], anc[..., 1:, :, None], axis=-2)
    if mid == _lib.SIR:
        cols = [par[..., 0] - new[..., 0], new[..., 2] - par[..., 2]]
    else:
        cols = [par[..., 0] - new[..., 0], (new[..., 2] + new[..., 3]) - (par[..., 2] + par[..., 3]),
                new[..., 3] - par[..., 3]]
    out = np.zeros(hid.shape[:-1] + (len(cols),), dtype=np.int64)
    out[..., 1:, :, :] = np.stack(cols, axis=-1)
    return out


class IncidenceResult:
    """loglik [S]: the log-likelihood of every report per chain (-inf where the chain is not OK); log_zetas [S, D + 2];
    status [S] (STATUS_*); best: the argmax of loglik over the chains whose status is OK, or None when there is none;
    states: the `Smoothed` compartments of the run over its D + 2 rows (Engine.smooth), or None without quantiles;
    incidence: the `Smoothed` true flows per day under the same quantiles and lag (Engine.incidence_smooth: mean
    [S, D + 2, F] and quantiles [S, Q, D + 2, F] in the model's flow columns, row 0 zeros), or None without quantiles or
    with lineage="reference"; history(): (hidden [S, D + 2, N, C], ancestry [S, D + 2, N]) of the run.  `incidence` is
    reduced from the engine's resident history when it is first read and kept from then on.  Engines are shared
    (`epipf.get_engine`), so another filter may have run on this one since: the read is then refused with a
    RuntimeError instead of handing out that filter's flows (read `incidence` before the next run to keep it).
    history() reads the resident history too and is the run's own until its engine runs again."""

    def __init__(self, log_zetas, status, states, eng, flows_options=None):
        self.log_zetas, self.status, self.states, self._eng = log_zetas, status, states, eng
        self._flows_options, self._incidence = flows_options, None
        # the engine's count of runs at this one (Engine.run_serial): what a later read of `incidence` is held against
        self._serial = getattr(eng, "run_serial", None)
        ok = status == _lib.STATUS_OK
        self.loglik = np.where(ok, log_zetas[:, -1], -np.inf)
        self.best = int(np.argmax(self.loglik)) if ok.any() else None

    def history(self):
        return self._eng.history(self.status.shape[0])

    @property
    def incidence(self):
        if self._incidence is None and self._flows_options is not None:
            if self._serial is None or self._eng.run_serial != self._serial:
                raise RuntimeError("the engine has run another filter since this one: its history, which `incidence` is "
                                   "reduced from, is no longer this result's (read `incidence` before the next run)")
            self._incidence = self._eng.incidence_smooth(self.status.shape[0], **self._flows_options)
        return self._incidence


def incidence_filter(cases, type_model, thetas, flows=("infections",), observations=False, probs=.5, n_particles=1000,
                     n_population=4820, mu=20, *, cumulate=False, key=None, keys=None, filter_index=None, device=0,
                     quantiles=None, lineage="genealogy", lag=None, dispersion=None):
    """Run one filter per row of `thetas` ([d] or [chains, d]) on the reports (the module's docstring).  `probs` is a
    scalar or one per chain, and so is `dispersion` (None: the binomial or normal model; else negative-binomial
    reports, not with observations=True).  key / keys / filter_index default to the module stream (`epipf.seed_stream`): chain s
    under chain_key(key, s), all at one filter index taken from the stream's counter.  With `quantiles` the run is
    smoothed on the device under `lineage` and `lag` (`epipf.smoothing`), and so are the particles' true flows
    (`IncidenceResult.incidence`).  The flows are defined by a particle's true parent, so they exist under the
    genealogy's multiplicities only: lineage="reference" leaves `incidence` None.  `incidence` is reduced when first
    read, and refused if the engine has run again by then.  Returns IncidenceResult."""
    mid = _model(type_model)
    d = DIMS[mid]
    th = np.asarray(thetas, dtype=np.float64)
    if th.ndim == 1:
        th = th[None, :]
    if th.ndim != 2 or th.shape[1] != d or th.shape[0] < 1:
        raise ValueError(f"thetas must be [{d}] or [chains, {d}], got {np.shape(thetas)}")
    if not (np.all(np.isfinite(th)) and np.all(th >= 0.0)):
        raise ValueError("thetas must be finite and >= 0")
    S, N = th.shape[0], int(n_particles)
    if N < 1:
        raise ValueError("n_particles must be >= 1")
    extra = {}
    if dispersion is not None:
        extra["dispersion"] = _check_dispersion(dispersion, observations, S)
    counts = counts_matrix(cases, mid, flows, observations)
    pr = _check_probs(probs, observations) if dispersion is None else _check_ratio(probs)
    if pr.shape not in ((), (S,)):
        raise ValueError(f"probs must be a scalar or [{S}], got {pr.shape}")
    if quantiles is not None:
        smoothing.check_options(lineage, "smoothing", quantiles)
        lag = smoothing.check_lag(lag, "smoothing")
    npop, mus = _population(mid, 1, n_population, mu)
    if keys is None:
        k = _STREAM.key if key is None else int(key)
        keys = np.array([chain_key(k, s) for s in range(S)], dtype=np.uint64)
    else:
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        if keys.shape != (S,):
            raise ValueError(f"keys must have {S} entries")
    f = _take_filter_index() if filter_index is None else filter_index
    eng = _engine.get_engine(mid, 1, N, counts.shape[0] + 2, S, device)
    eng.set_population(npop, mus)
    lz, st = eng.run_incidence(np.ascontiguousarray(th), np.broadcast_to(pr, (S,)), keys, f, counts,
                               observations=observations, cumulate=cumulate, **extra)
    states = flows_options = None
    if quantiles is not None:
        states = eng.smooth(S, quantiles=quantiles, lineage=lineage, kind="smoothing", lag=lag)
        if lineage == "genealogy":
            flows_options = dict(quantiles=quantiles, lag=lag)
    return IncidenceResult(lz, st, states, eng, flows_options)


def incidence_mcmc(cases, type_model, parameters, h, sigma=None, iters=1000, flows=("infections",), observations=False,
                   probs=.5, n_particles=1000, n_population=4820, mu=20, *, cumulate=False, chains=1, seed=0, rngs=None,
                   keys=None, device=0, filter_index_start=0, dispersion=None):
    """Random-walk Metropolis-Hastings on the incidence likelihood, `chains` chains in lockstep with one batched filter
    call per iteration.  parameters: the starting theta [d] or [chains, d] (with probs=None its last entry is the
    reporting probability, estimated with the rates); proposals are N(theta, h sigma) (sigma: identity, [d, d] or
    [chains, d, d]).  Chain c draws from rngs[c] (default RandomState(seed + c)) and filters under keys[c] (default
    chain_key(seed, c)) at filter indices counting from filter_index_start.

    Iteration 0 filters `parameters` itself (ValueError if a chain degenerates there) and one legacy_randint(N) picks
    its trajectory.  Iteration i >= 1 always draws the proposal (standard_normal(d)) and then one random_sample(), so
    the host stream advances the same whatever happens.  A proposal with a negative component (or, with probs=None, a
    reporting probability outside [0, 1]) is invalid: its chain runs no filter and consumes no filter index.  A
    proposal is accepted iff it is valid, its filter is OK and log u < lz_new - lz_old, lz = log_zetas[:, D + 1]; one
    more legacy_randint(N) then picks the trajectory (D + 2 rows), otherwise the previous row is copied.

    dispersion: a scalar fixes the negative-binomial dispersion; "estimate" appends it as the last
    entry of `parameters` (after the reporting probability when probs=None) and a proposal whose dispersion is <= 0 or
    > 1e6 is invalid in the same way.  With a dispersion the reporting probability is a mean ratio: any value >= 0 is
    valid.  Not with observations=True.

    Returns a list of ChainResult (thetas [iters, d], likelihoods, log_likelihoods [iters], sampled_trajs
    [D + 2, iters, C], acceptances = accepted proposals, filters_run)."""
    mid = _model(type_model)
    nc, N, iters = int(chains), int(n_particles), int(iters)
    if nc < 1 or N < 1 or iters < 1:
        raise ValueError("chains, n_particles and iters must be >= 1")
    dm = DIMS[mid]
    est_k = isinstance(dispersion, str)
    if est_k and dispersion != "estimate":
        raise ValueError('dispersion must be None, a scalar or "estimate"')
    if dispersion is not None and observations:
        raise ValueError("dispersion is the negative-binomial model's: it does not go with observations=True")
    d = dm + (1 if probs is None else 0) + (1 if est_k else 0)
    ip = dm if probs is None else None                   # the reporting probability's column of `parameters`
    P = np.asarray(parameters, dtype=np.float64)
    if P.shape not in ((d,), (nc, d)):
        raise ValueError(f"parameters must be [{d}] or [{nc}, {d}], got {P.shape}")
    P = np.ascontiguousarray(np.broadcast_to(P, (nc, d)))
    if not (np.all(np.isfinite(P)) and np.all(P >= 0.0)):
        raise ValueError("parameters must be finite and >= 0")
    check_p = _check_probs if dispersion is None else (lambda p, _obs: _check_ratio(p))
    if probs is None:
        check_p(P[:, ip], observations)
    else:
        if np.ndim(probs) != 0:
            raise ValueError("probs must be a scalar, or None to estimate it as the last parameter")
        check_p(probs, observations)
    if est_k:
        _check_dispersion(P[:, -1], observations)
    elif dispersion is not None:
        if np.ndim(dispersion) != 0:
            raise ValueError('dispersion must be a scalar, or "estimate" to estimate it as the last parameter')
        _check_dispersion(dispersion, observations)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("h must be finite and > 0")
    Sg = np.eye(d) if sigma is None else np.asarray(sigma, dtype=np.float64)
    if Sg.shape not in ((d, d), (nc, d, d)):
        raise ValueError(f"sigma must be [{d}, {d}] or [{nc}, {d}, {d}]")
    facs = [mvn_factor(h * (Sg[c] if Sg.ndim == 3 else Sg)) for c in range(nc if Sg.ndim == 3 else 1)]
    counts = counts_matrix(cases, mid, flows, observations)
    D = counts.shape[0]
    npop, mus = _population(mid, 1, n_population, mu)
    rngs = [np.random.RandomState(int(seed) + c) for c in range(nc)] if rngs is None else list(rngs)
    if len(rngs) != nc:
        raise ValueError(f"rngs has {len(rngs)} entries for {nc} chains")
    if keys is None:
        keys = np.array([chain_key(seed, c) for c in range(nc)], dtype=np.uint64)
    else:
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        if keys.shape != (nc,):
            raise ValueError(f"keys must have {nc} entries")
    eng = _engine.get_engine(mid, 1, N, D + 2, nc, device)
    eng.set_population(npop, mus)
    C = eng.C

    def split(theta):
        """(rates [nc, dm], probs [nc]) of full parameter rows"""
        return theta[:, :dm], (theta[:, ip] if probs is None else np.full(nc, float(probs)))

    def extra(theta):
        """the engine call's dispersion keyword: none without a dispersion"""
        if dispersion is None:
            return {}
        return {"dispersion": np.ascontiguousarray(theta[:, -1]) if est_k else np.full(nc, float(dispersion))}

    thetas = np.zeros((nc, iters, d))
    loglik = np.zeros((nc, iters))
    tr = np.zeros((nc, iters, D + 2, C))
    fnext = np.full(nc, int(filter_index_start), dtype=np.int64)
    filters_run = np.zeros(nc, dtype=np.int64)
    acceptances = np.zeros(nc, dtype=np.int64)

    th0, pr0 = split(P)
    lz, st = eng.run_incidence(np.ascontiguousarray(th0), pr0, keys, fnext.astype(np.uint64), counts,
                               observations=observations, cumulate=cumulate, **extra(P))
    fnext += 1
    filters_run += 1
    for c in range(nc):
        if st[c] != _lib.STATUS_OK:
            raise ValueError(f"chain {c}: the filter degenerates at its starting parameters {P[c].tolist()}")
    chosen = np.array([legacy_randint(rngs[c], N) for c in range(nc)], dtype=np.int32)
    paths = eng.path_sample(chosen)
    thetas[:, 0] = P
    loglik[:, 0] = lz[:, -1]
    tr[:, 0] = paths

    for i in range(1, iters):
        props = np.zeros((nc, d))
        logu = np.zeros(nc)
        act = np.zeros(nc, dtype=np.int32)
        fidx = np.zeros(nc, dtype=np.uint64)
        for c in range(nc):
            z = rngs[c].standard_normal(d)
            props[c] = mvn_apply(z, facs[c if len(facs) > 1 else 0], thetas[c, i - 1])
            u = rngs[c].random_sample()
            logu[c] = np.log(u) if u > 0.0 else -np.inf
            ok = not (props[c] < 0).any()
            if ok and probs is None and dispersion is None:
                ok = 0.0 <= props[c, ip] <= 1.0
            if ok and est_k:
                ok = 0.0 < props[c, -1] <= MAX_DISPERSION
            if ok:
                act[c] = 1
                fidx[c] = fnext[c]
                fnext[c] += 1
                filters_run[c] += 1
        take = np.zeros(nc, dtype=bool)
        if act.any():
            full = np.where(act[:, None] != 0, props, thetas[:, i - 1])
            th_all, pr_all = split(full)
            lz, st = eng.run_incidence(np.ascontiguousarray(th_all), pr_all, keys, fidx, counts,
                                       observations=observations, cumulate=cumulate, active=act, **extra(full))
            for c in range(nc):
                take[c] = bool(act[c]) and st[c] == _lib.STATUS_OK and logu[c] < lz[c, -1] - loglik[c, i - 1]
        if take.any():
            chosen = np.zeros(nc, dtype=np.int32)
            for c in np.nonzero(take)[0]:
                chosen[c] = legacy_randint(rngs[c], N)
            paths = eng.path_sample(chosen)
        for c in range(nc):
            if take[c]:
                acceptances[c] += 1
                thetas[c, i] = props[c]
                loglik[c, i] = lz[c, -1]
                tr[c, i] = paths[c]
            else:
                thetas[c, i] = thetas[c, i - 1]
                loglik[c, i] = loglik[c, i - 1]
                tr[c, i] = tr[c, i - 1]
    trajs = tr.transpose(0, 2, 1, 3)
    with np.errstate(under="ignore"):
        lik = np.exp(loglik)
    return [ChainResult(thetas[c], lik[c], loglik[c], trajs[c], int(acceptances[c]), int(filters_run[c]))
            for c in range(nc)]
