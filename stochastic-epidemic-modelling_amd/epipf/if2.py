"""Iterated filtering (IF2; Ionides, Nguyen, Atchade, Stoev, King, PNAS 2015; `mif2` in pomp): a maximum-likelihood
search for the SIR and SEIR models (`if2`: epipf_if2) and for the subgroup models with up to four
groups (`if2_subgroups`: epipf_iterated_filtering_subgroups, §17.1), on the GPU.

The reference has no counterpart: its PMCMC scripts take their start point and proposal covariance from an earlier,
hand-tuned run.  `if2` finds a usable theta from data alone:

    res = epipf.if2(Y, ModelType.SIR, start=[1.2, 0.5], rw=[0.1, 0.05], iterations=50, cooling=0.5,
                    n_particles=1000, n_population=300, mu=5, probs=.5, searches=4)
    theta0 = list(res.theta[res.best])                     # the start point of particle_mcmc

Each iteration is one pass of the bootstrap filter in which every particle carries its own parameter vector, jittered
uniformly by +-hw[m] at every step (reflected at 0), so that resampling selects parameters as well as states; the
half-widths shrink as hw[m] = rw * cooling ** (m / 50) (pomp's cooling.fraction.50) and the swarm contracts onto the
maximum-likelihood estimate.  `probs` is fixed.  Independent searches run as the chains of one batch.

Random numbers: key = the module stream (`epipf.seed_stream`), search s under chain_key(key, s), iteration m at filter
index filter_index + m (taken from the stream's counter, which advances by the iterations run).  The evaluation
filters of search s run under chain_key(key, searches + s) at filter indices 0..7: keys no search uses.
"""
import numpy as np

from . import _lib
from . import engine as _engine
from .pmcmc import _STREAM, _check_Y, _population, chain_key

EVALUATION_FILTERS = 8
DIMS = {_lib.SIR: 2, _lib.SEIR: 3}


def cooling_table(rw, cooling, iterations, first=0):
    """hw[m] = rw * cooling ** (m / 50.0) for m = first .. first + iterations - 1, in Python float64."""
    rw = [float(v) for v in np.asarray(rw, dtype=np.float64).reshape(-1)]
    return np.array([[v * float(cooling) ** (m / 50.0) for v in rw] for m in range(first, first + iterations)],
                    dtype=np.float64).reshape(iterations, len(rw))


def log_mean_exp(ll):
    """log(mean(exp(ll))) along the last axis; -inf where every entry is -inf."""
    ll = np.asarray(ll, dtype=np.float64)
    top = ll.max(axis=-1)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(top), safe + np.log(np.mean(np.exp(ll - safe[..., None]), axis=-1)), -np.inf)


class If2Result:
    """theta [S, d]: each search's final swarm mean; trace [S, M, d]: the swarm means after each iteration (NaN from a
    search's failed iteration on); loglik [S, M]: the perturbed model's log-likelihood of each pass; swarm [S, N, d];
    status [S] (STATUS_*); iterations_done [S]; with evaluate: loglik_at_theta [S] (unperturbed filters at theta,
    log-mean-exp over 8) and best (its argmax), else None."""

    def __init__(self, run, theta, trace, loglik, swarm, status, iterations_done, loglik_at_theta, groups=None):
        self._run = run
        self.groups = groups                             # G of the subgroup models (if2_subgroups), else None
        self.theta, self.trace, self.loglik, self.swarm = theta, trace, loglik, swarm
        self.status, self.iterations_done = status, iterations_done
        self.loglik_at_theta = loglik_at_theta
        self.best = None if loglik_at_theta is None else int(np.argmax(loglik_at_theta))

    @property
    def beta(self):
        """theta's contact matrices [S, G, G] (a view; subgroup models only)."""
        if self.groups is None:
            raise AttributeError("beta exists for the subgroup models' results (if2_subgroups)")
        G = self.groups
        return self.theta[:, :G * G].reshape(-1, G, G)

    @property
    def gamma(self):
        """theta's recovery rates [S] (a view; subgroup models only)."""
        if self.groups is None:
            raise AttributeError("gamma exists for the subgroup models' results (if2_subgroups)")
        return self.theta[:, -1]

    def continue_(self, iterations):
        """`iterations` more from this result's swarm: the next filter indices and the next rows of the cooling table.
        Every search runs on from the swarm it returned.  The new result's trace and loglik hold every iteration so
        far, its iterations_done their sum, its status the continuation's."""
        return self._run(self.swarm, self.trace.shape[1], int(iterations), self)


def _search(mid, G, call, Y, start, rw, iterations, cooling, n_particles, n_population, mu, observations, probs,
            searches, evaluate, key, filter_index, device):
    """The search both entry points run: `start` [S, d] and `rw` [d] are checked and flat, `call` names the engine's
    method (Engine.if2 / Engine.if2_subgroups)."""
    S, N, M = int(searches), int(n_particles), int(iterations)
    Y = _check_Y(mid, G, Y)
    npop, mus = _population(mid, G, n_population, mu)
    k = _STREAM.key if key is None else int(key)
    own_stream = filter_index is None
    f0 = _STREAM.next_filter if own_stream else int(filter_index)
    keys = np.array([chain_key(k, s) for s in range(S)], dtype=np.uint64)
    eval_keys = np.array([chain_key(k, S + s) for s in range(S)], dtype=np.uint64)
    eng = _engine.get_engine(mid, G, N, Y.shape[0], S * EVALUATION_FILTERS if evaluate else S, device)

    def run(swarm, first, n_iter, before):
        eng.set_observations(Y)
        eng.set_population(npop, mus)
        hw = cooling_table(rw, cooling, n_iter, first)
        swarm, mean, lz, done, st = getattr(eng, call)(swarm, hw, probs, keys, f0 + first, observations=observations)
        if own_stream:
            _STREAM.next_filter = max(_STREAM.next_filter, f0 + first + n_iter)
        theta = np.array([mean[s, done[s] - 1] if done[s] > 0 else swarm[s].mean(axis=0) for s in range(S)])
        at_theta = None
        if evaluate:
            E = EVALUATION_FILTERS
            elz, est = eng.run(np.repeat(theta, E, axis=0), probs, np.repeat(eval_keys, E), np.tile(np.arange(E), S),
                               observations=observations)
            ll = np.where(est == _lib.STATUS_OK, elz[:, -1], -np.inf).reshape(S, E)
            at_theta = log_mean_exp(ll)
        trace, loglik = mean, lz[:, :, -1]
        if before is not None:
            trace = np.concatenate([before.trace, trace], axis=1)
            loglik = np.concatenate([before.loglik, loglik], axis=1)
            done = before.iterations_done + done
        return If2Result(run, theta, trace, loglik, swarm, st, done, at_theta, G if mid >= _lib.SIR_SUBGROUPS else None)

    return run(np.repeat(start[:, None, :], N, axis=1), 0, M, None)


def if2(Y, type_model, start, rw, iterations=50, cooling=0.5, n_particles=1000, n_population=4820, mu=20,
        observations=False, probs=.1, searches=1, evaluate=True, *, key=None, filter_index=None, device=0):
    mid = _engine.model_id(type_model)
    if mid not in DIMS:
        raise ValueError("if2 covers the SIR and SEIR models; the subgroup models are out of its scope "
                         "(epipf.if2_subgroups runs them)")
    d = DIMS[mid]
    S, M = int(searches), int(iterations)
    if S < 1 or M < 1:
        raise ValueError("searches and iterations must be >= 1")
    start = np.asarray(start, dtype=np.float64)
    if start.shape not in ((d,), (S, d)):
        raise ValueError(f"start must be [{d}] or [{S}, {d}], got {start.shape}")
    start = np.ascontiguousarray(np.broadcast_to(start, (S, d)))
    rw = np.asarray(rw, dtype=np.float64).reshape(-1)
    if rw.size != d or not (rw >= 0).all() or not (start >= 0).all():
        raise ValueError(f"rw needs {d} entries; rw and start must be >= 0")
    return _search(mid, 1, "if2", Y, start, rw, iterations, cooling, n_particles, n_population, mu, observations, probs,
                   searches, evaluate, key, filter_index, device)


MAX_SUBGROUPS = 4                                        # per-particle rates exist for G <= 4


def _is_pair(v):
    """The reference's (beta[G][G], gamma): two entries, a square matrix and a scalar."""
    try:
        if len(v) != 2:
            return False
        beta = np.asarray(v[0], dtype=np.float64)
        return beta.ndim == 2 and beta.shape[0] == beta.shape[1] and np.ndim(v[1]) == 0
    except (TypeError, ValueError):
        return False


def flatten_theta(v):
    """(beta[G][G], gamma) -> ([G*G + 1], G): beta row-major, then gamma (theta_vector's layout)."""
    beta = np.asarray(v[0], dtype=np.float64)
    return np.append(beta.reshape(-1), float(v[1])), beta.shape[0]


def if2_subgroups(Y, type_model, start, rw, iterations=50, cooling=0.5, n_particles=1000, n_population=(2410, 2410),
                  mu=(10, 10), observations=False, probs=.1, searches=1, evaluate=True, *, key=None, filter_index=None,
                  device=0):
    """`if2` for SIR_SUBGROUPS / SIR_SUBGROUPS2 with G = 2..4 groups (epipf_iterated_filtering_subgroups): theta is
    beta[G][G] row-major then gamma, d = G*G + 1.  `start` is flat ([d] or [S, d]), the reference's (beta[G][G], gamma),
    or a list of S such pairs; `rw` is flat [d] or a pair.  G comes from beta, or from len(mu) for flat input.  An rw
    entry of 0 keeps that component fixed bit for bit (for example off-diagonal contacts at 0).  The result has
    `.beta` [S, G, G] and `.gamma` [S]; list(res.theta[res.best]) is particle_mcmc's flat params."""
    mid = _engine.model_id(type_model)
    if mid in DIMS:
        raise ValueError("if2_subgroups covers the subgroup models; epipf.if2 runs SIR and SEIR")
    S, M = int(searches), int(iterations)
    if S < 1 or M < 1:
        raise ValueError("searches and iterations must be >= 1")
    G = None
    if _is_pair(start):
        start, G = flatten_theta(start)
    elif len(start) == S and all(_is_pair(v) for v in start):
        rows = [flatten_theta(v) for v in start]
        if len({g for _, g in rows}) != 1:
            raise ValueError("every search's beta must have the same shape")
        start, G = np.array([r for r, _ in rows]), rows[0][1]
    if _is_pair(rw):
        rw, Gr = flatten_theta(rw)
        if G is not None and Gr != G:
            raise ValueError(f"rw's beta is {Gr} x {Gr}, start's {G} x {G}")
        G = Gr
    if G is None:
        G = int(np.atleast_1d(np.asarray(mu)).size)
    if G < 2 or G > MAX_SUBGROUPS:
        raise ValueError(f"if2_subgroups needs 2 <= G <= {MAX_SUBGROUPS} groups (per-particle rates exist for G <= 4), got {G}")
    d = G * G + 1
    start = np.asarray(start, dtype=np.float64)
    if start.shape not in ((d,), (S, d)):
        raise ValueError(f"start must be [{d}], [{S}, {d}] or (beta[{G}][{G}], gamma), got {start.shape}")
    start = np.ascontiguousarray(np.broadcast_to(start, (S, d)))
    rw = np.asarray(rw, dtype=np.float64).reshape(-1)
    if rw.size != d or not (rw >= 0).all() or not (start >= 0).all():
        raise ValueError(f"rw needs {d} entries; rw and start must be >= 0")
    return _search(mid, G, "if2_subgroups", Y, start, rw, iterations, cooling, n_particles, n_population, mu,
                   observations, probs, searches, evaluate, key, filter_index, device)
