"""Engine: one libepipf context (device buffers for a model / particle-count / horizon / chain batch).

This is the layer the drop-in `particle_filter` / `particle_mcmc` call.  An engine keeps the
observations, the log-factorial table and the whole particle history resident in HBM; a batched
`run()` moves only per-chain parameters in and log-likelihoods + status out.
"""
import atexit
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check, ptr

# Particle-steps of every epipf_run in this process, counted as bench.py's `value` counts them (N x T per chain that
# runs a filter; chains passed as inactive count nothing).  With EPIPF_PMC_COUNT=<file> the total is appended to <file>
# at exit: scripts/profile.sh divides each rocprofv3 pass's counter totals by it (scripts/parse_rocprof.py).
_PARTICLE_STEPS = [0]


def _write_pmc_count():
    with open(os.environ["EPIPF_PMC_COUNT"], "a") as f:
        f.write(f"{_PARTICLE_STEPS[0]}\n")


if os.environ.get("EPIPF_PMC_COUNT"):
    atexit.register(_write_pmc_count)

MODEL_IDS = {"sir": _lib.SIR, "seir": _lib.SEIR, "sir_subgroups": _lib.SIR_SUBGROUPS,
             "sir_subgroups2": _lib.SIR_SUBGROUPS2}


def model_id(type_model):
    """Accept this package's ModelType, the reference's ModelType (same .value strings) or a string."""
    name = getattr(type_model, "value", type_model)
    if isinstance(name, (int, np.integer)) and 0 <= int(name) <= 3:
        return int(name)
    if isinstance(name, str) and name.lower() in MODEL_IDS:
        return MODEL_IDS[name.lower()]
    raise ValueError(f"unknown model type {type_model!r}")


def n_compartments(mid, G):
    return 3 if mid == _lib.SIR else 4 if mid == _lib.SEIR else 3 * G


def max_groups():
    """Largest G of the subgroup models (epipf_max_groups)."""
    return int(_lib.load().epipf_max_groups())


def check_groups(mid, G):
    """The subgroup models' G against the library's limit, before any context is created."""
    if mid >= _lib.SIR_SUBGROUPS and int(G) > max_groups():
        raise ValueError(f"subgroup models support at most {max_groups()} groups, got {int(G)}")


def theta_vector(mid, theta):
    """Flatten a reference theta: SIR/SEIR arrays, or (beta[G][G], gamma) for the subgroup models
    (pmcmc.py:211-218 passes theta_proposal[0], theta_proposal[1])."""
    if mid in (_lib.SIR_SUBGROUPS, _lib.SIR_SUBGROUPS2):
        beta, gamma = theta
        beta = np.asarray(beta, dtype=np.float64)
        if beta.ndim != 2 or beta.shape[0] != beta.shape[1]:
            raise ValueError("subgroup theta must be (beta[G][G], gamma)")
        check_groups(mid, beta.shape[0])
        return np.append(beta.reshape(-1), float(gamma)), beta.shape[0]
    th = np.asarray(theta, dtype=np.float64).reshape(-1)
    need = 2 if mid == _lib.SIR else 3
    if th.size != need:
        raise ValueError(f"theta must have {need} entries for this model, got {th.size}")
    return th, 1


def dispersion_vector(dispersion, n, observations=False):
    """A negative-binomial dispersion (a scalar or [n]) as contiguous float64 [n]; not with observations=True.  The values
    are the callers' to check (epipf.incidence states the model's domain, the library refuses the rest)."""
    if observations:
        raise ValueError("dispersion is the negative-binomial model's: it does not go with observations=True")
    kap = np.asarray(dispersion, dtype=np.float64)
    if kap.shape not in ((), (n,)):
        raise ValueError(f"dispersion must be a scalar or [{n}], got {kap.shape}")
    return np.ascontiguousarray(np.broadcast_to(kap, (n,)))


class Engine:
    def __init__(self, type_model, groups=1, n_particles=1000, t_max=1, max_chains=1, device=0):
        L = _lib.load()
        self.model = model_id(type_model)
        self.G = int(groups) if self.model >= _lib.SIR_SUBGROUPS else 1
        check_groups(self.model, self.G)
        self.C = n_compartments(self.model, self.G)
        self.K = 3 if self.model == _lib.SIR_SUBGROUPS2 else self.C
        self.N = int(n_particles)
        self.t_max = int(t_max)
        self.max_chains = int(max_chains)
        self.device = int(device)
        h = ctypes.c_void_p()
        check(L.epipf_create(ctypes.byref(h), self.device, self.model, self.G, self.N, self.t_max, self.max_chains),
              "epipf_create")
        self._h = h
        self._L = L
        self._Y = None
        self._pop = None
        self.bound_to = None                             # token of the ChainSampler whose data is loaded (_bind)
        self.T = 0                                       # rows of the observations (set_observations)
        self._run_T = None                               # rows of the last run, as the context holds them (last_T)
        self._last_n = None
        self.run_serial = 0                              # filters run so far: each overwrites the resident history

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.epipf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ inputs
    def set_observations(self, Y):
        Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64))
        if Y.ndim != 2:
            raise ValueError("Y must be 2-D [T, K]")
        if self._Y is not None and self._Y.shape == Y.shape and np.array_equal(self._Y, Y, equal_nan=True):
            return
        check(self._L.epipf_set_observations(self._h, ptr(Y), Y.shape[0], Y.shape[1]), "epipf_set_observations")
        self._Y = Y.copy()
        self.bound_to = None                             # ChainSampler._bind: the data it bound is gone
        self.T = Y.shape[0]

    def set_population(self, n_population, mu):
        npop = np.ascontiguousarray(np.atleast_1d(np.asarray(n_population, dtype=np.float64)))
        mus = np.ascontiguousarray(np.atleast_1d(np.asarray(mu, dtype=np.float64)))
        if npop.size != self.G or mus.size != self.G:
            raise ValueError(f"n_population and mu need {self.G} entries")
        key = (tuple(npop), tuple(mus))
        if key == self._pop:
            return
        check(self._L.epipf_set_population(self._h, ptr(npop), ptr(mus)), "epipf_set_population")
        self._pop = key
        self.bound_to = None

    @property
    def run_T(self):
        """Rows of the last run's history: the observations' T after run / if2 / walk_filter, D + 2 after run_incidence
        and walk_incidence (before any run: T).  history(), path_sample(), smooth(), incidence_smooth(), walk_history()
        and walk_smooth() are sized by it, as the library writes them, whatever set_observations did since."""
        return self.T if self._run_T is None else self._run_T

    # ------------------------------------------------------------------ the filter
    def run(self, thetas, probs, keys, filter_indices, observations=False, active=None, resample="multinomial",
            chosen=None):
        """Run len(thetas) independent filters.  Returns (log_zetas [n, T], status [n]); with chosen [n] (the path
        sampler's final particles, -1 for none) also the sampled trajectories [n, T, C] int32 (epipf_run_sampled)."""
        thetas = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
        n = thetas.shape[0]
        probs = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, dtype=np.float64), (n,)))
        keys = np.ascontiguousarray(np.broadcast_to(np.asarray(keys, dtype=np.uint64), (n,)))
        fidx = np.ascontiguousarray(np.broadcast_to(np.asarray(filter_indices, dtype=np.uint64), (n,))
                                    .astype(np.uint32))
        act = None if active is None else np.ascontiguousarray(np.asarray(active, dtype=np.int32))
        lz = np.empty((n, self.T), dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        mode = _lib.RESAMPLE_MULTINOMIAL if resample == "multinomial" else _lib.RESAMPLE_SYSTEMATIC
        obs = _lib.OBS_NORMAL if observations else _lib.OBS_BINOMIAL
        if chosen is None:
            check(self._L.epipf_run(self._h, n, ptr(thetas), thetas.shape[1], obs, ptr(probs), ptr(keys), ptr(fidx),
                                    ptr(act), mode, ptr(lz), ptr(st)), "epipf_run")
        else:
            ch = np.ascontiguousarray(np.asarray(chosen, dtype=np.int32).reshape(-1))
            if ch.size != n:
                raise ValueError(f"chosen has {ch.size} entries for {n} filters")
            tr = np.empty((n, self.T, self.C), dtype=np.int32)
            check(self._L.epipf_run_sampled(self._h, n, ptr(thetas), thetas.shape[1], obs, ptr(probs), ptr(keys),
                                            ptr(fidx), ptr(act), mode, ptr(ch), ptr(lz), ptr(st), ptr(tr)),
                  "epipf_run_sampled")
        self._last_n = n
        self.run_serial += 1
        self._run_T = self.T
        self._last_status = st.copy()                    # Engine.smooth: rows of chains that did not run are NaN
        _PARTICLE_STEPS[0] += (n if act is None else int(np.count_nonzero(act))) * self.N * self.T
        return (lz, st) if chosen is None else (lz, st, tr)

    def run_incidence(self, thetas, probs, keys, filter_indices, counts, observations=False, cumulate=False,
                      active=None, dispersion=None):
        """epipf_run_incidence: len(thetas) filters on the reported transition counts `counts` [D, F] (F = 2 for SIR:
        infections, removals; 3 for SEIR: exposures, onsets, removals; NaN = not reported), shared by the chains.
        Returns (log_zetas [n, D + 2], status [n]); run_T becomes D + 2 (T stays the observations'), and history(),
        path_sample() and smooth() see the pass afterwards.  dispersion (a scalar or [n]): the reports are negative
        binomial with mean probs x flow and this dispersion (epipf_run_incidence_negbin) instead."""
        thetas = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
        if thetas.ndim != 2:
            raise ValueError("thetas must be [chains, d]")
        n = thetas.shape[0]
        counts = np.ascontiguousarray(np.asarray(counts, dtype=np.float64))
        F = 2 if self.model == _lib.SIR else 3
        if counts.ndim != 2 or counts.shape[1] != F:
            raise ValueError(f"counts must be [D, {F}] for this model")
        D = counts.shape[0]
        probs = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, dtype=np.float64), (n,)))
        keys = np.ascontiguousarray(np.broadcast_to(np.asarray(keys, dtype=np.uint64), (n,)))
        fidx = np.ascontiguousarray((np.broadcast_to(np.asarray(filter_indices, dtype=np.uint64), (n,))
                                     & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        act = None if active is None else np.ascontiguousarray(np.asarray(active, dtype=np.int32))
        if act is not None and act.shape != (n,):
            raise ValueError(f"active must have {n} entries")
        lz = np.empty((n, D + 2), dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        if dispersion is not None:
            kap = dispersion_vector(dispersion, n, observations)
            check(self._L.epipf_run_incidence_negbin(self._h, n, ptr(thetas), thetas.shape[1], ptr(probs), ptr(kap),
                                                     ptr(keys), ptr(fidx), ptr(act), ptr(counts), D,
                                                     1 if cumulate else 0, ptr(lz), ptr(st)),
                  "epipf_run_incidence_negbin")
        else:
            obs = _lib.OBS_NORMAL if observations else _lib.OBS_BINOMIAL
            check(self._L.epipf_run_incidence(self._h, n, ptr(thetas), thetas.shape[1], obs, ptr(probs), ptr(keys),
                                              ptr(fidx), ptr(act), ptr(counts), D, 1 if cumulate else 0, ptr(lz),
                                              ptr(st)),
                  "epipf_run_incidence")
        self._run_T = D + 2
        self._last_n = n
        self.run_serial += 1
        self._last_status = st.copy()
        _PARTICLE_STEPS[0] += (n if act is None else int(np.count_nonzero(act))) * self.N * (D + 2)
        return lz, st

    def if2(self, swarm, half_widths, probs, keys, filter_index0, observations=False):
        """epipf_if2: iterated filtering from the swarms [S, N, d] with the half-width table [M, d], search s at filter
        indices filter_index0[s] + m.  Returns (swarm [S, N, d], mean [S, M, d], log_zetas [S, M, T],
        iterations_done [S], status [S]); history() afterwards holds each search's last executed pass."""
        return self._if2("epipf_if2", swarm, half_widths, probs, keys, filter_index0, observations)

    def if2_subgroups(self, swarm, half_widths, probs, keys, filter_index0, observations=False):
        """epipf_iterated_filtering_subgroups: if2() for the subgroup models at G = 2..4, d = G*G + 1 with theta laid
        out as beta[G][G] row-major, then gamma.  Arguments and returns as if2()."""
        return self._if2("epipf_iterated_filtering_subgroups", swarm, half_widths, probs, keys, filter_index0,
                         observations)

    def _if2(self, entry, swarm, half_widths, probs, keys, filter_index0, observations):
        swarm = np.array(swarm, dtype=np.float64, order="C")          # a copy: the library writes the result into it
        hw = np.ascontiguousarray(np.asarray(half_widths, dtype=np.float64))
        if swarm.ndim != 3 or swarm.shape[1] != self.N:
            raise ValueError(f"swarm must be [searches, {self.N}, d]")
        S, _, d = swarm.shape
        if hw.ndim != 2 or hw.shape[1] != d:
            raise ValueError(f"half_widths must be [iterations, {d}]")
        M = hw.shape[0]
        probs = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,)))
        keys = np.ascontiguousarray(np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,)))
        f0 = np.ascontiguousarray((np.broadcast_to(np.asarray(filter_index0, dtype=np.uint64), (S,))
                                   & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        lz = np.empty((S, M, self.T), dtype=np.float64)
        mean = np.empty((S, M, d), dtype=np.float64)
        done = np.zeros(S, dtype=np.int32)
        st = np.empty(S, dtype=np.int32)
        obs = _lib.OBS_NORMAL if observations else _lib.OBS_BINOMIAL
        check(getattr(self._L, entry)(self._h, S, M, ptr(swarm), d, ptr(hw), obs, ptr(probs), ptr(keys), ptr(f0),
                                      ptr(lz), ptr(mean), ptr(done), ptr(st)), entry)
        self._last_n = S
        self.run_serial += 1
        self._run_T = self.T
        self._last_status = st.copy()
        _PARTICLE_STEPS[0] += int(np.minimum(done + 1, M).sum()) * self.N * self.T
        return swarm, mean, lz, done, st

    def history(self, n_chains=None):
        """(hidden [n, T, N, C] int32, ancestry [n, T, N] int32) of the last run."""
        n = self._last_n if n_chains is None else int(n_chains)
        hid = np.empty((n, self.run_T, self.N, self.C), dtype=np.int32)
        anc = np.empty((n, self.run_T, self.N), dtype=np.int32)
        check(self._L.epipf_copy_history(self._h, n, ptr(hid), ptr(anc)), "epipf_copy_history")
        return hid, anc

    def path_sample(self, chosen):
        chosen = np.ascontiguousarray(np.asarray(chosen, dtype=np.int32).reshape(-1))
        out = np.empty((chosen.size, self.run_T, self.C), dtype=np.int32)
        check(self._L.epipf_path_sample(self._h, chosen.size, ptr(chosen), ptr(out)), "epipf_path_sample")
        return out

    # ------------------------------------------------------------------ aux entry points
    def simulate(self, states, theta, max_time=1.0, key=0, filter_index=0, step=0):
        states = np.ascontiguousarray(np.asarray(states, dtype=np.int32).reshape(-1, self.C))
        th, _ = theta_vector(self.model, theta)
        th = np.ascontiguousarray(th)
        out = np.empty_like(states)
        ev = np.zeros(1, dtype=np.int64)
        check(self._L.epipf_simulate(self._h, states.shape[0], ptr(states), ptr(th), th.size, float(max_time),
                                     int(key) & (2**64 - 1), int(filter_index) & 0xFFFFFFFF, int(step), ptr(out),
                                     ptr(ev)), "epipf_simulate")
        return out, int(ev[0])

    def simulate_path(self, states, theta, max_time=1.0, key=0, filter_index=0, step=0, max_events=None):
        """Full event paths from int states [n, C]: (times [n, cap], states [n, cap, C] int32, n_events [n],
        final [n, C] int32); row j holds trajectory j's first n_events[j] events.  With max_events=None the buffer
        grows to the longest path (a second call with the same draws when the first guess was short)."""
        states = np.ascontiguousarray(np.asarray(states, dtype=np.int32).reshape(-1, self.C))
        th, _ = theta_vector(self.model, theta)
        th = np.ascontiguousarray(th)
        n = states.shape[0]
        cap = 1024 if max_events is None else int(max_events)
        while True:
            t = np.empty((n, max(cap, 1)))
            x = np.empty((n, max(cap, 1), self.C), dtype=np.int32)
            nev = np.zeros(n, dtype=np.int32)
            fin = np.empty((n, self.C), dtype=np.int32)
            check(self._L.epipf_simulate_path(self._h, n, ptr(states), ptr(th), th.size, float(max_time),
                                              int(key) & (2**64 - 1), int(filter_index) & 0xFFFFFFFF, int(step), cap,
                                              ptr(t), ptr(x), ptr(nev), ptr(fin)), "epipf_simulate_path")
            longest = int(nev.max()) if n else 0
            if max_events is not None or longest <= cap:
                return t[:, :cap], x[:, :cap], nev, fin
            cap = longest

    def forecast(self, thetas, states, horizon, replicates=1, key=0, filter_index=0, step=0, rows=True, bins=0):
        """epipf_forecast: draw d (thetas[d] flat [D, d], states[d] [D, C]) simulated `replicates` times over
        [0, horizon] and binned to daily rows.  Returns (rows [D, R, H, C] int32 or None, sums [H, C] int64,
        hist [H, C, bins] uint32 or None when bins == 0, events)."""
        thetas = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
        states = np.ascontiguousarray(np.asarray(states, dtype=np.int32).reshape(-1, self.C))
        D, H, R = states.shape[0], int(horizon), int(replicates)
        if thetas.ndim != 2 or thetas.shape[0] != D:
            raise ValueError(f"thetas must be [{D}, d], one row per start state")
        out = np.empty((D, R, H, self.C), dtype=np.int32) if rows else None
        sums = np.zeros((H, self.C), dtype=np.int64)
        hist = np.zeros((H, self.C, int(bins)), dtype=np.uint32) if bins else None
        ev = np.zeros(1, dtype=np.int64)
        check(self._L.epipf_forecast(self._h, D, R, H, ptr(thetas), thetas.shape[1], ptr(states),
                                     int(key) & (2**64 - 1), int(filter_index) & 0xFFFFFFFF, int(step), ptr(out),
                                     ptr(sums), ptr(hist), int(bins), ptr(ev)), "epipf_forecast")
        return out, sums, hist, int(ev[0])

    def forecast_summary(self, thetas, states, horizon, replicates=1, key=0, filter_index=0, step=0, per_path=False,
                         bins=0):
        """epipf_forecast_summary: path functionals of forecast()'s trajectories (same arguments, same paths).  Returns
        a dict of the raw arrays: totals [4] int64 (sum of peak, sum of infections, extinct paths, sum of events),
        peak_day [H], extinct_day [H + 1], extinct_per_draw [D] uint32, peak_hist / infections_hist [bins] uint32 (None
        when bins == 0), and paths: None, or (peak int32, peak_time, extinction_time float64, infections, events int32),
        each [D, R]."""
        thetas = np.ascontiguousarray(np.asarray(thetas, dtype=np.float64))
        states = np.ascontiguousarray(np.asarray(states, dtype=np.int32).reshape(-1, self.C))
        D, H, R = states.shape[0], int(horizon), int(replicates)
        if thetas.ndim != 2 or thetas.shape[0] != D:
            raise ValueError(f"thetas must be [{D}, d], one row per start state")
        paths = None
        if per_path:
            paths = tuple(np.zeros((D, max(R, 0)), dtype=t) for t in (np.int32, np.float64, np.float64, np.int32, np.int32))
        pp = paths or (None,) * 5
        totals = np.zeros(4, dtype=np.int64)
        peak_day = np.zeros(max(H, 0), dtype=np.uint32)
        extinct_day = np.zeros(max(H, 0) + 1, dtype=np.uint32)
        per_draw = np.zeros(D, dtype=np.uint32)
        peak_hist = np.zeros(int(bins), dtype=np.uint32) if bins else None
        inf_hist = np.zeros(int(bins), dtype=np.uint32) if bins else None
        check(self._L.epipf_forecast_summary(self._h, D, R, H, ptr(thetas), thetas.shape[1], ptr(states),
                                             int(key) & (2**64 - 1), int(filter_index) & 0xFFFFFFFF, int(step),
                                             ptr(pp[0]), ptr(pp[1]), ptr(pp[2]), ptr(pp[3]), ptr(pp[4]), ptr(totals),
                                             ptr(peak_hist), ptr(inf_hist), int(bins), ptr(peak_day), ptr(extinct_day),
                                             ptr(per_draw)), "epipf_forecast_summary")
        return dict(totals=totals, peak_day=peak_day, extinct_day=extinct_day, extinct_per_draw=per_draw,
                    peak_hist=peak_hist, infections_hist=inf_hist, paths=paths)

    def smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), lineage="genealogy", kind="smoothing", bins=None,
               lag=None):
        """Daily means, quantiles and surviving-lineage counts of the last run's first n_chains chains, from the history
        resident on the device (epipf_smooth; epipf.smoothing has the definition).  Returns Smoothed with a leading
        chain axis: mean [n, T, C], quantiles [n, Q, T, C] or None, lineages [n, T], sums [n, T, C], zetas None.  Rows
        of chains whose last status was not OK are NaN in mean and 0 elsewhere.  bins defaults to the population total
        + 1 (every model conserves it).  lag=L: the fixed-lag smoother instead (epipf_smooth_lag)."""
        from . import smoothing
        lin, knd, q = smoothing.check_options(lineage, kind, quantiles)
        lag = smoothing.check_lag(lag, kind)
        n = int(n_chains) if n_chains is not None else self._last_n or 1   # before any run: the library's EPIPF_ESTATE
        if bins is None:
            if self._pop is None:
                raise ValueError("bins=None needs set_population")
            bins = int(sum(self._pop[0])) + 1
        nq = 0 if q is None else q.size
        rows = max(n, 1)                                  # a bad n_chains is the library's EPIPF_EINVAL
        sums = np.zeros((rows, self.run_T, self.C), dtype=np.int64)
        lineages = np.zeros((rows, self.run_T), dtype=np.int32)
        quant = np.zeros((rows, nq, self.run_T, self.C), dtype=np.int32) if nq else None
        if lag is None:
            check(self._L.epipf_smooth(self._h, n, lin, knd, ptr(q), nq, int(bins) if nq else 0, ptr(sums), ptr(quant),
                                       ptr(lineages)), "epipf_smooth")
        else:
            check(self._L.epipf_smooth_lag(self._h, n, lin, min(lag, 2**31 - 1), ptr(q), nq, int(bins) if nq else 0,
                                           ptr(sums), ptr(quant), ptr(lineages)), "epipf_smooth_lag")
        mean = sums / float(self.N)
        mean[self._last_status[:n] != _lib.STATUS_OK] = np.nan
        return smoothing.Smoothed(mean, None if quant is None else quant.astype(np.int64), lineages, sums, None)

    def smooth_history(self, hidden, ancestry, lineage, kind, q, bins, lag=None):
        """epipf_smooth_history on int32 host arrays hidden [n, T, N, C], ancestry [n, T, N] (this engine's model and N
        are ignored): (sums [n, T, C] int64, quantiles [n, Q, T, C] int32 or None, lineages [n, T] int32).  lag=L (an
        integer >= 0, with kind EPIPF_SMOOTH_SMOOTHING): epipf_smooth_lag_history."""
        from . import smoothing
        lag = smoothing.check_lag(lag, "predictive" if int(kind) == _lib.SMOOTH_PREDICTIVE else "smoothing")
        hidden = np.ascontiguousarray(hidden, dtype=np.int32)
        ancestry = np.ascontiguousarray(ancestry, dtype=np.int32)
        n, T, N, C = hidden.shape
        nq = 0 if q is None else q.size
        sums = np.zeros((n, T, C), dtype=np.int64)
        lineages = np.zeros((n, T), dtype=np.int32)
        quant = np.zeros((n, nq, T, C), dtype=np.int32) if nq else None
        if lag is None:
            check(self._L.epipf_smooth_history(self._h, n, T, N, C, ptr(hidden), ptr(ancestry), int(lineage), int(kind),
                                               ptr(q), nq, int(bins) if nq else 0, ptr(sums), ptr(quant),
                                               ptr(lineages)), "epipf_smooth_history")
        else:
            check(self._L.epipf_smooth_lag_history(self._h, n, T, N, C, ptr(hidden), ptr(ancestry), int(lineage),
                                                   min(lag, 2**31 - 1), ptr(q), nq, int(bins) if nq else 0, ptr(sums),
                                                   ptr(quant), ptr(lineages)), "epipf_smooth_lag_history")
        return sums, quant, lineages

    # ------------------------------------------------------------------ time-varying rates (epipf.walk)
    def walk_filter(self, swarm, half_widths, probs, keys, filter_index, observations=False):
        """epipf_walk_filter: the random-walk filter from the swarms [S, N, d] with chain s's half-widths
        half_widths[s] ([S, d]).  Returns (log_zetas [S, T], status [S]); history(), smooth(), walk_history() and
        walk_smooth() see the pass afterwards."""
        swarm = np.ascontiguousarray(np.asarray(swarm, dtype=np.float64))
        hw = np.ascontiguousarray(np.asarray(half_widths, dtype=np.float64))
        if swarm.ndim != 3 or swarm.shape[1] != self.N:
            raise ValueError(f"swarm must be [chains, {self.N}, d]")
        S, _, d = swarm.shape
        if hw.shape != (S, d):
            raise ValueError(f"half_widths must be [{S}, {d}]")
        probs = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,)))
        keys = np.ascontiguousarray(np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,)))
        f = np.ascontiguousarray((np.broadcast_to(np.asarray(filter_index, dtype=np.uint64), (S,))
                                  & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        lz = np.empty((S, self.T), dtype=np.float64)
        st = np.empty(S, dtype=np.int32)
        obs = _lib.OBS_NORMAL if observations else _lib.OBS_BINOMIAL
        check(self._L.epipf_walk_filter(self._h, S, ptr(swarm), d, ptr(hw), obs, ptr(probs), ptr(keys), ptr(f), ptr(lz),
                                        ptr(st)), "epipf_walk_filter")
        self._last_n = S
        self.run_serial += 1
        self._run_T = self.T
        self._last_status = st.copy()
        _PARTICLE_STEPS[0] += S * self.N * self.T
        return lz, st

    def walk_incidence(self, swarm, half_widths, probs, keys, filter_index, counts, observations=False, cumulate=False,
                       dispersion=None):
        """epipf_incidence_walk: the random-walk filter from the swarms [S, N, d] with chain s's half-widths
        half_widths[s] ([S, d]), weighted by the reported transition counts `counts` [D, F] as run_incidence weighs
        them.  Returns (log_zetas [S, D + 2], status [S]); run_T becomes D + 2, and history(), path_sample(), smooth(),
        walk_history(), walk_smooth() and incidence_smooth() see the pass afterwards.  dispersion (a scalar or [S]):
        negative-binomial reports instead (epipf_incidence_walk_negbin)."""
        swarm = np.ascontiguousarray(np.asarray(swarm, dtype=np.float64))
        hw = np.ascontiguousarray(np.asarray(half_widths, dtype=np.float64))
        if swarm.ndim != 3 or swarm.shape[1] != self.N:
            raise ValueError(f"swarm must be [chains, {self.N}, d]")
        S, _, d = swarm.shape
        if hw.shape != (S, d):
            raise ValueError(f"half_widths must be [{S}, {d}]")
        counts = np.ascontiguousarray(np.asarray(counts, dtype=np.float64))
        F = 2 if self.model == _lib.SIR else 3
        if counts.ndim != 2 or counts.shape[1] != F:
            raise ValueError(f"counts must be [D, {F}] for this model")
        D = counts.shape[0]
        probs = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,)))
        keys = np.ascontiguousarray(np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,)))
        f = np.ascontiguousarray((np.broadcast_to(np.asarray(filter_index, dtype=np.uint64), (S,))
                                  & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        lz = np.empty((S, D + 2), dtype=np.float64)
        st = np.empty(S, dtype=np.int32)
        if dispersion is not None:
            kap = dispersion_vector(dispersion, S, observations)
            check(self._L.epipf_incidence_walk_negbin(self._h, S, ptr(swarm), d, ptr(hw), ptr(probs), ptr(kap), ptr(keys),
                                                      ptr(f), ptr(counts), D, 1 if cumulate else 0, ptr(lz), ptr(st)),
                  "epipf_incidence_walk_negbin")
        else:
            obs = _lib.OBS_NORMAL if observations else _lib.OBS_BINOMIAL
            check(self._L.epipf_incidence_walk(self._h, S, ptr(swarm), d, ptr(hw), obs, ptr(probs), ptr(keys), ptr(f),
                                               ptr(counts), D, 1 if cumulate else 0, ptr(lz), ptr(st)),
                  "epipf_incidence_walk")
        self._last_n = S
        self.run_serial += 1
        self._run_T = D + 2
        self._last_status = st.copy()
        _PARTICLE_STEPS[0] += S * self.N * (D + 2)
        return lz, st

    def incidence_smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), bins=None, lag=None):
        """epipf_incidence_smooth: the smoothed true flows per day of the last run_incidence or walk_incidence, reduced
        on the device under the genealogy's multiplicities.  Returns Smoothed with a leading chain axis: mean
        [n, D + 2, F], quantiles [n, Q, D + 2, F] or None, lineages [n, D + 2], sums [n, D + 2, F], zetas None; row 0 is
        all zeros (no flow leads into the initial draw).  Rows of chains whose status was not OK are NaN in mean and 0
        elsewhere.  bins defaults to the population total + 1 (no flow exceeds it).  lag=None is the full smoother."""
        from . import smoothing
        _, _, q = smoothing.check_options("genealogy", "smoothing", quantiles)
        lag = smoothing.check_lag(lag, "smoothing")
        n = int(n_chains) if n_chains is not None else self._last_n or 1
        if bins is None:
            if self._pop is None:
                raise ValueError("bins=None needs set_population")
            bins = int(sum(self._pop[0])) + 1
        F = 2 if self.model == _lib.SIR else 3
        nq = 0 if q is None else q.size
        rows = max(n, 1)
        sums = np.zeros((rows, self.run_T, F), dtype=np.int64)
        lineages = np.zeros((rows, self.run_T), dtype=np.int32)
        quant = np.zeros((rows, nq, self.run_T, F), dtype=np.int32) if nq else None
        check(self._L.epipf_incidence_smooth(self._h, n, -1 if lag is None else min(lag, 2**31 - 1), ptr(q), nq,
                                             int(bins) if nq else 0, ptr(sums), ptr(quant), ptr(lineages)),
              "epipf_incidence_smooth")
        mean = sums / float(self.N)
        mean[self._last_status[:n] != _lib.STATUS_OK] = np.nan
        return smoothing.Smoothed(mean, None if quant is None else quant.astype(np.int64), lineages, sums, None)

    def walk_history(self, n_chains=None):
        """theta [n, T, N, d] of the last walk_filter (epipf_walk_history)."""
        n = int(n_chains) if n_chains is not None else self._last_n or 1
        d = 2 if self.model == _lib.SIR else 3
        out = np.empty((max(n, 1), self.run_T, self.N, d), dtype=np.float64)
        check(self._L.epipf_walk_history(self._h, n, ptr(out)), "epipf_walk_history")
        return out

    def walk_smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), lineage="genealogy", lag=None):
        """epipf_walk_smooth on the last walk_filter's resident history: (mean [n, T, d + 1], quantiles
        [n, Q, T, d + 1] or None, lineages [n, T]); the last column is R_t.  Rows of chains whose status was not OK are
        NaN in mean and quantiles and 0 in lineages."""
        from . import smoothing
        lin, _, q = smoothing.check_options(lineage, "smoothing", quantiles)
        lag = smoothing.check_lag(lag, "smoothing")
        n = int(n_chains) if n_chains is not None else self._last_n or 1
        V = (2 if self.model == _lib.SIR else 3) + 1
        nq = 0 if q is None else q.size
        rows = max(n, 1)
        mean = np.zeros((rows, self.run_T, V), dtype=np.float64)
        quant = np.zeros((rows, nq, self.run_T, V), dtype=np.float64) if nq else None
        lineages = np.zeros((rows, self.run_T), dtype=np.int32)
        check(self._L.epipf_walk_smooth(self._h, n, lin, -1 if lag is None else min(lag, 2**31 - 1), ptr(q), nq, ptr(mean),
                                        ptr(quant), ptr(lineages)), "epipf_walk_smooth")
        bad = self._last_status[:n] != _lib.STATUS_OK
        mean[bad] = np.nan
        if quant is not None:
            quant[bad] = np.nan
        return mean, quant, lineages

    def walk_smooth_history(self, hidden, ancestry, theta, population_total, lineage, q, lag=None):
        """epipf_walk_smooth_history on host arrays hidden [n, T, N, C] int32, ancestry [n, T, N] int32 and theta
        [n, T, N, d] float64 (this engine's model and N are ignored); lineage is the library's id, q float64 [Q] or
        None: (mean [n, T, d + 1], quantiles [n, Q, T, d + 1] or None, lineages [n, T])."""
        from . import smoothing
        lag = smoothing.check_lag(lag, "smoothing")
        hidden = np.ascontiguousarray(hidden, dtype=np.int32)
        ancestry = np.ascontiguousarray(ancestry, dtype=np.int32)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        n, T, N, C = hidden.shape
        d = theta.shape[-1]
        if theta.shape != (n, T, N, d) or ancestry.shape != (n, T, N):
            raise ValueError("hidden [n, T, N, C], ancestry [n, T, N] and theta [n, T, N, d] must agree")
        nq = 0 if q is None else q.size
        mean = np.zeros((n, T, d + 1), dtype=np.float64)
        quant = np.zeros((n, nq, T, d + 1), dtype=np.float64) if nq else None
        lineages = np.zeros((n, T), dtype=np.int32)
        check(self._L.epipf_walk_smooth_history(self._h, n, T, N, C, d, ptr(hidden), ptr(ancestry), ptr(theta),
                                                float(population_total), int(lineage),
                                                -1 if lag is None else min(lag, 2**31 - 1), ptr(q), nq, ptr(mean),
                                                ptr(quant), ptr(lineages)), "epipf_walk_smooth_history")
        return mean, quant, lineages

    def resample(self, w, u):
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float64))
        out = np.empty(w.size, dtype=np.int32)
        fb = np.zeros(1, dtype=np.int64)
        rc = check(self._L.epipf_resample(self._h, w.size, ptr(w), ptr(u), ptr(out), ptr(fb)), "epipf_resample")
        return (None if rc == _lib.STATUS_DEGENERATE else out), int(fb[0])

    # ------------------------------------------------------------------ ABC rejection (abc_algo.py:17-109)
    @staticmethod
    def _abc_inputs(observed_data, priors):
        Y = np.ascontiguousarray(np.asarray(observed_data, dtype=np.float64))
        if Y.ndim != 2 or Y.shape[1] != 3:
            raise ValueError("observed_data must be [T, 3] (S, I, R), as abc_algo.py:38-45 unpacks it")
        pr = np.ascontiguousarray(np.array([priors["beta"][0], priors["beta"][1], priors["gamma"][0],
                                            priors["gamma"][1]], dtype=np.float64))
        return Y, pr

    def abc_trials(self, observed_data, priors, key=0, run_index=0, t0=0, n=1, rows=True):
        """Trials [t0, t0+n): theta [n,2], rows [n,T,3] int32 (S, I, R per day) or None, distance [n]."""
        Y, pr = self._abc_inputs(observed_data, priors)
        theta = np.empty((n, 2))
        rw = np.empty((n, Y.shape[0], 3), dtype=np.int32) if rows else None
        dist = np.empty(n)
        ev = np.zeros(1, dtype=np.int64)
        check(self._L.epipf_abc_trials(self._h, ptr(Y), Y.shape[0], ptr(pr), int(key) & (2**64 - 1),
                                       int(run_index) & 0xFFFFFFFF, int(t0), int(n), ptr(theta), ptr(rw), ptr(dist),
                                       ptr(ev)), "epipf_abc_trials")
        return theta, rw, dist

    def abc(self, observed_data, no_of_samples, threshold, priors, key=0, run_index=0, max_trials=2**32, batch=0):
        """(theta [n,2], trajectories [n,T,4], trials, accepted) of epipf_abc."""
        Y, pr = self._abc_inputs(observed_data, priors)
        n = int(no_of_samples)
        theta = np.empty((max(n, 1), 2))
        traj = np.empty((max(n, 1), Y.shape[0], 4))
        trials = np.zeros(1, dtype=np.int64)
        acc = np.zeros(1, dtype=np.int32)
        check(self._L.epipf_abc(self._h, ptr(Y), Y.shape[0], n, float(threshold), ptr(pr), int(key) & (2**64 - 1),
                                int(run_index) & 0xFFFFFFFF, int(max_trials), int(batch), ptr(theta), ptr(traj),
                                ptr(trials), ptr(acc)), "epipf_abc")
        a = int(acc[0])
        return theta[:a], traj[:a], int(trials[0]), a

    def abc_smc_generation(self, observed_data, no_of_samples, threshold, priors, prev_theta=None, prev_cdf=None,
                           half_width=None, key=0, run_index=0, t0=0, max_trials=None, batch=0):
        """One ABC-SMC generation (epipf_abc_smc_generation): (theta [n,2], trajectories [n,T,4], distances [n],
        ancestors [n] int32, trials, accepted).  prev_theta None or empty: the prior stage.  max_trials None: every
        trial index left from t0 (2^32 - t0)."""
        Y, pr = self._abc_inputs(observed_data, priors)
        if max_trials is None:
            max_trials = 2**32 - int(t0)
        n = int(no_of_samples)
        n_prev = 0 if prev_theta is None else len(prev_theta)
        pt = pc = hw = None
        if n_prev:
            pt = np.ascontiguousarray(np.asarray(prev_theta, dtype=np.float64).reshape(n_prev, 2))
            pc = np.ascontiguousarray(np.asarray(prev_cdf, dtype=np.float64).reshape(-1))
            hw = np.ascontiguousarray(np.asarray(half_width, dtype=np.float64).reshape(-1))
            if pc.shape[0] != n_prev or hw.shape[0] != 2:
                raise ValueError("prev_cdf must be [n_prev] and half_width [2]")
        theta = np.empty((max(n, 1), 2))
        traj = np.empty((max(n, 1), Y.shape[0], 4))
        dist = np.empty(max(n, 1))
        anc = np.empty(max(n, 1), dtype=np.int32)
        trials = np.zeros(1, dtype=np.int64)
        acc = np.zeros(1, dtype=np.int32)
        check(self._L.epipf_abc_smc_generation(self._h, ptr(Y), Y.shape[0], n, float(threshold), ptr(pr), ptr(pt),
                                               ptr(pc), n_prev, ptr(hw), int(key) & (2**64 - 1),
                                               int(run_index) & 0xFFFFFFFF, int(t0), int(max_trials), int(batch),
                                               ptr(theta), ptr(traj), ptr(dist), ptr(anc), ptr(trials), ptr(acc)),
              "epipf_abc_smc_generation")
        a = int(acc[0])
        return theta[:a], traj[:a], dist[:a], anc[:a], int(trials[0]), a

    def abc_smc_weights(self, theta, prev_theta, prev_w, half_width):
        """Weight denominators of new samples theta [n,2] against the previous population (epipf_abc_smc_weights)."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, 2))
        pt = np.ascontiguousarray(np.asarray(prev_theta, dtype=np.float64).reshape(-1, 2))
        pw = np.ascontiguousarray(np.asarray(prev_w, dtype=np.float64).reshape(-1))
        hw = np.ascontiguousarray(np.asarray(half_width, dtype=np.float64).reshape(-1))
        if pw.shape[0] != pt.shape[0] or hw.shape[0] != 2:
            raise ValueError("prev_w must be [n_prev] and half_width [2]")
        den = np.empty(th.shape[0])
        check(self._L.epipf_abc_smc_weights(self._h, ptr(th), th.shape[0], ptr(pt), ptr(pw), pt.shape[0], ptr(hw),
                                            ptr(den)), "epipf_abc_smc_weights")
        return den

    # ------------------------------------------------------------------ stats
    def set_profiling(self, level=_lib.PROFILE_COUNTERS):
        """level: PROFILE_OFF / PROFILE_TIMING (HIP events only, kernels unchanged) / PROFILE_COUNTERS
        (also device counters of SSA events and lane use).  True/False map to COUNTERS/OFF."""
        if level is True:
            level = _lib.PROFILE_COUNTERS
        elif level is False or level is None:
            level = _lib.PROFILE_OFF
        check(self._L.epipf_set_profiling(self._h, int(level)), "epipf_set_profiling")

    def set_streams(self, n):
        """Concurrent chain-group streams used by run() (1..8)."""
        check(self._L.epipf_set_streams(self._h, int(n)), "epipf_set_streams")

    def set_lanes(self, w, events_per_lane=0):
        """SSA lanes per particle used by run(): 0 = automatic, 1 (one-lane kernel), 2, 4, 8, 16 (lane groups), and
        the events each lane of a group draws per chunk (0 = automatic)."""
        check(self._L.epipf_set_lanes(self._h, int(w), int(events_per_lane)), "epipf_set_lanes")

    def stats(self):
        s = _lib.Stats()
        check(self._L.epipf_get_stats(self._h, ctypes.byref(s)), "epipf_get_stats")
        return s.as_dict()

    def reset_stats(self):
        check(self._L.epipf_reset_stats(self._h), "epipf_reset_stats")


_CACHE = {}


def release_engines():
    """Drop the cached engines: each context closes (its device buffers and HIP streams freed) with its last
    reference.  Idle contexts' streams still hold hardware queues (GPU_MAX_HW_QUEUES, 4 by default), on which the next
    concurrently running engines may otherwise be placed together."""
    _CACHE.clear()


def get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    """Cached engine large enough for (T, chains).  When a bigger one is needed a new context replaces the cached
    one; the old context is not closed here -- a sampler may still hold it -- but released with its last reference
    (Engine.__del__).  Callers that share a cached engine re-bind their observations / population before each run
    (set_observations / set_population are no-ops when nothing changed)."""
    mid = model_id(type_model)
    check_groups(mid, groups)
    key = (mid, groups if mid >= _lib.SIR_SUBGROUPS else 1, int(n_particles), int(device))
    eng = _CACHE.get(key)
    if eng is None or eng.t_max < T or eng.max_chains < chains:
        eng = Engine(type_model, groups, n_particles, max(T, eng.t_max if eng else 0),
                     max(chains, eng.max_chains if eng else 0), device)
        _CACHE[key] = eng
    return eng
