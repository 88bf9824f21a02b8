"""Drop-in for the reference's abc_algo.py (ABC rejection sampling for the SIR model), on the GPU.

`abc_algo(observed_data, no_of_samples, threshold, priors)` keeps the reference's signature and return
value (abc_algo.py:17-109): a dict {"beta": [...], "gamma": [...]} of accepted draws and the array of
accepted daily trajectories [no_of_samples, T, 4] with columns (day, S, I, R).  The rejection loop runs
batched in libepipf.so (epipf_abc): one GPU lane per trial, accepted trials taken in trial order, so the
result is the reference's sequential loop driven by the keyed ABC stream -- trial t draws its
prior, initial counts and Gillespie events from Philox counters (·, t, 3..5 << 24, run).

Random numbers: key = the module stream (`epipf.seed_stream`), run index = one per abc_algo call (counted
separately from the particle filter's indices).

`abc_smc(observed_data, no_of_samples, thresholds, priors, ...)` has no reference counterpart: population Monte Carlo
ABC over the same trials, for thresholds where rejection from the prior wastes most of its trials.
"""
import time

import numpy as np

from .engine import get_engine
from .pmcmc import _STREAM


def distance_function(I_1, I_2, R_1, R_2):
    """abc_algo.py:9-13 (host helper, identical arithmetic: numpy means of absolute differences)."""
    return (np.mean(abs(np.asarray(I_1) - np.asarray(I_2))) + np.mean(abs(np.asarray(R_1) - np.asarray(R_2)))) / 2


def _take_run_index():
    r = _STREAM.next_abc_run
    _STREAM.next_abc_run = r + 1
    return r


def abc_run(observed_data, no_of_samples, threshold, priors, key=None, run_index=None, max_trials=2**32, batch=0,
            device=0):
    """Full result of one ABC run: dict(beta, gamma, trajectories, trials, accepted, key, run_index)."""
    key = _STREAM.key if key is None else int(key)
    run_index = _take_run_index() if run_index is None else int(run_index)
    eng = get_engine("sir", 1, 1, 1, 1, device)
    theta, traj, trials, acc = eng.abc(observed_data, no_of_samples, threshold, priors, key, run_index, max_trials,
                                       batch)
    return dict(beta=[float(v) for v in theta[:, 0]], gamma=[float(v) for v in theta[:, 1]], trajectories=traj,
                trials=trials, accepted=acc, key=key, run_index=run_index)


# ----------------------------------------------------------------------------------- ABC-SMC
# Population Monte Carlo ABC (Toni et al. 2009; Beaumont et al. 2009) with a uniform prior and a uniform perturbation
# kernel.  The host parts below are plain numpy, in the order the definition fixes; the trials, the proposals and the
# O(N N_prev) weight sums run in libepipf.so (epipf_abc_smc_generation, epipf_abc_smc_weights).
def smc_cdf(weights):
    """Normalised cumulative weights of a population: np.cumsum(w); cdf /= cdf[-1]."""
    cdf = np.cumsum(np.asarray(weights, dtype=np.float64))
    cdf /= cdf[-1]
    return cdf


def smc_half_width(theta, kernel_scale=1.0):
    """Half-widths of the uniform kernel per component: kernel_scale * 0.5 * (max - min) of the population."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, 2)
    return np.array([kernel_scale * 0.5 * (theta[:, c].max() - theta[:, c].min()) for c in range(2)])


def smc_weights(den):
    """Weights of a generation from its denominators: w = 1/den; w /= np.cumsum(w)[-1].  A zero denominator (a sample
    that no previous point reaches, possible only through rounding at the kernel's edge) raises ValueError."""
    den = np.asarray(den, dtype=np.float64)
    if not np.all(den > 0.0):
        bad = int(np.nonzero(~(den > 0.0))[0][0])
        raise ValueError(f"abc_smc: sample {bad} has weight denominator {den[bad]} (no previous point within the kernel)")
    w = 1.0 / den
    w /= np.cumsum(w)[-1]
    return w


def smc_next_threshold(distances, quantile):
    """The adaptive schedule's next threshold: np.sort(dist)[ceil(quantile * N) - 1]."""
    d = np.sort(np.asarray(distances, dtype=np.float64))
    return float(d[int(np.ceil(quantile * len(d))) - 1])


def smc_schedule(thresholds, quantile=None, generations=None):
    """(explicit thresholds, total generations) of a run.  The first threshold is always explicit; either the list holds
    every generation, or quantile (0 < q <= 1) and generations (>= len(thresholds)) extend it adaptively."""
    if thresholds is None:
        raise ValueError("abc_smc: thresholds must give at least the first generation's threshold")
    th = [float(v) for v in np.atleast_1d(np.asarray(thresholds, dtype=np.float64))]
    if not th:
        raise ValueError("abc_smc: thresholds must give at least the first generation's threshold")
    if any(np.isnan(v) for v in th):
        raise ValueError("abc_smc: a threshold is NaN")
    if (quantile is None) != (generations is None):
        raise ValueError("abc_smc: quantile and generations go together")
    if quantile is None:
        return th, len(th)
    if not 0.0 < float(quantile) <= 1.0:
        raise ValueError(f"abc_smc: quantile {quantile} outside (0, 1]")
    if int(generations) < len(th):
        raise ValueError(f"abc_smc: generations {generations} below the {len(th)} explicit thresholds")
    return th, int(generations)


def abc_smc(observed_data, no_of_samples, thresholds=None, priors=None, *, quantile=None, generations=None,
            kernel_scale=1.0, key=None, run_index=None, max_trials=2**32, batch=0, device=0):
    """ABC-SMC for the SIR model: generation 0 is abc_algo's rejection sampler at thresholds[0]; each later generation
    proposes from the previous weighted population through a uniform kernel of half-width kernel_scale * (max - min)/2
    and accepts at the next threshold (explicit, or the `quantile` of the previous accepted distances until
    `generations` have run).  One global trial counter runs through the generations; at most max_trials trials in all.

    Returns dict(beta, gamma, weights, trajectories, ess, total_trials, generations, key, run_index); `generations` is
    a list of dict(threshold, theta, weights, distances, ancestors, trials, half_width, denominators, seconds), one
    per generation."""
    n = int(no_of_samples)
    if n < 1:
        raise ValueError("abc_smc: no_of_samples must be at least 1")
    if priors is None:
        raise ValueError("abc_smc: priors are required")
    if not (np.isfinite(kernel_scale) and kernel_scale > 0):
        raise ValueError(f"abc_smc: kernel_scale {kernel_scale} must be positive")
    explicit, n_gen = smc_schedule(thresholds, quantile, generations)
    max_trials = int(max_trials)
    key = _STREAM.key if key is None else int(key)
    run_index = _take_run_index() if run_index is None else int(run_index)
    eng = get_engine("sir", 1, 1, 1, 1, device)
    gens = []
    t0 = 0
    theta = w = traj = None
    for g in range(n_gen):
        eps = explicit[g] if g < len(explicit) else smc_next_threshold(gens[-1]["distances"], quantile)
        started = time.perf_counter()
        if g == 0:
            prev = dict(prev_theta=None, prev_cdf=None, half_width=None)
            hw = np.zeros(2)
        else:
            hw = smc_half_width(theta, kernel_scale)
            prev = dict(prev_theta=theta, prev_cdf=smc_cdf(w), half_width=hw)
        th, traj, dist, anc, trials, acc = eng.abc_smc_generation(observed_data, n, eps, priors, key=key,
                                                                  run_index=run_index, t0=t0,
                                                                  max_trials=max_trials - t0, batch=batch, **prev)
        if acc < n:
            raise RuntimeError(f"abc_smc: generation {g} accepted {acc} of {n} samples within {trials} trials "
                               f"(threshold {eps}; {t0 + trials} trials in all)")
        if g == 0:
            den = np.full(n, 1.0)
            w_new = np.full(n, 1.0 / n)
        else:
            den = eng.abc_smc_weights(th, theta, w, hw)
            w_new = smc_weights(den)
        gens.append(dict(threshold=eps, theta=th, weights=w_new, distances=dist, ancestors=anc, trials=trials,
                         half_width=hw, denominators=den, seconds=time.perf_counter() - started))
        theta, w = th, w_new
        t0 += trials
    return dict(beta=[float(v) for v in theta[:, 0]], gamma=[float(v) for v in theta[:, 1]], weights=w,
                trajectories=traj, ess=float(1.0 / np.sum(w * w)), total_trials=t0, generations=gens, key=key,
                run_index=run_index)


def abc_algo(observed_data, no_of_samples, threshold, priors, key=None, run_index=None, max_trials=2**32, batch=0,
             device=0):
    """abc_algo.py:17-109.  Returns (posterior_distr, trajectories).

    Unlike the reference, which loops forever when the threshold is unreachable, at most `max_trials` trials
    run; fewer than no_of_samples accepted draws then raise RuntimeError."""
    r = abc_run(observed_data, no_of_samples, threshold, priors, key, run_index, max_trials, batch, device)
    if r["accepted"] < int(no_of_samples):
        raise RuntimeError(f"abc_algo: {r['accepted']} of {no_of_samples} samples accepted within "
                           f"{r['trials']} trials (threshold {threshold})")
    return {"beta": r["beta"], "gamma": r["gamma"]}, r["trajectories"]
