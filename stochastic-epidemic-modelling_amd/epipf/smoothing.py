"""Particle smoother: state estimates with credible bands over the observed window, and the lineage diagnostic.

For one filter history h[T][N][C] (hidden_process) and a[T][N] (ancestry_matrix), with shift in {0, 1}:

    m[T-1][i] = 1                                          for all i
    m[p][i]   = sum of m[p+1][j] over j with a[p+shift][j] == i,   p = T-2 .. 0
    sums[p][c]    = sum_i m[p][i] h[p][i][c]               (int64, exact)
    hist[p][c][v] = sum of m[p][i] over i with h[p][i][c] == v
    lineages[p]   = #{i : m[p][i] > 0}
    quantile q of cell (p, c) = the smallest v with sum_{v' <= v} hist[p][c][v'] >= max(ceil(q N), 1)
                                (np.quantile(..., method="inverted_cdf"), as forecast.quantiles_from_hist)
    mean = sums / N

lineage="reference" (shift 0) follows ancestry[p] as particle_path_sampler does: m[p][i] counts the final picks
chosen in 0..N-1 whose sampled path visits particle i on day p, so every output is the statistic over those N
trajectories (row 0 of ancestry is zeros: day 0 is always particle 0).  lineage="genealogy" (shift 1, the default)
follows ancestry[p+1], the parent of a day-(p+1) particle: the true ancestral tree.  kind="predictive" sets m = 1 on
every day: the particle cloud hidden[p] itself, as the reference's per-particle plots show it.

On the device (epipf_smooth, csrc/epipf_smooth.hip) this is a backward pass of integer multiplicities over the history
resident in HBM; only [T, C] numbers per chain come back.  backend="numpy" of smooth_history restates it on the host.

lag=L (an integer >= 0, with kind="smoothing") is the fixed-lag smoother (Kitagawa 1996; epipf_smooth_lag,
csrc/epipf_smooth_lag.hip): day p is estimated from the particles of day e(p) = min(p + L, T-1) traced back L days,

    w_e[e][i] = 1                                          for all i
    w_e[q][i] = sum of w_e[q+1][j] over j with a[q+shift][j] == i,   q = e-1 .. p
    m[p][i]   = w_{e(p)}[p][i]

and sums, hist, lineages, quantiles and mean are the ones above with this m (sum_i m[p][i] = N on every day).  L = 0 is
kind="predictive" and L >= T-1 is kind="smoothing", bit for bit; L = 1 under lineage="genealogy" is the filtering
distribution (the resampled parents); lineages[p] does not increase with L.  At N = 10^4 a lag of ten days keeps about
1,500 lineages where the smoother keeps a hundred, at the price of ignoring data more than L days
ahead.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .forecast import HIST_LIMIT_BYTES, quantiles_from_hist

Smoothed = namedtuple("Smoothed", "mean quantiles lineages sums zetas")
Smoothed.__doc__ = """mean [T, C] float64 (sums / N); quantiles [Q, T, C] int64 or None; lineages [T] distinct surviving
lineages per day; sums [T, C] int64 (exact); zetas [T] (particle_smoother only, else None).  Batch calls add a leading
chain axis."""

DEFAULT_QUANTILES = (0.05, 0.5, 0.95)
_LINEAGES = {"reference": _lib.LINEAGE_REFERENCE, "genealogy": _lib.LINEAGE_GENEALOGY}
_KINDS = {"smoothing": _lib.SMOOTH_SMOOTHING, "predictive": _lib.SMOOTH_PREDICTIVE}


def check_options(lineage, kind, quantiles):
    """(lineage id, kind id, q float64 [Q] or None), or ValueError: before any device call."""
    if lineage not in _LINEAGES:
        raise ValueError(f"lineage must be 'reference' or 'genealogy', got {lineage!r}")
    if kind not in _KINDS:
        raise ValueError(f"kind must be 'smoothing' or 'predictive', got {kind!r}")
    q = None
    if quantiles is not None:
        q = np.ascontiguousarray(np.atleast_1d(np.asarray(quantiles, dtype=np.float64)))
        if q.ndim != 1 or np.any(~((q >= 0.0) & (q <= 1.0))):
            raise ValueError("quantiles must lie in [0, 1]")
        if q.size == 0:
            q = None
    return _LINEAGES[lineage], _KINDS[kind], q


def check_lag(lag, kind):
    """lag as an int >= 0, or None; ValueError for a bool, a non-integer, a negative value, or a lag with
    kind="predictive": before any device call."""
    if lag is None:
        return None
    if isinstance(lag, (bool, np.bool_)) or not isinstance(lag, (int, np.integer)):
        raise ValueError(f"lag must be None or an integer >= 0, got {lag!r}")
    if lag < 0:
        raise ValueError(f"lag must be >= 0, got {lag}")
    if kind == "predictive":
        raise ValueError("lag goes with kind='smoothing' (lag=0 is the predictive cloud itself)")
    return int(lag)


def multiplicities(ancestry, shift):
    """m [T, N] int64 of the definition above for one chain's ancestry [T, N] (integers in [0, N))."""
    T, N = ancestry.shape
    m = np.zeros((T, N), dtype=np.int64)
    m[T - 1] = 1
    for p in range(T - 2, -1, -1):
        np.add.at(m[p], ancestry[p + shift], m[p + 1])
    return m


def lag_multiplicities(ancestry, shift, lag):
    """m [T, N] int64 of the fixed-lag definition above: row p is the window from day min(p + lag, T-1) back to p."""
    T, N = ancestry.shape
    m = np.empty((T, N), dtype=np.int64)
    for p in range(T):
        w = np.ones(N, dtype=np.int64)
        for q in range(min(p + lag, T - 1) - 1, p - 1, -1):
            # counts up to N <= 2^30 are exact in bincount's float64 weights
            w = np.bincount(ancestry[q + shift], weights=w, minlength=N).astype(np.int64)
        m[p] = w
    return m


def _smooth_numpy(hid, anc, shift, predictive, q, bins, lag=None):
    """The host restatement for one chain: (sums [T, C], quantiles [Q, T, C] or None, lineages [T])."""
    T, N, C = hid.shape
    if lag is not None:
        m = lag_multiplicities(anc, shift, lag)
    else:
        m = np.ones((T, N), dtype=np.int64) if predictive else multiplicities(anc, shift)
    sums = np.einsum("pi,pic->pc", m, hid.astype(np.int64))
    lineages = np.count_nonzero(m, axis=1).astype(np.int32)
    qs = None
    if q is not None:
        hist = np.zeros((T, C, bins), dtype=np.int64)
        for p in range(T):
            for c in range(C):
                keep = hid[p, :, c] < bins               # a value outside the histogram is dropped
                hist[p, c] = np.bincount(hid[p, keep, c], weights=m[p, keep], minlength=bins).astype(np.int64)
        cdf = np.cumsum(hist, axis=-1)
        qs = np.empty((q.size, T, C), dtype=np.int64)
        for i, qi in enumerate(q):                       # quantiles_from_hist's rule with the total N, known here
            rank = max(int(np.ceil(qi * np.float64(N))), 1)
            qs[i] = np.sum(cdf < rank, axis=-1)
    return sums, qs, lineages


def smooth_history(hidden, ancestry, *, quantiles=DEFAULT_QUANTILES, lineage="genealogy", kind="smoothing", bins=None,
                   device=0, backend="gpu", lag=None):
    """Smooth histories from anywhere: hidden [T, N, C] with ancestry [T, N] (the reference's float64 arrays or
    integers), or a batch [n, T, N, C] / [n, T, N].  Inputs are rinted to int32; negative counts or ancestors outside
    [0, N) raise ValueError.  bins (values 0..bins-1 are counted) defaults to the largest count + 1.  backend="numpy"
    needs no library or device.  lag=L is the fixed-lag smoother (the module's docstring)."""
    lin, knd, q = check_options(lineage, kind, quantiles)
    lag = check_lag(lag, kind)
    if backend not in ("gpu", "numpy"):
        raise ValueError(f"backend must be 'gpu' or 'numpy', got {backend!r}")
    hid = np.asarray(hidden)
    anc = np.asarray(ancestry)
    batch = hid.ndim == 4
    if not batch:
        hid, anc = hid[None], anc[None]
    if hid.ndim != 4 or anc.ndim != 3 or anc.shape != hid.shape[:3]:
        raise ValueError(f"hidden must be [T, N, C] with ancestry [T, N] (or a batch of them), got {np.shape(hidden)} "
                         f"and {np.shape(ancestry)}")
    n, T, N, C = hid.shape
    if min(n, T, N, C) < 1:
        raise ValueError("n, T, N and C must be >= 1")
    if not (np.all(np.isfinite(hid)) and np.all(np.isfinite(anc))):
        raise ValueError("hidden and ancestry must be finite")
    hid = np.rint(hid).astype(np.int64)
    anc = np.rint(anc).astype(np.int64)
    if hid.min() < 0 or hid.max() > 2**31 - 1:
        raise ValueError("counts must be non-negative int32 values")
    if anc.min() < 0 or anc.max() >= N:
        raise ValueError("ancestors must lie in [0, N)")
    hid = hid.astype(np.int32)
    anc = anc.astype(np.int32)
    if q is None:
        bins = 0
    else:
        bins = int(hid.max()) + 1 if bins is None else int(bins)
        if bins < 1:
            raise ValueError("bins must be >= 1")
        if T * C * bins * 4 > HIST_LIMIT_BYTES:
            raise ValueError(f"the quantile histogram needs {T * C * bins * 4} bytes (> {HIST_LIMIT_BYTES}): call with "
                             "quantiles=None and reduce the history instead")
    if backend == "numpy":
        parts = [_smooth_numpy(hid[i], anc[i], lin, knd == _lib.SMOOTH_PREDICTIVE, q, bins, lag) for i in range(n)]
        sums = np.stack([s for s, _, _ in parts])
        qs = None if q is None else np.stack([x for _, x, _ in parts])
        lineages = np.stack([x for _, _, x in parts])
    else:
        from .engine import get_engine
        eng = get_engine(_lib.SIR, 1, 1, 1, 1, device)
        sums, qs, lineages = eng.smooth_history(hid, anc, lin, knd, q, bins, lag=lag)
        qs = None if qs is None else qs.astype(np.int64)
    mean = sums / float(N)
    if not batch:
        return Smoothed(mean[0], None if qs is None else qs[0], lineages[0], sums[0], None)
    return Smoothed(mean, qs, lineages, sums, None)


def particle_smoother(Y, type_model, theta_proposal, observations=False, probs=.1, n_particles=1000, n_population=4820,
                      mu=20, jobs=4, *, quantiles=DEFAULT_QUANTILES, lineage="genealogy", kind="smoothing", key=None,
                      filter_index=None, resample="multinomial", device=0, lag=None):
    """Run exactly the filter particle_filter would run with the same arguments (one filter index is taken from the
    stream in the same way), then smooth its history on the device.  Returns Smoothed (zetas [T] as particle_filter's),
    or None when the filter is degenerate.  `jobs` is accepted for compatibility and ignored.  lag=L smooths with a
    fixed lag of L days instead."""
    check_options(lineage, kind, quantiles)
    lag = check_lag(lag, kind)
    from . import pmcmc
    from .engine import get_engine, model_id, theta_vector
    mid = model_id(type_model)
    zetas, _, _ = pmcmc.particle_filter(Y, type_model, theta_proposal, observations, probs, n_particles, n_population,
                                        mu, jobs, key=key, filter_index=filter_index, resample=resample, device=device,
                                        return_history=False)
    if zetas is None:
        return None
    _, G = theta_vector(mid, theta_proposal)
    eng = get_engine(mid, G, n_particles, np.asarray(Y).shape[0], 1, device)   # the cached engine the filter ran on
    s = eng.smooth(1, quantiles=quantiles, lineage=lineage, kind=kind, lag=lag)
    return Smoothed(s.mean[0], None if s.quantiles is None else s.quantiles[0], s.lineages[0], s.sums[0], zetas)
