"""Posterior-predictive forecasts on the GPU (the reference's tests/pred_tmps.py traj_inf, :55-64, for a whole
posterior at once).

Every posterior draw has its own parameters and its own start state; `forecast` simulates each of them `replicates`
times over [0, horizon] in ONE launch (epipf_forecast: one lane per trajectory), bins each continuous path to one row
per day on the device, and reduces the ensemble there to exact sums and value histograms, from which the mean and the
quantiles follow without the trajectories ever leaving HBM.  Draw d, replicate r, event k draws from the keyed Philox
counter (k, r, step, filter_index + d): draw d's rows are those of `simulate_path_batch` of R copies of its state with
its theta at filter index filter_index + d, bit for bit, whatever else is in the batch.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .engine import check_groups, get_engine, model_id, n_compartments, theta_vector

Forecast = namedtuple("Forecast", "rows mean quantiles events sums")
Forecast.__doc__ = """rows [D, R, H, C] int32 or None; mean [H, C] float64 (sums / (D R)); quantiles [Q, H, C] or None;
events: accepted SSA events of the whole batch; sums [H, C] int64 (exact)."""

HIST_LIMIT_BYTES = 256 << 20


def quantiles_from_hist(hist, q):
    """Inverted-CDF quantiles from value counts: hist [..., M + 1] (hist[..., v] = samples equal to v) -> [Q, ...],
    out[i] = the smallest v with count(<= v) >= q[i] n -- np.quantile(samples, q, method="inverted_cdf")."""
    hist = np.asarray(hist)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(~((q >= 0.0) & (q <= 1.0))):
        raise ValueError("quantiles must lie in [0, 1]")
    cdf = np.cumsum(hist.astype(np.int64), axis=-1)
    n = cdf[..., -1]
    if np.any(n <= 0):
        raise ValueError("quantiles of an empty histogram")
    out = np.empty((q.size,) + hist.shape[:-1], dtype=np.int64)
    for i, qi in enumerate(q):
        # numpy's rule: the order statistic of 0-based index max(ceil(q n) - 1, 0), with q n in float64
        rank = np.maximum(np.ceil(qi * n.astype(np.float64)).astype(np.int64), 1)
        out[i] = np.sum(cdf < rank[..., None], axis=-1)
    return out


def _thetas(mid, thetas):
    """[D, d] float64 and G from a [D, d] array (subgroups: flattened beta row-major, then gamma, as theta_vector lays
    it out) or a sequence of reference thetas ((beta, gamma) pairs for the subgroup models)."""
    sub = mid >= _lib.SIR_SUBGROUPS
    arr = None
    try:
        arr = np.asarray(thetas, dtype=np.float64)
    except (ValueError, TypeError):
        pass
    if arr is not None and arr.ndim == 2:
        d = arr.shape[1]
        if sub:
            G = int(round(np.sqrt(max(d - 1, 0))))
            if G < 1 or G * G + 1 != d:
                raise ValueError(f"subgroup thetas need G*G + 1 columns (beta row-major, then gamma), got {d}")
            check_groups(mid, G)
        else:
            G = 1
            need = 2 if mid == _lib.SIR else 3
            if d != need:
                raise ValueError(f"thetas must have {need} columns for this model, got {d}")
        return np.ascontiguousarray(arr), G
    rows, Gs = [], set()
    for th in thetas:
        v, G = theta_vector(mid, th)
        rows.append(v)
        Gs.add(G)
    if not rows:
        raise ValueError("thetas is empty: the number of groups cannot be told from it")
    if len(Gs) != 1:
        raise ValueError("every theta must have the same number of groups")
    return np.ascontiguousarray(np.stack(rows)), Gs.pop()


def forecast(type_model, thetas, states, horizon, replicates=1, *, key=None, filter_index=None, step=0, device=0,
             rows=True, quantiles=(0.05, 0.5, 0.95)):
    """Forecast D posterior draws (thetas [D, d], states [D, C]) `horizon` days ahead, `replicates` trajectories each.
    Returns Forecast(rows, mean, quantiles, events, sums); rows=False keeps the trajectories on the device,
    quantiles=None requests no histogram."""
    mid = model_id(type_model)
    th, G = _thetas(mid, thetas)
    C = n_compartments(mid, G)
    st = np.asarray(states)
    if st.ndim == 3 and mid >= _lib.SIR_SUBGROUPS:       # [D, G, 3], as the reference keeps subgroup populations
        st = st.reshape(st.shape[0], -1)
    if st.ndim != 2 or st.shape[1] != C:
        raise ValueError(f"states must be [D, {C}] for this model, got {st.shape}")
    if st.shape[0] != th.shape[0]:
        raise ValueError(f"{th.shape[0]} thetas for {st.shape[0]} start states")
    H, R = int(horizon), int(replicates)
    if H < 1:
        raise ValueError("horizon must be >= 1")
    if R < 1:
        raise ValueError("replicates must be >= 1")
    st = np.rint(st).astype(np.int64)
    if st.size and st.min() < 0:
        raise ValueError("states must be non-negative")
    D = st.shape[0]
    if D * R > 2**31 - 1:
        raise ValueError("n_draws * replicates must fit int32")
    q = None if quantiles is None else np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if q is not None and np.any(~((q >= 0.0) & (q <= 1.0))):
        raise ValueError("quantiles must lie in [0, 1]")
    bins = 0
    if q is not None:
        bins = int(st.sum(axis=1).max()) + 1 if D else 1
        if H * C * bins * 4 > HIST_LIMIT_BYTES:
            raise ValueError(f"the quantile histogram needs {H * C * bins * 4} bytes (> {HIST_LIMIT_BYTES}): call with "
                             "quantiles=None, rows=True and reduce the rows instead")
    from .gillespie import _stream
    k, f = _stream(key, filter_index)
    eng = get_engine(mid, G, 1, 1, 1, device)
    out, sums, hist, events = eng.forecast(th, st.astype(np.int32), H, R, k, f, step, rows=bool(rows), bins=bins)
    mean = sums / float(D * R) if D else np.full((H, C), np.nan)
    qs = None
    if q is not None:
        qs = quantiles_from_hist(hist, q) if D else np.full((q.size, H, C), np.nan)
    return Forecast(out, mean, qs, events, sums)


def forecast_from_chain(type_model, thetas, sampled_trajs, horizon, burn_in=0, thin=1, **kw):
    """Forecast from what particle_mcmc returns: draw j (after burn-in and thinning) starts from its sampled
    trajectory's last state sampled_trajs[-1, j] with thetas[j].  Returns (Forecast, full [n, T + H, C]): each draw's
    sampled trajectory followed by replicate 0's forecast (the array tests/pred_tmps.py:75-77 builds)."""
    tr = np.asarray(sampled_trajs)
    if tr.ndim != 3:
        raise ValueError("sampled_trajs must be [T, n_iter, C]")
    if int(thin) < 1 or int(burn_in) < 0:
        raise ValueError("burn_in must be >= 0 and thin >= 1")
    sel = slice(int(burn_in), None, int(thin))
    tr = tr[:, sel]
    th = thetas[sel] if isinstance(thetas, np.ndarray) else list(thetas)[sel]
    if len(th) != tr.shape[1]:
        raise ValueError(f"{len(th)} thetas for {tr.shape[1]} sampled trajectories")
    kw["rows"] = True
    res = forecast(type_model, th, tr[-1], horizon, **kw)
    full = np.concatenate([np.transpose(tr, (1, 0, 2)), res.rows[:, 0].astype(tr.dtype)], axis=1)
    return res, full
