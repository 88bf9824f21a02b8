"""Forecast summaries on the GPU: what an epidemic report asks of a forecast -- how high the peak is and when, whether
and when the outbreak dies out, how many more infections there are -- as functionals of each whole continuous path,
reduced on the device (epipf_forecast_summary).

The trajectories are `forecast`'s, bit for bit: draw d, replicate r, event k draws from the keyed Philox counter
(k, r, step, filter_index + d), so a call with the same arguments describes the same paths, and a draw depends on nothing
else in its batch.  With i(t) the infectious count after the events up to t (SIR and SEIR: I; subgroups: the sum of I_g),
per path:
  peak             max of i over the start state and every event
  peak_time        time of the first event after which i == peak; 0.0 when no event exceeds the start value
  extinction_time  time of the event after which nobody is infectious (SEIR: nor exposed); 0.0 when the start state is
                   already so, +inf when the path is still active at the horizon
  infections       susceptibles at the start minus those at the end
  events           events of the path
"""
import numpy as np

from . import _lib
from .engine import get_engine, model_id, n_compartments
from .forecast import HIST_LIMIT_BYTES, _thetas, quantiles_from_hist


class ForecastSummary:
    """What forecast_summary returns.  n = D R paths.
    peak_mean, infections_mean: exact sums / n;  peak_quantiles, infections_quantiles: [Q] inverted-CDF quantiles from
    the value histograms, or None;  peak_day_prob [H]: P(floor(peak_time) == day) (a peak at exactly t = H: the last day);
    extinct_by_day [H]: P(extinct by the end of day k), cumulative, and p_extinct its last entry;  extinct_per_draw [D]:
    each draw's extinct fraction (parameter uncertainty apart from chance);  events: events of the whole batch;
    paths: None, or (peak, peak_time, extinction_time, infections, events), each [D, R];  hist: the raw integer arrays
    (totals [4], peak_day [H], extinct_day [H + 1] with the paths that are not extinct in its last bin, extinct_per_draw
    [D], peak_hist and infections_hist [bins] or None, n), for callers who pool several calls."""

    def __init__(self, raw, D, R, H, q):
        n = D * R
        self.n, self.paths = n, raw["paths"]
        self.hist = {k: raw[k] for k in ("totals", "peak_day", "extinct_day", "extinct_per_draw", "peak_hist",
                                         "infections_hist")}
        self.hist["n"] = n
        self.events = int(raw["totals"][3])
        nan = float("nan")
        self.peak_mean = raw["totals"][0] / float(n) if n else nan
        self.infections_mean = raw["totals"][1] / float(n) if n else nan
        self.peak_day_prob = raw["peak_day"] / float(n) if n else np.full(H, np.nan)
        self.extinct_by_day = np.cumsum(raw["extinct_day"][:H].astype(np.int64)) / float(n) if n else np.full(H, np.nan)
        self.p_extinct = float(self.extinct_by_day[-1])
        self.extinct_per_draw = raw["extinct_per_draw"] / float(R)
        self.peak_quantiles = self.infections_quantiles = None
        if q is not None:
            self.peak_quantiles = quantiles_from_hist(raw["peak_hist"], q) if n else np.full(q.size, np.nan)
            self.infections_quantiles = quantiles_from_hist(raw["infections_hist"], q) if n else np.full(q.size, np.nan)

    def exceed(self, K):
        """P(peak >= K), from the peak histogram (needs quantiles other than None)."""
        h = self.hist["peak_hist"]
        if h is None:
            raise ValueError("exceed needs the peak histogram: call forecast_summary with quantiles other than None")
        if not self.n:
            return float("nan")
        k = min(max(int(np.ceil(K)), 0), h.size)
        return int(h[k:].sum(dtype=np.int64)) / float(self.n)


def forecast_summary(type_model, thetas, states, horizon, replicates=1, *, key=None, filter_index=None, step=0, device=0,
                     per_path=False, quantiles=(0.05, 0.5, 0.95)):
    """Summaries of the forecast of D posterior draws (thetas [D, d], states [D, C]) `horizon` days ahead, `replicates`
    trajectories each: the paths `forecast` describes with the same arguments.  Returns ForecastSummary; per_path=True
    also returns the five per-path arrays, quantiles=None requests no value histograms."""
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
        if 2 * bins * 4 > HIST_LIMIT_BYTES:
            raise ValueError(f"the value histograms need {2 * bins * 4} bytes (> {HIST_LIMIT_BYTES}): call with "
                             "quantiles=None, per_path=True and reduce the paths instead")
    from .gillespie import _stream
    k, f = _stream(key, filter_index)
    eng = get_engine(mid, G, 1, 1, 1, device)
    raw = eng.forecast_summary(th, st.astype(np.int32), H, R, k, f, step, per_path=bool(per_path), bins=bins)
    return ForecastSummary(raw, D, R, H, q)


def forecast_summary_from_chain(type_model, thetas, sampled_trajs, horizon, burn_in=0, thin=1, **kw):
    """Summaries from what particle_mcmc returns: draw j (after burn-in and thinning) starts from its sampled
    trajectory's last state sampled_trajs[-1, j] with thetas[j] (forecast_from_chain's selection)."""
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
    return forecast_summary(type_model, th, tr[-1], horizon, **kw)
