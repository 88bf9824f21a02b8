"""Shared by tests/test_forecast_summary_host.py and tests/test_gpu_forecast_summary.py: the numpy restatement of the
forecast summary's definition on an event path, the summaries of oracle forecasts, the reductions
recomputed from per-path arrays, and the oracle's summaries of tests/forecast_cases.py's batches, computed once."""
import functools

import numpy as np

import forecast_cases
import oracle
from forecast_cases import DRAWS_FIDX, DRAWS_H, DRAWS_KEY, DRAWS_R
from forecast_helpers import _one_thread, reference_thetas

FIELDS = ("peak", "peak_time", "extinction_time", "infections", "events")


def infectious_columns(model, G):
    """Columns whose sum is i(t): SIR I, SEIR I (column 2, not E), the subgroup models every group's I."""
    return [1] if model == "sir" else [2] if model == "seir" else list(range(1, 3 * G, 3))


def susceptible_columns(model, G):
    return [0] if model in ("sir", "seir") else list(range(0, 3 * G, 3))


def path_summary(model, G, x0, times, states):
    """(peak, peak_time, extinction_time, infections, events) of one path: the start state x0 [C], then the accepted
    events' times and the states after them, in order.  The loop the kernel runs, restated: a strict > keeps the first
    attainment of the peak; the path is extinct when its last state is inactive, at its last event's time (0.0 without
    an event), else +inf."""
    x0 = np.asarray(x0, dtype=np.int64)
    ic, ac, sc = infectious_columns(model, G), forecast_cases.infected_columns(model, G), susceptible_columns(model, G)
    states = np.asarray(states, dtype=np.int64).reshape(len(times), x0.size)
    peak, peak_time, last_t = int(x0[ic].sum()), 0.0, 0.0
    # the per-event sums once, then plain Python numbers: the sweep walks some 10^5 events
    for t, i in zip(np.asarray(times, dtype=np.float64).tolist(), states[:, ic].sum(axis=1).tolist()):
        if i > peak:
            peak, peak_time = i, t
        last_t = t
    cur = states[-1] if len(times) else x0
    ext = float("inf") if cur[ac].sum() > 0 else last_t
    return peak, peak_time, ext, int(x0[sc].sum() - cur[sc].sum()), len(times)


def oracle_summaries(model, G, thetas, states, H, R, key, filter_index, step=0):
    """{field: [D, R]} of path_summary over oracle.simulate_path (draw d: R copies of states[d] with thetas[d] at filter
    index filter_index + d), plus "again" [D, R] bool: a later event leaves i at the peak value once more (a >= in place
    of the strict > would move peak_time there), and "longest", the longest path's events."""
    states = np.asarray(states)
    D = states.shape[0]
    ic = infectious_columns(model, G)
    out = {"peak": np.zeros((D, R), np.int32), "peak_time": np.zeros((D, R)), "extinction_time": np.zeros((D, R)),
           "infections": np.zeros((D, R), np.int32), "events": np.zeros((D, R), np.int32),
           "again": np.zeros((D, R), bool), "longest": 0}
    for d in range(D):
        t, x, n, fin = oracle.simulate_path(model, np.tile(states[d], (R, 1)), thetas[d], float(H), key=key,
                                            filter_index=(filter_index + d) & 0xFFFFFFFF, step=step)
        for r in range(R):
            s = path_summary(model, G, states[d], t[r, :n[r]], x[r, :n[r]])
            for f, v in zip(FIELDS, s):
                out[f][d, r] = v
            series = np.concatenate([[states[d][ic].sum()], x[r, :n[r]][:, ic].sum(axis=1)])
            out["again"][d, r] = np.count_nonzero(series == series.max()) > 1
            out["longest"] = max(out["longest"], int(n[r]))
            assert np.array_equal(x[r, n[r] - 1] if n[r] else states[d], fin[r])
    return out


def reductions(paths, H, bins=None):
    """The call's reductions recomputed from the per-path arrays (each [D, R]): totals [4] int64, peak_day [H],
    extinct_day [H + 1] (bin H: not extinct), extinct_per_draw [D], and with bins the two value histograms."""
    peak, pt, et, inf, ev = (np.asarray(paths[f]) for f in FIELDS) if isinstance(paths, dict) else paths
    gone = np.isfinite(et)
    out = {"totals": np.array([peak.sum(dtype=np.int64), inf.sum(dtype=np.int64), gone.sum(), ev.sum(dtype=np.int64)],
                              dtype=np.int64),
           "peak_day": np.bincount(np.minimum(np.floor(pt).astype(np.int64), H - 1).ravel(), minlength=H).astype(np.uint32),
           "extinct_day": np.bincount(np.where(gone, np.minimum(np.floor(np.where(gone, et, 0.0)).astype(np.int64), H - 1),
                                               H).ravel(), minlength=H + 1).astype(np.uint32),
           "extinct_per_draw": gone.sum(axis=1).astype(np.uint32)}
    if bins:
        out["peak_hist"] = np.bincount(peak.ravel(), minlength=bins).astype(np.uint32)
        out["infections_hist"] = np.bincount(inf.ravel(), minlength=bins).astype(np.uint32)
    return out


def batch(name):
    """(model, G, reference thetas, states) of a shared batch: "sir", "seir" (SIR_DRAWS, SEIR_DRAWS), or an instance
    (model, G) of forecast_cases.INSTANCES, whose subgroup batches are draws_case(G)."""
    model, G = (name, 1) if isinstance(name, str) else name
    if model == "sir":
        th, st = forecast_cases.SIR_DRAWS
        return model, 1, [tuple(t) for t in th], st
    if model == "seir":
        th, st = forecast_cases.SEIR_DRAWS
        return model, 1, [tuple(t) for t in th], st
    th, st = forecast_cases.draws_case(G)
    return model, G, th, st


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
@_one_thread
def draws_summaries(model, G):
    """oracle_summaries of batch((model, G)) at the shared call (DRAWS_R, DRAWS_H, DRAWS_KEY, DRAWS_FIDX); computed once
    per process, read-only."""
    model, G, thetas, states = batch((model, G))
    return _freeze(oracle_summaries(model, G, thetas, states, DRAWS_H, DRAWS_R, DRAWS_KEY, DRAWS_FIDX))


@functools.lru_cache(maxsize=None)
@_one_thread
def sweep_summaries(seed):
    """oracle_summaries of forecast_cases.sweep_case(seed); computed once per process, read-only."""
    c = forecast_cases.sweep_case(seed)
    return _freeze(oracle_summaries(c["model"], c["G"], reference_thetas(c["model"], c["G"], c["thetas"]), c["states"],
                                    c["H"], c["R"], c["key"], c["filter_index"], c["step"]))
