"""Shared by tests/test_forecast_host.py, tests/test_gpu_forecast.py and tests/test_gpu_forecast_draws.py: daily rows of
an event path by the forecast's row rule and by the reference's traj_inf rule (tests/pred_tmps.py:55-64, restated),
oracle forecasts, and the oracle's forecasts of tests/forecast_cases.py, computed once."""
import functools

import numpy as np

import forecast_cases
import oracle


def bin_rows(x0, times, states, H):
    """Row `day` (0..H-1) = the state after the last event with time < day + 1; a day without an event repeats the
    previous row.  On an event at time t: while day < H and day + 1 <= t, the pre-event state goes to row `day`."""
    rows = np.empty((H, len(x0)), dtype=np.int64)
    cur, day = np.asarray(x0), 0
    for t, x in zip(times, states):
        while day < H and day + 1 <= t:
            rows[day] = cur
            day += 1
        cur = x
    rows[day:] = cur
    return rows


def traj_inf_rows(x0, times, states, H):
    """pred_tmps.py:57-63: row j = the path entry of the last index with floor(time) == j (the path starts with the
    initial state at time 0.0), else the previous row."""
    time = np.concatenate([[0.0], np.asarray(times, dtype=np.float64)])
    vals = np.concatenate([np.asarray(x0)[None, :], np.asarray(states).reshape(len(times), len(x0))])
    traj = np.zeros((H, len(x0)), dtype=np.int64)
    day_of = np.floor(time)
    for j in range(H):
        hits = np.flatnonzero(day_of == j)
        traj[j] = vals[hits[-1]] if hits.size else traj[j - 1]
    return traj


def oracle_forecast(model, thetas, states, H, R, key, filter_index, step=0):
    """(rows [D, R, H, C], event counts [D, R]) from oracle.simulate_path: draw d is R copies of
    states[d] with thetas[d] at filter index filter_index + d."""
    states = np.asarray(states)
    D, C = states.shape
    rows = np.empty((D, R, H, C), dtype=np.int64)
    nev = np.empty((D, R), dtype=np.int64)
    for d in range(D):
        t, x, n, fin = oracle.simulate_path(model, np.tile(states[d], (R, 1)), thetas[d], float(H), key=key,
                                            filter_index=(filter_index + d) & 0xFFFFFFFF, step=step)
        nev[d] = n
        for r in range(R):
            rows[d, r] = bin_rows(states[d], t[r, :n[r]], x[r, :n[r]], H)
            assert np.array_equal(rows[d, r, -1], fin[r])      # no event at exactly t = H in these cases
    return rows, nev


def _one_thread(fn):
    """A forecast's oracle calls hold at most a few hundred paths each: the oracle's thread pool only costs there."""
    @functools.wraps(fn)
    def run(*args):
        n = oracle.num_threads()
        oracle.set_num_threads(1)
        try:
            return fn(*args)
        finally:
            oracle.set_num_threads(n)
    return run


@functools.lru_cache(maxsize=None)
@_one_thread
def draws_oracle(G):
    """oracle_forecast of forecast_cases.draws_case(G) at the call every draws test makes; computed once per process,
    read-only."""
    thetas, states = forecast_cases.draws_case(G)
    rows, nev = oracle_forecast("sir_subgroups", thetas, states, forecast_cases.DRAWS_H, forecast_cases.DRAWS_R,
                                forecast_cases.DRAWS_KEY, forecast_cases.DRAWS_FIDX)
    rows.setflags(write=False)
    nev.setflags(write=False)
    return rows, nev


def reference_thetas(model, G, thetas):
    """A flat [D, d] theta array as the reference's thetas ((beta, gamma) pairs for the subgroup models)."""
    if not model.startswith("sir_subgroups"):
        return [tuple(t) for t in thetas]
    return [(t[:-1].reshape(G, G), float(t[-1])) for t in thetas]


@functools.lru_cache(maxsize=None)
@_one_thread
def sweep_oracle(seed):
    """oracle_forecast of forecast_cases.sweep_case(seed); computed once per process, read-only."""
    c = forecast_cases.sweep_case(seed)
    rows, nev = oracle_forecast(c["model"], reference_thetas(c["model"], c["G"], c["thetas"]), c["states"], c["H"],
                                c["R"], c["key"], c["filter_index"], c["step"])
    rows.setflags(write=False)
    nev.setflags(write=False)
    return rows, nev


def extinct(model, G, rows):
    """[D, R] bool: nobody infected (SEIR: nor exposed) on the last day."""
    return rows[:, :, -1][..., forecast_cases.infected_columns(model, G)].sum(axis=-1) == 0
