"""Forecast summaries, host side (no device): the entry points exist through every layer; the numpy restatement of the
definition (tests/forecast_summary_helpers.py path_summary) agrees with an independent brute force on oracle paths; the
shared batches of tests/forecast_cases.py hold on the oracle every branch the device tests rely on; and the Python
layer (shapes, exceed, quantiles, extinct_by_day, from_chain's selection, every ValueError, empty D) runs over an
oracle-backed engine double.  Every comparison is exact."""
import os
import re
import sys

import numpy as np
import pytest

import oracle
from conftest import REPO
from forecast_cases import DRAWS_FIDX, DRAWS_H, DRAWS_KEY, DRAWS_R, SEIR_DRAWS, SIR_DRAWS, infected_columns
from forecast_summary_helpers import (FIELDS, batch, draws_summaries, infectious_columns, path_summary, reductions,
                                      susceptible_columns)

CALL = dict(key=DRAWS_KEY, filter_index=DRAWS_FIDX)
BATCHES = [("sir", 1), ("seir", 1), ("sir_subgroups", 2), ("sir_subgroups", 5), ("sir_subgroups", 8)]
IDS = ["sir", "seir", "sub2", "sub5", "sub8"]


def test_entry_points_exist_in_every_layer():
    import epipf
    import gillespie_algo
    from epipf import _lib
    from epipf.engine import Engine
    assert callable(epipf.forecast_summary) and callable(epipf.forecast_summary_from_chain)
    assert "forecast_summary" in epipf.__all__ and "forecast_summary_from_chain" in epipf.__all__
    assert gillespie_algo.forecast_summary is epipf.forecast_summary
    assert callable(Engine.forecast_summary)
    assert "epipf_forecast_summary" in _lib.EXPORTS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "epipf.h")).read(), flags=re.S)
    assert re.search(r"\bint epipf_forecast_summary\s*\(", header)
    L = _lib.load()
    assert L.epipf_forecast_summary.restype is not None and len(L.epipf_forecast_summary.argtypes) == 22


# ------------------------------------------------------------------------------- the restatement against brute force
def test_path_summary_on_hand_made_paths():
    # SIR: the peak 3 is reached at t = 0.5, left, and reached again at t = 2.0: the first attainment wins
    x0 = [5, 2, 0]
    times = [0.5, 1.25, 2.0, 2.5, 3.0, 3.5]
    states = [[4, 3, 0], [4, 2, 1], [3, 3, 1], [3, 2, 2], [3, 1, 3], [3, 0, 4]]
    assert path_summary("sir", 1, x0, times, states) == (3, 0.5, 3.5, 2, 6)
    assert path_summary("sir", 1, x0, times[:4], states[:4]) == (3, 0.5, float("inf"), 2, 4)
    assert path_summary("sir", 1, x0, [], np.empty((0, 3))) == (2, 0.0, float("inf"), 0, 0)
    assert path_summary("sir", 1, [5, 0, 1], [], np.empty((0, 3))) == (0, 0.0, 0.0, 0, 0)
    # no event exceeds the start value: peak_time 0.0 although the start value is met again
    assert path_summary("sir", 1, [5, 2, 0], [0.5, 0.75], [[5, 1, 1], [4, 2, 1]])[:2] == (2, 0.0)
    # SEIR: i is column 2, not E; the path is extinct only when E and I are both empty
    assert path_summary("seir", 1, [3, 2, 0, 0], [0.5, 1.0], [[3, 1, 1, 0], [3, 1, 0, 1]]) == (1, 0.5, float("inf"), 0, 2)
    assert path_summary("seir", 1, [3, 0, 1, 0], [0.5], [[3, 0, 0, 1]]) == (1, 0.0, 0.5, 0, 1)
    # subgroups: the sum over groups
    assert path_summary("sir_subgroups", 2, [4, 1, 0, 4, 1, 0], [0.25, 0.5], [[3, 2, 0, 4, 1, 0], [3, 2, 0, 3, 2, 0]]) \
        == (4, 0.5, float("inf"), 2, 2)


@pytest.mark.parametrize("name", BATCHES, ids=IDS)
def test_path_summary_is_the_brute_force_on_oracle_paths(name):
    model, G, thetas, states = batch(name)
    ic, ac, sc = infectious_columns(model, G), infected_columns(model, G), susceptible_columns(model, G)
    got = draws_summaries(*name)
    oracle.set_num_threads(1)
    for d in range(len(states)):
        t, x, n, fin = oracle.simulate_path(model, np.tile(states[d], (DRAWS_R, 1)), thetas[d], float(DRAWS_H),
                                            key=DRAWS_KEY, filter_index=(DRAWS_FIDX + d) & 0xFFFFFFFF)
        for r in range(DRAWS_R):
            series = np.concatenate([[states[d][ic].sum()], x[r, :n[r]][:, ic].sum(axis=1)])
            when = np.concatenate([[0.0], t[r, :n[r]]])
            first = int(np.argmax(series))                            # the first index of the maximum
            assert got["peak"][d, r] == series[first] and got["peak_time"][d, r] == when[first]
            want = when[-1] if fin[r][ac].sum() == 0 else np.inf
            assert got["extinction_time"][d, r] == want
            assert got["infections"][d, r] == states[d][sc].sum() - fin[r][sc].sum()
            assert got["events"][d, r] == n[r]


# the issue's table: paths, extinct, peak at the start, peak later, paths that reach their peak again later
TABLE = {("sir", 1): (185, 41, 62, 123, 40), ("seir", 1): (185, 24, 38, 147, 85),
         ("sir_subgroups", 2): (259, 142, 129, 130, 30), ("sir_subgroups", 5): (259, 123, 121, 138, 57),
         ("sir_subgroups", 8): (259, 107, 111, 148, 53)}


@pytest.mark.parametrize("name", BATCHES, ids=IDS)
def test_shared_batches_hold_every_branch(name):
    model, G, thetas, states = batch(name)
    o = draws_summaries(*name)
    gone = np.isfinite(o["extinction_time"])
    start = o["peak_time"] == 0.0
    assert (gone.size, int(gone.sum()), int(start.sum()), int((~start).sum()), int(o["again"].sum())) == TABLE[name]
    assert gone.sum() >= 20 and (~gone).sum() >= 20 and start.sum() >= 30 and (~start).sum() >= 30
    assert o["again"].sum() >= 1                                      # what the strict > pins
    assert o["longest"] <= 372
    # a peak after the start exceeds the start value; a peak at the start is the start value
    i0 = states[:, infectious_columns(model, G)].sum(axis=1)[:, None]
    assert np.all((o["peak"] > i0) == ~start)
    day = reductions(o, DRAWS_H)["extinct_day"]
    assert day[0] >= 1 and day[3:DRAWS_H].sum() >= 1 and day[DRAWS_H] == (~gone).sum()
    if name[0] in ("sir", "seir"):
        assert np.all(day[:DRAWS_H] > 0)                              # extinction days 0..5 all occur
    # one draw with an inactive start: extinct at 0.0, peak at 0.0, no event
    idle = np.flatnonzero(states[:, infected_columns(model, G)].sum(axis=1) == 0)
    frozen = [d for d in range(len(states)) if not np.any(np.asarray(thetas[d][0])) and not np.any(thetas[d][1:])
              and states[d][infected_columns(model, G)].sum() > 0]
    if model == "sir_subgroups":
        assert list(idle) == [1]
        assert np.all(o["extinction_time"][1] == 0.0) and np.all(o["peak_time"][1] == 0.0) and not o["events"][1].any()
        assert np.all(o["peak"][1] == 0) and not o["infections"][1].any()
    # one frozen draw with infected present: +inf, bin H
    assert len(frozen) == 1
    f = frozen[0]
    assert np.all(np.isposinf(o["extinction_time"][f])) and not o["events"][f].any() and np.all(o["peak"][f] == i0[f])
    assert reductions({k: o[k][f:f + 1] for k in FIELDS}, DRAWS_H)["extinct_day"][DRAWS_H] == DRAWS_R


def test_reductions_on_a_hand_made_batch():
    paths = {"peak": np.array([[3, 2], [0, 5]]), "peak_time": np.array([[0.5, 0.0], [0.0, 3.0]]),
             "extinction_time": np.array([[2.25, np.inf], [0.0, 3.0]]), "infections": np.array([[2, 0], [0, 4]]),
             "events": np.array([[6, 1], [0, 9]])}
    r = reductions(paths, 3, bins=7)
    np.testing.assert_array_equal(r["totals"], [10, 6, 3, 16])
    np.testing.assert_array_equal(r["peak_day"], [3, 0, 1])           # t = H goes to the last day
    np.testing.assert_array_equal(r["extinct_day"], [1, 0, 2, 1])
    np.testing.assert_array_equal(r["extinct_per_draw"], [1, 2])
    np.testing.assert_array_equal(r["peak_hist"], [1, 0, 1, 1, 0, 1, 0])
    np.testing.assert_array_equal(r["infections_hist"], [2, 0, 1, 0, 1, 0, 0])


# ------------------------------------------------------------------------------- the Python layer over the oracle
@pytest.fixture
def summary(monkeypatch):
    import epipf  # noqa: F401
    import forecast_summary_oracle_engine as fe
    mod = sys.modules["epipf.forecast_summary"]
    monkeypatch.setattr(mod, "get_engine", fe.fake_get_engine)
    fe.SummaryOracleEngine.calls = []
    return mod


QS = (0.0, 0.05, 0.5, 0.95, 1.0)


@pytest.mark.parametrize("name", [("sir", 1), ("seir", 1), ("sir_subgroups", 2)], ids=["sir", "seir", "sub2"])
def test_python_layer_over_the_oracle(summary, name):
    model, G, thetas, states = batch(name)
    o = draws_summaries(*name)
    D, R, H, n = len(states), DRAWS_R, DRAWS_H, len(states) * DRAWS_R
    s = summary.forecast_summary(model, thetas, states, H, R, per_path=True, quantiles=QS, **CALL)
    assert len(s.paths) == 5
    for got, f in zip(s.paths, FIELDS):
        assert got.shape == (D, R)
        np.testing.assert_array_equal(got, o[f])
    assert s.n == n and s.events == int(o["events"].sum())
    assert s.peak_mean == o["peak"].sum() / float(n) and s.infections_mean == o["infections"].sum() / float(n)
    assert s.peak_quantiles.shape == s.infections_quantiles.shape == (len(QS),)
    np.testing.assert_array_equal(s.peak_quantiles, np.quantile(o["peak"].ravel(), QS, method="inverted_cdf"))
    np.testing.assert_array_equal(s.infections_quantiles, np.quantile(o["infections"].ravel(), QS, method="inverted_cdf"))
    assert s.peak_day_prob.shape == (H,) and s.hist["peak_day"].sum() == n
    np.testing.assert_array_equal(s.peak_day_prob, s.hist["peak_day"] / float(n))
    gone = np.isfinite(o["extinction_time"])
    assert s.extinct_by_day.shape == (H,) and np.all(np.diff(s.extinct_by_day) >= 0)
    assert s.extinct_by_day[-1] == s.p_extinct == gone.sum() / float(n)
    for k in range(H):
        assert s.extinct_by_day[k] == np.sum(o["extinction_time"] < k + 1) / float(n)
    np.testing.assert_array_equal(s.extinct_per_draw, gone.sum(axis=1) / float(R))
    top = int(o["peak"].max())
    for K in (-1, 0, 1, top // 2, top, top + 1, 10**9, 2.5):
        assert s.exceed(K) == np.sum(o["peak"] >= K) / float(n)
    want = reductions(o, H, int(states.sum(axis=1).max()) + 1)
    assert set(s.hist) == set(want) | {"n"} and s.hist["n"] == n
    for k, v in want.items():
        np.testing.assert_array_equal(s.hist[k], v, err_msg=k)
    # quantiles=None: no value histograms, no exceed; per_path=False: no paths; a scalar quantile
    lean = summary.forecast_summary(model, thetas, states, H, R, quantiles=None, **CALL)
    assert lean.paths is None and lean.peak_quantiles is None and lean.infections_quantiles is None
    assert lean.hist["peak_hist"] is None and lean.hist["infections_hist"] is None
    assert lean.peak_mean == s.peak_mean and lean.p_extinct == s.p_extinct
    with pytest.raises(ValueError, match="exceed"):
        lean.exceed(3)
    one = summary.forecast_summary(model, thetas, states, H, R, quantiles=0.5, **CALL)
    np.testing.assert_array_equal(one.peak_quantiles, [np.quantile(o["peak"].ravel(), 0.5, method="inverted_cdf")])


def test_input_forms_reach_the_engine_alike(summary):
    import forecast_summary_oracle_engine as fe
    from forecast_cases import draws_case, flat_thetas
    thetas, states = draws_case(2)
    a = summary.forecast_summary("sir_subgroups", thetas, states, 3, 2, step=5, **CALL)
    b = summary.forecast_summary("sir_subgroups", flat_thetas(thetas), states.reshape(7, 2, 3) + 0.25, 3, 2, step=5, **CALL)
    (th_a, st_a, *rest_a), (th_b, st_b, *rest_b) = fe.SummaryOracleEngine.calls
    np.testing.assert_array_equal(th_a, th_b)
    np.testing.assert_array_equal(st_a, st_b)                        # [D, G, 3] flattened, rounded
    assert rest_a == rest_b == [3, 2, DRAWS_KEY, DRAWS_FIDX, 5]
    assert a.events == b.events and a.peak_mean == b.peak_mean


def test_from_chain_selects_like_forecast_from_chain(summary):
    import forecast_summary_oracle_engine as fe
    rs = np.random.RandomState(2)
    n_iter, T = 11, 4
    thetas = np.stack([rs.uniform(0.2, 2.0, n_iter), rs.uniform(0.1, 1.0, n_iter)], axis=1)
    trajs = np.stack([rs.randint(20, 60, (T, n_iter)), rs.randint(0, 6, (T, n_iter)), rs.randint(0, 9, (T, n_iter))],
                     axis=2).astype(float)
    s = summary.forecast_summary_from_chain("sir", thetas, trajs, 3, burn_in=3, thin=2, replicates=5, per_path=True,
                                            **CALL)
    th, st, H, R, key, fidx, step = fe.SummaryOracleEngine.calls[-1]
    np.testing.assert_array_equal(th, thetas[3::2])
    np.testing.assert_array_equal(st, trajs[-1, 3::2])
    assert (H, R, key, fidx, step) == (3, 5, DRAWS_KEY, DRAWS_FIDX, 0) and s.paths[0].shape == (4, 5)
    direct = summary.forecast_summary("sir", thetas[3::2], trajs[-1, 3::2], 3, 5, per_path=True, **CALL)
    for a, b in zip(s.paths, direct.paths):
        np.testing.assert_array_equal(a, b)
    as_list = summary.forecast_summary_from_chain("sir", [tuple(t) for t in thetas], trajs, 3, burn_in=3, thin=2,
                                                  replicates=5, **CALL)
    assert as_list.events == s.events
    with pytest.raises(ValueError, match="sampled_trajs"):
        summary.forecast_summary_from_chain("sir", thetas, np.zeros((4, 3)), 3)
    with pytest.raises(ValueError, match="thetas for"):
        summary.forecast_summary_from_chain("sir", thetas[:5], trajs, 3)
    with pytest.raises(ValueError, match="burn_in"):
        summary.forecast_summary_from_chain("sir", thetas, trajs, 3, thin=0)
    with pytest.raises(ValueError, match="burn_in"):
        summary.forecast_summary_from_chain("sir", thetas, trajs, 3, burn_in=-1)


def test_empty_batch_gives_nans(summary):
    s = summary.forecast_summary("sir", np.zeros((0, 2)), np.zeros((0, 3)), 4, 3, per_path=True, **CALL)
    assert s.n == 0 and s.events == 0
    assert np.isnan(s.peak_mean) and np.isnan(s.infections_mean) and np.isnan(s.p_extinct) and np.isnan(s.exceed(1))
    assert s.peak_day_prob.shape == s.extinct_by_day.shape == (4,)
    assert np.all(np.isnan(s.peak_day_prob)) and np.all(np.isnan(s.extinct_by_day))
    assert s.peak_quantiles.shape == (3,) and np.all(np.isnan(s.peak_quantiles)) and np.all(np.isnan(s.infections_quantiles))
    assert s.extinct_per_draw.shape == (0,) and all(p.shape == (0, 3) for p in s.paths)
    assert s.hist["extinct_day"].shape == (5,) and not s.hist["extinct_day"].any()


def test_bad_arguments_raise_before_any_context():
    import epipf
    from epipf import engine
    th, st = SIR_DRAWS[0][:2], SIR_DRAWS[1][:2]
    cached = dict(engine._CACHE)
    with pytest.raises(ValueError, match="horizon"):
        epipf.forecast_summary("sir", th, st, 0)
    with pytest.raises(ValueError, match="replicates"):
        epipf.forecast_summary("sir", th, st, 5, 0)
    with pytest.raises(ValueError, match="thetas for"):
        epipf.forecast_summary("sir", th[:1], st, 5)
    with pytest.raises(ValueError, match="states must be"):
        epipf.forecast_summary("sir", th, st[:, :2], 5)
    with pytest.raises(ValueError, match="columns"):
        epipf.forecast_summary("sir", np.ones((2, 3)), st, 5)
    with pytest.raises(ValueError, match="columns"):
        epipf.forecast_summary("sir_subgroups", np.ones((2, 4)), np.ones((2, 6)), 5)
    with pytest.raises(ValueError, match="states must be"):
        epipf.forecast_summary("sir_subgroups", [(np.full((2, 2), 0.5), 0.3)], np.ones((1, 3)), 5)
    with pytest.raises(ValueError, match="states must be"):
        epipf.forecast_summary("seir", SEIR_DRAWS[0], SIR_DRAWS[1], 5)
    with pytest.raises(ValueError, match="non-negative"):
        epipf.forecast_summary("sir", th, [[60, -3, 0], [80, 1, 4]], 5)
    with pytest.raises(ValueError, match="thetas is empty"):
        epipf.forecast_summary("sir_subgroups", [], np.zeros((0, 6)), 5)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        epipf.forecast_summary("sir", th, st, 5, quantiles=(0.5, 1.5))
    with pytest.raises(ValueError, match="fit int32"):
        epipf.forecast_summary("sir", th, st, 5, 2**30)
    # two histograms of 4 (M + 1) bytes each over 256 MiB
    with pytest.raises(ValueError, match="per_path=True"):
        epipf.forecast_summary("sir", th, [[40_000_000, 10, 0], [80, 1, 4]], 30)
    assert engine._CACHE == cached                                    # no context was created
