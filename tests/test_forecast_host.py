"""Posterior-predictive forecasts, host side (no device): the entry points exist through every layer, the
histogram-to-quantile step is numpy's inverted-CDF rule, the forecast's row rule is the reference's traj_inf rule
(tests/pred_tmps.py:55-64) on oracle paths, bad arguments raise before any context is created, and the cases of
tests/forecast_cases.py hold on the oracle what the device tests need them to hold."""
import os
import re

import numpy as np
import pytest

import oracle
from conftest import REPO
from forecast_cases import DRAWS_GS, DRAWS_H, DRAWS_R, INSTANCES, SWEEP_SEEDS, draws_case, infected_columns, sweep_case
from forecast_helpers import bin_rows, draws_oracle, extinct, sweep_oracle, traj_inf_rows


def test_entry_points_exist_in_every_layer():
    import epipf
    import gillespie_algo
    from epipf import _lib
    from epipf.engine import Engine
    assert callable(epipf.forecast) and callable(epipf.forecast_from_chain)
    assert "forecast" in epipf.__all__ and "forecast_from_chain" in epipf.__all__
    assert gillespie_algo.forecast is epipf.forecast and gillespie_algo.forecast_from_chain is epipf.forecast_from_chain
    assert callable(Engine.forecast)
    assert "epipf_forecast" in _lib.EXPORTS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "epipf.h")).read(), flags=re.S)
    assert re.search(r"\bint epipf_forecast\s*\(", header)
    L = _lib.load()
    assert L.epipf_forecast.restype is not None and len(L.epipf_forecast.argtypes) == 15


QS = [0.0, 0.05, 0.5, 0.95, 1.0]


@pytest.mark.parametrize("samples", [
    np.array([7]),                                            # a single sample
    np.array([3, 3, 3, 3, 3, 3]),                             # all tied
    np.array([0, 0, 1, 1, 1, 5, 5, 9, 9, 9, 9, 12]),          # ties, gaps, value 0
    np.arange(20),                                            # q n integral at 0.05, 0.5, 0.95
    np.arange(40)[::-1] // 3,
    np.random.RandomState(3).randint(0, 50, 1000),
    np.random.RandomState(4).randint(0, 4, 37),
], ids=["single", "tied", "gaps", "arange20", "thirds", "rand1000", "rand37"])
def test_quantiles_from_hist_is_numpys_inverted_cdf(samples):
    from epipf.forecast import quantiles_from_hist
    hist = np.bincount(samples, minlength=int(samples.max()) + 3).astype(np.uint32)     # empty bins above the maximum
    got = quantiles_from_hist(hist, QS)
    want = np.quantile(samples, QS, method="inverted_cdf")
    assert got.shape == (len(QS),)
    np.testing.assert_array_equal(got, want)


def test_quantiles_from_hist_keeps_leading_axes():
    from epipf.forecast import quantiles_from_hist
    rs = np.random.RandomState(8)
    samples = rs.randint(0, 30, (4, 3, 211))                  # [H, C, n]
    hist = np.zeros((4, 3, 30), dtype=np.uint32)
    for h in range(4):
        for c in range(3):
            hist[h, c] = np.bincount(samples[h, c], minlength=30)
    got = quantiles_from_hist(hist, QS)
    assert got.shape == (5, 4, 3)
    np.testing.assert_array_equal(got, np.quantile(samples, QS, axis=-1, method="inverted_cdf"))
    with pytest.raises(ValueError):
        quantiles_from_hist(hist, [1.5])
    with pytest.raises(ValueError):
        quantiles_from_hist(np.zeros((2, 5), dtype=np.uint32), [0.5])


B5 = 0.3 + 0.5 * np.eye(5)
PATH_CASES = [
    ("sir", [[60, 3, 0]], (0.9, 0.45), 12),
    ("sir", [[80, 1, 4]], (0.3, 0.6), 12),
    ("sir", [[40, 12, 9]], (1.7, 0.2), 12),
    ("seir", [[70, 4, 2, 0]], (0.8, 0.5, 0.3), 8),
    ("sir_subgroups", [[40, 2, 0, 30, 1, 1]], (np.array([[0.9, 0.3], [0.2, 0.7]]), 0.4), 8),
    ("sir_subgroups", [[30, 2, 0] * 5], (B5, 0.5), 8),
]


@pytest.mark.parametrize("model,x0,theta,H", PATH_CASES, ids=["sir0", "sir1", "sir2", "seir", "sub2", "sub5"])
def test_row_rule_is_traj_inf_on_oracle_paths(model, x0, theta, H):
    R = 60
    x0 = np.asarray(x0[0])
    t, x, n, fin = oracle.simulate_path(model, np.tile(x0, (R, 1)), theta, float(H), key=11, filter_index=5)
    quiet = 0
    for r in range(R):
        a = bin_rows(x0, t[r, :n[r]], x[r, :n[r]], H)
        b = traj_inf_rows(x0, t[r, :n[r]], x[r, :n[r]], H)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a[-1], fin[r])
        quiet += int(np.any(np.all(a[1:] == a[:-1], axis=1)))
    assert quiet > 0                                          # repeated rows (event-free days or extinction) occur


def test_row_rule_on_a_hand_made_path():
    x0 = [5, 1, 0]
    times = [0.5, 2.0, 2.25, 3.999]                           # an event exactly on a day boundary; day 1 has none
    states = [[4, 2, 0], [4, 1, 1], [3, 2, 1], [3, 1, 2]]
    want = [[4, 2, 0], [4, 2, 0], [3, 2, 1], [3, 1, 2], [3, 1, 2]]
    np.testing.assert_array_equal(bin_rows(x0, times, states, 5), want)
    np.testing.assert_array_equal(traj_inf_rows(x0, times, states, 5), want)
    np.testing.assert_array_equal(bin_rows(x0, [], np.empty((0, 3)), 3), [x0] * 3)


def test_bad_arguments_raise_before_any_context():
    import epipf
    from epipf import engine
    th = np.array([[0.9, 0.45], [0.3, 0.6]])
    st = np.array([[60, 3, 0], [80, 1, 4]])
    cached = dict(engine._CACHE)
    with pytest.raises(ValueError, match="horizon"):
        epipf.forecast("sir", th, st, 0)
    with pytest.raises(ValueError, match="replicates"):
        epipf.forecast("sir", th, st, 5, 0)
    with pytest.raises(ValueError, match="thetas for"):
        epipf.forecast("sir", th[:1], st, 5)
    with pytest.raises(ValueError, match="states must be"):
        epipf.forecast("sir", th, st[:, :2], 5)
    with pytest.raises(ValueError, match="columns"):
        epipf.forecast("sir", np.ones((2, 3)), st, 5)
    with pytest.raises(ValueError, match="columns"):
        epipf.forecast("sir_subgroups", np.ones((2, 4)), np.ones((2, 6)), 5)
    with pytest.raises(ValueError, match="states must be"):
        epipf.forecast("sir_subgroups", [(np.full((2, 2), 0.5), 0.3)], np.ones((1, 3)), 5)
    with pytest.raises(ValueError, match="non-negative"):
        epipf.forecast("sir", th, [[60, -3, 0], [80, 1, 4]], 5)
    # H C (M + 1) 4 bytes over 256 MiB: 30 x 3 x (10^6 + 1) x 4 = 360 MB
    with pytest.raises(ValueError, match="rows=True"):
        epipf.forecast("sir", th, [[999_990, 10, 0], [80, 1, 4]], 30)
    with pytest.raises(ValueError, match="sampled_trajs"):
        epipf.forecast_from_chain("sir", th, np.zeros((4, 3)), 5)
    with pytest.raises(ValueError, match="thetas for"):
        epipf.forecast_from_chain("sir", th, np.zeros((4, 3, 3)), 5)
    assert engine._CACHE == cached                            # no context was created


# ----------------------------------------------------- what tests/test_gpu_forecast_draws.py's cases hold (oracle only)
@pytest.mark.parametrize("G", DRAWS_GS)
def test_draws_case_holds_its_fate_mix(G):
    """draws_oracle's oracle_forecast also asserts that no path has an event at exactly t = H."""
    thetas, states = draws_case(G)
    rows, nev = draws_oracle(G)
    D, R = nev.shape
    assert (D, R) == (7, DRAWS_R) and rows.shape == (7, DRAWS_R, DRAWS_H, 3 * G)
    gone = extinct("sir_subgroups", G, rows).sum(axis=1)
    infected0 = states[:, 1::3].sum(axis=1)
    assert infected0[1] == 0 and nev[1].sum() == 0                   # nobody infected: no event
    assert list(states[2, 1::3]) == [1] + [0] * (G - 1)              # a single infected person, in group 0
    assert infected0[-1] > 0 and nev[-1].sum() == 0 and not np.any(thetas[-1][0]) and thetas[-1][1] == 0.0
    assert np.any((gone > 0) & (gone < R))                           # a draw with both fates among its replicates
    if G >= 3:
        assert np.any((gone == 0) & (nev.sum(axis=1) > 0))           # a live draw without extinction
    live = [d for d in range(D) if nev[d].sum() > 0]
    assert len(live) >= 4
    for i, a in enumerate(live):                                     # no two live draws could stand in for each other
        for b in live[i + 1:]:
            assert not np.array_equal(rows[a], rows[b]), (a, b)
            assert not np.array_equal(thetas[a][0], thetas[b][0]) and not np.array_equal(states[a], states[b])


def test_sweep_cases_hold_their_mix():
    cases = [sweep_case(s) for s in SWEEP_SEEDS]
    launched = [(c["model"], c["G"]) for c in cases]
    assert all(launched.count(inst) >= 2 for inst in INSTANCES)      # every kernel instance at least twice
    fates = set()
    for s, c in zip(SWEEP_SEEDS, cases):
        assert c["D"] * c["R"] <= 6500 and 0 <= c["key"] < 2**63 and 0 <= c["filter_index"] < 2**32
        assert 0 <= c["step"] < 2**24 and c["states"].min() >= 0 and c["states"].max() <= 60
        rows, nev = sweep_oracle(s)                                  # asserts: no event at exactly t = H
        gone = extinct(c["model"], c["G"], rows).sum(axis=1)
        fates |= {"all" if g == c["R"] else "none" if g == 0 else "mixed" for g in gone}
    assert fates == {"all", "none", "mixed"}
    lanes = [c["D"] * c["R"] for c in cases]
    assert min(lanes) < 64 and max(lanes) > 256                      # less than a wave; more than one 256-lane block
    assert any(n > 256 and n % 256 for n in lanes)                   # a partial last block
    assert any(c["R"] % 64 == 0 for c in cases)                      # wave-uniform draws
    assert any(c["R"] % 64 and c["D"] > 1 and c["D"] * c["R"] > 64 for c in cases)   # draws sharing waves
    assert any(c["filter_index"] >= 2**31 for c in cases) and any(c["step"] >= 2**16 for c in cases)
    idle = sum(int(np.sum(c["states"][:, infected_columns(c["model"], c["G"])].sum(axis=1) == 0)) for c in cases)
    frozen = sum(int(np.sum(~c["thetas"].any(axis=1))) for c in cases)
    draws = sum(c["D"] for c in cases)
    assert 0.08 * draws < idle < 0.25 * draws and 0.08 * draws < frozen < 0.25 * draws
