"""Posterior-predictive forecasts on the device (epipf_forecast, forecast_kernel): daily rows of every draw and
replicate equal the oracle's paths on the same keyed stream binned by the row rule, bit for bit; the device's sums and
histogram quantiles equal numpy's over those rows.  `-m gpu`; every shape is tiny."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from forecast_helpers import oracle_forecast

pytestmark = pytest.mark.gpu

KEY, FIDX = 11, 5
SIR_STATES = np.array([[60, 3, 0], [80, 1, 4], [40, 12, 9]])
SIR_THETAS = np.array([[0.9, 0.45], [0.3, 0.6], [1.7, 0.2]])
QS = (0.0, 0.05, 0.5, 0.95, 1.0)


@pytest.fixture(scope="module")
def sir_oracle():
    """Case 1's expected rows and event counts (D = 3, R = 100, H = 12), computed once."""
    return oracle_forecast("sir", SIR_THETAS, SIR_STATES, 12, 100, KEY, FIDX)


@pytest.fixture(scope="module")
def sir_call():
    """Case 1's device call: 300 lanes cross a wave and a 256-thread block boundary and leave a partial block."""
    import epipf
    return epipf.forecast("sir", SIR_THETAS, SIR_STATES, 12, 100, key=KEY, filter_index=FIDX, quantiles=QS)


def test_sir_mixed_fates_match_the_oracle(sir_oracle, sir_call):
    rows, nev = sir_oracle
    # the case holds what it is meant to: extinction, overshoot and event-free days inside a path
    extinct = rows[:, :, -1, 1] == 0
    assert 0 < extinct[0].sum() < 100 and extinct[1].all() and not extinct[2].any()
    assert np.any(np.all(rows[0, :, 1:] == rows[0, :, :-1], axis=-1) & (rows[0, :, 1:, 1] > 0))
    assert sir_call.rows.shape == (3, 100, 12, 3) and sir_call.rows.dtype == np.int32
    np.testing.assert_array_equal(sir_call.rows, rows)
    assert sir_call.events == int(nev.sum())


B2 = np.array([[0.9, 0.3], [0.2, 0.7]])
B5 = 0.3 + 0.5 * np.eye(5)
OTHER = {
    "seir": ("seir", np.array([[70, 4, 2, 0], [50, 0, 6, 3]]), [(0.8, 0.5, 0.3), (1.5, 0.9, 0.4)]),
    "sub_g2": ("sir_subgroups", np.array([[40, 2, 0, 30, 1, 1], [25, 0, 2, 45, 3, 0]]), [(B2, 0.4), (B2.T * 1.5, 0.25)]),
    "sub2_g2": ("sir_subgroups2", np.array([[40, 2, 0, 30, 1, 1], [25, 0, 2, 45, 3, 0]]), [(B2, 0.4), (B2.T * 1.5, 0.25)]),
    "sub_g5": ("sir_subgroups", np.array([[30, 2, 0] * 5, [30, 2, 0] * 5]), [(B5, 0.5), (B5, 0.5)]),
}


@pytest.mark.parametrize("name", sorted(OTHER))
def test_other_models_match_the_oracle(name):
    import epipf
    model, states, thetas = OTHER[name]
    rows, nev = oracle_forecast(model, thetas, states, 8, 70, KEY, FIDX)
    assert nev.max() > 8                                          # paths with events on most days
    res = epipf.forecast(model, thetas, states, 8, 70, key=KEY, filter_index=FIDX, quantiles=None)
    np.testing.assert_array_equal(res.rows, rows)
    assert res.events == int(nev.sum())
    assert res.quantiles is None
    np.testing.assert_array_equal(res.sums, rows.sum(axis=(0, 1)))
    if model != "seir":                                           # the flat [D, G G + 1] theta layout: same call
        flat = np.stack([np.append(np.asarray(b).reshape(-1), g) for b, g in thetas])
        res2 = epipf.forecast(model, flat, states, 8, 70, key=KEY, filter_index=FIDX, quantiles=None)
        np.testing.assert_array_equal(res2.rows, res.rows)


def test_a_draw_does_not_depend_on_its_batch(sir_call):
    import epipf
    one = epipf.forecast("sir", SIR_THETAS[1:2], SIR_STATES[1:2], 12, 100, key=KEY, filter_index=FIDX + 1)
    np.testing.assert_array_equal(one.rows[0], sir_call.rows[1])
    # the filter index wraps in uint32
    wrap = epipf.forecast("sir", SIR_THETAS[:2], SIR_STATES[:2], 12, 100, key=KEY, filter_index=2**32 - 1)
    two = epipf.forecast("sir", SIR_THETAS[1:2], SIR_STATES[1:2], 12, 100, key=KEY, filter_index=0)
    np.testing.assert_array_equal(wrap.rows[1], two.rows[0])


def test_summary_equals_numpy_over_the_rows(sir_call):
    import epipf
    flat = sir_call.rows.reshape(300, 12, 3)
    want_q = np.quantile(flat, QS, axis=0, method="inverted_cdf")
    np.testing.assert_array_equal(sir_call.sums, flat.sum(axis=0, dtype=np.int64))
    np.testing.assert_array_equal(sir_call.mean, flat.sum(axis=0, dtype=np.int64) / 300.0)
    assert sir_call.quantiles.shape == (5, 12, 3)
    np.testing.assert_array_equal(sir_call.quantiles, want_q)
    lean = epipf.forecast("sir", SIR_THETAS, SIR_STATES, 12, 100, key=KEY, filter_index=FIDX, rows=False, quantiles=QS)
    assert lean.rows is None
    np.testing.assert_array_equal(lean.sums, sir_call.sums)
    np.testing.assert_array_equal(lean.mean, sir_call.mean)
    np.testing.assert_array_equal(lean.quantiles, sir_call.quantiles)
    assert lean.events == sir_call.events
    bare = epipf.forecast("sir", SIR_THETAS, SIR_STATES, 12, 100, key=KEY, filter_index=FIDX, rows=False,
                          quantiles=None)
    assert bare.rows is None and bare.quantiles is None
    np.testing.assert_array_equal(bare.mean, sir_call.mean)


def test_summary_without_lds_sums_and_many_days():
    """H C 8 bytes beyond the launch's LDS budget for block sums (H = 1500 days x 3): sums go straight to HBM."""
    import epipf
    res = epipf.forecast("sir", SIR_THETAS[2:], SIR_STATES[2:], 1500, 70, key=KEY, filter_index=FIDX, quantiles=(0.5,))
    flat = res.rows.reshape(70, 1500, 3)
    np.testing.assert_array_equal(res.sums, flat.sum(axis=0, dtype=np.int64))
    np.testing.assert_array_equal(res.quantiles, np.quantile(flat, [0.5], axis=0, method="inverted_cdf"))
    short = epipf.forecast("sir", SIR_THETAS[2:], SIR_STATES[2:], 12, 70, key=KEY, filter_index=FIDX, quantiles=None)
    np.testing.assert_array_equal(res.rows[:, :, :12], short.rows)


def test_edges():
    import epipf
    one = epipf.forecast("sir", [[0.9, 0.45]], [[60, 3, 0]], 1, 1, key=KEY, filter_index=FIDX)
    rows, nev = oracle_forecast("sir", [(0.9, 0.45)], np.array([[60, 3, 0]]), 1, 1, KEY, FIDX)
    assert one.rows.shape == (1, 1, 1, 3)
    np.testing.assert_array_equal(one.rows, rows)
    assert one.events == int(nev.sum())
    # no infected: nothing can happen
    idle = epipf.forecast("sir", [[0.9, 0.45]], [[60, 0, 7]], 6, 5, key=KEY, filter_index=FIDX)
    np.testing.assert_array_equal(idle.rows, np.broadcast_to([60, 0, 7], (1, 5, 6, 3)))
    assert idle.events == 0
    np.testing.assert_array_equal(idle.quantiles, np.broadcast_to([60, 0, 7], (3, 6, 3)))
    # all-zero rates with infected present (the first waiting time is infinite)
    frozen = epipf.forecast("sir", [[0.0, 0.0]], [[60, 3, 0]], 6, 5, key=KEY, filter_index=FIDX)
    np.testing.assert_array_equal(frozen.rows, np.broadcast_to([60, 3, 0], (1, 5, 6, 3)))
    assert frozen.events == 0
    np.testing.assert_array_equal(frozen.mean, np.broadcast_to([60.0, 3.0, 0.0], (6, 3)))


def test_abi_rejects_bad_arguments():
    """epipf_forecast's own checks (the Python layer stops most of them earlier)."""
    from epipf import _lib
    from epipf.engine import Engine
    eng = Engine("sir", 1, 1, 1, 1)
    th = np.array([[0.9, 0.45]])
    st = np.array([[60, 3, 0]], dtype=np.int32)
    for kw, msg in ((dict(horizon=0), "horizon"), (dict(horizon=3, replicates=0), "replicates"),
                    (dict(horizon=3, bins=63), "bins must be > 63")):
        with pytest.raises(_lib.EpipfError, match=msg):
            eng.forecast(th, st, **kw)
    with pytest.raises(_lib.EpipfError, match="finite"):
        eng.forecast(np.array([[np.inf, 0.45]]), st, 3)
    with pytest.raises(_lib.EpipfError, match="int32|<="):
        eng.forecast(np.tile(th, (3, 1)), np.tile(st, (3, 1)), 1, 2**30, rows=False)
    rows, sums, hist, ev = eng.forecast(np.zeros((0, 2)), np.zeros((0, 3), dtype=np.int32), 3)
    assert rows.shape == (0, 1, 3, 3) and ev == 0 and not sums.any()
    eng.close()


def test_forecast_from_chain():
    import epipf
    from epipf import pmcmc as pm
    Y = np.load(os.path.join(GOLDEN, "datasets.npz"))["sir_binom"][:8]
    pm.seed_stream(21, 0)
    np.random.seed(5)
    th, lk, tr = pm.particle_mcmc(Y, "sir", [2.0, 1.0], 0.05, n_chains=20, probs=0.1, n_particles=64,
                                  n_population=4820, mu=20, progress=False, prefetch=0)
    T, H = Y.shape[0], 5
    assert tr.shape == (T, 20, 3)
    res, full = epipf.forecast_from_chain("sir", th, tr, H, key=21, filter_index=1000, step=9)
    assert full.shape == (20, T + H, 3)
    np.testing.assert_array_equal(full[:, :T], np.transpose(tr, (1, 0, 2)))
    np.testing.assert_array_equal(full[:, T], res.rows[:, 0, 0])
    np.testing.assert_array_equal(full[:, T:], res.rows[:, 0])
    rows, nev = oracle_forecast("sir", th, np.rint(tr[-1]).astype(np.int64), H, 1, 21, 1000, step=9)
    np.testing.assert_array_equal(res.rows, rows)
    res2, full2 = epipf.forecast_from_chain("sir", th, tr, H, burn_in=4, thin=3, key=21, filter_index=1000)
    assert full2.shape == (6, T + H, 3)                           # iterations 4, 7, 10, 13, 16, 19
    np.testing.assert_array_equal(full2[:, :T], np.transpose(tr[:, 4::3], (1, 0, 2)))
