"""forecast_kernel with per-draw parameters, at every one of its ten instances (SIR, SEIR, subgroups at G = 1..8):
the draws of a batch have different rates and start states and share waves, so a lane that read another draw's
ChainParam / WideParam block, a host loop that filled the blocks at the wrong stride, or a histogram cell off by a
compartment cannot pass.  Rows and event counts equal the oracle's (tests/forecast_cases.py holds the inputs,
tests/test_forecast_host.py pins on the CPU what they hold), sums and quantiles equal numpy's over the rows; integers
throughout, every comparison is assert_array_equal.  `-m gpu`; every shape is tiny."""
import numpy as np
import pytest

from forecast_cases import (DRAWS_FIDX, DRAWS_GS, DRAWS_H, DRAWS_KEY, DRAWS_R, SEIR_DRAWS, SIR_DRAWS, SWEEP_SEEDS,
                            draws_case, flat_thetas, sweep_case)
from forecast_helpers import draws_oracle, oracle_forecast, sweep_oracle

pytestmark = pytest.mark.gpu

QS = (0.0, 0.05, 0.5, 0.95, 1.0)
CALL = dict(key=DRAWS_KEY, filter_index=DRAWS_FIDX)


def _summary_is_numpys(res, rows, qs, msg=""):
    """sums, mean and quantiles of a Forecast against numpy over rows [D, R, H, C]."""
    D, R, H, C = rows.shape
    flat = np.asarray(rows).reshape(D * R, H, C)
    np.testing.assert_array_equal(res.sums, flat.sum(axis=0, dtype=np.int64), err_msg=msg)
    np.testing.assert_array_equal(res.mean, flat.sum(axis=0, dtype=np.int64) / float(D * R), err_msg=msg)
    assert res.quantiles.shape == (len(qs), H, C), msg
    np.testing.assert_array_equal(res.quantiles, np.quantile(flat, qs, axis=0, method="inverted_cdf"), err_msg=msg)


_CALLS = {}


def _draws_call(G):
    """draws_case(G)'s device call, made once per G and shared by the tests that compare with it."""
    if G not in _CALLS:
        import epipf
        thetas, states = draws_case(G)
        _CALLS[G] = epipf.forecast("sir_subgroups", thetas, states, DRAWS_H, DRAWS_R, quantiles=QS, **CALL)
        _CALLS[G].rows.setflags(write=False)
    return _CALLS[G]


# ------------------------------------------------------------------------------- a. per-draw parameters at every G
@pytest.mark.parametrize("G", DRAWS_GS)
def test_per_draw_parameters_match_the_oracle(G):
    import epipf
    thetas, states = draws_case(G)
    rows, nev = draws_oracle(G)
    res = _draws_call(G)
    assert res.rows.shape == (7, DRAWS_R, DRAWS_H, 3 * G) and res.rows.dtype == np.int32
    for d in range(7):                                            # per draw, so a failure names the draw
        np.testing.assert_array_equal(res.rows[d], rows[d], err_msg=f"G={G} draw {d}")
    assert res.events == int(nev.sum())
    _summary_is_numpys(res, rows, QS, f"G={G}")
    flat = epipf.forecast("sir_subgroups", flat_thetas(thetas), states, DRAWS_H, DRAWS_R, quantiles=QS, **CALL)
    for field in ("rows", "sums", "mean", "quantiles"):
        np.testing.assert_array_equal(getattr(flat, field), getattr(res, field), err_msg=f"G={G} {field}")
    assert flat.events == res.events


@pytest.mark.parametrize("G", [5, 8])
def test_both_subgroup_models_forecast_alike(G):
    import epipf
    thetas, states = draws_case(G)
    res = epipf.forecast("sir_subgroups2", thetas, states, DRAWS_H, DRAWS_R, quantiles=None, **CALL)
    np.testing.assert_array_equal(res.rows, _draws_call(G).rows)
    assert res.events == _draws_call(G).events


# ------------------------------------------------------------------------------- b. a draw does not depend on its batch
@pytest.mark.parametrize("G", [4, 5, 8])
def test_a_draw_alone_equals_its_rows_in_the_batch(G):
    import epipf
    thetas, states = draws_case(G)
    batch = _draws_call(G)
    events = 0
    for d in range(7):
        one = epipf.forecast("sir_subgroups", thetas[d:d + 1], states[d:d + 1], DRAWS_H, DRAWS_R, key=DRAWS_KEY,
                             filter_index=(DRAWS_FIDX + d) & 0xFFFFFFFF, quantiles=None)
        np.testing.assert_array_equal(one.rows[0], batch.rows[d], err_msg=f"G={G} draw {d}")
        events += one.events
    assert events == batch.events


# ------------------------------------------------------------------------------- c. a replicate does not depend on R
def _rows_do_not_depend_on_R(model, thetas, states):
    """The counter is (k, r, step, f + d): replicates 0..36 are the same paths whatever R is.  With R a multiple of 64
    every wave holds one draw, with R = 37 the draws share waves; no oracle is needed."""
    import epipf
    base = epipf.forecast(model, thetas, states, DRAWS_H, DRAWS_R, quantiles=None, **CALL)
    assert base.events > 0
    for R in (64, 128):
        res = epipf.forecast(model, thetas, states, DRAWS_H, R, quantiles=None, **CALL)
        assert res.rows.shape[1] == R
        np.testing.assert_array_equal(res.rows[:, :DRAWS_R], base.rows, err_msg=f"{model} R={R}")
    return base


@pytest.mark.parametrize("G", [5, 8])
def test_a_replicate_does_not_depend_on_R(G):
    base = _rows_do_not_depend_on_R("sir_subgroups", *draws_case(G))
    np.testing.assert_array_equal(base.rows, _draws_call(G).rows)


def test_a_replicate_does_not_depend_on_R_seir():
    _rows_do_not_depend_on_R("seir", *SEIR_DRAWS)


# ------------------------------------------------------------------------------- d. reduced outputs
@pytest.mark.parametrize("model,G", [("sir_subgroups", 6), ("seir", 1)])
def test_reduced_outputs_equal_the_full_call(model, G):
    import epipf
    thetas, states = draws_case(G) if model == "sir_subgroups" else SEIR_DRAWS
    full = _draws_call(G) if model == "sir_subgroups" else epipf.forecast(model, thetas, states, DRAWS_H, DRAWS_R,
                                                                          quantiles=QS, **CALL)
    assert full.events > 0 and full.rows.shape[-1] == (18 if G == 6 else 4)
    _summary_is_numpys(full, full.rows, QS, model)
    lean = epipf.forecast(model, thetas, states, DRAWS_H, DRAWS_R, rows=False, quantiles=QS, **CALL)
    assert lean.rows is None
    for field in ("sums", "mean", "quantiles"):
        np.testing.assert_array_equal(getattr(lean, field), getattr(full, field), err_msg=field)
    assert lean.events == full.events
    bare = epipf.forecast(model, thetas, states, DRAWS_H, DRAWS_R, rows=False, quantiles=None, **CALL)
    assert bare.rows is None and bare.quantiles is None
    np.testing.assert_array_equal(bare.sums, full.sums)
    np.testing.assert_array_equal(bare.mean, full.mean)
    assert bare.events == full.events


# ------------------------------------------------------------------------------- e. step
@pytest.mark.parametrize("model", ["sir", "sir_subgroups"])
def test_step_is_masked_to_24_bits(model):
    """The SSA counter's third word is (step & 0xFFFFFF) | the domain tag."""
    import epipf
    thetas, states = (SIR_DRAWS[0], SIR_DRAWS[1]) if model == "sir" else draws_case(5)
    ref = [tuple(t) for t in thetas] if model == "sir" else thetas

    def call(step):
        return epipf.forecast(model, thetas, states, DRAWS_H, DRAWS_R, step=step, quantiles=None, **CALL)

    top = call(2**24 - 1)
    rows, nev = oracle_forecast(model, ref, states, DRAWS_H, DRAWS_R, DRAWS_KEY, DRAWS_FIDX, step=2**24 - 1)
    np.testing.assert_array_equal(top.rows, rows)
    assert top.events == int(nev.sum()) > 0
    nine, wrapped, zero = call(9), call(9 + 2**24), call(0)
    np.testing.assert_array_equal(wrapped.rows, nine.rows)
    assert wrapped.events == nine.events
    assert not np.array_equal(nine.rows, zero.rows) and not np.array_equal(top.rows, zero.rows)


# ------------------------------------------------------------------------------- f. block sums at the LDS boundary
# The block sums take H C 8 bytes of LDS up to kForecastLdsSums = 32 KiB (csrc/epipf_forecast.hip) and go straight to
# HBM beyond; the horizons below are the last LDS size and the first HBM size for C = 3 and C = 24.  If the constant
# moves, move them with it.
LDS_SUMS_BYTES = 32 * 1024


@pytest.mark.parametrize("model,H", [("sir", 1365), ("sir", 1366), ("sir_subgroups", 170), ("sir_subgroups", 171)])
def test_block_sums_on_both_sides_of_the_lds_boundary(model, H):
    import epipf
    if model == "sir":
        thetas, states, R, C = SIR_DRAWS[0][2:3], SIR_DRAWS[1][2:3], 70, 3          # one live draw
    else:
        (thetas, states), R, C = draws_case(8), DRAWS_R, 24
    last_lds = LDS_SUMS_BYTES // (8 * C)
    assert H in (last_lds, last_lds + 1) and 8 * last_lds * C <= LDS_SUMS_BYTES < 8 * (last_lds + 1) * C
    res = epipf.forecast(model, thetas, states, H, R, quantiles=(0.5,), **CALL)
    assert res.rows.shape == (len(states), R, H, C) and res.events > 0
    _summary_is_numpys(res, res.rows, (0.5,), f"{model} H={H}")
    short = epipf.forecast(model, thetas, states, DRAWS_H, R, quantiles=None, **CALL)
    np.testing.assert_array_equal(res.rows[:, :, :DRAWS_H], short.rows)
    if model != "sir":
        np.testing.assert_array_equal(short.rows, _draws_call(8).rows)


# ------------------------------------------------------------------------------- g. the sweep
@pytest.mark.parametrize("seed", list(SWEEP_SEEDS))
def test_sweep(seed):
    import epipf
    c = sweep_case(seed)
    msg = "sweep seed %d: %s G=%d D=%d R=%d H=%d" % (seed, c["model"], c["G"], c["D"], c["R"], c["H"])
    rows, nev = sweep_oracle(seed)
    qs = (0.05, 0.5, 0.95)
    res = epipf.forecast(c["model"], c["thetas"], c["states"], c["H"], c["R"], key=c["key"],
                         filter_index=c["filter_index"], step=c["step"], quantiles=qs)
    assert res.rows.shape == rows.shape, msg
    for d in range(c["D"]):
        np.testing.assert_array_equal(res.rows[d], rows[d], err_msg=f"{msg} draw {d}")
    assert res.events == int(nev.sum()), msg
    _summary_is_numpys(res, rows, qs, msg)
    # without the oracle: the models' invariants on the device rows, with the start state in front
    got = res.rows.astype(np.int64)
    start = np.broadcast_to(c["states"][:, None, None, :], got[:, :, :1].shape)
    path = np.concatenate([start, got], axis=2)                   # [D, R, H + 1, C]
    assert path.min() >= 0, msg
    if c["model"] == "sir_subgroups":
        G = c["G"]
        grp = path.reshape(path.shape[:3] + (G, 3))
        assert np.all(grp.sum(axis=-1) == grp.sum(axis=-1)[:, :, :1]), msg       # every group keeps its people
        assert np.all(np.diff(grp[..., 0], axis=2) <= 0) and np.all(np.diff(grp[..., 2], axis=2) >= 0), msg
    else:
        assert np.all(path.sum(axis=-1) == path.sum(axis=-1)[:, :, :1]), msg
        assert np.all(np.diff(path[..., 0], axis=2) <= 0) and np.all(np.diff(path[..., -1], axis=2) >= 0), msg
