"""forecast_summary_kernel on the device, at every one of its ten instances (SIR, SEIR, subgroups at G = 1..8): the
per-path arrays equal the numpy restatement on the oracle's paths (tests/forecast_summary_helpers.py; the batches are
tests/forecast_cases.py's, and tests/test_forecast_summary_host.py pins on the CPU which branches they hold), every
reduction equals the one recomputed from the per-path arrays, and the call agrees with epipf.forecast on the same
arguments.  Integers are compared for equality and times as doubles with ==; no tolerance anywhere.  `-m gpu`; every
shape is tiny."""
import numpy as np
import pytest

from forecast_cases import (DRAWS_FIDX, DRAWS_H, DRAWS_KEY, DRAWS_R, INSTANCES, SWEEP_SEEDS, infected_columns,
                            sweep_case)
from forecast_summary_helpers import (FIELDS, batch, draws_summaries, infectious_columns, reductions,
                                      susceptible_columns, sweep_summaries)

pytestmark = pytest.mark.gpu

QS = (0.0, 0.05, 0.5, 0.95, 1.0)
CALL = dict(key=DRAWS_KEY, filter_index=DRAWS_FIDX)
IDS = ["%s%d" % (m, G) for m, G in INSTANCES]
REDUCED = ("totals", "peak_day", "extinct_day", "extinct_per_draw", "peak_hist", "infections_hist")


def _paths_equal(got, want, msg=""):
    """Per-path arrays, field by field and draw by draw so that a failure names both; dtypes as the ABI's."""
    assert len(got) == 5
    for a, f in zip(got, FIELDS):
        b = want[f] if isinstance(want, dict) else want[FIELDS.index(f)]
        assert a.shape == b.shape and a.dtype == (np.float64 if f.endswith("time") else np.int32), f"{msg} {f}"
        for d in range(a.shape[0]):
            np.testing.assert_array_equal(a[d], b[d], err_msg=f"{msg} {f} draw {d}")


def _reductions_equal(s, want, msg="", skip=()):
    for k in REDUCED:
        if k not in skip:
            np.testing.assert_array_equal(s.hist[k], want[k], err_msg=f"{msg} {k}")


_CALLS = {}


def _call(inst):
    """The shared call of an instance's batch with everything requested, made once and shared."""
    if inst not in _CALLS:
        import epipf
        model, G, thetas, states = batch(inst)
        _CALLS[inst] = epipf.forecast_summary(model, thetas, states, DRAWS_H, DRAWS_R, per_path=True, quantiles=QS, **CALL)
        for p in _CALLS[inst].paths:
            p.setflags(write=False)
    return _CALLS[inst]


# ------------------------------------------------------------------------------- a. the oracle, at every instance
@pytest.mark.parametrize("inst", INSTANCES, ids=IDS)
def test_paths_equal_the_oracle_and_reductions_equal_the_paths(inst):
    model, G, thetas, states = batch(inst)
    o = draws_summaries(*inst)
    s = _call(inst)
    D, n = len(states), len(states) * DRAWS_R
    assert all(p.shape == (D, DRAWS_R) for p in s.paths)
    _paths_equal(s.paths, o, IDS[INSTANCES.index(inst)])
    bins = int(states.sum(axis=1).max()) + 1
    _reductions_equal(s, reductions(s.paths, DRAWS_H, bins), str(inst))
    assert s.hist["peak_hist"].shape == s.hist["infections_hist"].shape == (bins,)
    assert s.n == n and s.events == int(o["events"].sum()) > 0
    assert s.peak_mean == o["peak"].sum() / float(n) and s.infections_mean == o["infections"].sum() / float(n)
    np.testing.assert_array_equal(s.peak_quantiles, np.quantile(o["peak"].ravel(), QS, method="inverted_cdf"))
    np.testing.assert_array_equal(s.infections_quantiles, np.quantile(o["infections"].ravel(), QS, method="inverted_cdf"))
    assert s.p_extinct == np.isfinite(o["extinction_time"]).sum() / float(n)
    assert s.exceed(int(o["peak"].max())) > 0.0 == s.exceed(int(o["peak"].max()) + 1)


@pytest.mark.parametrize("inst", INSTANCES, ids=IDS)
def test_reduced_calls_return_identical_reductions(inst):
    import epipf
    model, G, thetas, states = batch(inst)
    full = _call(inst)
    lean = epipf.forecast_summary(model, thetas, states, DRAWS_H, DRAWS_R, per_path=False, quantiles=QS, **CALL)
    assert lean.paths is None
    _reductions_equal(lean, full.hist, "per_path=False")
    np.testing.assert_array_equal(lean.peak_quantiles, full.peak_quantiles)
    bare = epipf.forecast_summary(model, thetas, states, DRAWS_H, DRAWS_R, per_path=True, quantiles=None, **CALL)
    assert bare.hist["peak_hist"] is None and bare.hist["infections_hist"] is None and bare.peak_quantiles is None
    _reductions_equal(bare, full.hist, "quantiles=None", skip=("peak_hist", "infections_hist"))
    _paths_equal(bare.paths, full.paths, "quantiles=None")
    none = epipf.forecast_summary(model, thetas, states, DRAWS_H, DRAWS_R, per_path=False, quantiles=None, **CALL)
    assert none.paths is None and none.events == full.events
    _reductions_equal(none, full.hist, "neither", skip=("peak_hist", "infections_hist"))


def test_both_subgroup_models_summarise_alike():
    import epipf
    model, G, thetas, states = batch(("sir_subgroups", 5))
    s = epipf.forecast_summary("sir_subgroups2", thetas, states, DRAWS_H, DRAWS_R, per_path=True, quantiles=QS, **CALL)
    _paths_equal(s.paths, _call(("sir_subgroups", 5)).paths)


# ------------------------------------------------------------------------------- b. against epipf.forecast
@pytest.mark.parametrize("inst", INSTANCES, ids=IDS)
def test_agrees_with_forecast_on_the_same_arguments(inst):
    import epipf
    model, G, thetas, states = batch(inst)
    s = _call(inst)
    f = epipf.forecast(model, thetas, states, DRAWS_H, DRAWS_R, rows=True, quantiles=None, **CALL)
    peak, _, _, infections, events = s.paths
    assert int(events.sum(dtype=np.int64)) == s.events == f.events
    rows = f.rows.astype(np.int64)                                     # [D, R, H, C]
    sc, ic, ac = susceptible_columns(model, G), infectious_columns(model, G), infected_columns(model, G)
    s0 = states[:, sc].sum(axis=1)[:, None]
    np.testing.assert_array_equal(infections, s0 - rows[:, :, -1][..., sc].sum(axis=-1))
    by_day = np.cumsum(s.hist["extinct_day"].astype(np.int64))
    for k in range(DRAWS_H):                                           # forecast_helpers.extinct's rule, per day
        assert by_day[k] == np.sum(rows[:, :, k][..., ac].sum(axis=-1) == 0), f"day {k}"
    assert by_day[DRAWS_H] == peak.size
    assert np.all(peak >= rows[..., ic].sum(axis=-1).max(axis=2))
    assert np.all(peak >= states[:, ic].sum(axis=1)[:, None])


# ------------------------------------------------------------------------------- c. a draw alone; a replicate and R
@pytest.mark.parametrize("inst", [("sir", 1), ("seir", 1), ("sir_subgroups", 4), ("sir_subgroups", 5),
                                  ("sir_subgroups", 8)], ids=["sir", "seir", "sub4", "sub5", "sub8"])
def test_a_draw_alone_and_a_replicate_at_any_R(inst):
    import epipf
    model, G, thetas, states = batch(inst)
    full = _call(inst)
    totals = np.zeros(4, dtype=np.int64)
    for d in range(len(states)):
        one = epipf.forecast_summary(model, thetas[d:d + 1], states[d:d + 1], DRAWS_H, DRAWS_R, per_path=True,
                                     quantiles=None, key=DRAWS_KEY, filter_index=(DRAWS_FIDX + d) & 0xFFFFFFFF)
        _paths_equal(one.paths, [p[d:d + 1] for p in full.paths], f"draw {d} alone")
        assert one.hist["extinct_per_draw"][0] == full.hist["extinct_per_draw"][d]
        totals += one.hist["totals"]
    np.testing.assert_array_equal(totals, full.hist["totals"])
    # the counter is (k, r, step, f + d): replicates 0..36 are the same paths whatever R is; with R a multiple of 64
    # every wave holds one draw, with R = 37 the draws share waves
    for R in (64, 128):
        s = epipf.forecast_summary(model, thetas, states, DRAWS_H, R, per_path=True, quantiles=QS, **CALL)
        assert s.paths[0].shape == (len(states), R)
        _paths_equal([p[:, :DRAWS_R] for p in s.paths], full.paths, f"R={R}")
        _reductions_equal(s, reductions(s.paths, DRAWS_H, s.hist["peak_hist"].size), f"R={R}")


# ------------------------------------------------------------------------------- d. the sweep
@pytest.mark.parametrize("seed", list(SWEEP_SEEDS))
def test_sweep(seed):
    import epipf
    c = sweep_case(seed)
    msg = "sweep seed %d: %s G=%d D=%d R=%d H=%d" % (seed, c["model"], c["G"], c["D"], c["R"], c["H"])
    o = sweep_summaries(seed)
    s = epipf.forecast_summary(c["model"], c["thetas"], c["states"], c["H"], c["R"], key=c["key"],
                               filter_index=c["filter_index"], step=c["step"], per_path=True, quantiles=(0.05, 0.5, 0.95))
    _paths_equal(s.paths, o, msg)
    bins = int(c["states"].sum(axis=1).max()) + 1
    _reductions_equal(s, reductions(o, c["H"], bins), msg)
    lean = epipf.forecast_summary(c["model"], c["thetas"], c["states"], c["H"], c["R"], key=c["key"],
                                  filter_index=c["filter_index"], step=c["step"], quantiles=None)
    _reductions_equal(lean, s.hist, msg, skip=("peak_hist", "infections_hist"))


# ------------------------------------------------------------------------------- e. the day histograms' LDS bound
# The two day histograms take 4 (2 H + 1) bytes of LDS per block up to kForecastSummaryLdsDays = 32 KiB
# (csrc/epipf_forecast_summary.hip) and global atomics beyond; EPIPF_FORECAST_SUMMARY_LDS lowers the bound, so both
# sides run at the shared call's H = 6 (52 bytes).
@pytest.mark.parametrize("inst", [("sir", 1), ("seir", 1), ("sir_subgroups", 3), ("sir_subgroups", 8)],
                         ids=["sir", "seir", "sub3", "sub8"])
@pytest.mark.parametrize("limit,side", [("52", "lds"), ("51", "global"), ("0", "global"), ("1000000", "lds")])
def test_day_histograms_on_both_sides_of_the_bound(monkeypatch, inst, limit, side):
    import epipf
    assert 4 * (2 * DRAWS_H + 1) == 52
    model, G, thetas, states = batch(inst)
    monkeypatch.setenv("EPIPF_FORECAST_SUMMARY_LDS", limit)
    s = epipf.forecast_summary(model, thetas, states, DRAWS_H, DRAWS_R, per_path=True, quantiles=QS, **CALL)
    monkeypatch.delenv("EPIPF_FORECAST_SUMMARY_LDS")
    full = _call(inst)                                                 # no override: the LDS side
    _paths_equal(s.paths, full.paths, side)
    _reductions_equal(s, full.hist, side)


LDS_DAYS_BYTES = 32 * 1024


@pytest.mark.parametrize("H", [4095, 4096])
def test_day_histograms_at_the_constant_itself(H):
    """The last horizon whose day histograms fit the constant, and the first that does not: if the constant moves, move
    them with it.  One SIR draw that starts from a single infected person, so many of its paths are soon over."""
    import epipf
    assert 4 * (2 * 4095 + 1) <= LDS_DAYS_BYTES < 4 * (2 * 4096 + 1)
    model, G, thetas, states = batch(("sir", 1))
    one = dict(key=DRAWS_KEY, filter_index=(DRAWS_FIDX + 1) & 0xFFFFFFFF)    # draw 1's stream in the shared call
    s = epipf.forecast_summary(model, thetas[1:2], states[1:2], H, 300, per_path=True, quantiles=(0.5,), **one)
    _reductions_equal(s, reductions(s.paths, H, int(states[1].sum()) + 1), f"H={H}")
    assert s.events > 0 and s.hist["peak_day"].sum() == 300 == s.hist["extinct_day"].sum()
    short = epipf.forecast_summary(model, thetas[1:2], states[1:2], DRAWS_H, DRAWS_R, per_path=True, quantiles=None, **one)
    _paths_equal(short.paths, [p[1:2] for p in _call(("sir", 1)).paths])
    # a path over by the short horizon is the same path at the long one
    over = np.isfinite(short.paths[2][0])
    assert over.sum() >= 5
    for a, b in zip(s.paths, short.paths):
        np.testing.assert_array_equal(a[0, :DRAWS_R][over], b[0][over])


# ------------------------------------------------------------------------------- f. the C ABI
def _abi(model="sir", G=1):
    from epipf import _lib
    from epipf.engine import get_engine
    return _lib, _lib.load(), get_engine(model, G, 1, 1, 1, 0)


def _raw(L, eng, D, R, H, theta, states, bins, per_path="all", hists="both", d=None, fill=0):
    """One raw call; per_path: "all", "none", or the number of leading non-NULL per-path pointers."""
    from epipf._lib import ptr
    keep = 5 if per_path == "all" else 0 if per_path == "none" else int(per_path)
    n = max(D * R, 1) if keep else 1
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(max(D, 1), -1)
    states = np.ascontiguousarray(states, dtype=np.int32).reshape(max(D, 1), -1)
    paths = [np.full(n, fill, dtype=t) for t in (np.int32, np.float64, np.float64, np.int32, np.int32)]
    pp = [p if i < keep else None for i, p in enumerate(paths)]
    out = dict(totals=np.full(4, fill, dtype=np.int64), peak_hist=np.full(max(bins, 1), fill, dtype=np.uint32),
               infections_hist=np.full(max(bins, 1), fill, dtype=np.uint32),
               peak_day=np.full(max(H, 1), fill, dtype=np.uint32), extinct_day=np.full(max(H, 1) + 1, fill, dtype=np.uint32),
               extinct_per_draw=np.full(max(D, 1), fill, dtype=np.uint32))
    ph = out["peak_hist"] if hists in ("both", "peak") else None
    ih = out["infections_hist"] if hists in ("both", "infections") else None
    rc = L.epipf_forecast_summary(eng._h, D, R, H, ptr(theta), theta.shape[1] if d is None else d, ptr(states),
                                  DRAWS_KEY, DRAWS_FIDX, 0, ptr(pp[0]), ptr(pp[1]), ptr(pp[2]), ptr(pp[3]), ptr(pp[4]),
                                  ptr(out["totals"]), ptr(ph), ptr(ih), int(bins), ptr(out["peak_day"]),
                                  ptr(out["extinct_day"]), ptr(out["extinct_per_draw"]))
    return rc, out, L.epipf_last_error().decode(errors="replace")


def test_abi_refuses_bad_arguments():
    lib, L, eng = _abi()
    th, st = [[0.9, 0.45], [0.3, 0.6]], [[60, 3, 0], [80, 1, 4]]       # the largest total is 85
    ok, out, _ = _raw(L, eng, 2, 3, 4, th, st, 86)
    assert ok == lib.OK and out["peak_day"].sum() == 6
    bad = [dict(bins=85), dict(bins=0), dict(H=0), dict(H=-1), dict(R=0), dict(R=-2), dict(d=3), dict(d=1),
           dict(hists="peak"), dict(hists="infections")] + [dict(per_path=k) for k in (1, 2, 3, 4)]
    for kw in bad:
        a = dict(D=2, R=3, H=4, theta=th, states=st, bins=86)
        a.update(kw)
        rc, _, err = _raw(L, eng, **a)
        assert rc == lib.EINVAL and err, kw
    # the per-path pointers may also be missing from the front
    from epipf._lib import ptr
    z = np.zeros(6, dtype=np.int32)
    zt, tot, day, eday = np.zeros(6), np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.uint32), np.zeros(5, dtype=np.uint32)
    tha, sta = np.array(th), np.array(st, dtype=np.int32)
    rc = L.epipf_forecast_summary(eng._h, 2, 3, 4, ptr(tha), 2, ptr(sta), 1, 0, 0, None, ptr(zt), ptr(zt), ptr(z), ptr(z),
                                  ptr(tot), None, None, 0, ptr(day), ptr(eday), None)
    assert rc == lib.EINVAL and L.epipf_last_error()
    # the other checks of epipf_forecast: theta finite and >= 0, states non-negative
    for theta in ([[0.9, -0.1], [0.3, 0.6]], [[0.9, np.inf], [0.3, 0.6]], [[np.nan, 0.4], [0.3, 0.6]]):
        rc, _, err = _raw(L, eng, 2, 3, 4, theta, st, 86)
        assert rc == lib.EINVAL and "theta" in err
    rc, _, err = _raw(L, eng, 2, 3, 4, th, [[60, -3, 0], [80, 1, 4]], 86)
    assert rc == lib.EINVAL and "non-negative" in err
    rc, _, err = _raw(L, eng, 2, 2**30, 4, th, st, 86, per_path="none")
    assert rc == lib.EINVAL and "n_draws * replicates" in err
    # histograms not requested: bins is not looked at; extinct_per_draw may be NULL
    rc, out, _ = _raw(L, eng, 2, 3, 4, th, st, 0, hists="none")
    assert rc == lib.OK and out["peak_day"].sum() == 6
    rc = L.epipf_forecast_summary(eng._h, 2, 3, 4, ptr(tha), 2, ptr(sta), DRAWS_KEY, DRAWS_FIDX, 0, None, None, None,
                                  None, None, ptr(tot), None, None, 0, ptr(day), ptr(eday), None)
    assert rc == lib.OK
    np.testing.assert_array_equal(tot, out["totals"])
    np.testing.assert_array_equal(day, out["peak_day"])
    np.testing.assert_array_equal(eday, out["extinct_day"])


@pytest.mark.parametrize("model,G", [("sir", 1), ("sir_subgroups", 6)])
def test_abi_empty_batch_is_ok_with_zeros(model, G):
    lib, L, eng = _abi(model, G)
    d = 2 if model == "sir" else G * G + 1
    rc, out, _ = _raw(L, eng, 0, 3, 4, np.zeros((1, d)), np.zeros((1, eng.C)), 5, fill=7)
    assert rc == lib.OK
    for k in ("totals", "peak_day", "extinct_day", "peak_hist", "infections_hist"):
        assert not out[k].any(), k
