"""The random-walk filter on incidence as DESIGN.md §20 defines it, on the CPU restatement
(tests/walk_incidence_restatement.py): anchored bit for bit to both restatements it composes, the "does it work" table
on the step fixture's half-reported case counts, and the smoothed true infections against the raw reports.  No GPU."""
import numpy as np
import pytest

import incidence_cases as ic
import incidence_restatement as ir
import walk_cases as wc
import walk_incidence_cases as wic
import walk_incidence_restatement as wir
import walk_restatement as wr
from epipf import walk

N = 65


# ------------------------------------------------------------------------------------------- 1. the anchors
@pytest.mark.parametrize("case", ["sir", "seir", "threeday"])
def test_zero_half_widths_are_the_incidence_filter_bit_for_bit(case):
    """rw = 0 and `start` tiled from theta: hidden, ancestry, log_zetas and the accumulators of
    incidence_restatement.one_pass."""
    model = "seir" if case == "seir" else "sir"
    cumulate = case == "threeday"
    counts = ic.fixture()[case][:ic.D]
    theta = ic.THETA[model]
    want = ic.restate(counts, model, theta, False, 0.5, n=N, cumulate=cumulate)
    got = wir.one_pass(counts, model, wic.swarm(theta, N), (0.0,) * len(theta), False, 0.5, ic.NPOP, ic.MU, ic.KEY, ic.F,
                       cumulate=cumulate)
    assert got["status"] == want["status"] == 0
    for k in ("hidden", "ancestry", "acc"):
        np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(wr.bits(got["log_zetas"]), wr.bits(want["log_zetas"]))
    assert (wr.bits(got["theta_hist"]) == wr.bits(np.array(theta))).all()
    if cumulate:
        assert (got["acc"] != ir.one_pass(counts, model, theta, False, 0.5, N, ic.NPOP, ic.MU, ic.KEY, ic.F)["acc"]).any()


@pytest.mark.parametrize("model", ["sir", "seir"])
def test_unreported_counts_are_the_walk_filter_on_a_zero_series(model):
    """Every count NaN: walk_restatement.one_pass on Y = 0 at probs = 0 (a binomial with p = 0 and y = 0 weighs 1)."""
    D = 6
    start = wic.swarm(ic.THETA[model], N)
    got = wir.one_pass(np.full((D, ir.F[model]), np.nan), model, start, wic.HW[model], False, 0.5, ic.NPOP, ic.MU, ic.KEY,
                       ic.F)
    want = wr.one_pass(np.zeros((D + 2, ir.C[model])), model, start, wic.HW[model], False, 0.0, ic.NPOP, ic.MU, ic.KEY, ic.F)
    assert got["status"] == want["status"] == 0
    np.testing.assert_array_equal(got["hidden"], want["hidden"])
    np.testing.assert_array_equal(got["ancestry"], want["ancestry"])
    np.testing.assert_array_equal(wr.bits(got["theta_hist"]), wr.bits(want["theta_hist"]))
    assert (got["log_zetas"] == 0.0).all() and (want["log_zetas"] == 0.0).all()
    assert len(np.unique(got["theta_hist"][-1], axis=0)) > 1


def test_a_dying_chain_keeps_its_rows_and_loses_the_rest():
    counts = ic.daily("sir", False, (0, 1))
    start, hw, probs, key = wic.BATCH[1]
    r = wic.restate(counts, "sir", start, hw, False, probs, key=key)
    assert r["status"] == wir.DEGENERATE and r["step"] == 3
    assert np.isfinite(r["log_zetas"][:3]).all() and np.isneginf(r["log_zetas"][3:]).all()
    assert np.isfinite(r["theta_hist"][:3]).all() and np.isnan(r["theta_hist"][3:]).all()


# ------------------------------------------------------------------------------------------- 2. does it work
def smoothed_beta_median(r):
    _, qs, _ = walk.smooth_history(r["hidden"], r["ancestry"], r["theta_hist"], wic.work()["npop"], lag=wic.LAG_WORK,
                                   quantiles=(0.5,))
    return qs[0, :, 0]


@pytest.mark.parametrize("key", wic.KEYS)
@pytest.mark.parametrize("which", ["both", "infections"])
def test_the_walk_finds_the_step_from_half_reported_case_counts(which, key):
    """DESIGN.md §20's table: the plateau gap of the smoothed median of beta_t and the likelihood gain of the walk over
    fixed rates, recorded figures to the digits the table gives, bounds at half the smallest finite value."""
    i = wic.KEYS.index(key)
    r, fixed = wic.restated(which, key, True), wic.restated(which, key, False)
    assert r["status"] == 0 and r["log_zetas"].shape == (31,)
    gap = wc.plateau_gap(smoothed_beta_median(r))
    gain = r["log_zetas"][-1] - (fixed["log_zetas"][-1] if fixed["status"] == 0 else -np.inf)
    print("which", which, "key", key, "gap", gap, "gain", gain)
    assert gap == pytest.approx(wic.GAPS[which][i], abs=6e-5)
    if np.isinf(wic.GAINS[which][i]):
        assert fixed["status"] == wir.DEGENERATE and gain == np.inf
    else:
        assert gain == pytest.approx(wic.GAINS[which][i], abs=6e-3)
    assert gap > wic.GAP_BOUND[which] and gain > wic.GAIN_BOUND[which]


@pytest.mark.parametrize("key", wic.KEYS)
def test_the_smoothed_true_infections_beat_the_raw_reports(key):
    """From infections alone at lag 5: the smoothed-mean infections' mean absolute error per day against the true
    flows, below the raw reports' by at least half the smallest margin measured over keys 1-4."""
    w = wic.work()
    raw = float(np.abs(w["counts"][:, 0] - w["flows"][:, 0]).mean())
    assert raw == pytest.approx(wic.RAW_ERROR, abs=1e-4)
    r = wic.restated("infections", key, True)
    sums, _, lin = wir.smoothed_flows("sir", r["hidden"], r["ancestry"], wic.LAG_WORK, None, 301)
    assert (sums[0] == 0).all() and (sums >= 0).all() and (lin > 0).all()
    err = wic.infection_error(sums[:, 0] / float(wic.N_WORK))
    print("key", key, "error", err, "raw", raw, "total", sums[:, 0].sum() / float(wic.N_WORK))
    assert err == pytest.approx(wic.ERRORS[wic.KEYS.index(key)], abs=6e-5)
    assert raw - err > wic.MARGIN_BOUND
