"""The numpy restatement of the incidence filter (tests/incidence_restatement.py) pinned on the CPU: its
anchor to the oracle's state filter, what each case of tests/incidence_cases.py contains, and that the likelihood tells
the true infection rate from half of it.  tests/test_gpu_incidence.py runs the same inputs on the device.  No GPU.

The 3-day series' log-likelihood is the committed fixture's (its thinning seed is tests/golden/make_incidence_fixture.py's
choice); every other figure is the one DESIGN.md §19 tabulates."""
import numpy as np
import pytest

import incidence_cases as ic
import incidence_restatement as ir
import oracle

# loglik at beta 0.8 minus loglik at beta 0.4 (gamma 0.3, N = 200, index 0, keys 1..4, 24 daily SIR reports)
GAPS = {(0, 1): (29.1, 29.3, 25.0, 27.0), (0,): (29.8, 21.2, 22.3, 23.3)}


@pytest.mark.parametrize("model", ["sir", "seir"])
@pytest.mark.parametrize("n,days", [(1, 1), (65, 10), (200, 2)])
def test_anchor_unreported_counts_are_the_state_filter_at_probs_zero(model, n, days):
    """A binomial with p = 0 and y = 0 weighs 1, as a row with nothing reported does."""
    counts = np.full((days, ir.F[model]), np.nan)
    r = ir.one_pass(counts, model, ic.THETA[model], False, 0.5, n, ic.NPOP, ic.MU, ic.KEY, ic.F)
    o = oracle.particle_filter(np.zeros((days + 2, ir.C[model])), model, ic.THETA[model], False, 0.0, n, ic.NPOP, ic.MU,
                               key=ic.KEY, filter_index=ic.F)
    assert r["status"] == o["status"] == 0
    assert np.array_equal(r["hidden"], o["hidden"]) and np.array_equal(r["ancestry"], o["ancestry"])
    assert (r["log_zetas"] == 0.0).all() and (o["log_zetas"] == 0.0).all()


@pytest.mark.parametrize("model", ["sir", "seir"])
def test_cumulate_changes_nothing_when_every_entry_is_reported(model):
    counts = ic.daily(model, False, ic.COLUMNS[model][-1])
    a = ic.restate(counts, model, ic.THETA[model], False, 0.5, cumulate=True)
    b = ic.restate(counts, model, ic.THETA[model], False, 0.5, cumulate=False)
    assert a["status"] == b["status"] == 0
    for k in ("hidden", "ancestry", "log_zetas", "acc"):
        assert np.array_equal(a[k], b[k]), k
    assert a["log_zetas"][1] == 0.0 and a["log_zetas"][-1] < a["log_zetas"][-2] < 0.0   # the last report is counted


def test_three_day_totals_need_cumulate():
    c = ic.fixture()["threeday"]
    assert np.isnan(c).sum() == 16 and not np.isnan(c[2::3]).any()
    r = ic.restate(c, "sir", (0.8, 0.3), False, 0.5, cumulate=True)
    assert r["status"] == 0 and r["log_zetas"][-1] == pytest.approx(-24.445, abs=5e-3)
    dead = ic.restate(c, "sir", (0.8, 0.3), False, 0.5, cumulate=False)    # a day cannot hold three days' cases
    assert dead["status"] == ir.DEGENERATE and dead["step"] == 10
    assert np.isneginf(dead["log_zetas"][10:]).all() and np.isfinite(dead["log_zetas"][:10]).all()
    # the accumulator of a reported day is the sum of its block's flows along the lineage
    a, h, acc = r["ancestry"], r["hidden"], r["acc"]
    for j in range(ic.N):
        i2 = a[3, j]
        i1 = a[2, i2]
        f = [ir.flows("sir", h[p - 1][a[p]], h[p]) for p in (1, 2, 3)]
        assert (acc[3, j] == f[0][i1] + f[1][i2] + f[2][j]).all()


def test_weekly_totals_need_cumulate():
    c = ic.fixture()["weekly"]
    ll = []
    for key in (1, 2, 3, 4):
        r = ic.restate(c, "sir", (0.8, 0.3), False, 0.5, n=200, key=key, f=0, cumulate=True)
        assert r["status"] == 0
        ll.append(r["log_zetas"][-1])
        assert ic.restate(c, "sir", (0.8, 0.3), False, 0.5, n=200, key=key, f=0)["status"] == ir.DEGENERATE
    assert -20.05 < min(ll) and max(ll) < -18.25, ll


@pytest.mark.parametrize("theta,key,step", [
    ((0.8, 0.3), 11, None), ((0.8, 0.3), 1, None), ((0.8, 0.3), 2, None), ((0.4, 0.3), 11, None),
    ((1.6, 0.3), 11, None), ((0.8, 0.1), 11, None), ((0.05, 0.3), 11, 3), ((0.05, 0.3), 1, 3), ((0.05, 0.3), 2, 3),
    ((3.0, 0.3), 11, 8), ((3.0, 0.3), 1, 8), ((3.0, 0.3), 2, 8)])
def test_statuses_of_the_daily_sir_case(theta, key, step):
    r = ic.restate(ic.daily("sir", False, (0, 1)), "sir", theta, False, 0.5, key=key)
    assert r["step"] == step and r["status"] == (0 if step is None else ir.DEGENERATE)


def test_statuses_of_the_batch_and_of_every_device_case():
    steps = [ic.restate(ic.daily("sir", False, (0, 1)), "sir", th, False, pr, key=k)["step"] for th, pr, k in ic.BATCH]
    assert steps == [None, 3, None]
    for model in ("sir", "seir"):
        for obs in (False, True):
            for cols in ic.COLUMNS[model]:
                r = ic.restate(ic.daily(model, obs, cols), model, ic.THETA[model], obs, ic.PROBS[obs])
                assert r["status"] == 0, (model, obs, cols)
    assert ic.restate(ic.mixed(), "sir", (0.8, 0.3), False, 0.5, cumulate=True)["status"] == 0


@pytest.mark.parametrize("cols", [(0, 1), (0,)])
def test_does_it_work_the_true_rate_beats_half_of_it(cols):
    """loglik at (0.8, 0.3) minus loglik at (0.4, 0.3) per key: the table of DESIGN.md §19, and at least half its
    smallest entry (the margin §17 and §18 took)."""
    c = ic.daily("sir", False, cols, days=24)
    gaps = []
    for key in (1, 2, 3, 4):
        hi = ir.loglik(ic.restate(c, "sir", (0.8, 0.3), False, 0.5, n=200, key=key, f=0))
        lo = ir.loglik(ic.restate(c, "sir", (0.4, 0.3), False, 0.5, n=200, key=key, f=0))
        gaps.append(hi - lo)
    print("gaps", cols, gaps)
    np.testing.assert_allclose(gaps, GAPS[cols], atol=0.06)
    assert min(gaps) > 0.5 * min(GAPS[cols])
