"""Host side of ABC-SMC, no GPU: the identity the restatement stands on (a degenerate prior returns theta exactly), the
schedule, cdf, half-width and weight helpers of epipf.abc against the restatement's, argument validation before any
engine exists, and a statistical check of the restatement itself against rejection sampling."""
import numpy as np
import pytest

import abc_smc_restatement as rs
import oracle
from conftest import load_golden


@pytest.fixture(scope="module")
def noisy():
    return load_golden("abc_golden.npz")["abc_noisy_150"]


def test_degenerate_prior_returns_theta_exactly(noisy):
    """oracle.abc_trials with prior [b, b] x [g, g]: theta == (b, g) bit for bit (lo + 0*U == lo), and a trial's
    table does not depend on how the call that runs it is batched."""
    Y = noisy["Y"]
    rng = np.random.RandomState(5)
    for b, g in rng.uniform(0.0, 5.0, size=(40, 2)):
        pr = {"beta": [b, b], "gamma": [g, g]}
        th, rows, dist, _ = oracle.abc_trials(Y, pr, 11, 2, 1000, 3)
        assert np.all(th[:, 0] == b) and np.all(th[:, 1] == g)
        th1, rows1, dist1, _ = oracle.abc_trials(Y, pr, 11, 2, 1001, 1)
        np.testing.assert_array_equal(rows1[0], rows[1])
        assert dist1[0] == dist[1]


def test_degenerate_prior_trial_equals_the_prior_trial(noisy):
    """Trial t under its own prior draw theta_t, and trial t under the degenerate prior at theta_t: the same table."""
    Y = noisy["Y"]
    wide = {"beta": [0.0, 5.0], "gamma": [0.0, 5.0]}
    th, rows, dist, _ = oracle.abc_trials(Y, wide, 3, 1, 50, 30)
    for i in range(30):
        pr = {"beta": [th[i, 0]] * 2, "gamma": [th[i, 1]] * 2}
        th1, rows1, dist1, _ = oracle.abc_trials(Y, pr, 3, 1, 50 + i, 1)
        np.testing.assert_array_equal(th1[0], th[i])
        np.testing.assert_array_equal(rows1[0], rows[i])
        assert dist1[0] == dist[i]


def test_schedule_and_quantile_indexing():
    from epipf.abc import smc_next_threshold, smc_schedule
    assert smc_schedule([400, 250, 150]) == ([400.0, 250.0, 150.0], 3)
    assert smc_schedule(400.0) == ([400.0], 1)
    assert smc_schedule([400], quantile=0.5, generations=5) == ([400.0], 5)
    assert smc_schedule([400, 300], quantile=1.0, generations=2) == ([400.0, 300.0], 2)
    d = np.array([7.0, 1.0, 5.0, 3.0, 9.0, 2.0, 8.0, 4.0])
    assert smc_next_threshold(d, 0.5) == 4.0          # ceil(0.5 * 8) - 1 = 3 of the sorted distances
    assert smc_next_threshold(d, 1.0) == 9.0
    assert smc_next_threshold(d, 0.01) == 1.0         # ceil(0.08) - 1 = 0
    assert smc_next_threshold(d[:7], 0.5) == 5.0      # ceil(3.5) - 1 = 3 of (1, 2, 3, 5, 7, 8, 9)
    for q in (0.3, 0.5, 0.77):
        assert smc_next_threshold(d, q) == rs.next_threshold(d, q)


def test_cdf_half_width_and_weight_helpers_match_the_restatement():
    from epipf.abc import smc_cdf, smc_half_width, smc_weights
    rng = np.random.RandomState(9)
    w = rng.uniform(0.0, 1.0, 300)
    w[::7] = 0.0
    np.testing.assert_array_equal(smc_cdf(w), rs.cdf_of(w))
    assert smc_cdf(w)[-1] == 1.0 and np.all(np.diff(smc_cdf(w)) >= 0.0)
    th = rng.uniform(0.0, 5.0, (300, 2))
    for scale in (1.0, 0.5, 0.3):
        np.testing.assert_array_equal(smc_half_width(th, scale), rs.half_width(th, scale))
    hw = smc_half_width(th, 1.0)
    assert hw[0] == 0.5 * (th[:, 0].max() - th[:, 0].min())
    den = rng.uniform(0.1, 1.0, 50)
    np.testing.assert_array_equal(smc_weights(den), rs.weights_of(den))
    assert abs(smc_weights(den).sum() - 1.0) < 1e-12
    den[13] = 0.0
    with pytest.raises(ValueError, match="sample 13"):
        smc_weights(den)


def test_zero_weight_members_are_never_ancestors():
    w = np.array([0.0, 0.2, 0.0, 0.0, 0.5, 0.3, 0.0])
    cdf = rs.cdf_of(w)
    u = np.concatenate([np.linspace(0.0, 1.0, 1001)[:-1], cdf[:-1], np.nextafter(cdf, 0.0)])
    u = u[(u >= 0.0) & (u < 1.0)]
    j = rs.ancestors(cdf, u)
    assert set(j) == {1, 4, 5}
    assert rs.ancestors(cdf, np.array([0.0]))[0] == 1 and rs.ancestors(cdf, np.array([cdf[1]]))[0] == 4


def test_argument_validation_before_any_engine(noisy, monkeypatch):
    from epipf import abc
    from epipf.abc import abc_smc, smc_schedule

    def boom(*a, **k):
        raise AssertionError("an engine was requested")
    monkeypatch.setattr(abc, "get_engine", boom)
    pr = {"beta": [0.0, 5.0], "gamma": [0.0, 5.0]}
    Y = noisy["Y"]
    for bad in (dict(thresholds=None), dict(thresholds=[]), dict(thresholds=[400.0, np.nan]),
                dict(thresholds=[400.0], quantile=0.5), dict(thresholds=[400.0], generations=3),
                dict(thresholds=[400.0], quantile=0.0, generations=3),
                dict(thresholds=[400.0], quantile=1.5, generations=3),
                dict(thresholds=[400.0, 300.0, 200.0], quantile=0.5, generations=2),
                dict(thresholds=[400.0], kernel_scale=0.0), dict(thresholds=[400.0], kernel_scale=np.nan)):
        with pytest.raises(ValueError):
            abc_smc(Y, 8, priors=pr, **bad)
    with pytest.raises(ValueError):
        abc_smc(Y, 0, [400.0], pr)
    with pytest.raises(ValueError):
        abc_smc(Y, 8, [400.0], None)
    with pytest.raises(ValueError):
        smc_schedule([400.0], quantile=-0.1, generations=2)


def test_restatement_agrees_with_rejection_sampling(noisy):
    """The weighted ABC-SMC posterior mean against the first 512 rejection samples at the same final threshold, from
    another run index: per component within 5 sd_rej sqrt(1/512 + 1/ESS), sd_rej from the rejection sample, ESS from
    the final weights recomputed here."""
    Y = noisy["Y"]
    pr = {"beta": [1.0, 3.0], "gamma": [0.5, 1.5]}
    n = 512
    gens = rs.run(Y, n, [400.0, 250.0, 170.0, 120.0], pr, 4242, 0)
    last, before = gens[-1], gens[-2]
    den = rs.denominators(last["theta"], before["theta"], before["weights"], rs.half_width(before["theta"]))
    w = rs.weights_of(den)
    np.testing.assert_array_equal(w, last["weights"])
    ess = 1.0 / np.sum(w * w)
    assert np.all(last["distances"] <= 120.0)
    post, _, _ = oracle.abc_algo(Y, n, 120.0, pr, key=4242, run_index=1)
    rej = np.array([post["beta"], post["gamma"]]).T
    for c in range(2):
        mean_smc = np.sum(w * last["theta"][:, c])
        sd = rej[:, c].std(ddof=1)
        z = (mean_smc - rej[:, c].mean()) / (sd * np.sqrt(1.0 / n + 1.0 / ess))
        print(f"component {c}: smc {mean_smc:.5f} rejection {rej[:, c].mean():.5f} sd {sd:.5f} ess {ess:.1f} z {z:.2f}")
        assert abs(z) < 5.0
