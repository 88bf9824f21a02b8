"""Negative-binomial reporting pinned on the CPU: the host's coefficients against mpmath bit for bit, the
restated factor (tests/negbin_restatement.py) against scipy.stats.nbinom and its pins, the special cases, what each
case of tests/negbin_cases.py contains, and the does-it-work table of §21.  tests/test_gpu_negbin.py runs the same
inputs on the device.  No GPU: epipf_negbin_coefficients is host code."""
import numpy as np
import pytest
from scipy import stats

import incidence_cases as ic
import incidence_restatement as ir
import negbin_cases as nc
import negbin_restatement as nr
from epipf import _lib

# (y, n, rho, kappa) -> c, factor: the prototype's values (mpmath at 60 digits, glibc's log, math.exp)
PINS = [((39, 31, .5, 2), "0x1.d82d33b32720dp+1", "0x1.2d48b7bb5df10p-8"),
        ((101, 96, .5, .5), "-0x1.70c9f17b49ea8p+1", "0x1.05ffd9a392638p-9"),
        ((7, 250, .1, 1e6), "0x1.60bbd600ccdb0p+6", "0x1.1a3664b983e81p-16"),
        ((0, 31, .5, 2), "0x0.0p+0", "0x1.abfd7e03c2fa4p-7"),
        ((3, 0, .5, 2), None, "0x0.0p+0"),
        ((0, 0, .5, 2), None, "0x1.0000000000000p+0")]
YS, KAPPAS = (0, 1, 2, 39, 101, 5000), (0.01, 0.5, 2, 50, 1e6)


@pytest.mark.skipif(not nr.HAVE_MPMATH, reason="mpmath is the reference of this comparison")
def test_library_coefficients_equal_mpmath_bit_for_bit():
    for k in KAPPAS:
        got = nr.library_coefficients(YS, k)
        for y, g in zip(YS, got):
            assert g.hex() == nr.coefficient(y, k).hex(), (y, k)
    for (y, _n, _rho, k), c, _f in PINS:
        if c is not None:
            assert nr.library_coefficients([y], k)[0].hex() == float.fromhex(c).hex() == nr.coefficient(y, k).hex()
    z = nr.library_coefficients([0, 0], 0.3)
    assert z.tolist() == [0.0, 0.0] and not np.signbit(z).any()            # exactly 0 at y = 0


@pytest.mark.parametrize("y,k", [([1.5], 2.0), ([-1.0], 2.0), ([np.nan], 2.0), ([np.inf], 2.0), ([1.0], 0.0),
                                 ([1.0], -1.0), ([1.0], 1.0000001e6), ([1.0], np.nan), ([1.0], np.inf)])
def test_library_coefficients_refusals(y, k):
    with pytest.raises(_lib.EpipfError, match="integer >= 0|outside"):
        nr.library_coefficients(y, k)
    assert nr.library_coefficients([1.0], 1e6).shape == (1,)               # the cap itself is inside


def test_the_pinned_factors():
    for (y, n, rho, k), _c, f in PINS:
        assert nr.factor(y, n, rho, k).hex() == float.fromhex(f).hex(), (y, n, rho, k)
        assert nr.factors(y, [n], rho, k)[0].hex() == float.fromhex(f).hex()
    assert nr.factor(7, 250, .1, 1e6) == pytest.approx(1.68e-5, rel=5e-3)  # Poisson(25) at 7, nearly


def test_factor_against_scipy_on_the_sweep():
    """3,000 draws of (y < 400, n < 400, rho in (0.01, 1.5), kappa in 10^(-2..6)) against scipy's pmf at rtol 1e-8: the
    derived bound is kappa (|log kappa| + |log t|) 2^-53 <= 3e-9 at kappa = 1e6, so the tolerance has three-fold
    headroom (DESIGN.md §21 records the measured worst value)."""
    rng = np.random.default_rng(21)
    y, n = rng.integers(0, 400, 3000), rng.integers(0, 400, 3000)
    rho, kap = rng.uniform(0.01, 1.5, 3000), 10.0 ** rng.uniform(-2, 6, 3000)
    got = np.array([nr.factor(*a) for a in zip(y, n, rho, kap)])
    m = rho * n
    want = stats.nbinom.pmf(y, kap, kap / (kap + m))
    zero = m == 0
    assert zero.any() and np.array_equal(got[zero], np.where(y[zero] == 0, 1.0, 0.0))
    pos = want > 0.0                                       # (some fifty pmfs underflow to 0.0, in both)
    rel = np.abs(got[pos] - want[pos]) / want[pos]
    print("worst relative difference", rel.max(), "over", pos.sum())
    assert pos.sum() > 2900
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=0.0)


def test_special_cases():
    # mean 0 (no flow, or a reporting ratio of 0): a point mass at 0, whatever the dispersion
    for k in (0.01, 2.0, 1e6):
        assert nr.factor(0, 0, .5, k) == 1.0 and nr.factor(5, 0, .5, k) == 0.0
        assert nr.factor(0, 31, 0.0, k) == 1.0 and nr.factor(1, 31, 0.0, k) == 0.0
    # a report above the particle's flow is possible, a ratio above 1 is a mean like any other
    assert 0.0 < nr.factor(40, 3, .5, 2) < nr.factor(4, 3, .5, 2)
    assert nr.factor(30, 20, 1.5, 2) > nr.factor(30, 20, 0.5, 2) > 0.0   # mean 30 against mean 10
    # y = 0: (kappa / (kappa + m))^kappa, c exactly 0
    assert nr.coefficient(0, 2.0) == 0.0
    assert nr.factor(0, 31, .5, 2) == pytest.approx((2 / 17.5) ** 2, rel=1e-15)
    # the factors sum to 1 over y, and their mean and variance are m and m + m^2 / kappa
    ys = np.arange(0, 4000)
    f = np.array([nr.factor(v, 30, .5, 2) for v in ys])
    assert f.sum() == pytest.approx(1.0, abs=1e-9)
    assert (f * ys).sum() == pytest.approx(15.0, rel=1e-6)
    assert (f * (ys - 15.0) ** 2).sum() == pytest.approx(15.0 + 15.0 ** 2 / 2, rel=1e-4)
    # the product over columns skips the unreported ones
    acc = np.array([[31, 96], [0, 5]])
    w = nr.weights(np.array([39.0, np.nan]), acc, .5, 2)
    assert w.tolist() == [nr.factor(39, 31, .5, 2), 0.0]
    w = nr.weights(np.array([0.0, 3.0]), acc, .5, 2)
    assert w.tolist() == [1.0 * nr.factor(0, 31, .5, 2) * nr.factor(3, 96, .5, 2), 1.0 * 1.0 * nr.factor(3, 5, .5, 2)]


def test_the_restatement_leaves_the_binomial_pass_as_it_was():
    saved = ir.weights
    with nr.negbin_weights(2.0):
        assert ir.weights is not saved
    assert ir.weights is saved
    nan = np.full((3, 2), np.nan)                         # nothing reported: both models weigh 1 everywhere
    a = nr.one_pass(nan, "sir", (0.8, 0.3), .5, 2.0, 9, nc.NPOP, nc.MU, 4, 1)
    b = ir.one_pass(nan, "sir", (0.8, 0.3), False, .5, 9, nc.NPOP, nc.MU, 4, 1)
    for k in ("hidden", "ancestry", "log_zetas"):
        assert np.array_equal(a[k], b[k]), k


# loglik at N = 65, D = 12, key 11, filter index 3, population 300, mu 5, rho 0.5, kappa 2: the prototype's figures,
# which this restatement reproduces to every digit given
CASES = [("sir", (0,), -41.9494), ("sir", (1,), -36.0491), ("sir", (0, 1), -78.4820), ("seir", (0,), -31.8651),
         ("seir", (1,), -32.0416), ("seir", (2,), -26.0071), ("seir", (0, 1, 2), -89.1264)]


@pytest.mark.parametrize("model,cols,ll", CASES)
def test_daily_cases(model, cols, ll):
    r = nc.restate(nc.daily(model, cols), model, nc.THETA[model])
    assert r["status"] == 0 and r["log_zetas"][1] == 0.0
    assert r["log_zetas"][-1] == pytest.approx(ll, abs=5e-5)


def test_three_day_totals_with_and_without_cumulate():
    """Unlike the binomial pass (test_incidence_restatement.py), a day can hold three days' cases: without cumulate the
    pass survives, 15.8 log units worse."""
    c = nc.fixture()["over_threeday"]
    assert np.isnan(c).sum() == 16 and c[2::3].tolist() == [[2, 10], [46, 8], [79, 27], [62, 14]]
    a = nc.restate(c, "sir", (0.8, 0.3), cumulate=True)
    b = nc.restate(c, "sir", (0.8, 0.3), cumulate=False)
    assert a["status"] == b["status"] == 0
    assert a["log_zetas"][-1] == pytest.approx(-34.0447, abs=5e-5)
    assert b["log_zetas"][-1] == pytest.approx(-49.8823, abs=5e-5)
    assert nc.restate(nc.mixed(), "sir", (0.8, 0.3), cumulate=True)["status"] == 0


def test_the_batch():
    got = [nc.restate(nc.daily("sir", (0, 1)), "sir", th, pr, k, key=key) for th, pr, k, key in nc.BATCH]
    assert [r["step"] for r in got] == [None, 3, None]
    assert got[0]["log_zetas"][-1] == pytest.approx(-78.482, abs=5e-4)
    assert got[2]["log_zetas"][-1] == pytest.approx(-138.1835, abs=5e-5)
    over = nc.fixture()["over"]
    assert over[0].tolist() == [0, 0] and over[1].tolist() == [2, 3]       # why the second dies at step 3
    assert got[1]["log_zetas"][2] == 0.0 and np.isneginf(got[1]["log_zetas"][3:]).all()


def test_fixture_values():
    fx = nc.fixture()
    assert fx["over"].shape == (24, 2) and fx["over_seir"].shape == (24, 3) and fx["over_threeday"].shape == (12, 2)
    assert fx["over"][:, 0].tolist() == [0, 2, 6, 14, 1, 26, 39, 39, 9, 8, 10, 13, 14, 1, 2, 1, 3, 0, 0, 0, 0, 2, 0, 0]
    assert fx["over"][:, 1].tolist() == [0, 3, 7, 2, 2, 1, 0, 22, 4, 1, 36, 10, 1, 10, 4, 5, 7, 2, 2, 4, 1, 1, 3, 4]
    assert fx["over_seir"][:8, 0].tolist() == [1, 3, 6, 0, 2, 6, 10, 11]
    flows = ic.fixture()["sir_flows"]
    assert (fx["over"][:, 0] > flows[:, 0]).any()          # reports above the true flow: impossible under thinning


# ------------------------------------------------------------------------------------------------- does it work
# infections alone on all 24 days of `over`, N = 200, population 300, mu 5, probs 0.5, filter index 0, keys 1..4: loglik
# under NB at kappa = 2 / at theta (0.4, 0.3) / at kappa = 0.5, 10, 1000 (DESIGN.md §21's table)
TABLE = {
    "nb2": (-60.18, -59.66, -59.07, -59.33),
    "low": (-77.79, -73.78, -73.95, -73.51),
    0.5: (-63.20, -62.91, -62.81, -63.03),                # key 2: -62.9146 here; the prototype's table printed -62.92
    10.0: (-65.06, -63.61, -63.53, -63.53),
    1000.0: (-75.91, -75.22, -73.99, -74.57),
}
BINOMIAL = {1: 14, 2: 14, 3: -95.15, 4: -98.71}           # the dying step, or the loglik


@pytest.fixture(scope="module")
def table():
    c = nc.daily("sir", (0,), days=24)
    out = {k: [] for k in TABLE}
    for key in (1, 2, 3, 4):
        out["nb2"].append(nr.loglik(nc.restate(c, "sir", (0.8, 0.3), n=200, key=key, f=0)))
        out["low"].append(nr.loglik(nc.restate(c, "sir", (0.4, 0.3), n=200, key=key, f=0)))
        for k in (0.5, 10.0, 1000.0):
            out[k].append(nr.loglik(nc.restate(c, "sir", (0.8, 0.3), kappa=k, n=200, key=key, f=0)))
    print("table", out)
    return {k: np.array(v) for k, v in out.items()}


def test_does_it_work_the_table(table):
    for k, want in TABLE.items():
        np.testing.assert_allclose(table[k], want, atol=5e-3, err_msg=str(k))


def test_does_it_work_the_claims(table):
    """Half the smallest gap of the table per claim."""
    assert np.isfinite(table["nb2"]).all()
    assert (table["nb2"] - table["low"]).min() > 7.0       # the true theta against half the infection rate
    assert (table["nb2"] - table[0.5]).min() > 1.5         # the dispersion is identified: 2 against 0.5,
    assert (table["nb2"] - table[10.0]).min() > 1.9        # against 10
    assert (table["nb2"] - table[1000.0]).min() > 7.4      # and against the near-Poisson 1000


@pytest.mark.parametrize("key", [1, 2, 3, 4])
def test_the_binomial_pass_fails_on_overdispersed_reports(key):
    """Thinning at the true parameters dies at step 14 for keys 1 and 2 and loses 35 log units for the others."""
    r = ic.restate(nc.daily("sir", (0,), days=24), "sir", (0.8, 0.3), False, 0.5, n=200, key=key, f=0)
    if BINOMIAL[key] == 14:
        assert r["status"] == ir.DEGENERATE and r["step"] == 14
    else:
        assert r["status"] == 0 and r["log_zetas"][-1] == pytest.approx(BINOMIAL[key], abs=5e-3)
        assert r["log_zetas"][-1] < max(TABLE["nb2"]) - 35.0

