"""The `dispersion` option of epipf.incidence and epipf.walk_incidence over engine doubles: shapes and broadcasting, every
refusal before a device call, incidence_mcmc's draw order, filter-index use and invalid-dispersion rule with
dispersion="estimate", that dispersion=None passes no keyword (the existing doubles run unchanged), the pinned seed of
the device comparison, and the public names.  No GPU."""
import re

import numpy as np
import pytest

import epipf
import incidence_cases as ic
import incidence_oracle_engine as ioe
import negbin_cases as nc
import negbin_oracle_engine as noe
from conftest import REPO
from epipf import _lib, incidence, pmcmc, walk_incidence
from test_incidence_host import Recorder


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(incidence._engine, "get_engine", noe.fake_get_engine)
    noe.ENGINES.clear()
    return noe.ENGINES


def over(days=6):
    return nc.fixture()["over"][:days]


def test_dispersion_shapes_and_broadcasting(fake):
    c = over()
    res = epipf.incidence_filter(c[:, 0], "sir", [0.8, 0.3], dispersion=2, probs=1.25, n_particles=12, n_population=300,
                                 mu=5, key=7, filter_index=1)
    call = fake[0].calls[0]
    assert call["dispersion"].tolist() == [2.0] and call["dispersion"].dtype == np.float64
    assert call["probs"].tolist() == [1.25] and not call["observations"]   # a mean ratio: above 1 is fine
    assert res.status.tolist() == [0] and res.log_zetas.shape == (1, 8)
    th = [[0.8, 0.3], [0.4, 0.3], [1.6, 0.3]]
    epipf.incidence_filter(c, "sir", th, flows=("infections", "removals"), dispersion=2.0, n_particles=8,
                           n_population=300, mu=5, key=7, filter_index=1)
    assert fake[1].calls[0]["dispersion"].tolist() == [2.0, 2.0, 2.0]
    res = epipf.incidence_filter(c, "sir", th, flows=("infections", "removals"), dispersion=[2.0, 0.5, 1e6],
                                 probs=[0.5, 0.0, 0.6], n_particles=24, n_population=300, mu=5, key=7, filter_index=1,
                                 cumulate=True)
    call = fake[2].calls[0]
    assert call["dispersion"].tolist() == [2.0, 0.5, 1e6] and call["probs"].tolist() == [0.5, 0.0, 0.6]
    assert call["cumulate"] and res.status.tolist() == [0, 1, 0]           # a mean of 0 against a report of 2
    # each chain is weighed under its own dispersion
    one = epipf.incidence_filter(c, "sir", th[2], flows=("infections", "removals"), dispersion=1e6, probs=0.6,
                                 n_particles=24, n_population=300, mu=5, keys=[epipf.chain_key(7, 2)], filter_index=1,
                                 cumulate=True)
    assert one.loglik[0] == res.loglik[2]
    two = epipf.incidence_filter(c, "sir", th[2], flows=("infections", "removals"), dispersion=2.0, probs=0.6,
                                 n_particles=24, n_population=300, mu=5, keys=[epipf.chain_key(7, 2)], filter_index=1,
                                 cumulate=True)
    assert two.loglik[0] != res.loglik[2]


def test_dispersion_none_passes_no_keyword(monkeypatch):
    """The existing doubles do not take the keyword: they run unchanged."""
    monkeypatch.setattr(incidence._engine, "get_engine", ioe.fake_get_engine)
    ioe.ENGINES.clear()
    c = over()
    epipf.incidence_filter(c[:, 0], "sir", [0.8, 0.3], n_particles=8, n_population=300, mu=5)
    epipf.incidence_filter(c[:, 0], "sir", [0.8, 0.3], n_particles=8, n_population=300, mu=5, dispersion=None)
    epipf.incidence_mcmc(ic.daily("sir", False, (0, 1), days=4), "sir", [0.8, 0.3], 0.05,
                         flows=("infections", "removals"), n_particles=8, n_population=300, mu=5, iters=3,
                         dispersion=None)                  # (thinned reports: the binomial pass survives them)
    assert len(ioe.ENGINES) == 3 and all(e.calls for e in ioe.ENGINES)
    with pytest.raises(TypeError, match="dispersion"):
        epipf.incidence_filter(c[:, 0], "sir", [0.8, 0.3], n_particles=8, n_population=300, mu=5, dispersion=2.0)

    class Walk:                                            # walk_incidence_filter: the keyword only with a dispersion
        def __init__(self):
            self.kw = []

        def set_population(self, *a):
            pass

        def walk_incidence(self, *a, **kw):
            self.kw.append(kw)
            raise StopIteration

    w = Walk()
    monkeypatch.setattr(walk_incidence._engine, "get_engine", lambda *a, **k: w)
    for extra in ({}, {"dispersion": None}, {"dispersion": [2.0, 3.0]}):
        with pytest.raises(StopIteration):
            epipf.walk_incidence_filter(c[:, 0], "sir", [0.8, 0.3], [0.1, 0.0], n_particles=4, n_population=300, mu=5,
                                        chains=2, probs=1.5 if extra.get("dispersion") else 0.5, **extra)
    assert "dispersion" not in w.kw[0] and "dispersion" not in w.kw[1]
    assert w.kw[2]["dispersion"].tolist() == [2.0, 3.0]


BAD_FILTER = [
    dict(dispersion=0.0), dict(dispersion=-1.0), dict(dispersion=np.nan), dict(dispersion=np.inf),
    dict(dispersion=1.0000001e6), dict(dispersion=[2.0, 2.0]), dict(dispersion=np.ones((1, 1))),
    dict(dispersion=2.0, observations=True), dict(dispersion=2.0, probs=-0.1), dict(dispersion=2.0, probs=np.nan),
    dict(dispersion=2.0, probs=np.inf), dict(dispersion=2.0, cases=[1.5, 2.0]), dict(dispersion=2.0, cases=[1.0, -1.0])]


@pytest.mark.parametrize("kw", BAD_FILTER)
def test_filter_refusals_come_before_any_device_call(monkeypatch, kw):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(incidence._engine, "get_engine", no_engine)
    monkeypatch.setattr(walk_incidence._engine, "get_engine", no_engine)
    args = dict(cases=over()[:, 0], flows=("infections",), n_particles=8, n_population=300, mu=5)
    args.update(kw)
    cases = args.pop("cases")
    with pytest.raises(ValueError):
        epipf.incidence_filter(cases, "sir", [0.8, 0.3], **args)
    with pytest.raises(ValueError):
        epipf.walk_incidence_filter(cases, "sir", [0.8, 0.3], [0.1, 0.0], **args)


def test_the_poisson_limit_is_refused_with_a_text_that_says_so():
    with pytest.raises(ValueError, match="Poisson limit.*out of scope"):
        epipf.incidence_filter(over()[:, 0], "sir", [0.8, 0.3], dispersion=2e6)


BAD_MCMC = [
    dict(dispersion="fit"), dict(dispersion=[2.0, 2.0]), dict(dispersion=0.0), dict(dispersion=2e6),
    dict(dispersion=2.0, observations=True), dict(dispersion="estimate", observations=True),
    dict(dispersion="estimate"),                                              # parameters lack the dispersion
    dict(dispersion="estimate", parameters=[0.8, 0.3, 0.0]), dict(dispersion="estimate", parameters=[0.8, 0.3, 2e6]),
    dict(dispersion="estimate", probs=None, parameters=[0.8, 0.3, 2.0]),      # ... and the reporting ratio
    dict(dispersion="estimate", probs=None, parameters=[0.8, 0.3, -0.5, 2.0]),
    dict(dispersion=2.0, probs=-0.5), dict(dispersion=2.0, probs=None, parameters=[0.8, 0.3])]


@pytest.mark.parametrize("kw", BAD_MCMC)
def test_mcmc_refusals_come_before_any_device_call(monkeypatch, kw):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(incidence._engine, "get_engine", no_engine)
    args = dict(parameters=[0.8, 0.3], h=0.1, chains=2, n_particles=8, n_population=300, mu=5, iters=3)
    args.update(kw)
    parameters, h = args.pop("parameters"), args.pop("h")
    with pytest.raises(ValueError):
        epipf.incidence_mcmc(over()[:, 0], "sir", parameters, h, **args)


def test_mcmc_with_a_fixed_dispersion_passes_it_on_every_call_and_takes_a_ratio_above_one(fake):
    res = epipf.incidence_mcmc(over(8)[:, 0], "sir", [0.8, 0.3, 1.05], 0.02, probs=None, dispersion=2.0, chains=1,
                               n_particles=16, n_population=300, mu=5, iters=30, seed=2)
    eng = fake[0]
    assert all(c["dispersion"].tolist() == [2.0] for c in eng.calls)
    rs = np.random.RandomState(2)
    rs.randint(0, 16)
    fac = pmcmc.mvn_factor(0.02 * np.eye(3))
    k, above = 1, 0
    for i in range(1, 30):
        prop = pmcmc.mvn_apply(rs.standard_normal(3), fac, res[0].thetas[i - 1])
        rs.random_sample()
        valid = not (prop < 0).any()                                          # no upper bound on the ratio
        if valid:
            call = eng.calls[k]
            k += 1
            above += bool(prop[2] > 1.0)
            assert call["probs"][0] == prop[2] and call["f"][0] == k - 1
        if not np.array_equal(res[0].thetas[i], res[0].thetas[i - 1]):
            assert valid
            rs.randint(0, 16)
    assert k == len(eng.calls) and above > 0               # a ratio above 1 was proposed and filtered


def test_mcmc_estimate_draw_order_filter_indices_and_the_invalid_dispersion_rule(fake):
    """Per iteration and chain: the proposal's normals (one more for the dispersion), then one uniform, whatever
    happens; one randint more exactly where the proposal is accepted.  A proposal whose dispersion is <= 0 or > 1e6 is
    invalid as a negative rate is: no filter, no filter index, the same host draws."""
    rngs = [Recorder(3), Recorder(4)]
    sigma = np.diag([1.0, 1.0, 200.0])
    iters = 25
    res = epipf.incidence_mcmc(over(8), "sir", [[0.8, 0.3, 2.0], [0.8, 0.3, 999998.0]], 0.05, sigma=sigma,
                               flows=("infections", "removals"), chains=2, n_particles=16, n_population=300, mu=5,
                               iters=iters, rngs=rngs, keys=[21, 22], filter_index_start=100, dispersion="estimate")
    eng = fake[0]
    first, later = eng.calls[0], eng.calls[1:]
    assert first["active"].tolist() == [1, 1] and first["f"].tolist() == [100, 100]
    assert first["thetas"].tolist() == [[0.8, 0.3], [0.8, 0.3]] and first["dispersion"].tolist() == [2.0, 999998.0]
    assert first["probs"].tolist() == [0.5, 0.5]
    fac = pmcmc.mvn_factor(0.05 * sigma)
    low = high = 0
    for ch, (r, rec) in enumerate(zip(res, rngs)):
        assert rec.log[0] == "randint" and r.thetas.shape == (iters, 3)
        log, pos = rec.log[1:], 0
        for i in range(1, iters):
            assert log[pos:pos + 2] == ["normal3", "uniform"], (ch, i)
            pos += 2
            if not np.array_equal(r.thetas[i], r.thetas[i - 1]):
                assert log[pos] == "randint"
                pos += 1
                assert (r.thetas[i] >= 0).all() and 0.0 < r.thetas[i, 2] <= 1e6
        assert pos == len(log)
        used = [k for k in later if k["active"][ch]]
        assert [int(k["f"][ch]) for k in used] == list(range(101, 101 + len(used))) and r.filters_run == 1 + len(used)
        # the replay: which proposals were valid, and that exactly those were filtered, with their dispersion
        rs = np.random.RandomState(3 + ch)
        rs.randint(0, 16)
        n = 0
        for i in range(1, iters):
            prop = pmcmc.mvn_apply(rs.standard_normal(3), fac, r.thetas[i - 1])
            rs.random_sample()
            valid = not (prop < 0).any() and 0.0 < prop[2] <= 1e6
            low += bool(prop[2] <= 0 and (prop[:2] >= 0).all())
            high += bool(prop[2] > 1e6 and (prop[:2] >= 0).all())
            took = not np.array_equal(r.thetas[i], r.thetas[i - 1])
            if valid:
                np.testing.assert_array_equal(used[n]["thetas"][ch], prop[:2])
                assert used[n]["dispersion"][ch] == prop[2]
                n += 1
            else:
                assert not took
            if took:
                np.testing.assert_array_equal(prop, r.thetas[i])
                rs.randint(0, 16)
        assert n == len(used)
        assert rs.random_sample() == rec.rs.random_sample()
    assert low > 0 and high > 0, (low, high)               # both ends of (0, 1e6] were crossed
    assert all(k["active"].any() for k in later)
    # an inactive chain's dispersion in the call is its current, valid one
    for k in later:
        assert ((k["dispersion"] > 0) & (k["dispersion"] <= 1e6)).all()


def test_mcmc_estimates_the_ratio_and_the_dispersion_in_that_order(fake):
    res = epipf.incidence_mcmc(over(6)[:, 0], "sir", [0.8, 0.3, 1.2, 3.0], 0.01, probs=None, dispersion="estimate",
                               n_particles=8, n_population=300, mu=5, iters=4, seed=1)
    call = fake[0].calls[0]
    assert call["thetas"].tolist() == [[0.8, 0.3]] and call["probs"].tolist() == [1.2]
    assert call["dispersion"].tolist() == [3.0] and res[0].thetas.shape == (4, 4)


def test_the_pinned_seed_keeps_every_decision_away_from_the_boundary(fake):
    """A condition on the input of the device comparison (tests/test_gpu_negbin.py): at nc.MCMC's seed every MH decision
    has |log u - (lz_new - lz_old)| > 1e-6, and both outcomes and an invalid dispersion occur."""
    res = nc.mcmc_run()
    eng = fake[0]
    nch, iters = nc.MCMC["chains"], nc.MCMC["iters"]
    fac = pmcmc.mvn_factor(nc.MCMC["h"] * nc.MCMC_SIGMA)
    lz_of = {}                                             # (chain, filter index) -> (status, loglik) of its filter
    for call in list(eng.calls):                           # (the double records the replays too)
        lz, st = eng.run_incidence(call["thetas"], call["probs"], call["keys"], call["f"], call["counts"],
                                   active=call["active"], dispersion=call["dispersion"])
        for c in range(nch):
            if call["active"][c]:
                lz_of[(c, int(call["f"][c]))] = (int(st[c]), float(lz[c, -1]))
    decisions = accepted = invalid_k = 0
    for c in range(nch):
        rs = np.random.RandomState(nc.MCMC["seed"] + c)
        rs.randint(0, nc.N)
        f = nc.MCMC["filter_index_start"] + 1
        for i in range(1, iters):
            prop = pmcmc.mvn_apply(rs.standard_normal(3), fac, res[c].thetas[i - 1])
            u = rs.random_sample()
            took = not np.array_equal(res[c].thetas[i], res[c].thetas[i - 1])
            if (prop < 0).any() or not (0.0 < prop[2] <= 1e6):
                invalid_k += bool((prop[:2] >= 0).all())
                assert not took
                continue
            st, lz_new = lz_of[(c, f)]
            f += 1
            if st != 0:
                assert not took
                continue
            margin = np.log(u) - (lz_new - res[c].log_likelihoods[i - 1])
            assert abs(margin) > 1e-6, (c, i, margin)
            assert took == (margin < 0)
            decisions += 1
            accepted += took
            if took:
                rs.randint(0, nc.N)
    assert decisions >= 15 and 0 < accepted < decisions and invalid_k > 0, (decisions, accepted, invalid_k)


def test_the_names_are_public_and_the_entry_points_are_declared():
    import inspect
    header = open(REPO + "/include/epipf.h").read()
    for n in ("epipf_run_incidence_negbin", "epipf_incidence_walk_negbin", "epipf_negbin_coefficients"):
        assert n in _lib.EXPORTS and not re.search(r"\d", n) and re.search(r"\b%s\s*\(" % n, header)
        assert not n.startswith("epipf_walk")
    assert _lib.ABI_VERSION == 9 and "#define EPIPF_ABI_VERSION 9" in header
    assert _lib.OBS_NEGBIN == 2 and "#define EPIPF_OBS_NEGBIN 2" in header
    for fn in (epipf.incidence_filter, epipf.incidence_mcmc, epipf.walk_incidence_filter):
        assert inspect.signature(fn).parameters["dispersion"].default is None
    from epipf.engine import Engine
    for fn in (Engine.run_incidence, Engine.walk_incidence):
        assert inspect.signature(fn).parameters["dispersion"].default is None
    L = _lib.load()
    assert all(hasattr(L, n) for n in ("epipf_run_incidence_negbin", "epipf_incidence_walk_negbin",
                                       "epipf_negbin_coefficients"))
