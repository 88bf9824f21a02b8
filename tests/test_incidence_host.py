"""epipf.incidence's host logic over an oracle-backed engine double (tests/incidence_oracle_engine.py): the flows mapping,
shapes, per-chain theta / probs, key and filter-index bookkeeping, every refusal before any device call, and
incidence_mcmc's draw order, filter-index use, probs=None and the pinned seed of the device comparison.  No GPU."""
import re

import numpy as np
import pytest

import epipf
import incidence_cases as ic
import incidence_oracle_engine as ioe
from conftest import REPO
from epipf import _lib, incidence, pmcmc


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(incidence._engine, "get_engine", ioe.fake_get_engine)
    ioe.ENGINES.clear()
    return ioe.ENGINES


def sir_cases(days=6):
    return ic.fixture()["sir"][:days]


def test_flows_map_into_the_models_columns(fake):
    c = sir_cases()
    epipf.seed_stream(77, 5)
    res = epipf.incidence_filter(c[:, 1], "sir", [0.8, 0.3], flows=("removals",), n_particles=12, n_population=300, mu=5)
    call = fake[0].calls[0]
    assert call["counts"].shape == (6, 2) and np.isnan(call["counts"][:, 0]).all()
    np.testing.assert_array_equal(call["counts"][:, 1], c[:, 1])
    assert call["keys"].tolist() == [77] and call["f"].tolist() == [5] and pmcmc._STREAM.next_filter == 6
    assert not call["cumulate"] and not call["observations"] and call["probs"].tolist() == [0.5]
    assert res.log_zetas.shape == (1, 8) and res.loglik.shape == (1,) and res.status.tolist() == [0]
    assert res.loglik[0] == res.log_zetas[0, -1] and res.best == 0 and res.states is None
    hid, anc = res.history()
    assert hid.shape == (1, 8, 12, 3) and anc.shape == (1, 8, 12)
    # both columns in another order, a string for one flow, SEIR's names and its alias
    epipf.incidence_filter(c[:, ::-1], "sir", [0.8, 0.3], flows=("removals", "infections"), n_particles=4,
                           n_population=300, mu=5)
    np.testing.assert_array_equal(fake[1].calls[0]["counts"], c)
    epipf.incidence_filter(c[:, 0], "sir", [0.8, 0.3], flows="infections", n_particles=4, n_population=300, mu=5)
    np.testing.assert_array_equal(fake[2].calls[0]["counts"][:, 0], c[:, 0])
    s = ic.fixture()["seir"][:4]
    epipf.incidence_filter(s[:, [2, 0]], "seir", [0.9, 0.6, 0.3], flows=("removals", "infections"), n_particles=4,
                           n_population=300, mu=5)
    got = fake[3].calls[0]["counts"]
    assert got.shape == (4, 3) and np.isnan(got[:, 1]).all()
    np.testing.assert_array_equal(got[:, [0, 2]], s[:, [0, 2]])
    epipf.incidence_filter(s[:, 1], "seir", [0.9, 0.6, 0.3], flows=("onsets",), n_particles=4, n_population=300, mu=5)
    np.testing.assert_array_equal(fake[4].calls[0]["counts"][:, 1], s[:, 1])


def test_per_chain_theta_probs_keys_and_smoothing(fake):
    c = sir_cases()
    th = [[0.8, 0.3], [0.05, 0.3], [1.6, 0.3]]
    res = epipf.incidence_filter(c, "sir", th, flows=("infections", "removals"), probs=[0.5, 0.4, 0.6], n_particles=24,
                                 n_population=300, mu=5, cumulate=True, key=9, filter_index=3, quantiles=(0.5,), lag=2)
    call = fake[0].calls[0]
    np.testing.assert_array_equal(call["thetas"], th)
    assert call["probs"].tolist() == [0.5, 0.4, 0.6] and call["cumulate"] and call["f"].tolist() == [3, 3, 3]
    assert call["keys"].tolist() == [epipf.chain_key(9, s) for s in range(3)]
    assert res.status.tolist() == [0, 1, 0] and np.isneginf(res.loglik[1])
    assert res.best == int(np.argmax(np.where(res.status == 0, res.log_zetas[:, -1], -np.inf))) and res.best != 1
    assert res.states == ("states", 3, "genealogy", 2)
    assert fake[0].smooth_calls == [dict(n=3, quantiles=(0.5,), lineage="genealogy", kind="smoothing", lag=2)]
    res = epipf.incidence_filter(c, "sir", th[:2], flows=("infections", "removals"), keys=[4, 5], filter_index=[1, 2],
                                 n_particles=4, n_population=300, mu=5, observations=True, probs=0.2)
    call = fake[1].calls[0]
    assert call["keys"].tolist() == [4, 5] and call["f"].tolist() == [1, 2] and call["observations"]
    r = incidence.IncidenceResult(np.full((2, 4), -np.inf), np.array([1, 1], dtype=np.int32), None, None)
    assert r.best is None and np.isneginf(r.loglik).all()


BAD_FILTER = [
    dict(thetas=[0.8]), dict(thetas=[0.8, 0.3, 0.1]), dict(thetas=[-0.1, 0.3]), dict(thetas=[np.nan, 0.3]),
    dict(thetas=np.ones((2, 2, 2))), dict(flows=("cases",)), dict(flows=()), dict(flows=("infections", "infections")),
    dict(flows=("exposures",)), dict(flows=("infections", "removals")), dict(cases=np.ones((6, 2))),
    dict(cases=np.ones((0,))), dict(cases=[1.0, -1.0]), dict(cases=[1.0, np.inf]), dict(cases=[1.5, 2.0]),
    dict(probs=1.5), dict(probs=-0.1), dict(probs=np.nan), dict(probs=[0.5, 0.5]), dict(n_particles=0),
    dict(keys=[1, 2]), dict(quantiles=(1.2,)), dict(quantiles=(0.5,), lag=-1), dict(quantiles=(0.5,), lineage="tree")]


@pytest.mark.parametrize("kw", BAD_FILTER)
def test_filter_refusals_come_before_any_device_call(monkeypatch, kw):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(incidence._engine, "get_engine", no_engine)
    args = dict(cases=sir_cases()[:, 0], thetas=[0.8, 0.3], flows=("infections",), n_particles=8, n_population=300, mu=5)
    args.update(kw)
    cases, thetas = args.pop("cases"), args.pop("thetas")
    with pytest.raises(ValueError):
        epipf.incidence_filter(cases, "sir", thetas, **args)


def test_normal_reports_need_not_be_integers_and_probs_may_exceed_one(fake):
    epipf.incidence_filter([1.5, 2.0], "sir", [0.8, 0.3], observations=True, probs=1.5, n_particles=4, n_population=300,
                           mu=5)
    assert fake[0].calls[0]["counts"][:, 0].tolist() == [1.5, 2.0]


@pytest.mark.parametrize("model", ["sir_subgroups", "sir_subgroups2"])
def test_subgroup_models_are_refused_before_any_device_call(monkeypatch, model):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(incidence._engine, "get_engine", no_engine)
    with pytest.raises(ValueError, match="SIR and SEIR"):
        epipf.incidence_filter(np.zeros(4), model, [0.5] * 5)
    with pytest.raises(ValueError, match="SIR and SEIR"):
        epipf.incidence_mcmc(np.zeros(4), model, [0.5] * 5, 0.1)


BAD_MCMC = [
    dict(parameters=[0.8]), dict(parameters=np.ones((3, 2))), dict(parameters=[-0.8, 0.3]), dict(h=0.0), dict(h=np.nan),
    dict(sigma=np.eye(3)), dict(iters=0), dict(chains=0), dict(n_particles=0), dict(probs=[0.5, 0.5]), dict(probs=2.0),
    dict(probs=None), dict(probs=None, parameters=[0.8, 0.3, 1.5]), dict(keys=[1]), dict(rngs=[np.random.RandomState(0)]),
    dict(flows=("onsets",))]


@pytest.mark.parametrize("kw", BAD_MCMC)
def test_mcmc_refusals_come_before_any_device_call(monkeypatch, kw):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(incidence._engine, "get_engine", no_engine)
    args = dict(parameters=[0.8, 0.3], h=0.1, chains=2, n_particles=8, n_population=300, mu=5, iters=3)
    args.update(kw)
    parameters, h = args.pop("parameters"), args.pop("h")
    with pytest.raises(ValueError):
        epipf.incidence_mcmc(sir_cases()[:, 0], "sir", parameters, h, **args)


def test_mcmc_refuses_a_start_that_degenerates(fake):
    with pytest.raises(ValueError, match="chain 1"):
        epipf.incidence_mcmc(sir_cases(), "sir", [[0.8, 0.3], [0.05, 0.3]], 0.1, flows=("infections", "removals"),
                             chains=2, n_particles=24, n_population=300, mu=5, iters=2, seed=11)


class Recorder:
    """A RandomState behind a log of the calls made on it (not a RandomState: legacy_randint falls back to randint)."""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def standard_normal(self, d):
        self.log.append("normal%d" % d)
        return self.rs.standard_normal(d)

    def random_sample(self):
        self.log.append("uniform")
        return self.rs.random_sample()

    def randint(self, lo, hi):
        self.log.append("randint")
        return self.rs.randint(lo, hi)


def test_mcmc_draw_order_and_filter_indices(fake):
    """Per iteration and chain: the proposal's normals, then one uniform, whatever happens; one randint more exactly
    where the proposal is accepted.  Invalid proposals run no filter and consume no filter index."""
    rngs = [Recorder(3), Recorder(4)]
    c = sir_cases(8)
    res = epipf.incidence_mcmc(c, "sir", [0.8, 0.3], 0.08, flows=("infections", "removals"), chains=2, n_particles=16,
                               n_population=300, mu=5, iters=25, rngs=rngs, keys=[21, 22], filter_index_start=100)
    eng = fake[0]
    first, later = eng.calls[0], eng.calls[1:]
    assert first["active"].tolist() == [1, 1] and first["f"].tolist() == [100, 100] and first["keys"].tolist() == [21, 22]
    n_valid = np.zeros(2, dtype=int)
    n_invalid = 0
    for ch, (r, rec) in enumerate(zip(res, rngs)):
        assert rec.log[0] == "randint"                                   # iteration 0: the trajectory pick alone
        log, pos, call = rec.log[1:], 0, 0
        fnext = 101
        for i in range(1, 25):
            assert log[pos:pos + 2] == ["normal2", "uniform"], (ch, i)
            pos += 2
            changed = not np.array_equal(r.thetas[i], r.thetas[i - 1])
            if changed:
                assert log[pos] == "randint"
                pos += 1
                assert (r.thetas[i] >= 0).all()
            else:
                assert np.array_equal(r.sampled_trajs[:, i], r.sampled_trajs[:, i - 1])
                assert r.log_likelihoods[i] == r.log_likelihoods[i - 1]
        assert pos == len(log)
        assert r.acceptances == sum(not np.array_equal(r.thetas[i], r.thetas[i - 1]) for i in range(1, 25))
        # this chain's filter indices: consecutive over the calls in which it was active
        used = [int(k["f"][ch]) for k in later if k["active"][ch]]
        assert used == list(range(101, 101 + len(used))) and r.filters_run == 1 + len(used)
        n_valid[ch] = len(used)
        # the stream position after the run is that of the replay: normals and a uniform per iteration, a pick per
        # acceptance, nothing for an invalid proposal or a rejected one
        rs = np.random.RandomState(3 + ch)
        rs.randint(0, 16)
        for i in range(1, 25):
            z = rs.standard_normal(2)
            prop = pmcmc.mvn_apply(z, pmcmc.mvn_factor(0.08 * np.eye(2)), r.thetas[i - 1])
            rs.random_sample()
            n_invalid += bool((prop < 0).any())
            if not np.array_equal(r.thetas[i], r.thetas[i - 1]):
                np.testing.assert_array_equal(prop, r.thetas[i])
                rs.randint(0, 16)
        assert rs.random_sample() == rec.rs.random_sample()
    assert n_invalid > 0 and (n_valid < 24).any() and (n_valid > 0).all()   # both kinds of proposal occurred
    assert all(k["active"].any() for k in later)                             # no call without an active chain
    assert res[0].sampled_trajs.shape == (10, 25, 3) and res[0].thetas.shape == (25, 2)


def test_mcmc_probs_none_estimates_the_reporting_probability(fake):
    c = sir_cases(8)
    res = epipf.incidence_mcmc(c[:, 0], "sir", [0.8, 0.3, 0.9], 0.02, probs=None, chains=1, n_particles=16,
                               n_population=300, mu=5, iters=30, seed=2)
    eng = fake[0]
    assert eng.calls[0]["thetas"].tolist() == [[0.8, 0.3]] and eng.calls[0]["probs"].tolist() == [0.9]
    rs = np.random.RandomState(2)
    rs.randint(0, 16)
    fac = pmcmc.mvn_factor(0.02 * np.eye(3))
    k, over = 1, 0
    for i in range(1, 30):
        prop = pmcmc.mvn_apply(rs.standard_normal(3), fac, res[0].thetas[i - 1])
        rs.random_sample()
        valid = not (prop < 0).any() and 0.0 <= prop[2] <= 1.0
        over += bool(prop[2] > 1.0 and not (prop < 0).any())
        if valid:
            call = eng.calls[k]
            k += 1
            np.testing.assert_array_equal(call["thetas"][0], prop[:2])
            assert call["probs"][0] == prop[2] and call["f"][0] == k - 1
        if not np.array_equal(res[0].thetas[i], res[0].thetas[i - 1]):
            assert valid
            rs.randint(0, 16)
    assert k == len(eng.calls) and over > 0                # a reporting probability above 1 was proposed and refused
    assert res[0].thetas.shape == (30, 3) and res[0].filters_run == k


def test_the_pinned_seed_keeps_every_decision_away_from_the_boundary(fake):
    """A condition on the input of the device comparison (tests/test_gpu_incidence.py): at ic.MCMC's seed every MH
    decision has |log u - (lz_new - lz_old)| > 1e-6, and both outcomes and an invalid proposal occur."""
    res = ic.mcmc_run()
    eng = fake[0]
    nc, iters = ic.MCMC["chains"], ic.MCMC["iters"]
    fac = pmcmc.mvn_factor(ic.MCMC["h"] * np.eye(2))
    lz_of = {}                                             # (chain, filter index) -> (status, loglik) of its filter
    for call in list(eng.calls):                           # (the double records the replays too)
        lz, st = eng.run_incidence(call["thetas"], call["probs"], call["keys"], call["f"], call["counts"],
                                   active=call["active"])
        for c in range(nc):
            if call["active"][c]:
                lz_of[(c, int(call["f"][c]))] = (int(st[c]), float(lz[c, -1]))
    decisions = accepted = invalid = 0
    for c in range(nc):
        rs = np.random.RandomState(ic.MCMC["seed"] + c)
        rs.randint(0, ic.N)
        f = ic.MCMC["filter_index_start"] + 1
        for i in range(1, iters):
            prop = pmcmc.mvn_apply(rs.standard_normal(2), fac, res[c].thetas[i - 1])
            u = rs.random_sample()
            took = not np.array_equal(res[c].thetas[i], res[c].thetas[i - 1])
            if (prop < 0).any():
                invalid += 1
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
                rs.randint(0, ic.N)
    assert decisions >= 20 and 0 < accepted < decisions and invalid > 0, (decisions, accepted, invalid)


def test_the_names_are_public_and_the_entry_point_is_declared():
    assert {"incidence_filter", "incidence_mcmc", "IncidenceResult"} <= set(epipf.__all__)
    assert "epipf_run_incidence" in _lib.EXPORTS and not re.search(r"\d", "epipf_run_incidence")
    header = open(REPO + "/include/epipf.h").read()
    assert re.search(r"\bepipf_run_incidence\s*\(", header)
    assert _lib.ABI_VERSION == 9 and "#define EPIPF_ABI_VERSION 9" in header
