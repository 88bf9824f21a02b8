"""epipf.walk_incidence_filter's host logic over an oracle-backed engine double
(tests/walk_incidence_oracle_engine.py): shapes over the D + 2 rows, the flows mapping, key and filter-index
bookkeeping, broadcasting of start, rw and probs, .best beside a degenerate chain, `incidence` on both result classes,
and every refusal before any device call.  No GPU."""
import re

import numpy as np
import pytest

import epipf
import incidence_cases as ic
import walk_incidence_cases as wic
import walk_incidence_oracle_engine as wioe
from conftest import REPO
from epipf import _lib, incidence, pmcmc, walk_incidence


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(walk_incidence._engine, "get_engine", wioe.fake_get_engine)
    wioe.ENGINES.clear()
    return wioe.ENGINES


def sir_cases(days=6):
    return ic.fixture()["sir"][:days]


def run(cases, start, rw, flows=("infections", "removals"), N=12, **kw):
    return epipf.walk_incidence_filter(cases, "sir", start, rw, flows, n_particles=N, n_population=300, mu=5, **kw)


def test_shapes_keys_and_filter_index(fake):
    c = sir_cases()
    epipf.seed_stream(77, 5)
    res = run(c, [0.8, 0.3], [[0.1, 0.0], [0.0, 0.0], [0.2, 0.05]], chains=3, lag=2, probs=[0.5, 0.4, 0.6], cumulate=True)
    T, N, S, Q = 8, 12, 3, 3
    assert isinstance(res, epipf.WalkResult)
    assert res.loglik.shape == (S,) and res.log_zetas.shape == (S, T) and res.status.tolist() == [0, 0, 0]
    assert res.theta_mean.shape == (S, T, 2) and res.theta_quantiles.shape == (S, Q, T, 2)
    assert res.rt_mean.shape == (S, T) and res.rt_quantiles.shape == (S, Q, T) and res.lineages.shape == (S, T)
    assert res.incidence.mean.shape == (S, T, 2) and res.incidence.quantiles.shape == (S, Q, T, 2)
    assert res.incidence.lineages.shape == (S, T) and (res.incidence.sums[:, 0] == 0).all()
    np.testing.assert_array_equal(res.loglik, res.log_zetas[:, -1])
    assert res.best == int(np.argmax(res.loglik)) and (res.log_zetas[:, 1] == 0.0).all()
    eng = fake[0]
    assert eng.t_max == T and eng.max_chains == S and not hasattr(eng, "Y")      # observations are not needed
    call = eng.calls[0]
    assert call["keys"].tolist() == [epipf.chain_key(77, s) for s in range(S)]
    assert call["f"].tolist() == [5, 5, 5] and pmcmc._STREAM.next_filter == 6
    assert call["swarm"].shape == (S, N, 2) and (call["swarm"] == [0.8, 0.3]).all()      # start [d] broadcast
    np.testing.assert_array_equal(call["hw"], [[0.1, 0.0], [0.0, 0.0], [0.2, 0.05]])
    assert call["probs"].tolist() == [0.5, 0.4, 0.6] and call["cumulate"] and not call["observations"]
    np.testing.assert_array_equal(call["counts"], c)
    # the same lag goes to the three reductions; .states is Engine.smooth's answer
    assert [s["kind"] for s in eng.smooth_calls] == ["walk", "states", "flows"]
    assert all(s["n"] == S and s["lineage"] == "genealogy" and s["lag"] == 2 for s in eng.smooth_calls)
    assert res.states == ("states", S, "genealogy", 2)
    # zero half-widths keep theta: the chain's smoothed parameters are the start, at every quantile
    assert (res.theta_quantiles[1] == np.array([0.8, 0.3])).all()
    # an explicit key does not touch the stream's key; lag=None is the full smoother; the reference lineage has no flows
    res2 = run(c, [0.8, 0.3], [0.1, 0.0], key=123, lag=None, quantiles=None, lineage="reference")
    assert fake[1].calls[0]["keys"].tolist() == [123] and fake[1].calls[0]["f"].tolist() == [6]
    assert [s["kind"] for s in fake[1].smooth_calls] == ["walk", "states"]
    assert fake[1].smooth_calls[0]["lag"] is None and fake[1].smooth_calls[0]["lineage"] == "reference"
    assert res2.theta_quantiles is None and res2.theta_mean.shape == (1, T, 2) and res2.incidence is None
    res3 = run(c, [0.8, 0.3], [0.1, 0.0], lag=None, quantiles=None)
    assert res3.incidence.quantiles is None and res3.incidence.mean.shape == (1, T, 2)


def test_the_smoothed_flows_are_the_histories_own(fake):
    """epipf.incidence.true_flows on the double's history, entry by entry, and `incidence` at lag 0: the cloud's sums."""
    c = sir_cases()
    res = run(c, [0.8, 0.3], [0.1, 0.05], lag=0, quantiles=(0.5,), key=3)
    hid, anc = fake[0].history(1)
    flow = incidence.true_flows(_lib.SIR, hid[0], anc[0])
    assert flow.shape == (8, 12, 2) and (flow[0] == 0).all() and (flow >= 0).all()
    np.testing.assert_array_equal(res.incidence.sums[0], flow.sum(axis=1))
    np.testing.assert_array_equal(res.incidence.lineages[0], np.full(8, 12))
    p, i = 4, 7
    par = hid[0, p - 1, anc[0, p, i]]
    assert flow[p, i].tolist() == [par[0] - hid[0, p, i, 0], hid[0, p, i, 2] - par[2]]
    # SEIR's three columns
    s = ic.fixture()["seir"][:4]
    r3 = epipf.walk_incidence_filter(s[:, 0], "seir", [0.9, 0.6, 0.3], [0.1, 0.0, 0.0], n_particles=8, n_population=300,
                                     mu=5, lag=1, key=2)
    hid, anc = fake[1].history(1)
    flow = incidence.true_flows(_lib.SEIR, hid, anc)
    assert flow.shape == (1, 6, 8, 3) and (flow >= 0).all() and r3.incidence.mean.shape == (1, 6, 3)
    p, i = 3, 5
    par, new = hid[0, p - 1, anc[0, p, i]], hid[0, p, i]
    assert flow[0, p, i].tolist() == [par[0] - new[0], new[2] + new[3] - par[2] - par[3], new[3] - par[3]]


def test_flows_map_into_the_models_columns(fake):
    c = sir_cases()
    run(c[:, 1], [0.8, 0.3], [0.1, 0.0], flows=("removals",), N=4)
    got = fake[0].calls[0]["counts"]
    assert got.shape == (6, 2) and np.isnan(got[:, 0]).all()
    np.testing.assert_array_equal(got[:, 1], c[:, 1])
    run(c[:, ::-1], [0.8, 0.3], [0.1, 0.0], flows=("removals", "infections"), N=4)
    np.testing.assert_array_equal(fake[1].calls[0]["counts"], c)
    run(c[:, 0], [0.8, 0.3], [0.1, 0.0], N=4, flows="infections")                # the default column, as a string
    np.testing.assert_array_equal(fake[2].calls[0]["counts"][:, 0], c[:, 0])
    assert np.isnan(fake[2].calls[0]["counts"][:, 1]).all()
    s = ic.fixture()["seir"][:4]
    epipf.walk_incidence_filter(s[:, [2, 0]], "seir", [0.9, 0.6, 0.3], [0.1, 0.0, 0.0], flows=("removals", "infections"),
                                n_particles=4, n_population=300, mu=5, observations=True, probs=0.2)
    got = fake[3].calls[0]
    assert got["counts"].shape == (4, 3) and np.isnan(got["counts"][:, 1]).all() and got["observations"]
    np.testing.assert_array_equal(got["counts"][:, [0, 2]], s[:, [0, 2]])
    assert got["swarm"].shape == (1, 4, 3) and got["probs"].tolist() == [0.2]


def test_start_and_rw_broadcast(fake):
    N, S = 6, 2
    rng = np.random.default_rng(0)
    prior = rng.uniform(0.2, 1.0, size=(N, 2))
    run(sir_cases(2), prior, [0.1, 0.05], N=N, chains=S)
    call = fake[0].calls[0]
    np.testing.assert_array_equal(call["swarm"], np.stack([prior, prior]))
    np.testing.assert_array_equal(call["hw"], [[0.1, 0.05]] * S)
    assert call["probs"].tolist() == [0.5, 0.5]
    per_chain = rng.uniform(0.2, 1.0, size=(S, N, 2))
    run(sir_cases(2), per_chain, [[0.1, 0.05], [0.0, 0.0]], N=N, chains=S)
    np.testing.assert_array_equal(fake[1].calls[0]["swarm"], per_chain)


def test_best_skips_a_degenerate_chain(fake, monkeypatch):
    """The batch's dying chain (walk_incidence_cases.BATCH[1] under its own key) between two good ones."""
    monkeypatch.setattr(walk_incidence, "chain_key", lambda k, s: wic.BATCH[s][3])
    epipf.seed_stream(11, wic.F)                         # the batch's filter index
    counts = ic.daily("sir", False, (0, 1))
    starts = np.stack([wic.swarm(b[0]) for b in wic.BATCH])
    res = run(counts, starts, [b[1] for b in wic.BATCH], N=wic.N, chains=3, probs=[b[2] for b in wic.BATCH], lag=3)
    assert fake[0].calls[0]["keys"].tolist() == [11, 1, 2]
    assert res.status.tolist() == [0, 1, 0] and res.best in (0, 2)
    assert np.isneginf(res.loglik[1]) and np.isneginf(res.log_zetas[1, 3:]).all() and np.isfinite(res.log_zetas[1, :3]).all()
    assert np.isnan(res.theta_mean[1]).all() and np.isnan(res.rt_quantiles[1]).all() and (res.lineages[1] == 0).all()
    assert np.isnan(res.incidence.mean[1]).all() and (res.incidence.lineages[1] == 0).all()
    assert np.isfinite(res.incidence.mean[[0, 2]]).all()


def test_incidence_filter_fills_incidence_when_it_smooths(monkeypatch):
    """IncidenceResult.incidence: Engine.incidence_smooth under the same quantiles and lag, read once; None without
    quantiles and under the reference lineage; refused, not another pass's flows, once the shared engine has run again."""
    calls = []

    class Eng(wioe.OracleWalkIncidenceEngine):
        run_serial = 0                                   # Engine.run_serial: every run counts

        def run_incidence(self, thetas, probs, keys, filter_indices, counts, observations=False, cumulate=False,
                          active=None):
            self.run_serial += 1
            th = np.asarray(thetas, dtype=np.float64)
            return self.walk_incidence(np.repeat(th[:, None, :], self.N, axis=1), np.zeros_like(th), probs, keys,
                                       filter_indices, counts, observations=observations, cumulate=cumulate)

        def incidence_smooth(self, n_chains=None, **kw):
            calls.append(dict(n=n_chains, **kw))
            return super().incidence_smooth(n_chains, **kw)

    shared = {}                                          # get_engine's cache: one engine per (model, N)

    def get_engine(m, g, N, T, chains=1, device=0):
        return shared.setdefault((m, int(N)), Eng(0, 1, int(N), T, chains))

    monkeypatch.setattr(incidence._engine, "get_engine", get_engine)
    c = sir_cases()
    kw = dict(flows=("infections", "removals"), n_particles=8, n_population=300, mu=5, key=4)
    res = epipf.incidence_filter(c, "sir", [[0.8, 0.3], [1.0, 0.3]], quantiles=(0.5,), lag=2, **kw)
    first = res.incidence
    assert calls == [dict(n=2, quantiles=(0.5,), lag=2)] and res.incidence is first
    assert first.mean.shape == (2, 8, 2) and first.quantiles.shape == (2, 1, 8, 2)
    assert epipf.incidence_filter(c, "sir", [0.8, 0.3], **kw).incidence is None
    assert epipf.incidence_filter(c, "sir", [0.8, 0.3], quantiles=(0.5,), lineage="reference", **kw).incidence is None
    assert len(calls) == 1
    # a second run on the shared engine between the call and the first read: the read is refused, the second run's own
    # result reads its flows, and what was read before the second run stays the first run's
    a = epipf.incidence_filter(c, "sir", [[0.8, 0.3], [1.0, 0.3]], quantiles=(0.5,), lag=2, **kw)
    b = epipf.incidence_filter(c, "sir", [[1.6, 0.3], [0.4, 0.3]], quantiles=(0.5,), lag=2, **kw)
    assert a._eng is b._eng
    with pytest.raises(RuntimeError, match="another filter"):
        a.incidence
    with pytest.raises(RuntimeError, match="another filter"):      # and again: nothing was cached
        a.incidence
    assert len(calls) == 1
    assert not np.array_equal(b.incidence.sums, first.sums) and len(calls) == 2
    np.testing.assert_array_equal(res.incidence.sums, first.sums)
    # an engine that keeps no run serial cannot vouch for its history
    class Bare:
        def incidence_smooth(self, *a, **k):
            raise AssertionError("read from an engine without a run serial")
    r = incidence.IncidenceResult(res.log_zetas, res.status, None, Bare(), dict(quantiles=(0.5,), lag=2))
    with pytest.raises(RuntimeError):
        r.incidence


@pytest.mark.parametrize("kw", [
    dict(start=[0.8]), dict(start=[0.8, 0.3, 0.1]), dict(start=np.ones((5, 2))), dict(start=np.ones((3, 12, 2))),
    dict(start=[-0.1, 0.3]), dict(start=[np.nan, 0.3]), dict(rw=[0.1]), dict(rw=[-0.1, 0.0]), dict(rw=[np.inf, 0.0]),
    dict(rw=np.ones((3, 2))), dict(lag=-1), dict(lag=1.5), dict(lag=True), dict(lineage="tree"), dict(quantiles=(1.2,)),
    dict(quantiles=(-0.1,)), dict(chains=0), dict(n_particles=0), dict(flows=()), dict(flows=("onsets",)),
    dict(flows=("infections", "infections")), dict(flows=("infections", "removals")), dict(cases=[1.0, -2.0]),
    dict(cases=[1.0, np.inf]), dict(cases=[1.0, 2.5]), dict(cases=[]), dict(cases=np.ones((3, 2))), dict(probs=1.5),
    dict(probs=-0.1), dict(probs=np.nan), dict(probs=[0.5, 0.5, 0.5]), dict(probs=-0.1, observations=True)])
def test_value_errors_come_before_any_device_call(monkeypatch, kw):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(walk_incidence._engine, "get_engine", no_engine)
    args = dict(cases=[1.0, 2.0, np.nan], start=[0.8, 0.3], rw=[0.1, 0.0], n_particles=12, chains=2)
    args.update(kw)
    cases, start, rw = args.pop("cases"), args.pop("start"), args.pop("rw")
    with pytest.raises(ValueError):
        epipf.walk_incidence_filter(cases, "sir", start, rw, n_population=300, mu=5, **args)


def test_what_the_normal_model_takes(fake):
    """Non-integer reports and a noise ratio above 1 are the normal model's to take."""
    res = run([1.0, 2.5, np.nan], [0.8, 0.3], [0.1, 0.0], flows=("infections",), N=4, observations=True, probs=1.5)
    assert res.log_zetas.shape == (1, 5) and fake[0].calls[0]["probs"].tolist() == [1.5]


@pytest.mark.parametrize("model", ["sir_subgroups", "sir_subgroups2"])
def test_subgroup_models_are_refused_before_any_device_call(monkeypatch, model):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(walk_incidence._engine, "get_engine", no_engine)
    with pytest.raises(ValueError, match="SIR and SEIR"):
        epipf.walk_incidence_filter(np.zeros(4), model, [0.5] * 5, [0.1] * 5)


def test_the_names_are_public_and_declared():
    assert "walk_incidence_filter" in epipf.__all__
    names = ["epipf_incidence_walk", "epipf_incidence_smooth"]
    header = open(REPO + "/include/epipf.h").read()
    for n in names:
        assert n in _lib.EXPORTS and not re.search(r"\d", n) and re.search(r"\b%s\s*\(" % n, header)
    assert _lib.ABI_VERSION == 9 and "#define EPIPF_ABI_VERSION 9" in header
