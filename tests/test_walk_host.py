"""epipf.walk_filter's host logic over an oracle-backed engine double (tests/walk_oracle_engine.py): shapes, key and
filter-index bookkeeping, broadcasting of start and rw, .best beside a degenerate chain, and every refusal before any
device call.  No GPU."""
import re

import numpy as np
import pytest

import epipf
import walk_oracle_engine as woe
from conftest import REPO
from epipf import _lib, pmcmc, walk


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(walk._engine, "get_engine", woe.fake_get_engine)
    woe.ENGINES.clear()
    return woe.ENGINES


def fixture():
    import if2_cases
    return if2_cases.load_fixture()


def run(fx, start, rw, T=8, N=12, **kw):
    return epipf.walk_filter(fx["sir"][:T], "sir", start, rw, n_particles=N, n_population=fx["npop"], mu=fx["mu"],
                             probs=fx["probs"], **kw)


def test_shapes_keys_and_filter_index(fake):
    fx = fixture()
    epipf.seed_stream(77, 5)
    res = run(fx, [0.8, 0.3], [[0.1, 0.0], [0.0, 0.0], [0.2, 0.05]], chains=3, lag=2)
    T, N, S, Q = 8, 12, 3, 3
    assert res.loglik.shape == (S,) and res.log_zetas.shape == (S, T) and res.status.shape == (S,)
    assert res.theta_mean.shape == (S, T, 2) and res.theta_quantiles.shape == (S, Q, T, 2)
    assert res.rt_mean.shape == (S, T) and res.rt_quantiles.shape == (S, Q, T) and res.lineages.shape == (S, T)
    np.testing.assert_array_equal(res.loglik, res.log_zetas[:, -1])
    assert res.best == int(np.argmax(res.loglik))
    call = fake[0].walk_calls[0]
    assert call["keys"].tolist() == [epipf.chain_key(77, s) for s in range(S)]
    assert call["f"].tolist() == [5, 5, 5] and pmcmc._STREAM.next_filter == 6
    assert call["swarm"].shape == (S, N, 2) and (call["swarm"] == [0.8, 0.3]).all()      # start [d] broadcast
    np.testing.assert_array_equal(call["hw"], [[0.1, 0.0], [0.0, 0.0], [0.2, 0.05]])
    # the same lineage and lag go to both reductions; .states is Engine.smooth's answer
    assert [c["kind"] for c in fake[0].smooth_calls] == ["walk", "states"]
    assert all(c["n"] == S and c["lineage"] == "genealogy" and c["lag"] == 2 for c in fake[0].smooth_calls)
    assert res.states == ("states", S, "genealogy", 2)
    # zero half-widths keep theta: the chain's smoothed parameters are the start, at every quantile
    assert (res.theta_quantiles[1] == np.array([0.8, 0.3])).all()
    # an explicit key does not touch the stream's key, and lag=None is the full smoother
    res2 = run(fx, [0.8, 0.3], [0.1, 0.0], key=123, lag=None, quantiles=None, lineage="reference")
    assert fake[1].walk_calls[0]["keys"].tolist() == [123] and fake[1].walk_calls[0]["f"].tolist() == [6]
    assert fake[1].smooth_calls[0]["lag"] is None and fake[1].smooth_calls[0]["lineage"] == "reference"
    assert res2.theta_quantiles is None and res2.rt_quantiles is None and res2.theta_mean.shape == (1, T, 2)


def test_start_and_rw_broadcast(fake):
    fx = fixture()
    N, S = 6, 2
    rng = np.random.default_rng(0)
    prior = rng.uniform(0.2, 1.0, size=(N, 2))
    run(fx, prior, [0.1, 0.05], T=3, N=N, chains=S)
    call = fake[0].walk_calls[0]
    np.testing.assert_array_equal(call["swarm"], np.stack([prior, prior]))
    np.testing.assert_array_equal(call["hw"], [[0.1, 0.05]] * S)
    per_chain = rng.uniform(0.2, 1.0, size=(S, N, 2))
    run(fx, per_chain, [[0.1, 0.05], [0.0, 0.0]], T=3, N=N, chains=S)
    np.testing.assert_array_equal(fake[1].walk_calls[0]["swarm"], per_chain)


def test_best_skips_a_degenerate_chain(fake):
    fx = fixture()
    starts = np.repeat(np.array([[1.2, 0.5], [2.0, 1.0], [1.0, 0.4]])[:, None, :], 48, axis=1)
    epipf.seed_stream(1, 0)
    res = epipf.walk_filter(fx["sir"], "sir", starts, [0.1, 0.05], n_particles=48, n_population=fx["npop"], mu=fx["mu"],
                            probs=fx["probs"], chains=3, lag=3)
    assert _lib.STATUS_DEGENERATE in res.status.tolist() and _lib.STATUS_OK in res.status.tolist()
    dead = res.status != _lib.STATUS_OK
    assert np.isneginf(res.loglik[dead]).all() and np.isnan(res.theta_mean[dead]).all() and np.isnan(res.rt_quantiles[dead]).all()
    assert res.status[res.best] == _lib.STATUS_OK
    assert res.best == int(np.argmax(np.where(dead, -np.inf, res.log_zetas[:, -1])))


def test_no_chain_left_has_no_best():
    r = walk.WalkResult(np.full((2, 3), -np.inf), np.array([1, 1], dtype=np.int32), np.full((2, 3, 3), np.nan), None,
                        np.zeros((2, 3), dtype=np.int32), None)
    assert r.best is None and np.isneginf(r.loglik).all()


@pytest.mark.parametrize("kw", [
    dict(start=[0.8]), dict(start=[0.8, 0.3, 0.1]), dict(start=np.ones((5, 2))), dict(start=np.ones((3, 12, 2))),
    dict(start=[-0.1, 0.3]), dict(start=[np.nan, 0.3]), dict(rw=[0.1]), dict(rw=[-0.1, 0.0]), dict(rw=[np.inf, 0.0]),
    dict(rw=np.ones((3, 2))), dict(lag=-1), dict(lag=1.5), dict(lag=True), dict(lineage="tree"), dict(quantiles=(1.2,)),
    dict(quantiles=(-0.1,)), dict(chains=0), dict(n_particles=0)])
def test_value_errors_come_before_any_device_call(monkeypatch, kw):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(walk._engine, "get_engine", no_engine)
    fx = fixture()
    args = dict(start=[0.8, 0.3], rw=[0.1, 0.0], n_particles=12, chains=2)
    args.update(kw)
    start, rw = args.pop("start"), args.pop("rw")
    with pytest.raises(ValueError):
        epipf.walk_filter(fx["sir"][:4], "sir", start, rw, n_population=fx["npop"], mu=fx["mu"], probs=fx["probs"], **args)


@pytest.mark.parametrize("model", ["sir_subgroups", "sir_subgroups2"])
def test_subgroup_models_are_refused_before_any_device_call(monkeypatch, model):
    def no_engine(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(walk._engine, "get_engine", no_engine)
    with pytest.raises(ValueError, match="SIR and SEIR"):
        epipf.walk_filter(np.zeros((4, 6)), model, [0.5] * 5, [0.1] * 5)


def test_the_names_are_public_and_the_entry_points_carry_no_digit():
    assert "walk_filter" in epipf.__all__ and "WalkResult" in epipf.__all__
    names = [n for n in _lib.EXPORTS if n.startswith("epipf_walk")]
    assert sorted(names) == ["epipf_walk_filter", "epipf_walk_history", "epipf_walk_smooth", "epipf_walk_smooth_history"]
    assert not any(re.search(r"\d", n) for n in names)
    header = open(REPO + "/include/epipf.h").read()
    assert all(re.search(r"\b%s\s*\(" % n, header) for n in names)
    assert _lib.ABI_VERSION == 9
