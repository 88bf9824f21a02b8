"""epipf.if2's host logic over an oracle-backed engine double (tests/if2_oracle_engine.py): the cooling table, the
broadcasting of `start`, the keys and filter indices, continue_, evaluate and best, and the subgroup ValueError.
No GPU."""
import importlib
import os
import re

import numpy as np
import pytest

import if2_oracle_engine
import if2_restatement as rs
from conftest import GOLDEN, REPO

mod = importlib.import_module("epipf.if2")               # epipf.if2 itself is the function


@pytest.fixture()
def engines(monkeypatch):
    made = []

    def get(*a, **k):
        made.append(if2_oracle_engine.fake_get_engine(*a, **k))
        return made[-1]
    monkeypatch.setattr(mod._engine, "get_engine", get)
    return made


@pytest.fixture(scope="module")
def data():
    z = np.load(os.path.join(GOLDEN, "if2_sir_small.npz"))
    return dict(Y=z["Y"][:8], n_population=float(z["population"]), mu=float(z["mu"]), probs=float(z["probs"]))


def call(data, start, **kw):
    import epipf
    epipf.seed_stream(21, 5)
    args = dict(iterations=3, cooling=0.5, n_particles=16, searches=1, evaluate=False)
    args.update(kw)
    return epipf.if2(data["Y"], "sir", start, (0.1, 0.05), n_population=data["n_population"], mu=data["mu"],
                     probs=data["probs"], **args)


def test_cooling_table_is_pomps_fraction_50():
    hw = mod.cooling_table((0.1, 0.05), 0.5, 4, first=48)
    assert hw.shape == (4, 2)
    for i, m in enumerate(range(48, 52)):
        assert hw[i, 0] == 0.1 * 0.5 ** (m / 50.0) and hw[i, 1] == 0.05 * 0.5 ** (m / 50.0)
    assert hw[2, 0] == 0.05                              # after 50 iterations: the cooling fraction
    np.testing.assert_array_equal(hw, rs.cooling_table((0.1, 0.05), 0.5, 4, first=48))


def test_the_call_the_engine_sees(data, engines):
    res = call(data, (1.0, 0.4), searches=2)
    (eng,) = engines
    assert eng.max_chains == 2 and eng.N == 16 and not eng.run_calls
    (c,) = eng.if2_calls
    np.testing.assert_array_equal(c["swarm"], np.tile([1.0, 0.4], (2, 16, 1)))     # every particle at the start point
    np.testing.assert_array_equal(c["hw"], mod.cooling_table((0.1, 0.05), 0.5, 3))
    assert c["keys"].tolist() == [21, 21 + (1 << 32)] and c["f0"].tolist() == [5, 5]
    assert mod._STREAM.next_filter == 8                  # the stream's counter moved past the three iterations
    assert res.theta.shape == (2, 2) and res.trace.shape == (2, 3, 2) and res.loglik.shape == (2, 3)
    assert res.swarm.shape == (2, 16, 2) and res.loglik_at_theta is None and res.best is None
    np.testing.assert_array_equal(res.theta, res.trace[:, -1])
    np.testing.assert_array_equal(res.theta, res.swarm.mean(axis=1))
    assert (res.status == 0).all() and (res.iterations_done == 3).all()
    assert not np.array_equal(res.swarm[0], res.swarm[1])                           # own keys: own searches


def test_start_per_search_and_its_shape_check(data, engines):
    call(data, [[1.0, 0.4], [0.7, 0.2]], searches=2, iterations=1)
    sw = engines[0].if2_calls[0]["swarm"]
    np.testing.assert_array_equal(sw[0], np.tile([1.0, 0.4], (16, 1)))
    np.testing.assert_array_equal(sw[1], np.tile([0.7, 0.2], (16, 1)))
    with pytest.raises(ValueError):
        call(data, [[1.0, 0.4], [0.7, 0.2], [0.5, 0.5]], searches=2)
    with pytest.raises(ValueError):
        call(data, (1.0, 0.4, 0.3))
    with pytest.raises(ValueError):
        call(data, (-1.0, 0.4))


def test_continue_equals_one_longer_run(data, engines):
    whole = call(data, (1.0, 0.4), iterations=3)
    part = call(data, (1.0, 0.4), iterations=1)
    more = part.continue_(2)
    c = engines[1].if2_calls
    assert len(c) == 2 and c[1]["f0"].tolist() == [6]
    np.testing.assert_array_equal(c[1]["swarm"], part.swarm)
    np.testing.assert_array_equal(c[1]["hw"], mod.cooling_table((0.1, 0.05), 0.5, 2, first=1))
    np.testing.assert_array_equal(more.swarm, whole.swarm)
    np.testing.assert_array_equal(more.trace, whole.trace)
    np.testing.assert_array_equal(more.loglik, whole.loglik)
    assert more.iterations_done.tolist() == [3] and mod._STREAM.next_filter == 8


def test_evaluate_scores_theta_with_plain_filters_and_picks_the_best(data, engines):
    res = call(data, [[1.0, 0.4], [2.0, 1.0]], searches=2, evaluate=True)
    (eng,) = engines
    assert eng.max_chains == 16
    (r,) = eng.run_calls                                 # one batched run: 8 filters per search
    np.testing.assert_array_equal(r["thetas"], np.repeat(res.theta, 8, axis=0))
    assert r["fidx"].tolist() == list(range(8)) * 2
    assert r["keys"].tolist() == [21 + (2 << 32)] * 8 + [21 + (3 << 32)] * 8       # keys no search uses
    for s in range(2):
        want = rs.score(data["Y"], "sir", res.theta[s], False, data["probs"], data["n_population"], data["mu"],
                        n_particles=16, key=int(r["keys"][8 * s]))
        assert res.loglik_at_theta[s] == pytest.approx(want, rel=1e-12)
    assert res.best == int(np.argmax(res.loglik_at_theta))


def test_a_degenerate_search_keeps_its_swarm_and_nan_rows(data, engines):
    z = np.load(os.path.join(GOLDEN, "if2_sir_small.npz"))
    full = dict(data, Y=z["Y"])
    res = call(full, [[2.0, 1.0], [1.0, 0.4]], searches=2, iterations=2, evaluate=True)
    assert res.status.tolist() == [1, 0] and res.iterations_done.tolist() == [0, 2]
    np.testing.assert_array_equal(res.swarm[0], np.tile([2.0, 1.0], (16, 1)))
    np.testing.assert_array_equal(res.theta[0], [2.0, 1.0])
    assert np.isnan(res.trace[0]).all() and np.isnan(res.loglik[0]).all() and np.isfinite(res.trace[1]).all()
    assert res.best == 1


def test_subgroup_models_raise_before_any_engine_exists(data, engines):
    import epipf
    for model in ("sir_subgroups", epipf.ModelType.SIR_SUBGROUPS2):
        with pytest.raises(ValueError, match="subgroup"):
            epipf.if2(data["Y"], model, (1.0, 0.4), (0.1, 0.05))
    assert not engines


def test_log_mean_exp():
    assert mod.log_mean_exp([[-np.inf, -np.inf]])[0] == -np.inf
    assert mod.log_mean_exp([[0.0, -np.inf]])[0] == pytest.approx(np.log(0.5))
    assert mod.log_mean_exp([[-1000.0, -1000.0]])[0] == pytest.approx(-1000.0)


def test_the_numbered_entry_point_is_declared_bound_and_exported():
    """tests/test_abi.py's checks for a name its letters-only pattern cannot see."""
    import ctypes
    from epipf import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "epipf.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(epipf_[a-z_]*[0-9][a-z0-9_]*)\s*\(", text)))
    assert declared == sorted(_lib.EXPORTS_NUMBERED) == ["epipf_if2"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, s) for s in declared) and hasattr(_lib.load(), "epipf_if2")
