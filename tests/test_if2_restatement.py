"""The numpy restatement of iterated filtering (tests/if2_restatement.py) against the CPU oracle: with no
jitter it is the oracle's particle filter bit for bit, and on the small SIR fixture it finds the likelihood's peak,
degenerates from a hopeless start, and reflects at 0.  No GPU."""
import os

import numpy as np
import pytest

import if2_restatement as rs
import oracle
from conftest import GOLDEN

SETTINGS = dict(N=48, M=12, rw=(0.1, 0.05), cooling=0.5 ** (50 / 12), start=(1.2, 0.5), keys=(1, 2, 3, 4))


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "if2_sir_small.npz"))
    return dict(Y=z["Y"], npop=float(z["population"]), mu=float(z["mu"]), probs=float(z["probs"]))


def search(fx, key, start, rw, M, N=SETTINGS["N"], cooling=SETTINGS["cooling"]):
    hw = rs.cooling_table(rw, cooling, M)
    swarm = np.tile(np.asarray(start, dtype=np.float64), (N, 1))
    return rs.run(fx["Y"], "sir", swarm, hw, False, fx["probs"], fx["npop"], fx["mu"], key, 0)


def test_fixture_is_the_issues_epidemic():
    z = np.load(os.path.join(GOLDEN, "if2_sir_small.npz"))
    assert z["X"][:, 1].tolist() == [5, 7, 9, 16, 19, 22, 43, 61, 70, 81, 92, 90, 84, 71, 61, 55, 42, 36, 29, 22, 19, 18,
                                     18, 13, 8]
    assert z["Y"].shape == (25, 3) and (z["Y"] <= z["X"]).all()
    assert np.array_equal(z["Y"], np.random.default_rng(5).binomial(z["X"], 0.5))


@pytest.mark.parametrize("model,theta,C", [("sir", (0.8, 0.3), 3), ("seir", (0.9, 0.6, 0.3), 4)])
@pytest.mark.parametrize("observations,probs", [(False, 0.5), (True, 0.2)])
def test_no_jitter_is_the_oracle_filter(fixture, model, theta, C, observations, probs):
    """(a) zero half-widths and equal theta: hidden, ancestry and log_zetas of oracle.particle_filter exactly."""
    N, T = 40, 12
    Y = fixture["Y"][:T]
    if C == 4:
        Y = np.concatenate([Y[:, :1], Y[:, 1:2] // 2, Y[:, 1:2] - Y[:, 1:2] // 2, Y[:, 2:]], axis=1)
    swarm = np.tile(np.array(theta), (N, 1))
    r = rs.one_pass(Y, model, swarm, np.zeros(len(theta)), observations, probs, fixture["npop"], fixture["mu"], 11, 3)
    o = oracle.particle_filter(Y, model, theta, observations, probs, N, fixture["npop"], fixture["mu"], key=11,
                               filter_index=3)
    assert r["status"] == o["status"] == 0
    np.testing.assert_array_equal(r["hidden"], o["hidden"])
    np.testing.assert_array_equal(r["ancestry"], o["ancestry"])
    np.testing.assert_array_equal(r["log_zetas"], o["log_zetas"])
    np.testing.assert_array_equal(r["theta"], swarm)


@pytest.fixture(scope="module")
def start_score(fixture):
    return rs.score(fixture["Y"], "sir", SETTINGS["start"], False, fixture["probs"], fixture["npop"], fixture["mu"])


@pytest.mark.parametrize("key", SETTINGS["keys"])
def test_search_gains_thirty_log_units(fixture, start_score, key):
    """(b) every key's final mean scores >= 30 log units above the start (measured: at least 62.9)."""
    r = search(fixture, key, SETTINGS["start"], SETTINGS["rw"], SETTINGS["M"])
    assert r["status"] == 0 and r["iterations_done"] == SETTINGS["M"]
    end = rs.score(fixture["Y"], "sir", r["mean"][-1], False, fixture["probs"], fixture["npop"], fixture["mu"])
    print(f"key {key}: theta {r['mean'][-1]}, score {end:.2f}, start {start_score:.2f}, gain {end - start_score:.2f}")
    assert end - start_score >= 30.0


@pytest.mark.parametrize("key", SETTINGS["keys"])
def test_hopeless_start_degenerates_in_iteration_zero(fixture, key):
    """(c) start (2.0, 1.0): every filter dies, the swarm is returned as it came and the rows are NaN."""
    r = search(fixture, key, (2.0, 1.0), SETTINGS["rw"], 2)
    assert r["status"] == rs.DEGENERATE and r["iterations_done"] == 0
    np.testing.assert_array_equal(r["swarm"], np.tile([2.0, 1.0], (SETTINGS["N"], 1)))
    assert np.isnan(r["mean"]).all() and np.isnan(r["loglik"]).all()


def test_reflection_keeps_theta_non_negative(fixture):
    """(d) a start of 0.01 with half-width 0.05 reflects at least once and never goes negative."""
    hw = np.tile([0.05, 0.05], (2, 1))
    swarm = np.tile([0.01, 0.01], (SETTINGS["N"], 1))
    r = rs.run(fixture["Y"][:4], "sir", swarm, hw, False, fixture["probs"], fixture["npop"], fixture["mu"], 5, 0)
    assert r["reflections"] >= 1 and r["status"] == 0 and r["iterations_done"] == 2
    assert (r["swarm"] >= 0.0).all()
    u = rs.perturb_uniforms(5, 0, 0, SETTINGS["N"], 2)
    t = 0.01 + 0.05 * (2.0 * u - 1.0)
    np.testing.assert_array_equal(rs.perturb(swarm, hw[0], 5, 0, 0), np.abs(t))
