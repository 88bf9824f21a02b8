"""The numpy restatement of iterated filtering (tests/if2_restatement.py) against the CPU oracle: with no
jitter it is the oracle's particle filter bit for bit, and on the small SIR fixture it finds the likelihood's peak,
degenerates from a hopeless start, and reflects at 0; and what each input of the device's path tests (tests/if2_cases.py,
tests/test_gpu_if2_paths.py) contains.  No GPU."""
import os

import numpy as np
import pytest

import if2_cases as ic
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


# ------------------------------------------------------------------------- the inputs of tests/test_gpu_if2_paths.py
@pytest.fixture(scope="module")
def fx():
    return ic.load_fixture()


def completes(c, M=2):
    r = ic.restate(c)
    assert r["status"] == 0 and r["iterations_done"] == M and len(r["swarms"]) == M
    assert np.isfinite(r["mean"]).all() and np.isfinite(r["log_zetas"]).all() and (r["events"] > 0).all()
    return r


@pytest.mark.parametrize("model,N,T", [("sir", 300, 5), ("seir", 300, 5), ("sir", 700, 3), ("sir", 70, 1), ("sir", 70, 2),
                                       ("sir", 70, 3), ("sir", 1, 3)])
def test_multi_block_and_short_cases_complete_with_distinct_rows(fx, model, N, T):
    """Cases 1 and 2: every row of the final swarm differs from every other."""
    c = ic.case(fx, model, N, T)
    r = ic.restate(c) if T == 1 else completes(c)
    assert r["status"] == 0 and r["iterations_done"] == 2 and ic.distinct(r["swarm"]) == N
    if T == 1:                                           # no step: the iteration's swarm is its step-0 jitter
        assert r["events"].tolist() == [0, 0]
        first = rs.perturb(c["swarm0"], c["hw"][0], ic.KEY, ic.F, 0)
        np.testing.assert_array_equal(r["swarms"][0], first)
        np.testing.assert_array_equal(r["swarm"], rs.perturb(first, c["hw"][1], ic.KEY, ic.F + 1, 0))


@pytest.mark.parametrize("model", ["sir", "seir"])
@pytest.mark.parametrize("observations", [True, False])
def test_seven_day_cases_complete(fx, model, observations):
    """Case 3 (normal observations) and its binomial twin (case 7's input): N = 130, T = 7."""
    r = completes(ic.case(fx, model, 130, 7, observations=observations))
    assert ic.distinct(r["swarm"]) == 130


@pytest.mark.parametrize("key", sorted(ic.LATE))
def test_late_degeneracy_keys(fx, key):
    """Case 5: the search completes `done` iterations, then dies at the given step of the next one."""
    status, done, step = ic.LATE[key]
    r = ic.restate(ic.late_case(fx, key))
    assert (r["status"], r["iterations_done"], ic.dying_step(r)) == (status, done, step)
    assert np.isfinite(r["mean"][:done]).all() and np.isnan(r["mean"][done:]).all()
    assert np.isfinite(r["log_zetas"][:done]).all() and np.isnan(r["log_zetas"][done:]).all()
    np.testing.assert_array_equal(r["swarm"], r["swarms"][done - 1])     # the last completed iteration's


@pytest.mark.parametrize("npop,mu,T", [(10 ** 6, 400, 6), (2 * 10 ** 4, 40, 8)])
@pytest.mark.parametrize("observations", [False, True])
def test_population_cases_complete(fx, npop, mu, T, observations):
    """Case 6: S I reaches 10^9 and more at the larger population, and every search completes."""
    c = ic.population_case(fx, npop, mu, T, observations)
    r = completes(c)
    assert ic.distinct(r["swarm"]) > 1
    if npop == 10 ** 6:
        assert (r["hidden"][:, :, 0].astype(np.int64) * r["hidden"][:, :, 1]).max() >= 10 ** 9


@pytest.mark.parametrize("T", [2, 7])
@pytest.mark.parametrize("odd_beta", [0.0, 1e-30])
def test_mixed_rate_cases_complete(fx, T, odd_beta):
    """Case 8: beta is never jittered, so the swarm holds the two start values only; at T = 2 it keeps both."""
    r = completes(ic.mixed_case(fx, T, odd_beta))
    assert set(np.unique(r["swarm"][:, 0])) <= {0.8, odd_beta}
    if T == 2:
        assert set(np.unique(r["swarm"][:, 0])) == {0.8, odd_beta}


@pytest.mark.parametrize("theta", [(0.0, 0.3), (0.8, 0.0), (0.0, 0.0)])
def test_zero_rate_anchors_complete(fx, theta):
    """Case 8's anchors: the oracle filter completes at N = 70, T = 4 with a rate of zero."""
    o = oracle.particle_filter(fx["sir"][:4], "sir", theta, False, 0.5, 70, fx["npop"], fx["mu"], key=ic.KEY,
                               filter_index=ic.F)
    assert o["status"] == 0


@pytest.mark.parametrize("N", [1, 70, 256, 257, 700])
def test_device_mean_is_the_mean(N):
    """The finish kernel's summation order against np.mean: 2 N 2^-53 relative, any order of non-negative terms."""
    swarm = np.random.default_rng(N).uniform(0.0, 2.0, (N, 3))
    got, want = rs.device_mean(swarm), swarm.mean(axis=0)
    assert (np.abs(got - want) <= 2.0 * N * 2.0 ** -53 * np.abs(want)).all()
    if N <= 256:                                         # one value per stride: the plain left-to-right sum
        tot = np.zeros(3)
        for row in swarm:
            tot = tot + row
        np.testing.assert_array_equal(got, tot / float(N))
