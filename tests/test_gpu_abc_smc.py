"""ABC-SMC on the GPU (epipf_abc_smc_generation / epipf_abc_smc_weights through the C ABI, epipf.abc_smc on top)
against the numpy restatement of DESIGN.md §15 (tests/abc_smc_restatement.py: numpy for everything new, the CPU oracle
for each simulated trial), bit for bit, and against the reference-exact rejection sampler statistically.  Needs an
MI355X."""
import numpy as np
import pytest

import abc_smc_restatement as rs
import oracle
from conftest import load_golden

pytestmark = pytest.mark.gpu

ABC_CASES = ["noisy_400", "noisy_150", "extinct_all", "float_obs_15", "float_obs_200"]
RUN = dict(n=64, thresholds=[400.0, 250.0, 150.0, 100.0], key=777, f=0)


@pytest.fixture(scope="module")
def abc_golden():
    return load_golden("abc_golden.npz")


@pytest.fixture(scope="module")
def engine():
    from epipf.engine import get_engine
    return get_engine("sir", 1, 1, 1, 1)


def priors_of(rec):
    p = rec["priors"]
    return {"beta": [float(p[0]), float(p[1])], "gamma": [float(p[2]), float(p[3])]}


@pytest.fixture(scope="module")
def restated(abc_golden):
    """The N = 64 run of the restatement (about a second), shared and never modified."""
    rec = abc_golden["abc_noisy_150"]
    return rs.run(rec["Y"], RUN["n"], RUN["thresholds"], priors_of(rec), RUN["key"], RUN["f"])


def assert_run_equals(res, gens):
    assert len(res["generations"]) == len(gens)
    for g, (d, o) in enumerate(zip(res["generations"], gens)):
        assert d["trials"] == o["trials"], g
        assert d["threshold"] == o["threshold"], g
        np.testing.assert_array_equal(d["half_width"], o["half_width"])
        np.testing.assert_array_equal(d["theta"], o["theta"])
        np.testing.assert_array_equal(d["ancestors"], o["ancestors"])
        np.testing.assert_array_equal(d["distances"], o["distances"])
        np.testing.assert_array_equal(d["denominators"], o["denominators"])
        np.testing.assert_array_equal(d["weights"], o["weights"])
    np.testing.assert_array_equal(res["trajectories"], gens[-1]["traj"])
    np.testing.assert_array_equal(res["weights"], gens[-1]["weights"])
    assert res["total_trials"] == sum(o["trials"] for o in gens)
    assert res["ess"] == 1.0 / np.sum(gens[-1]["weights"] ** 2)


@pytest.mark.parametrize("name", ABC_CASES)
def test_generation_zero_is_the_rejection_sampler(abc_golden, engine, name):
    """n_prev = 0: theta, trajectories and the trial count of the reference's golden run and of abc_run; ancestors -1;
    the accepted distances are the oracle's."""
    from epipf.abc import abc_run
    rec = abc_golden["abc_" + name]
    Y, pr, n, thr = rec["Y"], priors_of(rec), int(rec["n"]), float(rec["threshold"])
    theta, traj, dist, anc, trials, acc = engine.abc_smc_generation(Y, n, thr, pr, key=int(rec["key"]),
                                                                    run_index=int(rec["f"]))
    assert acc == n and trials == int(rec["trials"])
    np.testing.assert_array_equal(theta[:, 0], rec["beta"])
    np.testing.assert_array_equal(theta[:, 1], rec["gamma"])
    np.testing.assert_array_equal(traj, rec["trajectories"])
    np.testing.assert_array_equal(anc, np.full(n, -1))
    r = abc_run(Y, n, thr, pr, key=int(rec["key"]), run_index=int(rec["f"]))
    np.testing.assert_array_equal(theta[:, 0], r["beta"])
    np.testing.assert_array_equal(traj, r["trajectories"])
    assert trials == r["trials"]
    _, _, odist, _ = oracle.abc_trials(Y, pr, int(rec["key"]), int(rec["f"]), 0, trials, rows=False)
    np.testing.assert_array_equal(dist, odist[~(odist > thr)][:n])


def test_full_run_equals_the_restatement(abc_golden, restated):
    """Four generations, every array of every generation bit for bit; the run crosses the prior box's edge (a share
    of generation 1's proposals falls outside and is counted as trials without simulation)."""
    from epipf.abc import abc_smc
    rec = abc_golden["abc_noisy_150"]
    assert restated[1]["outside"] > 0.1 * restated[1]["proposed"]
    res = abc_smc(rec["Y"], RUN["n"], RUN["thresholds"], priors_of(rec), key=RUN["key"], run_index=RUN["f"])
    assert_run_equals(res, restated)
    assert res["beta"] == [float(v) for v in restated[-1]["theta"][:, 0]]


@pytest.mark.parametrize("early", ["0", "1"])
@pytest.mark.parametrize("batch", [0, 1, 7, 100, 100000])
def test_batching_and_early_rejection_change_nothing(abc_golden, restated, monkeypatch, batch, early):
    """The same run for every batch size and with early rejection off and on.  batch = 1 is the slow pair (6-9 s):
    about 3000 trials, each a launch of its own whose one lane walks an epidemic of up to 10^4 events."""
    from epipf.abc import abc_smc
    monkeypatch.setenv("EPIPF_ABC_EARLY", early)
    rec = abc_golden["abc_noisy_150"]
    res = abc_smc(rec["Y"], RUN["n"], RUN["thresholds"], priors_of(rec), key=RUN["key"], run_index=RUN["f"],
                  batch=batch)
    assert_run_equals(res, restated)


def weight_case(rng, n, n_prev):
    prev = rng.uniform(0.0, 5.0, (n_prev, 2))
    w = rng.uniform(0.0, 1.0, n_prev)
    w /= w.sum()
    hw = np.array([0.7, 0.4])
    theta = prev[rng.randint(0, n_prev, n)] + hw * rng.uniform(-1.0, 1.0, (n, 2))
    return theta, prev, w, hw


@pytest.mark.parametrize("n,n_prev", [(1, 1), (300, 257), (300, 513), (1000, 1000)])
def test_weight_kernel_equals_the_numpy_sum(engine, n, n_prev):
    """Random populations: one point, sizes that cross a 256-lane block and one or two LDS tiles (256 points each),
    and 1000 x 1000 with random weights; a tenth of the weights are zero."""
    rng = np.random.RandomState(100 + n_prev)
    theta, prev, w, hw = weight_case(rng, n, n_prev)
    if n_prev > 1:
        w[::10] = 0.0
    den = engine.abc_smc_weights(theta, prev, w, hw)
    np.testing.assert_array_equal(den, rs.denominators(theta, prev, w, hw))


def test_weight_kernel_edges(abc_golden, engine, monkeypatch):
    """Previous points exactly one half-width away are inside (<=); the next double beyond is outside; zero-weight
    entries add nothing; a sample with nothing in range gets 0.0, which abc_smc turns into an error."""
    hw = np.array([0.5, 0.25])                                    # exact in binary, as are the coordinates below
    prev = np.array([[1.0, 1.0], [2.0, 1.0], [2.0, 1.5], [3.0, 3.0], [1.5, 1.25]])
    w = np.array([0.125, 0.25, 0.0, 0.5, 0.125])
    theta = np.array([[1.5, 1.25],                                # 0, 1 at exactly +-hw in both; 2 zero weight; 4 on it
                      [np.nextafter(1.5, 0.0), 1.25],             # loses 1 (2.0 is now beyond hw)
                      [1.5, np.nextafter(1.25, 2.0)],             # loses 0 and 1 (1.0 is beyond 0.25 below)
                      [4.5, 4.5],                                 # nothing in range
                      [3.0, 3.0]])
    den = engine.abc_smc_weights(theta, prev, w, hw)
    np.testing.assert_array_equal(den, rs.denominators(theta, prev, w, hw))
    np.testing.assert_array_equal(den, [0.5, 0.25, 0.125, 0.0, 0.5])
    from epipf import abc
    with pytest.raises(ValueError, match="denominator"):
        abc.smc_weights(den)
    # the same through abc_smc: a weight kernel result with a zero raises out of the run
    rec = abc_golden["abc_noisy_150"]
    eng_cls = type(engine)
    real = eng_cls.abc_smc_weights

    def with_a_zero(self, *a, **k):
        out = real(self, *a, **k)
        out[3] = 0.0
        return out
    monkeypatch.setattr(eng_cls, "abc_smc_weights", with_a_zero)
    with pytest.raises(ValueError, match="sample 3"):
        abc.abc_smc(rec["Y"], 16, [400.0, 300.0], priors_of(rec), key=5, run_index=0)


def test_ancestors_follow_searchsorted_right(abc_golden, engine):
    """A previous population with zero-weight members (never chosen) and hence repeated cdf values: every accepted
    trial's ancestor, theta and distance equal the restatement's, from trial 0 and from a start near 4e9."""
    rec = abc_golden["abc_noisy_150"]
    Y, pr = rec["Y"], priors_of(rec)
    rng = np.random.RandomState(3)
    prev = np.column_stack([rng.uniform(0.3, 3.0, 40), rng.uniform(0.2, 1.6, 40)])     # proposals cross the box's edge
    w = rng.uniform(0.0, 1.0, 40)
    w[[0, 3, 4, 5, 17, 38, 39]] = 0.0
    w /= w.sum()
    cdf = rs.cdf_of(w)
    assert np.sum(np.diff(cdf) == 0.0) >= 5
    hw = rs.half_width(prev)
    for t0 in (0, 4_000_000_000):
        theta, traj, dist, anc, trials, acc = engine.abc_smc_generation(Y, 200, 300.0, pr, prev, cdf, hw, key=31,
                                                                        run_index=2, t0=t0)
        o = rs.generation(Y, 200, 300.0, pr, (prev, w, hw), 31, 2, t0)
        assert acc == 200 and trials == o["trials"]
        np.testing.assert_array_equal(anc, o["ancestors"])
        np.testing.assert_array_equal(theta, o["theta"])
        np.testing.assert_array_equal(dist, o["distances"])
        np.testing.assert_array_equal(traj, o["traj"])
        assert np.all(w[anc] > 0.0)
    # every proposal of a long stretch of trials, accepted or not: a threshold every simulated trial passes
    theta, traj, dist, anc, trials, acc = engine.abc_smc_generation(Y, 3000, 1e300, pr, prev, cdf, hw, key=31,
                                                                    run_index=2, t0=123)
    j, th, inside = rs.propose(prev, cdf, hw, pr, 31, 2, 123 + np.arange(trials))
    assert acc == 3000 and inside[-1] and inside.sum() == 3000 and not inside.all()
    np.testing.assert_array_equal(anc, j[inside])
    np.testing.assert_array_equal(theta, th[inside])
    assert np.all(w[anc] > 0.0)


def test_adaptive_schedule_equals_the_explicit_run(abc_golden):
    from epipf.abc import abc_smc
    rec = abc_golden["abc_noisy_150"]
    Y, pr = rec["Y"], priors_of(rec)
    ada = abc_smc(Y, 128, [400.0], pr, quantile=0.5, generations=5, key=909, run_index=4)
    ths = [g["threshold"] for g in ada["generations"]]
    assert len(ths) == 5 and ths[0] == 400.0 and all(a > b for a, b in zip(ths, ths[1:]))
    for g in range(1, 5):
        assert ths[g] == np.sort(ada["generations"][g - 1]["distances"])[63]      # ceil(0.5 * 128) - 1
    exp = abc_smc(Y, 128, ths, pr, key=909, run_index=4)
    assert exp["total_trials"] == ada["total_trials"]
    for a, b in zip(ada["generations"], exp["generations"]):
        for k in ("theta", "weights", "distances", "ancestors", "half_width"):
            np.testing.assert_array_equal(a[k], b[k])
        assert a["trials"] == b["trials"]
    np.testing.assert_array_equal(ada["trajectories"], exp["trajectories"])


def test_short_runs_and_bad_arguments(abc_golden, engine, restated):
    from epipf._lib import EpipfError
    from epipf.abc import abc_smc
    rec = abc_golden["abc_noisy_150"]
    Y, pr = rec["Y"], priors_of(rec)
    g0, g1 = restated[0], restated[1]
    prev = (g0["theta"], rs.cdf_of(g0["weights"]), g1["half_width"])
    short = g1["trials"] - 1                                      # one trial fewer than the 64th acceptance needs
    theta, traj, dist, anc, trials, acc = engine.abc_smc_generation(Y, 64, 250.0, pr, *prev, key=RUN["key"],
                                                                    run_index=RUN["f"], t0=g0["trials"],
                                                                    max_trials=short)
    assert acc == 63 and trials == short
    np.testing.assert_array_equal(theta, g1["theta"][:63])
    with pytest.raises(RuntimeError, match="generation 1"):
        abc_smc(Y, 64, RUN["thresholds"], pr, key=RUN["key"], run_index=RUN["f"], max_trials=g0["trials"] + short)
    with pytest.raises(RuntimeError, match="generation 0"):
        abc_smc(Y, 64, [-1.0], pr, key=1, run_index=0, max_trials=1000)
    ok = dict(key=1, run_index=0, t0=0, max_trials=1000)
    th, cdf, hw = prev
    bad_cdf = cdf.copy()
    bad_cdf[10] = cdf[9] - 1e-3
    for args in ((64, np.nan, pr, th, cdf, hw), (64, 250.0, pr, th, bad_cdf, hw), (64, 250.0, pr, th, cdf * 0.5, hw),
                 (64, 250.0, pr, th, cdf, np.array([-0.1, 0.2])), (64, 250.0, pr, th, cdf, np.array([0.1, np.nan])),
                 (64, np.inf, pr, th, cdf, hw), (-1, 250.0, pr, th, cdf, hw)):
        with pytest.raises(EpipfError):
            engine.abc_smc_generation(Y, *args, **ok)
    with pytest.raises(EpipfError):                               # t0 + max_trials beyond 2^32
        engine.abc_smc_generation(Y, 4, 250.0, pr, th, cdf, hw, key=1, run_index=0, t0=2**32 - 10, max_trials=11)
    with pytest.raises(EpipfError):
        engine.abc_smc_weights(g1["theta"], th, np.full(64, -1.0), hw)
    with pytest.raises(EpipfError):
        engine.abc_smc_weights(g1["theta"], th, g0["weights"], np.array([np.inf, 0.1]))


def test_large_run_agrees_with_rejection_sampling(abc_golden):
    """N = 2000 down to threshold 100 against abc_run's rejection sample at 100 (reference-exact): the weighted means
    within 5 sd_rej sqrt(1/2000 + 1/ESS) per component; every accepted trajectory passes the acceptance rule recomputed
    on the host, every theta lies in the prior box."""
    from epipf.abc import abc_run, abc_smc, distance_function
    rec = abc_golden["abc_noisy_150"]
    Y, pr = rec["Y"], priors_of(rec)
    n = 2000
    res = abc_smc(Y, n, [400.0, 250.0, 150.0, 100.0], pr, key=2025, run_index=10)
    rej = abc_run(Y, n, 100.0, pr, key=2025, run_index=11)
    assert rej["accepted"] == n
    w = res["weights"]
    ess = 1.0 / np.sum(w * w)
    assert res["ess"] == ess and abs(w.sum() - 1.0) < 1e-9
    for c, name in enumerate(("beta", "gamma")):
        x = np.array(rej[name])
        z = (np.sum(w * np.array(res[name])) - x.mean()) / (x.std(ddof=1) * np.sqrt(1.0 / n + 1.0 / ess))
        print(f"{name}: smc {np.sum(w * np.array(res[name])):.5f} rejection {x.mean():.5f} ess {ess:.0f} z {z:.2f}")
        assert abs(z) < 5.0
    traj = res["trajectories"]
    for s in range(n):
        assert not (distance_function(traj[s, :, 2], Y[:, 1], traj[s, :, 3], Y[:, 2]) > 100.0)
    th = res["generations"][-1]["theta"]
    assert np.all((th[:, 0] >= pr["beta"][0]) & (th[:, 0] <= pr["beta"][1]))
    assert np.all((th[:, 1] >= pr["gamma"][0]) & (th[:, 1] <= pr["gamma"][1]))
    assert res["total_trials"] < rej["trials"]
    print(f"trials: smc {res['total_trials']} rejection {rej['trials']}")
