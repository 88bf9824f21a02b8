"""Iterated filtering's device paths (csrc/epipf_if2.hip) on inputs that tell right from wrong: swarms
of several blocks with distinct thetas, odd and very short series, normal observations, the segmented scan, searches
that die after completed iterations, populations of 10^6, the exact-loop fallback forced and counted, mixed rates in one
wave, and an engine larger than the call.  Every case is compared with the numpy restatement (tests/if2_restatement.py)
through test_gpu_if2.check_against / check_search; tests/test_if2_restatement.py pins on the CPU what each input contains
(tests/if2_cases.py holds them).  Needs an MI355X."""
import numpy as np
import pytest

import if2_cases as ic
import if2_restatement as rs
from test_gpu_if2 import assert_same, check_against, check_anchor, check_search, lz_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return ic.load_fixture()


def new_engine(c, chains=1, t_max=None, N=None):
    from epipf.engine import Engine
    T = c["Y"].shape[0]
    eng = Engine(c["model"], 1, c["swarm0"].shape[0] if N is None else N, T if t_max is None else t_max, chains)
    eng.set_observations(c["Y"])
    eng.set_population(c["npop"], c["mu"])
    return eng


def against(eng, c, r):
    return check_against(eng, r, c["swarm0"], c["hw"], c["probs"], c["key"], c["f"], observations=c["observations"])


def run_case(c, r):
    eng = new_engine(c)
    swarm, mean = against(eng, c, r)
    eng.close()
    return swarm, mean


def completed(r, M=2):
    assert r["status"] == 0 and r["iterations_done"] == M


# ------------------------------------------------------------------------------------------- 1. multi-block, odd T
@pytest.mark.parametrize("model,N,T", [("sir", 300, 5), ("seir", 300, 5), ("sir", 700, 3)])
def test_multi_block_swarms_at_odd_T(fx, model, N, T):
    """Five (eleven) blocks of distinct thetas, the final swarm in buffer 0, up to three trips of the finish kernel's
    stride."""
    c = ic.case(fx, model, N, T)
    r = ic.restate(c)
    completed(r)
    assert ic.distinct(r["swarm"]) == N
    run_case(c, r)


# ------------------------------------------------------------------------------------------- 2. short series
@pytest.mark.parametrize("N,T", [(70, 1), (70, 2), (70, 3), (1, 3)])
def test_short_series_with_jitter(fx, N, T):
    c = ic.case(fx, "sir", N, T)
    r = ic.restate(c)
    completed(r)
    assert ic.distinct(r["swarm"]) == N
    swarm, _ = run_case(c, r)
    if T == 1:                                           # no step kernel: the swarm is the step-0 jitter, twice
        first = rs.perturb(c["swarm0"], c["hw"][0], c["key"], c["f"], 0)
        np.testing.assert_array_equal(swarm[0], rs.perturb(first, c["hw"][1], c["key"], c["f"] + 1, 0))


# ------------------------------------------------------------------------------------------- 3. normal observations
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_normal_observations_with_jitter(fx, model):
    c = ic.case(fx, model, 130, 7, observations=True)
    r = ic.restate(c)
    completed(r)
    assert ic.distinct(r["swarm"]) == 130
    run_case(c, r)


# ------------------------------------------------------------------------------------------- 4. the segmented scan
def test_segmented_scan_with_distinct_thetas(fx):
    """N = 12,864 (201 blocks: the block sums are scanned in segments) with a theta of its own in every row."""
    c = ic.case(fx, "sir", 12864, 2, hw=rs.cooling_table(ic.RW["sir"], 0.5, 2))
    r = ic.restate(c)
    completed(r)
    assert ic.distinct(r["swarm"]) == 12864 and len(np.unique(r["ancestry"][1])) > 201
    run_case(c, r)


# ------------------------------------------------------------------------------------------- 5. late degeneracy
@pytest.fixture(scope="module")
def late(fx):
    """The four searches of ic.LATE and their restatements (shared, never modified)."""
    keys = sorted(ic.LATE)
    cases = [ic.late_case(fx, k) for k in keys]
    return keys, cases, [ic.restate(c) for c in cases]


@pytest.mark.parametrize("streams", [1, 4])
def test_searches_that_die_after_completed_iterations(late, streams):
    keys, cases, rs_ = late
    for k, r in zip(keys, rs_):
        assert (r["status"], r["iterations_done"], ic.dying_step(r)) == ic.LATE[k]
    c0 = cases[0]
    eng = new_engine(c0, chains=4)
    eng.set_streams(streams)
    swarm0 = np.array([c["swarm0"] for c in cases])
    ukeys = np.array(keys, dtype=np.uint64)
    batch = eng.if2(swarm0, c0["hw"], c0["probs"], ukeys, 0) + eng.history(4)
    assert batch[4].tolist() == [ic.LATE[k][0] for k in keys] and batch[3].tolist() == [ic.LATE[k][1] for k in keys]
    for s, r in enumerate(rs_):
        swarm, mean, lz, done, st, hid, anc = [x[s] for x in batch]
        check_search(r, swarm, mean, lz, int(done), int(st), hid, anc)
        assert np.isfinite(mean[:done]).all() and np.isfinite(lz[:done]).all()
    for s in range(4):
        solo = eng.if2(swarm0[s:s + 1], c0["hw"], c0["probs"], ukeys[s:s + 1], 0) + eng.history(1)
        dead = ic.dying_step(rs_[s])
        rows = slice(None) if dead is None else slice(0, dead)        # rows from the dying step on are never written
        assert_same([x[s:s + 1] for x in batch[:5]], solo[:5], f"search {s}")
        assert_same([x[s:s + 1, rows] for x in batch[5:]], [x[:, rows] for x in solo[5:]], f"history of search {s}")
    eng.close()


# ------------------------------------------------------------------------------------------- 6. larger populations
@pytest.fixture(scope="module")
def populations(fx):
    """Case 6's inputs and restatements by (population, observations) (shared, never modified)."""
    out = {}
    for npop, mu, T in ((10 ** 6, 400, 6), (2 * 10 ** 4, 40, 8)):
        for observations in (False, True):
            c = ic.population_case(fx, npop, mu, T, observations)
            out[npop, observations] = (c, ic.restate(c))
    return out


@pytest.mark.parametrize("npop", [10 ** 6, 2 * 10 ** 4])
@pytest.mark.parametrize("observations", [False, True])
def test_larger_populations(populations, npop, observations):
    """The certified f32 loop with per-lane rates where its bands matter: S I up to 10^10."""
    c, r = populations[npop, observations]
    completed(r)
    assert ic.distinct(r["swarm"]) > 1
    if npop == 10 ** 6:
        assert (r["hidden"][:, :, 0].astype(np.int64) * r["hidden"][:, :, 1]).max() >= 10 ** 9
    run_case(c, r)


# ------------------------------------------------------------------------------------------- 7. forced paths
# EPIPF_CLOCK_SLACK per input: from 1e10 (tests/test_gpu_lanes.py) down by factors of 100 to the first value at which
# some but not all particle-steps run the exact loop.  Beside each value: the exact particle-steps observed on an
# MI355X (at 1e10 and 1e8 every one of them for all three inputs; with no slack 0, 0 and 27).
CLOCK_SLACK = {"sir": "1e6",            # 1549 of 1560 (1e4: 399, 1e2: 7)
               "seir": "1e6",           # 1554 of 1560 (1e4: 316, 1e2: 2)
               "population": "1e2"}     # 752 of 1300 (1e6 and 1e4: all 1300)
ENVS = {"default": {}, "exact": {"EPIPF_SSA_FAST": "0"}, "clock": {"EPIPF_CLOCK_SLACK": None},
        "band": {"EPIPF_BAND_SLACK": "3000"}}


@pytest.fixture(scope="module")
def forced(fx, populations):
    """Case 7's inputs, their restatements, and the plain filter's stats on a context that never ran IF2."""
    out = {}
    for name in ("sir", "seir"):
        c = ic.case(fx, name, 130, 7)
        out[name] = [c, ic.restate(c)]
    out["population"] = list(populations[10 ** 6, True])
    for name, (c, r) in out.items():
        out[name].append(filter_stats(new_counting_engine(c), c))
    return out


def new_counting_engine(c):
    from epipf import _lib
    eng = new_engine(c)
    eng.set_profiling(_lib.PROFILE_COUNTERS)
    return eng


def filter_stats(eng, c):
    """Engine.run at the search's start theta, closing the engine: (log_zetas, status, events, resample_fallbacks)."""
    lz, st = eng.run(c["swarm0"][:1], c["probs"], c["key"], c["f"], observations=c["observations"])
    s = eng.stats()
    eng.close()
    return lz, st, s["events"], s["resample_fallbacks"]


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("name", ["sir", "seir", "population"])
def test_forced_paths_give_the_same_arrays(forced, monkeypatch, name, env):
    c, r, plain = forced[name]
    completed(r)
    for k in ("EPIPF_SSA_FAST", "EPIPF_CLOCK_SLACK", "EPIPF_BAND_SLACK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, CLOCK_SLACK[name] if v is None else v)
    eng = new_counting_engine(c)                          # EPIPF_* is read when the context is created
    against(eng, c, r)
    s = eng.stats()
    N, T = c["swarm0"].shape[0], c["Y"].shape[0]
    steps = N * (T - 1) * 2
    print(f"{name} {env}: exact particle-steps {s['ssa_exact_lanes']} of {steps}, waves {s['ssa_exact_waves']}, "
          f"events {s['events']}, lane use {s['lane_iterations']}/{s['wave_lane_slots']}")
    assert s["events"] == r["events"].sum()
    assert s["lane_iterations"] >= s["events"] and s["wave_lane_slots"] >= s["lane_iterations"]
    if env == "exact":
        assert s["ssa_exact_lanes"] == steps and s["ssa_exact_waves"] == -(-N // 64) * (T - 1) * 2
    elif env == "clock":
        assert 0 < s["ssa_exact_lanes"] < steps and s["ssa_exact_waves"] > 0
    else:
        assert 0 <= s["ssa_exact_lanes"] <= steps
    # the filter afterwards on the same context reports its own counts only
    lz, st, events, fallbacks = filter_stats(eng, c)
    assert_same((lz, st), plain[:2], "the filter after if2")
    assert (events, fallbacks) == plain[2:]


# ------------------------------------------------------------------------------------------- 8. mixed rates in a wave
@pytest.mark.parametrize("T", [2, 7])
@pytest.mark.parametrize("odd_beta", [0.0, 1e-30])
def test_mixed_rates_in_one_wave(fx, T, odd_beta):
    """Every odd row starts with beta = 0 (or 1e-30) and beta is never jittered: lanes that cannot infect beside lanes
    that can, with no knob set."""
    c = ic.mixed_case(fx, T, odd_beta)
    r = ic.restate(c)
    completed(r)
    assert set(np.unique(r["swarm"][:, 0])) <= {0.8, odd_beta}
    if T == 2:
        assert set(np.unique(r["swarm"][:, 0])) == {0.8, odd_beta}
    run_case(c, r)


@pytest.mark.parametrize("theta", [(0.0, 0.3), (0.8, 0.0), (0.0, 0.0)])
def test_zero_rates_are_the_filter(fx, theta):
    eng = new_engine(ic.case(fx, "sir", 70, 4))
    assert check_anchor(eng, "sir", theta, False, 4) == 0
    eng.close()


# ------------------------------------------------------------------------------------------- 9. a larger engine, reused
def test_engine_larger_than_the_call_and_reused(fx):
    """t_max = 15 and five chains for two searches at T = 12, then at T = 5 on the same engine, then the filter."""
    import oracle
    from epipf.engine import Engine
    starts, keys, f0 = np.array([[0.8, 0.3], [1.0, 0.4]]), np.array([101, 202], dtype=np.uint64), np.array([0, 7])
    hw = rs.cooling_table(ic.RW["sir"], 0.5, 2)
    swarm0 = np.repeat(starts[:, None, :], 65, axis=1)
    eng = Engine("sir", 1, 65, 15, 5)
    eng.set_population(fx["npop"], fx["mu"])
    for T in (12, 5):
        eng.set_observations(fx["sir"][:T])
        out = eng.if2(swarm0, hw, fx["probs"], keys, f0) + eng.history(2)
        for s in range(2):
            r = rs.run(fx["sir"][:T], "sir", swarm0[s], hw, False, fx["probs"], fx["npop"], fx["mu"], int(keys[s]), int(f0[s]))
            completed(r)
            swarm, mean, lz, done, st, hid, anc = [x[s] for x in out]
            check_search(r, swarm, mean, lz, int(done), int(st), hid, anc)
    lz, st = eng.run(starts, fx["probs"], keys, f0)
    hid, anc = eng.history(2)
    for s in range(2):
        o = oracle.particle_filter(fx["sir"][:5], "sir", tuple(starts[s]), False, fx["probs"], 65, fx["npop"], fx["mu"],
                                   key=int(keys[s]), filter_index=int(f0[s]))
        assert st[s] == o["status"] == 0
        np.testing.assert_array_equal(hid[s], o["hidden"])
        np.testing.assert_array_equal(anc[s], o["ancestry"])
        lz_close(lz[s], o["log_zetas"])
    eng.close()
