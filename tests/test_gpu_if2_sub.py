"""Iterated filtering of the subgroup models on the GPU (epipf_iterated_filtering_subgroups through
Engine.if2_subgroups, epipf.if2_subgroups on top; csrc/epipf_if2_sub.hip): anchored to the existing
filter (no jitter: Engine.run bit for bit), against the numpy restatement (tests/if2_sub_restatement.py) with jitter,
reflection and fixed components, batch independence, continuation, degeneracy, the SSA paths and their counters, the
argument errors, and the search end to end on the G = 2 fixture.  tests/test_if2_sub_restatement.py pins on the CPU what
each input (tests/if2_sub_cases.py) contains.  Needs an MI355X."""
import numpy as np
import pytest

import if2_restatement as rs
import if2_sub_cases as sc
import if2_sub_restatement as srs
from test_gpu_if2 import assert_same, check_search, lz_close, mean_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return sc.load_fixture()


def new_engine(c, chains=1, N=None):
    from epipf.engine import Engine
    eng = Engine(c["model"], c["G"], c["swarm0"].shape[0] if N is None else N, max(c["Y"].shape[0], 1), chains)
    eng.set_observations(c["Y"])
    eng.set_population(c["npop"], c["mu"])
    return eng


def against(eng, c, r):
    swarm, mean, lz, done, st = eng.if2_subgroups(c["swarm0"][None], c["hw"], c["probs"], c["key"], c["f"],
                                                  observations=c["observations"])
    hid, anc = eng.history(1)
    check_search(r, swarm[0], mean[0], lz[0], int(done[0]), int(st[0]), hid[0], anc[0])
    return swarm, mean


def run_case(c, r):
    eng = new_engine(c)
    swarm, mean = against(eng, c, r)
    eng.close()
    return swarm, mean


# ------------------------------------------------------------------------------------------- 1. the anchor
def check_anchor(eng, c):
    """One iteration with zero half-widths from a swarm of equal theta is Engine.run at the same key and filter index."""
    N, d = c["swarm0"].shape
    obs = c["observations"]
    lz, st = eng.run(c["swarm0"][:1], c["probs"], c["key"], c["f"], observations=obs)
    hid, anc = eng.history(1)
    swarm, mean, ilz, done, ist = eng.if2_subgroups(c["swarm0"][None], np.zeros((1, d)), c["probs"], c["key"], c["f"],
                                                    observations=obs)
    ihid, ianc = eng.history(1)
    assert ist[0] == st[0]
    np.testing.assert_array_equal(swarm[0], c["swarm0"])
    if st[0] == 0:
        assert done[0] == 1
        np.testing.assert_array_equal(ihid, hid)
        np.testing.assert_array_equal(ianc, anc)
        lz_close(ilz[0, 0], lz[0])
        mean_close(mean[0, 0], swarm[0])
        np.testing.assert_array_equal(mean[0, 0], rs.device_mean(swarm[0]))
    else:                                                # both die at the same step; the rows before it agree
        dead = int(np.argmax(np.isneginf(lz[0])))
        assert done[0] == 0 and np.isnan(mean).all() and np.isnan(ilz).all()
        np.testing.assert_array_equal(ihid[0, :dead], hid[0, :dead])
        np.testing.assert_array_equal(ianc[0, :dead], anc[0, :dead])
    return st[0]


# (model, observations, G, N): how many of the T = 1, 2, 12 series complete on the oracle, where not all three
DYING = {("sir_subgroups", False, 2, 1): 2, ("sir_subgroups", False, 3, 1): 2, ("sir_subgroups", False, 4, 1): 1,
         ("sir_subgroups", True, 3, 1): 2, ("sir_subgroups", True, 4, 1): 2, ("sir_subgroups2", False, 4, 1): 2}


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("G", sc.GROUPS)
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", sc.MODELS)
def test_no_jitter_is_the_filter(fx, model, observations, G, N):
    ok = 0
    for T in (1, 2, 12):
        c = sc.case(fx, model, G, N, T, observations=observations)
        eng = new_engine(c)
        ok += check_anchor(eng, c) == 0
        eng.close()
    # every case completes on the oracle but these at N = 1, whose one particle dies (the dying path)
    assert ok == DYING.get((model, observations, G, N), 3)


def test_no_jitter_is_the_filter_on_the_segmented_scan(fx):
    """N = 12,864: 201 blocks, the first size whose block sums are scanned in segments."""
    c = sc.case(fx, "sir_subgroups", 2, 12864, 3)
    eng = new_engine(c)
    assert check_anchor(eng, c) == 0
    eng.close()


# ------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("G", sc.GROUPS)
@pytest.mark.parametrize("model", sc.MODELS)
def test_equals_the_restatement(fx, model, G):
    """N = 65, T = 12, M = 3 with jitter on: swarm, hidden, ancestry and iterations_done bit for bit, log_zetas to
    1e-9, the means bit for bit in the finish kernel's order."""
    c = sc.parity_case(fx, model, G)
    r = sc.restate(c)
    assert r["status"] == 0 and r["iterations_done"] == 3
    swarm, _ = run_case(c, r)
    assert sc.distinct(swarm[0]) > 1                     # the jitter and the selection did something


# ------------------------------------------------------------------------------------------- 3. reflection
def test_reflection_equals_the_restatement(fx):
    """A start of 0.01 with half-width 0.05 on every component: reflected at 0, never negative, the restatement's bits."""
    c = sc.reflection_case(fx)
    r = sc.restate(c)
    assert r["reflections"] >= 1 and r["status"] == 0 and r["iterations_done"] == 2
    swarm, _ = run_case(c, r)
    assert (swarm >= 0.0).all()


# ------------------------------------------------------------------------------------------- 4. fixed components
@pytest.mark.parametrize("model", sc.MODELS)
def test_fixed_components_come_back_bit_identical(fx, model):
    """Off-diagonal contacts with half-width 0, zero in the even rows and 0.3 in the odd ones: lanes with zero and
    non-zero rates in one wave.  The fixed components keep their bits, the rest is the restatement's."""
    c = sc.fixed_case(fx, model)
    r = sc.restate(c)
    assert r["status"] == 0 and r["iterations_done"] == 2
    swarm, _ = run_case(c, r)
    off = swarm[0][:, 1:3]
    assert set(np.unique(off)) == {0.0, 0.3} and (off[:, 0] == off[:, 1]).all()


# ------------------------------------------------------------------------------------------- 5. batching
def results(eng, swarm, hw, probs, keys, f0):
    out = eng.if2_subgroups(swarm, hw, probs, keys, f0)
    return out + eng.history(len(swarm))


@pytest.mark.parametrize("streams", [1, 3])
def test_searches_in_a_batch_equal_the_searches_alone(fx, streams):
    cases = sc.batch_cases(fx)
    eng = new_engine(cases[0], chains=3)
    eng.set_streams(streams)
    hw, probs = cases[0]["hw"], cases[0]["probs"]
    swarm0 = np.array([c["swarm0"] for c in cases])
    solo = [results(eng, swarm0[s:s + 1], hw, probs, sc.KEYS[s:s + 1], sc.F0[s:s + 1]) for s in range(3)]
    batch = results(eng, swarm0, hw, probs, sc.KEYS, sc.F0)
    assert (batch[4] == 0).all() and (batch[3] == 2).all()
    for s in range(3):
        assert_same([x[s:s + 1] for x in batch], solo[s], f"search {s}")
    # and the last search, whose second iteration wraps to filter index 0, is the restatement's
    swarm, mean, lz, done, st, hid, anc = [x[2] for x in batch]
    check_search(sc.restate(cases[2]), swarm, mean, lz, int(done), int(st), hid, anc)
    eng.close()


def test_three_iterations_equal_one_then_two(fx):
    c = sc.batch_cases(fx, 3)[1]
    eng = new_engine(c)
    swarm0, hw = c["swarm0"][None], c["hw"]
    whole = results(eng, swarm0, hw, c["probs"], c["key"], c["f"])
    first = eng.if2_subgroups(swarm0, hw[:1], c["probs"], c["key"], c["f"])
    rest = results(eng, first[0], hw[1:], c["probs"], c["key"], c["f"] + 1)
    np.testing.assert_array_equal(rest[0], whole[0])
    np.testing.assert_array_equal(np.concatenate([first[1], rest[1]], axis=1), whole[1])
    np.testing.assert_array_equal(np.concatenate([first[2], rest[2]], axis=1), whole[2])
    assert first[3][0] + rest[3][0] == whole[3][0] == 3
    assert_same(rest[5:], whole[5:], "history of the last iteration")
    eng.close()


def test_a_degenerate_search_between_two_good_ones(fx):
    cases = sc.degenerate_cases(fx)
    eng = new_engine(cases[0], chains=3)
    swarm0 = np.array([c["swarm0"] for c in cases])
    keys = np.array([c["key"] for c in cases], dtype=np.uint64)
    hw, probs = cases[0]["hw"], cases[0]["probs"]
    swarm, mean, lz, done, st = eng.if2_subgroups(swarm0, hw, probs, keys, 0)
    assert st.tolist() == [0, 1, 0] and done.tolist() == [3, 0, 3]
    np.testing.assert_array_equal(swarm[1], swarm0[1])
    assert np.isnan(mean[1]).all() and np.isnan(lz[1]).all()
    assert np.isfinite(mean[[0, 2]]).all() and np.isfinite(lz[[0, 2]]).all()
    for s in (0, 2):
        solo = eng.if2_subgroups(swarm0[s:s + 1], hw, probs, keys[s:s + 1], 0)
        assert_same([swarm[s:s + 1], mean[s:s + 1], lz[s:s + 1], done[s:s + 1], st[s:s + 1]], solo, f"search {s}")
    eng.close()


# ------------------------------------------------------------------------------------------- 6. paths
# EPIPF_CLOCK_SLACK: chosen as tests/test_gpu_if2_paths.py chooses its values, the first of 1e8, 1e6, 1e4, ... at which
# some but not all particle-steps run the exact loop.  Observed on an MI355X for the three inputs below, of 1560
# particle-steps: 1e6 and 1e8 all of them; 1e4: 413, 642, 787; 1e2: 5, 2, 7; no slack: 0, 0, 0.
ENVS = {"default": {}, "exact": {"EPIPF_SSA_FAST": "0"}, "clock": {"EPIPF_CLOCK_SLACK": "1e4"}}


@pytest.fixture(scope="module")
def path_restated(fx):
    """The path cases and their restatements (shared, never modified)."""
    out = {}
    for model, G in (("sir_subgroups", 2), ("sir_subgroups2", 3), ("sir_subgroups", 4)):
        c = sc.path_case(fx, model, G)
        out[model, G] = (c, sc.restate(c))
    return out


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("model,G", [("sir_subgroups", 2), ("sir_subgroups2", 3), ("sir_subgroups", 4)])
def test_forced_paths_give_the_same_arrays(path_restated, monkeypatch, model, G, env):
    from epipf import _lib
    c, r = path_restated[model, G]
    assert r["status"] == 0 and r["iterations_done"] == 2
    for k in ("EPIPF_SSA_FAST", "EPIPF_CLOCK_SLACK", "EPIPF_BAND_SLACK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    eng = new_engine(c)                                  # EPIPF_* is read when the context is created
    eng.set_profiling(_lib.PROFILE_COUNTERS)
    against(eng, c, r)
    s = eng.stats()
    N, T = c["swarm0"].shape[0], c["Y"].shape[0]
    steps = N * (T - 1) * 2
    print(f"{model} G={G} {env}: exact particle-steps {s['ssa_exact_lanes']} of {steps}, waves {s['ssa_exact_waves']}, "
          f"events {s['events']}, lane use {s['lane_iterations']}/{s['wave_lane_slots']}, "
          f"resample fallbacks {s['resample_fallbacks']}")
    assert s["events"] == r["events"].sum()
    assert s["lane_iterations"] >= s["events"] and s["wave_lane_slots"] >= s["lane_iterations"]
    assert s["resample_fallbacks"] >= 0
    if env == "exact":
        assert s["ssa_exact_lanes"] == steps and s["ssa_exact_waves"] == -(-N // 64) * (T - 1) * 2
    elif env == "clock":
        assert 0 < s["ssa_exact_lanes"] < steps and s["ssa_exact_waves"] > 0
    else:
        assert 0 <= s["ssa_exact_lanes"] <= steps
    eng.close()


# ------------------------------------------------------------------------------------------- 7. argument errors
def raw(eng, S, M, swarm, d, hw):
    from epipf import _lib
    from epipf._lib import ptr
    swarm = np.ascontiguousarray(swarm, dtype=np.float64)
    hw = np.ascontiguousarray(hw, dtype=np.float64)
    n = max(S, 1)
    probs, keys, f0 = np.full(n, 0.5), np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    mean = np.zeros((n, max(M, 1), max(d, 1)))
    done, st = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rc = eng._L.epipf_iterated_filtering_subgroups(eng._h, S, M, ptr(swarm), d, ptr(hw), _lib.OBS_BINOMIAL, ptr(probs),
                                                   ptr(keys), ptr(f0), None, ptr(mean), ptr(done), ptr(st))
    return rc, eng._L.epipf_last_error().decode()


def test_argument_errors_leave_the_context_usable(fx):
    import oracle
    from epipf import _lib
    from epipf.engine import Engine
    N, T = 32, 8
    g = fx[2]
    theta = g["theta"]
    good_swarm, good_hw = np.tile(theta, (2, N, 1)), np.full((2, 5), 0.01)
    eng = Engine("sir_subgroups", 2, N, T, 2)
    for ready in (lambda: None, lambda: eng.set_observations(g["sir_subgroups"][:T])):   # before the data, then the population
        ready()
        rc, msg = raw(eng, 2, 2, good_swarm, 5, good_hw)
        assert rc == _lib.ESTATE and msg
    eng.set_population(g["npop"], g["mu"])

    def bad(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    cases = {
        "wrong d": (2, 2, np.tile(theta[:4], (2, N, 1)), 4, np.full((2, 4), 0.01)),
        "d of three groups": (2, 2, np.tile(np.resize(theta, 10), (2, N, 1)), 10, np.full((2, 10), 0.01)),
        "too many searches": (3, 2, np.tile(theta, (3, N, 1)), 5, good_hw),
        "no searches": (0, 2, good_swarm, 5, good_hw),
        "no iterations": (2, 0, good_swarm, 5, good_hw),
        "negative half-width": (2, 2, good_swarm, 5, bad(good_hw, (1, 0), -0.01)),
        "NaN half-width": (2, 2, good_swarm, 5, bad(good_hw, (0, 4), np.nan)),
        "negative swarm entry": (2, 2, bad(good_swarm, (1, 5, 0), -0.5), 5, good_hw),
        "NaN swarm entry": (2, 2, bad(good_swarm, (0, 31, 4), np.nan), 5, good_hw),
    }
    for name, args in cases.items():
        rc, msg = raw(eng, *args)
        assert rc == _lib.EINVAL and msg, name
    sir = Engine("sir", 1, N, T, 2)
    rc, msg = raw(sir, 2, 2, np.tile([0.8, 0.3], (2, N, 1)), 2, np.full((2, 2), 0.01))
    assert rc == _lib.EINVAL and "epipf_if2" in msg
    sir.close()
    wide = Engine("sir_subgroups", 5, N, T, 2)
    rc, msg = raw(wide, 2, 2, np.full((2, N, 26), 0.5), 26, np.full((2, 26), 0.01))
    assert rc == _lib.EINVAL and "G <= 4" in msg
    wide.close()
    # the context still runs its usual filter
    lz, st = eng.run(theta[None], 0.5, sc.KEY, sc.F)
    hid, anc = eng.history(1)
    o = oracle.particle_filter(g["sir_subgroups"][:T], "sir_subgroups", srs.to_pair(theta), False, 0.5, N, g["npop"],
                               g["mu"], key=sc.KEY, filter_index=sc.F)
    assert st[0] == o["status"] == 0
    np.testing.assert_array_equal(hid[0], o["hidden"])
    np.testing.assert_array_equal(anc[0], o["ancestry"])
    lz_close(lz[0], o["log_zetas"])
    # and, after a good call, again
    assert eng.if2_subgroups(good_swarm, good_hw, 0.5, [1, 2], 0)[4].tolist() == [0, 0]
    lz2, st2 = eng.run(theta[None], 0.5, sc.KEY, sc.F)
    assert st2[0] == 0
    np.testing.assert_array_equal(lz2, lz)
    assert_same(eng.history(1), (hid, anc), "history after if2_subgroups, then run")
    eng.close()


# ------------------------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("model", sc.MODELS)
def test_the_search_finds_the_peak(fx, model):
    """Two searches of 12 iterations with 48 particles on the G = 2 fixture from (1.6, 0.6, 0.6, 1.4, 0.55), 30-40 % off
    the truth.  On the CPU restatement (tests/test_if2_sub_restatement.py) the start scores -113.10 (sir_subgroups) /
    -115.97 (sir_subgroups2), and the searches gain 25.74 and 14.91 / 35.38 and 30.67 log units (the truth scores -87.24 /
    -81.92).  Asserted: every search gains at least half the smaller of its model's two gains (7.45 / 15.33)."""
    import epipf
    s, g = sc.SEARCH, fx[2]
    epipf.seed_stream(sc.SEARCH_KEY, 0)
    res = epipf.if2_subgroups(g[model], model, s["start"], s["rw"], iterations=s["M"], cooling=s["cooling"],
                              n_particles=s["N"], n_population=g["npop"], mu=g["mu"], probs=fx["probs"],
                              searches=sc.SEARCHES, evaluate=True)
    assert res.status.tolist() == [0] * sc.SEARCHES and res.iterations_done.tolist() == [s["M"]] * sc.SEARCHES
    r = sc.restate(sc.search_case(fx, model, 0))
    np.testing.assert_array_equal(res.swarm[0], r["swarm"])
    np.testing.assert_array_equal(res.theta[0], rs.device_mean(r["swarm"]))
    lz_close(res.loglik[0], r["loglik"])
    assert res.beta.shape == (sc.SEARCHES, 2, 2) and res.best == int(np.argmax(res.loglik_at_theta))
    gains = res.loglik_at_theta - sc.START_SCORE[model]
    print(f"{model}: theta {res.theta.tolist()}, loglik_at_theta {res.loglik_at_theta.tolist()}, gains {gains.tolist()}, "
          f"CPU gains {sc.cpu_gains(model)}")
    assert (gains >= 0.5 * min(sc.cpu_gains(model))).all()
    # the best theta is particle_mcmc's flat start point as it stands
    np.random.seed(3)
    th, lk, _ = epipf.particle_mcmc(g[model], model, list(res.theta[res.best]), 0.01, n_chains=5, probs=fx["probs"],
                                    n_particles=s["N"], n_population=g["npop"], mu=g["mu"], progress=False, prefetch=0)
    assert len(lk) > 0 and np.isfinite(np.asarray(lk, dtype=np.float64)).all() and np.isfinite(np.asarray(th)).all()
