"""The subgroup models at G = 5..8 groups (30 to 72 reaction channels) on the GPU engine, against the CPU oracle: the
filter through the certified f32 event loop with its per-lane channel decision (FastSubgroupsWide), the streaming
exact loop alone (EPIPF_SSA_FAST=0), both fallbacks on purpose (widened decision band, widened clock band), simulate and
simulate_path, the routing (one lane per particle at every N: no lane-group or one-workgroup kernels for these G), the
drop-in Python names, and the reference's own output (tests/golden/wide_groups_golden.npz).  States and ancestors
bit-exact, log-likelihoods within rtol 1e-12 / atol 1e-9.  Needs an MI355X: `-m gpu`."""
import functools

import numpy as np
import pytest

import oracle
from conftest import case_args, load_golden

pytestmark = pytest.mark.gpu

KEYS, FIDX = [31, 32], [4, 9]


def _inputs(datasets_golden, model, G):
    """Inputs as tests/test_gpu_lanes.py builds them for G = 3, 4."""
    beta = np.random.RandomState(G).uniform(0.5, 3.0, (G, G))
    Y = (np.tile(datasets_golden["sub_binom"][:6, :3], (1, G)) if model == "sir_subgroups"
         else datasets_golden["sub2_binom"][:6])
    return dict(model=model, G=G, Y=np.asarray(Y, dtype=np.float64), theta=(beta, 0.7), npop=np.full(G, 1500.0),
                mu=np.full(G, 15.0))


@functools.lru_cache(maxsize=None)
def _oracle_cached(model, G, N, obs, probs, key, f, ykey):
    c = _oracle_cached.inputs[(model, G, ykey)]
    return oracle.particle_filter(c["Y"], model, c["theta"], obs, probs, N, c["npop"], c["mu"], key=key, filter_index=f)


_oracle_cached.inputs = {}


def _oracle(c, N, obs, probs, key, f):
    """The oracle's filter for a case, computed once and shared by the tests that compare against it."""
    ykey = c["Y"].tobytes()
    _oracle_cached.inputs[(c["model"], c["G"], ykey)] = c
    return _oracle_cached(c["model"], c["G"], N, obs, probs, key, f, ykey)


def _run(c, N, keys=KEYS, fidx=FIDX, obs=False, probs=0.1, lanes=None):
    from epipf.engine import Engine, model_id, theta_vector
    th, G = theta_vector(model_id(c["model"]), c["theta"])
    chains = len(keys)
    eng = Engine(c["model"], G, N, c["Y"].shape[0], chains)
    try:
        eng.set_observations(c["Y"])
        eng.set_population(c["npop"], c["mu"])
        if lanes is not None:
            eng.set_lanes(lanes)
        eng.set_profiling(True)
        lz, st = eng.run(np.repeat(th[None], chains, 0), [probs] * chains, keys, fidx, observations=obs)
        hid, anc = eng.history(chains)
        stats = eng.stats()
    finally:
        eng.close()
    return lz, st, hid, anc, stats


def _check(c, N, got, keys=KEYS, fidx=FIDX, obs=False, probs=0.1):
    lz, st, hid, anc, stats = got
    assert stats["last_lanes"] == 1 and stats["last_fused"] == 0
    for ch in range(len(keys)):
        o = _oracle(c, N, obs, probs, keys[ch], fidx[ch])
        assert int(st[ch]) == o["status"] == 0
        np.testing.assert_array_equal(hid[ch], o["hidden"])
        np.testing.assert_array_equal(anc[ch], o["ancestry"])
        np.testing.assert_allclose(lz[ch], o["log_zetas"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("G", [5, 6, 7, 8])
@pytest.mark.parametrize("model", ["sir_subgroups", "sir_subgroups2"])
def test_wide_filter_matches_oracle(datasets_golden, model, G):
    """N = 300: four full waves and a 44-lane tail; two chains with their own keys and filter indices."""
    c = _inputs(datasets_golden, model, G)
    _check(c, 300, _run(c, 300))


def test_wide_filter_normal_observations(datasets_golden):
    c = _inputs(datasets_golden, "sir_subgroups", 6)
    _check(c, 300, _run(c, 300, obs=True, probs=0.5), obs=True, probs=0.5)


@pytest.mark.parametrize("model,G,N", [("sir_subgroups", 7, 65), ("sir_subgroups2", 5, 1)])
def test_wide_filter_ragged_and_single_particle(datasets_golden, model, G, N):
    c = _inputs(datasets_golden, model, G)
    _check(c, N, _run(c, N))


@pytest.mark.parametrize("G", [5, 8])
@pytest.mark.parametrize("model", ["sir_subgroups", "sir_subgroups2"])
def test_wide_exact_loop_matches_oracle(datasets_golden, monkeypatch, model, G):
    """EPIPF_SSA_FAST=0: every particle-step on the streaming exact loop (SubgroupsStateWide, three-pass channel)."""
    monkeypatch.setenv("EPIPF_SSA_FAST", "0")
    c = _inputs(datasets_golden, model, G)
    got = _run(c, 300)
    assert got[4]["ssa_exact_lanes"] == 2 * 300 * 5          # every particle-step of steps 1..5, both chains
    _check(c, 300, got)


# EPIPF_BAND_SLACK per G: the share of unsure decisions is about 2 (NCH - 1) slack kBand (each of the NCH - 1
# boundaries is unsure over a width 2 slack kBand of the uniform), to lie between 2% and 20%:
#   G = 5: NCH = 30, kBand = 2^-17 ((2 (4 + 30) + 7) = 75 ulp -> 128 ulp of 2^-24): 2 x 29 x 128 x 2^-17 = 5.7%
#   G = 6: NCH = 42, kBand = 2^-17 ((2 (4 + 42) + 7) = 99 ulp -> 128 ulp):           2 x 41 x 128 x 2^-17 = 8.0%
#   G = 8: NCH = 72, kBand = 2^-16 ((2 (4 + 72) + 7) = 159 ulp -> 256 ulp):          2 x 71 x  32 x 2^-16 = 6.9%
BAND_SLACK = {5: "128", 6: "128", 8: "32"}


@pytest.mark.parametrize("G", [5, 6, 8])
@pytest.mark.parametrize("env", ["EPIPF_BAND_SLACK", "EPIPF_CLOCK_SLACK"])
def test_wide_fallback_paths_equal_oracle(datasets_golden, monkeypatch, env, G):
    """The f64 channel fallback on 6-8% of decisions (band slack 128 at G = 5 and 6, 32 at G = 8: the arithmetic above; the
    narrower models' 3000x would send every decision of 72 channels there), and the wave-cooperative replay of most
    particle-steps (clock band widened 1e10x, as the lane-group and one-workgroup tests widen it).  Where the f32 loop
    is routed to the exact loop (G > kWideFastMaxG = 6 as measured) the slacks have nothing to widen and
    the G = 8 cases check the exact loop under the same settings; they take the fallbacks again if that routing moves.
    G = 6 is the largest G whose particle-steps run the f32 loop.  The replays are visible in the counters (particle-steps
    handed to the exact path); the engine has no counter of f64 channel decisions, so the band case's only evidence that
    they happen is the arithmetic above."""
    monkeypatch.setenv(env, BAND_SLACK[G] if env == "EPIPF_BAND_SLACK" else "1e10")
    c = _inputs(datasets_golden, "sir_subgroups", G)
    got = _run(c, 300)
    if env == "EPIPF_CLOCK_SLACK" and G <= 6:
        # 1e10 x the clock band: essentially every particle-step that ends inside the step is replayed
        assert got[4]["ssa_exact_lanes"] > 0.5 * 2 * 300 * 5
    _check(c, 300, got)


def _sim_states(G):
    st = np.tile(np.array([1400, 20, 80], dtype=np.int32), (66, G))
    st[64, 1::3] = 0                                     # nobody infected: no event
    st[65, 1::3] = 0
    st[65, 3 * (G - 1) + 1] = 1                          # one infected, in the last group only
    return st


@pytest.mark.parametrize("max_time", [1.0, 2.5])
@pytest.mark.parametrize("G", [5, 8])
def test_wide_simulate_and_path_match_oracle(G, max_time):
    from epipf.engine import Engine
    theta = (np.random.RandomState(G).uniform(0.5, 3.0, (G, G)), 0.7)
    states = _sim_states(G)
    eng = Engine("sir_subgroups", G, 1, 1, 1)
    try:
        out, ev = eng.simulate(states, theta, max_time, key=77, filter_index=5, step=3)
        t, x, n, fin = eng.simulate_path(states, theta, max_time, key=77, filter_index=5, step=3)
    finally:
        eng.close()
    oout, oev = oracle.simulate("sir_subgroups", states, theta, max_time, key=77, filter_index=5, step=3)
    np.testing.assert_array_equal(out, oout)
    assert ev == oev
    ot, ox, on, ofin = oracle.simulate_path("sir_subgroups", states, theta, max_time, key=77, filter_index=5, step=3)
    np.testing.assert_array_equal(n, on)
    assert int(n[64]) == 0 and int(n.sum()) == oev
    np.testing.assert_array_equal(fin, ofin)
    np.testing.assert_array_equal(fin, oout)
    for j in range(states.shape[0]):
        k = int(n[j])
        np.testing.assert_array_equal(t[j, :k], ot[j, :k])           # event times bit-equal
        np.testing.assert_array_equal(x[j, :k], ox[j, :k])


@pytest.mark.parametrize("N", [300, 64])
def test_wide_runs_take_the_one_lane_step_kernels(datasets_golden, N):
    """N = 64 is the one-workgroup filter's territory and N = 300 the lane groups': G = 6 takes neither."""
    c = _inputs(datasets_golden, "sir_subgroups", 6)
    got = _run(c, N, keys=[5], fidx=[2])
    assert got[4]["last_fused"] == 0 and got[4]["last_lanes"] == 1
    _check(c, N, got, keys=[5], fidx=[2])


def test_wide_context_refuses_lane_groups(datasets_golden):
    from epipf import _lib
    from epipf.engine import Engine
    eng = Engine("sir_subgroups", 6, 64, 6, 1)
    try:
        with pytest.raises(_lib.EpipfError, match=r"G=6.*lane groups exist for G <= 4"):
            eng.set_lanes(8)
        eng.set_lanes(1)
        eng.set_lanes(0)
    finally:
        eng.close()


def test_four_groups_at_fused_size_still_equal_oracle(datasets_golden):
    """G = 4 at N = 64 may still take the one-workgroup filter: only that it runs and equals the oracle."""
    from epipf.engine import Engine, model_id, theta_vector
    c = _inputs(datasets_golden, "sir_subgroups", 4)
    th, G = theta_vector(model_id("sir_subgroups"), c["theta"])
    eng = Engine("sir_subgroups", G, 64, 6, 1)
    try:
        eng.set_observations(c["Y"])
        eng.set_population(c["npop"], c["mu"])
        lz, st = eng.run(th[None], [0.1], [5], [2])
        hid, anc = eng.history(1)
    finally:
        eng.close()
    o = _oracle(c, 64, False, 0.1, 5, 2)
    assert int(st[0]) == o["status"] == 0
    np.testing.assert_array_equal(hid[0], o["hidden"])
    np.testing.assert_array_equal(anc[0], o["ancestry"])
    np.testing.assert_allclose(lz[0], o["log_zetas"], rtol=1e-12, atol=1e-9)


def test_wide_drop_in_surface(datasets_golden, monkeypatch):
    """particle_filter and a 3-iteration particle_mcmc at G = 5 through epipf.pmcmc's names: the filter against the
    oracle, the MH run against the same call on the CPU stand-in engine (tests/oracle_engine.py)."""
    from epipf import pmcmc as pm
    from epipf.engine import release_engines
    from oracle_engine import fake_get_engine
    c = _inputs(datasets_golden, "sir_subgroups", 5)
    z, hid, anc = pm.particle_filter(c["Y"], pm.ModelType.SIR_SUBGROUPS, c["theta"], False, 0.1, 128, c["npop"],
                                     c["mu"], key=21, filter_index=3)
    o = _oracle(c, 128, False, 0.1, 21, 3)
    np.testing.assert_array_equal(hid, o["hidden"])
    np.testing.assert_array_equal(anc, o["ancestry"])
    np.testing.assert_allclose(np.log(z), o["log_zetas"], rtol=1e-12, atol=1e-9)
    params = list(c["theta"][0].reshape(-1)) + [c["theta"][1]]

    def mcmc():
        np.random.seed(11)
        pm.seed_stream(55, 0)
        return pm.particle_mcmc(c["Y"], pm.ModelType.SIR_SUBGROUPS, params, 0.01, False, None, 3, False, 0.1, 64,
                                c["npop"], c["mu"], progress=False, prefetch=0)

    gpu = mcmc()
    release_engines()
    monkeypatch.setattr(pm, "get_engine", fake_get_engine)
    cpu = mcmc()
    np.testing.assert_array_equal(gpu[0], cpu[0])
    # likelihoods = exp(log zeta): the parity bound on the logs (1e-9 absolute, 1e-12 relative at |log| ~ 100)
    np.testing.assert_allclose(gpu[1], cpu[1], rtol=2e-9)
    np.testing.assert_array_equal(gpu[2], cpu[2])


@pytest.mark.parametrize("case", ["wide_sir_subgroups_g6", "wide_sir_subgroups2_g5", "wide_sir_subgroups_g8"])
def test_wide_filter_equals_the_reference_fixture(case):
    """The device against the unmodified reference's own output (tests/golden/make_golden_wide.py)."""
    from epipf.engine import Engine, model_id, theta_vector
    a = case_args(load_golden("wide_groups_golden.npz")[case])
    rec = load_golden("wide_groups_golden.npz")[case]
    th, G = theta_vector(model_id(a["model"]), a["theta"])
    eng = Engine(a["model"], G, a["N"], a["Y"].shape[0], 1)
    try:
        eng.set_observations(a["Y"])
        eng.set_population(a["npop"], a["mu"])
        lz, st = eng.run(th[None], [a["probs"]], [a["key"]], [a["f"]])
        hid, anc = eng.history(1)
    finally:
        eng.close()
    assert int(st[0]) == 0
    np.testing.assert_array_equal(hid[0], rec["hidden"])
    np.testing.assert_array_equal(anc[0], rec["ancestry"])
    # the reference's weights are scipy's Boost pmf, the device's the compensated closed form: the parity tests' bound
    np.testing.assert_allclose(lz[0], np.log(rec["zetas"]), rtol=1e-12, atol=1e-9)
