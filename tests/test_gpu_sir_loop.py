"""The one-lane SIR event loop (fast_propagate_sir, csrc/epipf_device.hpp: D = 2S state, sign-bit channel, one exit
compare per event) against the CPU oracle, bit for bit: states, ancestry, log-likelihoods.  Small shapes around the
wave size, both observation models, the step launches and the one-workgroup filter (both inline the loop); the
channel's exact fallback, the overshoot undo and the hand-back to the exact loop on purpose (widened bands); start
states that end the loop at once or never enter it; and populations on both sides of 2^23 (D = 2S reaches 2^24
there), the largest the loop takes (2^24 - 1) and one it must leave to the exact loop.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 130]
T = 6
# (EPIPF_BAND_SLACK, EPIPF_CLOCK_SLACK): the f64 channel overwriting s for ~1% of events; a clock band 300x wider
# (some lanes undo an overshoot, some hand back) and 1e10x wider (every lane hands its step back)
SLACKS = [(None, None), ("3000", None), (None, "300"), ("3000", "1e10")]


def _case(datasets_golden, obs):
    if obs:
        return dict(Y=datasets_golden["sir_noisy"][:T], theta=(2.1, 0.9), obs=True, probs=0.5, npop=4820, mu=20)
    return dict(Y=datasets_golden["sir_binom"][:T], theta=(2.0, 1.0), obs=False, probs=0.1, npop=4820, mu=20)


def _env(monkeypatch, path, band=None, clock=None, fast=None):
    """Settings read when the engine is created.  path: "step" (the step launches, one lane per particle) or "fused"
    (the one-workgroup filter, one lane per particle)."""
    monkeypatch.setenv("EPIPF_FUSED", "1" if path == "fused" else "0")
    if path == "fused":
        monkeypatch.setenv("EPIPF_FUSED_LANES", "1")
    for k, v in (("EPIPF_BAND_SLACK", band), ("EPIPF_CLOCK_SLACK", clock), ("EPIPF_SSA_FAST", fast)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _filter(c, N, path, keys, fidx):
    from epipf.engine import Engine
    chains = len(keys)
    th = np.asarray(c["theta"], dtype=np.float64)
    eng = Engine("sir", 1, N, c["Y"].shape[0], chains)
    try:
        eng.set_observations(c["Y"])
        eng.set_population(c["npop"], c["mu"])
        if path == "step":
            eng.set_lanes(1)
        eng.set_profiling(2)
        lz, st = eng.run(np.repeat(th[None], chains, 0), [c["probs"]] * chains, keys, fidx, observations=c["obs"])
        hid, anc = eng.history(chains)
        return lz, st, hid, anc, eng.stats()
    finally:
        eng.close()


_ORACLE = {}


def _oracle(tag, c, N, key, f):
    """One oracle run per (case, N, key): shared by the tests, never modified."""
    k = (tag, N, key, f)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.particle_filter(c["Y"], "sir", c["theta"], c["obs"], c["probs"], N, c["npop"], c["mu"],
                                            key=key, filter_index=f)
    return _ORACLE[k]


def _check(tag, c, N, out, keys, fidx):
    lz, st, hid, anc, _ = out
    for ch in range(len(keys)):
        o = _oracle(tag, c, N, keys[ch], fidx[ch])
        assert int(st[ch]) == o["status"]
        if o["status"]:
            continue
        np.testing.assert_array_equal(hid[ch], o["hidden"])
        np.testing.assert_array_equal(anc[ch], o["ancestry"])
        np.testing.assert_allclose(lz[ch], o["log_zetas"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("path", ["step", "fused"])
def test_sir_filter_matches_oracle(datasets_golden, monkeypatch, path, N, obs, slack):
    _env(monkeypatch, path, band=slack[0], clock=slack[1])
    c = _case(datasets_golden, obs)
    keys, fidx = [61, 62], [2, 7]
    out = _filter(c, N, path, keys, fidx)
    _check(("golden", obs), c, N, out, keys, fidx)
    s = out[4]
    if slack[1] == "1e10" and N >= 63 and path == "step":
        assert s["ssa_exact_lanes"] > 0.5 * s["particle_steps"]        # the hand-back ran


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_fast_loop_on_equals_off(datasets_golden, monkeypatch, N, obs):
    """EPIPF_SSA_FAST=0 (every particle-step on the exact loop) against 1 on the same inputs: equal arrays."""
    c = _case(datasets_golden, obs)
    keys, fidx = [5, 6], [1, 4]
    outs = []
    for fast in ("1", "0"):
        _env(monkeypatch, "step", fast=fast)
        outs.append(_filter(c, N, "step", keys, fidx))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        np.testing.assert_array_equal(a, b)
    assert outs[0][4]["events"] == outs[1][4]["events"]


def _edge_states():
    """Start states for the SSA alone (the filter draws its own start from a Poisson law): S = 0 (recoveries only),
    I = 1 (often extinct after one event), I = 0 (the loop is never entered), and ordinary ones between them, so that
    lanes of one wave leave the loop at different events."""
    rows = []
    for k in range(130):
        m = k % 5
        if m == 0:
            rows.append((0, 1 + k, 10))
        elif m == 1:
            rows.append((50 + k, 1, 0))
        elif m == 2:
            rows.append((300 + k, 0, 7))
        elif m == 3:
            rows.append((0, 1, k))
        else:
            rows.append((400 - k, 30 + k, k))
    return np.array(rows, dtype=np.int32)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("n", SIZES)
def test_ssa_from_edge_states_matches_oracle(monkeypatch, n, slack):
    from epipf.engine import Engine
    _env(monkeypatch, "step", band=slack[0], clock=slack[1])
    states = _edge_states()[:n]
    theta = (1.5, 0.7)
    eng = Engine("sir", 1, 64, 2, 1)
    try:
        for step in (0, 3):
            got, nev = eng.simulate(states, theta, 1.0, key=91, filter_index=5, step=step)
            ref, ref_nev = oracle.simulate("sir", states, theta, 1.0, key=91, filter_index=5, step=step)
            np.testing.assert_array_equal(got, ref)
            assert nev == ref_nev
            never = states[:, 1] == 0
            np.testing.assert_array_equal(got[never], states[never])    # I = 0: nothing happens
            only_rec = states[:, 0] == 0
            assert np.all(got[only_rec, 0] == 0)                        # S = 0: recoveries only
    finally:
        eng.close()


# populations around the loop's exactness conditions: D = 2S is below 2^24 for the first, at or above it for the
# next two (even integers below 2^25 are exact in f32; an odd D - 1 above 2^24 would not be), the third the largest
# population the f32 loop takes, the last one it must refuse (population >= 2^24: the exact loop)
POPULATIONS = [2 ** 23 - 3, 12000001, 2 ** 24 - 1, 2 ** 24 + 5]


def _big_case(npop):
    """Normal observations (no log-factorial table), Y the states of one oracle trajectory; rates and mu small
    enough that a step has tens of events (total rate ~ (beta + gamma) I, I ~ 20)."""
    theta, mu = (0.8, 0.6), 20
    x = np.array([[npop - mu, mu, 0]], dtype=np.int32)
    Y = [x[0].astype(np.float64)]
    for p in range(1, T):
        x = oracle.simulate("sir", x, theta, 1.0, key=1234, filter_index=0, step=p)[0]
        Y.append(x[0].astype(np.float64))
    return dict(Y=np.array(Y), theta=theta, obs=True, probs=0.9, npop=float(npop), mu=float(mu))


@pytest.mark.parametrize("slack", [(None, None), ("3000", "300")])
@pytest.mark.parametrize("npop", POPULATIONS)
def test_populations_around_two_to_the_23_and_24(monkeypatch, npop, slack):
    _env(monkeypatch, "step", band=slack[0], clock=slack[1])
    c = _big_case(npop)
    keys, fidx = [17], [0]
    out = _filter(c, 64, "step", keys, fidx)
    o = _oracle(("big", npop), c, 64, keys[0], fidx[0])
    steps = 64 * (T - 1)
    assert o["status"] == 0 and 10 * steps < o["events"] < 1000 * steps   # tens of events per particle-step
    _check(("big", npop), c, 64, out, keys, fidx)
    s = out[4]
    if npop >= 2 ** 24:
        assert s["ssa_exact_lanes"] >= steps                           # every particle-step: the exact loop
    elif slack[1] is None:
        assert s["ssa_exact_lanes"] < 0.05 * steps                     # the f32 loop took them
