"""The one-lane SIR event loop with its Philox words formed where they are read (fast_propagate_sir,
csrc/epipf_device.hpp: y and w on every event, z in the f64 channel's block, x / ~x in the two small-x log blocks)
against the CPU oracle, bit for bit: states, ancestry, log-likelihoods.  Sizes around the row (16) and wave (64) sizes,
both observation models, the step launches and the one-workgroup filter; widened bands send ~1% of events through the
lazily formed z, and 0.4% of all events read ~x (1 - U < 2^-8); one case whose key provably holds a draw with
1 - U < 2^-20 (tiny_log2, which reads x); and the float64 bit patterns of log_zeta against a fixture recorded before
the loop changed (tests/golden/lazy_philox_log_zeta.npz): the order of the scans' additions, which certified ancestors
would not show.  Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import oracle
import philox

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 63, 64, 65, 130]
T = 6
# (EPIPF_BAND_SLACK, EPIPF_CLOCK_SLACK), as tests/test_gpu_sir_loop.py: the f64 channel (z) for ~1% of events; a clock
# band 300x wider (undone overshoots, some hand-backs); every lane handing its step back
SLACKS = [(None, None), ("3000", None), (None, "300"), ("3000", "1e10")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lazy_philox_log_zeta.npz")


def _case(datasets_golden, obs, t=T):
    if obs:
        return dict(Y=datasets_golden["sir_noisy"][:t], theta=(2.1, 0.9), obs=True, probs=0.5, npop=4820, mu=20)
    return dict(Y=datasets_golden["sir_binom"][:t], theta=(2.0, 1.0), obs=False, probs=0.1, npop=4820, mu=20)


def _env(monkeypatch, path, band=None, clock=None):
    """Settings read when the engine is created.  path: "step" (the step launches, one lane per particle) or "fused"
    (the one-workgroup filter, one lane per particle)."""
    monkeypatch.setenv("EPIPF_FUSED", "1" if path == "fused" else "0")
    if path == "fused":
        monkeypatch.setenv("EPIPF_FUSED_LANES", "1")
    else:
        monkeypatch.delenv("EPIPF_FUSED_LANES", raising=False)
    for k, v in (("EPIPF_BAND_SLACK", band), ("EPIPF_CLOCK_SLACK", clock)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    monkeypatch.delenv("EPIPF_SSA_FAST", raising=False)


def _filter(c, N, path, keys, fidx, counters=True):
    from epipf.engine import Engine
    chains = len(keys)
    th = np.asarray(c["theta"], dtype=np.float64)
    eng = Engine("sir", 1, N, c["Y"].shape[0], chains)
    try:
        eng.set_observations(c["Y"])
        eng.set_population(c["npop"], c["mu"])
        if path == "step":
            eng.set_lanes(1)
        if counters:
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
    keys, fidx = [73, 74], [3, 9]
    out = _filter(c, N, path, keys, fidx)
    _check(("golden", obs), c, N, out, keys, fidx)
    s = out[4]
    if slack[1] == "1e10" and N >= 63 and path == "step":
        assert s["ssa_exact_lanes"] > 0.5 * s["particle_steps"]        # the hand-back ran


# A chain key whose SSA stream holds, at filter index TINY_F, a block with ~y < 4096 (1 - U < 2^-20) at event 2 of
# particle 583 in step 2 and of particle 360 in step 5 (found on the CPU with oracle/philox.py over keys 1000..;
# a draw is that small with probability 2^-20, a key's 10 x 4096 x 5 first draws hold one with probability 0.18).
TINY_N, TINY_KEY, TINY_F = 4096, 1028, 3


def test_tiny_log2_branch_is_entered(datasets_golden, monkeypatch):
    k = np.arange(10)[:, None, None]
    j = np.arange(TINY_N)[None, :, None]
    p = np.arange(1, T)[None, None, :]
    r = philox.philox4x32_10(k, j, (p & 0xFFFFFF) | (philox.DOMAIN_SSA << 24), TINY_F, philox.split_key(TINY_KEY))
    hits = np.argwhere(((~r[1]) & np.uint64(0xFFFFFFFF)) < 4096)
    assert len(hits) > 0                                                # the counter exists
    c = _case(datasets_golden, False)
    o = _oracle(("tiny", False), c, TINY_N, TINY_KEY, TINY_F)
    assert o["status"] == 0
    # ... and its event happens: the particle's step has more than k events (each event moves one unit out of S or
    # into R), so the loop draws block k and takes its logarithm in the 1 - U < 2^-20 branch
    entered = 0
    for kk, jj, pi in hits:
        pp = int(pi) + 1
        parent = o["hidden"][pp - 1][o["ancestry"][pp][jj]].astype(np.int64)
        child = o["hidden"][pp][jj].astype(np.int64)
        nev = (parent[0] - child[0]) + (child[2] - parent[2])
        entered += int(nev > kk)
    assert entered > 0
    _env(monkeypatch, "step")
    out = _filter(c, TINY_N, "step", [TINY_KEY], [TINY_F])
    _check(("tiny", False), c, TINY_N, out, [TINY_KEY], [TINY_F])
    assert out[4]["ssa_exact_lanes"] < 0.05 * out[4]["particle_steps"]  # the f32 loop took the steps


# log_zeta as float64 bit patterns, T = 3, recorded on the build before this loop (and any scan) changed: N = 13,000 runs
# the segmented block-sum prefix (scan_segments), the others scan_block_sums; "fused" is the one-workgroup filter
SCAN_CASES = [("step", n) for n in SIZES + [13000]] + [("fused", n) for n in SIZES]
SCAN_KEYS, SCAN_FIDX = [61, 62], [2, 7]


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("path,N", SCAN_CASES)
def test_log_zeta_bits_unchanged(datasets_golden, monkeypatch, path, N, obs):
    _env(monkeypatch, path)
    c = _case(datasets_golden, obs, t=3)
    lz = _filter(c, N, path, SCAN_KEYS, SCAN_FIDX, counters=False)[0]
    want = np.load(GOLDEN)[f"{path}_obs{int(obs)}_N{N}"]
    got = np.ascontiguousarray(lz, dtype=np.float64).view(np.uint64)
    np.testing.assert_array_equal(got, want)
