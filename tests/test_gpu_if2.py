"""Iterated filtering on the GPU (epipf_if2 through Engine.if2, epipf.if2 on top): anchored to the
existing filter (no jitter: Engine.run bit for bit), against the numpy restatement (tests/if2_restatement.py), batch
independence, continuation, degeneracy, the argument errors, and the search end to end on the small SIR fixture.
Needs an MI355X."""
import os

import numpy as np
import pytest

import if2_restatement as rs
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KEY, F = 11, 3
THETA = {"sir": (0.8, 0.3), "seir": (0.9, 0.6, 0.3)}
RW = {"sir": (0.1, 0.05), "seir": (0.1, 0.08, 0.05)}
PROBS = {False: 0.5, True: 0.2}                         # binomial p / normal noise ratio


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "if2_sir_small.npz"))
    Y = z["Y"]
    Y4 = np.concatenate([Y[:, :1], Y[:, 1:2] // 2, Y[:, 1:2] - Y[:, 1:2] // 2, Y[:, 2:]], axis=1)   # S, E, I, R
    return dict(sir=Y, seir=Y4, npop=float(z["population"]), mu=float(z["mu"]), probs=float(z["probs"]))


def make_engine(fx, model, N, T, chains=1):
    from epipf.engine import Engine
    eng = Engine(model, 1, N, max(T, 1), chains)
    eng.set_observations(fx[model][:T])
    eng.set_population(fx["npop"], fx["mu"])
    return eng


def mean_close(mean, swarm):
    """A device mean against np.mean of the swarm it came from: 2 N 2^-53 relative, the bound for any summation order
    of non-negative terms."""
    want = np.asarray(swarm).mean(axis=-2)
    assert (np.abs(mean - want) <= 2.0 * swarm.shape[-2] * 2.0 ** -53 * np.abs(want)).all(), (mean, want)


def lz_close(got, want):
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=0.0)


# ------------------------------------------------------------------------------------------- 1. the anchor
def check_anchor(eng, model, theta, observations, T):
    """One iteration with zero half-widths from a swarm of equal theta is Engine.run at the same key and filter index."""
    N, d = eng.N, len(theta)
    lz, st = eng.run(np.array([theta]), PROBS[observations], KEY, F, observations=observations)
    hid, anc = eng.history(1)
    swarm0 = np.tile(np.array(theta), (1, N, 1))
    swarm, mean, ilz, done, ist = eng.if2(swarm0, np.zeros((1, d)), PROBS[observations], KEY, F, observations=observations)
    ihid, ianc = eng.history(1)
    assert ist[0] == st[0]
    np.testing.assert_array_equal(swarm, swarm0)
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


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_no_jitter_is_the_filter(fx, model, observations, N):
    ok = 0
    for T in (1, 2, 12):
        eng = make_engine(fx, model, N, T)
        ok += check_anchor(eng, model, THETA[model], observations, T) == 0
        eng.close()
    # every case completes on the oracle but SEIR binomial at N = 1, T = 12, whose one particle dies (the dying path)
    assert ok == (2 if (model, observations, N) == ("seir", False, 1) else 3)


def test_no_jitter_is_the_filter_on_the_segmented_scan(fx):
    """N = 12,864: 201 blocks, the first size whose block sums are scanned in segments."""
    eng = make_engine(fx, "sir", 12864, 3)
    assert check_anchor(eng, "sir", THETA["sir"], False, 3) == 0
    eng.close()


# ------------------------------------------------------------------------------------------- 2. the restatement
@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's N = 65, T = 12, M = 3 runs (shared, never modified)."""
    out = {}
    for model in ("sir", "seir"):
        swarm = np.tile(np.array(THETA[model]), (65, 1))
        hw = rs.cooling_table(RW[model], 0.5 ** (50 / 12), 3)
        out[model] = (hw, rs.run(fx[model][:12], model, swarm, hw, False, fx["probs"], fx["npop"], fx["mu"], KEY, F))
    return out


def check_search(r, swarm, mean, lz, done, st, hid, anc):
    """One search's results (the arrays of Engine.if2 and Engine.history at its index) against the restatement r."""
    assert st == r["status"] and done == r["iterations_done"]
    np.testing.assert_array_equal(swarm, r["swarm"])
    # a pass that died at a step leaves the rows from that step on unwritten, as epipf_run does
    rows = r["hidden"].shape[0] if st == 0 else int(np.argmax(np.isneginf(r["last_log_zetas"])))
    np.testing.assert_array_equal(hid[:rows], r["hidden"][:rows])
    np.testing.assert_array_equal(anc[:rows], r["ancestry"][:rows])
    for m in range(done):
        lz_close(lz[m], r["log_zetas"][m])
    assert np.isnan(lz[done:]).all() and np.isnan(mean[done:]).all()
    if done:
        mean_close(mean[done - 1], swarm)
        # the restatement's means are np.mean of each iteration's swarm, and the swarms are equal
        np.testing.assert_allclose(mean[:done], r["mean"][:done], rtol=2.0 * swarm.shape[0] * 2.0 ** -53, atol=0.0)
    for m in range(done):                                # and in the finish kernel's summation order, bit for bit
        np.testing.assert_array_equal(mean[m], rs.device_mean(r["swarms"][m]))


def check_against(eng, r, swarm0, hw, probs, key, f, observations=False):
    swarm, mean, lz, done, st = eng.if2(swarm0[None], hw, probs, key, f, observations=observations)
    hid, anc = eng.history(1)
    check_search(r, swarm[0], mean[0], lz[0], int(done[0]), int(st[0]), hid[0], anc[0])
    return swarm, mean


@pytest.mark.parametrize("model", ["sir", "seir"])
def test_equals_the_restatement(fx, restated, model):
    hw, r = restated[model]
    assert r["status"] == 0 and r["iterations_done"] == 3
    eng = make_engine(fx, model, 65, 12)
    swarm, _ = check_against(eng, r, np.tile(np.array(THETA[model]), (65, 1)), hw, fx["probs"], KEY, F)
    assert len(np.unique(swarm[0], axis=0)) > 1          # the jitter and the selection did something
    eng.close()


def test_reflection_equals_the_restatement(fx):
    """A start of 0.01 with half-width 0.05: reflected at 0, never negative, the restatement's bits."""
    hw = np.array([[0.05, 0.05], [0.05, 0.05]])
    swarm0 = np.tile([0.01, 0.01], (48, 1))
    r = rs.run(fx["sir"][:4], "sir", swarm0, hw, False, fx["probs"], fx["npop"], fx["mu"], 5, 0)
    assert r["reflections"] >= 1 and r["status"] == 0 and r["iterations_done"] == 2
    eng = make_engine(fx, "sir", 48, 4)
    swarm, _ = check_against(eng, r, swarm0, hw, fx["probs"], 5, 0)
    assert (swarm >= 0.0).all()
    eng.close()


# ------------------------------------------------------------------------------------------- 3. batch independence
STARTS = np.array([[0.8, 0.3], [1.0, 0.4], [0.7, 0.25]])
KEYS = np.array([101, 202, 303], dtype=np.uint64)
F0 = np.array([0, 7, 0xFFFFFFFF])                       # the last search's second iteration wraps to filter index 0


def results(eng, swarm, hw, probs, keys, f0):
    out = eng.if2(swarm, hw, probs, keys, f0)
    return out + eng.history(len(swarm))


def assert_same(a, b, what):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=what)


@pytest.mark.parametrize("streams", [1, 4])
def test_searches_in_a_batch_equal_the_searches_alone(fx, streams):
    eng = make_engine(fx, "sir", 65, 12, chains=3)
    eng.set_streams(streams)
    hw = rs.cooling_table(RW["sir"], 0.5, 2)
    swarm0 = np.repeat(STARTS[:, None, :], 65, axis=1)
    solo = [results(eng, swarm0[s:s + 1], hw, fx["probs"], KEYS[s:s + 1], F0[s:s + 1]) for s in range(3)]
    batch = results(eng, swarm0, hw, fx["probs"], KEYS, F0)
    assert (batch[4] == 0).all() and (batch[3] == 2).all()
    for s in range(3):
        assert_same([x[s:s + 1] for x in batch], solo[s], f"search {s}")
    eng.close()


# ------------------------------------------------------------------------------------------- 4. continuation
def test_three_iterations_equal_one_then_two(fx):
    eng = make_engine(fx, "sir", 65, 12)
    hw = rs.cooling_table(RW["sir"], 0.5 ** (50 / 12), 3)
    swarm0 = np.tile(np.array(THETA["sir"]), (1, 65, 1))
    whole = results(eng, swarm0, hw, fx["probs"], KEY, F)
    first = eng.if2(swarm0, hw[:1], fx["probs"], KEY, F)
    rest = results(eng, first[0], hw[1:], fx["probs"], KEY, F + 1)
    np.testing.assert_array_equal(rest[0], whole[0])
    np.testing.assert_array_equal(np.concatenate([first[1], rest[1]], axis=1), whole[1])
    np.testing.assert_array_equal(np.concatenate([first[2], rest[2]], axis=1), whole[2])
    assert first[3][0] + rest[3][0] == whole[3][0] == 3
    assert_same(rest[5:], whole[5:], "history of the last iteration")
    eng.close()


# ------------------------------------------------------------------------------------------- 5. degeneracy
def test_a_degenerate_search_between_two_good_ones(fx):
    eng = make_engine(fx, "sir", 48, 25, chains=3)
    hw = rs.cooling_table((0.1, 0.05), 0.5 ** (50 / 12), 3)
    starts = np.array([[1.2, 0.5], [2.0, 1.0], [1.0, 0.4]])
    swarm0 = np.repeat(starts[:, None, :], 48, axis=1)
    keys = np.array([1, 2, 3], dtype=np.uint64)
    swarm, mean, lz, done, st = eng.if2(swarm0, hw, fx["probs"], keys, 0)
    assert st.tolist() == [0, 1, 0] and done.tolist() == [3, 0, 3]
    np.testing.assert_array_equal(swarm[1], swarm0[1])
    assert np.isnan(mean[1]).all() and np.isnan(lz[1]).all()
    assert np.isfinite(mean[[0, 2]]).all() and np.isfinite(lz[[0, 2]]).all()
    for s in (0, 2):
        solo = eng.if2(swarm0[s:s + 1], hw, fx["probs"], keys[s:s + 1], 0)
        assert_same([swarm[s:s + 1], mean[s:s + 1], lz[s:s + 1], done[s:s + 1], st[s:s + 1]], solo, f"search {s}")
    eng.close()


# ------------------------------------------------------------------------------------------- 6. argument errors
def raw_if2(eng, S, M, swarm, d, hw):
    from epipf import _lib
    from epipf._lib import ptr
    swarm = np.ascontiguousarray(swarm, dtype=np.float64)
    hw = np.ascontiguousarray(hw, dtype=np.float64)
    n = max(S, 1)
    probs, keys, f0 = np.full(n, 0.5), np.arange(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    mean = np.zeros((n, max(M, 1), max(d, 1)))
    done, st = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rc = eng._L.epipf_if2(eng._h, S, M, ptr(swarm), d, ptr(hw), _lib.OBS_BINOMIAL, ptr(probs), ptr(keys), ptr(f0), None,
                          ptr(mean), ptr(done), ptr(st))
    return rc, eng._L.epipf_last_error().decode()


def test_argument_errors_leave_the_context_usable(fx):
    import oracle
    from epipf import _lib
    from epipf.engine import Engine
    N, T = 32, 8
    good_swarm, good_hw = np.tile([0.8, 0.3], (2, N, 1)), np.full((2, 2), 0.01)
    eng = Engine("sir", 1, N, T, 2)
    for ready in (lambda: None, lambda: eng.set_observations(fx["sir"][:T])):        # before the data, then before the population
        ready()
        rc, msg = raw_if2(eng, 2, 2, good_swarm, 2, good_hw)
        assert rc == _lib.ESTATE and msg
    eng.set_population(fx["npop"], fx["mu"])

    def bad(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    cases = {
        "wrong d": (2, 2, good_swarm, 3, good_hw),
        "too many searches": (3, 2, np.tile([0.8, 0.3], (3, N, 1)), 2, good_hw),
        "no searches": (0, 2, good_swarm, 2, good_hw),
        "no iterations": (2, 0, good_swarm, 2, good_hw),
        "negative half-width": (2, 2, good_swarm, 2, bad(good_hw, (1, 0), -0.01)),
        "NaN half-width": (2, 2, good_swarm, 2, bad(good_hw, (0, 1), np.nan)),
        "negative swarm entry": (2, 2, bad(good_swarm, (1, 5, 0), -0.5), 2, good_hw),
        "NaN swarm entry": (2, 2, bad(good_swarm, (0, 31, 1), np.nan), 2, good_hw),
    }
    for name, args in cases.items():
        rc, msg = raw_if2(eng, *args)
        assert rc == _lib.EINVAL and msg, name
    sub = Engine("sir_subgroups", 2, N, T, 2)
    rc, msg = raw_if2(sub, 2, 2, np.tile([0.8] * 5, (2, N, 1)), 5, np.full((2, 5), 0.01))
    assert rc == _lib.EINVAL and "subgroup" in msg
    sub.close()
    # the context still runs its usual filter
    lz, st = eng.run(np.array([[0.8, 0.3]]), 0.5, KEY, F)
    hid, anc = eng.history(1)
    o = oracle.particle_filter(fx["sir"][:T], "sir", (0.8, 0.3), False, 0.5, N, fx["npop"], fx["mu"], key=KEY, filter_index=F)
    assert st[0] == o["status"] == 0
    np.testing.assert_array_equal(hid[0], o["hidden"])
    np.testing.assert_array_equal(anc[0], o["ancestry"])
    lz_close(lz[0], o["log_zetas"])
    # and, after a good if2 call, again
    assert eng.if2(good_swarm, good_hw, 0.5, [1, 2], 0)[4].tolist() == [0, 0]
    lz2, st2 = eng.run(np.array([[0.8, 0.3]]), 0.5, KEY, F)
    assert st2[0] == 0
    np.testing.assert_array_equal(lz2, lz)
    assert_same(eng.history(1), (hid, anc), "history after if2, then run")
    eng.close()


# ------------------------------------------------------------------------------------------- 7. end to end
def test_the_search_finds_the_peak(fx):
    import epipf
    s = dict(N=48, M=12, rw=(0.1, 0.05), cooling=0.5 ** (50 / 12), start=(1.2, 0.5))
    hw = rs.cooling_table(s["rw"], s["cooling"], s["M"])
    r = rs.run(fx["sir"], "sir", np.tile(np.array(s["start"]), (s["N"], 1)), hw, False, fx["probs"], fx["npop"], fx["mu"], 1, 0)
    epipf.seed_stream(1, 0)
    res = epipf.if2(fx["sir"], epipf.ModelType.SIR, s["start"], s["rw"], iterations=s["M"], cooling=s["cooling"],
                    n_particles=s["N"], n_population=fx["npop"], mu=fx["mu"], probs=fx["probs"], searches=1, evaluate=True)
    assert res.status.tolist() == [0] and res.iterations_done.tolist() == [s["M"]] and res.best == 0
    np.testing.assert_array_equal(res.swarm[0], r["swarm"])
    mean_close(res.theta[0], res.swarm[0])
    np.testing.assert_array_equal(res.theta[0], rs.device_mean(r["swarm"]))
    np.testing.assert_allclose(res.theta[0], r["mean"][-1], rtol=2.0 * s["N"] * 2.0 ** -53, atol=0.0)
    lz_close(res.loglik[0], r["loglik"])
    start = rs.score(fx["sir"], "sir", s["start"], False, fx["probs"], fx["npop"], fx["mu"])
    print(f"theta {res.theta[0]}, loglik_at_theta {res.loglik_at_theta[0]:.2f}, loglik(start) {start:.2f}")
    assert res.loglik_at_theta[0] - start >= 30.0
    assert isinstance(res.continue_(1), epipf.If2Result)
