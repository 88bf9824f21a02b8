"""The random-walk filter on the GPU (epipf_walk_filter, epipf_walk_history through Engine): anchored to
Engine.if2 at one iteration bit for bit, every day's theta against the numpy restatement (tests/walk_restatement.py),
per-chain half-widths, a degenerate chain inside a batch, every refusal of the four entry points, and the "does it
work" assertions on the step fixture at the restatement's N.  Needs an MI355X."""
import numpy as np
import pytest

import if2_cases
import walk_cases as wc
import walk_restatement as wr

pytestmark = pytest.mark.gpu

KEY, F = 11, 3
THETA = {"sir": (0.8, 0.3), "seir": (0.9, 0.6, 0.3)}
RW = {"sir": (0.1, 0.05), "seir": (0.1, 0.08, 0.05)}
PROBS = {False: 0.5, True: 0.2}


@pytest.fixture(scope="module")
def fx():
    return if2_cases.load_fixture()


def make_engine(fx, model, N, T, chains=1):
    from epipf.engine import Engine
    eng = Engine(model, 1, N, max(T, 1), chains)
    eng.set_observations(fx[model][:T])
    eng.set_population(fx["npop"], fx["mu"])
    return eng


def lz_close(got, want):
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=0.0)


# ------------------------------------------------------------------------------------------- 1. the anchor
def check_anchor(eng, model, observations):
    """walk_filter against Engine.if2(iterations=1) at the same swarm, half-widths, key and index."""
    N, d, T = eng.N, len(THETA[model]), eng.T
    swarm0 = np.tile(np.array(THETA[model]), (1, N, 1))
    hw = np.array([RW[model]])
    swarm, _, ilz, done, ist = eng.if2(swarm0, hw, PROBS[observations], KEY, F, observations=observations)
    ihid, ianc = eng.history(1)
    lz, st = eng.walk_filter(swarm0, hw, PROBS[observations], KEY, F, observations=observations)
    hid, anc = eng.history(1)
    th = eng.walk_history(1)
    assert st[0] == ist[0]
    if st[0] == 0:
        assert done[0] == 1
        np.testing.assert_array_equal(hid, ihid)
        np.testing.assert_array_equal(anc, ianc)
        np.testing.assert_array_equal(wr.bits(lz[0]), wr.bits(ilz[0, 0]))
        np.testing.assert_array_equal(wr.bits(th[0, T - 1]), wr.bits(swarm[0]))
        assert np.isfinite(th).all()
    else:                                                # both die at the same step; the rows before it agree
        dead = int(np.argmax(np.isneginf(lz[0])))
        assert dead >= 1 and np.isneginf(lz[0, dead:]).all() and np.isfinite(lz[0, :dead]).all()
        np.testing.assert_array_equal(hid[0, :dead], ihid[0, :dead])
        np.testing.assert_array_equal(anc[0, :dead], ianc[0, :dead])
        assert np.isfinite(th[0, :dead]).all() and np.isnan(th[0, dead:]).all()
    return st[0]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_one_pass_of_if2_bit_for_bit(fx, model, observations, N):
    for T in (1, 2, 12):
        eng = make_engine(fx, model, N, T)
        check_anchor(eng, model, observations)
        eng.close()


def test_one_pass_of_if2_on_the_segmented_scan(fx):
    """N = 12,864: 201 blocks, the first size whose block sums are scanned in segments."""
    eng = make_engine(fx, "sir", 12864, 3)
    assert check_anchor(eng, "sir", False) == 0
    eng.close()


# ------------------------------------------------------------------------------------------- 2. the history
@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's N = 65, T = 12 passes (shared, never modified)."""
    return {m: wr.one_pass(fx[m][:12], m, np.tile(np.array(THETA[m]), (65, 1)), RW[m], False, fx["probs"], fx["npop"],
                           fx["mu"], KEY, F) for m in ("sir", "seir")}


@pytest.mark.parametrize("model", ["sir", "seir"])
def test_every_days_theta_is_the_restatements(fx, restated, model):
    r = restated[model]
    assert r["status"] == 0
    eng = make_engine(fx, model, 65, 12)
    lz, st = eng.walk_filter(np.tile(np.array(THETA[model]), (1, 65, 1)), [RW[model]], fx["probs"], KEY, F)
    hid, anc = eng.history(1)
    th = eng.walk_history(1)
    eng.close()
    assert st[0] == 0
    np.testing.assert_array_equal(wr.bits(th[0]), wr.bits(r["theta_hist"]))
    np.testing.assert_array_equal(hid[0], r["hidden"])
    np.testing.assert_array_equal(anc[0], r["ancestry"])
    lz_close(lz[0], r["log_zetas"])
    assert len(np.unique(th[0, -1], axis=0)) > 1


# ------------------------------------------------------------------------------------------- 3. per-chain widths
def test_three_widths_in_one_call_are_three_single_calls(fx):
    N, T = 130, 12
    hw = np.array([[0.1, 0.05], [0.0, 0.02], [0.3, 0.0]])
    swarm0 = np.tile(np.array(THETA["sir"]), (3, N, 1))
    keys = np.array([5, 6, 7], dtype=np.uint64)
    eng = make_engine(fx, "sir", N, T, chains=3)
    lz, st = eng.walk_filter(swarm0, hw, fx["probs"], keys, F)
    hid, anc = eng.history(3)
    th = eng.walk_history(3)
    assert st.tolist() == [0, 0, 0]
    for s in range(3):
        lz1, st1 = eng.walk_filter(swarm0[s:s + 1], hw[s:s + 1], fx["probs"], keys[s:s + 1], F)
        hid1, anc1 = eng.history(1)
        th1 = eng.walk_history(1)
        assert st1[0] == st[s]
        np.testing.assert_array_equal(wr.bits(lz1[0]), wr.bits(lz[s]))
        np.testing.assert_array_equal(hid1[0], hid[s])
        np.testing.assert_array_equal(anc1[0], anc[s])
        np.testing.assert_array_equal(wr.bits(th1[0]), wr.bits(th[s]))
    eng.close()
    # a zero entry keeps its column bit for bit; a positive one moves it
    assert (wr.bits(th[1, :, :, 0]) == wr.bits(np.float64(0.8))).all()
    assert (wr.bits(th[2, :, :, 1]) == wr.bits(np.float64(0.3))).all()
    assert len(np.unique(th[1, -1, :, 1])) > 1 and len(np.unique(th[2, -1, :, 0])) > 1


# ------------------------------------------------------------------------------------------- 4. a degenerate chain
def test_a_degenerate_chain_between_two_good_ones(fx):
    N, T = 48, 25
    starts = np.array([[1.2, 0.5], [2.0, 1.0], [1.0, 0.4]])
    swarm0 = np.repeat(starts[:, None, :], N, axis=1)
    hw = np.tile((0.1, 0.05), (3, 1))
    keys = np.array([1, 2, 3], dtype=np.uint64)
    want = [wr.one_pass(fx["sir"], "sir", swarm0[s], hw[s], False, fx["probs"], fx["npop"], fx["mu"], int(keys[s]), 0)
            for s in range(3)]
    assert [r["status"] for r in want] == [0, 1, 0]
    eng = make_engine(fx, "sir", N, T, chains=3)
    lz, st = eng.walk_filter(swarm0, hw, fx["probs"], keys, 0)
    hid, anc = eng.history(3)
    th = eng.walk_history(3)
    mean, quant, lin = eng.walk_smooth(3, lag=3)
    states = eng.smooth(3, lag=3)
    assert st.tolist() == [0, 1, 0]
    dead = int(np.argmax(np.isneginf(want[1]["log_zetas"])))
    for s in range(3):
        rows = T if s != 1 else dead
        lz_close(lz[s], want[s]["log_zetas"])
        np.testing.assert_array_equal(hid[s, :rows], want[s]["hidden"][:rows])
        np.testing.assert_array_equal(anc[s, :rows], want[s]["ancestry"][:rows])
        np.testing.assert_array_equal(wr.bits(th[s, :rows]), wr.bits(want[s]["theta_hist"][:rows]))
    assert np.isnan(th[1, dead:]).all()
    assert np.isnan(mean[1]).all() and np.isnan(quant[1]).all() and (lin[1] == 0).all() and np.isnan(states.mean[1]).all()
    assert np.isfinite(mean[[0, 2]]).all() and (lin[[0, 2]] > 0).all()
    # the neighbours are what they are alone
    for s in (0, 2):
        eng.walk_filter(swarm0[s:s + 1], hw[s:s + 1], fx["probs"], keys[s:s + 1], 0)
        m1, q1, l1 = eng.walk_smooth(1, lag=3)
        np.testing.assert_array_equal(wr.bits(m1[0]), wr.bits(mean[s]))
        np.testing.assert_array_equal(wr.bits(q1[0]), wr.bits(quant[s]))
        np.testing.assert_array_equal(l1[0], lin[s])
    eng.close()


# ------------------------------------------------------------------------------------------- 5. estate and einval
def test_refusals(fx):
    from epipf import _lib
    from epipf.engine import Engine
    E = _lib.EpipfError
    N, T = 16, 6
    eng = Engine("sir", 1, N, T, 2)
    swarm0 = np.tile(np.array(THETA["sir"]), (1, N, 1))
    hw = np.array([RW["sir"]])
    with pytest.raises(E, match=r"\(-4\)"):              # EPIPF_ESTATE: no observations yet
        eng.walk_filter(swarm0, hw, 0.5, KEY, F)
    eng.set_observations(fx["sir"][:T])
    with pytest.raises(E, match=r"\(-4\)"):              # no population yet
        eng.walk_filter(swarm0, hw, 0.5, KEY, F)
    eng.set_population(fx["npop"], fx["mu"])
    for call in (lambda: eng.walk_history(1), lambda: eng.walk_smooth(1)):
        with pytest.raises(E, match=r"\(-4\).*no random-walk filter"):
            call()
    for bad_swarm in (-0.5, np.nan, np.inf):
        s = swarm0.copy()
        s[0, 3, 1] = bad_swarm
        with pytest.raises(E, match=r"\(-1\).*swarm\[0\]\[3\]\[1\]"):
            eng.walk_filter(s, hw, 0.5, KEY, F)
    for bad_hw in (-0.1, np.nan, np.inf):
        with pytest.raises(E, match=r"\(-1\).*half_widths\[0\]\[1\]"):
            eng.walk_filter(swarm0, [[0.1, bad_hw]], 0.5, KEY, F)
    with pytest.raises(E, match=r"\(-1\).*n_chains"):    # more chains than the context holds
        eng.walk_filter(np.tile(swarm0, (3, 1, 1)), np.tile(hw, (3, 1)), 0.5, KEY, F)
    with pytest.raises(E, match=r"\(-1\).*entries per particle"):
        eng.walk_filter(np.ones((1, N, 3)), np.ones((1, 3)), 0.5, KEY, F)
    lz, st = eng.walk_filter(swarm0, hw, fx["probs"], KEY, F)
    assert st[0] == 0 and eng.walk_history(1).shape == (1, T, N, 2)
    for n in (0, 2):                                     # one chain ran
        with pytest.raises(E, match=r"\(-1\).*n_chains"):
            eng.walk_history(n)
        with pytest.raises(E, match=r"\(-1\).*n_chains"):
            eng.walk_smooth(n)
    def raw_smooth(lineage, q, with_quant=True):
        q = None if q is None else np.array(q, dtype=np.float64)
        nq = 0 if q is None else q.size
        quant = np.zeros((1, max(nq, 1), T, 3)) if with_quant else None
        _lib.check(eng._L.epipf_walk_smooth(eng._h, 1, lineage, 1, _lib.ptr(q), nq, _lib.ptr(np.zeros((1, T, 3))),
                                            _lib.ptr(quant), _lib.ptr(np.zeros((1, T), dtype=np.int32))), "epipf_walk_smooth")

    raw_smooth(_lib.LINEAGE_GENEALOGY, [0.5])
    with pytest.raises(E, match=r"\(-1\).*lineage"):
        raw_smooth(7, None)
    with pytest.raises(E, match=r"\(-1\).*q\[0\]"):
        raw_smooth(_lib.LINEAGE_GENEALOGY, [1.5])
    with pytest.raises(E, match=r"\(-1\).*quant_out"):
        raw_smooth(_lib.LINEAGE_GENEALOGY, [0.5], with_quant=False)
    # another run overwrites the context's history: the parameter history is no longer its companion
    eng.run(np.array([THETA["sir"]]), fx["probs"], KEY, F)
    for call in (lambda: eng.walk_history(1), lambda: eng.walk_smooth(1)):
        with pytest.raises(E, match=r"\(-4\).*overwrote"):
            call()
    eng.walk_filter(swarm0, hw, fx["probs"], KEY, F)
    eng.walk_history(1)
    eng.if2(swarm0, hw, fx["probs"], KEY, F)
    with pytest.raises(E, match=r"\(-4\).*overwrote"):
        eng.walk_history(1)
    # the host-array entry point: the first offending index is named
    hid, anc, th, _ = wc.chains(3, 5, 3, 2, limit=2)
    lin, q = _lib.LINEAGE_GENEALOGY, np.array([0.5])
    eng.walk_smooth_history(hid, anc, th, 300.0, lin, q)
    for v in (-1.0, np.nan, np.inf):
        bad = th.copy()
        bad[1, 2, 3, 1] = v
        bad[1, 2, 4, 0] = v
        with pytest.raises(E, match=r"\(-1\).*theta\[1\]\[2\]\[3\]\[1\]"):
            eng.walk_smooth_history(hid, anc, bad, 300.0, lin, q)
    bad = hid.copy()
    bad[0, 1, 2, 0] = -1
    with pytest.raises(E, match=r"\(-1\).*hidden\[0\]\[1\]\[2\]\[0\]"):
        eng.walk_smooth_history(bad, anc, th, 300.0, lin, q)
    for v in (-1, 5):
        bad = anc.copy()
        bad[1, 0, 4] = v
        with pytest.raises(E, match=r"\(-1\).*ancestry\[1\]\[0\]\[4\]"):
            eng.walk_smooth_history(hid, bad, th, 300.0, lin, q)
    for pop in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(E, match=r"\(-1\).*population_total"):
            eng.walk_smooth_history(hid, anc, th, pop, lin, q)
    with pytest.raises(E, match=r"\(-1\).*lineage"):
        eng.walk_smooth_history(hid, anc, th, 300.0, 9, q)
    with pytest.raises(E, match=r"\(-1\).*d=4"):
        eng.walk_smooth_history(hid, anc, np.ones((2, 3, 5, 4)), 300.0, lin, q)
    eng.close()
    sub = Engine("sir_subgroups", 2, N, T, 1)
    with pytest.raises(E, match=r"\(-1\).*SIR and SEIR"):
        sub.walk_filter(np.ones((1, N, 5)), np.ones((1, 5)), 0.5, KEY, F)
    sub.close()


# ------------------------------------------------------------------------------------------- 6. end to end
def test_the_walk_finds_the_step_on_the_device():
    """The CPU test's assertions (tests/test_walk_restatement.py) through epipf.walk_filter at the restatement's N; the
    device's history and quantiles are also what the CPU test judged, bit for bit."""
    import epipf
    from epipf import walk
    from epipf.engine import release_engines
    fx = wc.load_fixture()
    rw = np.array([wc.RW, (0.0, 0.0)])
    for key in wc.KEYS:
        epipf.seed_stream(key, wc.F_WORK)
        # chain_key(key, 0) = key: a single chain is the restatement's run
        got = epipf.walk_filter(fx["Y"], "sir", wc.START, rw[0], lag=wc.LAG_WORK, quantiles=(0.5,), n_particles=wc.N_WORK,
                                n_population=fx["npop"], mu=fx["mu"], probs=fx["probs"], key=key)
        r = wc.restated(key, True)
        assert got.status[0] == 0 and got.best == 0
        eng = epipf.get_engine("sir", 1, wc.N_WORK, fx["Y"].shape[0], 1, 0)
        np.testing.assert_array_equal(wr.bits(eng.walk_history(1)[0]), wr.bits(r["theta_hist"]))
        _, qs, lin = walk.smooth_history(r["hidden"], r["ancestry"], r["theta_hist"], fx["npop"], lag=wc.LAG_WORK,
                                         quantiles=(0.5,))
        np.testing.assert_array_equal(wr.bits(got.theta_quantiles[0, 0]), wr.bits(qs[0, :, :2]))
        np.testing.assert_array_equal(wr.bits(got.rt_quantiles[0, 0]), wr.bits(qs[0, :, 2]))
        np.testing.assert_array_equal(got.lineages[0], lin)
        epipf.seed_stream(key, wc.F_WORK)
        fixed = epipf.walk_filter(fx["Y"], "sir", wc.START, rw[1], lag=wc.LAG_WORK, quantiles=(0.5,),
                                  n_particles=wc.N_WORK, n_population=fx["npop"], mu=fx["mu"], probs=fx["probs"], key=key)
        gap = wc.plateau_gap(got.theta_quantiles[0, 0, :, 0])
        gain = got.loglik[0] - fixed.loglik[0]
        print("key", key, "gap", gap, "gain", gain)
        assert gap > wc.GAP_BOUND and gain > wc.GAIN_BOUND
    release_engines()
