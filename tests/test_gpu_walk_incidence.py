"""R_t from case counts on the GPU (epipf_incidence_walk and epipf_incidence_smooth through Engine):
anchored bit for bit to Engine.run_incidence at zero half-widths and to Engine.walk_filter on unreported counts, every
case against the numpy restatement (tests/walk_incidence_restatement.py), batches with a dying chain, the exact SSA
path, the smoothed true flows against a numpy reduction of history(), every refusal of both entry points, and the "does
it work" bounds through epipf.walk_incidence_filter.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import incidence_cases as ic
import incidence_restatement as ir
import walk_cases as wc
import walk_incidence_cases as wic
import walk_incidence_restatement as wir
import walk_restatement as wr

pytestmark = pytest.mark.gpu

COUNTERS = 2                                             # EPIPF_PROFILE_COUNTERS


def make_engine(model, N, T, chains=1):
    from epipf.engine import Engine
    eng = Engine(model, 1, N, T, chains)
    eng.set_population(wic.NPOP, wic.MU)
    return eng


def tiled(theta, N, chains=1):
    return np.tile(np.asarray(theta, dtype=np.float64), (chains, N, 1))


def lz_close(got, want):
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=0.0)


def dying_step(lz):
    dead = np.isneginf(lz)
    return int(np.argmax(dead)) if dead.any() else None


def assert_pass(eng, chain, lz, st, r):
    """Chain `chain` of the engine's last run against a restated pass: the rows before a dying step, all otherwise; the
    theta rows from a dying step on are NaN."""
    assert st == r["status"]
    lz_close(lz, r["log_zetas"])
    hid, anc = eng.history(chain + 1)
    th = eng.walk_history(chain + 1)
    T = r["hidden"].shape[0]
    rows = T if r["step"] is None else r["step"]
    np.testing.assert_array_equal(hid[chain, :rows], r["hidden"][:rows])
    np.testing.assert_array_equal(anc[chain, :rows], r["ancestry"][:rows])
    np.testing.assert_array_equal(wr.bits(th[chain]), wr.bits(r["theta_hist"]))
    assert np.isfinite(th[chain, :rows]).all() and np.isnan(th[chain, rows:]).all()


# ------------------------------------------------------------------------------------------- 1. the anchors
def check_incidence_anchor(model, observations, N, D):
    """Zero half-widths from theta tiled: Engine.run_incidence's hidden, ancestry, log_zeta bits and event counter."""
    T = D + 2
    eng = make_engine(model, N, T)
    eng.set_profiling(COUNTERS)
    theta, probs = wic.THETA[model], wic.PROBS[observations]
    counts = ic.daily(model, observations, range(ir.F[model]), days=D)
    assert np.isfinite(counts).all()
    rlz, rst = eng.run_incidence([theta], probs, wic.KEY, wic.F, counts, observations=observations)
    rhid, ranc = eng.history(1)
    revents = eng.stats()["events"]
    lz, st = eng.walk_incidence(tiled(theta, N), np.zeros((1, len(theta))), probs, wic.KEY, wic.F, counts,
                                observations=observations)
    hid, anc = eng.history(1)
    th = eng.walk_history(1)
    events = eng.stats()["events"]
    assert eng.run_T == T and lz.shape == (1, T) and st[0] == rst[0]
    np.testing.assert_array_equal(wr.bits(lz), wr.bits(rlz))
    rows = T if st[0] == 0 else dying_step(lz[0])
    assert rows >= 1
    np.testing.assert_array_equal(hid[0, :rows], rhid[0, :rows])
    np.testing.assert_array_equal(anc[0, :rows], ranc[0, :rows])
    assert (wr.bits(th[0, :rows]) == wr.bits(np.array(theta))).all() and np.isnan(th[0, rows:]).all()
    assert events == revents and (events > 0 or N == 1)
    eng.close()
    return st[0]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_zero_half_widths_are_run_incidence_bit_for_bit(model, observations, N):
    for D in (1, 2, 10):
        check_incidence_anchor(model, observations, N, D)


def test_zero_half_widths_on_the_segmented_block_sum_scan():
    """N = 12,864: 201 blocks, the first size whose block sums are scanned in segments."""
    assert check_incidence_anchor("sir", False, 12864, 1) == 0


@pytest.mark.parametrize("N", [1, 65, 200])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_unreported_counts_are_walk_filter_on_a_zero_series(model, N):
    """All-NaN counts against Engine.walk_filter on Y = 0 with probs = 0 (a binomial with p = 0 and y = 0 weighs 1),
    over D + 2 rows; the theta history bit for bit as well."""
    D = 10
    T = D + 2
    eng = make_engine(model, N, T)
    eng.set_observations(np.zeros((T, ir.C[model])))
    start, hw = tiled(wic.THETA[model], N), [wic.HW[model]]
    rlz, rst = eng.walk_filter(start, hw, 0.0, wic.KEY, wic.F)
    rhid, ranc = eng.history(1)
    rth = eng.walk_history(1)
    lz, st = eng.walk_incidence(start, hw, 0.5, wic.KEY, wic.F, np.full((D, ir.F[model]), np.nan))
    hid, anc = eng.history(1)
    th = eng.walk_history(1)
    assert st[0] == rst[0] == 0 and lz.shape == rlz.shape == (1, T) and th.shape == rth.shape
    np.testing.assert_array_equal(hid, rhid)
    np.testing.assert_array_equal(anc, ranc)
    np.testing.assert_array_equal(wr.bits(th), wr.bits(rth))
    assert (lz == 0.0).all() and (rlz == 0.0).all()
    assert N == 1 or len(np.unique(th[0, -1], axis=0)) > 1
    eng.close()


# ------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_each_column_and_all_columns_against_the_restatement(model, observations):
    eng = make_engine(model, wic.N, wic.D + 2)
    theta, hw, probs = wic.THETA[model], wic.HW[model], wic.PROBS[observations]
    for cols in wic.COLUMNS[model]:
        counts = ic.daily(model, observations, cols)
        r = wic.restate(counts, model, theta, hw, observations, probs)
        lz, st = eng.walk_incidence(tiled(theta, wic.N), [hw], probs, wic.KEY, wic.F, counts, observations=observations)
        assert st[0] == 0 and lz[0, 1] == 0.0
        assert_pass(eng, 0, lz[0], st[0], r)
        assert len(np.unique(eng.walk_history(1)[0, -1], axis=0)) > 1
    eng.close()


def test_cumulated_reports_against_the_restatement():
    eng = make_engine("sir", wic.N, wic.D + 2)
    theta, hw = wic.THETA["sir"], wic.HW["sir"]
    for counts in (ic.fixture()["threeday"], ic.mixed()):
        r = wic.restate(counts, "sir", theta, hw, False, 0.5, cumulate=True)
        lz, st = eng.walk_incidence(tiled(theta, wic.N), [hw], 0.5, wic.KEY, wic.F, counts, cumulate=True)
        assert_pass(eng, 0, lz[0], st[0], r)
        lz2, _ = eng.walk_incidence(tiled(theta, wic.N), [hw], 0.5, wic.KEY, wic.F, counts, cumulate=False)
        assert not np.array_equal(lz2, lz)               # the accumulator matters on these reports
    eng.close()


# ------------------------------------------------------------------------------------------- 3. batches
def test_three_widths_in_one_call_are_three_single_calls():
    N, D = 130, 10
    hw = np.array([[0.1, 0.05], [0.0, 0.02], [0.3, 0.0]])
    start = tiled(wic.THETA["sir"], N, 3)
    keys = np.array([5, 6, 7], dtype=np.uint64)
    counts = ic.mixed()[:D]
    eng = make_engine("sir", N, D + 2, chains=3)
    lz, st = eng.walk_incidence(start, hw, [0.5, 0.4, 0.6], keys, wic.F, counts, cumulate=True)
    hid, anc = eng.history(3)
    th = eng.walk_history(3)
    flows = eng.incidence_smooth(3, quantiles=(0.5,), lag=2)
    assert st.tolist() == [0, 0, 0]
    for s in range(3):
        lz1, st1 = eng.walk_incidence(start[s:s + 1], hw[s:s + 1], [0.5, 0.4, 0.6][s], keys[s:s + 1], wic.F, counts,
                                      cumulate=True)
        hid1, anc1 = eng.history(1)
        assert st1[0] == st[s]
        np.testing.assert_array_equal(wr.bits(lz1[0]), wr.bits(lz[s]))
        np.testing.assert_array_equal(hid1[0], hid[s])
        np.testing.assert_array_equal(anc1[0], anc[s])
        np.testing.assert_array_equal(wr.bits(eng.walk_history(1)[0]), wr.bits(th[s]))
        one = eng.incidence_smooth(1, quantiles=(0.5,), lag=2)
        np.testing.assert_array_equal(one.sums[0], flows.sums[s])
        np.testing.assert_array_equal(one.quantiles[0], flows.quantiles[s])
    eng.close()
    # a zero entry keeps its column bit for bit; a positive one moves it
    assert (wr.bits(th[1, :, :, 0]) == wr.bits(np.float64(0.8))).all()
    assert (wr.bits(th[2, :, :, 1]) == wr.bits(np.float64(0.3))).all()
    assert len(np.unique(th[1, -1, :, 1])) > 1 and len(np.unique(th[2, -1, :, 0])) > 1


def test_a_chain_that_dies_inside_a_batch_leaves_the_others_untouched():
    counts = ic.daily("sir", False, (0, 1))
    eng = make_engine("sir", wic.N, wic.D + 2, chains=3)
    start = np.stack([wic.swarm(b[0]) for b in wic.BATCH])
    hw, pr, keys = [b[1] for b in wic.BATCH], [b[2] for b in wic.BATCH], [b[3] for b in wic.BATCH]
    for cumulate in (False, True):
        lz, st = eng.walk_incidence(start, hw, pr, keys, wic.F, counts, cumulate=cumulate)
        assert st.tolist() == [0, 1, 0]
        for c, (t, h, p, k) in enumerate(wic.BATCH):
            assert_pass(eng, c, lz[c], st[c], wic.restate(counts, "sir", t, h, False, p, key=k, cumulate=cumulate))
        assert np.isneginf(lz[1, 3:]).all() and np.isfinite(lz[1, :3]).all()
        assert np.isnan(eng.walk_history(3)[1, 3:]).all()
    # the reductions skip the dead chain and give its neighbours what they get alone
    mean, quant, lin = eng.walk_smooth(3, lag=3)
    flows = eng.incidence_smooth(3, lag=3)
    states = eng.smooth(3, lag=3)
    assert np.isnan(mean[1]).all() and (lin[1] == 0).all() and np.isnan(states.mean[1]).all()
    assert np.isnan(flows.mean[1]).all() and (flows.sums[1] == 0).all() and (flows.lineages[1] == 0).all()
    assert (flows.quantiles[1] == 0).all() and np.isfinite(flows.mean[[0, 2]]).all() and (flows.lineages[[0, 2]] > 0).all()
    for s in (0, 2):
        eng.walk_incidence(start[s:s + 1], hw[s:s + 1], pr[s], keys[s], wic.F, counts, cumulate=True)
        one = eng.incidence_smooth(1, lag=3)
        np.testing.assert_array_equal(one.sums[0], flows.sums[s])
        np.testing.assert_array_equal(one.quantiles[0], flows.quantiles[s])
        np.testing.assert_array_equal(one.lineages[0], flows.lineages[s])
    eng.close()


# ------------------------------------------------------------------------------------------- 4. the exact path
def test_lanes_on_the_exact_path_give_the_unforced_run(monkeypatch):
    """With the clock and channel bands widened every lane that draws leaves the f32 loop for the per-lane exact loop
    (tests/test_gpu_step_phases.py): the same history, theta, log_zeta bits and event count as the unforced run."""
    from epipf.engine import Engine
    N, D = 65, 3
    counts = ic.mixed()[:D]
    theta, hw = wic.THETA["sir"], wic.HW["sir"]

    def run():
        eng = Engine("sir", 1, N, D + 2, 1)
        eng.set_population(wic.NPOP, wic.MU)
        eng.set_profiling(COUNTERS)
        lz, st = eng.walk_incidence(tiled(theta, N), [hw], 0.5, wic.KEY, wic.F, counts, cumulate=True)
        out = (lz, st, *eng.history(1), eng.walk_history(1), eng.stats())
        eng.close()
        return out

    lz, st, hid, anc, th, plain = run()
    monkeypatch.setenv("EPIPF_BAND_SLACK", "3000")
    monkeypatch.setenv("EPIPF_CLOCK_SLACK", "1e10")
    flz, fst, fhid, fanc, fth, forced = run()
    assert st[0] == fst[0] == 0
    infectious = sum(int((hid[0, p - 1][anc[0, p]][:, 1] > 0).sum()) for p in range(1, D + 2))
    assert forced["ssa_exact_lanes"] == infectious > 0 and plain["ssa_exact_lanes"] < infectious
    np.testing.assert_array_equal(fhid, hid)
    np.testing.assert_array_equal(fanc, anc)
    np.testing.assert_array_equal(wr.bits(fth), wr.bits(th))
    np.testing.assert_array_equal(wr.bits(flz), wr.bits(lz))
    assert forced["events"] == plain["events"] > 0


# ------------------------------------------------------------------------------------------- 5. the smoothed flows
QS = (0.0, 0.05, 0.5, 0.95, 1.0)


def check_flows(eng, model, n, bins=301):
    hid, anc = eng.history(n)
    for lag in (0, 1, 3, None):
        got = eng.incidence_smooth(n, quantiles=QS, lag=lag)
        assert got.quantiles.dtype == np.int64 and got.sums.shape == (n, eng.run_T, ir.F[model])
        for c in range(n):
            sums, qs, lin = wir.smoothed_flows(model, hid[c], anc[c], lag, QS, bins)
            np.testing.assert_array_equal(got.sums[c], sums)
            np.testing.assert_array_equal(got.quantiles[c], qs)
            np.testing.assert_array_equal(got.lineages[c], lin)
            np.testing.assert_array_equal(got.mean[c], sums / float(eng.N))
    assert eng.incidence_smooth(n, quantiles=None).quantiles is None


@pytest.mark.parametrize("N", [1, 64, 65, 200])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_smoothed_flows_are_the_numpy_reduction_of_the_history(model, N):
    """After walk_incidence and after run_incidence, with cumulate (the flows stay each day's own); D = 1 as well.
    Reported counts can kill a chain of a single particle, which is then not reduced; unreported ones (every weight 1)
    cannot, so on those the comparison runs at every N, N = 1 included."""
    theta, hw = wic.THETA[model], wic.HW[model]
    full = ic.daily(model, False, range(ir.F[model]))
    weekly = np.full(full.shape, np.nan)
    weekly[3::4] = full.reshape(-1, 4, ir.F[model]).sum(axis=1)
    unreported = np.full(full.shape, np.nan)
    eng = make_engine(model, N, wic.D + 2, chains=2)
    for counts, survives in ((weekly, N > 1), (full[:1], N > 1), (unreported, True), (unreported[:1], True)):
        _, st = eng.walk_incidence(tiled(theta, N, 2), [hw, hw], 0.5, [wic.KEY, 3], wic.F, counts, cumulate=True)
        assert (st == 0).all() or not survives
        if (st == 0).all():
            check_flows(eng, model, 2)
        _, st = eng.run_incidence([theta], 0.5, wic.KEY, wic.F, counts, cumulate=True)
        assert st[0] == 0 or not survives
        if st[0] == 0:
            check_flows(eng, model, 1)
    eng.close()


def test_incidence_filter_returns_the_smoothed_flows_of_its_own_run():
    """epipf.incidence_filter(...).incidence end to end: the numpy reduction of the run's own history; and after a second
    filter on the shared engine (same N, D and chains) the first result's unread flows are refused, not the second's."""
    import epipf
    from epipf.engine import release_engines
    counts = ic.daily("sir", False, (0, 1))              # the first and third chain of incidence_cases.BATCH: both OK
    kw = dict(flows=("infections", "removals"), n_particles=wic.N, n_population=wic.NPOP, mu=wic.MU,
              quantiles=QS, lag=3, filter_index=wic.F)
    a = epipf.incidence_filter(counts, "sir", [(0.8, 0.3), (1.6, 0.3)], probs=[0.5, 0.6], keys=[11, 2], **kw)
    assert a.status.tolist() == [0, 0]
    hid, anc = a.history()
    got = a.incidence
    assert got is a.incidence and got.mean.shape == (2, wic.D + 2, 2)
    for c in range(2):
        sums, qs, lin = wir.smoothed_flows("sir", hid[c], anc[c], 3, QS, 301)
        np.testing.assert_array_equal(got.sums[c], sums)
        np.testing.assert_array_equal(got.quantiles[c], qs)
        np.testing.assert_array_equal(got.lineages[c], lin)
    # the same run again, its flows not read before the next one
    a2 = epipf.incidence_filter(counts, "sir", [(0.8, 0.3), (1.6, 0.3)], probs=[0.5, 0.6], keys=[11, 2], **kw)
    b = epipf.incidence_filter(counts, "sir", [(1.6, 0.3), (0.8, 0.3)], probs=[0.6, 0.5], keys=[2, 11], **kw)
    with pytest.raises(RuntimeError, match="another filter"):
        a2.incidence
    np.testing.assert_array_equal(b.incidence.sums, got.sums[::-1])      # b's own flows: a's chains in the other order
    np.testing.assert_array_equal(a.incidence.sums, got.sums)            # what was read in time is kept
    release_engines()


def test_smoothed_flows_need_an_incidence_pass():
    from epipf import _lib
    E = _lib.EpipfError
    N, D = 16, 4
    eng = make_engine("sir", N, D + 2, chains=2)
    with pytest.raises(E, match=r"\(%d\).*no incidence pass" % _lib.ESTATE):
        eng.incidence_smooth(1)
    eng.set_observations(np.zeros((D + 2, 3)))
    counts = ic.daily("sir", False, (0, 1), days=D)
    theta, hw = wic.THETA["sir"], wic.HW["sir"]
    overwriting = [lambda: eng.run([theta], 0.0, 1, 0),
                   lambda: eng.walk_filter(tiled(theta, N), [hw], 0.0, 1, 0),
                   lambda: eng.if2(tiled(theta, N), [hw], 0.0, 1, 0)]
    for other in overwriting:
        eng.walk_incidence(tiled(theta, N), [hw], 0.5, 1, 0, counts)
        assert eng.incidence_smooth(1).sums.shape == (1, D + 2, 2)
        other()
        with pytest.raises(E, match=r"\(%d\).*overwrote" % _lib.ESTATE):
            eng.incidence_smooth(1)
    eng.run_incidence([theta], 0.5, 1, 0, counts)
    assert eng.incidence_smooth(1).sums.shape == (1, D + 2, 2)
    with pytest.raises(E, match=r"\(%d\).*overwrote" % _lib.ESTATE):     # run_incidence's pass has no theta history
        eng.walk_history(1)
    for n in (0, 2):                                     # one chain ran
        with pytest.raises(E, match=r"\(%d\).*n_chains" % _lib.EINVAL):
            eng.incidence_smooth(n)

    def raw(q, bins, with_quant=True, sums=True):
        q = None if q is None else np.array(q, dtype=np.float64)
        nq = 0 if q is None else q.size
        quant = np.zeros((1, max(nq, 1), D + 2, 2), dtype=np.int32) if with_quant else None
        _lib.check(eng._L.epipf_incidence_smooth(eng._h, 1, 2, _lib.ptr(q), nq, bins,
                                                 _lib.ptr(np.zeros((1, D + 2, 2), dtype=np.int64)) if sums else None,
                                                 _lib.ptr(quant), _lib.ptr(np.zeros((1, D + 2), dtype=np.int32))),
                   "epipf_incidence_smooth")

    raw([0.5], 301)
    with pytest.raises(E, match=r"\(%d\).*q\[0\]" % _lib.EINVAL):
        raw([1.5], 301)
    with pytest.raises(E, match=r"\(%d\).*quant_out" % _lib.EINVAL):
        raw([0.5], 301, with_quant=False)
    with pytest.raises(E, match=r"\(%d\).*bins" % _lib.EINVAL):
        raw([0.5], 0)
    with pytest.raises(E, match=r"\(%d\).*NULL" % _lib.EINVAL):
        raw(None, 0, sums=False)
    eng.close()


# ------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_of_the_filter():
    from epipf import _lib
    from epipf.engine import Engine
    N = 16
    eng = make_engine("sir", N, 6, chains=2)
    ok = np.array([[1.0, 2.0], [3.0, np.nan]])
    start, hw = tiled((0.8, 0.3), N), [(0.1, 0.0)]

    def refused(match, *a, code=_lib.EINVAL, **k):
        with pytest.raises(_lib.EpipfError, match=match) as e:
            eng.walk_incidence(*a, **k)
        assert "(%d)" % code in str(e.value)

    refused("D=5", start, hw, 0.5, 1, 0, np.full((5, 2), np.nan))                # D + 2 > t_max
    with pytest.raises(_lib.EpipfError, match="D=0"):
        eng.walk_incidence(start, hw, 0.5, 1, 0, np.ones((0, 2)))
    refused(r"counts\[1\]\[0\]=-3", start, hw, 0.5, 1, 0, [[1.0, 2.0], [-3.0, 1.0]])
    refused(r"counts\[0\]\[1\]=inf", start, hw, 0.5, 1, 0, [[1.0, np.inf], [3.0, 1.0]])
    refused(r"counts\[1\]\[1\]=2.5.*integer", start, hw, 0.5, 1, 0, [[1.0, 2.0], [3.0, 2.5]])
    refused(r"probs\[0\]=1.5", start, hw, 1.5, 1, 0, ok)
    refused(r"probs\[1\]=nan", tiled((0.8, 0.3), N, 2), hw * 2, [0.5, np.nan], 1, 0, ok)
    refused(r"probs\[0\]=-0.1", start, hw, -0.1, 1, 0, ok, observations=True)
    for bad in (-0.5, np.nan, np.inf):
        s = start.copy()
        s[0, 3, 1] = bad
        refused(r"swarm\[0\]\[3\]\[1\]", s, hw, 0.5, 1, 0, ok)
        refused(r"half_widths\[0\]\[1\]", start, [[0.1, bad]], 0.5, 1, 0, ok)
    refused("n_chains=3", tiled((0.8, 0.3), N, 3), hw * 3, 0.5, 1, 0, ok)
    refused("entries per particle", np.ones((1, N, 3)), np.ones((1, 3)), 0.5, 1, 0, ok)
    with pytest.raises(ValueError):
        eng.walk_incidence(start, hw, 0.5, 1, 0, np.ones((2, 3)))                # SEIR's columns on a SIR engine
    with pytest.raises(ValueError):
        eng.walk_incidence(np.ones((1, N + 1, 2)), hw, 0.5, 1, 0, ok)
    with pytest.raises(ValueError):
        eng.walk_incidence(start, [(0.1, 0.0)] * 2, 0.5, 1, 0, ok)
    # non-integer reports and a noise ratio above 1 are the normal model's to take; observations are not needed
    lz, st = eng.walk_incidence(start, hw, 1.5, 1, 0, [[1.0, 2.5]], observations=True)
    assert st[0] == 0 and lz.shape == (1, 3) and eng.run_T == 3 and eng.walk_history(1).shape == (1, 3, N, 2)
    eng.close()
    fresh = Engine("sir", 1, N, 6, 1)
    with pytest.raises(_lib.EpipfError, match=r"\(%d\).*epipf_set_population" % _lib.ESTATE):
        fresh.walk_incidence(start, hw, 0.5, 1, 0, ok)
    fresh.close()
    sub = Engine("sir_subgroups", 2, N, 6, 1)            # the library's own refusal, past the binding's column check
    sub.set_population([150, 150], [3, 3])
    sw5, hw5, one = np.full((1, N, 5), 0.5), np.full((1, 5), 0.1), np.array([0.5])
    key, f = np.array([1], dtype=np.uint64), np.array([0], dtype=np.uint32)
    lz, st = np.empty((1, 4)), np.empty(1, dtype=np.int32)
    L = _lib.load()
    rc = L.epipf_incidence_walk(sub._h, 1, _lib.ptr(sw5), 5, _lib.ptr(hw5), _lib.OBS_BINOMIAL, _lib.ptr(one), _lib.ptr(key),
                                _lib.ptr(f), _lib.ptr(np.ascontiguousarray(ok)), 2, 0, _lib.ptr(lz), _lib.ptr(st))
    assert rc == _lib.EINVAL and b"SIR and SEIR" in L.epipf_last_error()
    rc = L.epipf_incidence_walk(sub._h, 1, None, 5, _lib.ptr(hw5), _lib.OBS_BINOMIAL, _lib.ptr(one), _lib.ptr(key),
                                _lib.ptr(f), _lib.ptr(np.ascontiguousarray(ok)), 2, 0, _lib.ptr(lz), _lib.ptr(st))
    assert rc == _lib.EINVAL and b"NULL" in L.epipf_last_error()
    sub.close()


ENOMEM_SCRIPT = """
import numpy as np
from epipf import _lib
from epipf.engine import Engine
eng = Engine("sir", 1, 1000, 5, 2)
eng.set_population(300, 5)
c = np.ones((3, 2))
sw, hw = np.tile([0.8, 0.3], (2, 1000, 1)), [[0.1, 0.0]] * 2
lz, st = eng.walk_incidence(sw[:1], hw[:1], 0.5, 1, 0, c, cumulate=True)         # 16000 bytes: within the budget
try:
    eng.walk_incidence(sw, hw, 0.5, 1, 0, c, cumulate=True)                     # 32000 bytes: over it
    raise SystemExit("no error")
except _lib.EpipfError as e:
    assert "(%d)" % _lib.ENOMEM in str(e) and "32000 bytes" in str(e) and "20000" in str(e), str(e)
lz2, st2 = eng.walk_incidence(sw, hw, 0.5, 1, 0, c, cumulate=False)              # no accumulator: runs
lz3, st3 = eng.walk_incidence(sw[:1], hw[:1], 0.5, 1, 0, c, cumulate=True)       # and the context still works
assert np.array_equal(lz, lz3) and np.array_equal(lz2[0], lz[0])
print("enomem ok")
"""


def test_accumulator_over_its_budget_is_enomem_naming_the_bytes():
    """EPIPF_INCIDENCE_ACC_BYTES is read at epipf_create, so a fresh process (the subject of this test) sets it."""
    from conftest import PKG, REPO
    env = dict(os.environ, EPIPF_INCIDENCE_ACC_BYTES="20000", PYTHONPATH=os.pathsep.join([PKG, REPO]))
    out = subprocess.run([sys.executable, "-c", ENOMEM_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "enomem ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("which,flows", [("both", ("infections", "removals")), ("infections", ("infections",))])
def test_does_it_work_on_the_device(which, flows):
    """epipf.walk_incidence_filter on the step fixture's half-reported counts at the restatement's N, keys 1..4: the
    bounds of DESIGN.md §20 (tests/test_walk_incidence_restatement.py), and the smoothed true infections against the
    raw reports."""
    import epipf
    from epipf.engine import release_engines
    w = wic.work()
    cases = w["counts"][:, list(wic.COLUMNS_WORK[which])]
    for key in wic.KEYS:
        epipf.seed_stream(key, wic.F_WORK)               # chain_key(key, 0) = key: a single chain is the restatement's
        got = epipf.walk_incidence_filter(cases, "sir", wic.START, wic.RW, flows, probs=wic.PROBS_WORK, lag=wic.LAG_WORK,
                                          quantiles=(0.5,), n_particles=wic.N_WORK, n_population=w["npop"], mu=w["mu"],
                                          key=key)
        epipf.seed_stream(key, wic.F_WORK)
        fixed = epipf.walk_incidence_filter(cases, "sir", wic.START, (0.0, 0.0), flows, probs=wic.PROBS_WORK,
                                            lag=wic.LAG_WORK, quantiles=(0.5,), n_particles=wic.N_WORK,
                                            n_population=w["npop"], mu=w["mu"], key=key)
        assert got.status[0] == 0 and got.best == 0 and got.log_zetas.shape == (1, 31)
        gap = wc.plateau_gap(got.theta_quantiles[0, 0, :, 0])
        gain = got.loglik[0] - fixed.loglik[0]
        err = wic.infection_error(got.incidence.mean[0, :, 0])
        print("which", which, "key", key, "gap", gap, "gain", gain, "error", err)
        assert gap > wic.GAP_BOUND[which] and gain > wic.GAIN_BOUND[which]
        if which == "infections":
            assert wic.RAW_ERROR - err > wic.MARGIN_BOUND
    release_engines()
