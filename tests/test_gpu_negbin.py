"""Negative-binomial reporting on the GPU (epipf_run_incidence_negbin and epipf_incidence_walk_negbin through Engine;
DESIGN.md §21): every case of tests/negbin_cases.py against the restatements (tests/negbin_restatement.py,
tests/walk_negbin_restatement.py), per-chain dispersions in a batch with a chain that dies, the random-walk filter's
anchor, restatement and exact path, the anchors to the binomial pass, the history calls, incidence_mcmc with the
dispersion estimated against the engine-double run, the "does it work" bounds through epipf.incidence_filter, and every
refusal.  Needs an MI355X."""
import numpy as np
import pytest

import incidence_restatement as ir
import negbin_cases as nc
import smoothing_helpers as sh
import walk_incidence_cases as wic
import walk_incidence_restatement as wir
import walk_restatement as wr
from test_gpu_incidence import _first, assert_pass, make_engine
from test_gpu_walk_incidence import COUNTERS, tiled
from test_gpu_walk_incidence import assert_pass as assert_walk_pass

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_each_column_and_all_columns_against_the_restatement(model):
    eng = make_engine(model, nc.N, nc.D + 2)
    for cols in nc.COLUMNS[model]:
        counts = nc.daily(model, cols)
        r = nc.restate(counts, model, nc.THETA[model])
        lz, st = eng.run_incidence([nc.THETA[model]], nc.RHO, nc.KEY, nc.F, counts, dispersion=nc.KAPPA)
        assert st[0] == 0 and lz[0, 1] == 0.0
        assert_pass(eng, 0, lz[0], st[0], r)
    eng.close()


def test_cumulated_reports_against_the_restatement():
    eng = make_engine("sir", nc.N, nc.D + 2)
    three = nc.fixture()["over_threeday"]
    for counts, cumulate in [(three, True), (three, False), (nc.mixed(), True)]:
        r = nc.restate(counts, "sir", (0.8, 0.3), cumulate=cumulate)
        lz, st = eng.run_incidence([(0.8, 0.3)], nc.RHO, nc.KEY, nc.F, counts, cumulate=cumulate, dispersion=nc.KAPPA)
        assert st[0] == 0
        assert_pass(eng, 0, lz[0], st[0], r)
    eng.close()


@pytest.mark.parametrize("N,D", nc.SIZES)
def test_sizes_against_the_restatement(N, D):
    counts = nc.daily("sir", (0,), days=D)
    r = nc.restate(counts, "sir", (0.8, 0.3), n=N)
    assert r["status"] == 0
    eng = make_engine("sir", N, D + 2)
    lz, st = eng.run_incidence([(0.8, 0.3)], nc.RHO, nc.KEY, nc.F, counts, dispersion=nc.KAPPA)
    assert_pass(eng, 0, lz[0], st[0], r)
    eng.close()


def test_on_the_segmented_block_sum_scan():
    """N = 12,864: 201 blocks, the first size whose block sums are scanned in segments; against no restatement."""
    eng = make_engine("sir", 12864, 4)
    lz, st = eng.run_incidence([(0.8, 0.3)], nc.RHO, nc.KEY, nc.F, nc.daily("sir", (0, 1), days=2), dispersion=nc.KAPPA)
    assert st[0] == 0 and np.isfinite(lz).all() and lz[0, 1] == 0.0 and lz[0, -1] < 0.0
    eng.close()


# ------------------------------------------------------------------------------------------- 2. the batch
def test_per_chain_dispersions_and_a_chain_that_dies_inside_a_batch():
    counts = nc.daily("sir", (0, 1))
    eng = make_engine("sir", nc.N, nc.D + 2, chains=3)
    th, pr = [b[0] for b in nc.BATCH], [b[1] for b in nc.BATCH]
    kap, keys = [b[2] for b in nc.BATCH], [b[3] for b in nc.BATCH]
    lz, st = eng.run_incidence(th, pr, keys, nc.F, counts, dispersion=kap)
    hid, anc = eng.history(3)
    assert st.tolist() == [0, 1, 0]
    for c, (t, p, k, key) in enumerate(nc.BATCH):
        assert_pass(eng, c, lz[c], st[c], nc.restate(counts, "sir", t, p, k, key=key))
    assert np.isneginf(lz[1, 3:]).all() and (lz[1, :3] == 0.0).all()
    assert lz[0, -1] == pytest.approx(-78.482, abs=5e-4) and lz[2, -1] == pytest.approx(-138.1835, abs=5e-5)
    # per-chain kappa in one call equals three single calls, bit for bit
    for c in range(3):
        lz1, st1 = eng.run_incidence(th[c:c + 1], pr[c], keys[c], nc.F, counts, dispersion=kap[c])
        hid1, anc1 = eng.history(1)
        rows = nc.D + 2 if st1[0] == 0 else 3
        assert st1[0] == st[c]
        np.testing.assert_array_equal(wr.bits(lz1[0]), wr.bits(lz[c]))
        np.testing.assert_array_equal(hid1[0, :rows], hid[c, :rows])
        np.testing.assert_array_equal(anc1[0, :rows], anc[c, :rows])
    # an inactive chain runs nothing and its dispersion is not read
    lz3, st3 = eng.run_incidence(th, pr, keys, nc.F, counts, dispersion=[2.0, -1.0, 50.0], active=[1, 0, 1])
    assert st3.tolist() == [0, 2, 0] and np.isnan(lz3[1]).all()
    np.testing.assert_array_equal(lz3[[0, 2]], lz[[0, 2]])
    eng.close()


# ------------------------------------------------------------------------------------------- 3. the random-walk filter
@pytest.mark.parametrize("N", [1, 65, 200])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_walk_with_zero_half_widths_is_run_incidence_bit_for_bit(model, N):
    D = 10
    eng = make_engine(model, N, D + 2)
    theta = nc.THETA[model]
    counts = nc.daily(model, range(ir.F[model]), days=D)
    rlz, rst = eng.run_incidence([theta], nc.RHO, nc.KEY, nc.F, counts, dispersion=nc.KAPPA)
    rhid, ranc = eng.history(1)
    lz, st = eng.walk_incidence(tiled(theta, N), np.zeros((1, len(theta))), nc.RHO, nc.KEY, nc.F, counts,
                                dispersion=nc.KAPPA)
    hid, anc = eng.history(1)
    assert st[0] == rst[0] and lz.shape == (1, D + 2)
    np.testing.assert_array_equal(wr.bits(lz), wr.bits(rlz))
    rows = D + 2 if st[0] == 0 else int(np.argmax(np.isneginf(lz[0])))
    assert rows >= 1
    np.testing.assert_array_equal(hid[0, :rows], rhid[0, :rows])
    np.testing.assert_array_equal(anc[0, :rows], ranc[0, :rows])
    eng.close()


@pytest.mark.parametrize("model", ["sir", "seir"])
def test_walk_against_the_restatement(model):
    eng = make_engine(model, nc.N, nc.D + 2)
    theta, hw = nc.THETA[model], wic.HW[model]
    cases = [(nc.daily(model, nc.COLUMNS[model][-1]), False), (nc.daily(model, (0,)), False)]
    if model == "sir":
        cases.append((nc.mixed(), True))
    for counts, cumulate in cases:
        r = nc.restate_walk(counts, model, hw, cumulate=cumulate)
        lz, st = eng.walk_incidence(tiled(theta, nc.N), [hw], nc.RHO, nc.KEY, nc.F, counts, cumulate=cumulate,
                                    dispersion=nc.KAPPA)
        assert st[0] == 0 and lz[0, 1] == 0.0
        assert_walk_pass(eng, 0, lz[0], st[0], r)
    eng.close()


def test_walk_lanes_on_the_exact_path_give_the_unforced_run(monkeypatch):
    """With the clock and channel bands widened every lane that draws leaves the f32 loop for the per-lane exact loop:
    the same history, theta, log_zeta bits and event count as the unforced run (the log table is staged once for both
    the exact loop and the weight)."""
    from epipf.engine import Engine
    N, D = 65, 3
    counts = nc.mixed()[:D]
    theta, hw = nc.THETA["sir"], wic.HW["sir"]

    def run():
        eng = Engine("sir", 1, N, D + 2, 1)
        eng.set_population(nc.NPOP, nc.MU)
        eng.set_profiling(COUNTERS)
        lz, st = eng.walk_incidence(tiled(theta, N), [hw], nc.RHO, nc.KEY, nc.F, counts, cumulate=True,
                                    dispersion=nc.KAPPA)
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


# ------------------------------------------------------------------------------------------- 4. anchors
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_unreported_counts_are_the_binomial_pass_bit_for_bit(model):
    N, D = 65, 10
    eng = make_engine(model, N, D + 2)
    nan = np.full((D, ir.F[model]), np.nan)
    for cumulate in (False, True):
        blz, bst = eng.run_incidence([nc.THETA[model]], 0.5, nc.KEY, nc.F, nan, cumulate=cumulate)
        bhid, banc = eng.history(1)
        lz, st = eng.run_incidence([nc.THETA[model]], 0.5, nc.KEY, nc.F, nan, cumulate=cumulate, dispersion=nc.KAPPA)
        hid, anc = eng.history(1)
        assert st[0] == bst[0] == 0 and (lz == 0.0).all()
        np.testing.assert_array_equal(wr.bits(lz), wr.bits(blz))
        np.testing.assert_array_equal(hid, bhid)
        np.testing.assert_array_equal(anc, banc)
    eng.close()


def test_dispersion_none_runs_the_old_entry_points(monkeypatch):
    eng = make_engine("sir", 16, 5)
    called = []
    L = eng._L

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(L, name)

    counts = nc.daily("sir", (0, 1), days=3)
    monkeypatch.setattr(eng, "_L", Spy())
    eng.run_incidence([(0.8, 0.3)], 0.5, 1, 0, counts)
    eng.run_incidence([(0.8, 0.3)], 0.5, 1, 0, counts, dispersion=None)
    eng.walk_incidence(tiled((0.8, 0.3), 16), [(0.1, 0.0)], 0.5, 1, 0, counts, dispersion=None)
    assert called == ["epipf_run_incidence", "epipf_run_incidence", "epipf_incidence_walk"]
    eng.run_incidence([(0.8, 0.3)], 0.5, 1, 0, counts, dispersion=2.0)
    eng.walk_incidence(tiled((0.8, 0.3), 16), [(0.1, 0.0)], 0.5, 1, 0, counts, dispersion=2.0)
    assert called[3:] == ["epipf_run_incidence_negbin", "epipf_incidence_walk_negbin"]
    monkeypatch.undo()
    eng.close()


# ------------------------------------------------------------------------------------------- 5. the history calls
def test_history_path_sample_smooth_and_incidence_smooth_see_the_pass():
    import smoothing_lag_helpers as slh
    counts = nc.mixed()
    T = nc.D + 2
    eng = make_engine("sir", nc.N, T + 5)                # t_max beyond the run length: the calls use D + 2 rows
    lz, st = eng.run_incidence([(0.8, 0.3)], nc.RHO, nc.KEY, nc.F, counts, cumulate=True, dispersion=nc.KAPPA)
    r = nc.restate(counts, "sir", (0.8, 0.3), cumulate=True)
    assert st[0] == 0 and eng.run_T == T
    hid, anc = eng.history(1)
    assert hid.shape == (1, T, nc.N, 3)
    np.testing.assert_array_equal(hid[0], r["hidden"])
    np.testing.assert_array_equal(anc[0], r["ancestry"])
    hf, af = r["hidden"].astype(np.float64), r["ancestry"].astype(np.float64)
    paths, visited = sh.reference_paths(hf, af)
    for k in (0, 17, nc.N - 1):
        np.testing.assert_array_equal(eng.path_sample([k])[0], paths[k])
    want = sh.path_statistics(*sh.genealogy_paths(hf, af))
    sh.assert_smoothed_equal(_first(eng.smooth(1, quantiles=sh.QS, lineage="genealogy")), *want, nc.N)
    got = _first(eng.smooth(1, quantiles=sh.QS, lineage="genealogy", lag=3))
    sh.assert_smoothed_equal(got, *slh.lag_brute_force(r["hidden"], r["ancestry"], "genealogy", 3, sh.QS), nc.N)
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    for lag in (3, None):
        flows = eng.incidence_smooth(1, quantiles=qs, lag=lag)
        sums, quant, lin = wir.smoothed_flows("sir", r["hidden"], r["ancestry"], lag, qs, 301)
        np.testing.assert_array_equal(flows.sums[0], sums)
        np.testing.assert_array_equal(flows.quantiles[0], quant)
        np.testing.assert_array_equal(flows.lineages[0], lin)
    # after the random-walk filter the parameter history's calls see the pass as well
    from epipf import _lib
    with pytest.raises(_lib.EpipfError, match=r"\(%d\)" % _lib.ESTATE):
        eng.walk_history(1)
    lz, st = eng.walk_incidence(tiled((0.8, 0.3), nc.N), [wic.HW["sir"]], nc.RHO, nc.KEY, nc.F, counts, cumulate=True,
                                dispersion=nc.KAPPA)
    assert st[0] == 0 and eng.run_T == T and eng.walk_history(1).shape == (1, T, nc.N, 2)
    mean, quant, lin = eng.walk_smooth(1, lag=3)
    assert np.isfinite(mean).all() and eng.incidence_smooth(1, lag=3).sums.shape == (1, T, 2)
    eng.close()


# ------------------------------------------------------------------------------------------- 6. the public functions
def test_incidence_mcmc_estimating_the_dispersion_equals_the_engine_double_run(monkeypatch):
    """theta, acceptances and trajectories bit for bit at the pinned seed (tests/test_negbin_host.py checks that no
    decision of it lies within 1e-6 of its boundary)."""
    import negbin_oracle_engine as noe
    from epipf import incidence
    dev = nc.mcmc_run()
    monkeypatch.setattr(incidence._engine, "get_engine", noe.fake_get_engine)
    cpu = nc.mcmc_run()
    for a, b in zip(dev, cpu):
        np.testing.assert_array_equal(a.thetas, b.thetas)
        np.testing.assert_array_equal(a.sampled_trajs, b.sampled_trajs)
        assert a.acceptances == b.acceptances and a.filters_run == b.filters_run
        np.testing.assert_allclose(a.log_likelihoods, b.log_likelihoods, rtol=1e-9, atol=0.0)
        assert a.thetas.shape == (nc.MCMC["iters"], 3)


def test_does_it_work_on_the_device():
    """DESIGN.md §21's table through epipf.incidence_filter: infections alone on the 24 overdispersed days, N = 200,
    index 0, keys 1..4; the binomial filter fails at the true parameters, the negative-binomial one tells the true theta
    from half the infection rate and the true dispersion from 0.5, 10 and 1000 (half the smallest gap per claim, as on
    the CPU: tests/test_negbin_restatement.py)."""
    import epipf
    from test_negbin_restatement import BINOMIAL, TABLE
    cases = nc.fixture()["over"][:, 0]
    keys = [1, 2, 3, 4]
    common = dict(flows=("infections",), probs=0.5, n_particles=200, n_population=nc.NPOP, mu=nc.MU, keys=keys,
                  filter_index=0)
    b = epipf.incidence_filter(cases, "sir", [(0.8, 0.3)] * 4, **common)
    assert b.status.tolist() == [1, 1, 0, 0]
    assert np.isneginf(b.log_zetas[:2, 14:]).all() and np.isfinite(b.log_zetas[:2, :14]).all()
    np.testing.assert_allclose(b.loglik[2:], [BINOMIAL[3], BINOMIAL[4]], atol=5e-3)
    got = {}
    for name, theta, kappa in [("nb2", (0.8, 0.3), 2.0), ("low", (0.4, 0.3), 2.0), (0.5, (0.8, 0.3), 0.5),
                               (10.0, (0.8, 0.3), 10.0), (1000.0, (0.8, 0.3), 1000.0)]:
        res = epipf.incidence_filter(cases, "sir", [theta] * 4, dispersion=kappa, **common)
        assert (res.status == 0).all() and res.log_zetas.shape == (4, 26)
        got[name] = res.loglik
        np.testing.assert_allclose(res.loglik, TABLE[name], atol=5e-3, err_msg=str(name))
    print("table", {k: v.tolist() for k, v in got.items()})
    assert (got["nb2"] - got["low"]).min() > 7.0
    assert (got["nb2"] - got[0.5]).min() > 1.5
    assert (got["nb2"] - got[10.0]).min() > 1.9
    assert (got["nb2"] - got[1000.0]).min() > 7.4
    # one value per chain in a single call
    res = epipf.incidence_filter(cases, "sir", [(0.8, 0.3)] * 4, dispersion=[2.0, 0.5, 10.0, 1000.0], **common)
    want = [got["nb2"][0], got[0.5][1], got[10.0][2], got[1000.0][3]]
    np.testing.assert_array_equal(res.loglik, want)
    assert res.best == 0


def test_walk_incidence_filter_takes_a_dispersion():
    import epipf
    from epipf.engine import release_engines
    release_engines()
    cases = nc.fixture()["over"][:12, 0]
    res = epipf.walk_incidence_filter(cases, "sir", start=[0.8, 0.3], rw=[0.05, 0.0], probs=0.5, dispersion=2.0,
                                      n_particles=nc.N, n_population=nc.NPOP, mu=nc.MU, chains=2, key=nc.KEY, lag=3)
    assert (res.status == 0).all() and res.log_zetas.shape == (2, 14) and res.incidence.mean.shape == (2, 14, 2)
    with pytest.raises(ValueError, match="observations"):
        epipf.walk_incidence_filter(cases, "sir", start=[0.8, 0.3], rw=[0.05, 0.0], observations=True, dispersion=2.0,
                                    n_particles=nc.N, n_population=nc.NPOP, mu=nc.MU)
    release_engines()


# ------------------------------------------------------------------------------------------- 7. refusals
def test_every_refusal_of_the_entry_points():
    from epipf import _lib
    eng = make_engine("sir", 16, 6, chains=2)
    ok = np.array([[1.0, 2.0], [3.0, np.nan]])
    th = [(0.8, 0.3)]
    sw, hw = tiled((0.8, 0.3), 16), [(0.1, 0.0)]

    def refused(match, *a, **k):
        for call, head in ((eng.run_incidence, (th,)), (eng.walk_incidence, (sw, hw))):
            with pytest.raises(_lib.EpipfError, match=match) as e:
                call(*head, *a, **k)
            assert "(%d)" % _lib.EINVAL in str(e.value)

    refused(r"dispersion\[0\]=0", 0.5, 1, 0, ok, dispersion=0.0)
    refused(r"dispersion\[0\]=-2", 0.5, 1, 0, ok, dispersion=-2.0)
    refused(r"dispersion\[0\]=nan", 0.5, 1, 0, ok, dispersion=np.nan)
    refused(r"dispersion\[0\]=inf", 0.5, 1, 0, ok, dispersion=np.inf)
    refused(r"dispersion\[0\]=1e\+06.*Poisson limit.*out of scope", 0.5, 1, 0, ok, dispersion=1.0000001e6)
    refused(r"dispersion\[0\]=.*subnormal", 0.5, 1, 0, ok, dispersion=1e-310)
    refused(r"probs\[0\]=-0.1", -0.1, 1, 0, ok, dispersion=2.0)
    refused(r"probs\[0\]=nan", np.nan, 1, 0, ok, dispersion=2.0)
    refused(r"probs\[0\]=inf", np.inf, 1, 0, ok, dispersion=2.0)
    refused(r"probs\[0\]=.*out of scope", 1e-310, 1, 0, ok, dispersion=2.0)
    refused(r"counts\[1\]\[1\]=2.5.*negative-binomial model needs integer", 0.5, 1, 0, [[1.0, 2.0], [3.0, 2.5]],
            dispersion=2.0)
    refused(r"counts\[1\]\[0\]=-3", 0.5, 1, 0, [[1.0, 2.0], [-3.0, 1.0]], dispersion=2.0)
    refused("D=5", 0.5, 1, 0, np.full((5, 2), np.nan), dispersion=2.0)
    with pytest.raises(_lib.EpipfError, match=r"dispersion\[1\]=0"):
        eng.run_incidence(th * 2, 0.5, 1, 0, ok, dispersion=[2.0, 0.0])
    with pytest.raises(_lib.EpipfError, match=r"theta\[0\]\[1\]=-0.3"):
        eng.run_incidence([(0.8, -0.3)], 0.5, 1, 0, ok, dispersion=2.0)
    for call, head in ((eng.run_incidence, (th,)), (eng.walk_incidence, (sw, hw))):
        with pytest.raises(ValueError, match="observations"):
            call(*head, 0.5, 1, 0, ok, observations=True, dispersion=2.0)
        with pytest.raises(ValueError, match="dispersion must be a scalar"):
            call(*head, 0.5, 1, 0, ok, dispersion=[2.0, 2.0])
    # the cap itself, a ratio above 1 and a ratio of 0 are inside
    _, st = eng.run_incidence(th * 2, [1.5, 0.0], 1, 0, [[0.0, 0.0]], dispersion=[1e6, 0.01])
    assert st.tolist() == [0, 0]
    eng.close()
    from epipf.engine import Engine
    fresh = Engine("sir", 1, 16, 6, 1)
    with pytest.raises(_lib.EpipfError, match=r"\(%d\).*epipf_set_population" % _lib.ESTATE):
        fresh.run_incidence(th, 0.5, 1, 0, ok, dispersion=2.0)
    fresh.close()
    sub = Engine("sir_subgroups", 2, 16, 6, 1)
    sub.set_population([150, 150], [3, 3])
    th5, one = np.full((1, 5), 0.5), np.array([0.5])
    key, f = np.array([1], dtype=np.uint64), np.array([0], dtype=np.uint32)
    lz, st = np.empty((1, 4)), np.empty(1, dtype=np.int32)
    rc = _lib.load().epipf_run_incidence_negbin(sub._h, 1, _lib.ptr(th5), 5, _lib.ptr(one), _lib.ptr(one), _lib.ptr(key),
                                                _lib.ptr(f), None, _lib.ptr(np.ascontiguousarray(ok)), 2, 0,
                                                _lib.ptr(lz), _lib.ptr(st))
    assert rc == _lib.EINVAL and b"SIR and SEIR" in _lib.load().epipf_last_error()
    rc = _lib.load().epipf_run_incidence_negbin(sub._h, 1, _lib.ptr(th5), 5, _lib.ptr(one), None, _lib.ptr(key),
                                                _lib.ptr(f), None, _lib.ptr(np.ascontiguousarray(ok)), 2, 0,
                                                _lib.ptr(lz), _lib.ptr(st))
    assert rc == _lib.EINVAL and b"NULL" in _lib.load().epipf_last_error()
    sub.close()
