"""Incidence observations on the GPU (epipf_run_incidence through Engine): anchored to Engine.run at
Y = 0, probs = 0 bit for bit, every case of tests/incidence_cases.py against the numpy restatement
(tests/incidence_restatement.py), a degenerate chain inside a batch, history / path_sample / smooth on the D + 2 rows,
incidence_mcmc against the engine-double run at the pinned seed, the "does it work" assertion through
epipf.incidence_filter, and every refusal of the entry point.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import incidence_cases as ic
import incidence_restatement as ir
import smoothing_helpers as sh

pytestmark = pytest.mark.gpu


def make_engine(model, N, T, chains=1):
    from epipf.engine import Engine
    eng = Engine(model, 1, N, T, chains)
    eng.set_population(ic.NPOP, ic.MU)
    return eng


def lz_close(got, want):
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=0.0)


def assert_pass(eng, chain, lz, st, r):
    """Chain `chain` of the engine's last run against a restated pass: the rows before a dying step, all otherwise."""
    assert st == r["status"]
    lz_close(lz, r["log_zetas"])
    hid, anc = eng.history(chain + 1)
    rows = r["hidden"].shape[0] if r["step"] is None else r["step"]
    np.testing.assert_array_equal(hid[chain, :rows], r["hidden"][:rows])
    np.testing.assert_array_equal(anc[chain, :rows], r["ancestry"][:rows])


# ------------------------------------------------------------------------------------------- 1. the anchor
def check_anchor(model, N, D):
    """All-NaN counts against Engine.run on Y = 0 with probs = 0 (a binomial with p = 0 and y = 0 weighs 1)."""
    T = D + 2
    eng = make_engine(model, N, T)
    th = np.array([ic.THETA[model]])
    eng.set_observations(np.zeros((T, ir.C[model])))
    rlz, rst = eng.run(th, 0.0, ic.KEY, ic.F)
    rhid, ranc = eng.history(1)
    lz, st = eng.run_incidence(th, 0.5, ic.KEY, ic.F, np.full((D, ir.F[model]), np.nan))
    hid, anc = eng.history(1)
    assert st[0] == rst[0] == 0 and lz.shape == (1, T) and hid.shape == rhid.shape
    np.testing.assert_array_equal(hid, rhid)
    np.testing.assert_array_equal(anc, ranc)
    assert (lz == 0.0).all() and (rlz == 0.0).all()
    eng.close()


@pytest.mark.parametrize("D", [1, 2, 10])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_anchor_unreported_counts_are_the_state_filter_at_probs_zero(model, N, D):
    check_anchor(model, N, D)


def test_anchor_on_the_segmented_block_sum_scan():
    check_anchor("sir", 12864, 1)


# ------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_each_column_and_all_columns_against_the_restatement(model, observations):
    eng = make_engine(model, ic.N, ic.D + 2)
    for cols in ic.COLUMNS[model]:
        counts = ic.daily(model, observations, cols)
        r = ic.restate(counts, model, ic.THETA[model], observations, ic.PROBS[observations])
        lz, st = eng.run_incidence([ic.THETA[model]], ic.PROBS[observations], ic.KEY, ic.F, counts,
                                   observations=observations)
        assert st[0] == 0 and lz[0, 1] == 0.0
        assert_pass(eng, 0, lz[0], st[0], r)
    eng.close()


def test_cumulated_reports_against_the_restatement():
    eng = make_engine("sir", ic.N, ic.D + 2)
    three = ic.fixture()["threeday"]
    for counts, cumulate in [(three, True), (three, False), (ic.mixed(), True), (ic.daily("sir", False, (0, 1)), True)]:
        r = ic.restate(counts, "sir", (0.8, 0.3), False, 0.5, cumulate=cumulate)
        lz, st = eng.run_incidence([(0.8, 0.3)], 0.5, ic.KEY, ic.F, counts, cumulate=cumulate)
        assert_pass(eng, 0, lz[0], st[0], r)
    assert st[0] == 0                                    # every entry reported: cumulate changes nothing
    lz2, _ = eng.run_incidence([(0.8, 0.3)], 0.5, ic.KEY, ic.F, counts, cumulate=False)
    np.testing.assert_array_equal(lz2, lz)
    eng.close()


def test_seir_cumulated_reports_against_the_restatement():
    """Exposures daily, onsets and removals as 3-day totals of the thinned daily counts."""
    daily = ic.fixture()["seir"][:ic.D]
    counts = np.full(daily.shape, np.nan)
    counts[:, 0] = daily[:, 0]
    counts[2::3, 1:] = daily[:, 1:].reshape(-1, 3, 2).sum(axis=1)
    r = ic.restate(counts, "seir", ic.THETA["seir"], False, 0.5, cumulate=True)
    eng = make_engine("seir", ic.N, ic.D + 2)
    lz, st = eng.run_incidence([ic.THETA["seir"]], 0.5, ic.KEY, ic.F, counts, cumulate=True)
    assert_pass(eng, 0, lz[0], st[0], r)
    eng.close()


def test_a_chain_that_dies_inside_a_batch_leaves_the_others_untouched():
    counts = ic.daily("sir", False, (0, 1))
    eng = make_engine("sir", ic.N, ic.D + 2, chains=3)
    th = [b[0] for b in ic.BATCH]
    pr = [b[1] for b in ic.BATCH]
    keys = [b[2] for b in ic.BATCH]
    for cumulate in (False, True):
        lz, st = eng.run_incidence(th, pr, keys, ic.F, counts, cumulate=cumulate)
        assert st.tolist() == [0, 1, 0]
        for c, (t, p, k) in enumerate(ic.BATCH):
            r = ic.restate(counts, "sir", t, False, p, key=k, cumulate=cumulate)
            assert_pass(eng, c, lz[c], st[c], r)
        assert np.isneginf(lz[1, 3:]).all() and np.isfinite(lz[1, :3]).all()
    # an inactive chain runs nothing: status skipped, NaN log_zetas, the others as before
    lz3, st3 = eng.run_incidence(th, pr, keys, ic.F, counts, cumulate=True, active=[1, 0, 1])
    assert st3.tolist() == [0, 2, 0] and np.isnan(lz3[1]).all()
    np.testing.assert_array_equal(lz3[[0, 2]], lz[[0, 2]])
    eng.close()


# ------------------------------------------------------------------------------------------- 3. the history calls
def test_history_path_sample_and_smooth_see_the_pass():
    counts = ic.mixed()
    T = ic.D + 2
    eng = make_engine("sir", ic.N, T + 5)                # t_max beyond the run length: the calls use D + 2 rows
    eng.set_observations(np.zeros((4, 3)))               # other observations on the context: untouched, not used
    lz, st = eng.run_incidence([(0.8, 0.3)], 0.5, ic.KEY, ic.F, counts, cumulate=True)
    r = ic.restate(counts, "sir", (0.8, 0.3), False, 0.5, cumulate=True)
    assert st[0] == 0 and eng.run_T == T and eng.T == 4   # T stays the observations'
    hid, anc = eng.history(1)
    assert hid.shape == (1, T, ic.N, 3)
    np.testing.assert_array_equal(hid[0], r["hidden"])
    np.testing.assert_array_equal(anc[0], r["ancestry"])
    hf, af = r["hidden"].astype(np.float64), r["ancestry"].astype(np.float64)
    paths, visited = sh.reference_paths(hf, af)
    for k in (0, 17, ic.N - 1):                          # the last row is the one resampled on day D's weights
        np.testing.assert_array_equal(eng.path_sample([k])[0], paths[k])
    want = sh.path_statistics(*sh.genealogy_paths(hf, af))
    sh.assert_smoothed_equal(_first(eng.smooth(1, quantiles=sh.QS, lineage="genealogy")), *want, ic.N)
    want = sh.path_statistics(paths, visited)
    sh.assert_smoothed_equal(_first(eng.smooth(1, quantiles=sh.QS, lineage="reference")), *want, ic.N)
    import smoothing_lag_helpers as slh
    got = _first(eng.smooth(1, quantiles=sh.QS, lineage="genealogy", lag=3))
    sh.assert_smoothed_equal(got, *slh.lag_brute_force(r["hidden"], r["ancestry"], "genealogy", 3, sh.QS), ic.N)
    # observations loaded after the pass (fewer rows than D + 2, then the same again: the binding's early return) do not
    # move the rows the history calls are sized by
    eng.set_observations(np.ones((3, 3)))
    eng.set_observations(np.ones((3, 3)))
    assert eng.T == 3 and eng.run_T == T
    hid2, anc2 = eng.history(1)
    np.testing.assert_array_equal(hid2, hid)
    np.testing.assert_array_equal(anc2, anc)
    np.testing.assert_array_equal(eng.path_sample([17])[0], paths[17])
    assert eng.smooth(1, quantiles=None).sums.shape == (1, T, 3)
    # a filter on the observations afterwards runs over their rows
    lz4, _ = eng.run([(0.8, 0.3)], 0.0, ic.KEY, ic.F)
    assert lz4.shape == (1, 3) and eng.run_T == 3 and eng.history(1)[0].shape == (1, 3, ic.N, 3)
    eng.close()


def _first(s):
    from epipf.smoothing import Smoothed
    return Smoothed(s.mean[0], None if s.quantiles is None else s.quantiles[0], s.lineages[0], s.sums[0], None)


# ------------------------------------------------------------------------------------------- 4. the public functions
def test_incidence_mcmc_equals_the_engine_double_run(monkeypatch):
    """theta, acceptances and trajectories bit for bit at the pinned seed (tests/test_incidence_host.py checks that no
    decision of it lies within 1e-6 of its boundary)."""
    import incidence_oracle_engine as ioe
    from epipf import incidence
    dev = ic.mcmc_run()
    monkeypatch.setattr(incidence._engine, "get_engine", ioe.fake_get_engine)
    cpu = ic.mcmc_run()
    for a, b in zip(dev, cpu):
        np.testing.assert_array_equal(a.thetas, b.thetas)
        np.testing.assert_array_equal(a.sampled_trajs, b.sampled_trajs)
        assert a.acceptances == b.acceptances and a.filters_run == b.filters_run
        np.testing.assert_allclose(a.log_likelihoods, b.log_likelihoods, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("cols,flows", [((0, 1), ("infections", "removals")), ((0,), ("infections",))])
def test_does_it_work_on_the_device(cols, flows):
    """loglik at (0.8, 0.3) minus loglik at (0.4, 0.3), N = 200, index 0, keys 1..4: at least half the smallest gap of
    DESIGN.md §19's table, as on the CPU (tests/test_incidence_restatement.py)."""
    import epipf
    from test_incidence_restatement import GAPS
    cases = ic.fixture()["sir"][:, list(cols)]
    res = epipf.incidence_filter(cases, "sir", [(0.8, 0.3), (0.4, 0.3)] * 4, flows=flows, probs=0.5, n_particles=200,
                                 n_population=ic.NPOP, mu=ic.MU, keys=[1, 1, 2, 2, 3, 3, 4, 4], filter_index=0)
    assert (res.status == 0).all() and res.log_zetas.shape == (8, 26)
    gaps = res.loglik[0::2] - res.loglik[1::2]
    print("gaps", cols, gaps.tolist())
    np.testing.assert_allclose(gaps, GAPS[cols], atol=0.06)
    assert gaps.min() > 0.5 * min(GAPS[cols])
    assert res.best in (0, 2, 4, 6)


# ------------------------------------------------------------------------------------------- 5. refusals
def test_every_refusal_of_the_entry_point():
    from epipf import _lib
    from epipf.engine import Engine
    eng = make_engine("sir", 16, 6, chains=2)
    ok = np.array([[1.0, 2.0], [3.0, np.nan]])
    th = [(0.8, 0.3)]

    def refused(match, *a, **k):
        with pytest.raises(_lib.EpipfError, match=match) as e:
            eng.run_incidence(*a, **k)
        assert "(%d)" % _lib.EINVAL in str(e.value)

    refused("D=5", th, 0.5, 1, 0, np.full((5, 2), np.nan))                      # D + 2 > t_max
    refused(r"counts\[1\]\[0\]=-3", th, 0.5, 1, 0, [[1.0, 2.0], [-3.0, 1.0]])
    refused(r"counts\[0\]\[1\]=inf", th, 0.5, 1, 0, [[1.0, np.inf], [3.0, 1.0]])
    refused(r"counts\[1\]\[1\]=2.5.*integer", th, 0.5, 1, 0, [[1.0, 2.0], [3.0, 2.5]])
    refused(r"theta\[0\]\[1\]=-0.3", [(0.8, -0.3)], 0.5, 1, 0, ok)
    refused(r"theta\[1\]\[0\]=nan", [(0.8, 0.3), (np.nan, 0.3)], 0.5, 1, 0, ok)
    refused(r"probs\[0\]=1.5", th, 1.5, 1, 0, ok)
    refused(r"probs\[1\]=nan", [(0.8, 0.3)] * 2, [0.5, np.nan], 1, 0, ok)
    refused(r"probs\[0\]=-0.1", th, -0.1, 1, 0, ok, observations=True)
    refused("n_chains=3", [(0.8, 0.3)] * 3, 0.5, 1, 0, ok)
    refused("theta has 3 entries", [(0.8, 0.3, 0.1)], 0.5, 1, 0, ok)
    with pytest.raises(ValueError):
        eng.run_incidence(th, 0.5, 1, 0, np.ones((2, 3)))                       # SEIR's columns on a SIR engine
    with pytest.raises(_lib.EpipfError, match="D=0"):
        eng.run_incidence(th, 0.5, 1, 0, np.ones((0, 2)))
    # non-integer reports and a noise ratio above 1 are the normal model's to take; an inactive chain's theta is not read
    _, st = eng.run_incidence(th, 1.5, 1, 0, [[1.0, 2.5]], observations=True)
    _, st = eng.run_incidence([(0.8, 0.3), (-1.0, np.nan)], [0.5, 7.0], 1, 0, ok, active=[1, 0])
    assert st.tolist() == [0, 2]
    # the pass is not a random-walk filter's: epipf_walk_history is EPIPF_ESTATE after it
    with pytest.raises(_lib.EpipfError, match=r"\(%d\)" % _lib.ESTATE):
        eng.walk_history(1)
    eng.close()
    fresh = Engine("sir", 1, 16, 6, 1)
    with pytest.raises(_lib.EpipfError, match=r"\(%d\).*epipf_set_population" % _lib.ESTATE):
        fresh.run_incidence(th, 0.5, 1, 0, ok)
    fresh.close()
    sub = Engine("sir_subgroups", 2, 16, 6, 1)          # the library's own refusal, past the binding's column check
    sub.set_population([150, 150], [3, 3])
    th5, one = np.full((1, 5), 0.5), np.array([0.5])
    key, f = np.array([1], dtype=np.uint64), np.array([0], dtype=np.uint32)
    lz, st = np.empty((1, 4)), np.empty(1, dtype=np.int32)
    rc = _lib.load().epipf_run_incidence(sub._h, 1, _lib.ptr(th5), 5, _lib.OBS_BINOMIAL, _lib.ptr(one), _lib.ptr(key),
                                         _lib.ptr(f), None, _lib.ptr(np.ascontiguousarray(ok)), 2, 0, _lib.ptr(lz),
                                         _lib.ptr(st))
    assert rc == _lib.EINVAL and b"SIR and SEIR" in _lib.load().epipf_last_error()
    sub.close()


ENOMEM_SCRIPT = """
import numpy as np
from epipf import _lib
from epipf.engine import Engine
eng = Engine("sir", 1, 1000, 5, 2)
eng.set_population(300, 5)
c = np.ones((3, 2))
lz, st = eng.run_incidence([(0.8, 0.3)], 0.5, 1, 0, c, cumulate=True)            # 16000 bytes: within the budget
try:
    eng.run_incidence([(0.8, 0.3)] * 2, 0.5, 1, 0, c, cumulate=True)            # 32000 bytes: over it
    raise SystemExit("no error")
except _lib.EpipfError as e:
    assert "(%d)" % _lib.ENOMEM in str(e) and "32000 bytes" in str(e) and "20000" in str(e), str(e)
lz2, st2 = eng.run_incidence([(0.8, 0.3)] * 2, 0.5, 1, 0, c, cumulate=False)     # no accumulator: runs
lz3, st3 = eng.run_incidence([(0.8, 0.3)], 0.5, 1, 0, c, cumulate=True)          # and the context still works
assert np.array_equal(lz, lz3) and np.array_equal(lz2[0], lz[0])
print("enomem ok")
"""


def test_accumulator_over_its_budget_is_enomem_naming_the_bytes():
    """EPIPF_INCIDENCE_ACC_BYTES is read at epipf_create, so a fresh process (the subject of this test) sets it."""
    from conftest import PKG, REPO
    env = dict(os.environ, EPIPF_INCIDENCE_ACC_BYTES="20000", PYTHONPATH=os.pathsep.join([PKG, REPO]))
    out = subprocess.run([sys.executable, "-c", ENOMEM_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "enomem ok" in out.stdout, out.stdout + out.stderr
