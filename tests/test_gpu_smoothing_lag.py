"""The fixed-lag smoother on the device (epipf_smooth_lag, epipf_smooth_lag_history; csrc/epipf_smooth_lag.hip) against
the numpy backend of epipf.smoothing and the brute force that walks every particle of a window's end day back
(tests/smoothing_lag_helpers.py).  Integers throughout: every comparison is assert_array_equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_smoothing as base
from conftest import PKG, REPO, case_args
from smoothing_helpers import QS, assert_smoothed_equal, random_history
from smoothing_lag_helpers import lag_brute_force, lags_for

pytestmark = pytest.mark.gpu

LINEAGES = ("reference", "genealogy")
_same = base._same


def _both(hid, anc, **kw):
    from epipf import smooth_history
    got = smooth_history(hid, anc, backend="gpu", **kw)
    _same(got, smooth_history(hid, anc, backend="numpy", **kw))
    return got


def _gpu_lags(T):
    return lags_for(T, fixed=(0, 1, 2))


# 64 threads up to N = 64, then multiples of 64 up to 1024 (one stride, a partial wave, two and three strides); T = 1 and
# T = 2 have no window the kernel walks (L >= T - 1 is the smoother), T >= 3 has; C = 64 is the most a workgroup sums
EDGES = [(5, 1, 3, "random"), (5, 63, 3, "random"), (5, 64, 4, "random"), (5, 65, 6, "random"),
         (4, 1025, 3, "random"), (1, 70, 3, "random"), (2, 70, 15, "random"), (6, 130, 3, "last"),
         (6, 130, 4, "identity"), (6, 130, 6, "permutation"), (3, 2055, 15, "permutation"), (3, 70, 24, "random"),
         (2, 1, 64, "random")]


def _hand_made(T, N, C, how, lags=None):
    rng = np.random.default_rng(1000 * T + N + C)
    hid, anc = random_history(rng, T, N, C, ancestry=how)
    for lineage in LINEAGES:
        for L in _gpu_lags(T) if lags is None else lags:
            got = _both(hid, anc, quantiles=QS, lineage=lineage, lag=L)
            assert_smoothed_equal(got, *lag_brute_force(hid, anc, lineage, L), N)
            none = _both(hid, anc, quantiles=None, lineage=lineage, lag=L)
            np.testing.assert_array_equal(none.sums, got.sums)
            np.testing.assert_array_equal(none.lineages, got.lineages)
            if how == "last" and L >= 1:                 # one lineage wherever the window has a step
                assert list(got.lineages) == [1] * (T - 1) + [N]
            if how in ("identity", "permutation") and lineage == "genealogy":
                assert list(got.lineages) == [N] * T


@pytest.mark.parametrize("T,N,C,how", EDGES)
def test_hand_made_histories(T, N, C, how):
    _hand_made(T, N, C, how)


def test_several_clipped_windows():
    """T = 40: at L = 7 the last seven days share the end day T - 1, at L = 38 all but day 0 do, at L = 1 one does."""
    _hand_made(40, 200, 3, "random", lags=(1, 7, 38))


def test_the_limits_are_the_existing_device_entry_points():
    from epipf import smooth_history
    rng = np.random.default_rng(21)
    for T, N, C in ((7, 200, 4), (1, 70, 3)):
        hid, anc = random_history(rng, T, N, C)
        for lineage in LINEAGES:
            kw = dict(quantiles=QS, lineage=lineage)
            smoothing = smooth_history(hid, anc, kind="smoothing", **kw)
            for L in (T - 1, T, T + 3, 2**40):
                _same(smooth_history(hid, anc, lag=L, **kw), smoothing)
            _same(smooth_history(hid, anc, lag=0, **kw), smooth_history(hid, anc, kind="predictive", **kw))


def test_lineages_do_not_increase_with_the_lag():
    from epipf import smooth_history
    rng = np.random.default_rng(22)
    hid, anc = random_history(rng, 12, 300, 3)
    before = np.full(12, 300)
    for L in range(0, 13):
        got = smooth_history(hid, anc, quantiles=None, lag=L)
        assert np.all(got.lineages <= before), L
        before = got.lineages
    assert before[0] < 300


def test_a_count_equal_to_bins_minus_one_and_beyond():
    rng = np.random.default_rng(23)
    hid, anc = random_history(rng, 5, 100, 3, top=40)
    hid[1, :, 2] = 40                                    # bins - 1 with the default bins: the last value counted
    got = _both(hid, anc, quantiles=QS, lag=2)
    assert np.all(got.quantiles[:, 1, 2] == 40)
    hid[2, :60, 0] = 57                                  # beyond bins = 41: dropped, never stored
    got = _both(hid, anc, quantiles=QS, bins=41, lag=0)  # m = 1: 60 of the 100 are dropped
    assert got.quantiles[-1, 2, 0] == 41 and got.quantiles[0, 2, 0] < 41
    _both(hid, anc, quantiles=QS, bins=41, lag=2)


def _batch(top=50):
    rng = np.random.default_rng(24)
    hs = [random_history(rng, 8, 300, 3, top=top, ancestry=how) for how in ("random", "last", "permutation")]
    return np.stack([h for h, _ in hs]), np.stack([a for _, a in hs])


def test_a_batch_keeps_its_chains_apart():
    from epipf import smooth_history
    hid, anc = _batch()
    for L in (1, 3):
        got = _both(hid, anc, quantiles=QS, lag=L)
        assert got.mean.shape == (3, 8, 3) and got.quantiles.shape == (3, len(QS), 8, 3)
        for i in range(3):
            _same(smooth_history(hid[i], anc[i], quantiles=QS, lag=L),
                  smooth_history(hid[i], anc[i], quantiles=QS, lag=L, backend="numpy"))
            assert_smoothed_equal(smooth_history(hid[i], anc[i], quantiles=QS, lag=L),
                                  *lag_brute_force(hid[i], anc[i], "genealogy", L), 300)


def test_slices_give_the_unsliced_result(monkeypatch):
    """Three chains whose histograms (8 x 3 x 30001 x 4 B = 2.9 MB each) do not fit a 4 MiB budget together: one chain
    per slice, then with the rows in global memory as well."""
    hid, anc = _batch(top=30000)
    whole = _both(hid, anc, quantiles=QS, lag=3)
    monkeypatch.setenv("EPIPF_SMOOTH_SCRATCH_MB", "4")
    _same(_both(hid, anc, quantiles=QS, lag=3), whole)
    monkeypatch.setenv("EPIPF_SMOOTH_LDS", "0")
    _same(_both(hid, anc, quantiles=QS, lag=3), whole)


def test_global_rows_above_the_lds_limit_and_days_in_slices(monkeypatch):
    """N = 16,385 is the first size whose rows live in global memory.  At N = 60,000 a workgroup's two rows are 480 kB,
    so under a 1 MiB budget a chain's six days run two per launch, with and without the histogram beside them."""
    rng = np.random.default_rng(25)
    hid, anc = random_history(rng, 3, 16385, 3)
    _both(hid, anc, quantiles=QS, lag=1)
    hid, anc = random_history(rng, 6, 60000, 3)
    hid, anc = np.stack([hid, hid[:, ::-1]]), np.stack([anc, anc])
    whole = _both(hid, anc, quantiles=QS, lag=2)
    monkeypatch.setenv("EPIPF_SMOOTH_SCRATCH_MB", "1")
    _same(_both(hid, anc, quantiles=QS, lag=2), whole)
    none = _both(hid, anc, quantiles=None, lag=2)
    np.testing.assert_array_equal(none.sums, whole.sums)
    np.testing.assert_array_equal(none.lineages, whole.lineages)


CHILD = r"""
import sys, os
sys.path[:0] = [{tests!r}, {pkg!r}, {repo!r}]
assert os.environ["EPIPF_SMOOTH_LDS"] == "0"
import test_gpu_smoothing_lag as t
n = 0
for case in t.EDGES:
    t._hand_made(*case)
    n += 1
t.test_several_clipped_windows()
t.test_a_batch_keeps_its_chains_apart()
print("global-row fixed-lag cases green:", n + 2, flush=True)
"""


def test_global_multiplicity_rows_in_a_fresh_process():
    """EPIPF_SMOOTH_LDS=0: the rows in global memory instead of LDS, at sizes where both paths run."""
    code = CHILD.format(tests=os.path.join(REPO, "tests"), pkg=PKG, repo=REPO)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EPIPF_")}
    env["EPIPF_SMOOTH_LDS"] = "0"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "global-row fixed-lag cases green: %d" % (len(EDGES) + 2) in r.stdout, r.stdout[-2000:]


# ----------------------------------------------------------------------------------------- after a real filter run
def _engine_against_numpy(eng, n, bins, **kw):
    from epipf import smooth_history
    hid, anc = eng.history(n)
    got = eng.smooth(n, **kw)
    _same(got, smooth_history(hid, anc, backend="numpy", bins=bins, **kw))
    return got


@pytest.mark.parametrize("model,G,N", [("sir", 1, 100), ("sir", 1, 600), ("seir", 1, 100), ("sir_subgroups", 2, 100),
                                       ("sir_subgroups", 5, 100)])
def test_engine_smooth_equals_numpy_on_its_history(datasets_golden, model, G, N):
    from epipf.engine import Engine, model_id, theta_vector
    c = base._filter_case(datasets_golden, model, G)
    th, G_ = theta_vector(model_id(model), c["theta"])
    chains, T = 4, c["Y"].shape[0]
    eng = Engine(model, G_, N, T + 3, chains + 2)        # t_max > T, max_chains > n_chains: real strides
    try:
        eng.set_observations(c["Y"])
        eng.set_population(c["npop"], c["mu"])
        lz, st = eng.run(np.repeat(th[None], chains, 0), 0.1, np.arange(chains) + 11, np.arange(chains))
        assert np.all(st == 0)
        bins = int(np.sum(c["npop"])) + 1
        for lineage in LINEAGES:
            for L in (1, 2, T - 2):
                got = _engine_against_numpy(eng, chains, bins, quantiles=QS, lineage=lineage, lag=L)
                assert np.all(got.lineages[:, -1] == N)
                if L == 2:
                    assert np.any(got.lineages < N)      # the windows did something
        _engine_against_numpy(eng, chains, bins, quantiles=None, lag=2)
        _engine_against_numpy(eng, 2, bins, quantiles=(0.5,), lag=2)       # fewer chains than the run's
        _same(eng.smooth(chains, quantiles=QS, lag=0), eng.smooth(chains, quantiles=QS, kind="predictive"))
        _same(eng.smooth(chains, quantiles=QS, lag=T - 1), eng.smooth(chains, quantiles=QS))
        assert eng.smooth(lag=1).mean.shape == (chains, T, eng.C)
    finally:
        eng.close()


def test_chains_that_did_not_run_are_nan_and_zero(datasets_golden):
    from epipf import _lib
    from epipf.engine import Engine
    Y = datasets_golden["sir_binom"]
    eng = Engine("sir", 1, 100, Y.shape[0], 4)
    try:
        eng.set_observations(Y)
        eng.set_population(4820, 20)
        th = np.array([[2.0, 1.0]] * 4)
        keys, fidx = [1, 2, 3, 4], [0, 0, 0, 0]
        eng.run(th, 0.1, keys, fidx)
        clean = eng.smooth(4, quantiles=QS, lag=3)
        # chain 1 degenerate (a detection probability under which every weight is 0), chain 2 skipped
        lz, st = eng.run(th, [0.1, 1e-300, 0.1, 0.1], keys, fidx, active=np.array([1, 1, 0, 1]))
        assert list(st) == [_lib.STATUS_OK, _lib.STATUS_DEGENERATE, _lib.STATUS_SKIPPED, _lib.STATUS_OK]
        got = eng.smooth(4, quantiles=QS, lag=3)
        for i in (1, 2):
            assert np.all(np.isnan(got.mean[i]))
            assert not got.sums[i].any() and not got.quantiles[i].any() and not got.lineages[i].any()
        for i in (0, 3):
            for field in ("mean", "sums", "quantiles", "lineages"):
                np.testing.assert_array_equal(getattr(got, field)[i], getattr(clean, field)[i])
    finally:
        eng.close()


def test_particle_smoother_is_the_filter_then_the_smoother(filter_golden):
    from epipf import particle_filter, particle_smoother, seed_stream, smooth_history
    from epipf import pmcmc
    a = case_args(filter_golden["filter_seir_binom"])
    args = (a["Y"], "seir", np.array(a["theta"]), False, a["probs"], 300, a["npop"], a["mu"])
    seed_stream(77, 5)
    z, hid, anc = particle_filter(*args)
    after_filter = pmcmc._STREAM.next_filter
    seed_stream(77, 5)
    got = particle_smoother(*args, quantiles=QS, lag=3)
    assert pmcmc._STREAM.next_filter == after_filter == 6    # exactly one filter index
    want = smooth_history(hid, anc, quantiles=QS, lag=3, backend="numpy", bins=int(a["npop"]) + 1)
    np.testing.assert_array_equal(got.zetas, z)
    _same(got, want)
    assert got.mean.shape == (a["Y"].shape[0], 4)


def test_larger_case_on_the_large_n_path(datasets_golden):
    """N = 10,000: above the default dynamic LDS (two rows are 80 KB) and ten strides of the 1024-thread workgroup."""
    from epipf.engine import Engine
    Y = datasets_golden["cfg2_binom"][:20]              # BASELINE config 2's first 20 days, its theta and population
    eng = Engine("sir", 1, 10000, 20, 1)
    try:
        eng.set_observations(Y)
        eng.set_population(10000, 20)
        lz, st = eng.run(np.array([[0.25, 0.1]]), 0.1, 9, 0)
        assert st[0] == 0
        got = _engine_against_numpy(eng, 1, 10001, quantiles=QS, lag=5)
        assert got.lineages[0, -1] == 10000 and got.lineages[0, 0] < 10000
        full = eng.smooth(1, quantiles=None)
        assert np.all(got.lineages >= full.lineages) and got.lineages[0, 0] > full.lineages[0, 0]
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------- the C ABI's refusals
def _call_lag(L, h, n, lineage=1, lag=2, q=(0.5,), bins=10, T=15, C=3, quant=True):
    qa = np.asarray(q, dtype=np.float64)
    sums = np.zeros((max(n, 1), T, C), dtype=np.int64)
    lin = np.zeros((max(n, 1), T), dtype=np.int32)
    qo = np.zeros((max(n, 1), max(qa.size, 1), T, C), dtype=np.int32) if quant else None
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return L.epipf_smooth_lag(h, n, lineage, lag, p(qa) if qa.size else None, qa.size, bins, p(sums), p(qo), p(lin))


def test_state_and_argument_errors(datasets_golden):
    from epipf import _lib
    from epipf.engine import Engine
    L = _lib.load()
    Y = datasets_golden["sir_binom"]
    eng = Engine("sir", 1, 64, Y.shape[0], 3)
    try:
        eng.set_observations(Y)
        eng.set_population(4820, 20)
        assert _call_lag(L, eng._h, 1) == _lib.ESTATE
        with pytest.raises(_lib.EpipfError, match="no filter has run"):
            eng.smooth(lag=1)
        eng.run(np.array([[2.0, 1.0]] * 2), 0.1, [1, 2], [0, 0])
        assert _call_lag(L, eng._h, 2, bins=4821) == _lib.OK
        assert _call_lag(L, eng._h, 2, q=(), quant=False, bins=0) == _lib.OK        # means and lineages only
        assert _call_lag(L, eng._h, 2, bins=4821, lag=-1) == _lib.EINVAL
        assert b"lag" in L.epipf_last_error()
        for bad in (dict(n=0), dict(n=3), dict(q=(1.5,)), dict(q=(float("nan"),)), dict(bins=0), dict(quant=False),
                    dict(lineage=2), dict(lag=-(2**31))):
            kw = dict(n=2, bins=4821)
            kw.update(bad)
            assert _call_lag(L, eng._h, **kw) == _lib.EINVAL, bad
            assert L.epipf_last_error()
        # one chain's histogram above 256 MiB
        assert _call_lag(L, eng._h, 2, bins=2**21) == _lib.EINVAL
        assert b"histogram" in L.epipf_last_error()
        with pytest.raises(_lib.EpipfError):
            eng.smooth(5, lag=1)
        for bad in (dict(lag=True), dict(lag=1.0), dict(lag=-1), dict(lag=1, kind="predictive"),
                    dict(lag=1, kind="filtering")):
            with pytest.raises(ValueError):
                eng.smooth(**bad)
        # epipf_smooth_lag_history: the lag, shapes and contents
        hid = np.zeros((1, 4, 4, 3), dtype=np.int32)
        anc = np.zeros((1, 4, 4), dtype=np.int32)
        q = np.array([0.5])
        sums = np.zeros((1, 4, 3), dtype=np.int64)
        qo = np.zeros((1, 1, 4, 3), dtype=np.int32)
        lin = np.zeros((1, 4), dtype=np.int32)
        out = (_lib.ptr(q), 1, 5, _lib.ptr(sums), _lib.ptr(qo), _lib.ptr(lin))
        assert L.epipf_smooth_lag_history(eng._h, 1, 4, 4, 3, _lib.ptr(hid), _lib.ptr(anc), 1, 1, *out) == _lib.OK
        assert list(lin[0]) == [1, 1, 1, 4]              # every ancestor is particle 0
        assert L.epipf_smooth_lag_history(eng._h, 1, 4, 4, 3, _lib.ptr(hid), _lib.ptr(anc), 1, -1, *out) == _lib.EINVAL
        assert b"lag" in L.epipf_last_error()
        for shape in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3), (1, 4, 4, 0)):
            rc = L.epipf_smooth_lag_history(eng._h, *shape, _lib.ptr(hid), _lib.ptr(anc), 1, 1, *out)
            assert rc == _lib.EINVAL, shape
        anc[0, 1, 2] = 4
        with pytest.raises(_lib.EpipfError, match="ancestors"):
            eng.smooth_history(hid, anc, 1, 0, q, 5, lag=1)
        anc[0, 1, 2] = 0
        hid[0, 1, 2, 1] = -3
        with pytest.raises(_lib.EpipfError, match="non-negative"):
            eng.smooth_history(hid, anc, 1, 0, q, 5, lag=1)
    finally:
        eng.close()


def test_more_compartments_than_the_workgroup_sums_are_refused():
    """kSmoothMaxC = 64 compartments are the kernel's LDS sums: 64 run, 65 are EPIPF_EINVAL."""
    from epipf import _lib
    from epipf.engine import Engine
    L = _lib.load()
    eng = Engine("sir", 1, 1, 1, 1)
    try:
        q = np.array([0.5])
        for C, want in ((64, _lib.OK), (65, _lib.EINVAL)):
            hid = np.ones((1, 3, 4, C), dtype=np.int32)
            anc = np.zeros((1, 3, 4), dtype=np.int32)
            sums = np.zeros((1, 3, C), dtype=np.int64)
            qo = np.zeros((1, 1, 3, C), dtype=np.int32)
            lin = np.zeros((1, 3), dtype=np.int32)
            rc = L.epipf_smooth_lag_history(eng._h, 1, 3, 4, C, _lib.ptr(hid), _lib.ptr(anc), 1, 1, _lib.ptr(q), 1, 5,
                                            _lib.ptr(sums), _lib.ptr(qo), _lib.ptr(lin))
            assert rc == want, C
            if want == _lib.OK:
                assert np.all(sums == 4) and np.all(qo == 1) and list(lin[0]) == [1, 1, 4]
            else:
                assert b"at most 64 compartments" in L.epipf_last_error()
                assert not sums.any()
    finally:
        eng.close()
