"""The smoother on the device (epipf_smooth, epipf_smooth_history; csrc/epipf_smooth.hip) against the numpy backend of
epipf.smoothing and the brute force over sampled paths (tests/smoothing_helpers.py).  Integers throughout: every
comparison is assert_array_equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO, case_args
from smoothing_helpers import (QS, assert_smoothed_equal, genealogy_paths, golden_histories, path_statistics,
                               random_history, reference_paths)

pytestmark = pytest.mark.gpu

THREADS = 1024                                           # kSmoothThreads: the workgroup's largest thread count


def _same(got, want):
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.lineages, want.lineages)
    np.testing.assert_array_equal(got.mean, want.mean)
    if want.quantiles is None:
        assert got.quantiles is None
    else:
        np.testing.assert_array_equal(got.quantiles, want.quantiles)


def _both(hid, anc, **kw):
    from epipf import smooth_history
    got = smooth_history(hid, anc, backend="gpu", **kw)
    want = smooth_history(hid, anc, backend="numpy", **kw)
    _same(got, want)
    return got


@pytest.fixture(scope="module")
def histories(filter_golden):
    return golden_histories(filter_golden)


def test_golden_histories_every_lineage_and_kind(histories):
    for name, hid, anc in histories:
        N = hid.shape[1]
        for lineage, walk in (("reference", reference_paths), ("genealogy", genealogy_paths)):
            got = _both(hid, anc, quantiles=QS, lineage=lineage)
            assert_smoothed_equal(got, *path_statistics(*walk(hid, anc)), N)
            got = _both(hid, anc, quantiles=QS, lineage=lineage, kind="predictive")
            np.testing.assert_array_equal(got.lineages, np.full(hid.shape[0], N))
            np.testing.assert_array_equal(got.sums, np.rint(hid.sum(1)).astype(np.int64))


EDGES = [(T, N, C, how)
         for T, N, C, how in [(5, 1, 3, "random"), (5, 63, 3, "random"), (5, 64, 4, "random"), (5, 65, 6, "random"),
                              (4, THREADS + 1, 3, "random"), (1, 70, 3, "random"), (2, 70, 15, "random"),
                              (6, 130, 3, "last"), (6, 130, 4, "identity"), (6, 130, 6, "permutation"),
                              (3, 2 * THREADS + 7, 15, "permutation"),
                              # G = 8 histories have C = 24; C = 64 is kSmoothMaxC, and with N = 1 the workgroup is one
                              # wave in which every thread owns a compartment's sum
                              (3, 70, 24, "random"), (2, 1, 64, "random")]]


@pytest.mark.parametrize("T,N,C,how", EDGES)
def test_hand_made_histories(T, N, C, how):
    rng = np.random.default_rng(1000 * T + N + C)
    hid, anc = random_history(rng, T, N, C, ancestry=how)
    for lineage in ("reference", "genealogy"):
        got = _both(hid, anc, quantiles=QS, lineage=lineage)
        _both(hid, anc, quantiles=None, lineage=lineage)
        if how == "last" and T > 1:                      # one lineage carrying all N before the last day
            assert list(got.lineages) == [1] * (T - 1) + [N]
            shift = lineage == "genealogy"
            np.testing.assert_array_equal(got.sums[T - 2], N * hid[T - 2, N - 1 if T - 2 + shift > 0 else 0]
                                          .astype(np.int64))
        if how in ("identity", "permutation") and lineage == "genealogy":
            assert list(got.lineages) == [N] * T
    _both(hid, anc, quantiles=QS, kind="predictive")


def test_a_count_equal_to_bins_minus_one_and_beyond():
    rng = np.random.default_rng(2)
    hid, anc = random_history(rng, 4, 100, 3, top=40)
    hid[1, :, 2] = 40                                    # bins - 1 with the default bins: the last value counted
    got = _both(hid, anc, quantiles=QS)
    assert np.all(got.quantiles[:, 1, 2] == 40)
    hid[2, :60, 0] = 57                                  # beyond bins = 41: dropped, never stored
    got = _both(hid, anc, quantiles=QS, bins=41, kind="predictive")
    assert got.quantiles[-1, 2, 0] == 41 and got.quantiles[0, 2, 0] < 41


def test_a_batch_keeps_its_chains_apart():
    rng = np.random.default_rng(3)
    hs = [random_history(rng, 7, 200, 4, ancestry=how) for how in ("random", "last", "permutation")]
    hid, anc = np.stack([h for h, _ in hs]), np.stack([a for _, a in hs])
    from epipf import smooth_history
    got = _both(hid, anc, quantiles=QS)
    assert got.mean.shape == (3, 7, 4) and got.quantiles.shape == (3, len(QS), 7, 4)
    for i in range(3):
        _same(smooth_history(hid[i], anc[i], quantiles=QS), smooth_history(hid[i], anc[i], quantiles=QS,
                                                                           backend="numpy"))
        np.testing.assert_array_equal(got.sums[i], smooth_history(hid[i], anc[i], quantiles=None).sums)


def test_slices_give_the_unsliced_result(monkeypatch):
    """Five chains whose histograms (8 x 3 x 30001 x 4 B = 2.9 MB each) do not fit a 4 MiB budget together: one chain
    per slice."""
    rng = np.random.default_rng(4)
    hs = [random_history(rng, 8, 300, 3, top=30000) for _ in range(5)]
    hid, anc = np.stack([h for h, _ in hs]), np.stack([a for _, a in hs])
    whole = _both(hid, anc, quantiles=QS)
    monkeypatch.setenv("EPIPF_SMOOTH_SCRATCH_MB", "4")
    _same(_both(hid, anc, quantiles=QS), whole)
    monkeypatch.setenv("EPIPF_SMOOTH_LDS", "0")          # the global multiplicity rows are sliced with the histogram
    _same(_both(hid, anc, quantiles=QS), whole)


CHILD = r"""
import sys, os
sys.path[:0] = [{tests!r}, {pkg!r}, {repo!r}]
assert os.environ["EPIPF_SMOOTH_LDS"] == "0"
import numpy as np
import conftest
import test_gpu_smoothing as t
t.test_golden_histories_every_lineage_and_kind(t.golden_histories(conftest.load_golden("filter_golden.npz")))
n = 1
for case in t.EDGES:
    t.test_hand_made_histories(*case)
    n += 1
t.test_a_batch_keeps_its_chains_apart()
t.test_larger_case_on_the_large_n_path(dict(np.load(os.path.join(conftest.GOLDEN, "datasets.npz"))))
print("global-row smoother cases green:", n + 2, flush=True)
"""


def test_global_multiplicity_rows_in_a_fresh_process():
    """EPIPF_SMOOTH_LDS=0: the rows in global memory instead of LDS, at sizes where both paths run."""
    code = CHILD.format(tests=os.path.join(REPO, "tests"), pkg=PKG, repo=REPO)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EPIPF_")}
    env["EPIPF_SMOOTH_LDS"] = "0"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "global-row smoother cases green: %d" % (len(EDGES) + 3) in r.stdout, r.stdout[-2000:]


# ----------------------------------------------------------------------------------------- after a real filter run
def _filter_case(datasets_golden, model, G=2):
    if model == "sir":
        return dict(Y=datasets_golden["sir_binom"], theta=(2.0, 1.0), npop=4820, mu=20)
    if model == "seir":
        return dict(Y=datasets_golden["seir_binom"], theta=(4.0, 1.0, 1.0), npop=4820, mu=20)
    if G == 2:
        return dict(Y=datasets_golden["sub_binom"][:8], theta=(np.array([[5.0, 2.0], [1.0, 3.0]]), 0.5),
                    npop=np.array([2030.0, 3040.0]), mu=np.array([30.0, 40.0]))
    beta = np.random.RandomState(G).uniform(0.5, 3.0, (G, G))
    return dict(Y=np.tile(datasets_golden["sub_binom"][:6, :3], (1, G)), theta=(beta, 0.7), npop=np.full(G, 1500.0),
                mu=np.full(G, 15.0))


def _engine_against_numpy(eng, n, bins, **kw):
    from epipf import smooth_history
    hid, anc = eng.history(n)
    got = eng.smooth(n, **kw)
    want = smooth_history(hid, anc, backend="numpy", bins=bins, **kw)
    _same(got, want)
    return got


@pytest.mark.parametrize("model,G,N", [("sir", 1, 100), ("sir", 1, 600), ("seir", 1, 100), ("sir_subgroups", 2, 100),
                                       ("sir_subgroups", 5, 100)])
def test_engine_smooth_equals_numpy_on_its_history(datasets_golden, model, G, N):
    from epipf.engine import Engine, model_id, theta_vector
    c = _filter_case(datasets_golden, model, G)
    th, G_ = theta_vector(model_id(model), c["theta"])
    chains = 4
    eng = Engine(model, G_, N, c["Y"].shape[0] + 3, chains + 2)       # t_max > T, max_chains > n_chains: real strides
    try:
        eng.set_observations(c["Y"])
        eng.set_population(c["npop"], c["mu"])
        lz, st = eng.run(np.repeat(th[None], chains, 0), 0.1, np.arange(chains) + 11, np.arange(chains))
        assert np.all(st == 0)
        bins = int(np.sum(c["npop"])) + 1
        coalesced = False
        for lineage in ("genealogy", "reference"):
            got = _engine_against_numpy(eng, chains, bins, quantiles=QS, lineage=lineage)
            coalesced |= bool(np.any(got.lineages < N))
            assert np.all(got.lineages[:, -1] == N)
        assert coalesced                                 # the backward pass did something
        _engine_against_numpy(eng, chains, bins, quantiles=QS, kind="predictive")
        _engine_against_numpy(eng, chains, bins, quantiles=None)
        _engine_against_numpy(eng, 2, bins, quantiles=(0.5,))          # fewer chains than the run's
        assert eng.smooth().mean.shape == (chains, c["Y"].shape[0], eng.C)
    finally:
        eng.close()


def test_chains_that_did_not_run_are_nan_and_zero(datasets_golden, filter_golden):
    from epipf import _lib, particle_smoother
    from epipf.engine import Engine
    Y = datasets_golden["sir_binom"]
    eng = Engine("sir", 1, 100, Y.shape[0], 4)
    try:
        eng.set_observations(Y)
        eng.set_population(4820, 20)
        th = np.array([[2.0, 1.0]] * 4)
        keys, fidx = [1, 2, 3, 4], [0, 0, 0, 0]
        eng.run(th, 0.1, keys, fidx)
        clean = eng.smooth(4, quantiles=QS)
        # chain 1 degenerate (a detection probability under which every weight is 0), chain 2 skipped
        lz, st = eng.run(th, [0.1, 1e-300, 0.1, 0.1], keys, fidx, active=np.array([1, 1, 0, 1]))
        assert list(st) == [_lib.STATUS_OK, _lib.STATUS_DEGENERATE, _lib.STATUS_SKIPPED, _lib.STATUS_OK]
        got = eng.smooth(4, quantiles=QS)
        for i in (1, 2):
            assert np.all(np.isnan(got.mean[i]))
            assert not got.sums[i].any() and not got.quantiles[i].any() and not got.lineages[i].any()
        for i in (0, 3):
            for field in ("mean", "sums", "quantiles", "lineages"):
                np.testing.assert_array_equal(getattr(got, field)[i], getattr(clean, field)[i])
    finally:
        eng.close()
    # the degenerate golden itself: its theta and probs on its own observations
    a = case_args(filter_golden["filter_degenerate"])
    assert particle_smoother(a["Y"], "sir", a["theta"], a["observations"], a["probs"], a["N"], a["npop"], a["mu"],
                             key=a["key"], filter_index=0) is None


def test_particle_smoother_is_the_filter_then_the_smoother(filter_golden):
    from epipf import particle_filter, particle_smoother, seed_stream, smooth_history
    from epipf import pmcmc
    a = case_args(filter_golden["filter_seir_binom"])
    args = (a["Y"], "seir", np.array(a["theta"]), False, a["probs"], 300, a["npop"], a["mu"])
    for lineage in ("genealogy", "reference"):
        seed_stream(77, 5)
        z, hid, anc = particle_filter(*args)
        after_filter = pmcmc._STREAM.next_filter
        seed_stream(77, 5)
        got = particle_smoother(*args, quantiles=QS, lineage=lineage)
        assert pmcmc._STREAM.next_filter == after_filter == 6
        want = smooth_history(hid, anc, quantiles=QS, lineage=lineage, backend="numpy",
                              bins=int(a["npop"]) + 1)
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
        got = _engine_against_numpy(eng, 1, 10001, quantiles=QS)
        assert got.lineages[0, -1] == 10000 and got.lineages[0, 0] < 10000
        _engine_against_numpy(eng, 1, 10001, quantiles=QS, lineage="reference")
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------- the C ABI's refusals
def _call_smooth(L, h, n, lineage=1, kind=0, q=(0.5,), bins=10, T=15, C=3, quant=True):
    qa = np.asarray(q, dtype=np.float64)
    sums = np.zeros((max(n, 1), T, C), dtype=np.int64)
    lin = np.zeros((max(n, 1), T), dtype=np.int32)
    qo = np.zeros((max(n, 1), max(qa.size, 1), T, C), dtype=np.int32) if quant else None
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return L.epipf_smooth(h, n, lineage, kind, p(qa) if qa.size else None, qa.size, bins, p(sums), p(qo), p(lin))


def test_state_and_argument_errors(datasets_golden):
    from epipf import _lib
    from epipf.engine import Engine
    L = _lib.load()
    Y = datasets_golden["sir_binom"]
    eng = Engine("sir", 1, 64, Y.shape[0], 3)
    try:
        eng.set_observations(Y)
        eng.set_population(4820, 20)
        assert _call_smooth(L, eng._h, 1) == _lib.ESTATE
        with pytest.raises(_lib.EpipfError, match="no filter has run"):
            eng.smooth()
        eng.run(np.array([[2.0, 1.0]] * 2), 0.1, [1, 2], [0, 0])
        assert _call_smooth(L, eng._h, 2, bins=4821) == _lib.OK
        assert _call_smooth(L, eng._h, 2, q=(), quant=False, bins=0) == _lib.OK      # means and lineages only
        for bad in (dict(n=0), dict(n=3), dict(q=(1.5,)), dict(q=(-0.5,)), dict(q=(float("nan"),)), dict(bins=0),
                    dict(quant=False), dict(lineage=2), dict(lineage=-1), dict(kind=2)):
            kw = dict(n=2, bins=4821)
            kw.update(bad)
            assert _call_smooth(L, eng._h, **kw) == _lib.EINVAL, bad
            assert L.epipf_last_error()
        # one chain's histogram above 256 MiB
        assert _call_smooth(L, eng._h, 2, bins=2**21) == _lib.EINVAL
        assert b"histogram" in L.epipf_last_error()
        with pytest.raises(_lib.EpipfError):
            eng.smooth(5)
        for bad in (dict(lineage="true"), dict(kind="filtering"), dict(quantiles=(2.0,))):
            with pytest.raises(ValueError):
                eng.smooth(**bad)
        # epipf_smooth_history: shapes and contents
        hid = np.zeros((1, 2, 4, 3), dtype=np.int32)
        anc = np.zeros((1, 2, 4), dtype=np.int32)
        q = np.array([0.5])
        for shape in ((0, 2, 4, 3), (1, 0, 4, 3), (1, 2, 0, 3), (1, 2, 4, 0)):
            sums = np.zeros((1, 2, 3), dtype=np.int64)
            qo = np.zeros((1, 1, 2, 3), dtype=np.int32)
            lin = np.zeros((1, 2), dtype=np.int32)
            rc = L.epipf_smooth_history(eng._h, *shape, _lib.ptr(hid), _lib.ptr(anc), 1, 0, _lib.ptr(q), 1, 5,
                                        _lib.ptr(sums), _lib.ptr(qo), _lib.ptr(lin))
            assert rc == _lib.EINVAL, shape
        anc[0, 1, 2] = 4
        with pytest.raises(_lib.EpipfError, match="ancestors"):
            eng.smooth_history(hid, anc, 1, 0, q, 5)
        anc[0, 1, 2] = 0
        hid[0, 1, 2, 1] = -3
        with pytest.raises(_lib.EpipfError, match="non-negative"):
            eng.smooth_history(hid, anc, 1, 0, q, 5)
    finally:
        eng.close()


def test_more_compartments_than_the_workgroup_sums_are_refused():
    """kSmoothMaxC = 64 compartments are the kernel's LDS sums: 64 run (EDGES), 65 are EPIPF_EINVAL."""
    from epipf import _lib
    from epipf.engine import Engine
    L = _lib.load()
    eng = Engine("sir", 1, 1, 1, 1)
    try:
        q = np.array([0.5])
        for C, want in ((64, _lib.OK), (65, _lib.EINVAL)):
            hid = np.ones((1, 2, 4, C), dtype=np.int32)
            anc = np.zeros((1, 2, 4), dtype=np.int32)
            sums = np.zeros((1, 2, C), dtype=np.int64)
            qo = np.zeros((1, 1, 2, C), dtype=np.int32)
            lin = np.zeros((1, 2), dtype=np.int32)
            rc = L.epipf_smooth_history(eng._h, 1, 2, 4, C, _lib.ptr(hid), _lib.ptr(anc), 1, 0, _lib.ptr(q), 1, 5,
                                        _lib.ptr(sums), _lib.ptr(qo), _lib.ptr(lin))
            assert rc == want, C
            if want == _lib.OK:
                assert np.all(sums == 4) and np.all(qo == 1)
            else:
                assert b"at most 64 compartments" in L.epipf_last_error()
                assert not sums.any()
        with pytest.raises(_lib.EpipfError, match="at most 64 compartments"):
            eng.smooth_history(np.ones((1, 2, 4, 65), dtype=np.int32), np.zeros((1, 2, 4), dtype=np.int32), 1, 0, q, 5)
    finally:
        eng.close()
