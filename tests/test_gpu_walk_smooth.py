"""The reduction of the parameter history on the GPU (walk_smooth_kernel through epipf_walk_smooth_history and
epipf_walk_smooth) against the brute force of tests/walk_restatement.py: quantiles and lineages bit for
bit, means within the summation bound, a second call with identical bits; on hand-made histories whose values are chosen
to break a radix select or a sort and whose ancestries are chosen to break the backward walk (tests/walk_cases.py), and
on the history resident after a real walk_filter.  Needs an MI355X."""
import numpy as np
import pytest

import if2_cases
import walk_cases as wc
import walk_restatement as wr

pytestmark = pytest.mark.gpu

POP = 300.0


@pytest.fixture(scope="module")
def eng():
    from epipf.engine import Engine
    e = Engine("sir", 1, 1, 1, 1)                        # its own shape is ignored by the host-array entry point
    yield e
    e.close()


def lineage_id(name):
    from epipf import _lib
    return _lib.LINEAGE_GENEALOGY if name == "genealogy" else _lib.LINEAGE_REFERENCE


def check_batch(eng, hid, anc, th, lineage, lag, q, twice=False):
    """One device call over the batch against the brute force, chain by chain."""
    n, T, N = anc.shape
    q = None if q is None or len(q) == 0 else np.asarray(q, dtype=np.float64)
    mean, quant, lin = eng.walk_smooth_history(hid, anc, th, POP, lineage_id(lineage), q, lag=lag)
    assert (quant is None) == (q is None)
    for s in range(n):
        bmean, bqs, blin = wr.brute_force(hid[s], anc[s], th[s], POP, 1 if lineage == "genealogy" else 0, lag, q)
        np.testing.assert_array_equal(lin[s], blin)
        wr.assert_mean_close(mean[s], bmean, N)
        if q is not None:
            np.testing.assert_array_equal(wr.bits(quant[s]), wr.bits(bqs))
    if twice:
        mean2, quant2, lin2 = eng.walk_smooth_history(hid, anc, th, POP, lineage_id(lineage), q, lag=lag)
        np.testing.assert_array_equal(wr.bits(mean2), wr.bits(mean))
        np.testing.assert_array_equal(lin2, lin)
        if q is not None:
            np.testing.assert_array_equal(wr.bits(quant2), wr.bits(quant))
    return mean, quant, lin


# N: one particle, less than a wave, a wave, one more, several waves, more than one particle per thread (1025, 2049);
# T = 1 (no window), 2, 7; C = 3 and 4 alternate, d = 2 and 3 with them
SHAPES = [(1, 1, 3), (1, 7, 4), (5, 2, 4), (5, 7, 3), (64, 1, 4), (64, 7, 3), (65, 7, 4), (65, 2, 3), (300, 7, 3),
          (300, 2, 4), (1025, 7, 4), (2049, 7, 3), (2049, 1, 4)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-T%d-C%d" % s)
def test_hand_made_histories(eng, shape):
    N, T, C = shape
    d = C - 1
    hid, anc, th, names = wc.chains(T, N, C, d, seed=N + T, limit=6 if N > 1000 else None)
    k = 0
    for lineage in ("genealogy", "reference"):
        for L in wc.lags(T):
            Q = k % 6                                    # 0 (null output) .. 5 quantiles
            check_batch(eng, hid, anc, th, lineage, L, wc.QUANTILES[:Q], twice=(k == 1))
            k += 1
    # every quantile on the full smoother and on the cloud, whatever the rotation above gave them
    check_batch(eng, hid, anc, th, "genealogy", None, wc.QUANTILES)
    check_batch(eng, hid, anc, th, "genealogy", 0, wc.QUANTILES)


@pytest.mark.parametrize("values", wc.VALUES)
def test_every_kind_of_values_with_every_kind_of_ancestry(eng, values):
    T, N, C, d = 7, 130, 3, 2
    parts = [wc.history(values, a, T, N, C, d, 11 * i) for i, a in enumerate(wc.ANCESTRIES)]
    hid, anc, th = (np.stack([p[i] for p in parts]) for i in range(3))
    for lineage in ("genealogy", "reference"):
        for L in (1, 3, None):
            check_batch(eng, hid, anc, th, lineage, L, wc.QUANTILES)


def test_the_quantile_lands_on_infinity(eng):
    """gamma = 0 on two thirds of the particles: the median and the upper quantiles of R are +inf, and so is its mean."""
    T, N = 3, 66
    hid, anc, th = wc.history("gamma_zero", "identity", T, N, 3, 2, 5)
    mean, quant, _ = check_batch(eng, hid[None], anc[None], th[None], "genealogy", 1, wc.QUANTILES)
    assert np.isinf(quant[0, 2:, 1, 2]).all() and np.isfinite(quant[0, :2, 1, 2]).all() and np.isinf(mean[0, 1, 2])
    assert np.isfinite(quant[0, 2, 0, 2]) and np.isinf(quant[0, 4, 0, 2])


def test_signed_zeros_and_subnormals_order_as_numbers(eng):
    T, N = 2, 40
    hid, anc, th = wc.history("magnitudes", "identity", T, N, 3, 2, 9)
    _, quant, _ = check_batch(eng, hid[None], anc[None], th[None], "genealogy", 0, wc.QUANTILES)
    # a fifth of the values are +0.0 or -0.0: the minimum is +0.0 in bits, the maximum 1e300
    assert (wr.bits(quant[0, 0, :, 0]) == 0).all() and (quant[0, 4, :, 0] == 1e300).all()


def test_global_rows(eng, monkeypatch):
    """N = 20,000: the multiplicity rows live in global memory, one pair per workgroup; under a 1 MiB budget the three
    chains run in two slices."""
    T, N = 3, 20000
    hid, anc, th, _ = wc.chains(T, N, 3, 2, seed=3, limit=3)
    for lag, lineage in ((1, "genealogy"), (None, "reference")):
        want = check_batch(eng, hid, anc, th, lineage, lag, wc.QUANTILES[1:4], twice=True)
        monkeypatch.setenv("EPIPF_SMOOTH_SCRATCH_MB", "1")
        got = eng.walk_smooth_history(hid, anc, th, POP, lineage_id(lineage), wc.QUANTILES[1:4], lag=lag)
        monkeypatch.delenv("EPIPF_SMOOTH_SCRATCH_MB")
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                          b.view(np.uint64) if b.dtype == np.float64 else b)


def test_small_histories_on_global_rows(eng, monkeypatch):
    """EPIPF_SMOOTH_LDS=0 sends every size through the global-row instance: the same bits as the LDS one."""
    T, N = 7, 300
    hid, anc, th, _ = wc.chains(T, N, 3, 2, seed=8, limit=4)
    want = check_batch(eng, hid, anc, th, "genealogy", 3, wc.QUANTILES)
    monkeypatch.setenv("EPIPF_SMOOTH_LDS", "0")
    got = eng.walk_smooth_history(hid, anc, th, POP, lineage_id("genealogy"), wc.QUANTILES, lag=3)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      b.view(np.uint64) if b.dtype == np.float64 else b)


def test_the_resident_history(eng):
    """After a real walk_filter (N = 200, T = 12, 3 chains) walk_smooth on the resident history is walk_smooth_history
    on the copied one, and Engine.smooth is unchanged by the walk: the states of WalkResult."""
    from epipf.engine import Engine
    fx = if2_cases.load_fixture()
    N, T = 200, 12
    e = Engine("sir", 1, N, T, 3)
    e.set_observations(fx["sir"][:T])
    e.set_population(fx["npop"], fx["mu"])
    swarm0 = np.tile(np.array((0.8, 0.3)), (3, N, 1))
    hw = np.array([[0.1, 0.05], [0.05, 0.0], [0.0, 0.0]])
    lz, st = e.walk_filter(swarm0, hw, fx["probs"], np.array([4, 5, 6], dtype=np.uint64), 1)
    assert st.tolist() == [0, 0, 0]
    hid, anc = e.history(3)
    th = e.walk_history(3)
    for lineage in ("genealogy", "reference"):
        for L in (0, 1, 5, None):
            mean, quant, lin = e.walk_smooth(3, quantiles=(0.05, 0.5, 0.95), lineage=lineage, lag=L)
            hmean, hquant, hlin = eng.walk_smooth_history(hid, anc, th, fx["npop"], lineage_id(lineage),
                                                          np.array([0.05, 0.5, 0.95]), lag=L)
            np.testing.assert_array_equal(wr.bits(mean), wr.bits(hmean))
            np.testing.assert_array_equal(wr.bits(quant), wr.bits(hquant))
            np.testing.assert_array_equal(lin, hlin)
            states = e.smooth(3, quantiles=(0.05, 0.5, 0.95), lineage=lineage, lag=L)
            np.testing.assert_array_equal(states.lineages, lin)     # one genealogy, two reductions
    check_batch(eng, hid, anc, th, "genealogy", 5, (0.05, 0.5, 0.95))
    assert (wr.bits(quant[2, :, :, :2]) == wr.bits(np.array([0.8, 0.3]))).all()   # zero widths: theta never moved
    # the states are the smoother's own answer on the same run
    import epipf
    epipf.seed_stream(4, 1)
    res = epipf.walk_filter(fx["sir"][:T], "sir", (0.8, 0.3), hw[0], lag=5, n_particles=N, n_population=fx["npop"],
                            mu=fx["mu"], probs=fx["probs"], key=4)
    ce = epipf.get_engine("sir", 1, N, T, 1, 0)
    want = ce.smooth(1, lag=5)
    np.testing.assert_array_equal(res.states.sums, want.sums)
    np.testing.assert_array_equal(res.states.quantiles, want.quantiles)
    np.testing.assert_array_equal(res.states.lineages, res.lineages)
    m5, q5, _ = e.walk_smooth(1, lag=5)
    np.testing.assert_array_equal(wr.bits(res.theta_quantiles[0]), wr.bits(q5[0, :, :, :2]))
    np.testing.assert_array_equal(wr.bits(res.rt_mean[0]), wr.bits(m5[0, :, 2]))
    e.close()
    epipf.engine.release_engines()
