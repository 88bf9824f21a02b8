"""The fixed-lag smoother's definition on the host (epipf.smoothing, backend="numpy", lag=L; no device): against a brute
force that walks every particle of the window's end day back (tests/smoothing_lag_helpers.py), its two limits against
the existing backend, and the lineage counts the feature was proposed on.  Integers: every comparison is
assert_array_equal."""
import numpy as np
import pytest

from smoothing_helpers import QS, assert_smoothed_equal, golden_histories, random_history
from smoothing_lag_helpers import lag_brute_force, lags_for

from epipf import smooth_history  # noqa: E402  (conftest puts the package on the path)
from epipf.smoothing import lag_multiplicities

LINEAGES = ("reference", "genealogy")


@pytest.fixture(scope="module")
def histories(filter_golden):
    hs = golden_histories(filter_golden)
    assert len(hs) >= 5
    return hs


def _same(got, want):
    np.testing.assert_array_equal(got.sums, want.sums)
    np.testing.assert_array_equal(got.lineages, want.lineages)
    np.testing.assert_array_equal(got.quantiles, want.quantiles)
    np.testing.assert_array_equal(got.mean, want.mean)


def test_numpy_backend_equals_the_brute_force(histories):
    for name, hid, anc in histories:
        T, N = hid.shape[:2]
        for lineage in LINEAGES:
            for L in lags_for(T):
                got = smooth_history(hid, anc, quantiles=QS, lineage=lineage, lag=L, backend="numpy")
                assert got.zetas is None
                assert_smoothed_equal(got, *lag_brute_force(hid, anc, lineage, L), N)


def test_the_two_limits_are_the_existing_backend(histories):
    for name, hid, anc in histories:
        T = hid.shape[0]
        for lineage in LINEAGES:
            kw = dict(quantiles=QS, lineage=lineage, backend="numpy")
            _same(smooth_history(hid, anc, lag=0, **kw), smooth_history(hid, anc, kind="predictive", **kw))
            smoothing = smooth_history(hid, anc, kind="smoothing", **kw)
            for L in (T - 1, T, T + 3, 10**12):
                _same(smooth_history(hid, anc, lag=L, **kw), smoothing)
            # lag=None is that path itself
            _same(smooth_history(hid, anc, lag=None, **kw), smoothing)


def test_multiplicities_sum_to_n_and_lineages_fall_with_the_lag(histories):
    for name, hid, anc in histories:
        a = np.rint(anc).astype(np.int64)
        T, N = a.shape
        for shift in (0, 1):
            before = np.full(T, N)
            for L in range(0, T + 1):
                m = lag_multiplicities(a, shift, L)
                assert np.all(m >= 0) and np.all(m.sum(1) == N), (name, L)   # hence every histogram row sums to N
                lineages = np.count_nonzero(m, axis=1)
                assert np.all(lineages <= before), (name, L)                 # monotone in L, day by day
                before = lineages
                if L == 0:
                    assert np.all(lineages == N)


def test_lineage_counts_of_cfg1(filter_golden):
    """The counts the fixed-lag smoother was proposed on: filter_cfg1_sir (N = 100, T = 50), genealogy rule."""
    rec = filter_golden["filter_cfg1_sir"]
    hid, anc = rec["hidden"], rec["ancestry"]
    assert hid.shape[:2] == (50, 100)
    day0_day25 = {0: (100, 100), 1: (61, 60), 5: (26, 23), 10: (17, 16), 49: (4, 9)}
    least = {0: 100, 1: 55, 2: 41, 5: 20, 10: 10, 49: 4}
    for L in sorted(least):
        lin = smooth_history(hid, anc, quantiles=None, lag=L, backend="numpy").lineages
        if L in day0_day25:
            assert (lin[0], lin[25]) == day0_day25[L], L
        assert lin.min() == least[L], L


def test_batch_and_smallest_shapes():
    rng = np.random.default_rng(15)
    hs = [random_history(rng, 6, 17, 3, ancestry=k) for k in ("random", "last", "permutation")]
    hid, anc = np.stack([h for h, _ in hs]), np.stack([a for _, a in hs])
    got = smooth_history(hid, anc, quantiles=QS, lag=2, backend="numpy")
    assert got.mean.shape == (3, 6, 3) and got.quantiles.shape == (3, len(QS), 6, 3) and got.lineages.shape == (3, 6)
    for i in range(3):
        assert_smoothed_equal(smooth_history(hid[i], anc[i], quantiles=QS, lag=2, backend="numpy"),
                              got.sums[i], got.quantiles[i], got.lineages[i], 17)
        np.testing.assert_array_equal(got.sums[i], lag_brute_force(hid[i], anc[i], "genealogy", 2)[0])
    # every ancestor N - 1: one lineage wherever the window has a step, all N where it has none
    np.testing.assert_array_equal(got.lineages[1], [1, 1, 1, 1, 1, 17])
    np.testing.assert_array_equal(got.lineages[2], [17] * 6)             # permutations never coalesce
    hid, anc = random_history(rng, 1, 9, 4)              # T == 1 is valid: no window has a step
    for L in (0, 1, 4):
        got = smooth_history(hid, anc, quantiles=QS, lag=L, backend="numpy")
        assert_smoothed_equal(got, *lag_brute_force(hid, anc, "genealogy", L), 9)
        np.testing.assert_array_equal(got.lineages, [9])
    hid, anc = random_history(rng, 5, 1, 3)              # N == 1
    got = smooth_history(hid, anc, quantiles=None, lag=1, backend="numpy")
    assert got.quantiles is None
    np.testing.assert_array_equal(got.sums, hid[:, 0])


def test_a_value_beyond_bins_is_dropped():
    rng = np.random.default_rng(16)
    hid, anc = random_history(rng, 4, 12, 3, top=20)
    hid[1, :, 1] = 30
    got = smooth_history(hid, anc, quantiles=(0.5,), bins=21, lag=1, backend="numpy")
    assert got.quantiles[0, 1, 1] == 21
    hid[1, :, 1] = 20
    got = smooth_history(hid, anc, quantiles=(0.5,), bins=21, lag=1, backend="numpy")
    assert got.quantiles[0, 1, 1] == 20


@pytest.mark.parametrize("backend", ["numpy", "gpu"])
def test_lag_errors_are_raised_before_any_device_call(backend):
    """A bool, a non-integer, a negative value, and a lag with kind="predictive": ValueError whatever the backend (this
    runs without a device, so the gpu backend never got as far as one)."""
    from epipf import particle_smoother
    rng = np.random.default_rng(17)
    hid, anc = random_history(rng, 4, 12, 3)
    for bad in (True, False, np.True_, 1.0, 2.5, "3", (1,), -1, np.int64(-2)):
        with pytest.raises(ValueError, match="lag"):
            smooth_history(hid, anc, lag=bad, backend=backend)
        with pytest.raises(ValueError, match="lag"):
            particle_smoother(np.zeros((4, 1)), "sir", (2.0, 1.0), lag=bad)
    with pytest.raises(ValueError, match="lag"):
        smooth_history(hid, anc, lag=2, kind="predictive", backend=backend)
    with pytest.raises(ValueError, match="lag"):
        particle_smoother(np.zeros((4, 1)), "sir", (2.0, 1.0), lag=0, kind="predictive")
    with pytest.raises(ValueError):                      # kind keeps its two values
        smooth_history(hid, anc, lag=1, kind="filtering", backend=backend)
    for ok in (0, 3, np.int32(2), 10**12):
        smooth_history(hid, anc, lag=ok, backend="numpy")


def test_engine_methods_refuse_a_bad_lag_without_a_library_call():
    """Engine.smooth and Engine.smooth_history check the lag before they touch the library: on an object that has no
    library handle at all the ValueError still comes first."""
    from epipf.engine import Engine
    eng = Engine.__new__(Engine)                         # no __init__: no context, no library
    for bad in (True, 1.5, -1):
        with pytest.raises(ValueError, match="lag"):
            eng.smooth(1, lag=bad)
        with pytest.raises(ValueError, match="lag"):
            eng.smooth_history(np.zeros((1, 2, 3, 1), np.int32), np.zeros((1, 2, 3), np.int32), 1, 0, None, 0, lag=bad)
    with pytest.raises(ValueError, match="lag"):
        eng.smooth(1, lag=1, kind="predictive")
    with pytest.raises(ValueError, match="lag"):
        eng.smooth_history(np.zeros((1, 2, 3, 1), np.int32), np.zeros((1, 2, 3), np.int32), 1, 1, None, 0, lag=1)
