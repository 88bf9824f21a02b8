"""The smoother's definition on the host (epipf.smoothing, backend="numpy"; no device): against the brute force over the
N paths particle_path_sampler returns, against an independent walk of the true genealogy, and the premise the feature
rests on -- along ancestry[p + 1] every path is an epidemic, along the reference's ancestry[p] it is not."""
import numpy as np
import pytest

from smoothing_helpers import (QS, assert_smoothed_equal, cloud_statistics, genealogy_paths, golden_histories,
                               path_statistics, random_history, reference_paths)

from epipf import Smoothed, smooth_history  # noqa: E402  (conftest puts the package on the path)
from epipf.smoothing import multiplicities


@pytest.fixture(scope="module")
def histories(filter_golden):
    hs = golden_histories(filter_golden)
    assert len(hs) >= 5
    return hs


@pytest.fixture(scope="module")
def brute(histories):
    """Computed once: per case the path ensembles of both lineages."""
    return {name: (reference_paths(hid, anc), genealogy_paths(hid, anc)) for name, hid, anc in histories}


def test_reference_lineage_equals_the_sampled_path_ensemble(histories, brute):
    for name, hid, anc in histories:
        paths, visited = brute[name][0]
        sums, quant, lineages = path_statistics(paths, visited)
        got = smooth_history(hid, anc, quantiles=QS, lineage="reference", backend="numpy")
        assert isinstance(got, Smoothed) and got.zetas is None
        assert_smoothed_equal(got, sums, quant, lineages, hid.shape[1])
        assert got.lineages[-1] == hid.shape[1] and got.lineages[0] == 1, name


def test_genealogy_lineage_equals_the_per_path_walk(histories, brute):
    for name, hid, anc in histories:
        paths, visited = brute[name][1]
        sums, quant, lineages = path_statistics(paths, visited)
        got = smooth_history(hid, anc, quantiles=QS, backend="numpy")      # genealogy is the default
        assert_smoothed_equal(got, sums, quant, lineages, hid.shape[1])
        assert got.lineages[-1] == hid.shape[1], name
        assert np.all(np.diff(got.lineages) >= 0), name      # lineages only coalesce backwards in time


def _is_epidemic(paths, model):
    """S non-increasing and the last compartment non-decreasing along every path (per group for the subgroup models,
    whose compartments are [G][S, I, R])."""
    if model.startswith("sir_subgroups"):
        s, r = paths[:, :, 0::3], paths[:, :, 2::3]
    else:
        s, r = paths[:, :, :1], paths[:, :, -1:]
    return bool(np.all(np.diff(s, axis=1) <= 0) and np.all(np.diff(r, axis=1) >= 0))


def test_genealogy_paths_are_epidemics_and_reference_paths_are_not(filter_golden, histories, brute):
    checked = 0
    for name, hid, anc in histories:
        model = str(filter_golden[name]["model"]).lower()
        if model in ("sir", "seir"):
            assert _is_epidemic(brute[name][1][0], model), name
            checked += 1
    assert checked >= 3
    # the premise: the reference's own backtrace mixes lineages, so S rises or R falls along some path
    assert not _is_epidemic(brute["filter_sir_binom"][0][0], "sir")


def test_predictive_equals_column_statistics(histories):
    for name, hid, anc in histories:
        sums, quant, lineages = cloud_statistics(hid)
        for lineage in ("reference", "genealogy"):
            got = smooth_history(hid, anc, quantiles=QS, lineage=lineage, kind="predictive", backend="numpy")
            assert_smoothed_equal(got, sums, quant, lineages, hid.shape[1])


def test_multiplicities_sum_to_n_on_every_day(histories):
    for name, hid, anc in histories:
        a = np.rint(anc).astype(np.int64)
        for shift in (0, 1):
            m = multiplicities(a, shift)
            assert np.all(m.sum(1) == hid.shape[1]), name    # hence every histogram row sums to N
            assert np.all(m >= 0)


def test_batch_adds_a_chain_axis_and_keeps_chains_apart():
    rng = np.random.default_rng(5)
    hs = [random_history(rng, 6, 17, 3, ancestry=k) for k in ("random", "last", "permutation")]
    hid = np.stack([h for h, _ in hs])
    anc = np.stack([a for _, a in hs])
    got = smooth_history(hid, anc, quantiles=(0.25, 0.75), backend="numpy")
    assert got.mean.shape == (3, 6, 3) and got.quantiles.shape == (3, 2, 6, 3) and got.lineages.shape == (3, 6)
    for i in range(3):
        one = smooth_history(hid[i], anc[i], quantiles=(0.25, 0.75), backend="numpy")
        assert_smoothed_equal(one, got.sums[i], got.quantiles[i], got.lineages[i], 17)
    # every ancestor N - 1: one lineage before the last day, carrying all N
    np.testing.assert_array_equal(got.lineages[1], [1, 1, 1, 1, 1, 17])
    np.testing.assert_array_equal(got.sums[1][:-1], 17 * hid[1][:-1, 16].astype(np.int64))


def test_smallest_shapes():
    rng = np.random.default_rng(6)
    hid, anc = random_history(rng, 1, 9, 4)              # T == 1: day 0 with m = 1
    got = smooth_history(hid, anc, quantiles=QS, backend="numpy")
    sums, quant, lineages = cloud_statistics(hid.astype(np.float64))
    assert_smoothed_equal(got, sums, quant, lineages, 9)
    hid, anc = random_history(rng, 5, 1, 3)              # N == 1: the one particle is every quantile
    for lineage in ("reference", "genealogy"):
        got = smooth_history(hid, anc, quantiles=QS, lineage=lineage, backend="numpy")
        np.testing.assert_array_equal(got.sums, hid[:, 0])
        np.testing.assert_array_equal(got.quantiles, np.broadcast_to(hid[:, 0], (len(QS), 5, 3)))
        np.testing.assert_array_equal(got.lineages, np.ones(5))


def test_quantiles_none_and_values_beyond_bins():
    rng = np.random.default_rng(7)
    hid, anc = random_history(rng, 4, 12, 3, top=20)
    got = smooth_history(hid, anc, quantiles=None, backend="numpy")
    assert got.quantiles is None and got.sums.shape == (4, 3)
    hid[2, :, 1] = 30                                    # dropped with bins = 21: the counts never reach any rank
    got = smooth_history(hid, anc, quantiles=(0.5,), bins=21, kind="predictive", backend="numpy")
    assert got.quantiles[0, 2, 1] == 21
    hid[2, :, 1] = 20                                    # bins - 1 is the last value counted
    got = smooth_history(hid, anc, quantiles=(0.5,), bins=21, kind="predictive", backend="numpy")
    assert got.quantiles[0, 2, 1] == 20


def test_validation_errors():
    rng = np.random.default_rng(8)
    hid, anc = random_history(rng, 4, 12, 3)
    kw = dict(backend="numpy")
    for bad in (dict(lineage="true"), dict(kind="filtering"), dict(quantiles=(0.5, 1.5)), dict(quantiles=(-0.1,)),
                dict(quantiles=(float("nan"),)), dict(backend="torch"), dict(bins=0)):
        with pytest.raises(ValueError):
            smooth_history(hid, anc, **{**kw, **bad})
    neg = hid.copy()
    neg[1, 2, 0] = -1
    with pytest.raises(ValueError, match="non-negative"):
        smooth_history(neg, anc, **kw)
    for v in (-1, 12):
        out = anc.copy()
        out[2, 3] = v
        with pytest.raises(ValueError, match="ancestors"):
            smooth_history(hid, out, **kw)
    with pytest.raises(ValueError):
        smooth_history(hid, anc[:, :5], **kw)
    with pytest.raises(ValueError):
        smooth_history(hid[0], anc, **kw)
    # lineage, kind and quantiles are refused before any device call, whatever the backend
    with pytest.raises(ValueError):
        smooth_history(hid, anc, lineage="true", backend="gpu")
