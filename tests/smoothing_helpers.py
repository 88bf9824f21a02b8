"""Independent restatements for the smoother tests (tests/test_smoothing_host.py, tests/test_gpu_smoothing.py): the
brute force over sampled paths, and hand-made histories.  Nothing here calls epipf.smoothing."""
from unittest import mock

import numpy as np

QS = (0.0, 0.05, 0.5, 0.95, 1.0)


def golden_histories(filter_golden):
    """[(case, hidden [T, N, C] float64, ancestry [T, N] float64)] of the non-degenerate filter goldens."""
    out = []
    for name in sorted(filter_golden):
        rec = filter_golden[name]
        if "hidden" in rec and int(rec["status"]) == 0:
            out.append((name, rec["hidden"], rec["ancestry"]))
    return out


def reference_paths(hidden, ancestry):
    """(paths [N, T, C], visited [N, T]): epipf.particle_path_sampler run N times with np.random.randint patched to
    return 0..N-1, and the particle each of those paths visits per day (the sampler's own indexing, walked here)."""
    import epipf
    T, N, C = hidden.shape
    paths = np.empty((N, T, C))
    for k in range(N):
        with mock.patch("numpy.random.randint", return_value=k):
            paths[k] = epipf.particle_path_sampler(hidden, ancestry)
    visited = np.empty((N, T), dtype=np.int64)
    visited[:, T - 1] = np.arange(N)
    for p in range(T - 2, -1, -1):
        visited[:, p] = ancestry[p].astype(np.int64)[visited[:, p + 1]]
    return paths, visited


def genealogy_paths(hidden, ancestry):
    """(paths [N, T, C], visited [N, T]): one walk per final particle along ancestry[p + 1], the parent of a
    day-(p + 1) particle."""
    T, N, C = hidden.shape
    anc = ancestry.astype(np.int64)
    paths = np.empty((N, T, C))
    visited = np.empty((N, T), dtype=np.int64)
    for k in range(N):
        j = k
        for p in range(T - 1, -1, -1):
            visited[k, p] = j
            paths[k, p] = hidden[p, j]
            if p > 0:
                j = anc[p, j]
    return paths, visited


def path_statistics(paths, visited, qs=QS):
    """(sums [T, C] int64, quantiles [Q, T, C] int64, lineages [T]) over N paths."""
    sums = np.rint(paths.sum(0)).astype(np.int64)
    quant = np.rint(np.quantile(paths, qs, axis=0, method="inverted_cdf")).astype(np.int64)
    lineages = np.array([np.unique(visited[:, p]).size for p in range(visited.shape[1])])
    return sums, quant, lineages


def cloud_statistics(hidden, qs=QS):
    """Plain column statistics of the particle cloud: (sums, quantiles, lineages = N)."""
    T, N, C = hidden.shape
    sums = np.rint(hidden.sum(1)).astype(np.int64)
    quant = np.rint(np.quantile(hidden, qs, axis=1, method="inverted_cdf")).astype(np.int64)
    return sums, quant, np.full(T, N)


def random_history(rng, T, N, C, top=50, ancestry="random"):
    """A hand-made history: counts in [0, top], ancestors random / all N-1 / identity / one permutation per day."""
    hid = rng.integers(0, top + 1, size=(T, N, C)).astype(np.int32)
    if ancestry == "random":
        anc = rng.integers(0, N, size=(T, N))
    elif ancestry == "last":
        anc = np.full((T, N), N - 1)
    elif ancestry == "identity":
        anc = np.tile(np.arange(N), (T, 1))
    elif ancestry == "permutation":
        anc = np.stack([rng.permutation(N) for _ in range(T)])
    else:
        raise ValueError(ancestry)
    anc = anc.astype(np.int32)
    anc[0] = 0                                           # as the filter leaves row 0
    return hid, anc


def assert_smoothed_equal(got, want_sums, want_quant, want_lineages, N):
    np.testing.assert_array_equal(got.sums, want_sums)
    np.testing.assert_array_equal(got.lineages, want_lineages)
    if want_quant is None:
        assert got.quantiles is None
    else:
        np.testing.assert_array_equal(got.quantiles, want_quant)
    np.testing.assert_array_equal(got.mean, np.asarray(want_sums) / float(N))
