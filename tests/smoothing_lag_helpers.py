"""The fixed-lag smoother's brute force (tests/test_smoothing_lag_host.py, tests/test_gpu_smoothing_lag.py): every
particle of the window's end day walked back to day p, with no multiplicity recursion.  Nothing here calls
epipf.smoothing."""
import numpy as np

from smoothing_helpers import QS

SHIFT = {"reference": 0, "genealogy": 1}


def lags_for(T, fixed=(0, 1, 2, 5)):
    """The lags a history of T days is checked at: the fixed ones, T - 2 (the longest window the kernel walks), T - 1
    (the smoother) and T + 3 (clipped everywhere); L >= 0, no repeats."""
    return sorted({L for L in (*fixed, T - 2, T - 1, T + 3) if L >= 0})


def lag_brute_force(hidden, ancestry, lineage, lag, qs=QS):
    """(sums [T, C] int64, quantiles [Q, T, C] int64, lineages [T]) of one history under a fixed lag: for each day p the
    N particles of day e(p) = min(p + lag, T-1) are walked back to day p along ancestry[q + shift], and the statistics
    are taken over the N particles they visit there."""
    hid = np.rint(np.asarray(hidden)).astype(np.int64)
    anc = np.rint(np.asarray(ancestry)).astype(np.int64)
    T, N, C = hid.shape
    shift = SHIFT[lineage]
    sums = np.empty((T, C), dtype=np.int64)
    quant = np.empty((len(qs), T, C), dtype=np.int64)
    lineages = np.empty(T, dtype=np.int64)
    for p in range(T):
        e = min(p + lag, T - 1)
        at = np.arange(N)                                # the particle each walk stands on, from day e
        for q in range(e - 1, p - 1, -1):
            at = anc[q + shift][at]
        visited = hid[p][at]                             # [N, C]
        sums[p] = visited.sum(0)
        quant[:, p] = np.quantile(visited, qs, axis=0, method="inverted_cdf")
        lineages[p] = np.unique(at).size
    return sums, quant, lineages
