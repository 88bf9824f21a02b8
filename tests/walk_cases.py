"""Inputs shared by the time-varying-rates tests (a helper, no test itself): the "does it work" configuration on the
step fixture (tests/golden/walk_sir_step.npz) with its recorded numbers, and the hand-made histories that probe the
reduction (values chosen to break a radix select or a sort, ancestries chosen to break the backward walk)."""
import functools
import os

import numpy as np

import walk_restatement as wr
from conftest import GOLDEN

# ---------------------------------------------------------------------------------------------- does it work
START, RW, N_WORK, LAG_WORK, F_WORK = (0.3, 0.2), (0.1, 0.0), 200, 5, 0
KEYS = (1, 2, 3, 4)
EARLY, LATE = slice(2, 12), slice(17, 30)               # the plateaus: beta = 0.6 on days 1..11, 0.05 from day 12
# Measured on the CPU restatement at N = 200, lag 5: the smoothed median of beta averaged over the early
# and the late plateau, and log_zeta[T-1] with rw = (0.1, 0) against rw = (0, 0) from the same start.
#   key   early    late     gap      loglik walk   loglik fixed   gain
#   1     0.5902   0.1895   0.4007   -127.09       -267.24        140.15
#   2     0.5128   0.0926   0.4202   -126.67       -220.37         93.70
#   3     0.5252   0.1259   0.3992   -129.05       -197.58         68.53
#   4     0.5412   0.1188   0.4224   -133.26       -216.43         83.17
# The tests assert half the smallest value over the four keys (the margin of §17's fixture test).
GAP_BOUND, GAIN_BOUND = 0.3992 / 2, 68.53 / 2


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "walk_sir_step.npz"))
    return dict(Y=z["Y"], npop=float(z["population"]), mu=float(z["mu"]), probs=float(z["probs"]))


@functools.lru_cache(maxsize=None)
def restated(key, walking):
    """The restatement's pass on the fixture under `key`, with the walk's half-widths or none (shared, never modified)."""
    fx = load_fixture()
    hw = RW if walking else (0.0, 0.0)
    return wr.one_pass(fx["Y"], "sir", np.tile(START, (N_WORK, 1)), hw, False, fx["probs"], fx["npop"], fx["mu"], key,
                       F_WORK)


def plateau_gap(beta_median):
    """Early minus late plateau average of a smoothed median of beta [T]."""
    return float(beta_median[EARLY].mean() - beta_median[LATE].mean())


# ---------------------------------------------------------------------------------------------- hand-made histories
VALUES = ("equal", "two", "decreasing", "magnitudes", "gamma_zero", "ulp")
ANCESTRIES = ("zero", "identity", "permutation", "one_lineage", "random")
MAGNITUDES = (5e-324, 1e-310, 2.2250738585072014e-308, 1e-200, 1e-5, 1.0, 1e100, 1e300, 0.0, -0.0)
QUANTILES = np.array([0.0, 1e-12, 0.5, 1.0 - 1e-12, 1.0])


def make_theta(kind, T, N, d):
    i = np.arange(N, dtype=np.float64)
    th = np.empty((T, N, d))
    th[...] = np.array([0.7, 0.45, 0.3][:d - 1] + [0.25])
    for p in range(T):
        if kind == "two":                                # two distinct values, most particles on one
            th[p, :, 0] = np.where((np.arange(N) + p) % 7 == 0, 2.0, 0.25)
        elif kind == "decreasing":
            th[p, :, 0] = 1.0 + (N - i) * 0.01 + p
            th[p, :, d - 1] = 3.0 + (N - i) * 0.5
        elif kind == "magnitudes":                       # subnormal to 1e300 in one day, +0.0 and -0.0 together
            th[p, :, 0] = np.array(MAGNITUDES)[(np.arange(N) + p) % len(MAGNITUDES)]
        elif kind == "gamma_zero":                       # R = +inf on a third of the particles on even days, on two
            gz = (np.arange(N) % 3 == 0) if p % 2 == 0 else (np.arange(N) % 3 != 0)   # thirds (the median) on odd ones
            th[p, gz, d - 1] = 0.0
            th[p, :, 0] = 0.5 + 0.001 * ((np.arange(N) * 7 + p) % 11)
        elif kind == "ulp":                              # values that differ in the lowest mantissa bit only
            th[p, :, 0] = 1.0 + ((np.arange(N) * 3 + p) % 5) * 2.0 ** -52
            th[p, :, d - 1] = 0.25 * (1.0 + ((np.arange(N) + p) % 3) * 2.0 ** -52)
    return th


def make_hidden(T, N, C, seed):
    rng = np.random.default_rng(seed)
    hid = rng.integers(0, 300, size=(T, N, C)).astype(np.int32)
    hid[:, ::5, 0] = 0                                   # S = 0: R = 0 unless gamma = 0
    return hid


def make_ancestry(kind, T, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((T, N), dtype=np.int32)
    if kind == "identity":
        return np.tile(np.arange(N, dtype=np.int32), (T, 1))
    if kind == "permutation":
        return np.array([rng.permutation(N) for _ in range(T)], dtype=np.int32)
    anc = rng.integers(0, N, size=(T, N)).astype(np.int32)
    if kind == "one_lineage":                            # every particle of the middle day has one parent
        anc[T // 2] = (3 * T) % N
    return anc


def history(values, ancestry, T, N, C, d, seed):
    """(hidden [T, N, C], ancestry [T, N], theta [T, N, d]) of one hand-made chain."""
    return make_hidden(T, N, C, seed), make_ancestry(ancestry, T, N, seed + 1), make_theta(values, T, N, d)


def chains(T, N, C, d, seed=0, limit=None):
    """A batch of hand-made chains: every kind of values with two kinds of ancestry, rotating so that every pair of kinds
    appears in some shape; (hidden [n, T, N, C], ancestry [n, T, N], theta [n, T, N, d], names)."""
    picks = []
    for vi, v in enumerate(VALUES):
        for step in (0, 2):
            picks.append((v, ANCESTRIES[(vi + step + seed) % len(ANCESTRIES)]))
    picks = picks[:limit]
    parts = [history(v, a, T, N, C, d, 100 * seed + 7 * k) for k, (v, a) in enumerate(picks)]
    return (np.stack([h for h, _, _ in parts]), np.stack([a for _, a, _ in parts]), np.stack([t for _, _, t in parts]),
            picks)


def lags(T):
    """0, 1, T-2, T-1, 10^6 and full (None), without repeats or negatives."""
    out = []
    for L in (0, 1, T - 2, T - 1, 10 ** 6, None):
        if (L is None or L >= 0) and L not in out:
            out.append(L)
    return out
