"""Restatement of the negative-binomial factor as DESIGN.md §21 defines it, composed with the incidence filter's numpy
restatement (a helper for the tests, no test itself).

The factor is restated operation for operation in Python floats: c(y, kappa) from mpmath at 60 digits rounded once, the
logarithms from oracle.log_batch (glibc's), math.exp.  Without mpmath c comes from the library's
epipf_negbin_coefficients (HAVE_MPMATH tells the tests, which then skip the coefficient comparison).  The pass is
tests/incidence_restatement.py's one_pass with its `weights` replaced for the duration of the call: that file is not
edited and its rows, flows, accumulator, resampling and SSA are what the pass uses."""
import contextlib
import ctypes
import math

import numpy as np

import incidence_restatement as ir
import oracle

try:
    import mpmath
    HAVE_MPMATH = True
except ImportError:                                      # pragma: no cover
    mpmath = None
    HAVE_MPMATH = False

_C = {}


def library_coefficients(y, kappa):
    """epipf_negbin_coefficients (host only, no GPU); raises EpipfError on its refusals."""
    from epipf import _lib
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    out = np.zeros(y.shape[0])
    _lib.check(_lib.load().epipf_negbin_coefficients(_lib.ptr(y), y.shape[0], ctypes.c_double(float(kappa)), _lib.ptr(out)),
               "epipf_negbin_coefficients")
    return out


def coefficient(y, kappa):
    """c(y, kappa) = lgamma(y + kappa) - lgamma(kappa) - lgamma(y + 1), the real value rounded once to double."""
    y, kappa = float(y), float(kappa)
    if y == 0.0:
        return 0.0
    k = (y, kappa)
    if k not in _C:
        if HAVE_MPMATH:
            with mpmath.workprec(200):                   # 60 digits
                yy, kk = mpmath.mpf(y), mpmath.mpf(kappa)
                _C[k] = float(mpmath.loggamma(yy + kk) - mpmath.loggamma(kk) - mpmath.loggamma(yy + 1))
        else:
            _C[k] = float(library_coefficients([y], kappa)[0])
    return _C[k]


def _log(x):
    return float(oracle.log_batch(np.array([x], dtype=np.float64))[0])


def factor(y, n, rho, kappa):
    """One column's factor for scalars, in §21's order of operations."""
    y, n, rho, kappa = float(y), float(n), float(rho), float(kappa)
    m = rho * n
    if not (m > 0.0):
        return 1.0 if y == 0.0 else 0.0
    t = kappa + m
    c, logk, lt = coefficient(y, kappa), math.log(kappa), _log(t)
    L = (c + kappa * (logk - lt)) + y * (_log(m) - lt)
    return math.exp(L)


def factors(y, n, rho, kappa):
    """factor over an array n of accumulated flows, the logs batched (same values as factor)."""
    n = np.asarray(n, dtype=np.float64)
    y, rho, kappa = float(y), float(rho), float(kappa)
    m = rho * n
    out = np.where(y == 0.0, 1.0, 0.0) * np.ones(n.shape)
    pos = m > 0.0
    if pos.any():
        mp = m[pos]
        t = kappa + mp
        lt, lm = oracle.log_batch(t), oracle.log_batch(mp)
        c, logk = coefficient(y, kappa), math.log(kappa)
        L = (c + kappa * (logk - lt)) + y * (lm - lt)
        out[pos] = [math.exp(v) for v in L]
    return out


def weights(yrow, acc, rho, kappa):
    """The product over the reported columns, in column order from 1.0."""
    w = np.ones(acc.shape[0])
    for k in range(acc.shape[1]):
        if not np.isnan(yrow[k]):
            w = w * factors(yrow[k], acc[:, k], rho, kappa)
    return w


@contextlib.contextmanager
def negbin_weights(kappa):
    """incidence_restatement.weights replaced by the negative-binomial product at dispersion kappa (probs: the mean
    ratio), restored afterwards."""
    saved = ir.weights
    ir.weights = lambda yrow, acc, observations, probs: weights(yrow, acc, probs, kappa)
    try:
        yield
    finally:
        ir.weights = saved


def one_pass(counts, model, theta, probs, kappa, N, npop, mu, key, f, cumulate=False):
    """incidence_restatement.one_pass under negative-binomial reports; the same dict."""
    with negbin_weights(kappa):
        return ir.one_pass(counts, model, theta, False, probs, N, npop, mu, key, f, cumulate=cumulate)


loglik = ir.loglik
