"""numpy restatement of ABC-SMC as DESIGN.md §15 defines it (a helper for the tests, no test itself).

Everything new is restated here in numpy: the domain-6 proposal draws (oracle/philox.py), the ancestor rule, the
perturbation, the prior-box test, the accept loop over one global trial counter, the weights and the schedule.  Each
simulated trial is the CPU oracle's: oracle.abc_trials with the degenerate prior {"beta": [b, b], "gamma": [g, g]}
returns theta = (b, g) exactly (lo + 0*U == lo) and runs trial t's initial counts and SSA from the counters every ABC
trial uses."""
import numpy as np

import oracle
import philox

DOMAIN_ABC_SMC = 6


def proposal_uniforms(key, f, t):
    """(u_sel, u_beta, u_gamma) of trials t (array): blocks (0, t, 6<<24, f) and (1, t, 6<<24, f)."""
    k = philox.split_key(key)
    t = np.asarray(t, dtype=np.uint64)
    r0 = philox.philox4x32_10(0, t, DOMAIN_ABC_SMC << 24, f, k)
    r1 = philox.philox4x32_10(1, t, DOMAIN_ABC_SMC << 24, f, k)
    return philox.u01(r0[0], r0[1]), philox.u01(r1[0], r1[1]), philox.u01(r1[2], r1[3])


def cdf_of(w):
    cdf = np.cumsum(np.asarray(w, dtype=np.float64))
    cdf /= cdf[-1]
    return cdf


def half_width(theta, kernel_scale=1.0):
    theta = np.asarray(theta, dtype=np.float64)
    return np.array([kernel_scale * 0.5 * (theta[:, c].max() - theta[:, c].min()) for c in range(2)])


def ancestors(cdf, u_sel):
    return np.minimum(np.searchsorted(cdf, u_sel, side="right"), len(cdf) - 1)


def propose(prev_theta, cdf, hw, priors, key, f, t):
    """Ancestors, proposals [len(t), 2] and the in-box mask of trials t."""
    us, ub, ug = proposal_uniforms(key, f, t)
    j = ancestors(cdf, us)
    prev_theta = np.asarray(prev_theta, dtype=np.float64)
    th = np.empty((len(j), 2))
    th[:, 0] = prev_theta[j, 0] + hw[0] * (2.0 * ub - 1.0)
    th[:, 1] = prev_theta[j, 1] + hw[1] * (2.0 * ug - 1.0)
    (bl, bh), (gl, gh) = priors["beta"], priors["gamma"]
    inside = (th[:, 0] >= bl) & (th[:, 0] <= bh) & (th[:, 1] >= gl) & (th[:, 1] <= gh)
    return j, th, inside


def denominators(theta, prev_theta, prev_w, hw):
    theta = np.asarray(theta, dtype=np.float64)
    prev_theta = np.asarray(prev_theta, dtype=np.float64)
    prev_w = np.asarray(prev_w, dtype=np.float64)
    den = np.empty(len(theta))
    for i in range(len(theta)):
        mask = (np.abs(theta[i, 0] - prev_theta[:, 0]) <= hw[0]) & (np.abs(theta[i, 1] - prev_theta[:, 1]) <= hw[1])
        den[i] = np.cumsum(np.where(mask, prev_w, 0.0))[-1]
    return den


def weights_of(den):
    w = 1.0 / den
    w /= np.cumsum(w)[-1]
    return w


def next_threshold(dist, quantile):
    return float(np.sort(dist)[int(np.ceil(quantile * len(dist))) - 1])


def _rows_to_traj(rows):
    T = rows.shape[0]
    return np.concatenate([np.arange(T, dtype=np.float64)[:, None], rows.astype(np.float64)], 1)


def generation(Y, n, eps, priors, prev, key, f, t0, max_trials=10**7, chunk=256):
    """One generation from global trial t0.  prev = None (the prior stage) or (theta_prev, w_prev, hw).
    Returns dict(theta, traj, distances, ancestors, trials, accepted, outside, proposed)."""
    Y = np.asarray(Y, dtype=np.float64)
    th_acc, tr_acc, d_acc, a_acc = [], [], [], []
    last = -1
    outside = proposed = 0
    t = 0
    cdf = None if prev is None else cdf_of(prev[1])
    while len(th_acc) < n and t < max_trials:
        m = min(chunk, max_trials - t)
        ts = t0 + t + np.arange(m)
        if prev is None:
            theta, rows, dist, _ = oracle.abc_trials(Y, priors, key, f, t0 + t, m)
            anc = np.full(m, -1)
        else:
            anc, theta, inside = propose(prev[0], cdf, prev[2], priors, key, f, ts)
            dist = np.full(m, np.inf)
            rows = [None] * m
        for i in range(m):
            if len(th_acc) == n:
                break
            if prev is not None:
                proposed += 1
                if not inside[i]:
                    outside += 1
                    continue
                pr = {"beta": [theta[i, 0], theta[i, 0]], "gamma": [theta[i, 1], theta[i, 1]]}
                th1, rw1, d1, _ = oracle.abc_trials(Y, pr, key, f, int(ts[i]), 1)
                assert th1[0, 0] == theta[i, 0] and th1[0, 1] == theta[i, 1]
                dist[i], rows[i] = d1[0], rw1[0]
            if not (dist[i] > eps):
                th_acc.append(theta[i].copy())
                tr_acc.append(_rows_to_traj(rows[i]))
                d_acc.append(dist[i])
                a_acc.append(anc[i])
                last = t + i
        t += m
    full = len(th_acc) == n
    T = Y.shape[0]
    return dict(theta=np.array(th_acc).reshape(-1, 2), traj=np.array(tr_acc).reshape(-1, T, 4),
                distances=np.array(d_acc), ancestors=np.array(a_acc, dtype=np.int32),
                trials=last + 1 if full else min(t, max_trials), accepted=len(th_acc), outside=outside,
                proposed=proposed)


def run(Y, n, thresholds, priors, key, f, kernel_scale=1.0, quantile=None, generations=None):
    """The whole run: a list of generations, each generation()'s dict plus threshold, half_width, denominators,
    weights."""
    n_gen = len(thresholds) if generations is None else generations
    gens = []
    t0 = 0
    prev = None
    for g in range(n_gen):
        eps = float(thresholds[g]) if g < len(thresholds) else next_threshold(gens[-1]["distances"], quantile)
        if g > 0:
            hw = half_width(gens[-1]["theta"], kernel_scale)
            prev = (gens[-1]["theta"], gens[-1]["weights"], hw)
        r = generation(Y, n, eps, priors, prev, key, f, t0)
        assert r["accepted"] == n, (g, eps, r["accepted"])
        if g == 0:
            r.update(half_width=np.zeros(2), denominators=np.full(n, 1.0), weights=np.full(n, 1.0 / n))
        else:
            den = denominators(r["theta"], prev[0], prev[1], hw)
            r.update(half_width=hw, denominators=den, weights=weights_of(den))
        r["threshold"] = eps
        gens.append(r)
        t0 += r["trials"]
    return gens
