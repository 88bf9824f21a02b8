"""numpy restatement of iterated filtering (IF2) as DESIGN.md §17 defines it (a helper for the tests, no test itself).

What is new is restated here in numpy: the domain-7 perturbation draws (oracle/philox.py), the reflection at 0, the
per-particle parameters following their ancestors, the swarm mean and the iteration loop.  Everything else is the CPU
oracle's: the initial states are oracle.particle_filter's on one observation row, a weight is the minimum over the
columns of oracle.binom_pmf / norm_pdf, the ancestors are oracle.resample on the filter's resampling uniforms, the
logarithm is oracle.log_batch, and particle j's day is oracle.simulate on row j (the counter's particle word is the row
index) with that particle's own rates."""
import numpy as np

import oracle
import philox

DOMAIN_IF2 = 7
DIMS = {"sir": 2, "seir": 3}
DEGENERATE = 1


def perturb_uniforms(key, f, p, n, d):
    """u[j, c] of step p: block (c // 2, j, (p & 0xFFFFFF) | 7 << 24, f), words (0, 1) for even c and (2, 3) for odd."""
    k = philox.split_key(key)
    j = np.arange(n)
    u = np.empty((n, d))
    for b in range((d + 1) // 2):
        r = philox.philox4x32_10(b, j, (p & 0xFFFFFF) | (DOMAIN_IF2 << 24), f, k)
        u[:, 2 * b] = philox.u01(r[0], r[1])
        if 2 * b + 1 < d:
            u[:, 2 * b + 1] = philox.u01(r[2], r[3])
    return u


def perturb(theta, hw, key, f, p):
    """theta [n, d] jittered by the half-widths hw [d] at step p, reflected at 0."""
    theta = np.asarray(theta, dtype=np.float64)
    u = perturb_uniforms(key, f, p, theta.shape[0], theta.shape[1])
    t = theta + np.asarray(hw, dtype=np.float64) * (2.0 * u - 1.0)
    return np.where(t < 0.0, -t, t)


def weights(model, x, yrow, observations, probs):
    """min over the observed columns (np.min propagates NaN), pmcmc.py:178-181."""
    n, K = x.shape[0], len(yrow)
    cols = []
    for i in range(K):
        if observations:
            cols.append(oracle.norm_pdf(np.full(n, yrow[i]), x[:, i].astype(float), np.full(n, probs)))
        else:
            cols.append(oracle.binom_pmf(np.full(n, yrow[i]), x[:, i].astype(float), np.full(n, probs)))
    return np.min(np.array(cols), axis=0)


def one_pass(Y, model, theta, hw, observations, probs, npop, mu, key, f):
    """One iteration at filter index f from the swarm theta [N, d].  Returns dict(status, theta [N, d] (the swarm
    after the last step), hidden [T, N, C], ancestry [T, N], log_zetas [T], reflections, events (accepted SSA events of
    the steps that ran))."""
    Y = np.asarray(Y, dtype=np.float64)
    T = Y.shape[0]
    theta = np.asarray(theta, dtype=np.float64)
    N, d = theta.shape
    first = oracle.particle_filter(Y[:1], model, tuple(theta[0]), observations, probs, N, npop, mu, key=key,
                                   filter_index=f)
    C = first["hidden"].shape[2]
    hidden = np.zeros((T, N, C), dtype=np.int32)
    anc = np.zeros((T, N), dtype=np.int32)
    lz = np.zeros(T)
    hidden[0] = first["hidden"][0]
    reflections, events = 0, 0

    def jitter(th, p):
        nonlocal reflections
        u = perturb_uniforms(key, f, p, N, d)
        t = th + np.asarray(hw, dtype=np.float64) * (2.0 * u - 1.0)
        reflections += int(np.count_nonzero(t < 0.0))
        return np.where(t < 0.0, -t, t)

    th = jitter(theta, 0)
    status = 0
    for p in range(1, T):
        w = weights(model, hidden[p - 1], Y[p - 1], observations, probs)
        sw = 0.0
        for v in w:                                      # the sequential sum, pmcmc.py:183
            sw = sw + v
        with np.errstate(divide="ignore", invalid="ignore"):
            lz[p] = lz[p - 1] + oracle.log_batch(np.array([sw / float(N)]))[0]
        a = oracle.resample(w, philox.resample_uniforms(key, f, p, N))
        if a is None:
            status = DEGENERATE
            lz[p] = -np.inf
            lz[p + 1:] = -np.inf
            break
        anc[p] = a
        th = jitter(th[a], p)
        for j in range(N):
            rows = np.zeros((j + 1, C), dtype=np.int32)  # rows before j hold no infection: they draw nothing
            rows[j] = hidden[p - 1, a[j]]
            out, nev = oracle.simulate(model, rows, tuple(th[j]), 1.0, key, f, p)
            hidden[p, j] = out[j]
            events += nev
    return dict(status=status, theta=th, hidden=hidden, ancestry=anc, log_zetas=lz, reflections=reflections,
                events=events)


def device_mean(swarm):
    """Component means of swarm [N, d] in if2_finish_kernel's order: partial[t] is the left-to-right sum of
    swarm[t::256, c] (0.0 for an empty stride), the total the left-to-right sum of the 256 partials, over float(N)."""
    swarm = np.asarray(swarm, dtype=np.float64)
    N, d = swarm.shape
    mean = np.empty(d)
    for c in range(d):
        tot = 0.0
        for t in range(256):
            acc = 0.0
            for v in swarm[t::256, c]:
                acc = acc + float(v)
            tot = tot + acc
        mean[c] = tot / float(N)
    return mean


def run(Y, model, swarm, hw, observations, probs, npop, mu, key, f0):
    """M = len(hw) iterations from the swarm [N, d] at filter indices f0, f0 + 1, ...  Returns dict(swarm, mean [M, d],
    loglik [M], log_zetas [M, T], status, iterations_done, hidden, ancestry, last_log_zetas (of the last executed
    iteration), reflections, events [M] (accepted SSA events over particles and steps of each executed iteration, a
    failed one's steps before the dying one included), swarms [iterations_done, N, d] (each completed iteration's))."""
    swarm = np.array(swarm, dtype=np.float64)
    hw = np.asarray(hw, dtype=np.float64)
    M, T = hw.shape[0], np.asarray(Y).shape[0]
    mean = np.full((M, swarm.shape[1]), np.nan)
    loglik = np.full(M, np.nan)
    lzs = np.full((M, T), np.nan)
    events = np.zeros(M, dtype=np.int64)
    swarms = []
    status, done, reflections = 0, 0, 0
    last = None
    for m in range(M):
        last = one_pass(Y, model, swarm, hw[m], observations, probs, npop, mu, key, (f0 + m) & 0xFFFFFFFF)
        reflections += last["reflections"]
        events[m] = last["events"]
        if last["status"]:
            status = last["status"]
            break
        swarm = last["theta"]
        swarms.append(swarm)
        mean[m] = swarm.mean(axis=0)
        loglik[m] = last["log_zetas"][-1]
        lzs[m] = last["log_zetas"]
        done = m + 1
    return dict(swarm=swarm, mean=mean, loglik=loglik, log_zetas=lzs, status=status, iterations_done=done,
                hidden=last["hidden"], ancestry=last["ancestry"], last_log_zetas=last["log_zetas"],
                reflections=reflections, events=events,
                swarms=np.array(swarms).reshape(done, swarm.shape[0], swarm.shape[1]))


def cooling_table(rw, cooling, iterations, first=0):
    """hw[m] = rw * cooling ** (m / 50.0) for m = first .. first + iterations - 1 (pomp's cooling.fraction.50)."""
    rw = np.asarray(rw, dtype=np.float64)
    return np.array([rw * float(cooling) ** (m / 50.0) for m in range(first, first + iterations)])


def score(Y, model, theta, observations, probs, npop, mu, n_particles=400, key=77, indices=range(8)):
    """log-mean-exp of the oracle filter's log-likelihood at theta over the filter indices (-inf where degenerate)."""
    ll = []
    for f in indices:
        o = oracle.particle_filter(Y, model, tuple(theta), observations, probs, n_particles, npop, mu, key=key,
                                   filter_index=f)
        ll.append(o["log_zetas"][-1] if o["status"] == 0 else -np.inf)
    ll = np.array(ll)
    top = ll.max()
    if not np.isfinite(top):
        return -np.inf
    return float(top + np.log(np.mean(np.exp(ll - top))))
