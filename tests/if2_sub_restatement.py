"""numpy restatement of iterated filtering for the subgroup models as DESIGN.md §17.1 defines it (a helper for the
tests, no test itself).

tests/if2_restatement.py with theta = beta[G][G] row-major then gamma (d = G*G + 1): the same domain-7 draws
(rs.perturb_uniforms: component c from block c // 2), the same reflection, weights (rs.weights, on the sums over the
groups for sir_subgroups2), resampling, logarithm and swarm mean.  Particle j's day is oracle.simulate on row j with that
particle's own (beta, gamma)."""
import numpy as np

import if2_restatement as rs
import oracle
import philox

DEGENERATE = rs.DEGENERATE
MODELS = ("sir_subgroups", "sir_subgroups2")


def groups_of(d):
    """G of a flat theta with d = G*G + 1 entries."""
    G = int(round((d - 1) ** 0.5))
    assert G * G + 1 == d, d
    return G


def to_pair(theta):
    """flat [G*G + 1] -> the reference's (beta[G][G], gamma)."""
    theta = np.asarray(theta, dtype=np.float64)
    G = groups_of(theta.shape[-1])
    return theta[:G * G].reshape(G, G), float(theta[G * G])


def to_flat(beta, gamma):
    """(beta[G][G], gamma) -> flat [G*G + 1]: beta row-major, then gamma."""
    return np.append(np.asarray(beta, dtype=np.float64).reshape(-1), float(gamma))


def observed(model, x):
    """What the model observes of the states x [N, 3G]: every column, or for sir_subgroups2 the sums over the groups
    [N, 3] (S, I, R), added in group order as float64 (exact: they are counts)."""
    x = np.asarray(x)
    if model != "sir_subgroups2":
        return x
    G = x.shape[1] // 3
    out = np.zeros((x.shape[0], 3))
    for g in range(G):
        out = out + x[:, 3 * g:3 * g + 3].astype(np.float64)
    return out


def one_pass(Y, model, theta, hw, observations, probs, npop, mu, key, f):
    """One iteration at filter index f from the swarm theta [N, d]; rs.one_pass's returns."""
    assert model in MODELS
    Y = np.asarray(Y, dtype=np.float64)
    T = Y.shape[0]
    theta = np.asarray(theta, dtype=np.float64)
    N, d = theta.shape
    first = oracle.particle_filter(Y[:1], model, to_pair(theta[0]), observations, probs, N, npop, mu, key=key,
                                   filter_index=f)
    C = first["hidden"].shape[2]
    hidden = np.zeros((T, N, C), dtype=np.int32)
    anc = np.zeros((T, N), dtype=np.int32)
    lz = np.zeros(T)
    hidden[0] = first["hidden"][0]
    reflections, events = 0, 0

    def jitter(th, p):
        nonlocal reflections
        u = rs.perturb_uniforms(key, f, p, N, d)
        t = th + np.asarray(hw, dtype=np.float64) * (2.0 * u - 1.0)
        reflections += int(np.count_nonzero(t < 0.0))
        return np.where(t < 0.0, -t, t)

    th = jitter(theta, 0)
    status = 0
    for p in range(1, T):
        w = rs.weights(model, observed(model, hidden[p - 1]), Y[p - 1], observations, probs)
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
            out, nev = oracle.simulate(model, rows, to_pair(th[j]), 1.0, key, f, p)
            hidden[p, j] = out[j]
            events += nev
    return dict(status=status, theta=th, hidden=hidden, ancestry=anc, log_zetas=lz, reflections=reflections,
                events=events)


def run(Y, model, swarm, hw, observations, probs, npop, mu, key, f0):
    """M = len(hw) iterations from the swarm [N, d] at filter indices f0, f0 + 1, ...; rs.run's returns."""
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


def score(Y, model, theta, observations, probs, npop, mu, n_particles=400, key=77, indices=range(8)):
    """rs.score at a flat theta."""
    return rs.score(Y, model, to_pair(theta), observations, probs, npop, mu, n_particles=n_particles, key=key,
                    indices=indices)
