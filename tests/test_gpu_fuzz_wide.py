"""Randomised parity sweep of the HIP filter against the CPU oracle at G = 5..8 groups: the generator of
tests/test_gpu_fuzz.py restated for the wide subgroup models -- 24 seeded cases over both models, N from
{1, 63, 64, 65, 300} (single particle, ragged and full waves), T up to 6, populations of 60, 500 and 4820 per group
(the small ones die out inside a step and reach the eligibility bounds on sum(N)), beta scaled by 2 / G (the force
of infection sums over G groups), extinct starts (mu = 0), 1-3 chains
per launch with their own keys and filter indices, multinomial and systematic resampling, lanes automatic or 1 (the
only ones these G have).  The status, every state and every ancestor must equal the oracle's and the log-likelihoods
agree within 1e-9; a filter that degenerates on both sides is a valid case.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

CASES = 24


def _case(seed):
    rs = np.random.RandomState(9000 + seed)
    model = ["sir_subgroups", "sir_subgroups2"][seed % 2]
    G = 5 + (seed // 2) % 4
    C = 3 * G
    K = 3 if model == "sir_subgroups2" else C
    N = int(rs.choice([1, 63, 64, 65, 300]))
    T = int(rs.randint(1, 7))
    npop = np.round(rs.choice([60.0, 500.0, 4820.0], size=G)).astype(np.float64)
    mu = np.where(rs.rand(G) < 0.1, 0.0, np.round(rs.uniform(1, 40, G)))
    mu = np.minimum(mu, npop / 2)
    probs = float(rs.choice([0.05, 0.1, 0.4]))
    theta = (rs.uniform(0.2, 4.0, (G, G)) / G * 2.0, float(rs.uniform(0.2, 1.5)))
    # observations around probs x the initial compartments, growing a little with t
    base = np.zeros(C)
    for g in range(G):
        base[3 * g:3 * g + 3] = [npop[g] - mu[g], mu[g], 0.0]
    Y = np.zeros((T, K))
    for t in range(T):
        x = base.copy()
        for g in range(G):
            s = min(t * 3.0, x[3 * g])
            x[3 * g] -= s; x[3 * g + 1] += s / 2; x[3 * g + 2] += s / 2
        xo = x if model != "sir_subgroups2" else x.reshape(G, 3).sum(0)
        Y[t] = np.floor(probs * xo)
    chains = int(rs.randint(1, 4))
    lanes = int(rs.choice([0, 1]))
    resample = "systematic" if rs.rand() < 0.25 else "multinomial"
    keys = [int(k) for k in rs.randint(1, 2**31, chains)]
    fidx = [int(f) for f in rs.randint(0, 10**6, chains)]
    thetas = [(theta[0] * (1 + 0.05 * c), theta[1]) for c in range(chains)]   # chain c: theta scaled a little
    return dict(model=model, G=G, N=N, Y=Y, npop=npop, mu=mu, probs=probs, thetas=thetas, keys=keys, fidx=fidx,
                lanes=lanes, resample=resample)


@pytest.mark.parametrize("seed", range(CASES))
def test_random_wide_filters_match_oracle(seed):
    from epipf.engine import Engine, model_id, theta_vector
    a = _case(seed)
    mid = model_id(a["model"])
    th = np.stack([theta_vector(mid, t)[0] for t in a["thetas"]])
    chains = th.shape[0]
    eng = Engine(a["model"], a["G"], a["N"], a["Y"].shape[0], chains)
    try:
        eng.set_observations(a["Y"])
        eng.set_population(a["npop"], a["mu"])
        eng.set_lanes(a["lanes"])
        lz, st = eng.run(th, [a["probs"]] * chains, a["keys"], a["fidx"], resample=a["resample"])
        hid, anc = eng.history(chains)
        assert eng.stats()["last_lanes"] == 1 and eng.stats()["last_fused"] == 0
    finally:
        eng.close()
    for c in range(chains):
        o = oracle.particle_filter(a["Y"], a["model"], a["thetas"][c], False, a["probs"], a["N"], a["npop"], a["mu"],
                                   key=a["keys"][c], filter_index=a["fidx"][c], resample=a["resample"])
        assert int(st[c]) == o["status"], (seed, c, a["model"], a["G"], a["N"], int(st[c]), o["status"])
        # a degenerate filter (all weights 0 / NaN at some step: the reference's ValueError) is compared up to the
        # step that failed, where both report -inf
        olz = o["log_zetas"]
        P = len(olz) if not o["status"] else int(np.argmax(~np.isfinite(olz)))
        assert not o["status"] or not np.isfinite(lz[c, P]), (seed, c, lz[c, P])
        np.testing.assert_array_equal(hid[c][:P], o["hidden"][:P], err_msg=f"seed {seed} chain {c}")
        np.testing.assert_array_equal(anc[c][:P], o["ancestry"][:P], err_msg=f"seed {seed} chain {c}")
        np.testing.assert_allclose(lz[c][:P], olz[:P], rtol=1e-12, atol=1e-9, err_msg=f"seed {seed} chain {c}")
