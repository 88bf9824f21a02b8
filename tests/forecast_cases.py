"""Forecast inputs shared by tests/test_forecast_host.py (which pins on the oracle what each case holds) and
tests/test_gpu_forecast_draws.py (which runs them on the device).  Inputs only: nothing here touches the oracle or the
library."""
import numpy as np

# the call of every draws_case test: 7 x 37 = 259 lanes (draws share waves, the second block is partial) and the filter
# index wraps in uint32 inside the batch (draw 3 is at index 0)
DRAWS_R, DRAWS_H, DRAWS_KEY, DRAWS_FIDX = 37, 6, 11, 2**32 - 3
DRAWS_GS = (1, 3, 4, 5, 6, 7, 8)
GAMMAS = (0.9, 0.25, 0.5, 0.0, 1.5)


def draws_case(G, D=7, seed=None):
    """(thetas, states) for sir_subgroups with G groups: thetas a list of D (beta [G, G], gamma) pairs that all differ,
    states [D, 3 G] int64 ((S, I, R) per group).  Draw 1 has no infected, draw 2 one infected person in group 0, the
    last draw all-zero rates (with infected present)."""
    rs = np.random.RandomState(100 + G if seed is None else seed)
    thetas, states = [], []
    for d in range(D):
        beta = rs.uniform(0.05, 2.5, (G, G)) * (0.3 + 1.4 * d / max(D - 1, 1))
        gamma = GAMMAS[d % 5]
        x = np.stack([rs.randint(10, 40, G), rs.randint(0, 4, G), rs.randint(0, 5, G)], axis=1)
        if d == 1:
            x[:, 1] = 0
        elif d == 2:
            x[:, 1] = 0
            x[0, 1] = 1
        if d == D - 1:
            beta, gamma = np.zeros((G, G)), 0.0
            x[0, 1] = max(x[0, 1], 1)
        thetas.append((beta, gamma))
        states.append(x.reshape(-1))
    return thetas, np.array(states, dtype=np.int64)


def flat_thetas(thetas):
    """(beta, gamma) pairs -> the flat [D, G G + 1] layout (beta row-major, then gamma)."""
    return np.stack([np.append(np.asarray(b, dtype=np.float64).reshape(-1), g) for b, g in thetas])


# small fixed batches of the two narrow models, for the tests that are not about G
SIR_DRAWS = (np.array([[0.9, 0.45], [0.3, 0.6], [1.7, 0.2], [0.0, 0.0], [1.1, 0.0]]),
             np.array([[60, 3, 0], [80, 1, 4], [40, 12, 9], [30, 5, 1], [25, 2, 0]]))
SEIR_DRAWS = (np.array([[0.8, 0.5, 0.3], [1.5, 0.9, 0.4], [0.4, 1.2, 0.9], [2.0, 0.3, 0.0], [0.0, 0.0, 0.0]]),
              np.array([[70, 4, 2, 0], [50, 0, 6, 3], [45, 3, 0, 1], [30, 1, 1, 0], [20, 2, 2, 2]]))

# the ten instances of forecast_kernel: (model, G)
INSTANCES = [("sir", 1), ("seir", 1)] + [("sir_subgroups", G) for G in range(1, 9)]
SWEEP_SEEDS = range(24)


def sweep_case(seed):
    """One randomised forecast call as a dict (model, G, thetas [D, d], states [D, C], D, R, H, key, filter_index,
    step).  Seed s runs instance s mod 10, so 24 seeds launch every instance at least twice."""
    model, G = INSTANCES[seed % len(INSTANCES)]
    rs = np.random.RandomState(5000 + seed)
    R = int(rs.choice([1, 3, 37, 64, 100]))
    H = int(rs.choice([1, 2, 9]))
    D = int(rs.choice([1, 2, 5, 64, 65]))
    while D * R > 6500:
        D = int(rs.choice([1, 2, 5, 64, 65]))
    C = 3 if model == "sir" else 4 if model == "seir" else 3 * G
    states = rs.randint(0, 61, (D, C)).astype(np.int64)
    if model == "sir":
        thetas = np.stack([rs.uniform(0.1, 2.5, D), rs.uniform(0.05, 1.2, D)], axis=1)
    elif model == "seir":
        thetas = np.stack([rs.uniform(0.1, 2.5, D), rs.uniform(0.1, 1.5, D), rs.uniform(0.05, 1.2, D)], axis=1)
    else:
        # a row of beta sums to about what one SIR beta is, so the epidemics of wide models take days as well
        beta = rs.uniform(0.05, 2.5, (D, G, G)) / G
        thetas = np.concatenate([beta.reshape(D, -1), rs.uniform(0.05, 1.2, (D, 1))], axis=1)
    idle = rs.uniform(size=D) < 0.15                         # nobody infected
    frozen = rs.uniform(size=D) < 0.15                       # all-zero rates
    states[np.ix_(idle, infected_columns(model, G))] = 0
    thetas[frozen] = 0.0
    return dict(model=model, G=G, thetas=thetas, states=states, D=D, R=R, H=H,
                key=int(rs.randint(0, 2**63, dtype=np.int64)), filter_index=int(rs.randint(0, 2**32, dtype=np.int64)),
                step=int(rs.randint(0, 2**24)))


def infected_columns(model, G):
    """Columns of a state whose sum being zero means the path is extinct (SEIR: exposed and infectious)."""
    return [1] if model == "sir" else [1, 2] if model == "seir" else list(range(1, 3 * G, 3))
