"""The inputs of the IF2 path tests (a helper, no test itself): tests/test_if2_restatement.py pins on the CPU what each
case contains (status, completed iterations, distinct rows), tests/test_gpu_if2_paths.py runs the same inputs on the
device against the restatement (tests/if2_restatement.py)."""
import os

import numpy as np

import if2_restatement as rs
import oracle
from conftest import GOLDEN

KEY, F = 11, 3
THETA = {"sir": (0.8, 0.3), "seir": (0.9, 0.6, 0.3)}
RW = {"sir": (0.1, 0.05), "seir": (0.1, 0.08, 0.05)}
PROBS = {False: 0.5, True: 0.2}                         # binomial p / normal noise ratio
COOLING = 0.5 ** (50 / 12)


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "if2_sir_small.npz"))
    Y = z["Y"]
    Y4 = np.concatenate([Y[:, :1], Y[:, 1:2] // 2, Y[:, 1:2] - Y[:, 1:2] // 2, Y[:, 2:]], axis=1)   # S, E, I, R
    return dict(sir=Y, seir=Y4, npop=float(z["population"]), mu=float(z["mu"]), probs=float(z["probs"]))


def case(fx, model, N, T, M=2, observations=False, probs=None, hw=None, swarm0=None, key=KEY, f=F, Y=None, npop=None,
         mu=None):
    """One search's inputs; the defaults are the fixture's first T rows, the file's theta and cooled half-widths."""
    return dict(model=model, Y=np.asarray(fx[model][:T] if Y is None else Y, dtype=np.float64),
                swarm0=np.tile(np.array(THETA[model]), (N, 1)) if swarm0 is None else np.asarray(swarm0, dtype=np.float64),
                hw=rs.cooling_table(RW[model], COOLING, M) if hw is None else np.asarray(hw, dtype=np.float64),
                observations=observations, probs=PROBS[observations] if probs is None else probs,
                npop=fx["npop"] if npop is None else npop, mu=fx["mu"] if mu is None else mu, key=key, f=f)


def restate(c):
    return rs.run(c["Y"], c["model"], c["swarm0"], c["hw"], c["observations"], c["probs"], c["npop"], c["mu"], c["key"],
                  c["f"])


def distinct(swarm):
    return len(np.unique(np.asarray(swarm), axis=0))


# ------------------------------------------------------------------------------------------- 5. late degeneracy
LATE = {5: (1, 1, 3), 10: (1, 2, 7), 28: (1, 3, 4), 15: (0, 4, None)}    # key: status, done, dying step


def late_case(fx, key):
    return case(fx, "sir", 5, 25, hw=np.tile((0.1, 0.05), (4, 1)), key=key, f=0)


def dying_step(r):
    """The first -inf of the last executed pass's log_zetas (None: it completed)."""
    dead = np.isneginf(r["last_log_zetas"])
    return int(np.argmax(dead)) if dead.any() else None


# ------------------------------------------------------------------------------------------- 6. larger populations
def epidemic(npop, mu, T):
    """X [T, 3]: x_0 = (npop - mu, mu, 0), day p = oracle.simulate of day p - 1 at theta (1.2, 0.4), key 999, step p."""
    X = np.zeros((T, 3), dtype=np.int32)
    X[0] = (npop - mu, mu, 0)
    for p in range(1, T):
        X[p] = oracle.simulate("sir", X[p - 1:p], (1.2, 0.4), 1.0, 999, 0, p)[0][0]
    return X


def population_case(fx, npop, mu, T, observations):
    """N = 130 from (1.2, 0.4): binomial on Y = floor(0.3 X) with p = 0.3, or normal on Y = X with noise ratio 0.05."""
    X = epidemic(npop, mu, T)
    Y = X.astype(np.float64) if observations else np.floor(0.3 * X)
    return case(fx, "sir", 130, T, observations=observations, probs=0.05 if observations else 0.3,
                hw=rs.cooling_table((0.1, 0.05), 0.5, 2), swarm0=np.tile((1.2, 0.4), (130, 1)), Y=Y, npop=float(npop),
                mu=float(mu))


# ------------------------------------------------------------------------------------------- 8. mixed rates in a wave
def mixed_case(fx, T, odd_beta):
    swarm0 = np.tile((0.8, 0.3), (130, 1))
    swarm0[1::2, 0] = odd_beta
    return case(fx, "sir", 130, T, hw=[[0.0, 0.05], [0.0, 0.025]], swarm0=swarm0)
