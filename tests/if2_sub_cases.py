"""The inputs of the subgroup iterated-filtering tests (a helper, no test itself): tests/test_if2_sub_restatement.py
pins on the CPU what each case contains (status, completed iterations, reflections, event counts),
tests/test_gpu_if2_sub.py runs the same inputs on the device against the restatement (tests/if2_sub_restatement.py)."""
import os

import numpy as np

import if2_restatement as rs
import if2_sub_restatement as srs
from conftest import GOLDEN

KEY, F = 11, 3
GROUPS = (2, 3, 4)
MODELS = srs.MODELS
PROBS = {False: 0.5, True: 0.2}                         # binomial p / normal noise ratio
COOLING = 0.5 ** (50 / 12)


def rw_of(G, diag=0.1, off=0.05, gamma=0.05):
    """Random-walk half-widths: `diag` on beta's diagonal, `off` beside it, `gamma` last."""
    return srs.to_flat(np.where(np.eye(G, dtype=bool), diag, off), gamma)


def load_fixture():
    """{G: dict(sir_subgroups=Y [20, 3G], sir_subgroups2=Y summed over the groups [20, 3], theta, npop, mu)}, probs."""
    z = np.load(os.path.join(GOLDEN, "if2_sub_small.npz"))
    out = dict(probs=float(z["probs"]))
    for G in GROUPS:
        Y = z[f"g{G}_Y"]
        out[G] = dict(sir_subgroups=Y, sir_subgroups2=srs.observed("sir_subgroups2", Y), theta=z[f"g{G}_theta"],
                      npop=z[f"g{G}_population"], mu=z[f"g{G}_mu"])
    return out


def case(fx, model, G, N, T, M=2, observations=False, probs=None, hw=None, swarm0=None, key=KEY, f=F):
    """One search's inputs; the defaults are the fixture's first T rows, its true theta in every row and cooled
    half-widths."""
    g = fx[G]
    return dict(model=model, G=G, Y=np.asarray(g[model][:T], dtype=np.float64),
                swarm0=np.tile(g["theta"], (N, 1)) if swarm0 is None else np.asarray(swarm0, dtype=np.float64),
                hw=rs.cooling_table(rw_of(G), COOLING, M) if hw is None else np.asarray(hw, dtype=np.float64),
                observations=observations, probs=PROBS[observations] if probs is None else probs,
                npop=g["npop"], mu=g["mu"], key=key, f=f)


def restate(c):
    return srs.run(c["Y"], c["model"], c["swarm0"], c["hw"], c["observations"], c["probs"], c["npop"], c["mu"],
                   c["key"], c["f"])


def distinct(swarm):
    return len(np.unique(np.asarray(swarm), axis=0))


# ------------------------------------------------------------------------------------------- 2. parity with jitter
def parity_case(fx, model, G):
    return case(fx, model, G, 65, 12, M=3)


# ------------------------------------------------------------------------------------------- 3. reflection
REFLECT_KEY = 5


def reflection_case(fx):
    return case(fx, "sir_subgroups", 2, 48, 4, hw=np.full((2, 5), 0.05), swarm0=np.full((48, 5), 0.01), key=REFLECT_KEY,
                f=0)


# ------------------------------------------------------------------------------------------- 4. fixed components
def fixed_case(fx, model="sir_subgroups"):
    """Off-diagonal contacts never jittered (half-width 0): 0 in the even rows, 0.3 in the odd ones, so that lanes
    with zero and non-zero rates sit in one wave."""
    swarm0 = np.tile(fx[2]["theta"], (130, 1))
    swarm0[0::2, 1:3] = 0.0
    return case(fx, model, 2, 130, 7, hw=rs.cooling_table(rw_of(2, off=0.0), COOLING, 2), swarm0=swarm0)


# ------------------------------------------------------------------------------------------- 5. batching
STARTS = np.array([[1.2, 0.3, 0.3, 0.9, 0.35], [1.0, 0.2, 0.4, 1.1, 0.4], [1.4, 0.4, 0.2, 0.8, 0.3]])
KEYS = np.array([101, 202, 303], dtype=np.uint64)
F0 = np.array([0, 7, 0xFFFFFFFF])                       # the last search's second iteration wraps to filter index 0


def batch_cases(fx, M=2):
    return [case(fx, "sir_subgroups", 2, 65, 12, M=M, swarm0=np.tile(STARTS[s], (65, 1)), key=int(KEYS[s]), f=int(F0[s]),
                 hw=rs.cooling_table(rw_of(2), 0.5, M)) for s in range(3)]


# a search that dies at once between two that complete: rates far too high for the data
DEGENERATE_STARTS = np.array([[1.2, 0.3, 0.3, 0.9, 0.35], [6.0, 3.0, 3.0, 6.0, 0.01], [1.0, 0.2, 0.4, 1.1, 0.4]])


def degenerate_cases(fx):
    return [case(fx, "sir_subgroups", 2, 48, 20, M=3, swarm0=np.tile(DEGENERATE_STARTS[s], (48, 1)), key=s + 1, f=0)
            for s in range(3)]


# ------------------------------------------------------------------------------------------- 6. paths
def path_case(fx, model, G):
    return case(fx, model, G, 130, 7)


# ------------------------------------------------------------------------------------------- 8. end to end
SEARCH = dict(N=48, M=12, rw=(0.1, 0.05, 0.05, 0.1, 0.05), cooling=COOLING, start=(1.6, 0.6, 0.6, 1.4, 0.55))
SEARCH_KEY = 1                                           # epipf.if2_subgroups' key: search s runs under chain_key(1, s)
SEARCHES = 2
# the CPU restatement's searches (tests/test_if2_sub_restatement.py recomputes them): rs.score of the start, and of each
# search's final swarm mean (400 particles, key 77, 8 filters); a third search of sir_subgroups (chain_key(1, 2))
# degenerates in its third iteration, which is why two are run
START_SCORE = {"sir_subgroups": -113.09805325356199, "sir_subgroups2": -115.97170328039535}
FINAL_SCORE = {"sir_subgroups": (-87.35508248788959, -98.18450033038634),
               "sir_subgroups2": (-80.59282828751823, -85.30515545397009)}


def cpu_gains(model):
    return [v - START_SCORE[model] for v in FINAL_SCORE[model]]


def search_case(fx, model, s):
    """Search s of the end-to-end test: the whole G = 2 series from a start 30-40 % off."""
    k = SEARCH_KEY + (s << 32)                           # chain_key(SEARCH_KEY, s)
    return case(fx, model, 2, SEARCH["N"], 20, hw=rs.cooling_table(SEARCH["rw"], SEARCH["cooling"], SEARCH["M"]),
                swarm0=np.tile(np.array(SEARCH["start"]), (SEARCH["N"], 1)), key=k, f=0)
