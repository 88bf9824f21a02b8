"""Test double for Engine.if2 (TEST INFRASTRUCTURE ONLY): tests/oracle_engine.py's OracleEngine plus an if2() answered by
the numpy restatement (tests/if2_restatement.py), with every call recorded.  For the CPU tests of epipf.if2's host
logic; the product has no such fallback."""
import numpy as np

import if2_restatement as rs
from epipf.engine import model_id
from oracle_engine import OracleEngine


class OracleIf2Engine(OracleEngine):
    def __init__(self, *args):
        super().__init__(*args)
        self.if2_calls, self.run_calls = [], []

    def if2(self, swarm, half_widths, probs, keys, filter_index0, observations=False):
        swarm = np.array(swarm, dtype=np.float64)
        hw = np.asarray(half_widths, dtype=np.float64)
        S, M = swarm.shape[0], hw.shape[0]
        probs = np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,))
        keys = np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,))
        f0 = np.broadcast_to(np.asarray(filter_index0), (S,))
        self.if2_calls.append(dict(swarm=swarm.copy(), hw=hw.copy(), keys=keys.copy(), f0=f0.copy()))
        name = ["sir", "seir"][self.mid]
        mean = np.empty((S, M, swarm.shape[2]))
        lz = np.empty((S, M, self.T))
        done = np.zeros(S, dtype=np.int32)
        st = np.zeros(S, dtype=np.int32)
        for s in range(S):
            r = rs.run(self.Y, name, swarm[s], hw, observations, float(probs[s]), float(self.npop[0]),
                       float(self.mu[0]), int(keys[s]), int(f0[s]))
            swarm[s], mean[s], lz[s], done[s], st[s] = r["swarm"], r["mean"], r["log_zetas"], r["iterations_done"], r["status"]
        return swarm, mean, lz, done, st

    def run(self, thetas, probs, keys, fidx, **kw):
        self.run_calls.append(dict(thetas=np.array(thetas), keys=np.array(keys), fidx=np.array(fidx)))
        return super().run(thetas, probs, keys, fidx, **kw)


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    return OracleIf2Engine(model_id(type_model), 1, int(n_particles), T, chains)
