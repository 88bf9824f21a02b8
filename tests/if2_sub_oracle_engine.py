"""Test double for Engine.if2_subgroups (TEST INFRASTRUCTURE ONLY): tests/if2_oracle_engine.py's OracleIf2Engine plus an
if2_subgroups() answered by the numpy restatement (tests/if2_sub_restatement.py), with every call recorded.  For the CPU
tests of epipf.if2_subgroups' host logic; the product has no such fallback."""
import numpy as np

import if2_sub_restatement as srs
from epipf.engine import model_id
from if2_oracle_engine import OracleIf2Engine


class OracleIf2SubEngine(OracleIf2Engine):
    def if2_subgroups(self, swarm, half_widths, probs, keys, filter_index0, observations=False):
        swarm = np.array(swarm, dtype=np.float64)
        hw = np.asarray(half_widths, dtype=np.float64)
        S, M = swarm.shape[0], hw.shape[0]
        probs = np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,))
        keys = np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,))
        f0 = np.broadcast_to(np.asarray(filter_index0), (S,))
        self.if2_calls.append(dict(swarm=swarm.copy(), hw=hw.copy(), keys=keys.copy(), f0=f0.copy()))
        name = ["sir", "seir", "sir_subgroups", "sir_subgroups2"][self.mid]
        assert self.mid >= 2 and swarm.shape[2] == self.G * self.G + 1
        mean = np.empty((S, M, swarm.shape[2]))
        lz = np.empty((S, M, self.T))
        done = np.zeros(S, dtype=np.int32)
        st = np.zeros(S, dtype=np.int32)
        for s in range(S):
            r = srs.run(self.Y, name, swarm[s], hw, observations, float(probs[s]), self.npop, self.mu, int(keys[s]),
                        int(f0[s]))
            swarm[s], mean[s], lz[s], done[s], st[s] = r["swarm"], r["mean"], r["log_zetas"], r["iterations_done"], r["status"]
        return swarm, mean, lz, done, st


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    mid = model_id(type_model)
    return OracleIf2SubEngine(mid, groups if mid >= 2 else 1, int(n_particles), T, chains)
