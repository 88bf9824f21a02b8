"""Test double for Engine.walk_filter / walk_smooth / smooth (TEST INFRASTRUCTURE ONLY): tests/oracle_engine.py's
OracleEngine answered by the numpy restatement (tests/walk_restatement.py) and the numpy backends, with every call
recorded.  For the CPU tests of epipf.walk_filter's host logic; the product has no such fallback."""
import numpy as np

import walk_restatement as wr
from epipf import _lib, smoothing, walk
from epipf.engine import model_id
from oracle_engine import OracleEngine

ENGINES = []


class OracleWalkEngine(OracleEngine):
    def __init__(self, *args):
        super().__init__(*args)
        self.walk_calls, self.smooth_calls = [], []

    def walk_filter(self, swarm, half_widths, probs, keys, filter_index, observations=False):
        swarm = np.array(swarm, dtype=np.float64)
        hw = np.asarray(half_widths, dtype=np.float64)
        S = swarm.shape[0]
        probs = np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,))
        keys = np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,))
        f = np.broadcast_to(np.asarray(filter_index), (S,))
        self.walk_calls.append(dict(swarm=swarm.copy(), hw=hw.copy(), keys=keys.copy(), f=f.copy()))
        name = ["sir", "seir"][self.mid]
        self.passes = [wr.one_pass(self.Y, name, swarm[s], hw[s], observations, float(probs[s]), float(self.npop[0]),
                                   float(self.mu[0]), int(keys[s]), int(f[s])) for s in range(S)]
        return (np.array([r["log_zetas"] for r in self.passes]),
                np.array([r["status"] for r in self.passes], dtype=np.int32))

    def walk_smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), lineage="genealogy", lag=None):
        lin, _, q = smoothing.check_options(lineage, "smoothing", quantiles)
        self.smooth_calls.append(dict(kind="walk", n=n_chains, lineage=lineage, lag=lag))
        d = self.passes[0]["theta_hist"].shape[2]
        mean = np.full((n_chains, self.T, d + 1), np.nan)
        quant = None if q is None else np.full((n_chains, q.size, self.T, d + 1), np.nan)
        lineages = np.zeros((n_chains, self.T), dtype=np.int32)
        for s, r in enumerate(self.passes[:n_chains]):
            if r["status"] == 0:
                m, qs, li = walk._reduce_numpy(r["hidden"], r["ancestry"], r["theta_hist"], float(self.npop[0]), lin, lag, q)
                mean[s], lineages[s] = m, li
                if q is not None:
                    quant[s] = qs
        return mean, quant, lineages

    def smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), lineage="genealogy", kind="smoothing", bins=None,
               lag=None):
        self.smooth_calls.append(dict(kind="states", n=n_chains, lineage=lineage, lag=lag))
        return ("states", n_chains, lineage, lag)


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    eng = OracleWalkEngine(model_id(type_model), 1, int(n_particles), T, chains)
    ENGINES.append(eng)
    return eng
