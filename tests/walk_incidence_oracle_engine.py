"""Test double for Engine.walk_incidence / incidence_smooth / walk_smooth / smooth / history (TEST INFRASTRUCTURE ONLY):
tests/walk_oracle_engine.py's OracleWalkEngine answered by the numpy restatement (tests/walk_incidence_restatement.py)
and the numpy backends, with every call recorded.  For the CPU tests of epipf.walk_incidence_filter's host logic; the
product has no such fallback."""
import numpy as np

import walk_incidence_restatement as wir
from epipf import smoothing
from epipf.engine import model_id
from walk_oracle_engine import OracleWalkEngine

ENGINES = []


class OracleWalkIncidenceEngine(OracleWalkEngine):
    def __init__(self, *args):
        super().__init__(*args)
        self.calls = []

    def walk_incidence(self, swarm, half_widths, probs, keys, filter_index, counts, observations=False, cumulate=False):
        swarm = np.array(swarm, dtype=np.float64)
        hw = np.array(half_widths, dtype=np.float64)
        S = swarm.shape[0]
        probs = np.broadcast_to(np.asarray(probs, dtype=np.float64), (S,)).copy()
        keys = np.broadcast_to(np.asarray(keys, dtype=np.uint64), (S,)).copy()
        f = np.broadcast_to(np.asarray(filter_index), (S,)).copy()
        counts = np.array(counts, dtype=np.float64)
        self.calls.append(dict(swarm=swarm, hw=hw, probs=probs, keys=keys, f=f, counts=counts, observations=observations,
                               cumulate=cumulate))
        self.name = ["sir", "seir"][self.mid]
        self.T = counts.shape[0] + 2
        self.passes = [wir.one_pass(counts, self.name, swarm[s], hw[s], observations, float(probs[s]),
                                    float(self.npop[0]), float(self.mu[0]), int(keys[s]), int(f[s]), cumulate=cumulate)
                       for s in range(S)]
        return (np.array([r["log_zetas"] for r in self.passes]),
                np.array([r["status"] for r in self.passes], dtype=np.int32))

    def history(self, n_chains=None):
        n = len(self.passes) if n_chains is None else n_chains
        return (np.stack([r["hidden"] for r in self.passes[:n]]), np.stack([r["ancestry"] for r in self.passes[:n]]))

    def incidence_smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), bins=None, lag=None):
        _, _, q = smoothing.check_options("genealogy", "smoothing", quantiles)
        self.smooth_calls.append(dict(kind="flows", n=n_chains, lineage="genealogy", lag=lag))
        nf = wir.ir.F[self.name]
        bins = int(self.npop[0]) + 1 if bins is None else bins
        sums = np.zeros((n_chains, self.T, nf), dtype=np.int64)
        quant = None if q is None else np.zeros((n_chains, q.size, self.T, nf), dtype=np.int64)
        lineages = np.zeros((n_chains, self.T), dtype=np.int32)
        for s, r in enumerate(self.passes[:n_chains]):
            if r["status"] == 0:
                sm, qs, li = wir.smoothed_flows(self.name, r["hidden"], r["ancestry"], lag, q, bins)
                sums[s], lineages[s] = sm, li
                if q is not None:
                    quant[s] = qs
        mean = sums / float(self.N)
        mean[np.array([r["status"] != 0 for r in self.passes[:n_chains]], dtype=bool)] = np.nan
        return smoothing.Smoothed(mean, quant, lineages, sums, None)


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    eng = OracleWalkIncidenceEngine(model_id(type_model), 1, int(n_particles), T, chains)
    ENGINES.append(eng)
    return eng
