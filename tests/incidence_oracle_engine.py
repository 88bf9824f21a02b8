"""Test double for Engine.run_incidence / path_sample / history / smooth (TEST INFRASTRUCTURE ONLY):
tests/oracle_engine.py's OracleEngine answered by the numpy restatement (tests/incidence_restatement.py), with every call
recorded.  For the CPU tests of epipf.incidence's host logic; the product has no such fallback."""
import numpy as np

import incidence_restatement as ir
from epipf.engine import model_id
from oracle_engine import OracleEngine

ENGINES = []


class OracleIncidenceEngine(OracleEngine):
    def __init__(self, *args):
        super().__init__(*args)
        self.calls, self.smooth_calls = [], []

    def run_incidence(self, thetas, probs, keys, filter_indices, counts, observations=False, cumulate=False,
                      active=None):
        thetas = np.array(thetas, dtype=np.float64)
        n = thetas.shape[0]
        probs = np.broadcast_to(np.asarray(probs, dtype=np.float64), (n,)).copy()
        keys = np.broadcast_to(np.asarray(keys, dtype=np.uint64), (n,)).copy()
        f = np.broadcast_to(np.asarray(filter_indices), (n,)).copy()
        counts = np.array(counts, dtype=np.float64)
        act = np.ones(n, dtype=np.int32) if active is None else np.array(active, dtype=np.int32)
        self.calls.append(dict(thetas=thetas, probs=probs, keys=keys, f=f, counts=counts, observations=observations,
                               cumulate=cumulate, active=act))
        name = ["sir", "seir"][self.mid]
        self.T = counts.shape[0] + 2
        lz = np.full((n, self.T), np.nan)
        st = np.full(n, 2, dtype=np.int32)
        self.hist = {}
        for c in range(n):
            if not act[c]:
                continue
            r = ir.one_pass(counts, name, thetas[c], observations, float(probs[c]), self.N, float(self.npop[0]),
                            float(self.mu[0]), int(keys[c]), int(f[c]), cumulate=cumulate)
            lz[c], st[c] = r["log_zetas"], r["status"]
            if r["status"] == 0:
                self.hist[c] = (r["hidden"], r["ancestry"])
        return lz, st

    def history(self, n_chains=None):
        n = len(self.calls[-1]["thetas"]) if n_chains is None else n_chains
        hid = np.zeros((n, self.T, self.N, self.C), dtype=np.int32)
        anc = np.zeros((n, self.T, self.N), dtype=np.int32)
        for c, (h, a) in self.hist.items():
            if c < n:
                hid[c], anc[c] = h, a
        return hid, anc

    def smooth(self, n_chains=None, quantiles=(0.05, 0.5, 0.95), lineage="genealogy", kind="smoothing", bins=None,
               lag=None):
        self.smooth_calls.append(dict(n=n_chains, quantiles=quantiles, lineage=lineage, kind=kind, lag=lag))
        return ("states", n_chains, lineage, lag)


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    eng = OracleIncidenceEngine(model_id(type_model), 1, int(n_particles), T, chains)
    ENGINES.append(eng)
    return eng
