"""Test double for Engine.run_incidence with the `dispersion` keyword (TEST INFRASTRUCTURE ONLY):
tests/incidence_oracle_engine.py's OracleIncidenceEngine, which stays as it is, with the negative-binomial pass answered
by tests/negbin_restatement.py.  A call without a dispersion is the parent's, recorded with dispersion None."""
import numpy as np

import negbin_restatement as nr
from epipf.engine import model_id
from incidence_oracle_engine import OracleIncidenceEngine

ENGINES = []


class OracleNegBinEngine(OracleIncidenceEngine):
    def run_incidence(self, thetas, probs, keys, filter_indices, counts, observations=False, cumulate=False,
                      active=None, dispersion=None):
        if dispersion is None:
            out = super().run_incidence(thetas, probs, keys, filter_indices, counts, observations=observations,
                                        cumulate=cumulate, active=active)
            self.calls[-1]["dispersion"] = None
            return out
        assert not observations
        n = np.asarray(thetas).shape[0]
        kap = np.broadcast_to(np.asarray(dispersion, dtype=np.float64), (n,)).copy()
        act = np.ones(n, dtype=np.int32) if active is None else np.array(active, dtype=np.int32)
        # one chain at a time under its own dispersion: the parent's pass with the product weight replaced
        lz = st = None
        hist = {}
        for c in range(n):
            one = np.zeros(n, dtype=np.int32)
            one[c] = act[c]
            with nr.negbin_weights(float(kap[c])):
                lz_c, st_c = super().run_incidence(thetas, probs, keys, filter_indices, counts, cumulate=cumulate,
                                                   active=one)
            self.calls.pop()
            hist.update(self.hist)
            if lz is None:
                lz, st = lz_c, st_c
            else:
                lz[c], st[c] = lz_c[c], st_c[c]
        self.hist = hist
        thetas = np.array(thetas, dtype=np.float64)
        self.calls.append(dict(thetas=thetas, probs=np.broadcast_to(np.asarray(probs, dtype=np.float64), (n,)).copy(),
                               keys=np.broadcast_to(np.asarray(keys, dtype=np.uint64), (n,)).copy(),
                               f=np.broadcast_to(np.asarray(filter_indices), (n,)).copy(),
                               counts=np.array(counts, dtype=np.float64), observations=False, cumulate=cumulate,
                               active=act, dispersion=kap))
        return lz, st


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    eng = OracleNegBinEngine(model_id(type_model), 1, int(n_particles), T, chains)
    ENGINES.append(eng)
    return eng
