"""Test double for Engine.forecast_summary that answers from the CPU oracle (TEST INFRASTRUCTURE ONLY): the engine double
of tests/oracle_engine.py with the one method epipf.forecast_summary calls, so the Python layer above the C ABI runs
without a GPU.  The product has no such fallback."""
import numpy as np

from epipf.engine import model_id
from forecast_helpers import reference_thetas
from forecast_summary_helpers import FIELDS, oracle_summaries, reductions
from oracle_engine import OracleEngine

NAMES = ["sir", "seir", "sir_subgroups", "sir_subgroups2"]


class SummaryOracleEngine(OracleEngine):
    calls = []                                            # (thetas, states, H, R, key, filter_index, step) of each call

    def forecast_summary(self, thetas, states, horizon, replicates=1, key=0, filter_index=0, step=0, per_path=False,
                         bins=0):
        thetas, states = np.asarray(thetas, dtype=np.float64), np.asarray(states).reshape(-1, self.C)
        type(self).calls.append((thetas.copy(), states.copy(), horizon, replicates, key, filter_index, step))
        D, H, R = states.shape[0], int(horizon), int(replicates)
        model = NAMES[self.mid]
        o = oracle_summaries(model, self.G, reference_thetas(model, self.G, thetas), states, H, R, key, filter_index, step)
        out = reductions(o, H, bins)
        if not bins:
            out["peak_hist"] = out["infections_hist"] = None
        out["paths"] = tuple(o[f] for f in FIELDS) if per_path else None
        return out


def fake_get_engine(type_model, groups, n_particles, T, chains=1, device=0):
    mid = model_id(type_model)
    return SummaryOracleEngine(mid, groups if mid >= 2 else 1, int(n_particles), T, chains)
