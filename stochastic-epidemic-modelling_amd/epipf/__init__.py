"""epipf: MI355X-native bootstrap particle filter / PMCMC for stochastic epidemic models.

Drop-in for the reference's pmcmc.py hot path (particle_filter, particle_path_sampler,
particle_mcmc, ModelType) and its Gillespie simulators, with the filter running as HIP kernels in
libepipf.so (C ABI: include/epipf.h).  See DESIGN.md.
"""
from .engine import Engine, get_engine  # noqa: F401
from .pmcmc import (ModelType, chain_key, particle_filter, particle_mcmc, particle_mcmc_chains,  # noqa: F401
                    particle_path_sampler, seed_stream)
from .gillespie import (sir_simulate, seir_simulate, sir_subgroups_simulate, simulate_batch,  # noqa: F401
                        simulate_path_batch)
from .abc import abc_algo, abc_run, abc_smc  # noqa: F401
from .forecast import forecast, forecast_from_chain  # noqa: F401
from .forecast_summary import ForecastSummary, forecast_summary, forecast_summary_from_chain  # noqa: F401
from .smoothing import Smoothed, particle_smoother, smooth_history  # noqa: F401
from .if2 import If2Result, if2, if2_subgroups  # noqa: F401
from .walk import WalkResult, walk_filter  # noqa: F401
from .incidence import IncidenceResult, incidence_filter, incidence_mcmc  # noqa: F401
from .walk_incidence import walk_incidence_filter  # noqa: F401

__all__ = ["Engine", "get_engine", "ModelType", "particle_filter", "particle_mcmc", "particle_mcmc_chains",
           "particle_path_sampler", "seed_stream", "chain_key", "sir_simulate", "seir_simulate",
           "sir_subgroups_simulate", "simulate_batch", "simulate_path_batch", "abc_algo", "abc_run", "abc_smc", "forecast",
           "forecast_from_chain", "Smoothed", "particle_smoother", "smooth_history", "if2", "if2_subgroups", "If2Result",
           "ForecastSummary", "forecast_summary", "forecast_summary_from_chain", "walk_filter", "WalkResult",
           "incidence_filter", "incidence_mcmc", "IncidenceResult", "walk_incidence_filter"]
