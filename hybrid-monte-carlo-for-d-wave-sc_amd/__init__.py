"""MI355X-native fermionic action/force path of DwaveHMC.jl.

Layout:
  csrc/      gfx950 HIP kernels + the C ABI (include/dwhmc.h) -> libdwhmc.so
  _lib.py    ctypes binding of the ABI
  context.py FermionContext: batched device handle
  hmc.py     the reference's hot-path API (ModelParameters ... hmc_sweep)
  vertices.py sparse one-body vertices for measure_operator_response and Nambu
              vertices for measure_nambu_response; site / bond patterns, the
              contraction and the local stiffness maps for measure_response_map
              (host numpy)
  simulation.py run_simulation (src/Simulation.jl): adaptive Nt, log, observables.csv
  replicas.py one-process-per-GPU replica driver (RCCL only gathers observables)

The directory name is not a Python identifier; import it through
`dwhmc_loader.load_package()` (repo root) or `importlib`.
"""
from .hmc import (ComputeCache, ModelParameters, ObservablesResult, SimulationState, calc_optimal_dt,
                  compute_forces, compute_total_energy, diagonalize_H_BdG, hmc_sweep, init_static_H,
                  initialize_cache, initialize_state, measure_observables, neighbour_tables,
                  refresh_momentum, standard_complex_normal, update_H_BdG, SpectrumResult,
                  measure_transport_and_spectra)
from .context import (OBS_LOG_FIELDS, OMELYAN2_LAMBDA, FermionContext, sweep_log_layout, debug_cr_launch, debug_current_vertex, integrator_schedule,
                      selftest_mfma, spectral_window, transport_grid)
from .simulation import AdaptiveNt, SimulationResult, run_simulation, run_simulation_chains
from . import vertices
from ._lib import DwhError, SpectrumGuardError, lib_path, load as load_library

__all__ = [
    "ComputeCache", "ModelParameters", "ObservablesResult", "SimulationState", "calc_optimal_dt",
    "compute_forces", "compute_total_energy", "diagonalize_H_BdG", "hmc_sweep", "init_static_H",
    "initialize_cache", "initialize_state", "measure_observables", "neighbour_tables",
    "refresh_momentum", "standard_complex_normal", "update_H_BdG", "FermionContext", "selftest_mfma",
    "DwhError", "SpectrumGuardError", "lib_path", "load_library", "AdaptiveNt", "SimulationResult",
    "run_simulation", "run_simulation_chains", "SpectrumResult", "measure_transport_and_spectra", "transport_grid",
    "spectral_window", "debug_cr_launch", "debug_current_vertex", "vertices", "integrator_schedule",
    "OMELYAN2_LAMBDA", "OBS_LOG_FIELDS", "sweep_log_layout",
]
