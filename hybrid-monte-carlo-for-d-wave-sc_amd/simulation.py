"""run_simulation: the reference's driver (src/Simulation.jl:34-236) over the
MI355X hot path.

Same phases, adaptive-Nt rule, log lines and observables.csv format as the
reference; every sweep's fermionic work runs on the GPU through the C ABI
(hmc.py -> FermionContext), and the lightweight measurements come from the
factorisation outputs (P_ij, E_f, Tr ρ_hh; hmc.measure_observables).

Every measure_transport_freq sweeps the heavy measurement
(`measure_transport_and_spectra`, src/Observables.jl:314-526) runs on the
device as well (own eigensolver + HIP kernels) and fills transport.csv;
the JLD2 spectra bins become numpy files (no JLD2 writer in this image).
The reference's RNG is global and unseeded; here the caller
passes `rng` (draw order per sweep: randn(ComplexF64, N, 2), then rand()).
"""
from __future__ import annotations

import json
import math
import os
import time
from dataclasses import dataclass, field
from datetime import datetime

import numpy as np

from . import hmc as H
from . import vertices as VX
from .context import spectral_window, transport_grid

OBS_HEADER = ("Sweep,Accepted,dH,Energy,Delta_Amp,Delta_Loc,Delta_Glob,S_Delta,Hole_p,Delta_Diff,"
              "Delta_Pair,Delta_LocalPair")
TRANSPORT_HEADER = "Sweep,Superfluid_Stiffness,DC_Conductivity"


def obs_csv_line(sweep: int, acc: bool, dH: float, obs: H.ObservablesResult) -> str:
    """One observables.csv row, src/Simulation.jl:161-166 formats."""
    return "%d,%d,%.5e,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f\n" % (
        sweep, int(acc), dH, obs.total_energy, obs.Delta_amp, obs.Delta_local, obs.Delta_global,
        obs.S_Delta, obs.hole_conc, obs.Delta_diff, obs.Delta_pair, obs.Delta_localpair)


@dataclass
class AdaptiveNt:
    """Thermalisation step-count controller, src/Simulation.jl:103-129: every
    `window` sweeps, acceptance < 0.60 -> Nt += 2; > 0.95 and Nt > 4 -> Nt -= 1."""
    Nt: int
    window: int = 5
    recent: int = 0

    def record(self, i: int, accepted: bool):
        """Sweep i (1-based) finished.  Returns None between windows, else
        (rate, old_Nt, new_Nt)."""
        if accepted:
            self.recent += 1
        if i % self.window != 0:
            return None
        rate = self.recent / self.window
        self.recent = 0
        old = self.Nt
        if rate < 0.60:
            self.Nt += 2
        elif rate > 0.95 and self.Nt > 4:
            self.Nt -= 1
        return rate, old, self.Nt


@dataclass
class SimulationResult:
    Nt_final: int
    therm_acceptance: float
    meas_acceptance: float
    records: list = field(default_factory=list)   # (sweep, accepted, dH, ObservablesResult)
    transport: list = field(default_factory=list)  # (sweep, SpectrumResult)


def transport_csv_line(sweep: int, spec) -> str:
    """src/Simulation.jl:174-177."""
    return "%d,%.6f,%.6f\n" % (sweep, spec.superfluid_stiffness, spec.dc_conductivity)


def write_spectra_header(spec_dir: str, p) -> None:
    """jldsave(params, omega_grid) of src/Simulation.jl:89."""
    os.makedirs(spec_dir, exist_ok=True)
    params = {k: getattr(p, k) for k in ("Lx", "Ly", "t", "tp", "mu", "W", "n_imp", "beta", "J", "mass",
                                         "eta", "domega", "omega_max")}
    with open(os.path.join(spec_dir, "params.json"), "w") as f:
        json.dump(params, f, indent=1)
    n, _ = transport_grid(p.eta, p.domega, p.omega_max)
    np.save(os.path.join(spec_dir, "omega_grid.npy"), p.eta + p.domega * np.arange(n))


def write_maps_header(spec_dir: str, p, spectral_maps: dict) -> None:
    """maps_omega.npy: the frequencies of the spectral-maps window."""
    os.makedirs(spec_dir, exist_ok=True)
    np.save(os.path.join(spec_dir, "maps_omega.npy"),
            spectral_window(p.eta, p.domega, p.omega_max, **_maps_window(spectral_maps)))


def _maps_window(spectral_maps: dict) -> dict:
    """first / count / stride of a run's `spectral_maps` option."""
    extra = set(spectral_maps) - {"first", "count", "stride"}
    if extra:
        raise ValueError(f"spectral_maps: unknown keys {sorted(extra)}")
    return dict(first=spectral_maps.get("first", 0), count=spectral_maps.get("count"),
                stride=spectral_maps.get("stride", 1))


def _response_opts(current_response: dict) -> dict:
    """direction / q / n_matsubara of a run's `current_response` option."""
    extra = set(current_response) - {"direction", "q", "n_matsubara"}
    if extra:
        raise ValueError(f"current_response: unknown keys {sorted(extra)}")
    q = [(int(mx), int(my)) for mx, my in current_response.get("q", [(0, 1)])]
    return dict(direction=current_response.get("direction", "x"), q=q,
                n_matsubara=int(current_response.get("n_matsubara", 1)))


def response_csv_header(opts: dict) -> str:
    """sweep, dia, then Λ in the ABI order (momentum by momentum, l fastest), the
    columns named by direction, momentum indices and Matsubara index."""
    a = opts["direction"] if isinstance(opts["direction"], str) else "xy"[opts["direction"]]
    cols = [f"lam_{a}{a}(mx={mx};my={my};l={l})" for mx, my in opts["q"] for l in range(opts["n_matsubara"])]
    return ",".join(["sweep", f"dia_{a}"] + cols)


def response_csv_line(sweep: int, dia: float, lam) -> str:
    return ",".join(["%d" % sweep, "%.12e" % dia] + ["%.12e" % v for v in np.asarray(lam).ravel()]) + "\n"


def _operator_opts(operator_response: dict, p) -> dict:
    """ops / n_matsubara / omega / eta of a run's `operator_response` option:
    the vertices built once (vertices.build), the χ'' grid as (start, step,
    count) or None, eta defaulting to the run's."""
    extra = set(operator_response) - {"ops", "n_matsubara", "omega", "eta"}
    if extra:
        raise ValueError(f"operator_response: unknown keys {sorted(extra)}")
    names = [(str(kind), (int(m[0]), int(m[1]))) for kind, m in operator_response.get("ops", [("density", (0, 0))])]
    if not names:
        raise ValueError("operator_response: ops is empty")
    verts = [VX.build(kind, p, mx, my) for kind, (mx, my) in names]
    omega = operator_response.get("omega")
    if omega is not None:
        bad = set(omega) - {"start", "step", "count"}
        if bad or set(omega) != {"start", "step", "count"}:
            raise ValueError("operator_response: omega needs exactly start, step and count")
        omega = (float(omega["start"]), float(omega["step"]), int(omega["count"]))
    nl = int(operator_response.get("n_matsubara", 1))
    if nl < 0 or (nl == 0 and omega is None):
        raise ValueError("operator_response: n_matsubara >= 0, and an omega grid when it is 0")
    return dict(names=names, ops=verts, spin_sign=[v.spin_sign for v in verts], n_matsubara=nl, omega=omega,
                eta=float(operator_response.get("eta", p.eta)))


def operator_csv_header(opts: dict) -> str:
    """sweep, then χ operator by operator, l fastest, named by kind, momentum and l."""
    return ",".join(["sweep"] + [f"chi_{kind}(mx={mx};my={my};l={l})" for kind, (mx, my) in opts["names"]
                                 for l in range(opts["n_matsubara"])])


def operator_csv_line(sweep: int, chi) -> str:
    return ",".join(["%d" % sweep] + ["%.12e" % v for v in np.asarray(chi).ravel()]) + "\n"


class _NambuOpts(dict):
    """a `nambu_response` option after _nambu_opts parsed it"""


def _nambu_opts(nambu_response: dict, p) -> dict:
    """vertices / pairs / n_matsubara / omega / eta of a run's `nambu_response`
    option: the vertices built once (vertices.build_nambu), pairs defaulting to
    every (k, k), the grid as (start, step, count) or None, eta defaulting to
    the run's.  Options parsed before (the drivers hand theirs to their
    TransportQueues) are returned as they are."""
    if isinstance(nambu_response, _NambuOpts):
        return nambu_response
    extra = set(nambu_response) - {"vertices", "pairs", "n_matsubara", "omega", "eta"}
    if extra:
        raise ValueError(f"nambu_response: unknown keys {sorted(extra)}")
    names = [(str(kind), (int(m[0]), int(m[1])))
             for kind, m in nambu_response.get("vertices", [("pair_d_create", (0, 0))])]
    if not names:
        raise ValueError("nambu_response: vertices is empty")
    verts = [VX.build_nambu(kind, p, mx, my) for kind, (mx, my) in names]
    pairs = nambu_response.get("pairs")
    pairs = [(k, k) for k in range(len(names))] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    if not pairs or any(not (0 <= a < len(names) and 0 <= b < len(names)) for a, b in pairs):
        raise ValueError("nambu_response: pairs must be a non-empty list of vertex index pairs")
    omega = nambu_response.get("omega")
    if omega is not None:
        if set(omega) != {"start", "step", "count"}:
            raise ValueError("nambu_response: omega needs exactly start, step and count")
        omega = (float(omega["start"]), float(omega["step"]), int(omega["count"]))
    nl = int(nambu_response.get("n_matsubara", 1))
    if nl < 0 or (nl == 0 and omega is None):
        raise ValueError("nambu_response: n_matsubara >= 0, and an omega grid when it is 0")
    return _NambuOpts(names=names, vertices=verts, pairs=pairs, n_matsubara=nl, omega=omega,
                      eta=float(nambu_response.get("eta", p.eta)))


class _MapOpts(dict):
    """a `response_map` option after _map_opts parsed it"""


def _map_opts(response_map: dict, p) -> dict:
    """vertices / pattern / n_matsubara / omega / eta of a run's `response_map`
    option: the source vertices built once (vertices.build_nambu), the pattern
    from dict(ranges=, blocks=) (vertices.bond_pattern; None: all of it) or an
    (npat, 2) integer array, omega a list of real frequencies or None, eta
    defaulting to the run's.  Options parsed before are returned as they are."""
    if isinstance(response_map, _MapOpts):
        return response_map
    extra = set(response_map) - {"vertices", "pattern", "n_matsubara", "omega", "eta"}
    if extra:
        raise ValueError(f"response_map: unknown keys {sorted(extra)}")
    names = [(str(kind), (int(m[0]), int(m[1])))
             for kind, m in response_map.get("vertices", [("current_x", (0, 0))])]
    if not names:
        raise ValueError("response_map: vertices is empty")
    verts = [VX.build_nambu(kind, p, mx, my) for kind, (mx, my) in names]
    pattern = response_map.get("pattern")
    if pattern is None or isinstance(pattern, dict):
        bad = set(pattern or {}) - {"ranges", "blocks"}
        if bad:
            raise ValueError(f"response_map: unknown pattern keys {sorted(bad)}")
        pattern = VX.bond_pattern(p, **(pattern or {}))
    pattern = np.asarray(pattern)
    if pattern.ndim != 2 or pattern.shape[1] != 2 or len(pattern) < 1 or not np.issubdtype(pattern.dtype, np.integer) \
            or pattern.min() < 0 or pattern.max() >= 2 * p.N:
        raise ValueError("response_map: pattern must be a non-empty (npat, 2) integer array of indices in [0, 2N)")
    omega = response_map.get("omega")
    omega = None if omega is None else [float(w) for w in omega]
    nl = int(response_map.get("n_matsubara", 1))
    if nl < 0 or (nl == 0 and not omega):
        raise ValueError("response_map: n_matsubara >= 0, and a list of frequencies when it is 0")
    return _MapOpts(names=names, vertices=verts, pattern=np.ascontiguousarray(pattern, dtype=np.int64),
                    n_matsubara=nl, omega=omega or None, eta=float(response_map.get("eta", p.eta)))


def write_map_header(spec_dir: str, opts: dict) -> None:
    """response_map_pattern.npy: the (npat, 2) pattern of the response_map option."""
    os.makedirs(spec_dir, exist_ok=True)
    np.save(os.path.join(spec_dir, "response_map_pattern.npy"), opts["pattern"])


def nambu_csv_header(opts: dict) -> str:
    """sweep, then re and im of chi pair by pair, l fastest, named by the pair's
    two vertices (kind and momentum) and l."""
    def nm(k):
        kind, (mx, my) = opts["names"][k]
        return f"{kind}[mx={mx};my={my}]"
    return ",".join(["sweep"] + [f"{part}_chi({nm(a)}|{nm(b)};l={l})" for a, b in opts["pairs"]
                                 for l in range(opts["n_matsubara"]) for part in ("re", "im")])


def nambu_csv_line(sweep: int, chi) -> str:
    c = np.asarray(chi, dtype=np.complex128).ravel()
    return ",".join(["%d" % sweep] + ["%.12e" % v for z in c for v in (z.real, z.imag)]) + "\n"


def write_nambu_header(spec_dir: str, opts: dict) -> None:
    """nambu_chi2_omega.npy: the chi2 grid of the nambu_response option."""
    if opts["omega"] is None:
        return
    os.makedirs(spec_dir, exist_ok=True)
    w0, dw, nw = opts["omega"]
    np.save(os.path.join(spec_dir, "nambu_chi2_omega.npy"), w0 + dw * np.arange(nw))


def write_chi2_header(spec_dir: str, opts: dict) -> None:
    """chi2_omega.npy: the χ'' grid of the operator_response option."""
    if opts["omega"] is None:
        return
    os.makedirs(spec_dir, exist_ok=True)
    w0, dw, nw = opts["omega"]
    np.save(os.path.join(spec_dir, "chi2_omega.npy"), w0 + dw * np.arange(nw))


class SpectraBins:
    """Bin accumulator of src/Simulation.jl:180-220: sums the spectra of
    bin_size measurements, then writes their mean as group sweep_<i>.  With
    spectral maps (add's `maps`: the ldos / akw of that measurement, each
    (count, Ly, Lx)) the group also holds their bin means, summed the same way;
    so it does for chi2 ((nops, n_w)) of the operator_response option, the
    complex nambu_chi2 ((npairs, n_w)) of the nambu_response option and the
    complex response_map ((nops, nz, npat)) and rho_map ((npat,)) of the
    response_map option."""

    def __init__(self):
        self.count = 0
        self.acc = None
        self.maps = None

    def add(self, spec, maps=None) -> int:
        arrs = [spec.optical_conductivity, spec.dos, spec.dos_AN, spec.A_k_omega0]
        if self.count == 0:
            self.acc = [np.array(a, dtype=np.float64, copy=True) for a in arrs]
            # (float64 for every real map, as before; nambu_chi2 is complex and stays so)
            self.maps = None if maps is None else {k: np.array(v, dtype=np.result_type(v, np.float64), copy=True)
                                                   for k, v in maps.items()}
        else:
            for a, b in zip(self.acc, arrs):
                a += b
            if self.maps is not None:
                for k in self.maps:
                    self.maps[k] += maps[k]
        self.count += 1
        return self.count

    def flush(self, spec_dir: str, sweep: int) -> None:
        c = self.count
        oc, dos, dos_an, ak = (a / c for a in self.acc)
        extra = {} if self.maps is None else {k: v / c for k, v in self.maps.items()}
        np.savez(os.path.join(spec_dir, f"sweep_{sweep}.npz"), opt_cond=oc, dos=dos, dos_AN=dos_an,
                 A_k0=ak, count=c, **extra)
        self.count = 0
        self.acc = None
        self.maps = None


class ChainOutput:
    """The files of one run_simulation (src/Simulation.jl:45-56,69-73):
    simulation.log (appended, timestamped tee), observables.csv and
    transport.csv (truncated, headers written), spectra_bins/."""

    def __init__(self, out_dir: str, verbose: bool):
        os.makedirs(out_dir, exist_ok=True)
        self.verbose = verbose
        self.spec_dir = os.path.join(out_dir, "spectra_bins")
        self.f_log = open(os.path.join(out_dir, "simulation.log"), "a")
        self.f_obs = open(os.path.join(out_dir, "observables.csv"), "w")
        self.f_trans = open(os.path.join(out_dir, "transport.csv"), "w")
        self.f_obs.write(OBS_HEADER + "\n")
        self.f_trans.write(TRANSPORT_HEADER + "\n")
        self.bins = SpectraBins()
        self.out_dir = out_dir
        self.f_resp = None           # current_response.csv, only with the current_response option
        self.f_oper = None           # operator_response.csv, only with the operator_response option
        self.f_nambu = None          # nambu_response.csv, only with the nambu_response option

    def tee(self, msg: str):
        line = f"[{datetime.now().strftime('%Y-%m-%d %H:%M:%S')}] {msg}"
        print(line, file=self.f_log, flush=True)
        if self.verbose:
            print(line, flush=True)

    def header(self, p, n_therm, n_measure, measure_transport_freq, bin_size):
        self.tee("Starting Simulation...")
        self.tee(f"System: {p.Lx}x{p.Ly}, β={p.beta}, n_imp={p.n_imp}, J={p.J}")
        self.tee(f"Config: Therm={n_therm}, Sweep={n_measure}, TransFreq={measure_transport_freq}, "
                 f"BinSize={bin_size}")
        self.tee("Initializing State...")

    def observables(self, i, acc, dH, obs):
        self.f_obs.write(obs_csv_line(i, acc, dH, obs))
        self.f_obs.flush()

    def transport(self, i, spec, bin_size, maps=None):
        self.f_trans.write(transport_csv_line(i, spec))
        self.f_trans.flush()
        if self.bins.add(spec, maps) >= bin_size:
            self.bins.flush(self.spec_dir, i)

    def response(self, i, opts, dia, lam):
        """One row of current_response.csv (created, with its header, by the first)."""
        if self.f_resp is None:
            self.f_resp = open(os.path.join(self.out_dir, "current_response.csv"), "w")
            self.f_resp.write(response_csv_header(opts) + "\n")
        self.f_resp.write(response_csv_line(i, dia, lam))
        self.f_resp.flush()

    def operator(self, i, opts, chi):
        """One row of operator_response.csv (created, with its header, by the first)."""
        if opts["n_matsubara"] < 1:
            return
        if self.f_oper is None:
            self.f_oper = open(os.path.join(self.out_dir, "operator_response.csv"), "w")
            self.f_oper.write(operator_csv_header(opts) + "\n")
        self.f_oper.write(operator_csv_line(i, chi))
        self.f_oper.flush()

    def nambu(self, i, opts, chi):
        """One row of nambu_response.csv (created, with its header, by the first)."""
        if opts["n_matsubara"] < 1:
            return
        if self.f_nambu is None:
            self.f_nambu = open(os.path.join(self.out_dir, "nambu_response.csv"), "w")
            self.f_nambu.write(nambu_csv_header(opts) + "\n")
        self.f_nambu.write(nambu_csv_line(i, chi))
        self.f_nambu.flush()

    def close(self):
        self.f_log.close()
        self.f_obs.close()
        self.f_trans.close()
        if self.f_resp is not None:
            self.f_resp.close()
        if self.f_oper is not None:
            self.f_oper.close()
        if self.f_nambu is not None:
            self.f_nambu.close()


def thermalize(cache, p, state, out: ChainOutput, n_therm: int, Nt_therm_init: int, rng):
    """The adaptive thermalisation of src/Simulation.jl:92-130 for one chain;
    returns (final Nt, acceptance rate)."""
    ctl = AdaptiveNt(Nt_therm_init)
    dt = H.calc_optimal_dt(p.beta, p.J, p.mass, ctl.Nt)
    out.tee("--- Thermalization Start ---")
    out.tee(f"Init: Nt={ctl.Nt}, dt={round(dt, 5)}")
    t0 = time.time()
    acc_therm = 0
    for i in range(1, n_therm + 1):
        acc, _ = H.hmc_sweep(cache, p, state, Nt=ctl.Nt, dt=dt, rng=rng)
        acc_therm += int(acc)
        r = ctl.record(i, acc)
        if r is None:
            continue
        rate, old, new = r
        if new != old:
            dt = H.calc_optimal_dt(p.beta, p.J, p.mass, new)
            out.tee("Therm %d/%d. Rate=%.2f. Adjust Nt: %d -> %d, dt: %.4f" % (i, n_therm, rate, old, new, dt))
        elif i % 20 == 0:
            out.tee("Therm %d/%d. Rate=%.2f. Nt=%d (Stable)" % (i, n_therm, rate, new))
    out.tee(f"Thermalization Done. Time: {round(time.time() - t0, 2)}s")
    return ctl.Nt, acc_therm / max(n_therm, 1)


class TransportQueue:
    """Transport measurements (src/Simulation.jl:169-220) of one chain taken at
    the Δ of their sweeps and evaluated `batch` at a time: the eigensolves of
    a batch run as one batched call (dwh_measure_transport_deltas), ~3x the
    throughput of one call per sweep at L = 32.  Rows and bins come out in
    sweep order, each when its batch is measured (batch = 1: right away, as
    the reference writes them).  spectral_maps (first / count / stride, or
    None): every measurement also takes LDOS(i, ω) and A(k, ω) on that
    window (measure_spectral_maps, batched the same way) into the bins.
    current_response (direction / q / n_matsubara, or None): every
    measurement also appends its row (sweep, dia, Λ) to current_response.csv
    (measure_current_response, batched the same way).  operator_response
    (ops / n_matsubara / omega / eta, or None): every measurement also
    appends its row (sweep, χ) to operator_response.csv and puts χ''(ω) into
    the bins as chi2 (measure_operator_response, batched the same way).
    nambu_response (vertices / pairs / n_matsubara / omega / eta, or None):
    every measurement also appends its row (sweep, re and im of chi) to
    nambu_response.csv and puts the complex chi2 into the bins as nambu_chi2
    (measure_nambu_response, batched the same way).  response_map (vertices /
    pattern / n_matsubara / omega / eta, or None): every measurement also puts
    the complex dmap and ρ on the pattern into the bins as response_map and
    rho_map (measure_response_map, batched the same way)."""

    def __init__(self, ctx, p, out: ChainOutput, res: SimulationResult, bin_size: int, batch: int, chain: int = 0,
                 spectral_maps: dict | None = None, current_response: dict | None = None,
                 operator_response: dict | None = None, nambu_response: dict | None = None,
                 response_map: dict | None = None):
        self.ctx, self.p, self.out, self.res = ctx, p, out, res
        self.bin_size, self.batch, self.chain = bin_size, max(1, int(batch)), chain
        self.window = None if spectral_maps is None else _maps_window(spectral_maps)
        self.response = None if current_response is None else _response_opts(current_response)
        self.operator = None if operator_response is None else _operator_opts(operator_response, p)
        self.nambu = None if nambu_response is None else _nambu_opts(nambu_response, p)
        self.rmap = None if response_map is None else _map_opts(response_map, p)
        self.pending = []            # (sweep, Δ snapshot)

    def add(self, sweep: int, Delta):
        self.pending.append((sweep, np.array(Delta, dtype=np.complex128, copy=True)))
        if len(self.pending) >= self.batch:
            self.flush()

    def flush(self):
        if not self.pending:
            return
        p = self.p
        if self.batch == 1:
            specs = [self.ctx.measure_transport(p.eta, p.domega, p.omega_max, chain=self.chain)]
        else:
            specs = self.ctx.measure_transport_deltas(np.stack([d for _, d in self.pending]), p.eta, p.domega,
                                                      p.omega_max, chain=self.chain)
        maps = None
        if self.window is not None:
            deltas = None if self.batch == 1 else np.stack([d for _, d in self.pending])
            maps = self.ctx.measure_spectral_maps(p.eta, p.domega, p.omega_max, chain=self.chain, deltas=deltas,
                                                  **self.window)
        resp = None
        if self.response is not None:
            deltas = None if self.batch == 1 else np.stack([d for _, d in self.pending])
            resp = self.ctx.measure_current_response(chain=self.chain, deltas=deltas, **self.response)
            if deltas is None:
                resp = dict(dia=[resp["dia"]], lam=[resp["lam"]])
        oper = None
        if self.operator is not None:
            deltas = None if self.batch == 1 else np.stack([d for _, d in self.pending])
            oper = measure_operator_option(self.ctx, self.operator, self.chain, deltas)
        nam = None
        if self.nambu is not None:
            deltas = None if self.batch == 1 else np.stack([d for _, d in self.pending])
            nam = measure_nambu_option(self.ctx, self.nambu, self.chain, deltas)
        rmap = None
        if self.rmap is not None:
            deltas = None if self.batch == 1 else np.stack([d for _, d in self.pending])
            rmap = measure_map_option(self.ctx, self.rmap, self.chain, deltas)
        for k, ((i, _), r) in enumerate(zip(self.pending, specs)):
            spec = H.SpectrumResult(**r)
            extra = None if maps is None else {"ldos": maps["ldos"][k], "akw": maps["akw"][k]}
            if oper is not None and self.operator["omega"] is not None:
                extra = dict(extra or {}, chi2=oper["chi2"][k])
            if nam is not None and self.nambu["omega"] is not None:
                extra = dict(extra or {}, nambu_chi2=nam["chi2"][k])
            if rmap is not None:
                extra = dict(extra or {}, response_map=rmap["dmap"][k], rho_map=rmap["rho"][k])
            self.out.transport(i, spec, self.bin_size, extra)
            self.res.transport.append((i, spec))
            if resp is not None:
                self.out.response(i, self.response, float(resp["dia"][k]), resp["lam"][k])
            if oper is not None:
                self.out.operator(i, self.operator, oper["chi"][k])
            if nam is not None:
                self.out.nambu(i, self.nambu, nam["chi"][k])
        self.pending = []


def measure_operator_option(ctx, opts: dict, chain: int, deltas) -> dict:
    """measure_operator_response for the operator_response option: chi
    (nstates, nops, n_matsubara) and chi2 (nstates, nops, n_w), one state at
    the device Δ when deltas is None."""
    r = ctx.measure_operator_response(opts["ops"], opts["spin_sign"], n_matsubara=opts["n_matsubara"],
                                      omega=opts["omega"], eta=opts["eta"], chain=chain, deltas=deltas)
    if deltas is None:
        return dict(chi=r["chi"][None], chi2=r["chi2"][None])
    return r


def measure_nambu_option(ctx, opts: dict, chain: int, deltas) -> dict:
    """measure_nambu_response for the nambu_response option: complex chi
    (nstates, npairs, n_matsubara) and chi2 (nstates, npairs, n_w), one state
    at the device Δ when deltas is None."""
    r = ctx.measure_nambu_response(opts["vertices"], opts["pairs"], n_matsubara=opts["n_matsubara"],
                                   omega=opts["omega"], eta=opts["eta"], chain=chain, deltas=deltas)
    if deltas is None:
        return dict(chi=r["chi"][None], chi2=r["chi2"][None])
    return r


def measure_map_option(ctx, opts: dict, chain: int, deltas) -> dict:
    """measure_response_map for the response_map option: complex dmap
    (nstates, nops, nz, npat) and rho (nstates, npat), one state at the device
    Δ when deltas is None."""
    r = ctx.measure_response_map(opts["vertices"], opts["pattern"], n_matsubara=opts["n_matsubara"],
                                 omega=opts["omega"], eta=opts["eta"], chain=chain, deltas=deltas)
    if deltas is None:
        return dict(dmap=r["dmap"][None], rho=r["rho"][None])
    return r


def run_simulation(p: H.ModelParameters, out_dir: str, *, n_therm: int = 100, n_measure: int = 500,
                   Nt_therm_init: int = 10, Nt_measure: int = 5, measure_transport_freq: int = 1,
                   bin_size: int = 5, verbose: bool = True, rng: np.random.Generator | None = None,
                   device: int = 0, delta_cap: float = 0.0, state: H.SimulationState | None = None,
                   cache: H.ComputeCache | None = None, transport_batch: int = 1,
                   spectral_maps: dict | None = None, current_response: dict | None = None,
                   operator_response: dict | None = None,
                   nambu_response: dict | None = None, response_map: dict | None = None) -> SimulationResult:
    """src/Simulation.jl:34-236.  Files in out_dir: simulation.log (appended),
    observables.csv, transport.csv (one row per transport measurement, every
    measure_transport_freq sweeps; <= 0 disables), and spectra_bins/ — the
    reference's spectra_bins.jld2 (:52,89,206-214) as numpy files: params.json,
    omega_grid.npy, and one sweep_<i>.npz per completed bin of bin_size
    measurements (opt_cond, dos, dos_AN, A_k0 averaged; count).
    transport_batch > 1 evaluates that many measurement sweeps' transport in
    one batched call (TransportQueue): same rows and bins, written up to
    transport_batch - 1 sweeps later.
    spectral_maps = dict(first=, count=, stride=) (each optional; a window of
    the DOS grid, FermionContext.measure_spectral_maps): every transport
    measurement also takes LDOS(i, ω) and A(k, ω) there; each sweep_<i>.npz
    gains their bin means ldos and akw ((count, Ly, Lx)) and
    spectra_bins/maps_omega.npy holds the window's frequencies.  None (the
    default): no maps, the files as without the option.
    current_response = dict(direction=, q=, n_matsubara=) (each optional;
    FermionContext.measure_current_response): every transport measurement
    also appends one row (sweep, dia, then Λ(q, iΩ_l) momentum by momentum, l
    fastest) to current_response.csv, whose header names the momenta.  None
    (the default): no such file, everything else as without the option.
    operator_response = dict(ops=[(kind, (mx, my)), ...], n_matsubara=,
    omega=dict(start=, step=, count=), eta=) (each optional; kind a key of
    vertices.KINDS; FermionContext.measure_operator_response): every transport
    measurement also appends one row (sweep, then χ(iΩ_l) operator by
    operator, l fastest) to operator_response.csv, whose header names kind,
    momentum and l, and with an omega grid each sweep_<i>.npz gains the bin
    mean chi2 ((nops, count)) with the grid in spectra_bins/chi2_omega.npy
    (eta defaults to the run's).  None (the default): no such files,
    everything else as without the option.
    nambu_response = dict(vertices=[(kind, (mx, my)), ...], pairs=[(a, b), ...],
    n_matsubara=, omega=dict(start=, step=, count=), eta=) (each optional; kind
    a key of vertices.NAMBU_KINDS, pairs indices into vertices, default every
    (k, k); FermionContext.measure_nambu_response): every transport
    measurement also appends one row (sweep, then re and im of chi pair by
    pair, l fastest) to nambu_response.csv, whose header names each pair's
    vertices and l, and with an omega grid each sweep_<i>.npz gains the complex
    bin mean nambu_chi2 ((npairs, count)) with the grid in
    spectra_bins/nambu_chi2_omega.npy.  None (the default): no such files,
    everything else as without the option.
    response_map = dict(vertices=[(kind, (mx, my)), ...], pattern=dict(ranges=,
    blocks=) or an (npat, 2) array, n_matsubara=, omega=[ω, ...], eta=) (each
    optional; kind a key of vertices.NAMBU_KINDS, default the q = 0 x current
    on the whole vertices.bond_pattern; FermionContext.measure_response_map):
    every transport measurement also takes the linear-response density matrix
    of each source vertex and ρ on the pattern; each sweep_<i>.npz gains their
    complex bin means response_map ((nops, nz, npat)) and rho_map ((npat,)),
    and spectra_bins/response_map_pattern.npy holds the pattern.  None (the
    default): no such files, everything else as without the option."""
    rng = rng if rng is not None else np.random.default_rng()
    if current_response is not None:
        _response_opts(current_response)
    oper_opts = None if operator_response is None else _operator_opts(operator_response, p)
    nambu_opts = None if nambu_response is None else _nambu_opts(nambu_response, p)
    map_opts = None if response_map is None else _map_opts(response_map, p)
    out = ChainOutput(out_dir, verbose)
    try:
        out.header(p, n_therm, n_measure, measure_transport_freq, bin_size)
        if state is None:
            state = H.initialize_state(p, rng)
        if cache is None:
            cache = H.initialize_cache(p, device=device, delta_cap=delta_cap)
        H.init_static_H(cache, p, state)
        H.update_H_BdG(cache, p, state)
        H.diagonalize_H_BdG(cache, p)
        if measure_transport_freq > 0:
            write_spectra_header(out.spec_dir, p)
            if spectral_maps is not None:
                write_maps_header(out.spec_dir, p, spectral_maps)
            if oper_opts is not None:
                write_chi2_header(out.spec_dir, oper_opts)
            if nambu_opts is not None:
                write_nambu_header(out.spec_dir, nambu_opts)
            if map_opts is not None:
                write_map_header(out.spec_dir, map_opts)
        Nt_fin, acc_th = thermalize(cache, p, state, out, n_therm, Nt_therm_init, rng)

        dt_meas = H.calc_optimal_dt(p.beta, p.J, p.mass, Nt_measure)
        out.tee("--- Measurement Start ---")
        out.tee(f"Settings: Nt={Nt_measure}, dt={round(dt_meas, 5)}")
        t1 = time.time()
        acc_total = 0
        res = SimulationResult(Nt_fin, acc_th, 0.0)
        tq = TransportQueue(cache.require(), p, out, res, bin_size, transport_batch, spectral_maps=spectral_maps,
                            current_response=current_response, operator_response=operator_response,
                            nambu_response=nambu_opts, response_map=map_opts)
        for i in range(1, n_measure + 1):
            acc, dH = H.hmc_sweep(cache, p, state, Nt=Nt_measure, dt=dt_meas, rng=rng)
            acc_total += int(acc)
            obs = H.measure_observables(cache, p, state)
            out.observables(i, acc, dH, obs)
            res.records.append((i, acc, dH, obs))
            if measure_transport_freq > 0 and i % measure_transport_freq == 0:
                tq.add(i, state.Delta)
            if i % 10 == 0:
                out.tee("Meas %d/%d. Acc=%.2f. E=%.4f" % (i, n_measure, acc_total / i, obs.total_energy))
        tq.flush()
        res.meas_acceptance = acc_total / max(n_measure, 1)
        out.tee(f"Measurement Done. Total Time: {round(time.time() - t1, 2)}s")
        return res
    finally:
        out.close()


def run_simulation_chains(p: H.ModelParameters, out_dirs, rngs, *, n_therm: int = 100, n_measure: int = 500,
                          Nt_therm_init: int = 10, Nt_measure: int = 5, measure_transport_freq: int = 1,
                          bin_size: int = 5, verbose: bool = False, device: int = 0,
                          delta_cap: float = 0.0, transport_batch: int = 1,
                          spectral_maps: dict | None = None, current_response: dict | None = None,
                          operator_response: dict | None = None,
                          nambu_response: dict | None = None, response_map: dict | None = None) -> list:
    """len(out_dirs) independent run_simulation's (src/Simulation.jl:34-236),
    chain k writing out_dirs[k] and drawing from rngs[k] in the reference's
    order (initialize_state, then per sweep randn(ComplexF64) and rand() only
    when ΔH >= 0).  Each chain is thermalised on its own single-chain context
    (its own adaptive Nt, :92-130); the measurement phase, whose Nt_measure is
    common to all chains (:133-228), runs every chain in one batched context
    (one factorisation launch sequence per leapfrog step for all chains, and
    one batched eigensolve per transport measurement,
    dwh_measure_transport_batched; with transport_batch > 1, per chain
    transport_batch sweeps at once, TransportQueue).  Returns one
    SimulationResult per chain; each chain runs the same Markov chain as
    run_simulation up to the pole approximation (bit-equal on the oracle
    backend: on the device the batched context selects one pole set for the
    largest spectral bound over the chains, and a guard trip re-selects it
    for every chain, so dH differs at ~1e-12 and a Metropolis decision can
    differ).  spectral_maps, current_response, operator_response,
    nambu_response, response_map: as run_simulation's, for every chain."""
    K = len(out_dirs)
    window = None if spectral_maps is None else _maps_window(spectral_maps)
    response = None if current_response is None else _response_opts(current_response)
    oper_opts = None if operator_response is None else _operator_opts(operator_response, p)
    nambu_opts = None if nambu_response is None else _nambu_opts(nambu_response, p)
    map_opts = None if response_map is None else _map_opts(response_map, p)
    if len(rngs) != K or K < 1:
        raise ValueError("one rng per output directory")
    outs = [ChainOutput(d, verbose) for d in out_dirs]
    try:
        states, results = [], []
        for k in range(K):
            outs[k].header(p, n_therm, n_measure, measure_transport_freq, bin_size)
            st = H.initialize_state(p, rngs[k])
            cache = H.initialize_cache(p, device=device, delta_cap=delta_cap)
            H.init_static_H(cache, p, st)
            H.update_H_BdG(cache, p, st)
            H.diagonalize_H_BdG(cache, p)
            if measure_transport_freq > 0:
                write_spectra_header(outs[k].spec_dir, p)
                if spectral_maps is not None:
                    write_maps_header(outs[k].spec_dir, p, spectral_maps)
                if oper_opts is not None:
                    write_chi2_header(outs[k].spec_dir, oper_opts)
                if nambu_opts is not None:
                    write_nambu_header(outs[k].spec_dir, nambu_opts)
                if map_opts is not None:
                    write_map_header(outs[k].spec_dir, map_opts)
            Nt_fin, acc_th = thermalize(cache, p, st, outs[k], n_therm, Nt_therm_init, rngs[k])
            cache.ctx.close()
            states.append(st)
            results.append(SimulationResult(Nt_fin, acc_th, 0.0))

        dis = np.stack([st.disorder_pot for st in states])
        ctx = H.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis,
                             delta_cap=delta_cap, device=device)
        try:
            ctx.set_pairing(np.stack([st.Delta for st in states]))
            ctx.factorize()
            dt_meas = H.calc_optimal_dt(p.beta, p.J, p.mass, Nt_measure)
            for o in outs:
                o.tee("--- Measurement Start ---")
                o.tee(f"Settings: Nt={Nt_measure}, dt={round(dt_meas, 5)}")
            t1 = time.time()
            acc_total = np.zeros(K, dtype=np.int64)
            tqs = [TransportQueue(ctx, p, outs[k], results[k], bin_size, transport_batch, chain=k,
                                  spectral_maps=spectral_maps, current_response=current_response,
                                  operator_response=operator_response, nambu_response=nambu_opts,
                                  response_map=map_opts)
                   for k in range(K)] if transport_batch > 1 else None
            for i in range(1, n_measure + 1):
                noise = np.stack([H.standard_complex_normal(r, (p.N, 2)) for r in rngs])
                dH = ctx.hmc_trajectory(noise, Nt_measure, dt_meas, p.mass)
                acc = np.array([bool(dH[k] < 0 or rngs[k].random() < math.exp(-dH[k])) for k in range(K)])
                ctx.hmc_finish(acc)
                acc_total += acc
                D, _ = ctx.get_state()
                P, Ef, tr = ctx.pairing(), ctx.fermion_energy(), ctx.hole_trace()
                specs = None
                if measure_transport_freq > 0 and i % measure_transport_freq == 0:
                    if tqs is None:
                        specs = ctx.measure_transport_all(p.eta, p.domega, p.omega_max)
                    else:
                        for k in range(K):
                            tqs[k].add(i, D[k])
                for k in range(K):
                    obs = H.observables_from_outputs(p, D[k], P[k], Ef[k], tr[k])
                    outs[k].observables(i, acc[k], float(dH[k]), obs)
                    results[k].records.append((i, bool(acc[k]), float(dH[k]), obs))
                    if specs is not None:
                        spec = H.SpectrumResult(**specs[k])
                        maps = None
                        if window is not None:
                            m = ctx.measure_spectral_maps(p.eta, p.domega, p.omega_max, chain=k, **window)
                            maps = {"ldos": m["ldos"][0], "akw": m["akw"][0]}
                        oper = None if oper_opts is None else measure_operator_option(ctx, oper_opts, k, None)
                        if oper is not None and oper_opts["omega"] is not None:
                            maps = dict(maps or {}, chi2=oper["chi2"][0])
                        nam = None if nambu_opts is None else measure_nambu_option(ctx, nambu_opts, k, None)
                        if nam is not None and nambu_opts["omega"] is not None:
                            maps = dict(maps or {}, nambu_chi2=nam["chi2"][0])
                        if map_opts is not None:
                            rm = measure_map_option(ctx, map_opts, k, None)
                            maps = dict(maps or {}, response_map=rm["dmap"][0], rho_map=rm["rho"][0])
                        outs[k].transport(i, spec, bin_size, maps)
                        results[k].transport.append((i, spec))
                        if response is not None:
                            r = ctx.measure_current_response(chain=k, **response)
                            outs[k].response(i, response, r["dia"], r["lam"])
                        if oper is not None:
                            outs[k].operator(i, oper_opts, oper["chi"][0])
                        if nam is not None:
                            outs[k].nambu(i, nambu_opts, nam["chi"][0])
                    if i % 10 == 0:
                        outs[k].tee("Meas %d/%d. Acc=%.2f. E=%.4f" % (i, n_measure, acc_total[k] / i,
                                                                     obs.total_energy))
            for tq in tqs or []:
                tq.flush()
            for k in range(K):
                results[k].meas_acceptance = acc_total[k] / max(n_measure, 1)
                outs[k].tee(f"Measurement Done. Total Time: {round(time.time() - t1, 2)}s")
        finally:
            ctx.close()
        return results
    finally:
        for o in outs:
            o.close()
