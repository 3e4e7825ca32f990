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
from .context import integrator_schedule, spectral_window, transport_grid

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
    `window` sweeps, acceptance < 0.60 -> Nt += 2; > 0.95 and Nt > Nt_min ->
    Nt -= 1 (Nt_min = 4 is the reference's; an integrator that conserves
    energy with fewer steps lowers it, Integrator)."""
    Nt: int
    window: int = 5
    recent: int = 0
    Nt_min: int = 4

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
        elif rate > 0.95 and self.Nt > self.Nt_min:
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


class _Option:
    """One measurement option of the drivers: what run_simulation,
    run_simulation_chains and TransportQueue need to know about one of their
    keywords, parsed once from the user's dict (ValueError for what it
    refuses).  Every option is a dict whose entries are each optional, or None
    (the default): not taken, every file as without it.  With it, every
    transport measurement also makes the option's one FermionContext call, at
    the device Δ or batched over a TransportQueue's Δ snapshots.

    keyword    the drivers' keyword
    keys       the entries the dict may hold
    header     None, or (file name, array): the file written under
               spectra_bins/ before the run (write_headers)
    csv_file   None, or the CSV file that gets one row per measurement:
               sweep, then csv_values as %.12e under csv_columns
    measure    the FermionContext call; every result with the leading state
               axis, one state at the device Δ when deltas is None
    bins       the entries of state k for sweep_<i>.npz (their bin means are
               written, SpectraBins)"""
    keyword, keys, header, csv_file = None, (), None, None
    squeezed = ()        # result entries that FermionContext returns without the state axis at deltas=None

    def __init__(self, raw: dict, p):
        extra = set(raw) - set(self.keys)
        if extra:
            raise ValueError(f"{self.keyword}: unknown keys {sorted(extra)}")

    def _vertex_names(self, raw: dict, key: str, default) -> list:
        names = [(str(kind), (int(m[0]), int(m[1]))) for kind, m in raw.get(key, [default])]
        if not names:
            raise ValueError(f"{self.keyword}: {key} is empty")
        return names

    def _frequencies(self, raw: dict, p, omega, what: str):
        """n_matsubara, omega (None when empty) and eta (default: the run's)"""
        nl = int(raw.get("n_matsubara", 1))
        if nl < 0 or (nl == 0 and not omega):
            raise ValueError(f"{self.keyword}: n_matsubara >= 0, and {what} when it is 0")
        self.n_matsubara, self.omega, self.eta = nl, omega or None, float(raw.get("eta", p.eta))

    def measure(self, ctx, p, chain: int, deltas) -> dict:
        r = self._call(ctx, p, chain, deltas)
        if deltas is None:
            r = dict(r, **{k: np.asarray(r[k])[None] for k in self.squeezed})
        return r

    def bins(self, r: dict, k: int) -> dict:
        return {}


class SpectralMaps(_Option):
    """spectral_maps = dict(first=, count=, stride=): LDOS(i, ω) and A(k, ω)
    on the window first + q·stride, q < count, of the DOS grid (count None: to
    its end; FermionContext.measure_spectral_maps).  Each sweep_<i>.npz gains
    the bin means ldos and akw ((count, Ly, Lx));
    spectra_bins/maps_omega.npy holds the window's frequencies."""
    keyword, keys = "spectral_maps", ("first", "count", "stride")

    def __init__(self, raw, p):
        super().__init__(raw, p)
        self.window = dict(first=raw.get("first", 0), count=raw.get("count"), stride=raw.get("stride", 1))
        self.header = ("maps_omega.npy", spectral_window(p.eta, p.domega, p.omega_max, **self.window))

    def _call(self, ctx, p, chain, deltas):
        return ctx.measure_spectral_maps(p.eta, p.domega, p.omega_max, chain=chain, deltas=deltas, **self.window)

    def bins(self, r, k):
        return {"ldos": r["ldos"][k], "akw": r["akw"][k]}


class CurrentResponse(_Option):
    """current_response = dict(direction=, q=[(mx, my), ...], n_matsubara=)
    (defaults "x", [(0, 1)], 1; FermionContext.measure_current_response):
    current_response.csv gets sweep, dia, then Λ(q, iΩ_l) in the ABI order
    (momentum by momentum, l fastest), the columns named by direction,
    momentum indices and Matsubara index."""
    keyword, keys = "current_response", ("direction", "q", "n_matsubara")
    csv_file, squeezed = "current_response.csv", ("dia", "lam")

    def __init__(self, raw, p):
        super().__init__(raw, p)
        self.args = dict(direction=raw.get("direction", "x"),
                         q=[(int(mx), int(my)) for mx, my in raw.get("q", [(0, 1)])],
                         n_matsubara=int(raw.get("n_matsubara", 1)))

    def _call(self, ctx, p, chain, deltas):
        return ctx.measure_current_response(chain=chain, deltas=deltas, **self.args)

    def csv_columns(self):
        a = self.args["direction"] if isinstance(self.args["direction"], str) else "xy"[self.args["direction"]]
        return [f"dia_{a}"] + [f"lam_{a}{a}(mx={mx};my={my};l={l})" for mx, my in self.args["q"]
                               for l in range(self.args["n_matsubara"])]

    def csv_values(self, r, k):
        return [r["dia"][k], *np.asarray(r["lam"][k]).ravel()]


class _GridResponse(_Option):
    """What operator_response and nambu_response share: n_matsubara (default
    1; 0 with an omega grid skips the CSV file), omega = dict(start=, step=,
    count=) (default None: no chi2) and eta (default the run's).  With a grid
    each sweep_<i>.npz gains the bin mean of chi2 under bins_key and
    spectra_bins/<grid_file> holds the grid."""
    squeezed = ("chi", "chi2")
    grid_file = bins_key = None

    def _grid_frequencies(self, raw, p):
        omega = raw.get("omega")
        if omega is not None:
            if set(omega) != {"start", "step", "count"}:
                raise ValueError(f"{self.keyword}: omega needs exactly start, step and count")
            omega = (float(omega["start"]), float(omega["step"]), int(omega["count"]))
        self._frequencies(raw, p, omega, "an omega grid")
        if omega is not None:
            self.header = (self.grid_file, omega[0] + omega[1] * np.arange(omega[2]))
        if self.n_matsubara >= 1:
            self.csv_file = self.keyword + ".csv"

    def bins(self, r, k):
        return {} if self.omega is None else {self.bins_key: r["chi2"][k]}

    def csv_values(self, r, k):
        return np.ascontiguousarray(r["chi"][k]).ravel().view(np.float64)     # (complex: re, im)


class OperatorResponse(_GridResponse):
    """operator_response = dict(ops=[(kind, (mx, my)), ...], n_matsubara=,
    omega=, eta=) (kind a key of vertices.KINDS, default the q = 0 density;
    the vertices are built once, vertices.build;
    FermionContext.measure_operator_response): operator_response.csv gets
    sweep, then χ(iΩ_l) operator by operator, l fastest, named by kind,
    momentum and l; χ''(ω) goes to the bins as chi2 ((nops, count)), its grid
    to chi2_omega.npy."""
    keyword, keys = "operator_response", ("ops", "n_matsubara", "omega", "eta")
    grid_file, bins_key = "chi2_omega.npy", "chi2"

    def __init__(self, raw, p):
        super().__init__(raw, p)
        self.names = self._vertex_names(raw, "ops", ("density", (0, 0)))
        self.ops = [VX.build(kind, p, mx, my) for kind, (mx, my) in self.names]
        self.spin_sign = [v.spin_sign for v in self.ops]
        self._grid_frequencies(raw, p)

    def _call(self, ctx, p, chain, deltas):
        return ctx.measure_operator_response(self.ops, self.spin_sign, n_matsubara=self.n_matsubara,
                                             omega=self.omega, eta=self.eta, chain=chain, deltas=deltas)

    def csv_columns(self):
        return [f"chi_{kind}(mx={mx};my={my};l={l})" for kind, (mx, my) in self.names
                for l in range(self.n_matsubara)]


class NambuResponse(_GridResponse):
    """nambu_response = dict(vertices=[(kind, (mx, my)), ...], pairs=[(a, b),
    ...], n_matsubara=, omega=, eta=) (kind a key of vertices.NAMBU_KINDS,
    default the q = 0 pair_d_create, built once by vertices.build_nambu; pairs
    indices into vertices, default every (k, k);
    FermionContext.measure_nambu_response): nambu_response.csv gets sweep,
    then re and im of chi pair by pair, l fastest, named by the pair's two
    vertices (kind and momentum) and l; the complex chi2 goes to the bins as
    nambu_chi2 ((npairs, count)), its grid to nambu_chi2_omega.npy."""
    keyword, keys = "nambu_response", ("vertices", "pairs", "n_matsubara", "omega", "eta")
    grid_file, bins_key = "nambu_chi2_omega.npy", "nambu_chi2"

    def __init__(self, raw, p):
        super().__init__(raw, p)
        self.names = self._vertex_names(raw, "vertices", ("pair_d_create", (0, 0)))
        self.vertices = [VX.build_nambu(kind, p, mx, my) for kind, (mx, my) in self.names]
        n, pairs = len(self.names), raw.get("pairs")
        self.pairs = [(k, k) for k in range(n)] if pairs is None else [(int(a), int(b)) for a, b in pairs]
        if not self.pairs or any(not (0 <= a < n and 0 <= b < n) for a, b in self.pairs):
            raise ValueError("nambu_response: pairs must be a non-empty list of vertex index pairs")
        self._grid_frequencies(raw, p)

    def _call(self, ctx, p, chain, deltas):
        return ctx.measure_nambu_response(self.vertices, self.pairs, n_matsubara=self.n_matsubara,
                                          omega=self.omega, eta=self.eta, chain=chain, deltas=deltas)

    def csv_columns(self):
        def nm(k):
            kind, (mx, my) = self.names[k]
            return f"{kind}[mx={mx};my={my}]"
        return [f"{part}_chi({nm(a)}|{nm(b)};l={l})" for a, b in self.pairs
                for l in range(self.n_matsubara) for part in ("re", "im")]


class ResponseMap(_Option):
    """response_map = dict(vertices=[(kind, (mx, my)), ...], pattern=,
    n_matsubara=, omega=[ω, ...], eta=) (kind a key of vertices.NAMBU_KINDS,
    default the q = 0 current_x; pattern dict(ranges=, blocks=) for
    vertices.bond_pattern, default all of it, or an (npat, 2) integer array;
    omega a list of real frequencies, default None; eta default the run's;
    FermionContext.measure_response_map): the linear-response density matrix
    of each source vertex and ρ on the pattern.  Each sweep_<i>.npz gains
    their complex bin means response_map ((nops, nz, npat)) and rho_map
    ((npat,)); spectra_bins/response_map_pattern.npy holds the pattern."""
    keyword, keys = "response_map", ("vertices", "pattern", "n_matsubara", "omega", "eta")
    squeezed = ("dmap", "rho")

    def __init__(self, raw, p):
        super().__init__(raw, p)
        self.names = self._vertex_names(raw, "vertices", ("current_x", (0, 0)))
        self.vertices = [VX.build_nambu(kind, p, mx, my) for kind, (mx, my) in self.names]
        pattern = raw.get("pattern")
        if pattern is None or isinstance(pattern, dict):
            bad = set(pattern or {}) - {"ranges", "blocks"}
            if bad:
                raise ValueError(f"response_map: unknown pattern keys {sorted(bad)}")
            pattern = VX.bond_pattern(p, **(pattern or {}))
        pattern = np.asarray(pattern)
        if pattern.ndim != 2 or pattern.shape[1] != 2 or len(pattern) < 1 \
                or not np.issubdtype(pattern.dtype, np.integer) or pattern.min() < 0 or pattern.max() >= 2 * p.N:
            raise ValueError("response_map: pattern must be a non-empty (npat, 2) integer array of indices in [0, 2N)")
        self.pattern = np.ascontiguousarray(pattern, dtype=np.int64)
        self.header = ("response_map_pattern.npy", self.pattern)
        omega = raw.get("omega")
        self._frequencies(raw, p, None if omega is None else [float(w) for w in omega], "a list of frequencies")

    def _call(self, ctx, p, chain, deltas):
        return ctx.measure_response_map(self.vertices, self.pattern, n_matsubara=self.n_matsubara,
                                        omega=self.omega, eta=self.eta, chain=chain, deltas=deltas)

    def bins(self, r, k):
        return {"response_map": r["dmap"][k], "rho_map": r["rho"][k]}


class Correlations(_Option):
    """correlations = dict(families=[kind, ...], pairs=[(a, b), ...],
    ref_sites=[site, ...]) (kind a key of vertices.LOCAL_KINDS, default
    pair_d_create, built once by vertices.local_family; pairs indices into
    families, default every (k, k); ref_sites default None: no local output;
    FermionContext.measure_correlations): the equal-time correlations of local
    operators.  Each sweep_<i>.npz gains the complex bin means corr ((npairs,
    Ly, Lx), connected and translation-averaged), corr_mean ((nfam, Ly, Lx),
    from whose bin mean the disconnected part of the *bin-averaged* means
    follows; the disconnected part of each sweep needs the per-sweep means)
    and, with ref_sites, corr_local ((npairs, nref, Ly, Lx));
    spectra_bins/correlations_pairs.npy holds the pairs."""
    keyword, keys = "correlations", ("families", "pairs", "ref_sites")

    def __init__(self, raw, p):
        super().__init__(raw, p)
        self.names = [str(k) for k in raw.get("families", ["pair_d_create"])]
        if not self.names:
            raise ValueError("correlations: families is empty")
        self.families = [VX.local_family(k, p) for k in self.names]
        n, pairs = len(self.names), raw.get("pairs")
        self.pairs = [(k, k) for k in range(n)] if pairs is None else [(int(a), int(b)) for a, b in pairs]
        if not self.pairs or any(not (0 <= a < n and 0 <= b < n) for a, b in self.pairs):
            raise ValueError("correlations: pairs must be a non-empty list of family index pairs")
        ref = raw.get("ref_sites")
        self.ref_sites = None if ref is None else [int(q) for q in ref]
        if self.ref_sites is not None and (not self.ref_sites or any(not 0 <= q < p.N for q in self.ref_sites)):
            raise ValueError("correlations: ref_sites must be a non-empty list of sites in [0, N)")
        self.squeezed = ("corr", "mean") + (("local",) if self.ref_sites is not None else ())
        self.header = ("correlations_pairs.npy", np.asarray(self.pairs, dtype=np.int64).reshape(-1, 2))

    def _call(self, ctx, p, chain, deltas):
        return ctx.measure_correlations(self.families, pairs=self.pairs, ref_sites=self.ref_sites, chain=chain,
                                        deltas=deltas)

    def bins(self, r, k):
        out = {"corr": r["corr"][k], "corr_mean": r["mean"][k]}
        if self.ref_sites is not None:
            out["corr_local"] = r["local"][k]
        return out


# The drivers' measurement options, in the order of their results in the bins.  A further one is a
# description here and its keyword in the drivers' and TransportQueue's signatures.
OPTIONS = (SpectralMaps, CurrentResponse, OperatorResponse, NambuResponse, ResponseMap)
# The equal-time measurements, taken after OPTIONS.  A tuple of its own only because
# tests/test_measurement_options.py pins OPTIONS to its five keywords: merging the two waits for that test.
EQUAL_TIME_OPTIONS = (Correlations,)


def parse_options(p, **raw) -> list:
    """The options taken (not None) among the drivers' keywords, parsed, in the
    order of OPTIONS, then of EQUAL_TIME_OPTIONS."""
    return [o(raw[o.keyword], p) for o in OPTIONS + EQUAL_TIME_OPTIONS if raw.get(o.keyword) is not None]


class Integrator:
    """integrator = a name ("leapfrog", "omelyan2") or dict(kind=, lam=, kick=,
    drift=, Nt_min=): the splitting of every trajectory of the run
    (FermionContext.set_integrator's keywords; kind default "omelyan2") and the
    lower bound of the adaptive thermalisation's Nt (default 4, the
    reference's; >= 1).  Nt_therm_init and Nt_measure stay numbers of steps, so
    a trajectory makes stages·Nt factorisations.  The schedule is checked by
    the library's own rule (integrator_schedule, no device) when parsed;
    simulation.log records it and the factorisations per trajectory.  None,
    the drivers' default: no call, no log line, every file as without it."""
    keys = ("kind", "lam", "kick", "drift", "Nt_min")

    def __init__(self, raw):
        raw = dict(kind=raw) if isinstance(raw, str) else dict(raw)
        extra = set(raw) - set(self.keys)
        if extra:
            raise ValueError(f"integrator: unknown keys {sorted(extra)}")
        self.Nt_min = int(raw.pop("Nt_min", 4))
        if self.Nt_min < 1:
            raise ValueError("integrator: Nt_min >= 1")
        self.args = {k: v for k, v in raw.items() if v is not None}
        self.args.setdefault("kind", "omelyan2")
        kicks, _ = integrator_schedule(Nt=1, dt=1.0, mass=1.0, **self.args)
        self.stages = len(kicks) - 1

    def apply(self, ctx, out) -> None:
        """onto a context, with the log line of what the context then holds"""
        ctx.set_integrator(**self.args)
        g = ctx.integrator
        lam = f" lam={g['lam']!r}" if g["kind"] == "omelyan2" else ""
        out.tee(f"Integrator: {g['kind']}{lam}, {self.stages} factorisations per step, "
                f"kick={[float(a) for a in g['kick']]}, drift={[float(b) for b in g['drift']]}, Nt_min={self.Nt_min}")


def parse_integrator(integrator):
    return None if integrator is None else Integrator(integrator)


def write_headers(spec_dir: str, p, options=()) -> None:
    """jldsave(params, omega_grid) of src/Simulation.jl:89 as params.json and
    omega_grid.npy, and the options' header files."""
    os.makedirs(spec_dir, exist_ok=True)
    params = {k: getattr(p, k) for k in ("Lx", "Ly", "t", "tp", "mu", "W", "n_imp", "beta", "J", "mass",
                                         "eta", "domega", "omega_max")}
    with open(os.path.join(spec_dir, "params.json"), "w") as f:
        json.dump(params, f, indent=1)
    n, _ = transport_grid(p.eta, p.domega, p.omega_max)
    np.save(os.path.join(spec_dir, "omega_grid.npy"), p.eta + p.domega * np.arange(n))
    for o in options:
        if o.header is not None:
            np.save(os.path.join(spec_dir, o.header[0]), o.header[1])


class SpectraBins:
    """Bin accumulator of src/Simulation.jl:180-220: sums the spectra of
    bin_size measurements, then writes their mean as group sweep_<i>.  With
    spectral maps (add's `maps`: the ldos / akw of that measurement, each
    (count, Ly, Lx)) the group also holds their bin means, summed the same way;
    so it does for chi2 ((nops, n_w)) of the operator_response option, the
    complex nambu_chi2 ((npairs, n_w)) of the nambu_response option and the
    complex response_map ((nops, nz, npat)) and rho_map ((npat,)) of the
    response_map option, and corr, corr_mean and corr_local of the
    correlations option."""

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
        self.csv = {}                # the options' CSV files by name, each opened by its first row

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

    def option_row(self, i, option, values):
        """One row of the option's CSV file (created, with its header, by the first)."""
        f = self.csv.get(option.csv_file)
        if f is None:
            f = self.csv[option.csv_file] = open(os.path.join(self.out_dir, option.csv_file), "w")
            f.write(",".join(["sweep"] + option.csv_columns()) + "\n")
        f.write(",".join(["%d" % i] + ["%.12e" % v for v in values]) + "\n")
        f.flush()

    def close(self):
        for f in (self.f_log, self.f_obs, self.f_trans, *self.csv.values()):
            f.close()


def thermalize(cache, p, state, out: ChainOutput, n_therm: int, Nt_therm_init: int, rng, Nt_min: int = 4):
    """The adaptive thermalisation of src/Simulation.jl:92-130 for one chain;
    returns (final Nt, acceptance rate)."""
    ctl = AdaptiveNt(Nt_therm_init, Nt_min=Nt_min)
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


def record_transport(out: ChainOutput, res: SimulationResult, bin_size: int, i: int, spec, options, results,
                     k: int) -> None:
    """The transport measurement of sweep i into the files and res: spec's
    row of transport.csv and its spectra into the bins, with them state k of
    the options' results (Option.measure's, in the order of options) into the
    bins and the options' CSV files."""
    extra = {}
    for o, r in zip(options, results):
        extra.update(o.bins(r, k))
    out.transport(i, spec, bin_size, extra or None)
    res.transport.append((i, spec))
    for o, r in zip(options, results):
        if o.csv_file is not None:
            out.option_row(i, o, o.csv_values(r, k))


class TransportQueue:
    """Transport measurements (src/Simulation.jl:169-220) of one chain taken at
    the Δ of their sweeps and evaluated `batch` at a time: the eigensolves of
    a batch run as one batched call (dwh_measure_transport_deltas), ~3x the
    throughput of one call per sweep at L = 32.  Rows and bins come out in
    sweep order, each when its batch is measured (batch = 1: right away, as
    the reference writes them).  The measurement options (OPTIONS and
    EQUAL_TIME_OPTIONS; each
    keyword a dict or None) are measured with every batch, each by one call
    batched the same way."""

    def __init__(self, ctx, p, out: ChainOutput, res: SimulationResult, bin_size: int, batch: int, chain: int = 0,
                 spectral_maps: dict | None = None, current_response: dict | None = None,
                 operator_response: dict | None = None, nambu_response: dict | None = None,
                 response_map: dict | None = None, correlations: dict | None = None):
        self._init(ctx, p, out, res, bin_size, batch, chain,
                   parse_options(p, spectral_maps=spectral_maps, current_response=current_response,
                                 operator_response=operator_response, nambu_response=nambu_response,
                                 response_map=response_map, correlations=correlations))

    @classmethod
    def with_options(cls, options, ctx, p, out: ChainOutput, res: SimulationResult, bin_size: int, batch: int,
                     chain: int = 0):
        """A queue for options parsed before (parse_options), as the drivers, which parse once, make theirs."""
        tq = cls.__new__(cls)
        tq._init(ctx, p, out, res, bin_size, batch, chain, options)
        return tq

    def _init(self, ctx, p, out, res, bin_size, batch, chain, options):
        """all of a queue's state, for both ways of making one"""
        self.ctx, self.p, self.out, self.res = ctx, p, out, res
        self.bin_size, self.batch, self.chain = bin_size, max(1, int(batch)), chain
        self.options = options
        self.pending = []            # (sweep, Δ snapshot)
        # batch = 1 measures at the device Δ, which is the snapshot's when add()
        # follows its sweep at once; a caller whose device has moved on since
        # (the sweep-batch drivers) clears this
        self.at_device = True

    def add(self, sweep: int, Delta):
        self.pending.append((sweep, np.array(Delta, dtype=np.complex128, copy=True)))
        if len(self.pending) >= self.batch:
            self.flush()

    def flush(self):
        if not self.pending:
            return
        p = self.p
        if self.batch == 1 and self.at_device:
            deltas = None
            specs = [self.ctx.measure_transport(p.eta, p.domega, p.omega_max, chain=self.chain)]
        else:
            deltas = np.stack([d for _, d in self.pending])
            specs = self.ctx.measure_transport_deltas(deltas, p.eta, p.domega, p.omega_max, chain=self.chain)
        results = [o.measure(self.ctx, p, self.chain, deltas) for o in self.options]
        for k, ((i, _), r) in enumerate(zip(self.pending, specs)):
            record_transport(self.out, self.res, self.bin_size, i, H.SpectrumResult(**r), self.options, results, k)
        self.pending = []


def measure_in_batches(ctx, p, outs, results, rngs, tqs, *, n_measure: int, Nt: int, dt: float,
                       measure_transport_freq: int, sweep_batch: int, field_sq: bool) -> None:
    """The measurement phase (src/Simulation.jl:133-228) of the chains of ctx
    on the throughput path, up to sweep_batch sweeps per device batch: draw the
    batch (per sweep and chain standard_complex_normal(rng, (N, 2)), then one
    rng.random(), always), load_draws, sweep_log with the snapshot cadence
    measure_transport_freq at the offset that keeps the cadence of the global
    sweep number, run_sweeps, then the results, the observables records and the
    snapshots read back: the same observables.csv rows (chain k into outs[k],
    results[k]) and the snapshots into tqs[k].add(i, Δ).  field_sq: S_d(q),
    S_s(q) of every sweep into field_sq.npy, (n_measure, 2, Ly, Lx), of each
    chain's directory."""
    K, B = len(outs), int(sweep_batch)
    if B < 1:
        raise ValueError("sweep_batch must be at least 1 (or None)")
    freq = max(int(measure_transport_freq), 0)
    for o in outs:
        o.tee(f"Sweep batches: up to {B} sweeps per device batch, one Metropolis uniform drawn for every sweep")
    t1 = time.time()
    acc_total = np.zeros(K, dtype=np.int64)
    sq_all = []
    setting = None
    done = 0
    while done < n_measure:
        b = min(B, n_measure - done)
        noise = np.empty((b, K, p.N, 2), dtype=np.complex128)
        u = np.empty((b, K))
        for s in range(b):
            for k in range(K):
                noise[s, k] = H.standard_complex_normal(rngs[k], (p.N, 2))
                u[s, k] = rngs[k].random()
        ctx.load_draws(noise, u)
        # sweep s of the batch is sweep i = done + s + 1 of the run; snapshots where i % freq == 0
        want = (field_sq, freq, (freq - 1 - done) % freq if freq else 0)
        if want != setting:
            ctx.sweep_log(observables=True, field_sq=field_sq, snapshot_every=freq, snapshot_offset=want[2])
            setting = want
        ctx.run_sweeps(0, b, Nt, dt, p.mass)
        acc, dH = ctx.sweep_results(0, b)
        rec = ctx.sweep_observables(0, b)
        if field_sq:
            sq_all.append(ctx.sweep_field_sq(0, b))
        sweeps, snaps = ctx.sweep_snapshots(0, b) if freq else ((), None)
        at = {int(s): m for m, s in enumerate(sweeps)}
        for s in range(b):
            i = done + s + 1
            for k in range(K):
                obs = H.ObservablesResult(*(float(v) for v in rec[s, k, :9]))
                a, d = bool(acc[s, k]), float(dH[s, k])
                acc_total[k] += a
                outs[k].observables(i, a, d, obs)
                results[k].records.append((i, a, d, obs))
                if s in at:
                    tqs[k].add(i, snaps[at[s], k])
                if i % 10 == 0:
                    outs[k].tee("Meas %d/%d. Acc=%.2f. E=%.4f" % (i, n_measure, acc_total[k] / i, obs.total_energy))
        done += b
    for tq in tqs:
        tq.flush()
    ctx.sweep_log(observables=False)
    for k in range(K):
        if field_sq:
            sq = np.concatenate(sq_all)[:, k] if sq_all else np.zeros((0, 2, p.Ly, p.Lx))
            np.save(os.path.join(outs[k].out_dir, "field_sq.npy"), sq)
        results[k].meas_acceptance = acc_total[k] / max(n_measure, 1)
        outs[k].tee(f"Measurement Done. Total Time: {round(time.time() - t1, 2)}s")


def run_simulation(p: H.ModelParameters, out_dir: str, *, n_therm: int = 100, n_measure: int = 500,
                   Nt_therm_init: int = 10, Nt_measure: int = 5, measure_transport_freq: int = 1,
                   bin_size: int = 5, verbose: bool = True, rng: np.random.Generator | None = None,
                   device: int = 0, delta_cap: float = 0.0, state: H.SimulationState | None = None,
                   cache: H.ComputeCache | None = None, transport_batch: int = 1,
                   spectral_maps: dict | None = None, current_response: dict | None = None,
                   operator_response: dict | None = None,
                   nambu_response: dict | None = None, response_map: dict | None = None,
                   correlations: dict | None = None, integrator=None, sweep_batch: int | None = None,
                   field_sq: bool = False) -> SimulationResult:
    """src/Simulation.jl:34-236.  Files in out_dir: simulation.log (appended),
    observables.csv, transport.csv (one row per transport measurement, every
    measure_transport_freq sweeps; <= 0 disables), and spectra_bins/ — the
    reference's spectra_bins.jld2 (:52,89,206-214) as numpy files: params.json,
    omega_grid.npy, and one sweep_<i>.npz per completed bin of bin_size
    measurements (opt_cond, dos, dos_AN, A_k0 averaged; count).
    transport_batch > 1 evaluates that many measurement sweeps' transport in
    one batched call (TransportQueue): same rows and bins, written up to
    transport_batch - 1 sweeps later.
    spectral_maps, current_response, operator_response, nambu_response,
    response_map, correlations: the measurement options (OPTIONS and
    EQUAL_TIME_OPTIONS), each a dict that its description documents
    (SpectralMaps, CurrentResponse, OperatorResponse, NambuResponse,
    ResponseMap, Correlations) or None (the default): the files as without
    the option.  integrator: the trajectories' splitting and the adaptive
    Nt's lower bound (Integrator), a name, a dict or None (the default: the
    reference's leapfrog, the files as without the keyword).  All are checked
    before any file is opened.
    sweep_batch: None (the default) takes every measurement sweep through the
    single-sweep entries and writes every file as before.  B >= 1 runs the
    measurement phase on the throughput path in batches of up to B sweeps
    (measure_in_batches): observables and Δ snapshots are logged on the device
    and read back once per batch, the files are the same ones.  The
    throughput path wants every uniform before its first sweep, so this mode
    draws, per sweep, standard_complex_normal(rng, (N, 2)) and then one
    rng.random() always — the reference's "rand() only when ΔH >= 0"
    (src/HMC.jl:128) cannot be kept.  The Markov chain is then the same for
    every B and differs from sweep_batch=None only in which uniforms the
    generator hands out; simulation.log names the mode.  Thermalisation keeps
    its per-sweep adaptive loop.  field_sq (with sweep_batch only): S_d(q) and
    S_s(q) of the pairing field after every measurement sweep into
    field_sq.npy, (n_measure, 2, Ly, Lx)."""
    if field_sq and sweep_batch is None:
        raise ValueError("field_sq needs sweep_batch (the structure factors are logged on the throughput path)")
    rng = rng if rng is not None else np.random.default_rng()
    options = parse_options(p, spectral_maps=spectral_maps, current_response=current_response,
                            operator_response=operator_response, nambu_response=nambu_response,
                            response_map=response_map, correlations=correlations)
    integ = parse_integrator(integrator)
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
            write_headers(out.spec_dir, p, options)
        if integ is not None:
            integ.apply(cache.require(), out)
        Nt_fin, acc_th = thermalize(cache, p, state, out, n_therm, Nt_therm_init, rng,
                                    Nt_min=4 if integ is None else integ.Nt_min)

        dt_meas = H.calc_optimal_dt(p.beta, p.J, p.mass, Nt_measure)
        out.tee("--- Measurement Start ---")
        out.tee(f"Settings: Nt={Nt_measure}, dt={round(dt_meas, 5)}")
        if integ is not None:
            out.tee(f"Factorisations per trajectory: {integ.stages * Nt_measure}")
        t1 = time.time()
        acc_total = 0
        res = SimulationResult(Nt_fin, acc_th, 0.0)
        tq = TransportQueue.with_options(options, cache.require(), p, out, res, bin_size, transport_batch)
        if sweep_batch is not None:
            ctx = cache.require()
            tq.at_device = False
            ctx.set_state(state.Delta, None)
            measure_in_batches(ctx, p, [out], [res], [rng], [tq], n_measure=n_measure, Nt=Nt_measure, dt=dt_meas,
                               measure_transport_freq=measure_transport_freq, sweep_batch=sweep_batch,
                               field_sq=field_sq)
            D, P = ctx.get_state()
            state.Delta, state.pi = D[0], P[0]
            cache.E_fermion = float(ctx.fermion_energy()[0])
            cache.pairing = ctx.pairing()[0]
            return res
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
                          nambu_response: dict | None = None, response_map: dict | None = None,
                          correlations: dict | None = None, integrator=None, sweep_batch: int | None = None,
                          field_sq: bool = False) -> list:
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
    nambu_response, response_map, correlations, integrator: as
    run_simulation's, for every chain.  sweep_batch, field_sq: as
    run_simulation's (there the draw order of that mode); every chain then
    runs the Markov chain of its run_simulation with the same sweep_batch."""
    K = len(out_dirs)
    if field_sq and sweep_batch is None:
        raise ValueError("field_sq needs sweep_batch (the structure factors are logged on the throughput path)")
    options = parse_options(p, spectral_maps=spectral_maps, current_response=current_response,
                            operator_response=operator_response, nambu_response=nambu_response,
                            response_map=response_map, correlations=correlations)
    integ = parse_integrator(integrator)
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
                write_headers(outs[k].spec_dir, p, options)
            if integ is not None:
                integ.apply(cache.require(), outs[k])
            Nt_fin, acc_th = thermalize(cache, p, st, outs[k], n_therm, Nt_therm_init, rngs[k],
                                        Nt_min=4 if integ is None else integ.Nt_min)
            cache.ctx.close()
            states.append(st)
            results.append(SimulationResult(Nt_fin, acc_th, 0.0))

        dis = np.stack([st.disorder_pot for st in states])
        ctx = H.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis,
                             delta_cap=delta_cap, device=device)
        try:
            ctx.set_pairing(np.stack([st.Delta for st in states]))
            ctx.factorize()
            if integ is not None:
                ctx.set_integrator(**integ.args)
            dt_meas = H.calc_optimal_dt(p.beta, p.J, p.mass, Nt_measure)
            for o in outs:
                o.tee("--- Measurement Start ---")
                o.tee(f"Settings: Nt={Nt_measure}, dt={round(dt_meas, 5)}")
                if integ is not None:
                    o.tee(f"Factorisations per trajectory: {integ.stages * Nt_measure}")
            if sweep_batch is not None:
                tqs = [TransportQueue.with_options(options, ctx, p, outs[k], results[k], bin_size, transport_batch,
                                                   chain=k) for k in range(K)]
                for tq in tqs:
                    tq.at_device = False
                measure_in_batches(ctx, p, outs, results, rngs, tqs, n_measure=n_measure, Nt=Nt_measure, dt=dt_meas,
                                   measure_transport_freq=measure_transport_freq, sweep_batch=sweep_batch,
                                   field_sq=field_sq)
                return results
            t1 = time.time()
            acc_total = np.zeros(K, dtype=np.int64)
            tqs = [TransportQueue.with_options(options, ctx, p, outs[k], results[k], bin_size, transport_batch, chain=k)
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
                        record_transport(outs[k], results[k], bin_size, i, H.SpectrumResult(**specs[k]), options,
                                         [o.measure(ctx, p, k, None) for o in options], 0)
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
