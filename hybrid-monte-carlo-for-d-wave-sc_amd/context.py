"""FermionContext: a typed handle on one dwh_ctx (batched over chains).

Array conventions on the Python side follow the reference's Julia indexing:
per chain a bond field is (N, 2) with column 0 = +x, 1 = +y
(src/Types.jl:106-111); batched fields are (nchains, N, 2).  They are
converted to the ABI's column-major layout here and nowhere else.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr


def _to_abi(a: np.ndarray, nc: int, N: int) -> np.ndarray:
    a = np.asarray(a, dtype=np.complex128)
    if a.shape == (N, 2):
        a = a[None]
    if a.shape != (nc, N, 2):
        raise ValueError(f"expected bond field of shape ({nc}, {N}, 2) or ({N}, 2), got {a.shape}")
    return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))


def _from_abi(a: np.ndarray, nc: int, N: int) -> np.ndarray:
    return np.ascontiguousarray(np.transpose(a.reshape(nc, 2, N), (0, 2, 1)))


def table_to_abi(table: np.ndarray) -> np.ndarray:
    """(N, 4) 1-based Int table -> Julia column-major N x 4 Int64 buffer."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError("neighbour table must be (N, 4)")
    return np.ascontiguousarray(t.T, dtype=np.int64)


# factorisation algorithm (include/dwhmc.h DWH_ALGO_*): "auto" = env DWHMC_ALGO,
# else block cyclic reduction when 2 Lx <= 128, eigendecomposition ("eig") when
# β·E'/2 is beyond the pole table
ALGOS = {"auto": -1, "dense": 0, "cr": 1, "eig": 2}

# HMC integrators (include/dwhmc.h DWH_INT_*, DWH_OMELYAN2_LAMBDA)
INTEGRATORS = {"leapfrog": 0, "omelyan2": 1, "custom": 2}
_INTEGRATOR_NAMES = {v: k for k, v in INTEGRATORS.items()}
OMELYAN2_LAMBDA = 0.1931833275037836
MAX_STAGES = 16

# the sweep log (include/dwhmc.h DWH_LOG_*, DWH_OBS_FIELDS): the parts and the
# columns of the observables record
LOG_OBS, LOG_FIELD_SQ, LOG_SNAPSHOT = 1, 2, 4
OBS_LOG_FIELDS = ("total_energy", "Delta_amp", "Delta_local", "Delta_global", "S_Delta", "hole_conc", "Delta_diff",
                  "Delta_pair", "Delta_localpair", "E_fermion", "tr_hh", "sum_abs2_Delta")


def sweep_log_layout(nchains: int, N: int, ndraws: int, observables=True, field_sq=False, snapshot_every=0,
                     snapshot_offset=0, first=0, nsweeps=None, what=None, lib=None):
    """(doubles of observables, doubles of field_sq, snapshots) of the sweeps
    [first, first + nsweeps) of a log over ndraws loaded sweeps
    (dwh_sweep_log_layout; host arithmetic, no device).  `what` overrides the
    mask the three switches give.  ValueError for what dwh_sweep_log and the
    readers refuse."""
    lib = _lib.load() if lib is None else lib
    if what is None:
        what = (LOG_OBS if observables else 0) | (LOG_FIELD_SQ if field_sq else 0)
        what |= LOG_SNAPSHOT if snapshot_every else 0
    nsweeps = ndraws - first if nsweeps is None else nsweeps
    counts = np.zeros(3, dtype=np.int64)
    check(lib.dwh_sweep_log_layout(int(nchains), int(N), int(ndraws), int(what), int(snapshot_every),
                                   int(snapshot_offset), int(first), int(nsweeps), ptr(counts)))
    return tuple(int(c) for c in counts)


def _integrator_args(kind, lam, kick, drift):
    """(kind code, λ, S, kick array, drift array) as the ABI takes them; the
    arrays only for "custom", whose S is the drift's length.  The library
    checks the schedule itself."""
    if kind not in INTEGRATORS:
        raise ValueError(f"integrator kind must be one of {sorted(INTEGRATORS)}")
    if kind != "custom":
        if kick is not None or drift is not None:
            raise ValueError(f"integrator {kind}: kick and drift belong to kind='custom'")
        return INTEGRATORS[kind], float(lam), 0, None, None
    a = None if kick is None else np.ascontiguousarray(np.asarray(kick, dtype=np.float64).reshape(-1))
    b = None if drift is None else np.ascontiguousarray(np.asarray(drift, dtype=np.float64).reshape(-1))
    if a is not None and b is not None and len(a) != len(b) + 1:
        raise ValueError("integrator custom: kick has one entry more than drift (a_0..a_S, b_1..b_S)")
    S = len(b) if b is not None else len(a) - 1 if a is not None else 0
    return INTEGRATORS[kind], float(lam), S, a, b


def integrator_stages(kind="leapfrog", kick=None, drift=None) -> int:
    """Force evaluations (factorisations) per step of an integrator."""
    return {"leapfrog": 1, "omelyan2": 2}.get(kind) or _integrator_args(kind, 0.0, kick, drift)[2]


def integrator_schedule(kind, Nt: int, dt: float, mass: float, lam: float = OMELYAN2_LAMBDA, kick=None, drift=None,
                        nstage: int | None = None, lib=None):
    """(kicks, drifts) of a trajectory of Nt steps as the enqueue hands them to
    the kick/drift kernels (dwh_debug_integrator_schedule; host arithmetic, no
    device): S·Nt + 1 kicks and S·Nt drifts, leapfrog at Nt = 0 its two half
    kicks.  nstage overrides the S taken from the arrays' lengths.  ValueError
    for what the library refuses."""
    lib = _lib.load() if lib is None else lib
    k, lam, S, a, b = _integrator_args(kind, lam, kick, drift)
    S = S if nstage is None else int(nstage)
    args = (k, lam, S, ptr(a), ptr(b), int(Nt), float(dt), float(mass))
    nfact = C.c_int64()
    check(lib.dwh_debug_integrator_schedule(*args, C.byref(nfact), None, None))
    kicks, drifts = np.empty(max(nfact.value + 1, 2)), np.empty(nfact.value)
    check(lib.dwh_debug_integrator_schedule(*args, C.byref(nfact), ptr(kicks), ptr(drifts)))
    return kicks[:nfact.value + 1 if nfact.value else 2], drifts


class FermionContext:
    """Device-resident fermionic action/force evaluator for nchains chains.
    delta_cap <= 0 selects the ABI default for the guard (bond guard on
    max|Δ_ij|: max(2, 6 sqrt(2J/β)); site guard on the mean |Δ| of a site's
    4 bonds, CR path: max(1.25, 4 sqrt(2J/β)))
    on max|Δ_ij|; an uploaded Δ or a trajectory beyond it re-selects the pole
    set (include/dwhmc.h)."""

    def __init__(self, Lx, Ly, t, tp, mu, beta, J, nn_table, nnn_table, disorder,
                 delta_cap: float = 0.0, device: int = 0, lib_path: str | None = None,
                 algo: str = "auto"):
        self._lib = _lib.load() if lib_path is None else _lib.load_path(lib_path)
        dis = np.ascontiguousarray(np.atleast_2d(np.asarray(disorder, dtype=np.float64)))
        self.N = int(Lx) * int(Ly)
        if dis.shape[1] != self.N:
            raise ValueError(f"disorder must have N={self.N} entries per chain")
        self.nchains = dis.shape[0]
        self.beta, self.J = float(beta), float(J)
        h = C.c_void_p()
        nn = table_to_abi(nn_table)
        nnn = table_to_abi(nnn_table)
        if algo not in ALGOS:
            raise ValueError(f"algo must be one of {sorted(ALGOS)}")
        rc = self._lib.dwh_create_ex(C.byref(h), int(Lx), int(Ly), float(t), float(tp),
                                     float(mu), float(beta), float(J), ptr(nn), ptr(nnn),
                                     self.nchains, ptr(dis), float(delta_cap), ALGOS[algo],
                                     int(device))
        check(rc, None)
        self._h = h
        self.info_lattice = (int(Lx), int(Ly))

    # -- lifecycle -------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.dwh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc):
        check(rc, self._h)

    @property
    def info(self) -> dict:
        """dwh_info: sizes, pole set (kappa, npoles, delta_cap; a guard trip
        re-selects it), algorithm, device bytes."""
        return self._info()

    def _info(self):
        inf = _lib.dwh_info_t()
        self._c(self._lib.dwh_info(self._h, C.byref(inf)))
        return {k: getattr(inf, k) for k, _ in inf._fields_}

    # -- hot path --------------------------------------------------------
    def set_pairing(self, Delta):
        a = _to_abi(Delta, self.nchains, self.N)
        self._c(self._lib.dwh_update_pairing(self._h, ptr(a)))

    def factorize(self):
        self._c(self._lib.dwh_factorize(self._h))

    def forces(self, Delta=None) -> np.ndarray:
        d = None if Delta is None else _to_abi(Delta, self.nchains, self.N)
        out = np.empty((self.nchains, 2, self.N), dtype=np.complex128)
        self._c(self._lib.dwh_forces(self._h, ptr(d), ptr(out)))
        return _from_abi(out, self.nchains, self.N)

    def pairing(self) -> np.ndarray:
        out = np.empty((self.nchains, 2, self.N), dtype=np.complex128)
        self._c(self._lib.dwh_pairing(self._h, ptr(out)))
        return _from_abi(out, self.nchains, self.N)

    def fermion_energy(self) -> np.ndarray:
        out = np.empty(self.nchains)
        self._c(self._lib.dwh_fermion_energy(self._h, ptr(out)))
        return out

    def hole_trace(self) -> np.ndarray:
        out = np.empty(self.nchains)
        self._c(self._lib.dwh_hole_trace(self._h, ptr(out)))
        return out

    def total_energy(self, mass: float) -> np.ndarray:
        out = np.empty(self.nchains)
        self._c(self._lib.dwh_total_energy(self._h, float(mass), ptr(out)))
        return out

    def set_state(self, Delta=None, pi=None):
        d = None if Delta is None else _to_abi(Delta, self.nchains, self.N)
        p = None if pi is None else _to_abi(pi, self.nchains, self.N)
        self._c(self._lib.dwh_set_state(self._h, ptr(d), ptr(p)))

    def get_state(self):
        d = np.empty((self.nchains, 2, self.N), dtype=np.complex128)
        p = np.empty_like(d)
        self._c(self._lib.dwh_get_state(self._h, ptr(d), ptr(p)))
        return _from_abi(d, self.nchains, self.N), _from_abi(p, self.nchains, self.N)

    def hmc_sweep(self, noise, uniform, Nt: int, dt: float, mass: float):
        nz = _to_abi(noise, self.nchains, self.N)
        u = np.ascontiguousarray(np.atleast_1d(np.asarray(uniform, dtype=np.float64)))
        if u.shape != (self.nchains,):
            raise ValueError("one uniform per chain")
        acc = np.zeros(self.nchains, dtype=np.uint8)
        dH = np.zeros(self.nchains)
        self._c(self._lib.dwh_hmc_sweep(self._h, ptr(nz), ptr(u), int(Nt), float(dt), float(mass),
                                        ptr(acc), ptr(dH)))
        return acc.astype(bool), dH

    def hmc_trajectory(self, noise, Nt: int, dt: float, mass: float) -> np.ndarray:
        """hmc_sweep! up to H_new (dwh_hmc_trajectory); returns ΔH per chain.
        Finish with hmc_finish(accepted)."""
        nz = _to_abi(noise, self.nchains, self.N)
        dH = np.zeros(self.nchains)
        self._c(self._lib.dwh_hmc_trajectory(self._h, ptr(nz), int(Nt), float(dt), float(mass), ptr(dH)))
        return dH

    def hmc_finish(self, accepted):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(accepted)).astype(np.uint8))
        if a.shape != (self.nchains,):
            raise ValueError("one accept flag per chain")
        self._c(self._lib.dwh_hmc_finish(self._h, ptr(a)))

    def set_integrator(self, kind="omelyan2", lam: float = OMELYAN2_LAMBDA, kick=None, drift=None):
        """The splitting every trajectory of this context runs from now on
        (dwh_set_integrator): "leapfrog" (the default of a new context),
        "omelyan2" (two factorisations per step, `lam` its λ) or "custom" with
        kick = a_0..a_S and drift = b_1..b_S.  Nt stays the number of steps, so
        a trajectory makes S·Nt factorisations.  ValueError for a schedule the
        library refuses."""
        k, lam, S, a, b = _integrator_args(kind, lam, kick, drift)
        self._c(self._lib.dwh_set_integrator(self._h, k, lam, S, ptr(a), ptr(b)))

    @property
    def integrator(self) -> dict:
        """dwh_get_integrator: kind, lam (0 unless omelyan2), and the kick
        (S + 1) and drift (S) coefficients in use."""
        kind, lam, S = C.c_int32(), C.c_double(), C.c_int64()
        a, b = np.zeros(MAX_STAGES + 1), np.zeros(MAX_STAGES)
        self._c(self._lib.dwh_get_integrator(self._h, C.byref(kind), C.byref(lam), C.byref(S), ptr(a), ptr(b)))
        return dict(kind=_INTEGRATOR_NAMES[kind.value], lam=lam.value, kick=a[:S.value + 1].copy(),
                    drift=b[:S.value].copy())

    # -- throughput path -------------------------------------------------
    def load_draws(self, noise, uniform):
        noise = np.asarray(noise, dtype=np.complex128)
        ns = noise.shape[0]
        nz = np.ascontiguousarray(np.transpose(noise.reshape(ns, self.nchains, self.N, 2), (0, 1, 3, 2)))
        u = np.ascontiguousarray(np.asarray(uniform, dtype=np.float64).reshape(ns, self.nchains))
        self._c(self._lib.dwh_load_draws(self._h, ns, ptr(nz), ptr(u)))

    def run_sweeps(self, first: int, nsweeps: int, Nt: int, dt: float, mass: float):
        self._c(self._lib.dwh_run_sweeps(self._h, int(first), int(nsweeps), int(Nt), float(dt),
                                         float(mass)))

    def sweep_results(self, first: int, nsweeps: int):
        acc = np.zeros((nsweeps, self.nchains), dtype=np.uint8)
        dH = np.zeros((nsweeps, self.nchains))
        self._c(self._lib.dwh_sweep_results(self._h, int(first), int(nsweeps), ptr(acc), ptr(dH)))
        return acc.astype(bool), dH

    def sweep_log(self, observables: bool = True, field_sq: bool = False, snapshot_every: int = 0,
                  snapshot_offset: int = 0):
        """What every sweep of run_sweeps records on the device from now on
        (dwh_sweep_log): the observables record (OBS_LOG_FIELDS), the pairing
        field's structure factors, and Δ after the sweeps snapshot_offset +
        k·snapshot_every of the loaded draws (snapshot_every = 0: none).
        Nothing enabled frees the log.  The buffers start from zero."""
        what = (LOG_OBS if observables else 0) | (LOG_FIELD_SQ if field_sq else 0)
        what |= LOG_SNAPSHOT if snapshot_every else 0
        self._c(self._lib.dwh_sweep_log(self._h, what, int(snapshot_every), int(snapshot_offset)))

    def sweep_observables(self, first: int, nsweeps: int) -> np.ndarray:
        """(nsweeps, nchains, 12): the record of every chain after the sweeps
        first .. first + nsweeps - 1, columns OBS_LOG_FIELDS."""
        out = np.empty((nsweeps, self.nchains, len(OBS_LOG_FIELDS)))
        self._c(self._lib.dwh_sweep_observables(self._h, int(first), int(nsweeps), ptr(out)))
        return out

    def sweep_field_sq(self, first: int, nsweeps: int) -> np.ndarray:
        """(nsweeps, nchains, 2, Ly, Lx): S_d (channel 0) and S_s (1) of the
        pairing field after every sweep, indexed [ky, kx]."""
        Lx, Ly = self.info_lattice
        out = np.empty((nsweeps, self.nchains, 2, Ly, Lx))
        self._c(self._lib.dwh_sweep_field_sq(self._h, int(first), int(nsweeps), ptr(out)))
        return out

    def sweep_snapshots(self, first: int, nsweeps: int):
        """(sweeps (m,), Delta (m, nchains, N, 2)): the snapshots taken after
        the sweeps of [first, first + nsweeps), ascending."""
        m = C.c_int64()
        self._c(self._lib.dwh_sweep_snapshots(self._h, int(first), int(nsweeps), C.byref(m), None, None))
        sweeps = np.empty(m.value, dtype=np.int64)
        D = np.empty((m.value, self.nchains, 2, self.N), dtype=np.complex128)
        self._c(self._lib.dwh_sweep_snapshots(self._h, int(first), int(nsweeps), C.byref(m), ptr(sweeps), ptr(D)))
        return sweeps, np.ascontiguousarray(np.transpose(D, (0, 1, 3, 2)))

    def synchronize(self):
        self._c(self._lib.dwh_synchronize(self._h))

    def stream(self) -> int:
        s = C.c_void_p()
        self._c(self._lib.dwh_stream(self._h, C.byref(s)))
        return s.value or 0

    # -- measurement path (eigenpairs, transport / spectra) ---------------
    def eigensystem(self, chain: int = 0, vectors: bool = True):
        """(E, U) of H_BdG at the device Δ of `chain` (dwh_eigensystem):
        E ascending (2N,), U (2N, 2N) with eigenvectors in columns."""
        n2 = 2 * self.N
        E = np.empty(n2)
        Ucm = np.empty((n2, n2), dtype=np.complex128) if vectors else None   # row c = column c of U
        self._c(self._lib.dwh_eigensystem(self._h, int(chain), ptr(E), ptr(Ucm)))
        return E, (None if Ucm is None else Ucm.T)

    def measure_transport(self, eta: float, domega: float, omega_max: float, chain: int = 0) -> dict:
        """measure_transport_and_spectra (src/Observables.jl:314-526) for one
        chain at the device Δ; keys are the SpectrumResult fields
        (:293-308), A_k_omega0 indexed [kx, ky]."""
        o = _TransportOutputs(self, 1, eta, domega, omega_max)
        dp = C.POINTER(C.c_double)                       # (this entry declares its two scalars as double*)
        self._c(self._lib.dwh_measure_transport(self._h, int(chain), float(eta), float(domega), float(omega_max),
                                                o.st.ctypes.data_as(dp), o.dc.ctypes.data_as(dp), ptr(o.sigma),
                                                o.nw, ptr(o.dos), ptr(o.dos_an), o.nd, ptr(o.ak)))
        return o.results()[0]

    def measure_transport_all(self, eta: float, domega: float, omega_max: float) -> list:
        """measure_transport for every chain, the eigensolves and J_mn
        products batched (dwh_measure_transport_batched); one dict per chain."""
        o = _TransportOutputs(self, self.nchains, eta, domega, omega_max)
        self._c(self._lib.dwh_measure_transport_batched(self._h, float(eta), float(domega), float(omega_max),
                                                        ptr(o.st), ptr(o.dc), ptr(o.sigma), o.nw, ptr(o.dos),
                                                        ptr(o.dos_an), o.nd, ptr(o.ak)))
        return o.results()

    def measure_transport_deltas(self, deltas, eta: float, domega: float, omega_max: float,
                                 chain: int = 0) -> list:
        """measure_transport at a list of pairing fields (each (N, 2)) on the
        lattice and disorder of `chain`, eigensolves batched over the list
        (dwh_measure_transport_deltas); one dict per field, in order."""
        ns, d = self._states(deltas, min_states=0)
        o = _TransportOutputs(self, ns, eta, domega, omega_max)
        self._c(self._lib.dwh_measure_transport_deltas(self._h, int(chain), ns, ptr(d), float(eta), float(domega),
                                                       float(omega_max), ptr(o.st), ptr(o.dc), ptr(o.sigma), o.nw,
                                                       ptr(o.dos), ptr(o.dos_an), o.nd, ptr(o.ak)))
        return o.results()

    def _states(self, deltas, min_states: int = 1):
        """(nstates, pairing fields in the ABI layout) of a call's `deltas`
        ((nstates, N, 2)); None, where a call takes it, is the one state at
        the device Δ: (1, None)."""
        if deltas is None and min_states > 0:
            return 1, None
        D = np.asarray(deltas, dtype=np.complex128)
        if D.ndim != 3 or D.shape[1:] != (self.N, 2) or D.shape[0] < min_states:
            raise ValueError(f"expected (nstates, {self.N}, 2) pairing fields")
        return D.shape[0], np.ascontiguousarray(np.transpose(D, (0, 2, 1)))

    def measure_spectral_maps(self, eta: float, domega: float, omega_max: float, first: int = 0,
                              count: int | None = None, stride: int = 1, chain: int = 0, deltas=None,
                              ldos: bool = True, akw: bool = True) -> dict:
        """LDOS(i, ω) and A(k, ω) (dwh_measure_spectral_maps) on the window
        first + q·stride, q < count, of the DOS grid -ω_max:Δω:ω_max
        (count=None: up to the end of the grid), at the device Δ of `chain`
        or at the pairing fields `deltas` ((nstates, N, 2)) on its lattice
        and disorder.  Returns omega (count,) and, unless switched off, ldos
        and akw of shape (nstates, count, Ly, Lx): ldos[s, q, y, x] at site
        i = x + Lx·y, akw[s, q, ky, kx]."""
        first, stride = int(first), int(stride)
        omega = spectral_window(eta, domega, omega_max, first, count, stride, self._lib)
        count = len(omega)
        ns, d = self._states(deltas)
        Lx, Ly = self.info_lattice
        out_l = np.empty((ns, count, Ly, Lx)) if ldos else None
        out_a = np.empty((ns, count, Ly, Lx)) if akw else None
        self._c(self._lib.dwh_measure_spectral_maps(self._h, int(chain), ns, ptr(d), float(eta), float(domega),
                                                    float(omega_max), first, count, stride, ptr(out_l),
                                                    ptr(out_a)))
        res = dict(omega=omega)
        if ldos:
            res["ldos"] = out_l
        if akw:
            res["akw"] = out_a
        return res

    def measure_current_response(self, direction="x", q=((0, 1),), n_matsubara: int = 1, chain: int = 0,
                                 deltas=None) -> dict:
        """Current response Λ_αα(q, iΩ_l) and the diamagnetic term of
        direction α = "x" / "y" (or 0 / 1) (dwh_measure_current_response) at
        the lattice momenta q = 2π (mx/Lx, my/Ly) of the list of (mx, my)
        (not reduced modulo L) and Ω_l = 2π l/β, l < n_matsubara, at the
        device Δ of `chain` or at the pairing fields `deltas` ((nstates, N, 2))
        on its lattice and disorder.  Returns dia (float, or (nstates,) with
        deltas) and lam ((nq, n_matsubara), or (nstates, nq, n_matsubara));
        the stiffness of the transverse limit is dia - lam[q, 0]."""
        if direction not in ("x", "y", 0, 1):
            raise ValueError("direction must be 'x' or 'y'")
        d = 0 if direction in ("x", 0) else 1
        qa = np.ascontiguousarray(np.asarray(q, dtype=np.int64).reshape(-1, 2))
        nq, nl = qa.shape[0], int(n_matsubara)
        ns, D = self._states(deltas)
        dia = np.empty(ns)
        lam = np.empty((ns, max(nq, 0), max(nl, 0)))
        self._c(self._lib.dwh_measure_current_response(self._h, int(chain), ns, ptr(D), d, nq, ptr(qa), nl,
                                                       ptr(dia), ptr(lam)))
        return _per_state(deltas, scalars=("dia",), dia=dia, lam=lam)

    def measure_operator_response(self, ops, spin_sign=None, n_matsubara: int = 1, omega=None, eta=None,
                                  chain: int = 0, deltas=None) -> dict:
        """Response of one-body operators O = Σ_ij V_ij (c†_{i↑} c_{j↑} + s
        c†_{i↓} c_{j↓}) (dwh_measure_operator_response; Nambu matrix
        V ⊕ (-s V^T)): χ(iΩ_l), l < n_matsubara, in the conventions of
        measure_current_response's lam, and χ''(ω) on a real-frequency grid
        in the conventions of σ(ω) without its 1/ω.
        ops: a tuple (rowptr, col, val) — the CSR pattern shared by all
        operators (0-based, N rows) with val (nops, nnz) — or a list of
        operators, each a vertices.Vertex, a COO triple (row, col, val) or a
        dense (N, N) matrix, which vertices.union_csr puts on one pattern.
        spin_sign: ±1 per operator (one int for all; None: the Vertex's own).
        omega: None (no χ''), dict(start=, step=, count=) or (start, step,
        count): the grid start + j·step, j < count, of either sign; needs
        eta > 0.  At the device Δ of `chain` or at the pairing fields
        `deltas` ((nstates, N, 2)).  Returns chi ((nstates,) nops,
        n_matsubara), chi2 ((nstates,) nops, n_w) and omega (n_w,)."""
        from . import vertices as vx
        N = self.N
        if isinstance(ops, tuple):
            if len(ops) != 3:
                raise ValueError("ops: a CSR tuple (rowptr, col, val) or a list of operators")
            rowptr, col, val = _csr_tuple(ops, N, "ops: rowptr of {n} entries and val (nops, {nnz}) expected")
        else:
            ops = list(ops)
            if not ops:
                raise ValueError("ops is empty")
            if spin_sign is None:
                if not all(isinstance(o, vx.Vertex) for o in ops):
                    raise ValueError("spin_sign is needed unless every operator is a vertices.Vertex")
                spin_sign = [o.spin_sign for o in ops]
            rowptr, col, val = vx.union_csr(ops, N)
        nops, nnz = val.shape
        if spin_sign is None:
            raise ValueError("spin_sign is needed with a CSR tuple")
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(spin_sign, dtype=np.int32), (nops,)))
        nl = int(n_matsubara)
        w0, dw, nw = _omega_grid(omega, eta)
        ns, D = self._states(deltas)
        chi = np.empty((ns, nops, max(nl, 0)))
        chi2 = np.empty((ns, nops, max(nw, 0)))
        self._c(self._lib.dwh_measure_operator_response(
            self._h, int(chain), ns, ptr(D), nops, ptr(rowptr), ptr(col), nnz, ptr(val), ptr(sg), nl,
            ptr(chi) if nl > 0 else None, 0.0 if eta is None else float(eta), w0, dw, nw,
            ptr(chi2) if nw > 0 else None))
        return dict(_per_state(deltas, chi=chi, chi2=chi2), omega=w0 + dw * np.arange(max(nw, 0)))

    def measure_nambu_response(self, vertices, pairs=None, n_matsubara: int = 1, omega=None, eta=None,
                               chain: int = 0, deltas=None) -> dict:
        """Cross response <O_a ; O_b†> of general Nambu vertices, pairing parts
        included (dwh_measure_nambu_response): O_k = Ψ† W_k Ψ with W_k any
        complex 2N x 2N matrix in the basis Ψ = (c_{i↑}; c†_{i↓}).
        vertices: a tuple (rowptr, col, val) — one CSR pattern with 2N rows
        (rowptr an integer array of 2N + 1 entries, which is what tells it
        from a collection) and val (nops, nnz) — or a list or tuple of
        vertices, each a vertices.NambuVertex, a vertices.Vertex (lifted to
        V ⊕ (-s V^T)), a COO triple over 2N or a dense (2N, 2N) matrix; one
        NambuVertex / Vertex may be passed bare.  pairs: list of (a, b)
        indices into the vertices (None: every (k, k)).  omega / eta / chain / deltas as in
        measure_operator_response.  Returns complex chi ((nstates,) npairs,
        n_matsubara) = Σ (f_n - f_m)/(ΔE - iΩ_l) X^a conj(X^b) / N with the
        l = 0 rules of measure_current_response, complex chi2 ((nstates,)
        npairs, n_w), omega (n_w,) and pairs (npairs, 2)."""
        from . import vertices as vx
        N = self.N
        rowptr, col, val = _nambu_csr(vx, vertices, N)
        nops, nnz = val.shape
        if pairs is None:
            pr = np.stack([np.arange(nops, dtype=np.int64)] * 2, axis=1)
        else:
            pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        pr = np.ascontiguousarray(pr)
        npairs = pr.shape[0]
        nl = int(n_matsubara)
        w0, dw, nw = _omega_grid(omega, eta)
        ns, D = self._states(deltas)
        chi = np.empty((ns, npairs, max(nl, 0)), dtype=np.complex128)
        chi2 = np.empty((ns, npairs, max(nw, 0)), dtype=np.complex128)
        self._c(self._lib.dwh_measure_nambu_response(
            self._h, int(chain), ns, ptr(D), nops, ptr(rowptr), ptr(col), nnz, ptr(val), npairs, ptr(pr), nl,
            ptr(chi) if nl > 0 else None, 0.0 if eta is None else float(eta), w0, dw, nw,
            ptr(chi2) if nw > 0 else None))
        return dict(_per_state(deltas, chi=chi, chi2=chi2), omega=w0 + dw * np.arange(max(nw, 0)), pairs=pr)

    def measure_response_map(self, vertices, pattern, n_matsubara: int = 1, omega=None, eta=None, rho: bool = True,
                             chain: int = 0, deltas=None) -> dict:
        """Response maps (dwh_measure_response_map): the linear-response
        density matrix D(z)[W] = U (w(z) ∘ U^H W U) U^H of each source vertex
        W and the equal-time ρ = U f U^H, at the entries of a sparse pattern.
        vertices: as measure_nambu_response takes them.  pattern: an (npat, 2)
        integer array of Nambu index pairs (a, b) in [0, 2N), any order,
        duplicates allowed (vertices.bond_pattern builds the site / bond
        ones).  z runs over the n_matsubara Matsubara indices (the weights of
        measure_nambu_response's chi) and then the real frequencies omega (a
        list of either sign, w = (f_n - f_m)/(ΔE - ω - iη), needs eta > 0).
        No 1/N is applied: vertices.contract(pattern, D, B) = N·chi of the
        pair (W, B).  n_matsubara = 0 and omega None skips dmap, rho=False
        skips ρ.  Returns dmap ((nstates,) nops, nz, npat) or None, rho
        ((nstates,) npat) or None, pattern (npat, 2) and omega (n_w,)."""
        from . import vertices as vx
        N = self.N
        rowptr, col, val = _nambu_csr(vx, vertices, N)
        nops, nnz = val.shape
        pat = np.asarray(pattern)
        if pat.ndim != 2 or pat.shape[1] != 2 or not np.issubdtype(pat.dtype, np.integer):
            raise ValueError("pattern: an (npat, 2) integer array of Nambu index pairs")
        pat = np.ascontiguousarray(pat, dtype=np.int64)
        prow, pcol = np.ascontiguousarray(pat[:, 0]), np.ascontiguousarray(pat[:, 1])
        npat = pat.shape[0]
        nl = int(n_matsubara)
        w = np.zeros(0) if omega is None else np.ascontiguousarray(np.asarray(omega, dtype=np.float64).ravel())
        nw = len(w)
        if nw > 0 and eta is None:
            raise ValueError("eta is needed with omega")
        nz = max(nl, 0) + nw
        ns, D = self._states(deltas)
        dmap = np.empty((ns, nops, nz, npat), dtype=np.complex128) if nz > 0 else None
        r = np.empty((ns, npat), dtype=np.complex128) if rho else None
        self._c(self._lib.dwh_measure_response_map(
            self._h, int(chain), ns, ptr(D), nops, ptr(rowptr), ptr(col), nnz, ptr(val), npat, ptr(prow), ptr(pcol),
            nl, 0.0 if eta is None else float(eta), nw, ptr(w) if nw > 0 else None, ptr(r), ptr(dmap)))
        return dict(_per_state(deltas, dmap=dmap, rho=r), pattern=pat, omega=w)

    def measure_correlations(self, families, pairs=None, ref_sites=None, mean: bool = True, chain: int = 0,
                             deltas=None, corr: bool = True) -> dict:
        """Equal-time correlations of local operators (dwh_measure_correlations):
        C_AB(r) = (1/N) Σ_j G_AB(j ⊕ r, j), G_AB(i, j) = <O_A(i) O_B(j)†> -
        <O_A(i)><O_B(j)†> by Wick's theorem from the full ρ = U f U^H.
        families: a list of vertices.LocalFamily (vertices.local_family builds
        the named ones), or the term table (tptr, trow, tcol, tval) itself.
        pairs: list of (a, b) indices into the families (None: every (k, k)).
        ref_sites: sites around which the untranslated G(ref ⊕ r, ref) is
        returned too (None: no local output).  mean=False / corr=False skip
        those outputs (corr= is this binding's own switch for the ABI's
        nullable corr).  At the device Δ of `chain` or at the pairing fields
        `deltas` ((nstates, N, 2)).  Returns corr ((nstates,) npairs, Ly, Lx)
        at [ry, rx] or None, local ((nstates,) npairs, nref, Ly, Lx) or None,
        mean ((nstates,) nfam, Ly, Lx) at [y, x] or None, and pairs (npairs, 2).
        The disconnected part is vertices.disconnected(p, mean[a], mean[b])."""
        from . import vertices as vx
        N = self.N
        Lx, Ly = self.info_lattice
        if isinstance(families, tuple) and len(families) == 4 and not isinstance(families, vx.LocalFamily) \
                and not isinstance(families[0], vx.LocalFamily):          # (else: four families in a tuple)
            tptr = np.ascontiguousarray(families[0], dtype=np.int64).ravel()
            trow = np.ascontiguousarray(families[1], dtype=np.int64).ravel()
            tcol = np.ascontiguousarray(families[2], dtype=np.int64).ravel()
            tval = np.ascontiguousarray(families[3], dtype=np.complex128).ravel()
            if len(tptr) < 1 or (len(tptr) - 1) % N or not (len(trow) == len(tcol) == len(tval)) \
                    or tptr[-1] != len(tval):
                raise ValueError("families: a term table needs tptr of nfam N + 1 entries ending at the term count")
        else:
            if isinstance(families, vx.LocalFamily):
                families = [families]
            tptr, trow, tcol, tval = vx.local_terms(families, N)
        nfam = (len(tptr) - 1) // N
        if pairs is None:
            pr = np.stack([np.arange(nfam, dtype=np.int64)] * 2, axis=1)
        else:
            pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        pr = np.ascontiguousarray(pr)
        npairs = pr.shape[0]
        ref = None if ref_sites is None else np.ascontiguousarray(np.asarray(ref_sites, dtype=np.int64).ravel())
        nref = 0 if ref is None else len(ref)
        ns, D = self._states(deltas)
        out_m = np.empty((ns, nfam, Ly, Lx), dtype=np.complex128) if mean else None
        out_c = np.empty((ns, npairs, Ly, Lx), dtype=np.complex128) if corr else None
        out_l = np.empty((ns, npairs, nref, Ly, Lx), dtype=np.complex128) if ref is not None else None
        self._c(self._lib.dwh_measure_correlations(
            self._h, int(chain), ns, ptr(D), nfam, ptr(tptr), ptr(trow), ptr(tcol), ptr(tval), npairs, ptr(pr),
            nref, ptr(ref), ptr(out_m), ptr(out_c), ptr(out_l)))
        return dict(_per_state(deltas, corr=out_c, local=out_l, mean=out_m), pairs=pr)

    # -- assembly read-back (parity tests) --------------------------------
    def debug_dense_H(self, chain: int = 0) -> np.ndarray:
        """H_BdG(Δ) (2N, 2N) as the eigen/transport path assembles it (dwh_debug_dense_H)."""
        n2 = 2 * self.N
        Hcm = np.empty((n2, n2), dtype=np.complex128)          # row c = column c
        self._c(self._lib.dwh_debug_dense_H(self._h, int(chain), ptr(Hcm)))
        return Hcm.T.copy()

    def debug_set_eigensystem(self, E, U, ph: bool = False):
        """Stage eigensystems for the next measurement call's eigensolve
        (dwh_debug_set_eigensystem; one-shot): E (2N,) or (nstates, 2N)
        ascending, U (2N, 2N) or (nstates, 2N, 2N) with the vector of E[n] in
        column n.  The next measure_* call with as many states reduces these
        instead of solving; ph=True also takes transport's particle-hole
        half sums (column 2N-1-n must be the Nambu partner of column n)."""
        n2 = 2 * self.N
        E = np.asarray(E, dtype=np.float64)
        U = np.asarray(U, dtype=np.complex128)
        if E.ndim == 1:
            E, U = E[None], U[None]
        if E.ndim != 2 or E.shape[1] != n2 or U.shape != (E.shape[0], n2, n2):
            raise ValueError(f"expected E (nstates, {n2}) and U (nstates, {n2}, {n2})")
        Ecm = np.ascontiguousarray(E)
        Ucm = np.ascontiguousarray(np.transpose(U, (0, 2, 1)))     # row c = column c of U
        self._c(self._lib.dwh_debug_set_eigensystem(self._h, E.shape[0], ptr(Ecm), ptr(Ucm), int(bool(ph))))

    def debug_level0(self, chain: int = 0, pole: int = 0, refill: bool = True):
        """(M, y): H_BdG(Δ) - i y_pole I (2N, 2N) from the CR level-0 blocks the
        factorisation consumes (dwh_debug_level0), and the pole heights y_q."""
        n2 = 2 * self.N
        Mcm = np.empty((n2, n2), dtype=np.complex128)
        y = np.empty(self.info["npoles"])
        self._c(self._lib.dwh_debug_level0(self._h, int(chain), int(pole), int(bool(refill)), ptr(Mcm), ptr(y)))
        return Mcm.T.copy(), y

    def debug_cr_resolvent(self, chain: int = 0, pole: int = 0) -> dict:
        """What the CR gathers read for batch item (chain, pole) after a
        factorisation (dwh_debug_cr_resolvent): G12 (N, 4) = G[i, N + cols[i, s]]
        (cols -1: unused slot, G12 0), diag (N,) = G[i, i] (G22[i, i] =
        -conj(diag[i])), lndet = ln|det(H_BdG - i y_pole)|, and the pole
        heights y and weights c."""
        P = self.info["npoles"]
        G12 = np.empty((self.N, 4), dtype=np.complex128)
        cols = np.empty((self.N, 4), dtype=np.int32)
        diag = np.empty(self.N, dtype=np.complex128)
        ld = C.c_double()
        y, cq = np.empty(P), np.empty(P)
        self._c(self._lib.dwh_debug_cr_resolvent(self._h, int(chain), int(pole), ptr(G12), ptr(cols), ptr(diag),
                                                 C.byref(ld), ptr(y), ptr(cq)))
        return dict(G12=G12, cols=cols, diag=diag, lndet=ld.value, y=y, c=cq)

    # -- timing ----------------------------------------------------------
    TIMERS =("gj_update", "gj_pivot", "assemble", "contract", "step", "gj_edge", "cr_gemm", "cr_inv",
              "cr_inv_side", "eig_own", "eig_vendor", "cr_sparse", "spectral", "response", "operator",
              "nambu", "map", "corr_rho", "corr_contract", "corr_reduce", "sweep_log")

    def timing_enable(self, on=True):
        """on: True (all timers), False, or an iterable of timer names."""
        if on is True:
            mask = -1
        elif not on:
            mask = 0
        else:
            mask = sum(1 << self.TIMERS.index(n) for n in on)
        self._c(self._lib.dwh_timing_enable(self._h, mask))

    def timing_reset(self):
        self._c(self._lib.dwh_timing_reset(self._h))

    def bench_assembly(self, reps: int):
        """dwh_bench_assembly: reps back-to-back assembly launches (timer "assemble")."""
        self._c(self._lib.dwh_bench_assembly(self._h, int(reps)))

    def bench_response_product(self, reps: int) -> float:
        """dwh_bench_response_product: milliseconds per 2N-cubed complex product
        (the one measure_current_response runs per momentum), warm, reps launches."""
        ms = C.c_double()
        self._c(self._lib.dwh_bench_response_product(self._h, int(reps), C.byref(ms)))
        return ms.value

    def bench_response_map_stages(self, reps: int, nfreq: int = 1):
        """dwh_bench_response_map_stages: (weight_ms, sample_ms) per launch of
        the weight kernel and of the sampled product for nfreq frequencies, on
        the buffers of the last measure_response_map call with a dmap."""
        tw, ts = C.c_double(), C.c_double()
        self._c(self._lib.dwh_bench_response_map_stages(self._h, int(reps), int(nfreq), C.byref(tw), C.byref(ts)))
        return tw.value, ts.value

    def timing_read(self, name: str):
        ms = C.c_double()
        n = C.c_int64()
        w = C.c_double()
        self._c(self._lib.dwh_timing_read(self._h, name.encode(), C.byref(ms), C.byref(n), C.byref(w)))
        return ms.value, n.value, w.value


def _nambu_csr(vx, vertices, N: int):
    """(rowptr, col, val (nops, nnz)) of the Nambu vertices of a call: a CSR
    tuple as given, else a collection (or one bare vertex) on its union pattern."""
    if isinstance(vertices, (vx.NambuVertex, vx.Vertex)):
        vertices = [vertices]                                  # one vertex passed bare
    # a CSR tuple is told by its content: an integer rowptr of 2N + 1 entries first
    first = vertices[0] if isinstance(vertices, tuple) and len(vertices) == 3 else None
    if first is not None and not isinstance(first, (tuple, list)) and np.ndim(first) == 1 \
            and len(first) == 2 * N + 1 and np.issubdtype(np.asarray(first).dtype, np.integer):
        return _csr_tuple(vertices, 2 * N, "vertices: a CSR tuple needs val (nops, {nnz})")
    vertices = list(vertices)
    if not vertices:
        raise ValueError("vertices is empty")
    return vx.union_csr_nambu(vertices, N)


def _csr_tuple(csr, nrows: int, message: str):
    """(rowptr, col, val (nops, nnz)) of a CSR tuple over nrows rows as the ABI
    takes them: contiguous int64, int64 and complex128.  message: the caller's
    ValueError text for a wrong shape ({n}: nrows + 1, {nnz}: len(col))."""
    rowptr = np.ascontiguousarray(csr[0], dtype=np.int64).ravel()
    col = np.ascontiguousarray(csr[1], dtype=np.int64).ravel()
    val = np.ascontiguousarray(np.atleast_2d(np.asarray(csr[2], dtype=np.complex128)))
    if len(rowptr) != nrows + 1 or val.ndim != 2 or val.shape[1] != len(col):
        raise ValueError(message.format(n=nrows + 1, nnz=len(col)))
    return rowptr, col, val


def _omega_grid(omega, eta):
    """(start, step, count) of a call's real-frequency grid: None (no grid: 0
    points), dict(start=, step=, count=) or (start, step, count); it needs eta."""
    if omega is None:
        return 0.0, 0.0, 0
    if isinstance(omega, dict):
        extra = set(omega) - {"start", "step", "count"}
        if extra:
            raise ValueError(f"omega: unknown keys {sorted(extra)}")
        omega = (omega["start"], omega["step"], omega["count"])
    grid = float(omega[0]), float(omega[1]), int(omega[2])
    if eta is None:
        raise ValueError("eta is needed with omega")
    return grid


def _per_state(deltas, scalars=(), **arrays) -> dict:
    """A call's (nstates, ...) results as it returns them: as they are with
    `deltas`, else (the one state at the device Δ) without the state axis,
    those named in `scalars` as floats."""
    if deltas is not None:
        return arrays
    return {k: a if a is None else float(a[0]) if k in scalars else a[0] for k, a in arrays.items()}


class _TransportOutputs:
    """The output arrays of a transport call for ns states (st, dc (ns,);
    sigma (ns, nw); dos, dos_an (ns, nd); ak (ns, N)) and, after the call,
    its result dicts."""

    def __init__(self, ctx, ns: int, eta, domega, omega_max):
        self.nw, self.nd = transport_grid(eta, domega, omega_max, ctx._lib)
        self.Lx, self.Ly = ctx.info_lattice
        self.grids = eta + domega * np.arange(self.nw), -omega_max + domega * np.arange(self.nd)
        self.st, self.dc = np.empty(ns), np.empty(ns)
        self.sigma, self.dos, self.dos_an = np.empty((ns, self.nw)), np.empty((ns, self.nd)), np.empty((ns, self.nd))
        self.ak = np.empty((ns, self.Lx * self.Ly))

    def results(self) -> list:
        """One dict per state, keys the SpectrumResult fields; every dict owns its arrays."""
        wg, dg = self.grids
        return [dict(superfluid_stiffness=float(self.st[k]), dc_conductivity=float(self.dc[k]), omega_grid=wg.copy(),
                     optical_conductivity=self.sigma[k].copy(), dos_omega_grid=dg.copy(), dos=self.dos[k].copy(),
                     dos_AN=self.dos_an[k].copy(), A_k_omega0=self.ak[k].reshape(self.Ly, self.Lx).T.copy())
                for k in range(len(self.st))]


def transport_grid(eta: float, domega: float, omega_max: float, lib=None):
    """(n_omega, n_dos): lengths of η:Δω:ω_max and -ω_max:Δω:ω_max as Julia
    counts them (dwh_transport_grid; host arithmetic, no device)."""
    lib = _lib.load() if lib is None else lib
    nw, nd = C.c_int64(), C.c_int64()
    check(lib.dwh_transport_grid(float(eta), float(domega), float(omega_max), C.byref(nw), C.byref(nd)))
    return nw.value, nd.value


def spectral_window(eta: float, domega: float, omega_max: float, first: int = 0, count: int | None = None,
                    stride: int = 1, lib=None) -> np.ndarray:
    """Frequencies of the window first + q·stride, q < count, of the DOS grid
    -ω_max:Δω:ω_max (dwh_spectral_window; host arithmetic, no device);
    count=None: up to the end of the grid.  ValueError if the window leaves
    the grid."""
    lib = _lib.load() if lib is None else lib
    first, stride = int(first), int(stride)
    if count is None:
        _, nd = transport_grid(eta, domega, omega_max, lib)
        count = (nd - 1 - first) // stride + 1 if 0 <= first < nd and stride >= 1 else 0
    count = int(count)
    omega = np.empty(max(count, 0))
    check(lib.dwh_spectral_window(float(eta), float(domega), float(omega_max), first, count, stride, ptr(omega)))
    return omega


def debug_current_vertex(Lx, Ly, t, tp, nn_table, nnn_table, direction="x", q=((0, 1),), lib=None) -> np.ndarray:
    """The Nambu vertices J_α(q) = Jq ⊕ Jq that measure_current_response
    uploads for this lattice (dwh_debug_current_vertex; host arithmetic, no
    device), dense: (nq, 2N, 2N)."""
    lib = _lib.load() if lib is None else lib
    if direction not in ("x", "y", 0, 1):
        raise ValueError("direction must be 'x' or 'y'")
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.int64).reshape(-1, 2))
    n2 = 2 * int(Lx) * int(Ly)
    out = np.empty((qa.shape[0], n2, n2), dtype=np.complex128)
    nn, nnn = table_to_abi(nn_table), table_to_abi(nnn_table)
    check(lib.dwh_debug_current_vertex(int(Lx), int(Ly), float(t), float(tp), ptr(nn), ptr(nnn),
                                       0 if direction in ("x", 0) else 1, qa.shape[0], ptr(qa), ptr(out)))
    return np.ascontiguousarray(np.transpose(out, (0, 2, 1)))   # (column-major on the ABI side)


CR_KINDS = {"inv": 0, "inv0": 1, "gemm": 2, "inv_side": 3}


def debug_cr_launch(kind: str, BP: int, pool: np.ndarray, ldpart: np.ndarray, blk=None, dst=None, slot=None,
                    rblk=None, inv32: bool = True, tasks=None, ts: int = 16, ksplit: int = 1, sg: float = 1.0,
                    device: int = 0, lib=None):
    """One launch of the library's CR launchers on a caller-supplied pool
    (dwh_debug_cr_launch).  pool: (nbatch, nblk, BP // 2, BP) complex top
    halves; ldpart: (nbatch, nslots); tasks: rows of 16 ints {out, cin, nt, bq,
    a[4], b[4], r0, r1, c0, c1}.  Returns (pool, ldpart) after the launch;
    ValueError (no launch) for anything the entry's validation refuses."""
    lib = _lib.load() if lib is None else lib
    pool = np.array(pool, dtype=np.complex128, order="C")
    ld = np.array(ldpart, dtype=np.float64, order="C")
    if pool.ndim != 4 or ld.ndim != 2 or ld.shape[0] != pool.shape[0]:
        raise ValueError("pool must be (nbatch, nblk, HP, BP) and ldpart (nbatch, nslots)")
    nbatch, nblk = pool.shape[:2]
    if pool.shape[2:] != (int(BP) // 2, int(BP)):
        raise ValueError("pool blocks must be (BP // 2, BP)")

    def ilist(a):
        return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))

    blk, dst, slot, rblk = ilist(blk), ilist(dst), ilist(slot), ilist(rblk)
    ninv = 0 if blk is None else len(blk)
    for a in (dst, slot, rblk):
        if a is not None and len(a) != ninv:
            raise ValueError("inversion lists must have one length")
    tk = None if tasks is None else np.ascontiguousarray(np.asarray(tasks, dtype=np.int32).reshape(-1, 16))
    check(lib.dwh_debug_cr_launch(int(device), CR_KINDS[kind], int(BP), nblk, nbatch, ld.shape[1], ptr(pool),
                                  ptr(ld), ninv, ptr(blk), ptr(rblk), ptr(dst), ptr(slot), int(bool(inv32)),
                                  0 if tk is None else len(tk), ptr(tk), int(ts), int(ksplit), float(sg)))
    return pool, ld


def selftest_mfma(device: int = 0) -> int:
    return int(_lib.load().dwh_selftest_mfma(int(device)))
