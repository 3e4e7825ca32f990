"""Response maps (dwh_measure_response_map, csrc/dwhmc_map.hip): the
linear-response density matrix of a source vertex W at a frequency z and the
equal-time density matrix, at the entries (a_e, b_e) of a sparse pattern,

    D(z)[W] = U (w(z) ∘ U^H W U) U^H,      ρ = U f U^H,

w the Matsubara weights of the Nambu cross response (its l = 0 rules) or the
retarded (f_n - f_m)/(ΔE_nm - ω - iη) with χ'''s |f_n - f_m| >= 1e-12 rule.

The reference is the numpy restatement tests/response_map_reference.py (MapRef,
whole matrices by the definition) on the oracle's `evaluate` eigenpairs, or in
long double on injected eigensystems.  Tolerances are the project's, from
tests/test_nambu_response.py: TOL = 1e-9 on real and imaginary parts separately,
`_close` for scalars, `_close_max` for arrays; the P_ij and hole-density
comparisons carry tests/test_gpu_parity.py's 1e-11.

CPU (not gpu): the identities of the restatement (D(0) = -∂ρ/∂ε against a
central difference of eigh, the contraction to chi and chi2, Tr D(l >= 1) = 0,
D(0)[H] in closed form, Hermiticity), vertices.py (bond_pattern, contract and
the three local maps against the current response's dia and Λ), the host-only
planner with its argument errors, the NULL-context refusal and the binding, and
the driver option on the oracle backend.  GPU: parity on lattices below a wave,
in the tail of a 64 tile, at one 256-row tile and one tile plus a tail, on the
bond pattern, a random pattern (duplicates, a column heavier than one
workgroup's slice, empty columns), one entry and the dense pattern; agreement
with the merged calls; injected eigensystems; the structure (repeat calls,
groups, chunks, snapshots, chains, algorithms, skipped parts, the timer, state
and workspace reuse) and the argument errors.
"""
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest

import measure_reference as R
from nambu_reference import LD
from response_map_reference import MapRef, OracleMap
from oracle_measurements import CurrentRef as _RefCurrent, simulate as _simulate
from test_current_response import SIM_KW, _case, _ctx
from test_nambu_response import ETA, TOL, _close, _close_max, _free, _injected_spectrum, _random_w, _vset

NL = 3
OMEGA = (-0.6, 0.0, 0.3)
SLICE = 32                       # entries per workgroup of the sampled product (kMapSlice)


@pytest.fixture(scope="module")
def VX(dwhmc):
    return dwhmc.vertices


_refs = {}


def _map_case(O, VX, Lx, Ly, beta=8.0):
    """(p, disorder, Δ, MapRef, vertices, dense) of a disordered lattice (test_nambu_response's seeds),
    once per module; the vertices: current, d-wave amplitude, Hamiltonian, random non-Hermitian."""
    key = (Lx, Ly, beta)
    if key not in _refs:
        p, dis, D = _case(O, Lx, Ly, beta, seed=4 if (Lx, Ly) == (2, 4) else Lx * 17 + Ly)
        vs = [_vset(VX, p, dis, D)[k] for k in (1, 3, 5, 6)]
        _refs[key] = (p, dis, D, MapRef.from_oracle(O, p, dis, D), vs, [v.dense(p.N) for _, v in vs])
    return _refs[key]


def _random_pattern(n2, seed):
    """unsorted, with duplicates, one column holding every row three times (3 · 2N > one workgroup's
    slice at every size here) and columns that hold nothing"""
    rng = np.random.default_rng(seed)
    cols = rng.choice(n2, size=max(2, n2 // 3), replace=False)
    heavy = int(cols[0])
    n = 4 * n2
    a, b = rng.integers(0, n2, n), cols[rng.integers(0, len(cols), n)]
    a[1], b[1] = a[0], b[0]
    a[-1], b[-1] = a[2], b[2]
    a = np.concatenate([a, np.tile(np.arange(n2), 3)])
    b = np.concatenate([b, np.full(3 * n2, heavy)])
    perm = rng.permutation(len(a))
    pat = np.stack([a[perm], b[perm]], axis=1).astype(np.int64)
    counts = np.bincount(pat[:, 1], minlength=n2)
    assert counts.max() > SLICE and (counts == 0).any() and len(np.unique(pat, axis=0)) < len(pat)
    return pat


# --------------------------------------------------------------------------- CPU: the restatement
def test_d0_is_minus_the_density_derivative(oracle, VX):
    """D(l = 0)[W] = -∂ρ/∂ε under H -> H + εW, Hermitian W, against the central
    difference of eigh at ε = 1e-5.  The bar is the difference's own error: its
    truncation, ε² ρ'''/6, is a third of |FD(2ε) - FD(ε)| (the leading term of
    Richardson's estimate), so that difference itself bounds it three times
    over; the rounding of two eigh density matrices, 2N eps each, divided by
    2ε, is added."""
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 4, 4)
    H, n2, eps = Ws[2], 2 * p.N, 1e-5
    f = lambda E: R.logistic(-p.beta * E)

    def rho_at(e, W):
        E, U = np.linalg.eigh(H + e * W)
        return (U * f(E)[None, :]) @ U.conj().T

    cases = [("current_x(0,0)", VX.nambu(VX.current(p, 0, 0, "x"), p.N).dense(p.N)), (vs[1][0], Ws[1])]
    for name, W in cases:
        assert np.abs(W - W.conj().T).max() <= 1e-15
        fd1 = (rho_at(eps, W) - rho_at(-eps, W)) / (2 * eps)
        fd2 = (rho_at(2 * eps, W) - rho_at(-2 * eps, W)) / (4 * eps)
        bar = np.abs(fd2 - fd1).max() + n2 * np.finfo(np.float64).eps / eps
        err = np.abs(ref.dmat(W, 1)[0] + fd1).max()
        print("D(0) + dρ/dε", name, err, "bar", bar)
        assert err <= bar and bar < 1e-7
        assert np.abs(fd1).max() > 1e-3


def test_contraction_is_the_cross_response(oracle, VX):
    """Σ_e conj(B_e) D_e = N chi(W, B) per Matsubara index; its imaginary part at ω + iη is N chi2 for B = W."""
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 6, 4, beta=4.0)
    n2 = 2 * p.N
    full = np.stack(np.meshgrid(np.arange(n2), np.arange(n2), indexing="ij"), -1).reshape(-1, 2)
    for a, b in ((0, 0), (0, 1), (3, 1), (2, 3)):
        Dm = ref.dmat(Ws[a], NL, OMEGA, ETA)
        got = VX.contract(full, Dm.reshape(len(Dm), -1), vs[b][1])
        _close(got[:NL], p.N * ref.chi(Ws[a], Ws[b], NL), ("chi", a, b))
        if a == b:
            _close_max(got[NL:].imag, p.N * ref.chi2(Ws[a], Ws[a], np.array(OMEGA), ETA).real, ("chi2", a))
    assert abs(ref.chi(Ws[0], Ws[1], NL)[1]) > 1e-6


def test_trace_closed_form_and_hermiticity(oracle, VX):
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 6, 4, beta=4.0)
    f = np.asarray(ref.f, dtype=np.float64)
    for k, W in enumerate(Ws):
        Dm = ref.dmat(W, NL)
        assert np.abs(np.trace(Dm[1:], axis1=1, axis2=2)).max() <= TOL, k       # Tr D(l >= 1) = 0
    want = (ref.U * (p.beta * f * (1 - f) * ref.E)[None, :]) @ ref.U.conj().T   # D(0)[H_BdG]
    DH = ref.dmat(Ws[2], NL)
    _close_max(DH[0], want, "D(0)[H]")
    assert np.abs(DH[1:]).max() <= TOL                                         # H is diagonal in its own basis
    J0 = VX.nambu(VX.current(p, 0, 0, "y"), p.N).dense(p.N)
    for k, W in enumerate((J0, Ws[1], Ws[2])):                                 # Hermitian W: D(0) is Hermitian
        assert np.abs(W - W.conj().T).max() <= 1e-15
        D0 = ref.dmat(W, 1)[0]
        _close_max(D0, D0.conj().T, ("hermitian", k))
    D0 = ref.dmat(Ws[3], 1)[0]
    assert np.abs(D0 - D0.conj().T).max() > 1e-3                               # not for the non-Hermitian one
    rho = ref.rho()
    _close_max(rho, rho.conj().T, "rho")
    _close(np.trace(rho).real, np.sum(f), "Tr rho")


# --------------------------------------------------------------------------- CPU: vertices.py
def test_bond_pattern(oracle, VX):
    p, _, _ = _case(oracle, 5, 7, 8.0, seed=5)
    N = p.N
    full = VX.bond_pattern(p)
    assert full.shape == (36 * N, 2) and full.dtype == np.int64 and full.flags["C_CONTIGUOUS"]
    assert len(np.unique(full, axis=0)) == 36 * N                              # no ring shorter than 3
    for k, (ra, cb) in enumerate((("pp", (0, 0)), ("hh", (1, 1)), ("ph", (0, 1)), ("hp", (1, 0)))):
        blk = VX.bond_pattern(p, blocks=(ra,))
        assert np.array_equal(blk, full[9 * N * k:9 * N * (k + 1)])
        assert np.all(blk[:, 0] // N == cb[0]) and np.all(blk[:, 1] // N == cb[1])
    site = VX.bond_pattern(p, ranges=("site",), blocks=("pp", "hh"))
    assert np.array_equal(site, np.stack([np.arange(2 * N)] * 2, 1))
    nn = VX.bond_pattern(p, ranges=("nn",), blocks=("ph",))
    assert nn.shape == (4 * N, 2)
    assert np.array_equal(nn[:, 1] - N, (np.asarray(p.nn_table) - 1).T.ravel())
    assert np.array_equal(nn[:, 0], np.tile(np.arange(N), 4))
    nnn = VX.bond_pattern(p, ranges=("nnn",), blocks=("pp",))
    assert np.array_equal(nnn[:, 1], (np.asarray(p.nnn_table) - 1).T.ravel())
    p2, _, _ = _case(oracle, 2, 4, 8.0, seed=4)                                # Lx = 2: +x and -x coincide
    small = VX.bond_pattern(p2)
    assert small.shape == (36 * p2.N, 2) and len(np.unique(small, axis=0)) < 36 * p2.N
    for bad in (dict(ranges=("bond",)), dict(blocks=("up",)), dict(ranges=()), dict(blocks=())):
        with pytest.raises(ValueError):
            VX.bond_pattern(p, **bad)


def test_contract_sums_duplicates_and_refuses_uncovered(oracle, VX):
    p, _, _ = _case(oracle, 4, 4, 8.0, seed=3)
    N = p.N
    pat = np.array([[0, 1], [2, 2], [N, 3], [0, 1], [5, N + 5]], dtype=np.int64)
    D = np.arange(1, 11).reshape(2, 5) * (1 + 0.5j)
    B = VX.NambuVertex(np.array([0, N, 0]), np.array([1, 3, 1]), np.array([1 + 1j, 2.0, 0.5]))
    want = np.conj(1.5 + 1j) * D[:, 0] + 2.0 * D[:, 2]                       # duplicates of B summed, first copy of (0, 1)
    assert np.allclose(VX.contract(pat, D, B, N), want, rtol=0, atol=1e-15)
    assert np.allclose(VX.contract(pat, D[1], B), want[1], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="not in the pattern"):
        VX.contract(pat, D, VX.NambuVertex(np.array([0, 1]), np.array([1, 0]), np.ones(2)), N)
    with pytest.raises(ValueError):
        VX.contract(VX.bond_pattern(p, ranges=("site",)), np.zeros(4 * N), VX.current(p, 0, 0, "x"), N)
    with pytest.raises(ValueError):
        VX.contract(pat, D, VX.density(p))                                      # a Vertex needs N
    dens = VX.contract(VX.bond_pattern(p, ranges=("site",)), np.ones(4 * N), VX.density(p), p)
    assert abs(dens) <= 1e-15                                                  # Σ_i (1 - 1): particle minus hole block


@pytest.mark.parametrize("Lx,Ly", [(4, 4), (6, 4)])
@pytest.mark.parametrize("a", ["x", "y"])
def test_local_maps_sum_to_the_current_response(oracle, VX, Lx, Ly, a):
    """(1/N) Σ_i of dia_i, Λ_i and their difference are dia, Λ(q = 0, l = 0) and the stiffness."""
    p, dis, D, ref, _, _ = _map_case(oracle, VX, Lx, Ly)
    old = _RefCurrent(oracle, p, dis, D)
    pat = VX.bond_pattern(p, blocks=("pp", "hh"))
    dmap, rho = ref.response([VX.nambu(VX.current(p, 0, 0, a), p.N).dense(p.N)], pat, 1)
    dia, lam = VX.diamagnetic_map(p, pat, rho, a), VX.paramagnetic_map(p, pat, dmap[0, 0], a)
    st = VX.stiffness_map(p, pat, rho, dmap[0, 0], a)
    assert dia.shape == lam.shape == st.shape == (p.N,)
    want_dia, want_lam = old.dia(a), old.lam(a, [(0, 0)], 1)[0, 0]
    print(a, "dia", dia.mean(), want_dia, "lam", lam.mean(), want_lam)
    _close(dia.mean(), want_dia, "dia")
    _close(lam.mean(), want_lam, "lam")
    _close(st.mean(), want_dia - want_lam, "stiffness")
    assert dia.std() > 1e-3 and lam.std() > 1e-4                               # disorder: the maps are not flat
    with pytest.raises(ValueError):
        VX.paramagnetic_map(p, VX.bond_pattern(p, ranges=("site",)), dmap[0, 0][:4 * p.N], a)
    with pytest.raises(ValueError):
        VX.diamagnetic_map(p, pat, rho, "z")


# --------------------------------------------------------------------------- CPU: planner, refusals, binding
def _plan(lib, N, pat, npat=None, prow=True, pcol=True, order=True, colptr=True):
    pat = np.ascontiguousarray(np.asarray(pat, dtype=np.int64).reshape(-1, 2))
    a, b = np.ascontiguousarray(pat[:, 0]), np.ascontiguousarray(pat[:, 1])
    npat = len(pat) if npat is None else npat
    o, cp = np.full(max(len(pat), 1), -7, dtype=np.int64), np.full(2 * min(max(N, 0), 64) + 1, -7, dtype=np.int64)
    P = lambda x, on: x.ctypes.data_as(C.c_void_p) if on else None
    rc = lib.dwh_debug_response_map_plan(N, npat, P(a, prow), P(b, pcol), P(o, order), P(cp, colptr))
    return rc, o, cp


def _check_plan(N, pat, order, colptr):
    n2, pat = 2 * N, np.asarray(pat)
    assert sorted(order) == list(range(len(pat)))                              # a permutation
    assert colptr[0] == 0 and colptr[-1] == len(pat) and np.all(np.diff(colptr) >= 0)
    assert np.array_equal(np.diff(colptr), np.bincount(pat[:, 1], minlength=n2))
    for b in range(n2):
        grp = order[colptr[b]:colptr[b + 1]]
        assert np.all(pat[grp, 1] == b) and np.all(np.diff(grp) > 0), b       # grouped by b, stable inside


def test_planner(dwhmc, oracle, VX):
    lib = dwhmc.load_library()
    p, _, _ = _case(oracle, 2, 4, 8.0, seed=4)
    n2 = 2 * p.N
    pats = [_random_pattern(n2, 1), VX.bond_pattern(p), np.array([[3, n2 - 2]]),
            np.stack(np.meshgrid(np.arange(n2), np.arange(n2), indexing="ij"), -1).reshape(-1, 2)[::-1]]
    for pat in pats:
        rc, order, colptr = _plan(lib, p.N, pat)
        assert rc == 0, lib.dwh_last_error(None)
        _check_plan(p.N, pat, order, colptr)
    assert np.array_equal(_plan(lib, p.N, pats[0])[1], np.argsort(pats[0][:, 1], kind="stable"))


def test_planner_argument_errors(dwhmc):
    lib = dwhmc.load_library()
    N, good = 3, [[0, 1], [5, 5], [2, 0]]
    assert _plan(lib, N, good)[0] == 0
    cases = [(dict(N=0), b"N must be"), (dict(N=(1 << 24) + 1), b"N must be"), (dict(npat=0), b"npat"),
             (dict(npat=-1), b"npat"), (dict(npat=(1 << 24) + 1), b"npat"), (dict(prow=False), b"NULL"),
             (dict(pcol=False), b"NULL"), (dict(order=False), b"NULL"), (dict(colptr=False), b"NULL"),
             (dict(pat=[[0, 1], [6, 0]]), b"outside"), (dict(pat=[[0, -1]]), b"outside"),
             (dict(pat=[[-1, 0]]), b"outside"), (dict(pat=[[0, 6]]), b"outside")]
    for kw, text in cases:
        args = dict(N=N, pat=good)
        args.update(kw)
        rc, order, colptr = _plan(lib, args.pop("N"), args.pop("pat"), **args)
        assert rc == -1, kw
        assert text in lib.dwh_last_error(None), (kw, lib.dwh_last_error(None))
        assert np.all(order == -7) and np.all(colptr == -7), kw                # nothing written


def test_null_context_is_refused_and_binding(dwhmc):
    lib = dwhmc.load_library()
    buf = np.zeros(16)
    rowptr, col = np.zeros(3, dtype=np.int64), np.zeros(1, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_measure_response_map(None, 0, 1, None, 1, p(rowptr), p(col), 1, p(buf), 1, p(col), p(col), 1, 0.1,
                                      0, None, p(buf), p(buf))
    assert rc == -1
    assert b"NULL" in lib.dwh_last_error(None)
    sig = import_module(dwhmc.__name__ + "._lib").SIGNATURES
    assert "dwh_measure_response_map" in sig and "dwh_debug_response_map_plan" in sig
    assert len(sig["dwh_measure_response_map"][1]) == 18 and len(sig["dwh_debug_response_map_plan"][1]) == 6
    assert dwhmc.FermionContext.TIMERS.index("map") == 16


# --------------------------------------------------------------------------- CPU: the driver option
SIM_V = [("current_x", (0, 0)), ("pair_d_amplitude", (0, 0))]
SIM_OPT = dict(vertices=SIM_V, pattern=dict(ranges=("site", "nn"), blocks=("pp", "ph")), n_matsubara=2,
               omega=[-0.2, 0.1], eta=0.1)
SIM_NPAT = 2 * 5 * 16                                                           # 2 blocks x (site + 4 nn) x N


def _check_sim_outputs(with_opt, without, dwhmc):
    spec = "spectra_bins"
    assert not (without / spec / "response_map_pattern.npy").exists()
    for f in ("observables.csv", "transport.csv"):
        assert (with_opt / f).read_bytes() == (without / f).read_bytes(), f
    for f in ("params.json", "omega_grid.npy"):
        assert (with_opt / spec / f).read_bytes() == (without / spec / f).read_bytes(), f
    assert sorted(os.listdir(with_opt / spec)) == sorted(os.listdir(without / spec) + ["response_map_pattern.npy"])
    assert sorted(os.listdir(with_opt)) == sorted(os.listdir(without))
    p = dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)
    pat = np.load(with_opt / spec / "response_map_pattern.npy")
    assert np.array_equal(pat, dwhmc.vertices.bond_pattern(p, ranges=("site", "nn"), blocks=("pp", "ph")))
    assert pat.shape == (SIM_NPAT, 2)
    bins = sorted(f for f in os.listdir(with_opt / spec) if f.startswith("sweep_"))
    assert len(bins) == SIM_KW["n_measure"] // SIM_KW["bin_size"]
    out = []
    for f in bins:
        a, b = np.load(with_opt / spec / f), np.load(without / spec / f)
        assert sorted(a.files) == sorted(b.files + ["response_map", "rho_map"])
        dm, rho = a["response_map"], a["rho_map"]
        assert dm.shape == (2, 4, SIM_NPAT) and dm.dtype == np.complex128 and np.all(np.isfinite(dm))
        assert rho.shape == (SIM_NPAT,) and rho.dtype == np.complex128 and np.all(np.isfinite(rho))
        assert np.abs(rho[:16].imag).max() <= 1e-12 and np.all(rho[:16].real > 0) and np.all(rho[:16].real < 1)
        assert np.abs(dm).max() > 1e-3
        for k in b.files:
            assert np.array_equal(a[k], b[k]), k
        out.append((dm, rho))
    return out


@pytest.mark.parametrize("tb", [1, 3])
def test_simulation_option_on_oracle(dwhmc, tmp_path, tb):
    """run_simulation(response_map=...) on the oracle backend: dmap and ρ in
    the bins through TransportQueue's batches, the pattern written once; the
    other files are unchanged; nothing appears without the option."""
    _simulate(dwhmc, tmp_path / "with", OracleMap, response_map=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", OracleMap, transport_batch=tb, **SIM_KW)
    got = _check_sim_outputs(tmp_path / "with", tmp_path / "without", dwhmc)
    if tb == 1:
        _simulate(dwhmc, tmp_path / "b3", OracleMap, response_map=SIM_OPT, transport_batch=3, **SIM_KW)
        for (dm, rho), (dm3, rho3) in zip(got, _check_sim_outputs(tmp_path / "b3", tmp_path / "without", dwhmc)):
            assert dm.tobytes() == dm3.tobytes() and rho.tobytes() == rho3.tobytes()
    assert np.abs(got[0][1] - got[1][1]).max() > 1e-9                       # the sweeps' own Δ, not one state's


@pytest.mark.parametrize("tb", [1, 2])
def test_simulation_chains_option_on_oracle(dwhmc, tmp_path, tb):
    _simulate(dwhmc, tmp_path / "with", OracleMap, chains=2, response_map=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", OracleMap, chains=2, transport_batch=tb, **SIM_KW)
    for k in range(2):
        _check_sim_outputs(tmp_path / "with" / f"c{k}", tmp_path / "without" / f"c{k}", dwhmc)


def test_simulation_default_is_unchanged_and_unknown_keys_raise(dwhmc, tmp_path):
    """Without the option every file is what a run writes when the option does
    not exist at all (the oracle context that knows nothing of it); unknown
    keys and unusable values raise, for one chain and for several."""
    from oracle_context import OracleContext
    _simulate(dwhmc, tmp_path / "plain", OracleContext, **SIM_KW)
    _simulate(dwhmc, tmp_path / "none", OracleMap, response_map=None, **SIM_KW)
    for root, _, files in os.walk(tmp_path / "plain"):
        for f in files:
            if f == "simulation.log":                                            # (timestamps)
                continue
            a = os.path.join(root, f)
            b = os.path.join(tmp_path / "none", os.path.relpath(a, tmp_path / "plain"))
            assert open(a, "rb").read() == open(b, "rb").read(), f
    assert sorted(os.listdir(tmp_path / "plain" / "spectra_bins")) == sorted(os.listdir(tmp_path / "none" / "spectra_bins"))
    for k, opt in enumerate((dict(vertices=SIM_V, pairs=[(0, 0)]), dict(vertices=[("charge", (0, 0))]),
                             dict(vertices=[]), dict(pattern=dict(ranges=("site",), block=("pp",))),
                             dict(pattern=dict(ranges=("bond",))), dict(pattern=[[0, 32]]), dict(pattern=[0, 1]),
                             dict(pattern=np.zeros((0, 2), dtype=np.int64)), dict(n_matsubara=0),
                             dict(n_matsubara=-1, omega=[0.1]))):
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"a{k}", OracleMap, response_map=opt, **SIM_KW)
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"b{k}", OracleMap, chains=2, response_map=opt, **SIM_KW)


# --------------------------------------------------------------------------- GPU
def _measure(ctx, vs, pat, nl=NL, omega=OMEGA, eta=ETA, **kw):
    return ctx.measure_response_map([v for _, v in vs], pat, n_matsubara=nl, omega=omega, eta=eta, **kw)


def _check_parity(got, ref, Ws, pat, what, nl=NL, omega=OMEGA):
    dmap, rho = ref.response(Ws, pat, nl, omega, ETA)
    assert got["dmap"].shape == dmap.shape and got["dmap"].dtype == np.complex128, what
    assert got["rho"].shape == rho.shape and got["rho"].dtype == np.complex128, what
    for k in range(len(Ws)):
        print(what, "vertex", k, "max|ΔD|", float(np.abs(got["dmap"][k] - dmap[k]).max()), "max|D|",
              float(np.abs(dmap[k]).max()))
    print(what, "max|Δρ|", float(np.abs(got["rho"] - rho).max()))
    for k in range(len(Ws)):
        for z in range(dmap.shape[1]):
            _close_max(got["dmap"][k, z], dmap[k, z], (what, "dmap", k, z))
    _close_max(got["rho"], rho, (what, "rho"))


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(2, 4), (6, 4), (8, 16), (12, 12)])
def test_parity_with_numpy(dwhmc, oracle, VX, Lx, Ly):
    """2N = 16 (below one wave's rows), 48 (the tail of a 64 tile), 256 (exactly
    one 256-row tile), 288 (one tile plus a tail); the bond pattern, the random
    pattern, one entry and, at 2 x 4, every entry of the matrix."""
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, Lx, Ly)
    n2 = 2 * p.N
    pats = {"bond": VX.bond_pattern(p), "random": _random_pattern(n2, n2), "single": np.array([[3, n2 - 2]])}
    if (Lx, Ly) == (2, 4):
        pats["dense"] = np.stack(np.meshgrid(np.arange(n2), np.arange(n2), indexing="ij"), -1).reshape(-1, 2)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = {k: _measure(ctx, vs, pat) for k, pat in pats.items()}
    ctx.close()
    for k, pat in pats.items():
        assert np.array_equal(got[k]["pattern"], pat) and np.array_equal(got[k]["omega"], OMEGA)
        _check_parity(got[k], ref, Ws, pat, ((Lx, Ly), k))
    if "dense" in pats:
        whole = ref.dmat(Ws[3], NL, OMEGA, ETA)
        _close_max(got["dense"]["dmap"][3].reshape(whole.shape), whole, "the whole matrix")


@pytest.mark.gpu
def test_agrees_with_the_merged_calls(dwhmc, oracle, VX):
    """On one context: the contraction is N chi (and N chi2 for a = b) of
    measure_nambu_response, the maps' means are measure_current_response's dia
    and Λ(q = 0), ρ gives pairing()'s P_ij and hole_trace()."""
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 6, 4)
    N = p.N
    pat = VX.bond_pattern(p)
    pairs = [(0, 0), (1, 1), (0, 1)]
    w = (-0.6, 0.3, 3)                                                          # start, step, count: -0.6, -0.3, 0.0
    wl = R.grid(*w)
    cur = {a: VX.nambu(VX.current(p, 0, 0, a), N) for a in "xy"}
    ctx = _ctx(dwhmc, p, dis, algo="cr")
    ctx.set_pairing(D)
    ctx.factorize()
    P, hole = ctx.pairing()[0], ctx.hole_trace()[0]
    old = ctx.measure_nambu_response([v for _, v in vs[:2]], pairs, n_matsubara=NL, omega=w, eta=ETA)
    new = ctx.measure_response_map([v for _, v in vs[:2]], pat, n_matsubara=NL, omega=wl, eta=ETA)
    resp = {a: ctx.measure_current_response(direction=a, q=[(0, 0)], n_matsubara=1) for a in "xy"}
    maps = ctx.measure_response_map([cur["x"], cur["y"]], pat, n_matsubara=1)
    ctx.close()
    for k, (a, b) in enumerate(pairs):
        got = VX.contract(pat, new["dmap"][a], vs[b][1], N)
        _close(got[:NL], N * old["chi"][k], ("chi", a, b))
        if a == b:
            _close_max(got[NL:].imag, N * old["chi2"][k].real, ("chi2", a))
    for k, a in enumerate("xy"):
        dia = VX.diamagnetic_map(p, pat, maps["rho"], a)
        lam = VX.paramagnetic_map(p, pat, maps["dmap"][k, 0], a)
        print(a, dia.mean(), resp[a]["dia"], lam.mean(), resp[a]["lam"][0, 0])
        _close(dia.mean(), resp[a]["dia"], ("dia", a))
        _close(lam.mean(), resp[a]["lam"][0, 0], ("lam", a))
        _close(VX.stiffness_map(p, pat, maps["rho"], maps["dmap"][k, 0], a).mean(),
               resp[a]["dia"] - resp[a]["lam"][0, 0], ("stiffness", a))
    rho = new["rho"]
    i = np.arange(N)
    for d in range(2):                                                          # P_ij = -ρ[i, j+N] - ρ[j, i+N]
        j = np.asarray(p.nn_table)[:, d] - 1
        Pd = -rho[VX._pattern_index(pat, 2 * N, i, j + N, "P")] - rho[VX._pattern_index(pat, 2 * N, j, i + N, "P")]
        print("P", d, float(np.abs(Pd - P[:, d]).max()))
        assert np.abs(Pd - P[:, d]).max() <= 1e-11
    tr = np.sum(rho[VX._pattern_index(pat, 2 * N, i + N, i + N, "Tr")])
    print("Tr rho_hh", tr, hole)
    assert abs(tr.imag) <= 1e-11 and abs(2.0 * tr.real / N - 2.0 * hole / N) <= 1e-11


def _map_spectrum(n2, beta):
    """test_nambu_response's injected spectrum (a cluster of four within 1e-9:
    the l = 0 rule) with two levels so far above the Fermi level that their
    f_n - f_m is below 1e-12 (the retarded skip)"""
    E = _injected_spectrum(n2, beta)
    E[-3], E[-2] = 5.0, 5.5
    E = np.sort(E)
    br = R.Branches(E, beta)
    assert not br.ambiguous_df().any()
    off = ~np.eye(n2, dtype=bool)
    assert (br.deg & off).any() and (~br.keep & off).any()
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (5, 7)])
def test_injected_eigensystems(dwhmc, oracle, VX, Lx, Ly):
    """A Haar U, which diagonalises nothing, and a prescribed spectrum with an
    exactly degenerate cluster and a pair below the Δf rule
    (debug_set_eigensystem), against the long double restatement."""
    beta = 8.0
    p, dis, D = _free(oracle, VX, Lx, Ly, beta=beta)
    n2 = 2 * p.N
    E, U = _map_spectrum(n2, beta), R.haar(n2, 11 + n2)
    vs = [("d amplitude", VX.pair_field(p, 0, 0, "d", "amplitude")), ("random", _random_w(VX, p.N, 3)),
          ("current_x", VX.nambu(VX.current(p, 0, 0, "x"), p.N))]
    Ws = [v.dense(p.N) for _, v in vs]
    pat = np.concatenate([VX.bond_pattern(p), _random_pattern(n2, 7)])
    ref = MapRef(p, E, U, beta=beta, dt=LD)
    ctx = _ctx(dwhmc, p, dis, algo="eig")
    ctx.debug_set_eigensystem(E, U)
    got = _measure(ctx, vs, pat)
    ctx.close()
    _check_parity(got, ref, Ws, pat, ("injected", Lx, Ly))


@pytest.mark.gpu
def test_structure(dwhmc, oracle, VX, monkeypatch):
    """Repeat calls, one vertex per group and one frequency per chunk give the
    same bits; 3 snapshots equal their single-state calls; chain 1 of a
    2-chain context; dmap only and rho only; the context's Δ is unchanged."""
    O = oracle
    p, dis, D, ref, vs, Ws = _map_case(O, VX, 6, 4)
    vs, Ws = [vs[0], vs[1], vs[3]], [Ws[0], Ws[1], Ws[3]]                    # (the hamiltonian vertex belongs to one Δ)
    pat = np.concatenate([VX.bond_pattern(p, blocks=("pp", "ph")), _random_pattern(2 * p.N, 3)])
    p2, dis2, D2 = _case(O, 6, 4, 8.0, seed=77)
    rng = np.random.default_rng(8)
    fields = np.stack([D2, D2 * np.exp(0.1j), D2 + 0.05 * rng.standard_normal(D2.shape)])
    ctx = _ctx(dwhmc, p, np.stack([dis, dis2]))
    ctx.set_pairing(np.stack([D, D2]))
    before, _ = ctx.get_state()
    try:
        one = _measure(ctx, vs, pat)
        again = _measure(ctx, vs, pat)
        monkeypatch.setenv("DWHMC_RESPONSE_GROUP", "1")
        grouped = _measure(ctx, vs, pat)
        monkeypatch.delenv("DWHMC_RESPONSE_GROUP")
        monkeypatch.setenv("DWHMC_MAP_CHUNK", "1")
        chunked = _measure(ctx, vs, pat)
        monkeypatch.delenv("DWHMC_MAP_CHUNK")
        for r in (again, grouped, chunked):
            assert r["dmap"].tobytes() == one["dmap"].tobytes() and r["rho"].tobytes() == one["rho"].tobytes()
        _check_parity(one, ref, Ws, pat, "chain 0")
        r3 = _measure(ctx, vs, pat, chain=1, deltas=fields)
        ones = [_measure(ctx, vs, pat, chain=1, deltas=fields[s:s + 1]) for s in range(3)]
        dev1 = _measure(ctx, vs, pat, chain=1)                               # the device Δ of chain 1 = fields[0]
        assert r3["dmap"].shape == (3, len(vs), NL + len(OMEGA), len(pat)) and r3["rho"].shape == (3, len(pat))
        for k in ("dmap", "rho"):
            for s in range(3):
                assert ones[s][k][0].tobytes() == r3[k][s].tobytes(), (k, s)
            assert dev1[k].tobytes() == r3[k][0].tobytes(), k
        for s, Ds in ((0, D2), (2, fields[2])):
            _check_parity(dict(dmap=r3["dmap"][s], rho=r3["rho"][s]), MapRef.from_oracle(O, p2, dis2, Ds), Ws, pat,
                          ("chain 1 snapshot", s))
        only_d = _measure(ctx, vs, pat, rho=False)
        only_r = _measure(ctx, vs, pat, nl=0, omega=None)
        only_l = _measure(ctx, vs, pat, omega=None)
        only_w = _measure(ctx, vs, pat, nl=0)
        assert only_d["rho"] is None and only_d["dmap"].tobytes() == one["dmap"].tobytes()
        assert only_r["dmap"] is None and only_r["rho"].tobytes() == one["rho"].tobytes()
        assert only_l["dmap"].tobytes() == one["dmap"][:, :NL].tobytes()
        assert only_w["dmap"].tobytes() == one["dmap"][:, NL:].tobytes()
        after, _ = ctx.get_state()
        assert np.array_equal(before, after)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dense", "cr", "eig"])
def test_algorithms(dwhmc, oracle, VX, algo):
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 6, 4)
    pat = VX.bond_pattern(p)
    ctx = _ctx(dwhmc, p, dis, algo=algo)
    ctx.set_pairing(D)
    assert ctx.info["algo"] == {"dense": 0, "cr": 1, "eig": 2}[algo]
    got = _measure(ctx, vs, pat)
    ctx.close()
    _check_parity(got, ref, Ws, pat, algo)


@pytest.mark.gpu
def test_timer_and_workspace_reuse(dwhmc, oracle, VX):
    """One "map" record per state with the stated work; the other measurements
    return the same bytes before and after the new entry ran on the context."""
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 6, 4)
    pat = VX.bond_pattern(p)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    ops = [VX.density(p, 1, 0), VX.raman_b1g(p)]

    def others():
        r = ctx.measure_current_response(direction="y", q=[(0, 0), (1, 2)], n_matsubara=NL)
        t = ctx.measure_transport(0.01, 0.002, 4.0)
        o = ctx.measure_operator_response(ops, n_matsubara=NL, omega=(-0.6, 0.3, 5), eta=ETA)
        n = ctx.measure_nambu_response([v for _, v in vs], [(0, 1), (3, 3)], n_matsubara=NL, omega=(-0.6, 0.3, 5),
                                       eta=ETA)
        return [np.float64(r["dia"]).tobytes(), r["lam"].tobytes(), o["chi"].tobytes(), o["chi2"].tobytes(),
                n["chi"].tobytes(), n["chi2"].tobytes()] + [
            np.asarray(t[k]).tobytes() for k in ("superfluid_stiffness", "dc_conductivity", "optical_conductivity",
                                                 "dos", "dos_AN", "A_k_omega0")]

    try:
        before = others()
        with pytest.raises(dwhmc.DwhError):
            ctx.bench_response_map_stages(1)                                  # (no response map has run yet)
        ctx.timing_enable(["map"])
        _measure(ctx, vs, pat)
        tw, ts = ctx.bench_response_map_stages(2, NL + len(OMEGA))             # the bench entry, on that call's buffers
        assert tw > 0 and ts > 0
        with pytest.raises(ValueError):
            ctx.bench_response_map_stages(1, NL + len(OMEGA) + 1)
        after = others()
        _measure(ctx, vs[:2], pat, nl=1, omega=None, deltas=np.stack([D, D, D]))
        _measure(ctx, vs[:2], pat, nl=0, omega=None)                          # rho only: no product
        after2 = others()
        ms, launches, work = ctx.timing_read("map")
        nam = ctx.timing_read("nambu")
    finally:
        ctx.close()
    assert before == after == after2
    n3 = 8.0 * (2 * p.N) ** 3
    assert launches == 1 + 3 + 1 and ms > 0
    assert work == n3 * (len(vs) * (1 + NL + len(OMEGA)) + 3 * 2 * (1 + 1))
    assert nam[1] == 0


@pytest.mark.gpu
def test_argument_errors(dwhmc, oracle, VX):
    """Each DWH_ERR_ARG case launches nothing (the outputs keep their fill) and leaves the context usable."""
    p, dis, D, ref, vs, Ws = _map_case(oracle, VX, 2, 4)
    pat = VX.bond_pattern(p, blocks=("pp",))
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    try:
        full = _measure(ctx, vs, pat)
        lib, h = ctx._lib, ctx._h
        rowptr, col, val = VX.union_csr_nambu([v for _, v in vs], p.N)
        a, b = np.ascontiguousarray(pat[:, 0]), np.ascontiguousarray(pat[:, 1])
        w = np.array(OMEGA)
        nz = NL + len(w)
        fill = np.nan + 0j
        o_r, o_d = np.full(len(pat), fill), np.full(len(vs) * nz * len(pat), fill)
        P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

        def call(chain=0, ns=1, nops=len(vs), rp=rowptr, cl=col, nnz=len(col), vl=val, npat=len(pat), pr=a, pc=b,
                 nl=NL, eta=ETA, nw=len(w), om=w, rho=o_r, dm=o_d):
            return lib.dwh_measure_response_map(h, chain, ns, None, nops, P(rp), P(cl), nnz, P(vl), npat, P(pr), P(pc),
                                                nl, eta, nw, P(om), P(rho), P(dm))

        bad_col = col.copy()
        bad_col[0] = 2 * p.N
        bad_rp = rowptr.copy()
        bad_rp[1], bad_rp[2] = rowptr[2] + 1, rowptr[1]
        hi, lo = a.copy(), b.copy()
        hi[3], lo[0] = 2 * p.N, -1
        for kw in (dict(chain=1), dict(chain=-1), dict(ns=2), dict(ns=0), dict(nops=0), dict(nnz=0),
                   dict(nnz=len(col) - 1), dict(rp=bad_rp), dict(cl=bad_col), dict(rp=None), dict(cl=None),
                   dict(vl=None), dict(npat=0), dict(npat=-1), dict(pr=hi), dict(pc=lo), dict(pr=None), dict(pc=None),
                   dict(nl=-1), dict(nw=-1), dict(nl=0, nw=0), dict(rho=None, dm=None), dict(om=None),
                   dict(eta=0.0), dict(eta=-0.1), dict(eta=float("nan")), dict(eta=float("inf")),
                   dict(om=np.array([0.0, float("nan"), 0.1])), dict(om=np.array([float("inf"), 0.0, 0.1]))):
            assert call(**kw) == -1, kw
            assert lib.dwh_last_error(h), kw
            assert np.all(np.isnan(o_r)) and np.all(np.isnan(o_d)), kw
        assert call(nl=0, nw=0, dm=None) == 0 and not np.any(np.isnan(o_r))   # no frequency is fine without dmap
        assert o_r.tobytes() == full["rho"].tobytes()
        assert call(nw=0, om=None, eta=0.0) == 0                              # eta is unused without real frequencies
        assert call() == 0
        assert o_d.reshape(full["dmap"].shape).tobytes() == full["dmap"].tobytes()
        for kw in (dict(omega=OMEGA, eta=None), dict(omega=OMEGA, eta=0.0), dict(chain=1), dict(n_matsubara=-1),
                   dict(n_matsubara=0, omega=None, rho=False)):
            args = dict(n_matsubara=NL, omega=None, eta=ETA)
            args.update(kw)
            with pytest.raises(ValueError):
                ctx.measure_response_map([v for _, v in vs], pat, **args)
        for bad in (pat[:, 0], pat.astype(np.float64), np.array([[0, 2 * p.N]]), np.zeros((0, 2), dtype=np.int64)):
            with pytest.raises(ValueError):
                ctx.measure_response_map([v for _, v in vs], bad)
        _check_parity(_measure(ctx, vs, pat), ref, Ws, pat, "after errors")
    finally:
        ctx.close()
