"""Equal-time correlations of local operators (dwh_measure_correlations,
csrc/dwhmc_corr.hip): by Wick's theorem from the full ρ = U f U^H,

    G_AB(i, j) = <O_A(i) O_B(j)†> - <O_A(i)><O_B(j)†>,
    corr[r] = (1/N) Σ_j G(j ⊕ r, j),  local[q][r] = G(ref_q ⊕ r, ref_q),  mean = <O_A(i)>.

The reference is tests/correlation_reference.py (CorrRef, the definition with
a loop over the terms) on the oracle's `evaluate` eigenpairs, or in long double
on injected eigensystems.  Tolerances are the project's, from
tests/test_nambu_response.py: TOL = 1e-9 on real and imaginary parts
separately, `_close` for scalars, `_close_max` for arrays; the P_ij and hole
trace comparisons carry tests/test_gpu_parity.py's 1e-11.

The contraction kernel's constants (csrc/dwhmc_internal.h): TILE = 256
displacements per workgroup (kCorrTile), CHUNK = 16 sites j per workgroup
(kCorrChunk).  The GPU lattices: 4x2 (N = 8: below a wave, below a chunk),
6x4 (24: Lx != Ly, one chunk and a tail), 10x6 (60: a wave's tail, three
chunks and a tail), 16x16 (256: one tile, 16 chunks), 18x16 (288: a tile and
a tail, 18 chunks) and 18x15 (270: a tile and a tail, 16 chunks and a tail).

CPU (not gpu): CorrRef against a Fock-space thermal average, the lattice sum,
vertices.py (local_family, structure_factor, disconnected), translation
invariance on a clean lattice, the host-only expansion with every refusal, the
NULL-context refusal and the binding, and the driver option on the oracle
backend (OracleCorrelations).
"""
import ctypes as C
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import measure_reference as R
from correlation_reference import CorrRef, FockThermal, OracleCorrelations, translate_table
from nambu_reference import LD
from oracle_measurements import simulate as _simulate
from test_current_response import SIM_KW, _case, _clean, _ctx
from test_nambu_response import TOL, _close, _close_max, _free, _injected_spectrum

TILE, CHUNK, MAX_TERMS = 256, 16, 64
KINDS = ["density", "spin", "pair_d_create", "pair_d_amplitude", "current_x"]
# families 0 .. 4 = KINDS, 5 = random; (k, k) and mixed
PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (0, 2), (3, 0), (5, 0), (2, 5), (4, 3)]
PAIRS_BIG = [(0, 0), (2, 2), (3, 3), (4, 1), (5, 5), (0, 5), (5, 3)]           # N >= 256: fewer random pairs
GPU_LATTICES = [(4, 2), (6, 4), (10, 6), (16, 16), (18, 16), (18, 15)]


@pytest.fixture(scope="module")
def VX(dwhmc):
    return dwhmc.vertices


def _random_family(VX, N, seed):
    """0 .. 64 terms per site, site 0 empty and site 1 at the cap, all four
    Nambu blocks, indices anywhere, duplicates, complex values, unsorted"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, MAX_TERMS + 1, N)
    cnt[0] = 0
    if N > 1:
        cnt[1] = MAX_TERMS
    site = np.repeat(np.arange(N), cnt)
    n = len(site)
    row, col = rng.integers(0, 2 * N, n), rng.integers(0, 2 * N, n)
    for blk, (br, bc) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):          # every block is there
        row[blk], col[blk] = br * N + rng.integers(N), bc * N + rng.integers(N)
    row[5], col[5] = row[4], col[4]                                            # a duplicate at one site (site 1)
    val = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    perm = rng.permutation(n)
    return VX.LocalFamily(site[perm].astype(np.int64), row[perm].astype(np.int64), col[perm].astype(np.int64),
                          val[perm])


def _families(VX, p, seed=3):
    return [VX.local_family(k, p) for k in KINDS] + [_random_family(VX, p.N, seed + p.N)]


_refs = {}


def _corr_case(O, VX, Lx, Ly, beta=8.0):
    """(p, disorder, Δ, CorrRef, families, pairs, refs sites, (corr, local, mean)) of a disordered lattice,
    once per module"""
    key = (Lx, Ly, beta)
    if key not in _refs:
        p, dis, D = _case(O, Lx, Ly, beta, seed=Lx * 17 + Ly)
        ref = CorrRef.from_oracle(O, p, dis, D)
        fams = _families(VX, p)
        pairs = PAIRS if p.N < 256 else PAIRS_BIG
        sites = [0, p.N // 2 + 1, p.N - 1]
        _refs[key] = (p, dis, D, ref, fams, pairs, sites, ref.response(fams, pairs, sites))
    return _refs[key]


def _check_parity(got, want, what):
    corr, local, mean = want
    for k, w in (("corr", corr), ("local", local), ("mean", mean)):
        if got[k] is None:
            continue
        err = np.abs(got[k] - w).max()
        print(what, k, "max|Δ|", err, "max|ref|", np.abs(w).max())
        _close_max(got[k], w, (what, k))


# --------------------------------------------------------------------------- CPU: the formula
def test_wick_formula_against_fock_space():
    """m and G of random families on a random 6-mode quadratic Hamiltonian
    against the thermal average in the 64-dimensional Fock space: pins the
    formula, its signs and the ρ convention independently of the library.
    Bar: 64 x 64 products of O(1) matrices, a few hundred eps."""
    rng = np.random.default_rng(1)
    N, n2, beta = 3, 6, 1.7
    h = rng.standard_normal((n2, n2)) + 1j * rng.standard_normal((n2, n2))
    h = (h + h.conj().T) / 2
    E, U = np.linalg.eigh(h)
    p = SimpleNamespace(Lx=3, Ly=1, N=N, beta=beta)
    ref = CorrRef(p, E, U, beta=beta)
    fock = FockThermal(h, beta)
    for x in range(n2):
        for y in range(n2):
            assert abs(fock.avg(fock.d[y].conj().T @ fock.d[x]) - ref.rho()[x, y]) <= 1e-13
    fams = []
    for k in range(2):
        cnt = rng.integers(0, 5, N)
        cnt[k] = 0
        site = np.repeat(np.arange(N), cnt)
        n = len(site)
        fams.append(SimpleNamespace(site=site, row=rng.integers(0, n2, n), col=rng.integers(0, n2, n),
                                    val=rng.standard_normal(n) + 1j * rng.standard_normal(n)))
    ops = [[fock.bilinear(f.row[f.site == i], f.col[f.site == i], f.val[f.site == i]) for i in range(N)]
           for f in fams]
    worst = 0.0
    for a in range(2):
        m = ref.mean(fams[a])
        for i in range(N):
            worst = max(worst, abs(fock.avg(ops[a][i]) - m[i]))
        for b in range(2):
            G, Gl = ref.gmat(fams[a], fams[b]), ref.g_loops(fams[a], fams[b])
            assert np.abs(G - Gl).max() <= 1e-13
            for i in range(N):
                for j in range(N):
                    Ob = ops[b][j].conj().T
                    want = fock.avg(ops[a][i] @ Ob) - fock.avg(ops[a][i]) * fock.avg(Ob)
                    worst = max(worst, abs(want - G[i, j]))
    print("Fock space vs Wick: max|Δ|", worst)
    assert worst <= 1e-12
    assert np.abs(ref.gmat(fams[0], fams[1])).max() > 1e-2


def test_lattice_sum(oracle, VX):
    """Σ_ij G_AB(i, j) = Tr[W_A (1 - ρ) W_B† ρ] = Σ_nm X^A_nm conj(X^B_nm) f_n (1 - f_m), W the summed vertex."""
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, 6, 4)
    rho = ref.rho()
    one = np.eye(2 * p.N)
    f = np.asarray(ref.f, dtype=np.float64)
    for a, b in pairs:
        Wa, Wb = fams[a].dense(p.N).sum(0), fams[b].dense(p.N).sum(0)
        total = ref.gmat(fams[a], fams[b]).sum()
        _close(total, np.trace(Wa @ (one - rho) @ Wb.conj().T @ rho), ("trace", a, b))
        _close(total, np.sum(ref.x(Wa) * np.conj(ref.x(Wb)) * (f[:, None] * (1 - f)[None, :])), ("pairs", a, b))
        _close(want[0][pairs.index((a, b))].sum() * p.N, total, ("corr sum", a, b))
    assert abs(ref.gmat(fams[0], fams[2]).sum()) > 1e-6


def test_local_family(oracle, VX):
    """Σ_i O(i) is the q = 0 vertex entry for entry, for every kind; for the
    on-site kinds Σ_r e^{-iq·r} C_AA(r) = (1/N) Tr[W_q (1 - ρ) W_q† ρ]."""
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, 6, 4)
    assert set(VX.LOCAL_KINDS) == set(VX.NAMBU_KINDS)
    for kind in VX.LOCAL_KINDS:
        f = VX.local_family(kind, p)
        assert np.array_equal(f.dense(p.N).sum(0), VX.build_nambu(kind, p, 0, 0).dense(p.N)), kind
        v = VX.build_nambu(kind, p, 0, 0)
        assert np.array_equal(f.row, v.row) and np.array_equal(f.col, v.col) and np.array_equal(f.val, v.val)
        assert f.site.min() == 0 and f.site.max() == p.N - 1 and np.all(np.bincount(f.site) == len(f.site) // p.N)
    # the owner of a bond term is the site the bond starts at: one of its two ends, and for the particle
    # block of the current its row or its column
    f = VX.local_family("pair_d_create", p)
    assert np.all((f.row == f.site) | (f.col - p.N == f.site))
    with pytest.raises(ValueError):
        VX.local_family("charge", p)
    rho, one = ref.rho(), np.eye(2 * p.N)
    for kind in ("density", "spin", "pair_s_create"):
        f = VX.local_family(kind, p)
        G = ref.gmat(f, f)
        T = translate_table(p.Lx, p.Ly)
        corr = (G[T, np.arange(p.N)[None, :]].sum(axis=1) / p.N).reshape(p.Ly, p.Lx)
        S = VX.structure_factor(p, corr)
        for mx, my in ((1, 0), (2, 3)):
            W = VX.build_nambu(kind, p, mx, my).dense(p.N)
            _close(S[my, mx], np.trace(W @ (one - rho) @ W.conj().T @ rho) / p.N, (kind, mx, my))


def test_structure_factor_and_disconnected(oracle, VX):
    p = oracle.ModelParameters(5, 3, 1.0, -0.35, -1.08, 0.0, 0.0, 4.0, 0.8, 1.0)
    rng = np.random.default_rng(2)
    c = rng.standard_normal((2, p.Ly, p.Lx)) + 1j * rng.standard_normal((2, p.Ly, p.Lx))
    S = VX.structure_factor(p, c)
    y, x = np.mgrid[:p.Ly, :p.Lx]
    for my in range(p.Ly):
        for mx in range(p.Lx):
            ph = np.exp(-2j * np.pi * (mx * x / p.Lx + my * y / p.Ly))
            _close(S[:, my, mx], (c * ph).sum(axis=(1, 2)), (mx, my))
    with pytest.raises(ValueError):
        VX.structure_factor(p, c[:, :, :4])
    ma, mb = c[0], rng.standard_normal((p.Ly, p.Lx)) + 1j * rng.standard_normal((p.Ly, p.Lx))
    T = translate_table(p.Lx, p.Ly)
    want = (ma.ravel()[T] * np.conj(mb.ravel())[None, :]).sum(axis=1) / p.N
    _close_max(VX.disconnected(p, ma, mb), want.reshape(p.Ly, p.Lx), "disconnected")
    _close_max(VX.disconnected(p, c, mb)[1], VX.disconnected(p, c[1], mb), "disconnected, batched")


def test_clean_lattice_is_translation_invariant(oracle, VX):
    """uniform d-wave Δ without disorder: G(i, j) depends on i ⊖ j only, so the
    translation average (which carries the 1/N) equals local at every reference site"""
    p, dis, D = _clean(oracle, 4, -1.0)
    ref = CorrRef.from_oracle(oracle, p, dis, D)
    fams = [VX.local_family(k, p) for k in ("density", "pair_d_create", "current_x")]
    sites = [0, 5, p.N - 1]
    corr, local, mean = ref.response(fams, [(0, 0), (1, 1), (2, 2), (1, 0)], sites)
    for q in range(len(sites)):
        _close_max(local[:, q], corr, ("site", sites[q]))
    for m in mean:
        _close_max(m, np.full_like(m, m[0, 0]), "uniform mean")
    assert np.abs(corr[1]).max() > 1e-3


def test_pair_mean_is_the_pairing_amplitude(oracle, VX):
    """the convention behind the GPU comparison with dwh_pairing: mean of pair_d_create at i = -conj(P_x(i)) + conj(P_y(i)),
    and Σ_i mean of density = N - 2 Tr ρ_hh"""
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, 6, 4)
    P, _ = oracle.pairing_P(ref.U.astype(np.complex128), ref.E, p)
    _close_max(want[2][2].ravel(), -np.conj(P[:, 0]) + np.conj(P[:, 1]), "pairing")
    trhh = np.trace(ref.rho()[p.N:, p.N:]).real
    _close(want[2][0].sum(), p.N - 2 * trhh, "hole trace")


# --------------------------------------------------------------------------- CPU: the host entry and the binding
def _terms(VX, fams, N):
    return VX.local_terms(fams, N)


def _dense_call(lib, N, nfam, tptr, trow, tcol, tval, npairs=0, pairs=None, nref=0, ref=None, out=True, size=None):
    """size: elements of the out buffer (default: what the call fills; a refused call writes nothing)"""
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    buf = np.full(max(nfam, 1) * N * 4 * N * N if size is None else size, np.nan + 0j) if out else None
    rc = lib.dwh_debug_correlation_dense(N, nfam, P(tptr), P(trow), P(tcol), P(tval), npairs, P(pairs), nref, P(ref),
                                         P(buf))
    return rc, buf


def test_debug_correlation_dense(dwhmc, oracle, VX):
    """the terms as uploaded, expanded per (family, site), duplicates summed"""
    lib = dwhmc.load_library()
    p = oracle.ModelParameters(3, 2, 1.0, -0.35, -1.08, 0.0, 0.0, 4.0, 0.8, 1.0)
    N = p.N
    fams = [VX.local_family("pair_d_amplitude", p), _random_family(VX, N, 9), VX.local_family("current_x", p)]
    tptr, trow, tcol, tval = _terms(VX, fams, N)
    assert len(tptr) == 3 * N + 1 and tptr[0] == 0 and tptr[-1] == len(tval) and np.all(np.diff(tptr) >= 0)
    assert tptr[N + 1] - tptr[N] == 0 and tptr[N + 2] - tptr[N + 1] == MAX_TERMS
    pairs, ref = np.array([0, 1, 2, 2], dtype=np.int64), np.array([0, N - 1], dtype=np.int64)
    rc, out = _dense_call(lib, N, 3, tptr, trow, tcol, tval, 2, pairs, 2, ref)
    assert rc == 0, lib.dwh_last_error(None)
    out = out.reshape(3, N, 2 * N, 2 * N).transpose(0, 1, 3, 2)               # (column-major on the ABI side)
    for k, f in enumerate(fams):
        _close_max(out[k], f.dense(N), ("family", k), tol=1e-15)
    dup = fams[1].dense(N)
    assert np.count_nonzero(dup) < len(fams[1].val)                            # (duplicates were summed)
    rc, out2 = _dense_call(lib, N, 3, tptr, trow, tcol, tval)                  # no pairs, no reference sites
    assert rc == 0 and out2.tobytes() == out.transpose(0, 1, 3, 2).tobytes()


def test_argument_errors_host(dwhmc, oracle, VX):
    """every refusal of the validation, each with its text; nothing is written"""
    lib = dwhmc.load_library()
    p = oracle.ModelParameters(3, 2, 1.0, -0.35, -1.08, 0.0, 0.0, 4.0, 0.8, 1.0)
    N = p.N
    fams = [VX.local_family("density", p), VX.local_family("pair_d_create", p)]
    tptr, trow, tcol, tval = _terms(VX, fams, N)
    pairs, ref = np.array([0, 1], dtype=np.int64), np.array([N - 1], dtype=np.int64)
    base = dict(N=N, nfam=2, tptr=tptr, trow=trow, tcol=tcol, tval=tval, npairs=1, pairs=pairs, nref=1, ref=ref)

    def mod(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    dec = tptr.copy()
    dec[2], dec[3] = tptr[3], tptr[2] - 1
    many = np.full(2 * N + 1, MAX_TERMS + 1, dtype=np.int64)               # 65 terms at (family 0, site 0)
    many[0] = 0
    nbig = MAX_TERMS + 1
    big = dict(tptr=many, trow=np.zeros(nbig, dtype=np.int64), tcol=np.zeros(nbig, dtype=np.int64),
               tval=np.ones(nbig, dtype=np.complex128))
    cases = [
        (dict(nfam=0), "nfam"), (dict(nfam=-1), "nfam"),
        (dict(tptr=None), "NULL"), (dict(tptr=mod(tptr, 0, 1)), "start at 0"), (dict(tptr=dec), "decreases"),
        (dict(trow=None), "NULL"), (dict(tcol=None), "NULL"), (dict(tval=None), "NULL"),
        (dict(trow=mod(trow, 3, 2 * N)), "outside [0, 2N)"), (dict(trow=mod(trow, 0, -1)), "outside [0, 2N)"),
        (dict(tcol=mod(tcol, 5, 2 * N)), "outside [0, 2N)"), (dict(tcol=mod(tcol, 1, -3)), "outside [0, 2N)"),
        (dict(tval=mod(tval, 2, np.nan)), "non-finite"), (dict(tval=mod(tval, 4, 1j * np.inf)), "non-finite"),
        (big, "more than 64 terms"),
        (dict(npairs=-1), "npairs"), (dict(npairs=0), "npairs"), (dict(pairs=None), "NULL"),
        (dict(pairs=mod(pairs, 1, 2)), "pair index"), (dict(pairs=mod(pairs, 0, -1)), "pair index"),
        (dict(nref=0), "nref"), (dict(nref=-1), "nref"), (dict(ref=None), "NULL"),
        (dict(ref=mod(ref, 0, N)), "reference site"), (dict(ref=mod(ref, 0, -1)), "reference site"),
        (dict(N=0), "N must be"), (dict(N=4097, tptr=np.zeros(2 * 4097 + 1, dtype=np.int64)), "2N above 8192"),
    ]
    for kw, text in cases:
        args = dict(base)
        args.update(kw)
        rc, out = _dense_call(lib, size=2 * N * 4 * N * N, **args)
        msg = lib.dwh_last_error(None).decode()
        assert rc == -1 and text in msg, (list(kw), msg)
        assert msg.startswith("correlations"), msg
        assert np.all(np.isnan(out)), kw
    # more than 2^24 terms in all: at the cap of 64 per site that takes more than 2^18 (family, site) slots,
    # nfam = 65 at N = 4096; the count speaks before any term is read (a one-element out: nothing is written)
    Nc = 4096
    tp_over = np.arange(65 * Nc + 1, dtype=np.int64) * MAX_TERMS
    one = np.full(1, np.nan + 0j)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_debug_correlation_dense(Nc, 65, P(tp_over), None, None, None, 0, None, 0, None, P(one))
    assert rc == -1 and "2^24 terms" in lib.dwh_last_error(None).decode() and np.isnan(one[0])
    rc, _ = _dense_call(lib, **base, out=False)
    assert rc == -1 and "NULL" in lib.dwh_last_error(None).decode()


def test_null_context_is_refused_and_binding(dwhmc):
    lib = dwhmc.load_library()
    z = np.zeros(4, dtype=np.int64)
    buf = np.zeros(16, dtype=np.complex128)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_measure_correlations(None, 0, 1, None, 1, P(z), P(z), P(z), P(buf), 1, P(z), 1, P(z), P(buf), P(buf),
                                      P(buf))
    assert rc == -1
    assert b"NULL context" in lib.dwh_last_error(None)
    sig = import_module(dwhmc.__name__ + "._lib").SIGNATURES
    assert len(sig["dwh_measure_correlations"][1]) == 16 and len(sig["dwh_debug_correlation_dense"][1]) == 11
    T = dwhmc.FermionContext.TIMERS
    assert (T.index("corr_rho"), T.index("corr_contract"), T.index("corr_reduce")) == (17, 18, 19)
    assert T.index("map") == 16


def test_local_terms(oracle, VX):
    p = oracle.ModelParameters(3, 2, 1.0, -0.35, -1.08, 0.0, 0.0, 4.0, 0.8, 1.0)
    f = _random_family(VX, p.N, 4)
    tptr, trow, tcol, tval = VX.local_terms([f, f], p.N)
    assert tptr.dtype == trow.dtype == tcol.dtype == np.int64 and tval.dtype == np.complex128
    for i in range(p.N):
        k = np.flatnonzero(f.site == i)                                         # the family's own order inside a site
        for o in (0, len(f.val)):
            s = slice(tptr[i + (p.N if o else 0)], tptr[i + 1 + (p.N if o else 0)])
            assert np.array_equal(trow[s], f.row[k]) and np.array_equal(tcol[s], f.col[k])
            assert np.array_equal(tval[s], f.val[k])
    for bad in ([], [f._replace(site=f.site + p.N)], [f._replace(row=f.row[:-1])], [(f.site, f.row, f.col, f.val)]):
        with pytest.raises(ValueError):
            VX.local_terms(bad, p.N)


# --------------------------------------------------------------------------- CPU: the driver option
SIM_OPT = dict(families=["pair_d_create", "density", "current_x"], pairs=[(0, 0), (1, 1), (2, 1)], ref_sites=[0, 9])
SIM_SHAPES = dict(corr=(3, 4, 4), corr_mean=(3, 4, 4), corr_local=(3, 2, 4, 4))


def _check_sim_outputs(with_opt, without, opt=SIM_OPT):
    """the bins of a run with the option next to the same run without it: (corr, corr_mean, corr_local) per bin"""
    spec = "spectra_bins"
    assert not (without / spec / "correlations_pairs.npy").exists()
    for f in ("observables.csv", "transport.csv"):
        assert (with_opt / f).read_bytes() == (without / f).read_bytes(), f
    for f in ("params.json", "omega_grid.npy"):
        assert (with_opt / spec / f).read_bytes() == (without / spec / f).read_bytes(), f
    assert sorted(os.listdir(with_opt / spec)) == sorted(os.listdir(without / spec) + ["correlations_pairs.npy"])
    assert sorted(os.listdir(with_opt)) == sorted(os.listdir(without))
    pairs = np.load(with_opt / spec / "correlations_pairs.npy")
    assert pairs.dtype == np.int64 and np.array_equal(pairs, np.asarray(opt["pairs"]))
    keys = ["corr", "corr_mean"] + (["corr_local"] if opt.get("ref_sites") is not None else [])
    bins = sorted(f for f in os.listdir(with_opt / spec) if f.startswith("sweep_"))
    assert len(bins) == SIM_KW["n_measure"] // SIM_KW["bin_size"]
    out = []
    for f in bins:
        a, b = np.load(with_opt / spec / f), np.load(without / spec / f)
        assert sorted(a.files) == sorted(b.files + keys)
        for k in keys:
            assert a[k].shape == SIM_SHAPES[k] and a[k].dtype == np.complex128 and np.all(np.isfinite(a[k])), k
        assert np.abs(a["corr"]).max() > 1e-3
        for k in b.files:
            assert np.array_equal(a[k], b[k]), k
        out.append(tuple(a[k] for k in keys))
    return out


@pytest.mark.parametrize("tb", [1, 3])
def test_simulation_option_on_oracle(dwhmc, tmp_path, tb):
    """run_simulation(correlations=...) on the oracle backend: the three bin
    keys through TransportQueue's batches (tb = 1: unbatched), the pairs
    written once; the other files are unchanged; batched and unbatched runs
    give the same bytes."""
    _simulate(dwhmc, tmp_path / "with", OracleCorrelations, correlations=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", OracleCorrelations, transport_batch=tb, **SIM_KW)
    got = _check_sim_outputs(tmp_path / "with", tmp_path / "without")
    if tb == 1:
        _simulate(dwhmc, tmp_path / "b3", OracleCorrelations, correlations=SIM_OPT, transport_batch=3, **SIM_KW)
        for one, three in zip(got, _check_sim_outputs(tmp_path / "b3", tmp_path / "without")):
            for x, y in zip(one, three):
                assert x.tobytes() == y.tobytes()
    assert np.abs(got[0][0] - got[1][0]).max() > 1e-9                          # the sweeps' own Δ, not one state's


@pytest.mark.parametrize("tb", [1, 2])
def test_simulation_chains_option_on_oracle(dwhmc, tmp_path, tb):
    _simulate(dwhmc, tmp_path / "with", OracleCorrelations, chains=2, correlations=SIM_OPT, transport_batch=tb,
              **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", OracleCorrelations, chains=2, transport_batch=tb, **SIM_KW)
    for k in range(2):
        _check_sim_outputs(tmp_path / "with" / f"c{k}", tmp_path / "without" / f"c{k}")


def test_simulation_bin_means_are_means_of_single_calls(dwhmc, oracle, tmp_path):
    """every bin holds the mean of measure_correlations at the Δ of its own sweeps (bin_size 2): a queue
    fed with known fields, against single calls of the oracle context at each of them"""
    sim = import_module(dwhmc.__name__ + ".simulation")
    p = dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)
    st = dwhmc.initialize_state(p, np.random.default_rng(5))
    rng = np.random.default_rng(6)
    fields = [st.Delta + 0.1 * k * (rng.standard_normal((p.N, 2)) + 1j * rng.standard_normal((p.N, 2)))
              for k in range(1, 5)]
    ctx = OracleCorrelations(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, st.disorder_pot)
    VX = dwhmc.vertices
    fams = [VX.local_family(k, p) for k in SIM_OPT["families"]]
    singles = []
    for D in fields:
        ctx.set_pairing(D)
        singles.append(ctx.measure_correlations(fams, pairs=SIM_OPT["pairs"], ref_sites=SIM_OPT["ref_sites"]))
    for tb in (1, 2):
        out = sim.ChainOutput(str(tmp_path / f"tb{tb}"), False)
        try:
            sim.write_headers(out.spec_dir, p, sim.parse_options(p, correlations=SIM_OPT))
            tq = sim.TransportQueue(ctx, p, out, sim.SimulationResult(1, 0.0, 0.0), 2, tb, correlations=SIM_OPT)
            for i, D in enumerate(fields, start=1):
                ctx.set_pairing(D)                                              # (batch 1 measures at the context's Δ)
                tq.add(i, D)
            tq.flush()
        finally:
            out.close()
        for b, sweep in enumerate((2, 4)):
            a = np.load(tmp_path / f"tb{tb}" / "spectra_bins" / f"sweep_{sweep}.npz")
            for key, src in (("corr", "corr"), ("corr_mean", "mean"), ("corr_local", "local")):
                want = (singles[2 * b][src] + singles[2 * b + 1][src]) / 2
                _close_max(a[key], want, (tb, sweep, key), tol=1e-14)


def test_simulation_default_is_unchanged_and_unknown_keys_raise(dwhmc, tmp_path):
    """correlations=None: every file is what a run writes when the option
    does not exist at all (the oracle context that knows nothing of it); the
    defaults; unknown keys and unusable values raise, for one chain and for
    several; OPTIONS keeps its five keywords and the new one is walked after them."""
    from oracle_context import OracleContext
    sim = import_module(dwhmc.__name__ + ".simulation")
    assert [o.keyword for o in sim.EQUAL_TIME_OPTIONS] == ["correlations"] and len(sim.OPTIONS) == 5
    _simulate(dwhmc, tmp_path / "plain", OracleContext, **SIM_KW)
    _simulate(dwhmc, tmp_path / "none", OracleCorrelations, correlations=None, **SIM_KW)
    for root, _, files in os.walk(tmp_path / "plain"):
        for f in files:
            if f == "simulation.log":                                            # (timestamps)
                continue
            a = os.path.join(root, f)
            b = os.path.join(tmp_path / "none", os.path.relpath(a, tmp_path / "plain"))
            assert open(a, "rb").read() == open(b, "rb").read(), f
    assert sorted(os.listdir(tmp_path / "plain" / "spectra_bins")) == sorted(os.listdir(tmp_path / "none" / "spectra_bins"))
    p = dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)
    (o,) = sim.parse_options(p, correlations={})
    assert o.names == ["pair_d_create"] and o.pairs == [(0, 0)] and o.ref_sites is None
    assert [type(x).__name__ for x in sim.parse_options(p, correlations={}, spectral_maps={})] == \
        ["SpectralMaps", "Correlations"]
    for k, opt in enumerate((dict(family=["density"]), dict(families=["charge"]), dict(families=[]),
                             dict(pairs=[(0, 1)]), dict(pairs=[]), dict(families=["density"], pairs=[(-1, 0)]),
                             dict(ref_sites=[16]), dict(ref_sites=[-1]), dict(ref_sites=[]))):
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"a{k}", OracleCorrelations, correlations=opt, **SIM_KW)
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"b{k}", OracleCorrelations, chains=2, correlations=opt, **SIM_KW)


# --------------------------------------------------------------------------- GPU
def _measure(ctx, fams, pairs, sites, **kw):
    return ctx.measure_correlations(fams, pairs=pairs, ref_sites=sites, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", GPU_LATTICES)
def test_parity_with_numpy(dwhmc, oracle, VX, Lx, Ly):
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, Lx, Ly)
    ctx = _ctx(dwhmc, p, dis)
    try:
        ctx.set_pairing(D)
        got = _measure(ctx, fams, pairs, sites)
    finally:
        ctx.close()
    assert got["corr"].shape == (len(pairs), Ly, Lx) and got["local"].shape == (len(pairs), 3, Ly, Lx)
    assert got["mean"].shape == (len(fams), Ly, Lx) and np.array_equal(got["pairs"], np.asarray(pairs))
    _check_parity(got, want, (Lx, Ly))
    assert np.abs(want[0]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (5, 7)])
def test_injected_eigensystems(dwhmc, oracle, VX, Lx, Ly):
    """Haar U (no symmetry, it diagonalises nothing) and prescribed spectra
    against the long double restatement: test_nambu_response's spectrum (a
    cluster of four within 1e-9, a pair across zero, a level behind a huge
    gap), one with exact degeneracies, and one at β|E| where f is 0 or 1."""
    beta = 8.0
    p, dis, D = _free(oracle, VX, Lx, Ly, beta=beta)
    n2 = 2 * p.N
    fams = _families(VX, p, seed=7)
    pairs, sites = [(0, 0), (2, 2), (3, 4), (5, 5), (5, 2)], [0, 3, p.N - 1]
    deg = np.sort(np.repeat(np.linspace(-1.5, 1.5, n2 // 4), 4)[:n2])
    deg = np.sort(np.concatenate([deg, np.zeros(n2 - len(deg))]))
    sat = np.sort(np.where(np.arange(n2) % 2, 1.0, -1.0) * np.linspace(200.0, 900.0, n2))
    assert len(np.unique(deg)) < n2 / 2 and R.logistic(-beta * sat).min() == 0.0 and R.logistic(-beta * sat).max() == 1.0
    ctx = _ctx(dwhmc, p, dis, algo="eig")
    try:
        for k, E in enumerate((_injected_spectrum(n2, beta), deg, sat)):
            U = R.haar(n2, 11 + n2 + k)
            want = CorrRef(p, E, U, beta=beta, dt=LD).response(fams, pairs, sites)
            ctx.debug_set_eigensystem(E, U)
            _check_parity(_measure(ctx, fams, pairs, sites), want, ("injected", Lx, Ly, k))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(6, 4), (10, 6)])
def test_mean_against_the_factorisation(dwhmc, oracle, VX, Lx, Ly):
    """mean of the density family and of pair_d_create against dwh_hole_trace
    and dwh_pairing (the pole expansion's own results) at test_gpu_parity's
    1e-11 per entry; the hole trace is a sum of N such entries, hence 1e-11 N"""
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, Lx, Ly)
    ctx = _ctx(dwhmc, p, dis)
    try:
        ctx.set_pairing(D)
        ctx.factorize()
        P, trhh = ctx.pairing()[0], ctx.hole_trace()[0]
        got = ctx.measure_correlations([fams[0], fams[2]], corr=False)
    finally:
        ctx.close()
    assert got["corr"] is None and got["local"] is None
    m_pair = -np.conj(P[:, 0]) + np.conj(P[:, 1])
    e1 = np.abs(got["mean"][1].ravel() - m_pair).max()
    e2 = abs(got["mean"][0].sum() - (p.N - 2 * trhh))
    print("mean vs pairing", e1, "vs hole trace", e2)
    assert e1 <= 1e-11 and e2 <= 1e-11 * p.N
    assert np.abs(m_pair).max() > 1e-2


@pytest.mark.gpu
def test_structure(dwhmc, oracle, VX, monkeypatch):
    """Two calls and one-state groups give the same bits; 3 snapshots equal
    their single-state calls; chain 1 of a 2-chain context; each output
    skipped in turn; the context's Δ is unchanged."""
    O = oracle
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(O, VX, 10, 6)
    p2, dis2, D2 = _case(O, 10, 6, 8.0, seed=77)
    rng = np.random.default_rng(8)
    fields = np.stack([D2, D2 * np.exp(0.1j), D2 + 0.05 * rng.standard_normal(D2.shape)])
    ctx = _ctx(dwhmc, p, np.stack([dis, dis2]))
    keys = ("corr", "local", "mean")
    try:
        ctx.set_pairing(np.stack([D, D2]))
        before, _ = ctx.get_state()
        one = _measure(ctx, fams, pairs, sites)
        again = _measure(ctx, fams, pairs, sites)
        for k in keys:
            assert again[k].tobytes() == one[k].tobytes(), k
        _check_parity(one, want, "chain 0")
        r3 = _measure(ctx, fams, pairs, sites, chain=1, deltas=fields)
        monkeypatch.setenv("DWHMC_RESPONSE_GROUP", "1")
        g3 = _measure(ctx, fams, pairs, sites, chain=1, deltas=fields)
        monkeypatch.delenv("DWHMC_RESPONSE_GROUP")
        ones = [_measure(ctx, fams, pairs, sites, chain=1, deltas=fields[s:s + 1]) for s in range(3)]
        dev1 = _measure(ctx, fams, pairs, sites, chain=1)                    # the device Δ of chain 1 = fields[0]
        assert r3["corr"].shape == (3, len(pairs), p.Ly, p.Lx) and r3["local"].shape == (3, len(pairs), 3, p.Ly, p.Lx)
        assert r3["mean"].shape == (3, len(fams), p.Ly, p.Lx)
        for k in keys:
            assert g3[k].tobytes() == r3[k].tobytes(), k
            for s in range(3):
                assert ones[s][k][0].tobytes() == r3[k][s].tobytes(), (k, s)
            assert dev1[k].tobytes() == r3[k][0].tobytes(), k
        w2 = CorrRef.from_oracle(O, p2, dis2, fields[2]).response(fams, pairs, sites)
        _check_parity({k: r3[k][2] for k in keys}, w2, "chain 1 snapshot 2")
        no_mean = _measure(ctx, fams, pairs, sites, mean=False)
        no_corr = _measure(ctx, fams, pairs, sites, corr=False)
        no_local = _measure(ctx, fams, pairs, None)
        only_mean = ctx.measure_correlations(fams, corr=False)
        default = ctx.measure_correlations(fams)                              # every (k, k)
        assert no_mean["mean"] is None and no_corr["corr"] is None and no_local["local"] is None
        assert only_mean["corr"] is None and only_mean["local"] is None
        for r in (no_mean, no_corr, no_local, only_mean):
            for k in keys:
                assert r[k] is None or r[k].tobytes() == one[k].tobytes(), k
        assert np.array_equal(default["pairs"], np.stack([np.arange(6)] * 2, axis=1))
        four = ctx.measure_correlations(tuple(fams[:4]), mean=False)           # four families in a tuple: no term table
        assert four["corr"].tobytes() == one["corr"][:4].tobytes()
        assert default["corr"][:5].tobytes() == one["corr"][:5].tobytes()     # PAIRS starts with (k, k), k < 6
        after, _ = ctx.get_state()
        assert np.array_equal(before, after)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chains", [0, 2])
def test_simulation_option_on_the_device(dwhmc, tmp_path, chains):
    """the drivers with the keyword on the device context, batched: the three keys in every bin"""
    kw = dict(SIM_KW, n_therm=2)
    _simulate(dwhmc, tmp_path / "with", None, chains=chains, correlations=SIM_OPT, transport_batch=2, **kw)
    for d in ([tmp_path / "with" / f"c{k}" for k in range(chains)] if chains else [tmp_path / "with"]):
        assert np.array_equal(np.load(d / "spectra_bins" / "correlations_pairs.npy"), np.asarray(SIM_OPT["pairs"]))
        bins = sorted(f for f in os.listdir(d / "spectra_bins") if f.startswith("sweep_"))
        assert len(bins) == SIM_KW["n_measure"] // SIM_KW["bin_size"]
        for f in bins:
            a = np.load(d / "spectra_bins" / f)
            for k, shape in SIM_SHAPES.items():
                assert a[k].shape == shape and np.all(np.isfinite(a[k])), k
            assert np.abs(a["corr"]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dense", "cr", "eig"])
def test_algorithms(dwhmc, oracle, VX, algo):
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, 6, 4)
    ctx = _ctx(dwhmc, p, dis, algo=algo)
    try:
        ctx.set_pairing(D)
        assert ctx.info["algo"] == {"dense": 0, "cr": 1, "eig": 2}[algo]
        got = _measure(ctx, fams, pairs, sites)
    finally:
        ctx.close()
    _check_parity(got, want, algo)


@pytest.mark.gpu
def test_timers_and_workspace_reuse(dwhmc, oracle, VX):
    """One record per stage and state with the stated work; the call before
    and after the other five measurement calls on one context gives the same
    bits, and they give the same bytes before and after it."""
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, 6, 4)
    pat = VX.bond_pattern(p)
    vs = [VX.build_nambu("current_x", p, 0, 1), VX.build_nambu("pair_d_amplitude", p)]
    ops = [VX.density(p, 1, 0), VX.raman_b1g(p)]
    ctx = _ctx(dwhmc, p, dis)

    def others():
        r = ctx.measure_current_response(direction="y", q=[(0, 0), (1, 2)], n_matsubara=2)
        t = ctx.measure_transport(0.01, 0.002, 4.0)
        o = ctx.measure_operator_response(ops, n_matsubara=2, omega=(-0.6, 0.3, 5), eta=0.05)
        n = ctx.measure_nambu_response(vs, [(0, 1), (1, 1)], n_matsubara=2, omega=(-0.6, 0.3, 5), eta=0.05)
        m = ctx.measure_response_map(vs, pat, n_matsubara=2, omega=(0.1,), eta=0.05)
        s = ctx.measure_spectral_maps(0.05, 0.5, 4.0)
        return [np.float64(r["dia"]).tobytes(), r["lam"].tobytes(), o["chi"].tobytes(), o["chi2"].tobytes(),
                n["chi"].tobytes(), n["chi2"].tobytes(), m["dmap"].tobytes(), m["rho"].tobytes(),
                s["ldos"].tobytes(), s["akw"].tobytes()] + [
            np.asarray(t[k]).tobytes() for k in ("superfluid_stiffness", "dc_conductivity", "optical_conductivity",
                                                 "dos", "dos_AN", "A_k_omega0")]

    try:
        ctx.set_pairing(D)
        ctx.timing_enable(["corr_rho", "corr_contract", "corr_reduce"])
        first = _measure(ctx, fams, pairs, sites)                             # before any other measurement
        before = others()
        second = _measure(ctx, fams, pairs, sites)
        after = others()
        _measure(ctx, fams[:2], [(0, 1)], None, deltas=np.stack([D, D, D]))
        tr, tc, td = (ctx.timing_read(k) for k in ("corr_rho", "corr_contract", "corr_reduce"))
        nam = ctx.timing_read("map")
    finally:
        ctx.close()
    for k in ("corr", "local", "mean"):
        assert first[k].tobytes() == second[k].tobytes(), k
    assert before == after
    _check_parity(first, want, "first call on the context")
    assert tr[1] == tc[1] == td[1] == 2 + 3 and tr[0] > 0 and tc[0] > 0 and td[0] > 0
    assert tr[2] == 5 * 8.0 * (2 * p.N) ** 3
    cnt = [len(f.val) for f in fams]
    per = [np.bincount(f.site, minlength=p.N) for f in fams]
    issued = sum(32.0 * cnt[a] * (cnt[b] + sum(per[b][q] for q in sites)) for a, b in pairs)
    assert tc[2] == 2 * issued + 3 * 32.0 * cnt[0] * cnt[1]
    assert nam[1] == 0


@pytest.mark.gpu
def test_argument_errors(dwhmc, oracle, VX):
    """Each DWH_ERR_ARG case launches nothing (the outputs keep their fill) and leaves the context usable."""
    p, dis, D, ref, fams, pairs, sites, want = _corr_case(oracle, VX, 4, 2)
    N = p.N
    ctx = _ctx(dwhmc, p, dis)
    try:
        ctx.set_pairing(D)
        full = _measure(ctx, fams, pairs, sites)
        lib, h = ctx._lib, ctx._h
        tptr, trow, tcol, tval = VX.local_terms(fams, N)
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64))
        rf = np.asarray(sites, dtype=np.int64)
        fill = np.nan + 0j
        o_m, o_c = np.full(len(fams) * N, fill), np.full(len(pairs) * N, fill)
        o_l = np.full(len(pairs) * len(sites) * N, fill)
        P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

        def call(chain=0, ns=1, nfam=len(fams), tp=tptr, tr=trow, tc=tcol, tv=tval, npairs=len(pairs), prs=pr,
                 nref=len(sites), ref=rf, mean=o_m, corr=o_c, local=o_l):
            return lib.dwh_measure_correlations(h, chain, ns, None, nfam, P(tp), P(tr), P(tc), P(tv), npairs, P(prs),
                                                nref, P(ref), P(mean), P(corr), P(local))

        def mod(a, i, v):
            b = a.copy()
            b[i] = v
            return b

        dec = tptr.copy()
        dec[2], dec[3] = tptr[3], tptr[2] - 1
        over = tptr.copy()
        over[N + 1:] += MAX_TERMS + 1                                           # 65 more terms at (family 1, site 0)
        for kw in (dict(chain=1), dict(chain=-1), dict(ns=2), dict(ns=0), dict(nfam=0), dict(tp=None),
                   dict(tp=mod(tptr, 0, 1)), dict(tp=dec), dict(tp=over), dict(tr=None), dict(tc=None), dict(tv=None),
                   dict(tr=mod(trow, 1, 2 * N)), dict(tc=mod(tcol, 0, -1)), dict(tv=mod(tval, 3, np.nan)),
                   dict(npairs=0), dict(npairs=-1), dict(prs=None), dict(prs=mod(pr.ravel(), 3, len(fams))),
                   dict(nref=0), dict(ref=None), dict(ref=mod(rf, 1, N)), dict(ref=mod(rf, 0, -1)),
                   dict(mean=None, corr=None, local=None)):
            assert call(**kw) == -1, kw
            assert lib.dwh_last_error(h), kw
            assert np.all(np.isnan(o_m)) and np.all(np.isnan(o_c)) and np.all(np.isnan(o_l)), kw
        assert call(npairs=0, prs=None, nref=0, ref=None, corr=None, local=None) == 0   # mean alone needs no pairs
        assert o_m.tobytes() == full["mean"].tobytes() and np.all(np.isnan(o_c))
        assert call(nref=0, ref=None, local=None) == 0                          # no local: no reference sites
        assert o_c.tobytes() == full["corr"].tobytes() and np.all(np.isnan(o_l))
        assert call() == 0
        assert o_l.tobytes() == full["local"].tobytes()
        for kw in (dict(pairs=[(0, 6)]), dict(ref_sites=[N]), dict(chain=1), dict(mean=False, corr=False)):
            with pytest.raises(ValueError):
                ctx.measure_correlations(fams, **kw)
        with pytest.raises(ValueError):
            ctx.measure_correlations([])
        _check_parity(_measure(ctx, fams, pairs, sites), want, "after errors")
    finally:
        ctx.close()
