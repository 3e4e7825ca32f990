"""Response of any one-body operator (dwh_measure_operator_response,
csrc/dwhmc_operator.hip).  In the Nambu basis (c_{i↑}; c†_{i↓}), with E_n, U
the eigenpairs of H_BdG(Δ) and f_n = logistic(-β E_n), the operator

    O = Σ_ij V_ij (c†_{i↑} c_{j↑} + s c†_{i↓} c_{j↓}),   Ṽ = V ⊕ (-s V^T)

has, with V_nm = (U^H Ṽ U)[n, m], ΔE_nm = E_m - E_n,

    χ(l)   = (1/N) Σ_nm r_nm(l) |V_nm|²        (the r rules of the current response)
    χ''(ω) = (π/N) Σ_nm (f_n - f_m) |V_nm|² L_η(ω - ΔE_nm),  |f_n - f_m| >= 1e-12.

The reference is the numpy restatement `_Ref` here, on the oracle's `evaluate`
(LAPACK).  Tolerances are the project's (tests/test_transport.py header):
scalars |Δ| <= 1e-9 (1 + |ref|), χ''(ω) max|Δ| <= 1e-9 (1 + max|ref|).  χ'' is
a signed sum; `_Ref.chi2(reverse=True)` adds the pairs in the opposite order
and the two restatements agree within a tenth of the tolerance, so the
tolerance does not hide the sum's conditioning.

CPU (not gpu): the identities that tie the restatement to what the project
already pins (Λ(q, iΩ), the oracle's σ(ω), the uniform spin vertex, ±q, the
Lindhard function, the B1g closed form), vertices.py, the host construction of
Ṽ (dwh_debug_operator_nambu) with its argument errors, the pair skip, and the
driver option on the oracle backend.  GPU: parity on lattices below / at /
above the 256-pair tile with tails, the grouping loop, ω blocks, consistency
with measure_current_response and measure_transport, degenerate spectra with
both solvers, snapshots, chains, algorithms, skipped parts, errors, the timer
and a guard that the shared workspaces stay intact.
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from oracle_measurements import CurrentRef as _RefCurrent, OperatorRef as _Ref, OracleOperator as _OracleOperator, \
    grid as _grid, jq as _jq, nambu as _nambu, simulate as _simulate
from test_current_response import SIM_KW, T, TP, MU, _case, _clean, _ctx

TOL = 1e-9
NL = 3
ETA = 0.05
OMEGA = (-0.6, 0.3, 5)          # -0.6, -0.3, 0, 0.3, 0.6


def _close(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    assert np.all(err <= TOL * (1 + np.abs(b))), (what, float(err.max()), a, b)


def _close_max(a, b, what="", tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    assert err <= tol * (1 + float(np.abs(b).max())), (what, err)


def _random_vertex(VX, N, seed):
    """Complex non-symmetric V, s = -1, with duplicate (row, col) entries."""
    rng = np.random.default_rng(seed)
    n = 3 * N
    row, col = rng.integers(0, N, n), rng.integers(0, N, n)
    row[1], col[1] = row[0], col[0]                      # duplicates, whatever the draw
    row[-1], col[-1] = row[2], col[2]
    val = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return VX.Vertex(row.astype(np.int64), col.astype(np.int64), val, -1)


def _opset(VX, p):
    """The parity set: (name, Vertex)."""
    ops = [("density(1,0)", VX.density(p, 1, 0)), ("density(1,2)", VX.density(p, 1, 2)),
           ("spin(0,0)", VX.spin(p, 0, 0)), ("spin(-1,0)", VX.spin(p, -1, 0)),
           ("current_x(0,1)", VX.current(p, 0, 1, "x")), ("b1g", VX.raman_b1g(p)), ("b2g", VX.raman_b2g(p)),
           ("random", _random_vertex(VX, p.N, 5 + p.N))]
    return ops


def _want(ref, ops, nl=NL, omega=OMEGA, eta=ETA):
    N = ref.p.N
    chi = np.stack([ref.chi(v.dense(N), v.spin_sign, nl) for _, v in ops])
    chi2 = np.stack([ref.chi2(v.dense(N), v.spin_sign, _grid(omega), eta) for _, v in ops])
    return chi, chi2


_refs = {}


def _ref_case(O, VX, Lx, Ly, beta=8.0):
    """(p, disorder, Δ, _Ref, ops, chi, chi2) of a disordered lattice, once per module."""
    key = (Lx, Ly, beta)
    if key not in _refs:
        p, dis, D = _case(O, Lx, Ly, beta, seed=4 if (Lx, Ly) == (2, 4) else Lx * 17 + Ly)
        ref = _Ref(O, p, dis, D)
        ops = _opset(VX, p)
        _refs[key] = (p, dis, D, ref, ops) + _want(ref, ops)
    return _refs[key]


@pytest.fixture(scope="module")
def VX(dwhmc):
    return dwhmc.vertices


# --------------------------------------------------------------------------- CPU
def test_identity_1_current_vertex_is_lambda(oracle, VX):
    """V = Jq, s = +1: χ(l) = Λ_αα(q, l), both directions; vertices.current is _jq."""
    p, dis, D = _case(oracle, 5, 7, 8.0, seed=5 * 17 + 7)
    ref, cur = _Ref(oracle, p, dis, D), _RefCurrent(oracle, p, dis, D)
    qs = [(0, 0), (1, 2), (0, -1)]
    for a in "xy":
        lam = cur.lam(a, qs, NL)
        for k, (mx, my) in enumerate(qs):
            J = _jq(p, a, mx, my)
            got = ref.chi(J, +1, NL)
            print("identity 1", a, (mx, my), float(np.abs(got - lam[k]).max()))
            _close(got, lam[k], (a, mx, my))
            Vv = VX.current(p, mx, my, a)
            assert Vv.spin_sign == 1
            assert np.abs(Vv.dense(p.N) - J).max() <= 4e-16, (a, mx, my)   # same terms, summed per bond list
            assert np.array_equal(Vv.dense(p.N) != 0, J != 0)
    # Jq ⊕ Jq: the hole block of an antisymmetric V with s = +1 is V itself
    J = _jq(p, "y", 1, 2)
    assert np.array_equal(_nambu(J, +1)[p.N:, p.N:], J)


def test_identity_2_sigma_is_chi2_over_omega(oracle, VX):
    """q = 0, x: χ''(ω)/ω on the transport grid is the oracle's σ(ω)."""
    import dataclasses
    O = oracle
    p, dis, D = _case(O, 5, 7, 8.0, seed=5 * 17 + 7)
    p = dataclasses.replace(p, eta=0.01, domega=0.002, omega_max=4.0)
    cache, _, _ = O.evaluate(p, dis, D)
    spec = O.measure_transport_and_spectra(cache, p)
    w, sig = spec["omega_grid"], spec["optical_conductivity"]
    ref = _Ref(O, p, dis, D)
    V = VX.current(p, 0, 0, "x").dense(p.N)
    got = ref.chi2(V, +1, w, p.eta) / w
    print("identity 2", float(np.abs(got - sig).max()), float(np.abs(sig).max()))
    _close_max(got, sig, "sigma")
    rev = ref.chi2(V, +1, w, p.eta, reverse=True) / w
    _close_max(rev, got, "reversed order", tol=TOL / 10)


def test_identity_3_uniform_spin_vertex(oracle, VX):
    p, dis, D = _case(oracle, 5, 7, 8.0, seed=5 * 17 + 7)
    ref = _Ref(oracle, p, dis, D)
    v = VX.spin(p, 0, 0)
    assert np.array_equal(v.dense(p.N), np.eye(p.N)) and v.spin_sign == -1
    chi = ref.chi(v.dense(p.N), -1, NL)
    want = float(np.sum(p.beta * ref.f * (1 - ref.f))) / p.N
    print("identity 3", chi, want)
    _close(chi[0], want, "chi(0)")
    assert np.all(np.abs(chi[1:]) <= 1e-20)
    # the charge vertex at q = 0 is not the identity in Nambu space
    assert abs(ref.chi(np.eye(p.N), +1, 1)[0] - want) > 1e-3


def test_identity_4_pm_q_and_pair_skip(oracle, VX):
    """χ''(q, -ω) = -χ''(-q, ω) for site vertices (non-Hermitian at q != 0),
    not χ''(q, ω) = -χ''(q, -ω); the reversed-order restatement; the share of
    skipped pairs at β = 8 lies strictly inside (0, 1)."""
    p, dis, D = _case(oracle, 5, 7, 8.0, seed=5 * 17 + 7)
    ref = _Ref(oracle, p, dis, D)
    w = _grid(OMEGA)
    odd = 0.0
    for build, s in ((VX.density, +1), (VX.spin, -1)):
        for mx, my in ((1, 2), (0, -1)):
            vp, vm = build(p, mx, my), build(p, -mx, -my)
            assert vp.spin_sign == s
            assert np.abs(vp.dense(p.N) - vp.dense(p.N).conj().T).max() > 0.1
            a = ref.chi2(vp.dense(p.N), s, -w, ETA)
            b = ref.chi2(vm.dense(p.N), s, w, ETA)
            print("identity 4", s, (mx, my), float(np.abs(a + b).max()))
            _close_max(a, -b, (s, mx, my))
            _close_max(ref.chi2(vp.dense(p.N), s, w, ETA, reverse=True), ref.chi2(vp.dense(p.N), s, w, ETA),
                       "reversed order", tol=TOL / 10)
            odd = max(odd, float(np.abs(ref.chi2(vp.dense(p.N), s, w, ETA) + a).max()))
    assert odd > 1e-4                                    # no (n, m) <-> (m, n) fold is possible
    share = ref.skipped_share()
    print("skipped share", share)
    assert 0.0 < share < 1.0


def _bands(p):
    kx = 2 * np.pi * np.arange(p.Lx)[:, None] / p.Lx
    ky = 2 * np.pi * np.arange(p.Ly)[None, :] / p.Ly
    return kx, ky, -2 * p.t * (np.cos(kx) + np.cos(ky)) - 4 * p.tp * np.cos(kx) * np.cos(ky) - p.mu


def _r(beta, e1, e2, l):
    f1, f2 = 1 / (1 + np.exp(beta * e1)), 1 / (1 + np.exp(beta * e2))
    dE = e2 - e1
    if l == 0:
        deg = np.abs(dE) < 1e-8
        return np.where(deg, beta * f1 * (1 - f1), (f1 - f2) / np.where(deg, 1.0, dE))
    return (f1 - f2) * dE / (dE * dE + (2 * np.pi * l / beta) ** 2)


def _free(O, Lx=6, Ly=4, beta=4.0):
    p = O.ModelParameters(Lx, Ly, T, TP, MU, 0.0, 0.0, beta, 0.8, 1.0)
    return p, _Ref(O, p, np.zeros(p.N), np.zeros((p.N, 2), dtype=np.complex128))


def test_identity_5_lindhard(oracle, VX):
    """Clean 6 x 4, Δ = 0: density and spin vertices give (2/N) Σ_k r(ε_k, ε_{k+q})."""
    p, ref = _free(oracle)
    _, _, eps = _bands(p)
    for mx, my in ((1, 0), (2, 1), (0, 0)):
        epq = np.roll(np.roll(eps, -mx, axis=0), -my, axis=1)
        for l in (0, 1):
            want = 2.0 / p.N * float(np.sum(_r(p.beta, eps, epq, l)))
            for v in (VX.density(p, mx, my), VX.spin(p, mx, my)):
                got = ref.chi(v.dense(p.N), v.spin_sign, l + 1)[l]
                print("lindhard", (mx, my), l, v.spin_sign, got, want)
                _close(got, want, (mx, my, l, v.spin_sign))


def test_b1g_closed_form(oracle, VX):
    p, ref = _free(oracle)
    kx, ky, eps = _bands(p)
    f = 1 / (1 + np.exp(p.beta * eps))
    for v, gam in ((VX.raman_b1g(p), 2 * p.t * (np.cos(kx) - np.cos(ky))),
                   (VX.raman_b2g(p), -4 * p.tp * np.sin(kx) * np.sin(ky))):
        chi = ref.chi(v.dense(p.N), +1, NL)
        want = 2.0 / p.N * float(np.sum(gam ** 2 * p.beta * f * (1 - f)))
        print("raman", chi, want)
        _close(chi[0], want, "chi(0)")
        assert np.all(np.abs(chi[1:]) <= 1e-20)
        assert np.array_equal(v.dense(p.N), v.dense(p.N).T) and v.spin_sign == 1


def test_vertices_union_and_kinds(dwhmc, oracle, VX):
    p, _, _ = _case(oracle, 2, 4, 8.0, seed=4)
    ops = [VX.build(k, p, 1, -1) for k in sorted(VX.KINDS)] + [_random_vertex(VX, p.N, 3)]
    dense = [v.dense(p.N) for v in ops]
    rowptr, col, val = VX.union_csr(ops + [dense[1], (ops[2].row, ops[2].col, ops[2].val)], p.N)
    assert rowptr[0] == 0 and rowptr[-1] == len(col) and val.shape == (len(ops) + 2, len(col))
    for k, Vd in enumerate(dense + [dense[1], dense[2]]):
        back = np.zeros((p.N, p.N), dtype=np.complex128)
        for r in range(p.N):
            back[r, col[rowptr[r]:rowptr[r + 1]]] = val[k, rowptr[r]:rowptr[r + 1]]
        assert np.abs(back - Vd).max() <= 1e-15, k
    with pytest.raises(ValueError):
        VX.build("charge", p)
    with pytest.raises(ValueError):
        VX.union_csr([np.zeros((3, 3))], p.N)
    with pytest.raises(ValueError):
        VX.union_csr([(np.array([0]), np.array([p.N]), np.array([1.0]))], p.N)


def _raw_csr(N, row, col, vals):
    """CSR with the triplets as given: rows grouped, columns in the caller's order, duplicates kept."""
    order = np.argsort(row, kind="stable")
    rowptr = np.searchsorted(row[order], np.arange(N + 1)).astype(np.int64)
    return rowptr, np.ascontiguousarray(col[order], dtype=np.int64), np.ascontiguousarray(
        np.atleast_2d(vals)[:, order], dtype=np.complex128)


def _call_nambu(lib, N, rowptr, col, val, sign, nops=None, nnz=None, out=True):
    val = None if val is None else np.ascontiguousarray(np.atleast_2d(val), dtype=np.complex128)
    nops = (val.shape[0] if val is not None else 1) if nops is None else nops
    nnz = (len(col) if col is not None else 1) if nnz is None else nnz
    sg = None if sign is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sign, dtype=np.int32), (max(nops, 1),)))
    buf = np.full((max(nops, 1), 2 * N, 2 * N), np.nan + 0j, dtype=np.complex128) if out else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_debug_operator_nambu(N, nops, p(rowptr), p(col), nnz, p(val), p(sg), p(buf))
    return rc, (None if buf is None else buf.transpose(0, 2, 1))   # column-major -> [k, row, col]


def test_debug_operator_nambu(dwhmc, oracle, VX):
    """The host construction the device path uploads, against V ⊕ (-s V^T)."""
    lib = dwhmc.load_library()
    N = 6
    # unsorted columns, a duplicate that adds up, a pair that cancels to zero, row 4 empty, nops = 3
    row = np.array([0, 0, 0, 1, 2, 2, 2, 3, 5, 5, 5])
    col = np.array([5, 1, 3, 0, 4, 4, 0, 3, 2, 2, 1])
    rng = np.random.default_rng(2)
    vals = rng.standard_normal((3, len(row))) + 1j * rng.standard_normal((3, len(row)))
    vals[:, 9] = -vals[:, 8]                             # (5, 2) cancels
    signs = np.array([1, -1, 1], dtype=np.int32)
    rowptr, c, v = _raw_csr(N, row, col, vals)
    assert rowptr[4] == rowptr[5] and list(c[:3]) == [5, 1, 3]
    rc, got = _call_nambu(lib, N, rowptr, c, v, signs)
    assert rc == 0, lib.dwh_last_error(None)
    for k in range(3):
        V = np.zeros((N, N), dtype=np.complex128)
        np.add.at(V, (row, col), vals[k])
        assert abs(V[5, 2]) <= 1e-15 and abs(V[2, 4] - vals[k, 4] - vals[k, 5]) <= 1e-15
        assert np.abs(got[k] - _nambu(V, signs[k])).max() <= 1e-15, k
    assert np.abs(got[0, N:, N:] + got[0, :N, :N].T).max() <= 1e-15      # s = +1: -V^T
    assert np.abs(got[1, N:, N:] - got[1, :N, :N].T).max() <= 1e-15      # s = -1: +V^T
    # Lx = 2 ring: +x and -x neighbours coincide, the raw triplets carry the duplicates
    p, _, _ = _case(oracle, 2, 4, 8.0, seed=4)
    for mx, my, a in ((0, 0, "x"), (1, 0, "x"), (1, -1, "y")):
        vt = VX.current(p, mx, my, a)
        rowptr, c, v = _raw_csr(p.N, vt.row, vt.col, vt.val)
        assert len(c) > len(np.unique(vt.row * p.N + vt.col))            # duplicates are there
        rc, got = _call_nambu(lib, p.N, rowptr, c, v, +1)
        assert rc == 0
        J = _jq(p, a, mx, my)
        assert np.abs(got[0] - _nambu(J, +1)).max() <= 1e-15, (mx, my, a)
        assert np.abs(got[0, p.N:, p.N:] - J).max() <= 1e-15             # Jq ⊕ Jq
    assert np.abs(_jq(p, "x", 0, 0)[np.arange(p.N), p.nn_table[:, 0] - 1]).max() <= 1e-15   # t - t on the ring


def test_argument_errors_host(dwhmc):
    lib = dwhmc.load_library()
    N = 4
    rowptr = np.array([0, 1, 2, 2, 3], dtype=np.int64)
    col = np.array([1, 0, 2], dtype=np.int64)
    val = np.ones((1, 3), dtype=np.complex128)
    assert _call_nambu(lib, N, rowptr, col, val, 1)[0] == 0
    bad = [dict(nops=0), dict(nnz=0), dict(nops=-1),
           dict(rowptr=np.array([1, 1, 2, 2, 3], dtype=np.int64)),          # does not start at 0
           dict(rowptr=np.array([0, 1, 2, 2, 2], dtype=np.int64)),          # does not end at nnz
           dict(rowptr=np.array([0, 2, 1, 2, 3], dtype=np.int64)),          # decreases
           dict(col=np.array([1, -1, 2], dtype=np.int64)), dict(col=np.array([1, N, 2], dtype=np.int64)),
           dict(sign=0), dict(sign=2), dict(sign=-3),
           dict(rowptr=None), dict(col=None, nnz=3), dict(val=None, nops=1), dict(sign=None), dict(out=False)]
    for kw in bad:
        args = dict(rowptr=rowptr, col=col, val=val, sign=1)
        args.update(kw)
        rc, _ = _call_nambu(lib, N, args.pop("rowptr"), args.pop("col"), args.pop("val"), args.pop("sign"), **args)
        assert rc == -1, kw
        assert lib.dwh_last_error(None), kw


def test_null_context_is_refused(dwhmc):
    lib = dwhmc.load_library()
    buf = np.zeros(8)
    rowptr, col = np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.int64)
    sg = np.ones(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_measure_operator_response(None, 0, 1, None, 1, p(rowptr), p(col), 1, p(buf), p(sg), 1, p(buf),
                                           0.1, 0.0, 0.1, 1, p(buf))
    assert rc == -1
    assert b"NULL" in lib.dwh_last_error(None)
    assert dwhmc.FermionContext.TIMERS.index("response") == 13
    assert dwhmc.FermionContext.TIMERS.index("operator") == 14


SIM_OPS = [("density", (1, 0)), ("spin", (0, 0)), ("raman_b1g", (0, 0))]
SIM_OPT = dict(ops=SIM_OPS, n_matsubara=2, omega=dict(start=-0.2, step=0.2, count=3), eta=0.1)


def _check_sim_outputs(with_opt, without):
    assert not (without / "operator_response.csv").exists()
    assert not (without / "spectra_bins" / "chi2_omega.npy").exists()
    for f in ("observables.csv", "transport.csv"):
        assert (with_opt / f).read_bytes() == (without / f).read_bytes(), f
    for f in ("params.json", "omega_grid.npy"):
        assert (with_opt / "spectra_bins" / f).read_bytes() == (without / "spectra_bins" / f).read_bytes(), f
    assert sorted(os.listdir(with_opt / "spectra_bins")) == sorted(os.listdir(without / "spectra_bins") +
                                                                   ["chi2_omega.npy"])
    assert np.array_equal(np.load(with_opt / "spectra_bins" / "chi2_omega.npy"), [-0.2, 0.0, 0.2])
    bins = sorted(f for f in os.listdir(with_opt / "spectra_bins") if f.startswith("sweep_"))
    assert len(bins) == SIM_KW["n_measure"] // SIM_KW["bin_size"]
    for f in bins:
        a, b = np.load(with_opt / "spectra_bins" / f), np.load(without / "spectra_bins" / f)
        assert sorted(a.files) == sorted(b.files + ["chi2"])
        assert a["chi2"].shape == (3, 3) and np.all(np.isfinite(a["chi2"]))
        # Hermitian vertices: χ''(0) = 0; the identity spin vertex commutes with H; the density responds
        assert np.abs(a["chi2"][1:, 1]).max() <= 1e-12 and np.abs(a["chi2"][1]).max() <= 1e-12
        assert np.abs(a["chi2"][0]).max() > 1e-6 and np.abs(a["chi2"][2]).max() > 1e-6
        for k in b.files:
            assert np.array_equal(a[k], b[k]), k
    lines = (with_opt / "operator_response.csv").read_text().splitlines()
    head = lines[0].split(",")
    assert head == ["sweep"] + [f"chi_{kind}(mx={mx};my={my};l={l})" for kind, (mx, my) in SIM_OPS for l in range(2)]
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (SIM_KW["n_measure"], 1 + 3 * 2)
    assert np.array_equal(rows[:, 0], np.arange(1, SIM_KW["n_measure"] + 1))
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1] > 0)
    return rows


@pytest.mark.parametrize("tb", [1, 3])
def test_simulation_option_on_oracle(dwhmc, tmp_path, tb):
    """run_simulation(operator_response=...) on the oracle backend: one row per
    transport measurement through TransportQueue's batches, chi2 in the bins;
    the other files are unchanged; nothing appears without the option."""
    _simulate(dwhmc, tmp_path / "with", _OracleOperator, operator_response=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", _OracleOperator, transport_batch=tb, **SIM_KW)
    rows = _check_sim_outputs(tmp_path / "with", tmp_path / "without")
    if tb == 1:
        _simulate(dwhmc, tmp_path / "b3", _OracleOperator, operator_response=SIM_OPT, transport_batch=3, **SIM_KW)
        assert (tmp_path / "b3" / "operator_response.csv").read_bytes() == \
            (tmp_path / "with" / "operator_response.csv").read_bytes()
    assert len({tuple(r[1:]) for r in rows}) > 1                      # the sweeps' own Δ, not one state's


@pytest.mark.parametrize("tb", [1, 2])
def test_simulation_chains_option_on_oracle(dwhmc, tmp_path, tb):
    _simulate(dwhmc, tmp_path / "with", _OracleOperator, chains=2, operator_response=SIM_OPT, transport_batch=tb,
              **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", _OracleOperator, chains=2, transport_batch=tb, **SIM_KW)
    for k in range(2):
        _check_sim_outputs(tmp_path / "with" / f"c{k}", tmp_path / "without" / f"c{k}")


def test_simulation_option_rejects_unknown_keys(dwhmc, tmp_path):
    for k, opt in enumerate((dict(ops=SIM_OPS, momenta=[(0, 1)]), dict(ops=[("charge", (0, 0))]),
                             dict(ops=SIM_OPS, omega=dict(start=0.0, step=0.1, n=3)))):
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"a{k}", _OracleOperator, operator_response=opt, **SIM_KW)
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"b{k}", _OracleOperator, chains=2, operator_response=opt, **SIM_KW)


# --------------------------------------------------------------------------- GPU
def _measure(ctx, ops, nl=NL, omega=OMEGA, eta=ETA, **kw):
    return ctx.measure_operator_response([v for _, v in ops], n_matsubara=nl, omega=omega, eta=eta, **kw)


def _check_parity(got, ops, chi, chi2, what):
    assert got["chi"].shape == chi.shape and got["chi2"].shape == chi2.shape, what
    for k, (name, _) in enumerate(ops):
        print(what, name, "max|Δchi|", float(np.abs(got["chi"][k] - chi[k]).max()), "max|Δchi2|",
              float(np.abs(got["chi2"][k] - chi2[k]).max()), "max|chi2|", float(np.abs(chi2[k]).max()))
    for k, (name, _) in enumerate(ops):
        _close(got["chi"][k], chi[k], (what, name, "chi"))
        _close_max(got["chi2"][k], chi2[k], (what, name, "chi2"))


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (6, 6), (5, 7), (2, 4), (12, 11)])
def test_parity_with_numpy(dwhmc, oracle, VX, Lx, Ly):
    """2N = 32; 72 and 70 (tails in every tile, odd and unequal sides); the
    Lx = 2 ring; 264 (one full 256-pair tile plus a tail of 8)."""
    p, dis, D, ref, ops, chi, chi2 = _ref_case(oracle, VX, Lx, Ly)
    for _, v in ops[:2]:
        V = v.dense(p.N)
        _close_max(ref.chi2(V, v.spin_sign, _grid(OMEGA), ETA, reverse=True), ref.chi2(V, v.spin_sign, _grid(OMEGA), ETA),
                   "reversed order", tol=TOL / 10)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, ops)
    ctx.close()
    assert np.array_equal(got["omega"], _grid(OMEGA))
    _check_parity(got, ops, chi, chi2, (Lx, Ly))


@pytest.mark.gpu
def test_parity_16x16_grouped(dwhmc, oracle, VX, monkeypatch):
    """2N = 512: exactly two tiles per column, several product tiles;
    DWHMC_RESPONSE_GROUP=2 makes the eight operators four groups, bit-equal to one group."""
    monkeypatch.setenv("DWHMC_RESPONSE_GROUP", "2")
    p, dis, D, ref, ops, chi, chi2 = _ref_case(oracle, VX, 16, 16)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, ops)
    monkeypatch.delenv("DWHMC_RESPONSE_GROUP")
    one = _measure(ctx, ops)
    again = _measure(ctx, ops)
    ctx.close()
    _check_parity(got, ops, chi, chi2, "16x16")
    for k in ("chi", "chi2"):
        assert one[k].tobytes() == got[k].tobytes(), k
        assert one[k].tobytes() == again[k].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [1, 257])
def test_omega_blocks(dwhmc, oracle, VX, nw):
    """n_w = 1 and 257 (one ω block plus one) at 4 x 4."""
    p, dis, D, ref, ops, _, _ = _ref_case(oracle, VX, 4, 4)
    omega = (-1.1, 0.01, nw)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, ops, nl=1, omega=omega)
    ctx.close()
    chi, chi2 = _want(ref, ops, nl=1, omega=omega)
    _check_parity(got, ops, chi, chi2, ("nw", nw))


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(6, 6), (5, 7)])
def test_consistent_with_existing_device_results(dwhmc, oracle, VX, Lx, Ly):
    """The current vertex against measure_current_response (both directions),
    χ''/ω of the q = 0 x-current against measure_transport's σ(ω), and
    identities 3 and 4 from the device."""
    p, dis, D, ref, _, _, _ = _ref_case(oracle, VX, Lx, Ly)
    qs = [(0, 0), (1, 2), (0, -1)]
    eta, domega, wmax = 0.01, 0.002, 4.0
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    tr = ctx.measure_transport(eta, domega, wmax)
    w = tr["omega_grid"]
    lam = {a: ctx.measure_current_response(direction=a, q=qs, n_matsubara=NL)["lam"] for a in "xy"}
    cur = {a: ctx.measure_operator_response([VX.current(p, mx, my, a) for mx, my in qs], n_matsubara=NL)
           for a in "xy"}
    sig = ctx.measure_operator_response([VX.current(p, 0, 0, "x")], n_matsubara=0, omega=(eta, domega, len(w)),
                                        eta=eta)
    site = ctx.measure_operator_response([VX.spin(p, 0, 0), VX.density(p, 1, 2), VX.density(p, -1, -2),
                                          VX.spin(p, 0, -1), VX.spin(p, 0, 1)], n_matsubara=NL,
                                         omega=(-0.6, 0.3, 5), eta=ETA)
    ctx.close()
    for a in "xy":
        assert cur[a]["chi2"].shape == (3, 0)
        _close(cur[a]["chi"], lam[a], ("lam", a))
    got = sig["chi2"][0] / w
    print("sigma", float(np.abs(got - tr["optical_conductivity"]).max()), float(np.abs(got).max()))
    _close_max(got, tr["optical_conductivity"], "sigma")
    _close(site["chi"][0, 0], float(np.sum(p.beta * ref.f * (1 - ref.f))) / p.N, "identity 3")
    assert np.all(np.abs(site["chi"][0, 1:]) <= TOL)
    _close_max(site["chi2"][1][::-1], -site["chi2"][2], "identity 4 density")     # the grid is symmetric about 0
    _close_max(site["chi2"][3][::-1], -site["chi2"][4], "identity 4 spin")


@pytest.mark.gpu
@pytest.mark.parametrize("quat", ["0", "1"])
@pytest.mark.parametrize("mu", [-1.0, 0.0])
def test_degenerate_spectra(dwhmc, oracle, VX, monkeypatch, mu, quat):
    """Clean 8 x 8 at μ = -1 and μ = 0 (exact zero modes), both solvers."""
    monkeypatch.setenv("DWHMC_EIG_QUAT", quat)
    key = ("clean", mu)
    if key not in _refs:
        p, dis, D = _clean(oracle, 8, mu)
        ref = _Ref(oracle, p, dis, D)
        ops = _opset(VX, p)
        _refs[key] = (p, dis, D, ref, ops) + _want(ref, ops)
    p, dis, D, ref, ops, chi, chi2 = _refs[key]
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, ops)
    ctx.close()
    _check_parity(got, ops, chi, chi2, key)


@pytest.mark.gpu
def test_snapshots_chains_and_state_untouched(dwhmc, oracle, VX):
    """deltas with 3 states equals three single calls bit for bit; chain 1 of
    a 2-chain context; the context's Δ is unchanged."""
    O = oracle
    p, dis, D, ref, ops, chi, chi2 = _ref_case(O, VX, 6, 6)
    p2, dis2, D2 = _case(O, 6, 6, 8.0, seed=77)
    ref2 = _Ref(O, p2, dis2, D2)
    rng = np.random.default_rng(8)
    fields = np.stack([D2, D2 * np.exp(0.1j), D2 + 0.05 * rng.standard_normal(D2.shape)])
    ctx = _ctx(dwhmc, p, np.stack([dis, dis2]))
    ctx.set_pairing(np.stack([D, D2]))
    before, _ = ctx.get_state()
    r3 = _measure(ctx, ops, chain=1, deltas=fields)
    ones = [_measure(ctx, ops, chain=1, deltas=fields[s:s + 1]) for s in range(3)]
    dev1 = _measure(ctx, ops, chain=1)                               # the device Δ of chain 1 = fields[0]
    dev0 = _measure(ctx, ops, chain=0)
    after, _ = ctx.get_state()
    ctx.close()
    assert np.array_equal(before, after)
    assert r3["chi"].shape == (3, len(ops), NL) and r3["chi2"].shape == (3, len(ops), OMEGA[2])
    for k in ("chi", "chi2"):
        for s in range(3):
            assert ones[s][k][0].tobytes() == r3[k][s].tobytes(), (k, s)
        assert dev1[k].tobytes() == r3[k][0].tobytes(), k
    c1, c12 = _want(ref2, ops)
    _check_parity(dict(chi=r3["chi"][0], chi2=r3["chi2"][0]), ops, c1, c12, "chain 1")
    c2, c22 = _want(_Ref(O, p2, dis2, fields[2]), ops)
    _check_parity(dict(chi=r3["chi"][2], chi2=r3["chi2"][2]), ops, c2, c22, "snapshot 2")
    _check_parity(dev0, ops, chi, chi2, "chain 0")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dense", "eig"])
def test_other_algorithms(dwhmc, oracle, VX, algo):
    p, dis, D, ref, ops, chi, chi2 = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis, algo=algo)
    ctx.set_pairing(D)
    assert ctx.info["algo"] == {"dense": 0, "eig": 2}[algo]
    got = _measure(ctx, ops)
    ctx.close()
    _check_parity(got, ops, chi, chi2, algo)


@pytest.mark.gpu
def test_skipped_parts_and_argument_errors(dwhmc, oracle, VX):
    p, dis, D, ref, ops, chi, chi2 = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    try:
        full = _measure(ctx, ops)
        only_w = _measure(ctx, ops, nl=0)
        only_l = ctx.measure_operator_response([v for _, v in ops], n_matsubara=NL)
        assert only_w["chi"].shape == (len(ops), 0) and only_l["chi2"].shape == (len(ops), 0)
        assert only_w["chi2"].tobytes() == full["chi2"].tobytes()
        assert only_l["chi"].tobytes() == full["chi"].tobytes()
        # the generic CSR form with explicit signs
        rowptr, col, val = VX.union_csr([v for _, v in ops], p.N)
        csr = ctx.measure_operator_response((rowptr, col, val), [v.spin_sign for _, v in ops], n_matsubara=NL,
                                            omega=OMEGA, eta=ETA)
        assert csr["chi"].tobytes() == full["chi"].tobytes() and csr["chi2"].tobytes() == full["chi2"].tobytes()

        lib, h = ctx._lib, ctx._h
        sg = np.array([v.spin_sign for _, v in ops], dtype=np.int32)
        o1, o2 = np.zeros(len(ops) * NL), np.zeros(len(ops) * 5)
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

        def call(chain=0, ns=1, nops=len(ops), rp=rowptr, cl=col, nnz=len(col), vl=val, s=sg, nl=NL, c1=o1, eta=ETA,
                 w0=-0.6, dw=0.3, nw=5, c2=o2):
            return lib.dwh_measure_operator_response(h, chain, ns, None, nops, P(rp), P(cl), nnz, P(vl), P(s), nl,
                                                     P(c1), eta, w0, dw, nw, P(c2))

        assert call() == 0
        bad_col = col.copy()
        bad_col[0] = p.N
        bad_rp = rowptr.copy()
        bad_rp[1], bad_rp[2] = rowptr[2] + 1, rowptr[1]
        bad_sg = sg.copy()
        bad_sg[1] = 0
        for kw in (dict(chain=1), dict(chain=-1), dict(ns=2), dict(ns=0), dict(nops=0), dict(nnz=0),
                   dict(nnz=len(col) - 1), dict(rp=bad_rp), dict(cl=bad_col), dict(s=bad_sg), dict(rp=None),
                   dict(cl=None), dict(vl=None), dict(s=None), dict(nl=-1), dict(nw=-1), dict(nl=0, nw=0),
                   dict(c1=None), dict(c2=None), dict(eta=0.0), dict(eta=-0.1), dict(eta=float("nan")),
                   dict(w0=float("inf")), dict(dw=float("nan"))):
            assert call(**kw) == -1, kw
            assert lib.dwh_last_error(h), kw
        assert call(c1=None, nl=0) == 0 and call(c2=None, nw=0) == 0       # NULL is fine with a zero count
        for kw in (dict(omega=OMEGA), dict(omega=OMEGA, eta=0.0), dict(n_matsubara=0), dict(chain=1),
                   dict(omega=dict(start=0, step=1, n=2), eta=ETA)):
            with pytest.raises(ValueError):
                ctx.measure_operator_response([v for _, v in ops], **kw)
        with pytest.raises(ValueError):
            ctx.measure_operator_response([v.dense(p.N) for _, v in ops])  # dense operators need spin_sign
        # the context still measures after the refusals
        _check_parity(_measure(ctx, ops), ops, chi, chi2, "after errors")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_timer(dwhmc, oracle, VX):
    p, dis, D, ref, ops, _, _ = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    ctx.timing_enable(["operator"])
    _measure(ctx, ops)
    _measure(ctx, ops[:2], nl=1, omega=None, deltas=np.stack([D, D, D]))
    ms, launches, work = ctx.timing_read("operator")
    ctx.close()
    assert launches == 1 + 3 and ms > 0
    assert work == 8.0 * (2 * p.N) ** 3 * (len(ops) * 1 + 2 * 3)


@pytest.mark.gpu
def test_existing_measurements_unchanged_after_a_call(dwhmc, oracle, VX):
    """measure_current_response and measure_transport return the same bytes
    before and after the new entry ran on the context: the workspaces they
    share with it are re-uploaded, not corrupted."""
    p, dis, D, ref, ops, _, _ = _ref_case(oracle, VX, 6, 6)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    qs = [(0, 0), (0, 1), (1, 2)]

    def both():
        r = ctx.measure_current_response(direction="y", q=qs, n_matsubara=NL)
        t = ctx.measure_transport(0.01, 0.002, 4.0)
        return [np.float64(r["dia"]).tobytes(), r["lam"].tobytes()] + [
            np.asarray(t[k]).tobytes() for k in ("superfluid_stiffness", "dc_conductivity", "optical_conductivity",
                                                 "dos", "dos_AN", "A_k_omega0")]

    before = both()
    _measure(ctx, ops)
    after = both()
    _measure(ctx, ops, deltas=np.stack([D, D]))
    after2 = both()
    ctx.close()
    assert before == after == after2
