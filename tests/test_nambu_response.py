"""Cross response of general Nambu vertices (dwh_measure_nambu_response,
csrc/dwhmc_nambu.hip).  In the basis Ψ = (c_{i↑}; c†_{i↓}) any complex 2N x 2N
W is the operator Ψ† W Ψ; with X^k = U^H W_k U, M = X^a conj(X^b) for a pair
(a, b), ΔE_nm = E_m - E_n:

    chi[l]  = (1/N) Σ_nm [r_nm(l) + i s_nm(l)] M_nm,   (f_n - f_m)/(ΔE - iΩ_l), the
              l = 0 rules of the current response
    chi2[j] = (π/N) Σ_nm (f_n - f_m) M_nm L_η(ω_j - ΔE_nm),  |f_n - f_m| >= 1e-12.

The reference is the numpy restatement tests/nambu_reference.py on the
oracle's `evaluate` eigenpairs (LAPACK).  Tolerances are the project's
(tests/test_transport.py header), on real and imaginary parts separately:
scalars |Δ| <= 1e-9 (1 + |ref|), curves max|Δ| <= 1e-9 (1 + max|ref|); the
restatement summed in the reversed order agrees with itself within a tenth of
that.

CPU (not gpu): identities I1-I4 on the restatement (symmetry, H as a null
vector, the equation of motion, the clean d-wave pair bubble with its quoted
values), the reduction to the operator response, vertices.py (nambu,
hamiltonian, pair_field, commutator_with_h and the continuity equation on the
host), dwh_debug_nambu_dense with its argument errors, the NULL-context
refusal and the driver option on the oracle backend.  GPU: parity on lattices
below / at / above the 256-row tile with tails and every pair-group size, the
grouping loop, ω blocks and Matsubara chunks, agreement with
measure_operator_response, I2-I4 from the device, injected eigensystems against
the long double restatement, snapshots, chains, algorithms, skipped parts,
errors, the timer and a workspace guard.
"""
import ctypes as C
import os

import numpy as np
import pytest

import measure_reference as R
from nambu_reference import LD, NRef, OracleNambu, grid as _grid
from oracle_measurements import OperatorRef as _RefOperator, simulate as _simulate
from test_current_response import SIM_KW, T, TP, MU, _case, _ctx
from test_operator_response import _bands

TOL = 1e-9
NL = 3
ETA = 0.05
OMEGA = (-0.6, 0.3, 5)


def _close(a, b, what=""):
    """scalars: |Δ| <= TOL (1 + |ref|) on real and imaginary parts separately"""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for part in (np.real, np.imag):
        err = np.abs(part(a) - part(b))
        assert np.all(err <= TOL * (1 + np.abs(part(b)))), (what, part.__name__, float(err.max()), a, b)


def _close_max(a, b, what="", tol=TOL):
    """curves: max|Δ| <= tol (1 + max|ref|) on real and imaginary parts separately"""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return
    for part in (np.real, np.imag):
        err = float(np.abs(part(a) - part(b)).max())
        assert err <= tol * (1 + float(np.abs(part(b)).max())), (what, part.__name__, err)


@pytest.fixture(scope="module")
def VX(dwhmc):
    return dwhmc.vertices


def _random_w(VX, N, seed):
    """Dense-ish complex non-Hermitian W over 2N with duplicate (row, col) entries."""
    rng = np.random.default_rng(seed)
    n = 12 * N
    row, col = rng.integers(0, 2 * N, n), rng.integers(0, 2 * N, n)
    row[1], col[1] = row[0], col[0]
    row[-1], col[-1] = row[2], col[2]
    val = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return VX.NambuVertex(row.astype(np.int64), col.astype(np.int64), val)


def _vset(VX, p, dis, D):
    """The parity set: (name, NambuVertex)."""
    return [("density(1,0)", VX.nambu(VX.density(p, 1, 0), p.N)),
            ("current_x(0,1)", VX.nambu(VX.current(p, 0, 1, "x"), p.N)),
            ("d create", VX.pair_field(p, 0, 0, "d", "create")),
            ("d amplitude", VX.pair_field(p, 0, 0, "d", "amplitude")),
            ("d phase", VX.pair_field(p, 1, 0, "d", "phase")),
            ("hamiltonian", VX.hamiltonian(p, dis, D)),
            ("random", _random_w(VX, p.N, 5 + p.N))]


# diagonal and off-diagonal pairs; the first k of the list make the pair counts
# 1 .. 7: every instantiated group size P = 1 .. 4 alone, and 4 + 1, 4 + 2, 4 + 3
PAIRS = [(2, 2), (0, 1), (3, 4), (6, 6), (2, 6), (5, 0), (1, 1)]

_refs = {}


def _ref_case(O, VX, Lx, Ly, beta=8.0):
    """(p, disorder, Δ, NRef, vertices, dense, chi, chi2) of a disordered lattice, once per module."""
    key = (Lx, Ly, beta)
    if key not in _refs:
        p, dis, D = _case(O, Lx, Ly, beta, seed=4 if (Lx, Ly) == (2, 4) else Lx * 17 + Ly)
        ref = NRef.from_oracle(O, p, dis, D)
        vs = _vset(VX, p, dis, D)
        Ws = [v.dense(p.N) for _, v in vs]
        _refs[key] = (p, dis, D, ref, vs, Ws) + ref.response(Ws, PAIRS, NL, _grid(OMEGA), ETA)
    return _refs[key]


# --------------------------------------------------------------------------- CPU
def test_i1_symmetry(oracle, VX):
    p, dis, D, ref, vs, Ws, chi, chi2 = _ref_case(oracle, VX, 6, 4, beta=4.0)
    w = _grid(OMEGA)
    for a, b in ((0, 1), (2, 6), (4, 5)):
        _close_max(ref.chi2(Ws[b], Ws[a], w, ETA), np.conj(ref.chi2(Ws[a], Ws[b], w, ETA)), ("chi2", a, b))
        _close(ref.chi(Ws[b], Ws[a], 1), np.conj(ref.chi(Ws[a], Ws[b], 1)), ("chi0", a, b))
        _close_max(ref.chi2(Ws[a], Ws[b], w, ETA, reverse=True), ref.chi2(Ws[a], Ws[b], w, ETA), "reversed",
                   tol=TOL / 10)
    assert np.abs(ref.chi(Ws[0], Ws[1], NL)[1:] - np.conj(ref.chi(Ws[1], Ws[0], NL)[1:])).max() > 1e-6
    for k in (3, 4, 5):                                   # Hermitian W
        assert np.abs(Ws[k] - Ws[k].conj().T).max() <= 1e-15
        assert np.abs(ref.chi(Ws[k], Ws[k], NL).imag).max() <= TOL
        assert np.abs(ref.chi2(Ws[k], Ws[k], w, ETA).imag).max() <= TOL
    assert np.abs(ref.chi(Ws[6], Ws[6], NL).imag).max() > 1e-6      # not for a non-Hermitian one


def test_i2_hamiltonian_is_a_null_vector(oracle, VX):
    p, dis, D, ref, vs, Ws, _, _ = _ref_case(oracle, VX, 6, 4, beta=4.0)
    H = Ws[5]
    f = np.asarray(ref.f, dtype=np.float64)
    for b in (0, 2, 6):
        chi = ref.chi(H, Ws[b], NL)
        want = p.beta / p.N * np.sum(f * (1 - f) * ref.E * np.conj(np.diagonal(ref.x(Ws[b]))))
        print("I2", b, chi, want)
        assert np.abs(chi[1:]).max() <= TOL
        assert np.abs(ref.chi2(H, Ws[b], _grid(OMEGA), ETA)).max() <= TOL
        _close(chi[0], want, ("chi0", b))
    assert abs(ref.chi(H, Ws[0], 1)[0]) > 1e-3


def test_i3_equation_of_motion(oracle, VX):
    p, dis, D, ref, vs, Ws, _, _ = _ref_case(oracle, VX, 6, 4, beta=4.0)
    F = (ref.U * np.asarray(ref.f, dtype=np.float64)[None, :]) @ ref.U.conj().T
    for b in (0, 2, 6):
        Wb = Ws[b]
        Wa = VX.commutator_with_h(vs[b][1], p, dis, D).dense(p.N)
        assert np.abs(Wa - 1j * (Ws[5] @ Wb - Wb @ Ws[5])).max() <= 1e-12 * (1 + np.abs(Wb).max())
        got = ref.chi(Wa, Wb, 1)[0]
        want = -1j / p.N * np.trace(F @ (Wb @ Wb.conj().T - Wb.conj().T @ Wb))
        print("I3", b, got, want)
        _close(got, want, b)


def _free(O, VX, Lx=6, Ly=4, beta=4.0, mu=MU):
    p = O.ModelParameters(Lx, Ly, T, TP, mu, 0.0, 0.0, beta, 0.8, 1.0)
    return p, np.zeros(p.N), np.zeros((p.N, 2), dtype=np.complex128)


def _bubble(p, nl):
    """I4: the clean q = 0 d-wave pair bubble per Matsubara index."""
    kx, ky, eps = _bands(p)
    g2 = 4 * (np.cos(kx) - np.cos(ky)) ** 2
    th = np.tanh(p.beta * eps / 2)
    out = np.empty(nl, dtype=np.complex128)
    zero = np.abs(2 * eps) < 1e-8
    out[0] = np.sum(g2 * np.where(zero, p.beta / 4, th / np.where(zero, 1.0, 2 * eps))) / p.N
    for l in range(1, nl):
        om = 2 * np.pi * l / p.beta
        den = 4 * eps * eps + om * om
        out[l] = np.sum(g2 * th * 2 * eps / den) / p.N - 1j * np.sum(g2 * th * om / den) / p.N
    return out


def test_i4_clean_pair_bubble(oracle, VX):
    p, dis, D = _free(oracle, VX)
    ref = NRef.from_oracle(oracle, p, dis, D)
    Cd = VX.pair_field(p, 0, 0, "d", "create").dense(p.N)
    got, want = ref.chi(Cd, Cd, 2), _bubble(p, 2)
    print("I4", got, want)
    _close(got, want, "bubble")
    assert abs(want[0] - 2.43182495) <= 5e-9 and abs(want[1] - (0.78694835 + 0.60016811j)) <= 1e-8


def test_diagonal_lifted_pairs_are_the_operator_response(oracle, VX):
    """a = b, W = V ⊕ (-s V^T): Re chi and chi2 are the operator response's χ and χ''."""
    p, dis, D = _case(oracle, 5, 7, 8.0, seed=5 * 17 + 7)
    ref, old = NRef.from_oracle(oracle, p, dis, D), _RefOperator(oracle, p, dis, D)
    w = _grid(OMEGA)
    for v in (VX.density(p, 1, 2), VX.spin(p, 0, -1), VX.current(p, 1, 0, "y"), VX.raman_b1g(p)):
        W = VX.nambu(v, p.N).dense(p.N)
        _close(ref.chi(W, W, NL).real, old.chi(v.dense(p.N), v.spin_sign, NL), "chi")
        c2 = ref.chi2(W, W, w, ETA)
        _close_max(c2.real, old.chi2(v.dense(p.N), v.spin_sign, w, ETA), "chi2")
        assert np.abs(c2.imag).max() <= 1e-15


def _raw_csr(n, row, col, vals):
    """CSR with the triplets as given: rows grouped, columns in the caller's order, duplicates kept."""
    order = np.argsort(row, kind="stable")
    rowptr = np.searchsorted(row[order], np.arange(n + 1)).astype(np.int64)
    return rowptr, np.ascontiguousarray(col[order], dtype=np.int64), np.ascontiguousarray(
        np.atleast_2d(vals)[:, order], dtype=np.complex128)


def _call_dense(lib, N, rowptr, col, val, pairs=((0, 0),), nops=None, nnz=None, npairs=None, out=True):
    val = None if val is None else np.ascontiguousarray(np.atleast_2d(val), dtype=np.complex128)
    nops = (val.shape[0] if val is not None else 1) if nops is None else nops
    nnz = (len(col) if col is not None else 1) if nnz is None else nnz
    pr = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    npairs = (len(pr) if pr is not None else 1) if npairs is None else npairs
    buf = np.full((max(nops, 1), 2 * N, 2 * N), np.nan + 0j, dtype=np.complex128) if out else None
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_debug_nambu_dense(N, nops, P(rowptr), P(col), nnz, P(val), npairs, P(pr), P(buf))
    return rc, (None if buf is None else buf.transpose(0, 2, 1))    # column-major -> [k, row, col]


def test_nambu_lift_matches_debug_operator_nambu(dwhmc, oracle, VX):
    """vertices.nambu(v) is the matrix dwh_debug_operator_nambu builds for v."""
    from test_operator_response import _call_nambu
    lib = dwhmc.load_library()
    p, _, _ = _case(oracle, 2, 4, 8.0, seed=4)
    for v in (VX.density(p, 1, 0), VX.spin(p, 1, -1), VX.current(p, 1, 0, "x"), VX.raman_b2g(p, 0, 1)):
        rowptr, col, val = VX.union_csr([v], p.N)
        rc, want = _call_nambu(lib, p.N, rowptr, col, val, v.spin_sign)
        assert rc == 0
        assert np.abs(VX.nambu(v, p.N).dense(p.N) - want[0]).max() <= 1e-15
        assert np.abs(VX.nambu(v, p).dense(p.N) - want[0]).max() <= 1e-15       # p in place of N


@pytest.mark.parametrize("Lx,Ly", [(4, 4), (5, 7), (2, 4), (1, 3)])
def test_hamiltonian_is_the_oracles(oracle, VX, Lx, Ly):
    O = oracle
    p, dis, D = _case(O, Lx, Ly, 8.0, seed=3 + Lx)
    cache = O.initialize_cache(p)
    O.init_static_H(cache, p, dis)
    O.update_H_BdG(cache, p, D)
    want = O.hermitian_from_upper(cache.H_base)
    h = VX.hamiltonian(p, dis, D)
    assert len(np.unique(h.row * 2 * p.N + h.col)) == len(h.row)           # no duplicates: nothing is summed
    got = h.dense(p.N)
    assert np.array_equal(got, want)
    assert np.array_equal(got, got.conj().T)


def test_pair_field_symmetry_and_parts(oracle, VX):
    p, _, _ = _case(oracle, 5, 7, 8.0, seed=5)
    N = p.N
    for form in ("d", "s_ext", "s"):
        for mx, my in ((0, 0), (1, -2)):
            Cm = VX.pair_field(p, mx, my, form, "create").dense(N)
            Dm = Cm[:N, N:]
            assert np.abs(Dm - Dm.T).max() <= 1e-15                        # singlet
            assert np.abs(Cm[:N, :N]).max() == 0 and np.abs(Cm[N:]).max() == 0
            assert np.abs(VX.pair_field(p, mx, my, form, "destroy").dense(N) - Cm.conj().T).max() <= 1e-15
            A = VX.pair_field(p, mx, my, form, "amplitude").dense(N)
            Ph = VX.pair_field(p, mx, my, form, "phase").dense(N)
            assert np.abs(A - (Cm + Cm.conj().T)).max() <= 1e-15 and np.abs(A - A.conj().T).max() <= 1e-15
            assert np.abs(Ph - 1j * (Cm - Cm.conj().T)).max() <= 1e-15 and np.abs(Ph - Ph.conj().T).max() <= 1e-15
    kx, ky, _ = _bands(p)
    i = np.arange(N)
    x, y = i % p.Lx, i // p.Lx
    Dm = VX.pair_field(p, 0, 0, "d", "create").dense(N)[:N, N:]
    k1, k2 = 2, 3                                                           # D_k = 2 (cos kx - cos ky)
    e = np.exp(1j * (kx[k1, 0] * x + ky[0, k2] * y))
    assert abs(np.vdot(e, Dm @ e) / N - 2 * (np.cos(kx[k1, 0]) - np.cos(ky[0, k2]))) <= 1e-13
    assert np.array_equal(VX.pair_field(p, 1, 0, "s", "create").dense(N)[:N, N:],
                          np.diag(np.exp(-1j * 2 * np.pi * x / p.Lx)))
    for bad in (dict(form="p"), dict(part="both")):
        with pytest.raises(ValueError):
            VX.pair_field(p, 0, 0, **bad)
    assert set(VX.NAMBU_KINDS) >= set(VX.KINDS) | {"pair_d_create", "pair_s_ext_phase", "pair_s_amplitude"}
    assert np.array_equal(VX.build_nambu("pair_d_phase", p, 1, -2).dense(N),
                          VX.pair_field(p, 1, -2, "d", "phase").dense(N))
    assert np.array_equal(VX.build_nambu("spin", p, 1, 0).dense(N), VX.nambu(VX.spin(p, 1, 0), N).dense(N))
    with pytest.raises(ValueError):
        VX.build_nambu("charge", p)


def test_continuity_on_the_host(oracle, VX):
    """i[H, ρ_q] at fixed Δ = the lattice current divergence (every bond's
    current i t_b φ_b times 2i sin(q·δ_b/2), normal blocks only) + a purely
    anomalous pair source -i (Δ̃ V + V Δ̃) ⊕ h.c.-like lower block."""
    p, dis, D = _case(oracle, 5, 7, 8.0, seed=5 * 17 + 7)
    N = p.N
    nn, nnn = p.nn_table - 1, p.nnn_table - 1
    i = np.arange(N)
    x, y = i % p.Lx, i // p.Lx
    Hd = VX.hamiltonian(p, dis, D).dense(N)
    for mx, my in ((1, 0), (1, -2), (0, 0)):
        qx, qy = 2 * np.pi * mx / p.Lx, 2 * np.pi * my / p.Ly
        rho = VX.density(p, mx, my)
        got = VX.commutator_with_h(VX.nambu(rho, N), p, dis, D).dense(N)
        div = np.zeros((N, N), dtype=np.complex128)
        for j, tb, (dx, dy) in ((nn[:, 0], p.t, (1, 0)), (nn[:, 1], p.t, (0, 1)), (nnn[:, 0], p.tp, (1, 1)),
                                (nnn[:, 3], p.tp, (1, -1))):
            cur = 1j * tb * np.exp(-1j * (qx * (x + dx / 2) + qy * (y + dy / 2)))      # J[i, j_b]; J[j_b, i] = -cur
            s2 = 2j * np.sin((qx * dx + qy * dy) / 2)
            np.add.at(div, (i, j), s2 * cur)
            np.add.at(div, (j, i), -s2 * cur)
        normal = VX.nambu(VX.Vertex(*np.nonzero(div), div[np.nonzero(div)], +1), N).dense(N) if mx or my else \
            np.zeros((2 * N, 2 * N))
        src = got - normal
        scale = 1 + np.abs(got).max()
        assert np.abs(src[:N, :N]).max() <= 1e-13 * scale and np.abs(src[N:, N:]).max() <= 1e-13 * scale, (mx, my)
        V, Dt = rho.dense(N), Hd[:N, N:]
        assert np.abs(src[:N, N:] + 1j * (Dt @ V + V @ Dt)).max() <= 1e-13 * scale
        assert np.abs(src[N:, :N] - 1j * (Dt.conj().T @ V + V @ Dt.conj().T)).max() <= 1e-13 * scale
        assert np.abs(src[:N, N:]).max() > 0.05                               # the source is there
        if (mx, my) == (1, 0):                                                # and the x divergence is J_x's bonds
            assert np.abs(div).max() > 0.1


def test_debug_nambu_dense(dwhmc, oracle, VX):
    lib = dwhmc.load_library()
    N = 3
    # unsorted columns, a duplicate that adds up, a pair that cancels, row 4 empty, entries in all four blocks
    row = np.array([0, 0, 0, 1, 2, 2, 2, 3, 5, 5, 5])
    col = np.array([5, 1, 3, 0, 4, 4, 0, 3, 2, 2, 1])
    rng = np.random.default_rng(2)
    vals = rng.standard_normal((3, len(row))) + 1j * rng.standard_normal((3, len(row)))
    vals[:, 9] = -vals[:, 8]
    rowptr, c, v = _raw_csr(2 * N, row, col, vals)
    assert rowptr[4] == rowptr[5] and list(c[:3]) == [5, 1, 3]
    rc, got = _call_dense(lib, N, rowptr, c, v, pairs=[(0, 2), (1, 1)])
    assert rc == 0, lib.dwh_last_error(None)
    for k in range(3):
        W = np.zeros((2 * N, 2 * N), dtype=np.complex128)
        np.add.at(W, (row, col), vals[k])
        assert abs(W[5, 2]) <= 1e-15
        assert np.abs(got[k] - W).max() <= 1e-15, k
    # the union pattern of the builders, explicit zeros included
    p, dis, D = _case(oracle, 2, 4, 8.0, seed=4)
    vs = [v for _, v in _vset(VX, p, dis, D)] + [VX.density(p, 0, 1), np.eye(2 * p.N)]
    rowptr, c, v = VX.union_csr_nambu(vs, p.N)
    assert len(rowptr) == 2 * p.N + 1 and v.shape == (len(vs), len(c))
    rc, got = _call_dense(lib, p.N, rowptr, c, v)
    assert rc == 0
    for k, w in enumerate(vs[:7]):
        assert np.abs(got[k] - w.dense(p.N)).max() <= 1e-13, k
    assert np.abs(got[7] - VX.nambu(vs[7], p.N).dense(p.N)).max() <= 1e-15
    assert np.array_equal(got[8], np.eye(2 * p.N))
    with pytest.raises(ValueError):
        VX.union_csr_nambu([np.zeros((p.N, p.N))], p.N)
    with pytest.raises(ValueError):
        VX.union_csr_nambu([(np.array([0]), np.array([2 * p.N]), np.array([1.0]))], p.N)


def test_argument_errors_host(dwhmc):
    lib = dwhmc.load_library()
    N = 2
    rowptr = np.array([0, 1, 2, 2, 3], dtype=np.int64)
    col = np.array([1, 0, 3], dtype=np.int64)
    val = np.ones((2, 3), dtype=np.complex128)
    assert _call_dense(lib, N, rowptr, col, val, pairs=[(0, 1)])[0] == 0
    bad = [dict(nops=0), dict(nnz=0), dict(nops=-1),
           dict(rowptr=np.array([1, 1, 2, 2, 3], dtype=np.int64)),
           dict(rowptr=np.array([0, 1, 2, 2, 2], dtype=np.int64)),
           dict(rowptr=np.array([0, 2, 1, 2, 3], dtype=np.int64)),
           dict(col=np.array([1, -1, 3], dtype=np.int64)), dict(col=np.array([1, 2 * N, 3], dtype=np.int64)),
           dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]), dict(pairs=None), dict(npairs=0), dict(npairs=-1),
           dict(rowptr=None), dict(col=None, nnz=3), dict(val=None, nops=1), dict(out=False)]
    for kw in bad:
        args = dict(rowptr=rowptr, col=col, val=val, pairs=[(0, 1)])
        args.update(kw)
        rc, _ = _call_dense(lib, N, args.pop("rowptr"), args.pop("col"), args.pop("val"), **args)
        assert rc == -1, kw
        assert lib.dwh_last_error(None), kw
    # the resident limit: 17 vertices at 2N = 2048 are more than 1 GiB, 16 are not refused for it
    n2 = 2048
    rp = np.zeros(n2 + 1, dtype=np.int64)
    rp[1:] = 1
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    one = np.zeros(1, dtype=np.int64)
    pr = np.zeros(2, dtype=np.int64)
    v17 = np.ones((17, 1), dtype=np.complex128)
    assert lib.dwh_debug_nambu_dense(n2 // 2, 17, P(rp), P(one), 1, P(v17), 1, P(pr), P(v17)) == -1
    assert b"1 GiB" in lib.dwh_last_error(None)


def test_null_context_is_refused(dwhmc):
    lib = dwhmc.load_library()
    buf = np.zeros(16)
    rowptr, col = np.zeros(3, dtype=np.int64), np.zeros(1, dtype=np.int64)
    pr = np.zeros(2, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.dwh_measure_nambu_response(None, 0, 1, None, 1, p(rowptr), p(col), 1, p(buf), 1, p(pr), 1, p(buf),
                                        0.1, 0.0, 0.1, 1, p(buf))
    assert rc == -1
    assert b"NULL" in lib.dwh_last_error(None)
    assert dwhmc.FermionContext.TIMERS.index("nambu") == 15


SIM_V = [("pair_d_create", (0, 0)), ("pair_d_amplitude", (0, 0)), ("density", (1, 0))]
SIM_PAIRS = [(0, 0), (1, 1), (2, 1)]
SIM_OPT = dict(vertices=SIM_V, pairs=SIM_PAIRS, n_matsubara=2, omega=dict(start=-0.2, step=0.2, count=3), eta=0.1)


def _check_sim_outputs(with_opt, without):
    assert not (without / "nambu_response.csv").exists()
    assert not (without / "spectra_bins" / "nambu_chi2_omega.npy").exists()
    for f in ("observables.csv", "transport.csv"):
        assert (with_opt / f).read_bytes() == (without / f).read_bytes(), f
    for f in ("params.json", "omega_grid.npy"):
        assert (with_opt / "spectra_bins" / f).read_bytes() == (without / "spectra_bins" / f).read_bytes(), f
    assert sorted(os.listdir(with_opt / "spectra_bins")) == sorted(os.listdir(without / "spectra_bins") +
                                                                   ["nambu_chi2_omega.npy"])
    assert sorted(os.listdir(with_opt)) == sorted(os.listdir(without) + ["nambu_response.csv"])
    assert np.array_equal(np.load(with_opt / "spectra_bins" / "nambu_chi2_omega.npy"), [-0.2, 0.0, 0.2])
    bins = sorted(f for f in os.listdir(with_opt / "spectra_bins") if f.startswith("sweep_"))
    assert len(bins) == SIM_KW["n_measure"] // SIM_KW["bin_size"]
    for f in bins:
        a, b = np.load(with_opt / "spectra_bins" / f), np.load(without / "spectra_bins" / f)
        assert sorted(a.files) == sorted(b.files + ["nambu_chi2"])
        c2 = a["nambu_chi2"]
        assert c2.shape == (3, 3) and c2.dtype == np.complex128 and np.all(np.isfinite(c2))
        assert np.abs(c2[1].imag).max() <= 1e-12 and abs(c2[1, 1]) <= 1e-12      # Hermitian amplitude vertex
        assert np.abs(c2[0]).max() > 1e-6 and np.abs(c2[2]).max() > 1e-9
        for k in b.files:
            assert np.array_equal(a[k], b[k]), k
    lines = (with_opt / "nambu_response.csv").read_text().splitlines()
    head = lines[0].split(",")
    nm = [f"{kind}[mx={mx};my={my}]" for kind, (mx, my) in SIM_V]
    assert head == ["sweep"] + [f"{part}_chi({nm[a]}|{nm[b]};l={l})" for a, b in SIM_PAIRS for l in range(2)
                                for part in ("re", "im")]
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (SIM_KW["n_measure"], 1 + 3 * 2 * 2)
    assert np.array_equal(rows[:, 0], np.arange(1, SIM_KW["n_measure"] + 1))
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1] > 0) and np.all(rows[:, 5] > 0)
    return rows


@pytest.mark.parametrize("tb", [1, 3])
def test_simulation_option_on_oracle(dwhmc, tmp_path, tb):
    """run_simulation(nambu_response=...) on the oracle backend: one row per
    transport measurement through TransportQueue's batches, the complex chi2
    in the bins; the other files are unchanged; nothing appears without the option."""
    _simulate(dwhmc, tmp_path / "with", OracleNambu, nambu_response=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", OracleNambu, transport_batch=tb, **SIM_KW)
    rows = _check_sim_outputs(tmp_path / "with", tmp_path / "without")
    if tb == 1:
        _simulate(dwhmc, tmp_path / "b3", OracleNambu, nambu_response=SIM_OPT, transport_batch=3, **SIM_KW)
        assert (tmp_path / "b3" / "nambu_response.csv").read_bytes() == \
            (tmp_path / "with" / "nambu_response.csv").read_bytes()
    assert len({tuple(r[1:]) for r in rows}) > 1                      # the sweeps' own Δ, not one state's


@pytest.mark.parametrize("tb", [1, 2])
def test_simulation_chains_option_on_oracle(dwhmc, tmp_path, tb):
    _simulate(dwhmc, tmp_path / "with", OracleNambu, chains=2, nambu_response=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", OracleNambu, chains=2, transport_batch=tb, **SIM_KW)
    for k in range(2):
        _check_sim_outputs(tmp_path / "with" / f"c{k}", tmp_path / "without" / f"c{k}")


def test_simulation_option_rejects_unknown_keys(dwhmc, tmp_path):
    for k, opt in enumerate((dict(vertices=SIM_V, ops=[("density", (0, 0))]), dict(vertices=[("charge", (0, 0))]),
                             dict(vertices=SIM_V, pairs=[(0, 3)]), dict(vertices=SIM_V, pairs=[]),
                             dict(vertices=SIM_V, omega=dict(start=0.0, step=0.1, n=3)),
                             dict(vertices=SIM_V, n_matsubara=0))):
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"a{k}", OracleNambu, nambu_response=opt, **SIM_KW)
        with pytest.raises(ValueError):
            _simulate(dwhmc, tmp_path / f"b{k}", OracleNambu, chains=2, nambu_response=opt, **SIM_KW)


# --------------------------------------------------------------------------- GPU
def _measure(ctx, vs, pairs=PAIRS, nl=NL, omega=OMEGA, eta=ETA, **kw):
    return ctx.measure_nambu_response([v for _, v in vs], pairs, n_matsubara=nl, omega=omega, eta=eta, **kw)


def _check_parity(got, pairs, chi, chi2, what):
    assert got["chi"].shape == chi.shape and got["chi2"].shape == chi2.shape, what
    assert got["chi"].dtype == np.complex128 and got["chi2"].dtype == np.complex128
    for k, pr in enumerate(pairs):
        print(what, pr, "max|Δchi|", float(np.abs(got["chi"][k] - chi[k]).max()) if chi.shape[1] else 0.0,
              "max|Δchi2|", float(np.abs(got["chi2"][k] - chi2[k]).max()) if chi2.shape[1] else 0.0,
              "max|chi2|", float(np.abs(chi2[k]).max()) if chi2.shape[1] else 0.0)
    for k, pr in enumerate(pairs):
        _close(got["chi"][k], chi[k], (what, pr, "chi"))
        _close_max(got["chi2"][k], chi2[k], (what, pr, "chi2"))


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (6, 6), (5, 7), (2, 4), (12, 11)])
def test_parity_with_numpy(dwhmc, oracle, VX, Lx, Ly):
    """2N = 32; 72 and 70 (tails in every tile); the Lx = 2 ring; 264 (one full
    256-row tile plus a tail of 8).  Pair counts 1 .. 7: every group size of
    the chi2 kernel alone and as the partial last group after a full one."""
    p, dis, D, ref, vs, Ws, chi, chi2 = _ref_case(oracle, VX, Lx, Ly)
    _close_max(ref.chi2(Ws[2], Ws[6], _grid(OMEGA), ETA, reverse=True), ref.chi2(Ws[2], Ws[6], _grid(OMEGA), ETA),
               "reversed order", tol=TOL / 10)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    H = ctx.debug_dense_H()
    got = {k: _measure(ctx, vs, PAIRS[:k]) for k in range(1, len(PAIRS) + 1)}
    ctx.close()
    assert vs[5][1].dense(p.N).tobytes() == H.tobytes()                    # vertices.hamiltonian, bit for bit
    assert np.array_equal(got[7]["omega"], _grid(OMEGA)) and np.array_equal(got[7]["pairs"], PAIRS)
    for k in range(1, len(PAIRS) + 1):
        _check_parity(got[k], PAIRS[:k], chi[:k], chi2[:k], ((Lx, Ly), k))


@pytest.mark.gpu
def test_parity_16x16_grouped(dwhmc, oracle, VX, monkeypatch):
    """2N = 512: two tiles per column, every column chunk in use;
    DWHMC_RESPONSE_GROUP=2 splits the seven W U products into four groups,
    bit-equal to one group and to a repeat call."""
    monkeypatch.setenv("DWHMC_RESPONSE_GROUP", "2")
    p, dis, D, ref, vs, Ws, chi, chi2 = _ref_case(oracle, VX, 16, 16)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, vs)
    monkeypatch.delenv("DWHMC_RESPONSE_GROUP")
    one = _measure(ctx, vs)
    again = _measure(ctx, vs)
    ctx.close()
    _check_parity(got, PAIRS, chi, chi2, "16x16")
    for k in ("chi", "chi2"):
        assert one[k].tobytes() == got[k].tobytes(), k
        assert one[k].tobytes() == again[k].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [1, 257, 512, 513, 1025])
def test_omega_blocks(dwhmc, oracle, VX, nw):
    """At 4 x 4.  A thread of k_nb_spec owns two frequencies, so a block covers
    512: n_w = 1; 257 (the second slot of one thread only, a second block of
    the 64-wide sum kernel); 512 (one full block); 513 (one block plus one:
    blockIdx.x = 1 with one live slot) and 1025 (two full blocks plus one)."""
    p, dis, D, ref, vs, Ws, _, _ = _ref_case(oracle, VX, 4, 4)
    omega = (-1.1, 0.01, nw)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, vs, nl=1, omega=omega)
    ctx.close()
    chi, chi2 = ref.response(Ws, PAIRS, 1, _grid(omega), ETA)
    _check_parity(got, PAIRS, chi, chi2, ("nw", nw))


@pytest.mark.gpu
@pytest.mark.parametrize("nl", [1, 8, 9])
def test_matsubara_chunks(dwhmc, oracle, VX, nl):
    """n_matsubara = 1 (the one-index kernel), 8 and 9 (one chunk, one chunk plus one)."""
    p, dis, D, ref, vs, Ws, _, _ = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure(ctx, vs, nl=nl, omega=None)
    ctx.close()
    chi, chi2 = ref.response(Ws, PAIRS, nl, _grid(None), ETA)
    assert got["chi2"].shape == (len(PAIRS), 0)
    _check_parity(got, PAIRS, chi, chi2, ("nl", nl))


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(6, 6), (5, 7)])
def test_agrees_with_the_operator_response(dwhmc, oracle, VX, Lx, Ly):
    """Lifted vertices with (k, k) pairs: Re chi and chi2 are
    measure_operator_response's; Im chi2 vanishes for the Hermitian ones."""
    p, dis, D, _, _, _, _, _ = _ref_case(oracle, VX, Lx, Ly)
    ops = [VX.density(p, 1, 2), VX.spin(p, 0, -1), VX.current(p, 0, 1, "x"), VX.raman_b1g(p), VX.spin(p, 0, 0)]
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    old = ctx.measure_operator_response(ops, n_matsubara=NL, omega=OMEGA, eta=ETA)
    new = ctx.measure_nambu_response(ops, n_matsubara=NL, omega=OMEGA, eta=ETA)           # plain Vertex: lifted
    ctx.close()
    assert np.array_equal(new["pairs"], [(k, k) for k in range(len(ops))])
    for k in range(len(ops)):
        _close(new["chi"][k].real, old["chi"][k], ("chi", k))
        _close_max(new["chi2"][k].real, old["chi2"][k], ("chi2", k))
    for k in (3, 4):                                                           # Hermitian
        assert np.abs(new["chi2"][k].imag).max() <= TOL * (1 + np.abs(old["chi2"][k]).max())
        assert np.abs(new["chi"][k].imag).max() <= TOL


@pytest.mark.gpu
def test_i2_i3_from_the_device(dwhmc, oracle, VX):
    p, dis, D, ref, vs, Ws, _, _ = _ref_case(oracle, VX, 6, 6)
    bs = (0, 2, 6)
    comm = [VX.commutator_with_h(vs[b][1], p, dis, D) for b in bs]
    allv = [v for _, v in vs] + comm
    pairs = [(5, b) for b in bs] + [(len(vs) + k, b) for k, b in enumerate(bs)]
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = ctx.measure_nambu_response(allv, pairs, n_matsubara=NL, omega=OMEGA, eta=ETA)
    ctx.close()
    f = np.asarray(ref.f, dtype=np.float64)
    F = (ref.U * f[None, :]) @ ref.U.conj().T
    for k, b in enumerate(bs):
        want = p.beta / p.N * np.sum(f * (1 - f) * ref.E * np.conj(np.diagonal(ref.x(Ws[b]))))
        print("I2 device", b, got["chi"][k], want, float(np.abs(got["chi2"][k]).max()))
        _close(got["chi"][k, 0], want, ("I2 chi0", b))
        _close(got["chi"][k, 1:], np.zeros(NL - 1), ("I2 chi l>=1", b))
        _close_max(got["chi2"][k], np.zeros(OMEGA[2]), ("I2 chi2", b))
        want3 = -1j / p.N * np.trace(F @ (Ws[b] @ Ws[b].conj().T - Ws[b].conj().T @ Ws[b]))
        print("I3 device", b, got["chi"][3 + k, 0], want3)
        _close(got["chi"][3 + k, 0], want3, ("I3", b))


@pytest.mark.gpu
@pytest.mark.parametrize("quat", ["0", "1"])
@pytest.mark.parametrize("mu", [-1.0, 0.0])
def test_i4_clean_pair_bubble_from_the_device(dwhmc, oracle, VX, monkeypatch, mu, quat):
    """Clean 8 x 8, Δ = 0 at μ = -1 and μ = 0 (degenerate levels, exact zero
    modes), both solvers, against the closed form."""
    monkeypatch.setenv("DWHMC_EIG_QUAT", quat)
    p, dis, D = _free(oracle, VX, 8, 8, beta=8.0, mu=mu)
    Cd = VX.pair_field(p, 0, 0, "d", "create")
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = ctx.measure_nambu_response([Cd], n_matsubara=NL)
    ctx.close()
    want = _bubble(p, NL)
    print("I4 device", mu, quat, got["chi"][0], want)
    _close(got["chi"][0], want, (mu, quat))


def _injected_spectrum(n2, beta):
    """uniform levels in (-2, 2) with a cluster of four within 1e-9, a pair
    across zero and one level behind a huge gap"""
    rng = np.random.default_rng(n2)
    E = rng.uniform(-2.0, 2.0, n2)
    E[:4] = 0.3 + 3e-10 * np.arange(4)
    E[4], E[5] = -1e-11, 1e-11
    E[6] = 1e4
    E = np.sort(E)
    br = R.Branches(E, beta)
    assert not br.ambiguous_df().any()
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (5, 7)])
def test_injected_eigensystems(dwhmc, oracle, VX, Lx, Ly):
    """Haar U and a prescribed spectrum (debug_set_eigensystem) against the
    long double restatement."""
    beta = 8.0
    p, dis, D = _free(oracle, VX, Lx, Ly, beta=beta)
    n2 = 2 * p.N
    E, U = _injected_spectrum(n2, beta), R.haar(n2, 11 + n2)
    vs = [("d amplitude", VX.pair_field(p, 0, 0, "d", "amplitude")), ("random", _random_w(VX, p.N, 3)),
          ("density(1,0)", VX.nambu(VX.density(p, 1, 0), p.N)), ("d create", VX.pair_field(p, 1, 1, "d", "create"))]
    pairs = [(0, 0), (1, 1), (0, 1), (2, 1), (1, 3)]
    ref = NRef(p, E, U, beta=beta, dt=LD)
    chi, chi2 = ref.response([v.dense(p.N) for _, v in vs], pairs, NL, _grid(OMEGA), ETA)
    ctx = _ctx(dwhmc, p, dis, algo="eig")
    ctx.debug_set_eigensystem(E, U)
    got = _measure(ctx, vs, pairs)
    ctx.close()
    _check_parity(got, pairs, chi, chi2, ("injected", Lx, Ly))


@pytest.mark.gpu
def test_snapshots_chains_and_state_untouched(dwhmc, oracle, VX):
    """deltas with 3 states equals three single calls bit for bit; chain 1 of
    a 2-chain context; the context's Δ is unchanged."""
    O = oracle
    p, dis, D, ref, vs, Ws, chi, chi2 = _ref_case(O, VX, 6, 6)
    vs, Ws = vs[:5] + vs[6:], Ws[:5] + Ws[6:]                       # (the hamiltonian vertex belongs to one Δ)
    pairs = [(2, 2), (0, 1), (3, 4), (5, 5), (2, 5)]
    p2, dis2, D2 = _case(O, 6, 6, 8.0, seed=77)
    rng = np.random.default_rng(8)
    fields = np.stack([D2, D2 * np.exp(0.1j), D2 + 0.05 * rng.standard_normal(D2.shape)])
    ctx = _ctx(dwhmc, p, np.stack([dis, dis2]))
    ctx.set_pairing(np.stack([D, D2]))
    before, _ = ctx.get_state()
    r3 = _measure(ctx, vs, pairs, chain=1, deltas=fields)
    ones = [_measure(ctx, vs, pairs, chain=1, deltas=fields[s:s + 1]) for s in range(3)]
    dev1 = _measure(ctx, vs, pairs, chain=1)                         # the device Δ of chain 1 = fields[0]
    dev0 = _measure(ctx, vs, pairs, chain=0)
    after, _ = ctx.get_state()
    ctx.close()
    assert np.array_equal(before, after)
    assert r3["chi"].shape == (3, len(pairs), NL) and r3["chi2"].shape == (3, len(pairs), OMEGA[2])
    for k in ("chi", "chi2"):
        for s in range(3):
            assert ones[s][k][0].tobytes() == r3[k][s].tobytes(), (k, s)
        assert dev1[k].tobytes() == r3[k][0].tobytes(), k
    w = _grid(OMEGA)
    for s, Ds in ((0, D2), (2, fields[2])):
        c, c2 = NRef.from_oracle(O, p2, dis2, Ds).response(Ws, pairs, NL, w, ETA)
        _check_parity(dict(chi=r3["chi"][s], chi2=r3["chi2"][s]), pairs, c, c2, ("chain 1 snapshot", s))
    c, c2 = ref.response(Ws, pairs, NL, w, ETA)
    _check_parity(dev0, pairs, c, c2, "chain 0")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dense", "eig"])
def test_other_algorithms(dwhmc, oracle, VX, algo):
    p, dis, D, ref, vs, Ws, chi, chi2 = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis, algo=algo)
    ctx.set_pairing(D)
    assert ctx.info["algo"] == {"dense": 0, "eig": 2}[algo]
    got = _measure(ctx, vs)
    ctx.close()
    _check_parity(got, PAIRS, chi, chi2, algo)


@pytest.mark.gpu
def test_skipped_parts_and_argument_errors(dwhmc, oracle, VX):
    p, dis, D, ref, vs, Ws, chi, chi2 = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    try:
        full = _measure(ctx, vs)
        only_w = _measure(ctx, vs, nl=0)
        only_l = _measure(ctx, vs, omega=None)
        assert only_w["chi"].shape == (len(PAIRS), 0) and only_l["chi2"].shape == (len(PAIRS), 0)
        assert only_w["chi2"].tobytes() == full["chi2"].tobytes()
        assert only_l["chi"].tobytes() == full["chi"].tobytes()
        # the CSR form, dense matrices and COO triples give the same bits as the vertex list
        rowptr, col, val = VX.union_csr_nambu([v for _, v in vs], p.N)
        csr = ctx.measure_nambu_response((rowptr, col, val), PAIRS, n_matsubara=NL, omega=OMEGA, eta=ETA)
        mixed = ctx.measure_nambu_response([vs[0][1], (vs[1][1].row, vs[1][1].col, vs[1][1].val)] +
                                           [v for _, v in vs[2:]], PAIRS, n_matsubara=NL, omega=OMEGA, eta=ETA)
        for r in (csr, mixed):
            assert r["chi"].tobytes() == full["chi"].tobytes() and r["chi2"].tobytes() == full["chi2"].tobytes()
        # a tuple of three vertices is a collection, not a CSR tuple; one vertex may be passed bare
        three = [v for _, v in vs[:3]]
        as_list = ctx.measure_nambu_response(three, [(0, 1), (2, 2)], n_matsubara=NL, omega=OMEGA, eta=ETA)
        as_tuple = ctx.measure_nambu_response(tuple(three), [(0, 1), (2, 2)], n_matsubara=NL, omega=OMEGA, eta=ETA)
        bare = ctx.measure_nambu_response(three[2], n_matsubara=NL, omega=OMEGA, eta=ETA)
        for k in ("chi", "chi2"):
            assert as_tuple[k].tobytes() == as_list[k].tobytes(), k
            _close_max(bare[k][0], as_list[k][1], ("bare vertex", k))
        dense = ctx.measure_nambu_response(Ws, PAIRS, n_matsubara=NL, omega=OMEGA, eta=ETA)
        _check_parity(dense, PAIRS, chi, chi2, "dense vertices")

        lib, h = ctx._lib, ctx._h
        pr = np.ascontiguousarray(np.asarray(PAIRS, dtype=np.int64))
        o1, o2 = np.zeros(len(PAIRS) * NL, dtype=np.complex128), np.zeros(len(PAIRS) * 5, dtype=np.complex128)
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

        def call(chain=0, ns=1, nops=len(vs), rp=rowptr, cl=col, nnz=len(col), vl=val, np_=len(PAIRS), prs=pr, nl=NL,
                 c1=o1, eta=ETA, w0=-0.6, dw=0.3, nw=5, c2=o2):
            return lib.dwh_measure_nambu_response(h, chain, ns, None, nops, P(rp), P(cl), nnz, P(vl), np_, P(prs), nl,
                                                  P(c1), eta, w0, dw, nw, P(c2))

        assert call() == 0
        assert o1.reshape(len(PAIRS), NL).tobytes() == full["chi"].tobytes()
        bad_col = col.copy()
        bad_col[0] = 2 * p.N
        bad_rp = rowptr.copy()
        bad_rp[1], bad_rp[2] = rowptr[2] + 1, rowptr[1]
        bad_pr = pr.copy()
        bad_pr[1, 1] = len(vs)
        neg_pr = pr.copy()
        neg_pr[0, 0] = -1
        for kw in (dict(chain=1), dict(chain=-1), dict(ns=2), dict(ns=0), dict(nops=0), dict(nnz=0),
                   dict(nnz=len(col) - 1), dict(rp=bad_rp), dict(cl=bad_col), dict(prs=bad_pr), dict(prs=neg_pr),
                   dict(prs=None), dict(np_=0), dict(np_=-1), dict(rp=None), dict(cl=None), dict(vl=None),
                   dict(nl=-1), dict(nw=-1), dict(nl=0, nw=0), dict(c1=None), dict(c2=None), dict(eta=0.0),
                   dict(eta=-0.1), dict(eta=float("nan")), dict(w0=float("inf")), dict(dw=float("nan"))):
            assert call(**kw) == -1, kw
            assert lib.dwh_last_error(h), kw
        assert call(c1=None, nl=0) == 0 and call(c2=None, nw=0) == 0       # NULL is fine with a zero count
        for kw in (dict(omega=OMEGA), dict(omega=OMEGA, eta=0.0), dict(n_matsubara=0), dict(chain=1),
                   dict(omega=dict(start=0, step=1, n=2), eta=ETA), dict(pairs=[(0, len(vs))])):
            with pytest.raises(ValueError):
                ctx.measure_nambu_response([v for _, v in vs], **kw)
        with pytest.raises(ValueError):
            ctx.measure_nambu_response([np.zeros((p.N, p.N))])             # dense vertices are 2N x 2N
        _check_parity(_measure(ctx, vs), PAIRS, chi, chi2, "after errors")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_timer(dwhmc, oracle, VX):
    p, dis, D, ref, vs, Ws, _, _ = _ref_case(oracle, VX, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    ctx.timing_enable(["nambu"])
    _measure(ctx, vs)
    _measure(ctx, vs[:2], [(0, 1)], nl=1, omega=None, deltas=np.stack([D, D, D]))
    ms, launches, work = ctx.timing_read("nambu")
    ops = ctx.timing_read("operator")
    ctx.close()
    assert launches == 1 + 3 and ms > 0
    assert work == 8.0 * (2 * p.N) ** 3 * (len(vs) * 1 + 2 * 3)
    assert ops[1] == 0


@pytest.mark.gpu
def test_existing_measurements_unchanged_after_a_call(dwhmc, oracle, VX):
    """measure_transport, measure_current_response and measure_operator_response
    return the same bytes before and after the new entry ran on the context:
    the workspaces they share with it are re-uploaded, not corrupted."""
    p, dis, D, ref, vs, _, _, _ = _ref_case(oracle, VX, 6, 6)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    qs = [(0, 0), (0, 1), (1, 2)]
    ops = [VX.density(p, 1, 0), VX.spin(p, 0, 1), VX.raman_b1g(p)]

    def others():
        r = ctx.measure_current_response(direction="y", q=qs, n_matsubara=NL)
        t = ctx.measure_transport(0.01, 0.002, 4.0)
        o = ctx.measure_operator_response(ops, n_matsubara=NL, omega=OMEGA, eta=ETA)
        return [np.float64(r["dia"]).tobytes(), r["lam"].tobytes(), o["chi"].tobytes(), o["chi2"].tobytes()] + [
            np.asarray(t[k]).tobytes() for k in ("superfluid_stiffness", "dc_conductivity", "optical_conductivity",
                                                 "dos", "dos_AN", "A_k_omega0")]

    before = others()
    _measure(ctx, vs)
    after = others()
    _measure(ctx, vs, deltas=np.stack([D, D]))
    after2 = others()
    ctx.close()
    assert before == after == after2
