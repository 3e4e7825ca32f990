"""One-body vertices for FermionContext.measure_operator_response, as sparse
triplets on the host (numpy, O(N)).

An operator O = Σ_ij V_ij (c†_{i↑} c_{j↑} + s c†_{i↓} c_{j↓}) is a `Vertex`:
the COO triplets of V (0-based, duplicates add up, as `sparse()` adds them)
and the spin sign s.  Every builder takes (p, mx, my) with the lattice
momentum q = 2π (mx/Lx, my/Ly), m not reduced modulo L (the half-bond phase
is not periodic in m), site i at x = i mod Lx, y = i div Lx, and the midpoint
phase φ_b(i) = exp(-i q·(r_i + δ_b/2)) on a bond b from i to j_b(i) = i + δ_b:

    density, spin   V = diag e^{-i q·r_i},                s = +1 / -1
    current(α)      V[i, j_b] += i t_b φ_b(i), V[j_b, i] -= i t_b φ_b(i)
                    over the bond list of direction α of
                    dwh_measure_current_response,         s = +1
    raman_b1g       V[i, j_b] += g_b t φ_b(i), V[j_b, i] += g_b t φ_b(i),
                    b = (+x, g = +1), (+y, g = -1):  γ_k = 2t (cos kx - cos ky), s = +1
    raman_b2g       the same with t' on (+x+y, +1), (+x-y, -1):
                    γ_k = -4t' sin kx sin ky,             s = +1

For FermionContext.measure_nambu_response a vertex is a `NambuVertex`: the
COO triplets of any complex 2N x 2N matrix W, the operator Ψ† W Ψ in the basis
Ψ = (c_{i↑}; c†_{i↓}); D = W[:N, N:] multiplies c†_{i↑} c†_{j↓}:

    nambu(vertex, N)     V ⊕ (-s V^T) of a Vertex
    pair_field           the singlet pair field of a form factor at q:
                         D[i, j_b] += g_b φ_b(i), D[j_b, i] += g_b φ_b(i)
                         ("d": (+x, +1), (+y, -1); "s_ext": (+x, +1), (+y, +1);
                         "s": D[i, i] = e^{-i q·r_i}); part "create":
                         C = [[0, D], [0, 0]], "destroy": C†, "amplitude":
                         C + C†, "phase": i (C - C†)
    hamiltonian          H_BdG(Δ) itself, entry for entry what the device assembles
    commutator_with_h    i (H W - W H)

For FermionContext.measure_response_map, which samples the linear-response
density matrix D(z)[W] and ρ on a pattern of Nambu index pairs (a, b):

    bond_pattern         (npat, 2): every site with its 4 + 4 neighbours, per block
    contract             Σ_e conj(B_e) D_e = N·chi of the pair (W, B)
    diamagnetic_map,     the local dia_i, Λ_i and stiffness dia_i - Λ_i from ρ and
    paramagnetic_map,    D(0)[J_α(q = 0)]; their site means are the current
    stiffness_map        response's dia, Λ(q = 0, l = 0) and the stiffness

For FermionContext.measure_correlations, the equal-time correlations
C_AB(r) = (1/N) Σ_j <O_A(j ⊕ r) O_B(j)†>_c of local operators, a `LocalFamily`
gives every site i its own bilinear O(i) = Σ_t a_t Ψ†_{row_t} Ψ_{col_t} as
triplets tagged with their owner site:

    local_family         the q = 0 vertex of a NAMBU_KINDS name with every term
                         owned by the site i of the bond (i, j_b(i)) it was built
                         from, so Σ_i O(i) = build_nambu(kind, p, 0, 0)
    local_terms          the term table (tptr, trow, tcol, tval) of a list of families
    disconnected         (1/N) Σ_j m_A(j ⊕ r) conj(m_B(j)) from the means
    structure_factor     S(q) = Σ_r e^{-i q·r} C(r)

Phase convention: a family places a bond operator at its owner site, so the
Fourier transform Σ_r e^{-i q·r} C(r) carries e^{-i q·r_i} per bond where the
q-vertices above carry the midpoint phase e^{-i q·(r_i + δ_b/2)}: the two
differ by e^{-i q·δ_b/2} per bond and agree for on-site operators (density,
spin, pair_s).  S^x S^x is not a Ψ-bilinear (S^x flips one spin, which
changes the Nambu charge by two); S^z S^z ("spin") stands for it by spin
rotation symmetry.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Vertex(NamedTuple):
    row: np.ndarray        # int64
    col: np.ndarray        # int64
    val: np.ndarray        # complex128
    spin_sign: int

    def dense(self, N: int) -> np.ndarray:
        V = np.zeros((N, N), dtype=np.complex128)
        np.add.at(V, (self.row, self.col), self.val)
        return V


def _sites(p):
    i = np.arange(p.N, dtype=np.int64)
    return i, (i % p.Lx).astype(np.float64), (i // p.Lx).astype(np.float64)


def _q(p, mx, my):
    return 2 * np.pi * mx / p.Lx, 2 * np.pi * my / p.Ly


def _bond_lists(p):
    """name -> (neighbour j_b (0-based), bond vector δ_b)."""
    nn, nnn = np.asarray(p.nn_table) - 1, np.asarray(p.nnn_table) - 1
    return {"+x": (nn[:, 0], (1, 0)), "+y": (nn[:, 1], (0, 1)), "+x+y": (nnn[:, 0], (1, 1)),
            "-x+y": (nnn[:, 1], (-1, 1)), "+x-y": (nnn[:, 3], (1, -1))}


def _phase(p, mx, my, d):
    _, x, y = _sites(p)
    qx, qy = _q(p, mx, my)
    return np.exp(-1j * (qx * (x + d[0] / 2) + qy * (y + d[1] / 2)))


def _bond_vertex(p, mx, my, bonds, sym: float, pref: complex) -> Vertex:
    """V[i, j_b] += pref w_b φ_b(i), V[j_b, i] += sym pref w_b φ_b(i) over bonds (name, w_b)."""
    i, _, _ = _sites(p)
    lists = _bond_lists(p)
    rows, cols, vals = [], [], []
    for name, w in bonds:
        j, d = lists[name]
        v = pref * w * _phase(p, mx, my, d)
        rows += [i, j]
        cols += [j, i]
        vals += [v, sym * v]
    return Vertex(np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64),
                  np.concatenate(vals).astype(np.complex128), +1)


def density(p, mx: int = 0, my: int = 0) -> Vertex:
    i, _, _ = _sites(p)
    return Vertex(i, i.copy(), _phase(p, mx, my, (0, 0)).astype(np.complex128), +1)


def spin(p, mx: int = 0, my: int = 0) -> Vertex:
    return density(p, mx, my)._replace(spin_sign=-1)


def _current_bonds(p, direction):
    """(name, t_b) of the bond list of direction α of dwh_measure_current_response."""
    if direction not in ("x", "y", 0, 1):
        raise ValueError("direction must be 'x' or 'y'")
    if direction in ("x", 0):
        return [("+x", p.t), ("+x+y", p.tp), ("+x-y", p.tp)]
    return [("+y", p.t), ("+x+y", p.tp), ("-x+y", p.tp)]


def current(p, mx: int = 0, my: int = 0, direction="x") -> Vertex:
    return _bond_vertex(p, mx, my, _current_bonds(p, direction), -1.0, 1j)


def raman_b1g(p, mx: int = 0, my: int = 0) -> Vertex:
    return _bond_vertex(p, mx, my, [("+x", p.t), ("+y", -p.t)], 1.0, 1.0)


def raman_b2g(p, mx: int = 0, my: int = 0) -> Vertex:
    return _bond_vertex(p, mx, my, [("+x+y", p.tp), ("+x-y", -p.tp)], 1.0, 1.0)


KINDS = {"density": density, "spin": spin, "current_x": lambda p, mx, my: current(p, mx, my, "x"),
         "current_y": lambda p, mx, my: current(p, mx, my, "y"), "raman_b1g": raman_b1g, "raman_b2g": raman_b2g}


def build(kind: str, p, mx: int = 0, my: int = 0) -> Vertex:
    """The vertex named `kind` (a key of KINDS) at momentum indices (mx, my)."""
    if kind not in KINDS:
        raise ValueError(f"unknown vertex kind {kind!r}; one of {sorted(KINDS)}")
    return KINDS[kind](p, int(mx), int(my))


def as_triplets(op, N: int):
    """(row, col, val) of a Vertex, a COO triple or a dense (N, N) matrix."""
    if isinstance(op, Vertex):
        op = (op.row, op.col, op.val)
    if isinstance(op, (tuple, list)) and len(op) == 3:
        r, c, v = (np.asarray(a).ravel() for a in op)
        if not (len(r) == len(c) == len(v)):
            raise ValueError("COO operator: row, col and val differ in length")
        r, c = r.astype(np.int64), c.astype(np.int64)
        if len(r) and (r.min() < 0 or r.max() >= N or c.min() < 0 or c.max() >= N):
            raise ValueError(f"COO operator: index outside [0, {N})")
        return r, c, v.astype(np.complex128)
    V = np.asarray(op, dtype=np.complex128)
    if V.shape != (N, N):
        raise ValueError(f"expected a Vertex, a COO triple or a dense ({N}, {N}) operator")
    r, c = np.nonzero(V)
    return r.astype(np.int64), c.astype(np.int64), V[r, c]


def union_csr(ops, N: int):
    """One CSR pattern for a list of operators: (rowptr (N+1,), col (nnz,),
    val (nops, nnz)), each operator's duplicates added up and the entries it
    lacks explicit zeros.  An all-zero list gets one explicit zero at (0, 0)."""
    trips = [as_triplets(op, N) for op in ops]
    keys = np.concatenate([r * N + c for r, c, _ in trips]) if trips else np.zeros(0, dtype=np.int64)
    pat = np.unique(keys)
    if len(pat) == 0:
        pat = np.zeros(1, dtype=np.int64)
    val = np.zeros((len(trips), len(pat)), dtype=np.complex128)
    for k, (r, c, v) in enumerate(trips):
        np.add.at(val[k], np.searchsorted(pat, r * N + c), v)
    rowptr = np.searchsorted(pat // N, np.arange(N + 1)).astype(np.int64)
    return rowptr, (pat % N).astype(np.int64), val


# --------------------------------------------------------------------------
# general Nambu vertices (FermionContext.measure_nambu_response)
# --------------------------------------------------------------------------
class NambuVertex(NamedTuple):
    row: np.ndarray        # int64, in [0, 2N)
    col: np.ndarray        # int64, in [0, 2N)
    val: np.ndarray        # complex128

    def dense(self, N: int) -> np.ndarray:
        W = np.zeros((2 * N, 2 * N), dtype=np.complex128)
        np.add.at(W, (self.row, self.col), self.val)
        return W


def _nv(rows, cols, vals) -> NambuVertex:
    return NambuVertex(np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64),
                       np.concatenate(vals).astype(np.complex128))


def nambu(vertex: Vertex, N) -> NambuVertex:
    """V ⊕ (-s V^T): the Nambu matrix of a Vertex on N sites (N, or anything with .N)."""
    N = int(getattr(N, "N", N))
    r, c, v = as_triplets(vertex, N)
    return _nv([r, c + N], [c, r + N], [v, -float(vertex.spin_sign) * v])


PAIR_FORMS = {"d": [("+x", 1.0), ("+y", -1.0)], "s_ext": [("+x", 1.0), ("+y", 1.0)], "s": None}
PAIR_PARTS = ("create", "destroy", "amplitude", "phase")


def pair_field(p, mx: int = 0, my: int = 0, form: str = "d", part: str = "create") -> NambuVertex:
    """The singlet pair field Σ D_ij c†_{i↑} c†_{j↓} (D symmetric) of form
    factor `form` at q = 2π (mx/Lx, my/Ly), or its adjoint / Hermitian parts."""
    if form not in PAIR_FORMS:
        raise ValueError(f"unknown pair form {form!r}; one of {sorted(PAIR_FORMS)}")
    if part not in PAIR_PARTS:
        raise ValueError(f"unknown part {part!r}; one of {PAIR_PARTS}")
    i, _, _ = _sites(p)
    N = p.N
    if PAIR_FORMS[form] is None:
        rows, cols, vals = [i], [i], [_phase(p, mx, my, (0, 0))]
    else:
        lists = _bond_lists(p)
        rows, cols, vals = [], [], []
        for name, g in PAIR_FORMS[form]:
            j, d = lists[name]
            v = g * _phase(p, mx, my, d)
            rows += [i, j]
            cols += [j, i]
            vals += [v, v]
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals).astype(np.complex128)
    cre = (r, c + N, v)                       # C = [[0, D], [0, 0]]
    des = (c + N, r, np.conj(v))              # C†
    if part == "create":
        return _nv(*[[a] for a in cre])
    if part == "destroy":
        return _nv(*[[a] for a in des])
    if part == "amplitude":
        return _nv([cre[0], des[0]], [cre[1], des[1]], [cre[2], des[2]])
    return _nv([cre[0], des[0]], [cre[1], des[1]], [1j * cre[2], -1j * des[2]])


def hamiltonian(p, disorder, delta) -> NambuVertex:
    """H_BdG(Δ) as sparse triplets without duplicates: the reference's upper
    triangle (diagonal w_i - μ, hoppings -t / -t' to the neighbours j > i, the
    hole block their negatives, pairing Δ[i, 0]/2 at (i, i+x + N) and
    (i+x, i + N), Δ[i, 1]/2 at +y; later writes overwrite earlier ones, which
    matters on 1- and 2-site rings) and its Hermitian completion."""
    N = p.N
    nn, nnn = np.asarray(p.nn_table) - 1, np.asarray(p.nnn_table) - 1
    disorder = np.asarray(disorder, dtype=np.float64).ravel()
    delta = np.asarray(delta, dtype=np.complex128).reshape(N, 2)
    up = {}
    for i in range(N):
        term = disorder[i] - p.mu
        up[(i, i)] = term
        up[(i + N, i + N)] = -term
    for i in range(N):
        for tab, hop in ((nn, p.t), (nnn, p.tp)):
            for d in range(4):
                j = int(tab[i, d])
                if j > i:
                    up[(i, j)] = -hop
                    up[(i + N, j + N)] = hop
    for i in range(N):
        for b in range(2):
            j = int(nn[i, b])
            v = 0.5 * delta[i, b]
            up[(i, j + N)] = v
            up[(j, i + N)] = v
    rows, cols, vals = [], [], []
    for (r, c), v in up.items():
        rows.append(r)
        cols.append(c)
        vals.append(v)
        if r != c:
            rows.append(c)
            cols.append(r)
            vals.append(np.conj(v))
    return NambuVertex(np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64),
                       np.array(vals, dtype=np.complex128))


def as_nambu_triplets(op, N: int):
    """(row, col, val) over 2N of a NambuVertex, a Vertex (lifted by `nambu`),
    a COO triple or a dense (2N, 2N) matrix."""
    n2 = 2 * N
    if isinstance(op, Vertex):
        op = nambu(op, N)
    if isinstance(op, NambuVertex):
        op = (op.row, op.col, op.val)
    if isinstance(op, (tuple, list)) and len(op) == 3:
        r, c, v = (np.asarray(a).ravel() for a in op)
        if not (len(r) == len(c) == len(v)):
            raise ValueError("COO vertex: row, col and val differ in length")
        r, c = r.astype(np.int64), c.astype(np.int64)
        if len(r) and (r.min() < 0 or r.max() >= n2 or c.min() < 0 or c.max() >= n2):
            raise ValueError(f"COO vertex: index outside [0, {n2})")
        return r, c, v.astype(np.complex128)
    W = np.asarray(op, dtype=np.complex128)
    if W.shape != (n2, n2):
        raise ValueError(f"expected a NambuVertex, a Vertex, a COO triple or a dense ({n2}, {n2}) matrix")
    r, c = np.nonzero(W)
    return r.astype(np.int64), c.astype(np.int64), W[r, c]


def _spmm(a, b, n):
    """COO product a·b of two n x n triplet matrices (duplicates left to add up)."""
    ar, ac, av = a
    order = np.argsort(b[0], kind="stable")
    br, bc, bv = b[0][order], b[1][order], b[2][order]
    ptr = np.searchsorted(br, np.arange(n + 1))
    cnt = ptr[ac + 1] - ptr[ac]
    rep = np.repeat(np.arange(len(ar)), cnt)
    idx = np.repeat(ptr[ac], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return ar[rep], bc[idx], av[rep] * bv[idx]


def commutator_with_h(w, p, disorder, delta) -> NambuVertex:
    """i (H W - W H) with H = hamiltonian(p, disorder, delta), as a sparse
    product: the vertex of dO_W/dt at fixed Δ."""
    n2 = 2 * p.N
    h = as_nambu_triplets(hamiltonian(p, disorder, delta), p.N)
    wt = as_nambu_triplets(w, p.N)
    hw, wh = _spmm(h, wt, n2), _spmm(wt, h, n2)
    return _nv([hw[0], wh[0]], [hw[1], wh[1]], [1j * hw[2], -1j * wh[2]])


def union_csr_nambu(ops, N: int):
    """union_csr for 2N x 2N vertices: (rowptr (2N+1,), col (nnz,), val (nops, nnz))."""
    n2 = 2 * N
    trips = [as_nambu_triplets(op, N) for op in ops]
    keys = np.concatenate([r * n2 + c for r, c, _ in trips]) if trips else np.zeros(0, dtype=np.int64)
    pat = np.unique(keys)
    if len(pat) == 0:
        pat = np.zeros(1, dtype=np.int64)
    val = np.zeros((len(trips), len(pat)), dtype=np.complex128)
    for k, (r, c, v) in enumerate(trips):
        np.add.at(val[k], np.searchsorted(pat, r * n2 + c), v)
    rowptr = np.searchsorted(pat // n2, np.arange(n2 + 1)).astype(np.int64)
    return rowptr, (pat % n2).astype(np.int64), val


def _lifted(fn):
    return lambda p, mx, my: nambu(fn(p, mx, my), p.N)


def _pair_kind(form, part):
    return lambda p, mx, my: pair_field(p, mx, my, form, part)


# names for the driver's nambu_response option: every KINDS vertex lifted, and
# pair_<form>_<part>
NAMBU_KINDS = {k: _lifted(fn) for k, fn in KINDS.items()}
NAMBU_KINDS.update({f"pair_{form}_{part}": _pair_kind(form, part) for form in PAIR_FORMS for part in PAIR_PARTS})


def build_nambu(kind: str, p, mx: int = 0, my: int = 0) -> NambuVertex:
    """The Nambu vertex named `kind` (a key of NAMBU_KINDS) at momentum indices (mx, my)."""
    if kind not in NAMBU_KINDS:
        raise ValueError(f"unknown Nambu vertex kind {kind!r}; one of {sorted(NAMBU_KINDS)}")
    return NAMBU_KINDS[kind](p, int(mx), int(my))


# --------------------------------------------------------------------------
# patterns and contractions (FermionContext.measure_response_map)
# --------------------------------------------------------------------------
PATTERN_RANGES = ("site", "nn", "nnn")
PATTERN_BLOCKS = {"pp": (0, 0), "hh": (1, 1), "ph": (0, 1), "hp": (1, 0)}


def bond_pattern(p, ranges=PATTERN_RANGES, blocks=tuple(PATTERN_BLOCKS)) -> np.ndarray:
    """(npat, 2) Nambu index pairs (a, b): per block, every site's (i, i)
    ("site"), (i, j) over its 4 nearest ("nn") and 4 next-nearest ("nnn")
    neighbours j; block "pp" is (i, j), "hh" (i + N, j + N), "ph" (i, j + N),
    "hp" (i + N, j).  9N entries per block with all three ranges; on rings
    shorter than 3 a neighbour repeats and so does its entry."""
    ranges, blocks = tuple(ranges), tuple(blocks)
    for r in ranges:
        if r not in PATTERN_RANGES:
            raise ValueError(f"unknown range {r!r}; one of {PATTERN_RANGES}")
    for b in blocks:
        if b not in PATTERN_BLOCKS:
            raise ValueError(f"unknown block {b!r}; one of {tuple(PATTERN_BLOCKS)}")
    if not ranges or not blocks:
        raise ValueError("bond_pattern: ranges and blocks must not be empty")
    N = p.N
    i = np.arange(N, dtype=np.int64)
    nn, nnn = np.asarray(p.nn_table, dtype=np.int64) - 1, np.asarray(p.nnn_table, dtype=np.int64) - 1
    rows, cols = [], []
    for r in ranges:
        if r == "site":
            rows.append(i)
            cols.append(i)
        else:
            tab = nn if r == "nn" else nnn
            for d in range(4):
                rows.append(i)
                cols.append(tab[:, d])
    a, b = np.concatenate(rows), np.concatenate(cols)
    out = [np.stack([a + N * PATTERN_BLOCKS[k][0], b + N * PATTERN_BLOCKS[k][1]], axis=1) for k in blocks]
    return np.ascontiguousarray(np.concatenate(out), dtype=np.int64)


def _pattern_index(pattern, n2: int, rows, cols, what: str) -> np.ndarray:
    """index into the pattern of every (rows[k], cols[k]) (a duplicated
    pattern entry: its first copy); ValueError if one is missing"""
    pat = np.asarray(pattern, dtype=np.int64).reshape(-1, 2)
    keys = pat[:, 0] * n2 + pat[:, 1]
    order = np.argsort(keys, kind="stable")
    want = np.asarray(rows, dtype=np.int64) * n2 + np.asarray(cols, dtype=np.int64)
    pos = np.searchsorted(keys[order], want)
    ok = pos < len(keys)
    ok[ok] = keys[order][pos[ok]] == want[ok]
    if not np.all(ok):
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{what}: entry ({int(want[k] // n2)}, {int(want[k] % n2)}) is not in the pattern")
    return order[pos]


def contract(pattern, D, B, N=None):
    """Σ_e conj(B_e) D_e over the entries of the vertex B (a NambuVertex, or a
    Vertex lifted by `nambu`; duplicates summed first), D (..., npat) on
    `pattern`: N·chi of the pair (W, B) for D = dmap of W.  N (sites, or
    anything with .N) is needed for a Vertex and else taken from the largest
    index.  ValueError if an entry of B is missing from the pattern."""
    pat = np.asarray(pattern, dtype=np.int64).reshape(-1, 2)
    if isinstance(B, Vertex):
        if N is None:
            raise ValueError("contract: N is needed to lift a Vertex")
        B = nambu(B, N)
    r, c, v = (np.asarray(a).ravel() for a in (B.row, B.col, B.val))
    n2 = 2 * int(getattr(N, "N", N)) if N is not None else int(max(pat.max(), r.max(), c.max())) + 1
    keys, inv = np.unique(r.astype(np.int64) * n2 + c.astype(np.int64), return_inverse=True)
    val = np.zeros(len(keys), dtype=np.complex128)
    np.add.at(val, inv, v)
    idx = _pattern_index(pat, n2, keys // n2, keys % n2, "contract")
    return np.asarray(D)[..., idx] @ np.conj(val)


def _map_bonds(p, direction):
    """(j_b, t_b) per bond of direction α's current: site i owns the bonds that start at i."""
    lists = _bond_lists(p)
    return [(np.asarray(lists[name][0], dtype=np.int64), float(t)) for name, t in _current_bonds(p, direction)]


def diamagnetic_map(p, pattern, rho, direction="x") -> np.ndarray:
    """dia_i = Σ_b t_b 2 Re(ρ[j_b, i] - ρ[N + i, N + j_b]) per site i from ρ
    (npat,) on `pattern` (measure_response_map's rho); its mean over the sites
    is measure_current_response's dia."""
    N, rho = p.N, np.asarray(rho)
    i = np.arange(N, dtype=np.int64)
    out = np.zeros(N)
    for j, t in _map_bonds(p, direction):
        pp = rho[_pattern_index(pattern, 2 * N, j, i, "diamagnetic_map")]
        hh = rho[_pattern_index(pattern, 2 * N, N + i, N + j, "diamagnetic_map")]
        out += t * 2 * np.real(pp - hh)
    return out


def paramagnetic_map(p, pattern, D, direction="x") -> np.ndarray:
    """Λ_i = Σ_b Σ_{o in {0, N}} Re[conj(i t_b)(D[o + i, o + j_b] - D[o + j_b, o + i])]
    per site i from D (npat,) = dmap at l = 0 of the source nambu(current(p, 0,
    0, α)); its mean over the sites is Λ_αα(q = 0, l = 0)."""
    N, D = p.N, np.asarray(D)
    i = np.arange(N, dtype=np.int64)
    out = np.zeros(N)
    for j, t in _map_bonds(p, direction):
        for o in (0, N):
            fw = D[_pattern_index(pattern, 2 * N, o + i, o + j, "paramagnetic_map")]
            bw = D[_pattern_index(pattern, 2 * N, o + j, o + i, "paramagnetic_map")]
            out += np.real(np.conj(1j * t) * (fw - bw))
    return out


def stiffness_map(p, pattern, rho, D, direction="x") -> np.ndarray:
    """dia_i - Λ_i: the local superfluid stiffness, whose mean over the sites
    is the stiffness of the lattice-summed calls."""
    return diamagnetic_map(p, pattern, rho, direction) - paramagnetic_map(p, pattern, D, direction)


# --------------------------------------------------------------------------
# local families (FermionContext.measure_correlations)
# --------------------------------------------------------------------------
class LocalFamily(NamedTuple):
    site: np.ndarray       # int64, owner site of each term, in [0, N)
    row: np.ndarray        # int64, in [0, 2N)
    col: np.ndarray        # int64, in [0, 2N)
    val: np.ndarray        # complex128

    def dense(self, N: int) -> np.ndarray:
        """(N, 2N, 2N): the matrix of O(i) per site, duplicates summed."""
        W = np.zeros((N, 2 * N, 2 * N), dtype=np.complex128)
        np.add.at(W, (self.site, self.row, self.col), self.val)
        return W


def local_family(kind: str, p) -> LocalFamily:
    """The family of the Nambu vertex `kind` (a key of NAMBU_KINDS) at q = 0:
    its entries, each owned by the site i of the bond (i, j_b(i)) (or of the
    site term) it was built from.  Every builder above emits its entries in
    blocks of N, one per site in site order, which is what assigns the owner."""
    v = build_nambu(kind, p, 0, 0)
    N = p.N
    if len(v.row) % N:
        raise ValueError(f"{kind!r}: entries do not come in per-site blocks")
    site = np.tile(np.arange(N, dtype=np.int64), len(v.row) // N)
    return LocalFamily(site, v.row, v.col, v.val)


LOCAL_KINDS = tuple(NAMBU_KINDS)


def local_terms(families, N: int):
    """(tptr (nfam N + 1,), trow, tcol, tval) of a list of LocalFamily as
    dwh_measure_correlations takes them: the terms of family k at site i are
    tptr[k N + i] .. tptr[k N + i + 1] - 1, in the family's own order inside a
    site (duplicates kept)."""
    families = list(families)
    if not families:
        raise ValueError("families is empty")
    ptr, rows, cols, vals = [np.zeros(1, dtype=np.int64)], [], [], []
    base = 0
    for f in families:
        if not isinstance(f, LocalFamily):
            raise ValueError("families: a list of vertices.LocalFamily")
        site, r, c, v = (np.asarray(a).ravel() for a in f)
        if not (len(site) == len(r) == len(c) == len(v)):
            raise ValueError("LocalFamily: site, row, col and val differ in length")
        site = site.astype(np.int64)
        if len(site) and (site.min() < 0 or site.max() >= N):
            raise ValueError(f"LocalFamily: owner site outside [0, {N})")
        order = np.argsort(site, kind="stable")
        ptr.append(base + np.searchsorted(site[order], np.arange(1, N + 1)).astype(np.int64))
        rows.append(r[order].astype(np.int64))
        cols.append(c[order].astype(np.int64))
        vals.append(v[order].astype(np.complex128))
        base += len(site)
    cat = np.concatenate
    return (np.ascontiguousarray(cat(ptr)), np.ascontiguousarray(cat(rows)), np.ascontiguousarray(cat(cols)),
            np.ascontiguousarray(cat(vals)))


def disconnected(p, mean_a, mean_b) -> np.ndarray:
    """(1/N) Σ_j m_A(j ⊕ r) conj(m_B(j)) at [..., ry, rx] from the means
    (..., Ly, Lx) of two families (measure_correlations' mean)."""
    a = np.asarray(mean_a, dtype=np.complex128)
    b = np.asarray(mean_b, dtype=np.complex128)
    return np.fft.ifft2(np.fft.fft2(a) * np.conj(np.fft.fft2(b))) / p.N


def structure_factor(p, corr) -> np.ndarray:
    """S(q) = Σ_r e^{-i q·r} C(r), q = 2π (mx/Lx, my/Ly) at [..., my, mx], of
    corr (..., Ly, Lx)."""
    c = np.asarray(corr)
    if c.shape[-2:] != (p.Ly, p.Lx):
        raise ValueError(f"corr must end in (Ly, Lx) = ({p.Ly}, {p.Lx})")
    return np.fft.fft2(c)
