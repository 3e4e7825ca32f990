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


def current(p, mx: int = 0, my: int = 0, direction="x") -> Vertex:
    if direction not in ("x", "y", 0, 1):
        raise ValueError("direction must be 'x' or 'y'")
    if direction in ("x", 0):
        bonds = [("+x", p.t), ("+x+y", p.tp), ("+x-y", p.tp)]
    else:
        bonds = [("+y", p.t), ("+x+y", p.tp), ("-x+y", p.tp)]
    return _bond_vertex(p, mx, my, bonds, -1.0, 1j)


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
