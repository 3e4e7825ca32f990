"""Spectrum families at the eigensolvers' own thresholds (csrc/dwhmc_eig.hip,
csrc/dwhmc_qeig.hip), shared by tests/test_eig_algorithm.py (the numpy
prototypes) and tests/test_eig_edge_spectra.py (the device).

The solvers branch on
  kEigClusterTol = 1e-6 ||T||    levels orthonormalised together,
  kEigZeroTol    = 2.5e-4 ||T||  where the particle-hole half solve splits the
                                 spectrum (c0) and the crowd at zero (q_crowd),
  the cluster caps               kQMaxCluster = 32 (a crowd of 16 pairs),
                                 kEigMaxCluster = 64 (the long-cluster path).
||T|| is the Gershgorin bound of the solver's own tridiagonal: the host cannot
read it, but rho <= ||T|| <= 3 rho with rho = max|E|, so every prediction
below is evaluated at both ends and given only where they agree.

Every member is built from the oracle's init_static_H / update_H_BdG with an
explicit disorder array and Delta, deterministic in its seed, and classified
from numpy.linalg.eigvalsh(H)."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

T_HOP, TP_HOP = 1.0, -0.35
CLUSTER_TOL, ZERO_TOL = 1e-6, 2.5e-4
Q_MAX_CLUSTER, EIG_MAX_CLUSTER = 32, 64
TN_RANGE = (1.0, 3.0)   # ||T|| / rho

Case = namedtuple("Case", "name p disorder Delta H cls")


def _runs(gaps, tol):
    """(start, length) of every run of >= 2 levels with consecutive gaps <= tol."""
    out, j, n = [], 0, len(gaps) + 1
    while j < n:
        k = j + 1
        while k < n and gaps[k - 1] <= tol:
            k += 1
        if k - j > 1:
            out.append((j, k - j))
        j = k
    return out


def classify(H):
    """rho = max|E|; the cluster runs at gap <= 1e-6 rho (and at 3e-6 rho, the
    upper end of ||T||); the count of gaps in (1e-6, 1e-4] rho; g0 = the
    central gap / rho; c0 and the gap at the half-solve split (at ||T|| =
    rho); the run across zero and the longest run away from it."""
    E = np.linalg.eigvalsh(H)
    n, N = len(E), len(E) // 2
    rho = float(np.max(np.abs(E)))
    gaps = np.diff(E)
    runs = _runs(gaps, CLUSTER_TOL * rho)
    runs_hi = _runs(gaps, CLUSTER_TOL * TN_RANGE[1] * rho)
    across = [L for (s, L) in runs if s <= N - 1 and s + L > N]
    away = [L for (s, L) in runs if not (s <= N - 1 and s + L > N)]
    c0 = N
    while c0 > 0 and not (gaps[c0 - 1] > ZERO_TOL * rho):
        c0 -= 1
    return dict(E=E, n=n, rho=rho, runs=runs,
                longest_run=max([L for _, L in runs], default=1),
                longest_run_hi=max([L for _, L in runs_hi], default=1),
                longest_run_away=max(away, default=1),
                zero_run=max(across, default=0),
                mid_gaps=int(np.sum((gaps > CLUSTER_TOL * rho) & (gaps <= 1e-4 * rho))),
                g0=float(gaps[N - 1] / rho) if n > 1 else 0.0,
                c0=c0, split_gap=float(gaps[c0 - 1] / rho) if c0 > 0 else None)


# ---------------------------------------------------------------- predictions
def _q_crowd(E, j0, tn):
    """q_crowd of csrc/dwhmc_qeig.hip."""
    n = len(E)
    nv = n - j0
    zt, ct = ZERO_TOL * tn, CLUSTER_TOL * tn
    if nv < 2 or E[j0] + E[j0 + 1] > zt:
        return 0
    c = 2
    while c < nv and (E[j0 + c] + E[j0] <= zt or E[j0 + c] - E[j0 + c - 1] <= ct):
        c += 1
    return c


def _q_accepts(E, tn):
    """q_heev_enqueue's host decision (csrc/dwhmc_eigsolve.cpp)."""
    n = len(E)
    j0 = n // 2
    crowd = _q_crowd(E, j0, tn)
    if 2 * crowd > Q_MAX_CLUSTER:
        return False
    run = 1
    for j in range(j0 + max(crowd, 1), n):
        if not (E[j] - E[j - 1] > CLUSTER_TOL * tn):
            run += 1
            if run > Q_MAX_CLUSTER:
                return False
        else:
            run = 1
    return True


def _both(f, cls):
    a, b = (f(cls["E"], r * cls["rho"]) for r in TN_RANGE)
    return a if a == b else None


def predict_quat(cls):
    """dwh_info_t::eig_quat of a default solve: 1 / 0, or None where it depends on ||T||."""
    r = _both(_q_accepts, cls)
    return None if r is None else int(r)


def predict_half_one_stage(cls):
    """dwh_info_t::eig_half of the one-stage solver (DWHMC_EIG_QUAT=0): 1 when
    c0 = N (the central gap above kEigZeroTol ||T||) and no gap anywhere is
    within kEigClusterTol ||T||; None where it depends on ||T||."""
    def f(E, tn):
        g = np.diff(E)
        N = len(E) // 2
        return bool(g[N - 1] > ZERO_TOL * tn and np.all(g > CLUSTER_TOL * tn))
    r = _both(f, cls)
    return None if r is None else int(r)


# ------------------------------------------------------------------- builders
def dwave(N, d0):
    return np.stack([np.full(N, d0), np.full(N, -d0)], 1).astype(np.complex128)


def build(O, name, Lx, Ly, mu, disorder, Delta, tp=TP_HOP, beta=8.0):
    p = O.ModelParameters(Lx, Ly, T_HOP, tp, mu, 0.0, 0.0, beta, 0.8, 1.0)
    disorder = np.asarray(disorder, dtype=np.float64)
    cache = O.initialize_cache(p)
    O.init_static_H(cache, p, disorder)
    O.update_H_BdG(cache, p, Delta)
    H = O.hermitian_from_upper(cache.H_base)
    return Case(name, p, disorder, Delta, H, classify(H))


CLEAN_LATTICES = [(4, 4), (6, 6), (5, 7), (6, 4), (8, 8), (10, 10), (12, 12)]
CLEAN_D0 = [0.0, 1e-9, 1e-5, 1e-3, 0.2]
CLEAN_MU = [-1.0, -1.08, 0.0]
NESTED = [(4, 4), (8, 8), (12, 12)]   # tp = 0, mu = 0, Delta = 0: 2 (2 L - 2) levels at E = 0


@functools.lru_cache(maxsize=None)
def _clean_ladder(O):
    out = []
    for Lx, Ly in CLEAN_LATTICES:
        for mu in CLEAN_MU:
            for d0 in CLEAN_D0:
                out.append(build(O, f"clean-{Lx}x{Ly}-mu{mu:g}-d{d0:g}", Lx, Ly, mu, np.zeros(Lx * Ly),
                                 dwave(Lx * Ly, d0)))
    for L, _ in NESTED:
        out.append(build(O, f"nested-{L}x{L}", L, L, 0.0, np.zeros(L * L), dwave(L * L, 0.0), tp=0.0))
    return tuple(out)


def clean_ladder(O):
    """Family 1: W = 0, uniform d-wave Delta = +-d0; exact clusters (degenerate
    shells), exact zero modes at mu = 0 with L % 4 == 0, and the nested Fermi
    surface of tp = mu = Delta = 0 (a crowd at zero of 12 / 28 / 44 levels)."""
    return _clean_ladder(O)


LIFT_W = [1e-12, 1e-9, 1e-7, 3e-6, 1e-5, 1e-4, 1e-3, 1e-2]


@functools.lru_cache(maxsize=None)
def _lifted_ladder(O):
    out = []
    for L in (6, 8):
        for mu in (-1.0, 0.0):
            for k, w in enumerate(LIFT_W):
                rng = np.random.default_rng(1000 * L + 10 * k + int(mu == 0.0))
                out.append(build(O, f"lift-{L}x{L}-mu{mu:g}-w{w:g}", L, L, mu, w * rng.standard_normal(L * L),
                                 dwave(L * L, 0.2)))
    return tuple(out)


def lifted_ladder(O):
    """Family 2: the clean 6x6 / 8x8 (d0 = 0.2) plus w N(0,1) site potentials:
    the degenerate shells' gaps sweep through kEigClusterTol."""
    return _lifted_ladder(O)


ZERO_TARGETS = [0.3, 0.6, 0.9, 1.1, 1.5, 2.0, 3.0, 5.0, 9.0]   # g0 / kEigZeroTol
ZERO_LATTICES = [8, 12]
ZERO_LARGE = (16, 1.1)   # one 16 x 16 member (n = 512), just above the threshold


def _zero_member(O, L, target, seed0):
    """w (and the first seed from seed0) with g0 = target * kEigZeroTol within
    10 % and no gap within 3e-6 rho: g0 is ~linear in w for small w (the zero
    modes split at first order), so a secant step then bisection."""
    N = L * L
    want = target * ZERO_TOL
    for seed in range(seed0, seed0 + 20):
        v = np.random.default_rng(seed).standard_normal(N)

        def g0(w):
            return build(O, "", L, L, 0.0, w * v, dwave(N, 0.2))

        lo, hi = 0.0, 0.02
        while g0(hi).cls["g0"] < want and hi < 2.0:
            lo, hi = hi, 2.0 * hi
        c = None
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            c = g0(mid)
            if abs(c.cls["g0"] - want) <= 0.02 * want:
                break
            if c.cls["g0"] < want:
                lo = mid
            else:
                hi = mid
        if c is not None and abs(c.cls["g0"] - want) <= 0.1 * want and c.cls["longest_run_hi"] == 1:
            return c._replace(name=f"zero-{L}x{L}-g{target:g}")
    raise AssertionError(f"no zero-gap member for L = {L}, target {target}")


@functools.lru_cache(maxsize=None)
def _zero_gap_ladder(O):
    out = [_zero_member(O, L, t, 100 * L + 7 * k) for L in ZERO_LATTICES for k, t in enumerate(ZERO_TARGETS)]
    out.append(_zero_member(O, ZERO_LARGE[0], ZERO_LARGE[1], 1600))
    return tuple(out)


def zero_gap_ladder(O):
    """Family 3: clean mu = 0 with L % 4 == 0 (nodes on the grid: exact zero
    modes) plus w N(0,1) site potentials with w chosen so that the central gap
    g0 = (E[N] - E[N-1]) / rho sits at 0.3 .. 9 x kEigZeroTol."""
    return _zero_gap_ladder(O)


TINY = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 5), (6, 1), (3, 2)]


@functools.lru_cache(maxsize=None)
def _reducible(O):
    out = []
    for Lx, Ly in ((6, 6), (5, 7), (8, 8)):
        rng = np.random.default_rng(40 + Lx)
        out.append(build(O, f"normal-{Lx}x{Ly}-W0.5", Lx, Ly, -1.08, 0.5 * rng.standard_normal(Lx * Ly),
                         np.zeros((Lx * Ly, 2), np.complex128)))
    for Lx, Ly in TINY:
        rng = np.random.default_rng(70 + 10 * Lx + Ly)
        N = Lx * Ly
        D = 0.25 * (rng.standard_normal((N, 2)) + 1j * rng.standard_normal((N, 2)))
        out.append(build(O, f"tiny-{Lx}x{Ly}", Lx, Ly, -1.08, 0.3 * rng.standard_normal(N), D))
    return tuple(out)


def reducible(O):
    """Family 4: Delta = 0 with W = 0.5 N(0,1) potentials (particle and hole
    blocks decoupled, no clusters), and tiny / chain lattices with generic
    complex Delta (doubled bonds at L = 2, self bonds at L = 1, n = 2, 4)."""
    return _reducible(O)


FAMILIES = dict(clean=clean_ladder, lifted=lifted_ladder, zero=zero_gap_ladder, reducible=reducible)


def names(family):
    """The members' names without building them (pytest ids at collection)."""
    if family == "clean":
        return ([f"clean-{Lx}x{Ly}-mu{mu:g}-d{d0:g}" for Lx, Ly in CLEAN_LATTICES for mu in CLEAN_MU for d0 in CLEAN_D0]
                + [f"nested-{L}x{L}" for L, _ in NESTED])
    if family == "lifted":
        return [f"lift-{L}x{L}-mu{mu:g}-w{w:g}" for L in (6, 8) for mu in (-1.0, 0.0) for w in LIFT_W]
    if family == "zero":
        return ([f"zero-{L}x{L}-g{t:g}" for L in ZERO_LATTICES for t in ZERO_TARGETS]
                + [f"zero-{ZERO_LARGE[0]}x{ZERO_LARGE[0]}-g{ZERO_LARGE[1]:g}"])
    return [f"normal-{Lx}x{Ly}-W0.5" for Lx, Ly in ((6, 6), (5, 7), (8, 8))] + [f"tiny-{Lx}x{Ly}" for Lx, Ly in TINY]


def member(O, family, name):
    for c in FAMILIES[family](O):
        if c.name == name:
            return c
    raise KeyError(name)
