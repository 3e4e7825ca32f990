"""The cases of tests/test_measure_reductions_pairs.py (device) and of the CPU
pins in tests/test_measure_reference.py: prescribed eigensystems
(tests/measure_cases.py) for measure_nambu_response, measure_response_map and
measure_correlations, their vertices, pair lists, patterns and term tables,
and the references (long double) and yardsticks (fp64) of each case, computed
once per process and handed out unchanged.

Every reference is {output: (value, S)} in the working dtype, from
NRef.response_s, MapRef.sampled / rho_s and CorrRef.response_s.
"""
import numpy as np

import measure_cases as MC
import measure_reference as R
from correlation_reference import CorrRef
from nambu_reference import NRef
from response_map_reference import MapRef
from test_nambu_response import _random_w as random_w

LD, F8 = np.longdouble, np.float64
ETA = 0.05
MAX_TERMS, SLICE = 64, 32                 # kCorrMaxTerms, kMapSlice

_refs = {}


def once(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def system(family, n2, beta):
    """(E, U, Branches) of a case: Haar U, particle-hole closed for the ph family"""
    def make():
        E, U = MC.eigensystem(family, n2, beta)
        return E, U, R.Branches(E, beta)
    return once(("sys", family, n2, beta), make)


def grid(nw):
    """(start, step, count) of a grid through ω = 0"""
    step = 0.0625 if nw < 100 else 0.015625
    return (-step * (nw // 2), step, nw)


# --------------------------------------------------------------------------- Nambu response
def nambu_vertices(VX, p):
    """random, d-wave pair field (create, amplitude), lifted density, a second random one;
    two of them at 2N = 520"""
    vs = [random_w(VX, p.N, 3), VX.pair_field(p, 0, 0, "d", "create"), VX.pair_field(p, 0, 0, "d", "amplitude"),
          VX.nambu(VX.density(p, 1, 0), p.N), random_w(VX, p.N, 4)]
    return vs[:2] if 2 * p.N >= 520 else vs


_PAIR_ORDER = [(2, 2), (0, 1), (3, 4), (1, 1), (2, 0), (4, 4), (1, 3)]
_PAIR_ORDER += [(a, b) for a in range(5) for b in range(5) if (a, b) not in _PAIR_ORDER]


def nambu_pairs(count, nops):
    """diagonal and off-diagonal pairs mixed; from 3 pairs on the last repeats the first"""
    base = [q for q in _PAIR_ORDER if max(q) < nops] if nops < 5 else _PAIR_ORDER
    assert count <= len(base) + 1
    return base[:count] if count < 3 else base[:count - 1] + [base[0]]


# (family, β, 2N, n_matsubara, n_w, pairs)
NAMBU = [("generic", 4.0, 32, 1, 1, 1), ("generic", 8.0, 32, 2, 257, 2), ("generic", 4.0, 70, 8, 512, 3),
         ("generic", 8.0, 70, 9, 513, 4), ("twins", 8.0, 70, 17, 9, 5), ("twins", 8.0, 258, 2, 9, 6),
         ("dfedge", 8.0, 32, 9, 9, 7), ("dfedge", 8.0, 70, 2, 17, 16), ("dfedge", 8.0, 256, 2, 9, 5),
         ("cold15", 100.0, 70, 8, 9, 17), ("cold25", 1000.0, 258, 2, 9, 5), ("zeros", 8.0, 32, 9, 9, 23),
         ("ph", 8.0, 70, 8, 9, 7), ("generic", 4.0, 520, 2, 9, 4)]


def nambu_case(O, VX, family, beta, n2, nl, nw, npairs):
    """(E, U, vertices, pairs, omega, reference, yardstick); a reference: dict chi, chi2 -> (value, S)"""
    def make():
        p = MC.params(O, n2, beta)
        E, U, br = system(family, n2, beta)
        vs = nambu_vertices(VX, p)
        pairs = nambu_pairs(npairs, len(vs))
        Ws = [v.dense(p.N) for v in vs]
        out = []
        for dt in (LD, F8):
            ref = NRef(p, E, U, beta=beta, dt=dt, br=br)
            chi, chi2 = ref.response_s(Ws, pairs, nl, R.grid(*grid(nw)), ETA)
            out.append(dict(chi=chi, chi2=chi2))
        return (E, U, vs, pairs, grid(nw)) + tuple(out)
    return once(("nambu", family, beta, n2, nl, nw, npairs), make)


# --------------------------------------------------------------------------- response map
def pattern(VX, p, kind):
    """bond: site + nn ranges, pp + ph blocks.  random: 3 · 2N entries anywhere, with
    duplicates.  col70: one column b with 70 entries (slices of 32 + 32 + 6) among a few
    others, from every block"""
    n2 = 2 * p.N
    if kind == "bond":
        return VX.bond_pattern(p, ranges=("site", "nn"), blocks=("pp", "ph"))
    rng = np.random.default_rng(n2 + len(kind))
    if kind == "random":
        a, b = rng.integers(0, n2, 3 * n2), rng.integers(0, n2, 3 * n2)
        a[1], b[1] = a[0], b[0]
        a[-1], b[-1] = a[2], b[2]
    else:
        heavy = n2 - 3                                           # a hole column
        a = np.concatenate([rng.integers(0, n2, 70), rng.integers(0, n2, 40)])
        b = np.concatenate([np.full(70, heavy), np.delete(np.arange(n2), heavy)[rng.integers(0, n2 - 1, 40)]])
        perm = rng.permutation(len(a))
        a, b = a[perm], b[perm]
        assert np.bincount(b, minlength=n2).max() == 70 == 2 * SLICE + 6
    pat = np.stack([a, b], axis=1).astype(np.int64)
    hole = pat >= p.N
    assert (hole[:, 0] & hole[:, 1]).any() and (hole[:, 0] & ~hole[:, 1]).any()      # hole-hole, hole-particle
    assert kind != "random" or len(np.unique(pat, axis=0)) < len(pat)
    return pat


def map_vertices(VX, p):
    vs = [random_w(VX, p.N, 3), VX.pair_field(p, 0, 0, "d", "amplitude"), VX.nambu(VX.density(p, 1, 0), p.N)]
    return vs[:1] if 2 * p.N >= 520 else vs[:2] if 2 * p.N >= 256 else vs


OMEGAS = {0: (), 1: (0.3,), 2: (-0.6, 0.3), 4: (-0.6, 0.0, 0.3, 1.7)}

# (family, β, 2N, pattern, n_matsubara, frequencies, DWHMC_MAP_CHUNK)
MAP = [("generic", 4.0, 32, "bond", 3, 4, None), ("generic", 8.0, 32, "random", 0, 1, None),
       ("generic", 8.0, 70, "col70", 1, 4, None), ("generic", 4.0, 70, "random", 3, 0, None),
       ("generic", 8.0, 70, "random", 3, 2, 2), ("generic", 8.0, 70, "col70", 0, 0, None),
       ("twins", 8.0, 70, "bond", 3, 1, None), ("twins", 8.0, 258, "random", 1, 1, None),
       ("dfedge", 8.0, 32, "random", 3, 4, None), ("dfedge", 8.0, 70, "bond", 0, 4, None),
       ("dfedge", 8.0, 256, "bond", 1, 1, None), ("cold15", 100.0, 70, "random", 3, 1, None),
       ("cold25", 1000.0, 258, "bond", 1, 4, None), ("zeros", 8.0, 32, "col70", 3, 4, None),
       ("ph", 8.0, 70, "bond", 3, 1, None), ("generic", 4.0, 520, "bond", 3, 1, None)]


def map_case(O, VX, family, beta, n2, kind, nl, nfreq, chunk=None):
    """(E, U, vertices, pattern, omega, reference, yardstick); a reference: dict
    dmap -> (value, S) (nops, nz, npat) or None, rho -> (value, S) (npat,)"""
    def make():
        p = MC.params(O, n2, beta)
        E, U, br = system(family, n2, beta)
        vs, pat, om = map_vertices(VX, p), pattern(VX, p, kind), OMEGAS[nfreq]
        out = []
        for dt in (LD, F8):
            ref = MapRef(p, E, U, beta=beta, dt=dt, br=br)
            d = None
            if nl + nfreq > 0:
                parts = [ref.sampled(v.dense(p.N), pat, nl, om, ETA) for v in vs]
                d = tuple(np.stack([x[k] for x in parts]) for k in (0, 1))
            out.append(dict(dmap=d, rho=ref.rho_s(pat)))
        return (E, U, vs, pat, om) + tuple(out)
    return once(("map", family, beta, n2, kind, nl, nfreq), make)


# --------------------------------------------------------------------------- correlations
def hand_family(VX, N, seed=5):
    """a term table by hand: site 0 empty, site 1 at the cap of 64 terms, every other
    site 0 .. 3 terms (so more sites hold none), indices anywhere in the four Nambu
    blocks, duplicate terms at site 1, unsorted"""
    rng = np.random.default_rng(seed + N)
    cnt = rng.integers(0, 4, N)
    cnt[0], cnt[1] = 0, MAX_TERMS
    site = np.repeat(np.arange(N), cnt)
    n = len(site)
    row, col = rng.integers(0, 2 * N, n), rng.integers(0, 2 * N, n)
    row[5], col[5] = row[4], col[4]                                # (terms 0 .. 63 belong to site 1)
    row[9], col[9] = row[4], col[4]
    val = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    perm = rng.permutation(n)
    assert (cnt == 0).sum() > 1
    return VX.LocalFamily(site[perm].astype(np.int64), row[perm].astype(np.int64), col[perm].astype(np.int64), val[perm])


CORR_KINDS = ("density", "current_x", "pair_d_create")            # a site, a bond and a pair family; 3: by hand
CORR_PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 2), (3, 1), (2, 3)]
CORR_PAIRS_BIG = [(0, 0), (3, 3), (2, 1), (1, 3)]

# (family, β, 2N)
CORR = [("generic", 4.0, 32), ("generic", 8.0, 70), ("cold25", 1000.0, 256), ("zeros", 8.0, 258), ("ph", 8.0, 70),
        ("zeros", 8.0, 32), ("cold25", 1000.0, 70), ("generic", 4.0, 520)]


def corr_case(O, VX, family, beta, n2):
    """(E, U, families, pairs, reference sites, reference, yardstick); a reference:
    CorrRef.response_s's dict"""
    def make():
        p = MC.params(O, n2, beta)
        E, U, br = system(family, n2, beta)
        fams = [VX.local_family(k, p) for k in CORR_KINDS] + [hand_family(VX, p.N)]
        pairs = CORR_PAIRS_BIG if n2 >= 520 else CORR_PAIRS
        sites = [0, p.N // 2 + 1, p.N - 1]
        out = []
        for dt in (LD, F8):
            ref = CorrRef(p, E, U, beta=beta, dt=dt, br=br)
            out.append(ref.response_s(fams, pairs, sites))
        return (E, U, fams, pairs, sites) + tuple(out)
    return once(("corr", family, beta, n2), make)


def spectra():
    """every (family, β, 2N) a device case injects"""
    out = {c[:3] for c in NAMBU} | {c[:3] for c in MAP} | {c[:3] for c in CORR}
    return sorted(out | {(f, 8.0, 70) for f in BATCH})


BATCH = ("twins", "dfedge", "generic")                            # the three states of the batched call, 2N = 70
