"""Prescribed eigensystems for the tests of the measurement reductions
(tests/test_measure_reference.py on the CPU, tests/test_measure_reductions.py
and tests/test_measure_reductions_pairs.py on the device): spectrum families
that put levels on either side of every branch rule on purpose, each with its condition checked by `check_family`, and
the lattices whose 2N is chosen against the 256-pair tile.  U is the Q of a
seeded complex Gaussian matrix (measure_reference.haar) unless the family
says otherwise: nothing needs U to diagonalise anything.
"""
import functools

import numpy as np

import measure_reference as R

T, TP, MU = 1.0, -0.35, -1.08

# 2N -> (Lx, Ly)
LATTICES = {32: (4, 4), 70: (5, 7), 256: (16, 8), 258: (43, 3), 520: (20, 13)}

TWIN_GAPS = (0.0, 2.5e-9, 5e-9, 2e-8, 1e-7, 1e-6)
AK_CUT_ETA = 1e-5


def params(O, n2, beta):
    Lx, Ly = LATTICES[n2]
    return O.ModelParameters(Lx, Ly, T, TP, MU, 0.0, 0.0, float(beta), 0.8, 1.0)


def _settled(draw, count, fixed, build, beta):
    """Levels x (count of them, the first `fixed` prescribed) drawn by draw(k) -> k values,
    redrawn one by one until no pair of build(x) lies within a factor 2 of the Δf rule
    (|f_n - f_m| in [0.5e-12, 2e-12]): such a pair may fall either way on the device.
    At β = 8 this keeps levels out of a band around |E| ≈ 3.4 .. 3.5 when others lie above."""
    x = draw(count)
    x[: len(fixed)] = fixed
    fixed = len(fixed)
    for _ in range(200):
        amb = R.Branches(np.sort(build(x)), beta).ambiguous_df()
        if not amb.any():
            return x
        order = np.argsort(build(x), kind="stable") % count       # sorted index -> index into x
        bad = np.unique(order[np.nonzero(amb.any(axis=1))[0]])
        bad = bad[bad >= fixed]
        assert len(bad), "an ambiguous pair among the prescribed levels"
        x[bad[::2]] = draw(len(bad[::2]))                       # (one level of a pair is enough)
    raise AssertionError("no spectrum without ambiguous pairs found")


def spectrum(family, n2, beta, seed=0):
    """E ascending (2N,) of a family at inverse temperature beta (built once per process)."""
    return _spectrum(family, n2, float(beta), seed).copy()


@functools.lru_cache(maxsize=None)
def _spectrum(family, n2, beta, seed):
    rng = np.random.default_rng(1000 * seed + n2)
    N = n2 // 2

    def both(mag):
        return np.concatenate([-mag, mag])

    if family == "generic":
        E = _settled(lambda k: rng.uniform(-4.0, 4.0, k), n2, (), lambda x: x, beta)
    elif family == "twins":
        # every level has a partner at one of TWIN_GAPS; the pairs sit on a 1e-3
        # grid around 0, ±0.3, ±1, so any other gap is >= 1e-3 - 1e-6
        centres = (0.0, 0.3, -0.3, 1.0, -1.0)
        base = np.array([centres[k % 5] + 1e-3 * ((k // 5) - (N // 10)) for k in range(N)])
        gaps = np.array([TWIN_GAPS[k % len(TWIN_GAPS)] for k in range(N)])
        E = np.concatenate([base, base + gaps])
    elif family == "dfedge":
        # three groups per side at g = e^{-β|E|} ≈ 2.5e-13, 5.5e-13, 3.6e-12 (β|E| in
        # 26 .. 29), each spread over 0.01 in β|E|: same-side pairs across groups have
        # |Δf| ≈ 3e-13 (skipped) or 3e-12, 3.3e-12 (kept), inside a group <= 4e-14
        x0 = (29.0, 28.23, 26.35)
        x = np.array([x0[k % 3] + 0.01 * (k // 3) / max(1, N // 3) for k in range(N)])
        E = np.concatenate([-x / beta, x[: n2 - N] / beta])
    elif family.startswith("cold"):
        gap = float(family[4:]) / beta             # cold5, cold15, cold25: β min|E|
        E = both(_settled(lambda k: gap + rng.uniform(0.0, 2.0, k), N, (gap,), both, beta))
    elif family == "zeros":
        E = _settled(lambda k: rng.uniform(-4.0, 4.0, k), n2, (-1e-14, -0.0, 0.0, 1e-14), lambda x: x, beta)
    elif family == "akcut":
        # η = AK_CUT_ETA puts L(-E) = 1e-6 at |E| ≈ 1.784: keep every level 2 % away
        ec = np.sqrt(AK_CUT_ETA / (np.pi * 1e-6) - AK_CUT_ETA ** 2)

        def draw(k):
            e = rng.uniform(-4.0, 4.0, k)
            near = np.abs(np.abs(e) / ec - 1.0) < 0.02
            e[near] = np.sign(e[near]) * ec * np.where(rng.random(near.sum()) < 0.5, 0.95, 1.05)
            return e
        E = _settled(draw, n2, (), lambda x: x, beta)
    elif family == "ph":
        E = both(_settled(lambda k: rng.uniform(0.05, 4.0, k), N, (), both, beta))
    else:
        raise ValueError(family)
    # -0.0 before +0.0 and stable otherwise: the order the entry asks for
    return E[np.lexsort((np.signbit(E) == 0, E))] if family == "zeros" else np.sort(E)


def check_family(family, E, beta, eta=None):
    """the condition each family promises, on the fixture itself"""
    E = np.asarray(E)
    assert np.all(np.diff(E) >= 0)
    gaps = np.abs(E[None, :] - E[:, None])
    if family == "twins":
        assert not np.any((gaps >= 0.9e-8) & (gaps <= 1.1e-8))
        g1 = np.sort(gaps + np.diag(np.full(len(E), np.inf)), axis=1)[:, 0]
        assert np.all(g1 <= 1e-6 * (1 + 1e-6)), "every level has a twin"      # (the fp64 sum rounds the gap)
        for g in TWIN_GAPS:                       # both sides of the 1e-8 rule are populated
            assert np.any(np.abs(g1 - g) <= 1e-10 + 1e-3 * g), g
    if family == "dfedge":
        br = R.Branches(E, beta)
        x = beta * np.abs(E)
        assert x.min() >= 26 and x.max() <= 29.1
        same = np.sign(E)[:, None] == np.sign(E)[None, :]
        a = np.asarray(br.adf, dtype=np.float64)
        assert np.any(same & (a > 2e-13) & (a < 4e-13)) and np.any(same & (a > 2.5e-12) & (a < 4e-12))
        assert not br.ambiguous_df().any()
    if family.startswith("cold"):
        assert abs(beta * np.abs(E).min() - float(family[4:])) < 1e-9
    if family == "zeros":
        assert np.signbit(E[E == 0]).tolist() == [True, False] and 1e-14 in E and -1e-14 in E
    if family == "akcut":
        br = R.Branches(E, beta, eta)
        assert br.cut.any() and not br.cut.all() and br.cut_margin > 0.01
    if family == "ph":
        assert np.array_equal(E, -E[::-1])


def eigensystem(family, n2, beta, seed=0):
    E = spectrum(family, n2, beta, seed)
    U = R.ph_closed(n2, 7 + seed) if family == "ph" else R.haar(n2, 7 + seed)
    return E, U


def random_operator(N, seed, hermitian=False):
    """a sparse complex V (dense N x N here), non-Hermitian unless asked"""
    rng = np.random.default_rng(seed)
    V = np.zeros((N, N), dtype=np.complex128)
    n = 3 * N
    r, c = rng.integers(0, N, n), rng.integers(0, N, n)
    np.add.at(V, (r, c), rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return V + V.conj().T if hermitian else V
