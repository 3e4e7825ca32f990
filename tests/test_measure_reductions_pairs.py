"""The Nambu response, the response maps and the equal-time correlations on
prescribed eigensystems (gpu): measure_nambu_response, measure_response_map
and measure_correlations reduce eigenpairs that dwh_debug_set_eigensystem
injects (tests/measure_cases.py's families on both sides of the 1e-8 and
1e-12 rules, 2N = 32 .. 520), and every output value, real and imaginary part
each, is held to tests/test_measure_reductions.py's bar

    |device - reference| <= max(8 |yardstick - reference|, 2N eps S)

with reference / yardstick the long-double / fp64 runs of NRef.response_s,
MapRef.sampled / rho_s and CorrRef.response_s (tests/measure_pair_cases.py has
the cases, tests/test_measure_reference.py pins the references on the CPU:
the yardstick stays within the floor 2N eps S on every case and no spectrum
has a pair within a factor 2 of the Δf rule, so there is no allowance).  S:

    chi[p, l]     (1/N) Σ_nm |r_nm(l) + i s_nm(l)| |M_nm|,  M = X^a conj(X^b)
    chi2[p, j]    (η/N) Σ_kept |Δf_nm| |M_nm| / ((ω_j - ΔE_nm)² + η²)
    dmap[e, z]    Σ_nm |U[a_e, n]| |w_nm(z)| |X_nm| |U[b_e, m]|
    rho[e]        S_ρ[a_e, b_e],  S_ρ = |U| diag(f) |U|^T
    mean_A(i)     Σ_t |a_{i,t}| S_ρ[c, r]
    G_AB(i, j)    Σ_{t,u} |a| |b| S_ρ[r_A, r_B] (δ[c_A, c_B] + S_ρ[c_A, c_B])
    corr[r]       (1/N) Σ_j of G's;   local[q][r]: G's at the reference site

Measured on an MI355X, worst ratio  device error / max(yardstick error, 2N eps S)
per output over the cases of this file, on the parent commit's library and on
this commit's (profiles/measure_reductions.txt has them per entry and family):

    output                     parent     branch
    chi(l=0).re                0.0204     0.0204
    chi(l=0).im               0.00658    0.00658
    chi2.re                      0.11       0.11
    chi2.im                     0.111      0.111
    chi(l>=1).re               0.0456     0.0456
    chi(l>=1).im               0.0057     0.0057
    dmap(iΩ).re                0.0154     0.0154
    dmap(iΩ).im                0.0123     0.0123
    dmap(ω).re                 0.0196     0.0196
    dmap(ω).im                 0.0205     0.0205
    rho.re                     0.0329     0.0329
    rho.im                     0.0132     0.0132
    mean.re                    0.0389     0.0389
    mean.im                    0.0561     0.0561
    corr.re                   0.00979    0.00979
    corr.im                   0.00158    0.00158
    local.re                   0.0108     0.0108
    local.im                   0.0161     0.0161

Nothing had to be fixed: no kernel changed, the two libraries are the same
code and the two columns agree.  The yardstick's own error is at most 0.08 of
2N eps S on these cases, so the bar is in effect 2N eps S, and a ratio above 1
fails.  No output needs a deeper floor than 2N eps S (depth 1), nested sums
(X behind chi, X and the row product behind dmap, ρ twice behind G) included.
"""
import numpy as np
import pytest

import measure_pair_cases as MP
from test_measure_reductions import _ctx, _fresh_failures, _hold, _verdict  # noqa: F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu

ETA = MP.ETA


@pytest.fixture(scope="module")
def VX(dwhmc):
    return dwhmc.vertices


def _hold_c(what, dev, ref, yard, S, n2):
    """a complex output: both parts against the same S"""
    dev = np.asarray(dev)
    assert dev.dtype == np.complex128 and dev.shape == np.shape(ref), (what, dev.dtype, dev.shape, np.shape(ref))
    for name, part in ((".re", np.real), (".im", np.imag)):
        _hold(what + name, part(dev), part(ref), part(yard), S, n2)


def _tag(entry, case):
    return entry + " " + "-".join(f"{x:g}" if isinstance(x, float) else str(x) for x in case)


def _ids(c):
    return "-".join(str(x) for x in c)


def _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U, chunk=None):
    monkeypatch.delenv("DWHMC_RESPONSE_GROUP", raising=False)
    if chunk is None:
        monkeypatch.delenv("DWHMC_MAP_CHUNK", raising=False)
    else:
        monkeypatch.setenv("DWHMC_MAP_CHUNK", str(chunk))
    p, ctx = _ctx(dwhmc, oracle, n2, beta)
    ctx.debug_set_eigensystem(E, U)
    return p, ctx


# --------------------------------------------------------------------------- Nambu response
def _hold_nambu(tag, got, ref, yard, n2):
    (chi, Sc), (c2, S2) = ref["chi"], ref["chi2"]
    _hold_c(tag + " chi(l=0)", got["chi"][:, :1], chi[:, :1], yard["chi"][0][:, :1], Sc[:, :1], n2)
    if chi.shape[1] > 1:
        _hold_c(tag + " chi(l>=1)", got["chi"][:, 1:], chi[:, 1:], yard["chi"][0][:, 1:], Sc[:, 1:], n2)
    _hold_c(tag + " chi2", got["chi2"], c2, yard["chi2"][0], S2, n2)


@pytest.mark.parametrize("case", MP.NAMBU, ids=_ids)
def test_nambu_response(dwhmc, oracle, VX, monkeypatch, case):
    """chi[p, l] and chi2[p, j]: k_nb_pairs<1> and <8> (n_matsubara 1, 2, 8, 9, 17), grids
    through ω = 0 of 1, 257, 512 and 513 points, 1 .. 7 pairs (every group size of
    k_nb_spec alone and behind a full group), 16 (one batch), 17 (a second batch that is
    the one-pair tail) and 23 (a second batch of a full group and a tail of 3); at 2N >= 256
    the 256-row tiles, with cold25 the all-zero tiles that are skipped"""
    family, beta, n2, nl, nw, npairs = case
    E, U, vs, pairs, omega, ref, yard = MP.nambu_case(oracle, VX, *case)
    assert len(pairs) == npairs and omega[2] == nw
    p, ctx = _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U)
    got = ctx.measure_nambu_response(vs, pairs, n_matsubara=nl, omega=omega, eta=ETA)
    assert np.array_equal(got["pairs"], pairs) and 0.0 in got["omega"]
    _hold_nambu(_tag("nambu", case), got, ref, yard, n2)
    _verdict()


# --------------------------------------------------------------------------- response map
def _hold_map(tag, got, ref, yard, n2, nl):
    if ref["dmap"] is None:
        assert got["dmap"] is None
    else:
        (D, S), Y = ref["dmap"], yard["dmap"][0]
        if nl > 0:
            _hold_c(tag + " dmap(iΩ)", got["dmap"][:, :nl], D[:, :nl], Y[:, :nl], S[:, :nl], n2)
        if D.shape[1] > nl:
            _hold_c(tag + " dmap(ω)", got["dmap"][:, nl:], D[:, nl:], Y[:, nl:], S[:, nl:], n2)
    _hold_c(tag + " rho", got["rho"], ref["rho"][0], yard["rho"][0], ref["rho"][1], n2)


@pytest.mark.parametrize("case", MP.MAP, ids=_ids)
def test_response_map(dwhmc, oracle, VX, monkeypatch, case):
    """dmap[k, z, e] and rho[e] on the bond pattern, a random pattern with duplicates and
    hole-hole / hole-particle entries, and a column of 70 entries (slices of 32 + 32 + 6);
    0, 1 or 3 Matsubara indices and 0, 1 or 4 real frequencies of either sign (none at
    all: rho only); one case in chunks of 2 + 2 + 1 frequencies, the second chunk half
    Matsubara and half retarded; 2N = 70, 258, 520: the one-element tail, a pair plus
    the tail and the longer loop of k_map_sddmm"""
    family, beta, n2, kind, nl, nfreq, chunk = case
    E, U, vs, pat, om, ref, yard = MP.map_case(oracle, VX, *case)
    p, ctx = _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U, chunk)
    got = ctx.measure_response_map(vs, pat, n_matsubara=nl, omega=om if nfreq else None, eta=ETA)
    assert np.array_equal(got["pattern"], pat)
    _hold_map(_tag("map", case), got, ref, yard, n2, nl)
    _verdict()


# --------------------------------------------------------------------------- correlations
def _hold_corr(tag, got, ref, yard, n2):
    for k in ("mean", "corr", "local"):
        v, S = ref[k]
        _hold_c(f"{tag} {k}", np.asarray(got[k]).reshape(np.shape(v)), v, yard[k][0], S, n2)


@pytest.mark.parametrize("case", MP.CORR, ids=_ids)
def test_correlations(dwhmc, oracle, VX, monkeypatch, case):
    """mean, corr and local of the density, a bond and a pair family and of a term table
    by hand (a site at the cap of 64 terms, sites with none, duplicates), (k, k) and cross
    pairs, with reference sites (the site-list route, a site per workgroup); N = 260 has
    two displacement tiles, the second with 4 live lanes, and 17 chunks of sites"""
    family, beta, n2 = case
    E, U, fams, pairs, sites, ref, yard = MP.corr_case(oracle, VX, *case)
    p, ctx = _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U)
    got = ctx.measure_correlations(fams, pairs=pairs, ref_sites=sites)
    assert got["corr"].shape == (len(pairs), p.Ly, p.Lx) and got["local"].shape == (len(pairs), len(sites), p.Ly, p.Lx)
    _hold_corr(_tag("corr", case), got, ref, yard, n2)
    _verdict()


# --------------------------------------------------------------------------- one batched call per entry
def test_three_states_of_different_families(dwhmc, oracle, VX, monkeypatch):
    """nstates = 3 in one batched call of each of the three entries, a different family per state"""
    n2, beta = 70, 8.0
    nb = [MP.nambu_case(oracle, VX, f, beta, n2, 9, 17, 5) for f in MP.BATCH]
    mp = [MP.map_case(oracle, VX, f, beta, n2, "random", 3, 2) for f in MP.BATCH]
    cr = [MP.corr_case(oracle, VX, f, beta, n2) for f in MP.BATCH]
    E, U = np.stack([c[0] for c in nb]), np.stack([c[1] for c in nb])
    p, ctx = _ctx(dwhmc, oracle, n2, beta)
    deltas = np.zeros((3, p.N, 2), dtype=np.complex128)
    _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U)
    a = ctx.measure_nambu_response(nb[0][2], nb[0][3], n_matsubara=9, omega=nb[0][4], eta=ETA, deltas=deltas)
    _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U)
    b = ctx.measure_response_map(mp[0][2], mp[0][3], n_matsubara=3, omega=mp[0][4], eta=ETA, deltas=deltas)
    _inject(dwhmc, oracle, monkeypatch, n2, beta, E, U)
    c = ctx.measure_correlations(cr[0][2], pairs=cr[0][3], ref_sites=cr[0][4], deltas=deltas)
    for k, f in enumerate(MP.BATCH):
        assert np.array_equal(mp[k][0], E[k]) and np.array_equal(cr[k][1], U[k])
        _hold_nambu(f"batch {f}", {x: a[x][k] for x in ("chi", "chi2")}, nb[k][5], nb[k][6], n2)
        _hold_map(f"batch {f}", {x: b[x][k] for x in ("dmap", "rho")}, mp[k][5], mp[k][6], n2, 3)
        _hold_corr(f"batch {f}", {x: c[x][k] for x in ("mean", "corr", "local")}, cr[k][5], cr[k][6], n2)
    _verdict()
