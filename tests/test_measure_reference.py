"""Pins of tests/measure_reference.py (CPU): the one restatement that
tests/test_measure_reductions.py holds the device to.

  * against mpmath at 40 digits on the smallest case (2N = 32): the Fermi
    identities at the arguments where the plain forms cancel, and one full Λ(q,
    l = 0, 1), σ_DC, σ(ω) (as the reference writes it: every ordered pair, 1/ω,
    no fold), χ''(ω) and DOS value.  Bound: 16 · 2N · eps_longdouble · S — the
    products U^H A U sum 2N terms whose absolute sum is a few times the entry
    (Haar vectors), squared (×2), then the pair sum; eps = 1.08e-19.
  * against the fp64 restatements the suite already trusts — the oracle's
    transport, tests/test_current_response.py's `_Ref`, tests/
    test_operator_response.py's `_Ref` — on the eigenpairs of a disordered
    4 x 4 and 5 x 7 (β = 8) at their tolerances: 1e-9 (1 + |ref|) for scalars,
    1e-9 (1 + max|ref|) for grids.
  * the family conditions of tests/measure_cases.py, the Nambu partner map
    against the eigenvectors of a real H_BdG, and the ambiguity allowance:
    on every case of the device file the pairs within a factor 2 of the Δf
    rule may move σ(ω) / χ''(ω) by less than a tenth of the bound without them.
  * the (value, S) references of the Nambu response, the response maps and the
    correlations (tests/measure_pair_cases.py): the fp64 run is the restatement
    the parity tests use, S >= |value|, the sampled map is the whole matrix,
    g_loops is the vectorised G, every injected spectrum meets its family and
    keeps out of the Δf window, and the yardstick stays within 2N eps S on
    every device case.
"""
import mpmath as mp
import numpy as np
import pytest

import measure_cases as MC
import measure_pair_cases as MP
import measure_reference as R
from correlation_reference import CorrRef
from nambu_reference import NRef
from oracle_measurements import CurrentRef as RefCurrent, OperatorRef as RefOperator
from response_map_reference import MapRef
from test_current_response import QLIST, _case

LD, F8 = np.longdouble, np.float64
EPS_LD = float(np.finfo(LD).eps)


# --------------------------------------------------------------------------- mpmath
def _mpf(x):
    """exact mpf of a long double"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def test_fermi_identities_against_mpmath():
    mp.mp.dps = 40
    worst = 0.0
    for dt, eps in ((LD, EPS_LD), (F8, 2.3e-16)):
        for beta, e in ((8.0, -3.75), (8.0, 3.1), (100.0, -0.25), (1000.0, -0.03), (1000.0, 0.005), (4.0, 0.0), (8.0, -0.0)):
            f, g = R.fermi(np.array([e]), beta, dt)
            fm = 1 / (1 + mp.exp(mp.mpf(beta) * mp.mpf(e)))
            for got, want in ((f[0], fm), (g[0], 1 - fm), (dt(beta) * f[0] * g[0], beta * fm * (1 - fm))):
                rel = abs(_mpf(LD(got)) - want) / want
                worst = max(worst, float(rel / eps))
                assert rel <= 8 * eps, (dt, beta, e, float(rel))
        # f_n - f_m at the gaps around the 1e-8 rule, and far apart on one side
        for beta, e0, gap in ((8.0, 0.3, 2e-8), (8.0, -1.0, 1e-7), (8.0, 0.0, 1e-6), (8.0, -3.4, 0.2), (1000.0, 0.02, 5e-9)):
            E = np.array([e0, e0 + gap])
            df, dE = R.delta_f(E, beta, dt)
            d = mp.mpf(float(E[1])) - mp.mpf(float(E[0]))
            fa, fb = (1 / (1 + mp.exp(mp.mpf(beta) * mp.mpf(float(x)))) for x in E)
            rel = abs(_mpf(LD(df[0, 1])) - (fa - fb)) / (fa - fb)
            worst = max(worst, float(rel / eps))
            # dE is the fp64 difference of the inputs (the device's): its rounding is part of the rule
            assert rel <= 8 * eps + abs(_mpf(LD(dE[0, 1])) - d) / d, (dt, beta, e0, gap, float(rel))
            assert df[1, 0] == -df[0, 1]
    print("fermi identities: worst error / eps", worst)


def _mp_abs2(U, A):
    n = U.shape[0]
    Um = mp.matrix(n, n)
    Am = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Um[i, j] = mp.mpc(float(U[i, j].real), float(U[i, j].imag))
            Am[i, j] = A[i][j]
    M = Um.H * Am * Um
    return [[abs(M[i, j]) ** 2 for j in range(n)] for i in range(n)]


def test_full_values_against_mpmath(oracle):
    mp.mp.dps = 40
    n2, beta, eta = 32, 8.0, 0.05
    p = MC.params(oracle, n2, beta)
    N = p.N
    E, U = MC.eigensystem("generic", n2, beta)
    br = R.Branches(E, beta, eta)
    Em = [mp.mpf(float(e)) for e in E]
    f = [1 / (1 + mp.exp(beta * e)) for e in Em]
    pi = mp.pi

    def lor(x):
        return eta_m / (pi * (x * x + eta_m * eta_m))

    eta_m = mp.mpf(eta)
    # J_x(q) ⊕ J_x(q) at q = (1, 2) in mp, from the bond list
    mx, my = 1, 2
    A = [[mp.mpc(0) for _ in range(n2)] for _ in range(n2)]
    for j, tb, (dx, dy) in R.bonds(p, "x"):
        for i in range(N):
            x, y = i % p.Lx, i // p.Lx
            ang = -(2 * pi * mx / p.Lx * (x + mp.mpf(dx) / 2) + 2 * pi * my / p.Ly * (y + mp.mpf(dy) / 2))
            val = mp.mpc(0, 1) * mp.mpf(tb) * mp.expj(ang)
            for o in (0, N):
                A[i + o][int(j[i]) + o] += val
                A[int(j[i]) + o][i + o] -= val
    J2 = _mp_abs2(U, A)

    def r(n, m, l):
        dE = Em[m] - Em[n]
        if l == 0:
            return beta * f[n] * (1 - f[n]) if br.deg[n, m] else (f[n] - f[m]) / dE
        return (f[n] - f[m]) * dE / (dE * dE + (2 * pi * l / beta) ** 2)

    (_, _), (lam, S) = R.current_response(E, U, p, beta, "x", [(mx, my)], 2, LD, br)
    for l in range(2):
        want = sum(r(n, m, l) * J2[n][m] for n in range(n2) for m in range(n2)) / N
        err = abs(_mpf(lam[0, l]) - want)
        print("Λ l =", l, float(want), "error / (2N eps S)", float(err / (n2 * EPS_LD * _mpf(S[0, l]))))
        assert err <= 16 * n2 * EPS_LD * _mpf(S[0, l])

    # transport at q = 0: σ_DC, σ(ω_3) as written (ordered pairs, 1/ω), DOS(ω_5)
    A0 = [[mp.mpc(0) for _ in range(n2)] for _ in range(n2)]
    Jx = oracle.current_operator(p)
    for i in range(N):
        for j in range(N):
            if Jx[i, j] != 0:
                A0[i][j] = A0[i + N][j + N] = mp.mpc(float(Jx[i, j].real), float(Jx[i, j].imag))
    J20 = _mp_abs2(U, A0)
    nw, nd, dom = 8, 9, 0.25
    tr = R.transport(E, U, p, beta, eta, dom, nw, nd, 1.0, LD, br)
    want = pi / N * sum(beta * f[n] * (1 - f[n]) * J20[n][m] * lor(Em[m] - Em[n]) for n in range(n2) for m in range(n2))
    v, S = tr["dc_conductivity"]
    print("σ_DC", float(want), "error / (2N eps S)", float(abs(_mpf(v) - want) / (n2 * EPS_LD * _mpf(S))))
    assert abs(_mpf(v) - want) <= 16 * n2 * EPS_LD * _mpf(S)
    w3 = mp.mpf(float(R.grid(eta, dom, nw)[3]))
    want = pi / N * sum((f[n] - f[m]) / w3 * J20[n][m] * lor(w3 - (Em[m] - Em[n]))
                        for n in range(n2) for m in range(n2) if br.keep[n, m])
    v, S = tr["optical_conductivity"]
    print("σ(ω)", float(want), "error / (2N eps S)", float(abs(_mpf(v[3]) - want) / (n2 * EPS_LD * _mpf(S[3]))))
    assert abs(_mpf(v[3]) - want) <= 16 * n2 * EPS_LD * _mpf(S[3])
    w5 = mp.mpf(float(R.grid(-1.0, dom, nd)[5]))
    Wn = [sum(mp.mpf(float(abs(U[i, n]))) ** 2 for i in range(N)) for n in range(n2)]
    Wn = [sum(mp.mpf(float(U[i, n].real)) ** 2 + mp.mpf(float(U[i, n].imag)) ** 2 for i in range(N)) for n in range(n2)]
    want = sum(Wn[n] * lor(w5 - Em[n]) for n in range(n2)) / N
    v, S = tr["dos"]
    assert abs(_mpf(v[5]) - want) <= 16 * n2 * EPS_LD * _mpf(S[5])

    # χ''(ω) of a non-Hermitian V, s = -1, at ω = -0.3
    V = MC.random_operator(N, 3)
    Z = np.zeros((N, N))
    Vn = np.block([[V, Z], [Z, V.T]])                     # V ⊕ (-s V^T), s = -1
    V2 = _mp_abs2(U, [[mp.mpc(float(z.real), float(z.imag)) for z in row] for row in Vn])
    w = R.grid(-0.6, 0.3, 5)
    (_, _), (c2, S2), _ = R.operator_response(E, U, p, beta, V, -1, 1, eta, w, LD, br)
    wm = mp.mpf(float(w[1]))
    want = pi / N * sum((f[n] - f[m]) * V2[n][m] * lor(wm - (Em[m] - Em[n]))
                        for n in range(n2) for m in range(n2) if br.keep[n, m])
    print("χ''", float(want), "error / (2N eps S)", float(abs(_mpf(c2[1]) - want) / (n2 * EPS_LD * _mpf(S2[1]))))
    assert abs(_mpf(c2[1]) - want) <= 16 * n2 * EPS_LD * _mpf(S2[1])


# --------------------------------------------------------------------------- existing restatements
def _close(a, b, what):
    a, b = np.asarray(a, dtype=F8), np.asarray(b, dtype=F8)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    assert err <= 1e-9 * (1 + float(np.abs(b).max())), (what, err)


@pytest.mark.parametrize("Lx,Ly", [(4, 4), (5, 7)])
@pytest.mark.parametrize("dt", [F8, LD], ids=["yardstick", "reference"])
def test_against_the_fp64_restatements(oracle, Lx, Ly, dt):
    O = oracle
    p, dis, D = _case(O, Lx, Ly, 8.0, seed=Lx * 17 + Ly)
    cache, _, _ = O.evaluate(p, dis, D)
    E, U = cache.E_n.copy(), cache.U.copy()
    want = O.measure_transport_and_spectra(cache, p)
    nw, nd = len(want["omega_grid"]), len(want["dos_omega_grid"])
    assert np.array_equal(R.grid(p.eta, p.domega, nw), want["omega_grid"])
    got = R.transport(E, U, p, p.beta, p.eta, p.domega, nw, nd, p.omega_max, dt)
    for k in ("superfluid_stiffness", "dc_conductivity", "optical_conductivity", "dos", "dos_AN", "A_k_omega0"):
        _close(got[k][0], want[k], k)
    rc = RefCurrent(O, p, dis, D)
    for a in "xy":
        (d, _), (lam, _) = R.current_response(E, U, p, p.beta, a, QLIST, 3, dt)
        _close(d, rc.dia(a), "dia " + a)
        assert np.all(np.abs(np.asarray(lam, dtype=F8) - rc.lam(a, QLIST, 3)) <= 1e-9 * (1 + np.abs(rc.lam(a, QLIST, 3))))
    ro = RefOperator(O, p, dis, D)
    w = R.grid(-0.6, 0.3, 5)
    for s, herm in ((-1, False), (1, True)):
        V = MC.random_operator(p.N, 11 + s, hermitian=herm)
        (chi, _), (c2, _), _ = R.operator_response(E, U, p, p.beta, V, s, 3, 0.05, w, dt)
        assert np.all(np.abs(np.asarray(chi, dtype=F8) - ro.chi(V, s, 3)) <= 1e-9 * (1 + np.abs(ro.chi(V, s, 3))))
        _close(c2, ro.chi2(V, s, w, 0.05), "chi2")


# --------------------------------------------------------------------------- families, partner map, allowance
FAMILIES = [("generic", 4.0), ("generic", 8.0), ("twins", 8.0), ("dfedge", 8.0), ("cold5", 100.0), ("cold15", 100.0),
            ("cold25", 1000.0), ("zeros", 8.0), ("akcut", 8.0), ("ph", 8.0)]


@pytest.mark.parametrize("family,beta", FAMILIES)
@pytest.mark.parametrize("n2", sorted(MC.LATTICES))
def test_family_conditions(family, beta, n2):
    E = MC.spectrum(family, n2, beta)
    assert E.shape == (n2,) and np.all(np.isfinite(E))
    MC.check_family(family, E, beta, MC.AK_CUT_ETA)


def test_nambu_partner_is_the_map_of_h_bdg(oracle):
    """Θ(u; v) = (-conj v; conj u) sends the eigenvector of E to one of -E for the
    H_BdG the library assembles (here: the oracle's, which the assembly tests pin
    bit for bit), and ph_closed builds a unitary closed under it."""
    p, dis, D = _case(oracle, 4, 4, 8.0, seed=72)
    cache, _, _ = oracle.evaluate(p, dis, D)
    H = oracle.hermitian_from_upper(cache.H_base)
    n2 = 2 * p.N
    for n in (0, 5, n2 - 1):
        x = R.nambu_partner(cache.U[:, n], p.N)
        assert np.abs(H @ x + cache.E_n[n] * x).max() <= 1e-13 * (1 + np.abs(cache.E_n).max())
    for size in (32, 70):
        U = R.ph_closed(size, 7)
        assert np.abs(U.conj().T @ U - np.eye(size)).max() <= 1e-13
        for n in range(size // 2):
            assert np.array_equal(U[:, size - 1 - n], R.nambu_partner(U[:, n], size // 2))


@pytest.mark.parametrize("family,beta", FAMILIES)
@pytest.mark.parametrize("n2", [32, 70])
def test_ambiguity_allowance_is_small(oracle, family, beta, n2):
    """Pairs within a factor 2 of the Δf rule may fall either way on the device;
    what they can move is added to the bound, and must stay below a tenth of it."""
    p = MC.params(oracle, n2, beta)
    E, U = MC.eigensystem(family, n2, beta)
    eta = MC.AK_CUT_ETA if family == "akcut" else 0.05
    br = R.Branches(E, beta, eta)
    ref = R.transport(E, U, p, beta, eta, 0.125, 17, 9, 0.5, LD, br)
    yard = R.transport(E, U, p, beta, eta, 0.125, 17, 9, 0.5, F8, br)
    v, S = ref["optical_conductivity"]
    b = R.bound(v, yard["optical_conductivity"][0], S, n2)
    print(family, n2, "ambiguous pairs", int(br.ambiguous_df().sum()), "allowance / bound",
          float(np.max(np.abs(ref["amb_sigma"]) / b)))
    assert np.all(np.abs(ref["amb_sigma"]) <= b / 10)
    V = MC.random_operator(p.N, 5)
    w = R.grid(-0.5, 0.125, 9)
    _, (c2, S2), amb = R.operator_response(E, U, p, beta, V, -1, 1, eta, w, LD, br)
    _, (y2, _), _ = R.operator_response(E, U, p, beta, V, -1, 1, eta, w, F8, br)
    assert np.all(amb <= R.bound(c2, y2, S2, n2) / 10)


# --------------------------------------------------------------------------- the pair, map and correlation references
# (tests/measure_pair_cases.py, held on the device by tests/test_measure_reductions_pairs.py)
EPS = float(np.finfo(F8).eps)


@pytest.fixture(scope="module")
def VX(dwhmc):
    return dwhmc.vertices


def _parts(v):
    v = np.asarray(v)
    return (v.real, v.imag) if np.iscomplexobj(v) else (v,)


def _scale_covers(v, S, what):
    """S = Σ |term| >= |value| (a rounding of the sums apart)"""
    v, S = np.abs(np.asarray(v)).astype(LD), np.asarray(S, dtype=LD)
    assert v.shape == S.shape, (what, v.shape, S.shape)
    assert np.all(v <= S * (1 + LD(1e-12))), (what, float(np.max(v - S)))


@pytest.mark.parametrize("n2", [32, 70])
def test_value_and_scale_runs_are_the_restatements(oracle, VX, n2):
    """The fp64 (value, S) runs against NRef.response, MapRef.response (whole matrices) and
    CorrRef.response: the same bits where the code is shared, within 4 eps S where the map
    is summed in another order; and S >= |value| in both dtypes."""
    beta = 8.0
    p = MC.params(oracle, n2, beta)
    E, U, br = MP.system("generic", n2, beta)
    vs = MP.nambu_vertices(VX, p)
    Ws, pairs, w = [v.dense(p.N) for v in vs], MP.nambu_pairs(7, 5), R.grid(*MP.grid(9))
    pat = np.concatenate([MP.pattern(VX, p, k) for k in ("bond", "random", "col70")])
    fams = [VX.local_family(k, p) for k in MP.CORR_KINDS] + [MP.hand_family(VX, p.N)]
    sites = [0, p.N - 1]
    for dt in (F8, LD):
        nr = NRef(p, E, U, beta=beta, dt=dt, br=br)
        (chi, Sc), (c2, S2) = nr.response_s(Ws, pairs, 3, w, MP.ETA)
        _scale_covers(chi, Sc, "chi")
        _scale_covers(c2, S2, "chi2")
        mr = MapRef(p, E, U, beta=beta, dt=dt, br=br)
        D, SD = mr.sampled(Ws[0], pat, 3, MP.OMEGAS[4], MP.ETA)
        rho, Sr = mr.rho_s(pat)
        _scale_covers(D, SD, "dmap")
        _scale_covers(rho, Sr, "rho")
        cr = CorrRef(p, E, U, beta=beta, dt=dt, br=br)
        cs = cr.response_s(fams, MP.CORR_PAIRS, sites)
        for k, (v, S) in cs.items():
            _scale_covers(v, S, k)
        if dt is LD:
            continue
        old_chi, old_c2 = nr.response(Ws, pairs, 3, w, MP.ETA)
        assert np.array_equal(old_chi, chi) and np.array_equal(old_c2, c2)
        old_d, old_rho = mr.response(Ws[:1], pat, 3, MP.OMEGAS[4], MP.ETA)
        assert np.array_equal(old_rho, rho)
        for a, b in zip(_parts(D), _parts(old_d[0])):
            print("map, sampled against whole, worst / (eps S)", float(np.max(np.abs(a - b) / (EPS * SD))))
            assert np.all(np.abs(a - b) <= 4 * EPS * SD)
        old = cr.response(fams, MP.CORR_PAIRS, sites)
        for k, o in zip(("corr", "local", "mean"), old):
            assert np.array_equal(o.reshape(cs[k][0].shape), cs[k][0]), k


def test_sampled_map_is_the_whole_matrix(oracle, VX):
    """2N = 32, long double: the pattern entries of U (w ∘ X) U^H formed whole against the
    row products.  Both sum the same 2N x 2N terms of absolute sum S in another order:
    each within 2N eps S of the exact sum."""
    n2, beta = 32, 8.0
    p = MC.params(oracle, n2, beta)
    for family in ("generic", "twins", "dfedge"):
        E, U, br = MP.system(family, n2, beta)
        mr = MapRef(p, E, U, beta=beta, dt=LD, br=br)
        W = MP.map_vertices(VX, p)[0].dense(p.N)
        pat = np.stack(np.meshgrid(np.arange(n2), np.arange(n2), indexing="ij"), -1).reshape(-1, 2)
        D, S = mr.sampled(W, pat, 3, MP.OMEGAS[4], MP.ETA)
        whole = mr.dmat(W, 3, MP.OMEGAS[4], MP.ETA).reshape(D.shape)
        assert np.abs(whole).max() > 1e-3
        for a, b in zip(_parts(D), _parts(whole)):
            assert np.all(np.abs(a - b) <= 2 * n2 * EPS_LD * S), family
        rho, Sr = mr.rho_s(pat)
        assert np.all(np.abs(rho - mr.rho().reshape(-1)) <= 2 * n2 * EPS_LD * Sr)


@pytest.mark.parametrize("dt", [F8, LD], ids=["yardstick", "reference"])
def test_g_loops_is_the_vectorised_g(oracle, VX, dt):
    """4 x 4: the explicit loop over the terms against gmat_s.  Two orders of one sum of
    t_A t_B products of absolute sum <= S: apart by at most t_A t_B eps S."""
    n2, beta = 32, 8.0
    p = MC.params(oracle, n2, beta)
    E, U, br = MP.system("zeros", n2, beta)
    cr = CorrRef(p, E, U, beta=beta, dt=dt, br=br)
    fams = [VX.local_family("current_x", p), MP.hand_family(VX, p.N)]
    eps = EPS_LD if dt is LD else EPS
    for a, b in ((0, 0), (1, 1), (0, 1), (1, 0)):
        G, S = cr.gmat_s(fams[a], fams[b])
        L = cr.g_loops(fams[a], fams[b])
        ta, tb = (np.bincount(np.asarray(fams[k].site), minlength=p.N) for k in (a, b))
        terms = np.maximum(1, ta[:, None] * tb[None, :])
        assert np.abs(G).max() > 1e-3 and np.all(G[ta == 0] == 0) and np.all(G[:, tb == 0] == 0)
        for x, y in zip(_parts(G), _parts(L)):
            assert np.all(np.abs(x - y) <= terms * eps * S), (a, b)


def test_device_spectra_meet_their_families():
    """every spectrum a device case injects: its family's condition, and no pair within a
    factor 2 of the Δf rule, so the ambiguity allowance of those cases is 0"""
    for family, beta, n2 in MP.spectra():
        E, U, br = MP.system(family, n2, beta)
        MC.check_family(family, E, beta)
        assert not br.ambiguous_df().any(), (family, beta, n2)
        assert np.abs(U.conj().T @ U - np.eye(n2)).max() <= 1e-12
    fams = {f for f, _, _ in MP.spectra()}
    assert {"generic", "twins", "dfedge", "cold15", "cold25", "zeros", "ph"} <= fams


def _yardstick_within_floor(ref, yard, n2, what):
    """|yardstick - reference| <= 2N eps S on every value (so S >= |value| too): the bar of
    such a case is its floor, and only the device can miss it"""
    for k in ref:
        if ref[k] is None or ref[k][0] is None:
            continue
        (v, S), (y, _) = ref[k], yard[k]
        _scale_covers(v, S, (what, k))
        floor = LD(n2) * LD(EPS) * np.asarray(S, dtype=LD)
        worst = 0.0
        for a, b in zip(_parts(np.asarray(y).astype(R._c(LD)) if np.iscomplexobj(y) else y), _parts(v)):
            err = np.abs(np.asarray(a, dtype=LD) - b)
            assert np.all(err <= R.bound(b, a, S, n2)), (what, k)
            ok = floor > 0
            worst = max(worst, float(np.max(err[ok] / floor[ok])) if ok.any() else 0.0)
            assert np.all(err <= floor), (what, k, worst)
        print(f"YARDSTICK {what} {k}: {worst:.3g} of the floor")


@pytest.mark.parametrize("case", MP.NAMBU, ids=lambda c: "-".join(str(x) for x in c))
def test_yardstick_nambu(oracle, VX, case):
    *_, ref, yard = MP.nambu_case(oracle, VX, *case)
    _yardstick_within_floor(ref, yard, case[2], "nambu")


@pytest.mark.parametrize("case", MP.MAP, ids=lambda c: "-".join(str(x) for x in c))
def test_yardstick_map(oracle, VX, case):
    *_, ref, yard = MP.map_case(oracle, VX, *case)
    _yardstick_within_floor(ref, yard, case[2], "map")


@pytest.mark.parametrize("case", MP.CORR, ids=lambda c: "-".join(str(x) for x in c))
def test_yardstick_corr(oracle, VX, case):
    *_, ref, yard = MP.corr_case(oracle, VX, *case)
    _yardstick_within_floor(ref, yard, case[2], "corr")
