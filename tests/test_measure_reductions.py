"""The measurement reductions on prescribed eigensystems (gpu): transport,
spectral maps, Λ(q, iΩ_l) and the operator response reduce eigenpairs that
dwh_debug_set_eigensystem injects (tests/measure_cases.py: spectrum families
around every branch rule, U Haar or particle-hole closed, 2N chosen against
the 256-pair tile), and every output value is held to

    |device - reference| <= max(8 |yardstick - reference|, 2N eps S)  (+ allowance)

with reference / yardstick the long-double / fp64 runs of tests/
measure_reference.py (pinned by tests/test_measure_reference.py), S = Σ |term|
of the value's sum, and the allowance what pairs within a factor 2 of the Δf
rule could move (0 on every case here: the spectra keep out of that window).
The factor 8 is tests/test_cr_kernels.py's margin: the device may be 8 x worse
than cancellation-free fp64 on the same input, not more.

Measured on an MI355X, worst ratio  device error / max(yardstick error, 2N eps S)
per output over the cases of this file, on the parent commit's kernels and on
this commit's (profiles/measure_reductions.txt has them per entry and family):

    output                     parent     branch
    superfluid_stiffness          468     0.0116
    dc_conductivity          1.48e+09      0.169
    optical_conductivity         55.8      0.266
    dos                          6.88      0.112
    dos_AN                       6.92      0.129
    A_k_omega0                  0.129      0.129
    dia                      0.000669   0.000669
    Λ(q, l = 0)              1.34e+03     0.0225
    Λ(q, l >= 1)               0.0354     0.0319
    χ(l = 0)                 1.56e+03     0.0168
    χ(l >= 1)                  0.0258     0.0331
    χ''(ω)                       6.84      0.134
    LDOS(r, ω)                  0.108      0.108
    A(k, ω)                     0.137      0.137

The yardstick's own error is 1e-3 … 1e-2 of 2N eps S on these inputs, so the
bar is in effect 2N eps S, and a ratio above 1 fails.  No output needs a factor
above 8: none is raised.  The parent's failures were 1.0 - f (σ_DC on cold and
one-sided spectra), the plain f_n - f_m (the l = 0 quotient just above the
1e-8 rule; the σ and χ'' weights of two levels on one side of the Fermi level)
and frequency grids contracted to one fma (DOS, σ at small η): DESIGN.md §5.
"""
import numpy as np
import pytest

import measure_cases as MC
import measure_reference as R

pytestmark = pytest.mark.gpu

LD, F8 = np.longdouble, np.float64
EPS = float(np.finfo(F8).eps)
ETA = 0.05

_ctxs, _refs = {}, {}


def _ctx(dwhmc, oracle, n2, beta):
    key = (n2, float(beta))
    if key not in _ctxs:
        p = MC.params(oracle, n2, beta)
        _ctxs[key] = (p, dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table,
                                              np.zeros(p.N), algo="eig"))
    return _ctxs[key]


def _once(key, make):
    """a reference, computed once per module and handed out unchanged"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _hold(what, dev, ref, yard, S, n2, allowance=0):
    """the bar, per value; prints the measured ratio before it asserts"""
    dev = np.asarray(dev, dtype=F8).astype(LD)
    ref, yard, S = (np.asarray(x, dtype=LD) for x in (ref, yard, S))
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    err = np.abs(dev - ref)
    floor = LD(n2) * LD(EPS) * np.abs(S)
    scale = np.maximum(np.abs(yard - ref), floor)
    ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))
    print(f"RATIO {what}: {float(np.max(ratio)):.3g}")
    bound = R.bound(ref, yard, S, n2) + np.abs(np.asarray(allowance, dtype=LD))
    bad = err > bound
    if bad.any():
        k = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
        _failures.append(f"{what}: {int(bad.sum())} of {bad.size} values beyond the bar, worst ratio "
                         f"{float(np.max(ratio)):.3g} at {k}: device {float(dev[k])!r}, reference {float(ref[k])!r}, "
                         f"bound {float(bound[k]):.3g}")


_failures = []


@pytest.fixture(autouse=True)
def _fresh_failures():
    _failures.clear()


def _verdict():
    """every output of a case is measured and printed before the case fails"""
    msgs = list(_failures)
    _failures.clear()
    assert not msgs, "\n".join(msgs)


def _grid_lengths(O, eta, domega, omega_max):
    return len(O.julia_range(eta, domega, omega_max)), len(O.julia_range(-omega_max, domega, omega_max))


TR_KEYS = ("superfluid_stiffness", "dc_conductivity", "optical_conductivity", "dos", "dos_AN", "A_k_omega0")


def _transport_ref(O, family, n2, beta, eta, domega, omega_max, E=None, U=None):
    def make():
        p = MC.params(O, n2, beta)
        e, u = MC.eigensystem(family, n2, beta) if E is None else (E, U)
        nw, nd = _grid_lengths(O, eta, domega, omega_max)
        br = R.Branches(e, beta, eta)
        return e, u, R.transport(e, u, p, beta, eta, domega, nw, nd, omega_max, LD, br), \
            R.transport(e, u, p, beta, eta, domega, nw, nd, omega_max, F8, br)
    return _once(("tr", family, n2, beta, eta, domega, omega_max), make)


def _hold_transport(tag, got, ref, yard, n2):
    for k in TR_KEYS:
        _hold(f"{tag} {k}", got[k], ref[k][0], yard[k][0], ref[k][1], n2,
              ref["amb_sigma"] if k == "optical_conductivity" else 0)


# --------------------------------------------------------------------------- transport
TRANSPORT = [(f, b, n2) for n2 in (32, 70) for f, b in
             (("generic", 4.0), ("generic", 8.0), ("twins", 8.0), ("dfedge", 8.0), ("cold5", 100.0), ("cold15", 100.0),
              ("cold25", 100.0), ("cold5", 1000.0), ("cold25", 1000.0), ("zeros", 8.0), ("akcut", 8.0))]
TRANSPORT += [("generic", 4.0, 256), ("dfedge", 8.0, 256), ("twins", 8.0, 258), ("cold25", 1000.0, 258),
              ("generic", 4.0, 520)]


@pytest.mark.parametrize("family,beta,n2", TRANSPORT)
def test_transport(dwhmc, oracle, family, beta, n2):
    """every output of measure_transport; σ on 65 and the DOS on 81 points"""
    eta = MC.AK_CUT_ETA if family == "akcut" else ETA
    domega, omega_max = 0.0625, eta + 4.0
    E, U, ref, yard = _transport_ref(oracle, family, n2, beta, eta, domega, omega_max)
    MC.check_family(family, E, beta, eta)
    _, ctx = _ctx(dwhmc, oracle, n2, beta)
    ctx.debug_set_eigensystem(E, U)
    got = ctx.measure_transport(eta, domega, omega_max)
    assert ctx.info["eig_half"] == 0 and ctx.info["eig_quat"] == 0
    _hold_transport(f"transport {family} b{beta:g} n{n2}", got, ref, yard, n2)
    _verdict()


@pytest.mark.parametrize("which,length", [(w, n) for w in ("sigma", "dos") for n in (1, 63, 64, 65, 255, 256, 257, 600)])
def test_transport_grid_lengths(dwhmc, oracle, which, length):
    """σ and DOS grids around the 64- and 256-point tiles of their kernels, 2N = 70"""
    n2, beta, domega = 70, 8.0, 0.01
    if which == "sigma":
        eta, omega_max = ETA, ETA + (length - 1) * domega + domega / 4
    elif length == 1:
        eta, omega_max = 0.002, domega / 4           # -ω_max:Δω:ω_max is one point below Δω/2
    else:
        eta, omega_max = 0.004, (length - 1) * domega / 2
    nw, nd = _grid_lengths(oracle, eta, domega, omega_max)
    assert (nw if which == "sigma" else nd) == length, (nw, nd)
    E, U, ref, yard = _transport_ref(oracle, "generic", n2, beta, eta, domega, omega_max)
    _, ctx = _ctx(dwhmc, oracle, n2, beta)
    ctx.debug_set_eigensystem(E, U)
    got = ctx.measure_transport(eta, domega, omega_max)
    assert len(got["optical_conductivity"]) == nw and len(got["dos"]) == nd
    _hold_transport(f"grid {which} {length}", got, ref, yard, n2)
    _verdict()


@pytest.mark.parametrize("n2", [32, 70, 258, 520])
def test_particle_hole_closed(dwhmc, oracle, n2):
    """E antisymmetric, column 2N-1-n the Nambu partner of column n: the half-pair
    sums (ph = 1) and the full sums (ph = 0) both meet the reference, and each
    other within the sum of their bounds"""
    beta, domega, omega_max = 8.0, 0.0625, ETA + 4.0
    E, U, ref, yard = _transport_ref(oracle, "ph", n2, beta, ETA, domega, omega_max)
    MC.check_family("ph", E, beta)
    _, ctx = _ctx(dwhmc, oracle, n2, beta)
    got = {}
    for ph in (1, 0):
        ctx.debug_set_eigensystem(E, U, ph=bool(ph))
        got[ph] = ctx.measure_transport(ETA, domega, omega_max)
        assert ctx.info["eig_half"] == ph
        _hold_transport(f"ph={ph} n{n2}", got[ph], ref, yard, n2)
    for k in TR_KEYS:
        b = R.bound(ref[k][0], yard[k][0], ref[k][1], n2)
        d = np.abs(np.asarray(got[1][k], dtype=F8).astype(LD) - np.asarray(got[0][k], dtype=F8).astype(LD))
        assert np.all(d <= 2 * b), (k, float(np.max(d)))
    _verdict()


# --------------------------------------------------------------------------- current response
QS = [(0, 0), (0, 1), (1, 2)]
RESPONSE = [("generic", 8.0, 32, 1, None, "x"), ("generic", 8.0, 32, 2, None, "y"), ("twins", 8.0, 70, 2, 1, "x"),
            ("twins", 8.0, 32, 8, 2, "y"), ("cold15", 100.0, 70, 8, 2, "x"), ("cold25", 1000.0, 32, 9, None, "y"),
            ("zeros", 8.0, 32, 9, None, "x"), ("dfedge", 8.0, 70, 17, 2, "y"), ("twins", 8.0, 258, 17, 2, "x"),
            ("generic", 4.0, 256, 9, 1, "y"), ("generic", 4.0, 520, 9, None, "x")]


@pytest.mark.parametrize("family,beta,n2,nl,group,a", RESPONSE)
def test_current_response(dwhmc, oracle, monkeypatch, family, beta, n2, nl, group, a):
    """dia and Λ(q, iΩ_l): Matsubara chunks of 8 with the one-accumulator last launch
    (nl = 1, 2, 8, 9, 17), momentum groups of 1, 2 and all"""
    qs = QS[:1] if n2 == 520 else QS[:2] if n2 >= 256 else QS
    p, ctx = _ctx(dwhmc, oracle, n2, beta)

    def make():
        E, U = MC.eigensystem(family, n2, beta)
        br = R.Branches(E, beta)
        return E, U, R.current_response(E, U, p, beta, a, qs, nl, LD, br), R.current_response(E, U, p, beta, a, qs, nl, F8, br)
    E, U, ref, yard = _once(("rs", family, n2, beta, nl, a), make)
    if group is None:
        monkeypatch.delenv("DWHMC_RESPONSE_GROUP", raising=False)
    else:
        monkeypatch.setenv("DWHMC_RESPONSE_GROUP", str(group))
    ctx.debug_set_eigensystem(E, U)
    got = ctx.measure_current_response(a, qs, n_matsubara=nl)
    tag = f"response {family} b{beta:g} n{n2} nl{nl}"
    _hold(tag + " dia", got["dia"], ref[0][0], yard[0][0], ref[0][1], n2)
    _hold(tag + " lam0", got["lam"][:, 0], ref[1][0][:, 0], yard[1][0][:, 0], ref[1][1][:, 0], n2)
    if nl > 1:
        _hold(tag + " lam", got["lam"][:, 1:], ref[1][0][:, 1:], yard[1][0][:, 1:], ref[1][1][:, 1:], n2)
    _verdict()


# --------------------------------------------------------------------------- operator response
OPERATOR = [("generic", 8.0, 32, 1), ("generic", 8.0, 70, 63), ("twins", 8.0, 70, 64), ("dfedge", 8.0, 32, 65),
            ("dfedge", 8.0, 70, 255), ("cold15", 100.0, 32, 256), ("zeros", 8.0, 70, 257), ("generic", 4.0, 32, 601),
            ("dfedge", 8.0, 256, 65), ("twins", 8.0, 258, 65), ("generic", 4.0, 520, 65)]


@pytest.mark.parametrize("family,beta,n2,nw", OPERATOR)
def test_operator_response(dwhmc, oracle, monkeypatch, family, beta, n2, nw):
    """χ(iΩ_l) and χ''(ω) of a non-Hermitian V with either spin sign and a Hermitian
    one, on grids through ω = 0 of lengths around the 64- and 256-point tiles;
    operator groups of 1 (2N = 32), 2 (70) and all"""
    p, ctx = _ctx(dwhmc, oracle, n2, beta)
    N = p.N
    ops = [(MC.random_operator(N, 3), -1), (MC.random_operator(N, 4), 1), (MC.random_operator(N, 5, hermitian=True), 1)]
    ops = ops[:1] if n2 == 520 else ops[:2] if n2 >= 256 else ops
    nl = 9 if n2 < 256 else 2
    step = 0.0625 if nw < 100 else 0.015625
    w0 = -step * (nw // 2)
    w = R.grid(w0, step, nw)
    assert 0.0 in w and (nw == 1 or w[0] < 0 < w[-1])

    def make():
        E, U = MC.eigensystem(family, n2, beta)
        br = R.Branches(E, beta)
        return E, U, [R.operator_response(E, U, p, beta, V, s, nl, ETA, w, LD, br) for V, s in ops], \
            [R.operator_response(E, U, p, beta, V, s, nl, ETA, w, F8, br) for V, s in ops]
    E, U, ref, yard = _once(("op", family, n2, beta, nw), make)
    group = {32: "1", 70: "2"}.get(n2)
    if group is None:
        monkeypatch.delenv("DWHMC_RESPONSE_GROUP", raising=False)
    else:
        monkeypatch.setenv("DWHMC_RESPONSE_GROUP", group)
    ctx.debug_set_eigensystem(E, U)
    got = ctx.measure_operator_response([V for V, _ in ops], spin_sign=[s for _, s in ops], n_matsubara=nl,
                                        omega=(w0, step, nw), eta=ETA)
    assert np.array_equal(got["omega"], w)
    tag = f"operator {family} b{beta:g} n{n2} nw{nw}"
    for k in range(len(ops)):
        (chi, Sc), (c2, S2), amb = ref[k]
        _hold(f"{tag} chi0[{k}]", got["chi"][k, :1], chi[:1], yard[k][0][0][:1], Sc[:1], n2)
        _hold(f"{tag} chi[{k}]", got["chi"][k, 1:], chi[1:], yard[k][0][0][1:], Sc[1:], n2)
        _hold(f"{tag} chi2[{k}]", got["chi2"][k], c2, yard[k][1][0], S2, n2, amb)
    _verdict()


# --------------------------------------------------------------------------- spectral maps
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("n2,first,count,stride", [(70, 0, 1, 1), (70, 3, 63, 2), (70, 1, 64, 1), (258, 2, 65, 3),
                                                   (258, 0, 64, 2), (32, 5, 65, 1)])
def test_spectral_maps(dwhmc, oracle, monkeypatch, fused, n2, first, count, stride):
    """LDOS(r, ω) and A(k, ω) on both routes, windows of 1, 63, 64, 65 frequencies:
    the 64-wide tiles and 16-deep K chunks of the fused kernel with tails in
    rows (N = 35, 129, 16), columns and K (2N = 70, 258, 32)"""
    beta, domega, omega_max = 8.0, 0.03125, 4.0
    p, ctx = _ctx(dwhmc, oracle, n2, beta)
    w = R.grid(-omega_max, domega, first + (count - 1) * stride + 1)[first::stride]
    assert len(w) == count

    def make():
        E, U = MC.eigensystem("generic", n2, beta)
        return E, U, R.spectral_maps(E, U, p, ETA, w, LD), R.spectral_maps(E, U, p, ETA, w, F8)
    E, U, ref, yard = _once(("sp", n2, first, count, stride), make)
    monkeypatch.setenv("DWHMC_SPECTRAL_FUSED", fused)
    ctx.debug_set_eigensystem(E, U)
    got = ctx.measure_spectral_maps(ETA, domega, omega_max, first=first, count=count, stride=stride)
    assert np.array_equal(got["omega"], w)
    for k, name in enumerate(("ldos", "akw")):
        _hold(f"spectral fused={fused} n{n2} {name}", got[name][0], ref[k], yard[k], ref[k], n2)
    _verdict()


# --------------------------------------------------------------------------- batches, the entry
def test_three_states_of_different_families(dwhmc, oracle):
    """nstates = 3 in one batched call of each entry, a different family per state"""
    n2, beta, domega, omega_max = 70, 8.0, 0.0625, ETA + 4.0
    p, ctx = _ctx(dwhmc, oracle, n2, beta)
    fams = ("twins", "dfedge", "generic")
    tr = [_transport_ref(oracle, f, n2, beta, ETA, domega, omega_max) for f in fams]
    E, U = np.stack([t[0] for t in tr]), np.stack([t[1] for t in tr])
    deltas = np.zeros((3, p.N, 2), dtype=np.complex128)
    ctx.debug_set_eigensystem(E, U)
    got = ctx.measure_transport_deltas(deltas, ETA, domega, omega_max)
    for k, f in enumerate(fams):
        _hold_transport(f"batch {f}", got[k], tr[k][2], tr[k][3], n2)
    nl, w = 9, R.grid(-0.5, 0.0625, 17)
    V = MC.random_operator(p.N, 3)
    ctx.debug_set_eigensystem(E, U)
    rs = ctx.measure_current_response("x", QS, n_matsubara=nl, deltas=deltas)
    ctx.debug_set_eigensystem(E, U)
    op = ctx.measure_operator_response([V], spin_sign=[-1], n_matsubara=nl, omega=(-0.5, 0.0625, 17), eta=ETA,
                                       deltas=deltas)
    ctx.debug_set_eigensystem(E, U)
    sp = ctx.measure_spectral_maps(ETA, domega, omega_max, first=2, count=17, stride=3, deltas=deltas)
    for k, f in enumerate(fams):
        br = R.Branches(E[k], beta)
        r, y = (R.current_response(E[k], U[k], p, beta, "x", QS, nl, dt, br) for dt in (LD, F8))
        _hold(f"batch {f} dia", rs["dia"][k], r[0][0], y[0][0], r[0][1], n2)
        _hold(f"batch {f} lam", rs["lam"][k], r[1][0], y[1][0], r[1][1], n2)
        r, y = (R.operator_response(E[k], U[k], p, beta, V, -1, nl, ETA, w, dt, br) for dt in (LD, F8))
        _hold(f"batch {f} chi", op["chi"][k, 0], r[0][0], y[0][0], r[0][1], n2)
        _hold(f"batch {f} chi2", op["chi2"][k, 0], r[1][0], y[1][0], r[1][1], n2, r[2])
        r, y = (R.spectral_maps(E[k], U[k], p, ETA, sp["omega"], dt) for dt in (LD, F8))
        _hold(f"batch {f} ldos", sp["ldos"][k], r[0], y[0], r[0], n2)
        _hold(f"batch {f} akw", sp["akw"][k], r[1], y[1], r[1], n2)
    _verdict()


def test_entry_validation_and_one_shot(dwhmc, oracle):
    n2, beta = 32, 8.0
    p, ctx = _ctx(dwhmc, oracle, n2, beta)
    E, U = MC.eigensystem("ph", n2, beta)
    lib, h = ctx._lib, ctx._h
    Ecm, Ucm = np.ascontiguousarray(E), np.ascontiguousarray(U.T)
    pe, pu = Ecm.ctypes.data, Ucm.ctypes.data
    assert lib.dwh_debug_set_eigensystem(None, 1, pe, pu, 0) == -1
    assert lib.dwh_debug_set_eigensystem(h, 1, None, pu, 0) == -1 and b"NULL" in lib.dwh_last_error(h)
    assert lib.dwh_debug_set_eigensystem(h, 1, pe, None, 0) == -1
    for ns in (0, -1, 1 << 40):
        assert lib.dwh_debug_set_eigensystem(h, ns, pe, pu, 0) == -1 and b"nstates" in lib.dwh_last_error(h)
    for bad in (np.nan, np.inf):
        Eb = E.copy()
        Eb[3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ctx.debug_set_eigensystem(Eb, U)
        Ub = U.copy()
        Ub[2, 5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            ctx.debug_set_eigensystem(E, Ub)
    with pytest.raises(ValueError, match="ascending"):
        ctx.debug_set_eigensystem(E[::-1].copy(), U)
    Eb = E.copy()
    Eb[-1] += 1e-9
    ctx.debug_set_eigensystem(Eb, U)                      # fine without ph ...
    with pytest.raises(ValueError, match="ph"):
        ctx.debug_set_eigensystem(Eb, U, ph=True)         # ... refused with it, and the staging is gone:
    q = ctx.measure_current_response("x", [(0, 0)])       # a real solve of the context's own H_BdG
    ctx.debug_set_eigensystem(E, U)
    with pytest.raises(ValueError, match="staged 1"):     # three states against one staged
        ctx.measure_current_response("x", [(0, 0)], deltas=np.zeros((3, p.N, 2), dtype=np.complex128))
    again = ctx.measure_current_response("x", [(0, 0)])   # cleared by the refusal: the real solve again
    assert again["dia"] == q["dia"] and np.array_equal(again["lam"], q["lam"])
    ctx.debug_set_eigensystem(E, U)
    inj = ctx.measure_current_response("x", [(0, 0)])
    assert inj["dia"] != q["dia"]
    once = ctx.measure_current_response("x", [(0, 0)])    # one-shot
    assert once["dia"] == q["dia"]
