"""Finite-momentum current response (dwh_measure_current_response,
csrc/dwhmc_response.hip): with q = 2π (mx/Lx, my/Ly), Ω_l = 2π l/β,

    Jq[i, j_b(i)] += i t_b φ_b(i),  Jq[j_b(i), i] -= i t_b φ_b(i),
    φ_b(i) = exp(-i q·(r_i + δ_b/2)),   J_α(q) = Jq ⊕ Jq,
    Λ_αα(q, l) = (1/N) Σ_nm r_nm(l) |(U^H J_α(q) U)[n, m]|²

and dia_α = <-K_α> for the bond list of α (x: the reference's; y: +y, +x+y,
-x+y).  At q = 0, α = x, l = 0 this is the reference's stiffness
[src/Observables.jl:340-387], dia - Λ.

The reference values are a numpy restatement here (`_Ref`): E, U, f from the
oracle's `evaluate` (LAPACK), Jq by the triplet sum above, |U^H J U|², the r
rules (l = 0: the reference's, with β f (1 - f) where |E_m - E_n| < 1e-8;
l >= 1: (f_n - f_m) ΔE / (ΔE² + Ω_l²)).  Tolerance: the project's scalar
transport tolerance |Δ| <= 1e-9 (1 + |ref|) (tests/test_transport.py header);
every sum is basis-invariant inside degenerate levels.

CPU (not gpu): the restatement against the oracle's stiffness, its ±q and x<->y
identities, the clean 8 x 8 values, the NULL-context refusal, the vertices the
library uploads (dwh_debug_current_vertex) against the triplet sum and the driver
option on the oracle backend.  GPU: parity on lattices below / at / above the
product tile with tails and on the Lx = 2 ring, the grouping loop, consistency
with measure_transport, ±q, degenerate spectra with both solvers, snapshots,
chains, the other algorithms, errors and the timer.

Every column of J_nm is computed on the device (no particle-hole half sum), so
nothing here depends on DWHMC_EIG_HALF.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle_measurements import CurrentRef as _Ref, OracleResponse as _OracleResponse, jq as _jq, \
    simulate as _simulate

T, TP, MU = 1.0, -0.35, -1.08
TOL = 1e-9
QLIST = [(0, 0), (0, 1), (1, 0), (1, 2), (0, -1), (-1, 0)]
NL = 3


def _case(O, Lx, Ly, beta, seed, W=1.0, nimp=0.1, amp=0.25, mu=MU):
    p = O.ModelParameters(Lx, Ly, T, TP, mu, W, nimp, beta, 0.8, 1.0)
    rng = np.random.default_rng(seed)
    st = O.initialize_state(p, rng)
    N = p.N
    D = st.Delta + amp * np.stack([np.ones(N), -np.ones(N)], 1) * np.exp(0.3j * rng.standard_normal((N, 1)))
    return p, st.disorder_pot, D


def _clean(O, L, mu, beta=8.0):
    p = O.ModelParameters(L, L, T, TP, mu, 0.0, 0.0, beta, 0.8, 1.0)
    D = np.stack([np.full(p.N, 0.2), np.full(p.N, -0.2)], 1).astype(np.complex128)
    return p, np.zeros(p.N), D


def _close(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    assert np.all(err <= TOL * (1 + np.abs(b))), (what, float(err.max()), a, b)


def _ctx(dwhmc, p, dis, **kw):
    return dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis, **kw)


_refs = {}


def _ref_case(O, Lx, Ly, beta=8.0):
    """(p, disorder, Δ, _Ref, {direction: (dia, lam)}) of a disordered lattice, once per module."""
    key = (Lx, Ly, beta)
    if key not in _refs:
        p, dis, D = _case(O, Lx, Ly, beta, seed=4 if (Lx, Ly) == (2, 4) else Lx * 17 + Ly)
        ref = _Ref(O, p, dis, D)
        _refs[key] = (p, dis, D, ref, {a: (ref.dia(a), ref.lam(a, QLIST, NL)) for a in "xy"})
    return _refs[key]


# --------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (6, 6), (5, 7), (2, 4)])
def test_restatement_is_the_reference_stiffness(oracle, Lx, Ly):
    """q = 0, x, l = 0: dia - Λ is measure_transport_and_spectra's stiffness
    (the same operations in the same order: no rounding difference)."""
    O = oracle
    p, dis, D = _case(O, Lx, Ly, 8.0, seed=Lx * 17 + Ly)
    cache, _, _ = O.evaluate(p, dis, D)
    ref = _Ref(O, p, dis, D)
    st = ref.dia("x") - ref.lam("x", [(0, 0)], 1)[0, 0]
    want = O.measure_transport_and_spectra(cache, p)["superfluid_stiffness"]
    print("stiffness", Lx, Ly, st, want, st - want)
    assert st == want
    # and the q = 0 x operator is the reference's
    assert np.array_equal(_jq(p, "x", 0, 0), O.current_operator(p))


def test_restatement_pm_q(oracle):
    """Λ(q) = Λ(-q): J(-q) = J(q)^H and r is symmetric."""
    p, dis, D, ref, _ = _ref_case(oracle, 5, 7)
    qs = [(0, 1), (1, 0), (1, 2), (2, -3)]
    for a in "xy":
        lp, lm = ref.lam(a, qs, NL), ref.lam(a, [(-mx, -my) for mx, my in qs], NL)
        print("pm q", a, float(np.abs(lp - lm).max()))
        _close(lp, lm, a)
        J = _jq(p, a, 1, 2)
        assert np.array_equal(_jq(p, a, -1, -2), J.conj().T)
        assert np.abs(J - J.conj().T).max() > 0.1          # not Hermitian at q != 0


def test_restatement_clean_8x8(oracle):
    """Clean 8 x 8, μ = -1, β = 8, uniform d-wave 0.2: the x <-> y swap and
    the three limits: transverse < longitudinal < q = 0 (0.0948, 0.1387, 0.4746)."""
    p, dis, D = _clean(oracle, 8, -1.0)
    ref = _Ref(oracle, p, dis, D)
    qs = [(0, 0), (0, 1), (1, 0), (1, 2)]
    lx, ly = ref.lam("x", qs, NL), ref.lam("y", [(my, mx) for mx, my in qs], NL)
    print("clean 8x8", ref.dia("x"), ref.dia("y"), lx[:, 0])
    _close(lx, ly, "swap")
    _close(ref.dia("x"), ref.dia("y"), "dia")
    q0, tr, lo = (ref.dia("x") - lx[k, 0] for k in range(3))
    assert tr < lo < q0
    for got, want in ((q0, 0.4746), (tr, 0.0948), (lo, 0.1387)):
        assert abs(got - want) <= 5e-5, (got, want)         # the quoted digits


def test_null_context_is_refused(dwhmc):
    lib = dwhmc.load_library()
    buf = np.zeros(4)
    q = np.zeros(2, dtype=np.int64)
    pb, pq = buf.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)
    assert lib.dwh_measure_current_response(None, 0, 1, None, 0, 1, pq, 1, pb, pb) == -1
    assert b"NULL" in lib.dwh_last_error(None)
    assert dwhmc.FermionContext.TIMERS.index("response") == 13


@pytest.mark.parametrize("a", ["x", "y"])
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (5, 7), (2, 4)])
def test_debug_current_vertex(dwhmc, oracle, Lx, Ly, a):
    """The vertices the library uploads (dwh_debug_current_vertex, host only)
    are Jq ⊕ Jq of the triplet sum.  At Lx = 2 the +x and -x neighbours
    coincide: the duplicates' sum and the transposed entry share a slot."""
    p = oracle.ModelParameters(Lx, Ly, T, TP, MU, 0.0, 0.0, 8.0, 0.8, 1.0)
    N = p.N
    qs = [(0, 0), (1, 0), (0, 1), (-1, 2), (Lx, Ly)]
    got = dwhmc.debug_current_vertex(p.Lx, p.Ly, p.t, p.tp, p.nn_table, p.nnn_table, a, qs)
    assert got.shape == (len(qs), 2 * N, 2 * N)
    for k, (mx, my) in enumerate(qs):
        J = _jq(p, a, mx, my)
        err = max(np.abs(got[k, :N, :N] - J).max(), np.abs(got[k, N:, N:] - J).max())
        print("vertex", Lx, Ly, a, (mx, my), float(err))
        for blk in (got[k, :N, :N], got[k, N:, N:]):
            _close(blk.real, J.real, (a, mx, my, "re"))
            _close(blk.imag, J.imag, (a, mx, my, "im"))
        assert not got[k, :N, N:].any() and not got[k, N:, :N].any()
    assert np.abs(got).max() > 0.1                          # (Lx = 2, x, q = 0 alone cancels to zero)


SIM_KW = dict(n_therm=3, n_measure=4, Nt_therm_init=2, Nt_measure=12, bin_size=2)
SIM_OPT = dict(direction="y", q=[(0, 1), (1, 0), (-1, 2)], n_matsubara=2)


def _check_sim_outputs(with_opt, without):
    assert not (without / "current_response.csv").exists()
    for f in ("observables.csv", "transport.csv"):
        assert (with_opt / f).read_bytes() == (without / f).read_bytes(), f
    assert sorted(os.listdir(with_opt / "spectra_bins")) == sorted(os.listdir(without / "spectra_bins"))
    lines = (with_opt / "current_response.csv").read_text().splitlines()
    head = lines[0].split(",")
    assert head[:2] == ["sweep", "dia_y"]
    assert head[2:] == [f"lam_yy(mx={mx};my={my};l={l})" for mx, my in SIM_OPT["q"] for l in range(2)]
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == (SIM_KW["n_measure"], 2 + 3 * 2)
    assert np.array_equal(rows[:, 0], np.arange(1, SIM_KW["n_measure"] + 1))
    assert np.all(np.isfinite(rows)) and np.all(rows[:, 1] > 0)
    return rows


@pytest.mark.parametrize("tb", [1, 3])
def test_simulation_option_on_oracle(dwhmc, tmp_path, tb):
    """run_simulation(current_response=...) on the oracle backend: one row per
    transport measurement, through TransportQueue's batches with
    transport_batch; the other files are unchanged; no file without the option."""
    _simulate(dwhmc, tmp_path / "with", _OracleResponse, current_response=SIM_OPT, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", _OracleResponse, transport_batch=tb, **SIM_KW)
    rows = _check_sim_outputs(tmp_path / "with", tmp_path / "without")
    if tb == 1:
        _simulate(dwhmc, tmp_path / "b3", _OracleResponse, current_response=SIM_OPT, transport_batch=3, **SIM_KW)
        assert (tmp_path / "b3" / "current_response.csv").read_bytes() == \
            (tmp_path / "with" / "current_response.csv").read_bytes()
    assert len({tuple(r[1:]) for r in rows}) > 1                      # the sweeps' own Δ, not one state's


@pytest.mark.parametrize("tb", [1, 2])
def test_simulation_chains_option_on_oracle(dwhmc, tmp_path, tb):
    _simulate(dwhmc, tmp_path / "with", _OracleResponse, chains=2, current_response=SIM_OPT, transport_batch=tb,
              **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", _OracleResponse, chains=2, transport_batch=tb, **SIM_KW)
    for k in range(2):
        _check_sim_outputs(tmp_path / "with" / f"c{k}", tmp_path / "without" / f"c{k}")


def test_simulation_option_rejects_unknown_keys(dwhmc, tmp_path):
    with pytest.raises(ValueError):
        _simulate(dwhmc, tmp_path / "a", _OracleResponse, current_response=dict(direction="x", momenta=[(0, 1)]),
                  **SIM_KW)
    with pytest.raises(ValueError):
        _simulate(dwhmc, tmp_path / "b", _OracleResponse, chains=2, current_response=dict(nq=2), **SIM_KW)


# --------------------------------------------------------------------------- GPU
def _measure_both(ctx, **kw):
    return {a: ctx.measure_current_response(direction=a, q=QLIST, n_matsubara=NL, **kw) for a in "xy"}


def _check_parity(got, want, what):
    for a in "xy":
        dia, lam = want[a]
        print(what, a, "dia", got[a]["dia"], dia, "max|Δlam|", float(np.abs(got[a]["lam"] - lam).max()))
        assert got[a]["lam"].shape == (len(QLIST), NL)
        _close(got[a]["dia"], dia, (what, a, "dia"))
        _close(got[a]["lam"], lam, (what, a, "lam"))


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(4, 4), (6, 6), (5, 7), (2, 4)])
def test_parity_with_numpy(dwhmc, oracle, Lx, Ly):
    """2N = 32; 72 and 70 (tails in every tile dimension, odd and unequal
    sides); Lx = 2 (+x and -x neighbours coincide, duplicates summed:
    Λ_xx(q = 0) = 0, Λ_xx(1, 0) is not)."""
    p, dis, D, ref, want = _ref_case(oracle, Lx, Ly)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure_both(ctx)
    ctx.close()
    _check_parity(got, want, (Lx, Ly))
    if Lx == 2:
        assert np.all(np.abs(got["x"]["lam"][0]) <= TOL)
        assert np.all(np.abs(want["x"][1][0]) <= TOL)
        assert want["x"][1][2, 0] > 0.1 and got["x"]["lam"][2, 0] > 0.1


@pytest.mark.gpu
def test_parity_16x16_grouped(dwhmc, oracle, monkeypatch):
    """2N = 512: several product tiles; DWHMC_RESPONSE_GROUP=2 makes the six
    momenta three groups."""
    monkeypatch.setenv("DWHMC_RESPONSE_GROUP", "2")
    p, dis, D, ref, want = _ref_case(oracle, 16, 16)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure_both(ctx)
    monkeypatch.delenv("DWHMC_RESPONSE_GROUP")
    one = ctx.measure_current_response(direction="x", q=QLIST, n_matsubara=NL)      # one group
    ctx.close()
    _check_parity(got, want, "16x16")
    assert one["lam"].tobytes() == got["x"]["lam"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly", [(6, 6), (5, 7)])
def test_consistent_with_measure_transport_and_pm_q(dwhmc, oracle, Lx, Ly):
    """dia - lam[q = 0, l = 0] (x) is measure_transport's stiffness on the same
    context and Δ; lam(q) = lam(-q) from the device."""
    p, dis, D, ref, want = _ref_case(oracle, Lx, Ly)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    tr = ctx.measure_transport(0.01, 0.002, 4.0)
    got = _measure_both(ctx)
    ctx.close()
    _close(got["x"]["dia"] - got["x"]["lam"][0, 0], tr["superfluid_stiffness"], "stiffness")
    for a in "xy":
        lam = got[a]["lam"]
        _close(lam[1], lam[4], (a, "(0,1) vs (0,-1)"))
        _close(lam[2], lam[5], (a, "(1,0) vs (-1,0)"))


@pytest.mark.gpu
@pytest.mark.parametrize("quat", ["0", "1"])
@pytest.mark.parametrize("mu", [-1.0, 0.0])
def test_degenerate_spectra(dwhmc, oracle, monkeypatch, mu, quat):
    """Clean 8 x 8 at μ = -1 and μ = 0 (exact zero modes), both solvers:
    parity, and Λ_xx(mx, my, l) = Λ_yy(my, mx, l), dia_x = dia_y from the device."""
    monkeypatch.setenv("DWHMC_EIG_QUAT", quat)
    key = ("clean", mu)
    if key not in _refs:
        p, dis, D = _clean(oracle, 8, mu)
        ref = _Ref(oracle, p, dis, D)
        _refs[key] = (p, dis, D, ref, {a: (ref.dia(a), ref.lam(a, QLIST, NL)) for a in "xy"})
    p, dis, D, ref, want = _refs[key]
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    got = _measure_both(ctx)
    swapped = ctx.measure_current_response(direction="y", q=[(my, mx) for mx, my in QLIST], n_matsubara=NL)
    ctx.close()
    _check_parity(got, want, key)
    _close(swapped["lam"], got["x"]["lam"], "swap")
    _close(swapped["dia"], got["x"]["dia"], "dia swap")


@pytest.mark.gpu
def test_snapshots_chains_and_state_untouched(dwhmc, oracle):
    """deltas with 3 states equals three single calls; chain 1 of a 2-chain
    context; the context's Δ is unchanged."""
    O = oracle
    p, dis, D, ref, want = _ref_case(O, 6, 6)
    p2, dis2, D2 = _case(O, 6, 6, 8.0, seed=77)
    ref2 = _Ref(O, p2, dis2, D2)
    rng = np.random.default_rng(8)
    fields = np.stack([D2, D2 * np.exp(0.1j), D2 + 0.05 * rng.standard_normal(D2.shape)])
    ctx = _ctx(dwhmc, p, np.stack([dis, dis2]))
    ctx.set_pairing(np.stack([D, D2]))
    before, _ = ctx.get_state()
    kw = dict(direction="y", q=QLIST, n_matsubara=NL, chain=1)
    r3 = ctx.measure_current_response(deltas=fields, **kw)
    ones = [ctx.measure_current_response(deltas=fields[s:s + 1], **kw) for s in range(3)]
    dev1 = ctx.measure_current_response(**kw)                        # the device Δ of chain 1 = fields[0]
    dev0 = ctx.measure_current_response(direction="y", q=QLIST, n_matsubara=NL, chain=0)
    after, _ = ctx.get_state()
    ctx.close()
    assert np.array_equal(before, after)
    assert r3["lam"].shape == (3, len(QLIST), NL) and r3["dia"].shape == (3,)
    for s in range(3):
        assert ones[s]["lam"][0].tobytes() == r3["lam"][s].tobytes(), s
        assert ones[s]["dia"][0] == r3["dia"][s], s
    assert dev1["lam"].tobytes() == r3["lam"][0].tobytes() and dev1["dia"] == r3["dia"][0]
    _close(r3["lam"][0], ref2.lam("y", QLIST, NL), "chain 1")
    _close(r3["dia"][0], ref2.dia("y"), "chain 1 dia")
    _close(r3["lam"][2], _Ref(O, p2, dis2, fields[2]).lam("y", QLIST, NL), "snapshot 2")
    _close(dev0["lam"], want["y"][1], "chain 0")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["dense", "eig"])
def test_other_algorithms(dwhmc, oracle, algo):
    p, dis, D, ref, want = _ref_case(oracle, 4, 4)
    ctx = _ctx(dwhmc, p, dis, algo=algo)
    ctx.set_pairing(D)
    assert ctx.info["algo"] == {"dense": 0, "eig": 2}[algo]
    got = _measure_both(ctx)
    ctx.close()
    _check_parity(got, want, algo)


@pytest.mark.gpu
def test_argument_errors(dwhmc, oracle):
    p, dis, D, ref, want = _ref_case(oracle, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    lib, h = ctx._lib, ctx._h
    dia, lam = np.zeros(1), np.zeros(8)
    q = np.array([[0, 1]], dtype=np.int64)
    pd, pl, pq = (a.ctypes.data_as(C.c_void_p) for a in (dia, lam, q))

    def call(direction=0, nq=1, qp=pq, nl=1, d=pd, l=pl, ns=1):
        return lib.dwh_measure_current_response(h, 0, ns, None, direction, nq, qp, nl, d, l)

    try:
        bad_q = np.array([[p.Lx + 1, 0]], dtype=np.int64)
        bad_q2 = np.array([[0, -p.Ly - 1]], dtype=np.int64)
        for kw in (dict(direction=2), dict(direction=-1), dict(nq=0), dict(nl=0), dict(qp=None), dict(l=None),
                   dict(d=None), dict(qp=bad_q.ctypes.data_as(C.c_void_p)),
                   dict(qp=bad_q2.ctypes.data_as(C.c_void_p)), dict(ns=2), dict(ns=0)):
            assert call(**kw) == -1, kw
            assert lib.dwh_last_error(h), kw
        for kw in (dict(direction="z"), dict(q=[]), dict(n_matsubara=0), dict(q=[(p.Lx + 1, 0)]), dict(chain=1)):
            with pytest.raises(ValueError):
                ctx.measure_current_response(**kw)
        # |m| = L is allowed, and the context still measures after the refusals
        r = ctx.measure_current_response(direction="x", q=[(p.Lx, -p.Ly)] + QLIST, n_matsubara=NL)
        _close(r["lam"][1:], want["x"][1], "after errors")
        assert np.all(np.isfinite(r["lam"][0]))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_timer(dwhmc, oracle):
    p, dis, D, ref, want = _ref_case(oracle, 4, 4)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    ctx.timing_enable(["response"])
    ctx.measure_current_response(direction="x", q=QLIST, n_matsubara=NL)
    ctx.measure_current_response(direction="y", q=QLIST[:2], n_matsubara=1, deltas=np.stack([D, D, D]))
    ms, launches, work = ctx.timing_read("response")
    ctx.close()
    assert launches > 0 and ms > 0
    assert work == 8.0 * (2 * p.N) ** 3 * (len(QLIST) * 1 + 2 * 3)
