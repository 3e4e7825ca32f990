"""Selectable HMC integrators on the device (dwh_set_integrator): the context's
splitting schedule through every entry point that runs a trajectory, against a
numpy integrator written here from the oracle's update_H_BdG,
diagonalize_H_BdG, compute_forces and compute_total_energy.

One step of size dt: kick a_0·dt, then for s = 1..S drift b_s·dt, force
evaluation, kick a_s·dt (kick π += c·F, drift Δ += c/(2m)·π); steps are
concatenated with the adjacent end and start kicks merged into (a_S + a_0)·dt.

Tolerances of the parity tests are test_hmc_sweep_matches_oracle's
(tests/test_gpu_parity.py): |ΔdH| ≤ 1e-8 (1 + |dH|), Δ ≤ 1e-10, π ≤ 1e-9, the
accept flag equal.  Where two device runs are compared the comparison is bit
for bit.
"""
import math
from importlib import import_module

import numpy as np
import pytest

from test_gpu_parity import algo3, device_ctx, make_case  # noqa: F401  (algo3 is a fixture)

pytestmark = pytest.mark.gpu

LAM = 0.1931833275037836
OM2 = ([LAM, 1.0 - 2.0 * LAM, LAM], [0.5, 0.5])
LEAP = ([0.5, 0.5], [1.0])
CUSTOM3 = ([0.15, 0.35, 0.35, 0.15], [0.3, 0.4, 0.3])      # S = 3, palindromic, Σa = Σb = 1
ERR_STATE = -3


def flat_schedule(a, b, Nt, dt, mass):
    """The trajectory's kicks (S·Nt + 1) and drifts (S·Nt) by the definition above."""
    S = len(b)
    kicks, drifts = [a[0] * dt], []
    for step in range(Nt):
        for s in range(1, S + 1):
            drifts.append((b[s - 1] * dt) / (2.0 * mass))
            kicks.append((a[S] + a[0]) * dt if s == S and step < Nt - 1 else a[s] * dt)
    return kicks, drifts


class NumpyChain:
    """One chain on the oracle's functions: trajectory(noise, ...) integrates
    from the current Δ and returns ΔH; the Metropolis decision is the caller's."""

    def __init__(self, O, p, dis, Delta0):
        self.O, self.p = O, p
        self.cache = O.initialize_cache(p)
        O.init_static_H(self.cache, p, dis)
        self.Delta = np.array(Delta0, dtype=np.complex128)
        self.pi = np.zeros_like(self.Delta)
        O.update_H_BdG(self.cache, p, self.Delta)
        O.diagonalize_H_BdG(self.cache, p)

    def trajectory(self, noise, a, b, Nt, dt, keep=True):
        O, p, c = self.O, self.p, self.cache
        D0, E0, U0 = self.Delta.copy(), c.E_n.copy(), c.U.copy()
        self.pi = noise * math.sqrt(2 * p.mass)
        H_old = O.compute_total_energy(c, p, self.Delta, self.pi)
        kicks, drifts = flat_schedule(a, b, Nt, dt, p.mass)
        O.compute_forces(c, p, self.Delta)
        self.pi = self.pi + kicks[0] * c.forces
        for i, drift in enumerate(drifts):
            self.Delta = self.Delta + drift * self.pi
            O.update_H_BdG(c, p, self.Delta)
            O.diagonalize_H_BdG(c, p)
            O.compute_forces(c, p, self.Delta)
            self.pi = self.pi + kicks[i + 1] * c.forces
        dH = O.compute_total_energy(c, p, self.Delta, self.pi) - H_old
        if not keep:
            self.restore(D0, E0, U0)
        return dH

    def restore(self, D0, E0, U0):
        self.Delta = D0
        self.cache.E_n[:] = E0
        self.cache.U[:, :] = U0
        self.O.update_H_BdG(self.cache, self.p, self.Delta)

    def sweep(self, noise, u, a, b, Nt, dt):
        D0, E0, U0 = self.Delta.copy(), self.cache.E_n.copy(), self.cache.U.copy()
        dH = self.trajectory(noise, a, b, Nt, dt)
        acc = bool(dH < 0 or u < math.exp(-dH))
        if not acc:
            self.restore(D0, E0, U0)
        return acc, dH


def cnoise(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)


def set_scheme(ctx, name):
    if name == "om2":
        ctx.set_integrator("omelyan2")
        return OM2
    if name == "custom3":
        ctx.set_integrator("custom", kick=CUSTOM3[0], drift=CUSTOM3[1])
        return CUSTOM3
    ctx.set_integrator("leapfrog")
    return LEAP


# -- 1. oracle parity -------------------------------------------------------
@pytest.mark.parametrize("Lx,Ly", [(6, 6), (3, 2)])
@pytest.mark.parametrize("scheme,Nt", [("om2", 2), ("om2", 3), ("custom3", 2)])
def test_sweeps_match_numpy_integrator(dwhmc, oracle, algo3, scheme, Nt, Lx, Ly):
    """3x2 maps several bonds onto one pairing entry (the reference's overwrite
    order, src/Hamiltonian.jl:68-83) inside the trajectories."""
    O = oracle
    p, dis, Delta0 = make_case(O, Lx, Ly, 4.0, seed=77 + Lx, amp=0.1)
    dt = O.calc_optimal_dt(p.beta, p.J, p.mass, Nt)
    rng = np.random.default_rng(5)
    draws = [(cnoise(rng, (p.N, 2)), float(rng.random())) for _ in range(3)]
    ctx = device_ctx(dwhmc, p, dis, algo3)
    a, b = set_scheme(ctx, scheme)
    ctx.set_pairing(Delta0)
    ctx.factorize()
    ref = NumpyChain(O, p, dis, Delta0)
    for noise, u in draws:
        acc_r, dH_r = ref.sweep(noise, u, a, b, Nt, dt)
        acc, dH = ctx.hmc_sweep(noise, np.array([u]), Nt, dt, p.mass)
        D, pi = ctx.get_state()
        assert abs(dH[0] - dH_r) <= 1e-8 * (1 + abs(dH_r)), (dH[0], dH_r)
        assert bool(acc[0]) == acc_r
        assert np.max(np.abs(D[0] - ref.Delta)) <= 1e-10
        assert np.max(np.abs(pi[0] - ref.pi)) <= 1e-9
    ctx.close()


# -- 2. the default path is unchanged -----------------------------------------
def test_default_explicit_and_custom_leapfrog_agree_bitwise(dwhmc, oracle, algo3):
    O = oracle
    p, dis, Delta0 = make_case(O, 6, 6, 4.0, seed=83, amp=0.1)
    Nt = 4
    dt = O.calc_optimal_dt(p.beta, p.J, p.mass, Nt)
    rng = np.random.default_rng(6)
    draws = [(cnoise(rng, (p.N, 2)), rng.random(1)) for _ in range(3)]

    def run(prepare):
        ctx = device_ctx(dwhmc, p, dis, algo3)
        prepare(ctx)
        ctx.set_pairing(Delta0)
        ctx.factorize()
        out = []
        for noise, u in draws:
            acc, dH = ctx.hmc_sweep(noise, u, Nt, dt, p.mass)
            out.append((acc.copy(), dH.copy(), *ctx.get_state()))
        ctx.close()
        return out

    def detour(ctx):
        ctx.set_integrator("omelyan2")
        assert ctx.integrator["kind"] == "omelyan2"
        ctx.set_integrator("custom", kick=[0.5, 0.5], drift=[1.0])

    default = run(lambda ctx: None)
    for other in (run(lambda ctx: ctx.set_integrator("leapfrog")), run(detour)):
        for x, y in zip(default, other):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
    # and the default is the oracle's leapfrog
    st = O.SimulationState(dis, Delta0.copy(), np.zeros_like(Delta0))
    cache = O.initialize_cache(p)
    O.init_static_H(cache, p, dis)
    O.update_H_BdG(cache, p, st.Delta)
    O.diagonalize_H_BdG(cache, p)
    for (noise, u), (acc, dH, D, _) in zip(draws, default):
        acc_r, dH_r = O.hmc_sweep(cache, p, st, Nt, dt, noise, float(u[0]))
        assert bool(acc[0]) == acc_r and abs(dH[0] - dH_r) <= 1e-8 * (1 + abs(dH_r))
        assert np.max(np.abs(D[0] - st.Delta)) <= 1e-10


# -- 3. / 4. order of accuracy and energy conservation ------------------------
def _cold_start(O, Lx=6, Ly=6, seed=3):
    """oracle.initialize_state: the unthermalised small-Δ start"""
    p = O.ModelParameters(Lx, Ly, 1.0, -0.35, -1.08, 1.0, 0.05, 4.0, 0.8, 1.0)
    rng = np.random.default_rng(seed)
    st = O.initialize_state(p, rng)
    return p, st.disorder_pot, st.Delta, rng


def _device_dH(ctx, p, noise, Nt, O):
    """ΔH of one trajectory of length T/2 from the context's Δ, which it keeps"""
    dH = ctx.hmc_trajectory(noise, Nt, O.calc_optimal_dt(p.beta, p.J, p.mass, Nt), p.mass)[0]
    ctx.hmc_finish([0])
    return float(dH)


def test_omelyan2_is_second_order(dwhmc, oracle):
    """Halving dt at fixed trajectory length divides ΔH by 4: the ratio
    ΔH(Nt=16)/ΔH(Nt=32) lies in [3.5, 4.5], first for the numpy integrator
    here, then for the device."""
    O = oracle
    p, dis, Delta0, rng = _cold_start(O)
    noise = cnoise(rng, (p.N, 2))
    ref = NumpyChain(O, p, dis, Delta0)
    r = [ref.trajectory(noise, *OM2, Nt, O.calc_optimal_dt(p.beta, p.J, p.mass, Nt), keep=False) for Nt in (16, 32)]
    print(f"numpy  dH(16)={r[0]:.6e} dH(32)={r[1]:.6e} ratio={r[0] / r[1]:.4f}")
    assert 3.5 <= r[0] / r[1] <= 4.5, r
    ctx = device_ctx(dwhmc, p, dis)
    ctx.set_integrator("omelyan2")
    ctx.set_pairing(Delta0)
    ctx.factorize()
    d = [_device_dH(ctx, p, noise, Nt, O) for Nt in (16, 32)]
    print(f"device dH(16)={d[0]:.6e} dH(32)={d[1]:.6e} ratio={d[0] / d[1]:.4f}")
    ctx.close()
    assert 3.5 <= d[0] / d[1] <= 4.5, d


def test_omelyan2_four_factorisations_beat_leapfrog_four(dwhmc, oracle):
    """rms ΔH over 8 draws from the same start: om2 at Nt=2 below leapfrog at
    Nt=4, the same four factorisations (CPU: 0.029 against 2.06 on 6x6)."""
    O = oracle
    p, dis, Delta0, rng = _cold_start(O)
    noises = [cnoise(rng, (p.N, 2)) for _ in range(8)]
    ctx = device_ctx(dwhmc, p, dis)
    ctx.timing_enable(["step"])
    ctx.set_pairing(Delta0)
    ctx.factorize()
    rms = {}
    for name, Nt in (("leapfrog", 4), ("om2", 2)):
        set_scheme(ctx, name)
        ctx.timing_reset()
        dH = np.array([_device_dH(ctx, p, nz, Nt, O) for nz in noises])
        assert ctx.timing_read("step")[1] == 4 * len(noises)
        rms[name] = float(np.sqrt(np.mean(dH ** 2)))
    ctx.close()
    print(f"rms dH: leapfrog Nt=4 {rms['leapfrog']:.4e}, om2 Nt=2 {rms['om2']:.4e}")
    assert rms["om2"] < rms["leapfrog"], rms


# -- 5. reversibility ---------------------------------------------------------
def test_reversible(dwhmc, oracle, algo3):
    """A trajectory, then one from its end with the momenta reversed (noise =
    -π_final / sqrt(2m)) returns the starting Δ.  Allowed: 10 x the error the
    leapfrog path shows here with the same four factorisations (the margin
    covers the different rounding of the λ coefficients)."""
    O = oracle
    p, dis, Delta0 = make_case(O, 6, 6, 4.0, seed=91, amp=0.1)
    noise = cnoise(np.random.default_rng(8), (p.N, 2))
    ctx = device_ctx(dwhmc, p, dis, algo3)
    err = {}
    for name, Nt in (("leapfrog", 4), ("om2", 2)):
        set_scheme(ctx, name)
        dt = O.calc_optimal_dt(p.beta, p.J, p.mass, Nt)
        ctx.set_state(Delta0, None)
        ctx.factorize()
        ctx.hmc_trajectory(noise, Nt, dt, p.mass)
        ctx.hmc_finish([1])
        D1, pi1 = ctx.get_state()
        assert np.max(np.abs(D1[0] - Delta0)) > 1e-3            # it moved
        ctx.hmc_trajectory(-pi1[0] / math.sqrt(2 * p.mass), Nt, dt, p.mass)
        ctx.hmc_finish([1])
        err[name] = float(np.max(np.abs(ctx.get_state()[0][0] - Delta0)))
    ctx.close()
    print(f"return error: leapfrog Nt=4 {err['leapfrog']:.3e}, om2 Nt=2 {err['om2']:.3e}")
    assert err["om2"] <= 10 * err["leapfrog"], err


# -- 6. throughput path -------------------------------------------------------
def test_run_sweeps_equals_single_sweeps(dwhmc, oracle, algo3):
    O = oracle
    p, dis, Delta0 = make_case(O, 6, 6, 4.0, seed=9, amp=0.1)
    Nt, ns = 2, 3
    dt = O.calc_optimal_dt(p.beta, p.J, p.mass, Nt)
    rng = np.random.default_rng(11)
    noise = cnoise(rng, (ns, 2, p.N, 2))
    uni = rng.random((ns, 2))
    dis2 = np.stack([dis, dis[::-1].copy()])
    D2 = np.stack([Delta0, Delta0[::-1].copy()])

    def fresh(scheme):
        ctx = device_ctx(dwhmc, p, dis2, algo3)
        set_scheme(ctx, scheme)
        ctx.set_pairing(D2)
        ctx.factorize()
        return ctx

    single = {}
    for scheme in ("om2", "leapfrog"):
        a = fresh(scheme)
        single[scheme] = ([a.hmc_sweep(noise[s], uni[s], Nt, dt, p.mass) for s in range(ns)], a.get_state())
        a.close()
    assert not np.array_equal(single["om2"][1][0], single["leapfrog"][1][0])

    def same(ctx, scheme):
        acc, dH = ctx.sweep_results(0, ns)
        res, state = single[scheme]
        for s in range(ns):
            assert np.array_equal(acc[s], res[s][0]) and np.array_equal(dH[s], res[s][1]), (scheme, s)
        for x, y in zip(ctx.get_state(), state):
            assert np.array_equal(x, y)

    b = fresh("om2")
    b.load_draws(noise, uni)
    b.run_sweeps(0, ns, Nt, dt, p.mass)
    same(b, "om2")
    b.close()
    # set_integrator with sweeps pending: they finish under the schedule they
    # were enqueued with, the next batch runs the new one
    c = fresh("leapfrog")
    c.load_draws(noise, uni)
    c.run_sweeps(0, ns, Nt, dt, p.mass)
    c.set_integrator("omelyan2")
    same(c, "leapfrog")
    c.set_pairing(D2)
    c.factorize()
    c.run_sweeps(0, ns, Nt, dt, p.mass)
    same(c, "om2")
    with pytest.raises(ValueError):
        c.run_sweeps(0, ns, 0, dt, p.mass)          # Nt = 0 is leapfrog's alone
    c.close()


@pytest.mark.parametrize("algo_g,Lx,Ly", [("cr", 20, 4), ("cr", 12, 5), ("dense", 6, 6)])
def test_guard_trip_replays_the_schedule(dwhmc, oracle, algo_g, Lx, Ly):
    """test_guard_trip_recovers_in_throughput_path's shapes under om2: sweep 2
    of 5 trips the guard in chain 1, dwh_sweep_results re-selects the poles
    and replays sweeps 2..4 with the context's schedule, which the new device
    side keeps; bit for bit the single-sweep path.  A set_integrator between
    run_sweeps and the results does not reach the replay."""
    O = oracle
    p, dis, Delta0 = make_case(O, Lx, Ly, 4.0, seed=24 + Lx, amp=0.0)
    ns, Nt, dt = 5, 2, 0.2
    rng = np.random.default_rng(25)
    noise = cnoise(rng, (ns, 2, p.N, 2))
    scale = np.full((ns, 2), 0.05)
    scale[2, 1] = 8.0                                  # the trip: sweep 2, chain 1
    noise *= scale[:, :, None, None]
    uni = rng.random((ns, 2))
    dis2 = np.stack([dis, dis[::-1].copy()])
    D2 = np.stack([Delta0, Delta0[::-1].copy()])
    cap0 = 0.2

    def fresh():
        ctx = device_ctx(dwhmc, p, dis2, algo_g, delta_cap=cap0)
        ctx.set_integrator("omelyan2")
        ctx.set_pairing(D2)
        ctx.factorize()
        return ctx

    a = fresh()
    ref = []
    for s in range(ns):
        ref.append(a.hmc_sweep(noise[s], uni[s], Nt, dt, p.mass))
        if s == 1:
            assert a.info["delta_cap"] == cap0          # no trip before sweep 2
    assert a.info["delta_cap"] > cap0                   # sweep 2 tripped
    assert a.integrator["kind"] == "omelyan2"           # and the setting outlived the re-selection
    for switch in (False, True):
        b = fresh()
        b.load_draws(noise, uni)
        b.run_sweeps(0, ns, Nt, dt, p.mass)
        if switch:
            b.set_integrator("leapfrog")
        acc, dH = b.sweep_results(0, ns)
        for s in range(ns):
            assert np.array_equal(acc[s], ref[s][0]), s
            assert np.array_equal(dH[s], ref[s][1]), s
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
        assert b.info["delta_cap"] == a.info["delta_cap"]
        assert b.integrator["kind"] == ("leapfrog" if switch else "omelyan2")
        b.close()
    a.close()


# -- 7. state and timers ------------------------------------------------------
def test_state_timers_and_round_trip(dwhmc, oracle):
    O = oracle
    p, dis, Delta0 = make_case(O, 6, 6, 4.0, seed=13, amp=0.1)
    noise = cnoise(np.random.default_rng(14), (p.N, 2))
    binding = import_module(dwhmc.__name__ + "._lib")
    ctx = device_ctx(dwhmc, p, dis)
    g = ctx.integrator
    assert g["kind"] == "leapfrog" and g["kick"].tolist() == [0.5, 0.5] and g["drift"].tolist() == [1.0]
    ctx.set_integrator("custom", kick=CUSTOM3[0], drift=CUSTOM3[1])
    g = ctx.integrator
    assert g["kind"] == "custom" and g["kick"].tolist() == CUSTOM3[0] and g["drift"].tolist() == CUSTOM3[1]
    with pytest.raises(ValueError):
        ctx.set_integrator("custom", kick=[0.2, 0.5, 0.3], drift=[0.5, 0.5])
    assert ctx.integrator["kick"].tolist() == CUSTOM3[0]        # a refused schedule changes nothing
    ctx.set_integrator("omelyan2", lam=0.2)
    g = ctx.integrator
    assert g["kind"] == "omelyan2" and g["lam"] == 0.2 and g["kick"].tolist() == [0.2, 1.0 - 2.0 * 0.2, 0.2]
    # every pointer of dwh_get_integrator is nullable
    assert ctx._lib.dwh_get_integrator(ctx._h, None, None, None, None, None) == 0

    ctx.set_pairing(Delta0)
    ctx.factorize()
    ctx.timing_enable(["step"])
    for scheme, S in (("om2", 2), ("custom3", 3), ("leapfrog", 1)):
        set_scheme(ctx, scheme)
        for Nt in (1, 3):
            ctx.timing_reset()
            ctx.hmc_trajectory(noise, Nt, 0.05, p.mass)
            # between trajectory and finish the integrator cannot change
            rc = ctx._lib.dwh_set_integrator(ctx._h, 0, 0.0, 0, None, None)
            assert rc == ERR_STATE == binding.DWH_ERR_STATE
            ctx.hmc_finish([0])
            assert ctx.timing_read("step")[1] == S * Nt, (scheme, Nt)
    assert ctx._lib.dwh_set_integrator(ctx._h, 1, LAM, 0, None, None) == 0
    with pytest.raises(ValueError):
        ctx.hmc_trajectory(noise, 0, 0.05, p.mass)               # Nt = 0 is leapfrog's alone
    with pytest.raises(ValueError):
        ctx.hmc_sweep(noise, np.array([0.5]), 0, 0.05, p.mass)
    ctx.set_integrator("leapfrog")
    ctx.hmc_sweep(noise, np.array([0.5]), 0, 0.05, p.mass)
    ctx.close()


# -- 8. the driver --------------------------------------------------------------
def test_run_simulation_with_integrator(dwhmc, tmp_path):
    sim = import_module(dwhmc.__name__ + ".simulation")
    p = dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)
    kw = dict(n_therm=10, n_measure=4, Nt_therm_init=2, Nt_measure=2, measure_transport_freq=0, verbose=False)

    def run(name, **extra):
        res = sim.run_simulation(p, str(tmp_path / name), rng=np.random.default_rng(5), **kw, **extra)
        return res, (tmp_path / name / "observables.csv").read_bytes(), (tmp_path / name / "simulation.log").read_text()

    res, csv, log = run("om2", integrator=dict(kind="omelyan2", Nt_min=1))
    assert len(csv.splitlines()) == 5 and len(res.records) == 4
    assert "Integrator: omelyan2 lam=0.1931833275037836, 2 factorisations per step" in log
    assert "Nt_min=1" in log and "Factorisations per trajectory: 4" in log
    assert 1 <= res.Nt_final
    _, csv_plain, log_plain = run("plain")
    _, csv_none, log_none = run("none", integrator=None)
    assert csv_plain == csv_none
    assert "Integrator" not in log_none and "Factorisations" not in log_none
    assert csv != csv_plain
    _, csv_leap, _ = run("leap", integrator="leapfrog")
    assert csv_leap == csv_plain                                 # the explicit default, the same Markov chain
    with pytest.raises(ValueError):
        run("bad", integrator=dict(kind="omelyan2", lam=0.5))
    assert not (tmp_path / "bad").exists()                       # refused before any file is opened


def test_hmc_sweep_and_replicas_pass_the_setting(dwhmc, oracle):
    """hmc.hmc_sweep(integrator=) and ReplicaConfig.integrator reach the context."""
    rep = import_module(dwhmc.__name__ + ".replicas")
    p = dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)
    st = dwhmc.initialize_state(p, np.random.default_rng(1))
    cache = dwhmc.initialize_cache(p)
    dwhmc.init_static_H(cache, p, st)
    dwhmc.update_H_BdG(cache, p, st)
    dwhmc.diagonalize_H_BdG(cache, p)
    noise = cnoise(np.random.default_rng(2), (p.N, 2))
    D0 = st.Delta.copy()
    acc, dH = dwhmc.hmc_sweep(cache, p, st, Nt=2, dt=0.1, noise=noise, uniform=0.5, integrator=dict(kind="omelyan2"))
    assert cache.ctx.integrator["kind"] == "omelyan2"
    ref = NumpyChain(oracle, oracle.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0),
                     st.disorder_pot, D0)
    acc_r, dH_r = ref.sweep(noise, 0.5, *OM2, 2, 0.1)
    assert acc == acc_r and abs(dH - dH_r) <= 1e-8 * (1 + abs(dH_r))
    cache.ctx.close()

    def make_context(disorder):
        return dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, disorder)

    out = {}
    for kind in (None, "leapfrog", "omelyan2"):
        cfg = rep.ReplicaConfig(chains=1, n_sweeps=2, Nt=2, integrator=None if kind is None else dict(kind=kind))
        out[kind] = rep.run_local(p, cfg, 0, 0, make_context, dwhmc.initialize_state, dwhmc.calc_optimal_dt)
    assert np.array_equal(out[None], out["leapfrog"])
    assert not np.array_equal(out[None][:, :, 1], out["omelyan2"][:, :, 1])      # ΔH of another integrator
