"""The sparse level-0 stages read host-resolved row records (csrc/dwhmc_plan.cpp
cr_sparse_task_arrays -> k_cr_sp_fwd / k_cr_sp_bwd): per (task, output row)
the hopping slots with their static values and dense-row offsets, then the one
pairing slot (Δ index, ±1/2, the stored row behind the synthesised one).  The
GPU tests run the CR path with DWHMC_CR_SPARSE0=1 against the eigen oracle at
the tolerances of tests/test_gpu_parity.py::test_cr_sparse_level0:
  P <= 1e-11, F <= 1e-10 (1 + ‖F‖∞), E_f <= 1e-11 relative, hole density <= 1e-11,
on the smallest lattices (Ly = 4: the smallest sparse level 0) that reach each
part of the records: empty hopping slots and padded rows (t' = 0, Lx = 20 in
BP = 64), per-chain Δ and the x ± 1 wrap at an exactly filled block (Lx = 32,
two chains), two column groups per lane (Lx = 40, BP = 96), BP = 32 forced
sparse (Lx = 16), a pairing slot holding an exact zero, and the Δ the force
kernel scatters during a sweep."""
import ctypes as C
import math

import numpy as np
import pytest

T, TP, MU, J = 1.0, -0.35, -1.08, 0.8


def make_case(O, Lx, Ly, beta, seed, tp=TP):
    p = O.ModelParameters(Lx, Ly, T, tp, MU, 1.0, 0.05, beta, J, 1.0)
    rng = np.random.default_rng(seed)
    st = O.initialize_state(p, rng)
    N = p.N
    dwave = np.stack([np.ones(N), -np.ones(N)], axis=1) * 0.3
    Delta = st.Delta + dwave * (1 + 0.3 * rng.standard_normal((N, 1))) * np.exp(1j * 0.2 * rng.standard_normal((N, 1)))
    return p, st.disorder_pot, Delta


def cr_ctx(dwhmc, p, disorder):
    ctx = dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, disorder, algo="cr")
    assert ctx.info["algo"] == 1
    return ctx


def check_chain(O, ctx, c, p, dis, Delta):
    cache, F_ref, Ef_ref = O.evaluate(p, dis, Delta)
    P_ref, _ = O.pairing_P(cache.U, cache.E_n, p)
    assert np.max(np.abs(ctx.pairing()[c] - P_ref)) <= 1e-11
    assert np.max(np.abs(ctx.forces()[c] - F_ref)) <= 1e-10 * (1 + np.max(np.abs(F_ref)))
    assert abs(ctx.fermion_energy()[c] - Ef_ref) <= 1e-11 * abs(Ef_ref)
    hole_ref = O.measure_observables(cache, p, Delta)["hole_conc"]
    assert abs(2.0 * ctx.hole_trace()[c] / p.N - 1.0 - hole_ref) <= 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly,beta,tp,zero_bonds", [
    (20, 4, 16.0, 0.0, False),    # one hopping + one pairing entry per row: empty hopping slots; padded BP = 64
    (40, 4, 8.0, TP, False),      # BP = 96: two column groups per lane, the 2-wave budget
    (16, 4, 8.0, TP, False),      # BP = 32, sparse only when forced
    (20, 4, 16.0, TP, True),      # a pairing slot holding a true zero, not an empty one
])
def test_records_factorize(dwhmc, oracle, monkeypatch, Lx, Ly, beta, tp, zero_bonds):
    O = oracle
    monkeypatch.setenv("DWHMC_CR_SPARSE0", "1")
    p, dis, Delta = make_case(O, Lx, Ly, beta, seed=Lx * 31 + Ly, tp=tp)
    if zero_bonds:
        # vertical (+y) bonds: column 1 of Δ; one in the first block row, one
        # across the periodic edge, one in the middle
        for i in (3, p.N - 2, Lx + 7):
            Delta[i, 1] = 0.0
    ctx = cr_ctx(dwhmc, p, dis)
    ctx.set_pairing(Delta)
    ctx.factorize()
    check_chain(O, ctx, 0, p, dis, Delta)
    ctx.close()


@pytest.mark.gpu
def test_records_two_chains_full_block(dwhmc, oracle, monkeypatch):
    """Lx = 32 fills BP = 64 exactly (x ± 1 wraps across the block edge); the
    two chains differ in disorder and in Δ, so a pairing slot that indexed the
    wrong chain's Δ shows in either."""
    O = oracle
    monkeypatch.setenv("DWHMC_CR_SPARSE0", "1")
    cases = [make_case(O, 32, 4, 16.0, seed=s) for s in (41, 42)]
    p = cases[0][0]
    ctx = cr_ctx(dwhmc, p, np.stack([c[1] for c in cases]))
    ctx.set_pairing(np.stack([c[2] for c in cases]))
    ctx.factorize()
    for c, (pc, dc, Dc) in enumerate(cases):
        check_chain(O, ctx, c, pc, dc, Dc)
    ctx.close()


@pytest.mark.gpu
def test_records_follow_drifted_delta(dwhmc, oracle, monkeypatch):
    """One 3-step HMC sweep: the Δ the force kernel drifts and scatters is the
    Δ the pairing slots index (sweep tolerances of tests/test_gpu_parity.py:
    |ΔdH| <= 1e-8 (1 + |dH|), Δ <= 1e-10, equal accept flag)."""
    O = oracle
    monkeypatch.setenv("DWHMC_CR_SPARSE0", "1")
    p, dis, Delta = make_case(O, 20, 4, 16.0, seed=77)
    Nt = 3
    dt = O.calc_optimal_dt(p.beta, p.J, p.mass, Nt)
    rng = np.random.default_rng(5)
    noise = (rng.standard_normal((p.N, 2)) + 1j * rng.standard_normal((p.N, 2))) * math.sqrt(0.5)
    u = float(rng.random())
    # the oracle's sweep from the same state and draws
    cache = O.initialize_cache(p)
    O.init_static_H(cache, p, dis)
    st = O.SimulationState(dis, Delta.copy(), np.zeros_like(Delta))
    O.update_H_BdG(cache, p, st.Delta)
    O.diagonalize_H_BdG(cache, p)
    acc_r, dH_r = O.hmc_sweep(cache, p, st, Nt, dt, noise, u)
    ctx = cr_ctx(dwhmc, p, dis)
    ctx.set_pairing(Delta)
    ctx.factorize()
    acc, dH = ctx.hmc_sweep(noise, np.array([u]), Nt, dt, p.mass)
    assert bool(acc[0]) == acc_r
    assert abs(dH[0] - dH_r) <= 1e-8 * (1 + abs(dH_r))
    assert np.max(np.abs(ctx.get_state()[0][0] - st.Delta)) <= 1e-10
    ctx.close()


def test_plan_shape_with_records(dwhmc, monkeypatch):
    """The records change what the sparse stages read, not the plan: with the
    sparse level 0 on, C3 is still 25 launches — 6 inversions, 4 with side
    work, 19 product launches (tests/test_cr_plan_dataflow.py)."""
    lib = dwhmc.load_library()
    monkeypatch.setenv("DWHMC_CR_SPARSE0", "1")
    monkeypatch.delenv("DWHMC_CR_MERGE", raising=False)
    stats = np.zeros(6, dtype=np.int64)
    rc = lib.dwh_debug_cr_plan_check(32, 32, 14, 1, 1, stats.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.dwh_last_error(None).decode()
    assert list(stats[:4]) == [25, 6, 4, 19]
