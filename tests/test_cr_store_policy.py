"""The cache policy of the CR launches' pool stores (st16, csrc/dwhmc_device.h;
chosen per stage by the plan, csrc/dwhmc_plan.cpp cr_store_policies).

A store policy changes where a line lives after the store, never a bit of
what is stored: the GPU tests compare a context created with
DWHMC_CR_STORE=0 (plain stores everywhere, the switch is read at context
creation) against the default one, in one process, with exact equality, on
the smallest lattices that reach every store site that takes a policy; one
more checks the default against the eigen oracle.  The host-only test checks
that the plan gives each stage the policy DESIGN.md §4 ("Store policy")
states."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_parity import device_ctx, make_case

# Lx, Ly, beta, chains -> what it reaches
CASES = [
    (20, 6, 8.0, 1),    # BP = 64: sparse level 0 forward and backward, k_cr_inv0, k_cr_inv<4>, both gemm16 K splits
    (20, 11, 8.0, 1),   # BP = 64, odd chain: the side-work schedule (k_cr_inv_side)
    (36, 4, 16.0, 1),   # BP = 96: k_cr_inv0_96
    (8, 8, 8.0, 1),     # BP = 32: dense level 0, k_cr_inv0_32 / k_cr_inv32
    (20, 6, 8.0, 2),    # nbatch = 2 x poles
]
NT, NSWEEPS = 3, 2


def _case(O, Lx, Ly, beta, chains):
    p, dis, Delta = make_case(O, Lx, Ly, beta, seed=Lx * 100 + Ly, amp=0.1)
    if chains == 1:
        return p, dis, Delta
    return p, np.stack([dis, dis[::-1].copy()]), np.stack([Delta, Delta[::-1].copy()])


def _run(dwhmc, O, monkeypatch, store, p, dis, Delta, chains):
    """Everything the tests compare, from a context created with DWHMC_CR_STORE=store (None: unset)."""
    if store is None:
        monkeypatch.delenv("DWHMC_CR_STORE", raising=False)
    else:
        monkeypatch.setenv("DWHMC_CR_STORE", store)
    ctx = device_ctx(dwhmc, p, dis, "cr")
    ctx.set_pairing(Delta)
    ctx.factorize()
    out = {"pairing": ctx.pairing().copy(), "forces": ctx.forces().copy(),
           "fermion_energy": np.array(ctx.fermion_energy()), "hole_trace": np.array(ctx.hole_trace())}
    rng = np.random.default_rng(5)
    shape = (NSWEEPS, chains, p.N, 2)
    noise = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)
    ctx.load_draws(noise, rng.random((NSWEEPS, chains)))
    ctx.run_sweeps(0, NSWEEPS, NT, O.calc_optimal_dt(p.beta, p.J, p.mass, NT), p.mass)
    D, pi = ctx.get_state()
    acc, dH = ctx.sweep_results(0, NSWEEPS)
    out.update(Delta=D.copy(), pi=pi.copy(), accepted=np.array(acc), dH=np.array(dH))
    ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly,beta,chains", CASES)
def test_store_policy_changes_no_bit(dwhmc, oracle, monkeypatch, Lx, Ly, beta, chains):
    p, dis, Delta = _case(oracle, Lx, Ly, beta, chains)
    plain = _run(dwhmc, oracle, monkeypatch, "0", p, dis, Delta, chains)
    default = _run(dwhmc, oracle, monkeypatch, None, p, dis, Delta, chains)
    for k in plain:
        assert np.array_equal(plain[k], default[k]), k


@pytest.mark.gpu
def test_default_policy_matches_oracle(dwhmc, oracle, monkeypatch):
    """The default policy at 20 x 6 against the eigen oracle, at the tolerances of test_cr_ragged_chains."""
    O = oracle
    monkeypatch.delenv("DWHMC_CR_STORE", raising=False)
    p, dis, Delta = make_case(O, 20, 6, 8.0, seed=20 * 31 + 6)
    cache, F_ref, Ef_ref = O.evaluate(p, dis, Delta)
    P_ref, _ = O.pairing_P(cache.U, cache.E_n, p)
    ctx = device_ctx(dwhmc, p, dis, "cr")
    ctx.set_pairing(Delta)
    ctx.factorize()
    assert np.max(np.abs(ctx.pairing()[0] - P_ref)) <= 1e-11
    assert np.max(np.abs(ctx.forces()[0] - F_ref)) <= 1e-10 * (1 + np.max(np.abs(F_ref)))
    Ef = ctx.fermion_energy()[0]
    assert abs(Ef - Ef_ref) <= 1e-11 * abs(Ef_ref), (Ef, Ef_ref)
    ctx.close()


PLAIN, THROUGH = 0, 1
INV, GEMM, SP_FWD, SP_BWD = 0, 1, 2, 3
L2_BYTES = 8 * (4 << 20)


def _plan_stores(lib, L, nbatch):
    cap = 256
    out = np.zeros(10 * cap, dtype=np.int64)
    ns = C.c_int64(0)
    rc = lib.dwh_debug_cr_plan_stores(L, L, nbatch, 1, 1, out.ctypes.data_as(C.c_void_p), cap, C.byref(ns))
    assert rc == 0, lib.dwh_last_error(None).decode()
    assert 0 < ns.value <= cap
    return out[:10 * ns.value].reshape(-1, 10)


# C3 (L = 32, 12 poles), C2 (L = 16, 10 poles), C5 (L = 48, 4 chains x 14 poles)
@pytest.mark.parametrize("L,nbatch", [(32, 12), (16, 10), (48, 56)])
def test_plan_store_policy_follows_the_rule(dwhmc, monkeypatch, L, nbatch):
    """DESIGN.md §4 "Store policy": write-through for the product stages with
    a K split (the short launches of the coarse levels: each writes less than
    the L2 holds, in 8-byte pieces already) and for the side products of the
    inversion launches; plain for the inversions' own outputs, the sparse
    stages and the product stages without a K split; DWHMC_CR_STORE=0: plain
    everywhere."""
    lib = dwhmc.load_library()
    monkeypatch.delenv("DWHMC_CR_STORE", raising=False)
    rows = _plan_stores(lib, L, nbatch)
    nthrough = 0
    for kind, ksplit, nbytes, side_bytes, first, side_first, store, side_store, nxt, side_nxt in rows:
        assert nbytes > 0 and first == 1   # every stage feeds the very next launch with some of its outputs
        assert 0 <= nxt <= nbytes and 0 <= side_nxt <= side_bytes
        if kind == GEMM and ksplit > 1:
            assert store == THROUGH
            assert nbytes * nbatch < L2_BYTES
            nthrough += 1
        else:
            assert store == PLAIN, (kind, ksplit)
        if side_bytes:
            assert kind == INV and side_store == THROUGH
            assert side_nxt < side_bytes   # most of the side products wait for a later launch
    assert nthrough > 0
    if L == 32:   # the side-work schedule runs at BP = 64 only
        assert sum(1 for r in rows if r[3]) == 4
    monkeypatch.setenv("DWHMC_CR_STORE", "0")
    off = _plan_stores(lib, L, nbatch)
    assert np.all(off[:, 6] == PLAIN) and np.all(off[:, 7] == PLAIN)
    assert np.array_equal(off[:, [0, 1, 2, 3, 4, 5, 8, 9]], rows[:, [0, 1, 2, 3, 4, 5, 8, 9]])
