"""Batched HMC chains whose sweeps end differently, each chain against its own
CPU oracle (tests/hmc_chain_cases.py): four chains of different disorder in
one context, six sweeps whose outcomes are prescribed so that every launch of
the trajectory boundary (k_traj_begin / k_traj_end, k_restore, the CR path's
per-chain E_f counters, the throughput path's shared halt / flag pair) sees
accepted and rejected chains side by side, every chain rejects twice in a row
somewhere, and a chain c > 0 is looked at after its rejections.

Bars (the project's, tests/test_gpu_parity.py header; none is new):
  flags equal; |ΔH - ΔH_ref| <= 1e-8 (1 + |ΔH_ref|); Δ <= 1e-10; π <= 1e-9;
  P <= 1e-11; |E_f - E_f,ref| <= 1e-11 |E_f,ref|; |Tr ρ_hh - ref| <= 1e-11 N
and, between two device runs, equality bit for bit.

Cases (4 chains, 6 sweeps, β = 8; tests/hmc_chain_cases.py CASES):
  6x4      Nt 3, cr / dense / eig
  12x5     Nt 2, cr, BP 32, odd Ly
  20x4     Nt 2, cr, BP 64, sparse level 0 and side work
  3x2      Nt 3, cr / dense / eig; several bonds on one pairing entry
  6x4-om2  Nt 2, omelyan2, cr / eig
Guard cases (3 chains, 4 sweeps, β = 32, delta_cap 0.2): cr 20x4, dense 6x6.

Which assertion catches what:
  * a restore that skips or mis-indexes a chain c > 0 (k_traj_end, k_restore,
    the backup stride): the rejected chain's Δ, P, E_f, Tr ρ_hh, F are not the
    bits read before the sweep, and Δ misses the oracle, in
    test_mixed_outcomes_single_sweeps and test_split_path_mixed_flags; the
    final state misses it in test_mixed_outcomes_throughput
  * a stale Tr ρ_hh (or E_f, P) after a rejection: hole_trace() against the
    oracle's kept state and against the bits before the sweep, same tests
  * a finish that ignores the host's flags: the second run of
    test_split_path_mixed_flags (chains 0 and 2 keep every ΔH > 0 trajectory,
    chains 1 and 3 drop every ΔH < 0 one) against OracleContext.hmc_finish
  * a neighbour disturbed by a tripped chain (a halted sweep that clobbers a
    backup, a replay that starts a neighbour elsewhere, a counter not reset):
    test_guard_trip_in_one_chain, every chain against its oracle on all three
    paths, the tripped chain rejected and restored next to kept neighbours
  * arithmetic or state that leaks between chains or depends on the chain's
    position: test_chain_permutation, bit for bit

Measured on an MI355X: MEASURED below, the largest error / bar per case and
quantity over all algorithms, paths and sweeps (the assertions allow 1; every
test prints its own line).  The largest is 0.073 (P on 3x2, cr).  The tests
found nothing to fix in the library: no flag differed, restores are copies and
the permuted runs agree bit for bit.  That they can fail was checked once with
a build carrying three wrong-value changes (k_traj_end restoring Tr ρ_hh for
chain 0 only, k_restore reading chain 0's flag for every chain, k_traj_begin
ignoring the halt of a tripped batch): 35 of the 36 tests failed, each change
reported by the assertions listed above.
"""
import numpy as np
import pytest

import hmc_chain_cases as H
from test_gpu_parity import device_ctx

pytestmark = pytest.mark.gpu

QUANTITIES = ("dH", "Delta", "pi", "P", "Ef", "Tr")
# largest observed error / bar on an MI355X, per case (worst algorithm and path): dH, Δ, π, P, E_f, Tr ρ_hh
MEASURED = {
    "6x4": (0.002, 0.011, 0.001, 0.053, 0.012, 0.007),
    "12x5": (0.003, 0.014, 0.001, 0.044, 0.004, 0.026),
    "20x4": (0.005, 0.009, 0.001, 0.030, 0.006, 0.019),
    "3x2": (0.001, 0.025, 0.002, 0.073, 0.010, 0.061),
    "6x4-om2": (0.002, 0.013, 0.001, 0.065, 0.013, 0.007),
    "guard cr-20x4": (0.059, 0.000, 0.000, 0.005, 0.015, 0.010),
    "guard dense-6x6": (0.013, 0.001, 0.001, 0.010, 0.005, 0.007),
}

ALGO_CASES = [(name, algo) for name, k in H.CASES.items() for algo in k.algos]
PERMUTATION = (2, 0, 3, 1)
PERMUTED_CASES = [(name, algo) for name, algo in ALGO_CASES if name in ("6x4", "20x4")]

_SINGLE = {}       # (case, algo) -> the single-sweep device run, shared by the tests that compare with it


class Ratios:
    """error / bar per quantity for one test: printed before anything is asserted."""

    def __init__(self, label):
        self.label, self.worst, self.fails = label, dict.fromkeys(QUANTITIES, 0.0), []

    def add(self, q, err, bar, where):
        r = float(err) / bar
        self.worst[q] = max(self.worst[q], r)
        if not r <= 1.0:
            self.fails.append(f"{q} {where}: error {err:.3e} bar {bar:.3e}")

    def fail(self, text):
        self.fails.append(text)

    def settle(self):
        print(f"RATIOS {self.label}: " + " ".join(f"{q}={self.worst[q]:.3f}" for q in QUANTITIES))
        assert not self.fails, "\n".join(self.fails)


def open_ctx(dwhmc, ref, algo, block=0, **kw):
    ctx = device_ctx(dwhmc, ref.p, ref.dis, algo, **kw)
    assert ctx.info["nchains"] == ref.nchains
    if block:
        assert ctx.info["block"] == block
    if ref.scheme != "leapfrog":
        ctx.set_integrator(ref.scheme)
    ctx.set_pairing(ref.Delta0)
    ctx.factorize()
    return ctx


def read_cache(ctx):
    """Everything a chain keeps between sweeps, as the host reads it."""
    D, pi = ctx.get_state()
    return dict(Delta=D, pi=pi, P=ctx.pairing(), Ef=ctx.fermion_energy(), Tr=ctx.hole_trace(), F=ctx.forces())


def check_dH(r, ref, s, dH):
    for c in range(ref.nchains):
        r.add("dH", abs(dH[c] - ref.dH[s, c]), 1e-8 * (1 + abs(ref.dH[s, c])), f"sweep {s} chain {c}")


def check_cache(r, ref, s, cache):
    """The kept state after sweep s against the oracle's, chain by chain."""
    N = ref.p.N
    for c in range(ref.nchains):
        w = f"sweep {s} chain {c} ({'accepted' if ref.acc[s, c] else 'rejected'})"
        r.add("Delta", np.max(np.abs(cache["Delta"][c] - ref.Delta[s, c])), 1e-10, w)
        r.add("pi", np.max(np.abs(cache["pi"][c] - ref.pi[s, c])), 1e-9, w)
        r.add("P", np.max(np.abs(cache["P"][c] - ref.P[s, c])), 1e-11, w)
        r.add("Ef", abs(cache["Ef"][c] - ref.Ef[s, c]), 1e-11 * abs(ref.Ef[s, c]), w)
        r.add("Tr", abs(cache["Tr"][c] - ref.Tr[s, c]), 1e-11 * N, w)


def check_restore(r, ref, s, before, after, reselected=False):
    """Restore is a copy: a rejected chain has the bits it had before the
    sweep; an accepted neighbour has moved.  A sweep that re-selected the poles
    refactorised its starting Δ with the new ones, so there only Δ is a copy
    (P, E_f, Tr ρ_hh are held to the oracle by check_cache)."""
    for c in range(ref.nchains):
        for q in ("Delta",) if reselected else ("Delta", "P", "Ef", "Tr", "F"):
            same = np.array_equal(before[q][c], after[q][c])
            if same == bool(ref.acc[s, c]):
                how = "unchanged after an accepted" if same else "changed by a rejected"
                r.fail(f"{q} sweep {s} chain {c}: {how} sweep")


def same_bits(r, what, a, b):
    if not np.array_equal(a, b):
        diff = np.max(np.abs(np.asarray(a, dtype=np.complex128) - b))
        r.fail(f"{what}: the two device runs differ, max |difference| {diff:.3e}")


def run_single(dwhmc, ref, algo, r, block=0, **kw):
    """hmc_sweep sweep by sweep with every check of test 1; returns the device's
    (flags, ΔH, kept state) per sweep and the context's info at the end."""
    ctx = open_ctx(dwhmc, ref, algo, block, **kw)
    out = []
    before, cap = read_cache(ctx), ctx.info["delta_cap"]
    for s in range(ref.nsweeps):
        acc, dH = ctx.hmc_sweep(ref.noise[s], ref.u[s], ref.Nt, ref.dt, ref.p.mass)
        after, cap_before, cap = read_cache(ctx), cap, ctx.info["delta_cap"]
        if not np.array_equal(acc, ref.acc[s]):
            r.fail(f"flags sweep {s}: device {acc.astype(int)} oracle {ref.acc[s].astype(int)} "
                   f"(dH {dH}, ref {ref.dH[s]})")
        check_dH(r, ref, s, dH)
        check_cache(r, ref, s, after)
        check_restore(r, ref, s, before, after, cap != cap_before)
        out.append((acc, dH, after, cap))
        before = after
    ctx.close()
    return out


def single(dwhmc, name, algo):
    """The single-sweep device run of a table case, made once."""
    if (name, algo) not in _SINGLE:
        r = Ratios(f"{name} {algo} single")
        _SINGLE[name, algo] = run_single(dwhmc, H.reference(name), algo, r, H.CASES[name].block)
        r.settle()
    return _SINGLE[name, algo]


def run_throughput(dwhmc, ref, algo, r, windows, **kw):
    """load_draws + run_sweeps over all sweeps, the results read in `windows`
    ((first, count), ...); flags and ΔH per sweep and the final state against
    the oracle.  Returns (flags, ΔH, final kept state, delta_cap at the end)."""
    ctx = open_ctx(dwhmc, ref, algo, **kw)
    ctx.load_draws(ref.noise, ref.u)
    ctx.run_sweeps(0, ref.nsweeps, ref.Nt, ref.dt, ref.p.mass)
    parts = [ctx.sweep_results(first, count) for first, count in windows]
    acc, dH = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert acc.shape == (ref.nsweeps, ref.nchains)
    for s in range(ref.nsweeps):
        if not np.array_equal(acc[s], ref.acc[s]):
            r.fail(f"flags sweep {s}: device {acc[s].astype(int)} oracle {ref.acc[s].astype(int)}")
        check_dH(r, ref, s, dH[s])
    final = read_cache(ctx)
    check_cache(r, ref, ref.nsweeps - 1, final)
    cap = ctx.info["delta_cap"]
    ctx.close()
    return acc, dH, final, cap


def run_split(dwhmc, ref, algo, r, **kw):
    """hmc_trajectory + hmc_finish with the reference's flags, the checks of
    test 1 after every finish; returns (ΔH, kept state) per sweep."""
    ctx = open_ctx(dwhmc, ref, algo, **kw)
    out = []
    before, cap = read_cache(ctx), ctx.info["delta_cap"]
    for s in range(ref.nsweeps):
        dH = ctx.hmc_trajectory(ref.noise[s], ref.Nt, ref.dt, ref.p.mass)
        ctx.hmc_finish(ref.acc[s])
        after, cap_before, cap = read_cache(ctx), cap, ctx.info["delta_cap"]
        check_dH(r, ref, s, dH)
        check_cache(r, ref, s, after)
        check_restore(r, ref, s, before, after, cap != cap_before)
        out.append((dH, after, cap))
        before = after
    ctx.close()
    return out


# -- 1. hmc_sweep, sweep by sweep ------------------------------------------------
@pytest.mark.parametrize("name,algo", ALGO_CASES)
def test_mixed_outcomes_single_sweeps(dwhmc, name, algo):
    H.assert_pattern(H.reference(name).acc)
    _SINGLE.pop((name, algo), None)
    single(dwhmc, name, algo)


# -- 2. load_draws + run_sweeps ----------------------------------------------------
@pytest.mark.parametrize("name,algo", ALGO_CASES)
def test_mixed_outcomes_throughput(dwhmc, name, algo):
    ref = H.reference(name)
    H.assert_pattern(ref.acc)
    one = single(dwhmc, name, algo)
    r = Ratios(f"{name} {algo} throughput")
    acc, dH, final, _ = run_throughput(dwhmc, ref, algo, r, ((0, 2), (2, 4)))
    for s in range(ref.nsweeps):
        same_bits(r, f"flags of sweep {s}", acc[s], one[s][0])
        same_bits(r, f"dH of sweep {s}", dH[s], one[s][1])
    for q in ("Delta", "pi", "P", "Ef", "Tr"):
        same_bits(r, f"final {q}", final[q], one[-1][2][q])
    r.settle()


# -- 3. hmc_trajectory + hmc_finish ---------------------------------------------
@pytest.mark.parametrize("name,algo", ALGO_CASES)
def test_split_path_mixed_flags(dwhmc, name, algo):
    """The host decides.  First the realised flags of the reference run: bit
    for bit test 1.  Then flags that contradict Metropolis (chains 0 and 2 keep
    every trajectory, ΔH > 0 included; chains 1 and 3 drop every one, ΔH < 0
    included) against OracleContext.hmc_finish with the same flags."""
    ref = H.reference(name)
    H.assert_pattern(ref.acc)
    one = single(dwhmc, name, algo)
    r = Ratios(f"{name} {algo} split")
    split = run_split(dwhmc, ref, algo, r)
    for s in range(ref.nsweeps):
        same_bits(r, f"dH of sweep {s}", split[s][0], one[s][1])
        for q in ("Delta", "pi", "P", "Ef", "Tr", "F"):
            same_bits(r, f"{q} after sweep {s}", split[s][1][q], one[s][2][q])
    contrary = H.reference(name, H.contrary_flags)
    assert np.any(contrary.dH[:, [0, 2]] > 0) and np.all(~contrary.acc[:, [1, 3]])
    run_split(dwhmc, contrary, algo, r)
    r.settle()


# -- 4. the chains in another order ------------------------------------------------
@pytest.mark.parametrize("name,algo", PERMUTED_CASES)
def test_chain_permutation(dwhmc, name, algo):
    """The chains and their draws in the order (2, 0, 3, 1): every per-chain
    result of the single-sweep and of the throughput path equals the
    unpermuted run's bit for bit, so nothing a chain computes depends on its
    position in the batch or on its neighbours."""
    ref = H.reference(name)
    one = single(dwhmc, name, algo)
    order = list(PERMUTATION)
    perm = ref.permuted(order)
    r = Ratios(f"{name} {algo} permuted")
    moved = run_single(dwhmc, perm, algo, r, H.CASES[name].block)
    acc, dH, final, _ = run_throughput(dwhmc, perm, algo, r, ((0, ref.nsweeps),))
    for s in range(ref.nsweeps):
        same_bits(r, f"flags of sweep {s}", moved[s][0], one[s][0][order])
        same_bits(r, f"dH of sweep {s}", moved[s][1], one[s][1][order])
        same_bits(r, f"throughput flags of sweep {s}", acc[s], one[s][0][order])
        same_bits(r, f"throughput dH of sweep {s}", dH[s], one[s][1][order])
        for q in ("Delta", "pi", "P", "Ef", "Tr"):
            same_bits(r, f"{q} after sweep {s}", moved[s][2][q], one[s][2][q][order])
    for q in ("Delta", "pi", "P", "Ef", "Tr"):
        same_bits(r, f"throughput final {q}", final[q], one[-1][2][q][order])
    r.settle()


# -- 5. a guard trip in one chain of the batch ---------------------------------------
@pytest.mark.parametrize("name", list(H.GUARD_CASES))
def test_guard_trip_in_one_chain(dwhmc, name):
    """Chain 1 of 3 drifts past delta_cap in sweep 2 of 4: the poles are
    re-selected and the sweep replayed for the whole batch (the library's
    recoverable path).  The oracle has no guard.  The tripped chain's ΔH is
    ~1e2, so it is rejected and restored next to two accepted neighbours; every
    chain matches its oracle through hmc_sweep, through run_sweeps (where the
    later sweeps of the batch halt and are replayed) and through
    hmc_trajectory + hmc_finish — there also with the host rejecting untripped
    chain 2 in the tripped sweep (H.assert_guard_pattern says why Metropolis
    cannot be made to)."""
    k = H.GUARD_CASES[name]
    ref = H.guard_reference(name)
    H.assert_guard_pattern(ref.acc)
    host = H.guard_reference(name, H.guard_host_flags)
    H.assert_guard_pattern(host.acc, host_flags=True)
    cap0, trip = H.GUARD_CAP, H.TRIP[0]
    r = Ratios(f"guard {name}")
    one = run_single(dwhmc, ref, k.algo, r, delta_cap=cap0)
    caps = [o[3] for o in one]
    assert all(c == cap0 for c in caps[:trip]) and all(c > cap0 for c in caps[trip:]), caps
    acc, dH, final, cap = run_throughput(dwhmc, ref, k.algo, r, ((0, ref.nsweeps),), delta_cap=cap0)
    assert cap == caps[-1]
    for s in range(ref.nsweeps):
        same_bits(r, f"throughput flags of sweep {s}", acc[s], one[s][0])
        same_bits(r, f"throughput dH of sweep {s}", dH[s], one[s][1])
    for q in ("Delta", "pi"):
        same_bits(r, f"throughput final {q}", final[q], one[-1][2][q])
    for flags in (ref, host):
        split = run_split(dwhmc, flags, k.algo, r, delta_cap=cap0)
        caps = [o[2] for o in split]
        assert all(c == cap0 for c in caps[:trip]) and all(c > cap0 for c in caps[trip:]), caps
    r.settle()
