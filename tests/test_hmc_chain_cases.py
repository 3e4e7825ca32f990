"""CPU tests of tests/hmc_chain_cases.py, the reference side of
tests/test_hmc_chains.py: the outcome rule, the pattern conditions of every
case, and that the uniforms handed to the device make an ordinary hmc_sweep
(Metropolis decides) retrace the run whose outcomes were prescribed through
hmc_trajectory + hmc_finish."""
import math

import numpy as np
import pytest

import hmc_chain_cases as H


def test_prescribe_rule():
    dH = np.array([0.3, 0.3, 0.3, 0.3])
    acc, u = H.prescribe(0, dH)                              # wished: chains 0, 1 (s + c = 0, 1)
    assert acc.tolist() == [False, False, True, True]
    e = math.exp(-0.3)
    assert np.allclose(u, [0.5 * (1 + e), 0.5 * (1 + e), 0.5 * e, 0.5 * e])
    acc, u = H.prescribe(3, dH)                              # s + c = 3, 4, 5, 6 -> chains 1, 2
    assert acc.tolist() == [True, False, False, True]
    # a wished rejection below the threshold or at ΔH < 0 is an acceptance
    acc, u = H.prescribe(0, np.array([0.049, -0.2, 0.05, 1.0]))
    assert acc.tolist() == [True, True, True, True]
    assert u[1] == 0.5 and u[0] == 0.5 * math.exp(-0.049)
    acc, u = H.prescribe(0, np.array([0.05, 14.0, 14.0, -1e4]))
    assert acc.tolist() == [False, False, False, True]       # exp(-14) < 1e-6: whatever was wished
    assert u[1] == 0.5 and u[2] == 0.5 and u[3] == 0.5
    # every uniform decides as Metropolis would (src/HMC.jl:128)
    for s in range(6):
        d = np.array([-3.0, -0.01, 0.0, 0.04, 0.05, 0.7, 3.9, 13.0, 14.0, 500.0])
        for off in range(4):
            acc, u = H.prescribe(s + off, d)
            metro = (d < 0) | (u < np.exp(-d))
            assert np.array_equal(acc, metro)
            assert np.all(np.abs(u - np.exp(-d))[np.abs(d) <= 4] >= 0.009)
            assert np.all(np.abs(u - np.exp(-d))[~acc & (d <= 4)] >= 0.024)


def test_assert_pattern_refuses():
    good = np.array([[0, 1, 1, 0], [0, 1, 0, 1], [1, 0, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0], [1, 0, 0, 1]], dtype=bool)
    H.assert_pattern(good)
    bad = good.copy()
    bad[:, 3] = [1, 1, 1, 0, 1, 1]                           # chain 3 rejects once
    with pytest.raises(AssertionError):
        H.assert_pattern(bad)
    bad = good.copy()
    bad[2] = True                                            # a sweep with one outcome
    with pytest.raises(AssertionError):
        H.assert_pattern(bad)
    alternating = np.array([[0, 1], [1, 0]] * 3, dtype=bool)  # no two rejections in a row
    with pytest.raises(AssertionError):
        H.assert_pattern(alternating)


@pytest.mark.parametrize("name", list(H.CASES))
def test_case_meets_pattern(name):
    ref = H.reference(name)
    assert ref.acc.shape == (H.NSWEEPS, H.NCHAINS) and ref.p.beta == H.BETA
    H.assert_pattern(ref.acc)
    rej = ~ref.acc
    assert np.all(ref.dH[rej] >= H.MIN_REJECT_DH)
    # inside the range for which the distance of u from the threshold is stated
    assert np.max(np.abs(ref.dH)) <= 4.1, np.max(np.abs(ref.dH))
    assert np.all(np.abs(ref.u - np.exp(-ref.dH)) >= 0.008)
    # rejected: the state is the one before the sweep; accepted: it moved
    before = np.concatenate([ref.Delta0[None], ref.Delta[:-1]])
    for s, c in np.ndindex(*ref.acc.shape):
        assert np.array_equal(ref.Delta[s, c], before[s, c]) == bool(rej[s, c])
    # what the permutation test relies on
    order = (2, 0, 3, 1)
    perm = ref.permuted(order)
    assert np.array_equal(perm.dH[:, 1], ref.dH[:, 0]) and np.array_equal(perm.dis[0], ref.dis[2])


@pytest.mark.parametrize("name", list(H.CASES))
def test_sweep_with_prescribed_uniforms_retraces(name):
    """hmc_sweep with the prescribed u = hmc_trajectory + hmc_finish with the
    realised flags: outcomes, ΔH and every kept quantity, bit for bit (the
    same arithmetic in the same order)."""
    ref = H.reference(name)
    ctx = H.reference_context(ref.p, ref.dis, ref.scheme)
    ctx.set_pairing(ref.Delta0)
    ctx.factorize()
    for s in range(ref.nsweeps):
        acc, dH = ctx.hmc_sweep(ref.noise[s], ref.u[s], ref.Nt, ref.dt, ref.p.mass)
        assert np.array_equal(acc, ref.acc[s]) and np.array_equal(dH, ref.dH[s])
        D, pi = ctx.get_state()
        assert np.array_equal(D, ref.Delta[s]) and np.array_equal(pi, ref.pi[s])
        assert np.array_equal(ctx.pairing(), ref.P[s])
        assert np.array_equal(ctx.fermion_energy(), ref.Ef[s])
        assert np.array_equal(ctx.hole_trace(), ref.Tr[s])


def test_contrary_flags_run():
    """The second run of the split-path test: chains 0 and 2 keep every
    trajectory, chains 1 and 3 none, and both kinds of contradiction occur."""
    ref = H.reference("6x4", H.contrary_flags)
    assert np.all(ref.acc == np.array([True, False, True, False]))
    assert np.any(ref.dH[:, [0, 2]] > 0)                      # accepted against exp(-ΔH) < u for some u
    assert np.all(ref.Delta[:, [1, 3]] == ref.Delta0[[1, 3]])  # chains 1 and 3 never move


@pytest.mark.parametrize("name", list(H.GUARD_CASES))
def test_guard_case_meets_pattern(name):
    ref = H.guard_reference(name)
    assert ref.acc.shape == (H.GUARD_NSWEEPS, H.GUARD_NCHAINS)
    H.assert_guard_pattern(ref.acc)
    s, c = H.TRIP
    cap = H.GUARD_CAP
    # the trip is the tripped chain's alone, and no chain is near the cap in a kept state
    others = [k for k in range(H.GUARD_NCHAINS) if k != c]
    assert np.max(np.abs(ref.Delta[:, others])) < 0.5 * cap and np.max(np.abs(ref.Delta0)) < 0.5 * cap
    assert ref.dH[s, c] > -math.log(H.TINY_EXP) and np.all(ref.dH[s, others] < 0)
    host = H.guard_reference(name, H.guard_host_flags)
    H.assert_guard_pattern(host.acc, host_flags=True)
    # up to the tripped sweep the two runs are one
    assert np.array_equal(host.dH[:s + 1], ref.dH[:s + 1]) and not np.array_equal(host.Delta[s, 2], ref.Delta[s, 2])
