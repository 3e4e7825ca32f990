"""Reference runs for tests/test_hmc_chains.py: several chains in one context
whose sweeps end differently (accepted, rejected, tripped), every chain on the
CPU oracle by itself.

The reference runs hmc_trajectory, then decides, then hmc_finish, so the
outcome of every (sweep, chain) is prescribed here instead of left to a seed:

  wished     chain c of sweep s is to be rejected iff (s + c) % 4 in (0, 1)
  realised   a wished rejection only where the reference's own ΔH >= 0.05
             (MIN_REJECT_DH); otherwise the sweep is accepted; where
             exp(-ΔH) < 1e-6 (TINY_EXP) it is rejected whatever was wished

and the uniform the device is given follows from the realised outcome:

  accept             u = 0.5 min(1, exp(-ΔH))
  reject             u = 0.5 (1 + exp(-ΔH))
  reject, tiny exp   u = 0.5

u is then at least ~0.009 away from the device's threshold exp(-ΔH_dev) for
|ΔH| <= 4 (0.024 for rejections), while the ΔH bar of the project, 1e-8 (1 +
|ΔH|), moves that threshold by 1e-7 at most: a device flag that differs from
the reference's is wrong, not unlucky.

The whole reference run precedes the device run (the throughput path wants all
uniforms before its first sweep) and is computed once per case (reference(),
guard_reference()); nobody writes to what they return.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from oracle import dwhmc_oracle as O
from oracle_context import OracleContext
from test_gpu_parity import make_case
from test_integrator_gpu import LEAP, OM2, NumpyChain

MIN_REJECT_DH = 0.05
TINY_EXP = 1e-6
BETA, NCHAINS, NSWEEPS = 8.0, 4, 6


@dataclasses.dataclass(frozen=True)
class Case:
    """Chain c is make_case(Lx, Ly, BETA, seed=seed + c, amp=0.1); noise is
    default_rng(noise_seed), one (NCHAINS, N, 2) complex normal draw per sweep;
    dt = dt_mult · calc_optimal_dt."""
    Lx: int
    Ly: int
    Nt: int
    algos: tuple
    scheme: str = "leapfrog"
    seed: int = 500
    noise_seed: int = 21
    dt_mult: float = 2.0
    block: int = 0                  # the CR block size the case is there for (0: not checked)


CASES = {
    "6x4": Case(6, 4, 3, ("cr", "dense", "eig")),
    "12x5": Case(12, 5, 2, ("cr",), block=32),
    "20x4": Case(20, 4, 2, ("cr",), block=64),
    "3x2": Case(3, 2, 3, ("cr", "dense", "eig"), seed=516),
    "6x4-om2": Case(6, 4, 2, ("cr", "eig"), scheme="omelyan2", seed=548, noise_seed=22, dt_mult=2.1),
}
SCHEDULES = {"leapfrog": LEAP, "omelyan2": OM2}


@dataclasses.dataclass(frozen=True)
class GuardCase:
    """test_guard_trip_recovers_in_throughput_path's recipe on three chains:
    amp = 0, noise x 0.05 except chain 1 of sweep 2 (x 8), Nt = 4, dt = 0.1,
    delta_cap = 0.2 on the device; the reference has no guard.  β = 32 instead
    of that test's 4: the tripped trajectory's ΔH is then ~1e2 and the chain is
    rejected and restored, where at β = 4 (ΔH ~ 1) every sweep of the run would
    be accepted."""
    Lx: int
    Ly: int
    algo: str
    beta: float = 32.0
    seed: int = 24
    noise_seed: int = 25


GUARD_CASES = {
    "cr-20x4": GuardCase(20, 4, "cr"),
    "dense-6x6": GuardCase(6, 6, "dense"),
}
GUARD_NCHAINS, GUARD_NSWEEPS, GUARD_NT, GUARD_DT, GUARD_CAP = 3, 4, 4, 0.1, 0.2
TRIP = (2, 1)                       # (sweep, chain)


def wished_reject(s: int, c: int) -> bool:
    return (s + c) % 4 in (0, 1)


def prescribe(s: int, dH):
    """(accept flags, uniforms) of sweep s from the reference's ΔH per chain."""
    dH = np.asarray(dH, dtype=np.float64)
    acc = np.ones(len(dH), dtype=bool)
    u = np.empty(len(dH))
    for c, d in enumerate(dH):
        e = math.exp(min(-d, 700.0))
        if e < TINY_EXP:
            acc[c], u[c] = False, 0.5
        elif wished_reject(s, c) and d >= MIN_REJECT_DH:
            acc[c], u[c] = False, 0.5 * (1.0 + e)
        else:
            u[c] = 0.5 * min(1.0, e)
    return acc, u


def contrary_flags(s: int, dH):
    """Host flags that contradict Metropolis: chains 0 and 2 accept whatever
    ΔH is (every ΔH > 0 included), chains 1 and 3 reject whatever it is (every
    ΔH < 0 included).  No uniform belongs to them."""
    acc = np.array([c % 2 == 0 for c in range(len(dH))])
    return acc, np.full(len(dH), np.nan)


class ScheduleContext:
    """OracleContext's trajectory interface for a splitting other than
    leapfrog: one NumpyChain (tests/test_integrator_gpu.py) per chain."""

    def __init__(self, p, dis, schedule):
        self.p, self.dis, self.schedule = p, dis, schedule
        self.nchains = len(dis)
        self.chains = None

    def set_pairing(self, Delta):
        self.chains = [NumpyChain(O, self.p, self.dis[c], Delta[c]) for c in range(self.nchains)]

    def factorize(self):
        pass                                                    # NumpyChain diagonalises as it is built

    def get_state(self):
        return np.stack([ch.Delta for ch in self.chains]), np.stack([ch.pi for ch in self.chains])

    def pairing(self):
        return np.stack([O.pairing_P(ch.cache.U, ch.cache.E_n, self.p)[0] for ch in self.chains])

    def fermion_energy(self):
        return np.array([O.fermion_energy(ch.cache.E_n, self.p.beta) for ch in self.chains])

    def hole_trace(self):
        return np.array([(O.measure_observables(ch.cache, self.p, ch.Delta)["hole_conc"] + 1.0) * self.p.N / 2
                         for ch in self.chains])

    def hmc_trajectory(self, noise, Nt, dt, mass):
        assert mass == self.p.mass
        self._backup = [(ch.Delta.copy(), ch.cache.E_n.copy(), ch.cache.U.copy()) for ch in self.chains]
        return np.array([ch.trajectory(noise[c], *self.schedule, Nt, dt) for c, ch in enumerate(self.chains)])

    def hmc_finish(self, accepted):
        for ch, a, b in zip(self.chains, accepted, self._backup):
            if not a:
                ch.restore(*b)
        self._backup = None

    def hmc_sweep(self, noise, uniform, Nt, dt, mass):
        assert mass == self.p.mass
        res = [ch.sweep(noise[c], float(uniform[c]), *self.schedule, Nt, dt) for c, ch in enumerate(self.chains)]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def reference_context(p, dis, scheme="leapfrog"):
    if scheme == "leapfrog":
        return OracleContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis)
    return ScheduleContext(p, dis, SCHEDULES[scheme])


@dataclasses.dataclass(frozen=True)
class Reference:
    """A finished reference run.  Per sweep s and chain c: noise[s, c], u[s, c],
    acc[s, c], dH[s, c] and the kept state after the sweep: Delta, pi, P
    ([s, c, N, 2]), Ef, Tr ([s, c]; Tr is Tr ρ_hh)."""
    p: object
    dis: np.ndarray
    Delta0: np.ndarray
    Nt: int
    dt: float
    scheme: str
    noise: np.ndarray
    u: np.ndarray
    acc: np.ndarray
    dH: np.ndarray
    Delta: np.ndarray
    pi: np.ndarray
    P: np.ndarray
    Ef: np.ndarray
    Tr: np.ndarray

    @property
    def nsweeps(self):
        return self.noise.shape[0]

    @property
    def nchains(self):
        return self.noise.shape[1]

    def permuted(self, order):
        """The same run with the chains (and their draws) in another order."""
        o = list(order)
        per_chain = {k: getattr(self, k)[:, o] for k in ("noise", "u", "acc", "dH", "Delta", "pi", "P", "Ef", "Tr")}
        return dataclasses.replace(self, dis=self.dis[o], Delta0=self.Delta0[o], **per_chain)


def run_reference(p, dis, Delta0, noise, Nt, dt, scheme="leapfrog", decide=prescribe) -> Reference:
    """All sweeps of `noise` ((nsweeps, nchains, N, 2)) on the reference:
    trajectory, decide(s, ΔH) -> (flags, uniforms), finish."""
    ctx = reference_context(p, dis, scheme)
    ctx.set_pairing(Delta0)
    ctx.factorize()
    rec = {k: [] for k in ("u", "acc", "dH", "Delta", "pi", "P", "Ef", "Tr")}
    for s in range(noise.shape[0]):
        dH = ctx.hmc_trajectory(noise[s], Nt, dt, p.mass)
        acc, u = decide(s, dH)
        ctx.hmc_finish(acc)
        D, pi = ctx.get_state()
        for k, v in (("u", u), ("acc", acc), ("dH", dH), ("Delta", D), ("pi", pi), ("P", ctx.pairing()),
                     ("Ef", ctx.fermion_energy()), ("Tr", ctx.hole_trace())):
            rec[k].append(np.array(v))
    out = {k: np.stack(v) for k, v in rec.items()}
    for a in (noise, dis, Delta0, *out.values()):
        a.setflags(write=False)
    return Reference(p=p, dis=dis, Delta0=Delta0, Nt=Nt, dt=dt, scheme=scheme, noise=noise, **out)


def cnoise(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)


def case_inputs(name):
    """(p, disorder (nc, N), Δ0 (nc, N, 2), noise (ns, nc, N, 2), Nt, dt, scheme) of a table case."""
    k = CASES[name]
    chains = [make_case(O, k.Lx, k.Ly, BETA, seed=k.seed + c, amp=0.1) for c in range(NCHAINS)]
    p = chains[0][0]
    rng = np.random.default_rng(k.noise_seed)
    noise = np.stack([cnoise(rng, (NCHAINS, p.N, 2)) for _ in range(NSWEEPS)])
    dt = k.dt_mult * O.calc_optimal_dt(p.beta, p.J, p.mass, k.Nt)
    return p, np.stack([c[1] for c in chains]), np.stack([c[2] for c in chains]), noise, k.Nt, dt, k.scheme


@functools.lru_cache(maxsize=None)
def reference(name, decide=prescribe) -> Reference:
    return run_reference(*case_inputs(name), decide=decide)


def guard_inputs(name):
    k = GUARD_CASES[name]
    chains = [make_case(O, k.Lx, k.Ly, k.beta, seed=k.seed + k.Lx + c, amp=0.0) for c in range(GUARD_NCHAINS)]
    p = chains[0][0]
    rng = np.random.default_rng(k.noise_seed)
    noise = cnoise(rng, (GUARD_NSWEEPS, GUARD_NCHAINS, p.N, 2))
    scale = np.full((GUARD_NSWEEPS, GUARD_NCHAINS), 0.05)
    scale[TRIP] = 8.0
    noise = noise * scale[:, :, None, None]
    return p, np.stack([c[1] for c in chains]), np.stack([c[2] for c in chains]), noise, GUARD_NT, GUARD_DT, "leapfrog"


def guard_host_flags(s: int, dH):
    """prescribe(), but in the tripped sweep the host also rejects untripped
    chain 2 (whose ΔH < 0 there): a restored chain next to the tripped one.
    Only hmc_finish can be given this; Metropolis accepts every ΔH < 0."""
    acc, u = prescribe(s, dH)
    if s == TRIP[0]:
        acc[2], u[2] = False, np.nan
    return acc, u


@functools.lru_cache(maxsize=None)
def guard_reference(name, decide=prescribe) -> Reference:
    return run_reference(*guard_inputs(name), decide=decide)


def assert_pattern(outcomes):
    """Conditions on the reference's accept flags ((nsweeps, nchains)), asserted
    before any device call: every chain rejects at least twice and accepts at
    least twice, some chain rejects in two consecutive sweeps, and every sweep
    has both outcomes among its chains."""
    acc = np.asarray(outcomes, dtype=bool)
    rej = ~acc
    assert np.all(rej.sum(axis=0) >= 2), f"rejections per chain {rej.sum(axis=0)}"
    assert np.all(acc.sum(axis=0) >= 2), f"acceptances per chain {acc.sum(axis=0)}"
    assert np.any(rej[:-1] & rej[1:]), "no chain rejects in two consecutive sweeps"
    assert np.all(acc.any(axis=1) & rej.any(axis=1)), f"sweeps with one outcome only: {acc.astype(int).tolist()}"


def assert_guard_pattern(outcomes, host_flags=False):
    """The guard cases' condition on the tripped sweep: both outcomes among its
    chains.  With this recipe (momenta x 0.05 on a start that is not a minimum
    of the action) every untripped trajectory mostly slides downhill, and a
    leapfrog trajectory that starts near rest has ΔH <= 0: on the CPU the
    untripped ΔH of sweep 2 stayed negative (-1e-4 to -5) for β from 4 to
    1300 and jumped to +1.4e3 for all chains at once beyond the integrator's
    stability limit, so no seed or β makes Metropolis reject one untripped chain and
    accept the other.  What is asserted instead: the tripped chain is rejected
    (ΔH ~ 1e2, exp(-ΔH) < 1e-6) and both neighbours are accepted; with
    host_flags (guard_host_flags, the split path only) the tripped chain and
    chain 2 are rejected and chain 0 accepted — the mixed outcome among the
    untripped chains."""
    s, c = TRIP
    want = [True, False, not host_flags]
    assert c == 1 and [bool(a) for a in outcomes[s]] == want, np.asarray(outcomes).astype(int).tolist()
