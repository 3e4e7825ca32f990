"""Test infrastructure: OracleContext with the throughput path and its sweep
log (FermionContext.load_draws / run_sweeps / sweep_results / sweep_log /
sweep_observables / sweep_field_sq / sweep_snapshots), built on the oracle's
hmc_sweep, the host formula hmc.observables_from_outputs and numpy.fft.fft2.
The reference side of tests/test_sweep_log.py and tests/test_sweep_log_gpu.py;
never used by the product path."""
from __future__ import annotations

import numpy as np

import dwhmc_loader
from oracle import dwhmc_oracle as O
from oracle_context import OracleContext

OBS_FIELDS = 12


def record(p, Delta, P, Ef, tr_hh) -> np.ndarray:
    """The 12 doubles of one (sweep, chain): hmc.observables_from_outputs'
    nine fields in the reference's order, then E_f, Tr ρ_hh, Σ|Δ_ij|²."""
    hmc = dwhmc_loader.load_package().hmc
    o = hmc.observables_from_outputs(p, Delta, P, Ef, tr_hh)
    return np.array([o.total_energy, o.Delta_amp, o.Delta_local, o.Delta_global, o.S_Delta, o.hole_conc,
                     o.Delta_diff, o.Delta_pair, o.Delta_localpair, float(Ef), float(tr_hh),
                     float(np.sum(np.abs(np.asarray(Delta)) ** 2))])


def field_sq(Delta, Lx: int, Ly: int) -> np.ndarray:
    """(2, Ly, Lx): |fft2(f)|² / N² of f = d (channel 0) and s (1), site
    i = x + Lx·y, so [ky, kx] with the forward sign exp(-2πi (kx x/Lx + ky y/Ly))."""
    D = np.asarray(Delta)
    out = []
    for f in (0.5 * (D[:, 0] - D[:, 1]), 0.5 * (D[:, 0] + D[:, 1])):
        out.append(np.abs(np.fft.fft2(f.reshape(Ly, Lx))) ** 2 / (Lx * Ly) ** 2)
    return np.stack(out)


class LoggedOracleContext(OracleContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._noise = self._u = None
        self._what = (False, False, 0, 0)
        self._clear()

    def _clear(self):
        n = 0 if self._noise is None else len(self._noise)
        self._acc = np.zeros((n, self.nchains), dtype=bool)
        self._dH = np.zeros((n, self.nchains))
        self._obs = np.zeros((n, self.nchains, OBS_FIELDS))
        self._sq = np.zeros((n, self.nchains, 2, self.p.Ly, self.p.Lx))
        self._snap = {}

    def load_draws(self, noise, uniform):
        noise = np.asarray(noise, dtype=np.complex128)
        ns = noise.shape[0]
        self._noise = noise.reshape(ns, self.nchains, self.N, 2).copy()
        self._u = np.asarray(uniform, dtype=np.float64).reshape(ns, self.nchains).copy()
        if ns > len(self._acc):
            self._clear()

    def sweep_log(self, observables=True, field_sq=False, snapshot_every=0, snapshot_offset=0):
        if snapshot_every < 0 or snapshot_offset < 0:
            raise ValueError("snapshot cadence")
        self._what = (bool(observables), bool(field_sq), int(snapshot_every), int(snapshot_offset))
        self._clear()

    def run_sweeps(self, first, nsweeps, Nt, dt, mass):
        obs, sq, every, offset = self._what
        for sw in range(first, first + nsweeps):
            self._acc[sw], self._dH[sw] = self.hmc_sweep(self._noise[sw], self._u[sw], Nt, dt, mass)
            if obs:
                P, Ef, tr = self.pairing(), self.fermion_energy(), self.hole_trace()
                for c in range(self.nchains):
                    self._obs[sw, c] = record(self.p, self.Delta[c], P[c], Ef[c], tr[c])
            if sq:
                for c in range(self.nchains):
                    self._sq[sw, c] = field_sq_of(self, c)
            if every and sw >= offset and (sw - offset) % every == 0:
                self._snap[sw] = self.Delta.copy()

    def sweep_results(self, first, nsweeps):
        return self._acc[first:first + nsweeps].copy(), self._dH[first:first + nsweeps].copy()

    def sweep_observables(self, first, nsweeps):
        assert self._what[0]
        return self._obs[first:first + nsweeps].copy()

    def sweep_field_sq(self, first, nsweeps):
        assert self._what[1]
        return self._sq[first:first + nsweeps].copy()

    def sweep_snapshots(self, first, nsweeps):
        assert self._what[2]
        sweeps = [s for s in sorted(self._snap) if first <= s < first + nsweeps]
        D = np.stack([self._snap[s] for s in sweeps]) if sweeps else np.zeros((0, self.nchains, self.N, 2), complex)
        return np.array(sweeps, dtype=np.int64), D

    def measure_transport_deltas(self, deltas, eta, domega, omega_max, chain=0):
        """OracleContext's, with the chain's eigensystem put back: the device
        measures a list of Δ on buffers of its own, and a driver that measures
        an earlier sweep's snapshot goes on from the chain's own state."""
        cache = self.caches[chain]
        E, U = cache.E_n.copy(), cache.U.copy()
        out = super().measure_transport_deltas(deltas, eta, domega, omega_max, chain=chain)
        cache.E_n[:] = E
        cache.U[:, :] = U
        O.update_H_BdG(cache, self.p, self.Delta[chain])
        return out


def field_sq_of(ctx, c):
    return field_sq(ctx.Delta[c], ctx.p.Lx, ctx.p.Ly)
