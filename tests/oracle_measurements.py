"""Test infrastructure beside oracle_context.py: OracleContext mixins that
answer measure_spectral_maps, measure_current_response and
measure_operator_response by numpy restatements from the oracle's eigenpairs
(LAPACK), the restatements themselves, and `simulate`, which runs a driver of
simulation.py on such a backend.  With nambu_reference.OracleNambu and
response_map_reference.OracleMap a test combines all five by multiple
inheritance.  The formulas are stated in the headers of
tests/test_spectral_maps.py, test_current_response.py and
test_operator_response.py, whose tests check the restatements."""
import dataclasses
import importlib

import numpy as np

from oracle_context import OracleContext


# --------------------------------------------------------------------------- spectral maps
class MapsRef:
    """numpy maps of one (p, disorder, Δ): the eigenpairs once, any window after."""

    def __init__(self, O, p, dis, D):
        cache, _, _ = O.evaluate(p, dis, D)
        self.O, self.p = O, p
        N = p.N
        self.E = cache.E_n.copy()
        u = cache.U[:N]                                                   # (N, 2N)
        self.w_site = np.abs(u) ** 2
        uk = np.fft.fft2(u.T.reshape(2 * N, p.Ly, p.Lx), axes=(1, 2))     # [n, ky, kx]
        self.w_k = (np.abs(uk.reshape(2 * N, N)) ** 2 / N).T              # (N, 2N), k = kx + Lx ky

    def maps(self, omega, eta=0.01):
        lam = self.O.lorentzian(omega[None, :] - self.E[:, None], eta)    # (2N, count)
        shape = (len(omega), self.p.Ly, self.p.Lx)
        return (self.w_site @ lam).T.reshape(shape), (self.w_k @ lam).T.reshape(shape)


class OracleMaps(OracleContext):
    """OracleContext + measure_spectral_maps by the numpy restatement."""

    def measure_spectral_maps(self, eta, domega, omega_max, first=0, count=None, stride=1, chain=0, deltas=None,
                              ldos=True, akw=True):
        from oracle import dwhmc_oracle as O
        omega = O.julia_range(-omega_max, domega, omega_max)[first::stride][:count]
        fields = [self.Delta[chain]] if deltas is None else list(np.asarray(deltas))
        p = dataclasses.replace(self.p, eta=eta, domega=domega, omega_max=omega_max)
        both = [MapsRef(O, p, self.dis[chain], D).maps(omega, eta) for D in fields]
        return dict(omega=omega, ldos=np.stack([m[0] for m in both]), akw=np.stack([m[1] for m in both]))


# --------------------------------------------------------------------------- current response
def bonds(p, a):
    """(neighbour j_b (0-based), hopping t_b, bond vector δ_b) of direction a."""
    nn, nnn = p.nn_table - 1, p.nnn_table - 1
    if a == "x":
        return [(nn[:, 0], p.t, (1, 0)), (nnn[:, 0], p.tp, (1, 1)), (nnn[:, 3], p.tp, (1, -1))]
    return [(nn[:, 1], p.t, (0, 1)), (nnn[:, 0], p.tp, (1, 1)), (nnn[:, 1], p.tp, (-1, 1))]


def jq(p, a, mx, my):
    """Particle block of J_a(q): the triplet sum, duplicates added."""
    N = p.N
    qx, qy = 2 * np.pi * mx / p.Lx, 2 * np.pi * my / p.Ly
    J = np.zeros((N, N), dtype=np.complex128)
    for i in range(N):
        x, y = i % p.Lx, i // p.Lx
        for j, tb, (dx, dy) in bonds(p, a):
            val = 1j * tb * np.exp(-1j * (qx * (x + dx / 2) + qy * (y + dy / 2)))
            J[i, j[i]] += val
            J[j[i], i] -= val
    return J


class CurrentRef:
    """numpy response of one (p, disorder, Δ): the eigenpairs once."""

    def __init__(self, O, p, dis, D):
        cache, _, _ = O.evaluate(p, dis, D)
        self.p, self.E, self.U, self.f = p, cache.E_n.copy(), cache.U.copy(), cache.fermi_factors.copy()

    def dia(self, a):
        p, N, E = self.p, self.p.N, self.E
        u, v = self.U[:N], self.U[N:]
        i = np.arange(N)
        w = sum(tb * 2.0 * np.real(v[i] * np.conj(v[j]) - np.conj(u[i]) * u[j]).sum(axis=0) for j, tb, _ in bonds(p, a))
        pos = E > 0
        return float(np.sum(w[pos] * np.tanh(0.5 * p.beta * E[pos]))) / N

    def lam(self, a, qs, nl):
        p, N, E, U, f = self.p, self.p.N, self.E, self.U, self.f
        u, v = U[:N], U[N:]
        dE = E[None, :] - E[:, None]                     # [n, m]: E_m - E_n
        df = f[:, None] - f[None, :]
        deg = np.abs(dE) < 1e-8
        out = np.empty((len(qs), nl))
        for k, (mx, my) in enumerate(qs):
            J = jq(p, a, mx, my)
            J2 = np.abs(U.conj().T @ np.vstack([J @ u, J @ v])) ** 2
            for l in range(nl):
                if l == 0:
                    r = np.where(deg, (p.beta * f * (1.0 - f))[:, None], df / np.where(deg, 1.0, dE))
                else:
                    r = df * dE / (dE * dE + (2 * np.pi * l / p.beta) ** 2)
                out[k, l] = float(np.sum(r * J2)) / N
        return out


class OracleResponse(OracleContext):
    """OracleContext + measure_current_response by the numpy restatement."""

    def measure_current_response(self, direction="x", q=((0, 1),), n_matsubara=1, chain=0, deltas=None):
        from oracle import dwhmc_oracle as O
        qs = [tuple(k) for k in q]
        fields = [self.Delta[chain]] if deltas is None else list(np.asarray(deltas))
        refs = [CurrentRef(O, self.p, self.dis[chain], D) for D in fields]
        dia = np.array([r.dia(direction) for r in refs])
        lam = np.stack([r.lam(direction, qs, n_matsubara) for r in refs])
        return dict(dia=float(dia[0]), lam=lam[0]) if deltas is None else dict(dia=dia, lam=lam)


# --------------------------------------------------------------------------- operator response
def grid(omega):
    return omega[0] + omega[1] * np.arange(omega[2])


def nambu(V, s):
    N = V.shape[0]
    Z = np.zeros((N, N), dtype=np.complex128)
    return np.block([[V, Z], [Z, -s * V.T]])


class OperatorRef:
    """numpy response of one (p, disorder, Δ): the eigenpairs once."""

    def __init__(self, O, p, dis, D):
        cache, _, _ = O.evaluate(p, dis, D)
        self.p, self.E, self.U, self.f = p, cache.E_n.copy(), cache.U.copy(), cache.fermi_factors.copy()

    def v2(self, V, s):
        return np.abs(self.U.conj().T @ nambu(np.asarray(V, dtype=np.complex128), s) @ self.U) ** 2

    def chi(self, V, s, nl):
        p, E, f = self.p, self.E, self.f
        dE = E[None, :] - E[:, None]                     # [n, m]: E_m - E_n
        df = f[:, None] - f[None, :]
        deg = np.abs(dE) < 1e-8
        V2 = self.v2(V, s)
        out = np.empty(nl)
        for l in range(nl):
            if l == 0:
                r = np.where(deg, (p.beta * f * (1.0 - f))[:, None], df / np.where(deg, 1.0, dE))
            else:
                r = df * dE / (dE * dE + (2 * np.pi * l / p.beta) ** 2)
            out[l] = float(np.sum(r * V2)) / p.N
        return out

    def skipped_share(self):
        df = self.f[:, None] - self.f[None, :]
        return float(np.mean(np.abs(df) < 1e-12))

    def chi2(self, V, s, w, eta, reverse=False):
        E, f = self.E, self.f
        dE = (E[None, :] - E[:, None]).ravel()
        df = (f[:, None] - f[None, :]).ravel()
        keep = np.abs(df) >= 1e-12
        c, dE = (df * self.v2(V, s).ravel())[keep], dE[keep]
        if reverse:
            c, dE = c[::-1], dE[::-1]
        out = np.empty(len(w))
        for j, wj in enumerate(np.asarray(w, dtype=np.float64)):
            x = wj - dE
            out[j] = np.pi / self.p.N * float(np.sum(c * ((1.0 / np.pi) * eta / (x * x + eta * eta))))
        return out


class OracleOperator(OracleContext):
    """OracleContext + measure_operator_response by the numpy restatement."""

    def measure_operator_response(self, ops, spin_sign=None, n_matsubara=1, omega=None, eta=None, chain=0,
                                  deltas=None):
        from oracle import dwhmc_oracle as O
        fields = [self.Delta[chain]] if deltas is None else list(np.asarray(deltas))
        refs = [OperatorRef(O, self.p, self.dis[chain], D) for D in fields]
        w = np.zeros(0) if omega is None else grid(omega)
        dense = [(v.dense(self.N), s) for v, s in zip(ops, spin_sign)]
        chi = np.stack([np.stack([r.chi(V, s, n_matsubara) for V, s in dense]) for r in refs])
        chi2 = np.stack([np.stack([r.chi2(V, s, w, eta) for V, s in dense]) for r in refs])
        if deltas is None:
            return dict(chi=chi[0], chi2=chi2[0], omega=w)
        return dict(chi=chi, chi2=chi2, omega=w)


# --------------------------------------------------------------------------- the drivers on such a backend
def simulate(dwhmc, out_dir, ctx_cls, chains=0, **kw):
    """run_simulation (chains = 0) or run_simulation_chains on the 4 x 4 model
    with hmc.FermionContext replaced by ctx_cls (None: the device's)."""
    sim = importlib.import_module(dwhmc.__name__ + ".simulation")
    hmc_mod = importlib.import_module(dwhmc.__name__ + ".hmc")
    p = dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)
    saved = hmc_mod.FermionContext
    if ctx_cls is not None:
        hmc_mod.FermionContext = ctx_cls
    try:
        if chains:
            return sim.run_simulation_chains(p, [str(out_dir / f"c{k}") for k in range(chains)],
                                             [np.random.default_rng(21 + k) for k in range(chains)], **kw)
        return sim.run_simulation(p, str(out_dir), rng=np.random.default_rng(21), verbose=False, **kw)
    finally:
        hmc_mod.FermionContext = saved
