"""numpy restatement of dwh_measure_response_map (include/dwhmc.h) from given
eigenpairs, in a working dtype (np.float64, or np.longdouble for the injected
eigensystems), and an OracleContext that answers measure_response_map with it.

With X = U^H W U, ΔE_nm = E_m - E_n, Ω_l = 2π l/β, by the definition:

    D(z)[W] = U (w(z) ∘ X) U^H        ρ = U diag(f) U^H
    Matsubara l:  w = r(l) + i s(l), measure_reference.ratio's r (its l = 0
                  rules), s(0) = 0, s(l >= 1) = (f_n - f_m) Ω_l / (ΔE² + Ω_l²)
    retarded ω:   w = (f_n - f_m)/(ΔE - ω - iη), 0 where |f_n - f_m| < 1e-12

f_n - f_m and the branch decisions are measure_reference's (cancellation-free,
taken on the fp64 input).  `dmat` / `rho` / `response` form whole matrices and the
tests sample them; `sampled` / `rho_s` evaluate only the pattern entries and return
(value, S), S = Σ |term| of the value's sum, in the working dtype.
"""
import numpy as np

import measure_reference as R
from nambu_reference import NRef
from oracle_context import OracleContext


class MapRef(NRef):
    """D(z)[W] and ρ of one eigensystem (E ascending, U columns) as dense 2N x 2N matrices."""

    def weight(self, z, nl, omega, eta):
        """w_nm of frequency index z: Matsubara l = z below nl, else omega[z - nl]"""
        dt = self.dt
        if z < nl:
            r = R.ratio(self.br, z, dt)
            if z == 0:
                return r.astype(R._c(dt))
            om = 2 * R.pi_of(dt) * dt(z) / dt(self.beta)
            return r + 1j * (self.df * om / (self.dE * self.dE + om * om))
        a = self.dE - dt(np.float64(omega[z - nl]))
        e = dt(eta)
        w = self.df * (a + 1j * e) / (a * a + e * e)
        return np.where(self.br.keep, w, 0)

    def dmat(self, W, nl, omega=(), eta=None):
        """(nz, 2N, 2N): D(z)[W] for the nl Matsubara indices, then the frequencies omega"""
        X, U = self.x(W), self.U
        nz = nl + len(omega)
        out = np.empty((nz,) + X.shape, dtype=R._c(self.dt))
        for z in range(nz):
            out[z] = U @ ((self.weight(z, nl, omega, eta) * X) @ U.conj().T)
        return out

    def rho(self):
        return (self.U * self.f[None, :]) @ self.U.conj().T

    def sampled(self, W, pattern, nl, omega=(), eta=None):
        """(D, S) (nz, npat) in the working dtype, only at the pattern's entries and
        without forming D(z): D_e = (U[a_e, :] K_z) · conj(U[b_e, :]), one row product
        per distinct a; S_e = Σ_nm |U[a_e, n]| |w_nm(z)| |X_nm| |U[b_e, m]|"""
        X, U = self.x(W), self.U
        pat = np.asarray(pattern)
        rows, inv = np.unique(pat[:, 0], return_inverse=True)
        Ua, Ub = U[rows], np.conj(U[pat[:, 1]])
        aUa, aUb, aX = np.abs(Ua), np.abs(Ub), np.abs(X)
        nz = nl + len(omega)
        D, S = np.empty((nz, len(pat)), dtype=R._c(self.dt)), np.empty((nz, len(pat)), dtype=self.dt)
        for z in range(nz):
            w = self.weight(z, nl, omega, eta)
            D[z] = np.sum((Ua @ (w * X))[inv] * Ub, axis=1)
            S[z] = np.sum((aUa @ (np.abs(w) * aX))[inv] * aUb, axis=1)
        return D, S

    def rho_s(self, pattern):
        """(ρ[a_e, b_e], S_ρ[a_e, b_e]) in the working dtype, S_ρ = |U| diag(f) |U|^T"""
        pat = np.asarray(pattern)
        Ua, Ub = self.U[pat[:, 0]], self.U[pat[:, 1]]
        return np.sum(Ua * self.f[None, :] * np.conj(Ub), axis=1), np.sum(np.abs(Ua) * self.f[None, :] * np.abs(Ub), axis=1)

    def response(self, Ws, pattern, nl, omega=(), eta=None):
        """(dmap (nops, nz, npat), rho (npat,)) in complex128 on the pattern"""
        a, b = np.asarray(pattern)[:, 0], np.asarray(pattern)[:, 1]
        dmap = np.stack([self.dmat(W, nl, omega, eta)[:, a, b] for W in Ws]) if nl + len(omega) > 0 else None
        return (None if dmap is None else dmap.astype(np.complex128)), self.rho_s(pattern)[0].astype(np.complex128)


class OracleMap(OracleContext):
    """OracleContext + measure_response_map by the numpy restatement
    (vertices: objects with .dense(N), as vertices.build_nambu returns)."""

    def measure_response_map(self, vertices, pattern, n_matsubara=1, omega=None, eta=None, rho=True, chain=0,
                             deltas=None):
        from oracle import dwhmc_oracle as O
        fields = [self.Delta[chain]] if deltas is None else list(np.asarray(deltas))
        Ws = [v.dense(self.N) for v in vertices]
        pat = np.ascontiguousarray(np.asarray(pattern, dtype=np.int64).reshape(-1, 2))
        w = np.zeros(0) if omega is None else np.asarray(omega, dtype=np.float64).ravel()
        res = [MapRef.from_oracle(O, self.p, self.dis[chain], D).response(Ws, pat, n_matsubara, w, eta)
               for D in fields]
        dmap = None if res[0][0] is None else np.stack([r[0] for r in res])
        rh = np.stack([r[1] for r in res]) if rho else None
        if deltas is None:
            dmap, rh = (None if dmap is None else dmap[0]), (None if rh is None else rh[0])
        return dict(dmap=dmap, rho=rh, pattern=pat, omega=w)
