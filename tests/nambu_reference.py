"""numpy restatement of dwh_measure_nambu_response (include/dwhmc.h) from
given eigenpairs, in a working dtype (np.float64, or np.longdouble for the
injected eigensystems), and an OracleContext that answers
measure_nambu_response with it.

With X^k = U^H W_k U, M = X^a conj(X^b), ΔE_nm = E_m - E_n, Ω_l = 2π l/β:

    chi[l]  = (1/N) Σ_nm [r_nm(l) + i s_nm(l)] M_nm
    chi2[j] = (π/N) Σ_nm (f_n - f_m) M_nm L_η(ω_j - ΔE_nm),   |f_n - f_m| >= 1e-12

r as measure_reference.ratio (the current response's rules), s_nm(0) = 0,
s_nm(l >= 1) = (f_n - f_m) Ω_l / (ΔE² + Ω_l²).  f_n - f_m and the branch
decisions are measure_reference's (cancellation-free, taken on the fp64 input).
`chi_s` / `chi2_s` / `response_s` return (value, S) in the working dtype, S = Σ |term|
of the value's sum; `chi` / `chi2` / `response` are their values in complex128.
"""
import numpy as np

import measure_reference as R
from oracle_context import OracleContext

LD = np.longdouble


class NRef:
    """Response of one eigensystem (E ascending, U columns) at inverse temperature beta."""

    def __init__(self, p, E, U, beta=None, dt=np.float64, br=None):
        self.p, self.dt = p, dt
        self.beta = float(p.beta if beta is None else beta)
        self.E = np.asarray(E, dtype=np.float64).copy()
        self.U = np.asarray(U).astype(R._c(dt))
        self.br = br or R.Branches(self.E, self.beta)      # (br: the decisions shared between two dtypes)
        self.df, self.dE = R.delta_f(self.E, self.beta, dt)
        self.f, self.g = R.fermi(self.E, self.beta, dt)
        self._x = {}

    @classmethod
    def from_oracle(cls, O, p, dis, D, dt=np.float64):
        cache, _, _ = O.evaluate(p, dis, D)
        return cls(p, cache.E_n, cache.U, dt=dt)

    def x(self, W):
        """U^H W U in the working dtype (kept per matrix object)."""
        key = id(W)
        if key not in self._x:
            Wd = np.asarray(W).astype(R._c(self.dt))
            self._x[key] = (W, self.U.conj().T @ (Wd @ self.U))
        return self._x[key][1]

    def m(self, Wa, Wb):
        return self.x(Wa) * np.conj(self.x(Wb))

    def chi_s(self, Wa, Wb, nl):
        """(chi[l], S[l]) in the working dtype; S = (1/N) Σ_nm |r_nm(l) + i s_nm(l)| |M_nm|"""
        dt, N = self.dt, self.p.N
        M = self.m(Wa, Wb)
        aM = np.abs(M)
        out, S = np.empty(nl, dtype=R._c(dt)), np.empty(nl, dtype=dt)
        for l in range(nl):
            r = R.ratio(self.br, l, dt)
            if l == 0:
                out[l], S[l] = np.sum(r * M) / N, np.sum(np.abs(r) * aM) / N
            else:
                om = 2 * R.pi_of(dt) * dt(l) / dt(self.beta)
                s = self.df * om / (self.dE * self.dE + om * om)
                out[l], S[l] = np.sum((r + 1j * s) * M) / N, np.sum(np.hypot(r, s) * aM) / N
        return out, S

    def chi(self, Wa, Wb, nl):
        return self.chi_s(Wa, Wb, nl)[0].astype(np.complex128)

    def chi2_s(self, Wa, Wb, w, eta, reverse=False):
        """(chi2[j], S[j]) in the working dtype;
        S = (η/N) Σ_kept |f_n - f_m| |M_nm| / ((ω_j - ΔE_nm)² + η²)"""
        dt, N = self.dt, self.p.N
        keep = self.br.keep
        c, d = (self.df * self.m(Wa, Wb))[keep], self.dE[keep]
        if reverse:
            c, d = c[::-1], d[::-1]
        a = np.abs(c)
        e2 = dt(eta) * dt(eta)
        out, S = np.empty(len(w), dtype=R._c(dt)), np.empty(len(w), dtype=dt)
        for j, wj in enumerate(np.asarray(w, dtype=np.float64).astype(dt)):
            t = 1 / ((wj - d) * (wj - d) + e2)
            out[j], S[j] = np.sum(c * t), np.sum(a * t)
        return out * (dt(eta) / N), S * (dt(eta) / N)

    def chi2(self, Wa, Wb, w, eta, reverse=False):
        return self.chi2_s(Wa, Wb, w, eta, reverse)[0].astype(np.complex128)

    def response_s(self, Ws, pairs, nl, w, eta):
        """((chi, S) (npairs, nl), (chi2, S) (npairs, len(w))) in the working dtype"""
        chi = [self.chi_s(Ws[a], Ws[b], nl) for a, b in pairs]
        chi2 = [self.chi2_s(Ws[a], Ws[b], w, eta) for a, b in pairs]
        return tuple((np.stack([v for v, _ in part]), np.stack([S for _, S in part])) for part in (chi, chi2))

    def response(self, Ws, pairs, nl, w, eta):
        """(chi (npairs, nl), chi2 (npairs, len(w))) of dense vertices Ws"""
        chi = np.stack([self.chi(Ws[a], Ws[b], nl) for a, b in pairs]) if nl > 0 else \
            np.zeros((len(pairs), 0), dtype=np.complex128)
        chi2 = np.stack([self.chi2(Ws[a], Ws[b], w, eta) for a, b in pairs]) if len(w) > 0 else \
            np.zeros((len(pairs), 0), dtype=np.complex128)
        return chi, chi2


def grid(omega):
    return np.zeros(0) if omega is None else R.grid(*omega)


class OracleNambu(OracleContext):
    """OracleContext + measure_nambu_response by the numpy restatement
    (vertices: objects with .dense(N), as vertices.build_nambu returns)."""

    def measure_nambu_response(self, vertices, pairs=None, n_matsubara=1, omega=None, eta=None, chain=0,
                               deltas=None):
        from oracle import dwhmc_oracle as O
        fields = [self.Delta[chain]] if deltas is None else list(np.asarray(deltas))
        Ws = [v.dense(self.N) for v in vertices]
        pr = [(k, k) for k in range(len(Ws))] if pairs is None else [tuple(q) for q in pairs]
        w = grid(omega)
        res = [NRef.from_oracle(O, self.p, self.dis[chain], D).response(Ws, pr, n_matsubara, w, eta) for D in fields]
        chi, chi2 = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        prs = np.asarray(pr, dtype=np.int64)
        if deltas is None:
            return dict(chi=chi[0], chi2=chi2[0], omega=w, pairs=prs)
        return dict(chi=chi, chi2=chi2, omega=w, pairs=prs)
