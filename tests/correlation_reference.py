"""numpy restatement of dwh_measure_correlations (include/dwhmc.h) from given
eigenpairs, in a working dtype (np.float64, or np.longdouble for the injected
eigensystems), an OracleContext that answers measure_correlations with it,
and a Fock-space thermal average that pins the formula.

With ρ = U diag(f) U^H, ρ[x, y] = <Ψ†_y Ψ_x>, and the families' bilinears
O_A(i) = Σ_t a_{i,t} Ψ†_{r(i,t)} Ψ_{c(i,t)}, by the definition:

    m_A(i)    = Σ_t a_{i,t} ρ[c, r]
    G_AB(i,j) = Σ_{t,u} a_{i,t} conj(b_{j,u}) conj(ρ[r_A, r_B]) (δ[c_A, c_B] - ρ[c_A, c_B])
    corr[r]   = (1/N) Σ_j G(j ⊕ r, j),    local[q][r] = G(ref_q ⊕ r, ref_q)

`mean_s` / `gmat_s` / `response_s` return (value, S) in the working dtype, S the error
scale built from S_ρ = |U| diag(f) |U|^T; `mean` / `gmat` / `response` are their values.
`g_loops` is the explicit loop over terms; `gmat` is the same sum taken a site i
at a time over all terms of B at once (the tests check one against the other).
"""
import numpy as np

import measure_reference as R
from nambu_reference import NRef
from oracle_context import OracleContext


def translate_table(Lx, Ly):
    """T[r, j] = site of j ⊕ r (sites and r indexed y Lx + x)"""
    s = np.arange(Lx * Ly)
    x, y = s % Lx, s // Lx
    return ((y[None, :] + y[:, None]) % Ly) * Lx + (x[None, :] + x[:, None]) % Lx


def site_terms(fam, N):
    """per site the (row, col, val) of a LocalFamily, in the family's order"""
    site = np.asarray(fam.site)
    out = []
    for i in range(N):
        k = np.flatnonzero(site == i)
        out.append((np.asarray(fam.row)[k], np.asarray(fam.col)[k], np.asarray(fam.val)[k]))
    return out


class CorrRef(NRef):
    """mean, G, corr and local of one eigensystem (E ascending, U columns)."""

    def rho(self):
        """ρ = U diag(f) U^H (formed once)"""
        if "rho" not in self._x:
            self._x["rho"] = (self.U * self.f[None, :]) @ self.U.conj().T
        return self._x["rho"]

    def mean(self, fam):
        return self.mean_s(fam)[0]

    def g_loops(self, fa, fb):
        """G_AB(i, j) (N, N) by the explicit loop over the terms"""
        N, rho, ct = self.p.N, self.rho(), R._c(self.dt)
        A, B = site_terms(fa, N), site_terms(fb, N)
        G = np.zeros((N, N), dtype=ct)
        for i in range(N):
            for j in range(N):
                acc = ct(0)
                for ra, ca, a in zip(*A[i]):
                    for rb, cb, b in zip(*B[j]):
                        acc += ct(a) * np.conj(ct(b)) * np.conj(rho[ra, rb]) * ((1 if ca == cb else 0) - rho[ca, cb])
                G[i, j] = acc
        return G

    def srho(self):
        """S_ρ = |U| diag(f) |U|^T, the error scale of ρ's entries"""
        if "srho" not in self._x:
            A = np.abs(self.U)
            self._x["srho"] = (A * self.f[None, :]) @ A.T
        return self._x["srho"]

    def mean_s(self, fam):
        """(m_A(i), S(i)) in the working dtype, S = Σ_t |a_{i,t}| S_ρ[c, r]"""
        rho, sr, ct = self.rho(), self.srho(), R._c(self.dt)
        out, S = np.zeros(self.p.N, dtype=ct), np.zeros(self.p.N, dtype=self.dt)
        for i, (r, c, v) in enumerate(site_terms(fam, self.p.N)):
            if len(r):
                out[i], S[i] = np.sum(v.astype(ct) * rho[c, r]), np.sum(np.abs(v).astype(self.dt) * sr[c, r])
        return out, S

    def gmat_s(self, fa, fb, scale=True):
        """(G, S) (N, N) in the working dtype;
        S(i, j) = Σ_{t,u} |a| |b| S_ρ[r_A, r_B] (δ[c_A, c_B] + S_ρ[c_A, c_B]): δ + S_ρ, not
        |δ - ρ| (what of δ - ρ lies below eps is not resolved by ρ)"""
        N, rho, ct = self.p.N, self.rho(), R._c(self.dt)
        sr = self.srho() if scale else None
        A = site_terms(fa, N)
        order = np.argsort(np.asarray(fb.site), kind="stable")
        sb = np.asarray(fb.site)[order]
        rb, cb = np.asarray(fb.row)[order], np.asarray(fb.col)[order]
        vb = np.conj(np.asarray(fb.val)[order].astype(ct))
        G = np.zeros((N, N), dtype=ct)
        S = np.zeros((N, N), dtype=self.dt) if scale else None
        if len(sb) == 0:
            return G, S
        for i, (ra, ca, a) in enumerate(A):
            if len(ra) == 0:
                continue
            eq = ca[:, None] == cb[None, :]
            X = np.conj(rho[ra[:, None], rb[None, :]]) * (eq - rho[ca[:, None], cb[None, :]])
            w = (a.astype(ct)[:, None] * X).sum(axis=0) * vb
            np.add.at(G[i], sb, w)
            if scale:
                Y = sr[ra[:, None], rb[None, :]] * (eq + sr[ca[:, None], cb[None, :]])
                np.add.at(S[i], sb, (np.abs(a).astype(self.dt)[:, None] * Y).sum(axis=0) * np.abs(vb))
        return G, S

    def gmat(self, fa, fb):
        return self.gmat_s(fa, fb, scale=False)[0]

    def response_s(self, fams, pairs, ref_sites=(), scale=True):
        """dict corr (npairs, N), local (npairs, nref, N), mean (nfam, N): each (value, S) in the
        working dtype; corr's S is (1/N) Σ_j of G's, local's is G's at the reference site
        (scale=False: every S is None)"""
        p = self.p
        T = translate_table(p.Lx, p.Ly)
        j = np.arange(p.N)
        corr, local = [], []
        for a, b in pairs:
            G, S = self.gmat_s(fams[a], fams[b], scale)
            corr.append([M[T, j[None, :]].sum(axis=1) / p.N for M in (G, S) if M is not None])
            local.append([[M[T[:, q], q] for q in ref_sites] for M in (G, S) if M is not None])
        mean = [self.mean_s(f)[:2 if scale else 1] for f in fams]

        def both(parts, shape):
            out = [np.asarray([x[k] for x in parts]).reshape(shape) for k in range(2 if scale else 1)]
            return tuple(out) if scale else (out[0], None)
        return dict(corr=both(corr, (len(pairs), p.N)), local=both(local, (len(pairs), len(ref_sites), p.N)),
                    mean=both(mean, (len(fams), p.N)))

    def response(self, fams, pairs, ref_sites=()):
        """(corr (npairs, Ly, Lx), local (npairs, nref, Ly, Lx), mean (nfam, Ly, Lx)) in complex128"""
        r, shp = self.response_s(fams, pairs, ref_sites, scale=False), (self.p.Ly, self.p.Lx)
        return tuple(r[k][0].astype(np.complex128).reshape(r[k][0].shape[:-1] + shp) for k in ("corr", "local", "mean"))


class OracleCorrelations(OracleContext):
    """OracleContext + measure_correlations by the numpy restatement
    (families: objects with site, row, col, val, as vertices.local_family returns)."""

    def measure_correlations(self, families, pairs=None, ref_sites=None, mean=True, chain=0, deltas=None,
                             corr=True):
        from oracle import dwhmc_oracle as O
        fields = [self.Delta[chain]] if deltas is None else list(np.asarray(deltas))
        fams = list(families)
        pr = [(k, k) for k in range(len(fams))] if pairs is None else [tuple(int(x) for x in q) for q in pairs]
        sites = [] if ref_sites is None else [int(q) for q in ref_sites]
        res = [CorrRef.from_oracle(O, self.p, self.dis[chain], D).response(fams, pr, sites) for D in fields]
        out = dict(corr=np.stack([r[0] for r in res]) if corr else None,
                   local=np.stack([r[1] for r in res]) if ref_sites is not None else None,
                   mean=np.stack([r[2] for r in res]) if mean else None)
        if deltas is None:
            out = {k: None if v is None else v[0] for k, v in out.items()}
        return dict(out, pairs=np.asarray(pr, dtype=np.int64).reshape(-1, 2))


# --------------------------------------------------------------------------
# Fock space: n Jordan-Wigner modes, a quadratic H = Σ h[x, y] d†_x d_y
# --------------------------------------------------------------------------
def jw_modes(n):
    """annihilators d_0 .. d_{n-1} on the 2^n-dimensional Fock space"""
    a = np.array([[0.0, 1.0], [0.0, 0.0]])
    z = np.diag([1.0, -1.0])
    out = []
    for x in range(n):
        m = np.eye(1)
        for y in range(n):
            m = np.kron(m, z if y < x else a if y == x else np.eye(2))
        out.append(m.astype(np.complex128))
    return out


class FockThermal:
    """<·> = Tr(e^{-βH} ·)/Z of H = Σ h[x, y] d†_x d_y (h Hermitian, n x n)"""

    def __init__(self, h, beta):
        self.d = jw_modes(len(h))
        H = sum(h[x, y] * self.d[x].conj().T @ self.d[y] for x in range(len(h)) for y in range(len(h)))
        w, V = np.linalg.eigh(H)
        b = np.exp(-beta * (w - w.min()))
        self.dm = (V * (b / b.sum())[None, :]) @ V.conj().T

    def avg(self, O):
        return np.trace(self.dm @ O)

    def bilinear(self, r, c, v):
        """Σ_t v_t d†_{r_t} d_{c_t}"""
        O = np.zeros_like(self.dm)
        for rt, ct, vt in zip(r, c, v):
            O = O + vt * self.d[rt].conj().T @ self.d[ct]
        return O
