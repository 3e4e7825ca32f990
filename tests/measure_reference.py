"""One restatement of every output of the four measurement entries
(measure_transport, measure_spectral_maps, measure_current_response,
measure_operator_response) from given eigenpairs (E, U), the lattice tables,
β, η, the grids and the operators, parameterised by the working dtype:

    np.longdouble   "the reference"
    np.float64      "the yardstick": what plain fp64 reaches on the same input
                    with no cancellation inside any branch

Both runs take the same branches.  The branch decisions are taken once, on the
fp64 inputs exactly as the device takes them:

    |E_m - E_n| < 1e-8     one fp64 subtraction of the inputs (IEEE: the device's bits)
    E_n > 0                the fp64 input
    L(-E_n) > 1e-6         (1/π)(η / (E_n² + η²)) in fp64, as k_tr_colstats forms it
    |f_n - f_m| < 1e-12    on the cancellation-free Δf below (long double)

The first two do not depend on any rounding of the device, the last two do
(the device compares its own fp64 f_n - f_m, and its own L): `ambiguous_df`
and `cut_margin` say how far the input keeps from them.

Inside a branch nothing cancels:

    f_n = logistic(-βE_n),  g_n = 1 - f_n = logistic(+βE_n)
    β f (1 - f)            = β f_n g_n
    f_n - f_m              = f_lo g_hi (-expm1(-β |E_m - E_n|)), signed; lo / hi the
                             lower / upper level of the pair
    σ(ω)                   the ordered-pair sum of the reference folded pairwise,
                             (n, m) with (m, n): 4η/N Σ_{n<m} c_nm ΔE / (a (a + 4ωΔE)),
                             a = (ω - ΔE)² + η² — the same sum, every term >= 0
    dia                    tanh(βE/2) of the library (no 1 - 2f)

U^H V U, the DFTs and every sum run in the working dtype; grid points are the
fp64 start + step·k of the device's grid_point, then promoted.

Every function returns (value, S) with S = Σ |term| of the value's final sum,
its error scale.
"""
import numpy as np

LD = np.longdouble


def _c(dt):
    return np.clongdouble if dt == LD else np.complex128


def pi_of(dt):
    return dt(4) * np.arctan(dt(1))


def logistic(x):
    """1 / (1 + exp(-x)) without overflow or cancellation, in x's dtype."""
    x = np.asarray(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def fermi(E, beta, dt):
    """(f, g) = (logistic(-βE), logistic(+βE)) in dt."""
    x = dt(beta) * np.asarray(E, dtype=np.float64).astype(dt)
    return logistic(-x), logistic(x)


def grid(start, step, count):
    """fp64 start + step·k, the product and the sum rounded one after the other."""
    return np.float64(start) + np.float64(step) * np.arange(count, dtype=np.float64)


def delta_f(E, beta, dt):
    """df[n, m] = f_n - f_m and dE[n, m] = E_m - E_n in dt, no cancellation in df."""
    E64 = np.asarray(E, dtype=np.float64)
    f, g = fermi(E64, beta, dt)
    dE = (E64[None, :] - E64[:, None]).astype(dt)          # the device's fp64 difference, promoted
    up = dE >= 0
    flo = np.where(up, f[:, None], f[None, :])
    ghi = np.where(up, g[None, :], g[:, None])
    mag = flo * ghi * (-np.expm1(-dt(beta) * np.abs(dE)))
    return np.where(up, mag, -mag), dE


class Branches:
    """The branch decisions of one (E, β, η): the same for every dtype."""

    def __init__(self, E, beta, eta=None):
        E = np.asarray(E, dtype=np.float64)
        self.E, self.beta = E, float(beta)
        self.deg = np.abs(E[None, :] - E[:, None]) < 1e-8
        self.pos = E > 0
        df, _ = delta_f(E, beta, LD)
        self.adf = np.abs(df)
        self.keep = self.adf >= LD(1e-12)
        if eta is not None:
            l0 = 0.31830988618379067154 * (eta / (E * E + eta * eta))
            self.cut = l0 > 1e-6
            self.cut_margin = float(np.min(np.abs(l0 / 1e-6 - 1.0)))

    def ambiguous_df(self):
        """pairs whose |Δf| lies within a factor 2 of the 1e-12 rule"""
        return (self.adf >= LD(0.5e-12)) & (self.adf <= LD(2e-12))


# --------------------------------------------------------------------------- operators
def bonds(p, a):
    """(neighbour j_b (0-based), hopping t_b, bond vector δ_b) of direction a."""
    nn, nnn = p.nn_table - 1, p.nnn_table - 1
    if a in ("x", 0):
        return [(nn[:, 0], p.t, (1, 0)), (nnn[:, 0], p.tp, (1, 1)), (nnn[:, 3], p.tp, (1, -1))]
    return [(nn[:, 1], p.t, (0, 1)), (nnn[:, 0], p.tp, (1, 1)), (nnn[:, 1], p.tp, (-1, 1))]


def current_q(p, a, mx, my, dt):
    """Particle block of J_a(q), q = 2π (mx/Lx, my/Ly): Jq[i, j_b] += i t_b φ_b(i),
    Jq[j_b, i] -= i t_b φ_b(i), φ_b(i) = exp(-i q·(r_i + δ_b/2)); duplicates added."""
    N = p.N
    J = np.zeros((N, N), dtype=_c(dt))
    i = np.arange(N)
    x, y = (i % p.Lx).astype(dt), (i // p.Lx).astype(dt)
    two_pi = 2 * pi_of(dt)
    for j, tb, (dx, dy) in bonds(p, a):
        ang = -(two_pi * dt(mx) / dt(p.Lx) * (x + dt(dx) / 2) + two_pi * dt(my) / dt(p.Ly) * (y + dt(dy) / 2))
        val = (-dt(tb) * np.sin(ang)) + 1j * (dt(tb) * np.cos(ang))          # i t_b e^{i ang}
        np.add.at(J, (i, j), val)
        np.add.at(J, (j, i), -val)
    return J


def nambu(V, s, dt):
    V = np.asarray(V).astype(_c(dt))
    N = V.shape[0]
    Z = np.zeros((N, N), dtype=_c(dt))
    return np.block([[V, Z], [Z, -dt(s) * V.T]])


def mat2(U, A, dt):
    """|U^H A U|² in dt; A (2N, 2N)."""
    Ud = np.asarray(U).astype(_c(dt))
    M = Ud.conj().T @ (A @ Ud)
    return M.real * M.real + M.imag * M.imag


def mat2_blocks(U, J, dt):
    """|U^H (J ⊕ J) U|² in dt; J (N, N)."""
    Ud = np.asarray(U).astype(_c(dt))
    N = J.shape[0]
    M = Ud.conj().T @ np.vstack([J @ Ud[:N], J @ Ud[N:]])
    return M.real * M.real + M.imag * M.imag


# --------------------------------------------------------------------------- pair sums
def dia(U, br, p, a, dt):
    """dia_a = (1/N) Σ_{E_n > 0} w_n tanh(βE_n/2), w_n = Σ_i Σ_b t_b 2 Re(v_i v̄_j - ū_i u_j)."""
    N = p.N
    Ud = np.asarray(U).astype(_c(dt))
    u, v = Ud[:N], Ud[N:]
    w = np.zeros(2 * N, dtype=dt)
    wa = np.zeros(2 * N, dtype=dt)
    for j, tb, _ in bonds(p, a):
        w += dt(tb) * 2 * np.real(v * np.conj(v[j]) - np.conj(u) * u[j]).sum(axis=0)
        wa += abs(dt(tb)) * 2 * (np.abs(v) * np.abs(v[j]) + np.abs(u) * np.abs(u[j])).sum(axis=0)
    th = np.tanh(dt(br.beta) * br.E.astype(dt) / 2)
    pos = br.pos
    return np.sum(w[pos] * th[pos]) / N, np.sum(wa[pos] * th[pos]) / N


def ratio(br, l, dt):
    """r_nm(l): l = 0 the reference's quotient with its 1e-8 rule, l >= 1 the Matsubara weight."""
    df, dE = delta_f(br.E, br.beta, dt)
    if l == 0:
        f, g = fermi(br.E, br.beta, dt)
        return np.where(br.deg, (dt(br.beta) * f * g)[:, None], df / np.where(br.deg, dt(1), dE))
    om = 2 * pi_of(dt) * dt(l) / dt(br.beta)
    return df * dE / (dE * dE + om * om)


def matsubara(M2, br, N, nl, dt):
    """(1/N) Σ_nm r_nm(l) M2[n, m] for l < nl; every r >= 0, so S is the value."""
    out = np.array([np.sum(ratio(br, l, dt) * M2) / N for l in range(nl)], dtype=dt)
    return out, out.copy()


def dc_conductivity(J2, br, N, eta, dt):
    f, g = fermi(br.E, br.beta, dt)
    _, dE = delta_f(br.E, br.beta, dt)
    e = dt(eta)
    v = np.sum((dt(br.beta) * f * g)[:, None] * J2 * (e / (dE * dE + e * e))) / N     # π · (1/π)
    return v, v


def _pairs_upper(M2, br, dt, only=None):
    """(c, ΔE) of the kept pairs n < m: c = (f_n - f_m) M2[n, m]"""
    df, dE = delta_f(br.E, br.beta, dt)
    iu = np.triu(br.keep if only is None else only, 1)
    return (df * M2)[iu], dE[iu]


def sigma(J2, br, N, eta, w, dt, only=None):
    """σ(ω_k) for ω > 0 by the pairwise fold (module docstring); needs |J_nm| = |J_mn|.
    only: a mask of pairs to restrict the sum to (the ambiguity allowance)."""
    c, dE = _pairs_upper(J2, br, dt, only)
    e2 = dt(eta) * dt(eta)
    out = np.empty(len(w), dtype=dt)
    for k, wk in enumerate(np.asarray(w, dtype=np.float64).astype(dt)):
        a = (wk - dE) * (wk - dE) + e2
        out[k] = np.sum(c * dE / (a * (a + 4 * wk * dE)))
    out *= 4 * dt(eta) / N
    return out, np.abs(out)


def chi2(V2, br, N, eta, w, dt, only=None):
    """χ''(ω_j) = (η/N) Σ_{kept ordered pairs} (f_n - f_m) V2[n, m] / ((ω_j - ΔE)² + η²);
    only: a mask of pairs to restrict the sum to (the ambiguity allowance)."""
    df, dE = delta_f(br.E, br.beta, dt)
    sel = br.keep if only is None else only
    c, d = (df * V2)[sel], dE[sel]
    e2 = dt(eta) * dt(eta)
    out, S = np.empty(len(w), dtype=dt), np.empty(len(w), dtype=dt)
    for j, wj in enumerate(np.asarray(w, dtype=np.float64).astype(dt)):
        t = c / ((wj - d) * (wj - d) + e2)
        out[j], S[j] = np.sum(t), np.sum(np.abs(t))
    return out * (dt(eta) / N), S * (dt(eta) / N)


def lorentz(w, E, eta, dt):
    """L[q, n] = (1/π) η / ((ω_q - E_n)² + η²)"""
    d = np.asarray(w, dtype=np.float64).astype(dt)[:, None] - np.asarray(E, dtype=np.float64).astype(dt)[None, :]
    return (1 / pi_of(dt)) * (dt(eta) / (d * d + dt(eta) * dt(eta)))


def dft2(u, Lx, Ly, dt):
    """unnormalised forward 2-D DFT of the columns of u (N, K) as Lx x Ly images, site i = x + Lx y"""
    def tw(L):
        k = np.arange(L)
        ang = -2 * pi_of(dt) * ((k[:, None] * k[None, :]) % L).astype(dt) / dt(L)
        return np.cos(ang) + 1j * np.sin(ang)
    a = np.asarray(u).astype(_c(dt)).reshape(Ly, Lx, -1)            # [y, x, n]
    a = np.einsum("kx,yxn->ykn", tw(Lx), a)
    a = np.einsum("ky,yxn->kxn", tw(Ly), a)
    return a.reshape(Ly * Lx, -1)                                   # [kx + Lx ky, n]


# --------------------------------------------------------------------------- the four entries
def transport(E, U, p, beta, eta, domega, nw, nd, omega_max, dt, br=None):
    """measure_transport's outputs: dict name -> (value, S)."""
    N = p.N
    br = br or Branches(E, beta, eta)
    Ud = np.asarray(U).astype(_c(dt))
    u = Ud[:N]
    J2 = mat2_blocks(U, current_q(p, "x", 0, 0, dt), dt)
    d, Sd = dia(U, br, p, "x", dt)
    lam, Sl = matsubara(J2, br, N, 1, dt)
    res = dict(superfluid_stiffness=(d - lam[0], Sd + Sl[0]), dc_conductivity=dc_conductivity(J2, br, N, eta, dt))
    res["optical_conductivity"] = sigma(J2, br, N, eta, grid(eta, domega, nw), dt)
    # what the pairs within a factor 2 of the Δf rule could add or take away
    res["amb_sigma"] = sigma(J2, br, N, eta, grid(eta, domega, nw), dt, only=br.ambiguous_df())[0]
    Lg = lorentz(grid(-omega_max, domega, nd), E, eta, dt)
    Wn = np.sum(u.real * u.real + u.imag * u.imag, axis=0)
    i = np.arange(N)
    sx = np.where((i % p.Lx + 1) % 2 == 0, 1, -1).astype(dt)
    sy = np.where((i // p.Lx + 1) % 2 == 0, 1, -1).astype(dt)
    wan = (np.abs(sx @ u) ** 2 + np.abs(sy @ u) ** 2) / 2 / N
    dos, dan = Lg @ Wn / N, Lg @ wan
    res["dos"], res["dos_AN"] = (dos, dos), (dan, dan)
    E_dt = np.asarray(E, dtype=np.float64).astype(dt)
    w0 = np.where(br.cut, (1 / pi_of(dt)) * (dt(eta) / (E_dt * E_dt + dt(eta) * dt(eta))), dt(0))
    uk = dft2(u, p.Lx, p.Ly, dt)
    ak = (uk.real * uk.real + uk.imag * uk.imag) @ w0 / N           # [kx + Lx ky]
    ak = ak.reshape(p.Ly, p.Lx).T
    res["A_k_omega0"] = (ak, ak)
    return res


def spectral_maps(E, U, p, eta, w, dt):
    """(ldos, akw)[q, y, x] on the frequencies w; positive sums: S is the value."""
    N = p.N
    Ud = np.asarray(U).astype(_c(dt))
    u = Ud[:N]
    Lg = lorentz(w, E, eta, dt)                                      # [q, n]
    ld = Lg @ (u.real * u.real + u.imag * u.imag).T                 # [q, i]
    uk = dft2(u, p.Lx, p.Ly, dt)
    ak = Lg @ (uk.real * uk.real + uk.imag * uk.imag).T / N
    shape = (len(w), p.Ly, p.Lx)
    return ld.reshape(shape), ak.reshape(shape)


def current_response(E, U, p, beta, a, qs, nl, dt, br=None):
    """(dia, S), (lam[q, l], S)"""
    br = br or Branches(E, beta)
    lam = np.empty((len(qs), nl), dtype=dt)
    for k, (mx, my) in enumerate(qs):
        lam[k], _ = matsubara(mat2_blocks(U, current_q(p, a, mx, my, dt), dt), br, p.N, nl, dt)
    return dia(U, br, p, a, dt), (lam, lam.copy())


def operator_response(E, U, p, beta, V, s, nl, eta, w, dt, br=None):
    """(chi[l], S), (chi2[j], S), amb[j] of one operator V (N, N dense) with spin sign s;
    amb: Σ |term| of χ'' over the pairs within a factor 2 of the Δf rule"""
    br = br or Branches(E, beta)
    V2 = mat2(U, nambu(V, s, dt), dt)
    return (matsubara(V2, br, p.N, nl, dt), chi2(V2, br, p.N, eta, w, dt),
            chi2(V2, br, p.N, eta, w, dt, only=br.ambiguous_df())[1])


def bound(ref, yard, S, n2, factor=8.0):
    """the bar: max(factor |yardstick - reference|, 2N eps S), per output value, as long double"""
    ref, yard, S = (np.asarray(x, dtype=LD) for x in (ref, yard, S))
    return np.maximum(LD(factor) * np.abs(yard - ref), LD(n2) * LD(np.finfo(np.float64).eps) * np.abs(S))


# --------------------------------------------------------------------------- inputs
def haar(n2, seed):
    """Q of a seeded complex Gaussian matrix"""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((n2, n2)) + 1j * rng.standard_normal((n2, n2)))
    return Q * (np.diagonal(R) / np.abs(np.diagonal(R)))[None, :]


def nambu_partner(col, N):
    """Θ (u; v) = (-conj(v); conj(u)): with H_BdG = [[h, D], [conj(D), -h]], h real
    symmetric and D symmetric (k_tr_assemble's layout), H Θx = -E Θx for H x = E x."""
    return np.concatenate([-np.conj(col[N:]), np.conj(col[:N])])


def ph_closed(n2, seed):
    """(U, E-pattern helper): orthonormal U whose column n2-1-n is Θ of column n.
    Built by Gram-Schmidt over (x, Θx) pairs: Θ is antiunitary with Θ² = -1, so
    x ⟂ Θx always and span{x, Θx} is Θ-invariant."""
    N = n2 // 2
    rng = np.random.default_rng(seed)
    U = np.zeros((n2, n2), dtype=np.complex128)
    done = []
    for n in range(N):
        x = rng.standard_normal(n2) + 1j * rng.standard_normal(n2)
        for _ in range(2):
            for b in done:
                x = x - b * np.vdot(b, x)
        x /= np.linalg.norm(x)
        tx = nambu_partner(x, N)
        done += [x, tx]
        U[:, n], U[:, n2 - 1 - n] = x, tx
    return U
