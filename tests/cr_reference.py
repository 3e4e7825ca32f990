"""References and yardsticks of the CR kernel / per-pole tests
(tests/test_cr_kernels.py, tests/test_cr_per_pole.py, tests/test_cr_reference.py).
Pure numpy; no device, no fixtures.

High-precision reference (x86 long double, eps = 1.08e-19):
  inverse_ld   LAPACK's fp64 inverse refined by Newton steps X <- X + X (I - A X)
               with the residual I - A X accumulated in clongdouble (row-sparse
               A: only its nonzeros are multiplied); the correction X R is
               formed in fp64, which is exact to ~1e-16 |X| |R| with |R| ~ 1e-13.
               Returns the long-double residual max|I - A X| with the inverse.
  lnabsdet_ld  ln|det A| (np.longdouble) from the pivots of an LU with partial
               pivoting run in clongdouble (numpy has no long-double slogdet).
  product_ref  out = cin + sg sum_h A_h full(B_h) on top halves, the right
               operands expanded with the M-/Q-form rule and multiplied in
               clongdouble.

Yardsticks (plain fp64 restatements of what the kernels do, measured against
the reference on the same input by the tests):
  gj_unpivoted unpivoted Gauss-Jordan in complex128, scalar or 16 x 16 pivots,
               ln|det| from the pivots;
  cr_model     tools/cr_model.cr_selected_inverse on blocks_from_dense.

Generators of the synthetic blocks: level-0-like [h - i y | B] (padded with
identity like k_cr_fill) and Schur complements D1 - U D2^-1 U^H of a
particle-hole symmetric two-row system (M-form, non-normal).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import cr_model  # noqa: E402

LD = np.clongdouble
EPS = float(np.finfo(np.float64).eps)            # 2.2e-16
EPS_LD = float(np.finfo(np.longdouble).eps)      # 1.08e-19 on x86

M_FORM, Q_FORM = -1, +1


# ---------------------------------------------------------------------------
# top halves
# ---------------------------------------------------------------------------
def expand(T, s):
    """Full BP x BP block of a stored top half T = [A | B] (HP x BP):
    M-form (s = -1) [[A, B], [conj B, -conj A]], Q-form (s = +1)
    [[A, B], [-conj B, conj A]].  Keeps T's dtype."""
    n = T.shape[0]
    full = np.empty((2 * n, 2 * n), dtype=T.dtype)
    full[:n] = T
    full[n:, :n] = -s * np.conj(T[:, n:])
    full[n:, n:] = s * np.conj(T[:, :n])
    return full


def product_ref(item, task, sg):
    """Long-double reference of one product task on the blocks of one batch
    item (nblk, HP, BP): the full HP x BP top half cin + sg sum_h A_h B_h.
    task: (out, cin, nt, bq, a[4], b[4], r0, r1, c0, c1)."""
    out, cin, nt, bq = task[:4]
    a, b = task[4:8], task[8:12]
    acc = np.zeros(item.shape[1:], dtype=LD)
    for h in range(nt):
        s = Q_FORM if (bq >> h) & 1 else M_FORM
        acc += item[a[h]].astype(LD) @ expand(item[b[h]].astype(LD), s)
    acc *= sg
    if cin >= 0:
        acc += item[cin].astype(LD)
    return acc


def window_rounded(task, ts):
    """The rows / columns a task writes: its window rounded out to ts x ts tiles."""
    r0, r1, c0, c1 = task[12:16]
    return r0 // ts * ts, -(-r1 // ts) * ts, c0 // ts * ts, -(-c1 // ts) * ts


# ---------------------------------------------------------------------------
# high-precision reference
# ---------------------------------------------------------------------------
def _matmul_ld(A, X):
    """A @ X in clongdouble; a row-sparse A (BdG matrices: ~14 nonzeros per
    row) multiplies only its nonzeros."""
    n = A.shape[0]
    nz = A != 0
    width = int(nz.sum(axis=1).max())
    if width * 4 > n:
        return A.astype(LD) @ X
    order = np.argsort(~nz, axis=1, kind="stable")[:, :width]     # nonzero columns first
    vals = np.take_along_axis(A, order, axis=1).astype(LD)         # zeros pad short rows
    out = np.zeros(X.shape, dtype=LD)
    for k in range(width):
        out += vals[:, k, None] * X[order[:, k]]
    return out


def inverse_ld(A, steps=2):
    """(X, resid): the inverse of the complex128 matrix A in clongdouble and
    max|I - A X| evaluated in clongdouble."""
    A = np.asarray(A, dtype=np.complex128)
    n = A.shape[0]
    eye = np.eye(n, dtype=LD)
    X = np.linalg.inv(A).astype(LD)
    for _ in range(steps):
        R = eye - _matmul_ld(A, X)
        X = X + (X.astype(np.complex128) @ R.astype(np.complex128)).astype(LD)
    resid = float(np.abs(eye - _matmul_ld(A, X)).max())
    return X, resid


def lnabsdet_ld(A):
    """ln|det A| from the pivots of a partially pivoted LU in clongdouble."""
    U = np.array(A, dtype=LD)
    n = U.shape[0]
    ld = np.longdouble(0)
    for k in range(n):
        p = k + int(np.argmax(np.abs(U[k:, k])))
        if p != k:
            U[[k, p]] = U[[p, k]]
        piv = U[k, k]
        ld += np.log(np.abs(piv))
        if k + 1 < n:
            col = U[k + 1:, k] / piv
            live = np.nonzero(col)[0]                # band / sparse matrices: few rows change
            if live.size:
                U[k + 1 + live, k + 1:] -= col[live, None] * U[k, k + 1:][None, :]
    return ld


def inverse_error_bound(X, resid):
    """Bound on max|X - A^-1| of inverse_ld's result: A^-1 - X = X R (to first
    order) with max|R| = resid, so max|X R| <= ||X||_inf resid."""
    return float(np.abs(X).sum(axis=1).max()) * resid


def lnabsdet_error_estimate(A, ld):
    """|ld - ln|det A|| estimated from a second long-double elimination of the
    row-reversed matrix (same |det|, another pivot sequence)."""
    return float(abs(lnabsdet_ld(np.asarray(A)[::-1]) - ld))


# ---------------------------------------------------------------------------
# fp64 yardsticks
# ---------------------------------------------------------------------------
def gj_unpivoted(A, pivot=1):
    """(inverse, ln|det|) by unpivoted Gauss-Jordan in complex128 with scalar
    (pivot = 1) or pivot x pivot block pivots (each inverted by the scalar
    scheme); ln|det| = sum of ln|scalar pivots|."""
    M = np.array(A, dtype=np.complex128)
    n = M.shape[0]
    assert n % pivot == 0
    ld = 0.0
    for k in range(0, n, pivot):
        sl = slice(k, k + pivot)
        if pivot == 1:
            p = M[k, k]
            ld += np.log(np.abs(p))
            pinv = np.array([[1.0 / p]])
        else:
            pinv, l_ = gj_unpivoted(M[sl, sl], 1)
            ld += l_
        row = pinv @ M[sl, :]            # row panel X = P^-1 A_k:
        col = M[:, sl].copy()
        M -= col @ row                   # A_ij -= A_ik X_kj (rows i != k fixed up below)
        M[:, sl] = -col @ pinv           # column k <- -A_ik P^-1
        M[sl, :] = row
        M[sl, sl] = pinv
    return M, float(ld)


def model_resolvent(A, Lx, Ly):
    """tools/cr_model.py in fp64 on the 2N x 2N matrix A: (ln|det|, G) with
    G holding the block-tridiagonal part of A^-1 in A's index order and a mask
    of the entries it defines."""
    N = Lx * Ly
    Dg, U, L = cr_model.blocks_from_dense(A, Lx, Ly)
    ld, GD, GU, GL = cr_model.cr_selected_inverse(Dg, U, L)
    G = np.zeros((2 * N, 2 * N), dtype=np.complex128)
    mask = np.zeros((2 * N, 2 * N), dtype=bool)

    def idx(y):
        return np.r_[y * Lx:(y + 1) * Lx, N + y * Lx:N + (y + 1) * Lx]

    for y in range(Ly):
        yp = (y + 1) % Ly
        for (r, c, blk) in ((y, y, GD[y]), (y, yp, GU[y]), (yp, y, GL[y])):
            if blk is None:
                continue
            G[np.ix_(idx(r), idx(c))] = blk
            mask[np.ix_(idx(r), idx(c))] = True
    return float(ld), G, mask


# ---------------------------------------------------------------------------
# synthetic blocks (top halves, complex128)
# ---------------------------------------------------------------------------
def _cnormal(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def level0_block(rng, HP, y, Lx=None):
    """[h - i y | B]: h Hermitian, B complex symmetric and dense, entries
    O(1 / sqrt(Lx)) (norm ~ 2); sites Lx..HP-1 are padding as k_cr_fill writes
    it (1 on the diagonal of the A part, zero elsewhere)."""
    Lx = HP if Lx is None else Lx
    h = _cnormal(rng, Lx, Lx) / np.sqrt(2.0 * Lx)
    h = 0.5 * (h + h.conj().T)
    B = _cnormal(rng, Lx, Lx) / np.sqrt(2.0 * Lx)
    B = 0.5 * (B + B.T)
    T = np.zeros((HP, 2 * HP), dtype=np.complex128)
    T[:Lx, :Lx] = h - 1j * y * np.eye(Lx)
    T[:Lx, HP:HP + Lx] = B
    for x in range(Lx, HP):
        T[x, x] = 1.0
    return T


def coupling_block(rng, HP):
    """Top half [t | d] of an M-form off-diagonal block U = A[y, y+1] of a
    Hermitian BdG matrix (A[y+1, y] = U^H is M-form as well)."""
    return np.hstack([_cnormal(rng, HP, HP), _cnormal(rng, HP, HP)]) / np.sqrt(4.0 * HP)


def schur_block(rng, HP, y):
    """Top half of S = D1 - U D2^-1 U^H of a random particle-hole symmetric
    two-row system, formed in long double and rounded once: M-form, non-normal;
    i S keeps a Hermitian part >= y.  Also returns the full long-double S (for
    the M-form check)."""
    D1 = expand(level0_block(rng, HP, y), M_FORM).astype(LD)
    D2 = expand(level0_block(rng, HP, y), M_FORM)
    U = expand(coupling_block(rng, HP), M_FORM).astype(LD)
    D2inv, _ = inverse_ld(D2)
    S = D1 - U @ D2inv @ U.conj().T
    return np.ascontiguousarray(S[:HP].astype(np.complex128)), S


def block_reference(T):
    """Everything the inversion tests need for one M-form top half T, computed
    once: long-double inverse (top half) and ln|det|, the reference's residual,
    the scalar Gauss-Jordan yardstick's errors and LAPACK's."""
    HP = T.shape[0]
    full = expand(T, M_FORM)
    X, resid = inverse_ld(full)
    ld = lnabsdet_ld(full)
    Yy, ldy = gj_unpivoted(full, 1)
    Yb, ldb = gj_unpivoted(full, 16)
    return dict(full=full, inv=X[:HP], lndet=ld, resid=resid, e_ref=inverse_error_bound(X, resid),
                e_yard=float(np.abs(Yy - X).max()), e_yard_ld=float(abs(ldy - ld)),
                e_yard16=float(np.abs(Yb - X).max()), e_yard16_ld=float(abs(ldb - ld)),
                e_lapack=float(np.abs(np.linalg.inv(full) - X).max()),
                e_lapack_ld=float(abs(np.linalg.slogdet(full)[1] - ld)),
                ymax=float(np.abs(X).max()))


def inv_tolerances(ref, BP):
    """The issue's bars for one block: (tol on the inverse, tol on ln|det|)."""
    return (8.0 * max(ref["e_yard"], BP * EPS * ref["ymax"]),
            8.0 * max(ref["e_yard_ld"], EPS * (BP + float(abs(ref["lndet"])))))


# ---------------------------------------------------------------------------
# the inputs of tests/test_cr_kernels.py, generated once per block size and
# checked on the CPU by tests/test_cr_reference.py
# ---------------------------------------------------------------------------
# pi 1e-4: the lowest pole of the beta = 1e4 scans
Y_POLES = (np.pi * 1e-4, 0.05, 1.0, 60.0)
_BLOCKS, _POOLS = {}, {}


def inversion_blocks(BP):
    """The blocks every inversion test of block size BP draws from, each with
    its block_reference: per pole height a level-0-like block and a Schur
    complement, then two padded level-0 blocks (Lx < HP).  A list of dicts
    (name, T, Lx, ref)."""
    if BP not in _BLOCKS:
        HP = BP // 2
        rng = np.random.default_rng(1000 + BP)
        out = []
        for y in Y_POLES:
            out.append(dict(name=f"level0(y={y:.3g})", T=level0_block(rng, HP, y), Lx=HP))
            out.append(dict(name=f"schur(y={y:.3g})", T=schur_block(rng, HP, y)[0], Lx=HP))
        for y, Lx in ((Y_POLES[0], HP - 3), (Y_POLES[1], HP - 11)):
            out.append(dict(name=f"padded(y={y:.3g},Lx={Lx})", T=level0_block(rng, HP, y, Lx), Lx=Lx))
        for b in out:
            b["ref"] = block_reference(b["T"])
        _BLOCKS[BP] = out
    return _BLOCKS[BP]


# product tests: pool blocks 0..5 operands, 6 an accumulate input, 7 a
# well-conditioned block the side-work launches invert into block 8, 9..
# outputs
PROD_NBATCH, PROD_NBLK, PROD_OUT0 = 3, 9 + 16, 9


def product_pool(BP):
    """(nbatch, nblk, HP, BP) random top halves with entries in the unit
    square, different data per batch item; block 7: level-0-like at y = 1."""
    if BP not in _POOLS:
        rng = np.random.default_rng(2000 + BP)
        shape = (PROD_NBATCH, PROD_NBLK, BP // 2, BP)
        pool = rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)
        for bi in range(PROD_NBATCH):
            pool[bi, 7] = level0_block(rng, BP // 2, 1.0)
        _POOLS[BP] = dict(pool=pool, prod={})
    return _POOLS[BP]["pool"]


def product_stage_ref(BP, bi, task, sg):
    """product_ref on product_pool(BP)[bi] with the term products A_h B_h
    cached across the tests of one block size."""
    pool = product_pool(BP)
    cache = _POOLS[BP]["prod"]
    out, cin, nt, bq = task[:4]
    acc = np.zeros(pool.shape[2:], dtype=LD)
    for h in range(nt):
        s = Q_FORM if (bq >> h) & 1 else M_FORM
        key = (bi, task[4 + h], task[8 + h], s)
        if key not in cache:
            cache[key] = pool[bi, key[1]].astype(LD) @ expand(pool[bi, key[2]].astype(LD), s)
        acc += cache[key]
    acc *= sg
    if cin >= 0:
        acc += pool[bi, cin].astype(LD)
    return acc


def product_stages(BP):
    """The product launches of the contract tests, as (sign, tasks): stage A —
    16 full-window tasks of four terms, one per mix of M- and Q-form right
    operands, no accumulate input; stage B — 1..4 terms, accumulate inputs
    (another block, the output itself, none) and windows: one 16 x 16 tile, a
    window straddling the A | B boundary, two ragged ones.  Stage B's 16 x 16
    tile count is odd, so with 3 batch items the last workgroup of a 16 x 16
    launch is partly empty at 4 and at 2 tiles per workgroup."""
    HP, o = BP // 2, PROD_OUT0
    A = [(o + k, -1, 4, k, 0, 1, 2, 0, 3, 4, 5, 5, 0, HP, 0, BP) for k in range(16)]
    B = [(o + 0, 6, 1, 0b1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 16, 16, 32),
         (o + 1, o + 1, 2, 0b10, 1, 2, 0, 0, 4, 5, 0, 0, 0, HP, HP - 16, HP + 16),
         (o + 2, -1, 3, 0b101, 2, 0, 1, 0, 5, 4, 3, 0, 3, HP - 5, 7, BP - 9),
         (o + 3, -1, 4, 0b0110, 0, 1, 2, 1, 5, 3, 4, 4, 0, 5, HP - 3, HP + 2)]
    return [(+1.0, A), (-1.0, B)]


def product_tolerance(task, BP, ref):
    """tests/test_gemm.py's bar: 1e-13 sqrt(K) (1 + max|C_ref|), K = nt BP."""
    return 1e-13 * np.sqrt(task[2] * BP) * (1.0 + float(np.abs(ref).max()))


def bad_launches():
    """(name, keyword arguments of debug_cr_launch without pool / ldpart, BP,
    nblk) that dwh_debug_cr_launch must refuse on the host."""
    t = (2, -1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 16, 0, 16)
    inv = dict(blk=[0], dst=[1], slot=[0])
    return [
        ("unsupported BP", 48, 4, dict(kind="inv", **inv)),
        ("block id out of range", 64, 4, dict(kind="inv", blk=[4], dst=[1], slot=[0])),
        ("destination out of range", 64, 4, dict(kind="inv", blk=[0], dst=[-1], slot=[0])),
        ("slot out of range", 64, 4, dict(kind="inv", blk=[0], dst=[1], slot=[2])),
        ("two inversions, one destination", 64, 4, dict(kind="inv", blk=[0, 1], dst=[2, 2], slot=[0, 1])),
        ("ts=32 at BP 32", 32, 4, dict(kind="gemm", tasks=[t], ts=32, ksplit=1)),
        ("ts=32 at BP 96", 96, 4, dict(kind="gemm", tasks=[t], ts=32, ksplit=1)),
        ("ksplit=4 with ts=32", 64, 4, dict(kind="gemm", tasks=[t], ts=32, ksplit=4)),
        ("ksplit=3", 64, 4, dict(kind="gemm", tasks=[t], ts=16, ksplit=3)),
        ("operand out of range", 64, 4, dict(kind="gemm", tasks=[t[:8] + (4,) + t[9:]], ts=16)),
        ("output out of range", 64, 4, dict(kind="gemm", tasks=[(4,) + t[1:]], ts=16)),
        ("nt=5", 64, 4, dict(kind="gemm", tasks=[t[:2] + (5,) + t[3:]], ts=16)),
        ("nt=0", 64, 4, dict(kind="gemm", tasks=[t[:2] + (0,) + t[3:]], ts=16)),
        ("window past HP", 64, 4, dict(kind="gemm", tasks=[t[:13] + (33,) + t[14:]], ts=16)),
        ("window past BP", 64, 4, dict(kind="gemm", tasks=[t[:15] + (65,)], ts=16)),
        ("empty window", 64, 4, dict(kind="gemm", tasks=[t[:12] + (8, 8) + t[14:]], ts=16)),
        ("output is an operand", 64, 4, dict(kind="gemm", tasks=[(0,) + t[1:]], ts=16)),
        ("inv0 at BP 128", 128, 4, dict(kind="inv0", rblk=[2], **inv)),
        ("inv0 R block is a source", 64, 4, dict(kind="inv0", rblk=[0], **inv)),
        ("side work at BP 96", 96, 4, dict(kind="inv_side", tasks=[t], **inv)),
        ("side task writes an inverted block", 64, 4, dict(kind="inv_side", tasks=[(1,) + t[1:]], **inv)),
    ]


# ---------------------------------------------------------------------------
# per-pole reference of a whole factorisation
# ---------------------------------------------------------------------------
def pole_reference(M, Lx, Ly):
    """For M = H_BdG - i y (2N x 2N, the reference basis): the long-double
    inverse and ln|det|, the fp64 CR model's errors on the same matrix, LAPACK's,
    and the bars tol_G = 8 max(e_model, 2N eps max|G|), tol_ld =
    8 max(e_model_ld, eps (2N + |ln|det||))."""
    n2 = M.shape[0]
    X, resid = inverse_ld(M)
    ld = lnabsdet_ld(M)
    ldm, Gm, mask = model_resolvent(M, Lx, Ly)
    gmax = float(np.abs(X).max())
    e_model = float(np.abs(Gm - X)[mask].max())
    e_model_ld = float(abs(ldm - ld))
    return dict(G=X, lndet=ld, resid=resid, e_ref=inverse_error_bound(X, resid), gmax=gmax,
                e_model=e_model, e_model_ld=e_model_ld,
                e_lapack=float(np.abs(np.linalg.inv(M) - X).max()),
                e_lapack_ld=float(abs(np.linalg.slogdet(M)[1] - ld)),
                floor_G=n2 * EPS * gmax, floor_ld=EPS * (n2 + float(abs(ld))),
                tol_G=8.0 * max(e_model, n2 * EPS * gmax),
                tol_ld=8.0 * max(e_model_ld, EPS * (n2 + float(abs(ld)))))


def bdg_matrix(O, Lx, Ly, beta, seed, amp=0.3):
    """(p, disorder, Delta, H): a disordered d-wave-like case of the oracle O
    (oracle/dwhmc_oracle.py) and its Hermitian H_BdG."""
    p = O.ModelParameters(Lx, Ly, 1.0, -0.35, -1.08, 1.0, 0.05, beta, 0.8, 1.0)
    rng = np.random.default_rng(seed)
    st = O.initialize_state(p, rng)
    N = p.N
    dwave = np.stack([np.ones(N), -np.ones(N)], axis=1) * amp
    Delta = st.Delta + dwave * (1 + 0.3 * rng.standard_normal((N, 1))) * np.exp(1j * 0.2 * rng.standard_normal((N, 1)))
    cache = O.initialize_cache(p)
    O.init_static_H(cache, p, st.disorder_pot)
    O.update_H_BdG(cache, p, Delta)
    return p, st.disorder_pot, Delta, O.hermitian_from_upper(cache.H_base)
