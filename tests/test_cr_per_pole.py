"""The assembled cyclic-reduction factorisation one pole at a time: after
set_pairing + factorize, dwh_debug_level0(refill=0) gives the matrix
H_BdG(Δ) - i y_q the factorisation consumed (pinned bit for bit to the
reference assembly by tests/test_gpu_assembly.py) and dwh_debug_cr_resolvent
what the gathers read for that pole — G12 at every pairing slot, the diagonal,
ln|det| — compared with the long-double dense inverse of that same matrix
(tests/cr_reference.py).  The pole expansion is not in the comparison, so the
bar is rounding level:
  G:       <= 8 max(e_model, 2N eps max|G_ref|)
  ln|det|: <= 8 max(e_model_ld, eps (2N + |ln|det||))
with e_model the error of tools/cr_model.py (fp64 numpy) on the same matrix.

Code paths (block size BP, lattice rows per block, switches):
  (12, 5)   BP 32, odd Ly: k_cr_inv0_32; INV0=0: k_cr_inv32; INV0=0 INV32=0: k_cr_inv<2>
  (8, 8)    BP 32, two lattice rows per block
  (20, 4)   BP 64, sparse level-0 forward / backward + side work; SIDE=0: product stages only
  (20, 6)   the same with one more level; SPARSE0=0: dense level 0; INV0=0: k_cr_inv<4> at level 0
  (20, 16)  BP 64, backward merge off (MERGE=0) and on (MERGE=8); 2N = 640: lowest pole only
  (36, 4)   BP 96: k_cr_inv0_96, sparse level 0; INV0=0 SPARSE0=0: k_cr_inv<6>, dense level 0
  (50, 3)   BP 128: k_cr_inv<8>
  (6, 9)    beta = 1e4, strict pole table (37 poles): lowest pole, y ~ pi 1e-4
  (20, 4)   two chains of different disorder: the chain stride of the batch item
  mid-trajectory: after an accepted Nt = 3 sweep the pool's level-0 matrix
  (scattered by the force kernel) and the G of the last step agree

Measured on an MI355X: RATIOS below, the largest error / max(e_model, floor)
per case (the assertion allows 8).  Before the 16 x 16 register inversion
matched its pivot step's constant to large pivots (wave_inv16_dpp; found by
these tests and tests/test_cr_kernels.py, which has the analysis) the top pole
of every lattice missed the bar on diag G by 2e-14 (ratio 12 - 50), and 20 x 6
at beta = 1000 missed it at the lowest pole (G 8 - 15, ln|det| 12).
"""
import hashlib

import numpy as np
import pytest

import cr_reference as R

pytestmark = pytest.mark.gpu

# largest observed error / max(model error, floor) on an MI355X: (G, ln|det|)
RATIOS = {
    "12x5": (0.05, 0.26), "12x5 INV0=0": (0.05, 0.21), "12x5 INV0=0 INV32=0": (0.04, 0.18), "8x8": (0.04, 0.43),
    "20x4 b100": (2.40, 2.07), "20x4 b100 SIDE=0": (2.40, 2.07), "20x6 b1000": (2.60, 2.21),
    "20x6 b1000 SPARSE0=0": (4.69, 0.65), "20x6 b1000 INV0=0": (1.97, 0.34),
    "20x16 MERGE=0": (0.01, 0.06), "20x16 MERGE=8": (0.01, 0.06), "36x4": (0.02, 0.11),
    "36x4 INV0=0 SPARSE0=0": (0.02, 0.14), "50x3 b100": (0.14, 0.39), "6x9 b1e4 strict": (1.23, 4.82),
    "two chains": (1.61, 0.86), "mid-trajectory": (0.02, 0.25),
}

_REFS = {}


def reference(M, Lx, Ly):
    """pole_reference of the matrix M, computed once per distinct matrix."""
    key = hashlib.sha1(np.ascontiguousarray(M).tobytes()).hexdigest()
    if key not in _REFS:
        _REFS[key] = R.pole_reference(M, Lx, Ly)
    return _REFS[key]


def make_ctx(dwhmc, p, dis):
    ctx = dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis, algo="cr")
    assert ctx.info["algo"] == 1
    return ctx


def check_pole(ctx, Lx, Ly, chain, q, label):
    """Read back pole q of `chain`; returns (ratio_G, ratio_ld, failures)."""
    N = Lx * Ly
    M, y = ctx.debug_level0(chain, q, refill=False)
    res = ctx.debug_cr_resolvent(chain, q)
    assert np.array_equal(res["y"], y)
    assert np.array_equal(np.diag(M).imag[:N], np.full(N, -y[q]))
    ref = reference(M, Lx, Ly)
    G = ref["G"]
    cols = res["cols"]
    fails = []
    # the slots are the pairing pattern of the matrix, nothing else
    for i in range(N):
        assert set(cols[i][cols[i] >= 0]) == set(np.nonzero(M[i, N:])[0]), f"{label}: pairing slots of site {i}"
    used = cols >= 0
    assert not res["G12"][~used].any()
    ii = np.nonzero(used)
    want = G[ii[0], N + cols[used]]
    d12 = np.abs(res["G12"][used].astype(R.LD) - want)
    dd = np.abs(res["diag"].astype(R.LD) - np.diag(G)[:N])
    # the stated relation: the hole diagonal is -conj of the stored particle diagonal
    assert np.abs(np.diag(G)[N:] + np.conj(np.diag(G)[:N])).max() <= 1e3 * ref["e_ref"] + 1e-18
    err_ld = float(abs(np.longdouble(res["lndet"]) - ref["lndet"]))
    yard, yard_ld = max(ref["e_model"], ref["floor_G"]), max(ref["e_model_ld"], ref["floor_ld"])
    k = int(d12.argmax())
    e12, ed = float(d12.max()), float(dd.max())
    rG, rl = max(e12, ed) / yard, err_ld / yard_ld
    print(f"{label} pole {q} (y = {y[q]:.3e}): G12 err {e12:.2e}, diag err {ed:.2e}, ratio {rG:.2f} "
          f"(model {ref['e_model']:.1e}, floor {ref['floor_G']:.1e}); ln|det| err {err_ld:.2e} ratio {rl:.2f}")
    if e12 > ref["tol_G"]:
        fails.append(f"{label} pole {q}: G12[{ii[0][k]}, {cols[used][k]}] (slot {ii[1][k]}) off by {e12:.3e} > "
                     f"{ref['tol_G']:.3e}")
    if ed > ref["tol_G"]:
        fails.append(f"{label} pole {q}: diagonal entry {int(dd.argmax())} off by {ed:.3e} > {ref['tol_G']:.3e}")
    if err_ld > ref["tol_ld"]:
        fails.append(f"{label} pole {q}: ln|det| {res['lndet']!r} off by {err_ld:.3e} > {ref['tol_ld']:.3e}")
    return rG, rl, fails


def pick_poles(P, which):
    return {"3": sorted({0, P // 2, P - 1}), "low": [0]}[which]


CASES = [
    # Lx, Ly, beta, environment, poles
    (12, 5, 8.0, {}, "3"),
    (12, 5, 8.0, {"DWHMC_CR_INV0": "0"}, "3"),
    (12, 5, 8.0, {"DWHMC_CR_INV0": "0", "DWHMC_CR_INV32": "0"}, "3"),
    (8, 8, 8.0, {}, "3"),
    (20, 4, 100.0, {}, "3"),
    (20, 4, 100.0, {"DWHMC_CR_SIDE": "0"}, "3"),
    (20, 6, 1000.0, {}, "3"),
    (20, 6, 1000.0, {"DWHMC_CR_SPARSE0": "0"}, "3"),
    (20, 6, 1000.0, {"DWHMC_CR_INV0": "0"}, "3"),
    (20, 16, 8.0, {"DWHMC_CR_MERGE": "0"}, "low"),
    (20, 16, 8.0, {"DWHMC_CR_MERGE": "8"}, "low"),
    (36, 4, 8.0, {}, "3"),
    (36, 4, 8.0, {"DWHMC_CR_INV0": "0", "DWHMC_CR_SPARSE0": "0"}, "3"),
    (50, 3, 100.0, {}, "3"),
    (6, 9, 1e4, {"DWHMC_POLE_TABLE": "strict"}, "low"),
]
SWITCHES = ("DWHMC_CR_INV0", "DWHMC_CR_INV32", "DWHMC_CR_SIDE", "DWHMC_CR_SPARSE0", "DWHMC_CR_MERGE",
            "DWHMC_CR_GEMM", "DWHMC_POLE_TABLE")


def _id(c):
    return f"{c[0]}x{c[1]}-b{c[2]:g}" + "".join(f"-{k.split('_')[-1]}={v}" for k, v in c[3].items())


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("Lx,Ly,beta,env,poles", CASES, ids=[_id(c) for c in CASES])
def test_per_pole_resolvent(dwhmc, oracle, monkeypatch, Lx, Ly, beta, env, poles):
    set_env(monkeypatch, env)
    p, dis, Delta, _ = R.bdg_matrix(oracle, Lx, Ly, beta, seed=100 * Lx + Ly)
    ctx = make_ctx(dwhmc, p, dis)
    ctx.set_pairing(Delta)
    ctx.factorize()
    P = ctx.info["npoles"]
    if env.get("DWHMC_POLE_TABLE") == "strict":
        assert P >= 30      # the strict table at beta = 1e4
    fails, worst = [], (0.0, 0.0)
    for q in pick_poles(P, poles):
        rG, rl, f = check_pole(ctx, Lx, Ly, 0, q, _id((Lx, Ly, beta, env)))
        worst = (max(worst[0], rG), max(worst[1], rl))
        fails += f
    ctx.close()
    print(f"worst ratios {_id((Lx, Ly, beta, env))}: G {worst[0]:.2f} ln|det| {worst[1]:.2f}")
    assert not fails, "\n".join(fails)


def test_per_pole_two_chains(dwhmc, oracle, monkeypatch):
    """Batch item (chain, pole): each chain's pools hold its own disorder and Δ."""
    set_env(monkeypatch, {})
    Lx, Ly, beta = 20, 4, 100.0
    cases = [R.bdg_matrix(oracle, Lx, Ly, beta, seed=300 + c) for c in range(2)]
    p = cases[0][0]
    ctx = make_ctx(dwhmc, p, np.stack([c[1] for c in cases]))
    ctx.set_pairing(np.stack([c[2] for c in cases]))
    ctx.factorize()
    P = ctx.info["npoles"]
    fails = []
    for chain in range(2):
        M, y = ctx.debug_level0(chain, P - 1, refill=False)
        assert np.array_equal(M, cases[chain][3] - 1j * y[P - 1] * np.eye(2 * p.N))
        for q in (0, P - 1):
            fails += check_pole(ctx, Lx, Ly, chain, q, f"chain {chain}")[2]
    ctx.close()
    assert not fails, "\n".join(fails)


def test_per_pole_mid_trajectory(dwhmc, oracle, monkeypatch):
    """After an accepted Nt = 3 sweep the pool holds the level-0 matrix the
    force kernel scattered (no assembly launch inside a trajectory) and the G
    the last step then produced from it: the two must be consistent per pole —
    the only place a stale pairing entry would show per pole."""
    set_env(monkeypatch, {})
    Lx, Ly, beta = 20, 6, 8.0
    O = oracle
    p, dis, Delta, _ = R.bdg_matrix(O, Lx, Ly, beta, seed=77)
    ctx = make_ctx(dwhmc, p, dis)
    ctx.set_pairing(Delta)
    ctx.factorize()
    rng = np.random.default_rng(5)
    noise = (rng.standard_normal((p.N, 2)) + 1j * rng.standard_normal((p.N, 2))) * np.sqrt(0.5)
    dt = O.calc_optimal_dt(p.beta, p.J, p.mass, 3)
    acc, _ = ctx.hmc_sweep(noise, np.array([0.0]), 3, dt, p.mass)   # u = 0: always accepted
    assert acc[0]
    D_final, _ = ctx.get_state()
    assert np.abs(D_final[0] - Delta).max() > 1e-3      # the trajectory moved Δ
    P = ctx.info["npoles"]
    fails = []
    for q in sorted({0, P // 2, P - 1}):
        fails += check_pole(ctx, Lx, Ly, 0, q, "mid-trajectory")[2]
    ctx.close()
    assert not fails, "\n".join(fails)


def test_resolvent_needs_cr_and_a_factorisation(dwhmc, oracle):
    p, dis, Delta, _ = R.bdg_matrix(oracle, 4, 4, 8.0, seed=1)
    ctx = dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis, algo="dense")
    ctx.set_pairing(Delta)
    ctx.factorize()
    with pytest.raises(dwhmc.DwhError) as e:
        ctx.debug_cr_resolvent(0, 0)
    assert e.value.code == -3
    ctx.close()
    ctx = make_ctx(dwhmc, p, dis)
    with pytest.raises(dwhmc.DwhError) as e:
        ctx.debug_cr_resolvent(0, 0)
    assert e.value.code == -3
    ctx.set_pairing(Delta)
    ctx.factorize()
    with pytest.raises(ValueError):
        ctx.debug_cr_resolvent(0, ctx.info["npoles"])
    ctx.close()
