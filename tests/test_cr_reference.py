"""CPU tests of the machinery behind the CR kernel and per-pole GPU tests
(tests/cr_reference.py): the long-double reference, the fp64 yardsticks and
every generated input, checked without a device — the reference's residual in
long double; the generated Schur complements are M-form to rounding; on every
input the GPU tests feed, the reference's own error sits >= 1e3 below the
tolerance the GPU test applies and LAPACK's fp64 error sits below it; the
product reference agrees with tools/cr_model.top_product; and the launch
entry's host-side validation refuses bad arguments before touching a device.

The inversion tolerances checked here are the stricter ones (scalar-pivot
yardstick only); tests/test_cr_kernels.py states which one it applies.
"""
import numpy as np
import pytest

import cr_reference as R

BPS = (32, 64, 96, 128)


@pytest.mark.parametrize("BP", BPS)
def test_block_reference_and_yardsticks(BP):
    for b in R.inversion_blocks(BP):
        ref, name = b["ref"], f"BP {BP} {b['name']}"
        tol, tol_ld = R.inv_tolerances(ref, BP)
        n = BP
        # residual of the reference inverse in long double: a few n eps_ld |A| |X|
        full = ref["full"]
        scale = float(np.abs(full).sum(axis=1).max()) * ref["ymax"]
        assert ref["resid"] <= 4 * n * R.EPS_LD * max(1.0, scale), (name, ref["resid"])
        # the reference's own error >= 1e3 below the GPU tolerance; LAPACK's below it
        assert ref["e_ref"] * 1e3 <= tol, (name, ref["e_ref"], tol)
        assert R.lnabsdet_error_estimate(full, ref["lndet"]) * 1e3 <= tol_ld, name
        assert ref["e_lapack"] <= tol, (name, ref["e_lapack"], tol)
        assert ref["e_lapack_ld"] <= tol_ld, (name, ref["e_lapack_ld"], tol_ld)
        # both yardsticks invert the block (they are measured, not trusted)
        assert ref["e_yard"] <= 1e-9 * ref["ymax"] and ref["e_yard16"] <= 1e-7 * ref["ymax"], name
        # the long-double inverse of an M-form block is M-form: the top half says it all
        X, _ = R.inverse_ld(full)
        assert np.abs(R.expand(X[:BP // 2], R.M_FORM) - X).max() <= 1e3 * ref["e_ref"] + 1e-18, name


@pytest.mark.parametrize("BP", BPS)
def test_padded_blocks_have_identity_padding(BP):
    HP = BP // 2
    padded = [b for b in R.inversion_blocks(BP) if b["Lx"] < HP]
    assert len(padded) == 2
    for b in padded:
        Lx, X = b["Lx"], np.asarray(b["ref"]["inv"], dtype=np.complex128)
        want = np.zeros((HP - Lx, BP))
        want[np.arange(HP - Lx), np.arange(Lx, HP)] = 1.0
        assert np.array_equal(b["T"][Lx:], want)
        # and so has the inverse, exactly
        assert np.array_equal(X[Lx:], want)
        assert not X[:Lx, Lx:HP].any() and not X[:Lx, HP + Lx:].any()


@pytest.mark.parametrize("HP", [16, 32, 48, 64])
@pytest.mark.parametrize("y", R.Y_POLES)
def test_schur_complements_are_m_form(HP, y):
    rng = np.random.default_rng(int(HP * 1000 + y * 7))
    T, S = R.schur_block(rng, HP, y)
    smax = float(np.abs(S).max())
    # bottom half = the synthesised one to (far below) one fp64 ulp of the stored top half
    assert float(np.abs(R.expand(S[:HP], R.M_FORM) - S).max()) <= R.EPS * smax
    assert float(np.abs(T - S[:HP]).max()) <= R.EPS * smax
    # non-normal, and i S keeps a Hermitian part >= y (nothing near-singular)
    Sf = R.expand(T, R.M_FORM)
    assert np.abs(Sf @ Sf.conj().T - Sf.conj().T @ Sf).max() > 1e-3
    herm = 0.5 * (1j * Sf + (1j * Sf).conj().T)
    assert np.linalg.eigvalsh(herm).min() >= y * (1 - 1e-6) - 1e-12


@pytest.mark.parametrize("BP", BPS)
def test_product_reference_against_model(BP):
    """expand / product_stage_ref (long double) against tools/cr_model.top_product (fp64)."""
    pool = R.product_pool(BP)
    for sg, tasks in R.product_stages(BP):
        for task in tasks:
            out, cin, nt, bq = task[:4]
            ref = R.product_stage_ref(BP, 1, task, sg)
            acc = np.zeros(pool.shape[2:], dtype=np.complex128)
            for h in range(nt):
                s = R.Q_FORM if (bq >> h) & 1 else R.M_FORM
                acc += R.cr_model.top_product(pool[1, task[4 + h]], pool[1, task[8 + h]], s)
            acc = sg * acc + (pool[1, cin] if cin >= 0 else 0.0)
            assert np.abs(acc - ref).max() <= R.product_tolerance(task, BP, ref)
            assert np.array_equal(R.product_stage_ref(BP, 1, task, sg), R.product_ref(pool[1], task, sg))
            assert np.abs(ref).max() > 1.0   # O(1) operands, O(sqrt K) sums


def test_product_stage_shapes():
    """Stage B's 16 x 16 tile count is odd (partly empty last workgroup with 3
    batch items) and its windows are what the docstring says."""
    for BP in BPS:
        HP = BP // 2
        (_, A), (_, B) = R.product_stages(BP)
        n16 = sum((-(-t[13] // 16) - t[12] // 16) * (-(-t[15] // 16) - t[14] // 16) for t in B)
        assert n16 % 2 == 1 and R.PROD_NBATCH % 2 == 1
        assert sorted(t[3] for t in A) == list(range(16)) and {t[2] for t in B} == {1, 2, 3, 4}
        assert any(t[14] < HP < t[15] for t in B) and any(t[12] % 16 and t[14] % 16 for t in B)
        for t in A + B:
            assert 0 <= t[12] < t[13] <= HP and 0 <= t[14] < t[15] <= BP


@pytest.mark.parametrize("Lx,Ly,beta,ys", [(12, 5, 8.0, (np.pi / 8.0, 1.0, 60.0)), (8, 8, 8.0, (np.pi / 8.0,)),
                                           (6, 9, 1e4, (np.pi * 1e-4, 1.0))])
def test_pole_reference_and_model(oracle, Lx, Ly, beta, ys):
    """Whole-matrix reference: its error >= 1e3 below the per-pole tolerance,
    the fp64 CR model and LAPACK below it."""
    p, _, _, H = R.bdg_matrix(oracle, Lx, Ly, beta, seed=Lx + 10 * Ly)
    for y in ys:
        M = H - 1j * y * np.eye(2 * p.N)
        r = R.pole_reference(M, Lx, Ly)
        assert r["e_ref"] * 1e3 <= r["tol_G"], (y, r["e_ref"], r["tol_G"])
        assert R.lnabsdet_error_estimate(M, r["lndet"]) * 1e3 <= r["tol_ld"], y
        assert r["e_model"] <= r["tol_G"] and r["e_lapack"] <= r["tol_G"], (y, r["e_model"], r["e_lapack"])
        assert r["e_model_ld"] <= r["tol_ld"] and r["e_lapack_ld"] <= r["tol_ld"], y


@pytest.mark.parametrize("name,BP,nblk,kw", R.bad_launches(), ids=[b[0] for b in R.bad_launches()])
def test_launch_validation_is_host_side(dwhmc, name, BP, nblk, kw):
    """Every refusal happens before the device is touched: it is DWH_ERR_ARG
    (ValueError) here too, where there may be no device at all."""
    HP = max(BP, 32) // 2
    pool = np.zeros((1, nblk, HP, 2 * HP), dtype=np.complex128)
    with pytest.raises(ValueError, match="dwh_debug_cr_launch"):
        dwhmc.debug_cr_launch(BP=BP, pool=pool, ldpart=np.zeros((1, 2)), **kw)
