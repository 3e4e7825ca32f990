"""Contract tests of the block cyclic-reduction kernels (csrc/dwhmc_cr.hip),
one launch at a time on synthetic blocks through dwh_debug_cr_launch, against
the long-double references of tests/cr_reference.py (whose inputs, references
and yardsticks tests/test_cr_reference.py checks on the CPU).

Which test launches which compiled kernel:
  test_inversion[32-inv32]      k_cr_inv32
  test_inversion[32-inv]        k_cr_inv<2>
  test_inversion[64|96|128-inv] k_cr_inv<4>, <6>, <8>
  test_inversion[32|64|96-inv0] k_cr_inv0_32, k_cr_inv0, k_cr_inv0_96 (their R
                                blocks by k_cr_inv32 / <4> / <6>, as at context
                                creation)
  test_inversion[64-side]       k_cr_inv_side<4> (inversion workgroups)
  test_products[BP-16:K]        k_cr_gemm16<BP, K>, BP 32 / 64 / 96 / 128, K 1 / 2 / 4
  test_products[BP-32:K]        k_cr_gemm<BP, 2, K>, BP 64 / 128, K 1 / 2
  test_products[64-side]        k_cr_inv_side<4> (side-work workgroups, 32 x 32 tiles)
k_cr_gemm<32, 2, K> and k_cr_gemm<96, 2, K> are compiled but never dispatched:
32-wide tiles would straddle A | B there, cr_gemm_config never chooses them and
the test entry refuses them (test_argument_validation).

Tolerances.  Products: tests/test_gemm.py's bar, max|dC| <= 1e-13 sqrt(nt BP)
(1 + max|C_ref|).  Inversions: max|dY| <= 8 max(e_yard, BP eps max|Y_ref|) and
|d ln|det|| <= 8 max(e_yard_ld, eps (BP + |ln|det||)) per block, with e_yard
the error of the fp64 unpivoted Gauss-Jordan yardstick on the same block
against the long-double reference.  The yardstick is run with scalar pivots
and with 16 x 16 pivots, and e_yard is the larger of the two errors: the
kernels pivot on 16 x 16 tiles, and at the lowest pole height the two schemes
differ by more than the factor 8 allows for — a principal 16 x 16 tile of
h - i y is only as well conditioned as y makes it.  On the CPU (no kernel
involved), y = pi 1e-4: BP 96 Schur block 1.8e-12 with scalar pivots vs
6.8e-10 with 16 x 16 pivots, BP 128 level-0 block 5.9e-13 vs 1.2e-11; from
y = 0.05 on the two agree within 3x.  Every run prints both ratios per block.

Measured on an MI355X: RATIOS below, the largest error / max(yardstick, floor)
per kernel family (the assertion allows 8); against the scalar-pivot yardstick
alone the same runs give up to 215 (k_cr_inv<6>) at y = pi 1e-4 and stay below
8 from y = 0.05 on.

What these tests found.  With the select-free pivot step of the 16 x 16
register inversion (inv16_step, dwhmc_device.h) in its original form, every
inversion kernel missed the bar on the y = 60 blocks by 40 - 150x: max|dY|
1.4e-14 ... 2.1e-14, always on a diagonal element of size 1/60 (k_cr_inv32,
level-0 block: element (8, 8) off by 1.43e-14; k_cr_inv<8>: 2.1e-14), i.e.
8e-13 relative, where the yardstick errs by 1e-17.  The step formed 1/piv as
piv - (1 - 1/piv)(piv + 1), which cancels for |piv| >> 1 and leaves eps |piv|
absolutely.  The per-pole tests saw the same 2e-14 on diag G at the top pole
of every lattice (ratio 12 - 50) and, through Schur-complement tiles with
large entries, 2e-13 ... 4e-13 at the lowest pole of 20 x 6 at beta = 1000
(ratio 8 - 15, ln|det| 12).  The step's constant 1 is now a power of two of
the pivots' size for tiles with a large first pivot (wave_inv16_dpp); the same
elements are off by 1e-17 and every ratio is below 6.
"""
import numpy as np
import pytest

import cr_reference as R

pytestmark = pytest.mark.gpu

# largest observed error / max(yardstick, floor) on an MI355X: (inverse, ln|det|);
# products: largest error / tolerance
RATIOS = {
    "k_cr_inv32": (1.13, 2.30), "k_cr_inv<2>": (1.67, 1.35), "k_cr_inv<4>": (0.69, 0.84),
    "k_cr_inv<6>": (1.00, 0.82), "k_cr_inv<8>": (5.57, 2.98),
    "k_cr_inv0_32": (1.32, 1.52), "k_cr_inv0": (0.62, 1.28), "k_cr_inv0_96": (1.09, 2.96),
    "k_cr_inv_side<4>": (0.69, 0.84),
    "k_cr_gemm16 / k_cr_gemm / side work": 0.001,
}

INV_KERNELS = [(32, "inv32"), (32, "inv"), (64, "inv"), (96, "inv"), (128, "inv"),
               (32, "inv0"), (64, "inv0"), (96, "inv0"), (64, "side")]
# (inversions per launch, batch items): lists of 5 with 3 items of different
# data; 3 x 7 = 21 workgroups, not a multiple of 8 (xcd_grid2d's remainder branch)
INV_SHAPES = [(5, 3), (3, 7)]
NBLK, NSLOTS = 15, 8
# permuted, non-contiguous; entries 1 and 3 in place (inv0: out of place only)
BLK = [2, 0, 3, 7, 5]
DST = {True: [9, 0, 4, 7, 11], False: [9, 10, 4, 1, 11]}
SLOT = [3, 0, 4, 1, 6]
RBLK = [12, 6, 13, 8, 14]   # inv0's scratch blocks
SENTINEL_LD = 123.5


def _bits(a):
    """The bit patterns of a complex array (NaN sentinels compare equal to themselves): shape + (2,)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64).reshape(a.shape + (2,))


def _side_task(out, a, b):
    return (out, -1, 1, 0, a, 0, 0, 0, b, 0, 0, 0, 0, 32, 0, 64)


@pytest.mark.parametrize("n,nbatch", INV_SHAPES)
@pytest.mark.parametrize("BP,kernel", INV_KERNELS, ids=[f"{b}-{k}" for b, k in INV_KERNELS])
def test_inversion(dwhmc, BP, kernel, n, nbatch):
    HP = BP // 2
    blocks = R.inversion_blocks(BP)
    inplace_ok = kernel != "inv0"
    blk, dst, slot = BLK[:n], DST[inplace_ok][:n], SLOT[:n]
    rblk = RBLK[:n]
    rng = np.random.default_rng(BP + n)
    pool = rng.uniform(-1, 1, (nbatch, NBLK, HP, BP)) + 1j * rng.uniform(-1, 1, (nbatch, NBLK, HP, BP))
    which = {}
    for bi in range(nbatch):
        for i, b in enumerate(blk):
            which[bi, i] = blocks[(bi * n + i) % len(blocks)]      # every block of the set, different per item
            pool[bi, b] = which[bi, i]["T"]
    ld0 = np.full((nbatch, NSLOTS), SENTINEL_LD)
    kw = dict(blk=blk, dst=dst, slot=slot)
    touched = set(dst)
    if kernel == "inv0":
        kw.update(kind="inv0", rblk=rblk)
        touched |= set(rblk)
    elif kernel == "side":
        kw.update(kind="inv_side", tasks=[_side_task(13, 12, 6)])
        touched.add(13)
    else:
        kw.update(kind="inv", inv32=(kernel == "inv32"))
    got, ld = dwhmc.debug_cr_launch(BP=BP, pool=pool, ldpart=ld0, **kw)

    worst = dict(inv=0.0, inv_scalar=0.0, ld=0.0)
    fails = []
    for bi in range(nbatch):
        for i in range(n):
            b = which[bi, i]
            ref, name = b["ref"], f"{kernel} BP {BP} item {bi} block {blk[i]}->{dst[i]} {b['name']}"
            e_y, e_yl = max(ref["e_yard"], ref["e_yard16"]), max(ref["e_yard_ld"], ref["e_yard16_ld"])
            floor, floor_ld = BP * R.EPS * ref["ymax"], R.EPS * (BP + float(abs(ref["lndet"])))
            d = np.abs(got[bi, dst[i]].astype(R.LD) - ref["inv"])
            err, at = float(d.max()), np.unravel_index(int(d.argmax()), d.shape)
            err_ld = float(abs(np.longdouble(ld[bi, slot[i]]) - ref["lndet"]))
            r, rs = err / max(e_y, floor), err / max(ref["e_yard"], floor)
            rl = err_ld / max(e_yl, floor_ld)
            print(f"{name}: err {err:.2e} at {at} ratio {r:.2f} (scalar yardstick only: {rs:.2f}); "
                  f"ln|det| err {err_ld:.2e} ratio {rl:.2f}")
            worst = dict(inv=max(worst["inv"], r), inv_scalar=max(worst["inv_scalar"], rs), ld=max(worst["ld"], rl))
            if r > 8.0:
                fails.append(f"{name}: max|dY| {err:.3e} at element {at} = {r:.1f} x max(yardstick {e_y:.2e}, "
                             f"floor {floor:.2e})")
            if rl > 8.0:
                fails.append(f"{name}: ln|det| slot {slot[i]} off by {err_ld:.3e} = {rl:.1f} x "
                             f"max(yardstick {e_yl:.2e}, floor {floor_ld:.2e})")
            Lx = b["Lx"]
            if Lx < HP:   # padding comes back exactly identity / zero
                want = np.zeros((HP - Lx, BP))
                want[np.arange(HP - Lx), np.arange(Lx, HP)] = 1.0
                X = got[bi, dst[i]]
                if not (np.array_equal(X[Lx:], want) and not X[:Lx, Lx:HP].any() and not X[:Lx, HP + Lx:].any()):
                    fails.append(f"{name}: padded rows / columns of the inverse are not exactly identity / zero")
    print(f"worst ratios {kernel} BP {BP}: {worst}")
    assert not fails, "\n".join(fails)
    # unused ln|det| slots untouched; every block that is neither a destination
    # nor scratch (inv0's R blocks, the side task's output) bit-identical
    unused = [s for s in range(NSLOTS) if s not in slot]
    assert np.array_equal(ld[:, unused], ld0[:, unused])
    keep = [b for b in range(NBLK) if b not in touched]
    assert np.array_equal(_bits(got[:, keep]), _bits(pool[:, keep]))


PROD_CONFIGS = ([(BP, "gemm16", 16, k) for BP in (32, 64, 96, 128) for k in (1, 2, 4)]
                + [(BP, "gemm", 32, k) for BP in (64, 128) for k in (1, 2)] + [(64, "side", 32, 1)])


@pytest.mark.parametrize("BP,route,ts,ksplit", PROD_CONFIGS,
                         ids=[f"{b}-{'side' if r == 'side' else f'{t}:{k}'}" for b, r, t, k in PROD_CONFIGS])
def test_products(dwhmc, BP, route, ts, ksplit):
    HP = BP // 2
    base = R.product_pool(BP)
    nbatch = base.shape[0]
    worst, fails = 0.0, []
    for stage, (sg, tasks) in enumerate(R.product_stages(BP)):
        pool = base.copy()
        for t in tasks:
            if t[1] < 0:
                pool[:, t[0]] = complex(np.nan, np.nan)     # no accumulate input: the sentinel must not leak
        ld0 = np.full((nbatch, 2), SENTINEL_LD)
        if route == "side":
            # side-work task lists carry their own sign: alternate them
            signs = [sg if k % 2 == 0 else -sg for k in range(len(tasks))]
            tl = [t[:3] + (t[3] | (0x100 if s < 0 else 0),) + t[4:] for t, s in zip(tasks, signs)]
            got, ld = dwhmc.debug_cr_launch("inv_side", BP, pool, ld0, blk=[7], dst=[8], slot=[1], tasks=tl)
        else:
            signs = [sg] * len(tasks)
            got, ld = dwhmc.debug_cr_launch("gemm", BP, pool, ld0, tasks=tasks, ts=ts, ksplit=ksplit, sg=sg)
        written = {t[0] for t in tasks} | ({8} if route == "side" else set())
        for bi in range(nbatch):
            for t, s in zip(tasks, signs):
                ref = R.product_stage_ref(BP, bi, t, s)
                r0, r1, c0, c1 = R.window_rounded(t, ts)
                win = np.zeros((HP, BP), dtype=bool)
                win[r0:r1, c0:c1] = True
                d = np.where(win, np.abs(got[bi, t[0]].astype(R.LD) - ref), 0.0)
                d = np.where(np.isnan(d), np.inf, d)
                err, at = float(d.max()), np.unravel_index(int(d.argmax()), d.shape)
                tol = R.product_tolerance(t, BP, ref)
                worst = max(worst, err / tol)
                name = f"{route} {ts}:{ksplit} BP {BP} stage {stage} item {bi} task out={t[0]} nt={t[2]} bq={t[3]:#x}"
                if not err <= tol:
                    fails.append(f"{name}: max|dC| {err:.3e} at element {at} > {tol:.3e}")
                # outside the (rounded-out) window the output block is what was uploaded
                if not np.array_equal(_bits(got[bi, t[0]])[~win], _bits(pool[bi, t[0]])[~win]):
                    fails.append(f"{name}: output block changed outside rows {r0}:{r1} columns {c0}:{c1}")
        keep = [b for b in range(pool.shape[1]) if b not in written]
        assert np.array_equal(_bits(got[:, keep]), _bits(pool[:, keep])), "an operand or bystander block changed"
        if route == "side":
            ref7 = R.block_reference(base[0, 7])
            assert np.abs(got[0, 8] - ref7["inv"]).max() <= R.inv_tolerances(ref7, BP)[0]
            assert np.array_equal(ld[:, 0], ld0[:, 0])
        else:
            assert np.array_equal(ld, ld0)
    print(f"worst error / tolerance {route} {ts}:{ksplit} BP {BP}: {worst:.3f}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,BP,nblk,kw", R.bad_launches(), ids=[b[0] for b in R.bad_launches()])
def test_argument_validation(dwhmc, name, BP, nblk, kw):
    """DWH_ERR_ARG with no launch (tests/test_cr_reference.py runs the same
    refusals where there is no device at all)."""
    HP = max(BP, 32) // 2
    rng = np.random.default_rng(3)
    pool = rng.uniform(-1, 1, (1, nblk, HP, 2 * HP)) + 0j
    with pytest.raises(ValueError, match="dwh_debug_cr_launch"):
        dwhmc.debug_cr_launch(BP=BP, pool=pool, ldpart=np.zeros((1, 2)), **kw)
