"""The write-through store as one 16-byte buffer store (st16_through,
csrc/dwhmc_device.h; DESIGN.md §4 "Store policy").

The store form changes an instruction, never a bit or an address: the GPU tests
run single launches of the two store sites that are written through — the
K-split epilogue of the 16 x 16 product kernel at every block size and the
side products of an inversion launch — through dwh_debug_cr_launch with plain
stores and with DWHMC_DEBUG_CR_STORE=1 (the buffer store), on pools whose
untouched entries are NaN sentinels, and compare the WHOLE pool bit for bit:
a wrong offset shows as a changed bystander or a missing output.  The step
path's equality against plain stores is tests/test_cr_store_policy.py.  The
host-only test checks what the 32-bit byte offsets of the form rely on: the
largest lattices dwh_create takes stay far below 2^32 bytes per batch item."""
import ctypes as C

import numpy as np
import pytest

import cr_reference as R
from test_cr_kernels import _bits

SITES = [(BP, "gemm", k) for BP in (32, 64, 96, 128) for k in (2, 4)] + [(64, "side", 1)]


def _launch(dwhmc, BP, route, ksplit, pool, sg, tasks):
    ld0 = np.full((pool.shape[0], 2), 123.5)
    if route == "side":
        tl = [t[:3] + (t[3] | (0x100 if k % 2 else 0),) + t[4:] for k, t in enumerate(tasks)]
        return dwhmc.debug_cr_launch("inv_side", BP, pool, ld0, blk=[7], dst=[8], slot=[1], tasks=tl)
    return dwhmc.debug_cr_launch("gemm", BP, pool, ld0, tasks=tasks, ts=16, ksplit=ksplit, sg=sg)


@pytest.mark.gpu
@pytest.mark.parametrize("BP,route,ksplit", SITES, ids=[f"{b}-{r}-{k}" for b, r, k in SITES])
def test_buffer_store_writes_what_plain_stores_write(dwhmc, monkeypatch, BP, route, ksplit):
    base = R.product_pool(BP)
    for sg, tasks in R.product_stages(BP):
        pool = base.copy()
        for t in tasks:
            if t[1] < 0:
                pool[:, t[0]] = complex(np.nan, np.nan)   # outside the task's window the sentinel stays
        monkeypatch.delenv("DWHMC_DEBUG_CR_STORE", raising=False)
        plain, ldp = _launch(dwhmc, BP, route, ksplit, pool, sg, tasks)
        monkeypatch.setenv("DWHMC_DEBUG_CR_STORE", "1")
        through, ldt = _launch(dwhmc, BP, route, ksplit, pool, sg, tasks)
        assert np.array_equal(_bits(plain), _bits(through))
        assert np.array_equal(ldp, ldt)
        # the launch did write: some output block differs from the upload
        assert any(not np.array_equal(_bits(plain[:, t[0]]), _bits(pool[:, t[0]])) for t in tasks)


# the widest block with the longest chain, and long chains of narrower blocks, at dwh_create's limit Lx Ly <= 9216
@pytest.mark.parametrize("Lx,Ly", [(64, 144), (48, 192), (32, 288), (17, 542), (8, 1152)])
def test_item_byte_offsets_fit_32_bits(dwhmc, Lx, Ly):
    """A batch item's pool is nblk blocks of at most 64 x 128 elements of 16 bytes."""
    lib = dwhmc.load_library()
    stats = np.zeros(6, dtype=np.int64)
    rc = lib.dwh_debug_cr_plan_check(Lx, Ly, 14, 1, 1, stats.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.dwh_last_error(None).decode()
    assert 0 < int(stats[5]) * 64 * 128 * 16 < 2 ** 31
