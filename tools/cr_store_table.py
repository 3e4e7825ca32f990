#!/usr/bin/env python3
"""Per-dispatch table of one leapfrog step: duration, bytes written, who reads them first.

    python tools/cr_store_table.py --L 32 --nbatch 12 \
        [--trace <run_kernel_trace.csv>] [--pmc <dir of a rocprofv3 --pmc WRITE_SIZE pass>]

The plan columns (host only, dwh_debug_cr_plan_stores): the bytes the launch
stores per step (all batch items) and how many launches later the first of
them is read, for the stage's own outputs and for its side products.  With
--trace / --pmc the measured duration (rocprofv3 --kernel-trace) and
WRITE_SIZE (a counter pass of its own) of the same dispatch of one step are
set beside them; a step is the launches from one k_cr_pair_force to the next.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KIND = {0: "inv", 1: "gemm", 2: "sparse fwd", 3: "sparse bwd"}
POLICY = {0: "plain", 1: "through", 2: "stream"}


def short(name):
    return name.split("(")[0].replace("void ", "").replace("dwh::", "").strip() or "k_cr_sp_fwd/bwd"


def step_of(rows, key, marker, which):
    rows = sorted(rows, key=key)
    idx = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
    return rows[idx[which - 1]:idx[which]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=32)
    ap.add_argument("--Ly", type=int, default=None)
    ap.add_argument("--nbatch", type=int, default=12, help="chains x poles")
    ap.add_argument("--trace")
    ap.add_argument("--pmc")
    ap.add_argument("--marker", default="k_cr_pair_force")
    ap.add_argument("--which", type=int, default=-2)
    a = ap.parse_args()
    import dwhmc_loader
    m = dwhmc_loader.load_package()
    lib = m._lib.load()
    cap = 256
    out = np.zeros(10 * cap, dtype=np.int64)
    ns = C.c_int64(0)
    m._lib.check(lib.dwh_debug_cr_plan_stores(a.L, a.Ly or a.L, a.nbatch, 1, 1, out.ctypes.data_as(C.c_void_p), cap,
                                              C.byref(ns)))
    st = out[:10 * ns.value].reshape(-1, 10)
    dur = wsz = None
    if a.trace:
        rows = step_of(list(csv.DictReader(open(a.trace))), lambda r: int(r["Start_Timestamp"]), a.marker, a.which)
        dur = [(short(r["Kernel_Name"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000) for r in rows]
    if a.pmc:
        rows = []
        for fn in glob.glob(os.path.join(a.pmc, "**", "*counter_collection.csv"), recursive=True):
            rows += [r for r in csv.DictReader(open(fn)) if r["Counter_Name"] == "WRITE_SIZE"]
        rows = step_of(rows, lambda r: int(r["Dispatch_Id"]), a.marker, a.which)
        wsz = [(short(r["Kernel_Name"]), float(r["Counter_Value"]) * 1024 / 1e6) for r in rows]   # KiB -> MB

    def far(d):
        return "-" if d >= 1 << 20 else f"+{d}"

    print(f"# L={a.L}x{a.Ly or a.L} nbatch={a.nbatch}: launch 0 is k_cr_pair_force, launches 1..{ns.value} the CR stages")
    print("# own / side: the stage's own outputs / its side products, MB per step by the plan; (next): of them read by")
    print("# the very next launch; first: launches until the first read of any of them")
    print("#  i kernel                  dur_us WRITE_SIZE_MB   own_MB (next) first  side_MB (next) first   store side_store")
    tot = np.zeros(4)
    for i in range(ns.value + 1):
        name = dur[i][0] if dur else (wsz[i][0] if wsz else ("k_cr_pair_force" if i == 0 else KIND[int(st[i - 1][0])]))
        d = f"{dur[i][1]:7.1f}" if dur and i < len(dur) else "      -"
        w = f"{wsz[i][1]:8.2f}" if wsz and i < len(wsz) else "       -"
        if i == 0:   # the scatter of the drifted pairing entries: read by the first launches of the next step
            print(f"{i:4d} {name:22s} {d} {w}            -      -    +1")
            continue
        k = st[i - 1]
        mb = k[[2, 8, 3, 9]] * a.nbatch / 1e6
        tot += mb
        side = f"{mb[2]:7.2f} {mb[3]:6.2f} {far(int(k[5])):>5s} " if k[3] else " " * 21
        print(f"{i:4d} {name:22s} {d} {w}      {mb[0]:7.2f} {mb[1]:6.2f} {far(int(k[4])):>5s}  {side} "
              f"{POLICY[int(k[6])]:>7s} {POLICY[int(k[7])] if k[3] else '':>10s}")
    print(f"# plan total {tot[0] + tot[2]:.1f} MB per step, of it {tot[1] + tot[3]:.1f} MB read by the very next launch")
    if wsz:
        print(f"# WRITE_SIZE total {sum(x[1] for x in wsz):.1f} MB per step")
    if dur:
        print(f"# kernel time total {sum(x[1] for x in dur):.1f} us per step")


if __name__ == "__main__":
    main()
