"""Measured accuracy of the eigensolvers on the threshold spectra of
tests/eig_cases.py: one line per family member and solver route (eigenvalue
error and residual in units of 1 + max|E|, orthogonality, the flags), the
numpy prototypes' values beside the device's.  profiles/eig_edge_spectra.txt
is its output.

  python tools/eig_edge_profile.py --proto proto.json       (CPU, ~2 min)
  python tools/eig_edge_profile.py --device device.json     (one GPU)
  DWHMC_LIB=<another build> python tools/eig_edge_profile.py --device parent.json
  python tools/eig_edge_profile.py --merge device.json proto.json [--parent parent.json] > profiles/eig_edge_spectra.txt
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402

import eig_cases as EC  # noqa: E402
from oracle import dwhmc_oracle as O  # noqa: E402


class _Env:
    """monkeypatch's setenv / delenv on os.environ."""

    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def run_device(path, skip):
    import dwhmc_loader
    import test_eig_edge_spectra as TE
    m = dwhmc_loader.load_package()
    routes = dict(clean=("default", "one-stage", "long"), lifted=("default", "one-stage"),
                  zero=("default", "one-stage", "full"), reducible=("default", "one-stage", "full"))
    rows = []
    for fam in EC.FAMILIES:
        for c in EC.FAMILIES[fam](O):
            if any(s in c.name for s in skip):
                continue
            out = TE.solve_routes(m, _Env(), c, routes[fam])   # an error ends the run here
            for r in routes[fam]:
                E, U, f = out[r]
                dE, res, orth = TE.measure(E, U, c)
                rows.append(dict(name=c.name, route=r, dE=dE, res=res, orth=orth, finite=bool(np.all(np.isfinite(U))),
                                 **{k: int(v) for k, v in f.items()}))
            rows.append(dict(name=c.name, route="values",
                             dE=float(np.max(np.abs(out["values"] - c.cls["E"]))) / (1.0 + c.cls["rho"])))
            with open(path, "w") as fh:   # kept current: a later member's error loses nothing
                json.dump(rows, fh)
    return rows


def run_proto(path):
    import eig_proto as P
    import qeig_proto as Q
    rows = []
    for fam in EC.FAMILIES:
        for c in EC.FAMILIES[fam](O):
            if c.cls["n"] > 288:
                continue
            solvers = [("eigh_bdg", P.eigh_bdg), ("eigh", P.eigh)] + ([("eigh_quat", Q.eigh_quat)] if c.p.N <= 40 else [])
            scale = 1.0 + c.cls["rho"]
            for k, f in solvers:
                E, U = f(c.H)
                rows.append(dict(name=c.name, route=k, dE=float(np.max(np.abs(E - c.cls["E"]))) / scale,
                                 res=float(np.max(np.abs(c.H @ U - U * E[None, :]))) / scale,
                                 orth=float(np.max(np.abs(U.conj().T @ U - np.eye(len(E)))))))
    with open(path, "w") as fh:
        json.dump(rows, fh)


def merge(device, proto, parent=None):
    dev, pro = json.load(open(device)), json.load(open(proto))
    by = {}
    for r in pro:
        by.setdefault(r["name"], {})[r["route"]] = r
    print("# device (MI355X): eigenvalue error and residual / (1 + max|E|), orthogonality max|U^H U - I|, flags")
    print("# (q = eig_quat, h = eig_half, long = long clusters, v = rocSOLVER solves); prototype: tools/eig_proto.py")
    print("# eigh_bdg / eigh and tools/qeig_proto.py eigh_quat (N <= 40) as res/orth; bounds 1e-12 / 1e-11 / 1e-12")
    print(f"# {'member':28s} {'route':9s} {'dE':>8s} {'res':>8s} {'orth':>8s}  q h long v | proto bdg res/orth, eigh, quat")
    worst = {}
    for r in dev:
        if r["route"] == "values":
            print(f"  {r['name']:28s} {'values':9s} {r['dE']:8.1e}")
            continue
        p = by.get(r["name"], {})
        ptxt = " ".join(f"{p[k]['res']:.0e}/{p[k]['orth']:.0e}" if k in p else "-" for k in ("eigh_bdg", "eigh", "eigh_quat"))
        print(f"  {r['name']:28s} {r['route']:9s} {r['dE']:8.1e} {r['res']:8.1e} {r['orth']:8.1e}  "
              f"{r['quat']} {r['half']} {r['long']:4d} {r['vendor']} | {ptxt}")
        fam = r["name"].split("-")[0]
        w = worst.setdefault((fam, r["route"]), [0.0, 0.0, 0.0])
        for i, k in enumerate(("dE", "res", "orth")):
            w[i] = max(w[i], r[k])
    print("# worst per family and route: dE res orth")
    for (fam, route), w in sorted(worst.items()):
        print(f"# {fam:8s} {route:9s} {w[0]:8.1e} {w[1]:8.1e} {w[2]:8.1e}")
    if parent:
        # the same run on the parent commit's library (DWHMC_LIB), for comparison
        pw = {}
        for r in json.load(open(parent)):
            if r["route"] == "values":
                continue
            w = pw.setdefault((r["name"].split("-")[0], r["route"]), [0.0, 0.0, 0.0, 0])
            for i, k in enumerate(("dE", "res", "orth")):
                w[i] = max(w[i], r[k])
            w[3] += r["vendor"]
        print("# the parent commit's library on the same members, worst per family and route: dE res orth, rocSOLVER solves")
        for (fam, route), w in sorted(pw.items()):
            print(f"# {fam:8s} {route:9s} {w[0]:8.1e} {w[1]:8.1e} {w[2]:8.1e} {w[3]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device")
    ap.add_argument("--proto")
    ap.add_argument("--skip", default="", help="comma-separated substrings of member names to leave out")
    ap.add_argument("--merge", nargs=2)
    ap.add_argument("--parent", help="with --merge: a --device run of another build (DWHMC_LIB) to summarise beside it")
    a = ap.parse_args()
    if a.device:
        run_device(a.device, [s for s in a.skip.split(",") if s])
    if a.proto:
        run_proto(a.proto)
    if a.merge:
        merge(*a.merge, parent=a.parent)
