"""The device eigensolvers (csrc/dwhmc_eig.hip one-stage, csrc/dwhmc_qeig.hip
structure-preserving) on spectra at their own thresholds (tests/eig_cases.py):
exact clusters of 4 .. 44 levels, degeneracies lifted through kEigClusterTol,
central gaps around kEigZeroTol, reducible (Delta = 0) and tiny lattices.

Every member runs dwh_eigensystem by the default route, by the one-stage
solver (DWHMC_EIG_QUAT=0) and, where stated, with every column solved
(DWHMC_EIG_HALF=0) or the one-workgroup cluster limit lowered
(DWHMC_EIG_MAX_CLUSTER=4: the long-cluster path), against LAPACK on the
oracle's H at the project's bounds:
  max|E - E_ref| <= 1e-12 (1 + max|E|),  max|H U - U E| <= 1e-11 (1 + max|E|),
  max|U^H U - I| <= 1e-12,  U finite,  no rocSOLVER solve (eig_vendor == 0).
dwh_info_t::eig_quat / eig_half / eig_long_clusters must agree with what the
CPU classification predicts wherever that does not depend on ||T|| (the
device's Gershgorin bound, in [rho, 3 rho])."""
import numpy as np
import pytest

import eig_cases as EC
from test_transport import _check_transport

pytestmark = pytest.mark.gpu

ROUTES = {"default": {}, "one-stage": {"DWHMC_EIG_QUAT": "0"}, "full": {"DWHMC_EIG_QUAT": "0", "DWHMC_EIG_HALF": "0"},
          "long": {"DWHMC_EIG_QUAT": "0", "DWHMC_EIG_MAX_CLUSTER": "4"}}
ENV = ("DWHMC_EIG_QUAT", "DWHMC_EIG_HALF", "DWHMC_EIG_MAX_CLUSTER")


def _ctx(dwhmc, p, dis):
    return dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis)


def measure(E, U, c):
    """(eigenvalue error, residual, orthogonality): the first two in units of 1 + max|E|."""
    scale = 1.0 + c.cls["rho"]
    n = c.cls["n"]
    return (float(np.max(np.abs(E - c.cls["E"]))) / scale,
            float(np.max(np.abs(c.H @ U - U * E[None, :]))) / scale,
            float(np.max(np.abs(U.conj().T @ U - np.eye(n)))))


def solve_routes(dwhmc, monkeypatch, c, routes):
    """{route: (E, U, flags)} of one context; flags: eig_quat, eig_half, the
    long clusters and rocSOLVER solves of that call."""
    ctx = _ctx(dwhmc, c.p, c.disorder)
    out = {}
    try:
        ctx.set_pairing(c.Delta)
        ctx.timing_enable(["eig_own", "eig_vendor"])
        for r in routes:
            for k in ENV:
                monkeypatch.delenv(k, raising=False)
            for k, v in ROUTES[r].items():
                monkeypatch.setenv(k, v)
            long0, vend0 = ctx.info["eig_long_clusters"], ctx.timing_read("eig_vendor")[1]
            E, U = ctx.eigensystem(0)
            info = ctx.info
            flags = dict(quat=info["eig_quat"], half=info["eig_half"], long=info["eig_long_clusters"] - long0,
                         vendor=ctx.timing_read("eig_vendor")[1] - vend0)
            out[r] = (E, U, flags)
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        out["values"] = ctx.eigensystem(0, vectors=False)[0]
    finally:
        ctx.close()
    return out


def check_member(c, out):
    scale = 1.0 + c.cls["rho"]
    for r, val in out.items():
        if r == "values":
            assert np.max(np.abs(val - c.cls["E"])) <= 1e-12 * scale, (c.name, r)
            continue
        E, U, f = val
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(E)), (c.name, r)
        dE, res, orth = measure(E, U, c)
        print(f"{c.name} {r}: dE={dE:.1e} res={res:.1e} orth={orth:.1e} {f}")
        assert f["vendor"] == 0, (c.name, r, f)
        assert dE <= 1e-12 and res <= 1e-11 and orth <= 1e-12, (c.name, r, dE, res, orth, f)
        # the path taken, where the classification fixes it
        if r == "default":
            pq = EC.predict_quat(c.cls)
            assert pq is None or f["quat"] == pq, (c.name, r, f, pq)
            if f["quat"] == 1:
                assert f["half"] == 1, (c.name, r, f)
        else:
            assert f["quat"] == 0, (c.name, r, f)
        if r == "one-stage" or (r == "default" and f["quat"] == 0):
            ph = EC.predict_half_one_stage(c.cls)
            assert ph is None or f["half"] == ph, (c.name, r, f, ph)
        if r == "full":
            assert f["half"] == 0, (c.name, r, f)
        if r == "long":
            # (a run at rho stays inside one run at the device's ||T|| >= rho)
            if c.cls["longest_run"] > 4:
                assert f["long"] >= 1, (c.name, r, f)
        elif c.cls["longest_run_hi"] <= EC.EIG_MAX_CLUSTER:
            assert f["long"] == 0, (c.name, r, f)


@pytest.mark.parametrize("name", EC.names("clean"))
def test_clean_ladder(dwhmc, oracle, monkeypatch, name):
    """Exact clusters: shells of 4 .. 16 levels, zero modes at mu = 0 with
    L % 4 == 0, the nested Fermi surface's 12 / 28 / 44 levels at zero (the
    last beyond the structure-preserving solver's crowd of 16 pairs: it
    declines, the one-stage solver meets the bounds).  "long": every cluster
    of 5+ levels through the multi-workgroup Cholesky QR."""
    c = EC.member(oracle, "clean", name)
    check_member(c, solve_routes(dwhmc, monkeypatch, c, ("default", "one-stage", "long")))


@pytest.mark.parametrize("name", EC.names("lifted"))
def test_lifted_degeneracies(dwhmc, oracle, monkeypatch, name):
    c = EC.member(oracle, "lifted", name)
    check_member(c, solve_routes(dwhmc, monkeypatch, c, ("default", "one-stage")))


def test_zero_gap_ladder(dwhmc, oracle, monkeypatch):
    """Central gaps at 0.3 .. 9 x kEigZeroTol rho: the one-stage half solve
    must take both branches over the ladder (c0 < N below the threshold, the
    partner images above it), whatever ||T|| in [rho, 3 rho] the device has."""
    seen = set()
    for c in EC.zero_gap_ladder(oracle):
        out = solve_routes(dwhmc, monkeypatch, c, ("default", "one-stage", "full"))
        check_member(c, out)
        seen.add(out["one-stage"][2]["half"])
    assert seen == {0, 1}, seen


@pytest.mark.parametrize("name", EC.names("reducible"))
def test_reducible_and_tiny(dwhmc, oracle, monkeypatch, name):
    c = EC.member(oracle, "reducible", name)
    check_member(c, solve_routes(dwhmc, monkeypatch, c, ("default", "one-stage", "full")))


def test_family_conditions_on_device(oracle):
    """What the device tests rely on from the families (tests/test_eig_algorithm.py
    asserts the rest): clusters of 12+ and 16+ levels, a crowd beyond 16 pairs,
    and ladder members on both sides of the split for every ||T||."""
    clean = EC.clean_ladder(oracle)
    assert max(c.cls["longest_run_away"] for c in clean) >= 16 and max(c.cls["zero_run"] for c in clean) > 32
    assert any(EC.predict_quat(c.cls) == 0 for c in clean) and any(EC.predict_quat(c.cls) == 1 for c in clean)
    assert {EC.predict_half_one_stage(c.cls) for c in EC.zero_gap_ladder(oracle)} >= {0, 1}


TRANSPORT_MEMBERS = [("clean", "clean-6x6-mu-1-d0"), ("lifted", "lift-8x8-mu0-w1e-09"),
                     ("zero", "zero-8x8-g1.1"), ("reducible", "normal-6x6-W0.5"), ("reducible", "tiny-3x2")]


@pytest.mark.parametrize("family,name", TRANSPORT_MEMBERS)
def test_transport_on_edge_spectra(dwhmc, oracle, family, name):
    """measure_transport on one member per family (<= 8 x 8) against the oracle
    at _check_transport's 1e-9 bounds."""
    O = oracle
    c = EC.member(O, family, name)
    cache, _, _ = O.evaluate(c.p, c.disorder, c.Delta)
    ref = O.measure_transport_and_spectra(cache, c.p)
    ctx = _ctx(dwhmc, c.p, c.disorder)
    try:
        ctx.set_pairing(c.Delta)
        r = ctx.measure_transport(c.p.eta, c.p.domega, c.p.omega_max)
    finally:
        ctx.close()
    _check_transport(r, ref)


def test_transport_batched_mixed_spectra(dwhmc, oracle):
    """One batched call on 4 chains of a 6 x 6 lattice: a clean Delta = 0
    matrix (runs of 12), a lifted one (w = 1e-9), and two disordered ones, so
    the per-matrix c0 and the cluster paths differ inside one launch."""
    O = oracle
    clean = EC.member(O, "clean", "clean-6x6-mu-1-d0")
    lifted = EC.member(O, "lifted", "lift-6x6-mu-1-w1e-09")
    p, N = clean.p, clean.p.N
    rng = np.random.default_rng(66)
    chains = [(clean.disorder, clean.Delta), (lifted.disorder, lifted.Delta)]
    for _ in range(2):
        dis = 0.5 * rng.standard_normal(N)
        chains.append((dis, 0.25 * np.stack([np.ones(N), -np.ones(N)], 1) * np.exp(0.3j * rng.standard_normal((N, 1)))))
    ctx = _ctx(dwhmc, p, np.stack([d for d, _ in chains]))
    try:
        ctx.set_pairing(np.stack([D for _, D in chains]))
        ctx.timing_enable(["eig_own", "eig_vendor"])
        allr = ctx.measure_transport_all(p.eta, p.domega, p.omega_max)
        vendor = ctx.timing_read("eig_vendor")[1]
    finally:
        ctx.close()
    assert vendor == 0
    for r, (dis, D) in zip(allr, chains):
        cache, _, _ = O.evaluate(p, dis, D)
        _check_transport(r, O.measure_transport_and_spectra(cache, p))
