"""Site- and momentum-resolved spectral maps (dwh_measure_spectral_maps,
csrc/dwhmc_spectral.hip):

    LDOS(i, ω) = Σ_n |u_n(i)|² L(ω - E_n)
    A(k, ω)    = (1/N) Σ_n |û_n(k)|² L(ω - E_n)

on a window first + q·stride, q < count, of the DOS grid -ω_max:Δω:ω_max.

The reference values are a numpy restatement here (`_Ref`): E, U from the
oracle's `evaluate` (LAPACK), Λ = lorentzian(ω[None, :] - E[:, None], η),
ldos = |U[:N]|² @ Λ, akw = |fft2(u.reshape(Ly, Lx))|²/N @ Λ.  Tolerance: the
project's spectra tolerance max|Δ| ≤ 1e-9 (1 + max|ref|) (tests/test_transport.py
header).  Both maps are sums over eigenstates of functions of E_n weighted by
sums that are basis-invariant inside degenerate levels, so eigenvector phases
and the solver's basis inside a degenerate level do not enter.

CPU (not gpu): the host-only window entry, the argument checks that need no
device, the bin accumulator and the driver option on the oracle backend.
GPU: parity on lattices below / at / above the 16-row MFMA tile with row and
K tails, both routes (DWHMC_SPECTRAL_FUSED unset / 0 and the fused kernel, 1), the sum rules
against the existing measurement, degenerate and particle-hole-half spectra,
snapshots, options, errors and the simulation driver.
"""
import ctypes as C
import importlib
import os
import types

import numpy as np
import pytest

from oracle_measurements import MapsRef as _Ref, OracleMaps as _OracleMaps, simulate as _simulate

T, TP, MU = 1.0, -0.35, -1.08
ETA, DW, WMAX = 0.01, 0.002, 4.0      # the default grid: 4001 DOS points
ND = 4001
TOL = 1e-9


def _case(O, Lx, Ly, beta, seed, W=1.0, nimp=0.1, amp=0.25, mu=MU):
    p = O.ModelParameters(Lx, Ly, T, TP, mu, W, nimp, beta, 0.8, 1.0)
    rng = np.random.default_rng(seed)
    st = O.initialize_state(p, rng)
    N = p.N
    D = st.Delta + amp * np.stack([np.ones(N), -np.ones(N)], 1) * np.exp(0.3j * rng.standard_normal((N, 1)))
    return p, st.disorder_pot, D


def _close(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.max(np.abs(a - b)))
    assert err <= TOL * (1 + float(np.max(np.abs(b)))), (what, err)


def _ctx(dwhmc, p, dis, **kw):
    return dwhmc.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis, **kw)


def _grid(O):
    return O.julia_range(-WMAX, DW, WMAX)


# --------------------------------------------------------------------------- CPU
def test_spectral_window_matches_julia_range(dwhmc, oracle):
    g = _grid(oracle)
    assert len(g) == ND
    for first, count, stride in ((0, ND, 1), (0, 1, 1), (3, 37, 37), (ND - 1, 1, 1), (0, 81, 50), (7, 400, 10)):
        w = dwhmc.spectral_window(ETA, DW, WMAX, first, count, stride)
        assert np.array_equal(w, g[first::stride][:count]), (first, count, stride)
    # count=None: to the end of the grid, a length that is no multiple of the stride
    assert np.array_equal(dwhmc.spectral_window(ETA, DW, WMAX, 2, None, 7), g[2::7])
    assert len(g[2::7]) * 7 != ND - 2
    # another grid (41 points), stride 4 from 1
    g2 = oracle.julia_range(-2.0, 0.1, 2.0)
    assert len(g2) == 41
    assert np.array_equal(dwhmc.spectral_window(0.05, 0.1, 2.0, 1, None, 4), g2[1::4])
    assert np.array_equal(dwhmc.spectral_window(0.05, 0.1, 2.0, 1, 10, 4), g2[1::4][:10])


def test_spectral_window_errors(dwhmc):
    lib = dwhmc.load_library()
    for first, count, stride in ((0, ND + 1, 1), (ND, 1, 1), (3, 110, 37), (1, 2001, 2), (0, 0, 1), (0, 1, 0),
                                 (-1, 1, 1), (0, -3, 1)):
        assert lib.dwh_spectral_window(ETA, DW, WMAX, first, count, stride, None) == -1, (first, count, stride)
        assert lib.dwh_last_error(None)
        with pytest.raises(ValueError):
            dwhmc.spectral_window(ETA, DW, WMAX, first, count, stride)
    # the last window that fits, with no output array
    assert lib.dwh_spectral_window(ETA, DW, WMAX, 3, 109, 37, None) == 0
    assert lib.dwh_spectral_window(ETA, DW, WMAX, 0, 2001, 2, None) == 0
    assert lib.dwh_spectral_window(-1.0, DW, WMAX, 0, 1, 1, None) == -1


def test_measure_spectral_maps_null_context(dwhmc):
    lib = dwhmc.load_library()
    out = np.zeros(4)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.dwh_measure_spectral_maps(None, 0, 1, None, ETA, DW, WMAX, 0, 1, 1, p, p) == -1
    assert b"NULL" in lib.dwh_last_error(None)
    assert "spectral" in dwhmc.FermionContext.TIMERS


def _fake_spec(rng, nw=5, nd=7, N=6):
    return types.SimpleNamespace(optical_conductivity=rng.random(nw), dos=rng.random(nd), dos_AN=rng.random(nd),
                                 A_k_omega0=rng.random((3, 2)))


def test_bins_accumulate_maps(dwhmc, tmp_path):
    sim = importlib.import_module(dwhmc.__name__ + ".simulation")
    rng = np.random.default_rng(3)
    specs = [_fake_spec(rng) for _ in range(3)]
    maps = [dict(ldos=rng.random((4, 2, 3)), akw=rng.random((4, 2, 3))) for _ in range(3)]
    first = {k: maps[0][k].copy() for k in ("ldos", "akw")}
    b = sim.SpectraBins()
    for s, m in zip(specs, maps):
        n = b.add(s, m)
    assert n == 3
    b.flush(str(tmp_path), 9)
    z = np.load(tmp_path / "sweep_9.npz")
    assert sorted(z.files) == ["A_k0", "akw", "count", "dos", "dos_AN", "ldos", "opt_cond"]
    assert int(z["count"]) == 3
    for k in ("ldos", "akw"):
        assert np.array_equal(maps[0][k], first[k])            # the caller's arrays were not summed into
        assert np.array_equal(z[k], (maps[0][k] + maps[1][k] + maps[2][k]) / 3)
    assert np.array_equal(z["dos"], (specs[0].dos + specs[1].dos + specs[2].dos) / 3)
    # without maps the group holds what it always held
    for s in specs:
        b.add(s)
    b.flush(str(tmp_path), 12)
    assert sorted(np.load(tmp_path / "sweep_12.npz").files) == ["A_k0", "count", "dos", "dos_AN", "opt_cond"]


SIM_KW = dict(n_therm=4, n_measure=4, Nt_therm_init=2, Nt_measure=3, bin_size=2)
SIM_WIN = dict(first=1000, count=5, stride=500)


def _check_sim_outputs(with_maps, without, Lx=4, Ly=4):
    for f in ("observables.csv", "transport.csv"):
        assert (with_maps / f).read_bytes() == (without / f).read_bytes(), f
    assert sorted(os.listdir(without / "spectra_bins")) == ["omega_grid.npy", "params.json", "sweep_2.npz",
                                                            "sweep_4.npz"]
    assert sorted(os.listdir(with_maps / "spectra_bins")) == ["maps_omega.npy", "omega_grid.npy", "params.json",
                                                              "sweep_2.npz", "sweep_4.npz"]
    for f in ("omega_grid.npy", "params.json"):
        assert (with_maps / "spectra_bins" / f).read_bytes() == (without / "spectra_bins" / f).read_bytes(), f
    w = np.load(with_maps / "spectra_bins" / "maps_omega.npy")
    idx = SIM_WIN["first"] + SIM_WIN["stride"] * np.arange(SIM_WIN["count"])
    assert np.array_equal(w, (-WMAX + DW * np.arange(ND))[idx])
    for n in ("sweep_2.npz", "sweep_4.npz"):
        a, b = np.load(with_maps / "spectra_bins" / n), np.load(without / "spectra_bins" / n)
        assert sorted(b.files) == ["A_k0", "count", "dos", "dos_AN", "opt_cond"]
        assert sorted(a.files) == sorted(b.files + ["ldos", "akw"])
        for k in b.files:
            assert a[k].tobytes() == b[k].tobytes(), (n, k)
        assert a["ldos"].shape == a["akw"].shape == (SIM_WIN["count"], Ly, Lx)
        # sum rules survive the bin mean: site / k mean of the binned maps = binned dos at the window
        _close(a["ldos"].mean(axis=(1, 2)), a["dos"][idx], "binned ldos")
        _close(a["akw"].mean(axis=(1, 2)), a["dos"][idx], "binned akw")


@pytest.mark.parametrize("tb", [1, 3])
def test_simulation_option_on_oracle(dwhmc, tmp_path, tb):
    """run_simulation(spectral_maps=...) on the oracle backend: the existing
    files are unchanged by the option, the bins gain ldos / akw; with
    transport_batch the maps go through TransportQueue's batches."""
    _simulate(dwhmc, tmp_path / "with", _OracleMaps, spectral_maps=SIM_WIN, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", _OracleMaps, transport_batch=tb, **SIM_KW)
    _check_sim_outputs(tmp_path / "with", tmp_path / "without")


@pytest.mark.parametrize("tb", [1, 2])
def test_simulation_chains_option_on_oracle(dwhmc, tmp_path, tb):
    _simulate(dwhmc, tmp_path / "with", _OracleMaps, chains=2, spectral_maps=SIM_WIN, transport_batch=tb, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", _OracleMaps, chains=2, transport_batch=tb, **SIM_KW)
    for k in range(2):
        _check_sim_outputs(tmp_path / "with" / f"c{k}", tmp_path / "without" / f"c{k}")


def test_simulation_option_rejects_unknown_keys(dwhmc, tmp_path):
    with pytest.raises(ValueError):
        _simulate(dwhmc, tmp_path, _OracleMaps, spectral_maps=dict(first=0, step=2), **SIM_KW)


# --------------------------------------------------------------------------- GPU
_refs = {}


def _ref_case(O, Lx, Ly, beta):
    """(p, disorder, Δ, _Ref) of a disordered lattice, computed once per module."""
    key = (Lx, Ly, beta)
    if key not in _refs:
        p, dis, D = _case(O, Lx, Ly, beta, seed=Lx * 17 + Ly)
        _refs[key] = (p, dis, D, _Ref(O, p, dis, D))
    return _refs[key]


WINDOWS = [(0, 1, 1), (3, 37, 37), (ND - 1, 1, 1)]


def _set_route(monkeypatch, route):
    """DWHMC_SPECTRAL_FUSED unset / "0": |X|² + the library's real product
    (the default: the faster one at L = 32); "1": the fused k_sp_maps."""
    if route is None:
        monkeypatch.delenv("DWHMC_SPECTRAL_FUSED", raising=False)
    else:
        monkeypatch.setenv("DWHMC_SPECTRAL_FUSED", route)


ROUTES = [None, "0", "1"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("Lx,Ly,beta", [(2, 4, 8.0), (3, 5, 4.0), (5, 7, 4.0), (6, 4, 8.0), (16, 16, 8.0)])
def test_maps_match_numpy(dwhmc, oracle, monkeypatch, Lx, Ly, beta, route):
    """N = 8, 15 (below one 16-row tile), 35 (row tail; 2N = 70 a K tail of the
    4-deep MFMA step and of the 16-deep stage), 24 (Lx != Ly), 256 (several
    tiles and workgroups).  Windows of 1, 37 (no multiple of 16) and the last
    grid point; on 6 x 4 the whole grid (4001 = 3 chunks of 1024 + 929)."""
    _set_route(monkeypatch, route)
    O = oracle
    p, dis, D, ref = _ref_case(O, Lx, Ly, beta)
    g = _grid(O)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    ctx.timing_enable(["spectral"])
    wins = WINDOWS + ([(0, ND, 1)] if (Lx, Ly) == (6, 4) else [])
    work = 0.0
    for first, count, stride in wins:
        r = ctx.measure_spectral_maps(ETA, DW, WMAX, first, count, stride)
        w = g[first::stride][:count]
        assert np.array_equal(r["omega"], w)
        ldos, akw = ref.maps(w)
        assert r["ldos"].shape == r["akw"].shape == (1, count, Ly, Lx)
        _close(r["ldos"][0], ldos, ("ldos", first, count, stride))
        _close(r["akw"][0], akw, ("akw", first, count, stride))
        work += 2.0 * p.N * 2 * p.N * count * 2
    ms, launches, flops = ctx.timing_read("spectral")
    ctx.close()
    assert flops == work and launches >= len(wins) and ms > 0


@pytest.mark.gpu
@pytest.mark.parametrize("Lx,Ly,beta", [(6, 4, 8.0), (8, 8, 16.0), (5, 7, 4.0)])
def test_sum_rules_against_transport(dwhmc, oracle, Lx, Ly, beta):
    """(1/N) Σ_i LDOS = (1/N) Σ_k A = dos, and on even sides
    [A((Lx/2, 0)) + A((0, Ly/2))] / 2 = dos_AN, against measure_transport on
    the same context."""
    p, dis, D = _case(oracle, Lx, Ly, beta, seed=Lx * 19 + Ly)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    tr = ctx.measure_transport(ETA, DW, WMAX)
    first, count, stride = 5, 200, 20
    r = ctx.measure_spectral_maps(ETA, DW, WMAX, first, count, stride)
    ctx.close()
    idx = first + stride * np.arange(count)
    assert np.array_equal(r["omega"], tr["dos_omega_grid"][idx])
    _close(r["ldos"][0].mean(axis=(1, 2)), tr["dos"][idx], "site mean")
    _close(r["akw"][0].mean(axis=(1, 2)), tr["dos"][idx], "k mean")
    if Lx % 2 == 0 and Ly % 2 == 0:
        an = 0.5 * (r["akw"][0][:, 0, Lx // 2] + r["akw"][0][:, Ly // 2, 0])
        _close(an, tr["dos_AN"][idx], "antinodal")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["0", "1"])
def test_degenerate_spectrum(dwhmc, oracle, monkeypatch, route):
    """The 10 x 10 clean, β = 1000, uniform d-wave case of
    test_transport_clean_degenerate_spectrum: exactly degenerate levels, the
    maps invariant under the basis chosen inside them."""
    _set_route(monkeypatch, route)
    O = oracle
    p = O.ModelParameters(10, 10, 1.0, -0.35, -1.0, 0.0, 0.0, 1000.0, 1.6, 0.1)
    N = p.N
    D = np.stack([np.full(N, 0.2), np.full(N, -0.2)], 1).astype(np.complex128)
    ref = _Ref(O, p, np.zeros(N), D)
    ctx = _ctx(dwhmc, p, np.zeros(N))
    ctx.set_pairing(D)
    r = ctx.measure_spectral_maps(p.eta, p.domega, p.omega_max, 0, 81, 50)
    ctx.close()
    ldos, akw = ref.maps(r["omega"], p.eta)
    assert np.array_equal(r["omega"], _grid(O)[0::50][:81])
    _close(r["ldos"][0], ldos, "ldos")
    _close(r["akw"][0], akw, "akw")


@pytest.mark.gpu
def test_particle_hole_half_solve(dwhmc, oracle):
    """μ = 0 on 12 x 8 through the structure-preserving solver: the maps are
    read from the partner-completed U of the half solve (eig_half == 1)."""
    O = oracle
    p = O.ModelParameters(12, 8, 1.0, -0.35, 0.0, 0.0, 0.0, 16.0, 0.8, 1.0)
    N = p.N
    D = np.stack([np.full(N, 0.2), np.full(N, -0.2)], 1).astype(np.complex128)
    ref = _Ref(O, p, np.zeros(N), D)
    ctx = _ctx(dwhmc, p, np.zeros(N))
    ctx.set_pairing(D)
    assert ctx.info["eig_half"] == -1
    r = ctx.measure_spectral_maps(ETA, DW, WMAX, 1900, 21, 10)
    half = ctx.info["eig_half"]
    ctx.close()
    assert half == 1
    ldos, akw = ref.maps(r["omega"])
    _close(r["ldos"][0], ldos, "ldos")
    _close(r["akw"][0], akw, "akw")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["0", "1"])
def test_snapshots_bitwise_and_state_untouched(dwhmc, oracle, monkeypatch, route):
    """Three pairing fields in one call equal three single-state calls bit for
    bit; a repeated call is bit-identical; the context's Δ is unchanged."""
    _set_route(monkeypatch, route)
    O = oracle
    p, dis, D, ref = _ref_case(O, 6, 4, 8.0)
    rng = np.random.default_rng(8)
    fields = np.stack([D, D * np.exp(0.1j), D + 0.05 * rng.standard_normal(D.shape)])
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(fields[1])
    before, _ = ctx.get_state()
    win = (3, 37, 37)
    r3 = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, deltas=fields)
    again = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, deltas=fields)
    after, _ = ctx.get_state()
    assert np.array_equal(before, after)
    assert r3["ldos"].shape == r3["akw"].shape == (3, 37, 4, 6)
    for k in ("ldos", "akw"):
        assert r3[k].tobytes() == again[k].tobytes(), k
    for s in range(3):
        one = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, deltas=fields[s:s + 1])
        for k in ("ldos", "akw"):
            assert one[k][0].tobytes() == r3[k][s].tobytes(), (k, s)
    dev = ctx.measure_spectral_maps(ETA, DW, WMAX, *win)          # the device Δ = fields[1]
    ctx.close()
    for k in ("ldos", "akw"):
        assert dev[k][0].tobytes() == r3[k][1].tobytes(), k
    ldos, akw = ref.maps(r3["omega"])
    _close(r3["ldos"][0], ldos, "ldos")
    _close(r3["akw"][0], akw, "akw")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["0", "1"])
def test_options_one_map_and_chain_select(dwhmc, oracle, monkeypatch, route):
    _set_route(monkeypatch, route)
    O = oracle
    p, dis, D, ref = _ref_case(O, 6, 4, 8.0)
    p2, dis2, D2 = _case(O, 6, 4, 8.0, seed=77)
    ref2 = _Ref(O, p2, dis2, D2)
    ctx = _ctx(dwhmc, p, np.stack([dis, dis2]))
    ctx.set_pairing(np.stack([D, D2]))
    win = (10, 40, 99)
    both = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, chain=1)
    only_l = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, chain=1, akw=False)
    only_a = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, chain=1, ldos=False)
    c0 = ctx.measure_spectral_maps(ETA, DW, WMAX, *win, chain=0)
    ctx.close()
    assert sorted(only_l) == ["ldos", "omega"] and sorted(only_a) == ["akw", "omega"]
    assert only_l["ldos"].tobytes() == both["ldos"].tobytes()
    assert only_a["akw"].tobytes() == both["akw"].tobytes()
    for r, rf in ((both, ref2), (c0, ref)):
        ldos, akw = rf.maps(r["omega"])
        _close(r["ldos"][0], ldos, "ldos")
        _close(r["akw"][0], akw, "akw")


@pytest.mark.gpu
def test_eig_algorithm_context(dwhmc, oracle):
    O = oracle
    p, dis, D = _case(O, 4, 4, 8.0, seed=44)
    ref = _Ref(O, p, dis, D)
    ctx = _ctx(dwhmc, p, dis, algo="eig")
    ctx.set_pairing(D)
    assert ctx.info["algo"] == 2
    r = ctx.measure_spectral_maps(ETA, DW, WMAX, 0, None, 100)
    ctx.close()
    assert len(r["omega"]) == 41
    ldos, akw = ref.maps(r["omega"])
    _close(r["ldos"][0], ldos, "ldos")
    _close(r["akw"][0], akw, "akw")


@pytest.mark.gpu
def test_argument_errors(dwhmc, oracle):
    p, dis, D = _case(oracle, 4, 4, 8.0, seed=44)
    ctx = _ctx(dwhmc, p, dis)
    ctx.set_pairing(D)
    try:
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 0, 1, 1, chain=1)
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 0, 1, 1, chain=-1)
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 3, 110, 37)
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 0, 0, 1)
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 0, 1, 0)
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 0, 1, 1, ldos=False, akw=False)
        bad = np.stack([D, D])
        bad[1, 3, 0] = np.nan
        with pytest.raises(ValueError):
            ctx.measure_spectral_maps(ETA, DW, WMAX, 0, 1, 1, deltas=bad)
        # nstates != 1 with Delta == NULL, straight through the ABI
        out = np.zeros(2 * p.N)
        q = out.ctypes.data_as(C.c_void_p)
        assert ctx._lib.dwh_measure_spectral_maps(ctx._h, 0, 2, None, ETA, DW, WMAX, 0, 1, 1, q, q) == -1
        assert ctx._lib.dwh_measure_spectral_maps(ctx._h, 0, 0, None, ETA, DW, WMAX, 0, 1, 1, q, q) == -1
        # the context still measures after the refusals
        r = ctx.measure_spectral_maps(ETA, DW, WMAX, 2000, 1, 1)
        assert np.all(np.isfinite(r["ldos"])) and np.all(r["ldos"] >= 0)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_simulation_option_on_device(dwhmc, tmp_path):
    """4 x 4, a few sweeps, the same draws with and without spectral_maps:
    observables.csv, transport.csv and the existing npz fields byte-equal;
    the bins of the run with maps hold ldos / akw whose site mean is the
    binned dos at the window points."""
    _simulate(dwhmc, tmp_path / "with", None, spectral_maps=SIM_WIN, **SIM_KW)
    _simulate(dwhmc, tmp_path / "without", None, **SIM_KW)
    _check_sim_outputs(tmp_path / "with", tmp_path / "without")
