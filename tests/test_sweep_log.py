"""The sweep log off the device: dwh_sweep_log_layout (the validation and the
sizes dwh_sweep_log and its readers use) on hand-checked cases, and the
drivers' sweep_batch mode on the oracle context with the throughput path
(tests/sweep_log_oracle.py): the files do not depend on the batch size, equal
a hand loop of hmc_sweep with the same injected draws, and sweep_batch=None
writes what it wrote before."""
import importlib
import os

import numpy as np
import pytest

from oracle_context import OracleContext
from sweep_log_oracle import LoggedOracleContext

OBS, SQ, SNAP = 1, 2, 4


@pytest.fixture(scope="module")
def sim(dwhmc):
    return importlib.import_module(dwhmc.__name__ + ".simulation")


@pytest.fixture(scope="module")
def hmc_mod(dwhmc):
    return importlib.import_module(dwhmc.__name__ + ".hmc")


@pytest.fixture(scope="module")
def ctx_mod(dwhmc):
    return importlib.import_module(dwhmc.__name__ + ".context")


# -- layout ----------------------------------------------------------------------
def test_layout_counts(ctx_mod):
    L = ctx_mod.sweep_log_layout
    nc, N, nd = 2, 6, 10
    assert L(nc, N, nd, what=OBS) == (12 * 2 * 10, 0, 0)
    assert L(nc, N, nd, what=OBS | SQ, first=3, nsweeps=4) == (12 * 2 * 4, 2 * 6 * 2 * 4, 0)
    assert L(nc, N, nd, what=0) == (0, 0, 0)
    # every 2 from sweep 1: sweeps 1, 3, 5, 7, 9
    assert L(nc, N, nd, what=SNAP, snapshot_every=2, snapshot_offset=1) == (0, 0, 5)
    # the cadence across two consecutive ranges: 1, 3 | 5, 7, 9
    assert L(nc, N, nd, what=SNAP, snapshot_every=2, snapshot_offset=1, first=0, nsweeps=5)[2] == 2
    assert L(nc, N, nd, what=SNAP, snapshot_every=2, snapshot_offset=1, first=5, nsweeps=5)[2] == 3
    # every 3 from sweep 2 (2, 5, 8): [0, 2) none, [2, 3) one, [3, 8) one, [8, 10) one
    for first, n, want in ((0, 2, 0), (2, 1, 1), (3, 5, 1), (8, 2, 1), (0, 10, 3)):
        assert L(nc, N, nd, what=SNAP, snapshot_every=3, snapshot_offset=2, first=first, nsweeps=n)[2] == want
    # offset past the range, and past the draws
    assert L(nc, N, nd, what=SNAP, snapshot_every=1, snapshot_offset=7, first=0, nsweeps=5)[2] == 0
    assert L(nc, N, nd, what=SNAP, snapshot_every=1, snapshot_offset=7, first=5, nsweeps=5)[2] == 3
    assert L(nc, N, nd, what=SNAP, snapshot_every=1, snapshot_offset=15)[2] == 0
    # snap_every larger than the range: sweep 0 alone
    assert L(nc, N, nd, what=SNAP, snapshot_every=20, snapshot_offset=0)[2] == 1
    assert L(nc, N, nd, what=SNAP, snapshot_every=20, snapshot_offset=0, first=1, nsweeps=9)[2] == 0
    # an empty range, and no draws at all
    assert L(nc, N, nd, what=OBS | SQ | SNAP, snapshot_every=1, first=10, nsweeps=0) == (0, 0, 0)
    assert L(nc, N, 0, what=OBS) == (0, 0, 0)
    # the field part up to N = 4096
    assert L(1, 4096, 1, what=SQ) == (0, 2 * 4096, 0)
    assert L(1, 4097, 1, what=OBS | SNAP, snapshot_every=1) == (12, 0, 1)


@pytest.mark.parametrize("kw", [
    dict(what=8), dict(what=-1), dict(what=OBS | 16),
    dict(what=SNAP, snapshot_every=0), dict(what=SNAP, snapshot_every=-2),
    dict(what=SNAP | OBS, snapshot_every=1, snapshot_offset=-1),
    dict(what=SQ, N=4097), dict(what=SQ | OBS, N=8192),
    dict(what=OBS, first=0, nsweeps=11), dict(what=OBS, first=-1, nsweeps=2), dict(what=OBS, first=4, nsweeps=-1),
    dict(what=OBS, first=11, nsweeps=0), dict(what=OBS, nchains=0), dict(what=OBS, N=0), dict(what=OBS, ndraws=-1),
])
def test_layout_refusals(ctx_mod, kw):
    args = dict(nchains=2, N=6, ndraws=10)
    args.update(kw)
    if "ndraws" in kw:
        args.update(first=0, nsweeps=0)
    with pytest.raises(ValueError):
        ctx_mod.sweep_log_layout(**args)
    # a snapshot cadence is not looked at without the snapshot bit
    assert ctx_mod.sweep_log_layout(2, 6, 10, what=OBS, snapshot_every=0, snapshot_offset=-1) == (240, 0, 0)


# -- the drivers -------------------------------------------------------------------
KW = dict(n_therm=4, n_measure=10, Nt_therm_init=2, Nt_measure=3, measure_transport_freq=2, bin_size=2)
FILES = ("observables.csv", "transport.csv")


def params(dwhmc):
    return dwhmc.ModelParameters(6, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 4.0, 0.8, 1.0)


class patched:
    def __init__(self, hmc_mod, cls):
        self.mod, self.cls = hmc_mod, cls

    def __enter__(self):
        self.saved = self.mod.FermionContext
        self.mod.FermionContext = self.cls

    def __exit__(self, *a):
        self.mod.FermionContext = self.saved


def same_files(a, b, also=()):
    for f in FILES + tuple(also):
        assert (a / f).read_bytes() == (b / f).read_bytes(), (a.name, b.name, f)
    names = sorted(os.listdir(a / "spectra_bins"))
    assert names == sorted(os.listdir(b / "spectra_bins")), (a.name, b.name)
    for n in names:
        if n.endswith(".npz"):
            x, y = np.load(a / "spectra_bins" / n), np.load(b / "spectra_bins" / n)
            assert sorted(x.files) == sorted(y.files)
            for key in x.files:
                assert np.array_equal(x[key], y[key]), (a.name, b.name, n, key)


@pytest.fixture(scope="module")
def runs(sim, hmc_mod, dwhmc, tmp_path_factory):
    """run_simulation with seed 11 for sweep_batch = 1, 3, 10 and None on the
    logged oracle context, and None on the plain one; made once."""
    root = tmp_path_factory.mktemp("sweep_log")
    p = params(dwhmc)
    out = {}
    for name, cls, kw in (("b1", LoggedOracleContext, dict(sweep_batch=1, field_sq=True)),
                          ("b3", LoggedOracleContext, dict(sweep_batch=3, field_sq=True)),
                          ("b10", LoggedOracleContext, dict(sweep_batch=10, field_sq=True)),
                          ("b3tb2", LoggedOracleContext, dict(sweep_batch=3, transport_batch=2)),
                          ("none", LoggedOracleContext, {}), ("plain", OracleContext, {})):
        with patched(hmc_mod, cls):
            out[name] = (root / name, sim.run_simulation(p, str(root / name), rng=np.random.default_rng(11),
                                                         verbose=False, **KW, **kw))
    return out


def test_batch_size_does_not_change_the_files(runs):
    for other in ("b3", "b10"):
        same_files(runs["b1"][0], runs[other][0], also=("field_sq.npy",))
    same_files(runs["b1"][0], runs["b3tb2"][0])
    rows = (runs["b3"][0] / "observables.csv").read_text().splitlines()
    assert len(rows) == 11
    assert len((runs["b3"][0] / "transport.csv").read_text().splitlines()) == 6
    assert sorted(os.listdir(runs["b3"][0] / "spectra_bins")) == ["omega_grid.npy", "params.json", "sweep_4.npz",
                                                                  "sweep_8.npz"]
    sq = np.load(runs["b3"][0] / "field_sq.npy")
    assert sq.shape == (10, 2, 4, 6)
    s_delta = np.array([r[3].S_Delta for r in runs["b3"][1].records])
    assert np.max(np.abs(sq[:, 0, 0, 0] - s_delta)) <= 1e-15
    assert "Sweep batches: up to 3 sweeps per device batch" in (runs["b3"][0] / "simulation.log").read_text()
    assert not os.path.exists(runs["none"][0] / "field_sq.npy")


def test_default_writes_what_it_wrote(runs):
    same_files(runs["none"][0], runs["plain"][0])
    assert "Sweep batches" not in (runs["none"][0] / "simulation.log").read_text()
    # the uniforms differ from the batch mode's (drawn only when ΔH >= 0), so the chains do too
    assert [r[:3] for r in runs["none"][1].records] == [r[:3] for r in runs["plain"][1].records]


def test_batch_mode_equals_hand_loop(runs, sim, hmc_mod, dwhmc, tmp_path):
    """The driver's draws, in its order, injected into hmc.hmc_sweep on the
    plain oracle context: the same rows, and the bins the means of their
    members."""
    p = params(dwhmc)
    H = hmc_mod
    rng = np.random.default_rng(11)
    obs_rows, tr_rows, specs = [], [], []
    with patched(hmc_mod, OracleContext):
        out = sim.ChainOutput(str(tmp_path / "hand"), False)
        try:
            state = H.initialize_state(p, rng)
            cache = H.initialize_cache(p)
            H.init_static_H(cache, p, state)
            H.update_H_BdG(cache, p, state)
            H.diagonalize_H_BdG(cache, p)
            sim.thermalize(cache, p, state, out, KW["n_therm"], KW["Nt_therm_init"], rng)
        finally:
            out.close()
        dt = H.calc_optimal_dt(p.beta, p.J, p.mass, KW["Nt_measure"])
        for i in range(1, KW["n_measure"] + 1):
            noise = H.standard_complex_normal(rng, (p.N, 2))
            u = rng.random()
            acc, dH = H.hmc_sweep(cache, p, state, Nt=KW["Nt_measure"], dt=dt, noise=noise, uniform=u)
            obs_rows.append(sim.obs_csv_line(i, acc, dH, H.measure_observables(cache, p, state)))
            if i % KW["measure_transport_freq"] == 0:
                specs.append(H.measure_transport_and_spectra(cache, p))
                tr_rows.append(sim.transport_csv_line(i, specs[-1]))
    d = runs["b3"][0]
    assert (d / "observables.csv").read_text() == sim.OBS_HEADER + "\n" + "".join(obs_rows)
    assert (d / "transport.csv").read_text() == sim.TRANSPORT_HEADER + "\n" + "".join(tr_rows)
    for k, name in enumerate(("sweep_4.npz", "sweep_8.npz")):
        b = np.load(d / "spectra_bins" / name)
        a0, a1 = specs[2 * k], specs[2 * k + 1]
        for key, f in (("opt_cond", "optical_conductivity"), ("dos", "dos"), ("dos_AN", "dos_AN"),
                       ("A_k0", "A_k_omega0")):
            want = np.array(getattr(a0, f), dtype=np.float64)
            want = (want + getattr(a1, f)) / 2
            assert np.array_equal(b[key], want), (name, key)
    # the run is not a trivial one: the rng advanced as the driver's did
    assert len({r[2] for r in runs["b3"][1].records}) == KW["n_measure"]


def test_chains_equal_their_single_runs(sim, hmc_mod, dwhmc, tmp_path):
    p = params(dwhmc)
    with patched(hmc_mod, LoggedOracleContext):
        for k in range(2):
            sim.run_simulation(p, str(tmp_path / f"single{k}"), rng=np.random.default_rng(100 + k), verbose=False,
                               sweep_batch=3, field_sq=True, **KW)
        multi = sim.run_simulation_chains(p, [str(tmp_path / f"chain{k}") for k in range(2)],
                                          [np.random.default_rng(100 + k) for k in range(2)], sweep_batch=4,
                                          field_sq=True, **KW)
    for k in range(2):
        same_files(tmp_path / f"single{k}", tmp_path / f"chain{k}", also=("field_sq.npy",))
        assert len(multi[k].records) == KW["n_measure"] and len(multi[k].transport) == 5
    assert (tmp_path / "chain0" / "observables.csv").read_bytes() != (tmp_path / "chain1" / "observables.csv").read_bytes()


def test_field_sq_needs_the_batch_mode(sim, dwhmc, tmp_path):
    with pytest.raises(ValueError):
        sim.run_simulation(params(dwhmc), str(tmp_path / "x"), field_sq=True)
    assert not os.path.exists(tmp_path / "x")


def test_replicas_pass_sweep_batch(dwhmc, hmc_mod):
    """ReplicaConfig.sweep_batch: the same draws, so the same records as one
    call per sweep (flags and ΔH equal; the observables within the rounding of
    two formulas for the same numbers) and the same transport rows."""
    rep = importlib.import_module(dwhmc.__name__ + ".replicas")
    p = params(dwhmc)

    def make(dis):
        return LoggedOracleContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis)

    out = {}
    for B in (None, 2):
        cfg = rep.ReplicaConfig(chains=2, n_sweeps=5, Nt=3, transport_freq=2, sweep_batch=B)
        tr = []
        rec = rep.run_local(p, cfg, 0, 0, make, hmc_mod.initialize_state, hmc_mod.calc_optimal_dt, transport_out=tr)
        out[B] = (rec, np.stack(tr))
    assert np.array_equal(out[None][0][:, :, :2], out[2][0][:, :, :2])
    assert np.max(np.abs(out[None][0] - out[2][0])) <= 1e-14
    assert out[2][1].shape == (2, 2, 3) and np.array_equal(out[None][1], out[2][1])
