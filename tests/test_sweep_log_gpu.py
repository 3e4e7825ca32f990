"""The sweep log on the device (dwh_sweep_log): what run_sweeps records per
sweep and chain against the single-sweep path of a second context, the CPU
oracle and numpy's FFT.

Bars:
  accepted, ΔH      the throughput path's existing guarantee: the single-sweep path's bits
  12 record fields  <= 1e-12 (1 + |host value|) against hmc.observables_from_outputs on the single-sweep
                    context's Δ, P, E_f, Tr ρ_hh after the same sweep: the inputs are the same bits, the two
                    sides differ in summation order, and N ε = 4096 · 1.1e-16 < 5e-13 bounds that
  fields 0..8       <= 1e-10 (1 + |ref|) against O.measure_observables at the logged snapshot's Δ
                    (test_host_mirror_api_roundtrip's tolerance for the same nine fields)
  S_ch(q)           <= 1e-12 max(1, max_i |f_i|²) against |fft2(f)|² / N²; S_d(0) against field 4 <= 1e-12;
                    Σ_q S_ch(q) against (1/N) Σ_i |f_i|² <= 1e-12 (1 + that)
  snapshots         bit-equal to get_state() after the same sweep on the single-sweep context

Lattices (the smallest at which the kernels can go wrong): 3x2 (N = 6, far less
than a wave), 6x4, 12x5 (N = 60, BP 32, Lx != Ly), 20x4 (BP 64), each with the
mixed-outcome recipe of tests/hmc_chain_cases.py (4 chains, 6 sweeps,
prescribed accepts and rejects), and 18x16 (N = 288: more than the 256 threads
and not a multiple; 2 chains, 3 sweeps, Nt = 2).

Measured on an MI355X (every test prints its error / bar before it asserts):
the record against the single-sweep path below 0.0005 of its bar for every
field, case and algorithm, the guard case included; against the oracle 0.001
(6x4) and 0.004 (12x5); S(q) against the FFT and Parseval below 0.0005, also at
48x48 and 64x64; snapshots, flags and ΔH bit-equal."""
import importlib
import types

import numpy as np
import pytest

import hmc_chain_cases as H
from oracle import dwhmc_oracle as O
from sweep_log_oracle import LoggedOracleContext, field_sq, record
from test_gpu_parity import device_ctx, make_case
from test_hmc_chains import open_ctx

pytestmark = pytest.mark.gpu

TABLE = ("3x2", "6x4", "12x5", "20x4")
CASES = [(n, a) for n in TABLE for a in H.CASES[n].algos] + [("18x16", "cr")]
SQ_CASES = [("6x4", "cr"), ("12x5", "cr"), ("18x16", "cr")]
_RUNS = {}


def big_case():
    """18x16: 2 chains, 3 sweeps, Nt = 2, no prescribed outcomes (u = 0.5)."""
    chains = [make_case(O, 18, 16, H.BETA, seed=700 + c, amp=0.1) for c in range(2)]
    p = chains[0][0]
    noise = H.cnoise(np.random.default_rng(31), (3, 2, p.N, 2))
    return types.SimpleNamespace(p=p, dis=np.stack([c[1] for c in chains]), Delta0=np.stack([c[2] for c in chains]),
                                 noise=noise, u=np.full((3, 2), 0.5), Nt=2,
                                 dt=2.0 * O.calc_optimal_dt(p.beta, p.J, p.mass, 2), scheme="leapfrog", nsweeps=3,
                                 nchains=2)


def inputs(name):
    return big_case() if name == "18x16" else H.reference(name)


def single_path(dwhmc, ref, algo, **kw):
    """hmc_sweep sweep by sweep; per sweep the flags, ΔH, Δ and the host's
    record (observables_from_outputs) and S(q) (fft2) of every chain."""
    ctx = open_ctx(dwhmc, ref, algo, **kw)
    acc, dH, Delta, obs, sq = [], [], [], [], []
    for s in range(ref.nsweeps):
        a, d = ctx.hmc_sweep(ref.noise[s], ref.u[s], ref.Nt, ref.dt, ref.p.mass)
        D, _ = ctx.get_state()
        P, Ef, tr = ctx.pairing(), ctx.fermion_energy(), ctx.hole_trace()
        acc.append(a)
        dH.append(d)
        Delta.append(D)
        obs.append(np.stack([record(ref.p, D[c], P[c], Ef[c], tr[c]) for c in range(ref.nchains)]))
        sq.append(np.stack([field_sq(D[c], ref.p.Lx, ref.p.Ly) for c in range(ref.nchains)]))
    cap = ctx.info["delta_cap"]
    ctx.close()
    return types.SimpleNamespace(acc=np.stack(acc), dH=np.stack(dH), Delta=np.stack(Delta), obs=np.stack(obs),
                                 sq=np.stack(sq), cap=cap)


def logged_path(dwhmc, ref, algo, every=1, offset=0, **kw):
    """The same draws as one logged batch, all three parts."""
    ctx = open_ctx(dwhmc, ref, algo, **kw)
    ctx.load_draws(ref.noise, ref.u)
    ctx.sweep_log(observables=True, field_sq=True, snapshot_every=every, snapshot_offset=offset)
    ctx.timing_enable(["sweep_log"])
    ctx.run_sweeps(0, ref.nsweeps, ref.Nt, ref.dt, ref.p.mass)
    acc, dH = ctx.sweep_results(0, ref.nsweeps)
    out = types.SimpleNamespace(acc=acc, dH=dH, obs=ctx.sweep_observables(0, ref.nsweeps),
                                sq=ctx.sweep_field_sq(0, ref.nsweeps), snaps=ctx.sweep_snapshots(0, ref.nsweeps),
                                timer=ctx.timing_read("sweep_log"), final=ctx.get_state()[0], info=ctx.info)
    return ctx, out


def runs(dwhmc, name, algo):
    """(inputs, single-sweep run, logged run with a snapshot of every sweep), made once per case."""
    if (name, algo) not in _RUNS:
        ref = inputs(name)
        one = single_path(dwhmc, ref, algo)
        ctx, log = logged_path(dwhmc, ref, algo)
        ctx.close()
        _RUNS[name, algo] = (ref, one, log)
    return _RUNS[name, algo]


def check_record(log_obs, host_obs, label):
    err = np.abs(log_obs - host_obs)
    bar = 1e-12 * (1 + np.abs(host_obs))
    worst = np.max(err / bar, axis=tuple(range(err.ndim - 1)))
    print(f"RECORD {label}: error / bar per field " + " ".join(f"{w:.3f}" for w in worst))
    assert np.all(err <= bar), f"{label}: fields {np.unique(np.nonzero(err > bar)[-1])} miss, worst {worst.max():.3g}"


def check_sq(sq, Delta, p, label):
    """sq (..., 2, Ly, Lx) against the FFT of the Δ (..., N, 2) it was taken from."""
    D = Delta.reshape(-1, p.N, 2)
    S = sq.reshape(-1, 2, p.Ly, p.Lx)
    worst = [0.0, 0.0]
    for k in range(len(D)):
        want = field_sq(D[k], p.Lx, p.Ly)
        f = np.stack([0.5 * (D[k][:, 0] - D[k][:, 1]), 0.5 * (D[k][:, 0] + D[k][:, 1])])
        for ch in range(2):
            m2 = np.mean(np.abs(f[ch]) ** 2)
            e1 = np.max(np.abs(S[k, ch] - want[ch])) / (1e-12 * max(1.0, np.max(np.abs(f[ch]) ** 2)))
            e2 = abs(np.sum(S[k, ch]) - m2) / (1e-12 * (1 + m2))
            worst = [max(worst[0], e1), max(worst[1], e2)]
    print(f"FIELD_SQ {label}: error / bar fft {worst[0]:.3f} parseval {worst[1]:.3f}")
    assert worst[0] <= 1 and worst[1] <= 1, (label, worst)


# -- observables against the single-sweep path ---------------------------------------
@pytest.mark.parametrize("name,algo", CASES)
def test_record_matches_single_sweep_path(dwhmc, name, algo):
    ref, one, log = runs(dwhmc, name, algo)
    if name in TABLE:
        H.assert_pattern(ref.acc)
        assert np.array_equal(log.acc, ref.acc)
    assert np.array_equal(log.acc, one.acc) and np.array_equal(log.dH, one.dH)
    assert log.obs.shape == (ref.nsweeps, ref.nchains, 12)
    check_record(log.obs, one.obs, f"{name} {algo}")
    assert np.all(log.obs[..., 11] > 0)


# -- observables against the CPU oracle ------------------------------------------------
@pytest.mark.parametrize("name", ["6x4", "12x5"])
def test_record_matches_oracle_at_snapshots(dwhmc, name):
    ref, _, log = runs(dwhmc, name, "cr")
    sweeps, snaps = log.snaps
    assert list(sweeps) == list(range(ref.nsweeps))
    keys = ("total_energy", "Delta_amp", "Delta_local", "Delta_global", "S_Delta", "hole_conc", "Delta_diff",
            "Delta_pair", "Delta_localpair")
    worst = 0.0
    for m, s in enumerate(sweeps):
        for c in range(ref.nchains):
            cache, _, _ = O.evaluate(ref.p, ref.dis[c], snaps[m, c])
            want = O.measure_observables(cache, ref.p, snaps[m, c])
            for f, k in enumerate(keys):
                r = abs(log.obs[s, c, f] - want[k]) / (1e-10 * (1 + abs(want[k])))
                worst = max(worst, r)
                assert r <= 1, (name, s, c, k, log.obs[s, c, f], want[k])
    print(f"RECORD-ORACLE {name}: worst error / bar {worst:.3f}")


# -- field structure factors -------------------------------------------------------------
@pytest.mark.parametrize("name,algo", SQ_CASES)
def test_field_sq_matches_fft(dwhmc, name, algo):
    ref, one, log = runs(dwhmc, name, algo)
    assert log.sq.shape == (ref.nsweeps, ref.nchains, 2, ref.p.Ly, ref.p.Lx)
    check_sq(log.sq, one.Delta, ref.p, f"{name} {algo}")
    assert np.max(np.abs(log.sq[:, :, 0, 0, 0] - log.obs[:, :, 4])) <= 1e-12


def test_field_sq_plane_wave(dwhmc):
    """Δ = one plane wave of d symmetry at (kx, ky) = (2, 1) on 12x5, kept by a
    trajectory of no steps: all of S_d at q, nothing at -q, S_s zero — the sign
    and the q = kx + Lx·ky indexing."""
    Lx, Ly, kx, ky, A = 12, 5, 2, 1, 0.3
    p, dis, _ = make_case(O, Lx, Ly, 8.0, seed=3)
    x, y = np.arange(p.N) % Lx, np.arange(p.N) // Lx
    d = A * np.exp(2j * np.pi * (kx * x / Lx + ky * y / Ly))
    ctx = device_ctx(dwhmc, p, dis, "cr")
    ctx.set_pairing(np.stack([d, -d], axis=1))
    ctx.factorize()
    ctx.load_draws(H.cnoise(np.random.default_rng(4), (1, 1, p.N, 2)), np.full((1, 1), 0.5))
    ctx.sweep_log(observables=True, field_sq=True)
    ctx.run_sweeps(0, 1, 0, 0.1, p.mass)
    sq = ctx.sweep_field_sq(0, 1)[0, 0]
    obs = ctx.sweep_observables(0, 1)[0, 0]
    ctx.close()
    assert abs(sq[0, ky, kx] - A * A) <= 1e-12
    rest = sq[0].copy()
    rest[ky, kx] = 0.0
    assert np.max(rest) <= 1e-12 and sq[0, (-ky) % Ly, (-kx) % Lx] <= 1e-12
    assert np.max(sq[1]) <= 1e-12
    assert abs(obs[4]) <= 1e-12 and abs(obs[1] - A) <= 1e-12


@pytest.mark.parametrize("L", [48, 64])
def test_field_sq_large_lds(dwhmc, L):
    """N = 2304 (a production size, no power of two) and N = 4096 (the limit):
    72 and 128 KiB of LDS, above the 64 KiB a launch gets without asking.  The
    trajectory has no steps and the context is never factorised, so only the
    log's kernels run at this size; Δ is a random field."""
    p, dis, _ = make_case(O, L, L, 8.0, seed=L)
    rng = np.random.default_rng(L + 1)
    D = 0.2 * H.cnoise(rng, (p.N, 2))
    ctx = device_ctx(dwhmc, p, dis, "cr")
    ctx.set_pairing(D)
    ctx.load_draws(H.cnoise(rng, (1, 1, p.N, 2)), np.full((1, 1), 0.5))
    ctx.sweep_log(observables=True, field_sq=True)
    ctx.run_sweeps(0, 1, 0, 0.1, p.mass)
    sq = ctx.sweep_field_sq(0, 1)
    obs = ctx.sweep_observables(0, 1)[0, 0]
    ctx.close()
    check_sq(sq, D[None], p, f"{L}x{L}")
    assert abs(sq[0, 0, 0, 0, 0] - obs[4]) <= 1e-12
    assert abs(obs[11] - np.sum(np.abs(D) ** 2)) <= 1e-12 * (1 + obs[11])


# -- snapshots -----------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
def test_snapshots_every_second_sweep(dwhmc, offset):
    ref, one, _ = runs(dwhmc, "6x4", "cr")
    ctx, log = logged_path(dwhmc, ref, "cr", every=2, offset=offset)
    sweeps, snaps = log.snaps
    assert list(sweeps) == list(range(offset, ref.nsweeps, 2))
    assert snaps.shape == (len(sweeps), ref.nchains, ref.p.N, 2)
    for m, s in enumerate(sweeps):
        assert np.array_equal(snaps[m], one.Delta[s]), f"snapshot of sweep {s}"
    # a window of the range, and one without a snapshot
    part = ctx.sweep_snapshots(2, 3)
    assert list(part[0]) == [s for s in sweeps if 2 <= s < 5] and np.array_equal(part[1][0], one.Delta[part[0][0]])
    assert ctx.sweep_snapshots(offset + 1, 1)[1].shape == (0, ref.nchains, ref.p.N, 2)
    ctx.close()
    # rejected chains show the restored Δ: the bits of the sweep before
    rejected = [(m, s, c) for m, s in enumerate(sweeps) for c in range(ref.nchains) if s > 0 and not ref.acc[s, c]]
    assert rejected
    for m, s, c in rejected:
        assert np.array_equal(snaps[m, c], one.Delta[s - 1, c]), (s, c)
    accepted = [(m, s, c) for m, s in enumerate(sweeps) for c in range(ref.nchains) if s > 0 and ref.acc[s, c]]
    assert all(not np.array_equal(snaps[m, c], one.Delta[s - 1, c]) for m, s, c in accepted)


# -- a guard trip inside the logged batch -----------------------------------------------------
def test_guard_trip_replay_is_logged(dwhmc):
    """tests/hmc_chain_cases.py's guard recipe (cr 20x4: chain 1 of sweep 2
    drifts past delta_cap = 0.2, the batch halts, the poles are re-selected
    and sweeps 2.. replayed): every log equals the single-sweep path's, the
    sweeps after the tripped one included, and the log is still in the
    context's device bytes afterwards."""
    name = "cr-20x4"
    k, ref = H.GUARD_CASES[name], H.guard_reference(name)
    H.assert_guard_pattern(ref.acc)
    cap0 = H.GUARD_CAP
    one = single_path(dwhmc, ref, k.algo, delta_cap=cap0)
    ctx, log = logged_path(dwhmc, ref, k.algo, delta_cap=cap0)
    assert one.cap > cap0 and log.info["delta_cap"] == one.cap
    assert np.array_equal(log.acc, one.acc) and np.array_equal(log.dH, one.dH)
    check_record(log.obs, one.obs, f"guard {name}")
    check_sq(log.sq, one.Delta, ref.p, f"guard {name}")
    sweeps, snaps = log.snaps
    assert list(sweeps) == list(range(ref.nsweeps))
    for s in range(ref.nsweeps):
        assert np.array_equal(snaps[s], one.Delta[s]), f"snapshot of sweep {s}"
    assert np.array_equal(log.final, one.Delta[-1])
    ctx_mod = importlib.import_module(dwhmc.__name__ + ".context")
    n_obs, n_sq, n_snap = ctx_mod.sweep_log_layout(ref.nchains, ref.p.N, ref.nsweeps, field_sq=True, snapshot_every=1)
    log_bytes = 8 * (n_obs + n_sq) + 16 * n_snap * ref.nchains * 2 * ref.p.N
    before = ctx.info["device_bytes"]
    ctx.sweep_log(observables=False)
    assert before - ctx.info["device_bytes"] == log_bytes
    ctx.close()


# -- off means off ---------------------------------------------------------------------------
def test_off_means_off(dwhmc):
    ref, one, full = runs(dwhmc, "6x4", "cr")
    ns = ref.nsweeps

    def batch(prepare):
        ctx = open_ctx(dwhmc, ref, "cr")
        ctx.load_draws(ref.noise, ref.u)
        prepare(ctx)
        ctx.timing_enable(["sweep_log"])
        ctx.run_sweeps(0, ns, ref.Nt, ref.dt, ref.p.mass)
        acc, dH = ctx.sweep_results(0, ns)
        return ctx, acc, dH, ctx.get_state()[0], ctx.timing_read("sweep_log")[1]

    def on_then_off(ctx):
        ctx.sweep_log(observables=True, field_sq=True, snapshot_every=1)
        ctx.sweep_log(observables=False)

    never, acc0, dH0, D0, launches0 = batch(lambda ctx: None)
    off, acc1, dH1, D1, launches1 = batch(on_then_off)
    assert np.array_equal(acc0, acc1) and np.array_equal(dH0, dH1) and np.array_equal(D0, D1)
    assert np.array_equal(D0, one.Delta[-1]) and np.array_equal(D0, full.final)
    assert launches0 == 0 and launches1 == 0
    assert never.info["device_bytes"] == off.info["device_bytes"]
    for ctx in (never, off):
        for read in (ctx.sweep_observables, ctx.sweep_field_sq, ctx.sweep_snapshots):
            with pytest.raises(dwhmc.DwhError) as e:
                read(0, ns)
            assert e.value.code == -3
        ctx.close()
    # one launch per sweep per enabled part, and exactly the enabled parts readable
    assert full.timer[1] == 3 * ns
    for kw, parts in ((dict(observables=True), (1, 0, 0)), (dict(observables=False, field_sq=True), (0, 1, 0)),
                      (dict(observables=False, snapshot_every=2, snapshot_offset=1), (0, 0, 1)),
                      (dict(observables=True, snapshot_every=2), (1, 0, 1))):
        ctx, acc, dH, D, launches = batch(lambda c: c.sweep_log(**kw))
        assert np.array_equal(acc, acc0) and np.array_equal(dH, dH0) and np.array_equal(D, D0)
        assert launches == ns * (parts[0] + parts[1]) + (ns // 2) * parts[2], (kw, launches)
        for on, read in zip(parts, (ctx.sweep_observables, ctx.sweep_field_sq, ctx.sweep_snapshots)):
            if on:
                read(0, ns)
            else:
                with pytest.raises(dwhmc.DwhError) as e:
                    read(0, ns)
                assert e.value.code == -3
        enabled = [r for on, r in zip(parts, (ctx.sweep_observables, ctx.sweep_field_sq, ctx.sweep_snapshots)) if on]
        with pytest.raises(ValueError):
            enabled[0](1, ns)                                   # a range past the loaded draws
        ctx.close()


def test_refusals_change_nothing(dwhmc):
    ref, _, full = runs(dwhmc, "6x4", "cr")
    ctx, log = logged_path(dwhmc, ref, "cr")
    for bad in (dict(snapshot_every=-1), dict(snapshot_every=1, snapshot_offset=-1)):
        with pytest.raises(ValueError):
            ctx.sweep_log(**bad)
    with pytest.raises(ValueError):
        ctx._c(ctx._lib.dwh_sweep_log(ctx._h, 8, 1, 0))
    assert np.array_equal(ctx.sweep_observables(0, ref.nsweeps), full.obs)
    # between trajectory and finish the setting cannot change
    ctx.hmc_trajectory(ref.noise[0], ref.Nt, ref.dt, ref.p.mass)
    with pytest.raises(dwhmc.DwhError) as e:
        ctx.sweep_log(observables=True)
    assert e.value.code == -3
    ctx.hmc_finish(np.ones(ref.nchains, dtype=bool))
    # draws that grow: the log grows with them and starts from zero
    more = np.concatenate([ref.noise, ref.noise[:2]])
    ctx.load_draws(more, np.concatenate([ref.u, ref.u[:2]]))
    assert not np.any(ctx.sweep_observables(0, ref.nsweeps + 2))
    assert list(ctx.sweep_snapshots(0, ref.nsweeps + 2)[0]) == list(range(ref.nsweeps + 2))
    ctx.close()


# -- the driver ------------------------------------------------------------------------------
def test_driver_sweep_batch_device_matches_oracle(dwhmc, tmp_path):
    sim = importlib.import_module(dwhmc.__name__ + ".simulation")
    hmc_mod = importlib.import_module(dwhmc.__name__ + ".hmc")
    p = dwhmc.ModelParameters(6, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 4.0, 0.8, 1.0)
    kw = dict(n_therm=10, n_measure=10, Nt_therm_init=4, Nt_measure=5, measure_transport_freq=2, bin_size=2,
              sweep_batch=3, field_sq=True, verbose=False)
    saved = hmc_mod.FermionContext
    hmc_mod.FermionContext = LoggedOracleContext
    try:
        ref = sim.run_simulation(p, str(tmp_path / "ref"), rng=np.random.default_rng(5), **kw)
    finally:
        hmc_mod.FermionContext = saved
    dev = sim.run_simulation(p, str(tmp_path / "dev"), rng=np.random.default_rng(5), **kw)
    assert dev.Nt_final == ref.Nt_final and len(dev.records) == len(ref.records) == 10
    fields = ("total_energy", "Delta_amp", "Delta_local", "Delta_global", "S_Delta", "hole_conc", "Delta_diff",
              "Delta_pair", "Delta_localpair")
    for (i, a1, dh1, o1), (j, a2, dh2, o2) in zip(dev.records, ref.records):
        assert i == j and a1 == a2
        assert abs(dh1 - dh2) <= 1e-8 * (1 + abs(dh2)), (i, dh1, dh2)
        for f in fields:
            assert abs(getattr(o1, f) - getattr(o2, f)) <= 1e-9, (i, f, getattr(o1, f), getattr(o2, f))
    assert [i for i, _ in dev.transport] == [i for i, _ in ref.transport] == [2, 4, 6, 8, 10]
    for (i, s1), (j, s2) in zip(dev.transport, ref.transport):
        for f in ("superfluid_stiffness", "dc_conductivity"):
            assert abs(getattr(s1, f) - getattr(s2, f)) <= 1e-8 * (1 + abs(getattr(s2, f))), (i, f)
        assert np.max(np.abs(s1.optical_conductivity - s2.optical_conductivity)) <= \
            1e-8 * (1 + np.max(np.abs(s2.optical_conductivity)))
    sq, sq_ref = np.load(tmp_path / "dev" / "field_sq.npy"), np.load(tmp_path / "ref" / "field_sq.npy")
    assert sq.shape == sq_ref.shape == (10, 2, 4, 6)
    assert np.max(np.abs(sq - sq_ref)) <= 1e-9
    s_delta = np.array([o.S_Delta for _, _, _, o in dev.records])
    assert np.max(np.abs(sq[:, 0, 0, 0] - s_delta)) <= 1e-12
    rows = (tmp_path / "dev" / "observables.csv").read_text().splitlines()
    for k, (i, acc, dH, obs) in enumerate(dev.records):
        assert rows[k + 1] == sim.obs_csv_line(i, acc, dH, obs).rstrip("\n")
