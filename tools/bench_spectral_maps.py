"""Spectral maps LDOS(i, ω) / A(k, ω) at L x L, β = 16 (dwh_measure_spectral_maps):
the map stage by the "spectral" timer for both routes (DWHMC_SPECTRAL_FUSED=1:
the fused k_sp_maps / 0: k_sp_sqmod + gemm_d) in one process, interleaved
repetition by repetition, for one state and 8 snapshots, the full 4001-point
window and stride 10; the same calls' eigensolve ("eig_own") for scale; and
the host-numpy time for the same maps from a downloaded U.

    python tools/bench_spectral_maps.py [L] [reps]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = (("fused", "1"), ("unfused", "0"))   # DWHMC_SPECTRAL_FUSED


def set_route(val):
    if val is None:
        os.environ.pop("DWHMC_SPECTRAL_FUSED", None)
    else:
        os.environ["DWHMC_SPECTRAL_FUSED"] = val


def stats(x):
    x = np.asarray(x)
    return float(np.median(x)), float(x.min()), float(x.max())


def numpy_maps(E, U, p, omega):
    N = p.N
    lam = (1.0 / np.pi) * (p.eta / ((omega[None, :] - E[:, None]) ** 2 + p.eta ** 2))
    u = U[:N]
    ldos = (np.abs(u) ** 2) @ lam
    uk = np.fft.fft2(u.T.reshape(2 * N, p.Ly, p.Lx), axes=(1, 2)).reshape(2 * N, N)
    akw = (np.abs(uk) ** 2 / N).T @ lam
    return ldos, akw


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 10, 2)
    import dwhmc_loader
    m = dwhmc_loader.load_package()
    p = m.ModelParameters(L, L, 1.0, -0.35, -1.08, 1.0, 0.1, 16.0, 0.8, 1.0)
    st = m.initialize_state(p, np.random.default_rng(7))
    rng = np.random.default_rng(11)
    # thermalised-like Δ: d-wave amplitude with site phase noise
    D = st.Delta + 0.25 * np.stack([np.ones(p.N), -np.ones(p.N)], 1) * np.exp(0.3j * rng.standard_normal((p.N, 1)))
    snaps = np.stack([D + 0.01 * k * rng.standard_normal((p.N, 2)) for k in range(8)])
    ctx = m.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, st.disorder_pot)
    ctx.set_pairing(D)
    ctx.timing_enable(["spectral", "eig_own"])
    _, nd = m.transport_grid(p.eta, p.domega, p.omega_max)
    print(f"L={L} N={p.N} 2N={2 * p.N} beta={p.beta} DOS grid {nd} points; {reps} repetitions after 2 warm-up "
          f"calls, routes interleaved; median [min, max]", flush=True)
    verdict = []
    for ns, deltas in ((1, None), (8, snaps)):
        for stride in (1, 10):
            args = dict(first=0, count=None, stride=stride, deltas=deltas)
            ms = {r: [] for r, _ in ROUTES}
            eig = {r: [] for r, _ in ROUTES}
            wall = {r: [] for r, _ in ROUTES}
            work = 0.0
            for rep in range(reps + 2):
                for name, val in ROUTES:
                    set_route(val)
                    ctx.timing_reset()
                    t0 = time.perf_counter()
                    r = ctx.measure_spectral_maps(p.eta, p.domega, p.omega_max, **args)
                    dt = time.perf_counter() - t0
                    if rep < 2:
                        continue
                    t_sp, _, work = ctx.timing_read("spectral")
                    t_eig, _, _ = ctx.timing_read("eig_own")
                    ms[name].append(t_sp)
                    eig[name].append(t_eig)
                    wall[name].append(1e3 * dt)
            count = len(r["omega"])
            print(f"\n{ns} state(s), stride {stride}: count {count}, {work:.3e} flops (2 maps)", flush=True)
            for name, _ in ROUTES:
                md, lo, hi = stats(ms[name])
                print(f"  {name:8s} map stage {md:8.3f} ms [{lo:.3f}, {hi:.3f}]  {work / md * 1e-9:7.2f} TFLOP/s   "
                      f"eigensolve {stats(eig[name])[0]:8.2f} ms   call wall {stats(wall[name])[0]:8.1f} ms", flush=True)
            f, u = stats(ms["fused"]), stats(ms["unfused"])
            spread = max(f[2] - f[1], u[2] - u[1])
            verdict.append((ns, stride, u[0] - f[0], spread))
    set_route(None)
    print("\nA/B (unfused - fused medians against the larger min-max spread of the two):")
    for ns, stride, d, spread in verdict:
        print(f"  {ns} state(s), stride {stride}: {d:+.3f} ms, spread {spread:.3f} ms -> "
              f"{'fused faster' if d > spread else 'unfused faster' if -d > spread else 'within the spread'}")
    # what a user does without the entry: download U, numpy on the host
    t0 = time.perf_counter()
    E, U = ctx.eigensystem(0)
    t_dl = 1e3 * (time.perf_counter() - t0)
    print(f"\nhost numpy, one state (eigensystem with the {U.nbytes / 2**20:.0f} MiB U downloaded: {t_dl:.1f} ms):")
    for stride in (1, 10):
        omega = m.spectral_window(p.eta, p.domega, p.omega_max, 0, None, stride)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ldos, akw = numpy_maps(E, np.ascontiguousarray(U), p, omega)
            ts.append(1e3 * (time.perf_counter() - t0))
        r = ctx.measure_spectral_maps(p.eta, p.domega, p.omega_max, 0, None, stride)
        err = max(np.max(np.abs(r["ldos"][0].reshape(len(omega), -1).T - ldos)),
                  np.max(np.abs(r["akw"][0].reshape(len(omega), -1).T - akw)))
        print(f"  stride {stride}: numpy maps {stats(ts)[0]:.1f} ms [{min(ts):.1f}, {max(ts):.1f}] "
              f"({os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}); "
              f"max |device - numpy| {err:.2e}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
