"""What a measurement sweep costs through the drivers' loop, on the throughput
path, and on the throughput path with the sweep log, at the
bench's workload: C3 (L = 32, β = 16, bench.py's parameters, seeds and
thermalisation) unless L and β are given.

Three legs, each M sweeps from the same thermalised state with the same draws,
each a host clock around work that ends in a synchronise:

  (A) the driver's loop of sweep_batch=None: per sweep hmc.hmc_sweep (injected
      noise and uniform) and hmc.measure_observables
  (B) load_draws + run_sweeps with the log off + sweep_results
  (C) load_draws + run_sweeps with observables, field_sq and a snapshot of
      every sweep logged + sweep_results and the three logs read back

for leapfrog Nt = 5 (the drivers' default Nt_measure) and omelyan2 Nt = 2.
One process; the legs alternate repeat by repeat after one untimed round, in
which the "sweep_log" timer counts the log's launches and their device time.
Every leg starts from the thermalised Δ, refactorised before the clock starts.

    python tools/bench_sweep_log.py [R] [out] [M] [L] [beta]

R repeats (default 9) of M sweeps (default 20).  Writes the report to `out`
(default profiles/sweep_log_L<L>.txt) as well as to stdout.  Needs the device.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = (("leapfrog", 5), ("omelyan2", 2))


def main():
    R = max(int(sys.argv[1]) if len(sys.argv) > 1 else 9, 3)
    M = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    L = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    beta = float(sys.argv[5]) if len(sys.argv) > 5 else 16.0
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", f"sweep_log_L{L}.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch

    import bench
    import dwhmc_loader
    m = dwhmc_loader.load_package()
    m.load_library(build_if_missing=False)
    p = m.ModelParameters(L, L, 1.0, -0.35, -1.08, 1.0, 0.05, beta, 0.8, 1.0)
    dis, D0 = bench.synthetic_state(m, p, 0, 1)
    ctx = m.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, dis)
    ctx.set_pairing(D0)
    ctx.factorize()
    Nt_th, acc_th = bench.thermalise(m, ctx, p, 0, 1, 100, 10)
    start = ctx.get_state()[0]
    info = ctx.info
    noise, uni = bench.synthetic_draws(m, p.N, 0, 1, M, 17)
    cache = m.initialize_cache(p)
    cache.ctx = ctx

    def reset():
        ctx.set_state(start, None)
        ctx.factorize()

    def leg_a(Nt, dt):
        state = m.SimulationState(dis[0], start[0].copy(), np.zeros_like(start[0]))
        reset()
        t0 = time.perf_counter()
        for k in range(M):
            m.hmc_sweep(cache, p, state, Nt=Nt, dt=dt, noise=noise[k, 0], uniform=float(uni[k, 0]))
            m.measure_observables(cache, p, state)
        return time.perf_counter() - t0

    def leg_b(Nt, dt):
        ctx.sweep_log(observables=False)
        reset()
        t0 = time.perf_counter()
        ctx.load_draws(noise, uni)
        ctx.run_sweeps(0, M, Nt, dt, p.mass)
        ctx.sweep_results(0, M)
        return time.perf_counter() - t0

    def leg_c(Nt, dt):
        ctx.load_draws(noise, uni)                 # (sizes the log; the timed region uploads again)
        ctx.sweep_log(observables=True, field_sq=True, snapshot_every=1)
        reset()
        t0 = time.perf_counter()
        ctx.load_draws(noise, uni)
        ctx.run_sweeps(0, M, Nt, dt, p.mass)
        ctx.sweep_results(0, M)
        ctx.sweep_observables(0, M)
        ctx.sweep_field_sq(0, M)
        ctx.sweep_snapshots(0, M)
        return time.perf_counter() - t0

    legs = (leg_a, leg_b, leg_c)
    ms = np.zeros((len(SETTINGS), 3, R))
    log_us, log_n = [], []
    cap0 = ctx.info["delta_cap"]
    for s, (kind, Nt) in enumerate(SETTINGS):
        ctx.set_integrator(kind)
        dt = m.calc_optimal_dt(p.beta, p.J, p.mass, Nt)
        # the untimed round; its leg (C) reads the log's own timer
        leg_a(Nt, dt)
        leg_b(Nt, dt)
        ctx.timing_enable(["sweep_log"])
        ctx.timing_reset()
        leg_c(Nt, dt)
        t_ms, n, _ = ctx.timing_read("sweep_log")
        ctx.timing_enable(False)
        log_us.append(1e3 * t_ms / M)
        log_n.append(n / M)
        for r in range(R):
            for k, leg in enumerate(legs):
                ms[s, k, r] = 1e3 * leg(Nt, dt) / M
    tripped = ctx.info["delta_cap"] != cap0
    ctx.sweep_log(observables=False)
    ctx.close()

    say(f"L={L} N={p.N} beta={beta:g}, {info['npoles']} poles, algo {info['algo']}; measured on the device "
        f"({torch.cuda.get_device_name(0)})")
    say(f"thermalisation: 100 leapfrog sweeps, adaptive Nt 10 -> {Nt_th}, acceptance of the last 20: {acc_th:.2f}")
    say(f"{R} repeats of {M} sweeps per leg from the thermalised state, same draws, legs alternated repeat by "
        f"repeat after one untimed round; host clock, every leg ends in a synchronise")
    say("(A) hmc.hmc_sweep + hmc.measure_observables per sweep; (B) load_draws + run_sweeps (log off) + "
        "sweep_results; (C) as (B) with observables, field_sq and a snapshot logged every sweep and all three read back")
    say("ms per sweep: median [min, max] over the repeats; log: the \"sweep_log\" timer of the untimed round, "
        "device time of its launches per sweep")
    if tripped:
        say("NOTE: a guard trip re-selected the poles inside the timed loops")
    say("")
    say(f"{'setting':<18}{'leg':<5}{'ms/sweep':>10}  {'[min, max]':<20}")
    med = np.median(ms, axis=2)
    for s, (kind, Nt) in enumerate(SETTINGS):
        for k, name in enumerate("ABC"):
            say(f"{kind + ' Nt=' + str(Nt):<18}{'(' + name + ')':<5}{med[s, k]:>10.3f}  "
                f"{'[%.3f, %.3f]' % (ms[s, k].min(), ms[s, k].max()):<20}")
        say(f"{'':<18}log  {log_us[s]:>8.1f} us per sweep in {log_n[s]:.0f} launches")
        say(f"{'':<18}(A) - (B) = {med[s, 0] - med[s, 1]:.3f} ms, (C) - (B) = {med[s, 2] - med[s, 1]:.3f} ms, "
            f"(C) / (A) = {med[s, 2] / med[s, 0]:.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
