"""What an accepted trajectory costs under each HMC integrator,
at the bench's workload: C3 (L = 32, β = 16, bench.py's parameters, seeds and
thermalisation) unless L and β are given.

After bench.py's thermalisation (100 sweeps of leapfrog under the adaptive-Nt
rule from Nt = 10) every scheme runs the same K trajectories: from the same
thermalised state, with the same momentum draws, each of the same length T/2
(dt = calc_optimal_dt(β, J, m, Nt)).  A trajectory is dwh_hmc_trajectory
followed by dwh_hmc_finish with accepted = 0, which restores the start, so no
scheme sees another's end point.  The schemes alternate draw by draw, after
one untimed round.

Schemes: leapfrog at the thermalisation's final Nt and at Nt = 10; omelyan2 at
Nt = 1, 2, 3, 4; omelyan2 at Nt = 2 with λ = 0.18 and 0.21.

Per scheme: rms ΔH, ⟨min(1, e^-ΔH)⟩ (the expected acceptance), factorisations
per trajectory (checked against the "step" timer's launch count in the
untimed round), milliseconds per trajectory — HIP events on the context's
stream around dwh_hmc_trajectory: the noise upload, every launch of the
trajectory and the ΔH read-back; median [min, max] over the K draws — and
their quotient, ms per accepted trajectory (median ms / expected acceptance).

The headline is the omelyan2 row with the fewest factorisations whose
expected acceptance is at least leapfrog's at the thermalisation's Nt, and its
ms-per-accepted-trajectory ratio to that leapfrog row.

    python tools/bench_integrators.py [K] [out] [L] [beta]

Writes the report to `out` (default profiles/integrators_L<L>.txt) as well as
to stdout.  Needs the device; there is no CPU path.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAM = 0.1931833275037836


def main():
    K = max(int(sys.argv[1]) if len(sys.argv) > 1 else 64, 32)
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    beta = float(sys.argv[4]) if len(sys.argv) > 4 else 16.0
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", f"integrators_L{L}.txt")
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
    ctx.synchronize()
    info = ctx.info
    noise, _ = bench.synthetic_draws(m, p.N, 0, 1, K + 1, 17)
    stream = torch.cuda.ExternalStream(ctx.stream(), device=torch.device("cuda", 0))

    schemes = [("leapfrog", None, Nt_th), ("leapfrog", None, 10)]
    schemes += [("omelyan2", LAM, nt) for nt in (1, 2, 3, 4)]
    schemes += [("omelyan2", lam, 2) for lam in (0.18, 0.21)]
    if Nt_th == 10:
        schemes = schemes[1:]                    # (the two leapfrog rows coincide)
    nfact = [(1 if kind == "leapfrog" else 2) * nt for kind, _, nt in schemes]

    def trajectory(s, k):
        kind, lam, nt = schemes[s]
        ctx.set_integrator(kind, **({} if lam is None else {"lam": lam}))
        dt = m.calc_optimal_dt(p.beta, p.J, p.mass, nt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        dH = float(ctx.hmc_trajectory(noise[k], nt, dt, p.mass)[0])
        e1.record(stream)
        ctx.hmc_finish([0])                      # back to the common start
        e1.synchronize()
        return dH, e0.elapsed_time(e1)

    # the untimed round, which also counts the factorisations ("step" launches)
    ctx.timing_enable(["step"])
    for s in range(len(schemes)):
        ctx.timing_reset()
        trajectory(s, K)
        n = ctx.timing_read("step")[1]
        assert n == nfact[s], (schemes[s], n, nfact[s])
    ctx.timing_enable(False)
    cap0 = ctx.info["delta_cap"]
    dH = np.zeros((len(schemes), K))
    ms = np.zeros((len(schemes), K))
    for k in range(K):
        for s in range(len(schemes)):
            dH[s, k], ms[s, k] = trajectory(s, k)
    tripped = ctx.info["delta_cap"] != cap0
    ctx.close()

    say(f"L={L} N={p.N} beta={beta:g}, {info['npoles']} poles, algo {info['algo']}; measured on the device "
        f"({torch.cuda.get_device_name(0)})")
    say(f"thermalisation: 100 leapfrog sweeps, adaptive Nt 10 -> {Nt_th}, acceptance of the last 20: {acc_th:.2f}")
    say(f"{K} trajectories per scheme from the thermalised state, same momentum draws, length T/2 each, "
        f"schemes alternated draw by draw after one untimed round")
    say("ms/traj: HIP events around dwh_hmc_trajectory, median [min, max]; acc = <min(1, exp(-dH))>; "
        "ms/acc = median ms / acc")
    if tripped:
        say("NOTE: a guard trip re-selected the poles inside the timed loop; that trajectory ran twice and the "
            "later ones with more poles")
    say("")
    say(f"{'scheme':<28}{'fact.':>6}{'rms dH':>11}{'acc':>8}{'ms/traj':>10}  {'[min, max]':<18}{'ms/acc':>9}")
    acc = np.minimum(1.0, np.exp(-dH)).mean(axis=1)
    med = np.median(ms, axis=1)
    per_acc = med / acc
    for s, (kind, lam, nt) in enumerate(schemes):
        name = f"{kind} Nt={nt}" + ("" if lam is None else f" lam={lam:.10g}")
        say(f"{name:<28}{nfact[s]:>6}{np.sqrt(np.mean(dH[s] ** 2)):>11.4f}{acc[s]:>8.3f}{med[s]:>10.3f}  "
            f"{'[%.3f, %.3f]' % (ms[s].min(), ms[s].max()):<18}{per_acc[s]:>9.3f}")
    say("")
    om2 = [s for s, (kind, lam, _) in enumerate(schemes) if kind == "omelyan2" and lam == LAM and acc[s] >= acc[0]]
    if om2:
        s = min(om2, key=lambda q: nfact[q])
        say(f"headline: omelyan2 Nt={schemes[s][2]} ({nfact[s]} factorisations, acc {acc[s]:.3f}) against leapfrog "
            f"Nt={schemes[0][2]} ({nfact[0]} factorisations, acc {acc[0]:.3f}): {per_acc[s]:.3f} against "
            f"{per_acc[0]:.3f} ms per accepted trajectory, ratio {per_acc[s] / per_acc[0]:.3f} "
            f"({per_acc[0] / per_acc[s]:.2f}x)")
    else:
        say(f"headline: no omelyan2 row up to Nt=4 reaches leapfrog Nt={schemes[0][2]}'s acc {acc[0]:.3f}: "
            "no gain measured at this size")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
