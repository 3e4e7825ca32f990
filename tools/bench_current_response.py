"""Current response Λ(q, iΩ) at L x L, β = 16 (dwh_measure_current_response):
the stage after the eigensolve by the "response" timer for nq = 1, 4 and 8
momenta (n_matsubara = 3, direction x), the same calls' eigensolve
("eig_own"), and, in the same process, one complex 2N-cubed product of the
shape the stage runs per momentum (dwh_bench_response_product): the yardstick
for the per-momentum time.  Warm, HIP-event timed, medians of the repetitions.

    python tools/bench_current_response.py [L] [reps]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NL = 3


def stats(x):
    x = np.asarray(x)
    return float(np.median(x)), float(x.min()), float(x.max())


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
    ctx = m.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, st.disorder_pot)
    ctx.set_pairing(D)
    ctx.timing_enable(["response", "eig_own"])
    n2 = 2 * p.N
    flops = 8.0 * n2 ** 3
    print(f"L={L} N={p.N} 2N={n2} beta={p.beta} n_matsubara={NL} direction x; {reps} repetitions after 2 warm-up "
          f"calls; median [min, max]", flush=True)
    qs = [(0, 1), (1, 0), (0, 0), (1, 1), (0, 2), (2, 0), (1, 2), (2, 1)]
    per_q = {}
    for nq in (1, 4, 8):
        ms, eig, wall = [], [], []
        for rep in range(reps + 2):
            ctx.timing_reset()
            t0 = time.perf_counter()
            r = ctx.measure_current_response(direction="x", q=qs[:nq], n_matsubara=NL)
            dt = time.perf_counter() - t0
            if rep < 2:
                continue
            t_rs, _, work = ctx.timing_read("response")
            t_eig, _, _ = ctx.timing_read("eig_own")
            assert work == flops * nq
            ms.append(t_rs)
            eig.append(t_eig)
            wall.append(1e3 * dt)
        md, lo, hi = stats(ms)
        per_q[nq] = md / nq
        print(f"nq={nq}: response stage {md:9.3f} ms [{lo:.3f}, {hi:.3f}]  per momentum {md / nq:8.3f} ms "
              f"({flops * nq / md * 1e-9:6.2f} TFLOP/s of the product's flops)   eigensolve {stats(eig)[0]:8.2f} ms   "
              f"call wall {stats(wall)[0]:8.1f} ms   stiffness(q[0]) {r['dia'] - r['lam'][0, 0]:.6f}", flush=True)
    gm = [ctx.bench_response_product(10) for _ in range(reps)]
    g, glo, ghi = stats(gm)
    print(f"one product of that shape alone: {g:8.3f} ms [{glo:.3f}, {ghi:.3f}]  ({flops / g * 1e-9:6.2f} TFLOP/s)",
          flush=True)
    for nq in (1, 4, 8):
        rest = per_q[nq] - g
        print(f"nq={nq}: per momentum / product = {per_q[nq] / g:.3f}; everything around the product "
              f"(current apply, pair sums, reductions; U^H and dia once per state) {rest:+.3f} ms per momentum -> "
              f"{'LONGER than the product: the kernels around it are the path to work on' if rest > g else 'shorter than the product'}",
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
