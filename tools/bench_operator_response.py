"""Operator response χ(iΩ), χ''(ω) at L x L, β = 16 (dwh_measure_operator_response)
next to the current response it generalises, in one warm process, HIP-event
timed, median [min, max] of the repetitions:

(a) the "operator" stage per operator for 1, 4 and 8 density vertices with
    n_w = 0, alternated call by call with the "response" stage per momentum of
    measure_current_response for the same counts, and one complex 2N-cubed
    product of that shape alone (dwh_bench_response_product).  Both paths do
    the same product and the same pair sums, so the per-operator time should
    lie inside the alternation's [min, max] of the per-momentum time.  The
    same again with the x-current vertices of those momenta, the operator the
    "response" stage applies (12 entries per row instead of 1), which
    separates the path from the vertex.
(b) the same with n_w = the transport grid's n_omega: the difference to (a) is
    the χ'' kernels (k_op_spec + its sum), reported as (pair·ω)/s over all
    (2N)² ordered pairs and over the pairs of the tiles the kernel does not
    skip (counted on the host from E).  measure_transport runs in the same
    process; its σ(ω) kernel's time comes from a kernel trace of a separate
    run of this script (rocprofv3 --kernel-trace --stats -- python
    tools/bench_operator_response.py L reps), not from here.

    python tools/bench_operator_response.py [L] [reps] [out]

Writes the report to `out` (default profiles/operator_response_L<L>.txt) as
well as to stdout.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NL = 3
ETA, DOMEGA, OMEGA_MAX = 0.01, 0.002, 4.0


def stats(x):
    x = np.asarray(x)
    return float(np.median(x)), float(x.min()), float(x.max())


def live_pairs(E, beta, tile=256):
    """Pairs k_op_spec evaluates: per column m the 256-row tiles with any |f_n - f_m| >= 1e-12."""
    f = np.where(E >= 0, np.exp(-beta * np.abs(E)) / (1 + np.exp(-beta * np.abs(E))), 1 / (1 + np.exp(-beta * np.abs(E))))
    n2, live = len(E), 0
    for n0 in range(0, n2, tile):
        blk = f[n0:n0 + tile]
        live += int(np.sum(np.any(np.abs(blk[:, None] - f[None, :]) >= 1e-12, axis=0))) * tile
    return live


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 10, 2)
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"operator_response_L{L}.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import dwhmc_loader
    m = dwhmc_loader.load_package()
    VX = m.vertices
    p = m.ModelParameters(L, L, 1.0, -0.35, -1.08, 1.0, 0.1, 16.0, 0.8, 1.0)
    st = m.initialize_state(p, np.random.default_rng(7))
    rng = np.random.default_rng(11)
    # thermalised-like Δ: d-wave amplitude with site phase noise (as tools/bench_current_response.py)
    D = st.Delta + 0.25 * np.stack([np.ones(p.N), -np.ones(p.N)], 1) * np.exp(0.3j * rng.standard_normal((p.N, 1)))
    ctx = m.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, st.disorder_pot)
    ctx.set_pairing(D)
    ctx.timing_enable(["response", "operator"])
    n2 = 2 * p.N
    flops = 8.0 * n2 ** 3
    nw, _ = m.transport_grid(ETA, DOMEGA, OMEGA_MAX)
    say(f"L={L} N={p.N} 2N={n2} beta={p.beta} n_matsubara={NL}; {reps} repetitions after 2 warm-up rounds, the two "
        f"calls alternated; median [min, max] of the HIP-event stage timers")
    qs = [(0, 1), (1, 0), (0, 0), (1, 1), (0, 2), (2, 0), (1, 2), (2, 1)]
    verts = {"density": [VX.density(p, mx, my) for mx, my in qs],
             "current_x": [VX.current(p, mx, my, "x") for mx, my in qs]}
    tr = ctx.measure_transport(ETA, DOMEGA, OMEGA_MAX)        # (the σ(ω) kernel for the kernel trace; warms the slots)
    E, _ = ctx.eigensystem(vectors=False)
    live = live_pairs(E, p.beta)

    def round_of(k, n_w, kind):
        ctx.timing_reset()
        ctx.measure_operator_response(verts[kind][:k], n_matsubara=NL, omega=None if n_w == 0 else (ETA, DOMEGA, n_w),
                                      eta=ETA)
        t_op, n_op, work = ctx.timing_read("operator")
        assert n_op == 1 and work == flops * k
        ctx.measure_current_response(direction="x", q=qs[:k], n_matsubara=NL)
        t_rs, _, _ = ctx.timing_read("response")
        return t_op, t_rs

    res = {}
    for n_w, kind, tag in ((0, "density", "(a) n_w = 0, density vertices"),
                           (0, "current_x", "(a') n_w = 0, x-current vertices (the response stage's own operator)"),
                           (nw, "density", f"(b) n_w = {nw} (the transport grid η:Δω:ω_max = {ETA}:{DOMEGA}:{OMEGA_MAX}), "
                                           f"density vertices")):
        say(tag)
        for k in (1, 4, 8):
            t = np.array([round_of(k, n_w, kind) for _ in range(reps + 2)][2:])
            (o, olo, ohi), (r, rlo, rhi) = stats(t[:, 0] / k), stats(t[:, 1] / k)
            if kind == "density":
                res[(n_w, k)] = (o, olo, ohi, r, rlo, rhi)
            line = (f"  {k} operators: operator stage per operator {o:8.3f} ms [{olo:.3f}, {ohi:.3f}]   "
                    f"response stage per momentum {r:8.3f} ms [{rlo:.3f}, {rhi:.3f}]")
            if n_w == 0:
                inside = rlo <= o <= rhi
                overlap = olo <= rhi and rlo <= ohi
                line += f"   operator median inside the response window: {inside}; windows overlap: {overlap}"
            say(line)
    g, glo, ghi = stats([ctx.bench_response_product(10) for _ in range(reps)])
    say(f"one product of that shape alone: {g:8.3f} ms [{glo:.3f}, {ghi:.3f}]  ({flops / g * 1e-9:6.2f} TFLOP/s)")
    for k in (1, 4, 8):
        d = res[(nw, k)][0] - res[(0, k)][0]
        say(f"χ'' kernels, {k} operators: {d:8.3f} ms per operator = (b) - (a); {n2 * n2 * nw / d * 1e-9:8.2f} T(pair·ω)/s "
            f"over all (2N)² ordered pairs, {live * nw / d * 1e-9:8.2f} T(pair·ω)/s over the {live} pairs of the "
            f"{live // 256} tiles not skipped ({live / (n2 * n2):.3f} of all)")
    say(f"measure_transport ran in this process (σ(ω) on the same {nw} frequencies, stiffness "
        f"{tr['superfluid_stiffness']:.6f}); its k_tr_sigma time is read from a kernel trace of a separate run")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
