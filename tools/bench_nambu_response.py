"""Cross response of Nambu vertices at L x L, β = 16 (dwh_measure_nambu_response)
next to the operator response it generalises (dwh_measure_operator_response),
in one warm process, HIP-event timed ("nambu" / "operator" stage timers:
everything after the eigensolve), median [min, max] of the repetitions.  One
round runs the four calls nambu(n_w = 0), operator(n_w = 0), nambu(n_w),
operator(n_w) one after the other, so the two paths alternate call by call.

(a) n_w = 0: the "nambu" stage per vertex for 1, 4 and 8 lifted density
    vertices with their diagonal pairs against the "operator" stage per
    operator for the same vertices: the same product and the same apply; the
    new path keeps X resident and sums complex pairs.
(b) n_w = the transport grid's n_omega: the chi2 stage of either path, the
    difference of the two calls of one round, per pair / operator and as
    (pair·ω·operator)/s over all (2N)² ordered pairs.  The yardstick is the
    existing path in the same process.  For 4 and 8 pairs the new stage's
    median should lie below the old stage's [min, max]: one reciprocal serves
    4 pairs.  For 1 pair the ratio is recorded (complex weights cost one more
    fma per evaluation).
(c) 8 vertices with all 36 pairs a <= b, n_w as in (b): the chi2 stage per pair.

    python tools/bench_nambu_response.py [L] [reps] [out]

Writes the report to `out` (default profiles/nambu_response_L<L>.txt) as well
as to stdout.
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


def fmt(s):
    return f"{s[0]:8.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 10, 2)
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"nambu_response_L{L}.txt")
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
    # thermalised-like Δ: d-wave amplitude with site phase noise (as tools/bench_operator_response.py)
    D = st.Delta + 0.25 * np.stack([np.ones(p.N), -np.ones(p.N)], 1) * np.exp(0.3j * rng.standard_normal((p.N, 1)))
    ctx = m.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, st.disorder_pot)
    ctx.set_pairing(D)
    ctx.timing_enable(["operator", "nambu"])
    n2 = 2 * p.N
    flops = 8.0 * n2 ** 3
    nw, _ = m.transport_grid(ETA, DOMEGA, OMEGA_MAX)
    grid = (ETA, DOMEGA, nw)
    say(f"L={L} N={p.N} 2N={n2} beta={p.beta} n_matsubara={NL}; {reps} repetitions after 2 warm-up rounds, the calls "
        f"of a round alternated; median [min, max] of the HIP-event stage timers")
    qs = [(0, 1), (1, 0), (0, 0), (1, 1), (0, 2), (2, 0), (1, 2), (2, 1)]
    verts = [VX.density(p, mx, my) for mx, my in qs]
    lifted = [VX.nambu(v, p.N) for v in verts]

    def nambu(k, pairs, omega):
        ctx.timing_reset()
        ctx.measure_nambu_response(lifted[:k], pairs, n_matsubara=NL, omega=omega, eta=ETA)
        t, n, work = ctx.timing_read("nambu")
        assert n == 1 and work == flops * k
        return t

    def operator(k, omega):
        ctx.timing_reset()
        ctx.measure_operator_response(verts[:k], n_matsubara=NL, omega=omega, eta=ETA)
        t, n, work = ctx.timing_read("operator")
        assert n == 1 and work == flops * k
        return t

    rows = {}
    for k in (1, 4, 8):
        diag = [(a, a) for a in range(k)]
        t = np.array([(nambu(k, diag, None), operator(k, None), nambu(k, diag, grid), operator(k, grid))
                      for _ in range(reps + 2)][2:])
        rows[k] = dict(a_new=stats(t[:, 0] / k), a_old=stats(t[:, 1] / k), b_new=stats((t[:, 2] - t[:, 0]) / k),
                       b_old=stats((t[:, 3] - t[:, 1]) / k), w_new=stats(t[:, 2] / k), w_old=stats(t[:, 3] / k))
    say("(a) n_w = 0, lifted density vertices, diagonal pairs")
    for k in (1, 4, 8):
        r = rows[k]
        (o, olo, ohi), (n, _, _) = r["a_old"], r["a_new"]
        say(f"  {k} vertices: nambu stage per vertex {fmt(r['a_new'])}   operator stage per operator {fmt(r['a_old'])}   "
            f"nambu median inside the operator window: {olo <= n <= ohi}; ratio {n / o:.3f}")
    say(f"(b) n_w = {nw} (the transport grid η:Δω:ω_max = {ETA}:{DOMEGA}:{OMEGA_MAX}): chi2 stage = call with the grid - "
        f"call without, per round")
    for k in (1, 4, 8):
        r = rows[k]
        (n, _, _), (o, olo, _) = r["b_new"], r["b_old"]
        rate = lambda t: n2 * n2 * nw / t * 1e-9
        line = (f"  {k} pairs: nambu chi2 stage per pair {fmt(r['b_new'])} = {rate(n):6.2f} T(pair·ω·operator)/s   "
                f"operator chi2 stage per operator {fmt(r['b_old'])} = {rate(o):6.2f} T/s   ratio new/old {n / o:.3f}")
        if k > 1:
            line += f"   new median below the old window: {n < olo}"
        say(line)
        say(f"     whole stage per vertex: nambu {fmt(r['w_new'])}   operator {fmt(r['w_old'])}")
    k = 8
    tri = [(a, b) for a in range(k) for b in range(a, k)]
    t = np.array([(nambu(k, tri, None), nambu(k, tri, grid)) for _ in range(reps + 2)][2:])
    c2 = stats((t[:, 1] - t[:, 0]) / len(tri))
    say(f"(c) 8 vertices, all {len(tri)} pairs a <= b, n_w = {nw}: nambu stage {fmt(stats(t[:, 1]))}, without the grid "
        f"{fmt(stats(t[:, 0]))}; chi2 stage per pair {fmt(c2)} = {n2 * n2 * nw / c2[0] * 1e-9:6.2f} T(pair·ω·operator)/s")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
