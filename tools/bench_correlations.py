"""Equal-time correlations at L x L, β = 16 (dwh_measure_correlations) with 1
and with 4 snapshots, in one warm process, HIP-event timed by the call's own
stage timers ("corr_rho", "corr_contract", "corr_reduce"), median [min, max]
of the repetitions.  One round runs, one after the other, the call for each
pair and snapshot count and after each the product yardstick
(dwh_bench_response_product, the 2N-cubed complex product): the paths
alternate call by call.

Per state it reports the ρ product (S = diag(f) U^H and ρ = U S), the
contraction of one pair for (density, density), (pair_d_create, pair_d_create)
and (pair_d_amplitude, pair_d_amplitude) — 2·2, 4·4 and 8·8 term pairs per
pair of sites — and the chunk reduction, each over the yardstick, and the
contraction's bytes counted two ways: unique (ρ once, (2N)² · 16 B) and
issued (two 16-byte loads per term pair and pair of sites, 2·T_A·T_B·N²·16 B).

    python tools/bench_correlations.py [L] [reps] [out]

Writes the report to `out` (default profiles/correlations_L<L>.txt) as well as
to stdout.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("density", "pair_d_create", "pair_d_amplitude")
STAGES = ("corr_rho", "corr_contract", "corr_reduce")


def stats(x):
    x = np.asarray(x)
    return float(np.median(x)), float(x.min()), float(x.max())


def fmt(s):
    return f"{s[0]:8.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 10, 2)
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"correlations_L{L}.txt")
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
    # thermalised-like Δ: d-wave amplitude with site phase noise (as tools/bench_response_map.py)
    D = st.Delta + 0.25 * np.stack([np.ones(p.N), -np.ones(p.N)], 1) * np.exp(0.3j * rng.standard_normal((p.N, 1)))
    fields = np.stack([D * np.exp(0.1j * k) for k in range(4)])
    ctx = m.FermionContext(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, st.disorder_pot)
    ctx.set_pairing(D)
    ctx.timing_enable(STAGES)
    n2 = 2 * p.N
    flops = 8.0 * n2 ** 3
    fams = [VX.local_family(k, p) for k in KINDS]
    terms = [len(f.val) // p.N for f in fams]
    say(f"L={L} N={p.N} 2N={n2} beta={p.beta}; families {', '.join(f'{k} ({t} terms per site)' for k, t in zip(KINDS, terms))}; "
        f"{reps} repetitions after 2 warm-up rounds, the calls of a round alternated; per state, median [min, max]")

    def run(k, ns):
        ctx.timing_reset()
        ctx.measure_correlations([fams[k]], mean=False, deltas=fields[:ns])
        out = []
        for name in STAGES:
            t, n, work = ctx.timing_read(name)
            assert n == ns
            out.append(t / ns)
        return out

    cases = [(k, ns) for ns in (1, 4) for k in range(len(KINDS))]
    rounds = []
    for _ in range(reps + 2):
        row = []
        for k, ns in cases:
            row.append(run(k, ns) + [ctx.bench_response_product(10)])
        rounds.append(row)
    t = np.array(rounds[2:])                                                    # (rep, case, stage + yardstick)
    prod = stats(t[:, :, 3].ravel())
    say(f"the product yardstick (dwh_bench_response_product): {fmt(prod)} = {flops / prod[0] * 1e-9:.1f} TFLOP/s")
    unique = n2 * n2 * 16.0
    for c, (k, ns) in enumerate(cases):
        issued = 2.0 * terms[k] * terms[k] * p.N * p.N * 16.0
        rho, con, red = (stats(t[:, c, s]) for s in range(3))
        rc = stats(t[:, c, 1] / t[:, c, 3])
        say(f"{ns} snapshot{'s' if ns > 1 else ' '} ({KINDS[k]}, {KINDS[k]}), {terms[k]}·{terms[k]} term pairs:")
        say(f"    rho product    {fmt(rho)} = {stats(t[:, c, 0] / t[:, c, 3])[0]:.2f} products")
        say(f"    contraction    {fmt(con)} = {rc[0]:.3f} products [{rc[1]:.3f}, {rc[2]:.3f}]; unique bytes "
            f"{unique / 1e6:.1f} MB = {unique / con[0] * 1e-6:.0f} GB/s, issued bytes {issued / 1e9:.3f} GB = "
            f"{issued / con[0] * 1e-6:.0f} GB/s"
            f"{'' if rc[0] <= 1 else '   ABOVE 1: the contraction costs more than the product it follows'}")
        say(f"    chunk sum      {fmt(red)} = {stats(t[:, c, 2] / t[:, c, 3])[0]:.4f} products")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
