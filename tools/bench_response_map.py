"""Response maps at L x L, β = 16 (dwh_measure_response_map): one source vertex,
the q = 0 x current, on the whole vertices.bond_pattern (36 N entries), with 1
and with 4 Matsubara frequencies, in one warm process, HIP-event timed, median
[min, max] of the repetitions.  One round runs, one after the other,
map(1 frequency), the product yardstick, map(4 frequencies), the product
yardstick: the paths alternate call by call.

(a) the "map" stage timer (everything after the eigensolve: U^H, W U, X, and per
    frequency the weight kernel, the product S = K U^H and the sampled product)
    per (vertex, frequency), next to dwh_bench_response_product, the 2N-cubed
    complex product the library runs per vertex and per frequency;
(b) the stages around the product on their own (dwh_bench_response_map_stages):
    the weight kernel and the sampled product per frequency, and their sum over
    the product yardstick.  The sampled product's rate is over its algorithmic
    bytes: per entry one column of U^H (2N complex), per workgroup slice one
    staged column of S (2N complex), 16 bytes per entry written; the weight
    kernel's over X read once and one K written per frequency.

    python tools/bench_response_map.py [L] [reps] [out]

Writes the report to `out` (default profiles/response_map_L<L>.txt) as well as
to stdout.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLICE = 32          # entries per workgroup of the sampled product (kMapSlice, csrc/dwhmc_internal.h)


def stats(x):
    x = np.asarray(x)
    return float(np.median(x)), float(x.min()), float(x.max())


def fmt(s):
    return f"{s[0]:8.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = max(int(sys.argv[2]) if len(sys.argv) > 2 else 10, 2)
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", f"response_map_L{L}.txt")
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
    ctx.timing_enable(["map"])
    n2 = 2 * p.N
    flops = 8.0 * n2 ** 3
    src = [VX.nambu(VX.current(p, 0, 0, "x"), p.N)]
    pat = VX.bond_pattern(p)
    npat = len(pat)
    nslices = int(np.sum(-(-np.bincount(pat[:, 1], minlength=n2) // SLICE)))
    say(f"L={L} N={p.N} 2N={n2} beta={p.beta}; source current_x(0,0), pattern bond_pattern: {npat} entries in "
        f"{nslices} workgroup slices; {reps} repetitions after 2 warm-up rounds, the calls of a round alternated; "
        f"median [min, max]")

    def run_map(nz):
        ctx.timing_reset()
        ctx.measure_response_map(src, pat, n_matsubara=nz, rho=False)
        t, n, work = ctx.timing_read("map")
        assert n == 1 and work == flops * (1 + nz)
        return t

    t = np.array([(run_map(1), ctx.bench_response_product(10), run_map(4), ctx.bench_response_product(10))
                  for _ in range(reps + 2)][2:])
    prod = stats(np.concatenate([t[:, 1], t[:, 3]]))
    say(f"(a) the product yardstick (dwh_bench_response_product): {fmt(prod)} = {flops / prod[0] * 1e-9:.1f} TFLOP/s")
    for nz, col in ((1, 0), (4, 2)):
        s = stats(t[:, col] / nz)
        per_freq = stats((t[:, 2] - t[:, 0]) / 3)
        say(f"  {nz} frequenc{'y' if nz == 1 else 'ies'}: \"map\" stage per (vertex, frequency) {fmt(s)} = "
            f"{s[0] / prod[0]:.2f} products (its {1 + nz} products, U^H, W U, weights, sampling and the copy out)")
    say(f"  each further frequency (4 - 1 frequencies, per round): {fmt(per_freq)} = {per_freq[0] / prod[0]:.2f} products")
    # the stages on their own, on the buffers the 4-frequency call left
    sb = npat * (n2 * 16 + 16) + nslices * n2 * 16
    wb = lambda nz: (1 + nz) * n2 * n2 * 16
    say(f"(b) the stages around the product (dwh_bench_response_map_stages), per frequency; algorithmic bytes: "
        f"sampled product {sb / 1e9:.3f} GB per frequency ({npat} columns of U^H + {nslices} staged columns of S + the "
        f"entries), weight kernel {wb(1) / 1e9:.3f} GB for one frequency, {wb(4) / 1e9:.3f} GB for four")
    for nz in (1, 4):
        ts = np.array([(ctx.bench_response_map_stages(10, nz), ctx.bench_response_product(10))
                       for _ in range(reps + 2)][2:], dtype=object)
        w = stats([a[0] / nz for a, _ in ts])
        sp = stats([a[1] / nz for a, _ in ts])
        pr = stats([b for _, b in ts])
        ratio = stats([(a[0] + a[1]) / nz / b for a, b in ts])
        say(f"  {nz} frequenc{'y' if nz == 1 else 'ies'} per launch: weight kernel {fmt(w)} = "
            f"{wb(nz) / nz / w[0] * 1e-6:.0f} GB/s   sampled product {fmt(sp)} = {sb / sp[0] * 1e-6:.0f} GB/s   "
            f"product {fmt(pr)}")
        say(f"     (weight + sampled product) / product = {ratio[0]:.2f} [{ratio[1]:.2f}, {ratio[2]:.2f}]"
            f"{'' if ratio[0] <= 1 else '   ABOVE 1: the stages after the product cost more than the product'}")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
