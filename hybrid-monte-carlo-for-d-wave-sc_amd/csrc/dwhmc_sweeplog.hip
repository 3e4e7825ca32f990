// The sweep log of the throughput path (dwh_sweep_log): per sweep of
// dwh_run_sweeps and per chain, the observables record, the pairing field's
// structure factors S_d(q), S_s(q) and snapshots of Δ, written by launches
// that follow k_traj_end, so from the accepted or restored Δ, P, E_f and
// Tr ρ_hh.  Every kernel takes the batch's halt word and returns when a guard
// trip stopped the batch (SweepHalt, dwhmc_internal.h): the tripped sweep and
// the later ones log nothing, and the replay logs them.  Every sum has a fixed
// order and there are no atomics, so a replayed sweep logs the same bits.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

// Observables record of one chain (src/Observables.jl:88-222 from the
// factorisation outputs, hmc.observables_from_outputs): one workgroup of 256
// threads, sites strided over the threads, block_sum256's order.  Δ and P are
// (2, N) per chain: +x bonds, then +y bonds.
__global__ __launch_bounds__(256) void k_log_obs(const double2* __restrict__ Delta, const double2* __restrict__ Pair,
                                                 const double* __restrict__ Ef, const double* __restrict__ Trhh,
                                                 int N, double beta, double J, double* __restrict__ out,
                                                 const int* __restrict__ halt) {
  if (halt[0] != 0) return;
  const int c = blockIdx.x;
  __shared__ double red[4];
  const double2* D = Delta + (int64_t)c * 2 * N;
  const double2* P = Pair + (int64_t)c * 2 * N;
  double sq = 0.0, amp = 0.0, loc = 0.0, gr = 0.0, gi = 0.0, dif = 0.0, tr = 0.0, ti = 0.0, ta = 0.0;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const double2 dx = D[i], dy = D[N + i], px = P[i], py = P[N + i];
    sq += (dx.x * dx.x + dx.y * dx.y) + (dy.x * dy.x + dy.y * dy.y);
    amp += 0.5 * (hypot(dx.x, dx.y) + hypot(dy.x, dy.y));
    const double2 d = make_double2(0.5 * (dx.x - dy.x), 0.5 * (dx.y - dy.y));
    loc += hypot(d.x, d.y);
    gr += d.x;
    gi += d.y;
    dif += 0.5 * (hypot(dx.x - J * px.x, dx.y - J * px.y) + hypot(dy.x - J * py.x, dy.y - J * py.y));
    const double2 t = make_double2(J * 0.5 * (px.x - py.x), J * 0.5 * (px.y - py.y));
    tr += t.x;
    ti += t.y;
    ta += hypot(t.x, t.y);
  }
  sq = block_sum256(sq, red);
  amp = block_sum256(amp, red);
  loc = block_sum256(loc, red);
  gr = block_sum256(gr, red);
  gi = block_sum256(gi, red);
  dif = block_sum256(dif, red);
  tr = block_sum256(tr, red);
  ti = block_sum256(ti, red);
  ta = block_sum256(ta, red);
  if (threadIdx.x != 0) return;
  const double n = (double)N, g = hypot(gr / n, gi / n);
  double* o = out + (int64_t)c * kObsFields;
  o[0] = (Ef[c] + beta / (2.0 * J) * sq) / n;   // total_energy
  o[1] = amp / n;                               // Δ_amp
  o[2] = loc / n;                               // Δ_local
  o[3] = g;                                     // Δ_global
  o[4] = g * g;                                 // S_Δ
  o[5] = 2.0 * Trhh[c] / n - 1.0;               // hole_conc
  o[6] = dif / n;                               // Δ_diff
  o[7] = hypot(tr / n, ti / n);                 // Δ_pair
  o[8] = ta / n;                                // Δ_localpair
  o[9] = Ef[c];
  o[10] = Trhh[c];
  o[11] = sq;
}

// e^{-2πi k/L} for 0 <= k < L
__device__ __forceinline__ double2 twiddle(int k, int L) {
  double s, c;
  sincospi(2.0 * (double)k / (double)L, &s, &c);
  return make_double2(c, -s);
}

// S_ch(q) = |(1/N) Σ_i f_i e^{-2πi (kx x / Lx + ky y / Ly)}|², q = kx + Lx ky,
// of f = d (blockIdx.x = 0) or s (1) for chain blockIdx.y: f staged in LDS,
// then a row and a column DFT for any Lx, Ly (the lattice need not be a power
// of two), every sum in ascending order, the phase index reduced modulo L as
// an integer before it becomes an angle.  Dynamic LDS: 2 N double2.
__global__ __launch_bounds__(256) void k_log_field_sq(const double2* __restrict__ Delta, int Lx, int Ly,
                                                      double* __restrict__ out, const int* __restrict__ halt) {
  if (halt[0] != 0) return;
  extern __shared__ double2 lds[];
  const int N = Lx * Ly, ch = blockIdx.x, c = blockIdx.y;
  double2* f = lds;
  double2* g = lds + N;
  const double2* D = Delta + (int64_t)c * 2 * N;
  const double sg = ch == 0 ? -0.5 : 0.5;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const double2 dx = D[i], dy = D[N + i];
    f[i] = make_double2(0.5 * dx.x + sg * dy.x, 0.5 * dx.y + sg * dy.y);
  }
  __syncthreads();
  // rows: g[kx + Lx y] = Σ_x f[x + Lx y] e^{-2πi kx x / Lx}
  for (int o = threadIdx.x; o < N; o += blockDim.x) {
    const int kx = o % Lx;
    const double2* row = f + (o - kx);
    double2 a = make_double2(0.0, 0.0);
    int ph = 0;
    for (int x = 0; x < Lx; ++x) {
      a = cadd(a, cmul(row[x], twiddle(ph, Lx)));
      ph += kx;
      if (ph >= Lx) ph -= Lx;
    }
    g[o] = a;
  }
  __syncthreads();
  // columns: Σ_y g[kx + Lx y] e^{-2πi ky y / Ly}
  double* S = out + ((int64_t)c * 2 + ch) * N;
  const double inv = 1.0 / (double)N;
  for (int o = threadIdx.x; o < N; o += blockDim.x) {
    const int kx = o % Lx, ky = o / Lx;
    double2 a = make_double2(0.0, 0.0);
    int ph = 0;
    for (int y = 0; y < Ly; ++y) {
      a = cadd(a, cmul(g[kx + Lx * y], twiddle(ph, Ly)));
      ph += ky;
      if (ph >= Ly) ph -= Ly;
    }
    a = make_double2(a.x * inv, a.y * inv);
    S[o] = a.x * a.x + a.y * a.y;
  }
}

__global__ __launch_bounds__(256) void k_log_snapshot(const double2* __restrict__ Delta, int64_t n,
                                                      double2* __restrict__ out, const int* __restrict__ halt) {
  if (halt[0] != 0) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = Delta[i];
}

}  // namespace

void launch_log_obs(const Dims& d, const double2* Delta, const double2* Pair, const double* Ef, const double* Trhh,
                    double beta, double J, double* out, const int* halt, hipStream_t s) {
  hipLaunchKernelGGL(k_log_obs, dim3(d.nc), dim3(256), 0, s, Delta, Pair, Ef, Trhh, d.N, beta, J, out, halt);
}

int launch_log_field_sq(const Dims& d, int Lx, int Ly, const double2* Delta, double* out, const int* halt,
                        hipStream_t s) {
  if (Lx < 1 || Ly < 1 || Lx * Ly != d.N || d.N > kLogSqMaxN) return -1;
  const size_t lds = 2 * sizeof(double2) * (size_t)d.N;
  // above the default 64 KiB per workgroup the size has to be asked for (per
  // device, so with the launch and not once per process)
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_log_field_sq), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(k_log_field_sq, dim3(2, d.nc), dim3(256), lds, s, Delta, Lx, Ly, out, halt);
  return 0;
}

void launch_log_snapshot(const Dims& d, const double2* Delta, double2* out, const int* halt, hipStream_t s) {
  const int64_t n = (int64_t)d.nc * 2 * d.N;
  hipLaunchKernelGGL(k_log_snapshot, dim3(cdiv(n, 256)), dim3(256), 0, s, Delta, n, out, halt);
}

}  // namespace dwh
