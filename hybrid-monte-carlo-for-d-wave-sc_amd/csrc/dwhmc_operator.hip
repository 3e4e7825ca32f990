// Response of any one-body operator (dwh_measure_operator_response):
//   O = Σ_ij V_ij (c†_{i↑} c_{j↑} + s c†_{i↓} c_{j↓}),   Ṽ = V ⊕ (-s V^T)
// in the Nambu basis (c_{i↑}; c†_{i↓}), V any complex sparse N x N matrix and
// s = ±1 its spin parity.  With V_nm = (U^H Ṽ U)[n, m]:
//   χ(l)   = (1/N) Σ_nm r_nm(l) |V_nm|²                  (k_rs_pairs' r rules)
//   χ''(ω) = (π/N) Σ_nm (f_n - f_m) |V_nm|² L_η(ω - (E_m - E_n))
// the second over every ordered pair with |f_n - f_m| >= 1e-12: the
// reference's σ(ω) loop [src/Observables.jl:415-423] without its 1/ω.
//
// From the eigenpairs E, U of one state, driven by dwhmc_measure.cpp:
//   k_op_fermi     f_n = logistic(-β E_n)
//   k_op_apply     Ṽ U for a group of operators from the 2N-row CSR (one launch)
//   (V_nm = U^H (Ṽ U): the library's own batched product, U^H shared at stride 0;
//    the Matsubara sums are dwhmc_response.hip's k_rs_pairs / k_rs_sum)
//   k_op_spec      χ''(ω) partials: a thread owns one ω, a block streams the
//                  256-pair tiles (ΔE_nm, c_nm) of a chunk of columns m through
//                  LDS; no (n, m) <-> (m, n) fold (χ''(ω) is not odd in ω for a
//                  non-Hermitian V), ω of either sign, no 1/ω
//   k_op_spec_sum  the chunks added in a fixed order, times η/N (real rows here,
//                  the re / im rows of dwhmc_nambu.hip's pairs interleaved)
// All plain fp64 VALU, every sum in a fixed order (no atomics).  Matrices are
// column-major with leading dimension n2 = 2N, as in dwhmc_transport.hip.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

constexpr int kTB = 256;   // threads per block of every kernel here; pairs per tile of k_op_spec

__global__ void k_op_fermi(const double* __restrict__ E, int n2, double beta, double* __restrict__ f,
                           double* __restrict__ g) {
  const int n = blockIdx.x * kTB + threadIdx.x;
  if (n >= n2) return;
  f[n] = logistic_d(-beta * E[n]);
  g[n] = logistic_d(beta * E[n]);   // 1 - f_n from its own exponential
}

// VU_k = Ṽ_k U for the operators k of a group (blockIdx.z): Ṽ in CSR form with
// n2 rows (rows < N: V, columns < N; rows >= N: -s V^T, columns >= N; one
// pattern for every k, duplicates summed on the host), complex values
// val[k nz + e]; VU_k at VU + k sVU.  Column n of U per blockIdx.y.  A row
// >= N reads its own CSR row, whose columns point into the hole half of the
// column.  The current response's Jq ⊕ Jq and the Nambu vertices come in the
// same form.
__global__ void k_op_apply(const double2* __restrict__ U, double2* __restrict__ VU, int64_t sVU, int n2,
                           const int* __restrict__ rowptr, const int* __restrict__ col,
                           const double2* __restrict__ val, int nz) {
  const int r = blockIdx.x * kTB + threadIdx.x;
  if (r >= n2) return;
  const int n = blockIdx.y, k = blockIdx.z;
  const double2* u = U + (size_t)n * n2;
  const double2* a = val + (size_t)k * nz;
  double2 acc = make_double2(0.0, 0.0);
  for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) {
    const double2 v = a[e], b = u[col[e]];
    acc.x += v.x * b.x - v.y * b.y;
    acc.y += v.x * b.y + v.y * b.x;
  }
  VU[(size_t)k * sVU + (size_t)n * n2 + r] = acc;
}

// χ'' partials.  Block (x, y, z): ω_j for j in the x tile, columns m in
// [y cols, (y+1) cols) of V_nm of operator z.  Element [n, m] lies at
// n + m n2, so a tile is 256 consecutive n of one column m (contiguous reads):
//   ΔE_nm = E_m - E_n,  c_nm = (f_n - f_m) |V_nm|²  (0 where |f_n - f_m| < 1e-12,
//   so n = m drops out)
//   part[(z nchunk + y) nw + j] = Σ_{m in chunk} Σ_n c_nm / ((ω_j - ΔE_nm)² + η²)
// With E ascending f_n - f_m vanishes for whole runs of n on either side of
// the Fermi level; a tile whose c are all zero is skipped.  Tail lanes carry
// c = 0, ΔE = 0: their denominator ω² + η² > 0.
__global__ void __launch_bounds__(kTB)
k_op_spec(const double2* __restrict__ Vnm, int64_t sV, int n2, const double* __restrict__ E,
          const double* __restrict__ f, const double* __restrict__ g, double beta, double eta, double w_start,
          double w_step, int nw, int cols, double* __restrict__ part) {
  __shared__ double sdE[kTB], sc[kTB];
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kTB + tid;
  const double w = grid_point(w_start, w_step, j < nw ? j : nw - 1);
  const double eta2 = eta * eta;
  const int m0 = blockIdx.y * cols, m1 = min(m0 + cols, n2);
  const double2* V = Vnm + (size_t)blockIdx.z * sV;
  double acc0 = 0, acc1 = 0;
  for (int m = m0; m < m1; ++m) {
    const double Em = E[m], fm = f[m], gm = g[m];
    const double2* colm = V + (size_t)m * n2;
    for (int n0 = 0; n0 < n2; n0 += kTB) {
      const int n = n0 + tid;
      double c = 0.0, dE = 0.0;
      if (n < n2) {
        // (fermi_diff, dwhmc_device.h: f_n - f_m without the cancellation of two
        // levels on one side of the Fermi level)
        const double d = Em - E[n];
        const double df = fermi_diff(d, f[n], g[n], fm, gm, beta);
        if (fabs(df) >= 1e-12) {
          const double2 v = colm[n];
          dE = d;
          c = df * (v.x * v.x + v.y * v.y);
        }
      }
      if (!__syncthreads_or(c != 0.0)) continue;
      sc[tid] = c;
      sdE[tid] = dE;
      __syncthreads();
#pragma unroll 4
      for (int q = 0; q < kTB; q += 2) {
        const double a0 = w - sdE[q], a1 = w - sdE[q + 1];
        acc0 = fma(sc[q], rcp_nr1(fma(a0, a0, eta2)), acc0);
        acc1 = fma(sc[q + 1], rcp_nr1(fma(a1, a1, eta2)), acc1);
      }
      __syncthreads();
    }
  }
  if (j < nw) part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * nw + j] = acc0 + acc1;
}

// Row blockIdx.y of the partials summed over its chunks, times scale = η/N
// (π·(1/π) cancels): 64 ω per block, wave q sums the chunks [q nchunk/4,
// (q+1) nchunk/4), the four in wave order.  Real rows (χ''(ω_j) of operator
// blockIdx.y): out[blockIdx.y nw + j]; COMPLEX_OUT (row 2 p + c = re / im of
// pair p): out[2 (p nw + j) + c]
template <bool COMPLEX_OUT>
__global__ void k_op_spec_sum(const double* __restrict__ part, int nchunk, int nw, double scale,
                              double* __restrict__ out) {
  __shared__ double sh[4][64];
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + l;
  const double* p = part + (size_t)blockIdx.y * nchunk * nw;
  double s = 0;
  if (j < nw) {
    const int c0 = nchunk * q / 4, c1 = nchunk * (q + 1) / 4;
    for (int c = c0; c < c1; ++c) s += p[(size_t)c * nw + j];
  }
  sh[q][l] = s;
  __syncthreads();
  if (q == 0 && j < nw) {
    const size_t o = COMPLEX_OUT ? 2 * ((size_t)(blockIdx.y >> 1) * nw + j) + (blockIdx.y & 1)
                                 : (size_t)blockIdx.y * nw + j;
    out[o] = (((sh[0][l] + sh[1][l]) + sh[2][l]) + sh[3][l]) * scale;
  }
}

}  // namespace

void launch_op_fermi(const double* E, int N, double beta, double* f, double* g, hipStream_t s) {
  hipLaunchKernelGGL(k_op_fermi, dim3(cdiv(2 * N, kTB)), dim3(kTB), 0, s, E, 2 * N, beta, f, g);
}

void launch_op_apply(const double2* U, double2* VU, int64_t sVU, int N, const int* rowptr, const int* col,
                     const double2* val, int nz, int nops, hipStream_t s) {
  if (nops <= 0) return;
  hipLaunchKernelGGL(k_op_apply, dim3(cdiv(2 * N, kTB), 2 * N, nops), dim3(kTB), 0, s, U, VU, sVU, 2 * N, rowptr, col,
                     val, nz);
}

void launch_op_spec(const double2* Vnm, int64_t sV, int N, const double* E, const double* f, const double* g,
                    double beta, double eta, double w_start, double w_step, int nw, int nops, double* part,
                    double* out, hipStream_t s) {
  if (nops <= 0 || nw <= 0) return;
  int cols, used;
  op_spec_split(N, &cols, &used);
  hipLaunchKernelGGL(k_op_spec, dim3(cdiv(nw, kTB), used, nops), dim3(kTB), 0, s, Vnm, sV, 2 * N, E, f, g, beta, eta,
                     w_start, w_step, nw, cols, part);
  launch_op_spec_sum(part, used, nw, nops, eta / N, out, false, s);
}

void launch_op_spec_sum(const double* part, int nchunk, int nw, int nrows, double scale, double* out,
                        bool complex_out, hipStream_t s) {
  const dim3 grid(cdiv(nw, 64), nrows);
  if (complex_out) hipLaunchKernelGGL(k_op_spec_sum<true>, grid, dim3(256), 0, s, part, nchunk, nw, scale, out);
  else hipLaunchKernelGGL(k_op_spec_sum<false>, grid, dim3(256), 0, s, part, nchunk, nw, scale, out);
}

}  // namespace dwh
