// Finite-momentum current response Λ_αα(q, iΩ_l) (dwh_measure_current_response):
// the reference's paramagnetic sum [src/Observables.jl:366-384] taken from
// q = 0, direction x, iΩ = 0 to lattice momenta q = 2π (mx/Lx, my/Ly), both
// directions and the Matsubara frequencies Ω_l = 2π l / β.
//
// From the eigenpairs E, U of one state, driven by dwhmc_measure.cpp:
//   k_rs_colstats  f_n and the diamagnetic weight of direction α per eigenstate
//   (JU_q = (Jq ⊕ Jq) U for a group of momenta: dwhmc_operator.hip's k_op_apply
//    on the 2N-row CSR of Jq ⊕ Jq; J_nm(q) = U^H JU_q: the library's own batched
//    product, U^H shared at stride 0)
//   k_rs_pairs     per column m of J_nm(q): Σ_n r_nm(l) |J_nm|² for a chunk of l
//   k_rs_sum       the columns (and the eigenstates of dia) added in a fixed order
// All plain fp64 VALU; every sum has a fixed order (no atomics), so results
// are the same run to run.  Matrices are column-major with leading dimension
// n2 = 2N, as in dwhmc_transport.hip.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

constexpr int kTB = 256;   // threads per block of every kernel here

// Per eigenstate n (one block per column of U): f_n = logistic(-β E_n),
// g_n = 1 - f_n = logistic(+β E_n) (its own exponential: no cancellation) and
//   dia_n = [E_n > 0] w_n tanh(β E_n / 2),
//   w_n = Σ_i Σ_b t_b 2 Re(v_i conj(v_j) - conj(u_i) u_j),  j = nbr[b][i]
// (src/Observables.jl:345-362 with the bond list of the direction: nbr 3 x N,
// hopping tb[b]); k_tr_colstats' dia for the x list.
__global__ void k_rs_colstats(const double2* __restrict__ U, int n2, int N, const double* __restrict__ E, double beta,
                              double t0, double t1, double t2, const int* __restrict__ nbr, double* __restrict__ f,
                              double* __restrict__ g, double* __restrict__ dia) {
  __shared__ double sh[1][kTB];
  const int n = blockIdx.x;
  const double2* u = U + (size_t)n * n2;
  const double2* v = u + N;
  double acc[1] = {0};
  for (int i = threadIdx.x; i < N; i += kTB) {
    const double2 ui = u[i], vi = v[i];
    double w = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int j = nbr[b * N + i];
      const double2 uj = u[j], vj = v[j];
      const double bond = 2.0 * ((vi.x * vj.x + vi.y * vj.y) - (ui.x * uj.x + ui.y * uj.y));
      w += (b == 0 ? t0 : b == 1 ? t1 : t2) * bond;
    }
    acc[0] += w;
  }
  block_sum<1>(acc, sh);
  if (threadIdx.x == 0) {
    const double e = E[n];
    f[n] = logistic_d(-beta * e);
    g[n] = logistic_d(beta * e);
    dia[n] = e > 0 ? sh[0][0] * tanh(0.5 * beta * e) : 0.0;
  }
}

// Per column m of J_nm(q) (threads over n; blockIdx.y = q of the group): for
// the NL Matsubara indices l0 .. l0 + NL - 1 (those >= nl skipped on store)
//   part[(q nl + l) n2 + m] = Σ_n r_nm(l) |J_nm|²
//   l = 0:  r = (f_n - f_m)/(E_m - E_n), β f_n (1 - f_n) where |E_m - E_n| < 1e-8
//           (the reference's rule, src/Observables.jl:370-381)
//   l >= 1: r = (f_n - f_m)(E_m - E_n) / ((E_m - E_n)² + Ω_l²), Ω_l = 2π l / β
// with 1 - f_n = g_n and f_n - f_m = fermi_diff (dwhmc_device.h): neither cancels
template <int NL>
__global__ void __launch_bounds__(kTB)
k_rs_pairs(const double2* __restrict__ Jnm, int64_t sJ, int n2, const double* __restrict__ E,
           const double* __restrict__ f, const double* __restrict__ g, double beta, int l0, int nl,
           double* __restrict__ part) {
  __shared__ double sh[NL][kTB];
  const int m = blockIdx.x, q = blockIdx.y;
  const double2* colm = Jnm + (size_t)q * sJ + (size_t)m * n2;
  const double Em = E[m], fm = f[m], gm = g[m];
  double om2[NL], acc[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const double om = kTwoPi * (double)(l0 + k) / beta;
    om2[k] = om * om;
    acc[k] = 0.0;
  }
  for (int n = threadIdx.x; n < n2; n += kTB) {
    const double2 j = colm[n];
    const double J2 = j.x * j.x + j.y * j.y;
    const double dE = Em - E[n], fn = f[n], gn = g[n], df = fermi_diff(dE, fn, gn, fm, gm, beta);
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      if (l0 + k >= nl) break;   // (uniform: the last chunk's unused accumulators)
      double r;
      if (l0 + k == 0) r = fabs(dE) < 1e-8 ? beta * fn * gn : df / dE;
      else r = df * dE / (dE * dE + om2[k]);
      acc[k] += r * J2;
    }
  }
  block_sum<NL>(acc, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NL; ++k)
      if (l0 + k < nl) part[((size_t)q * nl + l0 + k) * n2 + m] = sh[k][0];
  }
}

// out[b] = scale Σ_{k<cnt} in[b cnt + k], one block per b, fixed order
__global__ void k_rs_sum(const double* __restrict__ in, int cnt, double scale, double* __restrict__ out) {
  __shared__ double sh[1][kTB];
  const double* p = in + (size_t)blockIdx.x * cnt;
  double acc[1] = {0};
  for (int k = threadIdx.x; k < cnt; k += kTB) acc[0] += p[k];
  block_sum<1>(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = scale * sh[0][0];
}

}  // namespace

void launch_rs_colstats(const double2* U, int N, const double* E, double beta, const double* tb, const int* nbr,
                        double* f, double* g, double* dia, hipStream_t s) {
  hipLaunchKernelGGL(k_rs_colstats, dim3(2 * N), dim3(kTB), 0, s, U, 2 * N, N, E, beta, tb[0], tb[1], tb[2], nbr, f,
                     g, dia);
}

void launch_rs_pairs(const double2* Jnm, int64_t sJ, int N, const double* E, const double* f, const double* g,
                     double beta, int nl, int nq, double* part, hipStream_t s) {
  if (nq <= 0) return;
  const int n2 = 2 * N;
  for (int l0 = 0; l0 < nl; l0 += kRsLChunk) {
    const dim3 grid(n2, nq);
    if (nl - l0 == 1)   // (the Ω = 0 call: one accumulator)
      hipLaunchKernelGGL(k_rs_pairs<1>, grid, dim3(kTB), 0, s, Jnm, sJ, n2, E, f, g, beta, l0, nl, part);
    else
      hipLaunchKernelGGL(k_rs_pairs<kRsLChunk>, grid, dim3(kTB), 0, s, Jnm, sJ, n2, E, f, g, beta, l0, nl, part);
  }
}

void launch_rs_sum(const double* in, int cnt, int nout, double scale, double* out, hipStream_t s) {
  if (nout <= 0) return;
  hipLaunchKernelGGL(k_rs_sum, dim3(nout), dim3(kTB), 0, s, in, cnt, scale, out);
}

}  // namespace dwh
