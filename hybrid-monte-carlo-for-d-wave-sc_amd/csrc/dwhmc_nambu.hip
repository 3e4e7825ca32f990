// Cross response of general Nambu vertices (dwh_measure_nambu_response): any
// 2N x 2N complex W_k is the operator O_k = Ψ† W_k Ψ in the basis
// Ψ = (c_{i↑}; c†_{i↓}), pairing (off-diagonal) blocks included.  With
// X^k = U^H W_k U and, for a pair p = (a, b), M_nm = X^a_nm conj(X^b_nm):
//   chi[p, l]  = (1/N) Σ_nm [r_nm(l) + i s_nm(l)] M_nm      (k_rs_pairs' r rules,
//                s_nm(0) = 0, s_nm(l >= 1) = (f_n - f_m) Ω_l / (ΔE² + Ω_l²))
//   chi2[p, j] = (π/N) Σ_nm (f_n - f_m) M_nm L_η(ω_j - ΔE_nm),  |f_n - f_m| >= 1e-12
// both complex.  From the eigenpairs E, U of one state, driven by
// dwhmc_measure.cpp: f_n (launch_op_fermi), W_k U (launch_op_apply), X^k (the
// library's batched product, resident for every vertex of the call), then
//   k_nb_pairs     per column m and pair: Σ_n (r + i s) M for a chunk of l, two
//                  accumulators per l, k_rs_pairs' grid and tree
//   (launch_rs_sum adds the columns: re and im are neighbouring rows)
//   k_nb_spec<P>   chi2 partials of a group of P pairs: a thread owns two ω, a
//                  block streams 256-row tiles (ΔE once, P complex weights) of a
//                  column chunk through LDS; one reciprocal per (n, m, ω) serves
//                  the 2P accumulators
//   (launch_op_spec_sum adds the chunks in a fixed order, times η/N)
// All plain fp64 VALU, every sum in a fixed order (no atomics).  Matrices are
// column-major with leading dimension n2 = 2N.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

constexpr int kTB = 256;   // threads per block of every kernel here; rows per tile of k_nb_spec
constexpr int kNbW = 2;   // frequencies per thread of k_nb_spec

// M = a conj(b)
__device__ inline double2 mul_conj(double2 a, double2 b) {
  return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// Per column m (blockIdx.x) and pair p = (pr[2p], pr[2p+1]) (blockIdx.y), for
// the NL Matsubara indices l0 .. l0 + NL - 1 (those >= nl skipped on store):
//   part[((p nl + l) 2 + c) n2 + m] = Σ_n Re / Im (c = 0 / 1) of (r_nm + i s_nm) M_nm
// with k_rs_pairs' r (l = 0: (f_n - f_m)/ΔE, β f_n g_n where |ΔE| < 1e-8) and
// s_nm(0) = 0, s_nm(l) = (f_n - f_m) Ω_l / (ΔE² + Ω_l²)
template <int NL>
__global__ void __launch_bounds__(kTB)
k_nb_pairs(const double2* __restrict__ X, int64_t sX, int n2, const int* __restrict__ pr,
           const double* __restrict__ E, const double* __restrict__ f, const double* __restrict__ g, double beta,
           int l0, int nl, double* __restrict__ part) {
  __shared__ double sh[2 * NL][kTB];
  const int m = blockIdx.x, p = blockIdx.y;
  const double2* ca = X + (size_t)pr[2 * p] * sX + (size_t)m * n2;
  const double2* cb = X + (size_t)pr[2 * p + 1] * sX + (size_t)m * n2;
  const double Em = E[m], fm = f[m], gm = g[m];
  double om[NL], acc[2 * NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    om[k] = kTwoPi * (double)(l0 + k) / beta;
    acc[2 * k] = acc[2 * k + 1] = 0.0;
  }
  for (int n = threadIdx.x; n < n2; n += kTB) {
    const double2 M = mul_conj(ca[n], cb[n]);
    const double dE = Em - E[n], fn = f[n], gn = g[n], df = fermi_diff(dE, fn, gn, fm, gm, beta);
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      if (l0 + k >= nl) break;   // (uniform: the last chunk's unused accumulators)
      double r, s;
      if (l0 + k == 0) {
        r = fabs(dE) < 1e-8 ? beta * fn * gn : df / dE;
        s = 0.0;
      } else {
        const double d = df / (dE * dE + om[k] * om[k]);
        r = d * dE;
        s = d * om[k];
      }
      acc[2 * k] += r * M.x - s * M.y;
      acc[2 * k + 1] += r * M.y + s * M.x;
    }
  }
  block_sum<2 * NL>(acc, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NL; ++k)
      if (l0 + k < nl) {
        part[(((size_t)p * nl + l0 + k) * 2) * n2 + m] = sh[2 * k][0];
        part[(((size_t)p * nl + l0 + k) * 2 + 1) * n2 + m] = sh[2 * k + 1][0];
      }
  }
}

// chi2 partials of the P pairs p0 + z P + k, k < P, of block (x, y, z): a
// thread owns the kNbW frequencies ω_j, j = x kNbW 256 + t 256 + tid, t < kNbW,
// so one broadcast LDS read of a weight serves kNbW evaluations; columns m in
// [y cols, (y+1) cols).  A tile is 256 consecutive n of one column m:
//   ΔE_nm = E_m - E_n,  c^k_nm = (f_n - f_m) X^a_nm conj(X^b_nm)   (0 where
//   |f_n - f_m| < 1e-12, so n = m drops out)
//   part[(((z P + k) 2 + c) nchunk + y) nw + j] = Σ_{m in chunk} Σ_n Re / Im c^k_nm / ((ω_j - ΔE_nm)² + η²)
// A tile is skipped only when every weight of every pair of the group is zero.
// Tail lanes carry c = 0, ΔE = 0: their denominator ω² + η² > 0; a frequency
// slot past the grid evaluates its last point and is not stored.
template <int P>
__global__ void __launch_bounds__(kTB)
k_nb_spec(const double2* __restrict__ X, int64_t sX, int n2, const int* __restrict__ pr, int p0,
          const double* __restrict__ E, const double* __restrict__ f, const double* __restrict__ g, double beta,
          double eta, double w_start, double w_step, int nw, int cols, double* __restrict__ part) {
  __shared__ double sdE[kTB];
  __shared__ double2 sc[kTB][P];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * (kNbW * kTB) + tid;
  double w[kNbW];
#pragma unroll
  for (int t = 0; t < kNbW; ++t) w[t] = grid_point(w_start, w_step, min(j0 + t * kTB, nw - 1));
  const double eta2 = eta * eta;
  const int m0 = blockIdx.y * cols, m1 = min(m0 + cols, n2);
  const int pg = blockIdx.z * P;   // first pair of the group, relative to p0
  const double2 *Xa[P], *Xb[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    Xa[k] = X + (size_t)pr[2 * (p0 + pg + k)] * sX;
    Xb[k] = X + (size_t)pr[2 * (p0 + pg + k) + 1] * sX;
  }
  double ar[kNbW][P], ai[kNbW][P];
#pragma unroll
  for (int t = 0; t < kNbW; ++t)
#pragma unroll
    for (int k = 0; k < P; ++k) ar[t][k] = ai[t][k] = 0.0;
  for (int m = m0; m < m1; ++m) {
    const double Em = E[m], fm = f[m], gm = g[m];
    const size_t cm = (size_t)m * n2;
    for (int n0 = 0; n0 < n2; n0 += kTB) {
      const int n = n0 + tid;
      double2 c[P];
#pragma unroll
      for (int k = 0; k < P; ++k) c[k] = make_double2(0.0, 0.0);
      double dE = 0.0;
      bool nz = false;
      if (n < n2) {
        const double d = Em - E[n];
        const double df = fermi_diff(d, f[n], g[n], fm, gm, beta);
        if (fabs(df) >= 1e-12) {
          dE = d;
#pragma unroll
          for (int k = 0; k < P; ++k) {
            const double2 M = mul_conj(Xa[k][cm + n], Xb[k][cm + n]);
            c[k] = make_double2(df * M.x, df * M.y);
            nz = nz || c[k].x != 0.0 || c[k].y != 0.0;
          }
        }
      }
      if (!__syncthreads_or(nz)) continue;
      sdE[tid] = dE;
#pragma unroll
      for (int k = 0; k < P; ++k) sc[tid][k] = c[k];
      __syncthreads();
#pragma unroll 4
      for (int q = 0; q < kTB; ++q) {
        const double d = sdE[q];
        double r[kNbW];
#pragma unroll
        for (int t = 0; t < kNbW; ++t) {
          const double a = w[t] - d;
          r[t] = rcp_nr1(fma(a, a, eta2));
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
          const double2 ck = sc[q][k];
#pragma unroll
          for (int t = 0; t < kNbW; ++t) {
            ar[t][k] = fma(ck.x, r[t], ar[t][k]);
            ai[t][k] = fma(ck.y, r[t], ai[t][k]);
          }
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int t = 0; t < kNbW; ++t) {
    const int j = j0 + t * kTB;
    if (j < nw) {
#pragma unroll
      for (int k = 0; k < P; ++k) {
        const size_t row = ((size_t)(pg + k) * 2) * gridDim.y + blockIdx.y;
        part[row * nw + j] = ar[t][k];
        part[(row + gridDim.y) * nw + j] = ai[t][k];
      }
    }
  }
}

template <int P>
void spec_group(dim3 grid, hipStream_t s, const double2* X, int64_t sX, int n2, const int* pr, int p0,
                const double* E, const double* f, const double* g, double beta, double eta, double w_start,
                double w_step, int nw, int cols, double* part) {
  hipLaunchKernelGGL(k_nb_spec<P>, grid, dim3(kTB), 0, s, X, sX, n2, pr, p0, E, f, g, beta, eta, w_start, w_step, nw,
                     cols, part);
}

}  // namespace

void launch_nb_pairs(const double2* X, int64_t sX, int N, const int* pairs, int npairs, const double* E,
                     const double* f, const double* g, double beta, int nl, double* part, hipStream_t s) {
  if (npairs <= 0) return;
  const int n2 = 2 * N;
  const dim3 grid(n2, npairs);
  for (int l0 = 0; l0 < nl; l0 += kRsLChunk) {
    if (nl - l0 == 1)   // (the Ω = 0 call: one accumulator pair)
      hipLaunchKernelGGL(k_nb_pairs<1>, grid, dim3(kTB), 0, s, X, sX, n2, pairs, E, f, g, beta, l0, nl, part);
    else
      hipLaunchKernelGGL(k_nb_pairs<kRsLChunk>, grid, dim3(kTB), 0, s, X, sX, n2, pairs, E, f, g, beta, l0, nl, part);
  }
}

void launch_nb_spec(const double2* X, int64_t sX, int N, const int* pairs, int p0, int npairs, const double* E,
                    const double* f, const double* g, double beta, double eta, double w_start, double w_step, int nw,
                    double* part, double* out, hipStream_t s) {
  if (npairs <= 0 || nw <= 0) return;
  const int n2 = 2 * N;
  int cols, used;
  op_spec_split(N, &cols, &used);
  const int full = npairs / kNbSpecGroup, rem = npairs % kNbSpecGroup;
  const int nx = cdiv(nw, kNbW * kTB);
  // the groups of kNbSpecGroup pairs, then the last, partial one on the
  // instantiation of its own size: no unused slot exists
  if (full > 0)
    spec_group<kNbSpecGroup>(dim3(nx, used, full), s, X, sX, n2, pairs, p0, E, f, g, beta, eta, w_start, w_step, nw,
                             cols, part);
  double* tail = part + (size_t)full * kNbSpecGroup * 2 * used * nw;
  const int pt = p0 + full * kNbSpecGroup;
  const dim3 gt(nx, used, 1);
  if (rem == 1) spec_group<1>(gt, s, X, sX, n2, pairs, pt, E, f, g, beta, eta, w_start, w_step, nw, cols, tail);
  if (rem == 2) spec_group<2>(gt, s, X, sX, n2, pairs, pt, E, f, g, beta, eta, w_start, w_step, nw, cols, tail);
  if (rem == 3) spec_group<3>(gt, s, X, sX, n2, pairs, pt, E, f, g, beta, eta, w_start, w_step, nw, cols, tail);
  static_assert(kNbSpecGroup == 4, "the tail dispatch covers group sizes 1 .. 3");
  // out[2 (j + nw p) + c] from the rows p 2 + c of the partials
  launch_op_spec_sum(part, used, nw, 2 * npairs, eta / N, out + 2 * (size_t)p0 * nw, true, s);
}

}  // namespace dwh
