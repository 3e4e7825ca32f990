// Response maps (dwh_measure_response_map): the linear-response density matrix
//   D(z)[W] = U (w(z) ∘ U^H W U) U^H
// of a source vertex W at a frequency z, and the equal-time ρ = U f U^H, both
// only at the entries (a_e, b_e) of a sparse pattern of Nambu index pairs.
// From the eigenpairs E, U of one state, driven by dwhmc_measure.cpp after
// X = U^H W U (vertex_run):
//   k_map_weight   K_z = w(z) ∘ X for a chunk of frequencies, X read once;
//                  Matsubara weights as k_nb_pairs forms them, retarded
//                  (f_n - f_m)/(ΔE_nm - ω - iη) with χ'''s |f_n - f_m| rule
//   (S_z = K_z U^H: the library's batched product, U^H shared at stride 0)
//   k_map_fscale   S = diag(f) U^H, the ρ analogue of S_z (no product)
//   k_map_sddmm    D_e = Σ_n conj(U^H[n, a_e]) S[n, b_e] over the pattern grouped
//                  by b: a workgroup stages column b of S in LDS once and its
//                  waves stream the columns a_e of U^H against it
// With S = K U^H (not U K) both operands of the sampled product are contiguous
// columns.  All plain fp64 VALU, every sum in a fixed order (no atomics).
// Matrices are column-major with leading dimension n2 = 2N.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

constexpr int kTB = 256;               // threads per block of every kernel here
constexpr int kWaves = kTB / 64;

// K[c][n, m] = w_nm(z0 + c) X[n, m], c < cnt, for row n = blockIdx.x kTB + tid of
// column m = blockIdx.y.  z < nl is the Matsubara index l = z: r + i s of
// k_nb_pairs (l = 0: (f_n - f_m)/ΔE, β f_n g_n where |ΔE| < 1e-8, s = 0;
// l >= 1: (f_n - f_m)(ΔE + iΩ_l)/(ΔE² + Ω_l²)); z >= nl the real frequency
// ω = omega[z - nl]: (f_n - f_m)(a + iη)/(a² + η²), a = ΔE - ω, and 0 where
// |f_n - f_m| < 1e-12.  ΔE = E_m - E_n.
__global__ void __launch_bounds__(kTB)
k_map_weight(const double2* __restrict__ X, int n2, const double* __restrict__ E, const double* __restrict__ f,
             const double* __restrict__ g, double beta, int z0, int cnt, int nl, const double* __restrict__ omega,
             double eta, double2* __restrict__ K, int64_t sK) {
  const int m = blockIdx.y, n = blockIdx.x * kTB + threadIdx.x;
  if (n >= n2) return;
  const size_t o = (size_t)m * n2 + n;
  const double2 x = X[o];
  const double fn = f[n], gn = g[n];
  const double dE = E[m] - E[n], df = fermi_diff(dE, fn, gn, f[m], g[m], beta);
  const bool keep = fabs(df) >= 1e-12;
  for (int c = 0; c < cnt; ++c) {
    const int z = z0 + c;
    double r, s;
    if (z == 0 && nl > 0) {
      r = fabs(dE) < 1e-8 ? beta * fn * gn : df / dE;
      s = 0.0;
    } else if (z < nl) {
      const double om = kTwoPi * (double)z / beta;
      const double d = df / (dE * dE + om * om);
      r = d * dE;
      s = d * om;
    } else {
      const double a = dE - omega[z - nl];
      const double d = keep ? df / (a * a + eta * eta) : 0.0;
      r = d * a;
      s = d * eta;
    }
    K[(size_t)c * sK + o] = make_double2(r * x.x - s * x.y, r * x.y + s * x.x);
  }
}

// S[n, b] = f_n UH[n, b]
__global__ void __launch_bounds__(kTB)
k_map_fscale(const double2* __restrict__ UH, int n2, const double* __restrict__ f, double2* __restrict__ S) {
  const int n = blockIdx.x * kTB + threadIdx.x;
  if (n >= n2) return;
  const size_t o = (size_t)blockIdx.y * n2 + n;
  const double fn = f[n];
  const double2 u = UH[o];
  S[o] = make_double2(fn * u.x, fn * u.y);
}

// Block (x, y): slice x = (b, i0, cnt) of the column-grouped pattern on the
// matrix S + y sS.  Column b of S goes to LDS (n2 complex); wave w takes the
// entries i0 + w, i0 + w + kWaves, ... < i0 + cnt: lane j adds its rows
// n = j, j + 64, ... of conj(UH[n, arow[i]]) S[n, b] in ascending order into
// two accumulators (even / odd trips), the lanes are added by a butterfly, and
// lane 0 stores the entry at its original index dst[i] of out + y sOut.
__global__ void __launch_bounds__(kTB)
k_map_sddmm(const double2* __restrict__ UH, const double2* __restrict__ S, int64_t sS, int n2,
            const int3* __restrict__ slices, const int* __restrict__ arow, const int* __restrict__ dst,
            double2* __restrict__ out, int64_t sOut) {
  extern __shared__ double2 col[];
  const int3 sl = slices[blockIdx.x];
  const double2* Sb = S + (size_t)blockIdx.y * sS + (size_t)sl.x * n2;
  for (int n = threadIdx.x; n < n2; n += kTB) col[n] = Sb[n];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double2* o = out + (size_t)blockIdx.y * sOut;
  for (int i = sl.y + wave; i < sl.y + sl.z; i += kWaves) {
    const double2* ua = UH + (size_t)arow[i] * n2;
    double2 a0 = make_double2(0.0, 0.0), a1 = a0;
    int n = lane;
    for (; n + 64 < n2; n += 128) {
      const double2 u0 = ua[n], u1 = ua[n + 64];
      const double2 s0 = col[n], s1 = col[n + 64];
      a0.x += u0.x * s0.x + u0.y * s0.y;
      a0.y += u0.x * s0.y - u0.y * s0.x;
      a1.x += u1.x * s1.x + u1.y * s1.y;
      a1.y += u1.x * s1.y - u1.y * s1.x;
    }
    if (n < n2) {
      const double2 u0 = ua[n], s0 = col[n];
      a0.x += u0.x * s0.x + u0.y * s0.y;
      a0.y += u0.x * s0.y - u0.y * s0.x;
    }
    const double re = wave_sum(a0.x + a1.x), im = wave_sum(a0.y + a1.y);
    if (lane == 0) o[dst[i]] = make_double2(re, im);
  }
}

}  // namespace

void launch_map_weight(const double2* X, int N, const double* E, const double* f, const double* g, double beta,
                       int z0, int cnt, int nl, const double* omega, double eta, double2* K, int64_t sK,
                       hipStream_t s) {
  if (cnt <= 0) return;
  const int n2 = 2 * N;
  hipLaunchKernelGGL(k_map_weight, dim3(cdiv(n2, kTB), n2), dim3(kTB), 0, s, X, n2, E, f, g, beta, z0, cnt, nl, omega,
                     eta, K, sK);
}

void launch_map_fscale(const double2* UH, int N, const double* f, double2* S, hipStream_t s) {
  const int n2 = 2 * N;
  hipLaunchKernelGGL(k_map_fscale, dim3(cdiv(n2, kTB), n2), dim3(kTB), 0, s, UH, n2, f, S);
}

void launch_map_sddmm(const double2* UH, const double2* S, int64_t sS, int N, const int* slices, int nslices,
                      const int* arow, const int* dst, double2* out, int64_t sOut, int nmat, hipStream_t s) {
  if (nslices <= 0 || nmat <= 0) return;
  const int n2 = 2 * N;
  hipLaunchKernelGGL(k_map_sddmm, dim3(nslices, nmat), dim3(kTB), (size_t)n2 * sizeof(double2), s, UH, S, sS, n2,
                     reinterpret_cast<const int3*>(slices), arow, dst, out, sOut);
}

}  // namespace dwh
