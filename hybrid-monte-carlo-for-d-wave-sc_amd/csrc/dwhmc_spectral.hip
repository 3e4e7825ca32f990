// Site- and momentum-resolved spectral maps from the eigenpairs of one
// H_BdG(Δ) (the resolved spectra src/Observables.jl:305-307 leaves out):
//   LDOS(i, ω_q) = Σ_n |u_n(i)|² L(ω_q - E_n)
//   A(k, ω_q)    = (1/N) Σ_n |û_n(k)|² L(ω_q - E_n)
// with u_n the particle rows of column n of U, û_n its unnormalised forward
// 2-D DFT as an Lx x Ly image (site i = x + Lx y, e^{-2πi(kx x/Lx + ky y/Ly)},
// the conventions of the A(k, 0) path in dwhmc_transport.hip), L the
// Lorentzian (1/π) η/(x² + η²) and ω_q points of the DOS grid.
//
// Both maps are one real product out = scale · W Λ with W[r, n] = |X[r, n]|²
// (X: the particle rows of U, or the DFT'd columns) against one Lorentzian
// table Λ[n, q] of a chunk of the frequency window (k_sp_lorentz; q
// contiguous).  Two routes (dwhmc_measure.cpp, DWHMC_SPECTRAL_FUSED):
//   * unfused (default): k_sp_sqmod writes W, the library's gemm_d takes the
//     product;
//   * fused (=1, k_sp_maps): the squared modulus is formed as the complex X
//     is staged, so no |X|² matrix is written.  Measured slower at L = 32
//     (1.54 against 1.23 ms for both maps on the full grid: the complex
//     operand doubles the staging traffic and its fp64 squares share the
//     MFMA's pipe, once per column tile), so it stays behind the switch.
// Either sums over n in a fixed order (no atomics, no split K): two calls give
// the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

constexpr int kTB = 256;
constexpr double kInvPi = 0.31830988618379067154;
constexpr int kMaxDft = 1024;   // longest lattice side with its twiddles in LDS (as k_tr_dft_x)

// Λ[n, q] = L(ω_q - E_n) at Lam[q + ldq n] for q < cnt, n < n2; ω_q = point
// first + q stride of the grid d0 + k dw; state s = blockIdx.z
__global__ void __launch_bounds__(kTB)
k_sp_lorentz(const double* __restrict__ E, int n2, double eta, double d0, double dw, int64_t first,
             int64_t stride, int cnt, double* __restrict__ Lam, int ldq, int64_t sLam) {
  const int q = blockIdx.x * kTB + threadIdx.x;
  if (q >= cnt) return;
  const int s = blockIdx.z;
  E += (int64_t)s * n2;
  Lam += (int64_t)s * sLam;
  const double w = grid_point(d0, dw, first + (int64_t)q * stride), eta2 = eta * eta;
  const int n0 = blockIdx.y * 64, n1 = min(n0 + 64, n2);
  for (int n = n0; n < n1; ++n) {
    const double d = w - E[n];
    Lam[q + (int64_t)n * ldq] = kInvPi * (eta / (d * d + eta2));
  }
}

// DFT pass x of every column's particle rows (unit weight):
// T[kx + Lx y, n] = Σ_x U[x + Lx y, n] e^{-2πi kx x / Lx}; U ld n2, T ld N
__global__ void __launch_bounds__(kTB)
k_sp_dft_x(const double2* __restrict__ U, int n2, int64_t sU, int Lx, int Ly, double2* __restrict__ T,
           int64_t sT) {
  __shared__ double2 tw[kMaxDft];
  const bool tab = Lx <= kMaxDft;
  if (tab)
    for (int q = threadIdx.x; q < Lx; q += kTB) sincospi(-2.0 * (double)q / Lx, &tw[q].y, &tw[q].x);
  __syncthreads();
  const int N = Lx * Ly;
  const int idx = blockIdx.x * kTB + threadIdx.x;
  if (idx >= N) return;
  const int n = blockIdx.y, s = blockIdx.z, kx = idx % Lx, y = idx / Lx;
  const double2* u = U + (int64_t)s * sU + (int64_t)n * n2 + (int64_t)y * Lx;
  double2 acc = make_double2(0.0, 0.0);
  for (int x = 0; x < Lx; ++x) {
    double2 t;
    if (tab) t = tw[(kx * x) % Lx];
    else sincospi(-2.0 * (double)((kx * x) % Lx) / Lx, &t.y, &t.x);
    const double2 a = u[x];
    acc.x += a.x * t.x - a.y * t.y;
    acc.y += a.x * t.y + a.y * t.x;
  }
  T[(int64_t)s * sT + (int64_t)n * N + idx] = acc;
}

// pass y: X[kx + Lx ky, n] = Σ_y T[kx + Lx y, n] e^{-2πi ky y / Ly}; both ld N
__global__ void __launch_bounds__(kTB)
k_sp_dft_y(const double2* __restrict__ T, int64_t sT, int Lx, int Ly, double2* __restrict__ X, int64_t sX) {
  __shared__ double2 tw[kMaxDft];
  const bool tab = Ly <= kMaxDft;
  if (tab)
    for (int q = threadIdx.x; q < Ly; q += kTB) sincospi(-2.0 * (double)q / Ly, &tw[q].y, &tw[q].x);
  __syncthreads();
  const int N = Lx * Ly;
  const int idx = blockIdx.x * kTB + threadIdx.x;
  if (idx >= N) return;
  const int n = blockIdx.y, s = blockIdx.z, kx = idx % Lx, ky = idx / Lx;
  const double2* tcol = T + (int64_t)s * sT + (int64_t)n * N + kx;
  double2 acc = make_double2(0.0, 0.0);
  for (int y = 0; y < Ly; ++y) {
    double2 t;
    if (tab) t = tw[(ky * y) % Ly];
    else sincospi(-2.0 * (double)((ky * y) % Ly) / Ly, &t.y, &t.x);
    const double2 a = tcol[(int64_t)y * Lx];
    acc.x += a.x * t.x - a.y * t.y;
    acc.y += a.x * t.y + a.y * t.x;
  }
  X[(int64_t)s * sX + (int64_t)n * N + idx] = acc;
}

// unfused route: W[r + M n] = |X[r + ldx n]|², r < M, n < K
__global__ void __launch_bounds__(kTB)
k_sp_sqmod(const double2* __restrict__ X, int ldx, int64_t sX, int M, double* __restrict__ W, int64_t sW) {
  const int r = blockIdx.x * kTB + threadIdx.x;
  if (r >= M) return;
  const int n = blockIdx.y, s = blockIdx.z;
  const double2 x = X[(int64_t)s * sX + (int64_t)n * ldx + r];
  W[(int64_t)s * sW + (int64_t)n * M + r] = x.x * x.x + x.y * x.y;
}

// out[r + ldo q] = scale Σ_{n<K} |X[r + ldx n]|² Lam[q + ldq n], r < M, q < Q.
// One 256-thread workgroup per 64 x 64 output tile (blockIdx.x: row tile,
// .y: column tile, .z: state), four waves of 32 x 32 (2 x 2 tiles of
// v_mfma_f64_16x16x4_f64); K in chunks of 16 staged through LDS k-major, as
// k_gemm does (dwhmc_gemm.hip): a wave's staging load of X is 64 consecutive
// rows of one column (1 KB coalesced), squared as it is stored; its load of Λ
// 64 consecutive q of one n.  The A fragment of a k-step is As[k][16
// consecutive rows], the B fragment Bs[k][16 consecutive q].  Rows >= M,
// columns >= Q and k >= K are staged as zeros and never stored.
// (64 x 128 tiles, two B loads per squared element, were slower at L = 32:
// profiles/spectral_maps_L32.txt.)
constexpr int SM = 64, SK = 16, SP = 1;
constexpr int kImg = SK * (SM + SP);   // one K-chunk image

struct SpStage {
  double a[4], b[4];
  __device__ __forceinline__ void load(const double2* X, int ldx, const double* Lam, int ldq, int m0, int q0, int k0,
                                       int M, int Q, int K) {
    const int t = threadIdx.x, c = t & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + (t >> 6) + 4 * j;
      const bool kin = k < K;
      double2 x = make_double2(0.0, 0.0);
      if (kin && m0 + c < M) x = X[(m0 + c) + (int64_t)k * ldx];
      a[j] = x.x * x.x + x.y * x.y;
      b[j] = (kin && q0 + c < Q) ? Lam[(q0 + c) + (int64_t)k * ldq] : 0.0;
    }
  }
  __device__ __forceinline__ void store(double* As, double* Bs) const {
    const int t = threadIdx.x, c = t & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      As[((t >> 6) + 4 * j) * (SM + SP) + c] = a[j];
      Bs[((t >> 6) + 4 * j) * (SM + SP) + c] = b[j];
    }
  }
};

__global__ void __launch_bounds__(256)
k_sp_maps(const double2* __restrict__ X, int ldx, int64_t sX, const double* __restrict__ Lam, int ldq, int64_t sLam,
          int M, int Q, int K, double scale, double* __restrict__ out, int ldo, int64_t sOut) {
  __shared__ double smem[4 * kImg];   // As[2], Bs[2]; the epilogue tile 64 x (64 + SP) reuses it
  static_assert(4 * kImg >= SM * (SM + SP), "epilogue tile fits the LDS images");
  const int m0 = blockIdx.x * SM, q0 = blockIdx.y * SM, s = blockIdx.z;
  X += (int64_t)s * sX;
  Lam += (int64_t)s * sLam;
  out += (int64_t)s * sOut;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
  d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  SpStage st;
  const int nk = (K + SK - 1) / SK;
  if (nk > 0) {
    st.load(X, ldx, Lam, ldq, m0, q0, 0, M, Q, K);
    st.store(smem, smem + 2 * kImg);
  }
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int cur = kc & 1;
    if (kc + 1 < nk) st.load(X, ldx, Lam, ldq, m0, q0, (kc + 1) * SK, M, Q, K);
    const double* as = smem + cur * kImg;
    const double* bs = smem + (2 + cur) * kImg;
#pragma unroll
    for (int ks = 0; ks < SK / 4; ++ks) {
      const int k = 4 * ks + lk;
      double av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = as[k * (SM + SP) + wm + 16 * i + lr];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = bs[k * (SM + SP) + wn + 16 * j + lr];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (kc + 1 < nk) st.store(smem + (cur ^ 1) * kImg, smem + (2 + (cur ^ 1)) * kImg);
    __syncthreads();
  }
  // epilogue: the tile column-major in LDS, then whole column segments per thread
  double* Cs = smem;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        Cs[(wn + 16 * j + lr) * (SM + SP) + wm + 16 * i + lk + 4 * rr] = acc[i][j][rr];
  __syncthreads();
  const int row = threadIdx.x & 63, gr = m0 + row;
  if (gr >= M) return;
#pragma unroll 4
  for (int c = threadIdx.x >> 6; c < SM; c += 4) {
    const int gc = q0 + c;
    if (gc >= Q) break;
    out[gr + (int64_t)gc * ldo] = scale * Cs[c * (SM + SP) + row];
  }
}

}  // namespace

void launch_sp_lorentz(const double* E, int n2, double eta, double d0, double dw, int64_t first, int64_t stride,
                       int cnt, double* Lam, int ldq, int64_t sLam, int m, hipStream_t s) {
  if (cnt <= 0 || n2 <= 0 || m <= 0) return;
  hipLaunchKernelGGL(k_sp_lorentz, dim3(cdiv(cnt, kTB), cdiv(n2, 64), m), dim3(kTB), 0, s, E, n2, eta, d0, dw, first,
                     stride, cnt, Lam, ldq, sLam);
}

void launch_sp_dft(const double2* U, int64_t sU, int Lx, int Ly, double2* T, int64_t sT, double2* X, int64_t sX,
                   int m, hipStream_t s) {
  const int N = Lx * Ly, n2 = 2 * N;
  const dim3 grid(cdiv(N, kTB), n2, m);
  hipLaunchKernelGGL(k_sp_dft_x, grid, dim3(kTB), 0, s, U, n2, sU, Lx, Ly, T, sT);
  hipLaunchKernelGGL(k_sp_dft_y, grid, dim3(kTB), 0, s, T, sT, Lx, Ly, X, sX);
}

void launch_sp_sqmod(const double2* X, int ldx, int64_t sX, int M, int K, double* W, int64_t sW, int m,
                     hipStream_t s) {
  if (M <= 0 || K <= 0 || m <= 0) return;
  hipLaunchKernelGGL(k_sp_sqmod, dim3(cdiv(M, kTB), K, m), dim3(kTB), 0, s, X, ldx, sX, M, W, sW);
}

void launch_sp_maps(const double2* X, int ldx, int64_t sX, const double* Lam, int ldq, int64_t sLam, int M, int Q,
                    int K, double scale, double* out, int ldo, int64_t sOut, int m, hipStream_t s) {
  if (M <= 0 || Q <= 0 || m <= 0) return;
  hipLaunchKernelGGL(k_sp_maps, dim3(cdiv(M, SM), cdiv(Q, SM), m), dim3(256), 0, s, X, ldx, sX, Lam, ldq, sLam, M, Q,
                     K, scale, out, ldo, sOut);
}

}  // namespace dwh
