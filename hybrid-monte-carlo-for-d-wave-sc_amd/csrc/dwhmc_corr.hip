// Equal-time correlations of local operators (dwh_measure_correlations): at a
// fixed Δ the fermions are free, so Wick's theorem gives, from the full
// density matrix ρ = U f U^H (ρ[x, y] = <Ψ†_y Ψ_x>, Ψ = (c_↑; c†_↓)),
//   G_AB(i, j) = Σ_{t,u} a_{i,t} conj(b_{j,u}) conj(ρ[r_A, r_B]) (δ[c_A, c_B] - ρ[c_A, c_B])
// for the bilinears O_A(i) = Σ_t a_{i,t} Ψ†_{r(i,t)} Ψ_{c(i,t)} of two local
// families.  Driven by dwhmc_measure.cpp after ρ = U (diag(f) U^H) (the
// library's product):
//   k_corr       for a fixed site j a lane per displacement r takes i = j ⊕ r:
//                both ρ factors carry the A side as the row, so the lanes of a
//                stencil family read neighbouring rows of one column of the
//                column-major ρ.  A workgroup owns kCorrTile displacements and
//                kCorrChunk sites j, added in registers in ascending j, and
//                writes one partial per (chunk, r).  With a site list (the
//                `local` output) a chunk is one listed site and the partial
//                is the result.
//   k_corr_sum   the chunks added in ascending order, times 1/N
//   k_corr_mean  m_k(i) = Σ_t a_{i,t} ρ[c(i,t), r(i,t)], a gather
// The terms of a site are read as uploaded (any indices, any count up to
// kCorrMaxTerms, duplicates kept).  All plain fp64 VALU, every sum in a fixed
// order (no atomics).  ρ is column-major with leading dimension n2 = 2N.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

// Block x = tile + ntiles (c + ny p): displacements r = tile kCorrTile + tid of
// pair p = (fa, fb) and the sites k = c chunk .. min((c + 1) chunk, nj) - 1 of
// the list (jlist[k]; NULL: site k).  part[(p ny + c) N + r] = Σ_k G(j_k ⊕ r, j_k).
__global__ void __launch_bounds__(kCorrTile)
k_corr(const double2* __restrict__ rho, int n2, int N, int Lx, const int* __restrict__ tptr,
       const int* __restrict__ trow, const int* __restrict__ tcol, const double2* __restrict__ tval,
       const int* __restrict__ pairs, const int* __restrict__ jlist, int chunk, int nj, int ntiles, int ny,
       double2* __restrict__ part) {
  const int tile = blockIdx.x % ntiles, cp = blockIdx.x / ntiles, c = cp % ny, p = cp / ny;
  const int r = tile * kCorrTile + threadIdx.x;
  if (r >= N) return;
  const int Ly = N / Lx, rx = r % Lx, ry = r / Lx;
  const int* pa = tptr + (size_t)pairs[2 * p] * N;
  const int* pb = tptr + (size_t)pairs[2 * p + 1] * N;
  double2 acc = make_double2(0.0, 0.0);
  const int k1 = min((c + 1) * chunk, nj);
  for (int k = c * chunk; k < k1; ++k) {
    const int j = jlist ? jlist[k] : k;
    int ix = j % Lx + rx, iy = j / Lx + ry;
    if (ix >= Lx) ix -= Lx;
    if (iy >= Ly) iy -= Ly;
    const int i = iy * Lx + ix;
    const int u0 = pb[j], u1 = pb[j + 1], t1 = pa[i + 1];
    for (int t = pa[i]; t < t1; ++t) {
      const double2 a = tval[t];
      const size_t ra = (size_t)trow[t], ca = (size_t)tcol[t];
      double2 s = make_double2(0.0, 0.0);
      for (int u = u0; u < u1; ++u) {
        const double2 b = tval[u];
        const size_t rb = (size_t)trow[u], cb = (size_t)tcol[u];
        const double2 x = rho[rb * n2 + ra], y = rho[cb * n2 + ca];
        const double dx = (ca == cb ? 1.0 : 0.0) - y.x, dy = -y.y;
        const double zr = x.x * dx + x.y * dy, zi = x.x * dy - x.y * dx;   // conj(x) (δ - y)
        s.x += b.x * zr + b.y * zi;                                        // conj(b) ·
        s.y += b.x * zi - b.y * zr;
      }
      acc.x += a.x * s.x - a.y * s.y;
      acc.y += a.x * s.y + a.y * s.x;
    }
  }
  part[((size_t)p * ny + c) * N + r] = acc;
}

// out[p N + r] = scale Σ_{c < nc} part[(p nc + c) N + r], c ascending
__global__ void __launch_bounds__(kCorrTile)
k_corr_sum(const double2* __restrict__ part, int N, int nc, int64_t total, double scale, double2* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kCorrTile + threadIdx.x;
  if (e >= total) return;
  const int64_t p = e / N, r = e % N;
  const double2* q = part + (size_t)p * nc * N + r;
  double2 acc = make_double2(0.0, 0.0);
  for (int c = 0; c < nc; ++c) {
    const double2 v = q[(size_t)c * N];
    acc.x += v.x;
    acc.y += v.y;
  }
  out[e] = make_double2(scale * acc.x, scale * acc.y);
}

// out[e] = Σ_t tval[t] ρ[tcol[t], trow[t]] over the terms of (family, site) e < total
__global__ void __launch_bounds__(kCorrTile)
k_corr_mean(const double2* __restrict__ rho, int n2, const int* __restrict__ tptr, const int* __restrict__ trow,
            const int* __restrict__ tcol, const double2* __restrict__ tval, int64_t total,
            double2* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kCorrTile + threadIdx.x;
  if (e >= total) return;
  double2 acc = make_double2(0.0, 0.0);
  const int t1 = tptr[e + 1];
  for (int t = tptr[e]; t < t1; ++t) {
    const double2 a = tval[t], y = rho[(size_t)trow[t] * n2 + tcol[t]];
    acc.x += a.x * y.x - a.y * y.y;
    acc.y += a.x * y.y + a.y * y.x;
  }
  out[e] = acc;
}

}  // namespace

void launch_corr(const double2* rho, int N, int Lx, const int* tptr, const int* trow, const int* tcol,
                 const double2* tval, const int* pairs, int npairs, const int* jlist, int nj, double2* part,
                 hipStream_t s) {
  if (npairs <= 0 || nj <= 0) return;
  const int chunk = jlist ? 1 : kCorrChunk;
  const int ntiles = cdiv(N, kCorrTile), ny = cdiv(nj, chunk);
  hipLaunchKernelGGL(k_corr, dim3((unsigned)((int64_t)ntiles * ny * npairs)), dim3(kCorrTile), 0, s, rho, 2 * N, N, Lx,
                     tptr, trow, tcol, tval, pairs, jlist, chunk, nj, ntiles, ny, part);
}

void launch_corr_sum(const double2* part, int N, int npairs, double2* out, hipStream_t s) {
  if (npairs <= 0) return;
  const int64_t total = (int64_t)npairs * N;
  hipLaunchKernelGGL(k_corr_sum, dim3((unsigned)cdiv(total, kCorrTile)), dim3(kCorrTile), 0, s, part, N,
                     corr_chunks(N), total, 1.0 / N, out);
}

void launch_corr_mean(const double2* rho, int N, const int* tptr, const int* trow, const int* tcol,
                      const double2* tval, int nfam, double2* out, hipStream_t s) {
  const int64_t total = (int64_t)nfam * N;
  hipLaunchKernelGGL(k_corr_mean, dim3((unsigned)cdiv(total, kCorrTile)), dim3(kCorrTile), 0, s, rho, 2 * N, tptr,
                     trow, tcol, tval, total, out);
}

}  // namespace dwh
