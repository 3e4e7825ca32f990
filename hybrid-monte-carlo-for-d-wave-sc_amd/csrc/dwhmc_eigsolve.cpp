// The eigensolver driver of the C-ABI context (include/dwhmc.h): the library's
// own solvers (dwhmc_eig.hip, dwhmc_qeig.hip), with rocSOLVER beyond their
// order and as the re-solve of a non-finite result, and the entry points that
// return or stage an eigensystem.  The measurements (dwhmc_measure.cpp) and
// the step path (algo eig) call eigen_solve.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "dwhmc_ctx.h"

using namespace dwh;

// the buffers of slot k
dwh::TrBufs dwh::tr_slot(const dwh_ctx* ctx, int k) {
  const size_t n2 = 2 * (size_t)ctx->d.N, N = ctx->d.N;
  dwh::TrBufs b = ctx->tr;
  const size_t mat = n2 * n2 * k, vec = n2 * k;
  b.U += mat;
  b.JU += mat;
  b.Jmn += mat;
  for (double** q : {&b.E, &b.f, &b.g, &b.dia, &b.Wn, &b.wan, &b.w0, &b.lam, &b.dc}) *q += vec;
  b.ak += N * k;
  b.scalars += 2 * k;
  b.sigma += (size_t)std::max<int64_t>(ctx->tr_nw, 0) * k;
  b.dos += (size_t)std::max<int64_t>(ctx->tr_nd, 0) * k;
  b.dos_an += (size_t)std::max<int64_t>(ctx->tr_nd, 0) * k;
  return b;
}

// dense H_BdG(Δ) of chains c0 .. c0+m-1 into slots 0 .. m-1 -> rocSOLVER zheevd
// (strided-batched for m > 1: its latency-bound panel kernels then cover every
// chain at once): eigenvalues ascending into E, eigenvectors into the columns
// of U (diagonalize_H_BdG!, src/Hamiltonian.jl:96-114; the reference's zheevr
// and zheevd agree to rounding)
TrSrc dwh::chains_src(const dwh_ctx* ctx, int64_t c0) {
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  return TrSrc{ctx->Delta + c0 * n2, n2, c0, 1};
}

namespace {

// dense H_BdG(Δ) of the m slots' chains into A (m matrices at stride n2^2)
int assemble_slots(dwh_ctx* ctx, const TrSrc& src, int m, double2* A) {
  const int N = ctx->d.N;
  const int64_t sA = 4 * (int64_t)N * N;
  HIPCHECK(ctx, hipMemsetAsync(A, 0, (size_t)m * sA * sizeof(double2), ctx->stream));
  for (int k = 0; k < m; ++k)
    dwh::launch_tr_assemble(A + k * sA, N, ctx->hcol,
                            ctx->hval + (size_t)(src.chain0 + (int64_t)k * src.cstep) * N * kHSlots, ctx->Dcol,
                            ctx->Dsrc, src.Delta + (size_t)k * src.dstride, ctx->stream);
  HIPCHECK(ctx, hipGetLastError());
  return DWH_OK;
}

// The own eigensolver (dwhmc_eig.hip): H assembled into the slots' JU, reduced
// to tridiagonal form in place (JU becomes the reflectors V), eigenvalues by
// bisection into E, eigenvectors of T by inverse iteration (Jmn and U as
// scratch), then U = V-reflectors · Z by blocked compact-WY zgemms
// DWHMC_EIG_DEBUG=1: synchronise after each phase of the own solver and print
// its wall time to stderr (diagnosing a slow or stuck phase on the device)
struct EigPhase {
  bool on;
  hipStream_t s;
  std::chrono::steady_clock::time_point t;
  explicit EigPhase(hipStream_t st) : s(st), t(std::chrono::steady_clock::now()) {
    const char* e = std::getenv("DWHMC_EIG_DEBUG");
    on = e && *e == '1';
  }
  void mark(const char* what) {
    if (!on) return;
    const hipError_t err = hipStreamSynchronize(s);
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "eig phase %-14s %9.3f ms  %s\n", what,
                 std::chrono::duration<double, std::milli>(now - t).count(), hipGetErrorString(err));
    std::fflush(stderr);
    t = now;
  }
};

// Clusters longer than maxc (runs of eigenvalues with gaps <= kEigClusterTol
// ||T||, e.g. the degenerate shells of clean lattices, which k_eig_orth's one
// workgroup does not take): Cholesky QR, twice, on the library's own real
// products — G = Y Y^T of the cluster's rows Y of Zt (the vectors), G = R^T R
// on the host, Y <- R^-T Y — before the Löwdin step.  Replaces round 4's
// rocSOLVER zheev fallback (minutes at n = 4608).  Ud: scratch (the slots' U
// buffers, free between inverse iteration and the Löwdin step).  A
// non-positive pivot sets d_tr_bad (eigen_solve's vendor fallback, as for a
// non-finite result).  Synchronises the stream when a long cluster exists.
int long_clusters(dwh_ctx* ctx, const std::vector<double>& Eh, const std::vector<double>& tn, double* Zt, double* Ud,
                  int n, int64_t sZ, int m, int maxc, bool half) {
  hipStream_t s = ctx->stream;
  std::vector<double> G, W;
  for (int k = 0; k < m; ++k) {
    const double* E = Eh.data() + (size_t)k * n;
    const double tol = dwh::kEigClusterTol * tn[k];
    const int jstart = half ? ctx->eig_c0h[k] : 0;
    for (int j = jstart; j < n;) {
      int end = j + 1;
      while (end < n && E[end] - E[end - 1] <= tol) ++end;
      const int L = end - j;
      if (L > maxc) {
        double* Y = Zt + (int64_t)k * sZ + j;   // L x n, leading dimension n (column-major Zt)
        double* Gd = Ud + (int64_t)k * sZ;      // L x L
        double* Tmp = Gd + (int64_t)L * L;      // L x n
        G.resize((size_t)L * L);
        W.assign((size_t)L * L, 0.0);
        for (int round = 0; round < 2; ++round) {
          dwh::gemm_d('N', 'T', L, L, n, 1.0, Y, n, 0, Y, n, 0, 0.0, Gd, L, 0, 1, s);
          HIPCHECK(ctx, hipGetLastError());
          HIPCHECK(ctx, hipMemcpyAsync(G.data(), Gd, G.size() * sizeof(double), hipMemcpyDeviceToHost, s));
          HIPCHECK(ctx, hipStreamSynchronize(s));
          // G = R^T R (R upper, stored in G's upper triangle, column-major)
          bool ok = true;
          for (int c = 0; c < L && ok; ++c) {
            for (int r = 0; r <= c; ++r) {
              double x = G[(size_t)c * L + r];
              for (int q = 0; q < r; ++q) x -= G[(size_t)r * L + q] * G[(size_t)c * L + q];
              if (r < c) {
                G[(size_t)c * L + r] = x / G[(size_t)r * L + r];
              } else {
                if (!(x > 0.0)) ok = false;
                G[(size_t)c * L + c] = ok ? std::sqrt(x) : 0.0;
              }
            }
          }
          if (!ok) {
            const int one = 1;
            HIPCHECK(ctx, hipMemcpyAsync(ctx->d_tr_bad, &one, sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHECK(ctx, hipStreamSynchronize(s));
            return DWH_OK;
          }
          // W = R^-T (lower triangular): R^T W = I, forward substitution per column
          // (R^T[i][q] = R[q][i] = G[i * L + q] for q <= i)
          std::fill(W.begin(), W.end(), 0.0);
          for (int c = 0; c < L; ++c)
            for (int i = c; i < L; ++i) {
              double x = i == c ? 1.0 : 0.0;
              for (int q = c; q < i; ++q) x -= G[(size_t)i * L + q] * W[(size_t)c * L + q];
              W[(size_t)c * L + i] = x / G[(size_t)i * L + i];
            }
          HIPCHECK(ctx, hipMemcpyAsync(Gd, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, s));
          dwh::gemm_d('N', 'N', L, n, L, 1.0, Gd, L, 0, Y, n, 0, 0.0, Tmp, L, 0, 1, s);
          HIPCHECK(ctx, hipMemcpy2DAsync(Y, (size_t)n * sizeof(double), Tmp, (size_t)L * sizeof(double),
                                         (size_t)L * sizeof(double), n, hipMemcpyDeviceToDevice, s));
          HIPCHECK(ctx, hipGetLastError());
        }
        ctx->eig_long_clusters++;
      }
      j = end;
    }
  }
  return DWH_OK;
}

// sub-batch streams of own_heev_enqueue's tridiagonalisation (default / most)
constexpr int kEigStreams = 2, kEigStreamsMax = 4;

// back-transform: W = V^H U is only NB x n, so with fewer than 4 matrices its
// K range is split into up to kEigKS chunks (one batched zgemm per matrix)
#ifndef EIG_KS
#define EIG_KS 8   // (A/B builds)
#endif
constexpr int kEigKS = EIG_KS;

// the own eigensolver's per-matrix workspace for m matrices (both solvers)
int eig_scratch(dwh_ctx* ctx, int m) {
  const int N = ctx->d.N, n = 2 * N;
  const int T = (n + dwh::kEigTB - 1) / dwh::kEigTB, NB = dwh::kEigNB;
  const int nblk = std::max(1, (n - 1 + NB - 1) / NB);
  constexpr int KS = kEigKS;
  const int64_t sP = (int64_t)T * n, sT = (int64_t)nblk * NB * NB, sW = (int64_t)NB * n;
  int rc;
  if (m > ctx->eig_slots) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (void* q : {(void*)ctx->d_eig_part, (void*)ctx->d_eig_vv, (void*)ctx->d_eig_ww, (void*)ctx->d_eig_tau,
                    (void*)ctx->d_eig_dpart, (void*)ctx->d_eig_pfin, (void*)ctx->d_eig_c0, (void*)ctx->d_eig_colfin, (void*)ctx->d_eig_gpart,
                    (void*)ctx->d_eig_T, (void*)ctx->d_eig_W, (void*)ctx->d_eig_W2, (void*)ctx->d_eig_d,
                    (void*)ctx->d_eig_e, (void*)ctx->d_eig_tn})
      drop_alloc(ctx, q);
    const size_t mm = (size_t)m;
    if ((rc = dalloc(ctx, &ctx->d_eig_part, mm * sP)) || (rc = dalloc(ctx, &ctx->d_eig_vv, mm * dwh::kEigRing * n)) ||
        (rc = dalloc(ctx, &ctx->d_eig_ww, mm * dwh::kEigRing * n)) || (rc = dalloc(ctx, &ctx->d_eig_tau, mm * n)) ||
        (rc = dalloc(ctx, &ctx->d_eig_dpart, mm * 2 * dwh::kEigDeferMax * T)) ||
        (rc = dalloc(ctx, &ctx->d_eig_pfin, mm * n)) || (rc = dalloc(ctx, &ctx->d_eig_colfin, mm * n)) ||
        (rc = dalloc(ctx, &ctx->d_eig_gpart, mm * 3 * dwh::kEigGP)) ||
        (rc = dalloc(ctx, &ctx->d_eig_T, mm * sT)) || (rc = dalloc(ctx, &ctx->d_eig_W, mm * std::max<int64_t>(KS * sW, (int64_t)nblk * dwh::kEigGS * NB * NB))) ||
        (rc = dalloc(ctx, &ctx->d_eig_W2, mm * sW)) || (rc = dalloc(ctx, &ctx->d_eig_d, mm * n)) ||
        (rc = dalloc(ctx, &ctx->d_eig_e, mm * n)) || (rc = dalloc(ctx, &ctx->d_eig_tn, mm)) ||
        (rc = dalloc(ctx, &ctx->d_eig_c0, mm)))
      return rc;
    ctx->eig_slots = m;
  }
  return DWH_OK;
}

// U = (I - V_0 T_0 V_0^H) ... (I - V_last T_last V_last^H) U on the columns
// j0.. of the slots' U: the reflectors' V (n x n per matrix, column c = v_c
// on the rows > c, zeros above) and complex tau (ctx->d_eig_tau), V^H block
// by block into Vt (an n x n slot buffer); the library's own products
// (dwhmc_gemm.hip)
int eig_back_transform(dwh_ctx* ctx, const double2* V, double2* Vt, int j0, int m) {
  const int N = ctx->d.N, n = 2 * N, NB = dwh::kEigNB;
  const dwh::TrBufs& b = ctx->tr;
  const int64_t sA = (int64_t)n * n;
  const int nblk = std::max(1, (n - 1 + NB - 1) / NB);
  const int64_t sT = (int64_t)nblk * NB * NB, sW = (int64_t)NB * n;
  const int M = n - j0;
  hipStream_t s = ctx->stream;
  dwh::launch_eig_tfac(V, n, sA, ctx->d_eig_tau, ctx->d_eig_W, ctx->d_eig_T, sT, m, s);   // W as Gram scratch
  HIPCHECK(ctx, hipGetLastError());
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0), mone = make_double2(-1.0, 0.0);
  const int ks = m >= 4 ? 1 : kEigKS;
  const int64_t sWs = ks * sW;
  const int ldv = std::min(NB, n - 1);   // as k_eig_vt lays the blocks out
  dwh::launch_eig_vt(V, n, sA, Vt, m, s);
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const int r0 = blk * NB, kb = std::min(NB, n - 1 - r0), ms = n - r0 - 1;
    const double2* Vb = V + (r0 + 1) + (int64_t)r0 * n;
    double2* Us = b.U + (r0 + 1) + (int64_t)j0 * n;
    const int ldw = ks * NB;
    // W = V^H U in K chunks of c rows (a multiple of 16, the last one shorter),
    // chunk s at rows s kb of W: one launch for every (matrix, chunk)
    const int c = ks == 1 ? ms : std::max(16, ((ms + ks - 1) / ks + 15) / 16 * 16);
    const int nfull = ms / c, rem = ms - nfull * c, S = nfull + (rem > 0);
    dwh::gemm_z_chunked('N', 'N', kb, M, c, rem > 0 ? rem : c, S, one, Vt + (int64_t)r0 * n, ldv, (int64_t)c * ldv, sA,
                        Us, n, c, sA, zero, ctx->d_eig_W, ldw, kb, sWs, m, s);
    if (S == 1)   // W2 = T W on the MFMA (4x faster than k_eig_tw's LDS MACs at 16 matrices)
      dwh::gemm_z('N', 'N', kb, M, kb, one, ctx->d_eig_T + (int64_t)blk * NB * NB, NB, sT, ctx->d_eig_W, ldw, sWs,
                  zero, ctx->d_eig_W2, NB, sW, m, s);
    else
      dwh::launch_eig_tw(ctx->d_eig_T + (int64_t)blk * NB * NB, sT, ctx->d_eig_W, ldw, sWs, S, kb, M,
                         ctx->d_eig_W2, sW, m, s);
    dwh::gemm_z('N', 'N', ms, M, kb, mone, Vb, n, sA, ctx->d_eig_W2, NB, sW, one, Us, n, sA, m, s);
  }
  HIPCHECK(ctx, hipGetLastError());
  return DWH_OK;
}

int own_heev_enqueue(dwh_ctx* ctx, const TrSrc& src, int m) {
  const int N = ctx->d.N, n = 2 * N;
  const dwh::TrBufs& b = ctx->tr;
  const int64_t sA = (int64_t)n * n, sZ = 2 * sA;   // sZ in doubles
  const int T = (n + dwh::kEigTB - 1) / dwh::kEigTB;
  const int64_t sP = (int64_t)T * n;
  int rc;
  if ((rc = eig_scratch(ctx, m))) return rc;
  hipStream_t s = ctx->stream;
  double2* A = b.JU;
  EigPhase ph(s);
  if ((rc = assemble_slots(ctx, src, m, A))) return rc;
  ph.mark("assemble");
  // Batches of 8+ matrices run as sub-batches of 4+ on their own streams,
  // column by column: one sub-batch's HBM-bound pass overlaps another's
  // latency-bound reduce and step (DWHMC_EIG_STREAMS: the number of streams,
  // 1 = one stream, A/B)
  int ng = m >= 8 ? kEigStreams : 1;
  if (const char* es = std::getenv("DWHMC_EIG_STREAMS")) ng = std::max(1, std::min(std::atoi(es), kEigStreamsMax));
  ng = std::max(1, std::min(ng, m / dwh::kEigDeferMin));
  for (int g = 1; g < ng; ++g)
    if (!ctx->eig_sx[g - 1] &&
        hipStreamCreateWithFlags(&ctx->eig_sx[g - 1], hipStreamNonBlocking) != hipSuccess)
      return fail(ctx, DWH_ERR_HIP, "eigensolver stream creation failed");
  for (int g = 0; g < ng && ng > 1; ++g)
    if (!ctx->eig_ev[g] && hipEventCreateWithFlags(&ctx->eig_ev[g], hipEventDisableTiming) != hipSuccess)
      return fail(ctx, DWH_ERR_HIP, "eigensolver event creation failed");
  if (ng > 1) {
    HIPCHECK(ctx, hipEventRecord(ctx->eig_ev[0], s));
    for (int g = 1; g < ng; ++g) HIPCHECK(ctx, hipStreamWaitEvent(ctx->eig_sx[g - 1], ctx->eig_ev[0], 0));
  }
  const int64_t sDp = (int64_t)2 * dwh::kEigDeferMax * T, sGp = (int64_t)3 * dwh::kEigGP, sR = (int64_t)dwh::kEigRing * n;
  const int sw = dwh::eig_switch_col(n);
  for (int i = 0; i < n; ++i) {
    if (ph.on && i % 512 == 0 && i > 0) ph.mark("tridiag/512");
    for (int g = 0; g < ng; ++g) {
      const int64_t k0 = (int64_t)m * g / ng;
      const int mg = (int)((int64_t)m * (g + 1) / ng - k0);
      dwh::launch_eig_column(A + k0 * sA, n, i, sA, ctx->d_eig_part + k0 * sP, sP, ctx->d_eig_pfin + k0 * n,
                             ctx->d_eig_colfin + k0 * n, ctx->d_eig_vv + k0 * sR, ctx->d_eig_ww + k0 * sR,
                             ctx->d_eig_d + k0 * n, ctx->d_eig_e + k0 * n, ctx->d_eig_tau + k0 * n,
                             ctx->d_eig_dpart + k0 * sDp, ctx->d_eig_gpart + k0 * sGp, mg,
                             g ? ctx->eig_sx[g - 1] : s, sw);
    }
  }
  for (int g = 1; g < ng; ++g) {
    HIPCHECK(ctx, hipEventRecord(ctx->eig_ev[g], ctx->eig_sx[g - 1]));
    HIPCHECK(ctx, hipStreamWaitEvent(s, ctx->eig_ev[g], 0));
  }
  ph.mark("tridiag");
  dwh::launch_eig_bisect(ctx->d_eig_d, ctx->d_eig_e, n, b.E, ctx->d_eig_tn, m, s);
  ph.mark("bisect");
  double* Zt = reinterpret_cast<double*>(b.Jmn);
  double* Ud = reinterpret_cast<double*>(b.U);
  // DWHMC_EIG_MAX_CLUSTER (tests): a shorter limit for the single-workgroup
  // cluster orthonormalisation, to exercise the long-cluster path below
  int maxc = dwh::kEigMaxCluster;
  if (const char* e = std::getenv("DWHMC_EIG_MAX_CLUSTER")) maxc = std::max(1, std::min(maxc, std::atoi(e)));
  // Particle-hole half solve (H_BdG: E <-> -E with eigenvectors (u; v) <->
  // (-v*; u*)): eigenvectors of T only for the indices from
  // c0, the largest index <= n/2 below which the spectrum has a gap wider
  // than kEigZeroTol ||T|| (n/2 unless levels crowd around zero, e.g. the
  // exact zero modes of clean lattices, which are then computed whole; 0 for
  // a spectrum with degenerate levels anywhere); the
  // columns below c0 are the partners of the columns above n - c0
  // (k_eig_theta after the back-transform).  c0 comes from the eigenvalues
  // on the host (one synchronisation); every matrix computes the columns
  // [j0, n), j0 = min c0, the ones below its own c0 zeroed.  Inverse
  // iteration, the orthogonalisation and the back-transform run on ~half the
  // columns.  DWHMC_EIG_HALF=0: every column (A/B).
  const char* eh = std::getenv("DWHMC_EIG_HALF");
  const bool half = n % 2 == 0 && !(eh && *eh == '0');
  ctx->eig_half = half;
  ctx->eig_c0h.assign(half ? m : 0, N);
  int j0 = 0;
  // the eigenvalues on the host (one synchronisation): the half solve's c0
  // and the clusters longer than maxc
  std::vector<double> Eh((size_t)m * n), tn(m);
  HIPCHECK(ctx, hipMemcpyAsync(Eh.data(), b.E, Eh.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(ctx, hipMemcpyAsync(tn.data(), ctx->d_eig_tn, m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  if (half) {
    j0 = N;
    for (int k = 0; k < m; ++k) {
      const double* E = Eh.data() + (size_t)k * n;
      const double tol = dwh::kEigZeroTol * tn[k];
      int c = N;
      while (c > 0 && !(E[c] - E[c - 1] > tol)) --c;   // (NaN gaps: keep going, c -> 0)
      // degenerate levels (clean lattices: most levels in clusters) leave the
      // partner images' overlaps with the computed vectors at ~1e-13 and
      // above; such a matrix computes every vector (c0 = 0)
      const double ctol = dwh::kEigClusterTol * tn[k];
      for (int j = 1; j < n && c > 0; ++j)
        if (!(E[j] - E[j - 1] > ctol)) c = 0;
      ctx->eig_c0h[k] = c;
      j0 = std::min(j0, c);
    }
    HIPCHECK(ctx, hipMemcpyAsync(ctx->d_eig_c0, ctx->eig_c0h.data(), m * sizeof(int), hipMemcpyHostToDevice, s));
    ph.mark("c0");
  }
  const int M = n - j0;   // eigenvector columns computed
  dwh::launch_eig_invit(ctx->d_eig_d, ctx->d_eig_e, n, b.E, ctx->d_eig_tn, Zt, Zt + sA, Ud, Ud + sA, sZ,
                        ctx->d_tr_bad, m, s, maxc, j0, half ? ctx->d_eig_c0 : nullptr);
  ph.mark("invit+orth");
  if ((rc = long_clusters(ctx, Eh, tn, Zt, Ud, n, sZ, m, maxc, half))) return rc;
  ph.mark("long clusters");
  // One symmetric (Löwdin) orthogonalisation step over the computed vectors:
  // with Y = Z^T (column-major Zt, its rows j0.. the vectors) and G = Y Y^T =
  // I + F, Y <- (3/2 I - 1/2 G) Y leaves ||F|| -> O(||F||^2).  Outside clusters
  // F_jl ~ c eps ||T|| / |λ_j - λ_l| (inverse iteration's per-vector error), so
  // the mixing moves each residual by ~ F_jl |λ_j - λ_l| ~ c eps ||T||:
  // orthogonality to rounding, accuracy kept.  (Zeroed partner rows stay zero.)
  double* G = Ud;          // the slots' U buffers (LU scratch until now)
  double* Y2 = Zt + sA;    // second half of the slots' Jmn buffers
  dwh::gemm_d('N', 'T', M, M, n, 1.0, Zt + j0, n, sZ, Zt + j0, n, sZ, 0.0, G, M, sZ, m, s);
  HIPCHECK(ctx, hipMemcpy2DAsync(Y2, sZ * sizeof(double), Zt, sZ * sizeof(double), sA * sizeof(double), m,
                                 hipMemcpyDeviceToDevice, s));
  dwh::gemm_d('N', 'N', M, n, M, -0.5, G, M, sZ, Zt + j0, n, sZ, 1.5, Y2 + j0, n, sZ, m, s);
  dwh::launch_eig_zt_to_u(Y2, b.U, n, sZ, sA, m, s, j0);
  HIPCHECK(ctx, hipGetLastError());
  ph.mark("lowdin");
  if (n < 2) return DWH_OK;
  // V^H block by block into the slots' Jmn buffers (free after the Löwdin step)
  if ((rc = eig_back_transform(ctx, A, b.Jmn, j0, m))) return rc;
  if (half) dwh::launch_eig_theta(b.U, n, sA, ctx->d_eig_c0, m, s);
  ph.mark("backtransform");
  HIPCHECK(ctx, hipGetLastError());
  return DWH_OK;
}

int eigen_enqueue(dwh_ctx* ctx, const TrSrc& src, int m, bool qr) {
  const int N = ctx->d.N, n2 = 2 * N;
  const dwh::TrBufs& b = ctx->tr;
  const int64_t sA = (int64_t)n2 * n2;
  if (int rc = assemble_slots(ctx, src, m, b.U)) return rc;
  auto* A = reinterpret_cast<rocblas_double_complex*>(b.U);
  rocblas_status st;
  if (qr)
    st = m == 1 ? rocsolver_zheev(ctx->blas, rocblas_evect_original, rocblas_fill_upper, n2, A, n2, b.E,
                                  ctx->d_tr_offd, ctx->d_tr_info)
                : rocsolver_zheev_strided_batched(ctx->blas, rocblas_evect_original, rocblas_fill_upper, n2, A, n2,
                                                  sA, b.E, n2, ctx->d_tr_offd, n2, ctx->d_tr_info, m);
  else
    st = m == 1 ? rocsolver_zheevd(ctx->blas, rocblas_evect_original, rocblas_fill_upper, n2, A, n2, b.E,
                                   ctx->d_tr_offd, ctx->d_tr_info)
                : rocsolver_zheevd_strided_batched(ctx->blas, rocblas_evect_original, rocblas_fill_upper, n2, A,
                                                   n2, sA, b.E, n2, ctx->d_tr_offd, n2, ctx->d_tr_info, m);
  if (st != rocblas_status_success)
    return fail(ctx, DWH_ERR_HIP, std::string("rocsolver_zheevd: ") + rocblas_status_to_string(st));
  return DWH_OK;
}

int q_heev_enqueue(dwh_ctx* ctx, const TrSrc& src, int m, bool* done);

}  // namespace

// The library's own eigensolver for every order up to kEigMaxN; rocSOLVER only
// beyond it (zheevd) and as the re-solve (QR-iteration zheev) of a solve that
// left a non-finite value: rocSOLVER's zheevd returns NaN eigenvectors for
// spectra with exactly degenerate eigenvalues (the clean lattice, W = 0).
// Synchronises the stream.
int dwh::eigen_solve(dwh_ctx* ctx, const TrSrc& src, int m) {
  int rc;
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  const bool own = n2 <= dwh::kEigMaxN;
  ctx->eig_ph = false;
  ctx->eig_ph_last = 0;   // dwh_info_t::eig_half describes this solve on every exit path
  ctx->eig_quat_last = 0;   // and eig_quat: 0 on the rocSOLVER route and after a zheev re-solve
  if (ctx->dbg_nstates > 0) {
    // dwh_debug_set_eigensystem: the staged (E, U) into the slots, once
    const int ns = ctx->dbg_nstates;
    const bool ph = ctx->dbg_ph;
    std::vector<double> Eh;
    std::vector<double2> Uh;
    Eh.swap(ctx->dbg_E);
    Uh.swap(ctx->dbg_U);
    ctx->dbg_nstates = 0;
    ctx->dbg_ph = false;
    if (ns != m)
      return fail(ctx, DWH_ERR_ARG, "dwh_debug_set_eigensystem staged " + std::to_string(ns) +
                                        " eigensystems, the eigensolve that followed has " + std::to_string(m) +
                                        " (staging cleared)");
    HIPCHECK(ctx, hipMemsetAsync(ctx->d_tr_info, 0, m * sizeof(int), ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->tr.E, Eh.data(), Eh.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->tr.U, Uh.data(), Uh.size() * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));   // (Eh, Uh leave scope)
    ctx->eig_ph = ph;
    ctx->eig_ph_last = ph ? 1 : 0;
    return DWH_OK;
  }
  HIPCHECK(ctx, hipMemsetAsync(ctx->d_tr_bad, 0, sizeof(int), ctx->stream));
  if (own) {
    // the own solver (k_eig_orth flags an over-long cluster in d_tr_bad);
    // rocSOLVER zheev only if it flagged or produced non-finite values
    HIPCHECK(ctx, hipMemsetAsync(ctx->d_tr_info, 0, m * sizeof(int), ctx->stream));
    Scope sc(ctx, T_EIG_OWN, m);
    // the structure-preserving solver first (DWHMC_EIG_QUAT=0: the one-stage
    // solver only, A/B); it declines spectra with over-long clusters or crowds
    bool done = false;
    const char* qe = std::getenv("DWHMC_EIG_QUAT");
    if (dwh::q_supported(ctx->d.N) && !(qe && *qe == '0')) rc = q_heev_enqueue(ctx, src, m, &done);
    else rc = DWH_OK;
    if (!rc && !done) rc = own_heev_enqueue(ctx, src, m);
    ctx->eig_quat_last = done ? 1 : 0;
  } else {
    Scope sc(ctx, T_EIG_VENDOR, m);
    rc = eigen_enqueue(ctx, src, m, false);
  }
  if (rc) return rc;
  dwh::launch_nonfinite(ctx->tr.U, m * n2 * n2, ctx->tr.E, m * n2, ctx->d_tr_bad, ctx->stream);
  int bad = 0;
  HIPCHECK(ctx, hipMemcpyAsync(&bad, ctx->d_tr_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (!bad && own && ctx->eig_half && (int)ctx->eig_c0h.size() == m)
    ctx->eig_ph = std::all_of(ctx->eig_c0h.begin(), ctx->eig_c0h.end(), [&](int c) { return c == ctx->d.N; });
  ctx->eig_ph_last = ctx->eig_ph ? 1 : 0;
  if (bad) {
    Scope sc(ctx, T_EIG_VENDOR, m);
    ctx->eig_quat_last = 0;   // the result is rocSOLVER's
    rc = eigen_enqueue(ctx, src, m, true);
  }
  return rc;
}

int dwh::eigen_info_check(dwh_ctx* ctx, int m) {
  std::vector<int> info(m, 0);
  HIPCHECK(ctx, hipMemcpyAsync(info.data(), ctx->d_tr_info, m * sizeof(int), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHECK(ctx, hipGetLastError());
  for (int k = 0; k < m; ++k)
    if (info[k] != 0)
      return fail(ctx, DWH_ERR_HIP, "the rocSOLVER eigensolver (zheevd / zheev fallback) did not converge (info = " +
                                        std::to_string(info[k]) + ")");
  return DWH_OK;
}

namespace {

// Workspace of the structure-preserving solver (dwhmc_qeig.hip) for q_slots
// matrices, one array per quantity (the kernels' per-matrix strides):
// reduction scratch, w, y, the diagonal blocks before / after the site
// rotations, the rotations, tau, ||T||; for the eigenvectors (q_vec_slots
// matrices, nv = N columns): Zt (n x nv), the inverse iteration's LU
// scratch, the Löwdin Gram matrix (nv x nv).
struct QBufs {
  double2 *part, *W, *Y, *qd, *rd, *G;
  double *tau, *qa, *ra, *rb, *tn;
  int64_t sP;
};
QBufs q_bufs(dwh_ctx* ctx) {
  const int M = ctx->d.N, n = 2 * M, m = ctx->q_slots;
  const int64_t sP = dwh::q_part_elems(M);
  double* w = ctx->d_q;
  QBufs q;
  q.sP = sP;
  int64_t o = 0;   // doubles
  auto take2 = [&](int64_t per) { double2* p = reinterpret_cast<double2*>(w + o); o += 2 * per * m; return p; };
  auto take1 = [&](int64_t per) { double* p = w + o; o += per * m; return p; };
  q.part = take2(sP);
  q.W = take2(n);
  q.Y = take2(n);
  q.qd = take2(M);
  q.rd = take2(M);
  q.G = take2(n);
  q.tau = take1(M);
  q.qa = take1(M);
  q.ra = take1(M);
  q.rb = take1(M);
  q.tn = take1(2);
  return q;
}
int64_t q_bufs_doubles(int M, int m) {
  const int n = 2 * M;
  return m * (2 * (int64_t)dwh::q_part_elems(M) + 2 * (3 * (int64_t)n + 2 * M) + 4 * (int64_t)M + 2);
}

// Eigenvalues by the structure-preserving reduction: H_BdG of the m sources
// assembled into the slots' JU, reduced site by site on their particle rows
// (the reflectors left in JU's bottom rows), site rotations, block Sturm
// bisection; the 2N ascending eigenvalues of each into the slots' E (device).
// ms (optional, m = 1): the reduction's device time (HIP events; synchronises).
int qeig_values(dwh_ctx* ctx, const TrSrc& src, int m, float* ms) {
  const int M = ctx->d.N, n = 2 * M;
  if (!dwh::q_supported(M)) return fail(ctx, DWH_ERR_ARG, "structure-preserving solver: lattice too large");
  const int64_t sA = (int64_t)n * n;
  int rc;
  if (m > ctx->q_slots) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    drop_alloc(ctx, ctx->d_q);
    ctx->d_q = nullptr;
    ctx->q_slots = 0;
    if ((rc = dalloc(ctx, &ctx->d_q, (size_t)q_bufs_doubles(M, m)))) return rc;
    ctx->q_slots = m;
  }
  const QBufs q = q_bufs(ctx);
  hipStream_t s = ctx->stream;
  double2* A = ctx->tr.JU;
  if ((rc = assemble_slots(ctx, src, m, A))) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ms) {
    HIPCHECK(ctx, hipEventCreate(&e0));
    HIPCHECK(ctx, hipEventCreate(&e1));
    HIPCHECK(ctx, hipEventRecord(e0, s));
  }
  dwh::launch_q_reduce(A, M, sA, q.part, q.sP, q.W, q.tau, q.Y, q.qa, q.qd, m, s);
  if (ms) HIPCHECK(ctx, hipEventRecord(e1, s));
  dwh::launch_q_rot(q.qa, q.qd, q.Y, M, q.ra, q.rd, q.rb, q.G, m, s);
  dwh::launch_q_bisect(q.ra, q.rd, q.rb, M, ctx->tr.E, q.tn, m, s);
  HIPCHECK(ctx, hipGetLastError());
  if (ms) {
    HIPCHECK(ctx, hipStreamSynchronize(s));
    HIPCHECK(ctx, hipEventElapsedTime(ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return DWH_OK;
}

// Every eigenpair by the structure-preserving solver (m matrices): qeig_values,
// then — when no matrix's spectrum has a cluster (consecutive gaps <=
// kEigClusterTol ||T||) longer than q_max_cluster() or a crowd at zero
// (q_zero_crowd) longer than half that, checked on the host from the
// eigenvalues (one synchronisation) — the particle-hole half: inverse
// iteration on T for the N upper eigenvalues (k_q_invit), the clusters and
// the crowd orthonormalised (k_q_orth), one Löwdin step (the library's complex
// products), the site rotations into U' (interleaved rows), the reflector
// pairs as a one-stage V and its back-transform, then the BdG row order and
// the Theta partners for the lower half (k_q_final).  *done = false: not
// taken (the caller runs the one-stage solver; the slots' JU / E are
// overwritten either way).
int q_heev_enqueue(dwh_ctx* ctx, const TrSrc& src, int m, bool* done) {
  *done = false;
  const int N = ctx->d.N, n = 2 * N, j0 = N, nv = n - j0;
  const dwh::TrBufs& b = ctx->tr;
  const int64_t sA = (int64_t)n * n;
  int rc;
  if ((rc = qeig_values(ctx, src, m, nullptr))) return rc;
  const QBufs q = q_bufs(ctx);
  hipStream_t s = ctx->stream;
  const char* eh = std::getenv("DWHMC_EIG_HALF");   // =0: every column solved (the one-stage solver)
  if (n % 2 || (eh && *eh == '0')) return DWH_OK;
  std::vector<double> Eh((size_t)m * n), tn((size_t)2 * m);
  HIPCHECK(ctx, hipMemcpyAsync(Eh.data(), b.E, Eh.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(ctx, hipMemcpyAsync(tn.data(), q.tn, m * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  // Crowding at zero matters through E_j + E_k of two computed vectors j != k
  // (x_j against the partner Theta x_k, which the Löwdin step does not
  // see): E_N + E_{N+1} <= kEigZeroTol ||T||, the one-stage half solve's
  // bound on it.  A single level near zero is harmless: x_N and Theta x_N
  // are orthogonal exactly (<u, Theta u> = 0 for Theta^2 = -1).
  // Clusters (consecutive gaps <= kEigClusterTol ||T||) up to q_max_cluster()
  // long are orthonormalised in the structure-preserving path (k_q_orth);
  // longer ones are declined.
  // A crowd at zero (q_zero_crowd) of up to q_max_cluster() / 2 levels is
  // orthonormalised together with its Theta partners (k_q_orth).
  bool clusters = false;
  for (int k = 0; k < m; ++k) {
    const double* E = Eh.data() + (size_t)k * n;
    const int crowd = dwh::q_zero_crowd(E, n, j0, tn[k]);
    if (2 * crowd > dwh::q_max_cluster()) return DWH_OK;
    clusters = clusters || crowd > 0;
    int run = 1;
    for (int j = j0 + std::max(crowd, 1); j < n; ++j) {
      if (!(E[j] - E[j - 1] > dwh::kEigClusterTol * tn[k])) {
        clusters = true;
        if (++run > dwh::q_max_cluster()) return DWH_OK;
      } else {
        run = 1;
      }
    }
  }
  // vector workspace
  const int64_t sZ = (int64_t)n * nv, sS = dwh::q_invit_scratch(N, j0), sG = (int64_t)nv * nv;
  if (m > ctx->q_vec_slots) {
    HIPCHECK(ctx, hipStreamSynchronize(s));
    for (void* p : {(void*)ctx->d_qz, (void*)ctx->d_qs, (void*)ctx->d_qg}) drop_alloc(ctx, p);
    ctx->d_qz = ctx->d_qs = ctx->d_qg = nullptr;
    ctx->q_vec_slots = 0;
    if ((rc = dalloc(ctx, &ctx->d_qz, (size_t)m * sZ)) || (rc = dalloc(ctx, &ctx->d_qs, (size_t)m * sS)) ||
        (rc = dalloc(ctx, &ctx->d_qg, (size_t)m * sG)))
      return rc;
    ctx->q_vec_slots = m;
  }
  if ((rc = eig_scratch(ctx, m))) return rc;
  EigPhase ph(s);
  ph.mark("q values");
  dwh::launch_q_invit(q.ra, q.rd, q.rb, N, b.E, q.tn, j0, ctx->d_qz, sZ, ctx->d_qs, sS, m, s);
  if (clusters) dwh::launch_q_orth(b.E, q.tn, N, j0, ctx->d_qz, sZ, dwh::kEigClusterTol, ctx->d_tr_bad, m, s);
  ph.mark("q invit");
  // Löwdin on X = Zt (nv x n, ld nv): G' = X X^H (= conj(Z^H Z)), Y^T = 1.5 X - 0.5 G' X into the slots' Jmn
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  dwh::gemm_z('N', 'C', nv, nv, n, one, ctx->d_qz, nv, sZ, ctx->d_qz, nv, sZ, zero, ctx->d_qg, nv, sG, m, s);
  HIPCHECK(ctx, hipMemcpy2DAsync(b.Jmn, sA * sizeof(double2), ctx->d_qz, sZ * sizeof(double2), sZ * sizeof(double2), m,
                                 hipMemcpyDeviceToDevice, s));
  dwh::gemm_z('N', 'N', nv, n, nv, make_double2(-0.5, 0.0), ctx->d_qg, nv, sG, ctx->d_qz, nv, sZ,
              make_double2(1.5, 0.0), b.Jmn, nv, sA, m, s);
  // the site rotations, transposed into the slots' U columns j0.. (interleaved rows)
  dwh::launch_q_ztu(b.Jmn, sA, q.G, N, j0, b.U, sA, m, s);
  ph.mark("q lowdin");
  // the reflector pairs as V (slots' Jmn) and complex tau; V^H blocks into the slots' JU
  dwh::launch_q_vexpand(b.JU, sA, q.tau, N, b.Jmn, ctx->d_eig_tau, m, s);
  HIPCHECK(ctx, hipGetLastError());
  if ((rc = eig_back_transform(ctx, b.Jmn, b.JU, j0, m))) return rc;
  ph.mark("q backtransform");
  // BdG row order and the Theta partners, through the slots' JU
  dwh::launch_q_final(b.U, sA, N, j0, b.JU, m, s);
  HIPCHECK(ctx, hipMemcpyAsync(b.U, b.JU, (size_t)m * sA * sizeof(double2), hipMemcpyDeviceToDevice, s));
  HIPCHECK(ctx, hipGetLastError());
  ph.mark("q final");
  ctx->eig_half = true;
  ctx->eig_c0h.assign(m, N);
  *done = true;
  return DWH_OK;
}

}  // namespace

extern "C" {

// Development entry (tools/qeig_check.py): qeig_values of `chain`, the
// eigenvalues into E and the reduction's device time into *ms.
int dwh_debug_qeig(dwh_ctx* ctx, int64_t chain, double* E, double* ms) {
  if (!ctx || !E) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), 1)))
    return rc;
  float t = 0.0f;
  if ((rc = qeig_values(ctx, chains_src(ctx, chain), 1, &t))) return rc;
  const int M = ctx->d.N;
  HIPCHECK(ctx, hipMemcpyAsync(E, ctx->tr.E, 2 * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (ms) *ms = t;
#ifdef QSTAMPS
  if (const char* f = std::getenv("QSTAMPS_FILE")) {   // diagnostic builds: the phase stamps
    std::vector<unsigned long long> st((size_t)std::min(M, 4096) * 16);
    if (dwh::q_stamps_read(st.data(), std::min(M, 4096)) == 0)
      if (FILE* fp = std::fopen(f, "wb")) {
        std::fwrite(st.data(), sizeof(unsigned long long), st.size(), fp);
        std::fclose(fp);
      }
  }
#endif
  return DWH_OK;
}

int dwh_eigensystem(dwh_ctx* ctx, int64_t chain, double* E, dwh_c128* U) {
  if (!ctx || !E) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), 1)))
    return rc;
  const size_t n2 = 2 * (size_t)ctx->d.N;
  if (!U && dwh::q_supported(ctx->d.N) && (int64_t)n2 <= dwh::kEigMaxN) {
    // eigenvalues only: the structure-preserving reduction (half the
    // launches and a quarter of the pass traffic of the one-stage path)
    Scope sc(ctx, T_EIG_OWN, 1);
    ctx->eig_ph = false;
    ctx->eig_ph_last = 0;
    if ((rc = qeig_values(ctx, chains_src(ctx, chain), 1, nullptr))) return rc;
    HIPCHECK(ctx, hipMemsetAsync(ctx->d_tr_bad, 0, sizeof(int), ctx->stream));
    dwh::launch_nonfinite(ctx->tr.U, 0, ctx->tr.E, (int64_t)n2, ctx->d_tr_bad, ctx->stream);
    int bad = 0;
    HIPCHECK(ctx, hipMemcpyAsync(E, ctx->tr.E, n2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(&bad, ctx->d_tr_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (!bad) return DWH_OK;   // (non-finite eigenvalues: the full solve below)
  }
  if ((rc = eigen_solve(ctx, chains_src(ctx, chain), 1))) return rc;
  HIPCHECK(ctx, hipMemcpyAsync(E, ctx->tr.E, n2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (U)
    HIPCHECK(ctx, hipMemcpyAsync(U, ctx->tr.U, n2 * n2 * sizeof(double2), hipMemcpyDeviceToHost,
                                 ctx->stream));
  return eigen_info_check(ctx, 1);
}

int dwh_debug_set_eigensystem(dwh_ctx* ctx, int64_t nstates, const double* E, const dwh_c128* U, int32_t ph) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  ctx->dbg_nstates = 0;   // a refused call leaves nothing staged
  ctx->dbg_E.clear();
  ctx->dbg_U.clear();
  if (!E || !U) return fail(ctx, DWH_ERR_ARG, "NULL argument (E or U)");
  const int64_t cap = tr_group(ctx, INT32_MAX);
  if (nstates < 1 || nstates > cap)
    return fail(ctx, DWH_ERR_ARG, "nstates must be in [1, " + std::to_string(cap) + "] (the slots of one eigensolve)");
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  for (int64_t k = 0; k < nstates; ++k) {
    const double* e = E + k * n2;
    double emax = 0.0;
    for (int64_t n = 0; n < n2; ++n) {
      if (!std::isfinite(e[n])) return fail(ctx, DWH_ERR_ARG, "non-finite eigenvalue in state " + std::to_string(k));
      if (n > 0 && e[n] < e[n - 1])
        return fail(ctx, DWH_ERR_ARG, "eigenvalues of state " + std::to_string(k) + " are not ascending at " +
                                          std::to_string(n));
      emax = std::max(emax, std::fabs(e[n]));
    }
    if (ph)
      for (int64_t n = 0; n < n2; ++n)
        if (std::fabs(e[n] + e[n2 - 1 - n]) > 1e-12 * (1.0 + emax))
          return fail(ctx, DWH_ERR_ARG, "ph: E[n] + E[2N-1-n] of state " + std::to_string(k) + " is not zero at " +
                                            std::to_string(n));
  }
  const int64_t nu = nstates * n2 * n2;
  for (int64_t i = 0; i < nu; ++i)
    if (!std::isfinite(U[i].re) || !std::isfinite(U[i].im))
      return fail(ctx, DWH_ERR_ARG, "non-finite eigenvector entry");
  ctx->dbg_E.assign(E, E + nstates * n2);
  ctx->dbg_U.resize((size_t)nu);
  for (int64_t i = 0; i < nu; ++i) ctx->dbg_U[(size_t)i] = make_double2(U[i].re, U[i].im);
  ctx->dbg_nstates = (int)nstates;
  ctx->dbg_ph = ph != 0;
  return DWH_OK;
}

}  // extern "C"
