// Measurement half of the C-ABI context (include/dwhmc.h): the eigensolver
// driver — the library's own solvers (dwhmc_eig.hip, dwhmc_qeig.hip), with
// rocSOLVER beyond their order and as the re-solve of a non-finite result —
// and the transport / spectra measurement built on it (dwhmc_transport.hip),
// with their entry points.  The step path (algo eig) calls eigen_solve too.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "dwhmc_ctx.h"

using namespace dwh;

namespace {

// ---------------------------------------------------------------------------
// transport / spectra measurement (src/Observables.jl:314-526)
// ---------------------------------------------------------------------------

// length(start:step:stop) of the Julia float ranges of src/Observables.jl:395,430:
// the step count is rounded when (stop - start)/step is an integer up to
// rounding (Base.floatrange), else floored
int64_t julia_range_len(double start, double step, double stop) {
  const double r = (stop - start) / step;
  const double n = std::nearbyint(r);
  const double k = std::fabs(r - n) < 1e-8 * std::max(1.0, std::fabs(r)) ? n : std::floor(r);
  return k < 0 ? 0 : (int64_t)k + 1;
}

// The current-response workspace (response_run allocates it on first use)
// goes where the slot buffers are reallocated: both scale with n2², so a
// caller that grows the slots gets this memory back first.  The operator
// response (operator_run) works in the same buffers plus its χ'' partials, the
// Nambu cross response (nambu_run) in them plus its resident X, chi2
// partials and pair list.
void response_release(dwh_ctx* ctx) {
  for (void* q : {(void*)ctx->d_rs_ws, (void*)ctx->d_rs_val, (void*)ctx->d_rs_part, (void*)ctx->d_rs_out,
                  (void*)ctx->d_rs_col, (void*)ctx->d_rs_idx, (void*)ctx->d_op_part, (void*)ctx->d_nb_x,
                  (void*)ctx->d_nb_part, (void*)ctx->d_nb_pairs})
    drop_alloc(ctx, q);
  ctx->d_rs_ws = ctx->d_rs_val = ctx->d_nb_x = nullptr;
  ctx->d_rs_part = ctx->d_rs_out = ctx->d_op_part = ctx->d_nb_part = nullptr;
  ctx->d_rs_col = ctx->d_rs_idx = ctx->d_nb_pairs = nullptr;
  ctx->rs_mats = ctx->rs_npart = ctx->rs_nout = ctx->rs_nval = ctx->rs_ncol = ctx->rs_nidx = ctx->op_npart = 0;
  ctx->nb_nx = ctx->nb_npart = ctx->nb_npairs = 0;
}

}  // namespace

// device buffers + rocBLAS handle on first use.  Buffers hold `slots` chains
// (one slot per chain of a batched measurement), each slot laid out as
// TrBufs; the σ partials are shared (chains are reduced one after another).
int dwh::transport_prepare(dwh_ctx* ctx, int64_t nw, int64_t nd, int slots) {
  const int N = ctx->d.N;
  const size_t n2 = 2 * (size_t)N;
  dwh::TrBufs& b = ctx->tr;
  int rc = DWH_OK;
  if (!ctx->blas) {
    if (rocblas_create_handle(&ctx->blas) != rocblas_status_success)
      return fail(ctx, DWH_ERR_HIP, "rocblas_create_handle failed");
    if (rocblas_set_stream(ctx->blas, ctx->stream) != rocblas_status_success)
      return fail(ctx, DWH_ERR_HIP, "rocblas_set_stream failed");
    const HostModel& m = *ctx->model;
    if ((rc = dalloc(ctx, &ctx->d_tr_nbr, m.tr_nbr.size())) ||
        (rc = dalloc(ctx, &ctx->d_tr_rowptr, m.tr_rowptr.size())) ||
        (rc = dalloc(ctx, &ctx->d_tr_col, m.tr_col.size())) ||
        (rc = dalloc(ctx, &ctx->d_tr_val, m.tr_val.size())) || (rc = dalloc(ctx, &ctx->d_tr_bad, 1)))
      return rc;
    auto up = [&](void* dst, const void* src, size_t bytes) {
      return bytes == 0 ? hipSuccess : hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream);
    };
    HIPCHECK(ctx, up(ctx->d_tr_nbr, m.tr_nbr.data(), m.tr_nbr.size() * sizeof(int)));
    HIPCHECK(ctx, up(ctx->d_tr_rowptr, m.tr_rowptr.data(), m.tr_rowptr.size() * sizeof(int)));
    HIPCHECK(ctx, up(ctx->d_tr_col, m.tr_col.data(), m.tr_col.size() * sizeof(int)));
    HIPCHECK(ctx, up(ctx->d_tr_val, m.tr_val.data(), m.tr_val.size() * sizeof(double)));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (slots > ctx->tr_slots) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (void* q : {(void*)b.U, (void*)b.JU, (void*)b.Jmn, (void*)b.E, (void*)b.f, (void*)b.g, (void*)b.dia, (void*)b.Wn,
                    (void*)b.wan, (void*)b.w0, (void*)b.lam, (void*)b.dc, (void*)ctx->d_tr_offd, (void*)b.ak,
                    (void*)b.scalars, (void*)ctx->d_tr_info})
      drop_alloc(ctx, q);
    response_release(ctx);
    const size_t m = (size_t)slots;
    if ((rc = dalloc(ctx, &b.U, m * n2 * n2)) || (rc = dalloc(ctx, &b.JU, m * n2 * n2)) ||
        (rc = dalloc(ctx, &b.Jmn, m * n2 * n2)))
      return rc;
    for (double** q : {&b.E, &b.f, &b.g, &b.dia, &b.Wn, &b.wan, &b.w0, &b.lam, &b.dc, &ctx->d_tr_offd})
      if ((rc = dalloc(ctx, q, m * n2))) return rc;
    if ((rc = dalloc(ctx, &b.ak, m * N)) || (rc = dalloc(ctx, &b.scalars, 2 * m)) ||
        (rc = dalloc(ctx, &ctx->d_tr_info, m)))
      return rc;
    ctx->tr_slots = slots;
    ctx->tr_nw = ctx->tr_nd = -1;   // per-slot outputs below are re-sized too
  }
  if (nw != ctx->tr_nw || nd != ctx->tr_nd) {
    // partials of the σ chunks and of the DOS slices (one after the other)
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    drop_alloc(ctx, b.part);
    drop_alloc(ctx, b.sigma);
    b.part = b.sigma = nullptr;
    const size_t np = std::max<size_t>((size_t)dwh::tr_sigma_chunks(N) * nw, (size_t)2 * dwh::tr_dos_slices(N) * nd);
    if ((rc = dalloc(ctx, &b.part, std::max<size_t>(np, 1))) ||
        (rc = dalloc(ctx, &b.sigma, (size_t)ctx->tr_slots * nw)))
      return rc;
    ctx->tr_nw = nw;
  }
  if (nd != ctx->tr_nd) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    drop_alloc(ctx, b.dos);
    drop_alloc(ctx, b.dos_an);
    b.dos = b.dos_an = nullptr;
    if ((rc = dalloc(ctx, &b.dos, (size_t)ctx->tr_slots * nd)) ||
        (rc = dalloc(ctx, &b.dos_an, (size_t)ctx->tr_slots * nd)))
      return rc;
    ctx->tr_nd = nd;
  }
  return DWH_OK;
}

namespace {

// the buffers of slot k
dwh::TrBufs tr_slot(const dwh_ctx* ctx, int k) {
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

}  // namespace

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

int transport_args(dwh_ctx* ctx, double eta, double domega, double omega_max, int64_t n_omega, int64_t n_dos,
                   int64_t* nw, int64_t* nd) {
  if (dwh_transport_grid(eta, domega, omega_max, nw, nd) != DWH_OK)
    return fail(ctx, DWH_ERR_ARG, g_create_error);
  if (n_omega != *nw || n_dos != *nd)
    return fail(ctx, DWH_ERR_ARG, "n_omega / n_dos differ from dwh_transport_grid (" + std::to_string(*nw) +
                                      ", " + std::to_string(*nd) + ")");
  return DWH_OK;
}

// measure_transport_and_spectra for chains c0 .. c0+m-1 (slots 0 .. m-1);
// outputs per chain at strides 1 / nw / nd / N
int transport_run(dwh_ctx* ctx, const TrSrc& src, int m, double eta, double domega, double omega_max, int64_t nw,
                  int64_t nd, double* stiffness, double* dc_cond, double* sigma, double* dos, double* dos_an,
                  double* ak0) {
  int rc;
  if ((rc = transport_prepare(ctx, nw, nd, m))) return rc;
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2;
  hipStream_t s = ctx->stream;
  // particle-hole closed U (eig_ph): only the columns < N of J_mn are read
  const bool ph = ctx->eig_ph;
  const int ncol = ph ? N : n2;
  for (int k = 0; k < m; ++k) {
    const dwh::TrBufs b = tr_slot(ctx, k);
    dwh::launch_tr_colstats(b.U, N, (int)ctx->model->Lx, b.E, ctx->beta, eta, ctx->model->t, ctx->model->tp, ctx->d_tr_nbr, b.f,
                            b.g, b.dia, b.Wn, b.wan, b.w0, s);
    dwh::launch_tr_current(b.U, b.JU, N, ctx->d_tr_rowptr, ctx->d_tr_col, ctx->d_tr_val, ncol, s);
  }
  HIPCHECK(ctx, hipGetLastError());
  // J_mn = U^H (J ⊕ J) U  (src/Observables.jl:334-335), the library's own product
  const dwh::TrBufs& b0 = ctx->tr;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  if (ph) {
    // only columns < N of J_mn: its columns [N, n2) hold U^H half by half
    // (N x n2, ld N), so both products are 'N','N' (1.6x faster than the
    // conjugate-transposed operand: profiles/r05_exp_backtransform_vt.txt)
    double2* Ut = b0.Jmn + (int64_t)N * n2;
    for (int h = 0; h < 2; ++h) {
      dwh::launch_tr_conj_transpose(b0.U + (int64_t)h * N * n2, n2, N, n2, sA, Ut, N, sA, m, s);
      dwh::gemm_z('N', 'N', N, ncol, n2, one, Ut, N, sA, b0.JU, n2, sA, zero, b0.Jmn + (int64_t)h * N, n2, sA, m, s);
    }
  } else {
    dwh::gemm_z('C', 'N', n2, ncol, n2, one, b0.U, n2, sA, b0.JU, n2, sA, zero, b0.Jmn, n2, sA, m, s);
  }
  HIPCHECK(ctx, hipGetLastError());
  const dwh::TrGrid g{eta, -omega_max, domega, (int)nw, (int)nd};
  for (int k = 0; k < m; ++k)
    dwh::launch_tr_reduce(tr_slot(ctx, k), N, (int)ctx->model->Lx, (int)ctx->model->Ly, ctx->beta, eta, g, ph, s);
  HIPCHECK(ctx, hipGetLastError());
  std::vector<double> sc(2 * (size_t)m);
  HIPCHECK(ctx, hipMemcpyAsync(sc.data(), b0.scalars, sc.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  if (nw > 0)
    HIPCHECK(ctx, hipMemcpyAsync(sigma, b0.sigma, m * nw * sizeof(double), hipMemcpyDeviceToHost, s));
  if (nd > 0) {
    HIPCHECK(ctx, hipMemcpyAsync(dos, b0.dos, m * nd * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHECK(ctx, hipMemcpyAsync(dos_an, b0.dos_an, m * nd * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHECK(ctx, hipMemcpyAsync(ak0, b0.ak, (size_t)m * N * sizeof(double), hipMemcpyDeviceToHost, s));
  if ((rc = eigen_info_check(ctx, m))) return rc;
  for (int k = 0; k < m; ++k) {
    stiffness[k] = sc[2 * k];
    dc_cond[k] = sc[2 * k + 1];
  }
  return DWH_OK;
}

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

// the nstates Δ snapshots of a _deltas call (finite, else DWH_ERR_ARG) into
// the staging buffer (grown on demand)
int stage_deltas(dwh_ctx* ctx, int64_t nstates, const dwh_c128* Delta) {
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  for (int64_t e = 0; e < nstates * n2; ++e)
    if (!std::isfinite(Delta[e].re) || !std::isfinite(Delta[e].im)) return fail(ctx, DWH_ERR_ARG, "non-finite Delta");
  if (nstates > ctx->tr_nstage) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    drop_alloc(ctx, ctx->d_tr_stage);
    ctx->d_tr_stage = nullptr;
    ctx->tr_nstage = 0;
    if (int rc = dalloc(ctx, &ctx->d_tr_stage, (size_t)nstates * n2)) return rc;
    ctx->tr_nstage = nstates;
  }
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_tr_stage, Delta, (size_t)nstates * n2 * sizeof(double2),
                               hipMemcpyHostToDevice, ctx->stream));
  return DWH_OK;
}

// states per batched eigensolve of a _deltas / batched call: groups whose
// three n2 x n2 work matrices fit in 16 GiB
int tr_group(const dwh_ctx* ctx, int64_t n) {
  const int N = ctx->d.N;
  const double per = 3.0 * 16.0 * 4.0 * N * (double)N;
  return std::max(1, (int)std::min<int64_t>(n, (int64_t)(16.0 * (1 << 30) / per)));
}

// LDOS(i, ω) and A(k, ω) (dwhmc_spectral.hip) of the m states of src on the
// window first + q stride, q < count, of the DOS grid: one eigensolve, the
// DFT of every column (akw), then per chunk of kSpChunk frequencies one
// Lorentzian table shared by both maps and one product per map, copied out
// chunk by chunk.  ldos / akw: host, N x count per state (either nullable).
// The product: |X|² written out (k_sp_sqmod) and gemm_d (unset or
// DWHMC_SPECTRAL_FUSED=0), or the fused k_sp_maps (=1), which the in-process
// A/B at L = 32 found slower (profiles/spectral_maps_L32.txt).
int spectral_run(dwh_ctx* ctx, const TrSrc& src, int m, double eta, double domega, double omega_max, int64_t first,
                 int64_t count, int64_t stride, double* ldos, double* akw) {
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), m)))
    return rc;
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, sLam = (int64_t)n2 * kSpChunk, sTile = (int64_t)N * kSpChunk, sOut = 2 * sTile;
  if (m > ctx->sp_slots) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    drop_alloc(ctx, ctx->d_sp_lam);
    drop_alloc(ctx, ctx->d_sp_out);
    ctx->d_sp_lam = ctx->d_sp_out = nullptr;
    ctx->sp_slots = 0;
    if ((rc = dalloc(ctx, &ctx->d_sp_lam, (size_t)m * sLam)) || (rc = dalloc(ctx, &ctx->d_sp_out, (size_t)m * sOut)))
      return rc;
    ctx->sp_slots = m;
  }
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  const char* fe = std::getenv("DWHMC_SPECTRAL_FUSED");
  const bool fused = fe && *fe == '1';
  const dwh::TrBufs& b = ctx->tr;
  hipStream_t s = ctx->stream;
  const int nmaps = (ldos ? 1 : 0) + (akw ? 1 : 0);
  // X (the DFT'd columns, N x n2, ld N) in the slots' Jmn, its x pass through
  // JU; unfused: |U|² and |X|² (N x n2 doubles each) then share the slots' JU
  double2* X = b.Jmn;
  double* W = reinterpret_cast<double*>(b.JU);
  const int64_t sW = 2 * sA, oWk = (int64_t)N * n2;
  {
    Scope sc(ctx, T_SPECTRAL, 0.0);
    if (akw) dwh::launch_sp_dft(b.U, sA, (int)ctx->model->Lx, (int)ctx->model->Ly, b.JU, sA, X, sA, m, s);
    if (!fused) {
      if (ldos) dwh::launch_sp_sqmod(b.U, n2, sA, N, n2, W, sW, m, s);
      if (akw) dwh::launch_sp_sqmod(X, N, sA, N, n2, W + oWk, sW, m, s);
    }
    HIPCHECK(ctx, hipGetLastError());
  }
  for (int64_t q0 = 0; q0 < count; q0 += kSpChunk) {
    const int cnt = (int)std::min<int64_t>(kSpChunk, count - q0);
    {
      Scope sc(ctx, T_SPECTRAL, 2.0 * N * (double)n2 * cnt * nmaps * m);
      dwh::launch_sp_lorentz(b.E, n2, eta, -omega_max, domega, first + q0 * stride, stride, cnt, ctx->d_sp_lam,
                             kSpChunk, sLam, m, s);
      if (fused) {
        if (ldos)
          dwh::launch_sp_maps(b.U, n2, sA, ctx->d_sp_lam, kSpChunk, sLam, N, cnt, n2, 1.0, ctx->d_sp_out, N, sOut, m, s);
        if (akw)
          dwh::launch_sp_maps(X, N, sA, ctx->d_sp_lam, kSpChunk, sLam, N, cnt, n2, 1.0 / N, ctx->d_sp_out + sTile, N,
                              sOut, m, s);
      } else {
        if (ldos)
          dwh::gemm_d('N', 'T', N, cnt, n2, 1.0, W, N, sW, ctx->d_sp_lam, kSpChunk, sLam, 0.0, ctx->d_sp_out, N, sOut,
                      m, s);
        if (akw)
          dwh::gemm_d('N', 'T', N, cnt, n2, 1.0 / N, W + oWk, N, sW, ctx->d_sp_lam, kSpChunk, sLam, 0.0,
                      ctx->d_sp_out + sTile, N, sOut, m, s);
      }
      HIPCHECK(ctx, hipGetLastError());
    }
    const size_t bytes = (size_t)N * cnt * sizeof(double);
    for (int k = 0; k < m; ++k) {
      const size_t dst = (size_t)N * q0 + (size_t)N * count * k;
      if (ldos)
        HIPCHECK(ctx, hipMemcpyAsync(ldos + dst, ctx->d_sp_out + k * sOut, bytes, hipMemcpyDeviceToHost, s));
      if (akw)
        HIPCHECK(ctx, hipMemcpyAsync(akw + dst, ctx->d_sp_out + k * sOut + sTile, bytes, hipMemcpyDeviceToHost, s));
    }
  }
  return eigen_info_check(ctx, m);
}

// ---------------------------------------------------------------------------
// finite-momentum current response (include/dwhmc.h, dwhmc_response.hip)
// ---------------------------------------------------------------------------

// Cap of the matrix workspace of one group of momenta (JU_q and J_nm(q), two
// n2 x n2 matrices per momentum); one momentum's pair is always allowed
constexpr double kRsCapBytes = 2.0 * (1u << 30);
constexpr int kRsMaxGroup = 64;

// The operator of one call on the host: the particle block Jq of direction
// dir at every momentum of the list as one CSR pattern (duplicates summed, as
// build_host_model's x operator) with nnz complex values per momentum, the
// direction's bond neighbours [3][N] and hoppings.
struct RsOp {
  std::vector<int> idx;   // rowptr (N + 1), then nbr (3 N)
  std::vector<int> col;
  std::vector<double2> val;
  double tb[3];
  int nnz = 0;
};

void build_response_op(const HostModel& m, int dir, int64_t nq, const int64_t* q, RsOp* op) {
  const int N = m.N, Lx = (int)m.Lx, Ly = (int)m.Ly;
  // B_x = (nn +x, t, (1,0)), (nnn +x+y, t', (1,1)), (nnn +x-y, t', (1,-1));
  // B_y = (nn +y, t, (0,1)), (nnn +x+y, t', (1,1)), (nnn -x+y, t', (-1,1))
  const int* js[3] = {m.nn.data() + (size_t)(dir == 0 ? 0 : 1) * N, m.nnn.data(),
                      m.nnn.data() + (size_t)(dir == 0 ? 3 : 1) * N};
  const double dx[3] = {dir == 0 ? 1.0 : 0.0, 1.0, dir == 0 ? 1.0 : -1.0};
  const double dy[3] = {dir == 0 ? 0.0 : 1.0, 1.0, dir == 0 ? -1.0 : 1.0};
  op->tb[0] = m.t;
  op->tb[1] = op->tb[2] = m.tp;
  std::vector<std::map<int, int>> rows(N);
  for (int i = 0; i < N; ++i)
    for (int b = 0; b < 3; ++b) {
      rows[i][js[b][i]] = 0;
      rows[js[b][i]][i] = 0;
    }
  op->idx.assign((size_t)4 * N + 1, 0);
  op->col.clear();
  for (int r = 0; r < N; ++r) {
    for (auto& kv : rows[r]) {
      kv.second = (int)op->col.size();
      op->col.push_back(kv.first);
    }
    op->idx[r + 1] = (int)op->col.size();
  }
  for (int b = 0; b < 3; ++b)
    for (int i = 0; i < N; ++i) op->idx[(size_t)N + 1 + (size_t)b * N + i] = js[b][i];
  const int nnz = op->nnz = (int)op->col.size();
  op->val.assign((size_t)nq * nnz, make_double2(0.0, 0.0));
  const double two_pi = 6.28318530717958647692;
  for (int64_t k = 0; k < nq; ++k) {
    const double qx = two_pi * (double)q[2 * k] / Lx, qy = two_pi * (double)q[2 * k + 1] / Ly;
    double2* v = op->val.data() + (size_t)k * nnz;
    for (int i = 0; i < N; ++i) {
      const double x = i % Lx, y = i / Lx;
      for (int b = 0; b < 3; ++b) {
        // i t_b φ_b(i), φ_b(i) = exp(-i q·(r_i + δ_b/2))
        const double a = -(qx * (x + 0.5 * dx[b]) + qy * (y + 0.5 * dy[b]));
        const double2 w = make_double2(-op->tb[b] * std::sin(a), op->tb[b] * std::cos(a));
        const int j = js[b][i];
        double2& p = v[rows[i][j]];
        p.x += w.x;
        p.y += w.y;
        double2& t = v[rows[j][i]];
        t.x -= w.x;
        t.y -= w.y;
      }
    }
  }
}

template <typename T>
int rs_grow(dwh_ctx* ctx, T** p, int64_t* cap, int64_t need) {
  if (need <= *cap) return DWH_OK;
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  drop_alloc(ctx, *p);
  *p = nullptr;
  *cap = 0;
  if (int rc = dalloc(ctx, p, (size_t)need)) return rc;
  *cap = need;
  return DWH_OK;
}

// momenta per group: JU_q and J_nm(q) of a group within kRsCapBytes
// (DWHMC_RESPONSE_GROUP: a smaller group, for tests of the grouping loop)
int rs_group(const dwh_ctx* ctx, int64_t nq) {
  const double n2 = 2.0 * ctx->d.N;
  int g = (int)std::min<double>(kRsMaxGroup, kRsCapBytes / (2.0 * 16.0 * n2 * n2));
  if (const char* e = std::getenv("DWHMC_RESPONSE_GROUP")) g = std::min(g, std::atoi(e));
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, nq));
}

// the call's workspace (capacities in elements) and its operator on the device
int response_prepare(dwh_ctx* ctx, const RsOp& op, int64_t nq, int64_t nl) {
  const int64_t n2 = 2 * (int64_t)ctx->d.N, g = rs_group(ctx, nq);
  int rc;
  if ((rc = rs_grow(ctx, &ctx->d_rs_ws, &ctx->rs_mats, 2 * g * n2 * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_part, &ctx->rs_npart, g * nl * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_out, &ctx->rs_nout, 1 + nq * nl)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_val, &ctx->rs_nval, (int64_t)op.val.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_col, &ctx->rs_ncol, (int64_t)op.col.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_idx, &ctx->rs_nidx, (int64_t)op.idx.size())))
    return rc;
  hipStream_t s = ctx->stream;
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_val, op.val.data(), op.val.size() * sizeof(double2), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_col, op.col.data(), op.col.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_idx, op.idx.data(), op.idx.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  return DWH_OK;
}

// dia_α and Λ_αα(q, iΩ_l) of the m states of src: one batched eigensolve, then
// per state the column statistic, U^H once (the slot's Jmn, so every product
// is 'N','N' as in transport_run), and per group of momenta JU_q, the batched
// product against the shared U^H (stride 0), the pair sums and their
// fixed-order reduction.  Every column of J_nm(q) is computed (no
// particle-hole half sum).  dia: m, lambda: nl x nq per state (host).
int response_run(dwh_ctx* ctx, const TrSrc& src, int m, const RsOp& op, int64_t nq, int64_t nl, double* dia,
                 double* lambda) {
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), m)))
    return rc;
  if ((rc = response_prepare(ctx, op, nq, nl))) return rc;   // (transport_prepare may have released it)
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, nout = 1 + nq * nl;
  const int g = rs_group(ctx, nq);
  hipStream_t s = ctx->stream;
  const int *rowptr = ctx->d_rs_idx, *nbr = ctx->d_rs_idx + N + 1;
  double2 *JU = ctx->d_rs_ws, *Jnm = ctx->d_rs_ws + (int64_t)g * sA;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  std::vector<double> out((size_t)m * nout);
  for (int k = 0; k < m; ++k) {
    Scope sc(ctx, T_RESPONSE, 8.0 * n2 * (double)n2 * n2 * nq);
    const dwh::TrBufs b = tr_slot(ctx, k);
    dwh::launch_rs_colstats(b.U, N, b.E, ctx->beta, op.tb, nbr, b.f, b.g, b.dia, s);
    dwh::launch_rs_sum(b.dia, n2, 1, 1.0 / N, ctx->d_rs_out, s);
    dwh::launch_tr_conj_transpose(b.U, n2, n2, n2, 0, b.Jmn, n2, 0, 1, s);
    for (int64_t q0 = 0; q0 < nq; q0 += g) {
      const int gq = (int)std::min<int64_t>(g, nq - q0);
      dwh::launch_rs_current(b.U, JU, sA, N, rowptr, ctx->d_rs_col, ctx->d_rs_val + q0 * op.nnz, op.nnz, gq, s);
      dwh::gemm_z('N', 'N', n2, n2, n2, one, b.Jmn, n2, 0, JU, n2, sA, zero, Jnm, n2, sA, gq, s);
      dwh::launch_rs_pairs(Jnm, sA, N, b.E, b.f, b.g, ctx->beta, (int)nl, gq, ctx->d_rs_part, s);
      dwh::launch_rs_sum(ctx->d_rs_part, n2, gq * (int)nl, 1.0 / N, ctx->d_rs_out + 1 + q0 * nl, s);
    }
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipMemcpyAsync(out.data() + (size_t)k * nout, ctx->d_rs_out, nout * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
  }
  if ((rc = eigen_info_check(ctx, m))) return rc;   // (synchronises)
  for (int k = 0; k < m; ++k) {
    dia[k] = out[(size_t)k * nout];
    std::copy(out.begin() + (size_t)k * nout + 1, out.begin() + (size_t)(k + 1) * nout, lambda + (size_t)k * nq * nl);
  }
  return DWH_OK;
}

// ---------------------------------------------------------------------------
// response of a one-body operator (include/dwhmc.h, dwhmc_operator.hip)
// ---------------------------------------------------------------------------

// The operators of one call on the host: Ṽ_k = V_k ⊕ (-s_k V_k^T) as one CSR
// pattern with n2 = 2N rows and columns in [0, 2N) — rows < N hold V, row
// N + j holds -s V[i, j] at column N + i — duplicates summed, columns
// ascending inside a row, nz complex values per operator.
struct OpNambu {
  std::vector<int> rowptr, col;
  std::vector<double2> val;
  int nz = 0;
};

// validates the caller's CSR and builds the above; ctx may be NULL (the text
// then goes where dwh_last_error(NULL) reads it)
int build_operator_nambu(dwh_ctx* ctx, int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col,
                         int64_t nnz, const dwh_c128* val, const int32_t* spin_sign, OpNambu* op) {
  if (N < 1 || N > (1 << 24)) return fail(ctx, DWH_ERR_ARG, "operator: N must be in [1, 2^24]");
  if (nops < 1 || nnz < 1) return fail(ctx, DWH_ERR_ARG, "operator: nops and nnz must be >= 1");
  if (nops > (1 << 16) || nnz > (1 << 28) || nops * nnz > (1ll << 29))
    return fail(ctx, DWH_ERR_ARG, "operator: more than 2^16 operators or 2^28 entries (2^29 values)");
  if (!rowptr || !col || !val || !spin_sign)
    return fail(ctx, DWH_ERR_ARG, "NULL argument (rowptr, col, val or spin_sign)");
  if (rowptr[0] != 0 || rowptr[N] != nnz)
    return fail(ctx, DWH_ERR_ARG, "operator: rowptr must start at 0 and end at nnz");
  for (int64_t r = 0; r < N; ++r)
    if (rowptr[r + 1] < rowptr[r]) return fail(ctx, DWH_ERR_ARG, "operator: rowptr decreases at row " + std::to_string(r));
  for (int64_t e = 0; e < nnz; ++e)
    if (col[e] < 0 || col[e] >= N)
      return fail(ctx, DWH_ERR_ARG, "operator: column " + std::to_string(col[e]) + " outside [0, N)");
  for (int64_t k = 0; k < nops; ++k)
    if (spin_sign[k] != 1 && spin_sign[k] != -1)
      return fail(ctx, DWH_ERR_ARG, "operator: spin_sign must be +1 or -1");
  const int n = (int)N;
  // pattern: per row the distinct columns in ascending order -> slot
  std::vector<std::map<int, int>> rows((size_t)2 * n);
  for (int i = 0; i < n; ++i)
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int j = (int)col[e];
      rows[i][j] = 0;
      rows[(size_t)n + j][n + i] = 0;
    }
  op->rowptr.assign((size_t)2 * n + 1, 0);
  op->col.clear();
  for (int r = 0; r < 2 * n; ++r) {
    for (auto& kv : rows[r]) {
      kv.second = (int)op->col.size();
      op->col.push_back(kv.first);
    }
    op->rowptr[r + 1] = (int)op->col.size();
  }
  const int nz = op->nz = (int)op->col.size();
  op->val.assign((size_t)nops * nz, make_double2(0.0, 0.0));
  for (int64_t k = 0; k < nops; ++k) {
    const dwh_c128* v = val + (size_t)k * nnz;
    double2* o = op->val.data() + (size_t)k * nz;
    const double hs = -(double)spin_sign[k];
    for (int i = 0; i < n; ++i)
      for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int j = (int)col[e];
        double2& p = o[rows[i][j]];
        p.x += v[e].re;
        p.y += v[e].im;
        double2& h = o[rows[(size_t)n + j][n + i]];
        h.x += hs * v[e].re;
        h.y += hs * v[e].im;
      }
  }
  return DWH_OK;
}

// counts and grid of a call, shared by the device entry's checks
int operator_args(dwh_ctx* ctx, int64_t nops, int64_t nl, const double* chi, double eta, double w_start,
                  double w_step, int64_t nw, const double* chi2) {
  if (nl < 0 || nw < 0) return fail(ctx, DWH_ERR_ARG, "n_matsubara and n_w must be >= 0");
  if (nl == 0 && nw == 0) return fail(ctx, DWH_ERR_ARG, "n_matsubara and n_w are both 0");
  if ((nl > 0 && !chi) || (nw > 0 && !chi2)) return fail(ctx, DWH_ERR_ARG, "NULL output (chi or chi2)");
  if (nops > (1 << 16) || nl > (1 << 24) || nw > (1 << 24) || nops * nl > (1 << 24) || nops * nw > (1 << 26))
    return fail(ctx, DWH_ERR_ARG, "more than 2^24 (operator, Matsubara) or 2^26 (operator, frequency) points");
  if (nw > 0) {
    if (!std::isfinite(eta) || !std::isfinite(w_start) || !std::isfinite(w_step))
      return fail(ctx, DWH_ERR_ARG, "eta, w_start and w_step must be finite");
    if (!(eta > 0)) return fail(ctx, DWH_ERR_ARG, "eta must be > 0");
  }
  return DWH_OK;
}

// the call's workspace (capacities in elements) and its operators on the
// device: the buffers of the current response (which uploads its own operator
// on every call) and the χ'' partials
int operator_prepare(dwh_ctx* ctx, const OpNambu& op, int64_t nops, int64_t nl, int64_t nw) {
  const int64_t n2 = 2 * (int64_t)ctx->d.N, g = rs_group(ctx, nops);
  int rc;
  if ((rc = rs_grow(ctx, &ctx->d_rs_ws, &ctx->rs_mats, 2 * g * n2 * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_part, &ctx->rs_npart, g * nl * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_op_part, &ctx->op_npart, g * dwh::op_spec_chunks(ctx->d.N) * nw)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_out, &ctx->rs_nout, nops * (nl + nw))) ||
      (rc = rs_grow(ctx, &ctx->d_rs_val, &ctx->rs_nval, (int64_t)op.val.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_col, &ctx->rs_ncol, (int64_t)op.col.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_idx, &ctx->rs_nidx, (int64_t)op.rowptr.size())))
    return rc;
  hipStream_t s = ctx->stream;
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_val, op.val.data(), op.val.size() * sizeof(double2), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_col, op.col.data(), op.col.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_idx, op.rowptr.data(), op.rowptr.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  return DWH_OK;
}

// χ(l) and χ''(ω_j) of the nops operators at the m states of src: one batched
// eigensolve, then per state f_n and U^H once (the slot's Jmn, as
// response_run) and per group of operators Ṽ U, the batched product against
// the shared U^H (stride 0), the Matsubara pair sums with their fixed-order
// reduction and the χ'' kernels.  chi: nl x nops, chi2: nw x nops per state (host).
int operator_run(dwh_ctx* ctx, const TrSrc& src, int m, const OpNambu& op, int64_t nops, int64_t nl, double eta,
                 double w_start, double w_step, int64_t nw, double* chi, double* chi2) {
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), m)))
    return rc;
  if ((rc = operator_prepare(ctx, op, nops, nl, nw))) return rc;   // (transport_prepare may have released it)
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, nout = nops * (nl + nw);
  const int g = rs_group(ctx, nops);
  hipStream_t s = ctx->stream;
  double2 *VU = ctx->d_rs_ws, *Vnm = ctx->d_rs_ws + (int64_t)g * sA;
  double *d_chi = ctx->d_rs_out, *d_chi2 = ctx->d_rs_out + nops * nl;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  std::vector<double> out((size_t)m * nout);
  for (int k = 0; k < m; ++k) {
    Scope sc(ctx, T_OPERATOR, 8.0 * n2 * (double)n2 * n2 * nops);
    const dwh::TrBufs b = tr_slot(ctx, k);
    dwh::launch_op_fermi(b.E, N, ctx->beta, b.f, b.g, s);
    dwh::launch_tr_conj_transpose(b.U, n2, n2, n2, 0, b.Jmn, n2, 0, 1, s);
    for (int64_t k0 = 0; k0 < nops; k0 += g) {
      const int gk = (int)std::min<int64_t>(g, nops - k0);
      dwh::launch_op_apply(b.U, VU, sA, N, ctx->d_rs_idx, ctx->d_rs_col, ctx->d_rs_val + k0 * op.nz, op.nz, gk, s);
      dwh::gemm_z('N', 'N', n2, n2, n2, one, b.Jmn, n2, 0, VU, n2, sA, zero, Vnm, n2, sA, gk, s);
      if (nl > 0) {
        dwh::launch_rs_pairs(Vnm, sA, N, b.E, b.f, b.g, ctx->beta, (int)nl, gk, ctx->d_rs_part, s);
        dwh::launch_rs_sum(ctx->d_rs_part, n2, gk * (int)nl, 1.0 / N, d_chi + k0 * nl, s);
      }
      if (nw > 0)
        dwh::launch_op_spec(Vnm, sA, N, b.E, b.f, b.g, ctx->beta, eta, w_start, w_step, (int)nw, gk, ctx->d_op_part,
                            d_chi2 + k0 * nw, s);
    }
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipMemcpyAsync(out.data() + (size_t)k * nout, ctx->d_rs_out, nout * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
  }
  if ((rc = eigen_info_check(ctx, m))) return rc;   // (synchronises)
  for (int k = 0; k < m; ++k) {
    const double* o = out.data() + (size_t)k * nout;
    if (nl > 0) std::copy(o, o + nops * nl, chi + (size_t)k * nops * nl);
    if (nw > 0) std::copy(o + nops * nl, o + nout, chi2 + (size_t)k * nops * nw);
  }
  return DWH_OK;
}

// ---------------------------------------------------------------------------
// cross response of general Nambu vertices (include/dwhmc.h, dwhmc_nambu.hip)
// ---------------------------------------------------------------------------

// Cap of the resident X^k = U^H W_k U of one call (16 vertices at L = 32)
constexpr int64_t kNbCapBytes = 1ll << 30;
// most pairs of a call (blockIdx.y of k_nb_pairs)
constexpr int64_t kNbMaxPairs = 65535;
// pairs per chi2 launch: bounds the partials (pairs x 2 x column chunks x n_w doubles)
constexpr int kNbPairBatch = 4 * dwh::kNbSpecGroup;

// validates the caller's 2N-row CSR and pair list and builds the vertices as
// build_operator_nambu does (one pattern, duplicates summed, columns ascending
// inside a row); ctx may be NULL
int build_nambu_vertices(dwh_ctx* ctx, int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col,
                         int64_t nnz, const dwh_c128* val, int64_t npairs, const int64_t* pairs, OpNambu* op) {
  if (N < 1 || N > (1 << 24)) return fail(ctx, DWH_ERR_ARG, "nambu: N must be in [1, 2^24]");
  if (nops < 1 || nnz < 1) return fail(ctx, DWH_ERR_ARG, "nambu: nops and nnz must be >= 1");
  if (nops > (1 << 16) || nnz > (1 << 28) || nops * nnz > (1ll << 29))
    return fail(ctx, DWH_ERR_ARG, "nambu: more than 2^16 vertices or 2^28 entries (2^29 values)");
  if (npairs < 1 || npairs > kNbMaxPairs) return fail(ctx, DWH_ERR_ARG, "nambu: npairs must be in [1, 65535]");
  if (!rowptr || !col || !val || !pairs)
    return fail(ctx, DWH_ERR_ARG, "NULL argument (rowptr, col, val or pairs)");
  const int64_t n2 = 2 * N;
  if (rowptr[0] != 0 || rowptr[n2] != nnz)
    return fail(ctx, DWH_ERR_ARG, "nambu: rowptr must start at 0 and end at nnz");
  for (int64_t r = 0; r < n2; ++r)
    if (rowptr[r + 1] < rowptr[r]) return fail(ctx, DWH_ERR_ARG, "nambu: rowptr decreases at row " + std::to_string(r));
  for (int64_t e = 0; e < nnz; ++e)
    if (col[e] < 0 || col[e] >= n2)
      return fail(ctx, DWH_ERR_ARG, "nambu: column " + std::to_string(col[e]) + " outside [0, 2N)");
  for (int64_t k = 0; k < 2 * npairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= nops)
      return fail(ctx, DWH_ERR_ARG, "nambu: pair index " + std::to_string(pairs[k]) + " outside [0, nops)");
  if ((double)nops * (double)n2 * (double)n2 * 16.0 > (double)kNbCapBytes)
    return fail(ctx, DWH_ERR_ARG, "nambu: " + std::to_string(nops) + " resident 2N x 2N matrices exceed 1 GiB");
  std::vector<std::map<int, int>> rows((size_t)n2);
  for (int64_t r = 0; r < n2; ++r)
    for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) rows[r][(int)col[e]] = 0;
  op->rowptr.assign((size_t)n2 + 1, 0);
  op->col.clear();
  for (int64_t r = 0; r < n2; ++r) {
    for (auto& kv : rows[r]) {
      kv.second = (int)op->col.size();
      op->col.push_back(kv.first);
    }
    op->rowptr[r + 1] = (int)op->col.size();
  }
  const int nz = op->nz = (int)op->col.size();
  op->val.assign((size_t)nops * nz, make_double2(0.0, 0.0));
  for (int64_t k = 0; k < nops; ++k) {
    const dwh_c128* v = val + (size_t)k * nnz;
    double2* o = op->val.data() + (size_t)k * nz;
    for (int64_t r = 0; r < n2; ++r)
      for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
        double2& p = o[rows[r][(int)col[e]]];
        p.x += v[e].re;
        p.y += v[e].im;
      }
  }
  return DWH_OK;
}

// the call's workspace (capacities in elements), its vertices and pairs on the
// device: the buffers of the operator response (W U of one group only), the
// resident X, the chi2 partials of one batch of pairs and the pair list
int nambu_prepare(dwh_ctx* ctx, const OpNambu& op, int64_t nops, const std::vector<int>& pairs, int64_t nl,
                  int64_t nw) {
  const int64_t n2 = 2 * (int64_t)ctx->d.N, g = rs_group(ctx, nops), np = (int64_t)pairs.size() / 2;
  const int64_t nb = std::min<int64_t>(np, kNbPairBatch);
  int rc;
  if ((rc = rs_grow(ctx, &ctx->d_rs_ws, &ctx->rs_mats, g * n2 * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_nb_x, &ctx->nb_nx, nops * n2 * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_part, &ctx->rs_npart, 2 * np * nl * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_nb_part, &ctx->nb_npart, 2 * nb * dwh::op_spec_chunks(ctx->d.N) * nw)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_out, &ctx->rs_nout, 2 * np * (nl + nw))) ||
      (rc = rs_grow(ctx, &ctx->d_nb_pairs, &ctx->nb_npairs, 2 * np)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_val, &ctx->rs_nval, (int64_t)op.val.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_col, &ctx->rs_ncol, (int64_t)op.col.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_idx, &ctx->rs_nidx, (int64_t)op.rowptr.size())))
    return rc;
  hipStream_t s = ctx->stream;
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_val, op.val.data(), op.val.size() * sizeof(double2), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_col, op.col.data(), op.col.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_idx, op.rowptr.data(), op.rowptr.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_nb_pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  return DWH_OK;
}

// chi[p, l] and chi2[p, j] of the pairs at the m states of src: one batched
// eigensolve, then per state f_n, U^H once (the slot's Jmn) and per group of
// vertices W U and the batched product into the resident X; the Matsubara
// pair sums of all pairs with their fixed-order reduction, and the chi2
// kernels per batch of pairs.  chi: nl x npairs, chi2: nw x npairs complex per
// state (host).
int nambu_run(dwh_ctx* ctx, const TrSrc& src, int m, const OpNambu& op, int64_t nops, const std::vector<int>& pairs,
              int64_t nl, double eta, double w_start, double w_step, int64_t nw, dwh_c128* chi, dwh_c128* chi2) {
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), m)))
    return rc;
  if ((rc = nambu_prepare(ctx, op, nops, pairs, nl, nw))) return rc;   // (transport_prepare may have released it)
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  const int N = ctx->d.N, n2 = 2 * N, np = (int)(pairs.size() / 2);
  const int64_t sA = (int64_t)n2 * n2, nout = 2 * (int64_t)np * (nl + nw);
  const int g = rs_group(ctx, nops);
  hipStream_t s = ctx->stream;
  double2 *WU = ctx->d_rs_ws, *X = ctx->d_nb_x;
  double *d_chi = ctx->d_rs_out, *d_chi2 = ctx->d_rs_out + 2 * np * nl;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  std::vector<double> out((size_t)m * nout);
  for (int k = 0; k < m; ++k) {
    Scope sc(ctx, T_NAMBU, 8.0 * n2 * (double)n2 * n2 * nops);
    const dwh::TrBufs b = tr_slot(ctx, k);
    dwh::launch_op_fermi(b.E, N, ctx->beta, b.f, b.g, s);
    dwh::launch_tr_conj_transpose(b.U, n2, n2, n2, 0, b.Jmn, n2, 0, 1, s);
    for (int64_t k0 = 0; k0 < nops; k0 += g) {
      const int gk = (int)std::min<int64_t>(g, nops - k0);
      dwh::launch_op_apply(b.U, WU, sA, N, ctx->d_rs_idx, ctx->d_rs_col, ctx->d_rs_val + k0 * op.nz, op.nz, gk, s);
      dwh::gemm_z('N', 'N', n2, n2, n2, one, b.Jmn, n2, 0, WU, n2, sA, zero, X + k0 * sA, n2, sA, gk, s);
    }
    if (nl > 0) {
      dwh::launch_nb_pairs(X, sA, N, ctx->d_nb_pairs, np, b.E, b.f, b.g, ctx->beta, (int)nl, ctx->d_rs_part, s);
      dwh::launch_rs_sum(ctx->d_rs_part, n2, 2 * np * (int)nl, 1.0 / N, d_chi, s);
    }
    if (nw > 0)
      for (int p0 = 0; p0 < np; p0 += kNbPairBatch)
        dwh::launch_nb_spec(X, sA, N, ctx->d_nb_pairs, p0, std::min(kNbPairBatch, np - p0), b.E, b.f, b.g, ctx->beta,
                            eta, w_start, w_step, (int)nw, ctx->d_nb_part, d_chi2, s);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipMemcpyAsync(out.data() + (size_t)k * nout, ctx->d_rs_out, nout * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
  }
  if ((rc = eigen_info_check(ctx, m))) return rc;   // (synchronises)
  for (int k = 0; k < m; ++k) {
    const dwh_c128* o = reinterpret_cast<const dwh_c128*>(out.data() + (size_t)k * nout);
    if (nl > 0) std::copy(o, o + np * nl, chi + (size_t)k * np * nl);
    if (nw > 0) std::copy(o + np * nl, o + np * (nl + nw), chi2 + (size_t)k * np * nw);
  }
  return DWH_OK;
}

}  // namespace

extern "C" {

int dwh_transport_grid(double eta, double domega, double omega_max, int64_t* n_omega, int64_t* n_dos) {
  if (!n_omega || !n_dos) return fail(nullptr, DWH_ERR_ARG, "NULL argument");
  if (!(eta > 0) || !(domega > 0) || !(omega_max > 0) || !std::isfinite(eta + domega + omega_max))
    return fail(nullptr, DWH_ERR_ARG, "eta, domega, omega_max must be finite and > 0");
  *n_omega = julia_range_len(eta, domega, omega_max);
  *n_dos = julia_range_len(-omega_max, domega, omega_max);
  if (*n_omega > (1 << 24) || *n_dos > (1 << 24))
    return fail(nullptr, DWH_ERR_ARG, "frequency grid longer than 2^24 points");
  return DWH_OK;
}

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

int dwh_measure_transport(dwh_ctx* ctx, int64_t chain, double eta, double domega, double omega_max,
                          double* stiffness, double* dc_cond, double* sigma, int64_t n_omega,
                          double* dos, double* dos_an, int64_t n_dos, double* ak0) {
  if (!ctx || !stiffness || !dc_cond || !ak0) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  int64_t nw = 0, nd = 0;
  int rc;
  if ((rc = transport_args(ctx, eta, domega, omega_max, n_omega, n_dos, &nw, &nd))) return rc;
  if ((nw > 0 && !sigma) || (nd > 0 && (!dos || !dos_an))) return fail(ctx, DWH_ERR_ARG, "NULL grid output");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  return transport_run(ctx, chains_src(ctx, chain), 1, eta, domega, omega_max, nw, nd, stiffness, dc_cond, sigma, dos, dos_an,
                       ak0);
}

int dwh_measure_transport_batched(dwh_ctx* ctx, double eta, double domega, double omega_max,
                                  double* stiffness, double* dc_cond, double* sigma, int64_t n_omega,
                                  double* dos, double* dos_an, int64_t n_dos, double* ak0) {
  if (!ctx || !stiffness || !dc_cond || !ak0) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  int64_t nw = 0, nd = 0;
  int rc;
  if ((rc = transport_args(ctx, eta, domega, omega_max, n_omega, n_dos, &nw, &nd))) return rc;
  if ((nw > 0 && !sigma) || (nd > 0 && (!dos || !dos_an))) return fail(ctx, DWH_ERR_ARG, "NULL grid output");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  // chains in groups whose three n2 x n2 work matrices fit in 16 GiB
  const int N = ctx->d.N, nc = ctx->d.nc;
  const double per = 3.0 * 16.0 * 4.0 * N * (double)N;
  const int group = std::max(1, std::min(nc, (int)(16.0 * (1 << 30) / per)));
  for (int c0 = 0; c0 < nc; c0 += group) {
    const int m = std::min(group, nc - c0);
    if ((rc = transport_run(ctx, chains_src(ctx, c0), m, eta, domega, omega_max, nw, nd, stiffness + c0, dc_cond + c0,
                            sigma ? sigma + (size_t)c0 * nw : nullptr, dos ? dos + (size_t)c0 * nd : nullptr,
                            dos_an ? dos_an + (size_t)c0 * nd : nullptr, ak0 + (size_t)c0 * N)))
      return rc;
  }
  return DWH_OK;
}

int dwh_measure_transport_deltas(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                 double eta, double domega, double omega_max, double* stiffness,
                                 double* dc_cond, double* sigma, int64_t n_omega, double* dos, double* dos_an,
                                 int64_t n_dos, double* ak0) {
  if (!ctx || !Delta || !stiffness || !dc_cond || !ak0) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  if (nstates < 1) return fail(ctx, DWH_ERR_ARG, "nstates must be >= 1");
  int64_t nw = 0, nd = 0;
  int rc;
  if ((rc = transport_args(ctx, eta, domega, omega_max, n_omega, n_dos, &nw, &nd))) return rc;
  if ((nw > 0 && !sigma) || (nd > 0 && (!dos || !dos_an))) return fail(ctx, DWH_ERR_ARG, "NULL grid output");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int N = ctx->d.N;
  const int64_t n2 = 2 * (int64_t)N;
  if ((rc = stage_deltas(ctx, nstates, Delta))) return rc;
  // groups whose three n2 x n2 work matrices fit in 16 GiB, as the batched call
  const int group = tr_group(ctx, nstates);
  for (int64_t s0 = 0; s0 < nstates; s0 += group) {
    const int m = (int)std::min<int64_t>(group, nstates - s0);
    const TrSrc src{ctx->d_tr_stage + s0 * n2, n2, chain, 0};
    if ((rc = transport_run(ctx, src, m, eta, domega, omega_max, nw, nd, stiffness + s0, dc_cond + s0,
                            sigma ? sigma + (size_t)s0 * nw : nullptr, dos ? dos + (size_t)s0 * nd : nullptr,
                            dos_an ? dos_an + (size_t)s0 * nd : nullptr, ak0 + (size_t)s0 * N)))
      return rc;
  }
  return DWH_OK;
}

int dwh_spectral_window(double eta, double domega, double omega_max, int64_t first, int64_t count, int64_t stride,
                        double* omega) {
#pragma clang fp contract(off)   // start + k·Δω rounded twice, as the device's grid_point
  int64_t nw = 0, nd = 0;
  if (int rc = dwh_transport_grid(eta, domega, omega_max, &nw, &nd)) return rc;
  if (count < 1 || stride < 1) return fail(nullptr, DWH_ERR_ARG, "spectral window: count and stride must be >= 1");
  if (first < 0 || first >= nd || count - 1 > (nd - 1 - first) / stride)
    return fail(nullptr, DWH_ERR_ARG, "spectral window leaves the DOS grid of " + std::to_string(nd) + " points");
  if (omega)
    for (int64_t q = 0; q < count; ++q) {
      const double step = domega * (double)(first + q * stride);
      omega[q] = -omega_max + step;
    }
  return DWH_OK;
}

int dwh_measure_spectral_maps(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta, double eta,
                              double domega, double omega_max, int64_t first, int64_t count, int64_t stride,
                              double* ldos, double* akw) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  if (!ldos && !akw) return fail(ctx, DWH_ERR_ARG, "ldos and akw are both NULL");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  if (nstates < 1) return fail(ctx, DWH_ERR_ARG, "nstates must be >= 1");
  if (!Delta && nstates != 1) return fail(ctx, DWH_ERR_ARG, "nstates must be 1 at the device Delta (Delta == NULL)");
  if (dwh_spectral_window(eta, domega, omega_max, first, count, stride, nullptr) != DWH_OK)
    return fail(ctx, DWH_ERR_ARG, g_create_error);
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int N = ctx->d.N;
  const int64_t n2 = 2 * (int64_t)N;
  if (!Delta)
    return spectral_run(ctx, chains_src(ctx, chain), 1, eta, domega, omega_max, first, count, stride, ldos, akw);
  int rc;
  if ((rc = stage_deltas(ctx, nstates, Delta))) return rc;
  const int group = tr_group(ctx, nstates);   // as dwh_measure_transport_deltas
  for (int64_t s0 = 0; s0 < nstates; s0 += group) {
    const int m = (int)std::min<int64_t>(group, nstates - s0);
    const TrSrc src{ctx->d_tr_stage + s0 * n2, n2, chain, 0};
    const size_t off = (size_t)N * count * s0;
    if ((rc = spectral_run(ctx, src, m, eta, domega, omega_max, first, count, stride, ldos ? ldos + off : nullptr,
                           akw ? akw + off : nullptr)))
      return rc;
  }
  return DWH_OK;
}

int dwh_measure_current_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                 int32_t direction, int64_t nq, const int64_t* q, int64_t n_matsubara, double* dia,
                                 double* lambda) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  if (!q || !dia || !lambda) return fail(ctx, DWH_ERR_ARG, "NULL argument (q, dia or lambda)");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  if (nstates < 1) return fail(ctx, DWH_ERR_ARG, "nstates must be >= 1");
  if (!Delta && nstates != 1) return fail(ctx, DWH_ERR_ARG, "nstates must be 1 at the device Delta (Delta == NULL)");
  if (direction != 0 && direction != 1) return fail(ctx, DWH_ERR_ARG, "direction must be 0 (x) or 1 (y)");
  if (nq < 1) return fail(ctx, DWH_ERR_ARG, "nq must be >= 1");
  if (n_matsubara < 1) return fail(ctx, DWH_ERR_ARG, "n_matsubara must be >= 1");
  if (nq > (1 << 24) || n_matsubara > (1 << 24) || nq * n_matsubara > (1 << 24))
    return fail(ctx, DWH_ERR_ARG, "more than 2^24 (momentum, frequency) points");
  const HostModel& model = *ctx->model;
  for (int64_t k = 0; k < nq; ++k)
    if (std::llabs(q[2 * k]) > model.Lx || std::llabs(q[2 * k + 1]) > model.Ly)
      return fail(ctx, DWH_ERR_ARG, "momentum index outside |mx| <= Lx, |my| <= Ly");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  RsOp op;
  build_response_op(model, direction, nq, q, &op);
  if (!Delta) return response_run(ctx, chains_src(ctx, chain), 1, op, nq, n_matsubara, dia, lambda);
  int rc;
  if ((rc = stage_deltas(ctx, nstates, Delta))) return rc;
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  const int group = tr_group(ctx, nstates);   // as dwh_measure_transport_deltas
  for (int64_t s0 = 0; s0 < nstates; s0 += group) {
    const int m = (int)std::min<int64_t>(group, nstates - s0);
    const TrSrc src{ctx->d_tr_stage + s0 * n2, n2, chain, 0};
    if ((rc = response_run(ctx, src, m, op, nq, n_matsubara, dia + s0, lambda + (size_t)s0 * nq * n_matsubara)))
      return rc;
  }
  return DWH_OK;
}

int dwh_measure_operator_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                  int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                                  const dwh_c128* val, const int32_t* spin_sign, int64_t n_matsubara, double* chi,
                                  double eta, double w_start, double w_step, int64_t n_w, double* chi2) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  if (nstates < 1) return fail(ctx, DWH_ERR_ARG, "nstates must be >= 1");
  if (!Delta && nstates != 1) return fail(ctx, DWH_ERR_ARG, "nstates must be 1 at the device Delta (Delta == NULL)");
  int rc;
  OpNambu op;
  if (nops < 1 || nnz < 1) return fail(ctx, DWH_ERR_ARG, "operator: nops and nnz must be >= 1");
  if ((rc = operator_args(ctx, nops, n_matsubara, chi, eta, w_start, w_step, n_w, chi2))) return rc;
  if ((rc = build_operator_nambu(ctx, ctx->d.N, nops, rowptr, col, nnz, val, spin_sign, &op))) return rc;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  if (!Delta)
    return operator_run(ctx, chains_src(ctx, chain), 1, op, nops, n_matsubara, eta, w_start, w_step, n_w, chi, chi2);
  if ((rc = stage_deltas(ctx, nstates, Delta))) return rc;
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  const int group = tr_group(ctx, nstates);   // as dwh_measure_transport_deltas
  for (int64_t s0 = 0; s0 < nstates; s0 += group) {
    const int m = (int)std::min<int64_t>(group, nstates - s0);
    const TrSrc src{ctx->d_tr_stage + s0 * n2, n2, chain, 0};
    if ((rc = operator_run(ctx, src, m, op, nops, n_matsubara, eta, w_start, w_step, n_w,
                           chi ? chi + (size_t)s0 * nops * n_matsubara : nullptr,
                           chi2 ? chi2 + (size_t)s0 * nops * n_w : nullptr)))
      return rc;
  }
  return DWH_OK;
}

int dwh_debug_operator_nambu(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                             const dwh_c128* val, const int32_t* spin_sign, dwh_c128* out) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "NULL argument (out)");
  OpNambu op;
  if (int rc = build_operator_nambu(nullptr, N, nops, rowptr, col, nnz, val, spin_sign, &op)) return rc;
  const size_t n2 = 2 * (size_t)N;
  std::fill(out, out + (size_t)nops * n2 * n2, dwh_c128{0.0, 0.0});
  for (int64_t k = 0; k < nops; ++k)
    for (size_t r = 0; r < n2; ++r)
      for (int e = op.rowptr[r]; e < op.rowptr[r + 1]; ++e) {
        const double2 v = op.val[(size_t)k * op.nz + e];
        out[(size_t)k * n2 * n2 + r + (size_t)op.col[e] * n2] = dwh_c128{v.x, v.y};
      }
  return DWH_OK;
}

int dwh_measure_nambu_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta, int64_t nops,
                               const int64_t* rowptr, const int64_t* col, int64_t nnz, const dwh_c128* val,
                               int64_t npairs, const int64_t* pairs, int64_t n_matsubara, dwh_c128* chi, double eta,
                               double w_start, double w_step, int64_t n_w, dwh_c128* chi2) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  if (nstates < 1) return fail(ctx, DWH_ERR_ARG, "nstates must be >= 1");
  if (!Delta && nstates != 1) return fail(ctx, DWH_ERR_ARG, "nstates must be 1 at the device Delta (Delta == NULL)");
  int rc;
  OpNambu op;
  // (the vertex and pair checks first: they bound npairs for the count checks)
  if ((rc = build_nambu_vertices(ctx, ctx->d.N, nops, rowptr, col, nnz, val, npairs, pairs, &op))) return rc;
  if ((rc = operator_args(ctx, npairs, n_matsubara, reinterpret_cast<const double*>(chi), eta, w_start, w_step, n_w,
                          reinterpret_cast<const double*>(chi2))))
    return rc;
  std::vector<int> pr(pairs, pairs + 2 * npairs);
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  if (!Delta)
    return nambu_run(ctx, chains_src(ctx, chain), 1, op, nops, pr, n_matsubara, eta, w_start, w_step, n_w, chi, chi2);
  if ((rc = stage_deltas(ctx, nstates, Delta))) return rc;
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  const int group = tr_group(ctx, nstates);   // as dwh_measure_transport_deltas
  for (int64_t s0 = 0; s0 < nstates; s0 += group) {
    const int m = (int)std::min<int64_t>(group, nstates - s0);
    const TrSrc src{ctx->d_tr_stage + s0 * n2, n2, chain, 0};
    if ((rc = nambu_run(ctx, src, m, op, nops, pr, n_matsubara, eta, w_start, w_step, n_w,
                        chi ? chi + (size_t)s0 * npairs * n_matsubara : nullptr,
                        chi2 ? chi2 + (size_t)s0 * npairs * n_w : nullptr)))
      return rc;
  }
  return DWH_OK;
}

int dwh_debug_nambu_dense(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                          const dwh_c128* val, int64_t npairs, const int64_t* pairs, dwh_c128* out) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "NULL argument (out)");
  OpNambu op;
  if (int rc = build_nambu_vertices(nullptr, N, nops, rowptr, col, nnz, val, npairs, pairs, &op)) return rc;
  const size_t n2 = 2 * (size_t)N;
  std::fill(out, out + (size_t)nops * n2 * n2, dwh_c128{0.0, 0.0});
  for (int64_t k = 0; k < nops; ++k)
    for (size_t r = 0; r < n2; ++r)
      for (int e = op.rowptr[r]; e < op.rowptr[r + 1]; ++e) {
        const double2 v = op.val[(size_t)k * op.nz + e];
        out[(size_t)k * n2 * n2 + r + (size_t)op.col[e] * n2] = dwh_c128{v.x, v.y};
      }
  return DWH_OK;
}

int dwh_bench_response_product(dwh_ctx* ctx, int64_t reps, double* ms) {
  if (!ctx || !ms) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (reps < 1 || reps > 1000) return fail(ctx, DWH_ERR_ARG, "reps must be in [1, 1000]");
  if (ctx->tr_slots < 1) return fail(ctx, DWH_ERR_STATE, "no measurement has run on this context yet");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int n2 = 2 * ctx->d.N;
  const int64_t sA = (int64_t)n2 * n2;
  const dwh::TrBufs& b = ctx->tr;
  hipStream_t s = ctx->stream;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHECK(ctx, hipEventCreate(&e0));
  HIPCHECK(ctx, hipEventCreate(&e1));
  dwh::gemm_z('N', 'N', n2, n2, n2, one, b.Jmn, n2, sA, b.U, n2, sA, zero, b.JU, n2, sA, 1, s);   // warm
  HIPCHECK(ctx, hipEventRecord(e0, s));
  for (int64_t r = 0; r < reps; ++r)
    dwh::gemm_z('N', 'N', n2, n2, n2, one, b.Jmn, n2, sA, b.U, n2, sA, zero, b.JU, n2, sA, 1, s);
  HIPCHECK(ctx, hipEventRecord(e1, s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  HIPCHECK(ctx, hipGetLastError());
  float t = 0.f;
  HIPCHECK(ctx, hipEventElapsedTime(&t, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *ms = (double)t / (double)reps;
  return DWH_OK;
}

}  // extern "C"
