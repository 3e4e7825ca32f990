// Measurement half of the C-ABI context (include/dwhmc.h), on the eigenpairs
// of dwhmc_eigsolve.cpp: transport and spectra (dwhmc_transport.hip), the
// spectral maps (dwhmc_spectral.hip) and the four vertex families — current
// (dwhmc_response.hip), one-body operator (dwhmc_operator.hip), Nambu cross
// response (dwhmc_nambu.hip), response maps (dwhmc_map.hip) — which share one
// host vertex type, one upload and one per-state driver; with their entry points.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
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

// The vertex responses' workspace (vertex_prepare allocates it on first use)
// goes where the slot buffers are reallocated: both scale with n2², so a
// caller that grows the slots gets this memory back first.  With it go what
// the families add: the current response's bond table, the operator
// response's χ'' partials, the Nambu cross response's resident X, chi2
// partials and pair list.
void response_release(dwh_ctx* ctx) {
  for (void* q : {(void*)ctx->d_rs_ws, (void*)ctx->d_rs_val, (void*)ctx->d_rs_part, (void*)ctx->d_rs_out,
                  (void*)ctx->d_rs_col, (void*)ctx->d_rs_idx, (void*)ctx->d_rs_nbr, (void*)ctx->d_op_part,
                  (void*)ctx->d_nb_x, (void*)ctx->d_nb_part, (void*)ctx->d_nb_pairs, (void*)ctx->d_map_ws,
                  (void*)ctx->d_map_out, (void*)ctx->d_map_omega, (void*)ctx->d_map_idx, (void*)ctx->d_map_slice,
                  (void*)ctx->d_cr_idx, (void*)ctx->d_cr_val, (void*)ctx->d_cr_part, (void*)ctx->d_cr_out})
    drop_alloc(ctx, q);
  ctx->d_rs_ws = ctx->d_rs_val = ctx->d_nb_x = nullptr;
  ctx->d_rs_part = ctx->d_rs_out = ctx->d_op_part = ctx->d_nb_part = nullptr;
  ctx->d_rs_col = ctx->d_rs_idx = ctx->d_rs_nbr = ctx->d_nb_pairs = nullptr;
  ctx->rs_mats = ctx->rs_npart = ctx->rs_nout = ctx->rs_nval = ctx->rs_ncol = ctx->rs_nidx = ctx->rs_nnbr = 0;
  ctx->op_npart = ctx->nb_nx = ctx->nb_npart = ctx->nb_npairs = 0;
  ctx->d_map_ws = ctx->d_map_out = nullptr;
  ctx->d_map_omega = nullptr;
  ctx->d_map_idx = ctx->d_map_slice = nullptr;
  ctx->map_nws = ctx->map_nout = ctx->map_nomega = ctx->map_nidx = ctx->map_nslice = 0;
  ctx->map_last_nslices = ctx->map_last_npat = ctx->map_last_chunk = ctx->map_last_x = 0;
  ctx->d_cr_idx = nullptr;
  ctx->d_cr_val = ctx->d_cr_part = ctx->d_cr_out = nullptr;
  ctx->cr_nidx = ctx->cr_nval = ctx->cr_npart = ctx->cr_nout = 0;
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

}  // namespace

// states per batched eigensolve of a _deltas / batched call: groups whose
// three n2 x n2 work matrices fit in 16 GiB
int dwh::tr_group(const dwh_ctx* ctx, int64_t n) {
  const int N = ctx->d.N;
  const double per = 3.0 * 16.0 * 4.0 * N * (double)N;
  return std::max(1, (int)std::min<int64_t>(n, (int64_t)(16.0 * (1 << 30) / per)));
}

namespace {

// the chain / nstates / Delta arguments every state-list entry point takes
int check_state_args(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta) {
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  if (nstates < 1) return fail(ctx, DWH_ERR_ARG, "nstates must be >= 1");
  if (!Delta && nstates != 1) return fail(ctx, DWH_ERR_ARG, "nstates must be 1 at the device Delta (Delta == NULL)");
  return DWH_OK;
}

// fn(src, m, s0) on the states of a call: the chain's own Δ on the device
// (Delta == NULL, one state), else the nstates snapshots staged and taken in
// groups of tr_group (cap > 0: of at most cap), m states from state s0 per call
template <class F>
int for_each_state_group(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta, F&& fn, int cap = 0) {
  if (!Delta) return fn(chains_src(ctx, chain), 1, (int64_t)0);
  if (int rc = stage_deltas(ctx, nstates, Delta)) return rc;
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  const int group = cap > 0 ? std::min(cap, tr_group(ctx, nstates)) : tr_group(ctx, nstates);
  for (int64_t s0 = 0; s0 < nstates; s0 += group) {
    const int m = (int)std::min<int64_t>(group, nstates - s0);
    if (int rc = fn(TrSrc{ctx->d_tr_stage + s0 * n2, n2, chain, 0}, m, s0)) return rc;
  }
  return DWH_OK;
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
// The vertex responses (include/dwhmc.h): the current response Λ(q, iΩ)
// (dwhmc_response.hip), the response of one-body operators (dwhmc_operator.hip)
// the cross response of Nambu vertices (dwhmc_nambu.hip) and the response maps
// on a pattern (dwhmc_map.hip).  Each turns its arguments into a Vertex, and
// vertex_run takes it through the same steps: W_k U, U^H (W_k U), the family's
// reductions.
// ---------------------------------------------------------------------------

// Cap of the matrix workspace of one group of vertices (W_k U and U^H W_k U,
// two n2 x n2 matrices per vertex); one vertex's pair is always allowed
constexpr double kRsCapBytes = 2.0 * (1u << 30);
constexpr int kRsMaxGroup = 64;
// Cap of the resident X^k = U^H W_k U of one Nambu call (16 vertices at L = 32)
constexpr int64_t kNbCapBytes = 1ll << 30;
// most pairs of a Nambu call (blockIdx.y of k_nb_pairs)
constexpr int64_t kNbMaxPairs = 65535;
// pairs per chi2 launch: bounds the partials (pairs x 2 x column chunks x n_w doubles)
constexpr int kNbPairBatch = 4 * dwh::kNbSpecGroup;

// The vertices of one call on the host: 2N x 2N matrices in the Nambu basis on
// one CSR pattern with 2N rows, columns ascending inside a row, duplicates
// summed, nz complex values per vertex at val[k nz + e].
struct Vertex {
  std::vector<int> rowptr, col;
  std::vector<double2> val;
  int nz = 0;
};

// nv vertices of n2 rows from their entries: each(k, emit) calls
// emit(row, col, value) for every entry of vertex k, in the same (row, col)
// sequence for every k.  Entries at one (row, col) are added in that sequence.
template <class Each>
void build_vertex(int n2, int64_t nv, Each&& each, Vertex* v) {
  // pattern: per row the distinct columns in ascending order -> slot
  std::vector<std::map<int, int>> rows((size_t)n2);
  each((int64_t)0, [&](int r, int c, double2) { rows[r][c] = 0; });
  v->rowptr.assign((size_t)n2 + 1, 0);
  v->col.clear();
  for (int r = 0; r < n2; ++r) {
    for (auto& kv : rows[r]) {
      kv.second = (int)v->col.size();
      v->col.push_back(kv.first);
    }
    v->rowptr[r + 1] = (int)v->col.size();
  }
  const int nz = v->nz = (int)v->col.size();
  v->val.assign((size_t)nv * nz, make_double2(0.0, 0.0));
  for (int64_t k = 0; k < nv; ++k) {
    double2* o = v->val.data() + (size_t)k * nz;
    each(k, [&](int r, int c, double2 x) {
      double2& p = o[rows[r][c]];
      p.x += x.x;
      p.y += x.y;
    });
  }
}

// the vertices as dense 2N x 2N column-major matrices (the debug entries)
void densify(const Vertex& v, int64_t N, int64_t nv, dwh_c128* out) {
  const size_t n2 = 2 * (size_t)N;
  std::fill(out, out + (size_t)nv * n2 * n2, dwh_c128{0.0, 0.0});
  for (int64_t k = 0; k < nv; ++k)
    for (size_t r = 0; r < n2; ++r)
      for (int e = v.rowptr[r]; e < v.rowptr[r + 1]; ++e) {
        const double2 x = v.val[(size_t)k * v.nz + e];
        out[(size_t)k * n2 * n2 + r + (size_t)v.col[e] * n2] = dwh_c128{x.x, x.y};
      }
}

// The counts and the CSR of a caller's vertex list with nrows rows and columns
// (N: one-body operators, 2N: Nambu vertices); pre: the family's message
// prefix, noun: what it calls its vertices.  rowptr and col are not NULL.
int check_csr(dwh_ctx* ctx, const std::string& pre, const char* noun, int64_t N, int64_t nrows, int64_t nops,
              const int64_t* rowptr, const int64_t* col, int64_t nnz) {
  if (N < 1 || N > (1 << 24)) return fail(ctx, DWH_ERR_ARG, pre + ": N must be in [1, 2^24]");
  if (nops < 1 || nnz < 1) return fail(ctx, DWH_ERR_ARG, pre + ": nops and nnz must be >= 1");
  if (nops > (1 << 16) || nnz > (1 << 28) || nops * nnz > (1ll << 29))
    return fail(ctx, DWH_ERR_ARG, pre + ": more than 2^16 " + noun + " or 2^28 entries (2^29 values)");
  if (rowptr[0] != 0 || rowptr[nrows] != nnz)
    return fail(ctx, DWH_ERR_ARG, pre + ": rowptr must start at 0 and end at nnz");
  for (int64_t r = 0; r < nrows; ++r)
    if (rowptr[r + 1] < rowptr[r]) return fail(ctx, DWH_ERR_ARG, pre + ": rowptr decreases at row " + std::to_string(r));
  for (int64_t e = 0; e < nnz; ++e)
    if (col[e] < 0 || col[e] >= nrows)
      return fail(ctx, DWH_ERR_ARG, pre + ": column " + std::to_string(col[e]) + " outside [0, " +
                                        (nrows == N ? "N)" : "2N)"));
  return DWH_OK;
}

// The bond list of the current of direction dir: neighbours nbr[3][N],
// hoppings and bond vectors,
//   x: (nn +x, t, (1,0)), (nnn +x+y, t', (1,1)), (nnn +x-y, t', (1,-1))
//   y: (nn +y, t, (0,1)), (nnn +x+y, t', (1,1)), (nnn -x+y, t', (-1,1))
struct CurrentBonds {
  std::vector<int> nbr;
  double tb[3], dx[3], dy[3];
};
CurrentBonds current_bonds(const HostModel& m, int dir) {
  const size_t N = m.N;
  const int* js[3] = {m.nn.data() + (dir == 0 ? 0 : 1) * N, m.nnn.data(), m.nnn.data() + (dir == 0 ? 3 : 1) * N};
  CurrentBonds cb{{}, {m.t, m.tp, m.tp}, {dir == 0 ? 1.0 : 0.0, 1.0, dir == 0 ? 1.0 : -1.0},
                  {dir == 0 ? 0.0 : 1.0, 1.0, dir == 0 ? -1.0 : 1.0}};
  for (int b = 0; b < 3; ++b) cb.nbr.insert(cb.nbr.end(), js[b], js[b] + N);
  return cb;
}

// current response: Jq ⊕ Jq at every momentum of the list (the hole block
// equals the particle block), Jq[i, j_b(i)] += i t_b φ_b(i), Jq[j_b(i), i] -=
// the same, φ_b(i) = exp(-i q·(r_i + δ_b/2)), as build_host_model's x operator
void build_current_vertex(const HostModel& m, const CurrentBonds& cb, int64_t nq, const int64_t* q, Vertex* v) {
  const int N = m.N, Lx = (int)m.Lx, Ly = (int)m.Ly;
  build_vertex(2 * N, nq, [&](int64_t k, auto&& emit) {
    const double qx = kTwoPi * (double)q[2 * k] / Lx, qy = kTwoPi * (double)q[2 * k + 1] / Ly;
    for (int i = 0; i < N; ++i) {
      const double x = i % Lx, y = i / Lx;
      for (int b = 0; b < 3; ++b) {
        const double a = -(qx * (x + 0.5 * cb.dx[b]) + qy * (y + 0.5 * cb.dy[b]));
        const double2 w = make_double2(-cb.tb[b] * std::sin(a), cb.tb[b] * std::cos(a));
        const double2 mw = make_double2(-w.x, -w.y);
        const int j = cb.nbr[(size_t)b * N + i];
        emit(i, j, w);
        emit(j, i, mw);
        emit(N + i, N + j, w);
        emit(N + j, N + i, mw);
      }
    }
  }, v);
}

// direction, counts and momenta of a current-response call; ctx may be NULL
int current_args(dwh_ctx* ctx, const HostModel& model, int32_t direction, int64_t nq, const int64_t* q, int64_t nl) {
  if (direction != 0 && direction != 1) return fail(ctx, DWH_ERR_ARG, "direction must be 0 (x) or 1 (y)");
  if (nq < 1) return fail(ctx, DWH_ERR_ARG, "nq must be >= 1");
  if (nl < 1) return fail(ctx, DWH_ERR_ARG, "n_matsubara must be >= 1");
  if (nq > (1 << 24) || nl > (1 << 24) || nq * nl > (1 << 24))
    return fail(ctx, DWH_ERR_ARG, "more than 2^24 (momentum, frequency) points");
  for (int64_t k = 0; k < nq; ++k)
    if (std::llabs(q[2 * k]) > model.Lx || std::llabs(q[2 * k + 1]) > model.Ly)
      return fail(ctx, DWH_ERR_ARG, "momentum index outside |mx| <= Lx, |my| <= Ly");
  return DWH_OK;
}

// operator response: Ṽ_k = V_k ⊕ (-s_k V_k^T) — rows < N hold V, row N + j
// holds -s V[i, j] at column N + i — from the caller's validated N-row CSR;
// ctx may be NULL (the text then goes where dwh_last_error(NULL) reads it)
int build_operator_nambu(dwh_ctx* ctx, int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col,
                         int64_t nnz, const dwh_c128* val, const int32_t* spin_sign, Vertex* v) {
  if (!rowptr || !col || !val || !spin_sign)
    return fail(ctx, DWH_ERR_ARG, "NULL argument (rowptr, col, val or spin_sign)");
  if (int rc = check_csr(ctx, "operator", "operators", N, N, nops, rowptr, col, nnz)) return rc;
  for (int64_t k = 0; k < nops; ++k)
    if (spin_sign[k] != 1 && spin_sign[k] != -1)
      return fail(ctx, DWH_ERR_ARG, "operator: spin_sign must be +1 or -1");
  const int n = (int)N;
  build_vertex(2 * n, nops, [&](int64_t k, auto&& emit) {
    const dwh_c128* x = val + (size_t)k * nnz;
    const double hs = -(double)spin_sign[k];
    for (int i = 0; i < n; ++i)
      for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int j = (int)col[e];
        emit(i, j, make_double2(x[e].re, x[e].im));
        emit(n + j, n + i, make_double2(hs * x[e].re, hs * x[e].im));
      }
  }, v);
  return DWH_OK;
}

// The caller's 2N-row CSR of Nambu vertices (the cross response's and the
// response maps'), checked; ctx may be NULL
int check_nambu_csr(dwh_ctx* ctx, const std::string& pre, int64_t N, int64_t nops, const int64_t* rowptr,
                    const int64_t* col, int64_t nnz, const dwh_c128* val) {
  if (!rowptr || !col || !val) return fail(ctx, DWH_ERR_ARG, pre + ": NULL argument (rowptr, col or val)");
  return check_csr(ctx, pre, "vertices", N, 2 * N, nops, rowptr, col, nnz);
}

// ... and as given, once checked
void fill_nambu_vertices(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                         const dwh_c128* val, Vertex* v) {
  const int64_t n2 = 2 * N;
  build_vertex((int)n2, nops, [&](int64_t k, auto&& emit) {
    const dwh_c128* x = val + (size_t)k * nnz;
    for (int64_t r = 0; r < n2; ++r)
      for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) emit((int)r, (int)col[e], make_double2(x[e].re, x[e].im));
  }, v);
}

// Nambu cross response: the caller's validated 2N-row CSR as given, and its
// pair list checked; ctx may be NULL
int build_nambu_vertices(dwh_ctx* ctx, int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col,
                         int64_t nnz, const dwh_c128* val, int64_t npairs, const int64_t* pairs, Vertex* v) {
  if (!pairs) return fail(ctx, DWH_ERR_ARG, "nambu: NULL argument (pairs)");
  if (int rc = check_nambu_csr(ctx, "nambu", N, nops, rowptr, col, nnz, val)) return rc;
  if (npairs < 1 || npairs > kNbMaxPairs) return fail(ctx, DWH_ERR_ARG, "nambu: npairs must be in [1, 65535]");
  const int64_t n2 = 2 * N;
  for (int64_t k = 0; k < 2 * npairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= nops)
      return fail(ctx, DWH_ERR_ARG, "nambu: pair index " + std::to_string(pairs[k]) + " outside [0, nops)");
  if ((double)nops * (double)n2 * (double)n2 * 16.0 > (double)kNbCapBytes)
    return fail(ctx, DWH_ERR_ARG, "nambu: " + std::to_string(nops) + " resident 2N x 2N matrices exceed 1 GiB");
  fill_nambu_vertices(N, nops, rowptr, col, nnz, val, v);
  return DWH_OK;
}

// The pattern of a response-map call, npat Nambu index pairs (prow[e],
// pcol[e]), grouped by column: order is the permutation of the entries sorted
// by pcol, stable inside a column; the entries of column b are
// order[colptr[b]] .. order[colptr[b + 1] - 1].  ctx may be NULL.
constexpr int64_t kMapMaxPat = 1 << 24;
struct MapPlan {
  std::vector<int> order, colptr;
};
int map_plan(dwh_ctx* ctx, int64_t N, int64_t npat, const int64_t* prow, const int64_t* pcol, MapPlan* pl) {
  const std::string pre = "response map";
  if (N < 1 || N > (1 << 24)) return fail(ctx, DWH_ERR_ARG, pre + ": N must be in [1, 2^24]");
  if (!prow || !pcol) return fail(ctx, DWH_ERR_ARG, pre + ": NULL argument (prow or pcol)");
  if (npat < 1 || npat > kMapMaxPat) return fail(ctx, DWH_ERR_ARG, pre + ": npat must be in [1, 2^24]");
  const int64_t n2 = 2 * N;
  for (int64_t e = 0; e < npat; ++e)
    if (prow[e] < 0 || prow[e] >= n2 || pcol[e] < 0 || pcol[e] >= n2)
      return fail(ctx, DWH_ERR_ARG, pre + ": pattern entry " + std::to_string(e) + " (" + std::to_string(prow[e]) +
                                        ", " + std::to_string(pcol[e]) + ") outside [0, 2N)");
  pl->colptr.assign((size_t)n2 + 1, 0);
  for (int64_t e = 0; e < npat; ++e) ++pl->colptr[(size_t)pcol[e] + 1];
  for (int64_t b = 0; b < n2; ++b) pl->colptr[b + 1] += pl->colptr[b];
  std::vector<int> next(pl->colptr.begin(), pl->colptr.end() - 1);
  pl->order.resize((size_t)npat);
  for (int64_t e = 0; e < npat; ++e) pl->order[(size_t)next[(size_t)pcol[e]]++] = (int)e;
  return DWH_OK;
}

// counts and frequencies of a response-map call
int map_args(dwh_ctx* ctx, int64_t N, int64_t nops, int64_t nl, double eta, int64_t nw, const double* omega,
             const dwh_c128* rho, const dwh_c128* dmap) {
  const std::string pre = "response map";
  if (!rho && !dmap) return fail(ctx, DWH_ERR_ARG, pre + ": rho and dmap are both NULL");
  if (nl < 0 || nw < 0) return fail(ctx, DWH_ERR_ARG, pre + ": n_matsubara and n_w must be >= 0");
  if (nl > (1 << 16) || nw > (1 << 16) || nops * (nl + nw) > (1 << 20))
    return fail(ctx, DWH_ERR_ARG, pre + ": more than 2^16 frequencies of a kind or 2^20 (vertex, frequency) points");
  if (dmap && nl + nw == 0) return fail(ctx, DWH_ERR_ARG, pre + ": n_matsubara and n_w are both 0 with a dmap output");
  if (2 * N > dwh::kMapMaxN2)
    return fail(ctx, DWH_ERR_ARG, pre + ": 2N above " + std::to_string(dwh::kMapMaxN2) +
                                      " (a staged column of the sampled product exceeds the LDS)");
  if (nw > 0) {
    if (!omega) return fail(ctx, DWH_ERR_ARG, pre + ": NULL omega with n_w > 0");
    if (!std::isfinite(eta)) return fail(ctx, DWH_ERR_ARG, pre + ": eta must be finite");
    if (!(eta > 0)) return fail(ctx, DWH_ERR_ARG, pre + ": eta must be > 0");
    for (int64_t j = 0; j < nw; ++j)
      if (!std::isfinite(omega[j])) return fail(ctx, DWH_ERR_ARG, pre + ": omega must be finite");
  }
  return DWH_OK;
}

// counts and grid of a call, shared by the device entries' checks
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

// vertices per group: W_k U and U^H W_k U of a group within kRsCapBytes
// (DWHMC_RESPONSE_GROUP: a smaller group, for tests of the grouping loop)
int rs_group(const dwh_ctx* ctx, int64_t nq) {
  const double n2 = 2.0 * ctx->d.N;
  int g = (int)std::min<double>(kRsMaxGroup, kRsCapBytes / (2.0 * 16.0 * n2 * n2));
  if (const char* e = std::getenv("DWHMC_RESPONSE_GROUP")) g = std::min(g, std::atoi(e));
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, nq));
}

// the shared workspace of a call (capacities in elements: mats n2 x n2
// matrices, the pair sums, one state's results) and its vertices on the
// device; the uploads are enqueued, not waited for
int vertex_prepare(dwh_ctx* ctx, const Vertex& v, int64_t mats, int64_t npart, int64_t nout) {
  const int64_t n2 = 2 * (int64_t)ctx->d.N;
  int rc;
  if ((rc = rs_grow(ctx, &ctx->d_rs_ws, &ctx->rs_mats, mats * n2 * n2)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_part, &ctx->rs_npart, npart)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_out, &ctx->rs_nout, nout)) ||
      (rc = rs_grow(ctx, &ctx->d_rs_val, &ctx->rs_nval, (int64_t)v.val.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_col, &ctx->rs_ncol, (int64_t)v.col.size())) ||
      (rc = rs_grow(ctx, &ctx->d_rs_idx, &ctx->rs_nidx, (int64_t)v.rowptr.size())))
    return rc;
  hipStream_t s = ctx->stream;
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_val, v.val.data(), v.val.size() * sizeof(double2), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_col, v.col.data(), v.col.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_idx, v.rowptr.data(), v.rowptr.size() * sizeof(int), hipMemcpyHostToDevice, s));
  return DWH_OK;
}

// What a family adds to vertex_run.  X^k = U^H W_k U goes either into the
// group's scratch behind W_k U, reduced group by group (reduce(b, X, k0, gk):
// X holds the vertices k0 .. k0 + gk - 1), or into the resident d_nb_x,
// reduced once after every group (reduce(b, X, 0, nk)).
struct VertexFamily {
  int timer;           // T_RESPONSE / T_OPERATOR / T_NAMBU / T_MAP
  int64_t nk;          // vertices of the call
  bool resident;
  int64_t npart, nout;   // elements of d_rs_part, results per state in d_rs_out
  std::function<int()> extras;                        // the family's own buffers and uploads
  std::function<void(const dwh::TrBufs&)> stats;      // f, g (and what else it takes from U, E) of a state
  std::function<void(const dwh::TrBufs&, const double2*, int64_t, int)> reduce;
  std::function<void(const dwh::TrBufs&)> with_uh;   // (optional) what it takes from U^H alone, before any vertex
  double extra_work = 0;                             // flops per state beyond the nk products of X
};

// The m states of src through the pipeline: one batched eigensolve, then per
// state the family's column statistic, U^H once (the slot's Jmn, so every
// product is 'N','N' as in transport_run) and per group of vertices W_k U
// (launch_op_apply on the CSR) and the batched product against the shared U^H
// (stride 0), with the family's reductions, every one in a fixed order.
// Every column of X is computed (no particle-hole half sum).  out: nout
// doubles per state, as the family laid d_rs_out out.
int vertex_run(dwh_ctx* ctx, const TrSrc& src, int m, const Vertex& v, const VertexFamily& fam,
               std::vector<double>* out) {
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), m)))
    return rc;
  // The workspace only now: transport_prepare releases it (response_release)
  // when it has to grow the slots.
  const int N = ctx->d.N, n2 = 2 * N, g = rs_group(ctx, fam.nk);
  const int64_t sA = (int64_t)n2 * n2;
  if ((rc = vertex_prepare(ctx, v, fam.resident ? g : 2 * g, fam.npart, fam.nout)) || (rc = fam.extras())) return rc;
  hipStream_t s = ctx->stream;
  HIPCHECK(ctx, hipStreamSynchronize(s));   // (the uploads)
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  double2* WU = ctx->d_rs_ws;
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  out->resize((size_t)m * fam.nout);
  for (int k = 0; k < m; ++k) {
    Scope sc(ctx, fam.timer, 8.0 * n2 * (double)n2 * n2 * fam.nk + fam.extra_work);
    const dwh::TrBufs b = tr_slot(ctx, k);
    fam.stats(b);
    dwh::launch_tr_conj_transpose(b.U, n2, n2, n2, 0, b.Jmn, n2, 0, 1, s);
    if (fam.with_uh) fam.with_uh(b);
    for (int64_t k0 = 0; k0 < fam.nk; k0 += g) {
      const int gk = (int)std::min<int64_t>(g, fam.nk - k0);
      double2* X = fam.resident ? ctx->d_nb_x + k0 * sA : WU + (int64_t)g * sA;
      dwh::launch_op_apply(b.U, WU, sA, N, ctx->d_rs_idx, ctx->d_rs_col, ctx->d_rs_val + k0 * v.nz, v.nz, gk, s);
      dwh::gemm_z('N', 'N', n2, n2, n2, one, b.Jmn, n2, 0, WU, n2, sA, zero, X, n2, sA, gk, s);
      if (!fam.resident) fam.reduce(b, X, k0, gk);
    }
    if (fam.resident) fam.reduce(b, ctx->d_nb_x, 0, (int)fam.nk);
    HIPCHECK(ctx, hipGetLastError());
    if (fam.nout > 0)
      HIPCHECK(ctx, hipMemcpyAsync(out->data() + (size_t)k * fam.nout, ctx->d_rs_out, fam.nout * sizeof(double),
                                   hipMemcpyDeviceToHost, s));
  }
  return eigen_info_check(ctx, m);   // (synchronises)
}

// dia_α and Λ_αα(q, iΩ_l) of the m states of src; the column statistic also
// gives the diamagnetic weight (launch_rs_colstats in place of launch_op_fermi).
// dia: m, lambda: nl x nq per state (host).
int response_run(dwh_ctx* ctx, const TrSrc& src, int m, const Vertex& v, const CurrentBonds& cb, int64_t nq,
                 int64_t nl, double* dia, double* lambda) {
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, g = rs_group(ctx, nq), nout = 1 + nq * nl;
  hipStream_t s = ctx->stream;
  VertexFamily fam{T_RESPONSE, nq, false, g * nl * n2, nout};
  fam.extras = [&]() -> int {
    if (int rc = rs_grow(ctx, &ctx->d_rs_nbr, &ctx->rs_nnbr, (int64_t)cb.nbr.size())) return rc;
    HIPCHECK(ctx, hipMemcpyAsync(ctx->d_rs_nbr, cb.nbr.data(), cb.nbr.size() * sizeof(int), hipMemcpyHostToDevice, s));
    return DWH_OK;
  };
  fam.stats = [&](const dwh::TrBufs& b) {
    dwh::launch_rs_colstats(b.U, N, b.E, ctx->beta, cb.tb, ctx->d_rs_nbr, b.f, b.g, b.dia, s);
    dwh::launch_rs_sum(b.dia, n2, 1, 1.0 / N, ctx->d_rs_out, s);
  };
  fam.reduce = [&](const dwh::TrBufs& b, const double2* Jnm, int64_t q0, int gq) {
    dwh::launch_rs_pairs(Jnm, sA, N, b.E, b.f, b.g, ctx->beta, (int)nl, gq, ctx->d_rs_part, s);
    dwh::launch_rs_sum(ctx->d_rs_part, n2, gq * (int)nl, 1.0 / N, ctx->d_rs_out + 1 + q0 * nl, s);
  };
  std::vector<double> out;
  if (int rc = vertex_run(ctx, src, m, v, fam, &out)) return rc;
  for (int k = 0; k < m; ++k) {
    dia[k] = out[(size_t)k * nout];
    std::copy(out.begin() + (size_t)k * nout + 1, out.begin() + (size_t)(k + 1) * nout, lambda + (size_t)k * nq * nl);
  }
  return DWH_OK;
}

// χ(l) and χ''(ω_j) of the nops operators at the m states of src: the
// Matsubara pair sums with their fixed-order reduction and the χ'' kernels,
// group by group.  chi: nl x nops, chi2: nw x nops per state (host).
int operator_run(dwh_ctx* ctx, const TrSrc& src, int m, const Vertex& v, int64_t nops, int64_t nl, double eta,
                 double w_start, double w_step, int64_t nw, double* chi, double* chi2) {
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, g = rs_group(ctx, nops), nout = nops * (nl + nw);
  hipStream_t s = ctx->stream;
  VertexFamily fam{T_OPERATOR, nops, false, g * nl * n2, nout};
  fam.extras = [&]() { return rs_grow(ctx, &ctx->d_op_part, &ctx->op_npart, g * dwh::op_spec_chunks(N) * nw); };
  fam.stats = [&](const dwh::TrBufs& b) { dwh::launch_op_fermi(b.E, N, ctx->beta, b.f, b.g, s); };
  fam.reduce = [&](const dwh::TrBufs& b, const double2* Vnm, int64_t k0, int gk) {
    double *d_chi = ctx->d_rs_out, *d_chi2 = ctx->d_rs_out + nops * nl;
    if (nl > 0) {
      dwh::launch_rs_pairs(Vnm, sA, N, b.E, b.f, b.g, ctx->beta, (int)nl, gk, ctx->d_rs_part, s);
      dwh::launch_rs_sum(ctx->d_rs_part, n2, gk * (int)nl, 1.0 / N, d_chi + k0 * nl, s);
    }
    if (nw > 0)
      dwh::launch_op_spec(Vnm, sA, N, b.E, b.f, b.g, ctx->beta, eta, w_start, w_step, (int)nw, gk, ctx->d_op_part,
                          d_chi2 + k0 * nw, s);
  };
  std::vector<double> out;
  if (int rc = vertex_run(ctx, src, m, v, fam, &out)) return rc;
  for (int k = 0; k < m; ++k) {
    const double* o = out.data() + (size_t)k * nout;
    if (nl > 0) std::copy(o, o + nops * nl, chi + (size_t)k * nops * nl);
    if (nw > 0) std::copy(o + nops * nl, o + nout, chi2 + (size_t)k * nops * nw);
  }
  return DWH_OK;
}

// chi[p, l] and chi2[p, j] of the pairs at the m states of src, from the
// resident X of every vertex: the Matsubara pair sums of all pairs with their
// fixed-order reduction, and the chi2 kernels per batch of pairs.  chi: nl x
// npairs, chi2: nw x npairs complex per state (host).
int nambu_run(dwh_ctx* ctx, const TrSrc& src, int m, const Vertex& v, int64_t nops, const std::vector<int>& pairs,
              int64_t nl, double eta, double w_start, double w_step, int64_t nw, dwh_c128* chi, dwh_c128* chi2) {
  const int N = ctx->d.N, n2 = 2 * N, np = (int)(pairs.size() / 2);
  const int64_t sA = (int64_t)n2 * n2, nout = 2 * (int64_t)np * (nl + nw);
  hipStream_t s = ctx->stream;
  VertexFamily fam{T_NAMBU, nops, true, 2 * (int64_t)np * nl * n2, nout};
  fam.extras = [&]() -> int {
    const int64_t nb = std::min<int64_t>(np, kNbPairBatch);
    int rc;
    if ((rc = rs_grow(ctx, &ctx->d_nb_x, &ctx->nb_nx, nops * sA)) ||
        (rc = rs_grow(ctx, &ctx->d_nb_part, &ctx->nb_npart, 2 * nb * dwh::op_spec_chunks(N) * nw)) ||
        (rc = rs_grow(ctx, &ctx->d_nb_pairs, &ctx->nb_npairs, 2 * (int64_t)np)))
      return rc;
    HIPCHECK(ctx, hipMemcpyAsync(ctx->d_nb_pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, s));
    return DWH_OK;
  };
  fam.stats = [&](const dwh::TrBufs& b) { dwh::launch_op_fermi(b.E, N, ctx->beta, b.f, b.g, s); };
  fam.reduce = [&](const dwh::TrBufs& b, const double2* X, int64_t, int) {
    double *d_chi = ctx->d_rs_out, *d_chi2 = ctx->d_rs_out + 2 * np * nl;
    if (nl > 0) {
      dwh::launch_nb_pairs(X, sA, N, ctx->d_nb_pairs, np, b.E, b.f, b.g, ctx->beta, (int)nl, ctx->d_rs_part, s);
      dwh::launch_rs_sum(ctx->d_rs_part, n2, 2 * np * (int)nl, 1.0 / N, d_chi, s);
    }
    if (nw > 0)
      for (int p0 = 0; p0 < np; p0 += kNbPairBatch)
        dwh::launch_nb_spec(X, sA, N, ctx->d_nb_pairs, p0, std::min(kNbPairBatch, np - p0), b.E, b.f, b.g, ctx->beta,
                            eta, w_start, w_step, (int)nw, ctx->d_nb_part, d_chi2, s);
  };
  std::vector<double> out;
  if (int rc = vertex_run(ctx, src, m, v, fam, &out)) return rc;
  for (int k = 0; k < m; ++k) {
    const dwh_c128* o = reinterpret_cast<const dwh_c128*>(out.data() + (size_t)k * nout);
    if (nl > 0) std::copy(o, o + np * nl, chi + (size_t)k * np * nl);
    if (nw > 0) std::copy(o + np * nl, o + np * (nl + nw), chi2 + (size_t)k * np * nw);
  }
  return DWH_OK;
}

// frequencies per chunk of a response-map call: the chunk's K_z and S_z = K_z U^H
// within kRsCapBytes and its sampled entries within 1 GiB; one frequency is
// always allowed (DWHMC_MAP_CHUNK: a smaller chunk, for tests of the chunk loop)
int map_chunk(const dwh_ctx* ctx, int64_t nz, int64_t npat) {
  const double n2 = 2.0 * ctx->d.N;
  int c = (int)std::min<double>(kRsMaxGroup, kRsCapBytes / (2.0 * 16.0 * n2 * n2));
  c = (int)std::min<int64_t>(c, (1ll << 26) / npat);
  if (const char* e = std::getenv("DWHMC_MAP_CHUNK")) c = std::min(c, std::atoi(e));
  return (int)std::max<int64_t>(1, std::min<int64_t>(c, nz));
}

// rho[e] and dmap[e + npat (z + nz k)] of the m states of src (host, per state
// npat and npat nz nops complex; either nullable).  Per state ρ from
// S = diag(f) U^H, then per vertex of a group and per chunk of frequencies:
// K_z = w(z) ∘ X (launch_map_weight), S_z = K_z U^H (the batched product, U^H
// at stride 0) and the sampled product on the column-grouped pattern, copied
// out chunk by chunk.  Without dmap no vertex is applied (nk = 0).
int map_run(dwh_ctx* ctx, const TrSrc& src, int m, const Vertex& v, int64_t nops, const MapPlan& pl,
            const int64_t* prow, int64_t nl, double eta, const std::vector<double>& omega, dwh_c128* rho,
            dwh_c128* dmap) {
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, npat = (int64_t)pl.order.size(), nw = (int64_t)omega.size(), nz = nl + nw;
  const int chunk = dmap ? map_chunk(ctx, nz, npat) : 0;
  hipStream_t s = ctx->stream;
  // the pattern as the kernel reads it: row a and original index of every
  // grouped entry, and the column groups cut into workgroup slices (b, first, count)
  std::vector<int> idx(2 * (size_t)npat), slices;
  for (int64_t i = 0; i < npat; ++i) {
    idx[(size_t)i] = (int)prow[pl.order[(size_t)i]];
    idx[(size_t)(npat + i)] = pl.order[(size_t)i];
  }
  for (int b = 0; b < n2; ++b)
    for (int i = pl.colptr[b]; i < pl.colptr[b + 1]; i += dwh::kMapSlice)
      slices.insert(slices.end(), {b, i, std::min(dwh::kMapSlice, pl.colptr[b + 1] - i)});
  const int nslices = (int)(slices.size() / 3);
  int state = -1, lrc = DWH_OK;
  auto copy_out = [&](dwh_c128* dst, int64_t count) {
    if (lrc == DWH_OK && hipMemcpyAsync(dst, ctx->d_map_out, (size_t)count * sizeof(double2), hipMemcpyDeviceToHost,
                                        s) != hipSuccess)
      lrc = fail(ctx, DWH_ERR_HIP, "response map: copying the sampled entries out failed");
  };
  VertexFamily fam{T_MAP, dmap ? nops : 0, false, 0, 0};
  fam.extra_work = dmap ? 8.0 * n2 * (double)n2 * n2 * (double)(nops * nz) : 0.0;
  fam.extras = [&]() -> int {
    int rc;
    if ((rc = rs_grow(ctx, &ctx->d_map_ws, &ctx->map_nws, std::max<int64_t>(2 * chunk, 1) * sA)) ||
        (rc = rs_grow(ctx, &ctx->d_map_out, &ctx->map_nout, std::max<int64_t>(chunk, 1) * npat)) ||
        (rc = rs_grow(ctx, &ctx->d_map_omega, &ctx->map_nomega, nw)) ||
        (rc = rs_grow(ctx, &ctx->d_map_idx, &ctx->map_nidx, 2 * npat)) ||
        (rc = rs_grow(ctx, &ctx->d_map_slice, &ctx->map_nslice, (int64_t)slices.size())))
      return rc;
    if (nw > 0)
      HIPCHECK(ctx, hipMemcpyAsync(ctx->d_map_omega, omega.data(), nw * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->d_map_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->d_map_slice, slices.data(), slices.size() * sizeof(int), hipMemcpyHostToDevice, s));
    return DWH_OK;
  };
  fam.stats = [&](const dwh::TrBufs& b) {
    ++state;
    dwh::launch_op_fermi(b.E, N, ctx->beta, b.f, b.g, s);
  };
  auto sample = [&](const dwh::TrBufs& b, const double2* S, int nmat) {
    dwh::launch_map_sddmm(b.Jmn, S, sA, N, ctx->d_map_slice, nslices, ctx->d_map_idx, ctx->d_map_idx + npat,
                          ctx->d_map_out, npat, nmat, s);
  };
  fam.with_uh = [&](const dwh::TrBufs& b) {
    if (!rho) return;
    dwh::launch_map_fscale(b.Jmn, N, b.f, ctx->d_map_ws, s);
    sample(b, ctx->d_map_ws, 1);
    copy_out(rho + (size_t)state * npat, npat);
  };
  fam.reduce = [&](const dwh::TrBufs& b, const double2* X, int64_t k0, int gk) {
    const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
    double2 *K = ctx->d_map_ws, *S = ctx->d_map_ws + (int64_t)chunk * sA;
    for (int j = 0; j < gk; ++j)
      for (int64_t z0 = 0; z0 < nz; z0 += chunk) {
        const int c = (int)std::min<int64_t>(chunk, nz - z0);
        dwh::launch_map_weight(X + (int64_t)j * sA, N, b.E, b.f, b.g, ctx->beta, (int)z0, c, (int)nl,
                               ctx->d_map_omega, eta, K, sA, s);
        dwh::gemm_z('N', 'N', n2, n2, n2, one, K, n2, sA, b.Jmn, n2, 0, zero, S, n2, sA, c, s);
        sample(b, S, c);
        copy_out(dmap + (size_t)npat * (z0 + nz * (k0 + j + nops * (int64_t)state)), c * npat);
      }
  };
  std::vector<double> out;
  ctx->map_last_chunk = 0;
  if (int rc = vertex_run(ctx, src, m, v, fam, &out)) return rc;
  if (dmap && lrc == DWH_OK) {
    ctx->map_last_nslices = nslices;
    ctx->map_last_npat = npat;
    ctx->map_last_chunk = chunk;
    ctx->map_last_x = (int64_t)rs_group(ctx, nops) * sA;
  }
  return lrc;
}

// ---------------------------------------------------------------------------
// Equal-time correlations of local families (dwhmc_corr.hip)
// ---------------------------------------------------------------------------

// The term table, pair list and reference sites of a correlation call as the
// device reads them (ints, terms in the caller's order, duplicates kept).
struct CorrPlan {
  std::vector<int> tptr, trow, tcol, pairs, ref;
  std::vector<double2> val;
};
constexpr int64_t kCorrMaxTermsAll = 1 << 24;
constexpr int64_t kCorrMaxPartials = 1 << 27;

// Checks the arguments and fills the plan; with_pairs / with_local: the pair
// list / the reference sites are needed (else ignored).  ctx may be NULL.
int corr_plan(dwh_ctx* ctx, int64_t N, int64_t nfam, const int64_t* tptr, const int64_t* trow, const int64_t* tcol,
              const dwh_c128* tval, bool with_pairs, int64_t npairs, const int64_t* pairs, bool with_local,
              int64_t nref, const int64_t* ref, CorrPlan* pl) {
  const std::string pre = "correlations";
  if (N < 1 || N > (1 << 24)) return fail(ctx, DWH_ERR_ARG, pre + ": N must be in [1, 2^24]");
  if (2 * N > dwh::kCorrMaxN2)
    return fail(ctx, DWH_ERR_ARG, pre + ": 2N above " + std::to_string(dwh::kCorrMaxN2));
  if (nfam < 1 || nfam > (1 << 16)) return fail(ctx, DWH_ERR_ARG, pre + ": nfam must be in [1, 2^16]");
  if (!tptr) return fail(ctx, DWH_ERR_ARG, pre + ": NULL argument (tptr)");
  if (tptr[0] != 0) return fail(ctx, DWH_ERR_ARG, pre + ": tptr must start at 0");
  const int64_t nsl = nfam * N;
  for (int64_t e = 0; e < nsl; ++e) {
    const std::string at = "(family " + std::to_string(e / N) + ", site " + std::to_string(e % N) + ")";
    if (tptr[e + 1] < tptr[e]) return fail(ctx, DWH_ERR_ARG, pre + ": tptr decreases at " + at);
    if (tptr[e + 1] - tptr[e] > dwh::kCorrMaxTerms)
      return fail(ctx, DWH_ERR_ARG, pre + ": more than " + std::to_string(dwh::kCorrMaxTerms) + " terms at " + at);
    if (tptr[e + 1] > kCorrMaxTermsAll) return fail(ctx, DWH_ERR_ARG, pre + ": more than 2^24 terms");
  }
  const int64_t nt = tptr[nsl], n2 = 2 * N;
  if (nt > 0 && (!trow || !tcol || !tval)) return fail(ctx, DWH_ERR_ARG, pre + ": NULL argument (trow, tcol or tval)");
  for (int64_t t = 0; t < nt; ++t) {
    if (trow[t] < 0 || trow[t] >= n2 || tcol[t] < 0 || tcol[t] >= n2)
      return fail(ctx, DWH_ERR_ARG, pre + ": term " + std::to_string(t) + " (" + std::to_string(trow[t]) + ", " +
                                        std::to_string(tcol[t]) + ") outside [0, 2N)");
    if (!std::isfinite(tval[t].re) || !std::isfinite(tval[t].im))
      return fail(ctx, DWH_ERR_ARG, pre + ": non-finite value at term " + std::to_string(t));
  }
  if (with_pairs) {
    if (npairs < 1) return fail(ctx, DWH_ERR_ARG, pre + ": npairs must be >= 1 with a corr or local output");
    if (!pairs) return fail(ctx, DWH_ERR_ARG, pre + ": NULL argument (pairs)");
    if (npairs > (1 << 16)) return fail(ctx, DWH_ERR_ARG, pre + ": more than 2^16 pairs");
    for (int64_t k = 0; k < 2 * npairs; ++k)
      if (pairs[k] < 0 || pairs[k] >= nfam)
        return fail(ctx, DWH_ERR_ARG, pre + ": pair index " + std::to_string(pairs[k]) + " outside [0, nfam)");
  }
  if (with_local) {
    if (nref < 1) return fail(ctx, DWH_ERR_ARG, pre + ": a local output needs nref >= 1");
    if (!ref) return fail(ctx, DWH_ERR_ARG, pre + ": NULL argument (ref)");
    if (nref > (1 << 16)) return fail(ctx, DWH_ERR_ARG, pre + ": more than 2^16 reference sites");
    for (int64_t q = 0; q < nref; ++q)
      if (ref[q] < 0 || ref[q] >= N)
        return fail(ctx, DWH_ERR_ARG, pre + ": reference site " + std::to_string(ref[q]) + " outside [0, N)");
  }
  if (with_pairs &&
      npairs * N * std::max<int64_t>(dwh::corr_chunks((int)N), with_local ? nref : 0) > kCorrMaxPartials)
    return fail(ctx, DWH_ERR_ARG, pre + ": more than 2^27 (pair, site, displacement) partials");
  pl->tptr.assign(tptr, tptr + nsl + 1);
  pl->trow.assign(trow, trow + nt);
  pl->tcol.assign(tcol, tcol + nt);
  pl->val.resize((size_t)nt);
  for (int64_t t = 0; t < nt; ++t) pl->val[(size_t)t] = make_double2(tval[t].re, tval[t].im);
  pl->pairs.clear();
  pl->ref.clear();
  if (with_pairs) pl->pairs.assign(pairs, pairs + 2 * npairs);
  if (with_local) pl->ref.assign(ref, ref + nref);
  return DWH_OK;
}

// mean, corr and local (host, per state nfam N, npairs N and npairs nref N
// complex; each nullable) of the m states of src.  Per state S = diag(f) U^H
// into the slot's JU, ρ = U S into its Jmn (the library's product; it runs
// for a mean-only call too: the gather reads ρ), then the gather, the
// contraction with its chunk sum, and the contraction on the reference sites.
int corr_run(dwh_ctx* ctx, const TrSrc& src, int m, const CorrPlan& pl, int64_t nfam, dwh_c128* mean, dwh_c128* corr,
             dwh_c128* local) {
  int rc;
  if ((rc = transport_prepare(ctx, std::max<int64_t>(ctx->tr_nw, 0), std::max<int64_t>(ctx->tr_nd, 0), m)))
    return rc;
  // (the workspace only now: transport_prepare releases it when it grows the slots)
  const int N = ctx->d.N, n2 = 2 * N, Lx = (int)ctx->model->Lx;
  const int64_t sA = (int64_t)n2 * n2, nsl = nfam * N, nt = (int64_t)pl.val.size();
  const int np = (int)(pl.pairs.size() / 2), nref = local ? (int)pl.ref.size() : 0, nc = dwh::corr_chunks(N);
  const int64_t n_mean = mean ? nsl : 0, n_corr = corr ? (int64_t)np * N : 0, n_loc = (int64_t)np * nref * N;
  const int64_t o_row = nsl + 1, o_col = o_row + nt, o_pair = o_col + nt, o_ref = o_pair + 2 * np;
  if ((rc = rs_grow(ctx, &ctx->d_cr_idx, &ctx->cr_nidx, o_ref + (int64_t)pl.ref.size())) ||
      (rc = rs_grow(ctx, &ctx->d_cr_val, &ctx->cr_nval, nt)) ||
      (rc = rs_grow(ctx, &ctx->d_cr_part, &ctx->cr_npart, corr ? (int64_t)np * nc * N : 0)) ||
      (rc = rs_grow(ctx, &ctx->d_cr_out, &ctx->cr_nout, n_mean + n_corr + n_loc)))
    return rc;
  hipStream_t s = ctx->stream;
  auto up = [&](void* dst, const void* p, size_t bytes) {
    return bytes == 0 ? hipSuccess : hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
  };
  int* ix = ctx->d_cr_idx;
  HIPCHECK(ctx, up(ix, pl.tptr.data(), pl.tptr.size() * sizeof(int)));
  HIPCHECK(ctx, up(ix + o_row, pl.trow.data(), pl.trow.size() * sizeof(int)));
  HIPCHECK(ctx, up(ix + o_col, pl.tcol.data(), pl.tcol.size() * sizeof(int)));
  HIPCHECK(ctx, up(ix + o_pair, pl.pairs.data(), pl.pairs.size() * sizeof(int)));
  HIPCHECK(ctx, up(ix + o_ref, pl.ref.data(), pl.ref.size() * sizeof(int)));
  HIPCHECK(ctx, up(ctx->d_cr_val, pl.val.data(), pl.val.size() * sizeof(double2)));
  HIPCHECK(ctx, hipStreamSynchronize(s));   // (the uploads)
  if ((rc = eigen_solve(ctx, src, m))) return rc;
  // bytes the contractions issue: two 16-byte loads per (term of A, term of B)
  std::vector<double> cnt((size_t)nfam, 0.0);
  for (int64_t k = 0; k < nfam; ++k) cnt[(size_t)k] = (double)(pl.tptr[(size_t)((k + 1) * N)] - pl.tptr[(size_t)(k * N)]);
  double issued = 0;
  for (int p = 0; p < np; ++p) {
    const int a = pl.pairs[2 * (size_t)p], b = pl.pairs[2 * (size_t)p + 1];
    if (corr) issued += 32.0 * cnt[(size_t)a] * cnt[(size_t)b];
    for (int q = 0; q < nref; ++q) {
      const size_t e = (size_t)b * N + (size_t)pl.ref[(size_t)q];
      issued += 32.0 * cnt[(size_t)a] * (double)(pl.tptr[e + 1] - pl.tptr[e]);
    }
  }
  const double2 one = make_double2(1.0, 0.0), zero = make_double2(0.0, 0.0);
  double2 *o_mean = ctx->d_cr_out, *o_corr = o_mean + n_mean, *o_loc = o_corr + n_corr;
  auto down = [&](dwh_c128* dst, const double2* p, int64_t count) {
    return hipMemcpyAsync(dst, p, (size_t)count * sizeof(double2), hipMemcpyDeviceToHost, s);
  };
  for (int k = 0; k < m; ++k) {
    const dwh::TrBufs b = tr_slot(ctx, k);
    double2* rho = b.Jmn;
    {
      Scope sc(ctx, T_CORR_RHO, 8.0 * n2 * (double)n2 * n2);
      dwh::launch_op_fermi(b.E, N, ctx->beta, b.f, b.g, s);
      dwh::launch_tr_conj_transpose(b.U, n2, n2, n2, 0, b.Jmn, n2, 0, 1, s);
      dwh::launch_map_fscale(b.Jmn, N, b.f, b.JU, s);
      dwh::gemm_z('N', 'N', n2, n2, n2, one, b.U, n2, sA, b.JU, n2, sA, zero, rho, n2, sA, 1, s);
    }
    if (np > 0 && (corr || local)) {
      Scope sc(ctx, T_CORR_CONTRACT, issued);
      if (corr)
        dwh::launch_corr(rho, N, Lx, ix, ix + o_row, ix + o_col, ctx->d_cr_val, ix + o_pair, np, nullptr, N,
                         ctx->d_cr_part, s);
      if (local)
        dwh::launch_corr(rho, N, Lx, ix, ix + o_row, ix + o_col, ctx->d_cr_val, ix + o_pair, np, ix + o_ref, nref,
                         o_loc, s);
    }
    {
      Scope sc(ctx, T_CORR_REDUCE, 16.0 * ((double)n_corr * (nc + 1) + (double)n_mean + 2.0 * (mean ? nt : 0)));
      if (corr) dwh::launch_corr_sum(ctx->d_cr_part, N, np, o_corr, s);
      if (mean) dwh::launch_corr_mean(rho, N, ix, ix + o_row, ix + o_col, ctx->d_cr_val, (int)nfam, o_mean, s);
    }
    HIPCHECK(ctx, hipGetLastError());
    if (mean) HIPCHECK(ctx, down(mean + (size_t)k * nsl, o_mean, n_mean));
    if (corr) HIPCHECK(ctx, down(corr + (size_t)k * n_corr, o_corr, n_corr));
    if (local) HIPCHECK(ctx, down(local + (size_t)k * n_loc, o_loc, n_loc));
    // (the next state overwrites d_cr_out: the copies are on the same stream)
  }
  return eigen_info_check(ctx, m);   // (synchronises)
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
  int64_t nw = 0, nd = 0;
  int rc;
  if ((rc = check_state_args(ctx, chain, nstates, Delta))) return rc;
  if ((rc = transport_args(ctx, eta, domega, omega_max, n_omega, n_dos, &nw, &nd))) return rc;
  if ((nw > 0 && !sigma) || (nd > 0 && (!dos || !dos_an))) return fail(ctx, DWH_ERR_ARG, "NULL grid output");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int N = ctx->d.N;
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    return transport_run(ctx, src, m, eta, domega, omega_max, nw, nd, stiffness + s0, dc_cond + s0,
                         sigma ? sigma + (size_t)s0 * nw : nullptr, dos ? dos + (size_t)s0 * nd : nullptr,
                         dos_an ? dos_an + (size_t)s0 * nd : nullptr, ak0 + (size_t)s0 * N);
  });
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
  if (int rc = check_state_args(ctx, chain, nstates, Delta)) return rc;
  if (dwh_spectral_window(eta, domega, omega_max, first, count, stride, nullptr) != DWH_OK)
    return fail(ctx, DWH_ERR_ARG, g_create_error);
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int N = ctx->d.N;
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    const size_t off = (size_t)N * count * s0;
    return spectral_run(ctx, src, m, eta, domega, omega_max, first, count, stride, ldos ? ldos + off : nullptr,
                        akw ? akw + off : nullptr);
  });
}

int dwh_measure_current_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                 int32_t direction, int64_t nq, const int64_t* q, int64_t n_matsubara, double* dia,
                                 double* lambda) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  if (!q || !dia || !lambda) return fail(ctx, DWH_ERR_ARG, "NULL argument (q, dia or lambda)");
  if (int rc = check_state_args(ctx, chain, nstates, Delta)) return rc;
  if (int rc = current_args(ctx, *ctx->model, direction, nq, q, n_matsubara)) return rc;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const CurrentBonds cb = current_bonds(*ctx->model, direction);
  Vertex v;
  build_current_vertex(*ctx->model, cb, nq, q, &v);
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    return response_run(ctx, src, m, v, cb, nq, n_matsubara, dia + s0, lambda + (size_t)s0 * nq * n_matsubara);
  });
}

int dwh_debug_current_vertex(int64_t Lx, int64_t Ly, double t, double tp, const int64_t* nn_table,
                             const int64_t* nnn_table, int32_t direction, int64_t nq, const int64_t* q,
                             dwh_c128* out) {
  if (!q || !out) return fail(nullptr, DWH_ERR_ARG, "NULL argument (q or out)");
  if (Lx < 1 || Ly < 1 || Lx > (1 << 24) / Ly) return fail(nullptr, DWH_ERR_ARG, "Lx, Ly must be >= 1, Lx Ly <= 2^24");
  HostModel model;
  const std::vector<double> clean((size_t)(Lx * Ly), 0.0);
  if (int rc = build_host_model(Lx, Ly, t, tp, 0.0, nn_table, nnn_table, 1, clean.data(), &model, false)) return rc;
  if (int rc = current_args(nullptr, model, direction, nq, q, 1)) return rc;
  Vertex v;
  build_current_vertex(model, current_bonds(model, direction), nq, q, &v);
  densify(v, model.N, nq, out);
  return DWH_OK;
}

int dwh_measure_operator_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                  int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                                  const dwh_c128* val, const int32_t* spin_sign, int64_t n_matsubara, double* chi,
                                  double eta, double w_start, double w_step, int64_t n_w, double* chi2) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  int rc;
  if ((rc = check_state_args(ctx, chain, nstates, Delta))) return rc;
  Vertex v;
  if (nops < 1 || nnz < 1) return fail(ctx, DWH_ERR_ARG, "operator: nops and nnz must be >= 1");
  if ((rc = operator_args(ctx, nops, n_matsubara, chi, eta, w_start, w_step, n_w, chi2))) return rc;
  if ((rc = build_operator_nambu(ctx, ctx->d.N, nops, rowptr, col, nnz, val, spin_sign, &v))) return rc;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    return operator_run(ctx, src, m, v, nops, n_matsubara, eta, w_start, w_step, n_w,
                        chi ? chi + (size_t)s0 * nops * n_matsubara : nullptr,
                        chi2 ? chi2 + (size_t)s0 * nops * n_w : nullptr);
  });
}

int dwh_debug_operator_nambu(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                             const dwh_c128* val, const int32_t* spin_sign, dwh_c128* out) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "NULL argument (out)");
  Vertex v;
  if (int rc = build_operator_nambu(nullptr, N, nops, rowptr, col, nnz, val, spin_sign, &v)) return rc;
  densify(v, N, nops, out);
  return DWH_OK;
}

int dwh_measure_nambu_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta, int64_t nops,
                               const int64_t* rowptr, const int64_t* col, int64_t nnz, const dwh_c128* val,
                               int64_t npairs, const int64_t* pairs, int64_t n_matsubara, dwh_c128* chi, double eta,
                               double w_start, double w_step, int64_t n_w, dwh_c128* chi2) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  int rc;
  if ((rc = check_state_args(ctx, chain, nstates, Delta))) return rc;
  Vertex v;
  // (the vertex and pair checks first: they bound npairs for the count checks)
  if ((rc = build_nambu_vertices(ctx, ctx->d.N, nops, rowptr, col, nnz, val, npairs, pairs, &v))) return rc;
  if ((rc = operator_args(ctx, npairs, n_matsubara, reinterpret_cast<const double*>(chi), eta, w_start, w_step, n_w,
                          reinterpret_cast<const double*>(chi2))))
    return rc;
  std::vector<int> pr(pairs, pairs + 2 * npairs);
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    return nambu_run(ctx, src, m, v, nops, pr, n_matsubara, eta, w_start, w_step, n_w,
                     chi ? chi + (size_t)s0 * npairs * n_matsubara : nullptr,
                     chi2 ? chi2 + (size_t)s0 * npairs * n_w : nullptr);
  });
}

int dwh_debug_nambu_dense(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                          const dwh_c128* val, int64_t npairs, const int64_t* pairs, dwh_c128* out) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "NULL argument (out)");
  Vertex v;
  if (int rc = build_nambu_vertices(nullptr, N, nops, rowptr, col, nnz, val, npairs, pairs, &v)) return rc;
  densify(v, N, nops, out);
  return DWH_OK;
}

int dwh_measure_response_map(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta, int64_t nops,
                             const int64_t* rowptr, const int64_t* col, int64_t nnz, const dwh_c128* val,
                             int64_t npat, const int64_t* prow, const int64_t* pcol, int64_t n_matsubara, double eta,
                             int64_t n_w, const double* omega, dwh_c128* rho, dwh_c128* dmap) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  int rc;
  if ((rc = check_state_args(ctx, chain, nstates, Delta))) return rc;
  const int64_t N = ctx->d.N;
  if ((rc = check_nambu_csr(ctx, "response map", N, nops, rowptr, col, nnz, val))) return rc;
  if ((rc = map_args(ctx, N, nops, n_matsubara, eta, n_w, omega, rho, dmap))) return rc;
  MapPlan pl;
  if ((rc = map_plan(ctx, N, npat, prow, pcol, &pl))) return rc;
  Vertex v;
  fill_nambu_vertices(N, nops, rowptr, col, nnz, val, &v);
  const std::vector<double> w(omega, omega + (n_w > 0 ? n_w : 0));
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int64_t nz = n_matsubara + n_w;
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    return map_run(ctx, src, m, v, nops, pl, prow, n_matsubara, eta, w, rho ? rho + (size_t)s0 * npat : nullptr,
                   dmap ? dmap + (size_t)s0 * nops * nz * npat : nullptr);
  });
}

int dwh_debug_response_map_plan(int64_t N, int64_t npat, const int64_t* prow, const int64_t* pcol, int64_t* order,
                                int64_t* colptr) {
  if (!order || !colptr) return fail(nullptr, DWH_ERR_ARG, "response map: NULL argument (order or colptr)");
  MapPlan pl;
  if (int rc = map_plan(nullptr, N, npat, prow, pcol, &pl)) return rc;
  std::copy(pl.order.begin(), pl.order.end(), order);
  std::copy(pl.colptr.begin(), pl.colptr.end(), colptr);
  return DWH_OK;
}

int dwh_measure_correlations(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta, int64_t nfam,
                             const int64_t* tptr, const int64_t* trow, const int64_t* tcol, const dwh_c128* tval,
                             int64_t npairs, const int64_t* pairs, int64_t nref, const int64_t* ref, dwh_c128* mean,
                             dwh_c128* corr, dwh_c128* local) {
  if (!ctx) return fail(nullptr, DWH_ERR_ARG, "NULL context");
  int rc;
  if ((rc = check_state_args(ctx, chain, nstates, Delta))) return rc;
  if (!mean && !corr && !local) return fail(ctx, DWH_ERR_ARG, "correlations: mean, corr and local are all NULL");
  const int64_t N = ctx->d.N;
  CorrPlan pl;
  if ((rc = corr_plan(ctx, N, nfam, tptr, trow, tcol, tval, corr || local, npairs, pairs, local != nullptr, nref, ref,
                      &pl)))
    return rc;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  // DWHMC_RESPONSE_GROUP=g: state groups of at most g (tests of the grouping loop).  Only this call reads
  // it for its states: the vertex responses spend it on their vertex groups (rs_group).
  int cap = 0;
  if (const char* e = std::getenv("DWHMC_RESPONSE_GROUP")) cap = std::max(1, std::atoi(e));
  const int64_t np = corr || local ? npairs : 0, nr = local ? nref : 0;
  return for_each_state_group(ctx, chain, nstates, Delta, [&](const TrSrc& src, int m, int64_t s0) {
    return corr_run(ctx, src, m, pl, nfam, mean ? mean + (size_t)s0 * nfam * N : nullptr,
                    corr ? corr + (size_t)s0 * np * N : nullptr, local ? local + (size_t)s0 * np * nr * N : nullptr);
  }, cap);
}

int dwh_debug_correlation_dense(int64_t N, int64_t nfam, const int64_t* tptr, const int64_t* trow,
                                const int64_t* tcol, const dwh_c128* tval, int64_t npairs, const int64_t* pairs,
                                int64_t nref, const int64_t* ref, dwh_c128* out) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "correlations: NULL argument (out)");
  CorrPlan pl;
  if (int rc = corr_plan(nullptr, N, nfam, tptr, trow, tcol, tval, npairs != 0 || pairs, npairs, pairs,
                         nref != 0 || ref, nref, ref, &pl))
    return rc;
  const size_t n2 = 2 * (size_t)N;
  std::fill(out, out + (size_t)nfam * N * n2 * n2, dwh_c128{0.0, 0.0});
  for (size_t e = 0; e < (size_t)(nfam * N); ++e)
    for (int t = pl.tptr[e]; t < pl.tptr[e + 1]; ++t) {
      dwh_c128& o = out[e * n2 * n2 + (size_t)pl.trow[(size_t)t] + (size_t)pl.tcol[(size_t)t] * n2];
      o.re += pl.val[(size_t)t].x;
      o.im += pl.val[(size_t)t].y;
    }
  return DWH_OK;
}

int dwh_bench_response_map_stages(dwh_ctx* ctx, int64_t reps, int64_t nfreq, double* weight_ms, double* sample_ms) {
  if (!ctx || !weight_ms || !sample_ms) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (reps < 1 || reps > 1000) return fail(ctx, DWH_ERR_ARG, "reps must be in [1, 1000]");
  if (ctx->map_last_chunk < 1 || !ctx->d_map_ws || !ctx->d_rs_ws)
    return fail(ctx, DWH_ERR_STATE, "no response map with a dmap output has run on this context yet");
  if (nfreq < 1 || nfreq > ctx->map_last_chunk)
    return fail(ctx, DWH_ERR_ARG, "nfreq must be in [1, " + std::to_string(ctx->map_last_chunk) +
                                      "], the last call's frequencies per chunk");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int N = ctx->d.N, n2 = 2 * N;
  const int64_t sA = (int64_t)n2 * n2, npat = ctx->map_last_npat;
  const dwh::TrBufs& b = ctx->tr;
  hipStream_t s = ctx->stream;
  double2 *K = ctx->d_map_ws, *S = ctx->d_map_ws + ctx->map_last_chunk * sA;
  const int c = (int)nfreq;
  // the last call's X, K_z, S_z, U^H and pattern, as it left them (Matsubara weights l < nfreq)
  auto weight = [&]() {
    dwh::launch_map_weight(ctx->d_rs_ws + ctx->map_last_x, N, b.E, b.f, b.g, ctx->beta, 0, c, c, nullptr, 1.0, K, sA, s);
  };
  auto sample = [&]() {
    dwh::launch_map_sddmm(b.Jmn, S, sA, N, ctx->d_map_slice, (int)ctx->map_last_nslices, ctx->d_map_idx,
                          ctx->d_map_idx + npat, ctx->d_map_out, npat, c, s);
  };
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  for (auto& ev : e) HIPCHECK(ctx, hipEventCreate(&ev));
  weight();   // warm
  sample();
  HIPCHECK(ctx, hipEventRecord(e[0], s));
  for (int64_t r = 0; r < reps; ++r) weight();
  HIPCHECK(ctx, hipEventRecord(e[1], s));
  for (int64_t r = 0; r < reps; ++r) sample();
  HIPCHECK(ctx, hipEventRecord(e[2], s));
  HIPCHECK(ctx, hipStreamSynchronize(s));
  HIPCHECK(ctx, hipGetLastError());
  float tw = 0.f, ts = 0.f;
  HIPCHECK(ctx, hipEventElapsedTime(&tw, e[0], e[1]));
  HIPCHECK(ctx, hipEventElapsedTime(&ts, e[1], e[2]));
  for (auto& ev : e) (void)hipEventDestroy(ev);
  *weight_ms = (double)tw / (double)reps;
  *sample_ms = (double)ts / (double)reps;
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
