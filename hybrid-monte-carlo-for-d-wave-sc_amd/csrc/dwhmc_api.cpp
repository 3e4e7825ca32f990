// C-ABI context of the MI355X fermionic action/force path (include/dwhmc.h):
// context creation, the leapfrog step (Gauss-Jordan / cyclic reduction / eig),
// the guards with their pole re-selection, and the HMC and state entry points.
// The context struct is in dwhmc_ctx.h, the eigensolver driver in
// dwhmc_eigsolve.cpp and the measurements in dwhmc_measure.cpp.
//
// Context creation is a sequence of host-only steps that live elsewhere — the
// lattice model and the pole selection (dwhmc_model.cpp), the choice of
// algorithm and the cyclic-reduction plan (dwhmc_plan.cpp) — followed by the
// device side here (device_side); a pole re-selection repeats poles, plan and
// device side on the model the context keeps.  Beyond the pole table runs the
// eigendecomposition path (algo eig: the library's own eigensolver per step,
// dwhmc_eig.hip — the reference's own diagonalize + compute_forces!).  The
// per-sweep launch sequence restates hmc_sweep! (src/HMC.jl:71-144).
// All arithmetic runs in the HIP kernels (dwhmc_kernels.hip); there is no CPU
// fallback: a missing device is an error.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "dwhmc_ctx.h"

using namespace dwh;

namespace {

double tile_flops() { return 8.0 * kGJ * kGJ * kGJ; }

void gj_pivot(dwh_ctx* ctx, double2* M, int k, double2* Pout, double2* XR, double2* colcopy,
              double2* nextcol) {
  const Dims& d = ctx->d;
  Scope s(ctx, T_GJ_PIVOT, (double)d.nbatch * d.nb * tile_flops());
  dwh::launch_gj_pivot(d, M, k, Pout, XR, colcopy, nextcol, ctx->ldpart, ctx->stream);
}

// complex K=64 terms of one update launch (per matrix), for the flop count
double gj_update_terms(const Dims& d, int mode) {
  const int nb = d.nb;
  if (nb < 2) return 0;
  if (mode == 0) return (double)(nb - 1) * nb;
  if (mode == 1) return 2.0 * nb - 2;
  return nb + (double)(nb - 2) * (1 + 2.0 * (nb - 1));
}

void gj_update(dwh_ctx* ctx, double2* M, int k, int mode, const dwh::GJPanelPtrs& p) {
  const Dims& d = ctx->d;
  Scope s(ctx, mode == 1 ? T_GJ_EDGE : T_GJ_UPDATE,
          (double)d.nbatch * gj_update_terms(d, mode) * tile_flops());
  dwh::launch_gj_update(d, M, k, mode, p, ctx->stream);
}

// Blocked no-pivot Gauss-Jordan inversion of all nbatch matrices in M, two
// 64-wide block steps at a time: pivot k, edge update (block row k+1 and the
// next column panel), pivot k+1, then ONE rank-128 update of the remaining
// tiles — every matrix tile is streamed through HBM once per two pivot steps.
// An odd last step uses the single rank-64 update.
void run_gj(dwh_ctx* ctx, double2* M) {
  const Dims& d = ctx->d;
  double2* CpA[2] = {ctx->CpA0, ctx->CpA1};
  if (d.nb == 1) {
    gj_pivot(ctx, M, 0, ctx->Pb1, ctx->XR1, nullptr, nullptr);
    return;
  }
  int cur = 0;
  for (int k = 0; k < d.nb;) {
    double2* colcopy = (k == 0) ? CpA[cur] : nullptr;
    if (k + 1 < d.nb) {
      gj_pivot(ctx, M, k, ctx->Pb1, ctx->XR1, colcopy, nullptr);
      dwh::GJPanelPtrs e{CpA[cur], nullptr, ctx->XR1, nullptr, ctx->Pb1, nullptr, ctx->CpB, nullptr};
      gj_update(ctx, M, k, 1, e);
      gj_pivot(ctx, M, k + 1, ctx->Pb2, ctx->XR2, nullptr, CpA[cur ^ 1]);
      dwh::GJPanelPtrs c{CpA[cur], ctx->CpB, ctx->XR1, ctx->XR2, ctx->Pb1, ctx->Pb2, nullptr,
                         k + 2 < d.nb ? CpA[cur ^ 1] : nullptr};
      gj_update(ctx, M, k, 2, c);
      cur ^= 1;
      k += 2;
    } else {
      gj_pivot(ctx, M, k, ctx->Pb1, ctx->XR1, colcopy, nullptr);
      dwh::GJPanelPtrs sg{CpA[cur], nullptr, ctx->XR1, nullptr, ctx->Pb1, nullptr, nullptr, nullptr};
      gj_update(ctx, M, k, 0, sg);
      k += 1;
    }
  }
}

// The per-factorisation assembly launch (timer "assemble"), with its
// algorithmic bytes.  CR: the pairing entries Δ/2 scattered into the level-0
// blocks of every batch item (16 B each; no level-0 block is rewritten, CR
// inverts them out of place); dense: S^T = -(h + z) - D^H R D written from R
// (read R once, write S^T).
void assembly_enqueue(dwh_ctx* ctx) {
  if (ctx->algo == ALGO_CR) {
    const dwh::CrDims& c = ctx->cr;
    const CrPlan& pl = ctx->plan;
    Scope s(ctx, T_ASSEMBLE,
            (double)pl.fill_step.size() * 8.0 * c.BP * (double)c.BP * c.nbatch + 16.0 * (double)pl.n_ph * c.nbatch);
    dwh::launch_cr_fill(c, ctx->bpool, ctx->d_fill_step, (int)pl.fill_step.size(), ctx->hcol, ctx->hval, ctx->Dcol,
                        ctx->Dsrc, ctx->Delta, ctx->d_y, ctx->d_off_ph, ctx->stream);
  } else {
    const Dims& d = ctx->d;
    Scope s(ctx, T_ASSEMBLE, (double)d.nbatch * 32.0 * d.N * (double)d.N);
    dwh::launch_assemble(d, ctx->R, ctx->S, ctx->Dcol, ctx->Dv, ctx->hcol, ctx->hval, ctx->d_y, ctx->stream);
  }
}

// level-0 blocks -> CR stages -> gather of the selected G entries
void cr_enqueue(dwh_ctx* ctx) {
  const dwh::CrDims& c = ctx->cr;
  const double bp3 = 8.0 * c.BP * (double)c.BP * c.BP * c.nbatch;
  {
    // algorithmic bytes: rewritten level-0 blocks (top halves, none with the
    // out-of-place level-0 inversions) + the pairing entries Δ/2 scattered
    // into the level-0 blocks of every batch item (16 B each)
    // inside a trajectory the previous step's force kernel already scattered
    // the drifted Δ into the pool (pairing_in_pool)
    if (!ctx->pairing_in_pool) assembly_enqueue(ctx);
    ctx->pairing_in_pool = false;
  }
  const CrPlan& plan = ctx->plan;
  // the site guard rides on the first (level-0) inversion launch: every
  // factorised Δ passes through it
  dwh::SiteGuard guard;
  if (ctx->site_guard) guard = dwh::SiteGuard{ctx->Delta, ctx->site4, 4.0 * ctx->delta_cap, ctx->flag};
  for (size_t si = 0; si < plan.stages.size(); ++si) {
    const CrStage& st = plan.stages[si];
    if (st.kind == 0 && st.ntiles > 0) {
      Scope s(ctx, T_CR_INVSIDE, st.n * bp3 + st.flops * c.nbatch);
      dwh::launch_cr_inv_side(c, ctx->bpool, ctx->d_inv_blk + st.first, ctx->d_inv_dst + st.first,
                              ctx->d_inv_slot + st.first, st.n, ctx->ldpart, ctx->d_tasks + st.tfirst,
                              st.ntiles, st.maxt32, ctx->stream, guard, st.store, st.store_side);
      guard = dwh::SiteGuard{};
    } else if (st.kind == 0 && st.l0) {
      Scope s(ctx, T_CR_INV, st.n * bp3);
      dwh::launch_cr_inv0(c, ctx->bpool, ctx->d_inv_blk + st.first, ctx->d_inv0_r, ctx->d_inv_dst + st.first,
                          ctx->d_inv_slot + st.first, st.n, ctx->ldpart, ctx->ldA, ctx->stream, guard.Delta,
                          guard.site4, guard.cap4, guard.flag, st.store);
      guard = dwh::SiteGuard{};
    } else if (st.kind == 0) {
      Scope s(ctx, T_CR_INV, st.n * bp3);
      dwh::launch_cr_inv(c, ctx->bpool, ctx->d_inv_blk + st.first, ctx->d_inv_dst + st.first,
                         ctx->d_inv_slot + st.first, st.n, ctx->ldpart, ctx->stream, guard, st.store);
      guard = dwh::SiteGuard{};
    } else if (st.kind == 2) {
      Scope s(ctx, T_CR_SPARSE, st.flops * c.nbatch);
      const size_t spE = (size_t)dwh::kCrSpNZ * c.BP, HP = (size_t)c.BP / 2;
      if (st.sp == 0)
        dwh::launch_cr_sp_fwd(c, ctx->bpool, ctx->d_sp_rf + st.first * HP, st.n, ctx->d_sp_cv + st.first * 3 * spE,
                              ctx->d_sp_cm + st.first * 3 * spE, ctx->Delta, ctx->stream, st.store);
      else
        dwh::launch_cr_sp_bwd(c, ctx->bpool, ctx->d_sp_rb + st.first * HP, st.n,
                              ctx->d_sp_cv + ctx->sp_arr.col_bwd0 + st.first * 2 * spE,
                              ctx->d_sp_cm + ctx->sp_arr.col_bwd0 + st.first * 2 * spE, ctx->Delta, ctx->stream,
                              st.store);
    } else {
      Scope s(ctx, T_CR_GEMM, st.flops * c.nbatch);
      dwh::launch_cr_gemm(c, ctx->bpool, ctx->d_tasks + st.first, st.n, st.maxt32, st.maxt16,
                          ctx->d_slots + st.sfirst, st.nswg, st.cfg, st.sg, ctx->stream, st.store);
    }
  }
}

dwh::KickDrift kickdrift(dwh_ctx* ctx, double kick, double drift) {
  // the site guard is checked by k_cr_inv0, not per bond by the drift
  const double cap = ctx->site_guard ? std::numeric_limits<double>::infinity() : ctx->delta_cap;
  return dwh::KickDrift{kick, drift, cap, ctx->flag};
}

// algo eig: the library's eigensolver on every chain's H_BdG
// (src/Hamiltonian.jl:96-114), ρ = U diag(f) U^H by one batched product, then
// P, Tr ρ_hh and E_f (src/Observables.jl:14-62, src/HMC.jl:21-27) in
// k_eig_gather
void eig_enqueue(dwh_ctx* ctx) {
  const int N = ctx->d.N, n2 = 2 * N, nc = ctx->d.nc;
  if (int rc = eigen_solve(ctx, chains_src(ctx, 0), nc)) {
    ctx->async_rc = rc;
    return;
  }
  const dwh::TrBufs& b = ctx->tr;
  dwh::launch_eig_scale(b.U, b.JU, b.E, N, nc, ctx->beta, ctx->stream);
  const int64_t sA = (int64_t)n2 * n2;
  // rho = (U f) U^H, the library's own product
  dwh::gemm_z('N', 'C', n2, n2, n2, make_double2(1.0, 0.0), b.JU, n2, sA, b.U, n2, sA, make_double2(0.0, 0.0),
              b.Jmn, n2, sA, nc, ctx->stream);
  if (hipGetLastError() != hipSuccess) {   // a refused launch surfaces at the next eig_check
    ctx->err = "eig path: rho product launch failed";
    ctx->async_rc = DWH_ERR_HIP;
    return;
  }
  dwh::launch_eig_gather(b.Jmn, b.E, N, nc, ctx->Dcol, ctx->bond_ij, ctx->beta, ctx->Pair, ctx->Ef, ctx->Trhh,
                         ctx->stream);
}

// after a stream synchronisation (eig): an enqueue-time refusal, then the
// eigensolver's convergence flags
int eig_check(dwh_ctx* ctx) {
  if (ctx->algo != ALGO_EIG) return DWH_OK;
  if (ctx->async_rc != DWH_OK) {
    const int rc = ctx->async_rc;
    ctx->async_rc = DWH_OK;
    return rc;
  }
  return eigen_info_check(ctx, ctx->d.nc);
}

// assemble -> factorisation -> P -> F (+ kick / next drift); E_f separately
void factorize_enqueue(dwh_ctx* ctx, const dwh::KickDrift& kd) {
  const Dims& d = ctx->d;
  Scope step(ctx, T_STEP, (double)d.nbatch * 8.0 * (double)d.N * d.N * d.N);
  if (ctx->algo == ALGO_EIG) {
    // E_f and Tr ρ_hh come with every decomposition (k_eig_gather)
    eig_enqueue(ctx);
    dwh::launch_force_from_pair(d, ctx->Pair, ctx->Delta, ctx->F, ctx->Pi, kd, ctx->beta, ctx->J, ctx->stream);
    return;
  }
  if (ctx->algo == ALGO_CR) {
    cr_enqueue(ctx);
    // the kernel scatters the drifted Δ into the pool only when it drifts
    ctx->pairing_in_pool = kd.drift != 0.0;
    dwh::launch_cr_pair_force(ctx->cr, ctx->bpool, ctx->d_bond4, ctx->d_c, ctx->Delta, ctx->Pair, ctx->F, ctx->Pi,
                              kd, ctx->beta, ctx->J, ctx->stream, ctx->plan.store_force);
    return;
  }
  dwh::launch_dvals(d, ctx->Dsrc, ctx->Delta, ctx->Dv, ctx->stream);
  assembly_enqueue(ctx);
  run_gj(ctx, ctx->S);
  {
    Scope s(ctx, T_CONTRACT, (double)d.nbatch * 32.0 * d.N * (double)d.N);
    dwh::launch_contract(d, ctx->R, ctx->S, ctx->Dcol, ctx->Dv, ctx->G12nn, ctx->diagS,
                         ctx->stream);
  }
  dwh::launch_pair_force(d, ctx->G12nn, ctx->bond_ij, ctx->bond_ji, ctx->d_c, ctx->Delta,
                         ctx->Pair, ctx->F, ctx->Pi, kd, ctx->beta, ctx->J, ctx->stream);
}

void fermion_energy_enqueue(dwh_ctx* ctx) {
  if (ctx->algo == ALGO_EIG) return;   // written by k_eig_gather with P
  if (ctx->algo == ALGO_CR)
    dwh::launch_cr_fermion_energy(ctx->cr, ctx->bpool, ctx->d_doff, ctx->ldpart, ctx->d_c, ctx->poles.Cx,
                                  ctx->beta, ctx->efpart, ctx->efdone, ctx->Ef, ctx->Trhh, ctx->stream);
  else
    dwh::launch_fermion_energy(ctx->d, ctx->ldstatic, ctx->ldpart, ctx->diagS, ctx->d_c, ctx->poles.Cx,
                               ctx->beta, ctx->Ef, ctx->Trhh, ctx->stream);
}

// Nt against the context's integrator (Nt = 0 is leapfrog's alone), with the
// reason for dwh_last_error
int trajectory_args(dwh_ctx* ctx, int64_t Nt, double dt, double mass) {
  dwh::FlatSchedule f;
  std::string why;
  if (dwh::flatten_schedule(ctx->integ, Nt, dt, mass, &f, &why) != DWH_OK) return fail(ctx, DWH_ERR_ARG, why);
  return DWH_OK;
}

// One hmc_sweep! trajectory reading its draws from device pointers
// (src/HMC.jl:71-122): refresh, H_old, backup, the integrator, H_new.
// The integrator is the context's splitting (dwhmc_integrator.h) flattened
// into one (kick, drift) pair per launch; leapfrog, the default, gives the
// reference's 0.5 dt, dt, ..., 0.5 dt kicks and dt / 2m drifts (:91-118).  The
// caller has checked Nt against the integrator (trajectory_args).
// with_hnew = false: the caller's k_traj_end forms H_new (with the Metropolis test)
void trajectory_enqueue(dwh_ctx* ctx, const double2* noise, int64_t Nt, double dt, double mass,
                        bool with_hnew = true, const dwh::SweepHalt& sh = dwh::SweepHalt{}) {
  const Dims& d = ctx->d;
  hipStream_t s = ctx->stream;
  dwh::FlatSchedule f;
  if (dwh::flatten_schedule(ctx->integ, Nt, dt, mass, &f, nullptr) != DWH_OK) return;
  const int64_t n = f.nfact;
  // :77 refresh, :80 H_old, :84-86 backup, :91-92 first kick fused with the
  // first drift (:101): one launch (k_traj_begin)
  dwh::launch_traj_begin(d, noise, std::sqrt(2.0 * mass), ctx->Pi, ctx->Delta, ctx->Pair, ctx->F, ctx->Ef,
                         ctx->Trhh, ctx->DeltaB, ctx->PairB, ctx->EfB, ctx->TrhhB, ctx->Hold, ctx->beta, ctx->J,
                         mass, kickdrift(ctx, f.kick(0), n > 0 ? f.drift(0) : 0.0), sh, s);
  for (int64_t i = 1; i <= n; ++i) {                                                  // :98
    // :105-107 update_H_BdG! + diagonalize + compute_forces!, then the kick
    // after this force evaluation (:111-113) and the next drift (:101), or
    // the final kick of :118 after the last one
    factorize_enqueue(ctx, kickdrift(ctx, f.kick(i), i < n ? f.drift(i) : 0.0));
  }
  if (n <= 0)
    dwh::launch_force_from_pair(d, ctx->Pair, ctx->Delta, ctx->F, ctx->Pi, kickdrift(ctx, f.kick(1), 0.0),
                                ctx->beta, ctx->J, s);
  else
    fermion_energy_enqueue(ctx);
  if (with_hnew)
    dwh::launch_total_energy(d, ctx->Delta, ctx->Pi, ctx->Ef, ctx->beta, ctx->J, mass,  // :122
                             ctx->Hnew, s);
}

// One hmc_sweep! body (src/HMC.jl:71-144): trajectory, Metropolis, restore.
void sweep_enqueue(dwh_ctx* ctx, const double2* noise, const double* uniform, uint8_t* acc,
                   double* dH, int64_t Nt, double dt, double mass, const dwh::SweepHalt& sh = dwh::SweepHalt{}) {
  const Dims& d = ctx->d;
  hipStream_t s = ctx->stream;
  trajectory_enqueue(ctx, noise, Nt, dt, mass, false, sh);
  // :122 H_new, :124-129 Metropolis, :130-141 restore: one launch
  dwh::launch_traj_end(d, ctx->Delta, ctx->Pi, ctx->Pair, ctx->Ef, ctx->Trhh, ctx->DeltaB, ctx->PairB, ctx->EfB,
                       ctx->TrhhB, ctx->Hold, ctx->Hnew, uniform, acc, dH, ctx->beta, ctx->J, mass, sh, s);
}

// a device buffer holding a host vector; the copy is asynchronous on
// ctx->stream, so the vector has to outlive device_side's synchronisation
template <typename T>
int upload(dwh_ctx* ctx, T** p, const std::vector<T>& v, const char* name) {
  if (int rc = dalloc(ctx, p, v.size())) return rc;
  if (!v.empty() && hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return fail(ctx, DWH_ERR_HIP, std::string("upload ") + name);
  return DWH_OK;
}

// The device side of a context whose host side (model, poles, dimensions,
// plan) is complete: stream, buffers, uploads, the zeroed cache and the static
// initialisation.  On an error the caller destroys the context.
int device_side(dwh_ctx* ctx) {
  const HostModel& m = *ctx->model;
  const Dims& d = ctx->d;
  const int N = d.N;
  const CrPlan& pl = ctx->plan;
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, DWH_ERR_HIP, "hipSetDevice failed");
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(ctx, DWH_ERR_HIP, "hipStreamCreate failed");
  hipStream_t s = ctx->stream;
  const size_t nmat = (size_t)d.nbatch * d.mat;
  const size_t nbond = (size_t)d.nc * 2 * N;
  std::vector<int64_t> bond4;
  int rc = DWH_OK;
#define ALLOC(p, n) \
  if ((rc = dalloc(ctx, &ctx->p, (n))) != DWH_OK) return rc
#define UPLOAD(p, v) \
  if ((rc = upload(ctx, &ctx->p, (v), #p)) != DWH_OK) return rc
  if (ctx->algo == ALGO_DENSE) {
    ALLOC(R, nmat);
    ALLOC(S, nmat);
    const size_t npanel = (size_t)d.nbatch * d.Np * kGJ;
    ALLOC(CpA0, npanel);
    ALLOC(CpA1, npanel);
    ALLOC(CpB, npanel);
    ALLOC(XR1, npanel);
    ALLOC(XR2, npanel);
    ALLOC(Pb1, (size_t)d.nbatch * kGJ * kGJ);
    ALLOC(Pb2, (size_t)d.nbatch * kGJ * kGJ);
    ALLOC(Dv, (size_t)d.nc * N * kSlots);
    ALLOC(G12nn, (size_t)d.nbatch * N * kSlots);
    ALLOC(diagS, (size_t)d.nbatch * N);
  } else if (ctx->algo == ALGO_CR) {
    ALLOC(bpool, (size_t)d.nbatch * ctx->cr.item);
    UPLOAD(d_tasks, pl.tasks);
    UPLOAD(d_slots, pl.slots);
    ctx->sp_arr = cr_sparse_task_arrays(pl, ctx->cr.Lx, ctx->cr.Ly, ctx->cr.BP, m.hcol, m.hval, m.Dcol, m.Dsrc);
    UPLOAD(d_sp_rf, ctx->sp_arr.rf);
    UPLOAD(d_sp_rb, ctx->sp_arr.rb);
    UPLOAD(d_sp_cv, ctx->sp_arr.cv);
    UPLOAD(d_sp_cm, ctx->sp_arr.cm);
    ALLOC(efpart, 2 * (size_t)d.nbatch);
    ALLOC(efdone, (size_t)d.nc);
    UPLOAD(d_inv_blk, pl.inv_blk);
    UPLOAD(d_inv_dst, pl.inv_dst);
    UPLOAD(d_inv_slot, pl.inv_slot);
    UPLOAD(d_inv0_r, pl.inv0_r);
    ALLOC(ldA, (size_t)d.nbatch * ctx->cr.Ly);
    UPLOAD(d_doff, pl.doff);
    UPLOAD(d_off_ph, pl.off_ph);
    // per bond b (2N of them): G12[i, j], G12[j, i] and the pairing entries
    // it writes (Dsrc picks the bond whose value an entry holds)
    bond4.resize(4 * m.bij.size());
    for (size_t b = 0; b < m.bij.size(); ++b) {
      const int e1 = m.bij[b], e2 = m.bji[b];
      bond4[4 * b] = pl.goff[e1];
      bond4[4 * b + 1] = pl.goff[e2];
      bond4[4 * b + 2] = m.Dsrc[e1] == (int)b ? pl.off_ph[e1] : -1;
      bond4[4 * b + 3] = m.Dsrc[e2] == (int)b ? pl.off_ph[e2] : -1;
    }
    UPLOAD(d_bond4, bond4);
    UPLOAD(d_fill_all, pl.fill_all);
    UPLOAD(d_fill_step, pl.fill_step);
  }
  ALLOC(ldpart, (size_t)d.nbatch * d.nld);
  ALLOC(ldstatic, (size_t)d.nbatch);
  UPLOAD(d_y, ctx->poles.y);
  UPLOAD(d_c, ctx->poles.cq);
  UPLOAD(Dcol, m.Dcol);
  UPLOAD(Dsrc, m.Dsrc);
  UPLOAD(hcol, m.hcol);
  UPLOAD(hval, m.hval);
  UPLOAD(bond_ij, m.bij);
  UPLOAD(bond_ji, m.bji);
  ALLOC(Delta, nbond);
  ALLOC(Pi, nbond);
  ALLOC(Pair, nbond);
  ALLOC(F, nbond);
  ALLOC(DeltaB, nbond);
  ALLOC(PairB, nbond);
  ALLOC(Ef, (size_t)d.nc);
  ALLOC(EfB, (size_t)d.nc);
  ALLOC(Trhh, (size_t)d.nc);
  ALLOC(TrhhB, (size_t)d.nc);
  ALLOC(Hold, (size_t)d.nc);
  ALLOC(Hnew, (size_t)d.nc);
  ALLOC(flag, 1);
  ALLOC(halt, 2);
  if (ctx->site_guard) UPLOAD(site4, m.site4);
  ALLOC(s_noise, nbond);
  ALLOC(s_uniform, (size_t)d.nc);
  ALLOC(s_acc, (size_t)d.nc);
  ALLOC(s_dH, (size_t)d.nc);
#undef UPLOAD
#undef ALLOC
  // zeroed cache, like initialize_cache (src/Types.jl:182-212): P = 0, E_f = 0
  for (double2* p : {ctx->Delta, ctx->Pi, ctx->Pair, ctx->F}) (void)hipMemsetAsync(p, 0, nbond * sizeof(double2), s);
  for (double* p : {ctx->Ef, ctx->Trhh}) (void)hipMemsetAsync(p, 0, d.nc * sizeof(double), s);
  if (ctx->efdone) (void)hipMemsetAsync(ctx->efdone, 0, (size_t)d.nc * sizeof(unsigned), s);
  (void)hipMemsetAsync(ctx->flag, 0, sizeof(int), s);
  (void)hipMemsetAsync(ctx->halt, 0, 2 * sizeof(int), s);
  if (ctx->diagS) (void)hipMemsetAsync(ctx->diagS, 0, (size_t)d.nbatch * N * sizeof(double2), s);
  if (ctx->algo == ALGO_DENSE) {
    // static R = (h - i y)^-1 and ln|det(h - i y)| for every (chain, pole)
    dwh::launch_fill_hz(d, ctx->R, ctx->hcol, ctx->hval, ctx->d_y, s);
    run_gj(ctx, ctx->R);
    dwh::launch_sum_ld(d, ctx->ldpart, ctx->ldstatic, s);
  } else if (ctx->algo == ALGO_CR) {
    // the CR path factorises the whole BdG matrix: no static part; every
    // level-0 block written once (pairing entries 0 until the first factorize)
    (void)hipMemsetAsync(ctx->ldstatic, 0, d.nbatch * sizeof(double), s);
    dwh::launch_cr_fill(ctx->cr, ctx->bpool, ctx->d_fill_all, (int)pl.fill_all.size(), ctx->hcol, ctx->hval,
                        ctx->Dcol, ctx->Dsrc, ctx->Delta, ctx->d_y, nullptr, s);
    // static R = A^-1 of the level-0 blocks k_cr_inv0 inverts: the Δ = 0
    // blocks [[A, 0], [0, -conj A]] inverted out of place give [R | 0] and
    // 2 ln|det A| (the pairing entries are still zero here)
    for (const CrStage& st : pl.stages)
      if (st.kind == 0 && st.l0)
        dwh::launch_cr_inv(ctx->cr, ctx->bpool, ctx->d_inv_blk + st.first, ctx->d_inv0_r, ctx->d_inv_slot + st.first,
                           st.n, ctx->ldA, s);
  }
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess)
    return fail(ctx, DWH_ERR_HIP, "static R initialisation failed on the device");
  // eig: rocBLAS handle and the per-chain U, JU (= U diag f), ρ, E buffers
  if (ctx->algo == ALGO_EIG) return transport_prepare(ctx, 0, 0, d.nc);
  return DWH_OK;
}

// A context on `model` for |Δ| within delta_cap (<= 0: the default cap):
// algorithm and guard, poles, plan — all host-only, the context exists only
// once they succeeded — then the device side.  Shared by context creation
// and the pole re-selection, which passes the model it already holds.
int create_on_model(dwh_ctx** out, const std::shared_ptr<const HostModel>& model, double beta, double J,
                    double delta_cap, int32_t algo_req, int32_t device) {
  const HostModel& m = *model;
  AlgoChoice ac;
  if (int rc = choose_algo(algo_req, m.Lx, m.Ly, &ac)) return rc;
  if (delta_cap <= 0) delta_cap = default_delta_cap(beta, J, ac.site_guard);
  PoleChoice pc;
  if (int rc = select_poles(m.hmax, beta, delta_cap, ac.want == DWH_ALGO_EIG, ac.want == DWH_ALGO_AUTO, &pc)) return rc;
  if (ac.want == DWH_ALGO_CR && !ac.cr_ok) return fail(nullptr, DWH_ERR_ARG, "DWHMC_ALGO=cr needs 2*Lx <= 128");
  const int algo = pc.eig ? ALGO_EIG : (ac.want == DWH_ALGO_DENSE || !ac.cr_ok) ? ALGO_DENSE : ALGO_CR;
  Dims d{};
  d.N = m.N;
  d.Np = ((m.N + kGJ - 1) / kGJ) * kGJ;
  d.nb = d.Np / kGJ;
  d.nc = (int)m.nchains;
  d.P = (int)pc.y.size();   // eig: one dummy batch item per chain
  d.nbatch = d.nc * d.P;
  d.mat = (int64_t)d.Np * d.Np;
  d.nld = d.nb;
  CrDims cr{};
  CrPlan plan;
  if (algo == ALGO_CR) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
    if (int rc = plan_cr(m.Lx, m.Ly, d.P, d.nbatch, m.Dcol, m.hcol, kCrFromEnv, kCrFromEnv, ncu, &cr, &plan)) return rc;
    d.nld = cr.Ly;
    cr_plan_dump(plan, d.nbatch, true);
  }
  dwh_ctx* ctx = new dwh_ctx();
  ctx->model = model;
  ctx->device = device;
  ctx->beta = beta;
  ctx->J = J;
  // the eigen path is exact for any Δ: no |Δ| guard
  ctx->delta_cap = pc.eig ? std::numeric_limits<double>::max() : delta_cap;
  ctx->site_guard = ac.site_guard && !pc.eig;
  ctx->poles = std::move(pc);
  ctx->d = d;
  ctx->algo = algo;
  ctx->cr = cr;
  ctx->plan = std::move(plan);
  if (int rc = device_side(ctx)) {
    g_create_error = ctx->err;
    dwh_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return DWH_OK;
}

// validate, device check (no CPU fallback: it precedes every table-derived
// refusal), the lattice model, then create_on_model
int create_impl(dwh_ctx** out, int64_t Lx, int64_t Ly, double t, double tp, double mu, double beta,
                double J, const int64_t* nn, const int64_t* nnn, int64_t nchains,
                const double* disorder, double delta_cap, int32_t algo_req, int32_t device) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "ctx pointer is NULL");
  *out = nullptr;
  // the lattice size before beta and J, the rest of the lattice arguments after: the precedence callers know
  if (Lx < 1 || Ly < 1) return fail(nullptr, DWH_ERR_ARG, "Lx, Ly must be >= 1");
  if (!(beta > 0)) return fail(nullptr, DWH_ERR_ARG, "beta must be > 0");
  if (J == 0 || !std::isfinite(J)) return fail(nullptr, DWH_ERR_ARG, "J must be finite and nonzero");
  if (int rc = check_lattice_args(Lx, Ly, nchains, nn, nnn, disorder)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(nullptr, DWH_ERR_HIP, "no HIP device available (the fermion path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, DWH_ERR_ARG, "device index out of range");
  const auto model = std::make_shared<HostModel>();
  if (int rc = build_host_model(Lx, Ly, t, tp, mu, nn, nnn, nchains, disorder, model.get())) return rc;
  return create_on_model(out, model, beta, J, delta_cap, algo_req, device);
}

}  // namespace

extern "C" {

int dwh_create(dwh_ctx** ctx, int64_t Lx, int64_t Ly, double t, double tp, double mu, double beta,
               double J, const int64_t* nn_table, const int64_t* nnn_table, const double* disorder,
               int32_t device) {
  return create_impl(ctx, Lx, Ly, t, tp, mu, beta, J, nn_table, nnn_table, 1, disorder, 0.0,
                     DWH_ALGO_AUTO, device);
}

int dwh_create_batched(dwh_ctx** ctx, int64_t Lx, int64_t Ly, double t, double tp, double mu,
                       double beta, double J, const int64_t* nn_table, const int64_t* nnn_table,
                       int64_t nchains, const double* disorder, double delta_cap, int32_t device) {
  return create_impl(ctx, Lx, Ly, t, tp, mu, beta, J, nn_table, nnn_table, nchains, disorder,
                     delta_cap, DWH_ALGO_AUTO, device);
}

int dwh_create_ex(dwh_ctx** ctx, int64_t Lx, int64_t Ly, double t, double tp, double mu, double beta,
                  double J, const int64_t* nn_table, const int64_t* nnn_table, int64_t nchains,
                  const double* disorder, double delta_cap, int32_t algo, int32_t device) {
  if (algo != DWH_ALGO_AUTO && algo != DWH_ALGO_DENSE && algo != DWH_ALGO_CR && algo != DWH_ALGO_EIG)
    return fail(nullptr, DWH_ERR_ARG, "algo must be DWH_ALGO_AUTO, DWH_ALGO_DENSE, DWH_ALGO_CR or DWH_ALGO_EIG");
  return create_impl(ctx, Lx, Ly, t, tp, mu, beta, J, nn_table, nnn_table, nchains, disorder,
                     delta_cap, algo, device);
}

void dwh_destroy(dwh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& r : ctx->recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : ctx->pool) (void)hipEventDestroy(e);
  if (ctx->blas) (void)rocblas_destroy_handle(ctx->blas);
  for (void* p : ctx->allocations) (void)hipFree(p);
  for (hipEvent_t ev : ctx->eig_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t st : ctx->eig_sx)
    if (st) (void)hipStreamDestroy(st);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* dwh_last_error(const dwh_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int dwh_info(dwh_ctx* ctx, dwh_info_t* out) {
  if (!ctx || !out) return DWH_ERR_ARG;
  out->N = ctx->d.N;
  out->Np = ctx->d.Np;
  out->nchains = ctx->d.nc;
  out->npoles = ctx->algo == ALGO_EIG ? 0 : ctx->d.P;
  out->kappa = ctx->poles.kappa;
  out->e_bound = ctx->poles.Ep;
  out->err_tanh = ctx->poles.err_tanh;
  out->delta_cap = ctx->delta_cap;
  out->device_bytes = ctx->device_bytes;
  out->algo = ctx->algo;
  out->block = ctx->algo == ALGO_CR ? ctx->cr.BP : ctx->algo == ALGO_EIG ? 0 : kGJ;
  out->eig_half = ctx->eig_ph_last;
  out->eig_long_clusters = ctx->eig_long_clusters;
  out->eig_quat = ctx->eig_quat_last;
  return DWH_OK;
}

int dwh_debug_cr_stamps(dwh_ctx* ctx, int32_t inv_stage, uint64_t* out, int64_t nwg) {
  if (!ctx || !out || nwg < 1) return fail(ctx, DWH_ERR_ARG, "dwh_debug_cr_stamps: bad argument");
  if (ctx->algo != ALGO_CR) return fail(ctx, DWH_ERR_STATE, "dwh_debug_cr_stamps: CR path only");
#ifdef CR_STAMPS
  int key = -1, k = 0;
  for (const CrStage& st : ctx->plan.stages)
    if (st.kind == 0 && k++ == inv_stage) key = ctx->plan.inv_blk[st.first];
  if (key < 0) return fail(ctx, DWH_ERR_ARG, "dwh_debug_cr_stamps: no such inversion stage");
  if (int rc = settle(ctx)) return rc;
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (dwh::cr_stamps_arm(key) != 0) return fail(ctx, DWH_ERR_HIP, "dwh_debug_cr_stamps: arm");
  cr_enqueue(ctx);
  HIPCHECK(ctx, hipGetLastError());
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (dwh::cr_stamps_arm(-1) != 0 ||
      dwh::cr_stamps_read(reinterpret_cast<unsigned long long*>(out), (int)std::min<int64_t>(nwg, dwh::kCrStampWG)) != 0)
    return fail(ctx, DWH_ERR_HIP, "dwh_debug_cr_stamps: read");
  return DWH_OK;
#else
  (void)inv_stage;
  return fail(ctx, DWH_ERR_STATE, "dwh_debug_cr_stamps: not a -DCR_STAMPS build");
#endif
}

int dwh_bench_assembly(dwh_ctx* ctx, int64_t reps) {
  if (!ctx || reps < 0) return fail(ctx, DWH_ERR_ARG, "dwh_bench_assembly: bad argument");
  if (ctx->algo == ALGO_EIG) return fail(ctx, DWH_ERR_STATE, "dwh_bench_assembly: the eig path has no per-step assembly");
  if (int rc = settle(ctx)) return rc;
  for (int64_t r = 0; r < reps; ++r) assembly_enqueue(ctx);
  HIPCHECK(ctx, hipGetLastError());
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

}  // extern "C"

namespace {

// Re-create the device side of `ctx` for |Δ_ij| <= new_cap: a new pole-table
// entry for the larger spectral bound E' = hmax + 2 new_cap and the plan for
// its pole count, on the lattice model the context already holds (same
// tables, ‖h‖ bound and algorithm); Δ, π, the throughput draws and the
// timing state carry over.  The context is left unfactorised.
int reselect_poles(dwh_ctx* ctx, double new_cap) {
  dwh_ctx* n = nullptr;
  const int32_t algo = ctx->algo == ALGO_CR ? DWH_ALGO_CR : ctx->algo == ALGO_EIG ? DWH_ALGO_EIG : DWH_ALGO_DENSE;
  int rc = create_on_model(&n, ctx->model, ctx->beta, ctx->J, new_cap, algo, ctx->device);
  // a spectral bound beyond the pole table: the eigendecomposition path
  if (rc == DWH_ERR_TABLE) rc = create_on_model(&n, ctx->model, ctx->beta, ctx->J, new_cap, DWH_ALGO_EIG, ctx->device);
  if (rc != DWH_OK)
    return fail(ctx, rc, "pole re-selection for delta_cap=" + std::to_string(new_cap) + ": " + g_create_error);
  const size_t nb = (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(n->Delta, ctx->Delta, nb, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(n->Pi, ctx->Pi, nb, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) {
    dwh_destroy(n);
    return fail(ctx, DWH_ERR_HIP, std::string("pole re-selection: ") + hipGetErrorString(e));
  }
  // the throughput draws move with the context
  const size_t nbond = (size_t)ctx->d.nc * 2 * ctx->d.N, nc = ctx->d.nc, ns = (size_t)ctx->ndraws;
  auto move = [&](void* p, size_t bytes) {
    if (!p) return;
    auto it = std::find(ctx->allocations.begin(), ctx->allocations.end(), p);
    if (it != ctx->allocations.end()) ctx->allocations.erase(it);
    bytes = std::max<size_t>(bytes, 1);
    ctx->device_bytes -= (int64_t)bytes;
    n->allocations.push_back(p);
    n->device_bytes += (int64_t)bytes;
  };
  move(ctx->noise, nbond * ns * sizeof(double2));
  move(ctx->uniform, nc * ns * sizeof(double));
  move(ctx->acc, nc * ns);
  move(ctx->dH, nc * ns * sizeof(double));
  n->noise = ctx->noise;
  n->uniform = ctx->uniform;
  n->acc = ctx->acc;
  n->dH = ctx->dH;
  n->ndraws = ctx->ndraws;
  ctx->noise = nullptr;
  ctx->uniform = nullptr;
  ctx->acc = nullptr;
  ctx->dH = nullptr;
  ctx->ndraws = 0;
  dwh::sweep_log_move(ctx, n);
  n->timing = ctx->timing;
  std::copy(ctx->t_ms, ctx->t_ms + T_COUNT, n->t_ms);
  std::copy(ctx->t_n, ctx->t_n + T_COUNT, n->t_n);
  std::copy(ctx->t_work, ctx->t_work + T_COUNT, n->t_work);
  n->reselections = ctx->reselections + 1;
  n->integ = ctx->integ;   // dwh_set_integrator's setting outlives the pole set
  // the context keeps its stream (a handle from dwh_stream stays valid); the
  // new device side's stream goes with the old one
  (void)hipStreamSynchronize(n->stream);
  std::swap(n->stream, ctx->stream);
  std::swap(*ctx, *n);
  if (ctx->blas) (void)rocblas_set_stream(ctx->blas, ctx->stream);
  dwh_destroy(n);
  return DWH_OK;
}

// Host-side guard for an uploaded Δ: re-select the poles when max|Δ_ij| (bond
// guard) or the largest mean |Δ| over a site's bonds (site guard) is above
// the cap (the reference accepts any Δ, src/HMC.jl:98-114).
int fit_cap(dwh_ctx* ctx, const dwh_c128* D, size_t n, bool* reselected = nullptr) {
  if (reselected) *reselected = false;
  double m = 0;
  for (size_t k = 0; k < n; ++k) {
    const double a = std::hypot(D[k].re, D[k].im);
    if (!std::isfinite(a)) return fail(ctx, DWH_ERR_ARG, "non-finite Delta");
    m = std::max(m, a);
  }
  if (ctx->site_guard) {
    const size_t N = (size_t)ctx->d.N, nc = n / (2 * N);
    m = 0;
    for (size_t c = 0; c < nc; ++c)
      for (size_t i = 0; i < N; ++i) {
        double sm = 0;
        for (int k = 0; k < 4; ++k) {
          const dwh_c128 v = D[c * 2 * N + ctx->model->site4[4 * i + k]];
          sm += std::hypot(v.re, v.im);
        }
        m = std::max(m, 0.25 * sm);
      }
  }
  if (m <= ctx->delta_cap) return DWH_OK;
  if (reselected) *reselected = true;
  return reselect_poles(ctx, std::max(2.0 * ctx->delta_cap, 1.5 * m));
}

// Reads and clears the device guard flag (set by the drift kernels when
// max|Δ_ij| > delta_cap).
int take_flag(dwh_ctx* ctx, int* f) {
  *f = 0;
  HIPCHECK(ctx, hipMemcpyAsync(f, ctx->flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (*f) HIPCHECK(ctx, hipMemsetAsync(ctx->flag, 0, sizeof(int), ctx->stream));
  return DWH_OK;
}

// A sweep drifted |Δ| past the cap, so its forces used poles not valid for
// its spectrum: back to the sweep's starting point (Δ backed up by k_backup,
// src/HMC.jl:84), re-select the poles for twice the cap and refactorise, so
// the caller can run the same sweep again.
constexpr int kMaxReselect = 12;
int redo_after_guard(dwh_ctx* ctx, int attempt) {
  if (attempt >= kMaxReselect)
    return fail(ctx, DWH_ERR_SPECTRUM, "|Delta_ij| kept exceeding the re-selected pole sets");
  const size_t nb = (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2);
  HIPCHECK(ctx, hipMemcpyAsync(ctx->Delta, ctx->DeltaB, nb, hipMemcpyDeviceToDevice, ctx->stream));
  int rc = reselect_poles(ctx, 2.0 * ctx->delta_cap);
  if (rc != DWH_OK) return rc;
  return dwh_factorize(ctx);
}

// one logged throughput sweep (sequence number = its index in ctx->enq)
void enqueue_logged(dwh_ctx* ctx, int64_t sw, int64_t Nt, double dt, double mass) {
  const Dims& d = ctx->d;
  const size_t nbond = (size_t)d.nc * 2 * d.N;
  const dwh::SweepHalt sh{ctx->halt, (int)ctx->enq.size(), ctx->flag};
  ctx->enq.push_back({sw, Nt, dt, mass});
  sweep_enqueue(ctx, ctx->noise + nbond * sw, ctx->uniform + (size_t)d.nc * sw, ctx->acc + (size_t)d.nc * sw,
                ctx->dH + (size_t)d.nc * sw, Nt, dt, mass, sh);
  if (ctx->log_what) dwh::sweep_log_enqueue(ctx, sw);
}

}  // namespace

// Waits for the enqueued throughput sweeps.  A guard trip in one of them
// (k_traj_end recorded its sequence number t, every later sweep of the batch
// was a no-op that kept the backups): Δ back to sweep t's start, poles
// re-selected for twice the cap, refactorised — exactly what dwh_hmc_sweep
// does for a trip — and sweeps t.. enqueued again, until a pass ends without
// a trip.  The results then equal the single-sweep path's bit for bit.
int dwh::settle(dwh_ctx* ctx) {
  for (int attempt = 0;; ++attempt) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = eig_check(ctx)) return rc;
    int f = 0;
    if (int rc = take_flag(ctx, &f)) return rc;
    if (!f) {
      ctx->enq.clear();
      return DWH_OK;
    }
    int h[2] = {0, 0};
    HIPCHECK(ctx, hipMemcpy(h, ctx->halt, sizeof h, hipMemcpyDeviceToHost));
    if (!h[0] || h[1] < 0 || h[1] >= (int)ctx->enq.size()) {
      ctx->enq.clear();
      char buf[256];
      std::snprintf(buf, sizeof buf,
                    "%s exceeded delta_cap=%g outside a logged sweep (the pole set was built for spectra "
                    "within E'=%g)",
                    ctx->site_guard ? "the mean |Delta| of a site's bonds" : "|Delta_ij|", ctx->delta_cap,
                    ctx->poles.Ep);
      return fail(ctx, DWH_ERR_SPECTRUM, buf);
    }
    const std::vector<dwh_ctx::EnqSweep> rest(ctx->enq.begin() + h[1], ctx->enq.end());
    ctx->enq.clear();
    HIPCHECK(ctx, hipMemsetAsync(ctx->halt, 0, 2 * sizeof(int), ctx->stream));
    if (int rc = redo_after_guard(ctx, attempt)) return rc;
    for (const auto& e : rest) enqueue_logged(ctx, e.sweep, e.Nt, e.dt, e.mass);
    HIPCHECK(ctx, hipGetLastError());
  }
}

extern "C" {

int dwh_update_pairing(dwh_ctx* ctx, const dwh_c128* Delta) {
  if (!ctx || !Delta) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  if (int rc = fit_cap(ctx, Delta, (size_t)ctx->d.nc * 2 * ctx->d.N)) return rc;
  HIPCHECK(ctx, hipMemcpyAsync(ctx->Delta, Delta, (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2),
                               hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_factorize(dwh_ctx* ctx) {
  if (!ctx) return DWH_ERR_ARG;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  factorize_enqueue(ctx, kickdrift(ctx, 0.0, 0.0));
  fermion_energy_enqueue(ctx);
  HIPCHECK(ctx, hipGetLastError());
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = eig_check(ctx)) return rc;
  ctx->factorized = true;
  drain_timing(ctx);
  return DWH_OK;
}

int dwh_forces(dwh_ctx* ctx, const dwh_c128* Delta, dwh_c128* F_out) {
  if (!ctx || !F_out) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const size_t nb = (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2);
  if (Delta)
    HIPCHECK(ctx, hipMemcpyAsync(ctx->DeltaB, Delta, nb, hipMemcpyHostToDevice, ctx->stream));
  dwh::launch_force_from_pair(ctx->d, ctx->Pair, Delta ? ctx->DeltaB : ctx->Delta, ctx->F, ctx->Pi,
                              kickdrift(ctx, 0.0, 0.0), ctx->beta, ctx->J, ctx->stream);
  HIPCHECK(ctx, hipMemcpyAsync(F_out, ctx->F, nb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_pairing(dwh_ctx* ctx, dwh_c128* P_out) {
  if (!ctx || !P_out) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  HIPCHECK(ctx, hipMemcpyAsync(P_out, ctx->Pair, (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2),
                               hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_fermion_energy(dwh_ctx* ctx, double* Ef) {
  if (!ctx || !Ef) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  HIPCHECK(ctx, hipMemcpyAsync(Ef, ctx->Ef, ctx->d.nc * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_hole_trace(dwh_ctx* ctx, double* tr) {
  if (!ctx || !tr) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  HIPCHECK(ctx, hipMemcpyAsync(tr, ctx->Trhh, ctx->d.nc * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_total_energy(dwh_ctx* ctx, double mass, double* H) {
  if (!ctx || !H) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  dwh::launch_total_energy(ctx->d, ctx->Delta, ctx->Pi, ctx->Ef, ctx->beta, ctx->J, mass, ctx->Hnew,
                           ctx->stream);
  HIPCHECK(ctx, hipMemcpyAsync(H, ctx->Hnew, ctx->d.nc * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_set_state(dwh_ctx* ctx, const dwh_c128* Delta, const dwh_c128* pi) {
  if (!ctx) return DWH_ERR_ARG;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const size_t nb = (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2);
  bool reselected = false;
  if (Delta)
    if (int rc = fit_cap(ctx, Delta, (size_t)ctx->d.nc * 2 * ctx->d.N, &reselected)) return rc;
  if (Delta) HIPCHECK(ctx, hipMemcpyAsync(ctx->Delta, Delta, nb, hipMemcpyHostToDevice, ctx->stream));
  if (pi) HIPCHECK(ctx, hipMemcpyAsync(ctx->Pi, pi, nb, hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  // a re-selected context has no factorisation yet: the cached P / E_f the next
  // sweep starts from must belong to this Δ
  if (reselected) return dwh_factorize(ctx);
  return DWH_OK;
}

int dwh_get_state(dwh_ctx* ctx, dwh_c128* Delta, dwh_c128* pi) {
  if (!ctx) return DWH_ERR_ARG;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const size_t nb = (size_t)ctx->d.nc * 2 * ctx->d.N * sizeof(double2);
  if (Delta) HIPCHECK(ctx, hipMemcpyAsync(Delta, ctx->Delta, nb, hipMemcpyDeviceToHost, ctx->stream));
  if (pi) HIPCHECK(ctx, hipMemcpyAsync(pi, ctx->Pi, nb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_hmc_sweep(dwh_ctx* ctx, const dwh_c128* noise, const double* uniform, int64_t Nt, double dt,
                  double mass, uint8_t* accepted, double* dH) {
  if (!ctx || !noise || !uniform || !accepted || !dH) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (Nt < 0 || !(mass > 0) || !std::isfinite(dt)) return fail(ctx, DWH_ERR_ARG, "bad Nt/dt/mass");
  if (int rc = trajectory_args(ctx, Nt, dt, mass)) return rc;
  if (ctx->pending) return fail(ctx, DWH_ERR_STATE, "dwh_hmc_finish the pending trajectory first");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->enq.empty())
    if (int rc = settle(ctx)) return rc;
  for (int attempt = 0;; ++attempt) {
    const Dims& d = ctx->d;
    HIPCHECK(ctx, hipMemcpyAsync(ctx->s_noise, noise, (size_t)d.nc * 2 * d.N * sizeof(double2),
                                 hipMemcpyHostToDevice, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(ctx->s_uniform, uniform, d.nc * sizeof(double), hipMemcpyHostToDevice,
                                 ctx->stream));
    sweep_enqueue(ctx, ctx->s_noise, ctx->s_uniform, ctx->s_acc, ctx->s_dH, Nt, dt, mass);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipMemcpyAsync(accepted, ctx->s_acc, d.nc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(dH, ctx->s_dH, d.nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = eig_check(ctx)) return rc;
    if (Nt > 0) ctx->factorized = true;
    drain_timing(ctx);
    int f = 0;
    if (int rc = take_flag(ctx, &f)) return rc;
    if (!f) return DWH_OK;
    if (int rc = redo_after_guard(ctx, attempt)) return rc;
  }
}

int dwh_hmc_trajectory(dwh_ctx* ctx, const dwh_c128* noise, int64_t Nt, double dt, double mass,
                       double* dH) {
  if (!ctx || !noise || !dH) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (Nt < 0 || !(mass > 0) || !std::isfinite(dt)) return fail(ctx, DWH_ERR_ARG, "bad Nt/dt/mass");
  if (int rc = trajectory_args(ctx, Nt, dt, mass)) return rc;
  if (ctx->pending) return fail(ctx, DWH_ERR_STATE, "dwh_hmc_finish the pending trajectory first");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->enq.empty())
    if (int rc = settle(ctx)) return rc;
  for (int attempt = 0;; ++attempt) {
    const Dims& d = ctx->d;
    HIPCHECK(ctx, hipMemcpyAsync(ctx->s_noise, noise, (size_t)d.nc * 2 * d.N * sizeof(double2),
                                 hipMemcpyHostToDevice, ctx->stream));
    // ΔH by the Metropolis kernel's own arithmetic (src/HMC.jl:124), with a
    // uniform of 2 > exp(-ΔH) for ΔH >= 0: its accept flags are not used
    std::vector<double> two((size_t)d.nc, 2.0);
    HIPCHECK(ctx, hipMemcpyAsync(ctx->s_uniform, two.data(), d.nc * sizeof(double), hipMemcpyHostToDevice,
                                 ctx->stream));
    trajectory_enqueue(ctx, ctx->s_noise, Nt, dt, mass);
    dwh::launch_metropolis(d, ctx->Hold, ctx->Hnew, ctx->s_uniform, ctx->s_acc, ctx->s_dH, ctx->stream);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipMemcpyAsync(dH, ctx->s_dH, d.nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = eig_check(ctx)) return rc;
    if (Nt > 0) ctx->factorized = true;
    drain_timing(ctx);
    int f = 0;
    if (int rc = take_flag(ctx, &f)) return rc;
    if (!f) {
      ctx->pending = true;
      return DWH_OK;
    }
    if (int rc = redo_after_guard(ctx, attempt)) return rc;
  }
}

int dwh_hmc_finish(dwh_ctx* ctx, const uint8_t* accepted) {
  if (!ctx || !accepted) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (!ctx->pending) return fail(ctx, DWH_ERR_STATE, "no pending trajectory (dwh_hmc_trajectory first)");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  const Dims& d = ctx->d;
  HIPCHECK(ctx, hipMemcpyAsync(ctx->s_acc, accepted, d.nc, hipMemcpyHostToDevice, ctx->stream));
  dwh::launch_restore(d, ctx->s_acc, ctx->DeltaB, ctx->PairB, ctx->EfB, ctx->TrhhB, ctx->Delta,  // :130-141
                      ctx->Pair, ctx->Ef, ctx->Trhh, ctx->stream);
  HIPCHECK(ctx, hipGetLastError());
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->pending = false;
  return DWH_OK;
}

int dwh_set_integrator(dwh_ctx* ctx, int32_t kind, double lambda, int64_t nstage, const double* kick,
                       const double* drift) {
  if (!ctx) return DWH_ERR_ARG;
  if (ctx->pending) return fail(ctx, DWH_ERR_STATE, "dwh_hmc_finish the pending trajectory first");
  dwh::Integrator integ;
  std::string why;
  if (dwh::make_integrator(kind, lambda, nstage, kick, drift, &integ, &why) != DWH_OK)
    return fail(ctx, DWH_ERR_ARG, why);
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  // enqueued throughput sweeps run, and after a guard trip replay, with the
  // schedule they were enqueued under
  SETTLE(ctx);
  ctx->integ = integ;
  return DWH_OK;
}

int dwh_get_integrator(dwh_ctx* ctx, int32_t* kind, double* lambda, int64_t* nstage, double* kick, double* drift) {
  if (!ctx) return DWH_ERR_ARG;
  const dwh::Integrator& g = ctx->integ;
  if (kind) *kind = g.kind;
  if (lambda) *lambda = g.lambda;
  if (nstage) *nstage = g.stages();
  if (kick) std::copy(g.kick.begin(), g.kick.end(), kick);
  if (drift) std::copy(g.drift.begin(), g.drift.end(), drift);
  return DWH_OK;
}

int dwh_load_draws(dwh_ctx* ctx, int64_t nsweeps, const dwh_c128* noise, const double* uniform) {
  if (!ctx || nsweeps < 1 || !noise || !uniform) return fail(ctx, DWH_ERR_ARG, "bad argument");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  // pending throughput sweeps replay from the loaded draws after a guard trip
  // (settle): finish them before the draws are replaced
  SETTLE(ctx);
  const Dims& d = ctx->d;
  const size_t nbond = (size_t)d.nc * 2 * d.N;
  if (nsweeps > ctx->ndraws) {
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    auto drop = [&](void* p, size_t bytes) {
      if (!p) return;
      auto it = std::find(ctx->allocations.begin(), ctx->allocations.end(), p);
      if (it != ctx->allocations.end()) ctx->allocations.erase(it);
      ctx->device_bytes -= (int64_t)std::max<size_t>(bytes, 1);
      (void)hipFree(p);
    };
    // allocate the new buffers first and swap them in only when all of them
    // exist, so a failed allocation leaves the old draws (and ndraws) intact
    double2* nz = nullptr;
    double* un = nullptr;
    uint8_t* ac = nullptr;
    double* dh = nullptr;
    const size_t ns = (size_t)nsweeps, nc = (size_t)d.nc;
    int rc = dalloc(ctx, &nz, nbond * ns);
    if (rc == DWH_OK) rc = dalloc(ctx, &un, nc * ns);
    if (rc == DWH_OK) rc = dalloc(ctx, &ac, nc * ns);
    if (rc == DWH_OK) rc = dalloc(ctx, &dh, nc * ns);
    const size_t old = (size_t)ctx->ndraws;
    if (rc != DWH_OK) {
      drop(nz, nbond * ns * sizeof(double2));
      drop(un, nc * ns * sizeof(double));
      drop(ac, nc * ns);
      drop(dh, nc * ns * sizeof(double));
      return rc;
    }
    drop(ctx->noise, nbond * old * sizeof(double2));
    drop(ctx->uniform, nc * old * sizeof(double));
    drop(ctx->acc, nc * old);
    drop(ctx->dH, nc * old * sizeof(double));
    ctx->noise = nz;
    ctx->uniform = un;
    ctx->acc = ac;
    ctx->dH = dh;
    ctx->ndraws = nsweeps;
    // the log grows with the draws and starts from zero
    if (int rc2 = dwh::sweep_log_resize(ctx)) return rc2;
  }
  HIPCHECK(ctx, hipMemcpyAsync(ctx->noise, noise, nbond * nsweeps * sizeof(double2),
                               hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(ctx->uniform, uniform, (size_t)d.nc * nsweeps * sizeof(double),
                               hipMemcpyHostToDevice, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_run_sweeps(dwh_ctx* ctx, int64_t first, int64_t nsweeps, int64_t Nt, double dt, double mass) {
  if (!ctx) return DWH_ERR_ARG;
  if (first < 0 || nsweeps < 0 || first + nsweeps > ctx->ndraws)
    return fail(ctx, DWH_ERR_ARG, "sweep range outside the loaded draws");
  if (Nt < 0 || !(mass > 0)) return fail(ctx, DWH_ERR_ARG, "bad Nt/mass");
  if (int rc = trajectory_args(ctx, Nt, dt, mass)) return rc;
  if (ctx->pending) return fail(ctx, DWH_ERR_STATE, "dwh_hmc_finish the pending trajectory first");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  const Dims& d = ctx->d;
  const size_t nbond = (size_t)d.nc * 2 * d.N;
  (void)d;
  (void)nbond;
  for (int64_t sw = first; sw < first + nsweeps; ++sw) enqueue_logged(ctx, sw, Nt, dt, mass);
  HIPCHECK(ctx, hipGetLastError());
  if (Nt > 0 && nsweeps > 0) ctx->factorized = true;
  return DWH_OK;
}

int dwh_sweep_results(dwh_ctx* ctx, int64_t first, int64_t nsweeps, uint8_t* accepted, double* dH) {
  if (!ctx) return DWH_ERR_ARG;
  if (first < 0 || nsweeps < 0 || first + nsweeps > ctx->ndraws)
    return fail(ctx, DWH_ERR_ARG, "sweep range outside the loaded draws");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  if (int rc = settle(ctx)) return rc;
  const size_t nc = ctx->d.nc;
  if (accepted)
    HIPCHECK(ctx, hipMemcpyAsync(accepted, ctx->acc + nc * first, nc * nsweeps, hipMemcpyDeviceToHost,
                                 ctx->stream));
  if (dH)
    HIPCHECK(ctx, hipMemcpyAsync(dH, ctx->dH + nc * first, nc * nsweeps * sizeof(double),
                                 hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_synchronize(dwh_ctx* ctx) {
  if (!ctx) return DWH_ERR_ARG;
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  if (int rc = settle(ctx)) return rc;
  HIPCHECK(ctx, hipGetLastError());
  drain_timing(ctx);
  return DWH_OK;
}

int dwh_stream(dwh_ctx* ctx, void** stream) {
  if (!ctx || !stream) return DWH_ERR_ARG;
  *stream = (void*)ctx->stream;
  return DWH_OK;
}

int dwh_timing_enable(dwh_ctx* ctx, int32_t enable) {
  if (!ctx) return DWH_ERR_ARG;
  drain_timing(ctx);
  ctx->timing = enable;
  return DWH_OK;
}

int dwh_timing_read(dwh_ctx* ctx, const char* name, double* total_ms, int64_t* launches,
                    double* work) {
  if (!ctx || !name) return DWH_ERR_ARG;
  drain_timing(ctx);
  for (int i = 0; i < T_COUNT; ++i)
    if (std::strcmp(name, kTimerNames[i]) == 0) {
      if (total_ms) *total_ms = ctx->t_ms[i];
      if (launches) *launches = ctx->t_n[i];
      if (work) *work = ctx->t_work[i];
      return DWH_OK;
    }
  return fail(ctx, DWH_ERR_ARG, std::string("unknown timer ") + name);
}

int dwh_timing_reset(dwh_ctx* ctx) {
  if (!ctx) return DWH_ERR_ARG;
  drain_timing(ctx);
  for (int i = 0; i < T_COUNT; ++i) {
    ctx->t_ms[i] = 0;
    ctx->t_n[i] = 0;
    ctx->t_work[i] = 0;
  }
  return DWH_OK;
}

int dwh_selftest_mfma(int32_t device) { return dwh::selftest_mfma_layout(device); }

int dwh_debug_gemm(int32_t device, int32_t cplx, char opa, char opb, int64_t M, int64_t N, int64_t K,
                   const double* alpha, const void* A, int64_t lda, const void* B, int64_t ldb, const double* beta,
                   void* C, int64_t ldc, int64_t batch) {
  if (M < 1 || N < 1 || K < 0 || batch < 1 || !alpha || !beta || !A || !B || !C)
    return fail(nullptr, DWH_ERR_ARG, "bad gemm arguments");
  if ((opa != 'N' && opa != 'C') || (opb != 'N' && opb != 'C'))
    return fail(nullptr, DWH_ERR_ARG, "op must be 'N' or 'C'");
  const int64_t acols = opa == 'N' ? K : M, bcols = opb == 'N' ? N : K;
  const int64_t arows = opa == 'N' ? M : K, brows = opb == 'N' ? K : N;
  if (lda < std::max<int64_t>(1, arows) || ldb < std::max<int64_t>(1, brows) || ldc < M)
    return fail(nullptr, DWH_ERR_ARG, "leading dimension too small");
  const size_t es = cplx ? sizeof(double2) : sizeof(double);
  const int64_t sA = lda * std::max<int64_t>(acols, 1), sB = ldb * std::max<int64_t>(bcols, 1), sC = ldc * N;
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, DWH_ERR_HIP, "hipSetDevice failed");
  void *dA = nullptr, *dB = nullptr, *dC = nullptr;
  auto cleanup = [&]() {
    (void)hipFree(dA);
    (void)hipFree(dB);
    (void)hipFree(dC);
  };
  if (hipMalloc(&dA, es * sA * batch) != hipSuccess || hipMalloc(&dB, es * sB * batch) != hipSuccess ||
      hipMalloc(&dC, es * sC * batch) != hipSuccess) {
    cleanup();
    return fail(nullptr, DWH_ERR_HIP, "hipMalloc (gemm test buffers)");
  }
  hipError_t e = hipMemcpy(dA, A, es * sA * batch, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dB, B, es * sB * batch, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dC, C, es * sC * batch, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (cplx)
      dwh::gemm_z(opa, opb, (int)M, (int)N, (int)K, make_double2(alpha[0], alpha[1]), (const double2*)dA, (int)lda,
                  sA, (const double2*)dB, (int)ldb, sB, make_double2(beta[0], beta[1]), (double2*)dC, (int)ldc, sC,
                  (int)batch, nullptr);
    else
      dwh::gemm_d(opa == 'C' ? 'T' : 'N', opb == 'C' ? 'T' : 'N', (int)M, (int)N, (int)K, alpha[0],
                  (const double*)dA, (int)lda, sA, (const double*)dB, (int)ldb, sB, beta[0], (double*)dC, (int)ldc,
                  sC, (int)batch, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(C, dC, es * sC * batch, hipMemcpyDeviceToHost);
  cleanup();
  if (e != hipSuccess) return fail(nullptr, DWH_ERR_HIP, std::string("gemm test: ") + hipGetErrorString(e));
  return DWH_OK;
}

// ---- assembly read-back (parity tests of init_static_H! / update_H_BdG!) ----

int dwh_debug_dense_H(dwh_ctx* ctx, int64_t chain, dwh_c128* H) {
  if (!ctx || !H) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (chain < 0 || chain >= ctx->d.nc) return fail(ctx, DWH_ERR_ARG, "chain index out of range");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  const int N = ctx->d.N;
  const size_t n2 = 2 * (size_t)N;
  double2* A = nullptr;
  HIPCHECK(ctx, hipMalloc(&A, n2 * n2 * sizeof(double2)));
  // the eigen path's assembly (eigen_enqueue): zero, then k_tr_assemble
  hipError_t e = hipMemsetAsync(A, 0, n2 * n2 * sizeof(double2), ctx->stream);
  if (e == hipSuccess) {
    dwh::launch_tr_assemble(A, N, ctx->hcol, ctx->hval + (size_t)chain * N * kHSlots, ctx->Dcol, ctx->Dsrc,
                            ctx->Delta + (size_t)chain * 2 * N, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(H, A, n2 * n2 * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(A);
  if (e != hipSuccess) return fail(ctx, DWH_ERR_HIP, std::string("dense H read-back: ") + hipGetErrorString(e));
  return DWH_OK;
}

int dwh_debug_level0(dwh_ctx* ctx, int64_t chain, int64_t pole, int32_t refill, dwh_c128* M, double* y) {
  if (!ctx || !M) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (ctx->algo != ALGO_CR) return fail(ctx, DWH_ERR_STATE, "level-0 blocks exist only on the CR path");
  const dwh::CrDims& c = ctx->cr;
  if (chain < 0 || chain >= ctx->d.nc || pole < 0 || pole >= c.P)
    return fail(ctx, DWH_ERR_ARG, "chain or pole index out of range");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  if (refill) {
    // exactly cr_enqueue's assembly launch (rewritten blocks + Δ/2 scatter)
    const CrPlan& pl = ctx->plan;
    dwh::launch_cr_fill(c, ctx->bpool, ctx->d_fill_step, (int)pl.fill_step.size(), ctx->hcol, ctx->hval,
                        ctx->Dcol, ctx->Dsrc, ctx->Delta, ctx->d_y, ctx->d_off_ph, ctx->stream);
    HIPCHECK(ctx, hipGetLastError());
  }
  const int Lx = c.Lx, Ly = c.Ly, N = c.N, BP = c.BP, HP = BP / 2;
  const size_t nblk0 = 3 * (size_t)Ly, bsz = (size_t)HP * BP;
  std::vector<double2> h(nblk0 * bsz);
  const int64_t bi = chain * c.P + pole;
  HIPCHECK(ctx, hipMemcpyAsync(h.data(), ctx->bpool + bi * c.item, h.size() * sizeof(double2),
                               hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  // expand the M-form top halves [A | B] into the reference basis (particles
  // i = y Lx + x, holes i + N): rows i: [A | B], rows i + N: [conj B | -conj A]
  const size_t n2 = 2 * (size_t)N;
  std::vector<uint8_t> seen(n2 * n2, 0);
  for (size_t k = 0; k < n2 * n2; ++k) M[k] = dwh_c128{0.0, 0.0};
  auto put = [&](size_t r, size_t col, double re, double im) -> bool {
    const size_t o = r + col * n2;   // column-major
    if (seen[o]) return false;
    seen[o] = 1;
    M[o] = dwh_c128{re, im};
    return true;
  };
  for (int t = 0; t < 3; ++t) {
    if ((t == 1 && Ly < 2) || (t == 2 && Ly < 3)) continue;   // k_cr_fill's zero blocks
    for (int yb = 0; yb < Ly; ++yb) {
      const int yr = (t == 2) ? (yb + 1) % Ly : yb, yc = (t == 1) ? (yb + 1) % Ly : yb;
      const double2* blk = h.data() + (size_t)(t * Ly + yb) * bsz;
      for (int r = 0; r < Lx; ++r)
        for (int x = 0; x < Lx; ++x) {
          const size_t i = (size_t)yr * Lx + r, j = (size_t)yc * Lx + x;
          const double2 a = blk[(size_t)r * BP + x], b = blk[(size_t)r * BP + HP + x];
          if (!put(i, j, a.x, a.y) || !put(i, j + N, b.x, b.y) || !put(i + N, j, b.x, -b.y) ||
              !put(i + N, j + N, -a.x, a.y))
            return fail(ctx, DWH_ERR_STATE, "level-0 blocks overlap");
        }
    }
  }
  if (y) std::copy(ctx->poles.y.begin(), ctx->poles.y.end(), y);
  return DWH_OK;
}

}  // extern "C"
