// The C-ABI context (struct dwh_ctx) and the helpers every file that drives
// the device shares: error returns, device allocation, the event timers, and
// the few functions that cross between dwhmc_api.cpp (steps, creation, HMC),
// dwhmc_eigsolve.cpp (eigensolver driver) and dwhmc_measure.cpp (transport,
// spectral maps, vertex responses).  Private to those files.  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dwhmc.h"
#include "dwhmc_integrator.h"
#include "dwhmc_internal.h"
#include "dwhmc_model.h"
#include "dwhmc_plan.h"

namespace dwh {

enum TimerName {
  T_GJ_UPDATE = 0, T_GJ_PIVOT, T_ASSEMBLE, T_CONTRACT, T_STEP, T_GJ_EDGE, T_CR_GEMM, T_CR_INV, T_CR_INVSIDE,
  T_EIG_OWN, T_EIG_VENDOR, T_CR_SPARSE, T_SPECTRAL, T_RESPONSE, T_OPERATOR, T_NAMBU, T_MAP,
  T_CORR_RHO, T_CORR_CONTRACT, T_CORR_REDUCE, T_SWEEP_LOG, T_COUNT
};
inline const char* const kTimerNames[T_COUNT] = {"gj_update", "gj_pivot", "assemble", "contract",
                                                 "step",      "gj_edge",  "cr_gemm",  "cr_inv",
                                                 "cr_inv_side",
                                                 "eig_own",   "eig_vendor",   // eigensolves (work: matrices)
                                                 "cr_sparse",
                                                 "spectral",    // LDOS / A(k, ω) map stage (work: flops)
                                                 "response",    // Λ(q, iΩ) after its eigensolve (work: flops)
                                                 "operator",    // χ(iΩ), χ''(ω) of sparse vertices after their eigensolve (work: flops)
                                                 "nambu",       // cross response of Nambu vertices after its eigensolve (work: flops)
                                                 "map",         // response maps after their eigensolve (work: flops)
                                                 "corr_rho",       // correlations: ρ = U f U^H (work: flops)
                                                 "corr_contract",  // ... the Wick contractions (work: bytes issued)
                                                 "corr_reduce",    // ... chunk sums and the mean gather (work: bytes)
                                                 "sweep_log"};     // the sweep log's launches (work: bytes written)

enum Algo { ALGO_DENSE = 0, ALGO_CR = 1, ALGO_EIG = 2 };

struct TimingRec {
  int name;
  hipEvent_t a, b;
  double work;
};

}  // namespace dwh

struct dwh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  dwh::Dims d{};
  // the lattice model (tables, ‖h‖ bound, current operator: dwhmc_model.h),
  // built once at creation; a pole re-selection's new context shares it
  std::shared_ptr<const dwh::HostModel> model;
  double beta = 0, J = 0, delta_cap = 2.0;
  // guard: per site (mean |Δ| of its 4 bonds <= delta_cap, checked by the
  // level-0 inversion launch) or per bond (|Δ_ij| <= delta_cap, the drift kernels)
  bool site_guard = false;
  int* site4 = nullptr;   // device copy of the model's site4 (site guard)
  dwh::PoleChoice poles;   // the pole set in use (select_poles)
  int reselections = 0;
  int64_t device_bytes = 0;
  bool factorized = false;
  std::string err;

  // device buffers
  double2 *R = nullptr, *S = nullptr;
  double2* Dv = nullptr;   // pairing values of D per chain (nc x N x kSlots)
  // Gauss-Jordan panels: column panels CpA[2] (parity), CpB; row panels XR1/XR2; pivots Pb1/Pb2
  double2 *CpA0 = nullptr, *CpA1 = nullptr, *CpB = nullptr, *XR1 = nullptr, *XR2 = nullptr,
          *Pb1 = nullptr, *Pb2 = nullptr;
  double2 *G12nn = nullptr, *diagS = nullptr;
  double *ldpart = nullptr, *ldstatic = nullptr, *d_y = nullptr, *d_c = nullptr;
  int *Dcol = nullptr, *Dsrc = nullptr, *hcol = nullptr, *bond_ij = nullptr, *bond_ji = nullptr;
  double* hval = nullptr;
  double2 *Delta = nullptr, *Pi = nullptr, *Pair = nullptr, *F = nullptr, *DeltaB = nullptr,
          *PairB = nullptr;
  double *Ef = nullptr, *EfB = nullptr, *Trhh = nullptr, *TrhhB = nullptr, *Hold = nullptr,
         *Hnew = nullptr;
  int* flag = nullptr;
  // guard trips inside a batch of throughput sweeps (dwh::SweepHalt): halt[0]
  // halted, halt[1] sequence number of the tripped sweep in `enq`
  int* halt = nullptr;
  struct EnqSweep {
    int64_t sweep, Nt;
    double dt, mass;
  };
  std::vector<EnqSweep> enq;   // throughput sweeps enqueued since the last settle()
  // the splitting every trajectory runs (dwh_set_integrator; default leapfrog);
  // it changes only with `enq` empty, so a replay runs what was enqueued
  dwh::Integrator integ;
  // draws / results: single-sweep scratch (s_*) and the throughput path
  double2* s_noise = nullptr;
  double* s_uniform = nullptr;
  uint8_t* s_acc = nullptr;
  double* s_dH = nullptr;
  int64_t ndraws = 0;
  double2* noise = nullptr;
  double* uniform = nullptr;
  uint8_t* acc = nullptr;
  double* dH = nullptr;
  // the sweep log (dwh_sweep_log, dwhmc_sweeplog.cpp): which parts every
  // throughput sweep records (DWH_LOG_* bits), the snapshot cadence, and the
  // buffers, sized for log_ndraws sweeps (obs: 12 per (sweep, chain); sq: 2 N
  // per (sweep, chain); snap: Δ per snapshot slot)
  int32_t log_what = 0;
  int64_t log_every = 1, log_offset = 0, log_ndraws = 0;
  double *log_obs = nullptr, *log_sq = nullptr;
  double2* log_snap = nullptr;
  std::vector<void*> allocations;

  // block cyclic-reduction path (algo == ALGO_CR)
  int algo = dwh::ALGO_DENSE;
  dwh::CrDims cr{};
  dwh::CrPlan plan;
  double2* bpool = nullptr;   // CR block pool (nbatch x nblk blocks)
  dwh::CrTask* d_tasks = nullptr;
  dwh::CrSlot* d_slots = nullptr;
  dwh::SpTaskArrays sp_arr;   // the sparse stages' row records and per-task column arrays
  dwh::CrSpRowFwd* d_sp_rf = nullptr;
  dwh::CrSpRowBwd* d_sp_rb = nullptr;
  int* d_sp_cm = nullptr;
  double2* d_sp_cv = nullptr;
  double* efpart = nullptr;     // per (chain, pole) E_f / Tr G22 partials
  unsigned* efdone = nullptr;   // per chain: pole blocks done (k_cr_fermion_energy)
  int *d_inv_blk = nullptr, *d_inv_dst = nullptr, *d_inv_slot = nullptr, *d_inv0_r = nullptr;
  double* ldA = nullptr;   // static ln|det| of the Δ = 0 level-0 blocks (= 2 ln|det A|) per slot
  int64_t *d_doff = nullptr, *d_off_ph = nullptr;
  int64_t* d_bond4 = nullptr;   // k_cr_pair_force: per bond its G12 offsets and pairing-entry offsets
  int *d_fill_all = nullptr, *d_fill_step = nullptr;
  // the pool's level-0 pairing entries already hold the current Δ (set by a
  // drifting k_cr_pair_force, consumed by the next factorisation); every
  // other path that changes Δ leaves it false
  bool pairing_in_pool = false;
  bool pending = false;    // dwh_hmc_trajectory done, dwh_hmc_finish not yet
  int async_rc = 0;        // eig path: a rocSOLVER / rocBLAS call refused while enqueuing

  // transport / spectra measurement (device side allocated on first use):
  // device copies of the model's x-current operator J (CSR) and of its +x,
  // +x+y, +x-y neighbours; the rocBLAS handle (rocSOLVER zheevd, zgemm) runs
  // on ctx->stream
  int tr_slots = 0;   // chains the per-chain transport buffers hold
  rocblas_handle blas = nullptr;
  dwh::TrBufs tr{};
  int *d_tr_nbr = nullptr, *d_tr_rowptr = nullptr, *d_tr_col = nullptr, *d_tr_info = nullptr;
  int* d_tr_bad = nullptr;   // eigen_solve: non-finite E / U after zheevd
  double* d_tr_val = nullptr;
  double* d_tr_offd = nullptr;   // zheevd off-diagonal workspace (2N)
  int64_t tr_nw = -1, tr_nd = -1;   // ω / DOS grid lengths the output buffers hold
  double2* d_tr_stage = nullptr;     // Δ snapshots of dwh_measure_transport_deltas
  int64_t tr_nstage = 0;
  // spectral maps (dwh_measure_spectral_maps) workspace for sp_slots states:
  // the Lorentzian table of one frequency chunk (2N x kSpChunk per state)
  // and the two maps' output tiles (N x kSpChunk each per state)
  int sp_slots = 0;
  double *d_sp_lam = nullptr, *d_sp_out = nullptr;
  // the vertex responses (current, one-body operator, Nambu cross response:
  // vertex_prepare / vertex_run, dwhmc_measure.cpp), allocated on first use,
  // grown on demand and freed where the slot buffers are reallocated: d_rs_ws
  // holds rs_mats n2 x n2 matrices (W_k U of one group of vertices, at most
  // kRsCapBytes, and for the current and operator responses the group's
  // U^H W_k U behind them), d_rs_part the per-column Matsubara pair sums,
  // d_rs_out one state's results, the rest the vertices of the call as one
  // 2N-row CSR: d_rs_idx its rowptr (2N + 1), d_rs_col the columns, d_rs_val
  // the complex values per vertex
  int64_t rs_mats = 0, rs_npart = 0, rs_nout = 0, rs_nval = 0, rs_ncol = 0, rs_nidx = 0;
  double2 *d_rs_ws = nullptr, *d_rs_val = nullptr;
  double *d_rs_part = nullptr, *d_rs_out = nullptr;
  int *d_rs_col = nullptr, *d_rs_idx = nullptr;
  // current response: the direction's bond neighbours (3 x N), for the
  // diamagnetic weight
  int64_t rs_nnbr = 0;
  int* d_rs_nbr = nullptr;
  // operator response: the χ'' partials of a group (operators x column
  // chunks x frequencies)
  int64_t op_npart = 0;
  double* d_op_part = nullptr;
  // Nambu cross response: d_nb_x keeps X^k = U^H W_k U of every vertex of the
  // call (a pair needs both of its matrices), d_nb_part the chi2 partials of
  // one batch of pairs, d_nb_pairs the pair list
  int64_t nb_nx = 0, nb_npart = 0, nb_npairs = 0;
  double2* d_nb_x = nullptr;
  double* d_nb_part = nullptr;
  int* d_nb_pairs = nullptr;
  // response maps: d_map_ws holds the weighted matrices K_z and the products
  // S_z = K_z U^H of one chunk of frequencies (2 x chunk n2 x n2 matrices, at
  // most kRsCapBytes; one frequency is always allowed), d_map_out the chunk's
  // sampled entries, d_map_omega the real frequencies, d_map_idx the
  // column-grouped pattern (rows a and original indices, npat each) and
  // d_map_slice its workgroup slices (3 ints each)
  int64_t map_nws = 0, map_nout = 0, map_nomega = 0, map_nidx = 0, map_nslice = 0;
  double2 *d_map_ws = nullptr, *d_map_out = nullptr;
  double* d_map_omega = nullptr;
  int *d_map_idx = nullptr, *d_map_slice = nullptr;
  // what the last call with a dmap output left there, for dwh_bench_response_map_stages:
  // slices, entries, frequencies per chunk, and where in d_rs_ws its last X lies
  int64_t map_last_nslices = 0, map_last_npat = 0, map_last_chunk = 0, map_last_x = 0;
  // equal-time correlations: d_cr_idx the call's term table, pair list and
  // reference sites (tptr, trow, tcol, pairs, ref, one after the other),
  // d_cr_val the term values, d_cr_part the translation average's partials
  // (pairs x chunks x N), d_cr_out one state's mean, corr and local.  ρ itself
  // takes the slot's Jmn (S = diag(f) U^H its JU).
  int64_t cr_nidx = 0, cr_nval = 0, cr_npart = 0, cr_nout = 0;
  int* d_cr_idx = nullptr;
  double2 *d_cr_val = nullptr, *d_cr_part = nullptr, *d_cr_out = nullptr;
  // own eigensolver (dwhmc_eig.hip) workspace for eig_slots matrices: hemv
  // partials, v ping-pong, w, tridiagonal (d, e), tau, compact-WY T blocks and
  // the back-transform's two nb x n products; the n x n work lives in the
  // slots' JU (A -> V), Jmn and U (eigenvector / LU scratch) buffers
  int eig_slots = 0;
  double2 *d_eig_part = nullptr, *d_eig_vv = nullptr, *d_eig_ww = nullptr, *d_eig_tau = nullptr;
  double2 *d_eig_T = nullptr, *d_eig_W = nullptr, *d_eig_W2 = nullptr, *d_eig_dpart = nullptr;
  double2* d_eig_pfin = nullptr;   // the hemv partials reduced per row (k_eig_reduce)
  double2* d_eig_colfin = nullptr;   // column i with its pending pairs (k_eig_reduce)
  double2* d_eig_gpart = nullptr;    // k_eig_reduce's g partials (one matrix)
  int* d_eig_c0 = nullptr;         // particle-hole half solve: first computed eigenvector per matrix
  bool eig_half = false;           // the last own solve ran the particle-hole half solve
  std::vector<int> eig_c0h;        // its c0 per matrix (N: no zero crowding)
  // the last eigen_solve's U of every slot is closed under the particle-hole
  // map column by column (half solve, c0 = N everywhere, no fallback):
  // transport's pair sums then run over half the pairs
  bool eig_ph = false;
  int64_t eig_long_clusters = 0;   // clusters longer than k_eig_orth's limit, orthonormalised by long_clusters
  int eig_ph_last = -1;    // dwh_info_t::eig_half: eig_ph of the last eigensolve (-1: none yet)
  int eig_quat_last = 0;   // the last eigensolve took the structure-preserving solver
  // dwh_debug_set_eigensystem: dbg_nstates > 0 eigensystems staged on the
  // host (E: 2N per state, U: 2N x 2N column-major per state), which the next
  // eigen_solve with m == dbg_nstates copies into the slots instead of solving
  int dbg_nstates = 0;
  bool dbg_ph = false;
  std::vector<double> dbg_E;
  std::vector<double2> dbg_U;
  double *d_eig_d = nullptr, *d_eig_e = nullptr, *d_eig_tn = nullptr;
  // structure-preserving solver (dwhmc_qeig.hip) workspace: q_slots matrices
  // (q_bufs), the eigenvector stage's for q_vec_slots (q_heev_enqueue)
  double* d_q = nullptr;
  int q_slots = 0, q_vec_slots = 0;
  double2 *d_qz = nullptr, *d_qs = nullptr, *d_qg = nullptr;
  hipStream_t eig_sx[3] = {};       // extra streams of the sub-batched tridiagonalisation
  hipEvent_t eig_ev[4] = {};

  // timing
  int timing = 0;   // bitmask over TimerName (bit i = kTimerNames[i])
  std::vector<dwh::TimingRec> recs;
  std::vector<hipEvent_t> pool;
  double t_ms[dwh::T_COUNT] = {0};
  int64_t t_n[dwh::T_COUNT] = {0};
  double t_work[dwh::T_COUNT] = {0};
};

namespace dwh {

// ctx == nullptr: the text goes where dwh_last_error(NULL) reads it (dwhmc_model.h)
inline int fail(dwh_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  else g_create_error = msg;
  return code;
}

#define HIPCHECK(ctx, x)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      return fail((ctx), DWH_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

int settle(dwh_ctx* ctx);   // dwhmc_api.cpp
// finish (and recover) pending throughput sweeps before the state is read or changed
#define SETTLE(ctx)                                 \
  do {                                              \
    if (!(ctx)->enq.empty())                        \
      if (int rc_ = settle(ctx)) return rc_;        \
  } while (0)

template <typename T>
int dalloc(dwh_ctx* ctx, T** p, size_t n) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess)
    return fail(ctx, DWH_ERR_HIP, "hipMalloc(" + std::to_string(bytes) + " B): " + hipGetErrorString(e));
  ctx->allocations.push_back(q);
  ctx->device_bytes += (int64_t)bytes;
  *p = static_cast<T*>(q);
  return DWH_OK;
}

inline void drop_alloc(dwh_ctx* ctx, void* p) {
  if (!p) return;
  auto it = std::find(ctx->allocations.begin(), ctx->allocations.end(), p);
  if (it != ctx->allocations.end()) ctx->allocations.erase(it);
  (void)hipFree(p);
}

inline hipEvent_t take_event(dwh_ctx* ctx) {
  if (!ctx->pool.empty()) {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  // no system-scope fence per record: the timers bracket device kernels only,
  // and the fence's L2 writeback would perturb the kernels being timed
  (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  return e;
}

struct Scope {
  dwh_ctx* ctx;
  int name;
  double work;
  hipStream_t st;
  hipEvent_t a{};
  bool on;
  Scope(dwh_ctx* c, int n, double w)
      : ctx(c), name(n), work(w), st(c->stream), on(((c->timing >> n) & 1) != 0) {
    if (on) {
      a = take_event(ctx);
      (void)hipEventRecord(a, st);
    }
  }
  ~Scope() {
    if (on) {
      hipEvent_t b = take_event(ctx);
      (void)hipEventRecord(b, st);
      ctx->recs.push_back({name, a, b, work});
    }
  }
};

inline void drain_timing(dwh_ctx* ctx) {
  if (ctx->recs.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& r : ctx->recs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    ctx->t_ms[r.name] += ms;
    ctx->t_n[r.name] += 1;
    ctx->t_work[r.name] += r.work;
    ctx->pool.push_back(r.a);
    ctx->pool.push_back(r.b);
  }
  ctx->recs.clear();
}

// dwhmc_sweeplog.cpp: the log's launches of throughput sweep sw (after
// launch_traj_end; nothing when no part is enabled); its buffers sized for
// ctx->ndraws and zero-filled (no-op when the log is off); setting and buffers
// handed from ctx to the new device side n of a pole re-selection
void sweep_log_enqueue(dwh_ctx* ctx, int64_t sw);
int sweep_log_resize(dwh_ctx* ctx);
void sweep_log_move(dwh_ctx* ctx, dwh_ctx* n);
// dwhmc_measure.cpp, called from the step and creation code as well:
// device buffers (+ the rocBLAS handle) of `slots` measurement slots
int transport_prepare(dwh_ctx* ctx, int64_t nw, int64_t nd, int slots);
// where the slots of a batched eigensolve take their H_BdG(Δ) from: slot k
// assembles Δ = Delta + k dstride with the hopping / disorder of chain
// chain0 + k cstep
struct TrSrc {
  const double2* Delta;
  int64_t dstride;
  int64_t chain0;
  int cstep;
};
// dwhmc_eigsolve.cpp: the chains' own Δ from chain c0 on, the buffers of slot
// k, the batched eigensolve of m slots (synchronises) and its rocSOLVER info
TrSrc chains_src(const dwh_ctx* ctx, int64_t c0);
TrBufs tr_slot(const dwh_ctx* ctx, int k);
int eigen_solve(dwh_ctx* ctx, const TrSrc& src, int m);
int eigen_info_check(dwh_ctx* ctx, int m);
// dwhmc_measure.cpp: states per batched eigensolve of a _deltas / batched call
int tr_group(const dwh_ctx* ctx, int64_t n);

}  // namespace dwh
