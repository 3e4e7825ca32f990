/*
 * dwhmc.h — C ABI of the MI355X-native fermionic action/force path of
 * DwaveHMC.jl (YinkaiYu/Hybrid-Monte-Carlo-for-d-wave-SC).
 *
 * The reference is pure Julia with no FFI; each entry point below replaces a
 * Julia function of the hot path (file:line of the reference in brackets) and
 * is what a Julia `ccall`, a C++ host or Python `ctypes` binds (see
 * INTEGRATION.md).  Conventions:
 *   - every array is borrowed for the duration of the call only;
 *   - complex numbers are interleaved fp64 pairs (Julia ComplexF64,
 *     numpy complex128, C99 double _Complex);
 *   - per-chain bond arrays (Δ, π, F, P) are Julia's column-major N×2 layout:
 *     element (i, dir) at offset i + N*dir, dir 0 = +x, dir 1 = +y
 *     (src/Types.jl:106-111); chain c starts at offset c*2N;
 *   - neighbour tables are Julia's column-major N×4 Int64 matrices, 1-based
 *     (src/Types.jl:53-80);
 *   - functions return DWH_OK (0) or a negative DWH_ERR_* code; the message is
 *     in dwh_last_error(ctx) (dwh_last_error(NULL) after a failed create);
 *   - a context is bound to one HIP device and one stream and is not
 *     thread-safe (one context per host thread).
 */
#ifndef DWHMC_H
#define DWHMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double re, im; } dwh_c128;
typedef struct dwh_ctx dwh_ctx;

enum {
  DWH_OK = 0,
  DWH_ERR_ARG = -1,       /* bad argument (Julia: ArgumentError / DimensionMismatch) */
  DWH_ERR_HIP = -2,       /* HIP runtime failure (no device, OOM, launch failure) */
  DWH_ERR_STATE = -3,     /* call out of order */
  DWH_ERR_SPECTRUM = -4,  /* |Δ| left the guarded range the pole set was built for */
  DWH_ERR_TABLE = -5      /* β·E_bound outside the pole table with DWH_ALGO_DENSE / _CR requested */
};

typedef struct {
  int64_t N;          /* sites Lx*Ly */
  int64_t Np;         /* N padded to the 64-row GJ block */
  int64_t nchains;
  int64_t npoles;     /* imaginary-axis pole pairs = no-pivot LUs per chain per step (eig: 0) */
  double kappa;       /* β·E'/2 of the pole table entry in use (eig: of the spectral bound) */
  double e_bound;     /* E' : spectral bound the poles are valid on */
  double err_tanh;    /* sup |tanh - rational| of the table entry (eig: 0) */
  double delta_cap;   /* guard cap: on max|Δ_ij| (bond guard), or on the mean |Δ| of each site's
                         4 bonds (site guard: the CR path, whose level-0
                         inversion launch checks it); eig: DBL_MAX, no guard */
  int64_t device_bytes;
  int64_t algo;       /* 0 = dense Schur-complement Gauss-Jordan, 1 = block cyclic reduction,
                         2 = eigendecomposition */
  int64_t block;      /* dense: GJ block (64); cr: padded lattice-row block BP >= 2 Lx; eig: 0 */
  int64_t eig_half;   /* last eigensolve (transport / eig path): 1 = particle-hole half solve,
                         J_mn and the pair sums over the columns < N; 0 = every column; -1 = none yet */
  int64_t eig_long_clusters; /* eigenvalue clusters so far too long for the one-workgroup
                                orthonormalisation, taken by the multi-workgroup Cholesky QR */
  int64_t eig_quat;   /* last eigensolve with vectors: 1 = the structure-preserving (quaternion)
                         solver, 0 = the one-stage tridiagonalisation (spectra with a cluster
                         longer than 32 levels or a crowd at zero longer than 16, or
                         DWHMC_EIG_QUAT=0) */
} dwh_info_t;

/* ModelParameters + initialize_cache + init_static_H!
 * [src/Types.jl:49-91, src/Types.jl:182-212, src/Hamiltonian.jl:10-47].
 * One chain, default delta_cap (bond guard max(2, 6 sqrt(2J/β)); site guard
 * max(1.25, 4 sqrt(2J/β))).  disorder: length N
 * (state.disorder_pot). */
int dwh_create(dwh_ctx** ctx, int64_t Lx, int64_t Ly, double t, double tp, double mu,
               double beta, double J, const int64_t* nn_table, const int64_t* nnn_table,
               const double* disorder, int32_t device);

/* Batched form: nchains independent Markov chains / disorder realisations on one
 * device (disorder: nchains*N).  delta_cap <= 0 selects the default
 * (bond guard max(2, 6 sqrt(2J/β)), site guard max(1.25, 4 sqrt(2J/β)));
 * either guard bounds the pairing block's norm by 2 delta_cap; the pole set
 * covers spectra within ‖h‖ + 2 delta_cap and is
 * re-selected for a larger cap when an uploaded Δ or a trajectory exceeds it. */
int dwh_create_batched(dwh_ctx** ctx, int64_t Lx, int64_t Ly, double t, double tp, double mu,
                       double beta, double J, const int64_t* nn_table, const int64_t* nnn_table,
                       int64_t nchains, const double* disorder, double delta_cap, int32_t device);

/* Factorisation algorithm of a context:
 *   DWH_ALGO_DENSE  Schur complement over the static particle block + blocked
 *                   Gauss-Jordan of the dense N x N complement per pole;
 *   DWH_ALGO_CR     block cyclic reduction of the block-tridiagonal (lattice-row
 *                   blocks, periodic) BdG matrix per pole; needs 2 Lx <= 128;
 *   DWH_ALGO_EIG    the reference's own method: the eigendecomposition of every chain's
 *                   2N x 2N H_BdG per step (dwh_eigensystem's solver), ρ = U diag(f) U^H by zgemm
 *                   [src/Hamiltonian.jl:96-114, src/Observables.jl:14-62]; any β,
 *                   no pole set, no |Δ| guard; O(N^3) with a large constant;
 *   DWH_ALGO_AUTO   DWHMC_ALGO from the environment (dense | cr | eig | auto),
 *                   else CR when supported, else dense; EIG when β·E'/2 is beyond
 *                   the pole table (β above a few hundred).  All give the same
 *                   results to fp64 rounding. */
enum { DWH_ALGO_AUTO = -1, DWH_ALGO_DENSE = 0, DWH_ALGO_CR = 1, DWH_ALGO_EIG = 2 };

/* dwh_create_batched with an explicit algorithm. */
int dwh_create_ex(dwh_ctx** ctx, int64_t Lx, int64_t Ly, double t, double tp, double mu,
                  double beta, double J, const int64_t* nn_table, const int64_t* nnn_table,
                  int64_t nchains, const double* disorder, double delta_cap, int32_t algo,
                  int32_t device);

void dwh_destroy(dwh_ctx* ctx);
const char* dwh_last_error(const dwh_ctx* ctx);
int dwh_info(dwh_ctx* ctx, dwh_info_t* out);

/* update_H_BdG! [src/Hamiltonian.jl:55-86]: set Δ (nchains*2N) on the device. */
int dwh_update_pairing(dwh_ctx* ctx, const dwh_c128* Delta);

/* diagonalize_H_BdG! replacement [src/Hamiltonian.jl:96-114]: pole-expanded
 * no-pivot LU of H_BdG(Δ) - i y_q for all poles; caches the pairing
 * amplitudes P_ij and the fermion energy E_f for the current Δ. */
int dwh_factorize(dwh_ctx* ctx);

/* compute_forces! [src/Observables.jl:14-62]: F = -β/2J (Δ - J P) with the
 * cached P.  Delta may be NULL (use the device Δ).  F_out: nchains*2N. */
int dwh_forces(dwh_ctx* ctx, const dwh_c128* Delta, dwh_c128* F_out);

/* P_ij = -ρ_{i,j+N} - ρ_{j,i+N} of the last factorisation [src/Observables.jl:37-53]. */
int dwh_pairing(dwh_ctx* ctx, dwh_c128* P_out);

/* Fermion part of compute_total_energy [src/HMC.jl:21-27], per chain. */
int dwh_fermion_energy(dwh_ctx* ctx, double* Ef);

/* Tr ρ_hh per chain (hole-block trace of the density matrix); with
 * Tr ρ_pp + Tr ρ_hh = N this gives hole_conc = 2 Tr ρ_hh / N - 1
 * [src/Observables.jl:120-145]. */
int dwh_hole_trace(dwh_ctx* ctx, double* tr_hh);

/* compute_total_energy [src/HMC.jl:12-41] for the device Δ, π and cached E_f. */
int dwh_total_energy(dwh_ctx* ctx, double mass, double* H);

/* Device state access (Δ, π: nchains*2N; either pointer may be NULL). */
int dwh_set_state(dwh_ctx* ctx, const dwh_c128* Delta, const dwh_c128* pi);
int dwh_get_state(dwh_ctx* ctx, dwh_c128* Delta, dwh_c128* pi);

/* hmc_sweep! [src/HMC.jl:71-144] with the RNG draws injected (the reference
 * is unseeded): noise = randn!(ComplexF64) draws (Var Re = Var Im = 1/2),
 * nchains*2N; uniform = the rand() of the Metropolis test, nchains.
 * Outputs accepted[nchains] (0/1) and dH[nchains]. */
int dwh_hmc_sweep(dwh_ctx* ctx, const dwh_c128* noise, const double* uniform, int64_t Nt,
                  double dt, double mass, uint8_t* accepted, double* dH);

/* hmc_sweep! split at its Metropolis test, so a host whose RNG must be
 * consumed exactly as the reference consumes it (src/HMC.jl:128 draws
 * rand() only when ΔH >= 0) decides acceptance itself:
 *   dwh_hmc_trajectory: momentum refresh from `noise`, H_old, backup,
 *     leapfrog, H_new [src/HMC.jl:76-122]; dH[nchains] = H_new - H_old.
 *   dwh_hmc_finish: accepted[nchains] (0/1) from the host; rejected chains are
 *     restored [src/HMC.jl:130-141].
 * Between the two calls the context refuses another sweep (DWH_ERR_STATE). */
int dwh_hmc_trajectory(dwh_ctx* ctx, const dwh_c128* noise, int64_t Nt, double dt, double mass,
                       double* dH);
int dwh_hmc_finish(dwh_ctx* ctx, const uint8_t* accepted);

/* The integrator of a context's trajectories (dwh_hmc_sweep,
 * dwh_hmc_trajectory, dwh_run_sweeps).  One step of size dt is a symmetric
 * splitting with S >= 1 force evaluations (factorisations):
 *   kick a_0·dt;  for s = 1..S: drift b_s·dt, force evaluation, kick a_s·dt
 * with kick π += c·F and drift Δ += c/(2m)·π, the two updates of
 * [src/HMC.jl:92,101,112,118].  Nt steps are concatenated with the adjacent
 * end and start kicks merged into one of (a_S + a_0)·dt, so a trajectory
 * makes S·Nt factorisations; Nt keeps its meaning (steps) in every entry
 * point, and the "step" timer counts factorisations.
 *   DWH_INT_LEAPFROG  S = 1, a = (1/2, 1/2), b = (1): the reference's
 *                     integrator [src/HMC.jl:88-118] and the default, bit for
 *                     bit what a context without this call runs; the only
 *                     one that takes Nt = 0 (two half kicks, no factorisation);
 *   DWH_INT_OMELYAN2  S = 2, a = (λ, 1 - 2λ, λ), b = (1/2, 1/2), 0 < λ < 1/2:
 *                     the second-order minimum-norm scheme at
 *                     λ = DWH_OMELYAN2_LAMBDA (Omelyan, Mryglod, Folk, Comput.
 *                     Phys. Commun. 151 (2003) 272); the optimum in λ is sharp
 *                     (DESIGN.md §4i), so pass that value unless exploring;
 *   DWH_INT_CUSTOM    kick = a_0..a_S (nstage + 1 entries), drift = b_1..b_S
 *                     (nstage entries), 1 <= nstage <= 16: all finite, Σa = 1
 *                     and Σb = 1 within 1e-12, palindromic bit for bit
 *                     (a_s = a_{S-s}, b_s = b_{S+1-s}).
 * lambda is read by OMELYAN2 only; nstage, kick and drift by CUSTOM only.
 * Pending throughput sweeps are settled first, so a batch never mixes
 * schedules; the setting survives pole re-selections.  DWH_ERR_STATE between
 * dwh_hmc_trajectory and dwh_hmc_finish; DWH_ERR_ARG for a schedule that
 * breaks a rule above (the context keeps its integrator). */
enum { DWH_INT_LEAPFROG = 0, DWH_INT_OMELYAN2 = 1, DWH_INT_CUSTOM = 2 };
#define DWH_OMELYAN2_LAMBDA 0.1931833275037836
int dwh_set_integrator(dwh_ctx* ctx, int32_t kind, double lambda, int64_t nstage, const double* kick,
                       const double* drift);
/* The context's integrator: kind and lambda as set (lambda 0 unless
 * OMELYAN2), nstage = S and the coefficients in use, presets included (kick:
 * S + 1 entries, drift: S; at most 17 and 16).  Every output may be NULL. */
int dwh_get_integrator(dwh_ctx* ctx, int32_t* kind, double* lambda, int64_t* nstage, double* kick,
                       double* drift);
/* Host only, no device: the coefficients a trajectory of Nt steps of the
 * given integrator hands to the kick/drift kernels, from the function the
 * enqueue itself calls.  nfact = S·Nt; kicks_out: nfact + 1 entries, the
 * first with the momentum refresh, entry i after factorisation i, in units of
 * F (merged kicks as one double); drifts_out: nfact entries, entry i before
 * factorisation i + 1, b·dt/(2 mass) in units of π.  Leapfrog with Nt = 0:
 * nfact = 0 and kicks_out gets the two half kicks.  Every output may be NULL
 * (nfact alone sizes the others).  DWH_ERR_ARG as dwh_set_integrator and the
 * trajectory entry points refuse (dwh_last_error(NULL)). */
int dwh_debug_integrator_schedule(int32_t kind, double lambda, int64_t nstage, const double* kick,
                                  const double* drift, int64_t Nt, double dt, double mass, int64_t* nfact,
                                  double* kicks_out, double* drifts_out);

/* Throughput path: upload the draws of nsweeps sweeps once (noise:
 * nsweeps*nchains*2N, uniform: nsweeps*nchains), then enqueue sweeps that
 * read them from HBM without host round trips.  A guard trip inside a batch
 * makes the batch's later sweeps no-ops on the device; the next
 * dwh_sweep_results / dwh_synchronize (or any call that reads or changes the
 * state) re-selects the pole set, resumes from the tripped sweep's starting Δ
 * and replays the remaining sweeps — the same steps dwh_hmc_sweep takes — so
 * the results equal the single-sweep path's bit for bit. */
int dwh_load_draws(dwh_ctx* ctx, int64_t nsweeps, const dwh_c128* noise, const double* uniform);
int dwh_run_sweeps(dwh_ctx* ctx, int64_t first_sweep, int64_t nsweeps, int64_t Nt, double dt,
                   double mass);
int dwh_sweep_results(dwh_ctx* ctx, int64_t first_sweep, int64_t nsweeps, uint8_t* accepted,
                      double* dH);
int dwh_synchronize(dwh_ctx* ctx);

/* The sweep log: what every sweep of dwh_run_sweeps records on the device for
 * every chain, by extra launches after the sweep's Metropolis step, so from
 * the accepted or restored Δ, P, E_f and Tr ρ_hh.  A context that never
 * enables it makes the launches it made before.  `what` is a mask of
 *   DWH_LOG_OBS       DWH_OBS_FIELDS doubles: fields 0..8 the reference's
 *                     ObservablesResult in its order [src/Observables.jl:70-80]
 *                     (total_energy, Δ_amp, Δ_local, Δ_global, S_Δ, hole_conc,
 *                     Δ_diff, Δ_pair, Δ_localpair), 9 E_f, 10 Tr ρ_hh,
 *                     11 Σ|Δ_ij|²;
 *   DWH_LOG_FIELD_SQ  the pairing field's structure factors: with
 *                     d_i = (Δ[i,0] - Δ[i,1])/2, s_i = (Δ[i,0] + Δ[i,1])/2,
 *                     channel 0 = d, 1 = s, site i = x + Lx·y,
 *                       S_ch(q) = |(1/N) Σ_i f_i exp(-2πi (kx·x/Lx + ky·y/Ly))|²,
 *                     q = kx + Lx·ky (the momentum indexing and sign of ak0 /
 *                     akw); S_0(0) is field 4 of the record.  N <= 4096;
 *   DWH_LOG_SNAPSHOT  Δ after the sweeps sw >= snap_offset with
 *                     (sw - snap_offset) % snap_every == 0, sw the index into
 *                     the loaded draws.
 * dwh_sweep_log settles pending sweeps first, so a batch is never half
 * logged; what = 0 frees the log.  The buffers are sized for the loaded draws
 * and zero-filled, by this call and by a dwh_load_draws that grows the draws.
 * The setting and the buffers survive pole re-selections; after a guard trip
 * the replayed sweeps are logged again, so the log equals what the
 * single-sweep path would have produced for every sweep.  DWH_ERR_STATE
 * between dwh_hmc_trajectory and dwh_hmc_finish; DWH_ERR_ARG, with nothing
 * changed, for bits outside the mask, for snap_every < 1 or snap_offset < 0
 * with the snapshot bit, and for N > 4096 with the field bit.
 * The readers settle like dwh_sweep_results; DWH_ERR_ARG for a range outside
 * the loaded draws, DWH_ERR_STATE for a part that is not enabled:
 *   dwh_sweep_observables  obs[f + 12·(c + nchains·k)], sweep first + k;
 *   dwh_sweep_field_sq     sq[q + N·(ch + 2·(c + nchains·k))];
 *   dwh_sweep_snapshots    the snapshots of the sweeps in [first, first +
 *                          nsweeps), ascending: *nsnap their number, sweep[m]
 *                          their sweeps, Delta per snapshot in dwh_get_state's
 *                          layout; Delta / sweep NULL: count only.
 * dwh_sweep_log_layout (host only) is the validation and the sizes those
 * calls use: counts[0] doubles of obs, counts[1] doubles of sq, counts[2]
 * snapshots of the range [first, first + nsweeps) of ndraws loaded sweeps. */
enum { DWH_LOG_OBS = 1, DWH_LOG_FIELD_SQ = 2, DWH_LOG_SNAPSHOT = 4 };
#define DWH_OBS_FIELDS 12
int dwh_sweep_log(dwh_ctx* ctx, int32_t what, int64_t snap_every, int64_t snap_offset);
int dwh_sweep_observables(dwh_ctx* ctx, int64_t first, int64_t nsweeps, double* obs);
int dwh_sweep_field_sq(dwh_ctx* ctx, int64_t first, int64_t nsweeps, double* sq);
int dwh_sweep_snapshots(dwh_ctx* ctx, int64_t first, int64_t nsweeps, int64_t* nsnap, int64_t* sweep,
                        dwh_c128* Delta);
int dwh_sweep_log_layout(int64_t nchains, int64_t N, int64_t ndraws, int32_t what, int64_t snap_every,
                         int64_t snap_offset, int64_t first, int64_t nsweeps, int64_t* counts);

/* hipStream_t the context launches on (for events / interop).  The handle
 * stays valid for the context's lifetime, pole re-selections included. */
int dwh_stream(dwh_ctx* ctx, void** stream);

/* Kernel timing with HIP events on the stream each kernel runs on
 * (bench/profiling).  enable is a bitmask over the timer names below
 * (bit 0 "gj_update", bit 1 "gj_pivot", bit 2 "assemble", bit 3 "contract",
 * bit 4 "step", bit 5 "gj_edge", bit 6 "cr_gemm", bit 7 "cr_inv", bit 8 "cr_inv_side",
 * bit 9 "eig_own", bit 10 "eig_vendor", bit 11 "cr_sparse", bit 12 "spectral",
 * bit 13 "response", bit 14 "operator", bit 15 "nambu", bit 16 "map",
 * bit 17 "corr_rho", bit 18 "corr_contract", bit 19 "corr_reduce",
 * bit 20 "sweep_log");
 * 0 disables, -1 times everything. */
int dwh_timing_enable(dwh_ctx* ctx, int32_t enable);
/* name: "gj_update" (rank-128 paired / rank-64 trailing updates),
 * "gj_edge" (edge update between the two pivots of a pair), "gj_pivot",
 * "cr_gemm" (cyclic-reduction block products), "cr_inv" (its block
 * inversions), "cr_inv_side" (inversion stages that also run the products off
 * the critical path; work = inversion + side-product flops), "cr_sparse" (the
 * sparse level-0 stages: products with the level-0 U / L blocks, work = their
 * sparse flops), "eig_own" / "eig_vendor" (eigensolves by the library's solver /
 * by rocSOLVER, opt-in or fallback; work = matrices), "spectral" (the map
 * stage of dwh_measure_spectral_maps after its eigensolve: column DFTs,
 * Lorentzian tables and the two products; work = 2·N·2N·count flops per map
 * per state), "response" (everything dwh_measure_current_response does after
 * its eigensolve, one record per state; work = 8·(2N)³ flops per momentum per
 * state, the J_nm product's), "operator" (the same for
 * dwh_measure_operator_response; work = 8·(2N)³ flops per operator per
 * state), "nambu" (the same for dwh_measure_nambu_response; work = 8·(2N)³
 * flops per vertex per state), "map" (the same for dwh_measure_response_map;
 * work = 8·(2N)³ flops per vertex, for X, plus 8·(2N)³ per (vertex, frequency),
 * per state; 0 without a dmap output), "corr_rho" / "corr_contract" /
 * "corr_reduce" (the stages of dwh_measure_correlations after its eigensolve,
 * one record each per state: S = diag(f) U^H and the product ρ = U S, work =
 * 8·(2N)³ flops; the contractions of every pair, corr and local, work = the
 * bytes they issue, 32 per (term of A, term of B); the chunk sums and the
 * mean gather, work = the bytes they move), "assemble",
 * "contract", "step"; returns total milliseconds, launches and the
 * algorithmic work summed over launches (fp64 flops; HBM bytes for
 * "assemble"). */
int dwh_timing_read(dwh_ctx* ctx, const char* name, double* total_ms, int64_t* launches,
                    double* work);
int dwh_timing_reset(dwh_ctx* ctx);
/* Enqueues the per-factorisation assembly launch (timer "assemble": CR, the
 * pairing entries Δ/2 scattered into the level-0 blocks, replacing
 * update_H_BdG! src/Hamiltonian.jl:55-86; dense, the Schur-complement
 * assembly) reps times back to back on the context's stream and waits, so a
 * bench reads a warm per-launch average with the timers instead of the one
 * launch a factorisation makes.  Idempotent: the pool keeps the current Δ.
 * eig path: DWH_ERR_STATE. */
int dwh_bench_assembly(dwh_ctx* ctx, int64_t reps);
/* Diagnostic: one CR factorisation at the context's Δ with per-workgroup phase
 * stamps of its inv_stage-th inversion launch (in the plan's own schedule,
 * side work included) into out (nwg rows of 32 uint64: [0]/[30]
 * s_memrealtime at entry/exit, [1..29] s_memtime phase stamps, [31] kind 1
 * inversion / 2 side work / 3 guard).  Only a library built with -DCR_STAMPS
 * records them (tools/cr_inv_sched_stamps.py); others return DWH_ERR_STATE. */
int dwh_debug_cr_stamps(dwh_ctx* ctx, int32_t inv_stage, uint64_t* out, int64_t nwg);

/* ---- measurement path (not the leapfrog step) ----------------------------
 * Eigen-decomposition of one chain's H_BdG(Δ) at the device Δ: what the
 * reference's diagonalize_H_BdG! [src/Hamiltonian.jl:96-114] leaves in
 * cache.E_n / cache.U, which the hot path replaces by the pole expansion but
 * transport and spectra need.  The library's own Hermitian eigensolver on
 * the context's stream (dwhmc_eig.hip: Householder tridiagonalisation,
 * multisection on Sturm counts, inverse iteration with cluster
 * orthonormalisation (clusters of any length), blocked back-transform; the
 * plain products on the library's own MFMA kernel, dwhmc_gemm.hip);
 * rocSOLVER runs only for an order above the own solver's 5120 (zheevd) and
 * as the re-solve (zheev) of a result with non-finite values.
 * E: 2N, ascending; U (nullable): 2N x 2N column-major, the eigenvector of
 * E[n] in column n (phases are the solver's). */
int dwh_eigensystem(dwh_ctx* ctx, int64_t chain, double* E, dwh_c128* U);

/* Lengths of the frequency grids of measure_transport_and_spectra
 * [src/Observables.jl:395,430]: ω = η:Δω:ω_max and -ω_max:Δω:ω_max, counted
 * as Julia's float ranges count them; point k of either grid is start + k·Δω. */
int dwh_transport_grid(double eta, double domega, double omega_max, int64_t* n_omega,
                       int64_t* n_dos);

/* measure_transport_and_spectra [src/Observables.jl:314-526] for one chain at
 * the device Δ, i.e. the SpectrumResult fields [:293-308]: superfluid
 * stiffness, DC conductivity, σ(ω) on the ω grid (n_omega values), DOS and
 * antinodal DOS on the DOS grid (n_dos values each) and A(k, ω=0) as the
 * column-major Lx x Ly map (element (kx, ky) at kx + Lx·ky, FFTW's forward
 * sign).  n_omega / n_dos must equal dwh_transport_grid's.  The current
 * operator J_x [:237-283] is built once per context; J_mn = U^H (J ⊕ J) U is
 * the library's own MFMA product (dwhmc_gemm.hip); the rest runs in
 * dwhmc_transport.hip. */
int dwh_measure_transport(dwh_ctx* ctx, int64_t chain, double eta, double domega, double omega_max,
                          double* stiffness, double* dc_cond, double* sigma, int64_t n_omega,
                          double* dos, double* dos_an, int64_t n_dos, double* ak0);

/* dwh_measure_transport for every chain of the context at once: the
 * eigensolves and J_mn products are batched over the chains (every kernel
 * of the eigensolver and the products take all chains per launch).
 * Outputs per chain c at stiffness[c], dc_cond[c], sigma[c*n_omega],
 * dos[c*n_dos], dos_an[c*n_dos], ak0[c*Lx*Ly]. */
int dwh_measure_transport_batched(dwh_ctx* ctx, double eta, double domega, double omega_max,
                                  double* stiffness, double* dc_cond, double* sigma, int64_t n_omega,
                                  double* dos, double* dos_an, int64_t n_dos, double* ak0);

/* measure_transport_and_spectra at nstates pairing fields of one chain's
 * lattice and disorder: Delta[k] (nstates x 2N, the Δ layout above), e.g. the
 * states of nstates consecutive measurement sweeps [src/Simulation.jl:169-171]
 * kept by the host and measured in one call.  The eigensolves and J_mn
 * products are batched over the snapshots as in
 * dwh_measure_transport_batched; outputs per snapshot k at stiffness[k],
 * dc_cond[k], sigma[k*n_omega], dos[k*n_dos], dos_an[k*n_dos], ak0[k*Lx*Ly].
 * The context's own Δ is not touched. */
int dwh_measure_transport_deltas(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                 double eta, double domega, double omega_max, double* stiffness,
                                 double* dc_cond, double* sigma, int64_t n_omega, double* dos, double* dos_an,
                                 int64_t n_dos, double* ak0);

/* ---- resolved spectral maps ----------------------------------------------
 * The site- and momentum-resolved spectra the reference leaves out
 * [src/Observables.jl:305-307], in its own DOS normalisation.  With E_n, U the
 * eigenpairs of H_BdG(Δ), u_n(i) = U[i, n] for the particle rows i < N,
 * L(x) = (1/π) η/(x² + η²) and û_n(k) the unnormalised forward 2-D DFT of u_n
 * as an Lx x Ly image (site i = x + Lx·y, e^{-2πi(kx·x/Lx + ky·y/Ly)}, the
 * conventions of A(k, ω=0) above):
 *   LDOS(i, ω) = Σ_{n<2N} |u_n(i)|² L(ω - E_n)
 *   A(k, ω)    = (1/N) Σ_{n<2N} |û_n(k)|² L(ω - E_n)
 * so that (1/N) Σ_i LDOS = (1/N) Σ_k A = dos(ω), and for even Lx, Ly
 * [A((Lx/2, 0), ω) + A((0, Ly/2), ω)] / 2 = dos_an(ω).
 * ω runs over a window of the DOS grid -ω_max:Δω:ω_max: the points
 * first + q·stride, q < count.
 *
 * Frequencies of a window of the DOS grid: points first + q*stride, q < count.
 * Host only.  omega (nullable): count values.  DWH_ERR_ARG if the window
 * leaves the grid (or count < 1, stride < 1). */
int dwh_spectral_window(double eta, double domega, double omega_max,
                        int64_t first, int64_t count, int64_t stride, double* omega);

/* LDOS and A(k, ω) of one chain at the device Δ (Delta == NULL, nstates == 1)
 * or at nstates pairing fields (the Delta layout of
 * dwh_measure_transport_deltas, eigensolves batched in the same groups).
 * ldos / akw: either may be NULL (that map is skipped; both NULL is
 * DWH_ERR_ARG).  Per state s, column-major N x count:
 *   ldos[i + N*q + N*count*s],  akw[kx + Lx*ky + N*q + N*count*s].
 * One eigensolve per state (not shared with a transport call), then two real
 * fp64 MFMA products against one Lorentzian table (dwhmc_spectral.hip).  The
 * window is processed in chunks of 1024 frequencies, which bounds the device
 * workspace per state by 32 KiB·N (table 2N x 1024, two output tiles N x
 * 1024).  The context's own Δ is not touched.  The products run as |X|²
 * written out, then the library's real product (the default, also
 * DWHMC_SPECTRAL_FUSED=0 in the environment); DWHMC_SPECTRAL_FUSED=1 selects
 * the fused kernel that squares X as it stages it (slower where measured,
 * kept for A/B). */
int dwh_measure_spectral_maps(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                              double eta, double domega, double omega_max,
                              int64_t first, int64_t count, int64_t stride,
                              double* ldos, double* akw);

/* ---- finite-momentum current response ------------------------------------
 * The current-current response Λ_αα(q, iΩ_l) and the diamagnetic term of
 * direction α (0 = x, 1 = y): the reference's stiffness terms
 * [src/Observables.jl:340-387], which it takes at q = 0, α = x, Ω = 0 only,
 * at lattice momenta q = 2π (mx/Lx, my/Ly) and Matsubara frequencies
 * Ω_l = 2π l/β, in its conventions and normalisation (at q = 0, α = x, l = 0,
 * dia - Λ is dwh_measure_transport's stiffness).  The limits at Ω = 0: q_x = 0,
 * q_y -> 0 of Λ_xx (transverse) gives the superfluid stiffness dia - Λ,
 * q_y = 0, q_x -> 0 (longitudinal) probes gauge invariance.
 * Site i has x = i mod Lx, y = i div Lx.  Current operator of direction α
 * with bonds b = (neighbour j_b(i), hopping t_b, bond vector δ_b), duplicate
 * (row, col) entries summed as in build_current_operator! [:237-283]:
 *   Jq[i, j_b(i)] += i t_b φ_b(i),  Jq[j_b(i), i] -= i t_b φ_b(i),
 *   φ_b(i) = exp(-i q·(r_i + δ_b/2)),
 *   x: (+x, t, (1,0)), (+x+y, t', (1,1)), (+x-y, t', (1,-1))   (the reference's)
 *   y: (+y, t, (0,1)), (+x+y, t', (1,1)), (-x+y, t', (-1,1)).
 * The Nambu operator is Jq ⊕ Jq (the hole block equals the particle block at
 * every q), J(-q) = J(q)^H.  With E_n, U the eigenpairs, f_n = logistic(-β E_n)
 * and J_nm = (U^H (Jq ⊕ Jq) U)[n, m]:
 *   Λ_αα(q, l) = (1/N) Σ_{n,m<2N} r_nm(l) |J_nm|²
 *   l = 0:  r_nm = (f_n - f_m)/(E_m - E_n), β f_n (1 - f_n) where
 *           |E_m - E_n| < 1e-8 [:370-381]
 *   l >= 1: r_nm = (f_n - f_m)(E_m - E_n) / ((E_m - E_n)² + Ω_l²)
 * and dia_α = <-K_α> of [:344-362] with the bond list of α.
 * Delta == NULL with nstates == 1: the device Δ of `chain`; otherwise nstates
 * pairing fields (the Delta layout and eigensolve groups of
 * dwh_measure_transport_deltas); the context's own Δ is not touched.  Works
 * on contexts of every algorithm.  q: nq pairs (mx, my), |mx| <= Lx,
 * |my| <= Ly; m is NOT reduced modulo L: the half-bond phase exp(-i q·δ/2) is
 * not periodic in m, so (mx, my) and (mx + Lx, my) are different operators.
 * Outputs: dia[s],
 *   lambda[l + n_matsubara·(k + nq·s)],  l < n_matsubara, k < nq, s < nstates.
 * One eigensolve per state, then per momentum one 2N-cubed product on the
 * library's own MFMA kernel around two O(N²) kernels (dwhmc_response.hip),
 * every sum in a fixed order.  Momenta run in groups whose two work matrices
 * per momentum stay within 2 GiB (one momentum's pair is always allowed; at
 * most 64 per group; DWHMC_RESPONSE_GROUP=g in the environment lowers the
 * group size), allocated on first use.  More than 8 Matsubara frequencies
 * re-read J_nm once per 8.  DWH_ERR_ARG: direction not 0 / 1, nq < 1,
 * n_matsubara < 1, a momentum index out of range, NULL q / dia / lambda. */
int dwh_measure_current_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                 int32_t direction, int64_t nq, const int64_t* q, int64_t n_matsubara,
                                 double* dia, double* lambda);
/* Host only (no device, no context): the vertices the call above uploads for
 * the lattice (Lx, Ly, t, tp and the 1-based neighbour tables of dwh_create),
 * Jq ⊕ Jq on one 2N-row CSR with duplicates summed, expanded to dense: out
 * holds nq matrices, 2N x 2N column-major.  DWH_ERR_ARG as above and for the
 * lattice as dwh_create, the text where dwh_last_error(NULL) reads it. */
int dwh_debug_current_vertex(int64_t Lx, int64_t Ly, double t, double tp, const int64_t* nn_table,
                             const int64_t* nnn_table, int32_t direction, int64_t nq, const int64_t* q,
                             dwh_c128* out);
/* Bench (tools/bench_current_response.py): the product of one momentum alone,
 * (2N x 2N)·(2N x 2N) 'N','N' on the measurement buffers of slot 0 as the last
 * measurement left them, reps times back to back after one warm-up launch,
 * HIP-event timed; *ms: milliseconds per product.  The yardstick the
 * "response" timer's per-momentum time is compared against.  Overwrites the
 * slot's JU.  DWH_ERR_STATE before the context's first measurement. */
int dwh_bench_response_product(dwh_ctx* ctx, int64_t reps, double* ms);

/* ---- response of any one-body operator ------------------------------------
 * The Kubo bubble of the current response with the vertex supplied by the
 * caller: charge and spin susceptibilities, Raman vertices, the current at
 * any q and direction (vertices.py builds these).  In the Nambu basis
 * ψ = (c_{i↑}; d_i = c†_{i↓}) with E_n, U the eigenpairs of H_BdG(Δ) and
 * f_n = logistic(-β E_n), an operator
 *   O = Σ_ij V_ij (c†_{i↑} c_{j↑} + s c†_{i↓} c_{j↓})
 * with V any complex N x N sparse matrix and s = +1 (spin-even: charge,
 * current, Raman) or -1 (spin-odd: S^z) has the Nambu matrix
 *   Ṽ = V ⊕ (-s V^T)
 * (plain transpose: c†_{i↓} c_{j↓} = δ_ij - d_j† d_i; the constant s Tr V
 * drops out of the response).  For the antisymmetric Jq and s = +1 this is
 * Jq ⊕ Jq.  With V_nm = (U^H Ṽ U)[n, m]:
 *   χ(l)   = (1/N) Σ_{n,m<2N} r_nm(l) |V_nm|²,  r_nm(l) exactly as in
 *            dwh_measure_current_response (so Re χ for a non-Hermitian V)
 *   χ''(ω) = (π/N) Σ_{n,m<2N} (f_n - f_m) |V_nm|² L_η(ω - (E_m - E_n)),
 *            L_η(x) = (1/π) η/(x² + η²), over all ordered pairs, those with
 *            |f_n - f_m| < 1e-12 skipped: the σ(ω) loop of
 *            [src/Observables.jl:415-423] without its 1/ω; ω = w_start +
 *            j·w_step, j < n_w, of either sign or zero.
 * Operators: nops matrices on one CSR pattern (N rows, 0-based, rowptr N + 1
 * entries, col nnz entries; the union of several patterns with explicit zeros
 * is fine), operator k's nnz values at val + k·nnz, spin_sign[k] = ±1.
 * Duplicate (row, col) entries are summed; columns inside a row may be
 * unsorted.  Delta / nstates / chain as in dwh_measure_current_response; the
 * context's own Δ is not touched; works on contexts of every algorithm; one
 * eigensolve per state.  Outputs:
 *   chi[l + n_matsubara·(k + nops·s)],  chi2[j + n_w·(k + nops·s)].
 * n_matsubara = 0 skips the Matsubara part, n_w = 0 the real-frequency part
 * (the matching pointer may then be NULL; both 0 is DWH_ERR_ARG).  Per
 * operator and state one 2N-cubed product on the library's own MFMA kernel
 * between Ṽ U (a sparse kernel) and the pair sums (dwhmc_operator.hip,
 * dwhmc_response.hip), every sum in a fixed order: two calls give the same
 * bits, a batch of snapshots equals its single-state calls and a call split
 * into smaller groups equals the unsplit one.  Operators run in the groups of
 * the current response (two 2N x 2N work matrices per operator within 2 GiB,
 * at most 64 per group, DWHMC_RESPONSE_GROUP=g lowers it); χ'' adds
 * min(2N, 512)·n_w doubles of partial sums per operator of a group.
 * DWH_ERR_ARG, nothing launched: NULL context, nops < 1, nnz < 1, rowptr not
 * starting at 0 / not ending at nnz / decreasing, a column outside [0, N), a
 * sign other than ±1, a negative count, a missing pointer, eta <= 0 with
 * n_w > 0, non-finite eta / w_start / w_step. */
int dwh_measure_operator_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                                  int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                                  const dwh_c128* val, const int32_t* spin_sign,
                                  int64_t n_matsubara, double* chi,
                                  double eta, double w_start, double w_step, int64_t n_w, double* chi2);
/* Host only (no device, no context): the validation of the call above and the
 * 2N-row CSR it uploads — rows < N hold V, row N + j holds -s V[i, j] at
 * column N + i, duplicates summed — expanded to dense: out holds nops
 * matrices Ṽ_k, 2N x 2N column-major.  Errors as above, the text where
 * dwh_last_error(NULL) reads it. */
int dwh_debug_operator_nambu(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                             const dwh_c128* val, const int32_t* spin_sign, dwh_c128* out);

/* ---- cross response of general Nambu vertices ------------------------------
 * The Kubo bubble <O_a ; O_b†> of any two one-body operators, pairing
 * (anomalous) parts included: pair-field susceptibilities, the amplitude and
 * phase modes, i[H, ρ_q], Λ_xy, density-current (vertices.py builds these).
 * The Nambu basis Ψ = (c_{i↑}; d_i = c†_{i↓}), i < N, is not redundant, so
 * any complex 2N x 2N matrix W is an operator O_W = Ψ† W Ψ (+ a constant):
 * W[:N, :N] is the particle block, W[N:, N:] the hole block,
 * D = W[:N, N:] multiplies c†_{i↑} c†_{j↓} and W[N:, :N] multiplies
 * c_{i↓} c_{j↑}.  With E_n, U the eigenpairs of H_BdG(Δ),
 * f_n = logistic(-β E_n), ΔE_nm = E_m - E_n, Ω_l = 2π l/β, X^k = U^H W_k U
 * and, for a pair p = (a, b), M_nm = X^a_nm conj(X^b_nm):
 *   chi[p, l]  = (1/N) Σ_{n,m<2N} [r_nm(l) + i s_nm(l)] M_nm       (complex)
 *                r_nm(l) exactly as in dwh_measure_current_response;
 *                s_nm(0) = 0, s_nm(l >= 1) = (f_n - f_m) Ω_l / (ΔE² + Ω_l²),
 *                i.e. (f_n - f_m)/(ΔE - iΩ_l)
 *   chi2[p, j] = (π/N) Σ_{n,m} (f_n - f_m) M_nm L_η(ω_j - ΔE_nm)   (complex)
 *                over all ordered pairs (n, m), those with |f_n - f_m| < 1e-12
 *                skipped; ω_j = w_start + j·w_step of either sign.
 * For a = b and W = V ⊕ (-s V^T), Re chi and chi2 are
 * dwh_measure_operator_response's χ and χ''.
 * Vertices: nops matrices on one CSR pattern with 2N rows (0-based, rowptr
 * 2N + 1 entries, col nnz entries in [0, 2N)), vertex k's values at
 * val + k·nnz; duplicates are summed, columns inside a row may be unsorted,
 * the union of several patterns with explicit zeros is fine.  pairs: 2·npairs
 * indices (a_p, b_p) in [0, nops).  Delta / nstates / chain, skipping a part
 * with a zero count, every algorithm, one eigensolve per state and "the
 * context's own Δ is not touched" as in dwh_measure_operator_response.
 * Outputs:
 *   chi[l + n_matsubara·(p + npairs·s)],  chi2[j + n_w·(p + npairs·s)].
 * Per vertex and state one 2N-cubed product on the library's own MFMA kernel
 * after W U (the sparse kernel of the operator response); X^k stays resident
 * for all nops vertices (a pair needs both of its matrices), at most 1 GiB
 * (16 vertices at L = 32): a larger set is DWH_ERR_ARG.  Only the W U scratch
 * runs in the groups of the current response (DWHMC_RESPONSE_GROUP=g lowers
 * them).  chi2 takes one reciprocal per (n, m, ω) for a group of 4 pairs and
 * min(2N, 512)·n_w·2 doubles of partial sums per pair, 16 pairs at a time
 * (dwhmc_nambu.hip).  Every sum has a fixed order: two calls give the same
 * bits, a batch of snapshots equals its single-state calls and smaller groups
 * give the same bits.  Allocated on first use, grown on demand.
 * DWH_ERR_ARG, nothing launched: every case dwh_measure_operator_response
 * refuses (the sign aside), a column outside [0, 2N), npairs < 1 or > 65535, a pair
 * index outside [0, nops), NULL pairs, the resident limit. */
int dwh_measure_nambu_response(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                               int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                               const dwh_c128* val, int64_t npairs, const int64_t* pairs,
                               int64_t n_matsubara, dwh_c128* chi,
                               double eta, double w_start, double w_step, int64_t n_w, dwh_c128* chi2);
/* Host only (no device, no context): the validation of the call above and
 * the CSR it uploads (duplicates summed) expanded to dense: out holds nops
 * matrices W_k, 2N x 2N column-major.  Errors as above, the text where
 * dwh_last_error(NULL) reads it. */
int dwh_debug_nambu_dense(int64_t N, int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                          const dwh_c128* val, int64_t npairs, const int64_t* pairs, dwh_c128* out);

/* ---- response maps: δρ(z)[W] and ρ on any site / bond pattern --------------
 * Where the responses above are lattice sums, this returns the matrix behind
 * them at the entries a caller names: the linear-response density matrix of a
 * source vertex W (a Nambu vertex, as in dwh_measure_nambu_response) at a
 * frequency z,
 *   D(z)[W] = U (w(z) ∘ U^H W U) U^H,
 * and the equal-time ρ = U f U^H, both only on a pattern of npat Nambu index
 * pairs (a_e, b_e) = (prow[e], pcol[e]) in [0, 2N): sites (a = b), bonds, any
 * block.  Any order, duplicates allowed (each gets its own value), outputs in
 * the caller's order, no 1/N applied:
 *   dmap[e + npat·(z + nz·(k + nops·s))] = Σ_nm U[a_e,n] w_nm(z) X^k_nm conj(U[b_e,m])
 *   rho [e + npat·s]                     = Σ_n  U[a_e,n] f_n conj(U[b_e,n])
 * with X^k = U^H W_k U, ΔE_nm = E_m - E_n, f_n = logistic(-β E_n) and
 * z over nz = n_matsubara + n_w points, Matsubara first:
 *   Matsubara l:  w_nm = r_nm(l) + i s_nm(l) exactly as in
 *                 dwh_measure_nambu_response (the l = 0 rule β f_n (1 - f_n)
 *                 where |ΔE| < 1e-8 included);
 *   retarded ω_j = omega[j], of either sign:  w_nm = (f_n - f_m)/(ΔE_nm - ω_j - iη),
 *                 0 where |f_n - f_m| < 1e-12 (the rule of χ''); eta > 0.
 * Every response of the calls above is a contraction: for a vertex B whose
 * entries lie in the pattern, Σ_e conj(B_e) D_e = N·chi of the pair (W, B),
 * its imaginary part at ω + iη N·chi2 for B = W; D(l = 0)[W] = -∂ρ/∂ε under
 * H → H + εW for Hermitian W; Tr D(l >= 1) = 0.  ρ gives the local density,
 * the bond kinetic energy (so the local diamagnetic term) and P_ij =
 * -ρ[i, j+N] - ρ[j, i+N] (vertices.py: bond_pattern, contract and the local
 * stiffness maps).
 * Vertices, Delta / nstates / chain, every algorithm, one eigensolve per state
 * and "the context's own Δ is not touched" as in dwh_measure_nambu_response.
 * Either output may be NULL, which skips that part (without dmap no vertex is
 * applied and n_matsubara + n_w may be 0).
 * Cost per (vertex, frequency) and state: one more 2N-cubed product on the
 * library's own MFMA kernel, S_z = K_z U^H with K_z = w(z) ∘ X (so that both
 * operands of the sampled product D_e = Σ_n conj(U^H[n, a_e]) S_z[n, b_e] are
 * contiguous columns), then the sampled product over the pattern grouped by b
 * (a workgroup stages column b of S_z in LDS and takes 32 entries of it;
 * dwhmc_map.hip); ρ the same on S = diag(f) U^H with no product.  Each real
 * frequency costs a product, hence a list and not a grid.  Workspace: the
 * vertices run in the groups of the current response (at most 2 GiB,
 * DWHMC_RESPONSE_GROUP=g lowers them) and the frequencies of one vertex in
 * chunks whose K_z and S_z take at most 2 GiB more (2·chunk·(2N)² complex;
 * one frequency is always allowed, at most 64 per chunk; DWHMC_MAP_CHUNK=c
 * lowers it) with chunk·npat sampled entries (at most 1 GiB); allocated on
 * first use, grown on demand, freed with the other response workspaces.
 * Every sum has a fixed order: two calls give the same bits, a batch of
 * snapshots equals its single-state calls, smaller groups and chunks give the
 * same bits.
 * DWH_ERR_ARG, nothing launched: every case dwh_measure_nambu_response refuses
 * for its vertices and states, rho and dmap both NULL, npat < 1 or > 2^24, a
 * pattern index outside [0, 2N), NULL prow / pcol, a negative count, more than
 * 2^16 frequencies of a kind or 2^20 (vertex, frequency) points, no frequency
 * with a dmap output, NULL omega with n_w > 0, a non-finite or non-positive
 * eta with n_w > 0, a non-finite ω, 2N > 8192 (the staged column). */
int dwh_measure_response_map(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                             int64_t nops, const int64_t* rowptr, const int64_t* col, int64_t nnz,
                             const dwh_c128* val, int64_t npat, const int64_t* prow, const int64_t* pcol,
                             int64_t n_matsubara, double eta, int64_t n_w, const double* omega,
                             dwh_c128* rho, dwh_c128* dmap);
/* Host only (no device, no context): the validation of the pattern above and
 * the column-grouped ordering the sampled product consumes.  order (npat): a
 * permutation of the entries sorted by b = pcol, stable inside a column;
 * colptr (2N + 1): the entries of column b are order[colptr[b]] ..
 * order[colptr[b+1] - 1].  Errors as above, the text where
 * dwh_last_error(NULL) reads it. */
int dwh_debug_response_map_plan(int64_t N, int64_t npat, const int64_t* prow, const int64_t* pcol,
                                int64_t* order, int64_t* colptr);
/* Bench (tools/bench_response_map.py): the two stages around the product of
 * dwh_measure_response_map alone — the weight kernel for nfreq frequencies of
 * one vertex, and the sampled product of nfreq matrices on the last call's
 * pattern — on the buffers as the last call with a dmap output left them,
 * each reps times back to back after one warm-up launch, HIP-event timed;
 * milliseconds per launch.  nfreq at most that call's frequencies per chunk.
 * Overwrites that call's K_z and sampled-entry buffers.  DWH_ERR_STATE before
 * such a call. */
int dwh_bench_response_map_stages(dwh_ctx* ctx, int64_t reps, int64_t nfreq, double* weight_ms,
                                  double* sample_ms);

/* ---- equal-time correlations C_AB(r) of local operators ------------------
 * At a fixed Δ the fermions are free, so Wick's theorem gives the equal-time
 * correlations of fermion bilinears exactly from the density matrix
 * ρ[x, y] = Σ_n U[x,n] f_n conj(U[y,n]) = <Ψ†_y Ψ_x> (dwh_measure_response_map's
 * ρ, here in full), Ψ = (c_{i↑}; c†_{i↓}).  A local family A gives every site
 * i its own bilinear
 *   O_A(i) = Σ_t a_{i,t} Ψ†_{r(i,t)} Ψ_{c(i,t)},
 * r, c Nambu indices in [0, 2N) anywhere on the lattice, a complex, any number
 * of terms per site up to 64 (zero allowed, duplicates allowed).  The nfam
 * families share one term table: the terms of family k at site i are
 * tptr[k·N + i] .. tptr[k·N + i + 1] - 1 of (trow, tcol, tval); tptr has
 * nfam·N + 1 entries, starts at 0 and does not decrease.  For the pairs
 * (A_p, B_p) = (pairs[2p], pairs[2p+1]) and sites i, j
 *   m_A(i)     = Σ_t a_{i,t} ρ[c(i,t), r(i,t)]                          = <O_A(i)> up to its constant
 *   G_AB(i, j) = Σ_{t,u} a_{i,t} conj(b_{j,u}) conj(ρ[r_A(i,t), r_B(j,u)])
 *                                            (δ[c_A(i,t), c_B(j,u)] - ρ[c_A(i,t), c_B(j,u)])
 *              = <O_A(i) O_B(j)†> - <O_A(i)><O_B(j)†>,
 * and with i = j ⊕ r the periodic translation (x_i = (x_j + r_x) mod Lx,
 * y_i = (y_j + r_y) mod Ly; sites and r indexed y·Lx + x, 0-based):
 *   corr [r + N·(p + npairs·s)]            = (1/N) Σ_j G_{A_p B_p}(j ⊕ r, j)
 *   local[r + N·(q + nref·(p + npairs·s))] = G_{A_p B_p}(ref[q] ⊕ r, ref[q])   (no 1/N)
 *   mean [i + N·(k + nfam·s)]              = m_k(i)
 * for state s.  The disconnected part (1/N) Σ_j m_A(j ⊕ r) conj(m_B(j)) follows
 * from mean on the host.  The Monte Carlo mean over Δ of connected plus
 * disconnected parts is the interacting correlator.
 * Delta / nstates / chain, every algorithm, one eigensolve per state and "the
 * context's own Δ is not touched" as in dwh_measure_nambu_response.  Any
 * output may be NULL, which skips that part; the ρ product runs for a
 * mean-only call too (the gather reads ρ).
 * Cost per state: S = diag(f) U^H and one 2N-cubed product ρ = U S on the
 * library's own MFMA kernel, then per pair the contraction (dwhmc_corr.hip):
 * for a fixed j a lane per displacement r, so the rows the lanes of a stencil
 * family read are neighbours in the column-major ρ; a workgroup takes 256
 * displacements and 16 sites j in ascending order, and a second kernel adds
 * the chunks in ascending order.  local is the same kernel on the reference
 * sites without the sum.  Correctness does not depend on locality or on equal
 * term counts, only speed does.  States run in the groups of the other
 * state-list calls; DWHMC_RESPONSE_GROUP=g, which elsewhere bounds the
 * vertices per group, here bounds the states per group (this call has no
 * vertex groups; the other calls' state groups ignore it).  ρ takes the measurement
 * slots' own matrices; the term table, partials and outputs are allocated on
 * first use, grown on demand and freed with the other response workspaces.
 * Every sum has a fixed order and no atomics: two calls give the same bits, a
 * batch of snapshots equals its single-state calls, smaller groups give the
 * same bits.
 * DWH_ERR_ARG, nothing launched: everything dwh_measure_nambu_response refuses
 * for its states, nfam < 1 (or > 2^16), a NULL or decreasing tptr or
 * tptr[0] != 0, NULL trow / tcol / tval with terms, an index outside [0, 2N),
 * a non-finite value, more than 64 terms at one (family, site), more than 2^24
 * terms in all, with a corr or local output npairs < 1 (or > 2^16), NULL pairs
 * or a pair index outside [0, nfam), with a local output nref < 1 (or > 2^16),
 * NULL ref or a reference site outside [0, N), more than 2^27 (pair, site,
 * displacement) partials, all three outputs NULL, 2N > 8192. */
int dwh_measure_correlations(dwh_ctx* ctx, int64_t chain, int64_t nstates, const dwh_c128* Delta,
                             int64_t nfam, const int64_t* tptr, const int64_t* trow, const int64_t* tcol,
                             const dwh_c128* tval, int64_t npairs, const int64_t* pairs,
                             int64_t nref, const int64_t* ref,
                             dwh_c128* mean, dwh_c128* corr, dwh_c128* local);
/* Host only (no device, no context): the validation above and the terms as
 * uploaded, expanded into out: nfam·N dense 2N x 2N column-major matrices,
 * one per (family, site) at out + (k·N + i)·(2N)², duplicates summed.  The
 * pair list is checked as for a corr output when npairs != 0 or pairs is not
 * NULL, the reference sites as for a local output when nref != 0 or ref is
 * not NULL.  Errors as above, the text where dwh_last_error(NULL) reads it. */
int dwh_debug_correlation_dense(int64_t N, int64_t nfam, const int64_t* tptr, const int64_t* trow,
                                const int64_t* tcol, const dwh_c128* tval, int64_t npairs,
                                const int64_t* pairs, int64_t nref, const int64_t* ref, dwh_c128* out);

/* ---- assembly read-back (parity tests; not on the hot path) -------------
 * The BdG matrix H_BdG(Δ) exactly as the device assembles it, so tests can
 * compare it bit-for-bit with init_static_H! + update_H_BdG!
 * [src/Hamiltonian.jl:10-47, 55-86] (Hermitian completion of the reference's
 * upper triangle, including its overwrite order on 1- and 2-site rings).
 *
 * dwh_debug_dense_H: the dense matrix the eigen/transport path builds
 * (k_tr_assemble) from the device Δ of `chain`; H: 2N x 2N column-major.
 *
 * dwh_debug_level0 (CR path only): the level-0 blocks of batch item
 * (chain, pole) — H_BdG(Δ) - i y_pole I as the factorisation consumes it —
 * expanded from the stored M-form top halves into the reference basis
 * (particles i = y Lx + x, holes i + N); M: 2N x 2N column-major, y (nullable):
 * the npoles pole heights y_q.  refill != 0 first runs the factorisation's
 * assembly launch on the device Δ; refill == 0 reads the pool as the last
 * trajectory step left it (Δ/2 scattered by the force kernel). */
int dwh_debug_dense_H(dwh_ctx* ctx, int64_t chain, dwh_c128* H);

/* Development entry of the structure-preserving (quaternion) eigensolver
 * (dwhmc_qeig.hip, tools/qeig_proto.py): the 2N eigenvalues of H_BdG(Δ of
 * `chain`) ascending into E, the site-by-site reduction's device time into
 * *ms (nullable). */
int dwh_debug_qeig(dwh_ctx* ctx, int64_t chain, double* E, double* ms);

/* Eigensystem injection (tests of the measurement reductions; debug only).
 * Stages nstates eigensystems on the host: E holds 2N values per state,
 * ascending; U is 2N x 2N column-major per state, column n belonging to E[n]
 * (U need not diagonalise anything).  The next eigensolve of this context
 * with exactly nstates matrices — the one dwh_measure_transport(_deltas),
 * dwh_measure_spectral_maps, dwh_measure_current_response,
 * dwh_measure_operator_response, dwh_measure_nambu_response,
 * dwh_measure_response_map and dwh_measure_correlations run after preparing
 * their buffers — copies
 * them into its slots instead of solving, reports the solve as particle-hole
 * closed (dwh_info_t::eig_half) iff ph != 0 and as not structure-preserving
 * (eig_quat = 0), and clears the staging: the injection is one-shot.  With
 * ph != 0 transport takes its half-pair sums, so column 2N-1-n of U must be
 * the Nambu partner (-conj(v); conj(u)) of column n = (u; v) up to a phase.
 * DWH_ERR_ARG (nothing staged) for NULL arguments, a non-finite E or U, E not
 * ascending, nstates outside [1, the slots of one eigensolve], and with ph
 * |E[n] + E[2N-1-n]| > 1e-12 (1 + max|E|).  A next eigensolve with another
 * number of matrices fails with DWH_ERR_ARG and clears the staging too. */
int dwh_debug_set_eigensystem(dwh_ctx* ctx, int64_t nstates, const double* E, const dwh_c128* U, int32_t ph);
int dwh_debug_level0(dwh_ctx* ctx, int64_t chain, int64_t pole, int32_t refill, dwh_c128* M, double* y);

/* ---- CR kernel and per-pole test entries (not on the step path) -----------
 * dwh_debug_cr_launch: ONE launch of the library's own cyclic-reduction
 * launchers on a caller-supplied pool (no context), for kernel contract tests
 * on synthetic blocks.  pool: nbatch x nblk top halves [A | B] (HP x BP
 * row-major, HP = BP / 2, BP in {32, 64, 96, 128}: exactly the device pool
 * layout), copied back after the launch; ldpart: nbatch x nslots, uploaded and
 * copied back (slots no inversion writes keep their value).  kind:
 *   DWH_CR_INV       block inversions blk[i] -> dst[i] (dst == blk: in place),
 *                    ln|det| into ldpart[bi][slot[i]], i < ninv; inv32 selects
 *                    the one-wave kernel at BP 32 (else the generic one);
 *   DWH_CR_INV0      the level-0 inversions from static R = A^-1 blocks (BP 32,
 *                    64, 96), out of place; the entry first forms rblk[i] = R
 *                    and ldA the way context creation does (the [A | 0] blocks
 *                    inverted out of place by the DWH_CR_INV launch), so the
 *                    rblk blocks are scratch the launch overwrites;
 *   DWH_CR_GEMM      a product stage: out = [cin] + sg sum_h A_h B_h per task on
 *                    the task's window, tile size ts (16, 32) and K split
 *                    ksplit (1, 2, 4); ts 16 runs the planner's own tile
 *                    expansion and slot order;
 *   DWH_CR_INV_SIDE  the DWH_CR_INV inversions with the tasks as side work (BP
 *                    64), each task's sign in bit 8 of its bq (set: negative).
 * tasks: ntasks x 16 int32 {out, cin (-1: none), nt, bq (bit h: B_h Q-form,
 * else M-form), a[4], b[4], r0, r1, c0, c1}; the output window rows [r0, r1) x
 * columns [c0, c1) is rounded out to whole ts x ts tiles (side work: 32 x 32)
 * and the rest of `out` is left untouched.  Every index and size is checked on
 * the host before anything is launched — block ids < nblk, windows inside
 * HP x BP, nt in 1..4, ts 32 only where HP % 32 == 0, ksplit 4 only with ts 16,
 * no task writing a block the launch reads or another task writes, no
 * inversion writing another's source: DWH_ERR_ARG with the reason in
 * dwh_last_error(NULL), and no launch.  Stores are plain; with
 * DWHMC_DEBUG_CR_STORE=1 (read at every call) the tiles of a 16 x 16 launch
 * with a K split and the side products are written through, as the plan
 * stores them on the step path. */
enum { DWH_CR_INV = 0, DWH_CR_INV0 = 1, DWH_CR_GEMM = 2, DWH_CR_INV_SIDE = 3 };
int dwh_debug_cr_launch(int32_t device, int32_t kind, int32_t BP, int32_t nblk, int32_t nbatch, int32_t nslots,
                        dwh_c128* pool, double* ldpart, int32_t ninv, const int32_t* blk, const int32_t* rblk,
                        const int32_t* dst, const int32_t* slot, int32_t inv32, int32_t ntasks,
                        const int32_t* tasks, int32_t ts, int32_t ksplit, double sg);

/* Per-pole read-back of a CR context after dwh_factorize (or a trajectory):
 * for batch item (chain, pole), with G = (H_BdG(Δ) - i y_pole)^-1, exactly
 * what the gathers read from the pool:
 *   G12[i * 4 + s] = G[i, N + j], j = cols[i * 4 + s], for the (up to 4)
 *     pairing partners j of site i (the entries the force sums; unused slots:
 *     cols -1, G12 0); cols nullable;
 *   diag[i] = G[i, i] as stored: the hole diagonal the trace needs follows
 *     from the M-form of G, G22[i, i] = G[N + i, N + i] = -conj(diag[i]);
 *   *lndet = ln|det(H_BdG - i y_pole)| = the sum of the block pivots' logs;
 *   y, cq (nullable, npoles each): pole heights y_q and weights c_q.
 * DWH_ERR_STATE on a context of another algorithm or before a factorisation. */
int dwh_debug_cr_resolvent(dwh_ctx* ctx, int64_t chain, int64_t pole, dwh_c128* G12, int32_t* cols, dwh_c128* diag,
                           double* lndet, double* y, double* cq);

/* Host-only check of the cyclic-reduction schedule dwh_create builds for an
 * Lx x Ly periodic lattice with nearest-neighbour pairing and nbatch = chains x
 * poles batch items (side / inv0: enable the side-work placement and the
 * static level-0 particle blocks, as dwh_create does where the block size
 * supports them): every block a stage reads was written by an earlier stage
 * (or is a level-0 / static block), no stage reads what it writes except a
 * task's own accumulate input, no block is written by two tasks of one stage,
 * and the force / E_f gathers read written blocks.  No device is touched.
 * stats (nullable, 6): stages, inversion stages, inversion stages with side
 * work, product stages, writes, pool blocks.  DWH_ERR_STATE with the first
 * violation in dwh_last_error(NULL). */
int dwh_debug_cr_plan_check(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, int64_t* stats);

/* Algorithmic fp64 flops per batch item of the same plan (host only), as the
 * "cr_*" timers count them: flops[0] block inversions (8 BP^3 each), flops[1]
 * block products of the product stages, flops[2] block products run as side
 * work inside inversion stages (8 BP rows cols per term on the restricted
 * output windows).  flops[1] + flops[2] does not depend on `side`. */
int dwh_debug_cr_plan_flops(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, double* flops);

/* What each launch of the same plan stores (host only): 10 values per stage in
 * out[10 i ..] (cap: stages out can hold; *nstages: the plan's count) — kind
 * (0 inversion, 1 products, 2 / 3 sparse level-0 forward / backward), the
 * products' K split, bytes per batch item written by the stage's own outputs
 * and by its side products, launches until either is first read (1: the very
 * next launch; the force gather follows the last stage; 2^20: not read within
 * the step), the store policy (0 plain, 1 write-through, 2 non-temporal) of
 * the two, and the bytes of the two that the very next launch reads. */
int dwh_debug_cr_plan_stores(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, int64_t* out,
                             int64_t cap, int64_t* nstages);

/* The ‖h‖ bound pole selection uses (host only; h = the static particle block
 * of src/Hamiltonian.jl:10-44 with w_i - mu on the diagonal, per chain):
 * out[0] Gershgorin, out[1] the Lanczos estimate, out[2] 1 if every chain
 * certified it (rho I -/+ h positive definite by band LDLᵀ), out[3] the bound
 * used (the Lanczos value if certified, else Gershgorin), out[4] a negative
 * control (1 if rho = 0 "certified": must be 0). */
int dwh_debug_h_bound(int64_t Lx, int64_t Ly, double t, double tp, double mu, const int64_t* nn_table,
                      const int64_t* nnn_table, int64_t nchains, const double* disorder, double* out);

/* Self-test of the f64 MFMA fragment layout (A = I, asymmetric B); 0 = pass. */
int dwh_selftest_mfma(int32_t device);

/* The library's own batched fp64 MFMA product (the measurement path's
 * J_mn = U^H J U, the eigensolver's back-transform and orthogonalisation, the
 * eig path's rho), through host buffers for tests:
 * C_k = alpha op(A_k) op(B_k) + beta C_k, k < batch, column-major, op 'N' or
 * 'C' (conjugate transpose; transpose when real); cplx 1: dwh_c128 data and
 * alpha / beta as {re, im}, 0: double (alpha[0], beta[0]).  Batch strides:
 * lda * (columns of A), ldb * (columns of B), ldc * N elements. */
int dwh_debug_gemm(int32_t device, int32_t cplx, char opa, char opb, int64_t M, int64_t N, int64_t K,
                   const double* alpha, const void* A, int64_t lda, const void* B, int64_t ldb, const double* beta,
                   void* C, int64_t ldc, int64_t batch);

#ifdef __cplusplus
}
#endif
#endif /* DWHMC_H */
