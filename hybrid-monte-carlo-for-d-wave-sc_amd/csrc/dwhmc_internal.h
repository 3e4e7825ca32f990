// Internal launch interface between the C-ABI context (dwhmc_api.cpp: steps,
// creation, HMC; dwhmc_eigsolve.cpp: eigensolver driver; dwhmc_measure.cpp: measurements;
// dwhmc_plan.cpp: the cyclic-reduction plan) and the gfx950 kernels
// (dwhmc_*.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace dwh {

constexpr double kTwoPi = 6.28318530717958647692;
// blocks of b that cover a items
inline int cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }

constexpr int kGJ = 64;        // Gauss-Jordan block (rows/cols of one diagonal block)
constexpr int kSlots = 4;      // pairing entries per BdG row (NN bonds)
constexpr int kHSlots = 9;     // hopping entries per row (diag + 4 NN + 4 NNN)

struct Dims {
  int N;        // sites
  int Np;       // padded to kGJ
  int nb;       // Np / kGJ
  int nc;       // chains
  int P;        // poles per chain
  int nbatch;   // nc * P
  int64_t mat;  // elements per padded matrix (Np*Np)
  int nld;      // ln|det| partials per batch item (dense: nb pivot blocks; cr: Ly block inversions)
};

// after the force: π += kick·F, then (drift != 0) Δ += drift·π with the
// |Δ| <= cap guard setting *flag (the next leapfrog step's drift, fused)
struct KickDrift {
  double kick, drift, cap;
  int* flag;
};

// Block cyclic-reduction path (dwhmc_cr.hip): every batch item owns a pool of
// nblk blocks (level-0 D/U/L, Schur complements, products, G blocks), each the
// top half (HP x BP, BP = 2 HP, HP = Lx rounded up to 16) of a BP x BP block
// of particle-hole form (see dwhmc_cr.hip).
struct CrDims {
  int Lx, Ly, N, BP, P, nbatch, nblk;
  int64_t item;   // elements per batch item pool (nblk * HP * BP)
  int inv32 = 1;  // BP = 32 inversions by the one-wave Schur complement (k_cr_inv32; else k_cr_inv<2>)
};
// out = [cin] + sg * sum_{h<nt} A_h B_h over pool block indices (cin = -1: zero),
// computed only on the output rows [r0, r1) x columns [c0, c1) (rounded out to
// whole wave tiles; the rest of `out` is left untouched); bit h of bq: B_h is
// Q-form (else M-form)
struct CrTask {
  int out, cin, nt, bq;
  int a[4], b[4];
  int r0, r1, c0, c1;
};
// CrTask::bq bit of side-work tasks whose stage sign is negative (side-work
// task lists mix stages of both signs)
constexpr int kCrNegBit = 1 << 8;
// One 16 x 16 output tile of a product stage with its task's operands, so a
// workgroup reads its whole descriptor with one 64-byte scalar load (tr, tc:
// tile row / column in 16-tile units)
struct alignas(64) CrTile {
  int out, cin, nt, bq;
  int a[4], b[4];
  int tr, tc, neg, pad1;   // neg: 1 = negative sign
};
// One 16 x 16 output tile of ONE batch item of a product stage, stored in
// dispatch order (slot blockIdx.x * tiles-per-workgroup + tile: the host applies
// the XCD-aware remap and the batch-item split), with every operand resolved
// to an element offset: a wave reads its whole descriptor with one 64-byte
// scalar load and forms no block, batch-item or tile address itself.
// base: the batch item's first pool element; out / cin: the tile origin (row
// 16 tr, column 16 tc) of the output / accumulate input within the item
// (cin kCrNone: none; out kCrNone: an empty slot); a[h]: A_h at row 16 tr;
// b[h]: B_h at column 16 tc; rot: the column shift of the synthesised B rows'
// source ((c + HP) mod BP - c); bit h of smask: term h's synthesised rows carry
// a negative sign.
constexpr uint32_t kCrNone = 0xffffffffu;
struct alignas(64) CrSlot {
  uint64_t base;
  uint32_t out, cin;
  int nt;
  unsigned smask;
  uint32_t a[4], b[4];
  int rot, pad;
};
static_assert(sizeof(CrSlot) == 64 && offsetof(CrSlot, out) == 8 && offsetof(CrSlot, nt) == 16 &&
                  offsetof(CrSlot, a) == 24 && offsetof(CrSlot, b) == 40 && offsetof(CrSlot, rot) == 56,
              "k_cr_gemm16 reads a slot as 16 dwords in this order");
// wave tiles of a task at tile size ts
inline int cr_task_tiles(const CrTask& t, int ts) {
  return ((t.r1 + ts - 1) / ts - t.r0 / ts) * ((t.c1 + ts - 1) / ts - t.c0 / ts);
}
inline bool cr_supported_bp(int BP) { return BP == 32 || BP == 64 || BP == 96 || BP == 128; }
// Cache policy of a launch's pool stores (st16, dwhmc_device.h): a template
// argument of the kernels, picked per stage by the plan (CrStage::store)
constexpr int kStorePlain = 0, kStoreThrough = 1, kStoreStream = 2;
// launchers: f(std::integral_constant<int, ST>{}) for the run-time policy.
// The kernels are built for the policies the plan can pick, plain and
// write-through; non-temporal stores won in no family
// (profiles/r07_store_policy_ab.txt), and adding the branch here builds them.
template <class F>
inline void with_store(int store, F&& f) {
  if (store == kStoreThrough) f(std::integral_constant<int, kStoreThrough>{});
  else f(std::integral_constant<int, kStorePlain>{});
}
// diagnostic stamp builds (-DCR_STAMPS, dwh_debug_cr_stamps): workgroups recorded per launch
constexpr int kCrStampWG = 2048;
#ifdef CR_STAMPS
int cr_stamps_arm(int key);   // key >= 0: clears the stamps, records the launch whose first block is `key`; -1: off
int cr_stamps_read(unsigned long long* out, int nwg);
#endif
// level-0 blocks of `list` (ids t*Ly + y, t = 0 D / 1 U / 2 L) fully
// rewritten, plus (off_ph != nullptr) the pairing entries Δ[Dsrc]/2 of the
// level-0 blocks outside the list, in one launch
void launch_cr_fill(const CrDims& c, double2* pool, const int* list, int nlist, const int* hcol,
                    const double* hval, const int* Dcol, const int* Dsrc, const double2* Delta,
                    const double* ypole, const int64_t* off_ph, hipStream_t s);
// P from the level-0 G blocks (pole weights), F, kick / drift; per bond b,
// bond4[4 b ..] = pool offsets of G12[i, j], G12[j, i] and of the two
// pairing entries the bond writes (-1: none); with kd.drift != 0 the drifted
// Δ/2 is also scattered into those level-0 entries (k_cr_fill's scatter)
void launch_cr_pair_force(const CrDims& c, double2* pool, const int64_t* bond4, const double* cpole,
                          double2* Delta, double2* Pair, double2* F, double2* Pi,
                          const KickDrift& kd, double beta, double J, hipStream_t s, int store = kStorePlain);
// E_f and Tr ρ_hh from the CR block pivots and the G22 diagonal (pool offsets doff)
// part: 2 x nbatch scratch, done: nchains counters (zero at creation; the
// kernel leaves them zero)
void launch_cr_fermion_energy(const CrDims& c, const double2* pool, const int64_t* doff,
                              const double* ldpart, const double* cpole, double Cx, double beta,
                              double* part, unsigned* done, double* Ef, double* Trhh, hipStream_t s);
// inverts blocks blk[i] into dst[i] (dst == blk: in place); ln|det| into ldpart slots
// Site spectral guard, checked by one extra workgroup per chain of the level-0
// inversion launch: Σ of |Δ| over each site's 4 bonds (site4[4 i ..], indices
// into a chain's N x 2 Δ) <= cap4, else *flag = 1.  Delta == nullptr: off.
struct SiteGuard {
  const double2* Delta = nullptr;
  const int* site4 = nullptr;
  double cap4 = 0.0;
  int* flag = nullptr;
};
void launch_cr_inv(const CrDims& c, double2* pool, const int* blk, const int* dst, const int* slot,
                   int n, double* ldpart, hipStream_t s, const SiteGuard& sg = SiteGuard{}, int store = kStorePlain);
// level-0 inversions of blocks blk[i] (BP = 32, 64, 96) from the static R = A^-1
// blocks rblk[i] (k_cr_inv0); ln|det| = ldA/2 + ln|det S| into ldpart slots
inline bool cr_supported_inv0(int BP) { return BP == 64 || BP == 32 || BP == 96; }
// Delta != nullptr: one extra workgroup per chain checks the site guard
// (Σ of |Δ| over each site's 4 bonds site4[4 i ..] <= cap4, else *flag = 1)
void launch_cr_inv0(const CrDims& c, double2* pool, const int* blk, const int* rblk, const int* dst,
                    const int* slot, int n, double* ldpart, const double* ldA, hipStream_t s,
                    const double2* Delta = nullptr, const int* site4 = nullptr, double cap4 = 0.0,
                    int* flag = nullptr, int store = kStorePlain);
// the same inversions plus nst side-work product tasks per batch item
// (32 x 32 wave tiles, maxt32 per task, each task's sign in bq & kCrNegBit)
// on the CUs the inversions leave idle
inline bool cr_supported_side(int BP) { return BP == 64; }
void launch_cr_inv_side(const CrDims& c, double2* pool, const int* blk, const int* dst, const int* slot,
                        int n, double* ldpart, const CrTask* stasks, int nst, int maxt32, hipStream_t s,
                        const SiteGuard& sg = SiteGuard{}, int store = kStorePlain, int store_side = kStorePlain);
// Sparse level-0 stages (dwhmc_cr_sparse.hip): the level-0 U / L blocks have
// at most kCrSpNZ nonzeros per row and column (vertical hopping + one pairing
// entry); rowpat / colpat hold them per pool block ([block][entry][BP], entry
// = top-half offset | index << 14 | op << 22, op 3 empty; dwhmc_cr_sparse.hip)
constexpr int kCrSpNZ = 4;
inline bool cr_supported_sparse0(int BP) { return BP == 32 || BP == 64 || BP == 96; }
// forward, per kept row k (er = k+1, el = k-1): D'_k = D_k + V1r L_k + V2l U_el,
// U'_k = V1r U_er, L'_k = V2r L_k with V1r = -U_k Dinv_er, V2r = -L_er Dinv_er,
// V2l = -L_el Dinv_el (pool block indices)
struct CrSpFwd {
  int dk, uk, lk, uel, lel, uer, ler, dir, dil, od, ou, ol;
};
// backward, per eliminated row e (a = e-1, c = e+1): Z_a = G_aa U_a + G_ac L_e,
// Z_c = G_ca U_a + G_cc L_e, Y_a = L_a G_aa + U_e G_ca, Y_c = L_a G_ac + U_e G_cc,
// M = L_a Z_a + U_e Z_c (= Y_a U_a + Y_c L_e, the form the kernel uses)
struct CrSpBwd {
  int gaa, gac, gca, gcc, ua, le, la, ue, oza, ozc, oya, oyc, omx, pad0, pad1, pad2;
};
// (CrSpFwd / CrSpBwd describe the tasks to the plan and its dataflow check;
// the kernels read the records below instead.)
//
// Row records: what a wave needs for output row r of task ti, resolved on the
// host (cr_sparse_task_arrays) into one 256-byte record at index ti * HP + r,
// read with a few wide scalar loads.  Row r of every sparse left operand
// (forward: U_k, L_er, L_el; backward: L_a, U_e) is kCrSpNZ slots in a fixed
// order: kCrSpNZ - 1 hopping slots, then the pairing slot.
//   hopping slot: hv — the static value (real; the forward stage's -U, -L sign
//     applied; 0.0 in an empty slot), ho — the dense operand's stored row the
//     entry multiplies, as a byte offset from the batch item's pool base
//     ((block * HP * BP + row * BP) * sizeof(double2); an empty slot points
//     at a valid row);
//   pairing slot: the entry is ps * Δ[pd] (ps = ±1/2 with the stage's sign, 0
//     when empty) and multiplies the synthesised bottom row HP + k of the
//     dense operand, read from its stored row k at po (same offset form).
// The other offsets are row r of the task's dense blocks in that form.
struct alignas(256) CrSpRowFwd {
  double hv[3][kCrSpNZ - 1];     // U_k, L_er, L_el
  double ps[3];
  uint32_t ho[3][kCrSpNZ - 1];   // rows of Dinv_er, Dinv_er, Dinv_el
  uint32_t po[3], pd[3];
  uint32_t dk, od, ou, ol;       // row r of D_k, D'_k, U'_k, L'_k
};
struct alignas(256) CrSpRowBwd {
  double hv[2][kCrSpNZ - 1];        // L_a, U_e
  double ps[2];
  uint32_t ho[2][2][kCrSpNZ - 1];   // [operand][0 / 1]: rows of G_aa / G_ac (L_a), G_ca / G_cc (U_e)
  uint32_t po[2][2], pd[2];
  uint32_t g[4];                    // row r of G_aa, G_ca, G_ac, G_cc
  uint32_t oza, ozc, oya, oyc, omx;
};
static_assert(sizeof(CrSpRowFwd) == 256 && sizeof(CrSpRowBwd) == 256, "one record: 256 bytes");
// recs: the stage's first record (n tasks x HP rows).  tcv / tcm — per task,
// [operand][entry][BP], the column entries of the sparse right operands
// (forward: L_k, U_el, U_er; backward: U_a, L_e): static hopping value with op
// applied, and meta = (Δ index + 1, 0 none) | op << 22 | row << 24.
// Delta: the chains' N x 2 Δ (batch item bi reads chain bi / P).
void launch_cr_sp_fwd(const CrDims& c, double2* pool, const CrSpRowFwd* recs, int n, const double2* tcv,
                      const int* tcm, const double2* Delta, hipStream_t s, int store = kStorePlain);
void launch_cr_sp_bwd(const CrDims& c, double2* pool, const CrSpRowBwd* recs, int n, const double2* tcv,
                      const int* tcm, const double2* Delta, hipStream_t s, int store = kStorePlain);
// block-product stage configuration: output tile TS x TS (16 or 32) and the
// number of waves splitting each tile's K range (1, 2, 4)
struct CrGemmCfg {
  int ts, ksplit;
};
// (chosen per stage by cr_gemm_config, dwhmc_plan.h)
// slots: the stage's cr_gemm_slots (16 x 16 stages, dwhmc_plan.h); tasks: 32 x 32 stages
void launch_cr_gemm(const CrDims& c, double2* pool, const CrTask* tasks, int ntasks, int maxt32,
                    int maxt16, const CrSlot* slots, int nslot_wgs, const CrGemmCfg& cfg, double sg,
                    hipStream_t s, int store = kStorePlain);

// dense h - i y_q (padded with identity) for every (chain, pole): R init input
void launch_fill_hz(const Dims& d, double2* M, const int* hcol, const double* hval,
                    const double* ypole, hipStream_t s);
// Blocked Gauss-Jordan (no pivoting) on all nbatch matrices in M, in pairs of
// 64-wide block steps (see k_gj_update in dwhmc_kernels.hip for the modes).
// pivot: every block inverts S_kk; block j writes X_kj = S_kk^-1 S_kj in place
// and to XRout; block k writes S_kk^-1 to Pout; colcopy (nullable) receives the
// column panel of block column k; nextcol (nullable) receives X_{k,k+1} as row
// block k of the next column panel.
void launch_gj_pivot(const Dims& d, double2* M, int k, double2* Pout, double2* XRout,
                     double2* colcopy, double2* nextcol, double* ldpart, hipStream_t s);
struct GJPanelPtrs {
  const double2 *CpA, *CpB, *XR1, *XR2, *Pb1, *Pb2;
  double2 *CpBw, *CpN;
};
int gj_update_tiles(const Dims& d, int mode);
void launch_gj_update(const Dims& d, double2* M, int k, int mode, const GJPanelPtrs& p,
                      hipStream_t s);
// Dv[c][r][s] = Δ_c[Dsrc[r][s]] / 2: the pairing values of D for every chain
void launch_dvals(const Dims& d, const int* Dsrc, const double2* Delta, double2* Dv,
                  hipStream_t s);
// S^T = -(h + i y) - (D† R D)^T for every (chain, pole)
void launch_assemble(const Dims& d, const double2* R, double2* S, const int* Dcol,
                     const double2* Dv, const int* hcol, const double* hval, const double* ypole,
                     hipStream_t s);
// G12 at the pairing pattern: G12nn[bi][i][s] = -(R D S^{-1})[i, Dcol[i][s]]; diag of S^{-1}
void launch_contract(const Dims& d, const double2* R, const double2* SinvT, const int* Dcol,
                     const double2* Dv, double2* G12nn, double2* diagS, hipStream_t s);
// P = Σ_q c_q (G12[i,j] + G12[j,i]); F = -β/2J (Δ - J P); kick / drift
void launch_pair_force(const Dims& d, const double2* G12nn, const int* bond_ij,
                       const int* bond_ji, const double* cpole, double2* Delta, double2* Pair,
                       double2* F, double2* Pi, const KickDrift& kd, double beta, double J,
                       hipStream_t s);
// F from cached P; kick / drift
void launch_force_from_pair(const Dims& d, const double2* Pair, double2* Delta, double2* F,
                            double2* Pi, const KickDrift& kd, double beta, double J, hipStream_t s);
// E_f and Tr ρ_hh from the pivots of the last factorisation
void launch_fermion_energy(const Dims& d, const double* ldstatic, const double* ldpart,
                           const double2* diagS, const double* cpole, double Cx, double beta,
                           double* Ef, double* Trhh, hipStream_t s);
// H = Σ|π|²/2m + β/2J Σ|Δ|² + E_f into Hout[c]
// trajectory start / end of the throughput path in one launch each (k_traj_begin:
// refresh + H_old + backup + force from the cached P + kick/drift; k_traj_end:
// H_new + Metropolis + restore).
// Guard trips inside a batch of sweeps (SweepHalt): k_traj_end of the sweep
// whose kernels set *flag records its sequence number in halt[1] and sets
// halt[0]; every later k_traj_begin / k_traj_end of the batch then returns at
// once, so the backups (Δ, P, E_f, Tr ρ_hh) keep the tripped sweep's starting
// point for the host to resume from.  halt == nullptr: off.
struct SweepHalt {
  int* halt = nullptr;   // [0] halted, [1] sequence number of the tripped sweep
  int seq = 0;           // this sweep's sequence number in the batch
  const int* flag = nullptr;
};
void launch_traj_begin(const Dims& d, const double2* noise, double scale, double2* Pi, double2* Delta,
                       const double2* Pair, double2* F, const double* Ef, const double* Trhh, double2* DeltaB,
                       double2* PairB, double* EfB, double* TrhhB, double* Hold, double beta, double J,
                       double mass, const KickDrift& kd, const SweepHalt& sh, hipStream_t s);
void launch_traj_end(const Dims& d, double2* Delta, const double2* Pi, double2* Pair, double* Ef, double* Trhh,
                     const double2* DeltaB, const double2* PairB, const double* EfB, const double* TrhhB,
                     const double* Hold, double* Hnew, const double* uniform, uint8_t* accepted, double* dH,
                     double beta, double J, double mass, const SweepHalt& sh, hipStream_t s);
void launch_total_energy(const Dims& d, const double2* Delta, const double2* Pi,
                         const double* Ef, double beta, double J, double mass, double* Hout,
                         hipStream_t s);
void launch_refresh(const Dims& d, const double2* noise, double2* Pi, double scale, hipStream_t s);
void launch_backup(const Dims& d, const double2* Delta, const double2* Pair, const double* Ef,
                   const double* Trhh, double2* DeltaB, double2* PairB, double* EfB,
                   double* TrhhB, hipStream_t s);
void launch_metropolis(const Dims& d, const double* Hold, const double* Hnew,
                       const double* uniform, uint8_t* accepted, double* dH, hipStream_t s);
void launch_restore(const Dims& d, const uint8_t* accepted, const double2* DeltaB,
                    const double2* PairB, const double* EfB, const double* TrhhB,
                    double2* Delta, double2* Pair, double* Ef, double* Trhh, hipStream_t s);
void launch_sum_ld(const Dims& d, const double* ldpart, double* ldsum, hipStream_t s);

// The sweep log (dwhmc_sweeplog.hip): extra launches after launch_traj_end of
// a throughput sweep, each returning at once when halt[0] != 0 (SweepHalt).
// obs: kObsFields doubles per chain from Δ, P, E_f, Tr ρ_hh (DWH_OBS_FIELDS);
// field_sq: S_d(q), S_s(q) of the pairing field, 2 N doubles per chain, one
// workgroup per (chain, channel) with 2 N double2 of dynamic LDS, so
// N <= kLogSqMaxN (non-zero return otherwise, nothing launched); snapshot: Δ
// of every chain copied to out.
constexpr int kObsFields = 12;
constexpr int kLogSqMaxN = 4096;
void launch_log_obs(const Dims& d, const double2* Delta, const double2* Pair, const double* Ef, const double* Trhh,
                    double beta, double J, double* out, const int* halt, hipStream_t s);
int launch_log_field_sq(const Dims& d, int Lx, int Ly, const double2* Delta, double* out, const int* halt,
                        hipStream_t s);
void launch_log_snapshot(const Dims& d, const double2* Delta, double2* out, const int* halt, hipStream_t s);

// Transport / spectra measurement (dwhmc_transport.hip): device buffers of one
// measurement (n2 = 2N; U, JU, Jmn: n2 x n2 column-major)
struct TrBufs {
  double2 *U, *JU, *Jmn;
  double *E, *f, *g, *dia, *Wn, *wan, *w0, *lam, *dc;   // n2 each (g = 1 - f = logistic(+β E))
  double *part, *sigma, *dos, *dos_an, *ak, *scalars;
};
// ω grid: w0 + k dw (k < nw); DOS grid: d0 + k dw (k < nd)
struct TrGrid {
  double w0, d0, dw;
  int nw, nd;
};
// DOS eigenvalue slices (k_tr_dos partials: 2 x slices x nd doubles in the
// σ partial buffer)
// out_k = in_k^H (in: R x C, ld lin; out: C x R, ld lout), k < m
void launch_tr_conj_transpose(const double2* in, int R, int C, int lin, int64_t sin, double2* out, int lout,
                              int64_t sout, int m, hipStream_t s);
int tr_dos_slices(int N);
int tr_sigma_chunks(int N);   // rows of TrBufs::part (each nw long)
// dense H_BdG of one chain into A (zeroed beforehand)
void launch_tr_assemble(double2* A, int N, const int* hcol, const double* hval, const int* Dcol,
                        const int* Dsrc, const double2* Delta, hipStream_t s);
// f, the diamagnetic / DOS / antinodal weights and the A(k,0) weight per eigenstate;
// nbr: 3 x N (+x, +x+y, +x-y neighbours, 0-based)
void launch_tr_colstats(const double2* U, int N, int Lx, const double* E, double beta, double eta,
                        double t, double tp, const int* nbr, double* f, double* g, double* dia, double* Wn,
                        double* wan, double* w0, hipStream_t s);
// JU = (J ⊕ J) U, J in CSR form (N rows, val = Im J)
// JU[:, :ncol] = (J ⊕ J) U[:, :ncol]
void launch_tr_current(const double2* U, double2* JU, int N, const int* rowptr, const int* col,
                       const double* val, int ncol, hipStream_t s);
// everything after J_mn: Λ, dc, σ(ω), stiffness, DOS, A(k,0) (overwrites JU and Jmn).
// ph: U is closed under the particle-hole map (column n2-1-j = Θ column j for
// every j, dwh eigensolver's half solve without a zero-straddling cluster), so
// J_mn is needed (and computed) only in its columns < N and every pair sum
// runs over half the pairs (the pair (n, m) and its partner (n2-1-m, n2-1-n)
// carry the same |J|², E differences and Fermi-factor differences)
void launch_tr_reduce(const TrBufs& b, int N, int Lx, int Ly, double beta, double eta,
                      const TrGrid& g, bool ph, hipStream_t s);

// Spectral maps LDOS(i, ω) / A(k, ω) (dwhmc_spectral.hip), every launch
// batched over m states at the given per-state strides (elements).
// Frequencies per chunk of the window: bounds the Lorentzian table (2N x
// kSpChunk doubles per state) and the two output tiles (N x kSpChunk each)
constexpr int kSpChunk = 1024;
// Λ[n, q] = L(ω_q - E_n) at Lam[q + ldq n], q < cnt, n < n2; ω_q = point
// first + q stride of the grid d0 + k dw (E: n2 per state)
void launch_sp_lorentz(const double* E, int n2, double eta, double d0, double dw, int64_t first, int64_t stride,
                       int cnt, double* Lam, int ldq, int64_t sLam, int m, hipStream_t s);
// X[:, n] = unnormalised forward 2-D DFT of the particle rows of column n of U
// (n2 x n2, ld n2) as an Lx x Ly image, for all 2N columns; T: scratch, X: N x
// n2 (ld N) each
void launch_sp_dft(const double2* U, int64_t sU, int Lx, int Ly, double2* T, int64_t sT, double2* X, int64_t sX,
                   int m, hipStream_t s);
// W[r + M n] = |X[r + ldx n]|², r < M, n < K
void launch_sp_sqmod(const double2* X, int ldx, int64_t sX, int M, int K, double* W, int64_t sW, int m,
                     hipStream_t s);
// out[r + ldo q] = scale Σ_{n<K} |X[r + ldx n]|² Lam[q + ldq n], r < M, q < Q (fp64 MFMA)
void launch_sp_maps(const double2* X, int ldx, int64_t sX, const double* Lam, int ldq, int64_t sLam, int M, int Q,
                    int K, double scale, double* out, int ldo, int64_t sOut, int m, hipStream_t s);

// Current response Λ_αα(q, iΩ_l) (dwhmc_response.hip), one state at a time,
// the momenta in groups.
// Matsubara indices per k_rs_pairs launch (one accumulator each per thread);
// a longer list re-reads J_nm once per chunk
constexpr int kRsLChunk = 8;
// f_n = logistic(-β E_n) and the diamagnetic weight per eigenstate for the
// bond list nbr (3 x N neighbours, 0-based) with hoppings tb[3] (host)
void launch_rs_colstats(const double2* U, int N, const double* E, double beta, const double* tb, const int* nbr,
                        double* f, double* g, double* dia, hipStream_t s);
// (JU_q = (Jq ⊕ Jq) U: launch_op_apply on the 2N-row CSR of Jq ⊕ Jq)
// part[(q nl + l) n2 + m] = Σ_n r_nm(l) |J_nm(q)|², l < nl, q < nq (J_nm(q) at Jnm + q sJ)
void launch_rs_pairs(const double2* Jnm, int64_t sJ, int N, const double* E, const double* f, const double* g,
                     double beta, int nl, int nq, double* part, hipStream_t s);
// out[b] = scale Σ_{k<cnt} in[b cnt + k], b < nout, in a fixed order
void launch_rs_sum(const double* in, int cnt, int nout, double scale, double* out, hipStream_t s);

// Response of a one-body operator (dwhmc_operator.hip), one state at a time,
// the operators in groups; the Matsubara sums are launch_rs_pairs / launch_rs_sum.
// Most column chunks of the χ'' partials (one partial per chunk, ω and operator)
constexpr int kOpSpecChunks = 512;
// the column chunks of the χ'' partials at this N: columns per chunk and chunks
// in use (every chunk non-empty; rows of the partial buffer per operator or
// per pair and part, each nw long)
inline void op_spec_split(int N, int* cols, int* used) {
  const int n2 = 2 * N, nchunk = n2 < kOpSpecChunks ? n2 : kOpSpecChunks;
  *cols = cdiv(n2, nchunk);
  *used = cdiv(n2, *cols);
}
inline int op_spec_chunks(int N) {
  int cols, used;
  op_spec_split(N, &cols, &used);
  return used;
}
// f_n = logistic(-β E_n), g_n = logistic(+β E_n), n < 2N
void launch_op_fermi(const double* E, int N, double beta, double* f, double* g, hipStream_t s);
// VU_k = Ṽ_k U, k < nops: Ṽ in CSR form (2N rows, columns < 2N, one pattern, nz
// complex values per operator at val + k nz), VU_k at VU + k sVU
void launch_op_apply(const double2* U, double2* VU, int64_t sVU, int N, const int* rowptr, const int* col,
                     const double2* val, int nz, int nops, hipStream_t s);
// out[j + nw k] = (η/N) Σ_{n,m} (f_n - f_m) |V_nm(k)|² / ((ω_j - (E_m - E_n))² + η²),
// ω_j = w_start + j w_step, j < nw, k < nops (V_nm(k) at Vnm + k sV); part:
// nops x op_spec_chunks(N) x nw
void launch_op_spec(const double2* Vnm, int64_t sV, int N, const double* E, const double* f, const double* g,
                    double beta, double eta, double w_start, double w_step, int nw, int nops, double* part,
                    double* out, hipStream_t s);

// out = scale Σ_chunks part[(b nchunk + chunk) nw + j], b < nrows, j < nw, the
// chunks in a fixed order; real rows: out[b nw + j]; complex_out (rows b = 2 p
// + c, re / im of pair p): out[2 (p nw + j) + c]
void launch_op_spec_sum(const double* part, int nchunk, int nw, int nrows, double scale, double* out,
                        bool complex_out, hipStream_t s);

// Cross response of general Nambu vertices (dwhmc_nambu.hip), one state at a
// time: X^k = U^H W_k U at X + k sX for every vertex of the call, pairs as 2
// ints (a_p, b_p) per pair on the device.
// Pairs per group of the chi2 kernel (one reciprocal serves a group; the last,
// partial group runs on the instantiation of its own size)
constexpr int kNbSpecGroup = 4;
// part[((p nl + l) 2 + c) n2 + m] = Σ_n Re / Im of (r_nm(l) + i s_nm(l)) X^a_nm conj(X^b_nm),
// p < npairs, l < nl: launch_rs_sum over n2 then gives chi[l + nl p] as (re, im)
void launch_nb_pairs(const double2* X, int64_t sX, int N, const int* pairs, int npairs, const double* E,
                     const double* f, const double* g, double beta, int nl, double* part, hipStream_t s);
// out[2 (j + nw p) + c] = (η/N) Σ_{n,m} (f_n - f_m) Re / Im X^a_nm conj(X^b_nm) / ((ω_j - (E_m - E_n))² + η²)
// for the pairs p0 <= p < p0 + npairs (out: the call's whole chi2); part:
// npairs x 2 x op_spec_chunks(N) x nw
void launch_nb_spec(const double2* X, int64_t sX, int N, const int* pairs, int p0, int npairs, const double* E,
                    const double* f, const double* g, double beta, double eta, double w_start, double w_step, int nw,
                    double* part, double* out, hipStream_t s);

// Response maps (dwhmc_map.hip), one state at a time: D(z)[W] = U (w(z) ∘ X) U^H
// with X = U^H W U, and ρ = U f U^H, at the entries of a sparse pattern.
// Entries per workgroup of the sampled product (a longer column group is cut
// into slices of this many)
constexpr int kMapSlice = 32;
// rows of the staged column the sampled product's LDS holds (128 KiB)
constexpr int kMapMaxN2 = 8192;
// K + c sK = w(z0 + c) ∘ X, c < cnt: z < nl the Matsubara index l = z
// (launch_nb_pairs' r + i s), z >= nl the real frequency omega[z - nl] (device):
// (f_n - f_m)/(ΔE_nm - ω - iη), 0 where |f_n - f_m| < 1e-12
void launch_map_weight(const double2* X, int N, const double* E, const double* f, const double* g, double beta,
                       int z0, int cnt, int nl, const double* omega, double eta, double2* K, int64_t sK,
                       hipStream_t s);
// S = diag(f) UH
void launch_map_fscale(const double2* UH, int N, const double* f, double2* S, hipStream_t s);
// out[dst[i] + y sOut] = Σ_n conj(UH[n, arow[i]]) S_y[n, b], S_y = S + y sS, y < nmat,
// for every entry i of every slice (b, i0, cnt) (3 ints each: i0 <= i < i0 +
// cnt <= i0 + kMapSlice); 2N <= kMapMaxN2
void launch_map_sddmm(const double2* UH, const double2* S, int64_t sS, int N, const int* slices, int nslices,
                      const int* arow, const int* dst, double2* out, int64_t sOut, int nmat, hipStream_t s);

// Equal-time correlations of local families (dwhmc_corr.hip), one state at a
// time, from the full ρ = U f U^H (n2 x n2 column-major).  The terms of family
// k at site i are tptr[k N + i] .. tptr[k N + i + 1] - 1 of (trow, tcol, tval);
// pairs: 2 ints (a_p, b_p) per pair; all on the device.
constexpr int kCorrTile = 256;      // displacements r per workgroup, a lane each
// sites j per workgroup of the translation average: a compile-time constant,
// because the association of the sum over j depends on it
constexpr int kCorrChunk = 16;
constexpr int kCorrMaxTerms = 64;   // most terms at one (family, site)
constexpr int kCorrMaxN2 = 8192;
inline int corr_chunks(int N) { return cdiv(N, kCorrChunk); }
// jlist == NULL: part[(p corr_chunks(N) + c) N + r] = Σ_{j in chunk c} G_p(j ⊕ r, j), nj = N;
// else part[(p nj + q) N + r] = G_p(jlist[q] ⊕ r, jlist[q]), q < nj
void launch_corr(const double2* rho, int N, int Lx, const int* tptr, const int* trow, const int* tcol,
                 const double2* tval, const int* pairs, int npairs, const int* jlist, int nj, double2* part,
                 hipStream_t s);
// out[p N + r] = (1/N) Σ_c part[(p corr_chunks(N) + c) N + r], c ascending
void launch_corr_sum(const double2* part, int N, int npairs, double2* out, hipStream_t s);
// out[k N + i] = Σ_t a_{i,t} ρ[c(i,t), r(i,t)] over the terms of family k at site i
void launch_corr_mean(const double2* rho, int N, const int* tptr, const int* trow, const int* tcol,
                      const double2* tval, int nfam, double2* out, hipStream_t s);

// Eigendecomposition leapfrog step (algo eig; U, JU, rho: nc chains of n2 x n2
// column-major, E: nc x n2): JU = U diag(logistic(-β E)); after rho = JU U^H,
// P at the bonds, Tr ρ_hh and E_f per chain
void launch_eig_scale(const double2* U, double2* JU, const double* E, int N, int nc, double beta, hipStream_t s);
void launch_eig_gather(const double2* rho, const double* E, int N, int nc, const int* Dcol, const int* bond_ij,
                       double beta, double2* Pair, double* Ef, double* Trhh, hipStream_t s);

// *bad = 1 when any entry of U (nu complex) or E (ne real) is not finite
void launch_nonfinite(const double2* U, int64_t nu, const double* E, int64_t ne, int* bad, hipStream_t s);

// Hermitian eigensolver (dwhmc_eig.hip): m matrices of order n <= kEigMaxN,
// column-major, per-matrix stride sA (complex) / sZ (double)
constexpr int kEigTB = 64;                  // trailing-update tile (one workgroup; hemv partial slots)
constexpr int kEigNB = 64;                  // reflectors per back-transform block
constexpr int kEigMaxN = 5120;              // rows k_eig_step holds in registers
// eigenvalue gap / ||T|| below which inverse-iteration vectors are
// orthonormalised together (Cholesky QR); wider gaps leave overlaps <= ~eps /
// 1e-6 that the symmetric orthogonalisation step squares away.  (2.5e-4 in
// round 3 made runs of >64 "clustered" levels from n ~ 3000 on; runs that
// long are now orthonormalised by the host-driven Cholesky QR.)
constexpr double kEigClusterTol = 1e-6;
// Inside such a run the inverse-iteration shifts are kept at least this x
// ||T|| apart (eig_cluster_shift; xSTEIN's perturbation of close eigenvalues):
// above the ulp spread of an exactly degenerate level's bisected values, so
// that its members do not all weight the eigenspace alike and come out nearly
// parallel; levels that bisection resolves by more keep their own values.
constexpr double kEigClusterSep = 8 * 2.220446049250313e-16;
// The shift of level j of the ascending E[0, n) (jlo: the first index whose
// vector is computed): sigma_j = max(E_j, sigma_{j-1} + sep) along the run that
// j belongs to, in closed form max_i (E_i + (j - i) sep) over the run's levels
// i <= j.  E_j itself outside runs (one comparison).
__host__ __device__ inline double eig_cluster_shift(const double* E, int j, int jlo, double tn) {
  const double ctol = kEigClusterTol * tn, sep = kEigClusterSep * tn;
  double lam = E[j];
  for (int i = j; i > jlo && E[i] - E[i - 1] <= ctol; --i) {
    const double c = E[i - 1] + (j - i + 1) * sep;
    lam = c > lam ? c : lam;
  }
  return lam;
}
// the particle-hole half solve computes the partners' vectors itself unless
// the gap below c0 exceeds this (the partner images are not orthogonalised
// against the computed vectors: their overlap is ~eps ||T|| / gap)
constexpr double kEigZeroTol = 2.5e-4;
constexpr int kEigMaxCluster = 64;          // longest such run (else *bad: vendor fallback)
// deferral of the tridiagonalisation's rank-2 pairs (dwhmc_eig.hip): batches
// of kEigDeferMin+ matrices apply them every kEigDefer-th pass (at most
// kEigDeferMax pending); v_j / w_j live in a ring of kEigRing slots per matrix
constexpr int kEigDefer = 8;
constexpr int kEigSwitchM = 512;   // trailing columns a batch runs in the one-matrix scheme (eig_switch_col)
constexpr int kEigDeferMax = 8;
constexpr int kEigRing = kEigDeferMax + 2;
constexpr int kEigGP = (kEigMaxN + 255) / 256;   // k_eig_reduce workgroups per matrix (g partials)
// column i of the tridiagonalisation (k_eig_reduce + k_eig_step): the pass
// partials (+ the read pass's pending-pair corrections) -> pfin, column i with
// the pending pairs -> colfin, then w_{i-1}, v_i (d, e, tau).
// vv, ww: kEigRing x n per matrix (v_j, w_j in slot j % kEigRing);
// dpart: ceil(n / kEigTB) x 2 kEigDeferMax per matrix (a read pass's dots);
// pfin, colfin: n per matrix
void launch_eig_step(double2* A, int n, int i, int64_t sA, const double2* part, int64_t sP, double2* pfin,
                     double2* colfin, double2* vv, double2* ww, double* d, double* e, double2* tau,
                     const double2* dpart, int m, int K, hipStream_t s);
// step i + pass i (one matrix: folded into one pass launch); gpart: 3 kEigGP per matrix
void launch_eig_column(double2* A, int n, int i, int64_t sA, double2* part, int64_t sP, double2* pfin,
                       double2* colfin, double2* vv, double2* ww, double* d, double* e, double2* tau,
                       double2* dpart, double2* gpart, int m, hipStream_t s, int sw);
// first column a batch runs in the one-matrix scheme (eig_switch_col: the last
// kEigSwitchM columns, DWHMC_EIG_SWITCH_M overrides, 0 = none), passed to
// launch_eig_column as sw
int eig_switch_col(int n);
// the pending pairs on the trailing triangle (write passes) + hemv partials of v_i
void launch_eig_pass(double2* A, int n, int i, int64_t sA, double2* part, int64_t sP, const double2* vv,
                     const double2* ww, double2* dpart, int m, int K, hipStream_t s);
// eigenvalues ascending into E, ||T|| bound per matrix into tnorm
void launch_eig_bisect(const double* d, const double* e, int n, double* E, double* tnorm, int m, hipStream_t s);
// eigenvectors of T into Zt (Zt[r n + j]: component r of vector j), clusters orthonormalised;
// a cluster longer than maxc (<= kEigMaxCluster) sets *bad (the caller's vendor fallback)
// Only the indices [j0, n), and with c0 (per matrix, device) only those >= c0
// (the columns j0 <= j < c0 of Zt are zeroed): the particle-hole half solve
void launch_eig_invit(const double* d, const double* e, int n, const double* E, const double* tnorm, double* Zt,
                      double* U0, double* U1, double* U2, int64_t sZ, int* bad, int m, hipStream_t s,
                      int maxc = kEigMaxCluster, int j0 = 0, const int* c0 = nullptr);
// columns j < c0[k] of U = the particle-hole partners of columns n-1-j:
// (u; v) -> (-conj v; conj u)
void launch_eig_theta(double2* U, int n, int64_t sA, const int* c0, int m, hipStream_t s);
// U[:, j0:] from Zt[:, j0:] (real -> complex, transposed through LDS)
void launch_eig_zt_to_u(const double* Zt, double2* U, int n, int64_t sZ, int64_t sA, int m, hipStream_t s,
                        int j0 = 0);
constexpr int kEigDeferMin = 4;             // batches from this many matrices defer their rank-2 pairs
int eig_defer_k(int m);                     // deferral depth for m matrices (1: none)
constexpr int kEigGS = 8;                   // row slices of each block's Gram sum
// compact-WY T of every reflector block; Gp: m x nblk x kEigGS x kEigNB^2 scratch
void launch_eig_tfac(const double2* V, int n, int64_t sA, const double2* tau, double2* Gp, double2* Tb, int64_t sT,
                     int m, hipStream_t s);
// W2 (kb x n, ld kEigNB) = T (sum of the S row chunks of W, chunk s at rows s kb, ld ldw)
// the reflector blocks of V conjugate-transposed (block b at Vt + b kEigNB n,
// leading dimension kEigNB), for the back-transform's W = V^H U
void launch_eig_vt(const double2* A, int n, int64_t sA, double2* Vt, int m, hipStream_t s);
void launch_eig_tw(const double2* Tb, int64_t sT, const double2* W, int ldw, int64_t sW, int S, int kb, int n,
                   double2* W2, int64_t sW2, int m, hipStream_t s);

// Structure-preserving (quaternion) eigensolver (dwhmc_qeig.hip): m matrices
// of order n = 2M, column-major at stride sA, reduced site by site on their
// particle rows (A's bottom rows then hold the reflectors); part: q_part_elems
// per matrix (stride sP); W: 2M per matrix; tau, qa: M; Y: 2M; qd: M
int q_part_elems(int M);
bool q_supported(int M);   // sites per matrix the reduction takes (1 .. 3072)
#ifdef QSTAMPS
int q_stamps_read(unsigned long long* out, int nsteps);   // diagnostic builds (-DQSTAMPS)
#endif
void launch_q_reduce(double2* A, int M, int64_t sA, double2* part, int64_t sP, double2* W, double* tau, double2* Y,
                     double* qa, double2* qd, int m, hipStream_t s);
// site rotations: (ra, rd, rb) = T's blocks (a', d', b), G: per site (al, be)
void launch_q_rot(const double* qa, const double2* qd, const double2* Y, int M, double* ra, double2* rd, double* rb,
                  double2* G, int m, hipStream_t s);
// the 2M eigenvalues of T ascending into E (stride 2M), ||T|| bound into tnorm
void launch_q_bisect(const double* ra, const double2* rd, const double* rb, int M, double* E, double* tnorm, int m,
                     hipStream_t s);
// eigenvectors of the particle-hole half (E indices j0 .. 2M-1, nv = 2M - j0):
// inverse iteration into Zt (row r of vector jj at Zt[r nv + jj], interleaved
// rows 2s / 2s+1 = particle / hole of site s; LU scratch S: q_invit_scratch
// double2 per matrix)
int64_t q_invit_scratch(int M, int j0);
void launch_q_invit(const double* ra, const double2* rd, const double* rb, int M, const double* E, const double* tnorm,
                    int j0, double2* Zt, int64_t sZ, double2* S, int64_t sS, int m, hipStream_t s);
// the vectors of eigenvalue clusters (gaps <= ctol ||T||, at most q_max_cluster()
// long) orthonormalised in Zt (two rounds of Cholesky QR); *bad = 1 on failure
int q_max_cluster();
// the crowd at zero of one matrix's eigenvalues E (n, computed from j0): the
// number of levels k_q_orth orthonormalises with their Theta partners, 0: none
int q_zero_crowd(const double* E, int n, int j0, double tn);
void launch_q_orth(const double* E, const double* tnorm, int M, int j0, double2* Zt, int64_t sZ, double ctol, int* bad,
                   int m, hipStream_t s);
// U' columns j0.. (n x n, interleaved rows) = site rotations G of Yt (nv x n, ld nv)
void launch_q_ztu(const double2* Yt, int64_t sY, const double2* G, int M, int j0, double2* U, int64_t sU, int m,
                  hipStream_t s);
// the reflector pairs as the one-stage back-transform's V (n x n, interleaved
// rows; columns 2j, 2j+1 = v_j, Theta v_j) and complex tau (n per matrix)
void launch_q_vexpand(const double2* A, int64_t sA, const double* tau, int M, double2* V, double2* tauc, int m,
                      hipStream_t s);
// U (BdG order) from U' (interleaved): columns >= j0 copied, below j0 the Theta partners
void launch_q_final(const double2* Ui, int64_t sU, int M, int j0, double2* U, int m, hipStream_t s);

// The library's own batched fp64 products (dwhmc_gemm.hip):
// C = alpha op(A) op(B) + beta C, column-major, op 'N' or 'C' (conjugate
// transpose; 'T' for real), per-matrix strides sA / sB / sC (elements)
void gemm_z(char opa, char opb, int M, int N, int K, double2 alpha, const double2* A, int lda, int64_t sA,
            const double2* B, int ldb, int64_t sB, double2 beta, double2* C, int ldc, int64_t sC, int batch,
            hipStream_t s);
// two-level batch: batch x S products, operands at outer * x2 + s * x1; the
// last inner one (s = S - 1) with K = Klast
void gemm_z_chunked(char opa, char opb, int M, int N, int K, int Klast, int S, double2 alpha, const double2* A,
                    int lda, int64_t a1, int64_t a2, const double2* B, int ldb, int64_t b1, int64_t b2,
                    double2 beta, double2* C, int ldc, int64_t c1, int64_t c2, int batch, hipStream_t s);
void gemm_d(char opa, char opb, int M, int N, int K, double alpha, const double* A, int lda, int64_t sA,
            const double* B, int ldb, int64_t sB, double beta, double* C, int ldc, int64_t sC, int batch,
            hipStream_t s);

int selftest_mfma_layout(int device);

}  // namespace dwh
