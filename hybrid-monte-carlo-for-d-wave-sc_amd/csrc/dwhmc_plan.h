// The cyclic-reduction plan of the C-ABI context (dwhmc_plan.cpp): the choice
// of algorithm and guard, and plan_cr, the one entry point that turns a
// lattice into what the CR launches index by — block geometry, the stage list
// build_cr_plan derives, the product stages' configurations and the
// dispatch-ordered slots of the 16 x 16 stages — plus the sparse level-0
// operand arrays.  Context creation and the host-only checks
// (dwh_debug_cr_plan_*) go through the same plan_cr.  Pure host index
// arithmetic: needs no device.  Not part of the public ABI.
#pragma once
#include <cstdint>
#include <set>
#include <vector>

#include "dwhmc_internal.h"

namespace dwh {

// One stage of the cyclic-reduction plan: a batch of block inversions or a
// task list of block products (all batch items at once).
struct CrStage {
  int kind;        // 0 inversion, 1 products
  int first, n;    // range in CrPlan::inv_blk / CrPlan::tasks
  double sg;       // products: sign of the sum
  double flops;    // products: algorithmic fp64 flops per batch item (restricted ranges)
  int maxt32, maxt16, ntmax;
  int tfirst, ntiles;   // products: range in CrPlan::tiles16 (the stage's (task, tile) pairs);
                        // inversions: their side-work tasks in CrPlan::tasks (launch_cr_inv_side,
                        // maxt32 tiles each), flops in `flops`
  dwh::CrGemmCfg cfg;   // products: tile / K-split chosen once per context
  int sfirst = 0, nswg = 0;   // 16 x 16 products: their dispatch-ordered slots (CrPlan::slots, nswg workgroups)
  int l0 = 0;           // inversions: level 0 from the static R = A^-1 blocks (k_cr_inv0)
  int sp = 0;           // kind 2 (sparse level-0 stage): 0 forward (CrPlan::sp_fwd), 1 backward (sp_bwd)
  int store = dwh::kStorePlain;        // cache policy of the launch's pool stores (cr_store_policies)
  int store_side = dwh::kStorePlain;   // inversions with side work: of the side products' stores
};

struct CrPlan {
  int nblk = 0;
  std::vector<CrStage> stages;
  std::vector<dwh::CrTask> tasks;
  std::vector<dwh::CrTile> tiles16;          // per product stage: its 16 x 16 tiles with their operands
  std::vector<dwh::CrSlot> slots;            // per 16 x 16 product stage: its tiles of every batch item,
                                             // dispatch order (dwh::cr_gemm_slots; built with the stage configs)
  std::vector<int> inv_blk, inv_dst, inv_slot;   // inversion source / destination block, ln|det| slot
  std::vector<int> inv0_r;                       // level-0 inversions (l0 stage): R = A^-1 block per entry
  std::vector<int64_t> goff, doff;
  std::vector<int> fill_all, fill_step;      // level-0 blocks written at create / every step
  std::vector<int64_t> off_ph;               // pairing entries outside fill_step (-1: none)
  int n_ph = 0;                              // entries of off_ph >= 0
  // sparse level 0 (dwhmc_cr_sparse.hip): the stages' tasks and the level-0
  // U / L patterns (CrPlan::rowpat / colpat: [3 Ly][kCrSpNZ][BP])
  std::vector<dwh::CrSpFwd> sp_fwd;
  std::vector<dwh::CrSpBwd> sp_bwd;
  std::vector<int> rowpat, colpat;
  int store_force = dwh::kStorePlain;   // k_cr_pair_force's Δ/2 scatter into the level-0 blocks
};

// What one launch of the step leaves behind: the bytes a stage writes per
// batch item (whole blocks for the inversions, the sparse stages and the side
// products; the 16 x 16 tiles of a product stage) and how many launches later
// the first of them is read (1: by the very next launch; the force gather
// follows the last stage; kCrNeverRead: by nothing the step launches) and how
// many of the bytes the very next launch reads, for the stage's own outputs
// and for its side products.
constexpr int kCrNeverRead = 1 << 20;
struct CrStageStores {
  int64_t bytes = 0, bytes_side = 0, bytes_next = 0, bytes_side_next = 0;
  int first_read = kCrNeverRead, first_read_side = kCrNeverRead;
};
std::vector<CrStageStores> cr_stage_stores(const CrPlan& pl, int BP);

// The sparse stages' per-task operand arrays (launch_cr_sp_fwd / _bwd,
// dwhmc_internal.h).  Per task: one host-resolved record per output row
// (rf / rb: [task][row r < HP], dwh::CrSpRowFwd / CrSpRowBwd) holding the row
// of each left sparse operand and the task's dense row offsets; and the
// column entries of its right operands, [operand][entry][column], value (cv)
// and meta word (cm: Δ index + 1 | op << 22 | row << 24), read coalesced
// (forward tasks first; the backward ones from col_bwd0).
struct SpTaskArrays {
  std::vector<dwh::CrSpRowFwd> rf;
  std::vector<dwh::CrSpRowBwd> rb;
  std::vector<int> cm;
  std::vector<double2> cv;
  size_t col_bwd0 = 0;
};

// Lx, Ly: the CR lattice (CrDims); the tables are the host model's
SpTaskArrays cr_sparse_task_arrays(const CrPlan& pl, int Lx, int Ly, int BP, const std::vector<int>& hcol,
                                   const std::vector<double>& hval, const std::vector<int>& Dcol,
                                   const std::vector<int>& Dsrc);
// column-pattern values of the level-0 U / L blocks (static hopping value, or
// the Δ index of a pairing entry) in the kernels' [block][entry][BP] order
void cr_sparse_colvals(const std::vector<int>& colpat, int Lx, int Ly, int BP, const std::vector<int>& hcol,
                       const std::vector<double>& hval, const std::vector<int>& Dcol, const std::vector<int>& Dsrc,
                       std::vector<double2>& colval, std::vector<int>& colsrc);
// The pieces of a 16 x 16 product stage the planner and the kernel test entry
// (dwh_debug_cr_launch) share: a task's 16 x 16 tiles (window rounded out to
// whole tiles, row-major; keep, nullable: only the tiles tr * ntc + tc it
// holds; returns the number appended), the stage's workgroup count and its
// dispatch-ordered slots (cr_gemm_slot_wgs x 4 / ksplit of them).
int cr_task_tiles16(const CrTask& t, int ntc, const std::set<int>* keep, std::vector<CrTile>* out);
int cr_gemm_slot_wgs(const CrDims& c, int ntl16, const CrGemmCfg& cfg);
void cr_gemm_slots(const CrDims& c, const CrTile* tl16, int ntl16, const CrGemmCfg& cfg, CrSlot* out);
// lattice rows per CR block; 0: a lattice row does not fit a supported block
// (2 Lx > 128), the CR path cannot run this lattice
int cr_rows_per_block(int64_t Lx, int64_t Ly);

// Which path a context runs and which guard protects it.  want: algo_req, or
// (DWH_ALGO_AUTO) DWHMC_ALGO = auto | dense | cr | eig.  auto runs cr when the
// lattice fits a CR block (cr_ok), else dense, and eig when the pole selection
// finds kappa beyond the table.  The site guard goes with the CR path (its
// level-0 inversion launch checks it) unless the poles end on eig.
struct AlgoChoice {
  int32_t want = 0;   // DWH_ALGO_*
  bool cr_ok = false, site_guard = false;
};
int choose_algo(int32_t algo_req, int64_t Lx, int64_t Ly, AlgoChoice* out);

// The CR path's whole host side for an Lx x Ly lattice with P poles and nbatch
// = chains x P batch items: the block geometry (*c), the stage list, each
// product stage's configuration and the dispatch-ordered slots of the 16 x 16
// stages.  side / inv0: side work on the inversion launches / level-0
// inversions from the static R blocks, where the block size supports them;
// kCrFromEnv: on unless DWHMC_CR_SIDE=0 / DWHMC_CR_INV0=0 (A/B runs, tests).
// DWHMC_CR_INV32=0: BP = 32 inversions by k_cr_inv<2>.  DWHMC_CR_STORE=0: every
// launch stores plain (else the plan's store policies).  DWH_ERR_ARG: a lattice
// row too wide, or a batch item of 2^32 elements or more.
constexpr int kCrFromEnv = -1;
int plan_cr(int64_t Lx, int64_t Ly, int P, int nbatch, const std::vector<int>& Dcol, const std::vector<int>& hcol,
            int side, int inv0, int ncu, CrDims* c, CrPlan* pl);
// DWHMC_CR_PLAN_DUMP=1: one line per stage to stderr (nbatch inversion
// workgroups per block; cfg: the product stages' configurations are chosen)
void cr_plan_dump(const CrPlan& pl, int64_t nbatch, bool cfg);

}  // namespace dwh
