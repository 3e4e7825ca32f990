// The cyclic-reduction plan (dwhmc_plan.h): block cyclic reduction of the
// periodic block-tridiagonal H_BdG - i y into launch stages, the sparse
// level-0 patterns, the product stages' configuration and dispatch-ordered
// slots — all behind plan_cr, which context creation and the host-only dataflow
// check of a plan (dwh_debug_cr_plan_*) both call — and choose_algo.
// Index arithmetic only — no device call, no vendor library:
// tools/host_check/plan_main.cpp links this file and dwhmc_model.cpp alone.
#include "dwhmc_plan.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <set>
#include <string>
#include <utility>

#include "../../include/dwhmc.h"
#include "dwhmc_model.h"

namespace dwh {

namespace {
// Top-half row r of level-0 block b (U[y]: Ly + y, L[y]: 2 Ly + y) in the
// records' canonical slot order (cr_sparse_patterns guarantees it fits):
// hopping entries (particle columns k < HP) with their static values, exactly
// as k_cr_fill resolves them (the last matching table slot), then the one
// pairing entry (hole column HP + k): the Δ index whose Δ/2 the pool holds.
struct SpRow {
  double hv[dwh::kCrSpNZ - 1] = {};
  int hk[dwh::kCrSpNZ - 1] = {};   // dense operand row of each hopping slot (0: empty)
  double ps = 0.0;                 // 1/2, or 0: no pairing entry
  int pk = 0, pd = 0;              // pairing: dense operand row HP + pk, Δ index
};
SpRow sp_row(const std::vector<int>& rowpat, int b, int r, int Lx, int Ly, int BP, const std::vector<int>& hcol,
             const std::vector<double>& hval, const std::vector<int>& Dcol, const std::vector<int>& Dsrc) {
  const int NZ = dwh::kCrSpNZ, HP = BP / 2, t = b / Ly, y = b % Ly;
  const int yr = (t == 2) ? (y + 1) % Ly : y, yc = (t == 1) ? (y + 1) % Ly : y;
  SpRow s;
  int nh = 0;
  for (int e = 0; e < NZ; ++e) {
    const int w = rowpat[((size_t)b * NZ + e) * BP + r];
    if (((w >> 22) & 3) == 3) continue;
    const int k = (w >> 14) & 0xff, i = yr * Lx + r;   // top rows: op 0, the stored element (r, k)
    if (k < HP) {
      if (nh >= NZ - 1) continue;
      const int j = yc * Lx + k;
      double h = 0.0;
      for (int sl = 0; sl < kHSlots; ++sl)
        if (hcol[(size_t)i * kHSlots + sl] == j) h = hval[(size_t)i * kHSlots + sl];
      s.hv[nh] = h;
      s.hk[nh++] = k;
    } else {
      const int j = yc * Lx + (k - HP);
      int src = -1;
      for (int sl = 0; sl < kSlots; ++sl)
        if (Dcol[(size_t)i * kSlots + sl] == j) src = Dsrc[(size_t)i * kSlots + sl];
      s.pk = k - HP;
      if (src >= 0) {
        s.ps = 0.5;
        s.pd = src;
      }
    }
  }
  return s;
}
}  // namespace

SpTaskArrays cr_sparse_task_arrays(const CrPlan& pl, int Lx, int Ly, int BP, const std::vector<int>& hcol,
                                   const std::vector<double>& hval, const std::vector<int>& Dcol,
                                   const std::vector<int>& Dsrc) {
  const int NZ = dwh::kCrSpNZ, E = NZ * BP, HP = BP / 2;
  SpTaskArrays a;
  if (pl.colpat.empty()) return a;
  std::vector<double2> colval;
  std::vector<int> colsrc;
  cr_sparse_colvals(pl.colpat, Lx, Ly, BP, hcol, hval, Dcol, Dsrc, colval, colsrc);
  auto row = [&](int b, int r) { return sp_row(pl.rowpat, b, r, Lx, Ly, BP, hcol, hval, Dcol, Dsrc); };
  // byte offset of row k of pool block b from the batch item's base
  auto at = [&](int b, int k) { return (uint32_t)(((int64_t)b * HP + k) * BP * (int64_t)sizeof(double2)); };
  auto cols = [&](int cb) {
    for (int k = cb * E; k < (cb + 1) * E; ++k) {
      const int w = pl.colpat[k], op = (w >> 22) & 3, idx = (w >> 14) & 0xff, src = colsrc[k];
      a.cv.push_back(colval[k]);
      a.cm.push_back((src < 0 ? 0 : src + 1) | op << 22 | idx << 24);
    }
  };
  for (const dwh::CrSpFwd& t : pl.sp_fwd) {
    const int sparse[3] = {t.uk, t.ler, t.lel}, dense[3] = {t.dir, t.dir, t.dil};
    for (int r = 0; r < HP; ++r) {
      dwh::CrSpRowFwd q{};
      for (int o = 0; o < 3; ++o) {
        const SpRow s = row(sparse[o], r);
        for (int e = 0; e < NZ - 1; ++e) {
          q.hv[o][e] = -s.hv[e];   // V = -U Dinv, -L Dinv
          q.ho[o][e] = at(dense[o], s.hk[e]);
        }
        q.ps[o] = -s.ps;
        q.po[o] = at(dense[o], s.pk);
        q.pd[o] = (uint32_t)s.pd;
      }
      q.dk = at(t.dk, r);
      q.od = at(t.od, r);
      q.ou = at(t.ou, r);
      q.ol = at(t.ol, r);
      a.rf.push_back(q);
    }
    cols(t.lk);
    cols(t.uel);
    cols(t.uer);
  }
  a.col_bwd0 = a.cv.size();
  for (const dwh::CrSpBwd& t : pl.sp_bwd) {
    const int sparse[2] = {t.la, t.ue}, dense[2][2] = {{t.gaa, t.gac}, {t.gca, t.gcc}};
    for (int r = 0; r < HP; ++r) {
      dwh::CrSpRowBwd q{};
      for (int o = 0; o < 2; ++o) {
        const SpRow s = row(sparse[o], r);
        for (int g = 0; g < 2; ++g) {
          for (int e = 0; e < NZ - 1; ++e) q.ho[o][g][e] = at(dense[o][g], s.hk[e]);
          q.po[o][g] = at(dense[o][g], s.pk);
        }
        for (int e = 0; e < NZ - 1; ++e) q.hv[o][e] = s.hv[e];
        q.ps[o] = s.ps;
        q.pd[o] = (uint32_t)s.pd;
      }
      q.g[0] = at(t.gaa, r);
      q.g[1] = at(t.gca, r);
      q.g[2] = at(t.gac, r);
      q.g[3] = at(t.gcc, r);
      q.oza = at(t.oza, r);
      q.ozc = at(t.ozc, r);
      q.oya = at(t.oya, r);
      q.oyc = at(t.oyc, r);
      q.omx = at(t.omx, r);
      a.rb.push_back(q);
    }
    cols(t.ua);
    cols(t.le);
  }
  return a;
}

namespace {
// Nonzero patterns of the level-0 U[y] = A[y, y+1] (pool block Ly + y) and
// L[y] = A[y+1, y] (2 Ly + y) blocks, from the hopping / pairing tables
// exactly as k_cr_fill writes them (top half: hopping at (x, x_j), pairing at
// (x, HP + x_j) for partners j in the other row), as entries of the FULL
// block: row x of the top half, and row HP + x synthesised from it (M-form:
// [conj B | -conj A]).  Entry = top-half offset | (column for rowpat, row for
// colpat) << 14 | op << 22 (op 0 as stored, 1 conj, 2 -conj, 3 empty).  False when a
// row or column holds more than kCrSpNZ entries, or a top-half row more than
// kCrSpNZ - 1 hopping entries or more than one pairing entry (the dense level
// 0 then runs).
bool cr_sparse_patterns(int Lx, int Ly, int BP, const std::vector<int>& hcol, const std::vector<int>& Dcol,
                        std::vector<int>& rowpat, std::vector<int>& colpat) {
  const int HP = BP / 2, NZ = dwh::kCrSpNZ;
  const int empty = 3 << 22;   // op 3: weight zero (dwhmc_cr_sparse.hip sp_val)
  rowpat.assign((size_t)3 * Ly * NZ * BP, empty);
  colpat.assign((size_t)3 * Ly * NZ * BP, empty);
  for (int t = 1; t <= 2; ++t)
    for (int y = 0; y < Ly; ++y) {
      if ((t == 1 && Ly < 2) || (t == 2 && Ly < 3)) continue;   // k_cr_fill's zero blocks
      const int b = t * Ly + y;
      const int yr = (t == 2) ? (y + 1) % Ly : y, yc = (t == 1) ? (y + 1) % Ly : y;
      std::set<std::pair<int, int>> top;
      for (int x = 0; x < Lx; ++x) {
        const int i = yr * Lx + x;
        for (int s = 0; s < kHSlots; ++s) {
          const int j = hcol[(size_t)i * kHSlots + s];
          if (j >= 0 && j / Lx == yc) top.insert({x, j % Lx});
        }
        for (int s = 0; s < kSlots; ++s) {
          const int j = Dcol[(size_t)i * kSlots + s];
          if (j >= 0 && j / Lx == yc) top.insert({x, HP + j % Lx});
        }
      }
      // canonical form of the row records (dwh::CrSpRowFwd / Bwd): a top-half
      // row holds at most NZ - 1 hopping entries and one pairing entry
      std::vector<int> nhop(HP, 0), npair(HP, 0);
      for (const auto& xc : top)
        if (++(xc.second < HP ? nhop : npair)[xc.first] > (xc.second < HP ? NZ - 1 : 1)) return false;
      std::vector<int> rn(BP, 0), cn(BP, 0);
      auto put = [&](int r, int c, int off, int op) {
        if (rn[r] >= NZ || cn[c] >= NZ) return false;
        rowpat[((size_t)b * NZ + rn[r]++) * BP + r] = off | (c << 14) | (op << 22);
        colpat[((size_t)b * NZ + cn[c]++) * BP + c] = off | (r << 14) | (op << 22);
        return true;
      };
      for (const auto& xc : top) {
        const int x = xc.first, c = xc.second, off = x * BP + c;
        if (!put(x, c, off, 0)) return false;
        if (!(c >= HP ? put(HP + x, c - HP, off, 1) : put(HP + x, c + HP, off, 2))) return false;
      }
    }
  return true;
}
}  // namespace

// Column-pattern values of the level-0 U / L blocks in the kernels' own
// [block][entry][BP] order, so the dense . sparse products read them
// coalesced instead of gathering one pool row per lane: the static hopping
// entries as stored (op applied; chain-independent: U / L hold no diagonal),
// and for the pairing entries the Δ index whose Δ/2 k_cr_fill / the force
// scatter writes there (src, the kernel applies op), exactly as k_cr_fill
// resolves both (the last matching table slot).
void cr_sparse_colvals(const std::vector<int>& colpat, int Lx, int Ly, int BP, const std::vector<int>& hcol,
                       const std::vector<double>& hval, const std::vector<int>& Dcol, const std::vector<int>& Dsrc,
                       std::vector<double2>& colval, std::vector<int>& colsrc) {
  const int HP = BP / 2, NZ = dwh::kCrSpNZ;
  colval.assign(colpat.size(), make_double2(0.0, 0.0));
  colsrc.assign(colpat.size(), -1);
  for (int t = 1; t <= 2; ++t)
    for (int y = 0; y < Ly; ++y) {
      const int b = t * Ly + y;
      const int yr = (t == 2) ? (y + 1) % Ly : y, yc = (t == 1) ? (y + 1) % Ly : y;
      for (int e = 0; e < NZ; ++e)
        for (int c = 0; c < BP; ++c) {
          const size_t k = ((size_t)b * NZ + e) * BP + c;
          const int w = colpat[k], op = (w >> 22) & 3;
          if (op == 3) continue;
          const int off = w & 0x3fff, x = off / BP, ct = off % BP;
          const int i = yr * Lx + x;
          if (ct < HP) {
            const int j = yc * Lx + ct;
            double h = 0.0;
            for (int sl = 0; sl < kHSlots; ++sl)
              if (hcol[(size_t)i * kHSlots + sl] == j) h = hval[(size_t)i * kHSlots + sl];
            colval[k] = make_double2(op == 2 ? -h : h, 0.0);
          } else {
            const int j = yc * Lx + (ct - HP);
            int src = -1;
            for (int sl = 0; sl < kSlots; ++sl)
              if (Dcol[(size_t)i * kSlots + sl] == j) src = Dsrc[(size_t)i * kSlots + sl];
            colsrc[k] = src;
          }
        }
    }
}

namespace {
// nonzeros of row r / column c of level-0 block b in the patterns
int sp_nrow(const std::vector<int>& pat, int b, int r, int BP) {
  int n = 0;
  for (int e = 0; e < dwh::kCrSpNZ; ++e) n += ((pat[((size_t)b * dwh::kCrSpNZ + e) * BP + r] >> 22) & 3) != 3;
  return n;
}
}  // namespace

// Lattice rows per CR block.  Default: as many rows as fill the narrowest
// block half (16 sites) — R = 16 / Lx, lowered to a divisor of Ly — so a
// lattice with Lx <= 8 runs fewer, unpadded blocks at no extra cost per block
// (8 x 8: 4 blocks of two rows instead of 8 half-empty ones, one CR level
// less).  Wider lattices keep one row per block: more rows would widen the
// blocks, and at L = 16 two rows per block (BP 64) measured slower than one
// (profiles/r04_exp_cr_two_row_blocks_C2.txt).  0: not even one row fits a
// supported block size.
int cr_rows_per_block(int64_t Lx, int64_t Ly) {
  auto ok = [&](int64_t r) { return r >= 1 && Ly % r == 0 && dwh::cr_supported_bp((int)(2 * ((r * Lx + 15) / 16 * 16))); };
  int64_t r = std::max<int64_t>(1, 16 / Lx);
  while (r > 1 && !ok(r)) --r;
  return ok(r) ? (int)r : 0;
}

int choose_algo(int32_t algo_req, int64_t Lx, int64_t Ly, AlgoChoice* out) {
  std::string want = "auto";
  if (algo_req == DWH_ALGO_DENSE) want = "dense";
  else if (algo_req == DWH_ALGO_CR) want = "cr";
  else if (algo_req == DWH_ALGO_EIG) want = "eig";
  else if (const char* e = std::getenv("DWHMC_ALGO")) want = e;
  if (want != "auto" && want != "dense" && want != "cr" && want != "eig")
    return fail(nullptr, DWH_ERR_ARG, "DWHMC_ALGO must be auto, dense, cr or eig");
  out->want = want == "dense" ? DWH_ALGO_DENSE : want == "cr" ? DWH_ALGO_CR : want == "eig" ? DWH_ALGO_EIG : DWH_ALGO_AUTO;
  out->cr_ok = cr_rows_per_block(Lx, Ly) > 0;
  out->site_guard = out->want == DWH_ALGO_CR || (out->want == DWH_ALGO_AUTO && out->cr_ok);
  return DWH_OK;
}

// The 16 x 16 output tiles of task t — its window rounded out to whole tiles,
// row-major — appended to *out with the task's operands; keep (nullable): only
// the tiles tr * ntc + tc it holds.  Returns the number appended.  Shared by
// the planner's product stages and dwh_debug_cr_launch.
int cr_task_tiles16(const CrTask& t, int ntc, const std::set<int>* keep, std::vector<CrTile>* out) {
  const int nk = dwh::cr_task_tiles(t, 16), ct = (t.c1 + 15) / 16 - t.c0 / 16;
  int kept = 0;
  for (int k = 0; k < nk; ++k) {
    const int tr = t.r0 / 16 + k / ct, tc = t.c0 / 16 + k % ct;
    if (keep && !keep->count(tr * ntc + tc)) continue;
    dwh::CrTile d{};
    d.out = t.out;
    d.cin = t.cin;
    d.nt = t.nt;
    d.bq = t.bq;
    for (int h = 0; h < 4; ++h) {
      d.a[h] = t.a[h];
      d.b[h] = t.b[h];
    }
    d.tr = tr;
    d.tc = tc;
    out->push_back(d);
    kept++;
  }
  return kept;
}

// Block cyclic reduction of the periodic block-tridiagonal H_BdG - i y (blocks
// = lattice rows) into stages; restates tools/cr_model.py
// cr_selected_inverse_top (checked there against dense inverses for Ly = 1 ..
// 24, odd and even).  Blocks are top halves (HP x BP); V, W are Q-form, every
// other block M-form (the form of each right operand goes into CrTask::bq).  Pool blocks:
// level-0 D[y] = y, U[y] = Ly + y, L[y] = 2 Ly + y (filled by k_cr_fill).
// Forward level (m blocks, eliminate odd e < m - m%2, keep even k):
//   inv D_e;  V1 = -U_a D_e^-1, V2 = -L_e D_e^-1, W1 = -D_e^-1 L_a, W2 = -D_e^-1 U_e
//   D'_k = D_k + V1(k+1) L_k + V2(k-1) U_(k-1);  U'_k = V1(k+1) U_(k+1);  L'_k = V2(k+1) L_k
//   (m = 2 folds the self-couplings of the 1-block chain into D': 4 terms)
// Backward (G of the next level known at its kept blocks and adjacent pairs):
//   G_ea = W1 G_aa + W2 G_ca,  G_ec = W1 G_ac + W2 G_cc,
//   G_ae = G_aa V1 + G_ac V2,  G_ce = G_ca V1 + G_cc V2,  G_ee = D_e^-1 + W1 G_ae + W2 G_ce.
//
// side: products off the critical path (W1/W2: operands of the backward pass
// only; U'/L': operands of the next level's products, which follow its
// inversion) leave the product stages and run as side work of a later
// inversion stage, on the CUs its few inversion workgroups leave idle; the
// product stages on the critical path keep only V1/V2 and D'.  Levels down
// to m = 4 (below that the stages are pure latency) and only where the
// receiving inversion stage leaves a quarter of the ncu CUs idle (nbatch =
// chains x poles inversion workgroups per block).
// side_woff = 2: inversion stages between a level and the one that runs its
// W products; side_m = 4: smallest level size m whose products move
// (profiles/r02_exp_cr_side_work.txt, r04_exp_cr_side_knobs_C3.txt).
//
// inv0: the level-0 inversions use static R = A^-1 blocks (k_cr_inv0), one
// per eliminated row, computed at context creation.
//
// Lx, Ly: the CR lattice — a block holds Lx consecutive sites of the linear
// site index i = y * Lx + x, i.e. R = Lx / Lx_lattice lattice rows when the
// context groups rows (cr_rows_per_block): every coupling stays between
// neighbouring blocks (hopping and pairing span one lattice row), so the
// recursion is the same; only which entries of the level-0 G blocks the
// force reads changes (computed from Dcol below, not assumed diagonal).
CrPlan build_cr_plan(int Lx, int Ly, int BP, const std::vector<int>& Dcol, bool side, int nbatch,
                     int ncu, bool inv0, const std::vector<int>* hcol) {
  // W products two inversion stages after their level, side work from m = 4
  // (profiles/r02_exp_cr_side_work.txt, r04_exp_cr_side_knobs_C3.txt)
  constexpr int side_woff = 2, side_m = 4;
  CrPlan pl;
  const int HP = BP / 2;
  // sparse level 0 (dwhmc_cr_sparse.hip): even Ly >= 4, a supported block,
  // patterns within kCrSpNZ, and BP >= 64 — at BP = 32 the dense level-0
  // products are cheaper than the two sparse launches (C2 L = 16: 10.3k vs
  // 9.5k steps/s; C3 L = 32: 3.82k vs 3.74k; C5 L = 48: 1.27k vs 1.08k,
  // profiles/r05_exp_sparse_level0.txt).  DWHMC_CR_SPARSE0=1 / 0 forces it
  // on (any supported BP) / off.
  const bool sparse0 = [&] {
    const char* e = std::getenv("DWHMC_CR_SPARSE0");
    const bool force = e && *e == '1';
    if ((e && *e == '0') || !hcol || Ly % 2 != 0 || Ly < 4 || !dwh::cr_supported_sparse0(BP)) return false;
    if (!force && BP < 64) return false;
    return cr_sparse_patterns(Lx, Ly, BP, *hcol, Dcol, pl.rowpat, pl.colpat);
  }();
  if (!sparse0) {
    pl.rowpat.clear();
    pl.colpat.clear();
  }
  // Backward merge (round 6): the G_ee stage of a coarse level u runs inside
  // the first backward stage of the next finer level f (m_f <= merge_max_m,
  // not level 0), one launch less per merged pair.  f's products that would
  // read G_ee(u) = Dinv + W1 G_ae + W2 G_ce = Dinv + G_ea V1 + G_ec V2 (u's
  // quantities at that position) read its expansion instead:
  //   W G_ee = (W Dinv) + (W W1) G_ae + (W W2) G_ce,
  //   G_ee V = (Dinv V) + G_ea (V1 V) + G_ec (V2 V),
  // the three forward products of each (W Dinv as the accumulate input)
  // formed off the critical path: side work of the final inversion (BP = 64)
  // or inside the top level's D' stage (other BP), while their cost fits
  // (tools/cr_model.py cr_flop_count restates the policy).
  // Default: levels up to m_f = 4 with side work (BP = 64; C3 +0.4 %, m_f = 8
  // -0.3 %: its products lengthen the final inversion and the merged m = 8
  // stage runs several workgroup rounds), up to 8 without (C2 +3.2 %;
  // profiles/r06_exp_cr_merge.txt).  DWHMC_CR_MERGE=m: levels up to m_f = m
  // (0: every G_ee stage on its own; A/B, tests).
  const int merge_max_m = [&] {
    const char* e = std::getenv("DWHMC_CR_MERGE");
    return e ? std::max(0, std::atoi(e)) : side ? 4 : 8;
  }();
  const bool merge = merge_max_m >= 2;
  auto nr = [&](int b, int r) { return sp_nrow(pl.rowpat, b, r, BP); };
  auto nc = [&](int b, int c) { return sp_nrow(pl.colpat, b, c, BP); };
  int nblk = 3 * Ly;
  std::vector<char> qform(3 * Ly, 0);   // per pool block: Q-form (products V, W)
  auto nb = [&]() {
    qform.push_back(0);
    return nblk++;
  };
  auto nbq = [&]() {
    qform.push_back(1);
    return nblk++;
  };
  struct Level {
    int m;
    std::vector<int> D, U, L, E, K;
    std::vector<int> Dinv;             // block holding D_e^-1 (then G_ee), by position e
    std::vector<int> V1, V2, W1, W2;   // indexed by position e
    std::vector<char> elim;
    bool sparse = false;               // level 0 by the sparse stages (no V / W blocks)
    // backward merge: this level's first backward stage also runs the G_ee
    // stage of the level above; xa / xc[e]: the blocks of the expansion of
    // G_aa / G_cc (when G_ee of the level above): {Dinv V, V1 V, V2 V,
    // W Dinv, W W1, W W2} (-1: none)
    bool merged = false;
    std::vector<std::array<int, 6>> xa, xc;
    std::vector<int> Gea, Gec, Gae, Gce;   // backward outputs by eliminated position
  };
  // Level-0 blocks are inverted out of place (they are never overwritten, so
  // per step only their pairing entries change), coarser blocks in place.
  // Returns the blocks that hold the inverses.
  // pending side work per inversion stage (ordinal: 0 = level 0, ..., the
  // last = the final single-block inversion)
  int n_inv = 1;
  std::vector<int> inv_wgs;   // inversion workgroups of each inversion stage
  for (int m = Ly; m > 1; m = (m + 1) / 2) {
    ++n_inv;
    inv_wgs.push_back(nbatch * (m / 2));
  }
  inv_wgs.push_back(nbatch);
  auto idle_ok = [&](int ord) { return 4 * inv_wgs[ord] <= 3 * ncu; };
  std::vector<std::vector<dwh::CrTask>> side_tasks(n_inv);
  std::vector<double> side_flops(n_inv, 0.0);
  int inv_ord = 0;
  auto add_inv = [&](const std::vector<int>& blocks, int& slot) {
    std::vector<dwh::CrTask>& stk = side_tasks[inv_ord];
    CrStage st{};
    st.kind = 0;
    st.first = (int)pl.inv_blk.size();
    st.n = (int)blocks.size();
    st.sg = 1.0;                        // side tasks carry their own sign (kCrNegBit)
    st.flops = side_flops[inv_ord];     // the side products' flops per batch item
    st.tfirst = (int)pl.tasks.size();
    st.ntiles = (int)stk.size();
    st.cfg = {32, 1};
    for (const dwh::CrTask& t : stk) st.maxt32 = std::max(st.maxt32, dwh::cr_task_tiles(t, 32));
    pl.tasks.insert(pl.tasks.end(), stk.begin(), stk.end());
    ++inv_ord;
    std::vector<int> dst;
    // level-0 blocks (the first inversion stage): from their static R blocks
    if (inv0 && std::all_of(blocks.begin(), blocks.end(), [&](int b) { return b < 3 * Ly; })) {
      st.l0 = 1;
      for (size_t i = 0; i < blocks.size(); ++i) pl.inv0_r.push_back(nb());
    }
    for (int b : blocks) {
      const int d = b < 3 * Ly ? nb() : b;
      pl.inv_blk.push_back(b);
      pl.inv_dst.push_back(d);
      pl.inv_slot.push_back(slot++);
      dst.push_back(d);
    }
    pl.stages.push_back(st);
    return dst;
  };
  struct Term { int a, b; };
  std::vector<dwh::CrTask> cur_tasks;
  // output window of the next tasks (full block unless restricted)
  int w_r0 = 0, w_r1 = HP, w_c0 = 0, w_c1 = BP;
  // The level-0 G blocks are read only by the gathers: the force reads the
  // pairing (B-part) entries (p_i, HP + p_j) of every bond, E_f and Tr rho_hh
  // the diagonal (p, p) of G_D.  need[k][y]: the 16 x 16 top-half tiles
  // (tr * (BP / 16) + tc) of G_D[y] (k = 0), G_U[y] = G[y, y+1] (1),
  // G_L[y] = G[y+1, y] (2) that hold such entries — the block the gathers
  // below resolve each bond to.  The last backward level computes only those
  // tiles of its G_ea (= G_L), G_ec (= G_U) and G_ee (= G_D).  One lattice
  // row per block: the diagonal B tiles of G_U / G_L (vertical bonds at
  // (x, HP + x)); two rows: the off-diagonal ones.
  const int ntc = BP / 16;
  std::vector<std::vector<std::set<int>>> need(3, std::vector<std::set<int>>(Ly));
  {
    const int Ns = Lx * Ly;
    for (int i = 0; i < Ns; ++i) {
      const int pi = i % Lx, y = i / Lx;
      need[0][y].insert((pi / 16) * ntc + pi / 16);
      for (int s = 0; s < kSlots; ++s) {
        const int j = Dcol[(size_t)i * kSlots + s];
        if (j < 0) continue;
        const int pj = j % Lx, yj = j / Lx;
        const int tile = (pi / 16) * ntc + (HP + pj) / 16;
        if (Ly == 1 || yj == y) need[0][y].insert(tile);
        else if (yj == (y + 1) % Ly) need[1][y].insert(tile);
        else need[2][(y - 1 + Ly) % Ly].insert(tile);
      }
    }
  }
  // per task of cur_tasks: the tiles to compute (nullptr: every tile of the window)
  std::vector<const std::set<int>*> cur_keep;
  const std::set<int>* keep_next = nullptr;
  auto task = [&](int out, int cin, std::initializer_list<Term> terms) {
    cur_keep.push_back(keep_next);
    dwh::CrTask t{};
    t.out = out;
    t.cin = cin;
    t.r0 = w_r0;
    t.r1 = w_r1;
    t.c0 = w_c0;
    t.c1 = w_c1;
    t.nt = 0;
    t.bq = 0;
    for (const Term& x : terms) {
      t.a[t.nt] = x.a;
      t.b[t.nt] = x.b;
      if (qform[x.b]) t.bq |= 1 << t.nt;
      t.nt++;
    }
    cur_tasks.push_back(t);
  };
  // to_side: the tasks become side work of inversion stage `ord` (tiles
  // with their own sign) instead of a product stage
  auto flush = [&](double sg, bool to_side = false, int ord = 0) {
    if (cur_tasks.empty()) return;
    if (to_side) {
      for (dwh::CrTask t : cur_tasks) {
        if (sg < 0) t.bq |= dwh::kCrNegBit;
        side_tasks[ord].push_back(t);
        side_flops[ord] += 8.0 * t.nt * BP * (double)(t.r1 - t.r0) * (t.c1 - t.c0);
      }
      cur_tasks.clear();
      cur_keep.clear();
      return;
    }
    CrStage st{};
    st.kind = 1;
    st.first = (int)pl.tasks.size();
    st.n = (int)cur_tasks.size();
    st.sg = sg;
    st.flops = 0.0;                     // accumulated per task below
    st.tfirst = (int)pl.tiles16.size();
    st.ntiles = 0;
    st.cfg = {16, 1};
    for (size_t ti = 0; ti < cur_tasks.size(); ++ti) {
      const dwh::CrTask& t = cur_tasks[ti];
      const int nk = dwh::cr_task_tiles(t, 16);
      const int kept = cr_task_tiles16(t, ntc, cur_keep[ti], &pl.tiles16);
      st.flops += 8.0 * t.nt * BP * (double)(t.r1 - t.r0) * (t.c1 - t.c0) * kept / nk;
      st.maxt32 = std::max(st.maxt32, dwh::cr_task_tiles(t, 32));
      st.maxt16 = std::max(st.maxt16, dwh::cr_task_tiles(t, 16));
      st.ntmax = std::max(st.ntmax, t.nt);
      pl.tasks.push_back(t);
    }
    st.ntiles = (int)pl.tiles16.size() - st.tfirst;
    pl.stages.push_back(st);
    cur_tasks.clear();
    cur_keep.clear();
  };

  Level cur;
  cur.m = Ly;
  for (int y = 0; y < Ly; ++y) {
    cur.D.push_back(y);
    cur.U.push_back(Ly + y);
    cur.L.push_back(2 * Ly + y);
  }
  std::vector<Level> levels;
  int slot = 0;
  while (cur.m > 1) {
    const int m = cur.m;
    // inv_ord: this level's inversion stage (added below)
    const bool side_ul = side && m >= side_m && idle_ok(inv_ord + 1);
    // with the backward merge the final inversion hosts the merge products,
    // which read W: the W products go at most to the stage before it
    const int w_ord = std::min(n_inv - (merge ? 2 : 1), inv_ord + side_woff);
    const bool side_w = side && m >= side_m && w_ord > inv_ord && idle_ok(w_ord);
    cur.elim.assign(m, 0);
    cur.E.clear();
    cur.K.clear();
    for (int e = 1; e < m - (m % 2); e += 2) {
      cur.E.push_back(e);
      cur.elim[e] = 1;
    }
    for (int k = 0; k < m; k += 2) cur.K.push_back(k);
    cur.V1.assign(m, -1);
    cur.V2.assign(m, -1);
    cur.W1.assign(m, -1);
    cur.W2.assign(m, -1);
    std::vector<int> inv;
    for (int e : cur.E) inv.push_back(cur.D[e]);
    const std::vector<int> dinv = add_inv(inv, slot);
    cur.Dinv.assign(m, -1);
    for (size_t i = 0; i < cur.E.size(); ++i) cur.Dinv[cur.E[i]] = dinv[i];
    if (sparse0 && levels.empty() && m % 2 == 0 && m >= 4) {
      // level 0: D', U', L' of every kept row in one sparse stage (no V / W)
      CrStage st{};
      st.kind = 2;
      st.sp = 0;
      st.first = (int)pl.sp_fwd.size();
      Level nxt;
      nxt.m = (int)cur.K.size();
      for (int k : cur.K) {
        const int er = k + 1, el = (k - 1 + m) % m;
        const int Dn = nb(), Un = nb(), Ln = nb();
        pl.sp_fwd.push_back(dwh::CrSpFwd{cur.D[k], cur.U[k], cur.L[k], cur.U[el], cur.L[el], cur.U[er], cur.L[er],
                                         cur.Dinv[er], cur.Dinv[el], Dn, Un, Ln});
        for (int r = 0; r < HP; ++r)   // V1r, V2r, V2l rows
          st.flops += 8.0 * BP * (nr(cur.U[k], r) + nr(cur.L[er], r) + nr(cur.L[el], r));
        for (int c = 0; c < BP; ++c)   // D' (2 terms), U', L'
          st.flops += 8.0 * HP * (2 * nc(cur.L[k], c) + nc(cur.U[el], c) + nc(cur.U[er], c));
        nxt.D.push_back(Dn);
        nxt.U.push_back(Un);
        nxt.L.push_back(Ln);
      }
      st.n = (int)pl.sp_fwd.size() - st.first;
      pl.stages.push_back(st);
      cur.sparse = true;
      levels.push_back(cur);
      cur = nxt;
      continue;
    }
    for (int e : cur.E) {
      const int a = e - 1;
      cur.V1[e] = nbq();
      task(cur.V1[e], -1, {{cur.U[a], cur.Dinv[e]}});
      cur.V2[e] = nbq();
      task(cur.V2[e], -1, {{cur.L[e], cur.Dinv[e]}});
    }
    if (side_w) flush(-1.0);
    for (int e : cur.E) {
      const int a = e - 1;
      cur.W1[e] = nbq();
      task(cur.W1[e], -1, {{cur.Dinv[e], cur.L[a]}});
      cur.W2[e] = nbq();
      task(cur.W2[e], -1, {{cur.Dinv[e], cur.U[e]}});
    }
    // W_l: first needed by the backward pass; placed three inversion stages
    // later (the coarse inversions leave ~240 of 256 CUs idle), the U'/L'
    // products of this level take the next one
    flush(-1.0, side_w, w_ord);
    Level nxt;
    nxt.m = (int)cur.K.size();
    std::vector<dwh::CrTask> ul_tasks;   // U'/L' (side work when `side`)
    for (int k : cur.K) {
      if (m == 2) {
        const int e = 1, Dn = nb();
        task(Dn, cur.D[0], {{cur.V1[e], cur.L[0]}, {cur.V2[e], cur.U[1]}, {cur.V1[e], cur.U[1]},
                            {cur.V2[e], cur.L[0]}});
        nxt.D.push_back(Dn);
        nxt.U.push_back(-1);
        nxt.L.push_back(-1);
        continue;
      }
      const int er = k + 1, el = (k - 1 + m) % m;
      const bool hr = er < m && cur.elim[er], hl = cur.elim[el];
      const int Dn = nb();
      if (hr && hl)
        task(Dn, cur.D[k], {{cur.V1[er], cur.L[k]}, {cur.V2[el], cur.U[el]}});
      else if (hr)
        task(Dn, cur.D[k], {{cur.V1[er], cur.L[k]}});
      else
        task(Dn, cur.D[k], {{cur.V2[el], cur.U[el]}});
      nxt.D.push_back(Dn);
      if (hr) {
        const int Un = nb(), Ln = nb();
        task(Un, -1, {{cur.V1[er], cur.U[er]}});
        task(Ln, -1, {{cur.V2[er], cur.L[k]}});
        if (side_ul) {   // move them behind the D' tasks of this stage
          ul_tasks.push_back(cur_tasks[cur_tasks.size() - 2]);
          ul_tasks.push_back(cur_tasks.back());
          cur_tasks.resize(cur_tasks.size() - 2);
          cur_keep.resize(cur_keep.size() - 2);
        }
        nxt.U.push_back(Un);
        nxt.L.push_back(Ln);
      } else {   // odd m: the kept pair (m-1, 0) keeps its direct coupling
        nxt.U.push_back(cur.U[k]);
        nxt.L.push_back(cur.L[k]);
      }
    }
    // the top level (its only kept block is the final one): plan the
    // backward merges now that every forward block exists; their products go
    // into this D' stage (no side work) or the final inversion (side work)
    std::vector<dwh::CrTask> merge_tasks;
    if (merge && nxt.m == 1) {
      std::vector<Level*> all;
      for (Level& lv : levels) all.push_back(&lv);
      all.push_back(&cur);
      // budget: side work of two workgroup rounds (4 wave tiles each) on the
      // CUs the final inversion leaves idle (a side workgroup takes ~6 us of
      // the inversion's ~16), or 16 x 16 tiles added to this (latency-bound)
      // D' stage
      const int64_t t32 = (int64_t)((HP + 31) / 32) * ((BP + 31) / 32), t16 = (int64_t)(HP / 16) * (BP / 16);
      int64_t side_t = 0;
      for (const dwh::CrTask& t : side_tasks[n_inv - 1]) side_t += dwh::cr_task_tiles(t, 32);
      const int64_t budget = side ? 8 * ((int64_t)ncu - nbatch) - side_t * nbatch : 1024;
      int64_t used = 0;
      for (int li = (int)all.size() - 2; li >= 1; --li) {
        Level& f = *all[li];
        const Level& u = *all[li + 1];
        if (f.sparse || f.m > merge_max_m) break;
        int nx = 0;
        for (int e : f.E) {
          const int a = e - 1, c = (e + 1) % f.m;
          nx += u.elim[a / 2] + u.elim[(c / 2) % u.m];
        }
        const int64_t cost = 6 * (int64_t)nx * nbatch * (side ? t32 : t16);
        if (used + cost > budget) break;
        used += cost;
        f.merged = true;
        f.xa.assign(f.m, {-1, -1, -1, -1, -1, -1});
        f.xc.assign(f.m, {-1, -1, -1, -1, -1, -1});
        for (int e : f.E) {
          const int a = e - 1, c = (e + 1) % f.m;
          // p: u's eliminated position next to e; V, W: the f products that meet G_ee(u)[p]
          auto expand = [&](int pu, int V, int W) {
            std::array<int, 6> x;
            x[0] = nb();    // Dinv V  (M Q -> M)
            x[1] = nbq();   // V1 V    (Q Q -> Q)
            x[2] = nbq();   // V2 V
            x[3] = nb();    // W Dinv  (Q M -> M)
            x[4] = nbq();   // W W1
            x[5] = nbq();   // W W2
            const int src[6][2] = {{u.Dinv[pu], V}, {u.V1[pu], V}, {u.V2[pu], V},
                                   {W, u.Dinv[pu]}, {W, u.W1[pu]}, {W, u.W2[pu]}};
            for (int k = 0; k < 6; ++k) {
              dwh::CrTask t{};
              t.out = x[k];
              t.cin = -1;
              t.r0 = 0;
              t.r1 = HP;
              t.c0 = 0;
              t.c1 = BP;
              t.nt = 1;
              t.a[0] = src[k][0];
              t.b[0] = src[k][1];
              t.bq = qform[src[k][1]] ? 1 : 0;
              merge_tasks.push_back(t);
            }
            return x;
          };
          if (u.elim[a / 2]) f.xa[e] = expand(a / 2, f.V1[e], f.W1[e]);
          if (u.elim[(c / 2) % u.m]) f.xc[e] = expand((c / 2) % u.m, f.V2[e], f.W2[e]);
        }
      }
      if (!side)
        for (const dwh::CrTask& t : merge_tasks) {
          cur_tasks.push_back(t);
          cur_keep.push_back(nullptr);
        }
    }
    flush(1.0);
    if (!ul_tasks.empty()) {
      cur_tasks = ul_tasks;
      cur_keep.assign(ul_tasks.size(), nullptr);
      flush(1.0, true, inv_ord);
    }
    if (side && !merge_tasks.empty()) {
      cur_tasks = merge_tasks;
      cur_keep.assign(merge_tasks.size(), nullptr);
      flush(1.0, true, n_inv - 1);
    }
    levels.push_back(cur);
    cur = nxt;
  }
  const int Dfin = add_inv({cur.D[0]}, slot)[0];
  std::vector<int> GD{Dfin}, GU{Dfin}, GL{Dfin};
  // the G_ee tasks of the level above when they run in this level's first stage
  struct GeeTask { int out, cin, a0, b0, a1, b1; };
  std::vector<GeeTask> pend;
  auto emit_pend = [&] {
    for (const GeeTask& t : pend) task(t.out, t.cin, {{t.a0, t.b0}, {t.a1, t.b1}});
    pend.clear();
  };
  for (int li = (int)levels.size() - 1; li >= 0; --li) {
    Level& lv = levels[li];
    // a pending G_ee stage whose finer level does not merge runs on its own
    if (!pend.empty() && !lv.merged) {
      emit_pend();
      flush(1.0);
    }
    const int m = lv.m, mn = (int)lv.K.size();
    std::vector<int> gd(m, -1), gu(m, -1), gl(m, -1);
    for (int kk = 0; kk < mn; ++kk) {
      const int k = lv.K[kk];
      gd[k] = GD[kk];
      if (!(k + 1 < m && lv.elim[k + 1])) {
        gu[k] = GU[kk];
        gl[k] = GL[kk];
      }
    }
    // Level 0 is the last backward level: G_ea, G_ec (cross-block bonds, not
    // operands of anything after them) are formed only on the B-part tiles
    // the vertical pairing bonds read (need); G_ae, G_ce (right operands of
    // G_ee in the dense level 0) need their whole top half there, and only
    // their need tiles in the sparse level 0 (G_ee from T = -Dinv M); G_ee
    // (in-block bonds, hole diagonal) its need tiles.
    const bool sel = (li == 0);
    const int H0 = sel ? HP : 0, H1 = sel ? HP + Lx : BP;
    if (lv.sparse) {
      // sparse level 0: Z_a, Z_c, Y_a, Y_c, M in one sparse stage, then
      // one-term products G_ae = -Z_a Dinv, G_ce = -Z_c Dinv, G_ea = -Dinv Y_a,
      // G_ec = -Dinv Y_c (need tiles), T = -Dinv M; then G_ee = Dinv - T Dinv
      CrStage st{};
      st.kind = 2;
      st.sp = 1;
      st.first = (int)pl.sp_bwd.size();
      struct Bw { int e, a, za, zc, ya, yc, mx; };
      std::vector<Bw> bw;
      for (int e : lv.E) {
        const int a = e - 1, c = (e + 1) % m;
        const int ia = a / 2, ic = (c / 2) % mn;
        const int Gaa = GD[ia], Gcc = GD[ic], Gac = GU[ia], Gca = GL[ia];
        const Bw x{e, a, nbq(), nbq(), nbq(), nbq(), nb()};
        bw.push_back(x);
        pl.sp_bwd.push_back(dwh::CrSpBwd{Gaa, Gac, Gca, Gcc, lv.U[a], lv.L[e], lv.L[a], lv.U[e], x.za, x.zc, x.ya,
                                         x.yc, x.mx, 0, 0, 0});
        for (int cc = 0; cc < BP; ++cc) st.flops += 8.0 * HP * 2 * (nc(lv.U[a], cc) + nc(lv.L[e], cc));   // Z_a, Z_c
        for (int r = 0; r < HP; ++r) st.flops += 8.0 * BP * 3 * (nr(lv.L[a], r) + nr(lv.U[e], r));       // Y_a, Y_c, M
      }
      st.n = (int)pl.sp_bwd.size() - st.first;
      pl.stages.push_back(st);
      std::vector<int> tn(m, -1);
      for (const Bw& x : bw) {
        const int e = x.e, a = x.a, D = lv.Dinv[e];
        const int gea = nb(), gec = nb(), gae = nb(), gce = nb();
        tn[e] = nbq();
        w_c0 = H0;
        w_c1 = H1;
        keep_next = &need[2][a];   // G_ea = G_L[a]
        task(gea, -1, {{D, x.ya}});
        keep_next = &need[1][e];   // G_ec = G_U[e]
        task(gec, -1, {{D, x.yc}});
        // G_ae = G_U[a] and G_ce = G_L[e] are read only by the gathers here
        // (G_ee comes from T, not from them): their need tiles only
        keep_next = &need[1][a];
        task(gae, -1, {{x.za, D}});
        keep_next = &need[2][e];
        task(gce, -1, {{x.zc, D}});
        keep_next = nullptr;
        w_c0 = 0;
        w_c1 = BP;
        task(tn[e], -1, {{D, x.mx}});
        gu[a] = gae;
        gl[a] = gea;
        gu[e] = gec;
        gl[e] = gce;
      }
      flush(-1.0);
      for (int e : lv.E) {
        const int gee = nb();
        keep_next = &need[0][e];
        task(gee, lv.Dinv[e], {{tn[e], lv.Dinv[e]}});
        gd[e] = gee;
      }
      keep_next = nullptr;
      flush(-1.0);
      GD = gd;
      GU = gu;
      GL = gl;
      continue;
    }
    // merged: this stage also runs the level above's G_ee (pend), and reads
    // G_ee(u) = Dinv + W1 G_ae + W2 G_ce = Dinv + G_ea V1 + G_ec V2 (u's
    // blocks at that position) through its expansion (xa / xc, formed in the
    // forward pass)
    const Level* up = lv.merged ? &levels[li + 1] : nullptr;
    emit_pend();
    lv.Gea.assign(m, -1);
    lv.Gec.assign(m, -1);
    lv.Gae.assign(m, -1);
    lv.Gce.assign(m, -1);
    for (int e : lv.E) {
      const int a = e - 1, c = (e + 1) % m;
      const int ia = a / 2, ic = (c / 2) % mn;
      const int Gaa = GD[ia], Gcc = GD[ic];
      const int Gac = mn == 1 ? GD[0] : GU[ia];
      const int Gca = mn == 1 ? GD[0] : GL[ia];
      const int gea = nb(), gec = nb(), gae = nb(), gce = nb();
      const bool xa = up && lv.xa[e][0] >= 0, xc = up && lv.xc[e][0] >= 0;
      w_c0 = H0;
      w_c1 = H1;
      keep_next = sel ? &need[2][a] : nullptr;   // G_ea = G[a + 1, a] = G_L[a]
      if (xa) {   // W1 G_aa = (W1 Dinv) + (W1 W1u) G_ae,u + (W1 W2u) G_ce,u
        const std::array<int, 6>& x = lv.xa[e];
        task(gea, x[3], {{x[4], up->Gae[ia]}, {x[5], up->Gce[ia]}, {lv.W2[e], Gca}});
      } else {
        task(gea, -1, {{lv.W1[e], Gaa}, {lv.W2[e], Gca}});
      }
      keep_next = sel ? &need[1][e] : nullptr;   // G_ec = G[e, e + 1] = G_U[e]
      if (xc) {   // W2 G_cc
        const std::array<int, 6>& x = lv.xc[e];
        task(gec, x[3], {{lv.W1[e], Gac}, {x[4], up->Gae[ic]}, {x[5], up->Gce[ic]}});
      } else {
        task(gec, -1, {{lv.W1[e], Gac}, {lv.W2[e], Gcc}});
      }
      keep_next = nullptr;
      w_c0 = 0;
      w_c1 = BP;
      if (xa) {   // G_aa V1 = (Dinv V1) + G_ea,u (V1u V1) + G_ec,u (V2u V1)
        const std::array<int, 6>& x = lv.xa[e];
        task(gae, x[0], {{up->Gea[ia], x[1]}, {up->Gec[ia], x[2]}, {Gac, lv.V2[e]}});
      } else {
        task(gae, -1, {{Gaa, lv.V1[e]}, {Gac, lv.V2[e]}});
      }
      if (xc) {   // G_cc V2
        const std::array<int, 6>& x = lv.xc[e];
        task(gce, x[0], {{Gca, lv.V1[e]}, {up->Gea[ic], x[1]}, {up->Gec[ic], x[2]}});
      } else {
        task(gce, -1, {{Gca, lv.V1[e]}, {Gcc, lv.V2[e]}});
      }
      gu[a] = gae;
      gl[a] = gea;
      gu[e] = gec;
      gl[e] = gce;
      lv.Gea[e] = gea;
      lv.Gec[e] = gec;
      lv.Gae[e] = gae;
      lv.Gce[e] = gce;
    }
    flush(1.0);
    // G_ee = Dinv + W1 G_ae + W2 G_ce, in place; deferred into the next finer
    // level's first stage when that one merges
    const bool defer = li >= 1 && levels[li - 1].merged;
    for (int e : lv.E) {
      if (defer) {
        pend.push_back(GeeTask{lv.Dinv[e], lv.Dinv[e], lv.W1[e], lv.Gae[e], lv.W2[e], lv.Gce[e]});
      } else {
        keep_next = sel ? &need[0][e] : nullptr;
        task(lv.Dinv[e], lv.Dinv[e], {{lv.W1[e], lv.Gae[e]}, {lv.W2[e], lv.Gce[e]}});
      }
      gd[e] = lv.Dinv[e];
    }
    keep_next = nullptr;
    if (!defer) flush(1.0);
    GD = gd;
    GU = gu;
    GL = gl;
  }
  // gather offsets of the level-0 G blocks
  const int N = Lx * Ly;
  const int64_t BB = (int64_t)HP * BP;
  pl.goff.assign((size_t)N * kSlots, -1);
  pl.doff.assign(N, 0);
  for (int i = 0; i < N; ++i) {
    const int x = i % Lx, y = i / Lx;
    for (int s = 0; s < kSlots; ++s) {
      const int j = Dcol[(size_t)i * kSlots + s];
      if (j < 0) continue;
      const int xj = j % Lx, yj = j / Lx;
      int blk;
      if (Ly == 1 || yj == y) blk = GD[y];
      else if (yj == (y + 1) % Ly) blk = GU[y];
      else blk = GL[(y - 1 + Ly) % Ly];
      pl.goff[(size_t)i * kSlots + s] = blk * BB + (int64_t)x * BP + (HP + xj);
    }
    pl.doff[i] = GD[y] * BB + (int64_t)x * BP + x;   // G22[x, x] = -conj(A[x, x])
  }
  // level-0 fill lists and pairing scatter offsets: CR never overwrites a
  // level-0 block (their inverses are formed out of place), so per step only
  // the pairing entries are scattered
  std::vector<char> rewrite(3 * Ly, 0);
  for (int b = 0; b < 3 * Ly; ++b) {
    pl.fill_all.push_back(b);
    if (rewrite[b]) pl.fill_step.push_back(b);
  }
  pl.off_ph.assign((size_t)N * kSlots, -1);
  auto blk_of = [&](int yr, int yc) {
    if (yc == yr) return yr;                              // D[yr]
    if (Ly >= 2 && yc == (yr + 1) % Ly) return Ly + yr;   // U[yr]
    return 2 * Ly + yc;                                   // L[yc] = A[yc+1, yc]
  };
  for (int i = 0; i < N; ++i)
    for (int s = 0; s < kSlots; ++s) {
      const int j = Dcol[(size_t)i * kSlots + s];
      if (j < 0) continue;
      const int yi = i / Lx, xi = i % Lx, yj = j / Lx, xj = j % Lx;
      const int b = blk_of(yi, yj);
      if (rewrite[b]) continue;
      pl.off_ph[(size_t)i * kSlots + s] = b * BB + (int64_t)xi * BP + (HP + xj);
      pl.n_ph++;
    }
  pl.nblk = nblk;
  return pl;
}

// Stage configuration (tile TS, K split).  16 x 16 tiles; the K split by the
// stage's size (ntiles16 16 x 16 output tiles per batch item x nbatch): a
// 4-way split (short serial MFMA chains on many waves) for the stages of a
// single L = 32 chain, whose stages are short and latency bound
// (profiles/r01_cr_gemm_config_sweep.txt: fastest on every stage there), no
// split once a stage has enough tiles to fill the chip by itself (batched
// chains, L = 48: no LDS reduction, one tile per wave;
// profiles/r03_exp_gemm_ksplit_by_size.txt: from 2048 tiles, C3 -0.9 %,
// C5 -5 %, 4 chains at L = 32 -3 %; C2's stages stay below it).
// DWHMC_CR_GEMM=TS:KSPLIT forces one
// configuration for every stage (A/B runs; tests/test_gpu_parity.py runs
// every compiled variant).
CrGemmCfg cr_gemm_config(const CrDims& c, int ntiles16) {
  // read at every context creation (tests switch it between contexts)
  const CrGemmCfg forced = [] {
    CrGemmCfg f{0, 1};
    if (const char* e = std::getenv("DWHMC_CR_GEMM")) {
      f.ts = std::atoi(e);
      if (const char* p = std::strchr(e, ':')) f.ksplit = std::atoi(p + 1);
    }
    if (f.ksplit != 1 && f.ksplit != 2 && f.ksplit != 4) f.ksplit = 1;
    if (f.ts == 32 && f.ksplit == 4) f.ksplit = 2;
    return f;
  }();
  const bool ts32_ok = (c.BP / 2) % 32 == 0;   // 32-wide tiles must not straddle A | B
  if (forced.ts == 16 || (forced.ts == 32 && ts32_ok)) return forced;
  const int64_t T = (int64_t)ntiles16 * c.nbatch;
  return CrGemmCfg{16, T >= 2048 ? 1 : 4};
}

namespace {
// host twin of xcd_remap (dwhmc_device.h)
int xcd_remap_host(int orig, int total) {
  const int q = total / 8, r = total % 8, xcd = orig % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}
}  // namespace

int cr_gemm_slot_wgs(const CrDims& c, int ntl16, const CrGemmCfg& cfg) {
  const int tpw = 4 / cfg.ksplit;
  return (c.nbatch * ntl16 + tpw - 1) / tpw;
}

// Slot b * TPW + j of the launch = tile (xcd_remap(b, nwg) * TPW + j) of the
// stage's nbatch x ntl16 tiles (batch item major): the order the round-5
// kernel derived on the device, so the work distribution over XCDs is kept.
void cr_gemm_slots(const CrDims& c, const CrTile* tl16, int ntl16, const CrGemmCfg& cfg, CrSlot* out) {
  const int tpw = 4 / cfg.ksplit, nwg = cr_gemm_slot_wgs(c, ntl16, cfg), HP = c.BP / 2;
  const int64_t total = (int64_t)c.nbatch * ntl16, BB = (int64_t)HP * c.BP;
  for (int b = 0; b < nwg; ++b)
    for (int j = 0; j < tpw; ++j) {
      CrSlot& sl = out[(size_t)b * tpw + j];
      sl = CrSlot{};
      const int64_t gt = (int64_t)xcd_remap_host(b, nwg) * tpw + j;
      if (gt >= total) {   // padding of the last workgroup
        sl.out = kCrNone;
        sl.cin = kCrNone;
        continue;
      }
      const int bi = (int)(gt / ntl16);
      const CrTile& t = tl16[gt - (int64_t)bi * ntl16];
      const int r0 = 16 * t.tr, c0 = 16 * t.tc;
      sl.base = (uint64_t)bi * (uint64_t)c.item;
      sl.out = (uint32_t)(t.out * BB + (int64_t)r0 * c.BP + c0);
      sl.cin = t.cin >= 0 ? (uint32_t)(t.cin * BB + (int64_t)r0 * c.BP + c0) : kCrNone;
      sl.nt = t.nt;
      for (int h = 0; h < t.nt; ++h) {
        sl.a[h] = (uint32_t)(t.a[h] * BB + (int64_t)r0 * c.BP);
        sl.b[h] = (uint32_t)(t.b[h] * BB + c0);
        const bool q = (t.bq >> h) & 1;
        if ((c0 < HP) == q) sl.smask |= 1u << h;   // synthesised rows: sgn < 0
      }
      sl.rot = (c0 < HP ? c0 + HP : c0 - HP) - c0;
    }
}

std::vector<CrStageStores> cr_stage_stores(const CrPlan& pl, int BP) {
  const int ns = (int)pl.stages.size();
  const int64_t BB = (int64_t)(BP / 2) * BP, blk_bytes = BB * (int64_t)sizeof(double2);
  // per stage: the blocks it reads; its own outputs and its side products with their bytes
  typedef std::vector<std::pair<int, int64_t>> Writes;
  std::vector<std::vector<int>> rd(ns + 1);
  std::vector<Writes> wr(ns), wrs(ns);
  auto task_reads = [](const dwh::CrTask& t, std::vector<int>& r) {
    for (int h = 0; h < t.nt; ++h) {
      r.push_back(t.a[h]);
      r.push_back(t.b[h]);
    }
    if (t.cin >= 0) r.push_back(t.cin);
  };
  for (int si = 0; si < ns; ++si) {
    const CrStage& st = pl.stages[si];
    if (st.kind == 0) {
      for (int k = 0; k < st.n; ++k) {
        rd[si].push_back(pl.inv_blk[st.first + k]);
        wr[si].push_back({pl.inv_dst[st.first + k], blk_bytes});
      }
      if (st.l0) rd[si].insert(rd[si].end(), pl.inv0_r.begin(), pl.inv0_r.end());
      for (int k = 0; k < st.ntiles; ++k) {
        task_reads(pl.tasks[st.tfirst + k], rd[si]);
        wrs[si].push_back({pl.tasks[st.tfirst + k].out, blk_bytes});
      }
    } else if (st.kind == 2) {
      for (int k = 0; k < st.n; ++k) {
        if (st.sp == 0) {
          const dwh::CrSpFwd& t = pl.sp_fwd[st.first + k];
          for (int b : {t.dk, t.uk, t.lk, t.uel, t.lel, t.uer, t.ler, t.dir, t.dil}) rd[si].push_back(b);
          for (int b : {t.od, t.ou, t.ol}) wr[si].push_back({b, blk_bytes});
        } else {
          const dwh::CrSpBwd& t = pl.sp_bwd[st.first + k];
          for (int b : {t.gaa, t.gac, t.gca, t.gcc, t.ua, t.le, t.la, t.ue}) rd[si].push_back(b);
          for (int b : {t.oza, t.ozc, t.oya, t.oyc, t.omx}) wr[si].push_back({b, blk_bytes});
        }
      }
    } else {
      for (int k = 0; k < st.n; ++k) task_reads(pl.tasks[st.first + k], rd[si]);
      for (int k = 0; k < st.ntiles; ++k)
        wr[si].push_back({pl.tiles16[st.tfirst + k].out, 256 * (int64_t)sizeof(double2)});
    }
  }
  // the force gather is the launch after the last stage
  for (int64_t o : pl.goff)
    if (o >= 0) rd[ns].push_back((int)(o / BB));
  for (auto& r : rd) {
    std::sort(r.begin(), r.end());
    r.erase(std::unique(r.begin(), r.end()), r.end());
  }
  std::vector<CrStageStores> out(ns);
  for (int si = 0; si < ns; ++si) {
    auto tally = [&](const Writes& w, int64_t* bytes, int64_t* next, int* first) {
      for (const auto& bw : w) {
        int d = kCrNeverRead;
        for (int sj = si + 1; sj <= ns && d == kCrNeverRead; ++sj)
          if (std::binary_search(rd[sj].begin(), rd[sj].end(), bw.first)) d = sj - si;
        *bytes += bw.second;
        if (d == 1) *next += bw.second;
        *first = std::min(*first, d);
      }
    };
    tally(wr[si], &out[si].bytes, &out[si].bytes_next, &out[si].first_read);
    tally(wrs[si], &out[si].bytes_side, &out[si].bytes_side_next, &out[si].first_read_side);
  }
  return out;
}

namespace {
// Store policy of every launch (CrStage::store / store_side,
// CrPlan::store_force), by family as measured at C3 / C2 / C5 (DESIGN.md §4
// "Store policy", profiles/r07_store_policy_ab.txt): write-through for the
// product stages with a K split — the short launches of the coarse levels,
// whose epilogue already stores 8-byte pieces, so the two sc1 stores cost no
// instruction, and whose dirty lines no longer wait for the release that ends
// the launch — and for the side products of the inversion launches (issued
// beside the 16 us inversions, mostly read two or more launches later);
// plain for everything else: the bandwidth-bound sparse stages and the
// products without a K split lose to the 8-byte stores, the inversions and
// the force scatter do not move, and non-temporal stores won nowhere.
// DWHMC_CR_STORE=0: plain everywhere (A/B runs, tests); read at every context
// creation.
void cr_store_policies(CrPlan& pl) {
  const char* e = std::getenv("DWHMC_CR_STORE");
  const bool on = !(e && *e == '0');
  for (CrStage& st : pl.stages) {
    st.store = st.store_side = dwh::kStorePlain;
    if (!on) continue;
    if (st.kind == 0 && st.ntiles > 0) st.store_side = dwh::kStoreThrough;
    // (the 32 x 32 tile configurations, A/B only, store plain)
    if (st.kind == 1 && st.cfg.ts == 16 && st.cfg.ksplit > 1) st.store = dwh::kStoreThrough;
  }
  pl.store_force = dwh::kStorePlain;
}
}  // namespace

void cr_plan_dump(const CrPlan& pl, int64_t nbatch, bool cfg) {
  const char* e = std::getenv("DWHMC_CR_PLAN_DUMP");
  if (!e || *e != '1') return;
  int i = 0;
  for (const CrStage& st : pl.stages) {
    if (st.kind == 0) {
      std::fprintf(stderr, "cr stage %2d: inv%s blocks=%d (x%lld wg) side_tasks=%d maxt32=%d side_flops/item=%.3g\n", i,
                   st.l0 ? "0 " : "  ", st.n, (long long)nbatch, st.ntiles, st.maxt32, st.flops);
    } else if (st.kind == 2) {
      std::fprintf(stderr, "cr stage %2d: sparse %s tasks=%d flops/item=%.3g\n", i, st.sp ? "bwd" : "fwd", st.n,
                   st.flops);
    } else {
      std::fprintf(stderr, "cr stage %2d: gemm  tasks=%d maxt32=%d maxt16=%d ntmax=%d flops/item=%.3g ntiles=%d", i,
                   st.n, st.maxt32, st.maxt16, st.ntmax, st.flops, st.ntiles);
      if (cfg) std::fprintf(stderr, " cfg=%d:%d", st.cfg.ts, st.cfg.ksplit);
      std::fprintf(stderr, "\n");
    }
    ++i;
  }
}

int plan_cr(int64_t Lx, int64_t Ly, int P, int nbatch, const std::vector<int>& Dcol, const std::vector<int>& hcol,
            int side, int inv0, int ncu, CrDims* cd, CrPlan* plan) {
  const int rows = cr_rows_per_block(Lx, Ly);
  if (!rows) return fail(nullptr, DWH_ERR_ARG, "lattice row too wide for the CR path");
  auto on = [](int arg, const char* name) {
    if (arg != kCrFromEnv) return arg != 0;
    const char* e = std::getenv(name);
    return !(e && *e == '0');
  };
  CrDims& c = *cd;
  c = CrDims{};
  c.Lx = (int)Lx * rows;   // the CR lattice: `rows` lattice rows per block
  c.Ly = (int)Ly / rows;
  c.N = (int)(Lx * Ly);
  c.BP = 2 * ((c.Lx + 15) / 16 * 16);   // top halves HP x BP, HP = c.Lx rounded to 16
  c.P = P;
  c.nbatch = nbatch;
  c.inv32 = on(kCrFromEnv, "DWHMC_CR_INV32");
  CrPlan& pl = *plan;
  pl = build_cr_plan(c.Lx, c.Ly, c.BP, Dcol, dwh::cr_supported_side(c.BP) && on(side, "DWHMC_CR_SIDE"), nbatch, ncu,
                     dwh::cr_supported_inv0(c.BP) && on(inv0, "DWHMC_CR_INV0"), &hcol);
  c.nblk = pl.nblk;
  c.item = (int64_t)c.nblk * (c.BP / 2) * c.BP;
  if ((uint64_t)c.item >= (uint64_t)dwh::kCrNone)
    return fail(nullptr, DWH_ERR_ARG, "CR pool: a batch item exceeds 2^32 elements (32-bit block-product offsets)");
  // (no lattice dwh_create takes comes near it: tests/test_cr_store_form.py)
  if ((uint64_t)c.item * sizeof(double2) >= (uint64_t)dwh::kCrNone)
    return fail(nullptr, DWH_ERR_ARG,
                "CR pool: a batch item exceeds 2^32 bytes (32-bit byte offsets: sparse rows, write-through stores)");
  pl.slots.clear();
  for (CrStage& st : pl.stages) {
    if (st.kind != 1) continue;
    st.cfg = cr_gemm_config(c, st.ntiles);
    if (st.cfg.ts != 16) continue;
    st.nswg = cr_gemm_slot_wgs(c, st.ntiles, st.cfg);
    st.sfirst = (int)pl.slots.size();
    pl.slots.resize(pl.slots.size() + (size_t)st.nswg * (4 / st.cfg.ksplit));
    cr_gemm_slots(c, pl.tiles16.data() + st.tfirst, st.ntiles, st.cfg, pl.slots.data() + st.sfirst);
  }
  cr_store_policies(pl);
  return DWH_OK;
}

namespace {
// What dwh_create plans for a periodic Lx x Ly lattice with the reference's
// tables (src/Types.jl:60-80) and NN pairing bonds, nbatch batch items
int plan_periodic(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, CrDims* c, CrPlan* pl) {
  if (Lx < 1 || Ly < 1 || nbatch < 1) return fail(nullptr, DWH_ERR_ARG, "bad lattice / batch");
  if (Lx > 9216 || Ly > 9216 || Lx * Ly > 9216) return fail(nullptr, DWH_ERR_ARG, "lattice larger than dwh_create takes");
  const int N = (int)(Lx * Ly);
  std::vector<int64_t> nn((size_t)4 * N), nnn((size_t)4 * N);
  auto idx = [&](int x, int y) { return (int64_t)(((y % Ly + Ly) % Ly) * Lx + ((x % Lx + Lx) % Lx)) + 1; };
  for (int y = 0; y < Ly; ++y)
    for (int x = 0; x < Lx; ++x) {
      const int i = y * Lx + x;
      nn[0 * N + i] = idx(x + 1, y);
      nn[1 * N + i] = idx(x, y + 1);
      nn[2 * N + i] = idx(x - 1, y);
      nn[3 * N + i] = idx(x, y - 1);
      nnn[0 * N + i] = idx(x + 1, y + 1);
      nnn[1 * N + i] = idx(x - 1, y + 1);
      nnn[2 * N + i] = idx(x - 1, y - 1);
      nnn[3 * N + i] = idx(x + 1, y - 1);
    }
  const std::vector<double> clean((size_t)N, 0.0);
  HostModel m;
  if (int rc = build_host_model(Lx, Ly, 1.0, -0.35, 0.0, nn.data(), nnn.data(), 1, clean.data(), &m, false)) return rc;
  return plan_cr(Lx, Ly, 1, (int)nbatch, m.Dcol, m.hcol, side != 0, inv0 != 0, 256, c, pl);
}
}  // namespace

}  // namespace dwh

using namespace dwh;

extern "C" {

// ---- host-only check of the CR schedule (no device) -------------------------
// Builds the plan dwh_create would for an Lx x Ly periodic lattice (NN pairing
// bonds) and nbatch = chains x poles batch items, then checks its dataflow:
// every block a stage reads is a level-0 / static block or was written by an
// EARLIER stage (launches are stream ordered, workgroups of one launch are
// not), no block is read and written in one stage except a task's own
// accumulate input, no two tasks of a stage write the same block, and every
// block the force / E_f gather reads was written.
int dwh_debug_cr_plan_check(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, int64_t* stats) {
  CrDims c;
  CrPlan pl;
  if (int rc = plan_periodic(Lx, Ly, nbatch, side, inv0, &c, &pl)) return rc;
  const int Lyc = c.Ly, BP = c.BP;
  cr_plan_dump(pl, nbatch, false);
  std::vector<int> written(pl.nblk, -1);   // stage of the first write; -2: ready from the start
  for (int b = 0; b < 3 * Lyc && b < pl.nblk; ++b) written[b] = -2;
  for (int r : pl.inv0_r) written[r] = -2;
  int64_t nside = 0, ninv = 0, ngemm = 0, ntask = 0;
  char buf[256];
  // 16 x 16 tiles written so far (block, tile row, tile column): product
  // stages write only their tile lists (restricted level-0 G blocks);
  // inversions and side-work tasks whole blocks (whole[b])
  const int ntc = BP / 16;
  std::set<std::pair<int, int>> tiles_written;   // (block, tr * ntc + tc)
  std::vector<char> whole(pl.nblk, 0);
  for (int b = 0; b < pl.nblk; ++b) whole[b] = written[b] == -2;
  for (int si = 0; si < (int)pl.stages.size(); ++si) {
    const CrStage& st = pl.stages[si];
    if (st.kind == 0) {
      for (int k = 0; k < st.n; ++k) whole[pl.inv_dst[st.first + k]] = 1;
      for (int k = 0; k < st.ntiles; ++k) whole[pl.tasks[st.tfirst + k].out] = 1;
    } else if (st.kind == 2) {
      for (int k = 0; k < st.n; ++k) {
        if (st.sp == 0) {
          const dwh::CrSpFwd& t = pl.sp_fwd[st.first + k];
          whole[t.od] = whole[t.ou] = whole[t.ol] = 1;
        } else {
          const dwh::CrSpBwd& t = pl.sp_bwd[st.first + k];
          whole[t.oza] = whole[t.ozc] = whole[t.oya] = whole[t.oyc] = whole[t.omx] = 1;
        }
      }
    } else {
      for (int k = 0; k < st.ntiles; ++k) {
        const dwh::CrTile& t = pl.tiles16[st.tfirst + k];
        tiles_written.insert({t.out, t.tr * ntc + t.tc});
      }
    }
    std::vector<std::pair<int, int>> rd;   // (block, task id or -1)
    std::vector<std::pair<int, int>> wr;
    // ids: task k -> k (its accumulate input may be its output), its
    // operands -> k + 2^20 (never its output); inversion entry k -> -1 - k
    // (in place: reads and writes its own block)
    auto add_task = [&](const dwh::CrTask& t, int id) {
      for (int h = 0; h < t.nt; ++h) {
        rd.push_back({t.a[h], id + (1 << 20)});
        rd.push_back({t.b[h], id + (1 << 20)});
      }
      if (t.cin >= 0) rd.push_back({t.cin, id});
      wr.push_back({t.out, id});
    };
    if (st.kind == 0) {
      ++ninv;
      for (int k = 0; k < st.n; ++k) {
        rd.push_back({pl.inv_blk[st.first + k], -1 - k});
        wr.push_back({pl.inv_dst[st.first + k], -1 - k});
      }
      if (st.ntiles > 0) ++nside;
      for (int k = 0; k < st.ntiles; ++k) add_task(pl.tasks[st.tfirst + k], k);
    } else if (st.kind == 2) {
      ++ngemm;
      for (int k = 0; k < st.n; ++k) {
        const int id = k + (1 << 21);
        if (st.sp == 0) {
          const dwh::CrSpFwd& t = pl.sp_fwd[st.first + k];
          for (int b : {t.dk, t.uk, t.lk, t.uel, t.lel, t.uer, t.ler, t.dir, t.dil}) rd.push_back({b, id});
          for (int b : {t.od, t.ou, t.ol}) wr.push_back({b, id});
        } else {
          const dwh::CrSpBwd& t = pl.sp_bwd[st.first + k];
          for (int b : {t.gaa, t.gac, t.gca, t.gcc, t.ua, t.le, t.la, t.ue}) rd.push_back({b, id});
          for (int b : {t.oza, t.ozc, t.oya, t.oyc, t.omx}) wr.push_back({b, id});
        }
      }
    } else {
      ++ngemm;
      for (int k = 0; k < st.n; ++k) add_task(pl.tasks[st.first + k], k);
    }
    ntask += (int64_t)wr.size();
    for (const auto& r : rd) {
      if (r.first < 0 || r.first >= pl.nblk || written[r.first] == -1) {
        std::snprintf(buf, sizeof buf, "stage %d reads block %d before any stage writes it", si, r.first);
        return fail(nullptr, DWH_ERR_STATE, buf);
      }
      for (const auto& w : wr)
        if (w.first == r.first && w.second != r.second) {
          std::snprintf(buf, sizeof buf, "stage %d reads block %d that the same stage writes", si, r.first);
          return fail(nullptr, DWH_ERR_STATE, buf);
        }
    }
    for (size_t i = 0; i < wr.size(); ++i)
      for (size_t j = i + 1; j < wr.size(); ++j)
        if (wr[i].first == wr[j].first && wr[i].second != wr[j].second) {
          std::snprintf(buf, sizeof buf, "stage %d writes block %d from two tasks", si, wr[i].first);
          return fail(nullptr, DWH_ERR_STATE, buf);
        }
    for (const auto& w : wr) {
      // level-0 blocks (refilled only at their pairing entries) and the static
      // R = A^-1 blocks of k_cr_inv0 are read on every step: nothing may
      // overwrite them
      if (w.first >= 0 && w.first < pl.nblk && written[w.first] == -2) {
        std::snprintf(buf, sizeof buf, "stage %d overwrites static block %d", si, w.first);
        return fail(nullptr, DWH_ERR_STATE, buf);
      }
      if (w.first >= 0 && w.first < pl.nblk && written[w.first] == -1) written[w.first] = si;
    }
  }
  const int64_t BB = (int64_t)(BP / 2) * BP;
  // the gathers read entries of tiles some stage wrote (the level-0 backward
  // stages compute only the tiles of their need sets, build_cr_plan)
  auto tile_ok = [&](int64_t o) {
    const int b = (int)(o / BB), r = (int)((o % BB) / BP), col = (int)(o % BP);
    return whole[b] || tiles_written.count({b, (r / 16) * ntc + col / 16}) > 0;
  };
  for (int64_t o : pl.goff)
    if (o >= 0 && (written[o / BB] == -1 || !tile_ok(o)))
      return fail(nullptr, DWH_ERR_STATE, "force gather reads an unwritten block / tile");
  for (int64_t o : pl.doff)
    if (written[o / BB] == -1 || !tile_ok(o)) return fail(nullptr, DWH_ERR_STATE, "E_f gather reads an unwritten block / tile");
  if (stats) {
    stats[0] = (int64_t)pl.stages.size();
    stats[1] = ninv;
    stats[2] = nside;
    stats[3] = ngemm;
    stats[4] = ntask;
    stats[5] = pl.nblk;
  }
  return DWH_OK;
}

// Per stage of the same plan, 10 values in out[10 i ..] (cap: stages out
// holds; *nstages: the plan's): kind (0 inversion, 1 products, 2 sparse
// forward, 3 sparse backward), the products' K split, bytes written per batch
// item by the stage's own outputs / its side products, launches until the
// first read of either (CrStageStores), the two store policies, and the bytes
// of either that the very next launch reads.
int dwh_debug_cr_plan_stores(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, int64_t* out,
                             int64_t cap, int64_t* nstages) {
  if (!out || !nstages || cap < 0) return fail(nullptr, DWH_ERR_ARG, "bad output");
  CrDims c;
  CrPlan pl;
  if (int rc = plan_periodic(Lx, Ly, nbatch, side, inv0, &c, &pl)) return rc;
  const std::vector<CrStageStores> ss = cr_stage_stores(pl, c.BP);
  *nstages = (int64_t)pl.stages.size();
  for (int64_t i = 0; i < *nstages && i < cap; ++i) {
    const CrStage& st = pl.stages[i];
    int64_t* o = out + 10 * i;
    o[0] = st.kind == 2 ? 2 + st.sp : st.kind;
    o[1] = st.kind == 1 ? st.cfg.ksplit : 0;
    o[2] = ss[i].bytes;
    o[3] = ss[i].bytes_side;
    o[4] = ss[i].first_read;
    o[5] = ss[i].first_read_side;
    o[6] = st.store;
    o[7] = st.store_side;
    o[8] = ss[i].bytes_next;
    o[9] = ss[i].bytes_side_next;
  }
  return DWH_OK;
}

int dwh_debug_cr_plan_flops(int64_t Lx, int64_t Ly, int64_t nbatch, int32_t side, int32_t inv0, double* flops) {
  if (!flops) return fail(nullptr, DWH_ERR_ARG, "bad lattice / batch / output");
  CrDims c;
  CrPlan pl;
  if (int rc = plan_periodic(Lx, Ly, nbatch, side, inv0, &c, &pl)) return rc;
  const int BP = c.BP;
  const double bp3 = 8.0 * BP * (double)BP * BP;
  flops[0] = flops[1] = flops[2] = 0.0;
  for (const CrStage& st : pl.stages) {
    if (st.kind == 0) {
      flops[0] += st.n * bp3;
      flops[2] += st.flops;
    } else {
      flops[1] += st.flops;
    }
  }
  return DWH_OK;
}

}  // extern "C"
