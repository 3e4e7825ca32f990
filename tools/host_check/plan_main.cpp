// Stand-alone host check of the cyclic-reduction planner and the model bounds,
// under AddressSanitizer and UBSan, without a device.  Build and run from the
// repository root:
//
//   C=hybrid-monte-carlo-for-d-wave-sc_amd/csrc
//   hipcc -Xarch_host -fsanitize=address,undefined -O1 -g -std=c++17 -Iinclude -I$C \
//       $C/dwhmc_plan.cpp $C/dwhmc_model.cpp tools/host_check/plan_main.cpp -o /tmp/plan_main
//   /tmp/plan_main
//
// It links dwhmc_plan.cpp and dwhmc_model.cpp only: that it links at all shows
// the two files call nothing that needs a device or a vendor library.  Runs
// dwh_debug_cr_plan_check, _flops and _stores over the lattices of
// tests/test_cr_plan_dataflow.py (both batch sizes, side / inv0 on and off,
// DWHMC_CR_SPARSE0 and DWHMC_CR_MERGE both ways) and dwh_debug_h_bound for one
// lattice.  Then the host side context creation runs, called directly:
// (a) build_host_model's tables on small and degenerate lattices against a
// dense restatement of the reference, (b) its refusals with their texts,
// (c) the dispatch-ordered slots plan_cr builds for the hottest kernel, over
// the same configurations, (d) the sparse level-0 stages' row records against
// a dense restatement of the level-0 U / L blocks, and the canonical-form
// rejection.  Exit status 0: every check passed (and no
// sanitizer report).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "dwhmc.h"
#include "dwhmc_model.h"   // build_host_model; dwh::g_create_error: the text dwh_last_error(NULL) returns in the library
#include "dwhmc_plan.h"    // plan_cr

namespace {

int failures = 0;

void expect(bool ok, const char* what, int Lx, int Ly, int nbatch, int side, int inv0, const char* sp, const char* mg) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: Lx=%d Ly=%d nbatch=%d side=%d inv0=%d SPARSE0=%s MERGE=%s: %s\n", what, Lx, Ly,
               nbatch, side, inv0, sp, mg, dwh::g_create_error.c_str());
}

void flunk(const char* what, int Lx, int Ly, long a = -1, long b = -1) {
  ++failures;
  std::fprintf(stderr, "FAIL %s: Lx=%d Ly=%d (%ld, %ld)\n", what, Lx, Ly, a, b);
}

// the reference's neighbour tables of a periodic Lx x Ly lattice
// (src/Types.jl:60-80), 1-based, [dir][site]
struct Tables {
  int Lx, Ly, N;
  std::vector<int64_t> nn, nnn;
  std::vector<double> dis;   // two chains
  Tables(int lx, int ly) : Lx(lx), Ly(ly), N(lx * ly), nn(4 * N), nnn(4 * N), dis(2 * N) {
    auto idx = [&](int x, int y) { return (int64_t)(((y + Ly) % Ly) * Lx + (x + Lx) % Lx) + 1; };
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
    for (int i = 0; i < 2 * N; ++i) dis[i] = 0.8 * std::sin(1.0 + 0.37 * i);
  }
  int build(dwh::HostModel* m, bool lanczos = true, double tp = -0.35) const {
    return dwh::build_host_model(Lx, Ly, 1.0, tp, -1.08, nn.data(), nnn.data(), 2, dis.data(), m, lanczos);
  }
};

// (a) the model's tables against dense N x N matrices filled in the
// reference's loop order, later writes winning: h (src/Hamiltonian.jl:10-47),
// the pairing source index (:55-86: entry (r, c) of the pairing block holds
// Delta[src] / 2) and the summed x-current operator (src/Observables.jl:237-283)
void check_tables(int Lx, int Ly) {
  using namespace dwh;
  const Tables T(Lx, Ly);
  const int N = T.N;
  const double t = 1.0, tp = -0.35, mu = -1.08;
  HostModel m;
  if (T.build(&m) != DWH_OK) return flunk("build_host_model", Lx, Ly);
  auto NN = [&](int i, int dir) { return (int)T.nn[(size_t)dir * N + i] - 1; };
  auto NNN = [&](int i, int dir) { return (int)T.nnn[(size_t)dir * N + i] - 1; };
  std::vector<double> h((size_t)N * N, 0.0), J((size_t)N * N, 0.0);
  std::vector<int> src((size_t)N * N, -1);
  for (int i = 0; i < N; ++i) {   // upper triangle, NN then NNN
    for (int dir = 0; dir < 4; ++dir)
      if (NN(i, dir) > i) h[(size_t)i * N + NN(i, dir)] = -t;
    for (int dir = 0; dir < 4; ++dir)
      if (NNN(i, dir) > i) h[(size_t)i * N + NNN(i, dir)] = -tp;
  }
  for (int i = 0; i < N; ++i)   // Hermitian completion
    for (int j = i + 1; j < N; ++j) h[(size_t)j * N + i] = h[(size_t)i * N + j];
  for (int i = 0; i < N; ++i)   // +x bond, then +y bond, both orientations
    for (int dir = 0; dir < 2; ++dir) {
      const int j = NN(i, dir);
      src[(size_t)i * N + j] = i + N * dir;
      src[(size_t)j * N + i] = i + N * dir;
    }
  for (int i = 0; i < N; ++i) {   // imaginary parts: +val at (i, j), conj(val) at (j, i)
    const int js[3] = {NN(i, 0), NNN(i, 0), NNN(i, 3)};
    const double ts[3] = {t, tp, tp};
    for (int b = 0; b < 3; ++b) {
      J[(size_t)i * N + js[b]] += ts[b];
      J[(size_t)js[b] * N + i] -= ts[b];
    }
  }
  if ((int)m.hcol.size() != N * kHSlots || (int)m.hval.size() != 2 * N * kHSlots || (int)m.Dcol.size() != N * kSlots ||
      (int)m.Dsrc.size() != N * kSlots || (int)m.bij.size() != 2 * N || (int)m.bji.size() != 2 * N ||
      (int)m.tr_rowptr.size() != N + 1 || (int)m.tr_nbr.size() != 3 * N)
    return flunk("table sizes", Lx, Ly);
  for (int r = 0; r < N; ++r) {
    // hopping: slot 0 the diagonal w - mu of each chain, then the partners
    std::vector<char> seen(N, 0);
    for (int s = 0; s < kHSlots; ++s) {
      const int c = m.hcol[(size_t)r * kHSlots + s];
      if (s == 0 ? c != r : (c < -1 || c >= N || c == r)) return flunk("hcol entry", Lx, Ly, r, s);
      for (int ch = 0; ch < 2; ++ch) {
        const double v = m.hval[((size_t)ch * N + r) * kHSlots + s];
        const double want = s == 0 ? T.dis[(size_t)ch * N + r] - mu : c < 0 ? 0.0 : h[(size_t)r * N + c];
        if (v != want) flunk("hval entry", Lx, Ly, r, s);
      }
      if (c >= 0 && s > 0) {
        if (seen[c]) flunk("hcol duplicate", Lx, Ly, r, c);
        seen[c] = 1;
      }
    }
    for (int c = 0; c < N; ++c)
      if (h[(size_t)r * N + c] != 0.0 && !seen[c]) flunk("h entry missing from hcol", Lx, Ly, r, c);
    // pairing pattern
    std::fill(seen.begin(), seen.end(), 0);
    for (int s = 0; s < kSlots; ++s) {
      const int c = m.Dcol[(size_t)r * kSlots + s], sr = m.Dsrc[(size_t)r * kSlots + s];
      if (c < -1 || c >= N) return flunk("Dcol entry", Lx, Ly, r, s);
      if (sr != (c < 0 ? -1 : src[(size_t)r * N + c])) flunk("Dsrc entry", Lx, Ly, r, s);
      if (c >= 0) {
        if (seen[c]) flunk("Dcol duplicate", Lx, Ly, r, c);
        seen[c] = 1;
      }
    }
    for (int c = 0; c < N; ++c)
      if (src[(size_t)r * N + c] >= 0 && !seen[c]) flunk("pairing entry missing from Dcol", Lx, Ly, r, c);
    // current operator: ascending columns, every stored value the dense sum
    std::fill(seen.begin(), seen.end(), 0);
    const int e0 = m.tr_rowptr[r], e1 = m.tr_rowptr[r + 1];
    if (e0 < 0 || e1 < e0 || e1 > (int)m.tr_col.size() || m.tr_col.size() != m.tr_val.size())
      return flunk("current rowptr", Lx, Ly, r);
    for (int e = e0; e < e1; ++e) {
      const int c = m.tr_col[e];
      if (c < 0 || c >= N || (e > e0 && c <= m.tr_col[e - 1])) return flunk("current column", Lx, Ly, r, e);
      if (m.tr_val[e] != J[(size_t)r * N + c]) flunk("current value", Lx, Ly, r, c);
      seen[c] = 1;
    }
    for (int c = 0; c < N; ++c)
      if (J[(size_t)r * N + c] != 0.0 && !seen[c]) flunk("current entry missing from the CSR", Lx, Ly, r, c);
  }
  if (m.tr_rowptr[0] != 0 || m.tr_rowptr[N] != (int)m.tr_col.size()) flunk("current rowptr ends", Lx, Ly);
  // bond slots: (row, slot) entries whose column is the bond's other end
  for (int dir = 0; dir < 2; ++dir)
    for (int i = 0; i < N; ++i) {
      const int j = NN(i, dir), e1 = m.bij[(size_t)dir * N + i], e2 = m.bji[(size_t)dir * N + i];
      if (e1 < 0 || e1 >= N * kSlots || e2 < 0 || e2 >= N * kSlots) return flunk("bond slot range", Lx, Ly, dir, i);
      if (e1 / kSlots != i || m.Dcol[e1] != j) flunk("bij", Lx, Ly, dir, i);
      if (e2 / kSlots != j || m.Dcol[e2] != i) flunk("bji", Lx, Ly, dir, i);
      if (m.tr_nbr[i] != NN(i, 0) || m.tr_nbr[N + i] != NNN(i, 0) || m.tr_nbr[2 * N + i] != NNN(i, 3))
        flunk("tr_nbr", Lx, Ly, dir, i);
    }
}

// (b) one refusal of build_host_model with its text
void expect_refusal(const char* what, const Tables& T, const char* text) {
  dwh::HostModel m;
  const int rc = T.build(&m);
  if (rc == DWH_ERR_ARG && dwh::g_create_error == text) return;
  ++failures;
  std::fprintf(stderr, "FAIL refusal (%s): rc=%d \"%s\", expected \"%s\"\n", what, rc, dwh::g_create_error.c_str(), text);
}

// (c) the dispatch-ordered slots k_cr_gemm16 indexes, as plan_cr built them.
// cr_gemm_slots' contract: a stage's nbatch x ntiles output tiles (batch item
// major) are dealt to nswg = ceil(nbatch ntiles / tpw) workgroups of tpw =
// 4 / ksplit slots, workgroup b taking the tpw consecutive tiles from
// xcd_remap(b, nswg) tpw.  The remap is a permutation of the workgroups, so
// every tile has exactly one slot: nbatch ntiles slots are filled, each (batch
// item, output tile) once, and the < tpw slots left over are marked empty.
// A filled slot's offsets address 16 x 16 tiles inside a block of its batch
// item: out / cin at (16 tr, 16 tc) of an HP x BP block, a[h] at the start of
// rows 16 tr, b[h] at column 16 tc of row 0.
void check_slots(const dwh::CrDims& c, const dwh::CrPlan& pl, int Lx, int Ly, int nbatch) {
  using namespace dwh;
  const int HP = c.BP / 2;
  const int64_t BB = (int64_t)HP * c.BP;
  if (c.item != BB * c.nblk) flunk("slots: item size", Lx, Ly);
  // row / column of an offset's 16 x 16 tile inside its block; false when the
  // tile leaves the block or the batch item
  auto tile_in_block = [&](uint32_t off, int* row, int* col) {
    if ((int64_t)off + 15 * c.BP + 16 > c.item) return false;
    *row = (int)((off % BB) / c.BP);
    *col = (int)(off % c.BP);
    return *row + 16 <= HP && *col + 16 <= c.BP;
  };
  size_t covered = 0;
  for (const CrStage& st : pl.stages) {
    if (st.kind != 1) continue;
    if (st.cfg.ts != 16 || (st.cfg.ksplit != 1 && st.cfg.ksplit != 2 && st.cfg.ksplit != 4))
      return flunk("slots: stage configuration", Lx, Ly, st.cfg.ts, st.cfg.ksplit);
    const int tpw = 4 / st.cfg.ksplit;
    const int64_t total = (int64_t)nbatch * st.ntiles, nslot = (int64_t)st.nswg * tpw;
    if (st.nswg != (total + tpw - 1) / tpw || st.sfirst < 0 || (size_t)st.sfirst != covered ||
        (size_t)(st.sfirst + nslot) > pl.slots.size())
      return flunk("slots: stage range", Lx, Ly, st.sfirst, st.nswg);
    covered += (size_t)nslot;
    int64_t filled = 0;
    std::set<std::pair<uint64_t, uint32_t>> outs;
    for (int64_t k = 0; k < nslot; ++k) {
      const CrSlot& sl = pl.slots[(size_t)(st.sfirst + k)];
      if (sl.out == kCrNone) {
        if (sl.cin != kCrNone) flunk("slots: empty slot with an accumulate input", Lx, Ly, k);
        continue;
      }
      ++filled;
      int r = 0, col = 0, r2 = 0, col2 = 0;
      if (sl.base % (uint64_t)c.item != 0 || sl.base / (uint64_t)c.item >= (uint64_t)nbatch)
        flunk("slots: batch item", Lx, Ly, k);
      if (!tile_in_block(sl.out, &r, &col) || r % 16 || col % 16) flunk("slots: out", Lx, Ly, k);
      if (sl.cin != kCrNone && (!tile_in_block(sl.cin, &r2, &col2) || r2 != r || col2 != col)) flunk("slots: cin", Lx, Ly, k);
      if (sl.nt < 1 || sl.nt > 4) {
        flunk("slots: nt", Lx, Ly, k, sl.nt);
        continue;
      }
      for (int h = 0; h < sl.nt; ++h) {
        if (!tile_in_block(sl.a[h], &r2, &col2) || r2 != r || col2 != 0) flunk("slots: a[h]", Lx, Ly, k, h);
        if (!tile_in_block(sl.b[h], &r2, &col2) || r2 != 0 || col2 != col) flunk("slots: b[h]", Lx, Ly, k, h);
      }
      if (!outs.insert({sl.base, sl.out}).second) flunk("slots: output tile dealt twice", Lx, Ly, k);
    }
    if (filled != total) flunk("slots: filled count", Lx, Ly, (long)filled, (long)total);
  }
  if (covered != pl.slots.size()) flunk("slots: array size", Lx, Ly, (long)covered, (long)pl.slots.size());
}

// (d) the row records of the sparse level-0 stages (cr_sparse_task_arrays):
// every top-half row of every level-0 U[y] = A[y, y+1] / L[y] = A[y+1, y]
// rebuilt from the records' slots equals the dense restatement (h in the
// reference's loop order, later writes winning; the pairing source index),
// with the forward stage's sign; every offset is a row start inside the block
// it is meant for.  Blocks are rows of the CR lattice (rows lattice rows each).
int sparse_stages(const dwh::CrPlan& pl) {
  int n = 0;
  for (const dwh::CrStage& st : pl.stages) n += st.kind == 2;
  return n;
}
void check_records(int Lx, int Ly, double tp) {
  using namespace dwh;
  const Tables T(Lx, Ly);
  const int N = T.N;
  HostModel m;
  if (T.build(&m, false, tp) != DWH_OK) return flunk("records: build_host_model", Lx, Ly);
  CrDims c;
  CrPlan pl;
  if (plan_cr(Lx, Ly, 7, 14, m.Dcol, m.hcol, 1, 1, 256, &c, &pl) != DWH_OK) return flunk("records: plan_cr", Lx, Ly);
  if (sparse_stages(pl) != 2) return flunk("records: not a sparse level 0", Lx, Ly, sparse_stages(pl));
  const SpTaskArrays a = cr_sparse_task_arrays(pl, c.Lx, c.Ly, c.BP, m.hcol, m.hval, m.Dcol, m.Dsrc);
  const int HP = c.BP / 2, Lc = c.Lx, Lyc = c.Ly;
  if (a.rf.size() != pl.sp_fwd.size() * HP || a.rb.size() != pl.sp_bwd.size() * HP)
    return flunk("records: count", Lx, Ly, (long)a.rf.size(), (long)a.rb.size());
  auto NN = [&](int i, int dir) { return (int)T.nn[(size_t)dir * N + i] - 1; };
  auto NNN = [&](int i, int dir) { return (int)T.nnn[(size_t)dir * N + i] - 1; };
  std::vector<double> h((size_t)N * N, 0.0);
  std::vector<int> src((size_t)N * N, -1);
  for (int i = 0; i < N; ++i) {
    for (int dir = 0; dir < 4; ++dir)
      if (NN(i, dir) > i) h[(size_t)i * N + NN(i, dir)] = -1.0;
    for (int dir = 0; dir < 4; ++dir)
      if (NNN(i, dir) > i) h[(size_t)i * N + NNN(i, dir)] = -tp;
  }
  for (int i = 0; i < N; ++i)
    for (int j = i + 1; j < N; ++j) h[(size_t)j * N + i] = h[(size_t)i * N + j];
  for (int i = 0; i < N; ++i)
    for (int dir = 0; dir < 2; ++dir) {
      const int j = NN(i, dir);
      src[(size_t)i * N + j] = i + N * dir;
      src[(size_t)j * N + i] = i + N * dir;
    }
  const uint64_t rowb = (uint64_t)c.BP * sizeof(double2), blkb = rowb * HP;
  std::vector<char> covered(3 * Lyc, 0);
  // row r of sparse level-0 block sb (record slots hv / ho / ps / po / pd,
  // values times sg) against the dense rows; the slots address rows of block db
  auto row = [&](int sb, int r, const double* hv, const uint32_t* const* ho, int nho, double ps,
                 const uint32_t* const* po, uint32_t pd, double sg, const int* db) {
    const int t = sb / Lyc, y = sb % Lyc;
    if (t < 1 || t > 2) return flunk("records: sparse operand is not a level-0 U / L", Lx, Ly, sb);
    covered[sb] = 1;
    const int yr = (t == 2) ? (y + 1) % Lyc : y, yc = (t == 1) ? (y + 1) % Lyc : y;
    std::vector<double> got(HP, 0.0), want(HP, 0.0);
    int wk = -1, wsrc = -1;
    if (r < Lc)
      for (int k = 0; k < Lc; ++k) {
        const int i = yr * Lc + r, j = yc * Lc + k;
        want[k] = h[(size_t)i * N + j];
        if (src[(size_t)i * N + j] >= 0) {
          if (wk >= 0) flunk("records: two pairing partners in one row", Lx, Ly, sb, r);
          wk = k;
          wsrc = src[(size_t)i * N + j];
        }
      }
    for (int e = 0; e < kCrSpNZ - 1; ++e) {
      int k = -1;
      for (int g = 0; g < nho; ++g) {
        const uint64_t o = ho[g][e], b0 = (uint64_t)db[g] * blkb;
        if (o < b0 || o >= b0 + blkb || (o - b0) % rowb) return flunk("records: hopping offset outside its block", Lx, Ly, sb, r);
        if (g && (int)((o - b0) / rowb) != k) flunk("records: the two dense rows of a slot differ", Lx, Ly, sb, r);
        k = (int)((o - b0) / rowb);
      }
      got[k] += sg * hv[e];
    }
    for (int k = 0; k < HP; ++k)
      if (got[k] != want[k]) flunk("records: hopping row", Lx, Ly, sb, r);
    int pk = -1;
    for (int g = 0; g < nho; ++g) {
      const uint64_t o = po[g][0], b0 = (uint64_t)db[g] * blkb;
      if (o < b0 || o >= b0 + blkb || (o - b0) % rowb) return flunk("records: pairing offset outside its block", Lx, Ly, sb, r);
      if (g && (int)((o - b0) / rowb) != pk) flunk("records: the two dense rows of the pairing slot differ", Lx, Ly, sb, r);
      pk = (int)((o - b0) / rowb);
    }
    if (pd >= (uint32_t)(2 * N)) return flunk("records: pairing index outside Delta", Lx, Ly, sb, r);
    if (wk < 0 ? ps != 0.0 : (sg * ps != 0.5 || pk != wk || (int)pd != wsrc)) flunk("records: pairing slot", Lx, Ly, sb, r);
  };
  auto in_row = [&](uint32_t o, int b, int r) { return (uint64_t)o == (uint64_t)b * blkb + (uint64_t)r * rowb; };
  for (size_t ti = 0; ti < pl.sp_fwd.size(); ++ti) {
    const CrSpFwd& t = pl.sp_fwd[ti];
    const int sparse[3] = {t.uk, t.ler, t.lel}, dense[3] = {t.dir, t.dir, t.dil};
    for (int r = 0; r < HP; ++r) {
      const CrSpRowFwd& q = a.rf[ti * HP + r];
      for (int o = 0; o < 3; ++o) {
        const uint32_t *ho = q.ho[o], *po = &q.po[o];
        row(sparse[o], r, q.hv[o], &ho, 1, q.ps[o], &po, q.pd[o], -1.0, &dense[o]);
      }
      if (!in_row(q.dk, t.dk, r) || !in_row(q.od, t.od, r) || !in_row(q.ou, t.ou, r) || !in_row(q.ol, t.ol, r))
        flunk("records: forward dense rows", Lx, Ly, (long)ti, r);
    }
  }
  for (size_t ti = 0; ti < pl.sp_bwd.size(); ++ti) {
    const CrSpBwd& t = pl.sp_bwd[ti];
    const int sparse[2] = {t.la, t.ue}, dense[2][2] = {{t.gaa, t.gac}, {t.gca, t.gcc}};
    for (int r = 0; r < HP; ++r) {
      const CrSpRowBwd& q = a.rb[ti * HP + r];
      for (int o = 0; o < 2; ++o) {
        const uint32_t *ho[2] = {q.ho[o][0], q.ho[o][1]}, *po[2] = {&q.po[o][0], &q.po[o][1]};
        row(sparse[o], r, q.hv[o], ho, 2, q.ps[o], po, q.pd[o], 1.0, dense[o]);
      }
      if (!in_row(q.g[0], t.gaa, r) || !in_row(q.g[1], t.gca, r) || !in_row(q.g[2], t.gac, r) ||
          !in_row(q.g[3], t.gcc, r) || !in_row(q.oza, t.oza, r) || !in_row(q.ozc, t.ozc, r) ||
          !in_row(q.oya, t.oya, r) || !in_row(q.oyc, t.oyc, r) || !in_row(q.omx, t.omx, r))
        flunk("records: backward dense rows", Lx, Ly, (long)ti, r);
    }
  }
  for (int b = Lyc; b < 3 * Lyc; ++b)
    if (!covered[b]) flunk("records: a level-0 U / L block no record reads", Lx, Ly, b);
}

// a top-half row the records cannot hold — a second pairing partner, or a
// fourth hopping partner, in the neighbouring row — makes the plan run the
// dense level 0, exactly as an over-full row does
void check_canonical_rejection() {
  const int Lx = 20, Ly = 4;
  dwh::HostModel m;
  if (Tables(Lx, Ly).build(&m, false) != DWH_OK) return flunk("rejection: build_host_model", Lx, Ly);
  dwh::CrDims c;
  dwh::CrPlan pl;
  auto stages = [&](const std::vector<int>& Dcol, const std::vector<int>& hcol) {
    return dwh::plan_cr(Lx, Ly, 7, 14, Dcol, hcol, 1, 1, 256, &c, &pl) == DWH_OK ? sparse_stages(pl) : -1;
  };
  if (stages(m.Dcol, m.hcol) != 2) flunk("rejection: the plain lattice is sparse-capable", Lx, Ly);
  // site 0: its same-row partner (site 1) replaced by a site of the next row
  std::vector<int> Dcol = m.Dcol, hcol = m.hcol;
  bool did = false;
  for (int s = 0; s < dwh::kSlots; ++s)
    if (Dcol[s] == 1) Dcol[s] = Lx + 5, did = true;
  if (!did || stages(Dcol, m.hcol) != 0) flunk("rejection: two pairing entries in a top-half row", Lx, Ly);
  did = false;
  for (int s = 1; s < dwh::kHSlots; ++s)
    if (hcol[s] == 1) hcol[s] = Lx + 5, did = true;
  if (!did || stages(m.Dcol, hcol) != 0) flunk("rejection: four hopping entries in a top-half row", Lx, Ly);
}

}  // namespace

int main() {
  const int lattices[][2] = {{4, 1},   {4, 2},   {3, 3},   {5, 7},   {8, 8},  {6, 9},   {17, 4},
                             {20, 6},  {32, 2},  {32, 3},  {32, 5},  {32, 16}, {32, 31}, {32, 32},
                             {32, 33}, {40, 3},  {48, 12}, {64, 2},  {64, 9}};
  int nconf = 0;
  for (const char* sp : {"1", "0"})
    for (const char* mg : {"8", "0"}) {
      setenv("DWHMC_CR_SPARSE0", sp, 1);
      setenv("DWHMC_CR_MERGE", mg, 1);
      for (const auto& l : lattices)
        for (int nbatch : {14, 56})
          for (int side = 0; side < 2; ++side)
            for (int inv0 = 0; inv0 < 2; ++inv0) {
              ++nconf;
              int64_t st[6] = {0, 0, 0, 0, 0, 0};
              const int rc = dwh_debug_cr_plan_check(l[0], l[1], nbatch, side, inv0, st);
              // every stage is an inversion or a product launch, at least one inversion
              expect(rc == DWH_OK && st[0] == st[1] + st[3] && st[1] >= 1, "plan_check", l[0], l[1], nbatch, side,
                     inv0, sp, mg);
              double fl[3] = {0, 0, 0};
              const int rf = dwh_debug_cr_plan_flops(l[0], l[1], nbatch, side, inv0, fl);
              expect(rf == DWH_OK && std::isfinite(fl[0] + fl[1] + fl[2]) && fl[0] > 0 && fl[1] >= 0 && fl[2] >= 0 &&
                         (side || fl[2] == 0.0),
                     "plan_flops", l[0], l[1], nbatch, side, inv0, sp, mg);
              // what every stage stores: some bytes, and never more read by the next launch than written
              std::vector<int64_t> ss(10 * (size_t)st[0]);
              int64_t ns = 0;
              bool ok = dwh_debug_cr_plan_stores(l[0], l[1], nbatch, side, inv0, ss.data(), st[0], &ns) == DWH_OK &&
                        ns == st[0];
              for (int64_t i = 0; ok && i < ns; ++i) {
                const int64_t* o = &ss[10 * i];
                ok = o[2] > 0 && o[8] >= 0 && o[8] <= o[2] && o[9] >= 0 && o[9] <= o[3] && o[4] >= 1 && o[6] >= 0 &&
                     o[6] <= 2 && o[7] >= 0 && o[7] <= 2;
              }
              expect(ok, "plan_stores", l[0], l[1], nbatch, side, inv0, sp, mg);
            }
    }
  // a lattice row too wide for the CR path is refused, not planned
  if (dwh_debug_cr_plan_check(65, 4, 14, 1, 1, nullptr) == DWH_OK) {
    ++failures;
    std::fprintf(stderr, "FAIL plan_check accepted Lx = 65\n");
  }


  // ||h|| bound of a periodic 6 x 5 lattice with the reference's tables, two chains
  {
    const Tables T(6, 5);
    double out[5] = {0, 0, 0, 0, 0};
    const int rc = dwh_debug_h_bound(T.Lx, T.Ly, 1.0, -0.35, -1.08, T.nn.data(), T.nnn.data(), 2, T.dis.data(), out);
    // the bound used is the Gershgorin one or a smaller certified Lanczos value
    if (rc != DWH_OK || !(out[3] > 0) || !(out[3] <= out[0]) || !(out[2] == 0.0 || out[3] == out[1])) {
      ++failures;
      std::fprintf(stderr, "FAIL h_bound rc=%d gersh=%g lanczos=%g certified=%g used=%g: %s\n", rc, out[0], out[1],
                   out[2], out[3], dwh::g_create_error.c_str());
    }
  }

  // (a) tables, the degenerate lattices included: 1 x 1, a single row, Lx or
  // Ly = 2 (where +x and -x are the same site)
  const int small[][2] = {{1, 1}, {1, 4}, {2, 2}, {2, 5}, {3, 3}, {4, 6}, {7, 5}};
  for (const auto& l : small) check_tables(l[0], l[1]);

  // (b) refusals
  {
    Tables zero(3, 3), past(3, 3), nonfinite(3, 3), crowded(1, 6);
    zero.nn[5] = 0;
    past.nnn[7] = past.N + 1;
    nonfinite.dis[4] = std::nan("");
    for (int i = 0; i < crowded.N; ++i) crowded.nn[i] = 1;   // every +x neighbour is site 1
    expect_refusal("neighbour entry 0", zero, "neighbour table entry out of [1, N]");
    expect_refusal("neighbour entry N + 1", past, "neighbour table entry out of [1, N]");
    expect_refusal("non-finite disorder", nonfinite, "non-finite disorder");
    expect_refusal("six partners of one site", crowded, "more than 4 pairing partners per site");
  }

  // (c) the slots of every 16 x 16 product stage, over the same configurations
  int nslotconf = 0;
  for (const char* sp : {"1", "0"})
    for (const char* mg : {"8", "0"}) {
      setenv("DWHMC_CR_SPARSE0", sp, 1);
      setenv("DWHMC_CR_MERGE", mg, 1);
      for (const auto& l : lattices) {
        dwh::HostModel m;
        if (Tables(l[0], l[1]).build(&m, false) != DWH_OK) {
          flunk("build_host_model", l[0], l[1]);
          continue;
        }
        for (int nbatch : {14, 56})
          for (int side = 0; side < 2; ++side)
            for (int inv0 = 0; inv0 < 2; ++inv0) {
              ++nslotconf;
              dwh::CrDims c;
              dwh::CrPlan pl;
              if (dwh::plan_cr(l[0], l[1], 7, nbatch, m.Dcol, m.hcol, side, inv0, 256, &c, &pl) != DWH_OK)
                flunk("plan_cr", l[0], l[1], side, inv0);
              else
                check_slots(c, pl, l[0], l[1], nbatch);
            }
      }
    }
  if (nslotconf != nconf) flunk("slot configurations", nslotconf, nconf);

  // (d) row records: t' = 0 (empty hopping slots), Lx = 3 (x - 1 = x + 1 + wrap,
  // grouped rows), 8 x 8 (two-row blocks), Ly = 4 with a padded (Lx = 20) and an
  // exactly filled (Lx = 32) BP = 64, BP = 96 (Lx = 40), and a longer chain
  setenv("DWHMC_CR_SPARSE0", "1", 1);
  setenv("DWHMC_CR_MERGE", "8", 1);
  const int reclat[][2] = {{20, 4}, {3, 16}, {3, 20}, {8, 8}, {32, 4}, {40, 4}, {16, 4}, {20, 6}, {32, 32}};
  for (const auto& l : reclat)
    for (double tp : {-0.35, 0.0}) check_records(l[0], l[1], tp);
  check_canonical_rejection();
  std::printf("plan_main: %d plan configurations, %d failure(s)\n", nconf, failures);
  return failures ? 1 : 0;
}
