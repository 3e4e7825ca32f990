// Sparse level-0 stages of the block cyclic reduction (round 5).
//
// The level-0 off-diagonal blocks U[y] = A[y, y+1] and L[y] = A[y+1, y] of
// A = H_BdG - i y_q couple neighbouring lattice rows only through the vertical
// hopping (-t at x, -t' at x ± 1: src/Hamiltonian.jl:26-43) and the vertical
// pairing entry Δ/2 (src/Hamiltonian.jl:68-83): at most 4 nonzeros in every
// row and column of the BP x BP block.  Level 0 is the largest level of the
// recursion, and every product there that has a U or L factor is a sparse one,
// so the level-0 forward pass after the inversions and the sparse half of the
// backward pass run here on the vector units, with no dense V1, V2, W1, W2
// (tools/cr_model.py cr_selected_inverse_top_sparse0 states the algebra and
// checks it against dense inverses):
//
//   forward (k_cr_sp_fwd, per kept row k, er = k+1, el = k-1):
//     V1r = -U_k Dinv_er,  V2r = -L_er Dinv_er,  V2l = -L_el Dinv_el   (one row at a time, in LDS)
//     D'_k = D_k + V1r L_k + V2l U_el,  U'_k = V1r U_er,  L'_k = V2r L_k
//   backward (k_cr_sp_bwd, per eliminated row e, a = e-1, c = e+1):
//     Z_a = G_aa U_a + G_ac L_e,  Z_c = G_ca U_a + G_cc L_e     (dense . sparse)
//     Y_a = L_a G_aa + U_e G_ca,  Y_c = L_a G_ac + U_e G_cc     (sparse . dense)
//     M   = L_a Z_a + U_e Z_c = Y_a U_a + Y_c L_e               (dense . sparse, Y rows in LDS)
//   after which one-term dense products (k_cr_gemm) finish the level:
//     G_ae = -Z_a Dinv, G_ce = -Z_c Dinv, G_ea = -Dinv Y_a, G_ec = -Dinv Y_c,
//     T = -Dinv M, then G_ee = Dinv - T Dinv.
//
// Blocks are top halves (HP x BP) of M-form [[A, B], [conj B, -conj A]] or
// Q-form [[A, B], [-conj B, conj A]] blocks (dwhmc_cr.hip).  Everything about
// the sparse operands except Δ is fixed at context creation, so the host
// resolves it (dwhmc_plan.cpp):
//   left operands (sparse . dense): one record per (task, output row)
//   (CrSpRowFwd / CrSpRowBwd, dwhmc_internal.h) with the row's kCrSpNZ - 1
//   hopping slots — static value, sign applied, and the offset of the dense
//   operand's stored row — then its pairing slot — ±1/2, the Δ index and the
//   stored row the synthesised bottom row comes from — and the task's own
//   dense rows.  A wave reads it with a few wide scalar loads at an index
//   that needs only the workgroup id; the Δ load of the pairing slots is the
//   one dependent value before the dense element loads.  Which slot reads a
//   stored row and which a synthesised one is fixed by the slot order.
//   right operands (dense . sparse): per-task column arrays [operand][entry]
//   [BP] of values and meta words, staged once per workgroup in LDS.
// One wave per output row: every row of every output depends only on rows of
// the inputs, and the backward M = L_a Z_a + U_e Z_c is formed as
// Y_a U_a + Y_c L_e (the same sum regrouped), from the wave's own Y rows.
#include "dwhmc_device.h"
#include "dwhmc_internal.h"

namespace dwh {
namespace {

// a += b c
__device__ __forceinline__ void cmac(double2& a, double2 b, double2 c) {
  a.x = fma(b.x, c.x, fma(-b.y, c.y, a.x));
  a.y = fma(b.x, c.y, fma(b.y, c.x, a.y));
}
// a += s c, s real
__device__ __forceinline__ void rmac(double2& a, double s, double2 c) {
  a.x = fma(s, c.x, a.x);
  a.y = fma(s, c.y, a.y);
}

__device__ __forceinline__ double sp_flip(double x, unsigned m) {
  return __builtin_bit_cast(double, __builtin_bit_cast(unsigned long long, x) ^ ((unsigned long long)m << 32));
}

// a wave-uniform double back in scalar registers
__device__ __forceinline__ double sp_uniform(double x) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return __builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);
}

// Column c of the synthesised bottom half of an M-form block whose top half
// is stored: element (HP + k, c) = conj(X[k, c + HP]) (c < HP) or
// -conj(X[k, c - HP]) (c >= HP) — one load at the rotated column and two
// lane-constant sign-bit XORs.  Columns and rows as byte offsets.
template <int BP>
struct BotCol {
  unsigned crot;
  unsigned mx, my;   // sign-bit masks of the real / imaginary part
  __device__ __forceinline__ explicit BotCol(unsigned cb) {
    constexpr unsigned HB = BP / 2 * sizeof(double2);
    crot = cb < HB ? cb + HB : cb - HB;
    mx = cb >= HB ? 0x80000000u : 0u;
    my = cb < HB ? 0x80000000u : 0u;
  }
  // the stored element behind it: row = the stored row k of a pool block,
  // from the batch item's base; sign() then makes it the synthesised one
  __device__ __forceinline__ double2 ld(const double2* base, unsigned row) const {
    return *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(base) + (row + crot));
  }
  __device__ __forceinline__ double2 sign(double2 u) const {
    return make_double2(sp_flip(u.x, mx), sp_flip(u.y, my));
  }
};

// column entry: a static hopping value (v, op applied) or, for a pairing
// entry, op(Δ[src] / 2) (the value k_cr_fill keeps in the pool) — never both;
// meta word m: src + 1 (0: none) in bits 0-21, op in 22-23 (1 conj,
// 2 -conj), row in 24-31.  x: the entry's one load (tcv or Δ).
__device__ __forceinline__ double2 sp_cval(double2 x, int m) {
  if ((m & 0x3fffff) == 0) return x;
  const int op = (m >> 22) & 3;
  return make_double2(op == 2 ? -0.5 * x.x : 0.5 * x.x, op == 0 ? 0.5 * x.y : -0.5 * x.y);   // op 1: conj, 2: -conj
}

constexpr int kSpRowsWG = 4;   // one output row per wave at a time, four waves per workgroup
constexpr int NZ = kCrSpNZ, NH = kCrSpNZ - 1;   // slots per row: NH hopping, then the pairing slot
// waves per SIMD the register budget is sized for at BP <= 64: six (<= 80
// VGPRs) for both stages, so the C3 stages (1536 workgroups of 25.5 / 25 KB
// LDS, six per CU) are resident in one round (-DSP_WAVES_F / -DSP_WAVES_B
// for A/B builds)
#ifndef SP_WAVES_F
#define SP_WAVES_F 6
#endif
#ifndef SP_WAVES_B
#define SP_WAVES_B 6
#endif
// output rows a backward wave takes in turn (its workgroup stages the column
// data once for all of them).  One: two rows (-DSP_RPW_B=2), at five or six
// waves, and five waves with one row all measured slower
// (profiles/sparse_records_ab.txt)
#ifndef SP_RPW_B
#define SP_RPW_B 1
#endif
template <int BP>
constexpr int kSpWavesF = BP <= 64 ? SP_WAVES_F : 2;
template <int BP>
constexpr int kSpWavesB = BP <= 64 ? SP_WAVES_B : 2;

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// element at byte offset off (32 bits: a uniform base plus one offset
// register per load) of a batch item's pool / of a staged LDS row
__device__ __forceinline__ double2 sp_ld(const double2* base, unsigned off) {
  return *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(base) + off);
}
// ST: the store policy of a pool store (st16); the staged LDS rows stay plain
template <int ST = kStorePlain>
__device__ __forceinline__ void sp_st(double2* base, unsigned off, double2 v) {
  st16<ST>(reinterpret_cast<double2*>(reinterpret_cast<char*>(base) + off), v);
}

// Column data of the sparse right operands (dense . sparse products): every
// output row of a workgroup uses the same column patterns, so the workgroup
// stages them once in LDS — the value of each entry and the LDS byte offset
// of its row's element in a staged double2 row — from the task's own column
// arrays (tcm / tcv: [NB][kCrSpNZ][BP], coalesced).  Three steps, so the meta
// words are the kernel's first loads and the values (one load per entry
// behind its meta word: the static value or Δ) follow the dense loads.
template <int BP, int NB>
struct ColStage {
  static constexpr int TOT = NB * NZ * BP, IT = (TOT + 64 * kSpRowsWG - 1) / (64 * kSpRowsWG);
  int m[IT];
  double2 x[IT];
  __device__ __forceinline__ void load_meta(const int* __restrict__ tcm) {
#pragma unroll
    for (int i = 0; i < IT; ++i) m[i] = tcm[min((int)threadIdx.x + 64 * kSpRowsWG * i, TOT - 1)];
  }
  __device__ __forceinline__ void load_values(const double2* __restrict__ tcv, const double2* __restrict__ Dc) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = min((int)threadIdx.x + 64 * kSpRowsWG * i, TOT - 1), s = m[i] & 0x3fffff;
      x[i] = *(s ? Dc + (s - 1) : tcv + q);
    }
  }
  // the meta words have arrived, and are not looked at before this point
  __device__ __forceinline__ void pin_meta() {
#pragma unroll
    for (int i = 0; i < IT; ++i) asm volatile("" : "+v"(m[i]));
  }
  // The same with no value registers (backward stage): the raw values land
  // in cv directly (asynchronous global -> LDS loads; the 64 entries of a
  // wave's load are contiguous) and what is left of each meta word waits in
  // ci (the row's byte offset, a multiple of 16, | 4 for a pairing entry |
  // op), so nothing is held in registers while the loads are in flight.
  // Once they have landed finish() applies it to the lane's own entries.
  __device__ __forceinline__ void dma_values(double2 (*cv)[kCrSpNZ][BP], unsigned short (*ci)[kCrSpNZ][BP],
                                             const double2* __restrict__ tcv, const double2* __restrict__ Dc) const {
    static_assert(TOT % 64 == 0, "a wave's entries are all inside the arrays or all outside");
    // (pin_meta() comes first: a wait for a meta word behind a load into LDS
    // in flight would wait for that load, and all before it, as well)
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = (int)threadIdx.x + 64 * kSpRowsWG * i, s = m[i] & 0x3fffff;
      const int q0 = __builtin_amdgcn_readfirstlane(((int)threadIdx.x & ~63) + 64 * kSpRowsWG * i);
      if (TOT % (64 * kSpRowsWG) != 0 && q0 >= TOT) continue;
      (&ci[0][0][0])[q] = (unsigned short)((((unsigned)m[i] >> 20) & 0xff0u) | (s ? 4u : 0u) | (((unsigned)m[i] >> 22) & 3u));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s ? Dc + (s - 1) : tcv + q),
                                       (__attribute__((address_space(3))) void*)(&cv[0][0][0] + q0), 16, 0, 0);
    }
  }
  __device__ __forceinline__ static void finish(double2 (*cv)[kCrSpNZ][BP], unsigned short (*ci)[kCrSpNZ][BP]) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = threadIdx.x + 64 * kSpRowsWG * i;
      if (q < TOT) {
        const unsigned k = (&ci[0][0][0])[q];
        // the meta word's Δ-index and op fields as sp_cval reads them
        (&cv[0][0][0])[q] = sp_cval((&cv[0][0][0])[q], (int)((k >> 2 & 1u) | (k & 3u) << 22));
        (&ci[0][0][0])[q] = (unsigned short)(k & 0xff0u);
      }
    }
  }
  __device__ __forceinline__ void store(double2 (*cv)[kCrSpNZ][BP], unsigned short (*ci)[kCrSpNZ][BP]) const {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = threadIdx.x + 64 * kSpRowsWG * i;
      if (q < TOT) {
        (&cv[0][0][0])[q] = sp_cval(x[i], m[i]);
        (&ci[0][0][0])[q] = (unsigned short)(((unsigned)m[i] >> 20) & 0xff0u);   // row * sizeof(double2)
      }
    }
  }
};

// forward: one wave per output row r of the kept row k's D', U', L'.  The
// record load is followed by the Δ load of the three pairing slots and every
// dense element load at once; the V rows meet in LDS.
template <int BP, int ST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kSpWavesF<BP>))) void k_cr_sp_fwd(
    double2* __restrict__ pool, int64_t item, const CrSpRowFwd* __restrict__ recs, const double2* __restrict__ tcv,
    const int* __restrict__ tcm, const double2* __restrict__ Delta, int twoN, int P) {
  constexpr int HP = BP / 2, NCL = (BP + 63) / 64, NRB = HP / kSpRowsWG;
  constexpr int TA = 3 * NZ * BP;   // per-task column array size
  __shared__ double2 cv[3][NZ][BP];
  __shared__ unsigned short ci[3][NZ][BP];
  __shared__ double2 sc[kSpRowsWG][3][BP];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int2 xy = xcd_grid2d();   // batch items grouped per XCD; x = task * NRB + row block
  const CrSpRowFwd t = recs[__builtin_amdgcn_readfirstlane(xy.x * kSpRowsWG + w)];
  ColStage<BP, 3> cs;
  cs.load_meta(tcm + (int64_t)(xy.x / NRB) * TA);
  const double2* Dc = Delta + (int64_t)(xy.y / P) * twoN;
  double2* base = pool + (int64_t)xy.y * item;
  unsigned cl[NCL];   // this lane's columns, as byte offsets within a row
#pragma unroll
  for (int j = 0; j < NCL; ++j) cl[j] = min(l + 64 * j, BP - 1) * (unsigned)sizeof(double2);
  // pairing entries of row r of -U_k, -L_er, -L_el: ∓Δ/2 (wave-uniform)
  double2 pw[3];
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    const double2 d = Dc[t.pd[o]];
    pw[o] = make_double2(sp_uniform(t.ps[o] * d.x), sp_uniform(t.ps[o] * d.y));
  }
  double2 dk[NCL], xh[3][NH][NCL], xp[3][NCL];
#pragma unroll
  for (int j = 0; j < NCL; ++j) {
    const BotCol<BP> bc(cl[j]);
    dk[j] = sp_ld(base, t.dk + cl[j]);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
#pragma unroll
      for (int e = 0; e < NH; ++e) xh[o][e][j] = sp_ld(base, t.ho[o][e] + cl[j]);
      xp[o][j] = bc.ld(base, t.po[o]);
    }
  }
  cs.load_values(tcv + (int64_t)(xy.x / NRB) * TA, Dc);
  // V1r = -U_k Dinv_er, V2r = -L_er Dinv_er, V2l = -L_el Dinv_el
#pragma unroll
  for (int j = 0; j < NCL; ++j) {
    const BotCol<BP> bc(cl[j]);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      double2 v = make_double2(0.0, 0.0);
#pragma unroll
      for (int e = 0; e < NH; ++e) rmac(v, t.hv[o][e], xh[o][e][j]);
      cmac(v, pw[o], bc.sign(xp[o][j]));
      if (l + 64 * j < BP) sp_st(sc[w][o], cl[j], v);
    }
  }
  cs.store(cv, ci);
  __syncthreads();
  // D'_k = D_k + V1r L_k + V2l U_el, U'_k = V1r U_er, L'_k = V2r L_k
#pragma unroll
  for (int j = 0; j < NCL; ++j) {
    const int c = cl[j] / sizeof(double2);
    double2 d = dk[j], u = make_double2(0.0, 0.0), lo = make_double2(0.0, 0.0);
#pragma unroll
    for (int e = 0; e < NZ; ++e) {
      const double2 vl = cv[0][e][c], vu = cv[1][e][c], vr = cv[2][e][c];
      const unsigned kl = ci[0][e][c], ku = ci[1][e][c], kr = ci[2][e][c];
      cmac(d, sp_ld(sc[w][0], kl), vl);
      cmac(lo, sp_ld(sc[w][1], kl), vl);
      cmac(d, sp_ld(sc[w][2], ku), vu);
      cmac(u, sp_ld(sc[w][0], kr), vr);
    }
    if (l + 64 * j < BP) {
      sp_st<ST>(base, t.od + cl[j], d);
      sp_st<ST>(base, t.ou + cl[j], u);
      sp_st<ST>(base, t.ol + cl[j], lo);
    }
  }
}

// backward: one wave per output row r of the eliminated row e's Z_a, Z_c,
// Y_a, Y_c and M = Y_a U_a + Y_c L_e (RPW rows in turn).  Row r of each G
// block is staged in the wave's LDS (Z gathers from it), full rows of the G
// blocks feed Y.
template <int BP, int RPW, int ST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kSpWavesB<BP>))) void k_cr_sp_bwd(
    double2* __restrict__ pool, int64_t item, const CrSpRowBwd* __restrict__ recs, const double2* __restrict__ tcv,
    const int* __restrict__ tcm, const double2* __restrict__ Delta, int twoN, int P) {
  constexpr int HP = BP / 2, NCL = (BP + 63) / 64, NRB = HP / (kSpRowsWG * RPW);
  constexpr int TA = 2 * NZ * BP;   // per-task column array size
  static_assert(HP % (kSpRowsWG * RPW) == 0, "row blocks tile the top half");
  __shared__ double2 cv[2][NZ][BP];
  __shared__ unsigned short ci[2][NZ][BP];
  __shared__ double2 gr[kSpRowsWG][4][BP];
  double2(*sc)[4][BP] = gr;   // the Y rows (sc[w][0 / 1]) reuse the wave's G rows once Z is formed
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int2 xy = xcd_grid2d();   // batch items grouped per XCD; x = task * NRB + row block
  ColStage<BP, 2> cs;
  cs.load_meta(tcm + (int64_t)(xy.x / NRB) * TA);
  const double2* Dc = Delta + (int64_t)(xy.y / P) * twoN;
  double2* base = pool + (int64_t)xy.y * item;
  unsigned cl[NCL];   // this lane's columns, as byte offsets within a row
#pragma unroll
  for (int j = 0; j < NCL; ++j) cl[j] = min(l + 64 * j, BP - 1) * (unsigned)sizeof(double2);
#pragma unroll 1
  for (int i = 0; i < RPW; ++i) {
    const CrSpRowBwd t = recs[__builtin_amdgcn_readfirstlane((xy.x * RPW + i) * kSpRowsWG + w)];
    // pairing entries of row r of L_a, U_e: Δ/2 (wave-uniform)
    double2 pw[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const double2 d = Dc[t.pd[o]];
      pw[o] = make_double2(sp_uniform(t.ps[o] * d.x), sp_uniform(t.ps[o] * d.y));
    }
    // What Z needs goes straight into LDS (asynchronous global -> LDS loads,
    // no registers, so the six-wave budget holds both operands' rows without
    // scratch): the column data and row r of the G blocks (lane l's 16 bytes
    // land at the row's base + 16 l, the row's own layout).  They go first:
    // the meta words, loaded alongside the record, are here when it is, and
    // their decode is out of the way before the rows fill the registers.
    // (The order is pinned: left to itself the compiler moves the decode
    // among the dense loads and sinks the Y sums below the barriers, which
    // keeps every loaded row live across them, and spills.)
    cs.pin_meta();
    if (i == 0) cs.dma_values(cv, ci, tcv + (int64_t)(xy.x / NRB) * TA, Dc);
#pragma unroll
    for (int j = 0; j < NCL; ++j)
      if (l + 64 * j < BP) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(base) + (t.g[g] + cl[j])),
              (__attribute__((address_space(3))) void*)&gr[w][g][64 * j], 16, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    // [operand L_a / U_e][G_aa, G_ac / G_ca, G_cc]
    double2 gh[2][2][NH][NCL], gp[2][2][NCL];
#pragma unroll
    for (int j = 0; j < NCL; ++j) {
      const BotCol<BP> bc(cl[j]);
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
#pragma unroll
          for (int e = 0; e < NH; ++e) gh[o][g][e][j] = sp_ld(base, t.ho[o][g][e] + cl[j]);
          gp[o][g][j] = bc.ld(base, t.po[o][g]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // Y_a[r, :] = L_a[r, :] G_aa + U_e[r, :] G_ca, Y_c[r, :] = L_a[r, :] G_ac + U_e[r, :] G_cc
    double2 yk[NCL][2];
#pragma unroll
    for (int j = 0; j < NCL; ++j) {
      const BotCol<BP> bc(cl[j]);
      double2 ya = make_double2(0.0, 0.0), yc = ya;
#pragma unroll
      for (int o = 0; o < 2; ++o) {
#pragma unroll
        for (int e = 0; e < NH; ++e) {
          rmac(ya, t.hv[o][e], gh[o][0][e][j]);
          rmac(yc, t.hv[o][e], gh[o][1][e][j]);
        }
        cmac(ya, pw[o], bc.sign(gp[o][0][j]));
        cmac(yc, pw[o], bc.sign(gp[o][1][j]));
      }
      yk[j][0] = ya;
      yk[j][1] = yc;
    }
#pragma unroll
    for (int j = 0; j < NCL; ++j)
      asm volatile("" : "+v"(yk[j][0].x), "+v"(yk[j][0].y), "+v"(yk[j][1].x), "+v"(yk[j][1].y));
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // every wave's loads into LDS have landed
    if (i == 0) {
      cs.finish(cv, ci);
      __syncthreads();
    }
    // Z_a[r, :] = G_aa[r, :] U_a + G_ac[r, :] L_e, Z_c[r, :] = G_ca[r, :] U_a + G_cc[r, :] L_e
#pragma unroll
    for (int j = 0; j < NCL; ++j) {
      const int c = cl[j] / sizeof(double2);
      double2 za = make_double2(0.0, 0.0), zc = za;
#pragma unroll
      for (int e = 0; e < NZ; ++e) {
        const double2 wa = cv[0][e][c], we = cv[1][e][c];
        const unsigned ka = ci[0][e][c], ke = ci[1][e][c];
        cmac(za, sp_ld(gr[w][0], ka), wa);
        cmac(zc, sp_ld(gr[w][1], ka), wa);
        cmac(za, sp_ld(gr[w][2], ke), we);
        cmac(zc, sp_ld(gr[w][3], ke), we);
      }
      if (l + 64 * j < BP) {
        sp_st<ST>(base, t.oya + cl[j], yk[j][0]);
        sp_st<ST>(base, t.oyc + cl[j], yk[j][1]);
        sp_st<ST>(base, t.oza + cl[j], za);
        sp_st<ST>(base, t.ozc + cl[j], zc);
      }
    }
    wave_sync();   // every lane's Z gathers from gr[w] are done
#pragma unroll
    for (int j = 0; j < NCL; ++j)
      if (l + 64 * j < BP) {
        sp_st(sc[w][0], cl[j], yk[j][0]);
        sp_st(sc[w][1], cl[j], yk[j][1]);
      }
    wave_sync();
    // M[r, :] = Y_a[r, :] U_a + Y_c[r, :] L_e
#pragma unroll
    for (int j = 0; j < NCL; ++j) {
      const int c = cl[j] / sizeof(double2);
      double2 mx = make_double2(0.0, 0.0);
#pragma unroll
      for (int e = 0; e < NZ; ++e) {
        cmac(mx, sp_ld(sc[w][0], ci[0][e][c]), cv[0][e][c]);
        cmac(mx, sp_ld(sc[w][1], ci[1][e][c]), cv[1][e][c]);
      }
      if (l + 64 * j < BP) sp_st<ST>(base, t.omx + cl[j], mx);
    }
    if (RPW > 1) wave_sync();   // the M gathers are done before the next row's G rows land
  }
}

}  // namespace

void launch_cr_sp_fwd(const CrDims& c, double2* pool, const CrSpRowFwd* recs, int n, const double2* tcv,
                      const int* tcm, const double2* Delta, hipStream_t s, int store) {
  if (n <= 0) return;
  const dim3 g(n * (c.BP / 2 / kSpRowsWG), c.nbatch), b(64 * kSpRowsWG);
  with_store(store, [&](auto st) {
    constexpr int ST = decltype(st)::value;
    switch (c.BP) {
      case 32: hipLaunchKernelGGL((k_cr_sp_fwd<32, ST>), g, b, 0, s, pool, c.item, recs, tcv, tcm, Delta, 2 * c.N, c.P); break;
      case 64: hipLaunchKernelGGL((k_cr_sp_fwd<64, ST>), g, b, 0, s, pool, c.item, recs, tcv, tcm, Delta, 2 * c.N, c.P); break;
      default: hipLaunchKernelGGL((k_cr_sp_fwd<96, ST>), g, b, 0, s, pool, c.item, recs, tcv, tcm, Delta, 2 * c.N, c.P); break;
    }
  });
}

void launch_cr_sp_bwd(const CrDims& c, double2* pool, const CrSpRowBwd* recs, int n, const double2* tcv,
                      const int* tcm, const double2* Delta, hipStream_t s, int store) {
  if (n <= 0) return;
  constexpr int RPW = SP_RPW_B;
  const dim3 g(n * (c.BP / 2 / (kSpRowsWG * RPW)), c.nbatch), b(64 * kSpRowsWG);
  with_store(store, [&](auto st) {
    constexpr int ST = decltype(st)::value;
    switch (c.BP) {
      case 32: hipLaunchKernelGGL((k_cr_sp_bwd<32, RPW, ST>), g, b, 0, s, pool, c.item, recs, tcv, tcm, Delta, 2 * c.N, c.P); break;
      case 64: hipLaunchKernelGGL((k_cr_sp_bwd<64, RPW, ST>), g, b, 0, s, pool, c.item, recs, tcv, tcm, Delta, 2 * c.N, c.P); break;
      default: hipLaunchKernelGGL((k_cr_sp_bwd<96, RPW, ST>), g, b, 0, s, pool, c.item, recs, tcv, tcm, Delta, 2 * c.N, c.P); break;
    }
  });
}

}  // namespace dwh
