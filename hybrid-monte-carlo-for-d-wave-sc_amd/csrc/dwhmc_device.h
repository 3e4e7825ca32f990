// Device helpers shared by the dense Gauss-Jordan (dwhmc_kernels.hip), the
// block cyclic-reduction (dwhmc_cr.hip) and the measurement kernels: complex
// arithmetic, the Fermi factors, the fixed-order block sum, the
// XCD-aware grid remap, wave reductions, the wave-local 16x16 complex
// inversion and the LDS-operand complex MFMA step (v_mfma_f64_16x16x4_f64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

// CDNA4 only: LDS footprints above 64 KiB per workgroup, f64 MFMA layouts of gfx950
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdwhmc device code targets gfx950 (MI355X) only"
#endif

namespace dwh {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// a * conj(b)
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) {
  return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cinv(double2 a) {
  const double s = 1.0 / (a.x * a.x + a.y * a.y);
  return make_double2(a.x * s, -a.y * s);
}
// Point k of a float range: start + step·k, the product and the sum rounded
// one after the other, as the host forms the grids it returns
// (dwh_spectral_window, the bindings' omega arrays).  The pragma matters: HIP's
// __dmul_rn / __dadd_rn are plain operators, which the device default
// (-ffp-contract=fast) fuses into one fma — an ulp away on about half the
// points, and a Lorentzian of width η turns an ulp of ω into ulp/η.
__device__ __forceinline__ double grid_point(double start, double step, int64_t k) {
#pragma clang fp contract(off)
  const double p = step * (double)k;
  return start + p;
}

// f_n - f_m of the Fermi factors f = logistic(-βE), g = 1 - f = logistic(+βE)
// (each from its own exponential), dE = E_m - E_n, without the cancellation of
// the plain difference: f_n - f_m = f_n g_m (1 - e^{-β dE}) exactly, taken from
// the side on which the exponential decays.  A few ulp at any gap; the plain
// difference loses eps / |f_n - f_m| (8e-10 of the l = 0 quotient at
// dE = 2e-8).
__device__ __forceinline__ double fermi_diff(double dE, double fn, double gn, double fm, double gm, double beta) {
  const double x = beta * dE;
  return x >= 0 ? -(fn * gm) * expm1(-x) : (fm * gn) * expm1(x);
}
// LogExpFunctions.logistic, overflow-safe (the Fermi factor f_n = logistic(-β E_n))
__device__ inline double logistic_d(double x) {
  if (x >= 0) return 1.0 / (1.0 + exp(-x));
  const double e = exp(x);
  return e / (1.0 + e);
}
// 1/p with v_rcp_f64 + one Newton step (<= ~11 ulp): the reciprocal of the
// Lorentzian sums (k_tr_sigma, k_op_spec, k_nb_spec), a few ulp of the sum of
// the terms' absolute values
__device__ inline double rcp_nr1(double p) {
  const double r = __builtin_amdgcn_rcp(p);
  return fma(r, fma(-p, r, 1.0), r);
}
// fixed-order tree sum of NV values per thread over a block of TB threads (a
// power of two); result in sh[v][0]
template <int NV, int TB>
__device__ inline void block_sum(double (&v)[NV], double (*sh)[TB]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) sh[k][tid] = v[k];
  __syncthreads();
  for (int s = TB / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < NV; ++k) sh[k][tid] += sh[k][tid + s];
    }
    __syncthreads();
  }
}
// 1/a with v_rcp_f64 + two Newton steps (error ~1 ulp; the IEEE division
// sequence has ~3x the latency and sits on the pivot dependency chain).
__device__ __forceinline__ double rcp_nr(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  r = fma(r, fma(-d, r, 1.0), r);
  return r;
}
__device__ __forceinline__ double2 cinv_fast(double2 a) {
  const double s = rcp_nr(fma(a.x, a.x, a.y * a.y));
  return make_double2(a.x * s, -a.y * s);
}

// One 16-byte store of a CR pool element with a cache policy (the values of
// dwh::kStore*, dwhmc_internal.h; a compile-time parameter of each kernel
// instantiation, chosen per stage by the plan).  The value stored is the same
// under every policy; only where the line lives afterwards differs:
//   plain    global_store_dwordx4: the line stays dirty in this XCD's L2 and
//            is written back at the end of the launch (the release every
//            dependent launch ends with);
//   through  written through while the kernel runs, the L2 drops the line: one
//            16-byte buffer store with sc1 where the site has a wave-uniform
//            base (st16_through below: every site the plan writes through);
//            this pointer form issues two relaxed agent-scope 8-byte stores
//            (global_store_dwordx2 sc1);
//   stream   non-temporal (global_store_dwordx4 nt): the line is marked for
//            early eviction but stays in the L2.
template <int POL>
__device__ __forceinline__ void st16(double2* p, double2 v) {
  if constexpr (POL == 1) {
    double* q = reinterpret_cast<double*>(p);
    __hip_atomic_store(q, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if constexpr (POL == 2) {
    typedef double v2d __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(v2d{v.x, v.y}, reinterpret_cast<v2d*>(p));
  } else {
    static_assert(POL == 0, "store policy: 0 plain, 1 write-through, 2 non-temporal");
    *p = v;
  }
}

// The (base, offset) form of the write-through store, used where the plan
// picks write-through (the K-split product epilogues and the side products):
// ONE 16-byte buffer store with sc1 (buffer_store_dwordx4 ... sc1), which
// costs the writer what a plain store does and leaves a same-XCD reader most
// of its L2 hits (tools/micro/boundary_dirty.hip, THROUGH16).  base: the batch
// item's first pool element, wave-uniform (the resource descriptor lives in
// SGPRs); soff / voff: the uniform and the per-lane part of the element
// offset within the item, whose byte offsets fit 32 bits (plan_cr refuses a
// lattice whose batch item reaches 2^32 bytes; none dwh_create takes does).
// In the built code the descriptor and soff are SGPRs at every site
// (buffer_store_dwordx4 v[..], v, s[..:..], s.. offen sc1, no waterfall loop):
// the bases come from a scalar slot load (k_cr_gemm16) or a readfirstlane'd
// tile index (cr_gemm_wg).  The pointer form above keeps the two
// halves: the sites that use it have no uniform base, and the plan stores
// plain there.  -DDWH_ST16_THROUGH_HALVES: the two halves here too (A/B
// libraries only).
__device__ __forceinline__ void st16_through(double2* base, uint32_t soff, uint32_t voff, double2 v) {
#ifdef DWH_ST16_THROUGH_HALVES
  st16<1>(base + soff + voff, v);
#else
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  // raw buffer over the item: stride 0, no record limit (the plan bounds the
  // offsets), descriptor word 3 = DATA_FORMAT 32-bit (bits 15-18 = 4; an
  // untyped store ignores the format); cache policy bit 4 of the builtin's aux
  // operand = sc1 (bit 0 sc0, bit 1 nt)
  constexpr int kRsrcNoLimit = -1, kRsrcWord3Raw32 = 0x00020000, kAuxSc1 = 16;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, kRsrcNoLimit, kRsrcWord3Raw32);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)(voff * 16u), (int)(soff * 16u), kAuxSc1);
#endif
}

// Bijective XCD-aware remap of a 1D grid (cdna_hip_programming.md §5): blocks
// b and b+8 share an XCD, so item ranges [x*q, (x+1)*q) are given to one XCD
// and neighbouring rows of one matrix share that XCD's L2.  Speed only.
// Host twin: xcd_remap_host (dwhmc_plan.cpp), which orders the product slots.
__device__ __forceinline__ int xcd_remap(int orig, int total) {
  const int q = total / 8, r = total % 8, xcd = orig % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}

// The same grouping for a 2D grid (x: work within a batch item, y: batch
// item): this workgroup's (x, y) after remapping its linear index, so a
// batch item's workgroups share an XCD (and the XCD the block-product stages
// give it, up to rounding), and the blocks one stage writes are read by the
// next through that XCD's L2.  -DCR_XCD_ITEMS=0: hardware order (A/B).
#ifndef CR_XCD_ITEMS
#define CR_XCD_ITEMS 1
#endif
__device__ __forceinline__ int2 xcd_grid2d() {
#if CR_XCD_ITEMS
  const int nx = gridDim.x, g = xcd_remap(blockIdx.x + nx * blockIdx.y, nx * gridDim.y);
  return make_int2(g % nx, g / nx);
#else
  return make_int2(blockIdx.x, blockIdx.y);
#endif
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// fixed-order sum over a block of 256 threads: wave sums, then the 4 partials
// in order (red: 4 doubles of LDS); every thread gets the result
__device__ __forceinline__ double block_sum256(double v, double* red) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  v = wave_sum(v);
  if (l == 0) red[w] = v;
  __syncthreads();
  const double t = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return t;
}

// 16x16 complex block in one wave: lane l holds row l>>2, columns (l&3)*4..+3.
// Row p and column p are exchanged through a per-wave LDS scratch (xb: 16
// row + 16 column entries) between wavefront-scope fences; the update is
// branch-free (selects instead of a divergent row-p path).  pm receives
// |pivot|^2 (lane 0) when non-null.
__device__ __forceinline__ void wave_inv16(double2 (&a)[4], double2* xb, double* pm, int pbase) {
  const int l = threadIdx.x & 63;
  const int r = l >> 2, cq = l & 3;
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    const int ps = p >> 2, pe = p & 3;
    const bool prow = (r == p);
    if (prow) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) xb[cq * 4 + jj] = a[jj];
    }
    if (cq == ps) xb[16 + r] = a[pe];
    // cross-lane hand-off: the fences are compiler ordering points (a plain
    // predicated store/load pair may legally be reordered for other lanes)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double2 piv = xb[p];
    const double2 colp = xb[16 + r];
    double2 rowp[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) rowp[jj] = xb[cq * 4 + jj];
    const double2 inv = cinv_fast(piv);
    if (pm != nullptr && l == 0) pm[pbase + p] = piv.x * piv.x + piv.y * piv.y;
    // row p: a <- rowp * inv ; other rows: a <- a - (colp*inv) * rowp
    const double2 fi = cmul(colp, inv);
    const double2 g = prow ? make_double2(-inv.x, -inv.y) : fi;
    const double2 pc = prow ? inv : make_double2(-fi.x, -fi.y);   // new value in column p
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const double2 base = prow ? make_double2(0.0, 0.0) : a[jj];
      const double2 v = csub(base, cmul(g, rowp[jj]));
      a[jj] = (cq * 4 + jj == p) ? pc : v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// acc(16x16, C layout) += sgn * Aop(16 x 16, k) * Bop(16 x 16), complex, 4 MFMA per k-step.
// Aop(m, k) = A[(m) * lda + k], Bop(k, n) = B[k * ldb + n]  (LDS pointers)
template <bool NEG>
__device__ __forceinline__ void mma16_lds(d4& acr, d4& aci, const double2* A, int lda,
                                          const double2* B, int ldb) {
  const int l = threadIdx.x & 63;
  const int lr = l & 15, lk = l >> 4;
#pragma unroll
  for (int ks = 0; ks < 16; ks += 4) {
    const double2 av = A[lr * lda + ks + lk];
    const double2 bv = B[(ks + lk) * ldb + lr];
    const double ar = NEG ? -av.x : av.x, ai = NEG ? -av.y : av.y;
    acr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bv.x, acr, 0, 0, 0);
    aci = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bv.y, aci, 0, 0, 0);
    acr = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bv.y, acr, 0, 0, 0);
    aci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bv.x, aci, 0, 0, 0);
  }
}

// kick π += kick·F, then (drift != 0) the next leapfrog step's drift
// Δ += drift·π with the |Δ| guard (src/HMC.jl:101 fused with :111-113)
__device__ __forceinline__ void kick_drift(double2 Fv, int64_t o, double2* __restrict__ Delta,
                                           double2* __restrict__ Pi, double kick, double drift,
                                           double cap2, int* __restrict__ flag) {
  if (kick == 0.0 && drift == 0.0) return;
  double2 p = Pi[o];
  p.x += kick * Fv.x;
  p.y += kick * Fv.y;
  Pi[o] = p;
  if (drift != 0.0) {
    double2 d = Delta[o];
    d.x += drift * p.x;
    d.y += drift * p.y;
    Delta[o] = d;
    if (d.x * d.x + d.y * d.y > cap2) atomicOr(flag, 1);
  }
}

// kick_drift with Pi[o] and Delta[o] already loaded (p, d): the caller issues
// those loads before its own long-latency work; returns the drifted Δ
__device__ __forceinline__ double2 kick_drift_pre(double2 Fv, int64_t o, double2 p, double2 d,
                                                  double2* __restrict__ Delta, double2* __restrict__ Pi,
                                                  double kick, double drift, double cap2, int* __restrict__ flag) {
  if (kick == 0.0 && drift == 0.0) return d;
  p.x += kick * Fv.x;
  p.y += kick * Fv.y;
  Pi[o] = p;
  if (drift != 0.0) {
    d.x += drift * p.x;
    d.y += drift * p.y;
    Delta[o] = d;
    if (d.x * d.x + d.y * d.y > cap2) atomicOr(flag, 1);
  }
  return d;
}

// ---------------------------------------------------------------------------
// Register-only 16x16 complex no-pivot Gauss-Jordan inversion in one wave.
// Layout: lane l holds row r = l & 15, columns 4q .. 4q+3 with q = l >> 4.
// Pivot p (compile time): row p reaches every lane of its 16-lane row through
// DPP row_newbcast:p, column p reaches the other column quarters through
// ds_bpermute (LDS crossbar, no LDS storage), the pivot value through
// readlane.  No barriers.  pprod accumulates Π |pivot|^2 (uniform in the wave).
// ---------------------------------------------------------------------------
template <int P>
__device__ __forceinline__ double dpp_rowbcast(double x) {
  // full row/bank masks + bound_ctrl: every lane is written, the old value is dead
  return __builtin_amdgcn_update_dpp(x, x, 0x150 + P, 0xf, 0xf, true);
}

// value of quarter QS (lanes 16 QS .. 16 QS + 15) broadcast to all quarters, per row position
template <int QS>
__device__ __forceinline__ double bcast_quarter(double x) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  // one LDS-crossbar permute per dword (no LDS storage): lane l reads lane
  // 16 QS + (l & 15); 2 instructions per double instead of ~6 with the
  // v_permlane16/32_swap pair and their register copies (the inversion is
  // issue-bound)
  const int src = ((QS << 4) | (threadIdx.x & 15)) << 2;
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)(unsigned)(b >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double readlane_f64(double x, int lane) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// STRIDED: lane l holds columns q, q + 4, q + 8, q + 12 (q = l >> 4) instead
// of 4q .. 4q + 3 — the MFMA C layout of the transposed tile, so a tile kept
// transposed in MFMA registers is inverted in place without an LDS transpose.
// chi: the high dword of c (wave-uniform, a power of two, so its low dword is
// zero; 1 for ordinary tiles), the constant of the select-free form below; the
// pivoted row and column come out scaled by c (wave_inv16_dpp).
template <int P, bool STRIDED = false>
__device__ __forceinline__ void inv16_step(double2 (&a)[4], double& pprod, unsigned chi) {
  constexpr int PS = STRIDED ? (P & 3) : (P >> 2), PE = STRIDED ? (P >> 2) : (P & 3);
  const int l = threadIdx.x & 63, r = l & 15, q = l >> 4;
  double2 rowp[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) rowp[jj] = make_double2(dpp_rowbcast<P>(a[jj].x), dpp_rowbcast<P>(a[jj].y));
  const double2 colp = make_double2(bcast_quarter<PS>(a[PE].x), bcast_quarter<PS>(a[PE].y));
  // the pivot straight from its owner lane, off the column broadcast's chain
  const double2 piv = make_double2(readlane_f64(a[PE].x, PS * 16 + P), readlane_f64(a[PE].y, PS * 16 + P));
  const double m2 = fma(piv.x, piv.x, piv.y * piv.y);
  const double s = rcp_nr(m2);
  const double2 inv = make_double2(piv.x * s, -piv.y * s);
  pprod *= m2;
  const bool prow = (r == P);
  // Select-free form: one update a <- a - f rowp' for every entry.  On the
  // pivot row colp' = piv - c, so f = (piv - c)/piv = 1 - c/piv and the row
  // becomes c a_p / piv; in column p rowp' = piv + c, so the column becomes
  // colp - f (piv + c) = -c colp/piv (c^2/piv on the pivot row) up to one
  // rounding of colp - f piv.  Replaces ~12 per-lane selects by two adds.
  // (c or 0 selected on the high dword alone: one v_cndmask, as with a literal 1.0)
  const double cr = __builtin_bit_cast(double, (unsigned long long)(prow ? chi : 0u) << 32);
  const double cc = __builtin_bit_cast(double, (unsigned long long)((q == PS) ? chi : 0u) << 32);
  const double2 fi = cmul(make_double2(colp.x - cr, colp.y), inv);
  rowp[PE].x += cc;
  const double2 f = fi;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const double2 x = rowp[jj];
    double2 v;
    v.x = fma(-f.x, x.x, fma(f.y, x.y, a[jj].x));
    v.y = fma(-f.x, x.y, fma(-f.y, x.x, a[jj].y));
    a[jj] = v;
  }
}

template <bool STRIDED, int... Ps>
__device__ __forceinline__ void inv16_all(double2 (&a)[4], double& pprod, unsigned chi,
                                          std::integer_sequence<int, Ps...>) {
  (inv16_step<Ps, STRIDED>(a, pprod, chi), ...);
}

// returns Π |pivot|^2 of the 16 pivots
//
// With c = 1 the select-free pivot step forms the pivot row a_p / piv as
// a_p - (1 - 1/piv) a_p (and 1/piv itself as piv - (1 - 1/piv)(piv + 1)): for
// |piv| >> 1 that difference cancels and leaves an absolute error eps |piv|
// in entries of size 1/|piv| — eps |piv|^2 relative, 3.5 digits at the top
// poles (|piv| ~ y ~ 60; tests/test_cr_kernels.py).  With c of the pivots'
// size nothing cancels: every pivoted row and column carries a factor c, the
// not yet pivoted part (and so every pivot) is what it was, and the 16 steps
// leave c^2 A^-1.  So a tile whose first pivot is large (|a_00| >= 4) runs
// with c = 2^e <= |a_00| < 2 c (the diagonal of H - i y and of its Schur
// complements is of one size) and is scaled back by the exact c^-2; every
// other tile runs with c = 1: the same steps as before, bit for bit.  c is
// derived beside the first reciprocal, off the pivot chain.
template <bool STRIDED = false>
__device__ __forceinline__ double wave_inv16_dpp(double2 (&a)[4]) {
  const double p0x = readlane_f64(a[0].x, 0), p0y = readlane_f64(a[0].y, 0);
  const int ex = __builtin_amdgcn_frexp_exp(fma(p0x, p0x, p0y * p0y));   // |a_00|^2 in [2^(ex-1), 2^ex)
  const int e = ex >= 5 ? (ex - 1) >> 1 : 0;                              // wave-uniform
  double pprod = 1.0;
  inv16_all<STRIDED>(a, pprod, (unsigned)(1023 + e) << 20, std::make_integer_sequence<int, 16>{});
  if (e != 0) {
    const double s2 = __builtin_ldexp(1.0, -2 * e);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) a[jj] = make_double2(a[jj].x * s2, a[jj].y * s2);
  }
  return pprod;
}

// In-place inverse of a 16 x 16 tile held in the MFMA C layout (lane: rows
// lk + 4 rr, column lr).  Those registers are the strided layout of the
// transposed tile, and inverting M^T in that layout leaves (M^T)^-1 =
// (M^-1)^T strided, i.e. M^-1 in the C layout.  Returns Π |pivot|^2.
__device__ __forceinline__ double wave_inv16_c(d4& cr, d4& ci) {
  double2 dv[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) dv[jj] = make_double2(cr[jj], ci[jj]);
  const double p = wave_inv16_dpp<true>(dv);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    cr[jj] = dv[jj].x;
    ci[jj] = dv[jj].y;
  }
  return p;
}

}  // namespace dwh
