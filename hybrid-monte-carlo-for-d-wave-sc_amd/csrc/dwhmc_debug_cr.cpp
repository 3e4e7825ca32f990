// Test entries of the block cyclic-reduction path (include/dwhmc.h):
// dwh_debug_cr_launch runs ONE launch of the library's own CR launchers
// (launch_cr_inv / _inv0 / _gemm / _inv_side, dwhmc_cr.hip) on a pool the
// caller supplies, and dwh_debug_cr_resolvent reads back, for one (chain,
// pole), exactly the pool entries the force and E_f gathers read.  Neither is
// on the step path; both allocate and free their own scratch and synchronise.
// Every index and size of a launch is validated on the host before the device
// is touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "dwhmc_ctx.h"

using namespace dwh;

namespace {

// device buffers of one test launch, freed on every return path
struct Scratch {
  std::vector<void*> p;
  ~Scratch() {
    for (void* q : p) (void)hipFree(q);
  }
  template <typename T>
  hipError_t up(T** d, const T* h, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    p.push_back(q);
    *d = static_cast<T*>(q);
    return n ? hipMemcpy(q, h, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
};

int bad(const std::string& msg) { return fail(nullptr, DWH_ERR_ARG, "dwh_debug_cr_launch: " + msg); }

// the inversion lists of a launch: indices in range, destinations and slots
// distinct, no destination is another entry's source
int check_inv_lists(int nblk, int nslots, int n, const int32_t* blk, const int32_t* dst, const int32_t* slot) {
  if (n < 1 || n > nblk) return bad("inversion count out of range");
  if (!blk || !dst || !slot) return bad("NULL inversion list");
  std::set<int> ds, ss;
  for (int i = 0; i < n; ++i) {
    if (blk[i] < 0 || blk[i] >= nblk || dst[i] < 0 || dst[i] >= nblk) return bad("inversion block id out of range");
    if (slot[i] < 0 || slot[i] >= nslots) return bad("ln|det| slot out of range");
    if (!ds.insert(dst[i]).second) return bad("two inversions write one block");
    if (!ss.insert(slot[i]).second) return bad("two inversions write one ln|det| slot");
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (i != j && dst[i] == blk[j]) return bad("an inversion writes another inversion's source");
  return DWH_OK;
}

// the product tasks of a launch (16 int32 each, CrTask's field order) into
// *out: indices and windows in range; no task writes a block any task of the
// launch reads (its own accumulate input excepted) or another task writes
int check_tasks(int nblk, int BP, int ntasks, const int32_t* tasks, bool side, std::vector<CrTask>* out) {
  const int HP = BP / 2;
  if (ntasks < 1 || ntasks > 64) return bad("task count out of range (1..64)");
  if (!tasks) return bad("NULL task list");
  out->resize(ntasks);
  static_assert(sizeof(CrTask) == 16 * sizeof(int32_t), "a task is 16 int32");
  std::memcpy(out->data(), tasks, (size_t)ntasks * sizeof(CrTask));
  std::set<int> outs;
  for (const CrTask& t : *out) {
    if (t.out < 0 || t.out >= nblk) return bad("task output block out of range");
    if (t.cin < -1 || t.cin >= nblk) return bad("task accumulate block out of range");
    if (t.nt < 1 || t.nt > 4) return bad("task term count out of range (1..4)");
    if (t.bq & ~(0xf | (side ? kCrNegBit : 0))) return bad("task form bits out of range");
    for (int h = 0; h < t.nt; ++h)
      if (t.a[h] < 0 || t.a[h] >= nblk || t.b[h] < 0 || t.b[h] >= nblk) return bad("task operand block out of range");
    if (t.r0 < 0 || t.r0 >= t.r1 || t.r1 > HP || t.c0 < 0 || t.c0 >= t.c1 || t.c1 > BP)
      return bad("task window outside the HP x BP top half");
    if (!outs.insert(t.out).second) return bad("two tasks write one block");
  }
  for (const CrTask& t : *out) {
    for (int h = 0; h < t.nt; ++h)
      if (outs.count(t.a[h]) || outs.count(t.b[h])) return bad("a task reads a block the launch writes");
    if (t.cin >= 0 && t.cin != t.out && outs.count(t.cin)) return bad("a task accumulates a block another task writes");
  }
  return DWH_OK;
}

}  // namespace

extern "C" {

int dwh_debug_cr_launch(int32_t device, int32_t kind, int32_t BP, int32_t nblk, int32_t nbatch, int32_t nslots,
                        dwh_c128* pool, double* ldpart, int32_t ninv, const int32_t* blk, const int32_t* rblk,
                        const int32_t* dst, const int32_t* slot, int32_t inv32, int32_t ntasks,
                        const int32_t* tasks, int32_t ts, int32_t ksplit, double sg) {
  // ---- host-side validation: nothing below it can index outside the pool ----
  if (!pool || !ldpart) return bad("NULL pool or ldpart");
  if (!cr_supported_bp(BP)) return bad("unsupported block size (BP must be 32, 64, 96 or 128)");
  if (nblk < 1 || nblk > 4096 || nbatch < 1 || nbatch > 4096 || nslots < 1 || nslots > 4096)
    return bad("nblk, nbatch, nslots must be in 1..4096");
  const int HP = BP / 2;
  const int64_t BB = (int64_t)HP * BP;
  const bool inv = kind == DWH_CR_INV || kind == DWH_CR_INV0 || kind == DWH_CR_INV_SIDE;
  const bool prod = kind == DWH_CR_GEMM || kind == DWH_CR_INV_SIDE;
  if (!inv && !prod) return bad("unknown launch kind");
  // inv0 keeps its [A | 0] source blocks behind the caller's nblk blocks
  const int nextra = kind == DWH_CR_INV0 ? std::max(ninv, 0) : 0;
  if ((int64_t)(nblk + nextra) * BB * nbatch > ((int64_t)1 << 25)) return bad("pool larger than 2^25 elements");
  std::vector<CrTask> tk;
  if (inv)
    if (int rc = check_inv_lists(nblk, nslots, ninv, blk, dst, slot)) return rc;
  if (kind == DWH_CR_INV0) {
    if (!cr_supported_inv0(BP)) return bad("level-0 inversions from static R blocks: BP 32, 64, 96 only");
    if (!rblk) return bad("NULL R block list");
    std::set<int> rs;
    for (int i = 0; i < ninv; ++i) {
      if (rblk[i] < 0 || rblk[i] >= nblk) return bad("R block id out of range");
      if (!rs.insert(rblk[i]).second) return bad("two inversions share an R block");
    }
    for (int i = 0; i < ninv; ++i)
      for (int j = 0; j < ninv; ++j) {
        if (rs.count(blk[j]) || rs.count(dst[j])) return bad("an R block is an inversion's source or destination");
        if (dst[i] == blk[j]) return bad("level-0 inversions run out of place");
      }
  }
  if (prod) {
    if (kind == DWH_CR_INV_SIDE && !cr_supported_side(BP)) return bad("side work: BP 64 only");
    if (int rc = check_tasks(nblk, BP, ntasks, tasks, kind == DWH_CR_INV_SIDE, &tk)) return rc;
  }
  if (kind == DWH_CR_GEMM) {
    if (ts != 16 && ts != 32) return bad("tile size must be 16 or 32");
    if (ksplit != 1 && ksplit != 2 && ksplit != 4) return bad("K split must be 1, 2 or 4");
    if (ts == 32 && HP % 32 != 0) return bad("32 x 32 tiles need HP % 32 == 0 (BP 64, 128)");
    if (ts == 32 && ksplit == 4) return bad("K split 4 runs 16 x 16 tiles only");
    if (sg != 1.0 && sg != -1.0) return bad("stage sign must be +1 or -1");
  }
  if (kind == DWH_CR_INV_SIDE) {
    // side tasks run beside the inversions: they neither write a block an
    // inversion touches nor read one an inversion writes
    std::set<int> src(blk, blk + ninv), dd(dst, dst + ninv);
    for (const CrTask& t : tk) {
      if (src.count(t.out) || dd.count(t.out)) return bad("a side task writes an inversion's block");
      if (t.cin >= 0 && dd.count(t.cin)) return bad("a side task reads an inversion's destination");
      for (int h = 0; h < t.nt; ++h)
        if (dd.count(t.a[h]) || dd.count(t.b[h])) return bad("a side task reads an inversion's destination");
    }
  }

  CrDims c{};
  c.Lx = HP;
  c.Ly = nslots;   // the launchers' ln|det| row length
  c.N = HP * nslots;
  c.BP = BP;
  c.P = 1;
  c.nbatch = nbatch;
  c.nblk = nblk + nextra;
  c.item = (int64_t)c.nblk * BB;
  c.inv32 = inv32 != 0;

  // product stage: the planner's own tile expansion and slot order
  int maxt32 = 0, maxt16 = 0, nswg = 0;
  std::vector<CrSlot> slots;
  const CrGemmCfg cfg{ts, ksplit};
  if (prod)
    for (const CrTask& t : tk) {
      maxt32 = std::max(maxt32, cr_task_tiles(t, 32));
      maxt16 = std::max(maxt16, cr_task_tiles(t, 16));
    }
  if (kind == DWH_CR_GEMM && ts == 16) {
    std::vector<CrTile> tiles;
    for (const CrTask& t : tk) cr_task_tiles16(t, BP / 16, nullptr, &tiles);
    nswg = cr_gemm_slot_wgs(c, (int)tiles.size(), cfg);
    slots.resize((size_t)nswg * (4 / ksplit));
    cr_gemm_slots(c, tiles.data(), (int)tiles.size(), cfg, slots.data());
  }

  // ---- device ----
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, DWH_ERR_HIP, "hipSetDevice failed");
  const size_t user_item = (size_t)nblk * BB;
  std::vector<double2> hp((size_t)c.item * nbatch, make_double2(0.0, 0.0));
  std::vector<int32_t> tmp(nextra);
  for (int bi = 0; bi < nbatch; ++bi) {
    double2* it = hp.data() + (size_t)bi * c.item;
    std::memcpy(it, pool + (size_t)bi * user_item, user_item * sizeof(double2));
    for (int i = 0; i < nextra; ++i) {   // [A | 0] of blk[i]
      tmp[i] = nblk + i;
      for (int r = 0; r < HP; ++r)
        std::memcpy(it + (size_t)(nblk + i) * BB + (size_t)r * BP, it + (size_t)blk[i] * BB + (size_t)r * BP,
                    HP * sizeof(double2));
    }
  }
  Scratch sc;
  double2* dpool = nullptr;
  double *dld = nullptr, *dldA = nullptr;
  int32_t *dblk = nullptr, *drblk = nullptr, *ddst = nullptr, *dslot = nullptr, *dtmp = nullptr;
  CrTask* dtasks = nullptr;
  CrSlot* dslots = nullptr;
  const size_t nld = (size_t)nbatch * nslots;
  const std::vector<double> zero(nld, 0.0);
  hipError_t e = sc.up(&dpool, hp.data(), hp.size());
  if (e == hipSuccess) e = sc.up(&dld, ldpart, nld);
  if (e == hipSuccess && inv) {
    e = sc.up(&dblk, blk, (size_t)ninv);
    if (e == hipSuccess) e = sc.up(&ddst, dst, (size_t)ninv);
    if (e == hipSuccess) e = sc.up(&dslot, slot, (size_t)ninv);
  }
  if (e == hipSuccess && kind == DWH_CR_INV0) {
    e = sc.up(&drblk, rblk, (size_t)ninv);
    if (e == hipSuccess) e = sc.up(&dtmp, tmp.data(), tmp.size());
    if (e == hipSuccess) e = sc.up(&dldA, zero.data(), nld);
  }
  if (e == hipSuccess && prod) e = sc.up(&dtasks, tk.data(), tk.size());
  if (e == hipSuccess && !slots.empty()) e = sc.up(&dslots, slots.data(), slots.size());
  if (e != hipSuccess) return fail(nullptr, DWH_ERR_HIP, std::string("cr test buffers: ") + hipGetErrorString(e));
  // DWHMC_DEBUG_CR_STORE=1: the product tiles of a K-split 16 x 16 launch and
  // the side products are written through, as the plan has them on the step
  // path (the default here: plain everywhere)
  const char* se = std::getenv("DWHMC_DEBUG_CR_STORE");
  const int through = se && *se == '1' ? kStoreThrough : kStorePlain;
  switch (kind) {
    case DWH_CR_INV:
      launch_cr_inv(c, dpool, dblk, ddst, dslot, ninv, dld, nullptr);
      break;
    case DWH_CR_INV0:
      // the static R = A^-1 blocks and ldA = 2 ln|det A| as context creation
      // forms them: the [A | 0] blocks inverted out of place
      launch_cr_inv(c, dpool, dtmp, drblk, dslot, ninv, dldA, nullptr);
      launch_cr_inv0(c, dpool, dblk, drblk, ddst, dslot, ninv, dld, dldA, nullptr);
      break;
    case DWH_CR_GEMM:
      launch_cr_gemm(c, dpool, dtasks, ntasks, maxt32, maxt16, dslots, nswg, cfg, sg, nullptr,
                     ts == 16 && ksplit > 1 ? through : kStorePlain);
      break;
    default:
      launch_cr_inv_side(c, dpool, dblk, ddst, dslot, ninv, dld, dtasks, ntasks, maxt32, nullptr, SiteGuard{},
                         kStorePlain, through);
      break;
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(hp.data(), dpool, hp.size() * sizeof(double2), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ldpart, dld, nld * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, DWH_ERR_HIP, std::string("cr test launch: ") + hipGetErrorString(e));
  for (int bi = 0; bi < nbatch; ++bi)
    std::memcpy(pool + (size_t)bi * user_item, hp.data() + (size_t)bi * c.item, user_item * sizeof(double2));
  return DWH_OK;
}

int dwh_debug_cr_resolvent(dwh_ctx* ctx, int64_t chain, int64_t pole, dwh_c128* G12, int32_t* cols, dwh_c128* diag,
                           double* lndet, double* y, double* cq) {
  if (!ctx || !G12 || !diag || !lndet) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  if (ctx->algo != ALGO_CR) return fail(ctx, DWH_ERR_STATE, "the resolvent read-back exists only on the CR path");
  if (!ctx->factorized) return fail(ctx, DWH_ERR_STATE, "no factorisation yet");
  const CrDims& c = ctx->cr;
  if (chain < 0 || chain >= ctx->d.nc || pole < 0 || pole >= c.P)
    return fail(ctx, DWH_ERR_ARG, "chain or pole index out of range");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  SETTLE(ctx);
  const int64_t bi = chain * c.P + pole;
  std::vector<double2> item((size_t)c.item);
  std::vector<double> ld((size_t)c.Ly);
  HIPCHECK(ctx, hipMemcpyAsync(item.data(), ctx->bpool + bi * c.item, item.size() * sizeof(double2),
                               hipMemcpyDeviceToHost, ctx->stream));
  HIPCHECK(ctx, hipMemcpyAsync(ld.data(), ctx->ldpart + bi * c.Ly, ld.size() * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  const CrPlan& pl = ctx->plan;
  const std::vector<int>& Dcol = ctx->model->Dcol;
  for (size_t k = 0; k < (size_t)c.N * kSlots; ++k) {
    const int64_t o = pl.goff[k];
    G12[k] = o >= 0 ? dwh_c128{item[o].x, item[o].y} : dwh_c128{0.0, 0.0};
    if (cols) cols[k] = Dcol[k];
  }
  for (int i = 0; i < c.N; ++i) diag[i] = dwh_c128{item[pl.doff[i]].x, item[pl.doff[i]].y};
  double s = 0.0;
  for (double v : ld) s += v;
  *lndet = s;
  if (y) std::copy(ctx->poles.y.begin(), ctx->poles.y.end(), y);
  if (cq) std::copy(ctx->poles.cq.begin(), ctx->poles.cq.end(), cq);
  return DWH_OK;
}

}  // extern "C"
