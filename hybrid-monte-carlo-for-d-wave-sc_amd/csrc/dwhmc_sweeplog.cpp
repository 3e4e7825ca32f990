// Host side of the sweep log (include/dwhmc.h, dwh_sweep_log): the layout
// arithmetic, the log's buffers, the launches a logged throughput sweep adds
// (kernels: dwhmc_sweeplog.hip) and the readers.
#include <string>

#include "dwhmc_ctx.h"

using namespace dwh;

namespace {

constexpr int32_t kLogMask = DWH_LOG_OBS | DWH_LOG_FIELD_SQ | DWH_LOG_SNAPSHOT;
static_assert(DWH_OBS_FIELDS == dwh::kObsFields, "the record the kernel writes");

// snapshots of the sweeps below x: sw = offset, offset + every, ...
int64_t snaps_below(int64_t x, int64_t every, int64_t offset) {
  return x > offset ? (x - 1 - offset) / every + 1 : 0;
}

// The one validation of a log setting and of a sweep range within ndraws
// loaded sweeps; counts (3): doubles of obs, doubles of sq, snapshots of the
// range.  why: the reason for dwh_last_error.
int layout(int64_t nchains, int64_t N, int64_t ndraws, int32_t what, int64_t every, int64_t offset, int64_t first,
           int64_t nsweeps, int64_t* counts, std::string* why) {
  auto bad = [&](const char* m) {
    *why = m;
    return (int)DWH_ERR_ARG;
  };
  if (nchains < 1 || N < 1 || ndraws < 0) return bad("sweep log: nchains, N >= 1 and ndraws >= 0");
  if (what & ~kLogMask) return bad("sweep log: bits outside DWH_LOG_OBS | DWH_LOG_FIELD_SQ | DWH_LOG_SNAPSHOT");
  if ((what & DWH_LOG_SNAPSHOT) && (every < 1 || offset < 0))
    return bad("sweep log: snapshots need snap_every >= 1 and snap_offset >= 0");
  if ((what & DWH_LOG_FIELD_SQ) && N > dwh::kLogSqMaxN)
    return bad("sweep log: the field structure factors need N <= 4096");
  if (first < 0 || nsweeps < 0 || first + nsweeps > ndraws) return bad("sweep range outside the loaded draws");
  if (counts) {
    counts[0] = (what & DWH_LOG_OBS) ? DWH_OBS_FIELDS * nchains * nsweeps : 0;
    counts[1] = (what & DWH_LOG_FIELD_SQ) ? 2 * N * nchains * nsweeps : 0;
    counts[2] = (what & DWH_LOG_SNAPSHOT)
                    ? snaps_below(first + nsweeps, every, offset) - snaps_below(first, every, offset)
                    : 0;
  }
  return DWH_OK;
}

int layout(const dwh_ctx* ctx, int64_t ndraws, int64_t first, int64_t nsweeps, int64_t* counts, std::string* why) {
  return layout(ctx->d.nc, ctx->d.N, ndraws, ctx->log_what, ctx->log_every, ctx->log_offset, first, nsweeps, counts,
                why);
}

// bytes of the three buffers for log_ndraws sweeps
void log_bytes(const dwh_ctx* ctx, size_t* b) {
  int64_t n[3] = {0, 0, 0};
  std::string why;
  (void)layout(ctx, ctx->log_ndraws, 0, ctx->log_ndraws, n, &why);
  b[0] = (size_t)n[0] * sizeof(double);
  b[1] = (size_t)n[1] * sizeof(double);
  b[2] = (size_t)n[2] * ctx->d.nc * 2 * ctx->d.N * sizeof(double2);
}

void log_free(dwh_ctx* ctx) {
  size_t b[3];
  log_bytes(ctx, b);
  void* p[3] = {ctx->log_obs, ctx->log_sq, ctx->log_snap};
  for (int k = 0; k < 3; ++k)
    if (p[k]) {
      ctx->device_bytes -= (int64_t)std::max<size_t>(b[k], 1);
      dwh::drop_alloc(ctx, p[k]);
    }
  ctx->log_obs = ctx->log_sq = nullptr;
  ctx->log_snap = nullptr;
  ctx->log_ndraws = 0;
}

// a reader's common start: the part enabled, the range valid, pending sweeps settled
int reader(dwh_ctx* ctx, int32_t part, const char* name, int64_t first, int64_t nsweeps, int64_t* counts) {
  if (!ctx) return DWH_ERR_ARG;
  if (!(ctx->log_what & part)) return fail(ctx, DWH_ERR_STATE, std::string("the sweep log does not record ") + name);
  std::string why;
  if (int rc = layout(ctx, ctx->ndraws, first, nsweeps, counts, &why)) return fail(ctx, rc, why);
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  return dwh::settle(ctx);
}

}  // namespace

void dwh::sweep_log_enqueue(dwh_ctx* ctx, int64_t sw) {
  const Dims& d = ctx->d;
  const size_t nc = (size_t)d.nc, nbond = nc * 2 * d.N;
  if (sw >= ctx->log_ndraws) return;
  if (ctx->log_what & DWH_LOG_OBS) {
    Scope t(ctx, T_SWEEP_LOG, (double)(nc * kObsFields * sizeof(double)));
    launch_log_obs(d, ctx->Delta, ctx->Pair, ctx->Ef, ctx->Trhh, ctx->beta, ctx->J,
                   ctx->log_obs + nc * kObsFields * sw, ctx->halt, ctx->stream);
  }
  if (ctx->log_what & DWH_LOG_FIELD_SQ) {
    Scope t(ctx, T_SWEEP_LOG, (double)(nbond * sizeof(double)));
    (void)launch_log_field_sq(d, ctx->model->Lx, ctx->model->Ly, ctx->Delta, ctx->log_sq + nbond * sw, ctx->halt,
                              ctx->stream);
  }
  if ((ctx->log_what & DWH_LOG_SNAPSHOT) && sw >= ctx->log_offset && (sw - ctx->log_offset) % ctx->log_every == 0) {
    Scope t(ctx, T_SWEEP_LOG, (double)(nbond * sizeof(double2)));
    launch_log_snapshot(d, ctx->Delta, ctx->log_snap + nbond * ((sw - ctx->log_offset) / ctx->log_every), ctx->halt,
                        ctx->stream);
  }
}

int dwh::sweep_log_resize(dwh_ctx* ctx) {
  log_free(ctx);
  if (!ctx->log_what || ctx->ndraws < 1) return DWH_OK;
  ctx->log_ndraws = ctx->ndraws;
  size_t b[3];
  log_bytes(ctx, b);
  int rc = DWH_OK;
  if (b[0] && rc == DWH_OK) rc = dalloc(ctx, &ctx->log_obs, b[0] / sizeof(double));
  if (b[1] && rc == DWH_OK) rc = dalloc(ctx, &ctx->log_sq, b[1] / sizeof(double));
  if (b[2] && rc == DWH_OK) rc = dalloc(ctx, &ctx->log_snap, b[2] / sizeof(double2));
  if (rc != DWH_OK) {
    log_free(ctx);
    ctx->log_what = 0;
    return rc;
  }
  void* p[3] = {ctx->log_obs, ctx->log_sq, ctx->log_snap};
  for (int k = 0; k < 3; ++k)
    if (p[k]) HIPCHECK(ctx, hipMemsetAsync(p[k], 0, b[k], ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

void dwh::sweep_log_move(dwh_ctx* ctx, dwh_ctx* n) {
  size_t b[3];
  log_bytes(ctx, b);
  void* p[3] = {ctx->log_obs, ctx->log_sq, ctx->log_snap};
  for (int k = 0; k < 3; ++k) {
    if (!p[k]) continue;
    auto it = std::find(ctx->allocations.begin(), ctx->allocations.end(), p[k]);
    if (it != ctx->allocations.end()) ctx->allocations.erase(it);
    ctx->device_bytes -= (int64_t)std::max<size_t>(b[k], 1);
    n->allocations.push_back(p[k]);
    n->device_bytes += (int64_t)std::max<size_t>(b[k], 1);
  }
  n->log_what = ctx->log_what;
  n->log_every = ctx->log_every;
  n->log_offset = ctx->log_offset;
  n->log_ndraws = ctx->log_ndraws;
  n->log_obs = ctx->log_obs;
  n->log_sq = ctx->log_sq;
  n->log_snap = ctx->log_snap;
  ctx->log_obs = ctx->log_sq = nullptr;
  ctx->log_snap = nullptr;
  ctx->log_what = 0;
  ctx->log_ndraws = 0;
}

extern "C" {

int dwh_sweep_log_layout(int64_t nchains, int64_t N, int64_t ndraws, int32_t what, int64_t snap_every,
                         int64_t snap_offset, int64_t first, int64_t nsweeps, int64_t* counts) {
  std::string why;
  if (int rc = layout(nchains, N, ndraws, what, snap_every, snap_offset, first, nsweeps, counts, &why))
    return fail(nullptr, rc, why);
  return DWH_OK;
}

int dwh_sweep_log(dwh_ctx* ctx, int32_t what, int64_t snap_every, int64_t snap_offset) {
  if (!ctx) return DWH_ERR_ARG;
  std::string why;
  if (int rc = layout(ctx->d.nc, ctx->d.N, ctx->ndraws, what, snap_every, snap_offset, 0, 0, nullptr, &why))
    return fail(ctx, rc, why);
  if (ctx->pending) return fail(ctx, DWH_ERR_STATE, "dwh_hmc_finish the pending trajectory first");
  HIPCHECK(ctx, hipSetDevice(ctx->device));
  // a batch is never half logged
  SETTLE(ctx);
  dwh::drain_timing(ctx);
  log_free(ctx);
  ctx->log_what = what;
  ctx->log_every = (what & DWH_LOG_SNAPSHOT) ? snap_every : 1;
  ctx->log_offset = (what & DWH_LOG_SNAPSHOT) ? snap_offset : 0;
  return dwh::sweep_log_resize(ctx);
}

int dwh_sweep_observables(dwh_ctx* ctx, int64_t first, int64_t nsweeps, double* obs) {
  int64_t n[3];
  if (int rc = reader(ctx, DWH_LOG_OBS, "observables", first, nsweeps, n)) return rc;
  if (!obs) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  const size_t per = (size_t)ctx->d.nc * DWH_OBS_FIELDS;
  if (n[0] == 0) return DWH_OK;
  HIPCHECK(ctx, hipMemcpyAsync(obs, ctx->log_obs + per * first, (size_t)n[0] * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_sweep_field_sq(dwh_ctx* ctx, int64_t first, int64_t nsweeps, double* sq) {
  int64_t n[3];
  if (int rc = reader(ctx, DWH_LOG_FIELD_SQ, "the field structure factors", first, nsweeps, n)) return rc;
  if (!sq) return fail(ctx, DWH_ERR_ARG, "NULL argument");
  const size_t per = (size_t)ctx->d.nc * 2 * ctx->d.N;
  if (n[1] == 0) return DWH_OK;
  HIPCHECK(ctx, hipMemcpyAsync(sq, ctx->log_sq + per * first, (size_t)n[1] * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  return DWH_OK;
}

int dwh_sweep_snapshots(dwh_ctx* ctx, int64_t first, int64_t nsweeps, int64_t* nsnap, int64_t* sweep,
                        dwh_c128* Delta) {
  int64_t n[3];
  if (int rc = reader(ctx, DWH_LOG_SNAPSHOT, "snapshots", first, nsweeps, n)) return rc;
  if (nsnap) *nsnap = n[2];
  const int64_t slot0 = snaps_below(first, ctx->log_every, ctx->log_offset);
  if (sweep)
    for (int64_t m = 0; m < n[2]; ++m) sweep[m] = ctx->log_offset + (slot0 + m) * ctx->log_every;
  if (Delta && n[2] > 0) {
    const size_t per = (size_t)ctx->d.nc * 2 * ctx->d.N;
    HIPCHECK(ctx, hipMemcpyAsync(Delta, ctx->log_snap + per * slot0, per * n[2] * sizeof(double2),
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return DWH_OK;
}

}  // extern "C"
