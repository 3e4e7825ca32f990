// HMC integrator schedules (dwhmc_integrator.h): the presets, the checks of a
// custom splitting, the flattened coefficient list of a trajectory, and the
// host-only debug entry that returns it.
#include "dwhmc_integrator.h"

#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/dwhmc.h"
#include "dwhmc_model.h"

namespace dwh {

namespace {

int refuse(std::string* why, const std::string& msg) {
  if (why) *why = msg;
  return DWH_ERR_ARG;
}

bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

}  // namespace

int make_integrator(int32_t kind, double lambda, int64_t nstage, const double* kick, const double* drift,
                    Integrator* out, std::string* why) {
  Integrator r;
  r.kind = kind;
  if (kind == DWH_INT_LEAPFROG) {
    *out = r;   // S = 1, a = (½, ½), b = (1)
    return DWH_OK;
  }
  if (kind == DWH_INT_OMELYAN2) {
    if (!(lambda > 0.0 && lambda < 0.5)) return refuse(why, "integrator: omelyan2 needs 0 < lambda < 1/2");
    r.lambda = lambda;
    r.kick = {lambda, 1.0 - 2.0 * lambda, lambda};
    r.drift = {0.5, 0.5};
    *out = r;
    return DWH_OK;
  }
  if (kind != DWH_INT_CUSTOM) return refuse(why, "integrator: unknown kind");
  if (nstage < 1 || nstage > kMaxStages)
    return refuse(why, "integrator: a custom schedule has 1 <= nstage <= " + std::to_string(kMaxStages));
  if (!kick || !drift) return refuse(why, "integrator: a custom schedule needs its kick and drift arrays");
  const int S = (int)nstage;
  double sa = 0, sb = 0;
  for (int s = 0; s <= S; ++s) {
    if (!std::isfinite(kick[s])) return refuse(why, "integrator: non-finite kick coefficient");
    sa += kick[s];
  }
  for (int s = 0; s < S; ++s) {
    if (!std::isfinite(drift[s])) return refuse(why, "integrator: non-finite drift coefficient");
    sb += drift[s];
  }
  if (!(std::fabs(sa - 1.0) <= 1e-12)) return refuse(why, "integrator: the kick coefficients must sum to 1 (within 1e-12)");
  if (!(std::fabs(sb - 1.0) <= 1e-12)) return refuse(why, "integrator: the drift coefficients must sum to 1 (within 1e-12)");
  // a_s = a_{S-s}, b_s = b_{S+1-s} (b_1 is drift[0]), bit for bit
  for (int s = 0; s <= S; ++s)
    if (!same_bits(kick[s], kick[S - s])) return refuse(why, "integrator: the kick coefficients are not palindromic");
  for (int s = 0; s < S; ++s)
    if (!same_bits(drift[s], drift[S - 1 - s])) return refuse(why, "integrator: the drift coefficients are not palindromic");
  r.kick.assign(kick, kick + S + 1);
  r.drift.assign(drift, drift + S);
  *out = r;
  return DWH_OK;
}

int flatten_schedule(const Integrator& integ, int64_t Nt, double dt, double mass, FlatSchedule* out,
                     std::string* why) {
  if (Nt < 0 || Nt > std::numeric_limits<int64_t>::max() / kMaxStages) return refuse(why, "bad Nt/dt/mass");
  if (Nt == 0 && integ.kind != DWH_INT_LEAPFROG)
    return refuse(why, "Nt = 0 (two half kicks, no factorisation) is defined for the leapfrog integrator only");
  FlatSchedule f;
  f.S = integ.stages();
  f.nfact = (int64_t)f.S * Nt;
  f.nkick = Nt == 0 ? 2 : f.nfact + 1;
  f.dt = dt;
  f.mass = mass;
  f.integ = &integ;
  *out = f;
  return DWH_OK;
}

}  // namespace dwh

extern "C" int dwh_debug_integrator_schedule(int32_t kind, double lambda, int64_t nstage, const double* kick,
                                             const double* drift, int64_t Nt, double dt, double mass, int64_t* nfact,
                                             double* kicks_out, double* drifts_out) {
  std::string why;
  dwh::Integrator integ;
  dwh::FlatSchedule f;
  int rc = dwh::make_integrator(kind, lambda, nstage, kick, drift, &integ, &why);
  if (rc == DWH_OK && (!(mass > 0) || !std::isfinite(dt))) {
    rc = DWH_ERR_ARG;
    why = "bad Nt/dt/mass";
  }
  if (rc == DWH_OK) rc = dwh::flatten_schedule(integ, Nt, dt, mass, &f, &why);
  if (rc != DWH_OK) {
    dwh::g_create_error = why;   // dwh_last_error(NULL)
    return rc;
  }
  if (nfact) *nfact = f.nfact;
  if (kicks_out)
    for (int64_t i = 0; i < f.nkick; ++i) kicks_out[i] = f.kick(i);
  if (drifts_out)
    for (int64_t i = 0; i < f.nfact; ++i) drifts_out[i] = f.drift(i);
  return DWH_OK;
}
