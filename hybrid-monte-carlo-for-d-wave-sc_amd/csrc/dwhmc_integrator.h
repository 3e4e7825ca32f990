// The HMC integrator of a context: a symmetric splitting of one step of size
// dt into S force evaluations (kick a_0, then S times drift b_s, force, kick
// a_s), and the flattened (kick, drift) list of a whole trajectory that
// trajectory_enqueue hands to the kick/drift kernels.  Host only; private to
// dwhmc_api.cpp and dwhmc_integrator.cpp.  Not part of the public ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace dwh {

constexpr int kMaxStages = 16;

// kick: a_0..a_S (S + 1 entries), drift: b_1..b_S (S entries); kind and lambda
// are what the caller asked for (dwh_get_integrator reports them)
struct Integrator {
  int32_t kind = 0;   // DWH_INT_LEAPFROG
  double lambda = 0.0;
  std::vector<double> kick{0.5, 0.5};
  std::vector<double> drift{1.0};
  int stages() const { return (int)drift.size(); }
};

// The preset or the checked custom schedule.  Returns DWH_OK, or DWH_ERR_ARG
// with the reason in *why.
int make_integrator(int32_t kind, double lambda, int64_t nstage, const double* kick, const double* drift,
                    Integrator* out, std::string* why);

// A trajectory of Nt steps as the launches see it: nfact = S·Nt
// factorisations, kick(0) with k_traj_begin, kick(i) after factorisation i
// (adjacent end and start kicks of two steps merged into one coefficient),
// drift(i) before factorisation i + 1.  The coefficients are the kernels'
// own: kick in units of F, drift = b·dt/(2m) in units of π.
// Nt = 0 (leapfrog only): no factorisation and the two half kicks today's
// code makes, nkick = 2.
struct FlatSchedule {
  int64_t nfact = 0, nkick = 0;
  int S = 1;
  double dt = 0, mass = 1;
  const Integrator* integ = nullptr;
  double kick(int64_t i) const {
    const std::vector<double>& a = integ->kick;
    if (i == 0) return a[0] * dt;
    if (i >= nfact) return a[S] * dt;
    const int s = (int)(i % S);
    // one double formed on the host: leapfrog's (½ + ½)·dt is dt exactly
    return s == 0 ? (a[S] + a[0]) * dt : a[s] * dt;
  }
  double drift(int64_t i) const { return (integ->drift[i % S] * dt) / (2.0 * mass); }
};

// DWH_OK, or DWH_ERR_ARG (Nt < 0, or Nt = 0 with anything but leapfrog)
int flatten_schedule(const Integrator& integ, int64_t Nt, double dt, double mass, FlatSchedule* out,
                     std::string* why);

}  // namespace dwh
