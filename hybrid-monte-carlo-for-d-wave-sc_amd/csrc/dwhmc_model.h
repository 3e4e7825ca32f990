// Host-only model pieces of the C-ABI context (dwhmc_model.cpp): the compiled
// pole tables, the static hopping rows and the bound on ||h|| the pole
// selection uses, and the error text of calls that have no context.  Needs no
// device and no vendor library.  Not part of the public ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace dwh {

// Error text of a call that failed without a context (dwh_create*, the
// host-only debug entry points): what dwh_last_error(NULL) returns.
extern thread_local std::string g_create_error;
inline int fail(std::nullptr_t, int code, const std::string& msg) {
  g_create_error = msg;
  return code;
}

struct PoleView {
  double kappa;
  int m;
  double C_u, err_tanh;
  const double *t, *a;
};
struct PoleTable {
  const char* name;
  int size;
  PoleView (*at)(int);
};
// the table DWHMC_POLE_TABLE selects (budget | strict; default budget);
// nullptr with *err set for any other value
const PoleTable* pole_table(std::string* err);

// static h (off-diagonal rows): the reference's upper-triangle loop with
// overwrite (Hamiltonian.jl:26-44), nnn after nn
std::vector<std::vector<std::pair<int, double>>> build_hrow(int N, double t, double tp, const int64_t* nn,
                                                            const int64_t* nnn);
// ‖h‖ bound over the chains: min(Gershgorin, Lanczos) when every chain's
// h certifies the Lanczos value, else Gershgorin
double h_norm_bound(const std::vector<std::vector<std::pair<int, double>>>& hrow, const double* disorder, double mu,
                    int N, int Lx, int Ly, int64_t nchains, double gersh, double* lanczos = nullptr,
                    bool* certified = nullptr);
// default guard cap (bond guard or site guard; dwhmc_model.cpp)
double default_delta_cap(double beta, double J, bool site_guard);

}  // namespace dwh
