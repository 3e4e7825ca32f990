// Host-only model pieces of the C-ABI context (dwhmc_model.cpp): the lattice
// model build_host_model derives once from the neighbour tables (hopping and
// pairing tables, bond slots, the bound on ||h||, the current operator, the
// site guard's bond list), the compiled pole tables with the pole selection,
// and the error text of calls that have no context.  Needs no device and no
// vendor library.  Not part of the public ABI.
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

// Everything context creation derives from (Lx, Ly, t, t', mu, the neighbour
// tables, the chains' disorder) that does not depend on the guard cap, the poles
// or the algorithm.  Built once by build_host_model; a pole re-selection reuses it.
struct HostModel {
  int64_t Lx = 0, Ly = 0, nchains = 0;
  int N = 0;
  double t = 0, tp = 0;
  // static h, off-diagonal rows: the reference's upper-triangle loop with
  // overwrite (src/Hamiltonian.jl:26-44), nnn after nn
  std::vector<std::vector<std::pair<int, double>>> hrow;
  // per site kHSlots hopping entries: the site itself (w_i - mu per chain,
  // src/Hamiltonian.jl:18-22), then hrow's partners; -1 / 0 unused
  std::vector<int> hcol;      // N x kHSlots
  std::vector<double> hval;   // nchains x N x kHSlots
  // pairing pattern D[r, c] <- Delta[src]/2 with the reference's overwrite
  // order (src/Hamiltonian.jl:68-83): per site kSlots partners, ascending; -1 unused
  std::vector<int> Dcol, Dsrc;   // N x kSlots
  // bond dir * N + i (i -- nn[i, dir], dir = +x, +y): entries r * kSlots + s of D[i, j], D[j, i]
  std::vector<int> bij, bji;
  // ||h|| over the chains: Gershgorin sum, Lanczos estimate, whether every
  // chain certified it, and the bound the pole selection uses
  double gersh = 0, lanczos = 0, hmax = 0;
  bool certified = false;
  // x-current operator J (src/Observables.jl:237-283): i t at (i, i+x), i t' at
  // (i, i+x+y) and (i, i+x-y), plus their conjugate transposes, summed into CSR
  // (duplicates added), as imaginary parts; tr_nbr: those neighbours, [3][N]
  std::vector<int> tr_nbr, tr_rowptr, tr_col;
  std::vector<double> tr_val;
  // the neighbour tables themselves, 0-based, [dir][N] (the finite-momentum
  // current operators of either direction are built from them per call)
  std::vector<int> nn, nnn;
  // site i: the Delta indices of its bonds (i, +x), (i, +y), (i - x, +x), (i - y, +y) (site guard)
  std::vector<int> site4;
};
// the lattice arguments of dwh_create*: sizes, NULL tables, neighbour entries in [1, N] (DWH_ERR_ARG)
int check_lattice_args(int64_t Lx, int64_t Ly, int64_t nchains, const int64_t* nn, const int64_t* nnn,
                       const double* disorder);
// check_lattice_args, then the tables; refuses (DWH_ERR_ARG) a site with more
// than 8 hopping or 4 pairing partners and non-finite disorder.  lanczos =
// false leaves hmax at the Gershgorin sum (callers that need only the tables)
int build_host_model(int64_t Lx, int64_t Ly, double t, double tp, double mu, const int64_t* nn, const int64_t* nnn,
                     int64_t nchains, const double* disorder, HostModel* m, bool lanczos = true);

// The pole set for spectra within E' = hmax + 2 delta_cap >= ||H_BdG|| (the
// pairing block's norm <= its max row sum <= 2 delta_cap; bond guard: each of
// the 4 bonds <= cap; site guard: their mean <= cap): the first table entry with
// kappa >= beta E'/2; beyond the table the eigendecomposition path (eig: no
// pole set, one dummy batch item per chain, y = cq = {0}).
struct PoleChoice {
  bool eig = false;
  double kappa = 0, Ep = 0, Cx = 0, err_tanh = 0;
  std::vector<double> y, cq;   // per pole: E' sqrt(t_q), a_q E'/2
};
// eig_requested: the eig path whatever the table holds; eig_allowed: eig when
// beyond the table, else DWH_ERR_TABLE.  DWH_ERR_ARG: DWHMC_POLE_TABLE.
int select_poles(double hmax, double beta, double delta_cap, bool eig_requested, bool eig_allowed, PoleChoice* out);
// default guard cap (bond guard or site guard; dwhmc_model.cpp)
double default_delta_cap(double beta, double J, bool site_guard);

}  // namespace dwh
