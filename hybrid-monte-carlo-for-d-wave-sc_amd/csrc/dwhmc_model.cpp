// Host-only model pieces of the C-ABI context (dwhmc_model.h): the lattice
// model (build_host_model: argument checks, hopping and pairing tables with
// the reference's overwrite order, bond slots, the bound on ||h|| — Gershgorin
// or a certified Lanczos value —, the x-current operator, the site guard's
// bond list), the pole tables with the pole selection (select_poles) and the
// default guard cap.  No device and no vendor library:
// tools/host_check/plan_main.cpp links this file and dwhmc_plan.cpp alone and
// checks the tables against a dense restatement of the reference.
#include "dwhmc_model.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../include/dwhmc.h"
#include "dwhmc_internal.h"

// Two compiled pole tables (tools/gen_pole_table.py): "budget", sup|tanh
// error| <= 5e-12 — half the 1e-11 absolute budget the pairing tolerance
// leaves for the expansion (|δP_ij| <= ε; E_f and F budgets are looser,
// DESIGN.md §2) — and "strict" (<= 2e-14).  DWHMC_POLE_TABLE selects one;
// default "budget".
namespace tab_strict {
#include "pole_table.inc"
}
namespace tab_budget {
#include "pole_table_eps5e-12.inc"
}

namespace dwh {

thread_local std::string g_create_error;

namespace {
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
template <typename E>
PoleView pole_view(const E& e, const double* T, const double* A) {
  return PoleView{e.kappa, e.m, e.C_u, e.err_tanh, T + e.off, A + e.off};
}
const PoleTable kPoleTables[2] = {
    {"budget", tab_budget::kPoleTableSize,
     [](int e) { return pole_view(tab_budget::kPoleEntries[e], tab_budget::kPoleT, tab_budget::kPoleA); }},
    {"strict", tab_strict::kPoleTableSize,
     [](int e) { return pole_view(tab_strict::kPoleEntries[e], tab_strict::kPoleT, tab_strict::kPoleA); }},
};
}  // namespace

int select_poles(double hmax, double beta, double delta_cap, bool eig_requested, bool eig_allowed, PoleChoice* out) {
  const double Eb = hmax + 2.0 * delta_cap;
  const double kneed = 0.5 * beta * Eb;
  // the table DWHMC_POLE_TABLE selects (budget | strict; default budget)
  const char* name = std::getenv("DWHMC_POLE_TABLE");
  const PoleTable* tab = !name || !*name ? &kPoleTables[0] : nullptr;
  for (const PoleTable& pt : kPoleTables)
    if (name && std::strcmp(name, pt.name) == 0) tab = &pt;
  if (!tab) return fail(nullptr, DWH_ERR_ARG, "DWHMC_POLE_TABLE must be budget or strict");
  int sel = -1;
  for (int e = 0; e < tab->size; ++e)
    if (tab->at(e).kappa >= kneed * (1.0 - 1e-12)) {
      sel = e;
      break;
    }
  PoleChoice& pc = *out;
  pc = PoleChoice{};
  pc.eig = eig_requested || (sel < 0 && eig_allowed);
  if (sel < 0 && !pc.eig) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "beta*E_bound/2 = %g exceeds the pole table (max kappa %g)", kneed,
                  tab->at(tab->size - 1).kappa);
    return fail(nullptr, DWH_ERR_TABLE, buf);
  }
  if (pc.eig) {   // exact for any Δ: no pole set
    pc.kappa = kneed;
    pc.Ep = Eb;
    pc.y = pc.cq = {0.0};
    return DWH_OK;
  }
  const PoleView pe = tab->at(sel);
  pc.kappa = pe.kappa;
  pc.Ep = 2.0 * pe.kappa / beta;
  pc.y.resize(pe.m);
  pc.cq.resize(pe.m);
  double suma = 0;
  for (int q = 0; q < pe.m; ++q) {
    pc.y[q] = pc.Ep * std::sqrt(pe.t[q]);
    pc.cq[q] = 0.5 * pe.a[q] * pc.Ep;
    suma += pe.a[q];
  }
  pc.err_tanh = pe.err_tanh;
  pc.Cx = pe.C_u - pc.kappa * std::log(pc.Ep) * suma;
  return DWH_OK;
}

namespace {

// Spectral radius of the static particle block h of one chain (real
// symmetric, rows hrow + diagonal w_i - mu), by Lanczos with full
// reorthogonalisation from a fixed pseudo-random start: the extreme Ritz
// values converge first; the returned bound adds the residual |β s_m| of the
// extreme Ritz pairs and a 2 % margin.  For
// N <= the step count the Krylov space is all of R^N and the Ritz values are
// the spectrum.  The caller takes min(this, the Gershgorin bound).
double spectral_radius_bound(const std::vector<std::vector<std::pair<int, double>>>& hrow,
                             const double* diag, int N) {
  const int k = std::min(N, 160);
  std::vector<std::vector<double>> Q;
  std::vector<double> alpha, beta;
  std::vector<double> q(N), w(N);
  uint64_t st = 0x9E3779B97F4A7C15ull;
  double nrm = 0;
  for (int i = 0; i < N; ++i) {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    q[i] = (double)(st >> 11) * 0x1.0p-53 - 0.5;
    nrm += q[i] * q[i];
  }
  for (double& x : q) x /= std::sqrt(nrm);
  double bnext = 0;
  for (int j = 0; j < k; ++j) {
    Q.push_back(q);
    for (int i = 0; i < N; ++i) {
      double v = diag[i] * q[i];
      for (const auto& e : hrow[i]) v += e.second * q[e.first];
      w[i] = v;
    }
    double a = 0;
    for (int i = 0; i < N; ++i) a += w[i] * q[i];
    alpha.push_back(a);
    for (int pass = 0; pass < 2; ++pass)
      for (const auto& qq : Q) {
        double c = 0;
        for (int i = 0; i < N; ++i) c += w[i] * qq[i];
        for (int i = 0; i < N; ++i) w[i] -= c * qq[i];
      }
    double b = 0;
    for (int i = 0; i < N; ++i) b += w[i] * w[i];
    b = std::sqrt(b);
    bnext = b;
    if (j + 1 == k || b < 1e-12) break;
    beta.push_back(b);
    for (int i = 0; i < N; ++i) q[i] = w[i] / b;
  }
  // extreme eigenvalues of the tridiagonal T by bisection on Sturm counts
  const int m = (int)alpha.size();
  double lo = 0, hi = 0;
  for (int i = 0; i < m; ++i) {
    const double r = (i > 0 ? std::fabs(beta[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(beta[i]) : 0.0);
    lo = std::min(lo, alpha[i] - r);
    hi = std::max(hi, alpha[i] + r);
  }
  auto count_below = [&](double x) {   // eigenvalues of T < x
    int c = 0;
    double d = 1.0;
    for (int i = 0; i < m; ++i) {
      d = alpha[i] - x - (i > 0 ? beta[i - 1] * beta[i - 1] / d : 0.0);
      if (d == 0.0) d = 1e-300;
      if (d < 0) ++c;
    }
    return c;
  };
  auto kth = [&](int idx) {   // idx-th smallest (0-based)
    double a = lo, b = hi;
    for (int it = 0; it < 200 && b - a > 1e-13 * std::max(1.0, std::fabs(b)); ++it) {
      const double mid = 0.5 * (a + b);
      if (count_below(mid) > idx) b = mid;
      else a = mid;
    }
    return b;
  };
  // residual of the Ritz pair (θ, Q s) is |β_m s_m|: last component of the
  // eigenvector s of T for θ, by inverse iteration on the tridiagonal system
  auto resid_of = [&](double th) {
    if (m == N) return 0.0;
    std::vector<double> x(m, 1.0), c(m), d(m), y(m);
    const double sh = th + 1e-10 * std::max(1.0, std::fabs(th));
    for (int it = 0; it < 3; ++it) {
      // Thomas solve (T - sh I) y = x
      for (int i = 0; i < m; ++i) {
        const double b = alpha[i] - sh - (i > 0 ? beta[i - 1] * c[i - 1] : 0.0);
        const double bb = (b == 0.0) ? 1e-300 : b;
        c[i] = (i + 1 < m) ? beta[i] / bb : 0.0;
        d[i] = (x[i] - (i > 0 ? beta[i - 1] * d[i - 1] : 0.0)) / bb;
      }
      y[m - 1] = d[m - 1];
      for (int i = m - 2; i >= 0; --i) y[i] = d[i] - c[i] * y[i + 1];
      double n2 = 0;
      for (double v : y) n2 += v * v;
      const double inv = 1.0 / std::sqrt(n2);
      for (int i = 0; i < m; ++i) x[i] = y[i] * inv;
    }
    return std::fabs(bnext * x[m - 1]);
  };
  const double tmin = kth(0), tmax = kth(m - 1);
  const double rho = std::max(std::fabs(tmin) + resid_of(tmin), std::fabs(tmax) + resid_of(tmax));
  return 1.02 * rho + 1e-12;
}

// Certifies rho >= ‖h‖ for the real symmetric h (off-diagonal hrow, diagonal
// diag): rho I - h and rho I + h are positive definite iff every pivot of
// their LDLᵀ factorisations is > 0 (Sylvester's law of inertia), so a
// Lanczos estimate that missed an eigenvalue fails here.  Band LDLᵀ in the
// folded row order (lattice rows 0, Ly-1, 1, Ly-2, ...: with the periodic
// corner folded in, the lattice couplings lie within 3 Lx - 1 of the
// diagonal), O(N b²); a bandwidth over 512 (a table that is not a lattice of
// rows) is not certified and the caller keeps the Gershgorin bound.
bool certify_spectral_bound(const std::vector<std::vector<std::pair<int, double>>>& hrow, const double* diag,
                            int N, int Lx, int Ly, double rho) {
  auto pos = [&](int i) {
    const int x = i % Lx, y = i / Lx;
    const int f = 2 * y < Ly ? 2 * y : 2 * (Ly - 1 - y) + 1;
    return f * Lx + x;
  };
  std::vector<int> p(N), inv(N);
  int b = 0;
  for (int i = 0; i < N; ++i) {
    p[i] = pos(i);
    inv[p[i]] = i;
  }
  for (int i = 0; i < N; ++i)
    for (const auto& e : hrow[i]) b = std::max(b, std::abs(p[i] - p[e.first]));
  if (b > 512) return false;
  const size_t W = (size_t)b + 1;
  std::vector<double> A((size_t)N * W), Lw((size_t)N * W), d(N);
  for (int sgn = -1; sgn <= 1; sgn += 2) {   // rho I + sgn h
    std::fill(A.begin(), A.end(), 0.0);
    for (int k = 0; k < N; ++k) {   // row k of the lower band: A[k][k - j] at k * W + j
      const int i = inv[k];
      A[(size_t)k * W] = rho + sgn * diag[i];
      for (const auto& e : hrow[i]) {
        const int c = p[e.first];
        if (c < k) A[(size_t)k * W + (k - c)] += sgn * e.second;
      }
    }
    // L[k][j] d[j] kept as Lw (the row's W entries), L[k][j] recovered on use
    for (int k = 0; k < N; ++k) {
      const int j0 = std::max(0, k - b);
      double dk = A[(size_t)k * W];
      for (int j = j0; j < k; ++j) {
        // s = A[k][j] - Σ_{i < j} L[k][i] d[i] L[j][i]
        double sacc = A[(size_t)k * W + (k - j)];
        const int i0 = std::max(j0, j - b);
        for (int i = i0; i < j; ++i)
          sacc -= Lw[(size_t)k * W + (k - i)] * (Lw[(size_t)j * W + (j - i)] / d[i]);
        Lw[(size_t)k * W + (k - j)] = sacc;   // = L[k][j] d[j]
        dk -= sacc * sacc / d[j];
      }
      if (!(dk > 0)) return false;
      d[k] = dk;
    }
  }
  return true;
}

}  // namespace

// Default guard cap.  Bond guard (max|Δ_ij| <= cap): 2 (the ordered phase), or
// 6 standard deviations of the Gaussian boson fluctuations <|Δ|²> = 2J/β at
// high temperature.  Site guard (the mean of |Δ| over each site's four bonds
// <= cap, CR path: its level-0 inversion launch checks it): max(1.25, 4 sqrt(2J/β)) — the same ≈ 1.6x
// margin over the largest value thermalised L = 32 chains reach (site mean
// 0.79 / 1.08 / 1.49 at β = 16 / 8 / 4 over 300 sweeps against max|Δ_ij|
// 1.27 / 1.78 / 2.49, tools/delta_stats.py, profiles/r02_delta_stats.txt).
// Either way the pairing block's norm is at most its max row sum <= 2 cap.
double default_delta_cap(double beta, double J, bool site_guard) {
  const double s = std::sqrt(2.0 * std::fabs(J) / beta);
  return site_guard ? std::max(1.25, 4.0 * s) : std::max(2.0, 6.0 * s);
}

namespace {

// ‖h‖ bound over the chains: min(Gershgorin, Lanczos) when every chain's
// h certifies the Lanczos value, else Gershgorin
double h_norm_bound(const std::vector<std::vector<std::pair<int, double>>>& hrow, const double* disorder, double mu,
                    int N, int Lx, int Ly, int64_t nchains, double gersh, double* lanczos, bool* certified) {
  double rho = 0;
  std::vector<double> diag(N);
  for (int64_t c = 0; c < nchains; ++c) {
    for (int i = 0; i < N; ++i) diag[i] = disorder[c * (int64_t)N + i] - mu;
    rho = std::max(rho, spectral_radius_bound(hrow, diag.data(), N));
  }
  bool ok = rho < gersh;
  for (int64_t c = 0; c < nchains && ok; ++c) {
    for (int i = 0; i < N; ++i) diag[i] = disorder[c * (int64_t)N + i] - mu;
    ok = certify_spectral_bound(hrow, diag.data(), N, Lx, Ly, rho);
  }
  if (lanczos) *lanczos = rho;
  if (certified) *certified = ok;
  return ok ? rho : gersh;
}

// static h (off-diagonal rows): the reference's upper-triangle loop with
// overwrite (Hamiltonian.jl:26-44), nnn after nn
std::vector<std::vector<std::pair<int, double>>> build_hrow(int N, double t, double tp, const int64_t* nn,
                                                            const int64_t* nnn) {
  auto NN = [&](int i, int dir) { return (int)(nn[(int64_t)dir * N + i] - 1); };
  auto NNN = [&](int i, int dir) { return (int)(nnn[(int64_t)dir * N + i] - 1); };
  std::map<std::pair<int, int>, double> up;
  for (int i = 0; i < N; ++i) {
    for (int dir = 0; dir < 4; ++dir) {
      const int j = NN(i, dir);
      if (j > i) up[{i, j}] = -t;
    }
    for (int dir = 0; dir < 4; ++dir) {
      const int j = NNN(i, dir);
      if (j > i) up[{i, j}] = -tp;
    }
  }
  std::vector<std::vector<std::pair<int, double>>> hrow(N);
  for (auto& kv : up) {
    hrow[kv.first.first].push_back({kv.first.second, kv.second});
    hrow[kv.first.second].push_back({kv.first.first, kv.second});
  }
  return hrow;
}

}  // namespace

int check_lattice_args(int64_t Lx, int64_t Ly, int64_t nchains, const int64_t* nn, const int64_t* nnn,
                       const double* disorder) {
  if (Lx < 1 || Ly < 1) return fail(nullptr, DWH_ERR_ARG, "Lx, Ly must be >= 1");
  if (nchains < 1) return fail(nullptr, DWH_ERR_ARG, "nchains must be >= 1");
  if (!nn || !nnn || !disorder) return fail(nullptr, DWH_ERR_ARG, "NULL table or disorder");
  const int64_t N64 = Lx * Ly;
  if (N64 > 9216) return fail(nullptr, DWH_ERR_ARG, "N = Lx*Ly > 9216 not supported (LDS row staging)");
  for (int64_t e = 0; e < 4 * N64; ++e)
    if (nn[e] < 1 || nn[e] > N64 || nnn[e] < 1 || nnn[e] > N64)
      return fail(nullptr, DWH_ERR_ARG, "neighbour table entry out of [1, N]");
  return DWH_OK;
}

int build_host_model(int64_t Lx, int64_t Ly, double t, double tp, double mu, const int64_t* nn, const int64_t* nnn,
                     int64_t nchains, const double* disorder, HostModel* out, bool lanczos) {
  if (int rc = check_lattice_args(Lx, Ly, nchains, nn, nnn, disorder)) return rc;
  HostModel& m = *out;
  m = HostModel{};
  const int N = (int)(Lx * Ly);
  m.Lx = Lx;
  m.Ly = Ly;
  m.nchains = nchains;
  m.N = N;
  m.t = t;
  m.tp = tp;
  auto NN = [&](int i, int dir) { return (int)(nn[(int64_t)dir * N + i] - 1); };
  auto NNN = [&](int i, int dir) { return (int)(nnn[(int64_t)dir * N + i] - 1); };

  // --- static h: reference upper-triangle loop with overwrite (Hamiltonian.jl:26-44)
  m.hrow = build_hrow(N, t, tp, nn, nnn);
  const auto& hrow = m.hrow;
  m.hcol.assign((size_t)N * kHSlots, -1);
  m.hval.assign((size_t)nchains * N * kHSlots, 0.0);
  for (int i = 0; i < N; ++i) {
    if ((int)hrow[i].size() + 1 > kHSlots)
      return fail(nullptr, DWH_ERR_ARG, "more than 8 hopping partners per site");
    m.hcol[(size_t)i * kHSlots] = i;
    double off = 0;
    for (size_t s = 0; s < hrow[i].size(); ++s) {
      m.hcol[(size_t)i * kHSlots + 1 + s] = hrow[i][s].first;
      off += std::fabs(hrow[i][s].second);
    }
    for (int64_t c = 0; c < nchains; ++c) {
      const double w = disorder[c * (int64_t)N + i];
      if (!std::isfinite(w)) return fail(nullptr, DWH_ERR_ARG, "non-finite disorder");
      m.hval[((size_t)c * N + i) * kHSlots] = w - mu;  // Hamiltonian.jl:18-22
      for (size_t s = 0; s < hrow[i].size(); ++s)
        m.hval[((size_t)c * N + i) * kHSlots + 1 + s] = hrow[i][s].second;
      m.gersh = std::max(m.gersh, std::fabs(w - mu) + off);
    }
  }
  // --- pairing pattern with the reference overwrite order (Hamiltonian.jl:68-83);
  // both orientations of a bond are written together, so the map is symmetric
  std::map<std::pair<int, int>, int> dmap;
  for (int i = 0; i < N; ++i)
    for (int dir = 0; dir < 2; ++dir) {
      const int j = NN(i, dir);
      const int src = i + N * dir;
      dmap[{i, j}] = src;
      dmap[{j, i}] = src;
    }
  m.Dcol.assign((size_t)N * kSlots, -1);
  m.Dsrc.assign((size_t)N * kSlots, -1);
  std::vector<int> dcount(N, 0);
  for (auto& kv : dmap) {
    const int r = kv.first.first;
    if (dcount[r] >= kSlots) return fail(nullptr, DWH_ERR_ARG, "more than 4 pairing partners per site");
    m.Dcol[(size_t)r * kSlots + dcount[r]] = kv.first.second;
    m.Dsrc[(size_t)r * kSlots + dcount[r]] = kv.second;
    dcount[r]++;
  }
  auto slot_of = [&](int r, int c) {
    for (int s = 0; s < kSlots; ++s)
      if (m.Dcol[(size_t)r * kSlots + s] == c) return s;
    return -1;
  };
  m.bij.resize(2 * (size_t)N);
  m.bji.resize(2 * (size_t)N);
  for (int dir = 0; dir < 2; ++dir)
    for (int i = 0; i < N; ++i) {
      const int j = NN(i, dir);
      const int sij = slot_of(i, j), sji = slot_of(j, i);
      if (sij < 0 || sji < 0) return fail(nullptr, DWH_ERR_ARG, "bond missing from the pairing pattern");
      m.bij[(size_t)dir * N + i] = i * kSlots + sij;
      m.bji[(size_t)dir * N + i] = j * kSlots + sji;
    }
  // --- ‖h‖ <= min(Gershgorin, Lanczos bound), the latter only where certified
  m.hmax = m.gersh;
  if (lanczos)
    m.hmax = h_norm_bound(hrow, disorder, mu, N, (int)Lx, (int)Ly, nchains, m.gersh, &m.lanczos, &m.certified);
  // --- x-current operator (Observables.jl:237-283), duplicates summed
  {
    std::vector<std::map<int, double>> jrow(N);
    m.tr_nbr.assign(3 * (size_t)N, 0);
    for (int i = 0; i < N; ++i) {
      const int js[3] = {NN(i, 0), NNN(i, 0), NNN(i, 3)};
      const double ts[3] = {t, tp, tp};
      for (int b = 0; b < 3; ++b) {
        jrow[i][js[b]] += ts[b];
        jrow[js[b]][i] -= ts[b];
        m.tr_nbr[(size_t)b * N + i] = js[b];
      }
    }
    m.tr_rowptr.assign(N + 1, 0);
    for (int r = 0; r < N; ++r) {
      for (auto& kv : jrow[r]) {
        m.tr_col.push_back(kv.first);
        m.tr_val.push_back(kv.second);
      }
      m.tr_rowptr[r + 1] = (int)m.tr_col.size();
    }
  }
  m.nn.resize(4 * (size_t)N);
  m.nnn.resize(4 * (size_t)N);
  for (int dir = 0; dir < 4; ++dir)
    for (int i = 0; i < N; ++i) {
      m.nn[(size_t)dir * N + i] = NN(i, dir);
      m.nnn[(size_t)dir * N + i] = NNN(i, dir);
    }
  m.site4.resize(4 * (size_t)N);
  for (int i = 0; i < N; ++i)   // (i, +x), (i, +y), (i - x, +x), (i - y, +y): Delta index = site + N * (bond is +y)
    for (int k = 0; k < 4; ++k) m.site4[4 * i + k] = (k < 2 ? i : NN(i, k)) + N * (k & 1);
  return DWH_OK;
}

}  // namespace dwh

using namespace dwh;

// out: Gershgorin, Lanczos estimate, certified, the bound used, and whether
// the band test accepts rho = 0 for the clean h (it must not)
extern "C" int dwh_debug_h_bound(int64_t Lx, int64_t Ly, double t, double tp, double mu, const int64_t* nn_table,
                      const int64_t* nnn_table, int64_t nchains, const double* disorder, double* out) {
  if (!out) return fail(nullptr, DWH_ERR_ARG, "NULL output");
  HostModel m;
  if (int rc = build_host_model(Lx, Ly, t, tp, mu, nn_table, nnn_table, nchains, disorder, &m)) return rc;
  out[0] = m.gersh;
  out[1] = m.lanczos;
  out[2] = m.certified ? 1.0 : 0.0;
  out[3] = m.hmax;
  out[4] = certify_spectral_bound(m.hrow, std::vector<double>(m.N, -mu).data(), m.N, (int)Lx, (int)Ly, 0.0) ? 1.0 : 0.0;
  return DWH_OK;
}
