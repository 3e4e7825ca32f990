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
// dwh_debug_cr_plan_check and dwh_debug_cr_plan_flops over the lattices of
// tests/test_cr_plan_dataflow.py (both batch sizes, side / inv0 on and off,
// DWHMC_CR_SPARSE0 and DWHMC_CR_MERGE both ways) and dwh_debug_h_bound for one
// lattice.  Exit status 0: every call succeeded (and no sanitizer report).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dwhmc.h"
#include "dwhmc_model.h"   // dwh::g_create_error: the text dwh_last_error(NULL) returns in the library

namespace {

int failures = 0;

void expect(bool ok, const char* what, int Lx, int Ly, int nbatch, int side, int inv0, const char* sp, const char* mg) {
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: Lx=%d Ly=%d nbatch=%d side=%d inv0=%d SPARSE0=%s MERGE=%s: %s\n", what, Lx, Ly,
               nbatch, side, inv0, sp, mg, dwh::g_create_error.c_str());
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
            }
    }
  // a lattice row too wide for the CR path is refused, not planned
  if (dwh_debug_cr_plan_check(65, 4, 14, 1, 1, nullptr) == DWH_OK) {
    ++failures;
    std::fprintf(stderr, "FAIL plan_check accepted Lx = 65\n");
  }

  // ||h|| bound of a periodic 6 x 5 lattice with the reference's tables, two chains
  {
    const int Lx = 6, Ly = 5, N = Lx * Ly;
    std::vector<int64_t> nn(4 * N), nnn(4 * N);
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
    std::vector<double> dis(2 * N);
    for (int i = 0; i < 2 * N; ++i) dis[i] = 0.8 * std::sin(1.0 + 0.37 * i);
    double out[5] = {0, 0, 0, 0, 0};
    const int rc = dwh_debug_h_bound(Lx, Ly, 1.0, -0.35, -1.08, nn.data(), nnn.data(), 2, dis.data(), out);
    // the bound used is the Gershgorin one or a smaller certified Lanczos value
    if (rc != DWH_OK || !(out[3] > 0) || !(out[3] <= out[0]) || !(out[2] == 0.0 || out[3] == out[1])) {
      ++failures;
      std::fprintf(stderr, "FAIL h_bound rc=%d gersh=%g lanczos=%g certified=%g used=%g: %s\n", rc, out[0], out[1],
                   out[2], out[3], dwh::g_create_error.c_str());
    }
  }
  std::printf("plan_main: %d plan configurations, %d failure(s)\n", nconf, failures);
  return failures ? 1 : 0;
}
