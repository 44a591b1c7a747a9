// The checks every dense-map call that takes a scan and a pose makes (fmx::scan_check,
// form_amd/csrc/probe_host.hpp, no HIP headers) under each caller's own text for too many
// points: fmx_dense_integrate's, fmx_carve_rays' and, through probe_check, the probes'.  Only
// that text differs; the order is the pose, the count, the points.  Built by
// __graft_entry__.build() (tests/cpp/scan_check.mk) with the address and undefined-behaviour
// sanitizers linked in statically; tests/test_scan_check_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "probe_host.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double T[12] = {1, 0, 0, 0.5, 0, 1, 0, -2.0, 0, 0, 1, 3.0};
  float pts[8] = {1, 2, 3, 0, 4, 5, 6, 0};
  for (const char* text : {"an integration holds fewer than 2^32 points", "a carve holds fewer than 2^32 points"}) {
    // want: the refusal's text, or null for FMX_OK (which leaves *why alone)
    const auto says = [&](const void* p, unsigned long long n, const double* pose, const char* want) {
      const char* w = nullptr;
      const fmx_status st = fmx::scan_check(p, n, pose, text, &w);
      return want ? st == FMX_E_INVAL && w && std::string(w) == want : st == FMX_OK && w == nullptr;
    };
    CHECK(says(pts, 2, T, nullptr) && says(nullptr, 0, T, nullptr) && says(pts, (1ull << 32) - 1, T, nullptr));
    CHECK(says(pts, 1ull << 32, T, text) && says(nullptr, 1ull << 32, T, text));  // the count before the points
    CHECK(says(nullptr, 2, T, "null points"));
    CHECK(says(nullptr, 1ull << 32, nullptr, "null pose") && says(pts, 2, nullptr, "null pose"));  // the pose first
    for (int k = 0; k < 12; ++k)
      for (double bad : {nan, inf, -inf}) {
        const double keep = T[k];
        T[k] = bad;
        CHECK(says(nullptr, 1ull << 32, T, "non-finite pose") && says(pts, 2, T, "non-finite pose"));
        T[k] = keep;
      }
  }
  // the probes' text, as before the checks were shared
  const char* why = nullptr;
  CHECK(fmx::probe_check(pts, 1ull << 32, T, &why) == FMX_E_INVAL && why &&
        std::string(why) == "a probe holds fewer than 2^32 points");
  why = nullptr;
  CHECK(fmx::probe_check(nullptr, 2, nullptr, &why) == FMX_E_INVAL && why && std::string(why) == "null pose");
  std::puts("scan check ok");
  return 0;
}
