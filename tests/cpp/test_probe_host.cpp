// The host-only parts of probing the dense map (form_amd/csrc/probe_host.hpp, no HIP
// headers): the argument checks of fmx_probe_points / fmx_probe_rays, the ray origin's range
// rule and the tag -> scan_idx resolution of the per-point results.  Built by
// __graft_entry__.build() (tests/cpp/probe_host.mk) with the address and undefined-behaviour
// sanitizers linked in statically; tests/test_probe_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "probe_host.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static void arguments() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double T[12] = {1, 0, 0, 0.5, 0, 1, 0, -2.0, 0, 0, 1, 3.0};
  float pts[8] = {1, 2, 3, 0, 4, 5, 6, 0};
  const char* why = nullptr;
  CHECK(fmx::probe_check(pts, 2, T, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::probe_check(nullptr, 0, T, &why) == FMX_OK && why == nullptr);  // no points: nothing to read
  CHECK(fmx::probe_check(pts, 2, nullptr, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::probe_check(nullptr, 1, T, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::probe_check(pts, 1ull << 32, T, &why) == FMX_E_INVAL && why);
  CHECK(fmx::probe_check(pts, (1ull << 32) - 1, T, &why) == FMX_OK);
  for (int k = 0; k < 12; ++k)
    for (double bad : {nan, inf, -inf}) {
      const double keep = T[k];
      T[k] = bad;
      why = nullptr;
      CHECK(fmx::probe_check(pts, 2, T, &why) == FMX_E_INVAL && why);
      T[k] = keep;
    }
  // the filter: min_hits 0 is 1, the fraction passes through
  fmx::ProbeFilter f = fmx::probe_filter(0, 0, 0);
  CHECK(f.min_hits == 1 && f.num == 0 && f.den == 0);
  f = fmx::probe_filter(0xFFFFFFFFu, 32768, 65536);
  CHECK(f.min_hits == 0xFFFFFFFFu && f.num == 32768 && f.den == 65536);
}

static void origin() {
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  // the carve's rule, value for value
  for (double x : {0.0, 1048574.5, 1048575.0, -1048574.5, -1048574.0, 1e300, -1e300})
    for (double w : {1.0, 0.2, 0.5}) {
      T[3] = x;
      CHECK(fmx::probe_origin_ok(T, w) == fmx::carve_origin_ok(T, w));
    }
  T[3] = 1048574.5;  // a_x = 2^20 - 2: the last one in range
  CHECK(fmx::probe_origin_ok(T, 1.0));
  T[3] = 1048575.0;
  CHECK(!fmx::probe_origin_ok(T, 1.0));
  T[3] = 0.0;
  T[7] = std::numeric_limits<double>::quiet_NaN();
  CHECK(!fmx::probe_origin_ok(T, 1.0));
}

static void resolve() {
  const std::vector<uint64_t> seq_scan = {1ull << 40, 7, 0xFFFFFFFFFFFFFFFFull};
  const uint8_t state[6] = {FMX_PROBE_ABSENT, FMX_PROBE_FILTERED, FMX_PROBE_SOLID, FMX_PROBE_OUT_OF_RANGE,
                            FMX_PROBE_INVALID, FMX_PROBE_SOLID};
  // (a tag where no voxel is reported is not looked at: give those an integration nobody knows)
  const unsigned long long tag[6] = {(99ull << 32) | 5, (1ull << 32) | 11, (0ull << 32) | 0xFFFFFFFFull,
                                     (99ull << 32) | 6, ~0ull, (2ull << 32) | 3};
  std::vector<uint64_t> scan(7, 0xAAAAAAAAAAAAAAAAull);
  std::vector<uint32_t> index(7, 0xBBBBBBBBu);
  CHECK(fmx::probe_resolve(state, tag, 6, seq_scan, scan.data(), index.data()));
  CHECK(scan[0] == 0 && index[0] == 0 && scan[3] == 0 && index[3] == 0 && scan[4] == 0 && index[4] == 0);
  CHECK(scan[1] == 7 && index[1] == 11 && scan[2] == (1ull << 40) && index[2] == 0xFFFFFFFFu);
  CHECK(scan[5] == 0xFFFFFFFFFFFFFFFFull && index[5] == 3);
  CHECK(scan[6] == 0xAAAAAAAAAAAAAAAAull && index[6] == 0xBBBBBBBBu);  // exactly n entries
  // either output alone; none; no points
  std::vector<uint64_t> only_scan(6, 1);
  std::vector<uint32_t> only_index(6, 1);
  CHECK(fmx::probe_resolve(state, tag, 6, seq_scan, only_scan.data(), nullptr) && only_scan == std::vector<uint64_t>(scan.begin(), scan.begin() + 6));
  CHECK(fmx::probe_resolve(state, tag, 6, seq_scan, nullptr, only_index.data()) && only_index[1] == 11 && only_index[0] == 0);
  CHECK(fmx::probe_resolve(state, tag, 6, seq_scan, nullptr, nullptr));
  CHECK(fmx::probe_resolve(nullptr, nullptr, 0, seq_scan, nullptr, nullptr));
  // a reported voxel whose integration the table does not hold: refused, not read out of bounds
  const uint8_t one[1] = {FMX_PROBE_FILTERED};
  const unsigned long long far[1] = {3ull << 32};
  uint64_t s1 = 42;
  CHECK(!fmx::probe_resolve(one, far, 1, seq_scan, &s1, nullptr) && s1 == 42);
  CHECK(!fmx::probe_resolve(one, far, 1, std::vector<uint64_t>{}, &s1, nullptr));
  CHECK(fmx::probe_reports_voxel(FMX_PROBE_SOLID) && fmx::probe_reports_voxel(FMX_PROBE_FILTERED));
  CHECK(!fmx::probe_reports_voxel(FMX_PROBE_ABSENT) && !fmx::probe_reports_voxel(FMX_PROBE_INVALID) &&
        !fmx::probe_reports_voxel(FMX_PROBE_OUT_OF_RANGE) && !fmx::probe_reports_voxel(200));
}

int main() {
  arguments();
  origin();
  resolve();
  std::puts("probe host ok");
  return 0;
}
