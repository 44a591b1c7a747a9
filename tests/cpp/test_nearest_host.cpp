// The host-only parts of the dense map's nearest-voxel search (form_amd/csrc/nearest_host.hpp,
// no HIP headers): the argument checks of fmx_nearest_voxels, the cube's offsets in shell order
// and the number of storable cells of a cube.  Built by __graft_entry__.build()
// (tests/cpp/nearest_host.mk) with the address and undefined-behaviour sanitizers linked in
// statically; tests/test_nearest_cpu.py runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <vector>

#include "nearest_host.hpp"

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
  CHECK(fmx::nearest_check(pts, 2, T, 1, 1.0, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::nearest_check(pts, 2, T, 0, 0.0, &why) == FMX_OK);  // the own voxel, coincident points
  CHECK(fmx::nearest_check(pts, 2, T, FMX_NEAREST_MAX_REACH, inf, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::nearest_check(nullptr, 0, T, 1, inf, &why) == FMX_OK && why == nullptr);  // no points: nothing to read
  CHECK(fmx::nearest_check(pts, 2, T, FMX_NEAREST_MAX_REACH + 1, 1.0, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::nearest_check(pts, 2, T, 0xFFFFFFFFu, 1.0, &why) == FMX_E_INVAL && why);
  for (double bad : {nan, -1.0, -inf, -std::numeric_limits<double>::denorm_min()}) {
    why = nullptr;
    CHECK(fmx::nearest_check(pts, 2, T, 1, bad, &why) == FMX_E_INVAL && why);
  }
  CHECK(fmx::nearest_check(pts, 2, T, 1, -0.0, &why) == FMX_OK);
  // the probes' cases, unchanged
  why = nullptr;
  CHECK(fmx::nearest_check(pts, 2, nullptr, 1, 1.0, &why) == FMX_E_INVAL && why);
  CHECK(fmx::nearest_check(nullptr, 1, T, 1, 1.0, &why) == FMX_E_INVAL);
  CHECK(fmx::nearest_check(pts, 1ull << 32, T, 1, 1.0, &why) == FMX_E_INVAL);
  CHECK(fmx::nearest_check(pts, (1ull << 32) - 1, T, 1, 1.0, &why) == FMX_OK);
  T[7] = nan;
  CHECK(fmx::nearest_check(pts, 2, T, 1, 1.0, &why) == FMX_E_INVAL);
}

static void offsets() {
  for (uint32_t reach = 0; reach <= FMX_NEAREST_MAX_REACH; ++reach) {
    const std::vector<uint32_t> o = fmx::nearest_offsets(reach);
    const uint32_t side = 2 * reach + 1;
    CHECK(o.size() == (size_t)side * side * side && o.size() == fmx::nearest_shell_begin(reach + 1));
    std::set<uint32_t> seen(o.begin(), o.end());
    CHECK(seen.size() == o.size());  // every cell once
    for (uint32_t s = 0; s <= reach; ++s)
      for (uint32_t at = fmx::nearest_shell_begin(s); at < fmx::nearest_shell_begin(s + 1); ++at) {
        int d[3];
        fmx::nearest_unpack(o[at], d);
        CHECK(std::max({std::abs(d[0]), std::abs(d[1]), std::abs(d[2])}) == (int)s);
        CHECK(fmx::nearest_pack(d[0], d[1], d[2]) == o[at]);
      }
  }
  // a shorter list is a prefix of the longest: the kernel reads the one built for the maximum
  const std::vector<uint32_t> all = fmx::nearest_offsets(FMX_NEAREST_MAX_REACH), two = fmx::nearest_offsets(2);
  CHECK(all.size() == 4913 && std::equal(two.begin(), two.end(), all.begin()));
  CHECK(fmx::nearest_shell_begin(0) == 0 && fmx::nearest_shell_begin(1) == 1 && fmx::nearest_shell_begin(2) == 27 &&
        fmx::nearest_shell_begin(9) == 4913);
  int d[3];
  fmx::nearest_unpack(all[0], d);
  CHECK(d[0] == 0 && d[1] == 0 && d[2] == 0);
}

static uint64_t cells_by_loop(const int c[3], int reach) {
  uint64_t m = 0;
  const long long lim = (1ll << 20) - 1;
  for (int x = -reach; x <= reach; ++x)
    for (int y = -reach; y <= reach; ++y)
      for (int z = -reach; z <= reach; ++z)
        m += std::llabs((long long)c[0] + x) < lim && std::llabs((long long)c[1] + y) < lim && std::llabs((long long)c[2] + z) < lim;
  return m;
}

static void cells() {
  const int e = (1 << 20) - 2;  // the last storable coordinate
  const int cs[][3] = {{0, 0, 0}, {e, 0, 0}, {e, -e, e}, {e - 1, 5, -e + 3}, {-e, -e, -e}, {e - 8, e - 7, 0}};
  for (const auto& c : cs)
    for (int reach = 0; reach <= FMX_NEAREST_MAX_REACH; ++reach)
      CHECK(fmx::nearest_cube_cells(c, (uint32_t)reach) == cells_by_loop(c, reach));
  const int o[3] = {0, 0, 0}, edge[3] = {e, 0, 0};
  CHECK(fmx::nearest_cube_cells(o, 8) == 4913 && fmx::nearest_cube_cells(o, 0) == 1);
  CHECK(fmx::nearest_cube_cells(edge, 2) == 3 * 5 * 5);
}

int main() {
  arguments();
  offsets();
  cells();
  std::puts("nearest host ok");
  return 0;
}
