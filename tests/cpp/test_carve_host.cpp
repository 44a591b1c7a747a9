// The host-only parts of carving (form_amd/csrc/carve_host.hpp, no HIP headers): the
// parameter check of fmx_carve_configure, the origin's range rule and the roll's host spill
// with its miss counts.  Built by __graft_entry__.build() (tests/cpp/carve_host.mk) with the
// address and undefined-behaviour sanitizers linked in statically; tests/test_carve_cpu.py
// runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "carve_host.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static void params() {
  using fmx::CarveCfg;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const char* why = nullptr;
  CarveCfg c;
  c.margin = 77;
  CHECK(fmx::carve_check(nullptr, 1e4, &c, &why) == FMX_E_INVAL && why && c.margin == 77);
  for (double gate : {nan, -1.0, -inf, -1e-300}) {
    fmx_carve_params p{1, gate, 3, 4, 5};
    why = nullptr;
    CHECK(fmx::carve_check(&p, 1e4, &c, &why) == FMX_E_INVAL && why && c.margin == 77);  // (out untouched)
  }
  fmx_carve_params p{1, 0.0, 0, 0, 0};
  CHECK(fmx::carve_check(&p, 1e4, &c, &why) == FMX_OK);
  CHECK(c.on && c.max2 == 1e4 && c.margin == 0 && c.stride == 1 && c.every == 1);  // 0: the dense gate's; 0 = 1
  p = fmx_carve_params{0, 25.0, 0xFFFFFFFFu, 3, 7};
  CHECK(fmx::carve_check(&p, 1e4, &c, &why) == FMX_OK);
  CHECK(!c.on && c.max2 == 25.0 && c.margin == 0xFFFFFFFFu && c.stride == 3 && c.every == 7);
  p = fmx_carve_params{-5, inf, 1, 1, 1};  // any nonzero enables; an infinite gate gates nothing
  CHECK(fmx::carve_check(&p, 1e4, &c, &why) == FMX_OK && c.on && c.max2 == inf);
}

static void origin() {
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  CHECK(fmx::carve_origin_ok(T, 0.2));
  T[3] = 1048574.5;  // a_x = 2^20 - 2: the last one in range
  CHECK(fmx::carve_origin_ok(T, 1.0));
  T[3] = 1048575.0;
  CHECK(!fmx::carve_origin_ok(T, 1.0));
  T[3] = -1048574.5;  // floor: -(2^20 - 1)
  CHECK(!fmx::carve_origin_ok(T, 1.0));
  T[3] = -1048574.0;
  CHECK(fmx::carve_origin_ok(T, 1.0));
  T[3] = 0.0;
  T[11] = 1e300;
  CHECK(!fmx::carve_origin_ok(T, 1e-3));
  T[11] = std::numeric_limits<double>::quiet_NaN();
  CHECK(!fmx::carve_origin_ok(T, 1.0));
  T[11] = 3.0;
  T[7] = 0.5 * 1048575.0;  // the width scales the range
  CHECK(fmx::carve_origin_ok(T, 1.0) && !fmx::carve_origin_ok(T, 0.5) && fmx::carve_origin_ok(T, 0.5000001));
}

static void fill(fmx::Spill& sp, size_t at, size_t n, uint32_t tag) {
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) sp.xyz[3 * (at + i) + k] = (double)tag + 0.25 * k + (double)i;
    sp.scan[at + i] = ((uint64_t)tag << 32) + i;
    sp.index[at + i] = tag * 1000u + (uint32_t)i;
    sp.hits[at + i] = 1u + (uint32_t)i;
    sp.misses[at + i] = tag + 7u * (uint32_t)i;
  }
}

static void spill() {
  fmx::Spill sp;
  CHECK(sp.size() == 0);
  sp.drain(nullptr, nullptr, nullptr, nullptr, nullptr);  // empty: nothing to copy, nothing to free twice
  // three rolls: reserve, then grow within the reserved room (no reallocation), then fill
  size_t total = 0;
  for (uint32_t roll = 1; roll <= 3; ++roll) {
    const size_t n = 100 * roll + 1;
    sp.reserve(n);
    const double* before = sp.xyz.data();
    const uint32_t* mbefore = sp.misses.data();
    const size_t at = sp.grow(n);
    CHECK(at == total && sp.size() == total + n);
    CHECK(sp.xyz.data() == before && sp.misses.data() == mbefore);
    CHECK(sp.misses[at] == 0 && sp.misses[at + n - 1] == 0);  // appended zeroed
    fill(sp, at, n, roll);
    total += n;
  }
  sp.grow(0);
  CHECK(sp.size() == total && sp.xyz.size() == 3 * total && sp.misses.size() == total);
  // a drain with some arrays left out: exactly `total` entries written to the others
  std::vector<double> xyz(3 * total + 3, -1.0);
  std::vector<uint32_t> hits(total + 1, 0xAAAAAAAAu), misses(total + 1, 0xBBBBBBBBu);
  sp.drain(xyz.data(), nullptr, nullptr, hits.data(), misses.data());
  CHECK(sp.size() == 0 && sp.misses.empty() && sp.xyz.empty());
  CHECK(xyz[3 * total] == -1.0 && hits[total] == 0xAAAAAAAAu && misses[total] == 0xBBBBBBBBu);
  CHECK(misses[0] == 1 && misses[1] == 8 && hits[100] == 101 && misses[101] == 2 && misses[101 + 201] == 3);
  CHECK(xyz[0] == 1.0 && xyz[1] == 1.25 && xyz[3 * 101 + 2] == 2.5);
  // refilled after a drain; every array out
  sp.reserve(5);
  fill(sp, sp.grow(5), 5, 9);
  std::vector<uint64_t> scan(5);
  std::vector<uint32_t> index(5);
  xyz.assign(15, 0.0);
  hits.assign(5, 0);
  misses.assign(5, 0);
  sp.drain(xyz.data(), scan.data(), index.data(), hits.data(), misses.data());
  CHECK(scan[4] == ((9ull << 32) + 4) && index[4] == 9004 && hits[4] == 5 && misses[4] == 9 + 28 && xyz[14] == 9.5 + 4.0);
  CHECK(sp.size() == 0);
}

int main() {
  params();
  origin();
  spill();
  std::puts("carve host ok");
  return 0;
}
