// The host-only parts of loading voxels back into the dense map
// (form_amd/csrc/upload_host.hpp, no HIP headers): the argument checks of fmx_upload_voxels,
// the entry classes and the owner numbers of a call's scan values.  Built by
// __graft_entry__.build() (tests/cpp/upload_host.mk) with the address and undefined-behaviour
// sanitizers linked in statically; tests/test_upload_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "upload_host.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static void arguments() {
  const double xyz[6] = {1, 2, 3, 4, 5, 6};
  const uint32_t misses[2] = {0, 1};
  fmx_voxel_input in{};
  const char* why = nullptr;
  in.xyz = xyz;
  CHECK(fmx::upload_check(&in, 2, true, false, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::upload_check(&in, 2, false, false, &why) == FMX_E_STATE && why);  // the map is off
  why = nullptr;
  CHECK(fmx::upload_check(nullptr, 0, false, false, &why) == FMX_E_STATE && why);  // ... comes first
  why = nullptr;
  CHECK(fmx::upload_check(nullptr, 0, true, true, &why) == FMX_E_INVAL && why);
  in.xyz = nullptr;
  why = nullptr;
  CHECK(fmx::upload_check(&in, 1, true, true, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::upload_check(&in, 0, true, true, &why) == FMX_OK && why == nullptr);  // no entries: nothing to read
  in.xyz = xyz;
  in.misses = misses;
  CHECK(fmx::upload_check(&in, 2, true, true, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::upload_check(&in, 2, true, false, &why) == FMX_E_STATE && why);  // no array to hold them
  why = nullptr;
  CHECK(fmx::upload_check(&in, 0, true, false, &why) == FMX_E_STATE && why);  // ... with no entries too
}

static void classes() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  long long v[3] = {9, 9, 9};
  const uint32_t zero = 0, one = 1, many = 0xFFFFFFFFu;
  const double o[3] = {0.0, 0.0, 0.0};
  CHECK(fmx::upload_classify(o, nullptr, 0.5, v) == 0 && v[0] == 0 && v[1] == 0 && v[2] == 0);  // a world point
  CHECK(fmx::upload_classify(o, &one, 0.5, v) == 0 && fmx::upload_classify(o, &many, 0.5, v) == 0);
  CHECK(fmx::upload_classify(o, &zero, 0.5, v) == 1);
  const double q[3] = {-0.25, 1.0, 2.75};
  CHECK(fmx::upload_classify(q, nullptr, 0.5, v) == 0 && v[0] == -1 && v[1] == 2 && v[2] == 5);
  for (int k = 0; k < 3; ++k)
    for (double bad : {nan, inf, -inf}) {
      double p[3] = {1, 2, 3};
      p[k] = bad;
      CHECK(fmx::upload_classify(p, nullptr, 1.0, v) == 1);
    }
  // the ends of the key range, both signs, per axis: 2^20 - 2 is the last voxel in range
  for (int k = 0; k < 3; ++k)
    for (double sg : {1.0, -1.0}) {
      double p[3] = {0.5, 0.5, 0.5};
      p[k] = sg > 0 ? 1048574.5 : -1048573.5;  // floor: +-(2^20 - 2)
      CHECK(fmx::upload_classify(p, nullptr, 1.0, v) == 0 && v[k] == (long long)(sg * 1048574.0));
      p[k] = sg > 0 ? 1048575.0 : -1048574.5;  // floor: +-(2^20 - 1)
      CHECK(fmx::upload_classify(p, nullptr, 1.0, v) == 3);
      p[k] = sg * 1e300;
      CHECK(fmx::upload_classify(p, nullptr, 1e-300, v) == 3);  // an infinite quotient
    }
}

static void owners() {
  fmx::UploadOwners o;
  const std::vector<uint64_t> scan = {7, 1ull << 40, 7, 0, 0xFFFFFFFFFFFFFFFFull, 1ull << 40};
  CHECK(fmx::upload_owners(scan.data(), scan.size(), 5, &o));
  CHECK((o.scans == std::vector<uint64_t>{0, 7, 1ull << 40, 0xFFFFFFFFFFFFFFFFull}) && o.temp == 9);
  CHECK(o.owner.size() == scan.size());
  for (size_t i = 0; i < scan.size(); ++i) {  // each entry's owner names its scan; all at or past `next`, below temp
    CHECK(o.owner[i] >= 5 && o.owner[i] < o.temp && o.scans[o.owner[i] - 5] == scan[i]);
  }
  // many distinct values (the table of distinct values grows several times), each seen twice
  std::vector<uint64_t> many;
  for (uint64_t k = 0; k < 3000; ++k) many.push_back((k * 0x9E3779B97F4A7C15ull) ^ (k << 40));
  for (uint64_t k = 0; k < 3000; ++k) many.push_back(many[2999 - k]);
  CHECK(fmx::upload_owners(many.data(), many.size(), 100, &o) && o.scans.size() == 3000 && o.temp == 3100);
  for (size_t k = 1; k < o.scans.size(); ++k) CHECK(o.scans[k - 1] < o.scans[k]);
  for (size_t i = 0; i < many.size(); ++i) CHECK(o.owner[i] >= 100 && o.owner[i] < 3100 && o.scans[o.owner[i] - 100] == many[i]);
  // no scan array: one owner, scan 0
  CHECK(fmx::upload_owners(nullptr, 3, 0, &o) && o.scans == std::vector<uint64_t>{0} && o.temp == 1);
  CHECK((o.owner == std::vector<uint32_t>{0, 0, 0}));
  // no entries: nothing drawn
  CHECK(fmx::upload_owners(nullptr, 0, 11, &o) && o.scans.empty() && o.owner.empty() && o.temp == 11);
  CHECK(fmx::upload_owners(scan.data(), 0, 11, &o) && o.scans.empty() && o.temp == 11);
  // exhaustion: the temporary number may be the largest owner, never past it
  CHECK(fmx::upload_owners(scan.data(), scan.size(), fmx::kOwnerMax - 4, &o) && o.temp == 0xFFFFFFFEu);
  CHECK(o.owner[4] == 0xFFFFFFFDu);
  CHECK(!fmx::upload_owners(scan.data(), scan.size(), fmx::kOwnerMax - 3, &o));
  CHECK(!fmx::upload_owners(nullptr, 1, fmx::kOwnerMax, &o));
  CHECK(!fmx::upload_owners(nullptr, 0, fmx::kOwnerMax + 1, &o));
  CHECK(!fmx::upload_owners(nullptr, 1, ~0ull, &o));  // (no wrap in 64 bits either: next is checked first)
}

int main() {
  arguments();
  classes();
  owners();
  std::puts("upload host ok");
  return 0;
}
