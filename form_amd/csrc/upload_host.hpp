// upload_host.hpp — the host-only parts of loading voxels back into the dense map
// (include/fmx/fmx.h, fmx_upload_voxels; densemap.hip, the upload block): the argument checks,
// the entry classes and the owner numbers that a call's scan values get.  No device code and
// no HIP header: tests/cpp/test_upload_host.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "fmx/fmx.h"

namespace fmx {

// The largest owner number a tag may carry: (0xFFFFFFFF << 32 | 0xFFFFFFFF) is the empty tag.
constexpr uint64_t kOwnerMax = 0xFFFFFFFEull;

// FMX_OK, or the status and *why.  on: the dense map is configured and enabled; carve_have:
// the miss array exists (carving has been enabled on this map at least once).
inline fmx_status upload_check(const fmx_voxel_input* in, uint32_t n, bool on, bool carve_have, const char** why) {
  if (!on) {
    *why = "the dense map is not enabled (fmx_dense_configure)";
    return FMX_E_STATE;
  }
  if (!in) {
    *why = "null voxel input";
    return FMX_E_INVAL;
  }
  if (n && !in->xyz) {
    *why = "null voxel points";
    return FMX_E_INVAL;
  }
  if (in->misses && !carve_have) {
    *why = "upload: misses given, but carving has never been enabled on this map (fmx_carve_configure)";
    return FMX_E_STATE;
  }
  return FMX_OK;
}

// The class of one entry, as the device's claim decides it: 0 valid (v its voxel), 1 invalid,
// 3 out of range.  hits: null (1 for every entry) or the entry's count.
inline int upload_classify(const double xyz[3], const uint32_t* hits, double w, long long v[3]) {
  if (!(std::isfinite(xyz[0]) && std::isfinite(xyz[1]) && std::isfinite(xyz[2])) || (hits && *hits == 0)) return 1;
  double c[3];
  for (int k = 0; k < 3; ++k) c[k] = std::floor(xyz[k] / w);
  // in fp64, before the cast (an infinite quotient fails the comparison)
  if (!(std::fabs(c[0]) < 1048575.0 && std::fabs(c[1]) < 1048575.0 && std::fabs(c[2]) < 1048575.0)) return 3;
  for (int k = 0; k < 3; ++k) v[k] = (long long)c[k];
  return 0;
}

// The owner numbers of one call.  A tag's high word names an owner: an integration, or one
// distinct scan value of an upload, all drawn from one rising sequence whose next free number
// is `next`.  The call's distinct scan values, ascending, get next, next + 1, ...; `temp`, the
// number after them, is the one the claim's temporary tags carry (larger than every resident
// owner, gone from the table when the call ends, so the next call or integration may have it).
struct UploadOwners {
  std::vector<uint64_t> scans;  // distinct, ascending: owner next + k is scans[k]
  std::vector<uint32_t> owner;  // per entry
  uint32_t temp = 0;
};
// False, *out unspecified, when the numbering would be exhausted (temp past kOwnerMax).
// scan: n values, or null (0 for every entry).  May throw std::bad_alloc.
// One pass over the entries with a growing open-addressed table of the distinct values (a
// spill names a few hundred scans in a million entries: the table stays in cache), then a
// sort of the distinct values alone.
inline bool upload_owners(const uint64_t* scan, size_t n, uint64_t next, UploadOwners* out) {
  out->scans.clear();
  out->owner.assign(n, 0u);  // first: each entry's distinct value in first-seen order
  std::vector<uint64_t> seen;
  if (scan && n) {
    std::vector<uint64_t> key(1024);
    std::vector<uint32_t> val(1024, 0u);  // 0: empty, else the value's place in `seen` + 1
    const auto home = [](uint64_t k, size_t mask) {  // the splitmix64 finalizer
      k ^= k >> 30;
      k *= 0xBF58476D1CE4E5B9ull;
      k ^= k >> 27;
      k *= 0x94D049BB133111EBull;
      k ^= k >> 31;
      return (size_t)k & mask;
    };
    for (size_t i = 0; i < n; ++i) {
      if (2 * (seen.size() + 1) > key.size()) {  // load at most 1/2: a probe meets an empty slot
        std::vector<uint64_t> k2(2 * key.size());
        std::vector<uint32_t> v2(2 * key.size(), 0u);
        for (size_t s = 0; s < seen.size(); ++s) {
          size_t h = home(seen[s], k2.size() - 1);
          while (v2[h]) h = (h + 1) & (k2.size() - 1);
          k2[h] = seen[s];
          v2[h] = (uint32_t)s + 1;
        }
        key.swap(k2);
        val.swap(v2);
      }
      const size_t mask = key.size() - 1;
      size_t h = home(scan[i], mask);
      while (val[h] && key[h] != scan[i]) h = (h + 1) & mask;
      if (!val[h]) {
        key[h] = scan[i];
        seen.push_back(scan[i]);
        val[h] = (uint32_t)seen.size();
      }
      out->owner[i] = val[h] - 1;
    }
  } else if (n) {
    seen.push_back(0);
  }
  const uint64_t temp = next + seen.size();
  if (next > kOwnerMax || temp > kOwnerMax) return false;
  out->temp = (uint32_t)temp;
  std::vector<uint32_t> order(seen.size()), rank(seen.size());
  for (size_t s = 0; s < seen.size(); ++s) order[s] = (uint32_t)s;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return seen[a] < seen[b]; });
  out->scans.resize(seen.size());
  for (size_t k = 0; k < order.size(); ++k) {
    out->scans[k] = seen[order[k]];
    rank[order[k]] = (uint32_t)k;
  }
  for (size_t i = 0; i < n; ++i) out->owner[i] = (uint32_t)(next + rank[out->owner[i]]);
  return true;
}

}  // namespace fmx
