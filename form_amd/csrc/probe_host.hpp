// probe_host.hpp — the host-only parts of probing the dense map (include/fmx/fmx.h,
// fmx_probe_points; densemap.hip, the probe block; called from dense_api.cpp): the argument
// checks (the scan-and-pose part of them also fmx_dense_integrate's and fmx_carve_rays'), the
// ray origin's range rule and the tag -> scan_idx resolution of the per-point results.  No
// device code and no HIP header: tests/cpp/test_probe_host.cpp builds it alone, under the
// host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "carve_host.hpp"
#include "fmx/fmx.h"

namespace fmx {

// The checks every call that takes a scan and a pose makes, in this order.  FMX_OK, or
// FMX_E_INVAL and *why: a NULL or non-finite pose, 2^32 points or more (too_many: the call's
// own text for that), NULL points with n > 0.
inline fmx_status scan_check(const void* points, unsigned long long n, const double* pose34, const char* too_many,
                             const char** why) {
  if (!pose34) {
    *why = "null pose";
    return FMX_E_INVAL;
  }
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(pose34[k])) {
      *why = "non-finite pose";
      return FMX_E_INVAL;
    }
  if (n >= (1ull << 32)) {
    *why = too_many;
    return FMX_E_INVAL;
  }
  if (n && !points) {
    *why = "null points";
    return FMX_E_INVAL;
  }
  return FMX_OK;
}
// The probes' (and, through nearest_check and align_check, the search's and the alignment's).
inline fmx_status probe_check(const void* points, unsigned long long n, const double* pose34, const char** why) {
  return scan_check(points, n, pose34, "a probe holds fewer than 2^32 points", why);
}

// A ray cast starts in the voxel of the pose's translation: the carve's rule, unchanged.
inline bool probe_origin_ok(const double pose34[12], double w) { return carve_origin_ok(pose34, w); }

// The filter as the kernels take it: min_hits 0 is 1.
struct ProbeFilter {
  uint32_t min_hits, num, den;
};
inline ProbeFilter probe_filter(uint32_t min_hits, uint32_t miss_num, uint32_t miss_den) {
  return ProbeFilter{min_hits ? min_hits : 1u, miss_num, miss_den};
}

inline bool probe_reports_voxel(uint8_t state) { return state == FMX_PROBE_FILTERED || state == FMX_PROBE_SOLID; }

// Per point: the tag (integration number << 32 | input index) of the voxel it reports to
// (scan_idx, index) through the host's integration -> scan_idx table; zeros where the state
// reports no voxel (the tag word is then not looked at).  Either output may be NULL.  False,
// nothing further written, when a tag names an integration the table does not hold.
inline bool probe_resolve(const uint8_t* state, const unsigned long long* tag, size_t n,
                          const std::vector<uint64_t>& seq_scan, uint64_t* scan, uint32_t* index) {
  for (size_t i = 0; i < n; ++i) {
    const bool have = probe_reports_voxel(state[i]);
    const size_t seq = have ? (size_t)(tag[i] >> 32) : 0;
    if (have && seq >= seq_scan.size()) return false;
    if (scan) scan[i] = have ? seq_scan[seq] : 0;
    if (index) index[i] = have ? (uint32_t)tag[i] : 0u;
  }
  return true;
}

}  // namespace fmx
