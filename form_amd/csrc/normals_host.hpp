// normals_host.hpp — the host-only parts of the dense map's surface normals and of the
// point-to-plane alignment that reads them (include/fmx/fmx.h, fmx_normals_* and fmx_plane_*;
// densemap.hip, the normals block): the argument checks, the support threshold, what a
// download takes from the build's counts and the plane system's counts.  No device code and no HIP header:
// tests/cpp/test_normals_host.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "fmx/fmx.h"
#include "align_host.hpp"

namespace fmx {

// FMX_OK, or FMX_E_INVAL and *why: NULL params, a reach of 0 (the own cell alone supports
// nothing) or past FMX_NEAREST_MAX_REACH, a NaN or negative max_dist2, a max_flatness that is
// not finite and in [0, 1].
inline fmx_status normals_check(const fmx_normals_params* prm, const char** why) {
  if (!prm) {
    *why = "null params";
    return FMX_E_INVAL;
  }
  if (prm->reach < 1u || prm->reach > (uint32_t)FMX_NEAREST_MAX_REACH) {
    *why = "reach is in [1, FMX_NEAREST_MAX_REACH]";
    return FMX_E_INVAL;
  }
  if (!(prm->max_dist2 >= 0.0)) {  // (a NaN fails the comparison)
    *why = "max_dist2 must be a number >= 0";
    return FMX_E_INVAL;
  }
  if (!(prm->max_flatness >= 0.0 && prm->max_flatness <= 1.0)) {
    *why = "max_flatness must be in [0, 1]";
    return FMX_E_INVAL;
  }
  return FMX_OK;
}

// Values below 3 read as 3: two points fix no plane.
inline uint32_t normals_min_support(const fmx_normals_params& p) { return p.min_support < 3u ? 3u : p.min_support; }

// What a download takes, from the build's counts: the solid voxels (every class but filtered),
// or the oriented ones.
inline uint64_t normals_take(const fmx_normals_counts& k, bool oriented_only) {
  return oriented_only ? (uint64_t)k.oriented : (uint64_t)k.oriented + k.flat_rejected + k.sparse;
}

// The plane system's six classes from the kernel's counters {found (oriented winners), none,
// out_of_range, invalid, lookups, unoriented} over n points on the stride.
inline fmx_plane_counts plane_counts(const unsigned long long k[6], unsigned long long n, uint32_t stride) {
  return fmx_plane_counts{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3],
                          (uint32_t)(n - align_kept(n, stride)), (uint32_t)k[5], k[4]};
}

}  // namespace fmx
