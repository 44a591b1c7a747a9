// nearest_host.hpp — the host-only parts of the dense map's nearest-voxel search
// (include/fmx/fmx.h, fmx_nearest_voxels; densemap.hip, the nearest block): the argument
// checks, the cube's offsets in shell order as the kernel reads them, and the number of
// storable cells of a voxel's cube, which bounds the call's `lookups`.  No device code and no
// HIP header: tests/cpp/test_nearest_host.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "fmx/fmx.h"
#include "probe_host.hpp"

namespace fmx {

// FMX_OK, or FMX_E_INVAL and *why: probe_check's cases, a reach past FMX_NEAREST_MAX_REACH, a
// NaN or negative max_dist2 (+inf: no limit; 0: coincident points only).
inline fmx_status nearest_check(const void* points, unsigned long long n, const double* pose34, uint32_t reach,
                                double max_dist2, const char** why) {
  const fmx_status st = probe_check(points, n, pose34, why);
  if (st != FMX_OK) return st;
  if (reach > (uint32_t)FMX_NEAREST_MAX_REACH) {
    *why = "reach is at most FMX_NEAREST_MAX_REACH";
    return FMX_E_INVAL;
  }
  if (!(max_dist2 >= 0.0)) {  // (a NaN fails the comparison)
    *why = "max_dist2 must be a number >= 0";
    return FMX_E_INVAL;
  }
  return FMX_OK;
}

// Shell s = max |d_k| of the cube is the index range [nearest_shell_begin(s), nearest_shell_begin(s + 1))
// of the offset list.
inline uint32_t nearest_shell_begin(uint32_t s) { return s ? (2 * s - 1) * (2 * s - 1) * (2 * s - 1) : 0u; }

// One offset as the kernel unpacks it: d_k + FMX_NEAREST_MAX_REACH in byte k.
inline uint32_t nearest_pack(int dx, int dy, int dz) {
  const int b = FMX_NEAREST_MAX_REACH;
  return (uint32_t)(dx + b) | ((uint32_t)(dy + b) << 8) | ((uint32_t)(dz + b) << 16);
}
inline void nearest_unpack(uint32_t o, int d[3]) {
  const int b = FMX_NEAREST_MAX_REACH;
  d[0] = (int)(o & 255u) - b, d[1] = (int)((o >> 8) & 255u) - b, d[2] = (int)((o >> 16) & 255u) - b;
}

// The (2 reach + 1)^3 offsets with every |d_k| <= reach, sorted by shell (the order inside a
// shell is of no account: ties go by key, not by visit order).
inline std::vector<uint32_t> nearest_offsets(uint32_t reach) {
  std::vector<uint32_t> out;
  const int r = (int)reach;
  out.reserve((size_t)nearest_shell_begin(reach + 1));
  for (int s = 0; s <= r; ++s)
    for (int dx = -s; dx <= s; ++dx)
      for (int dy = -s; dy <= s; ++dy) {
        const bool face = dx == -s || dx == s || dy == -s || dy == s;
        for (int dz = -s; dz <= s; dz += (face || s == 0) ? 1 : 2 * s) out.push_back(nearest_pack(dx, dy, dz));
      }
  return out;
}

// The cells c + d, every |d_k| <= reach, that can be stored (every coordinate |.| < 2^20 - 1)
// for an own voxel c that is itself in range: the definition's number of candidates.
inline uint64_t nearest_cube_cells(const int c[3], uint32_t reach) {
  const long long lim = (1ll << 20) - 2;  // the largest storable |coordinate|
  uint64_t cells = 1;
  for (int k = 0; k < 3; ++k) {
    long long lo = (long long)c[k] - (long long)reach, hi = (long long)c[k] + (long long)reach;
    if (lo < -lim) lo = -lim;
    if (hi > lim) hi = lim;
    cells *= hi >= lo ? (uint64_t)(hi - lo + 1) : 0ull;
  }
  return cells;
}

}  // namespace fmx
