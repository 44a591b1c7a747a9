// carve_host.hpp — the host-only parts of carving the dense map (include/fmx/fmx.h,
// fmx_carve_configure; densemap.hip, the carve block): the parameter check, the origin's
// range rule and the roll's host spill with its miss counts.  No device code and no HIP
// header: tests/cpp/test_carve_host.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "fmx/fmx.h"

namespace fmx {

// fmx_carve_params resolved: the gate's 0 replaced by the dense gate's, stride and every 0 by 1
struct CarveCfg {
  bool on = false;
  double max2 = 0.0;
  uint32_t margin = 0, stride = 1, every = 1;
};

// FMX_OK and *out, or FMX_E_INVAL and *why (out untouched).  dense_max2: the dense gate's
// max_norm_squared.
inline fmx_status carve_check(const fmx_carve_params* p, double dense_max2, CarveCfg* out, const char** why) {
  if (!p) {
    *why = "null carve parameters";
    return FMX_E_INVAL;
  }
  if (!(p->max_norm_squared >= 0.0)) {  // also rejects NaN
    *why = "carve: the gate must be a number >= 0";
    return FMX_E_INVAL;
  }
  CarveCfg c;
  c.on = p->enable != 0;
  c.max2 = p->max_norm_squared == 0.0 ? dense_max2 : p->max_norm_squared;
  c.margin = p->margin;
  c.stride = p->ray_stride ? p->ray_stride : 1;
  c.every = p->every ? p->every : 1;
  *out = c;
  return FMX_OK;
}

// The origin's voxel a_k = floor(t_k / w), the integration's own expression: a launch casts
// rays only if every |a_k| < 2^20 - 1 (in fp64, before any cast; a NaN fails)
inline bool carve_origin_ok(const double pose34[12], double w) {
  for (int k = 0; k < 3; ++k) {
    const double v = std::floor(pose34[4 * k + 3] / w);
    if (!(std::fabs(v) < 1048575.0)) return false;
  }
  return true;
}

// The host spill of the register path's rolls: resolved scan_idx values, not tags (a later
// clear cannot invalidate it), and each voxel's miss count (0 with carving never enabled).
struct Spill {
  std::vector<double> xyz;
  std::vector<uint64_t> scan;
  std::vector<uint32_t> index, hits, misses;
  size_t size() const { return scan.size(); }
  // room for `more` further voxels (may throw std::bad_alloc; nothing changes then)
  void reserve(size_t more) {
    const size_t n = size() + more;
    xyz.reserve(3 * n);
    scan.reserve(n);
    index.reserve(n);
    hits.reserve(n);
    misses.reserve(n);
  }
  // `more` voxels appended (zeroed); returns the first one's position.  Within reserved
  // room this allocates nothing.
  size_t grow(size_t more) {
    const size_t at = size(), n = at + more;
    xyz.resize(3 * n);
    scan.resize(n);
    index.resize(n);
    hits.resize(n);
    misses.resize(n);
    return at;
  }
  // Every voxel to the caller (a null array is skipped), then empty.
  void drain(double* o_xyz, uint64_t* o_scan, uint32_t* o_index, uint32_t* o_hits, uint32_t* o_misses) {
    const size_t n = size();
    if (n) {
      if (o_xyz) std::memcpy(o_xyz, xyz.data(), 3 * n * sizeof(double));
      if (o_scan) std::memcpy(o_scan, scan.data(), n * sizeof(uint64_t));
      if (o_index) std::memcpy(o_index, index.data(), n * sizeof(uint32_t));
      if (o_hits) std::memcpy(o_hits, hits.data(), n * sizeof(uint32_t));
      if (o_misses) std::memcpy(o_misses, misses.data(), n * sizeof(uint32_t));
    }
    xyz.clear();
    scan.clear();
    index.clear();
    hits.clear();
    misses.clear();
  }
};

}  // namespace fmx
