// align_host.hpp — the host-only parts of aligning a scan to the dense map (include/fmx/fmx.h,
// fmx_align_system and fmx_align_dense; densemap.hip, the align block): the argument checks,
// the packed 7 x 7 system taken apart into H and g, and the Gauss-Newton loop over a callable
// that evaluates the system at a pose, so that the loop runs without a device.  No device code
// and no HIP header: tests/cpp/test_align_host.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "fmx/fmx.h"
#include "nearest_host.hpp"
#include "pose.hpp"

namespace fmx {

// FMX_OK, or FMX_E_INVAL and *why: NULL params, nearest_check's cases on params' reach and
// max_dist2, a sigma that is not finite and positive.
inline fmx_status align_check(const void* points, unsigned long long n, const double* pose34,
                              const fmx_align_params* prm, const char** why) {
  if (!prm) {
    *why = "null params";
    return FMX_E_INVAL;
  }
  const fmx_status st = nearest_check(points, n, pose34, prm->reach, prm->max_dist2, why);
  if (st != FMX_OK) return st;
  if (!(prm->sigma > 0.0) || !std::isfinite(prm->sigma)) {  // (a NaN fails the comparison)
    *why = "sigma must be finite and > 0";
    return FMX_E_INVAL;
  }
  return FMX_OK;
}

// fmx_align_dense's own: NULL pose_out, a NaN or negative threshold.
inline fmx_status align_loop_check(const double* pose_out, double threshold, const char** why) {
  if (!pose_out) {
    *why = "null pose_out";
    return FMX_E_INVAL;
  }
  if (!(threshold >= 0.0)) {
    *why = "threshold must be a number >= 0";
    return FMX_E_INVAL;
  }
  return FMX_OK;
}

inline uint32_t align_stride(const fmx_align_params& p) { return p.stride ? p.stride : 1u; }
// The points with i % stride == 0 among n.
inline unsigned long long align_kept(unsigned long long n, uint32_t stride) { return (n + stride - 1) / stride; }

// The packed upper 7 x 7 (index r * 7 - r (r - 1) / 2 + (q - r)) into H (6 x 6, both halves)
// and g (column 6).
inline void align_unpack(const double S[29], double H[6][6], double g[6]) {
  for (int r = 0; r < 7; ++r)
    for (int q = r; q < 7; ++q) {
      const double v = S[r * 7 - r * (r - 1) / 2 + (q - r)];
      if (q < 6) H[r][q] = H[q][r] = v;
      else if (r < 6) g[r] = v;
    }
}

// fmx_register_points' loop.  system_at(pose34, S, counts) evaluates the packed system at a
// pose.  FMX_OK with pose_out and *res (may be NULL) written, or FMX_E_STATE with neither
// touched when a system is singular.  Result: fmx_align_result, or fmx_plane_result for the
// point-to-plane system (the same fields over another set of counts).
template <class Result, class SystemAt>
fmx_status align_loop_as(const double pose_init[12], uint32_t max_iters, double threshold, SystemAt&& system_at,
                         double pose_out[12], Result* res, const char** why) {
  fmxh::Pose T;
  std::memcpy(T.m, pose_init, sizeof(T.m));
  Result R{};
  while (R.iters < max_iters) {
    double S[29];
    system_at(T.m, S, &R.counts);
    ++R.iters;
    R.error = S[28];
    double H[6][6], g[6], dx[6];
    align_unpack(S, H, g);
    if (!fmxh::chol_solve6(H, g, dx)) {
      *why = "singular normal equations (too few found points)";
      return FMX_E_STATE;
    }
    T = fmxh::compose(T, fmxh::expmap(dx));
    double n2 = 0.0;
    for (double x : dx) n2 += x * x;
    R.last_step = std::sqrt(n2);
    R.converged = R.last_step < threshold ? 1 : 0;
    if (R.converged) break;
  }
  std::memcpy(pose_out, T.m, sizeof(T.m));
  if (res) *res = R;
  return FMX_OK;
}
template <class SystemAt>
fmx_status align_loop(const double pose_init[12], uint32_t max_iters, double threshold, SystemAt&& system_at,
                      double pose_out[12], fmx_align_result* res, const char** why) {
  return align_loop_as<fmx_align_result>(pose_init, max_iters, threshold, system_at, pose_out, res, why);
}

}  // namespace fmx
