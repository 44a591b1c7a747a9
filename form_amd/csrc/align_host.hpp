// align_host.hpp — the host-only parts of aligning a scan to the dense map (include/fmx/fmx.h,
// fmx_align_system and fmx_align_dense; densemap.hip, the align block): the argument checks,
// the packed 7 x 7 system taken apart into H and g, the Gauss-Newton step and the loop over a
// callable that evaluates the system at a pose, so that the loop runs without a device; and what
// the pose batches built on it share (score_host.hpp, refine_host.hpp): the identity pose and the
// plan of a batch.  No device code
// and no HIP header: tests/cpp/test_align_host.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "fmx/fmx.h"
#include "nearest_host.hpp"
#include "pose.hpp"

namespace fmx {

// The identity pose, row-major [R | t]: where a check or a launch needs a pose and the poses
// proper come from a list.
constexpr double kEye34[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};

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

// The tiling and chunking of a pose batch (fmx_score_plan's and fmx_refine_plan's out, in its
// order): work items of `tile` kept points, chunks of at most chunk_poses poses whose partial
// records (record_bytes each, one per pose and tile) fit partial_bytes.
struct BatchPlan {
  uint32_t kept, tile, tiles, chunk, chunks, cap;
};
constexpr uint32_t kBatchGridCap = 2048;      // blocks of the first launch at the most (k_nearest's cap)
constexpr uint32_t kBatchChunkPoses = 16384;  // poses per chunk at the most
constexpr uint64_t kBatchPartialBytes = 32ull << 20;  // ... and the partial records of a chunk
// n < 2^32 (the caller checked): the kept points fit a word.
inline BatchPlan batch_plan(unsigned long long n, uint32_t stride, uint32_t n_poses, uint32_t tile, uint64_t record_bytes) {
  BatchPlan p{};
  p.kept = (uint32_t)align_kept(n, stride ? stride : 1u);
  p.tile = tile;
  p.tiles = (uint32_t)(((unsigned long long)p.kept + tile - 1) / tile);
  const uint64_t fit = kBatchPartialBytes / record_bytes / (p.tiles ? p.tiles : 1u);
  p.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kBatchChunkPoses, fit));
  p.chunks = p.kept ? (n_poses + p.chunk - 1) / p.chunk : 0u;
  p.cap = kBatchGridCap;
  return p;
}

// One Gauss-Newton step on the packed system S at the pose T: false, with nothing touched, when
// the normal equations are singular; else T <- T * exp(dx), *last_step = |dx| and *converged =
// (|dx| < threshold).  The one step of align_loop_as and of refine_loop (refine_host.hpp): the
// single and the batched loops agree bit for bit because they step here.
inline bool gn_step(const double S[29], fmxh::Pose& T, double threshold, double* last_step, int32_t* converged) {
  double H[6][6], g[6], dx[6];
  align_unpack(S, H, g);
  if (!fmxh::chol_solve6(H, g, dx)) return false;
  T = fmxh::compose(T, fmxh::expmap(dx));
  double n2 = 0.0;
  for (double x : dx) n2 += x * x;
  *last_step = std::sqrt(n2);
  *converged = *last_step < threshold ? 1 : 0;
  return true;
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
    if (!gn_step(S, T, threshold, &R.last_step, &R.converged)) {
      *why = "singular normal equations (too few found points)";
      return FMX_E_STATE;
    }
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
