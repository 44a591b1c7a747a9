// refine_host.hpp — the host-only parts of refining many candidate poses of a scan against the
// dense map (include/fmx/fmx.h, fmx_refine_systems, fmx_refine_poses and fmx_refine_plan;
// densemap.hip, the refine block): the argument checks on top of score_check and align_check,
// the plan (align_host.hpp's batch_plan at the refine tile and record) and the lockstep
// Gauss-Newton loop over a callable that evaluates the systems of a list of poses, so that the
// loop runs without a device.  No device code and no HIP header: tests/cpp/test_refine_host.cpp
// builds it alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "align_host.hpp"
#include "fmx/fmx.h"
#include "pose.hpp"
#include "score_host.hpp"

namespace fmx {

// Kept points per work item: FMX_REFINE_TILE / 256 block-wide passes with the 28 sums kept in
// registers over them, one reduction per item.  256, one pass: against 1024 it is as fast at
// 1024 poses and more than twice as fast at 1 to 8, where a 4096-point scan is 16 items, not 4
// (DESIGN.md §Dense map, Refining; profiles/refine_tile_ab.json).
#ifndef FMX_REFINE_TILE
#define FMX_REFINE_TILE 256
#endif
constexpr uint32_t kRefineTile = FMX_REFINE_TILE;
static_assert(kRefineTile >= 256 && kRefineTile % 256 == 0, "a tile is a whole number of block-wide passes");

// One (pose, tile) partial record, written whole by the item's block.
struct RefinePart {
  double S[28];
  uint32_t cnt[5];  // found, none, out_of_range, invalid, unoriented
  uint32_t reserved;
  unsigned long long lookups;
};
static_assert(sizeof(RefinePart) == 256, "a partial record is 256 bytes");
static_assert(sizeof(fmx_refine_system) == 264, "a system record is 264 bytes");
static_assert(sizeof(fmx_refine_result) == 64, "a result record is 64 bytes");
static_assert(FMX_REFINE_MAX_POSES == FMX_SCORE_MAX_POSES, "score_check's limit is this one");

// FMX_OK, or FMX_E_INVAL and *why: n_poses past FMX_REFINE_MAX_POSES, then score_check's cases
// (NULL params, NULL poses or out with n_poses > 0, a non-finite entry of any pose, align_check's
// on the points, n, reach, max_dist2 and sigma).  out: the systems, or the loop's poses_out.
inline fmx_status refine_check(const void* points, unsigned long long n, const double* poses34, unsigned long long n_poses,
                               const fmx_align_params* prm, const void* out, const char** why) {
  if (n_poses > (unsigned long long)FMX_REFINE_MAX_POSES) {
    *why = "n_poses is at most FMX_REFINE_MAX_POSES";
    return FMX_E_INVAL;
  }
  const fmx_status st = score_check(points, n, poses34, n_poses, prm, out, why);
  if (st != FMX_OK && prm && n_poses && poses34 && !out) *why = "null output";
  return st;
}
// fmx_refine_poses' own: align_loop_check's threshold rule.
inline fmx_status refine_loop_check(double threshold, const char** why) {
  const double any[12] = {};
  return align_loop_check(any, threshold, why);
}

// The plan of a call (align_host.hpp, batch_plan).
using RefinePlan = BatchPlan;
inline RefinePlan refine_plan(unsigned long long n, uint32_t stride, uint32_t n_poses) {
  return batch_plan(n, stride, n_poses, kRefineTile, sizeof(RefinePart));
}

// align_loop_as's recurrence for n_poses poses in lockstep.  systems_at(poses, count, records)
// evaluates the systems of `count` poses (12 doubles each) into `count` records; each round it
// gets the poses still running, in list order.  Pose k steps with align_loop_as's gn_step, so
// that its pose and result are what the one-pose loop gives.  A singular
// system ends its pose: singular = 1, poses_out[k] = poses_init[k].  poses_out and results (may
// be NULL) are written at the end; may throw std::bad_alloc before the first evaluation.
template <class SystemsAt>
void refine_loop(const double* poses_init, uint32_t n_poses, uint32_t max_iters, double threshold, SystemsAt&& systems_at,
                 double* poses_out, fmx_refine_result* results) {
  std::vector<fmxh::Pose> T(n_poses);
  std::vector<fmx_refine_result> R(n_poses);  // (value-initialized: all zero)
  std::vector<uint32_t> active;
  std::vector<double> staged;
  std::vector<fmx_refine_system> rec;
  if (max_iters) {
    active.resize(n_poses);
    staged.resize((size_t)n_poses * 12);
    rec.resize(n_poses);
  }
  for (uint32_t k = 0; k < n_poses; ++k) {
    std::memcpy(T[k].m, poses_init + (size_t)k * 12, sizeof(T[k].m));
    if (max_iters) active[k] = k;
  }
  while (!active.empty()) {
    const uint32_t count = (uint32_t)active.size();
    for (uint32_t a = 0; a < count; ++a) std::memcpy(&staged[(size_t)a * 12], T[active[a]].m, 12 * sizeof(double));
    systems_at((const double*)staged.data(), count, rec.data());
    uint32_t left = 0;
    for (uint32_t a = 0; a < count; ++a) {
      const uint32_t k = active[a];
      const fmx_refine_system& s = rec[a];
      fmx_refine_result& r = R[k];
      ++r.iters;
      r.error = s.S[28];
      r.found = s.found, r.none = s.none, r.out_of_range = s.out_of_range, r.invalid = s.invalid;
      r.unoriented = s.unoriented, r.lookups = s.lookups;
      if (!gn_step(s.S, T[k], threshold, &r.last_step, &r.converged)) {
        r.singular = 1;
        r.converged = 0;
        std::memcpy(T[k].m, poses_init + (size_t)k * 12, sizeof(T[k].m));
        continue;
      }
      if (!r.converged && r.iters < max_iters) active[left++] = k;
    }
    active.resize(left);
  }
  for (uint32_t k = 0; k < n_poses; ++k) std::memcpy(poses_out + (size_t)k * 12, T[k].m, sizeof(T[k].m));
  if (results)
    for (uint32_t k = 0; k < n_poses; ++k) results[k] = R[k];
}

}  // namespace fmx
