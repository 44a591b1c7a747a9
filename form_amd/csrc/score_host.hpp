// score_host.hpp — the host-only parts of scoring many candidate poses of a scan against the
// dense map (include/fmx/fmx.h, fmx_score_poses and fmx_score_plan; densemap.hip, the score
// block): the argument checks on top of align_check, the plan (align_host.hpp's batch_plan at
// the score tile) and the ranking rule of the Python layer, restated.  No device
// code and no HIP header: tests/cpp/test_score_host.cpp builds it alone, under the host
// sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "align_host.hpp"
#include "fmx/fmx.h"

namespace fmx {

constexpr uint32_t kScoreTile = 256;  // kept points per work item: one block-wide pass

static_assert(sizeof(fmx_pose_score) == 32, "a score record is 32 bytes");

// FMX_OK, or FMX_E_INVAL and *why: NULL params, n_poses past FMX_SCORE_MAX_POSES, NULL poses or
// scores with n_poses > 0, a non-finite entry of any pose, then align_check's cases on the
// points, n, reach, max_dist2 and sigma.
inline fmx_status score_check(const void* points, unsigned long long n, const double* poses34, unsigned long long n_poses,
                              const fmx_align_params* prm, const void* scores, const char** why) {
  if (!prm) {
    *why = "null params";
    return FMX_E_INVAL;
  }
  if (n_poses > (unsigned long long)FMX_SCORE_MAX_POSES) {
    *why = "n_poses is at most FMX_SCORE_MAX_POSES";
    return FMX_E_INVAL;
  }
  if (n_poses && (!poses34 || !scores)) {
    *why = poses34 ? "null scores" : "null poses";
    return FMX_E_INVAL;
  }
  for (unsigned long long k = 0; k < n_poses * 12ull; ++k)
    if (!std::isfinite(poses34[k])) {
      *why = "non-finite pose";
      return FMX_E_INVAL;
    }
  return align_check(points, n, kEye34, prm, why);  // (the poses are checked above)
}

// The plan of a call (align_host.hpp, batch_plan): a partial record is a score record.
using ScorePlan = BatchPlan;
inline ScorePlan score_plan(unsigned long long n, uint32_t stride, uint32_t n_poses) {
  return batch_plan(n, stride, n_poses, kScoreTile, sizeof(fmx_pose_score));
}

// before(a, b): record i = a ranks ahead of record j = b.  found descending, then sum_d2
// ascending, then the index ascending: integers and doubles compared, nothing computed.
inline bool score_before(const fmx_pose_score* s, uint32_t a, uint32_t b) {
  if (s[a].found != s[b].found) return s[a].found > s[b].found;
  if (s[a].sum_d2 != s[b].sum_d2) return s[a].sum_d2 < s[b].sum_d2;
  return a < b;
}
// order[0 .. n): the indices by rank (form_amd/fmx.py, rank_scores).
inline void score_rank(const fmx_pose_score* s, uint32_t n, uint32_t* order) {
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  std::sort(order, order + n, [s](uint32_t a, uint32_t b) { return score_before(s, a, b); });
}

}  // namespace fmx
