// score_host.hpp — the host-only parts of scoring many candidate poses of a scan against the
// dense map (include/fmx/fmx.h, fmx_score_poses and fmx_score_plan; densemap.hip, the score
// block): the argument checks on top of align_check, the plan (tiling and chunking, the one
// place their constants live) and the ranking rule of the Python layer, restated.  No device
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

constexpr uint32_t kScoreTile = 256;          // kept points per work item: one block-wide pass
constexpr uint32_t kScoreGridCap = 2048;      // blocks of the first launch at the most (k_nearest's cap)
constexpr uint32_t kScoreChunkPoses = 16384;  // poses per chunk at the most
constexpr uint64_t kScorePartialBytes = 32ull << 20;  // ... and the partial records of a chunk

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
  const double eye[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};  // (the poses are checked above)
  return align_check(points, n, eye, prm, why);
}

// The tiling and chunking of a call (fmx_score_plan's out, in its order).
struct ScorePlan {
  uint32_t kept, tile, tiles, chunk, chunks, cap;
};
// n < 2^32 (the caller checked): the kept points fit a word.
inline ScorePlan score_plan(unsigned long long n, uint32_t stride, uint32_t n_poses) {
  ScorePlan p{};
  p.kept = (uint32_t)align_kept(n, stride ? stride : 1u);
  p.tile = kScoreTile;
  p.tiles = (uint32_t)(((unsigned long long)p.kept + kScoreTile - 1) / kScoreTile);
  const uint64_t fit = kScorePartialBytes / sizeof(fmx_pose_score) / (p.tiles ? p.tiles : 1u);
  p.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kScoreChunkPoses, fit));
  p.chunks = p.kept ? (n_poses + p.chunk - 1) / p.chunk : 0u;
  p.cap = kScoreGridCap;
  return p;
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
