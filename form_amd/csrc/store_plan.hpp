// Host-only planning of the two stores that move their contents while a stream runs: the
// keypoint pool (fmx_api.cpp: compact_pool / ensure_pool_room) and the smoothing-mode window
// store (window.hip: win_persist / win_reserve / win_remove).  No HIP headers: whether to
// compact, the new capacities, the list of copies (source offset, destination offset, length
// in records or rows) and the rebased range, segment and pair offsets are computed here; the
// callers execute the copies on the device.  tests/cpp/test_store_plan.cpp drives exactly
// this code on the host (tests/test_store_cpu.py against tests/store_ref.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

namespace fmx {

// Elements DBuf::ensure(n) allocates when it has to grow: geometric, and at least 256k
// elements (fmx_internal.hpp says why).
inline size_t dbuf_alloc_elems(size_t n) { return std::max<size_t>(2 * n + 64, (size_t)1 << 18); }

// ---- test-only limits (FMX_TEST_STORE_LIMITS="pool,plane_rows,point_rows"), read when the
// context is created.  0 or absent: the production sizes, allocation for allocation.
//   pool:       logical record limit of both keypoint pools (clamped to the allocated size)
//   plane_rows: the window store's initial plane-row capacity, used exactly (the arenas'
//               over-allocation is not adopted, now or after a growth)
//   point_rows: likewise for point rows, independently
struct StoreLimits {
  uint64_t pool = 0, win_pl = 0, win_pt = 0;
};
inline StoreLimits parse_store_limits(const char* v) {
  StoreLimits l;
  if (!v || !*v) return l;
  uint64_t* f[3] = {&l.pool, &l.win_pl, &l.win_pt};
  for (int k = 0; k < 3 && *v; ++k) {
    char* end = nullptr;
    *f[k] = std::strtoull(v, &end, 10);
    if (end == v) break;
    v = end;
    if (*v == ',') ++v;
  }
  return l;
}

struct StoreCopy {  // records (pool) or rows (window store)
  uint64_t src, dst, n;
};

// ---------------------------------------------------------------- keypoint pool
using PoolRanges = std::map<uint64_t, std::pair<uint64_t, uint32_t>>;  // scan -> (offset, count)

inline bool pool_has_room(uint64_t used, uint64_t need, uint64_t limit) { return used + need <= limit; }

// n more records of `scan` at the fill mark (KeypointMap::get(scan).push_back).  False, and
// nothing changed but a possibly new empty range: they would not follow the scan's own.
inline bool pool_append(PoolRanges& ranges, uint64_t& used, uint64_t scan, uint32_t n) {
  auto& rg = ranges[scan];
  if (rg.second == 0) rg.first = used;
  else if (rg.first + rg.second != used) return false;
  rg.second += n;
  used += n;
  return true;
}

// Pack every range to the front in offset order (ties: scan order).  Rewrites the ranges'
// offsets, returns the copies old pool -> new pool and the new fill.
struct PoolPlan {
  std::vector<StoreCopy> copies;
  uint64_t used = 0;
};
inline PoolPlan plan_pool_compact(PoolRanges& ranges) {
  PoolPlan pl;
  std::vector<std::pair<uint64_t, uint64_t>> order;  // (offset, scan)
  for (auto& [s, r] : ranges) order.push_back({r.first, s});
  std::sort(order.begin(), order.end());
  uint64_t o = 0;
  for (auto& [off, s] : order) {
    auto& r = ranges[s];
    if (r.second) pl.copies.push_back(StoreCopy{off, o, r.second});
    r.first = o;
    o += r.second;
  }
  pl.used = o;
  return pl;
}

// ---------------------------------------------------------------- window store
struct WinPair {  // one FeatureFactor(X(i), X(j))'s rows in the arena
  uint64_t i, j;
  uint64_t pl_off, pt_off;
  uint32_t pl_n, pt_n;
};
struct WinSeg {  // scan j's correspondences (the last match of its ICP loop)
  uint64_t pl_off = 0, pt_off = 0;
  uint32_t pl_n = 0, pt_n = 0;
  std::vector<WinPair> pairs;  // i ascending
};
using WinSegs = std::map<uint64_t, WinSeg>;

// Row capacities asked of the first allocation.
inline void win_initial_caps(uint64_t keypoint_pool_capacity, const StoreLimits& lim, uint64_t& cap_pl,
                             uint64_t& cap_pt) {
  cap_pl = std::max<uint64_t>(keypoint_pool_capacity, 1u << 20);
  cap_pt = std::max<uint64_t>(cap_pl / 4, 1u << 18);
  if (lim.win_pl) cap_pl = lim.win_pl;
  if (lim.win_pt) cap_pt = lim.win_pt;
}
// The capacity the store uses of an arena of `alloc` elements it asked `want` rows of
// (`width` values per row): all of it (DBuf over-allocates), or exactly `want` under a limit.
inline uint64_t win_cap_of(uint64_t want, size_t alloc, int width, bool exact) {
  return exact ? want : alloc / (size_t)width;
}

// Segment j at the tail: pairs (map_scans[k], j) for every k with rows, in k order.
inline WinSeg win_make_seg(uint64_t j, uint64_t tail_pl, uint64_t tail_pt, const uint64_t* map_scans,
                           const uint32_t* cnt_pl, const uint32_t* cnt_pt, uint32_t K) {
  WinSeg s;
  s.pl_off = tail_pl;
  s.pt_off = tail_pt;
  uint64_t op = 0, ot = 0;
  for (uint32_t k = 0; k < K; ++k) {
    if (cnt_pl[k] + cnt_pt[k] > 0)
      s.pairs.push_back(WinPair{map_scans[k], j, s.pl_off + op, s.pt_off + ot, cnt_pl[k], cnt_pt[k]});
    op += cnt_pl[k];
    ot += cnt_pt[k];
  }
  s.pl_n = (uint32_t)op;
  s.pt_n = (uint32_t)ot;
  return s;
}

// Erase of scan s: its segment and every pair (s, j) of the other segments.
inline void win_erase_scan(WinSegs& segs, uint64_t s) {
  segs.erase(s);
  for (auto& [j, seg] : segs)
    seg.pairs.erase(std::remove_if(seg.pairs.begin(), seg.pairs.end(), [&](const WinPair& p) { return p.i == s; }),
                    seg.pairs.end());
}

// Room for (npl, npt) more rows at the tail.  compact false: they fit, nothing moves.
// Otherwise the live segments go to the other arena in segment order (copies, in rows, one
// per segment and row type; the source has leading dimension cap_*, the destination the
// capacity the caller derives from want_*), and `segs` is rebased.  want_* doubles the
// capacity until the live rows (the new ones included) fill at most half of it.
struct WinPlan {
  bool compact = false;
  uint64_t want_pl = 0, want_pt = 0;  // == cap_* where that arena does not grow
  std::vector<StoreCopy> pl, pt;
  uint64_t tail_pl = 0, tail_pt = 0;
};
inline WinPlan plan_win_reserve(WinSegs& segs, uint64_t tail_pl, uint64_t tail_pt, uint64_t cap_pl, uint64_t cap_pt,
                                uint64_t npl, uint64_t npt) {
  WinPlan P;
  P.want_pl = cap_pl;
  P.want_pt = cap_pt;
  P.tail_pl = tail_pl;
  P.tail_pt = tail_pt;
  if (tail_pl + npl <= cap_pl && tail_pt + npt <= cap_pt) return P;
  P.compact = true;
  uint64_t live_pl = npl, live_pt = npt;
  for (auto& [j, s] : segs) {
    live_pl += s.pl_n;
    live_pt += s.pt_n;
  }
  while (2 * live_pl > P.want_pl) P.want_pl *= 2;
  while (2 * live_pt > P.want_pt) P.want_pt *= 2;
  uint64_t tpl = 0, tpt = 0;
  for (auto& [j, s] : segs) {
    P.pl.push_back(StoreCopy{s.pl_off, tpl, s.pl_n});
    P.pt.push_back(StoreCopy{s.pt_off, tpt, s.pt_n});
    for (auto& p : s.pairs) {
      p.pl_off = p.pl_off - s.pl_off + tpl;
      p.pt_off = p.pt_off - s.pt_off + tpt;
    }
    s.pl_off = tpl;
    s.pt_off = tpt;
    tpl += s.pl_n;
    tpt += s.pt_n;
  }
  P.tail_pl = tpl;
  P.tail_pt = tpt;
  return P;
}

}  // namespace fmx
