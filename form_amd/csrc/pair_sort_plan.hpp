// pair_sort_plan.hpp — which kernels sort one match's accepted queries into pair-major
// rows, decided on the host from the query counts and the window size alone.  No HIP
// includes: match_group_for (fmx_api.cpp) and run_match (voxelmap.hip) dispatch by it,
// and fmx_pair_sort_plan exports it for the tests (tests/test_pairsort_cpu.py).
//
//   group 8 (fmx::g8, 32 queries per match block)  fewer than kMatchLargeMin queries,
//                                                  or a window wider than kMatchTileMaxPairs
//   group 1 (fmx::gl, 256 queries per match block) otherwise
//   per-block       K > kMatchTileMaxPairs: k_match writes a [type][pair][block] histogram,
//                   exclusive_scan (k_scan_single up to kScanSingleMaxWords, else
//                   k_scan_reduce + k_scan_blocks + k_scan_tiles) + k_pair_base +
//                   k_pair_scatter (one wave per match block: group 8 only)
//   tail-scanned    k_match counts per (type, pair, tile); its last block scans them
//                   (pair_sort_tail, pair_sort_finish); k_pair_scatter_t
//   scatter-scanned the same counts while the whole table fits kScatterTab words of
//                   LDS: k_pair_scatter_s scans them itself (scatter_meta)
#pragma once
#include <cstddef>
#include <cstdint>

namespace fmx {

#ifndef FMX_MATCH_LARGE_MIN
#define FMX_MATCH_LARGE_MIN (128u << 10)  // queries from which the large-set build (fmx::gl) is used
#endif
#ifndef FMX_TILE_Q
#define FMX_TILE_Q 1024  // queries per pair-scatter tile (A/B switch)
#endif
constexpr uint64_t kMatchLargeMin = FMX_MATCH_LARGE_MIN;
constexpr int kMatchBlockThreads = 256;  // k_match: group lanes per query, 256 / group queries per block
// Windows of at most this many map scans (pairs) use the tiled pair sort; wider ones a
// per-match-block histogram whose scatter ranks within one wave, so they take the g8
// build (32 queries per block) whatever the query count.
constexpr uint32_t kMatchTileMaxPairs = 256;
constexpr uint32_t kScatterTab = 6144;  // words of k_pair_scatter_s's LDS count table
// device-wide scan (fmx_device.hpp): words per block and pass, and the most one block scans alone
constexpr size_t kScanTileWords = 4096;
constexpr size_t kScanSingleMaxWords = kScanTileWords * 4;

enum PairSortForm : uint32_t {
  kPairSortNone = 0,  // not sorted: per-pair counts only
  kPairSortPerBlock = 1,
  kPairSortTail = 2,
  kPairSortScatter = 3,
};

struct PairSortPlan {
  uint32_t group;  // lanes per query: 8 (fmx::g8) or 1 (fmx::gl)
  PairSortForm form;
  uint32_t nb_pl, nb_pt;    // match blocks per type
  uint32_t ntl_pl, ntl_pt;  // tiles per type (a tile = the match blocks of FMX_TILE_Q queries)
  uint64_t hist_words;      // per-block form: the words scanned (K * match blocks), else 0
  uint32_t scan_launches;   // per-block form: 0 (nothing to scan), 1 (k_scan_single) or 3
};

inline uint32_t match_group(uint64_t nq, uint32_t K) {
  return nq >= kMatchLargeMin && K <= kMatchTileMaxPairs ? 1u : 8u;
}

// The plan of a build with `group` lanes per query (voxelmap.hip passes its own).
inline PairSortPlan pair_sort_plan_group(uint32_t group, uint32_t n_qpl, uint32_t n_qpt, uint32_t K, bool sorted) {
  PairSortPlan p{};
  p.group = group;
  const uint32_t qpb = (uint32_t)kMatchBlockThreads / group;
  const uint32_t tile_blocks = FMX_TILE_Q / qpb > 0 ? FMX_TILE_Q / qpb : 1;
  p.nb_pl = (uint32_t)(((uint64_t)n_qpl + qpb - 1) / qpb);
  p.nb_pt = (uint32_t)(((uint64_t)n_qpt + qpb - 1) / qpb);
  p.ntl_pl = (p.nb_pl + tile_blocks - 1) / tile_blocks;
  p.ntl_pt = (p.nb_pt + tile_blocks - 1) / tile_blocks;
  // wider windows: per-block histograms; a count table that fits the scatter's LDS: no
  // match tail (the scatter scans it)
  const uint64_t tab = (uint64_t)K * (p.ntl_pl + p.ntl_pt);
  p.form = !sorted ? kPairSortNone
           : K > kMatchTileMaxPairs ? kPairSortPerBlock
           : tab <= kScatterTab ? kPairSortScatter
                                : kPairSortTail;
  if (p.form == kPairSortPerBlock) {
    p.hist_words = (uint64_t)K * ((uint64_t)p.nb_pl + p.nb_pt);
    p.scan_launches = p.hist_words == 0 ? 0u : p.hist_words <= kScanSingleMaxWords ? 1u : 3u;
  }
  return p;
}

inline PairSortPlan pair_sort_plan(uint32_t n_qpl, uint32_t n_qpt, uint32_t K, bool sorted) {
  return pair_sort_plan_group(match_group((uint64_t)n_qpl + n_qpt, K), n_qpl, n_qpt, K, sorted);
}

}  // namespace fmx
