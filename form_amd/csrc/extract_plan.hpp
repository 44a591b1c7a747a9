// extract_plan.hpp — which kernels one extraction runs, decided on the host from the scan
// geometry and the extraction parameters alone.  No HIP includes: extract.hip launches by
// it, and tests/cpp/test_extract_plan.cpp checks it with plain g++.
//
//   rows     k_extract_rows<KC, true>  (sector-parallel: wave s owns sector s) or
//            k_extract_rows<KC, false> (sectors in order, ranked by counting)
//   KC       5 when neighbor_points == 5 (unrolled), else 0 (read from the arguments)
//   normals  k_normals (rows r-1..r+1 in LDS) or k_row_blocks + k_closest + k_fit
#pragma once
#include <cstddef>

namespace fmx {

// The sector-parallel kernel sorts one sector's candidate keys in one wave's registers:
// 8 keys per lane x 64 lanes.  A sector that could hold more candidates must not run there.
constexpr int kSortCapacity = 512;
constexpr int kParMaxSectors = 16;  // one wave per sector, 16 waves per workgroup
constexpr int kExtractMaxC = 4096;  // widest scan line the API accepts
constexpr int kNrmMaxC = 2048;      // widest scan line of the fused k_normals
// k_extract_rows per column: the point (16), its key (8), curvature (4), four byte flags
constexpr size_t kRowLdsPerCol = 16 + 8 + 4 + 4;
// dynamic LDS granted to the kernels (hipFuncAttributeMaxDynamicSharedMemorySize)
constexpr size_t kRowLdsMax = (size_t)kExtractMaxC * kRowLdsPerCol;
constexpr size_t kNrmLdsMax = 160 * 1024 - 256;  // 160 KB per CU, minus the kernel's few static bytes

struct ExtractPlan {
  bool sector_parallel;  // k_extract_rows<KC, true>
  bool kc5;              // KC = 5
  bool fused_normals;    // k_normals
  size_t lds_rows;       // dynamic LDS of k_extract_rows
  size_t lds_normals;    // dynamic LDS k_normals asks for (launched only when fused_normals)
};

// Candidates a sector can hold at most: its columns that can be planar-valid.  Sectors
// are pps = C / S columns wide and the last one runs to C; the first k columns of the
// line (sector 0) and the last k (sector S - 1) are never valid.
inline int extract_longest_sector(int C, int k, int S) {
  const int pps = C / S;
  int longest = 0;
  for (int s = 0; s < S; ++s) {
    const int b = s * pps, e = s == S - 1 ? C : b + pps;
    const int n = (e < C - k ? e : C - k) - (b > k ? b : k);  // [b, e) within [k, C - k)
    if (n > longest) longest = n;
  }
  return longest;
}

// R does not enter any decision today (one workgroup per line either way).
inline ExtractPlan extract_plan(int R, int C, int k, int S, int P) {
  (void)R;
  ExtractPlan p;
  const int pps = C / S;
  const size_t nwd = (size_t)(C + 63) / 64 + 1;   // accepted-bitmap words
  const size_t cap_pl = (size_t)S * (P + 1);      // kept planar points per line
  // sector-parallel selection when every sector sorts in one wave's registers (at most
  // kSortCapacity candidates, the wider last sector included), there is a wave per
  // sector, sectors are longer than the suppression reach, and the two kept lists fit
  // the dead point area of LDS behind the sorted columns and the bitmap
  p.sector_parallel = pps <= kSortCapacity && extract_longest_sector(C, k, S) <= kSortCapacity &&
                      S <= kParMaxSectors && pps >= 2 * k &&
                      8 * (size_t)C + 8 * nwd + 2 * 4 * cap_pl <= 16 * (size_t)C;
  p.kc5 = k == 5;
  p.lds_rows = (size_t)C * kRowLdsPerCol;
  // k_normals: three padded rows, the block boxes of rows r-1 / r+1, per kept point its
  // closest columns (8), best key (8) and column (4), and the block work list
  const size_t nblk = (size_t)(C + 63) / 64;
  p.lds_normals = (size_t)3 * (C + (C >> 6) + 1) * 16 + (size_t)4 * nblk * 16 + cap_pl * 20 + cap_pl * nblk * 4;
  p.fused_normals = C <= kNrmMaxC && p.lds_normals <= kNrmLdsMax;
  return p;
}

}  // namespace fmx
