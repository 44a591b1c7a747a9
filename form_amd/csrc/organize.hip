// organize.hip — an unorganized cloud of returns -> the organized R x C scan the pipeline
// reads (DESIGN.md §Unorganized clouds; include/fmx/fmx.h, fmx_organize).  Two launches on
// one stream, no host round trip between them:
//
//   claim   one lane per point: its cell (column from the azimuth in fp64, row from the
//           ring table or a binary search over the elevation midpoints), then one
//           return-less 64-bit atomicMin of (float bits of r2) << 32 | index on the cell's
//           key.  Non-negative floats order like their bit patterns, so the smallest key is
//           the nearest point, the lowest input index among equal ranges — whatever order
//           the lanes run in.  Invalid and off-grid points are counted with one atomic per
//           wave (ballot + popcount).
//   gather  one lane per cell, row-major (coalesced float4 stores): reads the key, copies
//           the winner's point (pad 0), index and clamped sweep fraction, and puts the key
//           back to all-ones, so the table is cleared once, when it is allocated.  Each
//           block adds (1 << 32 | its filled cells) to one 64-bit word with a single
//           atomic: the block that finds every other block's ticket in the value it gets
//           back also has the total in it, publishes the four counts and zeroes the
//           counters for the next scan.  One word carries ticket and count, so no fence
//           orders two locations (measured at C4: a device-scope fence per wave, which on
//           gfx950 writes the XCD's L2 back, made this kernel 107 us; counting the filled
//           cells with returning atomics in the claim made that one 54 us instead of 12).
//
// r2 = (x x + y y) + z z in fp32 without contraction (-ffp-contract=off), as the
// restatement in tests/organize_ref.py computes it.
#include <cmath>

#include "fmx_internal.hpp"

namespace fmx {

constexpr int kOrgThreads = 256;
// the gather's blocks each end with one atomic on the same word: large blocks, few of them
// (C4, 1024 blocks of 256: 17 us; 256 blocks of 1024: see DESIGN.md)
constexpr int kOrgGatherThreads = 1024;
constexpr unsigned long long kOrgEmpty = ~0ull;

struct OrgArgs {
  int R, C;
  int elevation;          // 0: row = ring_to_row[ring] (identity without a table)
  int clockwise;
  double az_off;
  const int32_t* ring_to_row;  // n_rings entries (-1: off-grid) or null
  uint32_t n_rings;       // with a null table: R
  // elevation mode: R - 1 midpoints and the two outer limits of the table, all negated
  // on the host when the table descends, so that they ascend with the row index
  const double* mid;
  double lo, hi, sign;
};

__global__ __launch_bounds__(kOrgThreads) void k_org_claim(const float4* __restrict__ pts,
                                                           const uint16_t* __restrict__ ring, uint32_t n, OrgArgs a,
                                                           unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kOrgThreads + threadIdx.x;
  const bool live = i < n;
  bool invalid = false, off = false;
  if (live) {
    const float4 p = pts[i];
    invalid = !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) || (p.x == 0.0f && p.y == 0.0f && p.z == 0.0f);
    if (!invalid) {
      const double x = p.x, y = p.y, z = p.z;
      int row;
      if (a.elevation) {
        const double el = a.sign * atan2(z, sqrt(x * x + y * y));
        off = el < a.lo || el > a.hi;
        // the number of midpoints below el: a tie stays with the lower row
        int l = 0, h = a.R - 1;
        while (l < h) {
          const int m = (l + h) >> 1;
          if (el > a.mid[m]) l = m + 1;
          else h = m;
        }
        row = l;
      } else {
        const uint32_t g = ring[i];
        row = g < a.n_rings ? (a.ring_to_row ? a.ring_to_row[g] : (int)g) : -1;
        off = row < 0 || row >= a.R;
      }
      if (!off) {
        double u = (atan2(y, x) - a.az_off) * (double)a.C / (2.0 * M_PI);
        if (a.clockwise) u = -u;
        int cl = (int)fmod(floor(u + 0.5), (double)a.C);  // exact, in (-C, C)
        if (cl < 0) cl += a.C;
        const float r2 = (p.x * p.x + p.y * p.y) + p.z * p.z;
        const unsigned long long key = ((unsigned long long)__float_as_uint(r2) << 32) | (unsigned long long)i;
        atomicMin(&keys[(size_t)row * (size_t)a.C + (size_t)cl], key);  // result unused: return-less
      }
    }
  }
  const unsigned long long bi = __ballot(invalid), bo = __ballot(off);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&cnt[0], (uint32_t)__popcll(bi));
    if (bo) atomicAdd(&cnt[1], (uint32_t)__popcll(bo));
  }
}

// cnt: {invalid, off_grid} (final since the claim ended); tick: finished blocks << 32 |
// filled cells; res (device-visible, 4 words): {placed, displaced, off_grid, invalid}
__global__ __launch_bounds__(kOrgGatherThreads) void k_org_gather(const float4* __restrict__ pts,
                                                            const float* __restrict__ frac, uint32_t n, uint32_t cells,
                                                            unsigned long long* __restrict__ keys,
                                                            float4* __restrict__ out, uint32_t* __restrict__ index,
                                                            float* __restrict__ out_frac, uint32_t* __restrict__ cnt,
                                                            unsigned long long* __restrict__ tick,
                                                            uint32_t* __restrict__ res) {
  const uint32_t cell = blockIdx.x * (uint32_t)kOrgGatherThreads + threadIdx.x;
  bool placed = false;
  if (cell < cells) {
    const unsigned long long key = keys[cell];
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t idx = 0xFFFFFFFFu;
    float f = 0.f;
    if (key != kOrgEmpty) keys[cell] = kOrgEmpty;
    // (a key's index is below n: claim and gather of one cloud run back to back)
    if (key != kOrgEmpty && (uint32_t)key < n) {
      placed = true;
      idx = (uint32_t)key;
      const float4 p = pts[idx];
      q = make_float4(p.x, p.y, p.z, 0.f);
      if (frac) f = fminf(fmaxf(frac[idx], 0.f), 1.f);  // a fraction outside [0, 1] is clamped (NaN: 0)
    }
    out[cell] = q;
    index[cell] = idx;
    if (out_frac) out_frac[cell] = f;
  }
  const unsigned long long mine = (1ull << 32) | (unsigned long long)__syncthreads_count(placed);
  if (threadIdx.x != 0) return;
  const unsigned long long all = atomicAdd(tick, mine) + mine;
  if ((uint32_t)(all >> 32) == gridDim.x) {  // every other block's ticket, so its count too, is in
    const uint32_t inv = cnt[0], offg = cnt[1], pl = (uint32_t)all;
    cnt[0] = cnt[1] = 0;
    *tick = 0;
    res[0] = pl;
    res[1] = n - inv - offg - pl;
    res[2] = offg;
    res[3] = inv;
  }
}

// The n points at d_pts (d_ring in ring mode, d_frac or null) -> d_out / d_index / d_frac_out
// (R * C each; d_frac_out null without fractions) on stream st.  The counts land in
// c->org.h_cnt once the stream has passed the gather.
void run_organize(fmx_ctx* c, const float4* d_pts, const uint16_t* d_ring, const float* d_frac, size_t n,
                  float4* d_out, uint32_t* d_index, float* d_frac_out, hipStream_t st) {
  auto& o = c->org;
  const auto& E = c->P.extraction;
  OrgArgs a{};
  a.R = E.num_rows;
  a.C = E.num_columns;
  a.elevation = o.elevation ? 1 : 0;
  a.clockwise = o.clockwise ? 1 : 0;
  a.az_off = o.az_off;
  a.ring_to_row = o.have_ring_map ? o.ring_to_row.p : nullptr;
  a.n_rings = o.have_ring_map ? o.n_rings : (uint32_t)E.num_rows;
  a.mid = o.mid.p;
  a.lo = o.lo;
  a.hi = o.hi;
  a.sign = o.sign;
  const size_t cells = (size_t)a.R * (size_t)a.C;
  if (n) {
    const uint32_t blocks = (uint32_t)((n + kOrgThreads - 1) / kOrgThreads);
    // DESIGN.md §Unorganized clouds: the point, its ring and fraction (the stage's inputs,
    // each read once) and the 8 B atomic
    ProfScope ps(c->prof, PROF_ORGANIZE, (double)n * (16.0 + (d_ring ? 2.0 : 0.0) + (d_frac ? 4.0 : 0.0) + 8.0), st);
    hipLaunchKernelGGL(k_org_claim, dim3(blocks), dim3(kOrgThreads), 0, st, d_pts, d_ring, (uint32_t)n, a, o.keys.p,
                       o.cnt.p);
    FMX_HIP(hipGetLastError());
  }
  {
    const uint32_t blocks = (uint32_t)((cells + kOrgGatherThreads - 1) / kOrgGatherThreads);
    // 8 key + 16 winner + 16 scan + 4 index (+ 4 fraction) per cell
    ProfScope ps(c->prof, PROF_ORGANIZE, (double)cells * (44.0 + (d_frac ? 4.0 : 0.0)), st);
    hipLaunchKernelGGL(k_org_gather, dim3(blocks), dim3(kOrgGatherThreads), 0, st, d_pts, d_frac, (uint32_t)n, (uint32_t)cells,
                       o.keys.p, d_out, d_index, d_frac ? d_frac_out : nullptr, o.cnt.p,
                       reinterpret_cast<unsigned long long*>(o.cnt.p + 2), o.h_cnt.d);
    FMX_HIP(hipGetLastError());
  }
}

}  // namespace fmx
