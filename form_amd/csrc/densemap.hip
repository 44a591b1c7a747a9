// densemap.hip — the opt-in dense voxel map of the registered scans (DESIGN.md §Dense map;
// include/fmx/fmx.h, fmx_dense_integrate).  A fixed-capacity open-addressed hash of world
// voxels, structure-of-arrays, 44 B per slot: keys (u64), tags (u64), hits (u32), xyz
// (3 doubles); 52 B once carving has been enabled (misses and seen, u32 each: the carve
// block further down; the probe, nearest, align and normals blocks behind it only read the
// table, the normals into 20 B per slot of their own; the upload block behind those puts
// downloaded voxels back).  An integration is
// two launches on one stream, no host round trip between them; the kernel boundary is the
// only ordering (no in-kernel device-scope fence: see organize.hip's header for what one per
// wave costs on gfx950).
//
//   claim   one lane per point: classify it (invalid / gated / out of range), compute its
//           voxel key, find or insert the key's slot (home = mix64(key) & (slots - 1),
//           linear probing, a 64-bit atomicCAS on the key word only while the slot reads
//           empty), then one return-less atomicMin of the tag (seq << 32 | index) on the
//           slot's tag word, one return-less atomicAdd on its hit count, and the slot (or
//           the dropped marker) into the n-word scratch.  Adjacent lanes with one key share
//           one lane's probe and atomics (the in-wave merge below).  The rejected classes
//           are counted with one atomic per wave and class (ballot + popcount).
//   fill    one lane per point: the lane whose tag equals the slot's is the voxel's
//           representative, which only a point of the integration that opened the voxel
//           can be (an earlier integration's tag is smaller), and writes the world point,
//           recomputed with the same expression.  Each block adds (1 << 32 | its winners)
//           to one word: the block that finds every ticket in the value it gets back has
//           the number of new voxels in it, publishes the counts, the voxel total and the
//           completion word to pinned host memory and re-arms the counters.
//
// The content of the map does not depend on the order the lanes run in: keys are only
// ever inserted (between integrations a roll, further down, may rebuild the table from the
// voxels it keeps), the tag is a minimum, the hit count a sum, and a slot's point is written
// by exactly one lane.  The host keeps the load at or below 1/2 (it refuses an integration
// unless voxels + n <= max_voxels, and slots >= 2 * max_voxels), so a probe sequence always
// meets an empty slot.
//
// r2 = (x x + y y) + z z in fp32 and the world point ((R0 x + R1 y) + R2 z) + t in fp64,
// both without contraction (-ffp-contract=off), as tests/dense_ref.py restates them.
#include <cmath>

#include "fmx_device.hpp"
#include "fmx_internal.hpp"

namespace fmx {

constexpr int kDenseThreads = 256;
// the fill's blocks each end with one atomic on the same word (as organize.hip's gather)
constexpr int kDenseFillThreads = 1024;
constexpr int kDenseScanBlocks = 2048;  // count / compact: grid-stride over the slots
constexpr unsigned long long kDenseEmpty = ~0ull;
constexpr uint32_t kDenseDropped = 0xFFFFFFFFu;
constexpr double kDenseLimit = 1048575.0;  // 2^20 - 1: valid voxel coordinates |c| < this
constexpr long long kDenseBias = 1ll << 20;

struct DenseArgs {
  Pose34 T;
  double w, min2, max2;
  uint32_t slot_mask;
};

// 0 valid (key set), 1 invalid, 2 gated, 3 out of range
__device__ __forceinline__ int dense_classify(const float4 p, const DenseArgs& a, unsigned long long* key) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) || (p.x == 0.0f && p.y == 0.0f && p.z == 0.0f)) return 1;
  const float r2f = (p.x * p.x + p.y * p.y) + p.z * p.z;
  const double r2 = (double)r2f;
  if (!(r2 > a.min2 && r2 < a.max2)) return 2;
  double wp[3];
  d_xform(a.T.m, (double)p.x, (double)p.y, (double)p.z, wp);
  const double cx = floor(wp[0] / a.w), cy = floor(wp[1] / a.w), cz = floor(wp[2] / a.w);
  // in fp64, before the cast (a NaN or an infinity fails the comparison)
  if (!(fabs(cx) < kDenseLimit && fabs(cy) < kDenseLimit && fabs(cz) < kDenseLimit)) return 3;
  *key = ((unsigned long long)((long long)cx + kDenseBias) << 42) |
         ((unsigned long long)((long long)cy + kDenseBias) << 21) | (unsigned long long)((long long)cz + kDenseBias);
  return 0;
}

// In-wave merge: adjacent lanes with one key (neighbouring columns that fall into one voxel)
// form a run; its first lane probes and issues the atomics for all of them (its index is
// the run's lowest, the hit count the run's length), the others take its slot by a shuffle.
// Same map, fewer atomics: 0.87-0.94 of the plain form's time per C4 scan, same box,
// alternated (profiles/dense_merge_ab.json; FMX_DENSE_MERGE=0 builds the plain form).
#ifndef FMX_DENSE_MERGE
#define FMX_DENSE_MERGE 1
#endif

// cnt: {invalid, gated, out_of_range, voxels, ticket (2 words)}
__global__ __launch_bounds__(kDenseThreads) void k_dense_claim(const float4* __restrict__ pts, uint32_t n, DenseArgs a,
                                                               uint32_t seq, unsigned long long* keys,
                                                               unsigned long long* tags, uint32_t* hits,
                                                               uint32_t* __restrict__ slot_of,
                                                               uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  int cls = -1;  // past the end
  unsigned long long key = 0;
  if (i < n) cls = dense_classify(pts[i], a, &key);
  bool head = cls == 0;
  uint32_t run = 1;
#if FMX_DENSE_MERGE
  const int lane = lane_id();
  const unsigned long long pkey = __shfl_up(key, 1, 64);
  const int pcls = __shfl_up(cls, 1, 64);
  head = cls == 0 && (lane == 0 || pcls != 0 || pkey != key);
  const unsigned long long H = __ballot(head), V = __ballot(cls == 0);
  {
    const unsigned long long brk = lane == 63 ? 0ull : ((~V | H) >> (lane + 1));  // the run ends before the next break
    run = 1u + (brk ? (uint32_t)__builtin_ctzll(brk) : (uint32_t)(63 - lane));
  }
#endif
  uint32_t slot = kDenseDropped;
  if (head) {
    uint32_t h = (uint32_t)mix64(key) & a.slot_mask;
    // (bounded by the table: the host's capacity rule leaves half the slots empty)
    for (uint32_t probe = 0; probe <= a.slot_mask; ++probe) {
      unsigned long long k = keys[h];  // a stale empty is settled by the CAS; keys never change once set
      if (k == kDenseEmpty) k = atomicCAS(&keys[h], kDenseEmpty, key);
      if (k == kDenseEmpty || k == key) {
        slot = h;
        break;
      }
      h = (h + 1) & a.slot_mask;
    }
    if (slot != kDenseDropped) {
      atomicMin(&tags[slot], ((unsigned long long)seq << 32) | (unsigned long long)i);  // results unused:
      atomicAdd(&hits[slot], run);                                                       // return-less
    }
  }
#if FMX_DENSE_MERGE
  {
    const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
    const unsigned long long mine = H & le;
    const int hl = mine ? 63 - __builtin_clzll(mine) : lane;  // the run's first lane
    const uint32_t hs = (uint32_t)__shfl((int)slot, hl, 64);
    if (cls == 0) slot = hs;
  }
#endif
  if (i < n) slot_of[i] = slot;
  const unsigned long long bi = __ballot(cls == 1), bg = __ballot(cls == 2), bo = __ballot(cls == 3);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&cnt[0], (uint32_t)__popcll(bi));
    if (bg) atomicAdd(&cnt[1], (uint32_t)__popcll(bg));
    if (bo) atomicAdd(&cnt[2], (uint32_t)__popcll(bo));
  }
}

// res (pinned, device-visible): {added, merged, gated, out_of_range, invalid, voxels}; flag: the
// completion word, seq_flag its value for this launch
__global__ __launch_bounds__(kDenseFillThreads) void k_dense_fill(const float4* __restrict__ pts, uint32_t n,
                                                                  DenseArgs a, uint32_t seq,
                                                                  const unsigned long long* __restrict__ tags,
                                                                  const uint32_t* __restrict__ slot_of,
                                                                  double* __restrict__ xyz, uint32_t* __restrict__ cnt,
                                                                  unsigned long long* __restrict__ tick,
                                                                  uint32_t* __restrict__ res, uint32_t* flag,
                                                                  uint32_t seq_flag) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseFillThreads + threadIdx.x;
  bool winner = false;
  if (i < n) {
    const uint32_t slot = slot_of[i];
    if (slot != kDenseDropped && tags[slot] == (((unsigned long long)seq << 32) | (unsigned long long)i)) {
      winner = true;
      const float4 p = pts[i];
      double wp[3];
      d_xform(a.T.m, (double)p.x, (double)p.y, (double)p.z, wp);
      double* o = xyz + 3 * (size_t)slot;
      o[0] = wp[0];
      o[1] = wp[1];
      o[2] = wp[2];
    }
  }
  // (every lane's reads of pts have returned by this barrier: the host may hand the scan
  // back to its owner once the completion word is in)
  const unsigned long long mine = (1ull << 32) | (unsigned long long)__syncthreads_count(winner);
  if (threadIdx.x != 0) return;
  const unsigned long long all = atomicAdd(tick, mine) + mine;
  if ((uint32_t)(all >> 32) == gridDim.x) {  // every other block's ticket, so its count too, is in
    const uint32_t inv = cnt[0], gat = cnt[1], oor = cnt[2], added = (uint32_t)all;
    const uint32_t vox = cnt[3] + added;
    cnt[0] = cnt[1] = cnt[2] = 0;
    cnt[3] = vox;
    *tick = 0;
    host_store(&res[0], added);
    host_store(&res[1], n - inv - gat - oor - added);
    host_store(&res[2], gat);
    host_store(&res[3], oor);
    host_store(&res[4], inv);
    host_store(&res[5], vox);
    publish_flag(flag, seq_flag);
  }
}

// What a download takes: hits >= min_hits and, with den != 0, misses * den <= hits * num in
// 64-bit integers (fmx_carve_download).  misses: the carve block's array, or null (reads 0).
struct DenseTake {
  uint32_t min_hits, num, den;
  const uint32_t* misses;
};
__device__ __forceinline__ uint32_t dense_misses(const DenseTake& t, uint64_t s) { return t.misses ? t.misses[s] : 0u; }
__device__ __forceinline__ bool dense_take(const DenseTake& t, uint32_t h, uint64_t s) {
  if (h < t.min_hits) return false;
  if (!t.den) return true;
  return (unsigned long long)dense_misses(t, s) * t.den <= (unsigned long long)h * t.num;
}

// Slots a download takes: counted (out_n), one atomic per wave.
__global__ __launch_bounds__(kDenseThreads) void k_dense_count(const uint32_t* __restrict__ hits, uint64_t slots,
                                                               DenseTake tk, uint32_t* __restrict__ out_n) {
  uint32_t mine = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kDenseThreads; base < slots; base += (uint64_t)gridDim.x * kDenseThreads) {
    const uint64_t s = base + threadIdx.x;
    const bool take = s < slots && dense_take(tk, hits[s], s);
    mine += (uint32_t)__popcll(__ballot(take));  // the same in every lane of the wave
  }
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out_n, mine);
}

// ... appended: (xyz, tag, hits, and misses when o_miss is given) of each, in no particular
// order; cap: the room in the outputs.
// Each wave walks its slots twice: once to count what it will take, then ONE atomic for its
// place in the output, then again to copy (an atomic per wave and step, one word for all:
// 4.0 ms for 430k voxels in 2^26 slots at C4, profiles/dense_cost.json has this form's time).
__global__ __launch_bounds__(kDenseThreads) void k_dense_compact(const uint32_t* __restrict__ hits,
                                                                 const unsigned long long* __restrict__ tags,
                                                                 const double* __restrict__ xyz, uint64_t slots,
                                                                 DenseTake tk, uint32_t cap,
                                                                 uint32_t* __restrict__ out_n, double* __restrict__ o_xyz,
                                                                 unsigned long long* __restrict__ o_tag,
                                                                 uint32_t* __restrict__ o_hits,
                                                                 uint32_t* __restrict__ o_miss) {
  const int lane = threadIdx.x & 63;
  const uint64_t first = (uint64_t)blockIdx.x * kDenseThreads, step = (uint64_t)gridDim.x * kDenseThreads;
  uint32_t mine = 0;
  for (uint64_t base = first; base < slots; base += step) {
    const uint64_t s = base + threadIdx.x;
    mine += (uint32_t)__popcll(__ballot(s < slots && dense_take(tk, hits[s], s)));  // the same in every lane of the wave
  }
  if (!mine) return;  // (the whole wave)
  uint32_t at = 0;
  if (lane == 0) at = atomicAdd(out_n, mine);
  at = (uint32_t)__shfl((int)at, 0, 64);
  for (uint64_t base = first; base < slots; base += step) {
    const uint64_t s = base + threadIdx.x;
    const uint32_t h = s < slots ? hits[s] : 0u;
    const bool take = s < slots && dense_take(tk, h, s);
    const unsigned long long b = __ballot(take);
    if (take) {
      const uint32_t o = at + (uint32_t)__popcll(b & lanemask_lt());
      if (o < cap) {  // (the count pass sized the outputs: never false)
        o_xyz[3 * (size_t)o + 0] = xyz[3 * s + 0];
        o_xyz[3 * (size_t)o + 1] = xyz[3 * s + 1];
        o_xyz[3 * (size_t)o + 2] = xyz[3 * s + 2];
        o_tag[o] = tags[s];
        o_hits[o] = h;
        if (o_miss) o_miss[o] = dense_misses(tk, s);
      }
    }
    at += (uint32_t)__popcll(b);
  }
}

// ---- rolling (DESIGN.md §Dense map, Rolling; include/fmx/fmx.h, fmx_roll_evict).  The
// voxels outside a box leave the table and the ones inside are put back by their keys: a
// slot emptied in place would cut the probe chains that run through it (a later claim
// would stop at the hole and insert the key behind it a second time), and a tombstone
// would count towards the load that bounds the probe loops.  Three launches on one stream,
// the kernel boundary the only ordering, as above.
//
//   count     every key: inside / outside, one atomic per wave and counter
//   split     two walks per wave (as k_dense_compact): what it will move to each of the two
//             streams, ONE returning atomic per stream for its place, then the copy.  The
//             lane that moves a slot empties it (key, tag, hits); no other lane reads it in
//             this launch, so the table is empty when the launch ends, without a memset.
//   reinsert  one lane per kept voxel: the claim's probe with its own (distinct) key, then
//             plain stores of tag, hits and point; sets the device's voxel total.
//
// With carving enabled a voxel's miss count travels with it (both streams) and the slot it
// leaves is zeroed in misses and seen: seen is nonzero only in occupied slots, so a roll
// leaves it all zero (a kept voxel's new slot has no mark from the integration before).
//
// A voxel is inside iff |v_k - cc_k| <= half_k on every axis, v decoded from the key, in
// 64-bit integers (tests/roll_ref.py restates it).
struct RollBox {
  long long cc[3], half[3];
};

__device__ __forceinline__ bool roll_inside(unsigned long long key, const RollBox& b) {
  const long long v[3] = {(long long)((key >> 42) & 0x1FFFFFull) - kDenseBias,
                          (long long)((key >> 21) & 0x1FFFFFull) - kDenseBias, (long long)(key & 0x1FFFFFull) - kDenseBias};
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long d = v[k] - b.cc[k];
    in = in && (d < 0 ? -d : d) <= b.half[k];
  }
  return in;
}

// out: {inside, outside}
__global__ __launch_bounds__(kDenseThreads) void k_roll_count(const unsigned long long* __restrict__ keys, uint64_t slots,
                                                              RollBox box, uint32_t* __restrict__ out) {
  uint32_t n_in = 0, n_out = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kDenseThreads; base < slots; base += (uint64_t)gridDim.x * kDenseThreads) {
    const uint64_t s = base + threadIdx.x;
    const unsigned long long k = s < slots ? keys[s] : kDenseEmpty;
    const bool occ = k != kDenseEmpty, in = occ && roll_inside(k, box);
    n_in += (uint32_t)__popcll(__ballot(in));  // the same in every lane of the wave
    n_out += (uint32_t)__popcll(__ballot(occ && !in));
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_in) atomicAdd(&out[0], n_in);
    if (n_out) atomicAdd(&out[1], n_out);
  }
}

// cur: {evicted, kept} cursors; cap_e / cap_k: the room in the outputs (e_*) and the staging list (s_*);
// misses, seen, e_miss, s_miss: all null unless carving has been enabled
__global__ __launch_bounds__(kDenseThreads) void k_roll_split(
    unsigned long long* keys, unsigned long long* tags, uint32_t* hits, const double* __restrict__ xyz, uint64_t slots,
    RollBox box, uint32_t cap_e, uint32_t cap_k, uint32_t* __restrict__ cur,
    double* __restrict__ e_xyz, unsigned long long* __restrict__ e_tag, uint32_t* __restrict__ e_hits,
    unsigned long long* __restrict__ s_key, unsigned long long* __restrict__ s_tag, uint32_t* __restrict__ s_hits,
    double* __restrict__ s_xyz, uint32_t* misses, uint32_t* seen, uint32_t* __restrict__ e_miss,
    uint32_t* __restrict__ s_miss) {
  const int lane = threadIdx.x & 63;
  const uint64_t first = (uint64_t)blockIdx.x * kDenseThreads, step = (uint64_t)gridDim.x * kDenseThreads;
  uint32_t n_e = 0, n_k = 0;
  for (uint64_t base = first; base < slots; base += step) {
    const uint64_t s = base + threadIdx.x;
    const unsigned long long k = s < slots ? keys[s] : kDenseEmpty;
    const bool occ = k != kDenseEmpty, in = occ && roll_inside(k, box);
    n_k += (uint32_t)__popcll(__ballot(in));
    n_e += (uint32_t)__popcll(__ballot(occ && !in));
  }
  if (!n_e && !n_k) return;  // (the whole wave)
  uint32_t at_e = 0, at_k = 0;
  if (lane == 0) {
    if (n_e) at_e = atomicAdd(&cur[0], n_e);
    if (n_k) at_k = atomicAdd(&cur[1], n_k);
  }
  at_e = (uint32_t)__shfl((int)at_e, 0, 64);
  at_k = (uint32_t)__shfl((int)at_k, 0, 64);
  for (uint64_t base = first; base < slots; base += step) {
    const uint64_t s = base + threadIdx.x;
    const unsigned long long k = s < slots ? keys[s] : kDenseEmpty;  // this lane's own slot: not yet emptied
    const bool occ = k != kDenseEmpty, in = occ && roll_inside(k, box);
    const unsigned long long b_k = __ballot(in), b_e = __ballot(occ && !in);
    if (occ) {
      const unsigned long long t = tags[s];
      const uint32_t h = hits[s];
      const uint32_t ms = misses ? misses[s] : 0u;
      const double x = xyz[3 * s + 0], y = xyz[3 * s + 1], z = xyz[3 * s + 2];
      if (in) {
        const uint32_t o = at_k + (uint32_t)__popcll(b_k & lanemask_lt());
        if (o < cap_k) {  // (the count pass sized both: never false)
          s_key[o] = k;
          s_tag[o] = t;
          s_hits[o] = h;
          if (s_miss) s_miss[o] = ms;
          s_xyz[3 * (size_t)o + 0] = x;
          s_xyz[3 * (size_t)o + 1] = y;
          s_xyz[3 * (size_t)o + 2] = z;
        }
      } else {
        const uint32_t o = at_e + (uint32_t)__popcll(b_e & lanemask_lt());
        if (o < cap_e) {
          e_tag[o] = t;
          e_hits[o] = h;
          if (e_miss) e_miss[o] = ms;
          e_xyz[3 * (size_t)o + 0] = x;
          e_xyz[3 * (size_t)o + 1] = y;
          e_xyz[3 * (size_t)o + 2] = z;
        }
      }
      keys[s] = kDenseEmpty;
      tags[s] = ~0ull;
      hits[s] = 0u;
      if (misses) {
        misses[s] = 0u;
        seen[s] = 0u;
      }
    }
    at_k += (uint32_t)__popcll(b_k);
    at_e += (uint32_t)__popcll(b_e);
  }
}

// The kept voxels back into the (empty) table; cnt[3]: the device's voxel total (k_dense_fill adds to it).
__global__ __launch_bounds__(kDenseThreads) void k_roll_reinsert(
    const unsigned long long* __restrict__ s_key, const unsigned long long* __restrict__ s_tag,
    const uint32_t* __restrict__ s_hits, const double* __restrict__ s_xyz, uint32_t kept, unsigned long long* keys,
    unsigned long long* __restrict__ tags, uint32_t* __restrict__ hits, double* __restrict__ xyz, uint32_t slot_mask,
    uint32_t* __restrict__ cnt, const uint32_t* __restrict__ s_miss, uint32_t* __restrict__ misses) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  if (i == 0) cnt[3] = kept;
  if (i >= kept) return;
  const unsigned long long key = s_key[i];
  uint32_t h = (uint32_t)mix64(key) & slot_mask;
  // (bounded by the table: kept <= max_voxels leaves half the slots empty; the keys are
  // distinct, so a CAS wins an empty slot or meets another key)
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
    unsigned long long k = keys[h];
    if (k == kDenseEmpty) k = atomicCAS(&keys[h], kDenseEmpty, key);
    if (k == kDenseEmpty) {
      tags[h] = s_tag[i];
      hits[h] = s_hits[i];
      if (misses) misses[h] = s_miss[i];
      xyz[3 * (size_t)h + 0] = s_xyz[3 * (size_t)i + 0];
      xyz[3 * (size_t)h + 1] = s_xyz[3 * (size_t)i + 1];
      xyz[3 * (size_t)h + 2] = s_xyz[3 * (size_t)i + 2];
      return;
    }
    h = (h + 1) & slot_mask;
  }
}

// ---- carving (DESIGN.md §Dense map, Carving; include/fmx/fmx.h, fmx_carve_configure).  A
// return at range r proves the segment from the sensor to it empty at that moment: every
// point that the integration took also casts a ray through the table, and a stored voxel
// counts the rays that passed through it (misses).  Two more u32 per slot, allocated when
// carving is first enabled: misses, and seen = (the number of the last integration that put
// a point into the slot) + 1.  After an integration's claim and fill, on the same stream, the
// kernel boundary again the only ordering:
//
//   mark    one lane per point: seen[slot_of[i]] = seq + 1, a plain store (every writer of a
//           slot writes the same value).
//   rays    one lane per ray (adjacent columns of an organized scan have similar lengths):
//           the voxel walk of the header, one fp64 division per step (tau_k changes only
//           when cur_k does), and per examined voxel a find-only probe of the table: the key
//           word (8 B), and when it is there the seen word (4) and, unless that exempts the
//           voxel, one return-less atomicAdd on misses (4).  The walk is bound by those
//           dependent random loads, not by bytes; what hides them is waves in flight, so the
//           walk's state stays in registers (no dynamically indexed array).
//
// The launch's counters: rays rides in the ticket word as the fill's count does; steps,
// misses and exempt are 64-bit, so each wave adds its sums with one atomic per counter and
// WAITS for them (returning atomics: they have been performed when the wave goes on) before
// the block's barrier, and the block's ticket follows the barrier.  The block that finds
// every ticket in therefore finds every sum in, reads them with device-scope loads,
// publishes and re-arms.  The barrier also stands behind every lane's read of its point.
//
// The result does not depend on the order the lanes run in: the set of (ray, voxel) pairs is
// fixed by the definition, keys and seen do not change during the launch, misses is a sum.
//
// Look-ahead: a lane's walk is one dependent chain only in its arithmetic; which voxels it
// examines does not depend on what the lookups return.  So the lane walks FMX_CARVE_AHEAD
// voxels, issues their home-slot loads back to back, and only then looks at what came back
// (a chain past the home slot is then followed load by load).  FMX_CARVE_AHEAD=1 builds the
// plain form, one load in flight per lane: about 1.4x this form's time per C4 carve at
// 0.2 m voxels, same box, alternated; 8 is within 2 % of 4 and costs 24 more registers per
// lane (profiles/carve_ahead_ab.json).  Sharing one atomic among lanes that examine the same
// voxel, as the claim's in-wave merge does, was not built: in that workload about 2 % of the
// examined voxels are present at all and under 1 % take an atomic (profiles/carve_cost.json).
#ifndef FMX_CARVE_AHEAD
#define FMX_CARVE_AHEAD 4
#endif
struct CarveArgs {
  double max2;
  uint32_t margin, stride;
  uint32_t exempt;  // seq + 1 of the integration whose voxels are exempt; 0: none are
};

__global__ __launch_bounds__(kDenseThreads) void k_carve_mark(const uint32_t* __restrict__ slot_of, uint32_t n,
                                                              uint32_t mark, uint32_t* __restrict__ seen) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = slot_of[i];
  if (slot != kDenseDropped) seen[slot] = mark;
}

__device__ __forceinline__ unsigned long long carve_add_wait(unsigned long long* p, unsigned long long v) {
  const unsigned long long r = __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::"v"(r) : "memory");  // the value is back: the add has been performed
  return r;
}

// Find only, from the home slot h whose key word k is already here (bounded by the table: the
// load is at most 1/2, a chain meets an empty slot).  0 absent, 1 a miss counted, 2 exempt.
__device__ __forceinline__ int carve_find(unsigned long long key, uint32_t h, unsigned long long k,
                                          const unsigned long long* __restrict__ keys, uint32_t slot_mask, uint32_t exempt,
                                          const uint32_t* __restrict__ seen, uint32_t* misses) {
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
    if (k == key) {
      if (exempt && seen[h] == exempt) return 2;
      atomicAdd(&misses[h], 1u);  // result unused: return-less
      return 1;
    }
    if (k == kDenseEmpty) return 0;
    h = (h + 1) & slot_mask;
    k = keys[h];
  }
  return 0;
}

// cnt: {-, steps, misses, exempt, ticket << 32 | rays}; res (pinned, device-visible): {rays,
// steps, misses, exempt}; flag: the completion word, seq_flag its value for this launch
__global__ __launch_bounds__(kDenseThreads) void k_carve_rays(const float4* __restrict__ pts, uint32_t n, DenseArgs a,
                                                              CarveArgs cv, const unsigned long long* __restrict__ keys,
                                                              const uint32_t* __restrict__ seen, uint32_t* misses,
                                                              unsigned long long* cnt, unsigned long long* __restrict__ res,
                                                              uint32_t* flag, uint32_t seq_flag) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  bool ray = false;
  uint32_t nex = 0;  // voxels to examine
  int c0 = 0, c1 = 0, c2 = 0, b0 = 0, b1 = 0, b2 = 0, s0 = 0, s1 = 0, s2 = 0;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0, t0 = inf, t1 = inf, t2 = inf;
  if (i < n && i % cv.stride == 0) {
    const float4 p = pts[i];
    unsigned long long pkey = 0;
    if (dense_classify(p, a, &pkey) == 0 && (double)((p.x * p.x + p.y * p.y) + p.z * p.z) < cv.max2) {
      ray = true;
      double e[3];
      d_xform(a.T.m, (double)p.x, (double)p.y, (double)p.z, e);
      o0 = a.T.m[3], o1 = a.T.m[7], o2 = a.T.m[11];
      // (both in range: the host checked a, the classification b; |c| < 2^20 fits an int)
      c0 = (int)floor(o0 / a.w), c1 = (int)floor(o1 / a.w), c2 = (int)floor(o2 / a.w);
      b0 = (int)floor(e[0] / a.w), b1 = (int)floor(e[1] / a.w), b2 = (int)floor(e[2] / a.w);
      d0 = e[0] - o0, d1 = e[1] - o1, d2 = e[2] - o2;
      s0 = b0 > c0 ? 1 : -1, s1 = b1 > c1 ? 1 : -1, s2 = b2 > c2 ? 1 : -1;
      const uint32_t S = (uint32_t)abs(b0 - c0) + (uint32_t)abs(b1 - c1) + (uint32_t)abs(b2 - c2);
      nex = S > cv.margin ? S - cv.margin : 0u;
      if (c0 != b0) t0 = ((double)(c0 + (s0 > 0 ? 1 : 0)) * a.w - o0) / d0;
      if (c1 != b1) t1 = ((double)(c1 + (s1 > 0 ? 1 : 0)) * a.w - o1) / d1;
      if (c2 != b2) t2 = ((double)(c2 + (s2 > 0 ? 1 : 0)) * a.w - o2) / d2;
    }
  }
  uint32_t n_miss = 0, n_ex = 0;
  for (uint32_t s = 0; s < nex; s += (uint32_t)FMX_CARVE_AHEAD) {
    // The path does not depend on what the table holds: walk FMX_CARVE_AHEAD voxels first and
    // issue their home-slot loads together, so that many misses are in flight per lane.
    unsigned long long key[FMX_CARVE_AHEAD], k0[FMX_CARVE_AHEAD];
    uint32_t h0[FMX_CARVE_AHEAD];
#pragma unroll
    for (int u = 0; u < FMX_CARVE_AHEAD; ++u) {
      // (cur stays in the box between a and b, so each coordinate + bias is a 21-bit field)
      key[u] = ((unsigned long long)((long long)c0 + kDenseBias) << 42) |
               ((unsigned long long)((long long)c1 + kDenseBias) << 21) | (unsigned long long)((long long)c2 + kDenseBias);
      h0[u] = (uint32_t)mix64(key[u]) & a.slot_mask;
      k0[u] = s + (uint32_t)u < nex ? keys[h0[u]] : kDenseEmpty;  // (past the last examined voxel: nothing to find)
      // the axis with the smallest tau, the lowest among equal ones; only its tau changes
      if (t0 <= t1 && t0 <= t2) {
        c0 += s0;
        t0 = c0 != b0 ? ((double)(c0 + (s0 > 0 ? 1 : 0)) * a.w - o0) / d0 : inf;
      } else if (t1 <= t2) {
        c1 += s1;
        t1 = c1 != b1 ? ((double)(c1 + (s1 > 0 ? 1 : 0)) * a.w - o1) / d1 : inf;
      } else {
        c2 += s2;
        t2 = c2 != b2 ? ((double)(c2 + (s2 > 0 ? 1 : 0)) * a.w - o2) / d2 : inf;
      }
    }
#pragma unroll
    for (int u = 0; u < FMX_CARVE_AHEAD; ++u) {
      const int hit = carve_find(key[u], h0[u], k0[u], keys, a.slot_mask, cv.exempt, seen, misses);
      n_miss += hit == 1 ? 1u : 0u;
      n_ex += hit == 2 ? 1u : 0u;
    }
  }
  // (per wave: at most 64 * 3 * 2^21 steps, so the 32-bit sums cannot wrap)
  const uint32_t w_rays = (uint32_t)__popcll(__ballot(ray));
  const uint32_t w_steps = wave_sum(nex), w_miss = wave_sum(n_miss), w_ex = wave_sum(n_ex);
  if ((threadIdx.x & 63) == 0) {
    if (w_steps) carve_add_wait(&cnt[1], w_steps);
    if (w_miss) carve_add_wait(&cnt[2], w_miss);
    if (w_ex) carve_add_wait(&cnt[3], w_ex);
  }
  __shared__ uint32_t sh_rays[kDenseThreads / 64];
  if ((threadIdx.x & 63) == 0) sh_rays[threadIdx.x >> 6] = w_rays;
  // (every lane's read of pts has returned, and every wave's sums are in, by this barrier)
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t b_rays = 0;
  for (int wv = 0; wv < kDenseThreads / 64; ++wv) b_rays += sh_rays[wv];
  const unsigned long long mine = (1ull << 32) | (unsigned long long)b_rays;
  const unsigned long long all = atomicAdd(&cnt[4], mine) + mine;
  if ((uint32_t)(all >> 32) == gridDim.x) {  // every other block's ticket, so its sums too, are in
    const unsigned long long steps = __hip_atomic_load(&cnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long miss = __hip_atomic_load(&cnt[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long ex = __hip_atomic_load(&cnt[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cnt[1] = cnt[2] = cnt[3] = cnt[4] = 0;
    host_store(&res[0], (unsigned long long)(uint32_t)all);
    host_store(&res[1], steps);
    host_store(&res[2], miss);
    host_store(&res[3], ex);
    publish_flag(flag, seq_flag);
  }
}

// ---- probing (DESIGN.md §Dense map, Probing; include/fmx/fmx.h, fmx_probe_points).  The read
// path: neither launch writes to the table's arrays, so both commute with each other and
// repeat bit for bit.  One launch per call, on the context stream behind whatever
// integration or roll is queued there.
//
//   points  one lane per point: classify it (the integration's rule without the gate), one
//           find-only probe of the table; hits, misses, tag and point are loaded only on a
//           key match.
//   rays    one lane per ray: the carve's walk from the sensor's voxel to the point's voxel,
//           which is examined too, its state in registers as in k_carve_rays (no dynamically
//           indexed array, no LDS, no scratch).  The lane stops at the first voxel that is
//           present and solid under the filter; each step remembers the tau it was taken at,
//           so the hit carries the parameter at which the ray entered its voxel.
//
// Look-ahead, as the carve's: the path does not depend on what the table holds, so the lane
// walks FMX_PROBE_AHEAD voxels, issues their home-slot key loads back to back and then
// examines them in order.  A voxel behind the hit has been loaded and is never looked at:
// the outputs and `steps` are the definition's, whatever was loaded ahead
// (FMX_PROBE_AHEAD=1 builds the plain form; tools/probe_cost.py compares the two).
//
// Outputs are structure-of-arrays, each entry written by the lane that owns the index, zeros
// where no voxel is reported; the only shared words are the counters, one atomic per wave
// and counter (ballot + popcount, the steps a wave sum).
#ifndef FMX_PROBE_AHEAD
#define FMX_PROBE_AHEAD 4
#endif

__device__ __forceinline__ unsigned long long dense_key(int cx, int cy, int cz) {
  return ((unsigned long long)((long long)cx + kDenseBias) << 42) | ((unsigned long long)((long long)cy + kDenseBias) << 21) |
         (unsigned long long)((long long)cz + kDenseBias);
}

// dense_classify without the gate: 0 in range (wp the world point, v its voxel), 1 invalid, 3
// out of range
__device__ __forceinline__ int probe_classify(const float4 p, const DenseArgs& a, double wp[3], int v[3]) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) || (p.x == 0.0f && p.y == 0.0f && p.z == 0.0f)) return 1;
  d_xform(a.T.m, (double)p.x, (double)p.y, (double)p.z, wp);
  const double cx = floor(wp[0] / a.w), cy = floor(wp[1] / a.w), cz = floor(wp[2] / a.w);
  // in fp64, before the cast (a NaN or an infinity fails the comparison)
  if (!(fabs(cx) < kDenseLimit && fabs(cy) < kDenseLimit && fabs(cz) < kDenseLimit)) return 3;
  v[0] = (int)cx, v[1] = (int)cy, v[2] = (int)cz;
  return 0;
}

// Find only, from the home slot h whose key word k is already here (bounded by the table: the
// load is at most 1/2, a chain meets an empty slot): the key's slot, or the dropped marker.
__device__ __forceinline__ uint32_t probe_find(unsigned long long key, uint32_t h, unsigned long long k,
                                               const unsigned long long* __restrict__ keys, uint32_t slot_mask) {
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
    if (k == key) return h;
    if (k == kDenseEmpty) return kDenseDropped;
    h = (h + 1) & slot_mask;
    k = keys[h];
  }
  return kDenseDropped;
}

// Point i's voxel fields: those of `slot` (h its hit count, already here), zeros for the
// dropped marker.
__device__ __forceinline__ void probe_store(const ProbeOut& o, uint32_t i, uint32_t slot, uint32_t h, const DenseTake& tk,
                                            const unsigned long long* __restrict__ tags,
                                            const double* __restrict__ xyz) {
  const bool have = slot != kDenseDropped;
  if (o.tag) o.tag[i] = have ? tags[slot] : 0ull;
  if (o.hits) o.hits[i] = h;
  if (o.misses) o.misses[i] = have ? dense_misses(tk, slot) : 0u;
  if (o.xyz) {
    double* q = o.xyz + 3 * (size_t)i;
    q[0] = have ? xyz[3 * (size_t)slot + 0] : 0.0;
    q[1] = have ? xyz[3 * (size_t)slot + 1] : 0.0;
    q[2] = have ? xyz[3 * (size_t)slot + 2] : 0.0;
  }
}

// cnt: {absent, filtered, solid, out_of_range, invalid}
__global__ __launch_bounds__(kDenseThreads) void k_probe_points(const float4* __restrict__ pts, uint32_t n, DenseArgs a,
                                                                DenseTake tk,
                                                                const unsigned long long* __restrict__ keys,
                                                                const unsigned long long* __restrict__ tags,
                                                                const uint32_t* __restrict__ hits,
                                                                const double* __restrict__ xyz, ProbeOut o,
                                                                unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  int st = -1;  // past the end
  if (i < n) {
    double wp[3];
    int v[3];
    const int cls = probe_classify(pts[i], a, wp, v);
    uint32_t slot = kDenseDropped, h = 0;
    if (cls == 0) {
      const unsigned long long key = dense_key(v[0], v[1], v[2]);
      const uint32_t h0 = (uint32_t)mix64(key) & a.slot_mask;
      slot = probe_find(key, h0, keys[h0], keys, a.slot_mask);
      st = FMX_PROBE_ABSENT;
      if (slot != kDenseDropped) {
        h = hits[slot];
        st = dense_take(tk, h, slot) ? FMX_PROBE_SOLID : FMX_PROBE_FILTERED;
      }
    } else {
      st = cls == 1 ? FMX_PROBE_INVALID : FMX_PROBE_OUT_OF_RANGE;
    }
    o.state[i] = (uint8_t)st;
    probe_store(o, i, slot, h, tk, tags, xyz);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned long long b = __ballot(st == k);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt[k], (unsigned long long)__popcll(b));  // results unused: return-less
  }
}

// One step of the carve's walk: the axis with the smallest tau, the lowest among equal ones;
// only its tau changes.  tin: the tau the step was taken at, where the ray enters the new voxel.
__device__ __forceinline__ void probe_step(int& c0, int& c1, int& c2, double& t0, double& t1, double& t2, double& tin,
                                           int b0, int b1, int b2, int s0, int s1, int s2, double o0, double o1,
                                           double o2, double d0, double d1, double d2, double w, double inf) {
  if (t0 <= t1 && t0 <= t2) {
    tin = t0;
    c0 += s0;
    t0 = c0 != b0 ? ((double)(c0 + (s0 > 0 ? 1 : 0)) * w - o0) / d0 : inf;
  } else if (t1 <= t2) {
    tin = t1;
    c1 += s1;
    t1 = c1 != b1 ? ((double)(c1 + (s1 > 0 ? 1 : 0)) * w - o1) / d1 : inf;
  } else {
    tin = t2;
    c2 += s2;
    t2 = c2 != b2 ? ((double)(c2 + (s2 > 0 ? 1 : 0)) * w - o2) / d2 : inf;
  }
}

// cnt: {hit, clear, out_of_range, invalid, steps}
__global__ __launch_bounds__(kDenseThreads) void k_probe_rays(const float4* __restrict__ pts, uint32_t n, DenseArgs a,
                                                              DenseTake tk, uint32_t skip,
                                                              const unsigned long long* __restrict__ keys,
                                                              const unsigned long long* __restrict__ tags,
                                                              const uint32_t* __restrict__ hits,
                                                              const double* __restrict__ xyz, ProbeOut o,
                                                              unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  int cls = -1;      // past the end
  uint32_t nex = 0;  // voxels to examine: v_skip ... v_S
  int c0 = 0, c1 = 0, c2 = 0, b0 = 0, b1 = 0, b2 = 0, s0 = 0, s1 = 0, s2 = 0;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0, t0 = inf, t1 = inf, t2 = inf, tin = 0.0;
  if (i < n) {
    double e[3];
    int b[3];
    cls = probe_classify(pts[i], a, e, b);
    if (cls == 0) {
      o0 = a.T.m[3], o1 = a.T.m[7], o2 = a.T.m[11];
      // (both in range: the host checked a, the classification b; |c| < 2^20 fits an int)
      c0 = (int)floor(o0 / a.w), c1 = (int)floor(o1 / a.w), c2 = (int)floor(o2 / a.w);
      b0 = b[0], b1 = b[1], b2 = b[2];
      d0 = e[0] - o0, d1 = e[1] - o1, d2 = e[2] - o2;
      s0 = b0 > c0 ? 1 : -1, s1 = b1 > c1 ? 1 : -1, s2 = b2 > c2 ? 1 : -1;
      const uint32_t S = (uint32_t)abs(b0 - c0) + (uint32_t)abs(b1 - c1) + (uint32_t)abs(b2 - c2);
      if (c0 != b0) t0 = ((double)(c0 + (s0 > 0 ? 1 : 0)) * a.w - o0) / d0;
      if (c1 != b1) t1 = ((double)(c1 + (s1 > 0 ? 1 : 0)) * a.w - o1) / d1;
      if (c2 != b2) t2 = ((double)(c2 + (s2 > 0 ? 1 : 0)) * a.w - o2) / d2;
      if (skip <= S) {
        nex = S - skip + 1u;
        for (uint32_t s = 0; s < skip; ++s)  // the skipped voxels: walked, not looked up
          probe_step(c0, c1, c2, t0, t1, t2, tin, b0, b1, b2, s0, s1, s2, o0, o1, o2, d0, d1, d2, a.w, inf);
      }
    }
  }
  bool hit = false;
  uint32_t h_at = 0, h_slot = kDenseDropped, h_hits = 0;  // the hit: its place among the examined, its slot and hit count
  double h_t = inf;
  for (uint32_t s = 0; s < nex && !hit; s += (uint32_t)FMX_PROBE_AHEAD) {
    unsigned long long key[FMX_PROBE_AHEAD], k0[FMX_PROBE_AHEAD];
    uint32_t h0[FMX_PROBE_AHEAD];
    double te[FMX_PROBE_AHEAD];
#pragma unroll
    for (int u = 0; u < FMX_PROBE_AHEAD; ++u) {
      // (cur stays in the box between a and b while s + u < nex, so each coordinate + bias is a
      // 21-bit field; past the end voxel the key is not used and the masked slot is not loaded)
      key[u] = dense_key(c0, c1, c2);
      h0[u] = (uint32_t)mix64(key[u]) & a.slot_mask;
      k0[u] = s + (uint32_t)u < nex ? keys[h0[u]] : kDenseEmpty;
      te[u] = tin;
      probe_step(c0, c1, c2, t0, t1, t2, tin, b0, b1, b2, s0, s1, s2, o0, o1, o2, d0, d1, d2, a.w, inf);
    }
#pragma unroll
    for (int u = 0; u < FMX_PROBE_AHEAD; ++u) {
      if (!hit && s + (uint32_t)u < nex) {
        const uint32_t slot = probe_find(key[u], h0[u], k0[u], keys, a.slot_mask);
        if (slot != kDenseDropped) {
          const uint32_t h = hits[slot];
          if (dense_take(tk, h, slot)) {  // (present and not solid: transparent)
            hit = true;
            h_at = s + (uint32_t)u;
            h_slot = slot;
            h_hits = h;
            h_t = te[u];
          }
        }
      }
    }
  }
  int st = -1;
  if (i < n) {
    st = cls == 1 ? FMX_PROBE_INVALID : cls == 3 ? FMX_PROBE_OUT_OF_RANGE : hit ? FMX_PROBE_SOLID : FMX_PROBE_ABSENT;
    o.state[i] = (uint8_t)st;
    if (o.step) o.step[i] = hit ? skip + h_at : FMX_PROBE_NO_STEP;
    if (o.t) o.t[i] = h_t;
    probe_store(o, i, h_slot, h_hits, tk, tags, xyz);
  }
  // (per wave: at most 64 * (3 * 2^21 + 1) examined voxels, so the 32-bit sum cannot wrap)
  const uint32_t w_steps = wave_sum(hit ? h_at + 1u : nex);
  const unsigned long long bh = __ballot(st == FMX_PROBE_SOLID), bc = __ballot(st == FMX_PROBE_ABSENT),
                           bo = __ballot(st == FMX_PROBE_OUT_OF_RANGE), bi = __ballot(st == FMX_PROBE_INVALID);
  if ((threadIdx.x & 63) == 0) {  // results unused: return-less
    if (bh) atomicAdd(&cnt[0], (unsigned long long)__popcll(bh));
    if (bc) atomicAdd(&cnt[1], (unsigned long long)__popcll(bc));
    if (bo) atomicAdd(&cnt[2], (unsigned long long)__popcll(bo));
    if (bi) atomicAdd(&cnt[3], (unsigned long long)__popcll(bi));
    if (w_steps) atomicAdd(&cnt[4], (unsigned long long)w_steps);
  }
}

// ---- nearest (DESIGN.md §Dense map, Nearest; include/fmx/fmx.h, fmx_nearest_voxels).  The
// nearest solid representative in the cube of cells around a point's own voxel.  Read only, one
// launch per call on the context stream, as the probes.
//
// A group of FMX_NEAREST_LANES adjacent lanes serves one point.  The cube is enumerated by
// Chebyshev shell s = max |d_k| from the offset list (nearest_host.hpp: sorted by shell, built
// once by the host, 4 B per cell, resident in the caches); the lanes of a group stride through
// a shell's cells.  Which cells a point examines does not depend on what the table holds, so a
// lane issues FMX_NEAREST_AHEAD home-slot key loads back to back and then examines them: hits
// on a key match only, misses only under a ratio filter (dense_take), the representative only
// for a solid voxel.  Each lane keeps its best (d2 bits, key, slot); d2 >= 0, so its bit
// pattern orders like its value, and the pair is reduced lexicographically over the group by an
// xor butterfly after every shell s >= 1 and after the last one.  The order of visits plays no
// part: the minimum of a set is the same however it is split.
//
// Early stop: after shell s >= 1 a group is done once its best d2, or max_dist2, is below
// (1 - 2^-20) (s w)^2: every cell of a later shell differs from the own voxel by s + 1 or more
// on one axis, so its representative is farther than (s - 2^-32) w on that axis and its
// computed d2 is strictly larger than that bound (DESIGN.md has the derivation): neither the
// minimum nor a tie can change.  FMX_NEAREST_STOP=0 builds the form that walks every shell.
//
// The shell loop is uniform over the wave (it ends when every group of the wave is done; a
// done group idles), so every lane meets every shuffle.  No LDS, no scratch, no dynamically
// indexed array.  The group's first lane writes the outputs and loads the winner's remaining
// fields once; the counters get one return-less atomic per wave and counter (ballot +
// popcount, the lookups a wave sum).
#ifndef FMX_NEAREST_LANES
#define FMX_NEAREST_LANES 4
#endif
#ifndef FMX_NEAREST_AHEAD
#define FMX_NEAREST_AHEAD 4
#endif
#ifndef FMX_NEAREST_STOP
#define FMX_NEAREST_STOP 1
#endif
static_assert(FMX_NEAREST_LANES >= 1 && FMX_NEAREST_LANES <= 64 && (FMX_NEAREST_LANES & (FMX_NEAREST_LANES - 1)) == 0,
              "FMX_NEAREST_LANES is a power of two from 1 to 64");
static_assert(FMX_NEAREST_AHEAD >= 1, "FMX_NEAREST_AHEAD is at least 1");
#ifndef FMX_NEAREST_BLOCKS
#define FMX_NEAREST_BLOCKS 2048
#endif
constexpr int kNearestBlocks = FMX_NEAREST_BLOCKS;  // the grid's cap: a grid stride beyond it

// The walk over a range of the cube: the cells [lo, hi) of the offset list around the cell c,
// every L-th of them from lo + gl, with the look-ahead described above; each present voxel that
// is solid under tk goes to visit(key, slot).  `looked` grows by the cells looked up.  Shared by
// nearest_search (a shell per call) and k_normals_build (the whole cube in one).
template <uint32_t L, class Visit>
__device__ __forceinline__ void cube_visit(uint32_t lo, uint32_t hi, uint32_t gl, int c0, int c1, int c2, uint32_t slot_mask,
                                           const DenseTake& tk, const uint32_t* __restrict__ offs,
                                           const unsigned long long* __restrict__ keys,
                                           const uint32_t* __restrict__ hits, unsigned long long& looked, Visit&& visit) {
  constexpr int kLimit = (1 << 20) - 1;
  for (uint32_t base = lo + gl; base < hi; base += L * (uint32_t)FMX_NEAREST_AHEAD) {
    unsigned long long key[FMX_NEAREST_AHEAD], k0[FMX_NEAREST_AHEAD];
    uint32_t h0[FMX_NEAREST_AHEAD];
    bool ok[FMX_NEAREST_AHEAD];
#pragma unroll
    for (int u = 0; u < FMX_NEAREST_AHEAD; ++u) {
      const uint32_t at = base + (uint32_t)u * L;
      // (at < hi <= (2 reach + 1)^3, the list's length: the host checked the reach)
      const uint32_t od = at < hi ? offs[at] : 0u;
      const int x = c0 + (int)(od & 255u) - FMX_NEAREST_MAX_REACH, y = c1 + (int)((od >> 8) & 255u) - FMX_NEAREST_MAX_REACH,
                z = c2 + (int)((od >> 16) & 255u) - FMX_NEAREST_MAX_REACH;
      // a cell that cannot be stored is skipped (each coordinate + bias is then a 21-bit field)
      ok[u] = at < hi && abs(x) < kLimit && abs(y) < kLimit && abs(z) < kLimit;
      key[u] = dense_key(x, y, z);
      h0[u] = (uint32_t)mix64(key[u]) & slot_mask;
      k0[u] = ok[u] ? keys[h0[u]] : kDenseEmpty;
      looked += ok[u] ? 1ull : 0ull;
    }
#pragma unroll
    for (int u = 0; u < FMX_NEAREST_AHEAD; ++u) {
      if (ok[u]) {
        const uint32_t slot = probe_find(key[u], h0[u], k0[u], keys, slot_mask);
        if (slot != kDenseDropped && dense_take(tk, hits[slot], slot)) visit(key[u], slot);
      }
    }
  }
}

// One point group's search, the per-trip body under search_winner: the shell loop,
// the look-ahead loads, the group butterfly and the early stop, as described above.  cls: the
// point's class (0: in range, p its world point and c its own voxel; anything else: no point
// to search for, the group idles); gl: the lane's place in
// its group of L.  On return every lane of the group holds the group's best (b_bits, b_key,
// b_slot), untouched when nothing was admitted; `looked` has grown by this lane's lookups.
// Every lane of the wave calls it, a group without a point idling: the loop is wave-uniform.
template <uint32_t L>
__device__ __forceinline__ void nearest_search(int cls, double p0, double p1, double p2, int c0, int c1, int c2,
                                               uint32_t gl, const DenseArgs& a, const DenseTake& tk, uint32_t reach,
                                               double max_d2, const uint32_t* __restrict__ offs,
                                               const unsigned long long* __restrict__ keys,
                                               const uint32_t* __restrict__ hits, const double* __restrict__ xyz,
                                               unsigned long long& b_bits, unsigned long long& b_key, uint32_t& b_slot,
                                               unsigned long long& looked) {
  bool done = cls != 0;
  for (uint32_t s = 0; s <= reach; ++s) {
    if (!__any(!done)) break;  // (the whole wave)
    if (!done) {
      const uint32_t lo = s ? (2u * s - 1u) * (2u * s - 1u) * (2u * s - 1u) : 0u, hi = (2u * s + 1u) * (2u * s + 1u) * (2u * s + 1u);
      cube_visit<L>(lo, hi, gl, c0, c1, c2, a.slot_mask, tk, offs, keys, hits, looked,
                    [&](unsigned long long key, uint32_t slot) {
                      const double e0 = xyz[3 * (size_t)slot + 0] - p0, e1 = xyz[3 * (size_t)slot + 1] - p1,
                                   e2 = xyz[3 * (size_t)slot + 2] - p2;
                      const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                      const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);
                      if (d2 <= max_d2 && (bits < b_bits || (bits == b_bits && key < b_key))) {
                        b_bits = bits;
                        b_key = key;
                        b_slot = slot;
                      }
                    });
    }
    if (s == 0 && reach != 0) continue;  // (uniform: the own cell alone certifies nothing)
    // the group's best in every lane of it (a done group repeats its own: harmless)
#pragma unroll
    for (uint32_t x = 1; x < L; x <<= 1) {
      const unsigned long long ob = __shfl_xor(b_bits, (int)x, 64), ok2 = __shfl_xor(b_key, (int)x, 64);
      const uint32_t os = (uint32_t)__shfl_xor((int)b_slot, (int)x, 64);
      if (ob < b_bits || (ob == b_bits && ok2 < b_key)) {
        b_bits = ob;
        b_key = ok2;
        b_slot = os;
      }
    }
#if FMX_NEAREST_STOP
    if (s >= 1) {
      const double sw = (double)s * a.w;
      const double lim = (1.0 - 0x1p-20) * (sw * sw);
      if (__longlong_as_double((long long)b_bits) < lim || max_d2 < lim) done = true;
    }
#endif
  }
}

// A kept point of a search.  cls: -1 past the end, else probe_classify's class; p: the world
// point, s: the sensor-frame point (both of a valid point), c: the own cell (of one in range).
// Each kernel fills it in its own text: as a function of its own the same lines cost every one
// of them its register allocation (DESIGN.md §Dense map, Refining, "One text").
struct PointQuery {
  int cls = -1;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int c0 = 0, c1 = 0, c2 = 0;
};
// A search's winner: the bit pattern of its d2, its key and its slot; +inf, all ones (no stored
// key is) and the dropped marker when nothing was admitted.
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;
struct Winner {
  unsigned long long bits, key;
  uint32_t slot;
};
// nearest_search for the point q; every lane of the group holds the group's winner.
template <uint32_t L>
__device__ __forceinline__ Winner search_winner(const PointQuery& q, uint32_t gl, const DenseArgs& a, const DenseTake& tk,
                                                uint32_t reach, double max_d2, const uint32_t* __restrict__ offs,
                                                const unsigned long long* __restrict__ keys,
                                                const uint32_t* __restrict__ hits, const double* __restrict__ xyz,
                                                unsigned long long& looked) {
  Winner win{kInfBits, kDenseEmpty, kDenseDropped};
  nearest_search<L>(q.cls, q.p0, q.p1, q.p2, q.c0, q.c1, q.c2, gl, a, tk, reach, max_d2, offs, keys, hits, xyz, win.bits,
                    win.key, win.slot, looked);
  return win;
}
__device__ __forceinline__ bool found(const PointQuery& q, const Winner& win) { return q.cls == 0 && win.key != kDenseEmpty; }
// The state of a point that is there (q.cls >= 0): one of FMX_PROBE_*.
__device__ __forceinline__ int point_state(const PointQuery& q, const Winner& win) {
  return q.cls == 1 ? FMX_PROBE_INVALID : q.cls == 3 ? FMX_PROBE_OUT_OF_RANGE : found(q, win) ? FMX_PROBE_SOLID : FMX_PROBE_ABSENT;
}

constexpr int kAlignUnoriented = 5;  // a point's state beside FMX_PROBE_* (0 .. 4): found, winner without a normal

// A wave's class counts, by ballots: the same in every lane of the wave (a wave meets fewer
// than 2^32 points in all: n is below that).  st: the state in the lane that speaks for the
// point, -1 in every other.
struct ClassTally {
  uint32_t found = 0, none = 0, oor = 0, inv = 0, unor = 0;
  __device__ __forceinline__ void add(int st) {
    unor += (uint32_t)__popcll(__ballot(st == kAlignUnoriented));
    found += (uint32_t)__popcll(__ballot(st == FMX_PROBE_SOLID));
    none += (uint32_t)__popcll(__ballot(st == FMX_PROBE_ABSENT));
    oor += (uint32_t)__popcll(__ballot(st == FMX_PROBE_OUT_OF_RANGE));
    inv += (uint32_t)__popcll(__ballot(st == FMX_PROBE_INVALID));
  }
  // cnt: {found, none, out_of_range, invalid, lookups, unoriented (kCounters = 6)}: one atomic
  // per wave and counter, the lookups a wave sum (results unused: return-less).  Every lane calls.
  template <int kCounters>
  __device__ __forceinline__ void flush(unsigned long long* __restrict__ cnt, unsigned long long looked) const {
    const unsigned long long w_looked = wave_sum(looked);
    if ((threadIdx.x & 63) == 0) {
      if (found) atomicAdd(&cnt[0], (unsigned long long)found);
      if (none) atomicAdd(&cnt[1], (unsigned long long)none);
      if (oor) atomicAdd(&cnt[2], (unsigned long long)oor);
      if (inv) atomicAdd(&cnt[3], (unsigned long long)inv);
      if (w_looked) atomicAdd(&cnt[4], w_looked);
      if constexpr (kCounters == 6)
        if (unor) atomicAdd(&cnt[5], (unsigned long long)unor);
    }
  }
  // ... or the four into the wave's row of a block's LDS table (k_score), for one lane to call
  __device__ __forceinline__ void store(uint32_t (&row)[4]) const { row[0] = found, row[1] = none, row[2] = oor, row[3] = inv; }
};

// cnt: {found, none, out_of_range, invalid, lookups}.  o.t takes dist2; o.step is not used.
__global__ __launch_bounds__(kDenseThreads) void k_nearest(const float4* __restrict__ pts, uint32_t n, DenseArgs a,
                                                           DenseTake tk, uint32_t reach, double max_d2,
                                                           const uint32_t* __restrict__ offs,
                                                           const unsigned long long* __restrict__ keys,
                                                           const unsigned long long* __restrict__ tags,
                                                           const uint32_t* __restrict__ hits,
                                                           const double* __restrict__ xyz, ProbeOut o,
                                                           unsigned long long* __restrict__ cnt) {
  constexpr uint32_t L = (uint32_t)FMX_NEAREST_LANES;
  // Grid stride over the groups (64-bit: n * L may pass 2^32), uniform over the wave: it runs
  // while the wave's first group has a point.  The grid is capped (kNearestBlocks) so that the
  // counters' atomics, all on five words, are few: one per wave and launch, not per point group.
  const unsigned long long stride = (unsigned long long)gridDim.x * (unsigned long long)kDenseThreads / L;
  const unsigned long long g0 = ((unsigned long long)blockIdx.x * (unsigned long long)kDenseThreads + threadIdx.x) / L;
  const unsigned long long w0 = ((unsigned long long)blockIdx.x * (unsigned long long)kDenseThreads + (threadIdx.x & ~63u)) / L;
  const uint32_t gl = threadIdx.x & (L - 1u);  // the lane's place in its group
  unsigned long long looked = 0;
  ClassTally tally;
  for (unsigned long long it = 0; w0 + it < (unsigned long long)n; it += stride) {
    const unsigned long long g = g0 + it;
    PointQuery q;  // past the end
    if (g < (unsigned long long)n) {
      const float4 pf = pts[g];
      double wp[3];
      int v[3];
      q.cls = probe_classify(pf, a, wp, v);
      q.p0 = wp[0], q.p1 = wp[1], q.p2 = wp[2];
      if (q.cls == 0) q.c0 = v[0], q.c1 = v[1], q.c2 = v[2];
    }
    const Winner win = search_winner<L>(q, gl, a, tk, reach, max_d2, offs, keys, hits, xyz, looked);
    int st = -1;
    if (q.cls >= 0 && gl == 0) {
      const bool have = found(q, win);
      st = point_state(q, win);
      const uint32_t i = (uint32_t)g;
      o.state[i] = (uint8_t)st;
      if (o.t) o.t[i] = __longlong_as_double((long long)(have ? win.bits : kInfBits));
      const uint32_t slot = have ? win.slot : kDenseDropped;
      probe_store(o, i, slot, (have && o.hits) ? hits[slot] : 0u, tk, tags, xyz);
    }
    tally.add(st);
  }
  tally.flush<5>(cnt, looked);
}

// ---- aligning (DESIGN.md §Dense map, Aligning; include/fmx/fmx.h, fmx_align_system).  The
// nearest search fused with the point-to-point linearization against the winner: per launch
// the packed 7 x 7 system of a scan at a pose (28 doubles + the error) and five counts, nothing
// per point.  Read only, one launch per system on the context stream.
//
// A group of FMX_ALIGN_LANES adjacent lanes serves one kept point; group g has point
// i = g * every (the points in between are skipped: never loaded), so a strided launch is dense
// in lanes.  The point is a PointQuery, the search search_winner's, the winner stays in
// registers; the group's first lane runs the row step (add_rows: the winner's representative q
// loaded, the three rows of point_row<1> with X(i) the identity, p_i = q, p_j the sensor-frame
// point) into 28 fp64 accumulators that persist over the grid-stride trips.  The reduction is
// k_linearize_total's (linearize.hip): the block's sums (block_sums28: the wave's reduce-scatter,
// the block's waves added in wave order through LDS), the block partial out with
// agent-scope stores, an agent-scope ticket, the last block summing the partials in block
// order and writing the system, and the counters, to mapped host memory behind the completion
// word.  Every sum's order is fixed by n, every and the grid: the bits do not depend on the
// order the lanes run in.  The class counts are ClassTally's, as k_nearest's.
#ifndef FMX_ALIGN_LANES
#define FMX_ALIGN_LANES 1
#endif
static_assert(FMX_ALIGN_LANES >= 1 && FMX_ALIGN_LANES <= 64 && (FMX_ALIGN_LANES & (FMX_ALIGN_LANES - 1)) == 0,
              "FMX_ALIGN_LANES is a power of two from 1 to 64");
constexpr int kAlignWaves = kDenseThreads / kWave;
constexpr int kAlignLd = 32;  // doubles per block partial (28 used)
constexpr int kAlignOutCounts = 32;  // out[32..36] (..37: PlaneRows): the counters' bit patterns behind the 29 doubles

namespace {
#include "factor_rows.hpp"
}  // namespace

//
// The row kind is the template parameter of k_align, of k_refine and of the row step they
// share.  PointRows: the three point-to-point rows
// above.  PlaneRows (DESIGN.md §Dense map, Plane alignment; fmx_plane_system): the winner's
// slot also names its record of the normal snapshot (16 B more per found point); a winner
// without a normal makes the point *unoriented* (a sixth counter, nothing added), any other
// adds the one row of plane_row<1> (X(i) the identity, p_i = q, n_i = n) into the same 28 sums.
struct PointRows {
  static constexpr int kCounters = 5;
};
struct PlaneRows {
  static constexpr int kCounters = 6;
  const float4* __restrict__ nrm;  // per slot: {n0, n1, n2, flatness}, all-zero n unless oriented
};

// The row step, for the lane that speaks for a found point: the winner's representative q
// loaded, the rows of the kind added into acc (inv: 1 / sigma).  Returns the point's state:
// FMX_PROBE_SOLID, or kAlignUnoriented (PlaneRows: the winner has no normal, nothing added).
template <class Rows>
__device__ __forceinline__ int add_rows(const Rows& rows, const DenseArgs& a, const PointQuery& p, const Winner& win,
                                        const double* __restrict__ xyz, double inv, double (&acc)[32]) {
  const double q[3] = {xyz[3 * (size_t)win.slot + 0], xyz[3 * (size_t)win.slot + 1], xyz[3 * (size_t)win.slot + 2]};
  const double pj[3] = {p.s0, p.s1, p.s2}, wpj[3] = {p.p0, p.p1, p.p2};
  double H[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) H[i] = 0.0;
  if constexpr (Rows::kCounters == 6) {
    const float4 nf = rows.nrm[win.slot];
    if (nf.x == 0.0f && nf.y == 0.0f && nf.z == 0.0f) return kAlignUnoriented;
    const double ni[3] = {(double)nf.x, (double)nf.y, (double)nf.z};
    const double eye[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};  // X(i)
    double r;
    plane_row<1>(eye, a.T.m, q, ni, pj, r, H);
    accum_row<1>(H, r, inv, acc);
  } else {
#pragma unroll
    for (int r3 = 0; r3 < 3; ++r3) {
      double r;
      point_row<1>(a.T.m, a.T.m, q, pj, q, wpj, r3, r, H);  // (X(i) is not read in this mode)
      accum_row<1>(H, r, inv, acc);
    }
  }
  return FMX_PROBE_SOLID;
}

// The block's 28 sums of its lanes' acc: the wave's reduce-scatter (entry lane / 2 in the even
// lanes), then the waves added in wave order through sw.  Entry t is returned in thread t < 28
// (0.0 in the others); one barrier, which also covers what the caller stored to LDS before.
__device__ __forceinline__ double block_sums28(double (&acc)[32], double (*sw)[28]) {
  const int w = threadIdx.x / kWave, lane = lane_id();
  const double mine = wave_reduce_scatter32(acc);
  if ((lane & 1) == 0 && (lane >> 1) < 28) sw[w][lane >> 1] = mine;
  __syncthreads();
  double bp = 0.0;
  if (threadIdx.x < 28) {
    bp = sw[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < kDenseThreads / kWave; ++i) bp += sw[i][threadIdx.x];
  }
  return bp;
}

// m: the kept points, ceil(n / every).  cnt: {found, none, out_of_range, invalid, lookups,
// unoriented (PlaneRows)}, zeroed by the caller.  ticket: 0 at launch, 0 again afterwards.  out:
// mapped host memory.
template <class Rows>
__global__ __launch_bounds__(kDenseThreads) void k_align(const float4* __restrict__ pts, uint32_t m, uint32_t every,
                                                         DenseArgs a, DenseTake tk, uint32_t reach, double max_d2,
                                                         double inv, const uint32_t* __restrict__ offs,
                                                         const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ hits,
                                                         const double* __restrict__ xyz,
                                                         unsigned long long* __restrict__ cnt, double* __restrict__ bpart,
                                                         uint32_t* __restrict__ ticket, double* __restrict__ out,
                                                         uint32_t* __restrict__ flag, uint32_t seq, Rows rows) {
  constexpr uint32_t L = (uint32_t)FMX_ALIGN_LANES;
  constexpr int NG = 28;
  constexpr int kGroups = kDenseThreads / NG;  // final reduction: lane groups x 28 entries
  const unsigned long long stride = (unsigned long long)gridDim.x * (unsigned long long)kDenseThreads / L;
  const unsigned long long g0 = ((unsigned long long)blockIdx.x * (unsigned long long)kDenseThreads + threadIdx.x) / L;
  const unsigned long long w0 = ((unsigned long long)blockIdx.x * (unsigned long long)kDenseThreads + (threadIdx.x & ~63u)) / L;
  const uint32_t gl = threadIdx.x & (L - 1u);
  unsigned long long looked = 0;
  ClassTally tally;
  double acc[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) acc[i] = 0.0;
  for (unsigned long long it = 0; w0 + it < (unsigned long long)m; it += stride) {
    const unsigned long long g = g0 + it;
    PointQuery q;  // past the end
    if (g < (unsigned long long)m) {
      const float4 pf = pts[g * (unsigned long long)every];  // (g < m: the index is below n)
      double wp[3];
      int v[3];
      q.cls = probe_classify(pf, a, wp, v);
      q.p0 = wp[0], q.p1 = wp[1], q.p2 = wp[2];
      q.s0 = (double)pf.x, q.s1 = (double)pf.y, q.s2 = (double)pf.z;
      if (q.cls == 0) q.c0 = v[0], q.c1 = v[1], q.c2 = v[2];
    }
    const Winner win = search_winner<L>(q, gl, a, tk, reach, max_d2, offs, keys, hits, xyz, looked);
    int st = -1;
    if (q.cls >= 0 && gl == 0) {
      st = point_state(q, win);
      if (st == FMX_PROBE_SOLID) st = add_rows(rows, a, q, win, xyz, inv, acc);
    }
    tally.add(st);
  }
  tally.flush<Rows::kCounters>(cnt, looked);
  __shared__ double sw[kAlignWaves][NG];
  __shared__ double sq[kGroups][NG];
  __shared__ int s_last;
  const double bp = block_sums28(acc, sw);
  if (threadIdx.x < NG)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(bpart + (size_t)blockIdx.x * kAlignLd + threadIdx.x),
                       (unsigned long long)__double_as_longlong(bp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // every wave's partial stores and counter atomics are acknowledged before its block's ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  // last block: lane group j (9 of them) sums entry e of blocks j, j + 9, ...; then the group
  // sums in order
  const int nblk = gridDim.x;
  if (threadIdx.x < kGroups * NG) {
    const int e = threadIdx.x % NG, j = threadIdx.x / NG;
    double s = 0.0;
    for (int b = j; b < nblk; b += kGroups)
      s += __longlong_as_double((long long)__hip_atomic_load(
          reinterpret_cast<const unsigned long long*>(bpart + (size_t)b * kAlignLd + e), __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT));
    sq[j][e] = s;
  }
  __syncthreads();
  if (threadIdx.x < NG) {
    const int e = threadIdx.x;
    double s = sq[0][e];
#pragma unroll
    for (int j = 1; j < kGroups; ++j) s += sq[j][e];
    host_store(out + e, s);
    if (e == NG - 1) host_store(out + NG, 0.5 * s);
  } else if (threadIdx.x >= 32 && threadIdx.x < 32 + Rows::kCounters) {  // (wave 0 too: it publishes what it stored)
    const int k = threadIdx.x - 32;
    host_store(reinterpret_cast<unsigned long long*>(out) + kAlignOutCounts + k,
               __hip_atomic_load(cnt + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    publish_flag(flag, seq);
  }
}

// ---- scoring candidate poses (DESIGN.md §Dense map, Scoring; include/fmx/fmx.h,
// fmx_score_poses).  The nearest search of one staged scan at many poses: per pose one 32-byte
// record (four class counts, the sum of the winners' d2, the lookups), nothing per point.  Read
// only, two launches per chunk of poses on the context stream.
//
// A work item is one pose and one tile of kScoreTile kept points (score_host.hpp; the tile is
// the block: one lane per kept point, as k_align's FMX_ALIGN_LANES = 1).  The items of a chunk
// are tile-major (item = tile * poses + pose: neighbouring blocks share a tile's points and take
// neighbouring poses of the list; FMX_SCORE_TILE_MAJOR=0 builds the pose-major order, 8 to 15 %
// slower at 1024 poses in tools/score_cost.py --ab: the records are the same bits either way)
// and a block walks them with a grid stride under k_nearest's cap.  The item's pose comes
// from the staged pose array and is uniform over the block (item_pose); the DenseArgs around it
// goes to probe_classify and search_winner unchanged.  Reduction, every order fixed: a wave's d2 by
// wave_sum's xor butterfly (a point that found nothing adds +0.0: exact), its counts by
// ClassTally's ballots over point_state (the predicate k_nearest and k_align count by), then the block's waves in wave order through LDS, one partial record per item.
// k_score_finish then sums a pose's tiles: one wave per pose, lane l takes tiles l, l + 64, ...
// in that order, then the same butterfly.  Which block ran an item, how many poses the chunk
// holds and where the pose stands in it enter neither: a record depends on the points, the
// stride, the search and its own pose alone.  The launch boundary is the hand-off between the
// two: no ticket, no agent-scope protocol, no floating-point atomic.
#ifndef FMX_SCORE_TILE_MAJOR
#define FMX_SCORE_TILE_MAJOR 1
#endif
static_assert(kScoreTile == (uint32_t)kDenseThreads, "a tile is one block-wide pass");
static_assert(kBatchGridCap == (uint32_t)kNearestBlocks, "the score and refine grids are capped as k_nearest's");
constexpr int kScoreWaves = kDenseThreads / kWave;

// Work item `item` of `items` = poses of the chunk * tiles (uniform over the block): its tile
// and pose in the order above, the pose's 12 doubles from the staged array into a.T.  Shared by
// k_score and k_refine (FMX_SCORE_TILE_MAJOR=0 reorders both; their records do not change).
__device__ __forceinline__ void item_pose(uint32_t item, uint32_t items, uint32_t tiles, const double* __restrict__ poses,
                                          DenseArgs& a, uint32_t& tile, uint32_t& pose) {
#if FMX_SCORE_TILE_MAJOR
  const uint32_t n_poses = items / tiles;
  tile = item / n_poses, pose = item - tile * n_poses;
#else
  pose = item / tiles, tile = item - pose * tiles;
#endif
#pragma unroll
  for (int k = 0; k < 12; ++k) a.T.m[k] = poses[(size_t)pose * 12 + k];
}

// m: the kept points; tiles = ceil(m / kScoreTile); items = poses of the chunk * tiles.
// part[pose * tiles + tile]: written whole by the item's block.
__global__ __launch_bounds__(kDenseThreads) void k_score(const float4* __restrict__ pts, uint32_t m, uint32_t every,
                                                         const double* __restrict__ poses, uint32_t tiles, uint32_t items,
                                                         DenseArgs a, DenseTake tk, uint32_t reach, double max_d2,
                                                         const uint32_t* __restrict__ offs,
                                                         const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ hits,
                                                         const double* __restrict__ xyz,
                                                         fmx_pose_score* __restrict__ part) {
  __shared__ double s_d2[kScoreWaves];
  __shared__ unsigned long long s_look[kScoreWaves];
  __shared__ uint32_t s_cnt[kScoreWaves][4];
  const int w = threadIdx.x / kWave;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {  // (uniform over the block)
    uint32_t tile, pose;
    item_pose(item, items, tiles, poses, a, tile, pose);
    const unsigned long long g = (unsigned long long)tile * kScoreTile + threadIdx.x;
    PointQuery q;  // past the end
    if (g < (unsigned long long)m) {
      const float4 pf = pts[g * (unsigned long long)every];  // (g < m: the index is below n)
      double wp[3];
      int v[3];
      q.cls = probe_classify(pf, a, wp, v);
      q.p0 = wp[0], q.p1 = wp[1], q.p2 = wp[2];
      if (q.cls == 0) q.c0 = v[0], q.c1 = v[1], q.c2 = v[2];
    }
    unsigned long long looked = 0;
    const Winner win = search_winner<1u>(q, 0u, a, tk, reach, max_d2, offs, keys, hits, xyz, looked);
    const double wd = wave_sum(found(q, win) ? __longlong_as_double((long long)win.bits) : 0.0);
    const unsigned long long wl = wave_sum(looked);
    ClassTally tally;
    tally.add(q.cls >= 0 ? point_state(q, win) : -1);
    if ((threadIdx.x & 63) == 0) {
      s_d2[w] = wd;
      s_look[w] = wl;
      tally.store(s_cnt[w]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      fmx_pose_score r{s_cnt[0][0], s_cnt[0][1], s_cnt[0][2], s_cnt[0][3], s_d2[0], s_look[0]};
#pragma unroll
      for (int i = 1; i < kScoreWaves; ++i) {  // in wave order
        r.found += s_cnt[i][0], r.none += s_cnt[i][1], r.out_of_range += s_cnt[i][2], r.invalid += s_cnt[i][3];
        r.sum_d2 += s_d2[i];
        r.lookups += s_look[i];
      }
      part[(size_t)pose * tiles + tile] = r;
    }
    __syncthreads();  // (the next item writes the same words)
  }
}

// One wave per pose of the chunk: lane l sums the partial records of tiles l, l + 64, ... in
// that order, the wave by wave_sum's butterfly; lane 0 writes the pose's record.
__global__ __launch_bounds__(kDenseThreads) void k_score_finish(const fmx_pose_score* __restrict__ part, uint32_t tiles,
                                                                uint32_t poses, fmx_pose_score* __restrict__ out) {
  const uint32_t pose = blockIdx.x * (uint32_t)kScoreWaves + threadIdx.x / kWave;  // (uniform over the wave)
  if (pose >= poses) return;
  const uint32_t lane = threadIdx.x & 63u;
  fmx_pose_score r{0u, 0u, 0u, 0u, 0.0, 0ull};
  for (uint32_t t = lane; t < tiles; t += 64u) {
    const fmx_pose_score q = part[(size_t)pose * tiles + t];
    r.found += q.found, r.none += q.none, r.out_of_range += q.out_of_range, r.invalid += q.invalid;
    r.sum_d2 += q.sum_d2;
    r.lookups += q.lookups;
  }
  r.found = wave_sum(r.found), r.none = wave_sum(r.none), r.out_of_range = wave_sum(r.out_of_range),
  r.invalid = wave_sum(r.invalid);
  r.sum_d2 = wave_sum(r.sum_d2);
  r.lookups = wave_sum(r.lookups);
  if (lane == 0) out[pose] = r;
}

// ---- refining candidate poses (DESIGN.md §Dense map, Refining; include/fmx/fmx.h,
// fmx_refine_systems).  k_align's system of one staged scan at many poses: per pose one 264-byte
// record (the 28 sums and the error, the class counts, the lookups), nothing per point.  Read
// only, two launches per chunk of poses on the context stream.
//
// k_score's item scheme with k_align's rows.  A work item is one pose and one tile of
// kRefineTile kept points (refine_host.hpp), the items of a chunk tile-major, a block walking
// them with a grid stride under k_nearest's cap; the item's pose comes from the staged pose
// array, uniform over the block, into the DenseArgs (item_pose) that probe_classify and
// search_winner<1> take unchanged.  A tile is kRefineTile / 256 block-wide passes: one lane per
// kept point and pass, the rows added by add_rows, the row step k_align calls, into 28 fp64
// accumulators that are reset per item and persist over its passes, as k_align's over its
// trips.  Per item one reduction: block_sums28, as k_align's per block; the counts by
// ballots over point_state's states (in this kernel's own text: see below).  One partial record per item, written whole by the
// item's block (an item that found nothing writes zeros: the finisher reads every record).
// k_refine_finish sums a pose's tiles in an order fixed by their number, one block per pose.
// Every order is fixed by the kept points and the tile: which block ran an item, how many poses the chunk holds and
// where the pose stands in it enter nothing.  The launch boundary is the hand-off: no ticket, no
// agent-scope protocol, no floating-point atomic; nothing is shared with k_align's partials,
// ticket and counters or with the score buffers.
static_assert(kRefineTile % (uint32_t)kDenseThreads == 0, "a tile is a whole number of block-wide passes");
constexpr int kRefineWaves = kDenseThreads / kWave;
constexpr uint32_t kRefinePasses = kRefineTile / (uint32_t)kDenseThreads;

// m: the kept points; tiles = ceil(m / kRefineTile); items = poses of the chunk * tiles.
// part[pose * tiles + tile]: written whole by the item's block.
template <class Rows>
__global__ __launch_bounds__(kDenseThreads) void k_refine(const float4* __restrict__ pts, uint32_t m, uint32_t every,
                                                          const double* __restrict__ poses, uint32_t tiles, uint32_t items,
                                                          DenseArgs a, DenseTake tk, uint32_t reach, double max_d2,
                                                          double inv, const uint32_t* __restrict__ offs,
                                                          const unsigned long long* __restrict__ keys,
                                                          const uint32_t* __restrict__ hits,
                                                          const double* __restrict__ xyz, RefinePart* __restrict__ part,
                                                          Rows rows) {
  constexpr int NG = 28;
  __shared__ double sw[kRefineWaves][NG];
  __shared__ unsigned long long s_look[kRefineWaves];
  __shared__ uint32_t s_cnt[kRefineWaves][5];
  const int w = threadIdx.x / kWave;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {  // (uniform over the block)
    uint32_t tile, pose;
    item_pose(item, items, tiles, poses, a, tile, pose);
    unsigned long long looked = 0;
    // (the same in every lane of the wave.  ClassTally's counts, in this kernel's own text: with
    // the struct the kernel allocates 103 / 133 VGPRs, not 144 / 213, and runs at another
    // occupancy, faster for some batch sizes and slower for others)
    uint32_t n_found = 0, n_none = 0, n_oor = 0, n_inv = 0, n_unor = 0;
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = 0.0;
    const unsigned long long w0 = (unsigned long long)tile * kRefineTile + (threadIdx.x & ~63u);
    for (uint32_t ps = 0; ps < kRefinePasses; ++ps) {
      const unsigned long long off = (unsigned long long)ps * kDenseThreads;
      if (w0 + off >= (unsigned long long)m) break;  // (uniform over the wave)
      const unsigned long long g = w0 + off + (threadIdx.x & 63u);
      PointQuery q;  // past the end
      if (g < (unsigned long long)m) {
        const float4 pf = pts[g * (unsigned long long)every];  // (g < m: the index is below n)
        double wp[3];
        int v[3];
        q.cls = probe_classify(pf, a, wp, v);
        q.p0 = wp[0], q.p1 = wp[1], q.p2 = wp[2];
        q.s0 = (double)pf.x, q.s1 = (double)pf.y, q.s2 = (double)pf.z;
        if (q.cls == 0) q.c0 = v[0], q.c1 = v[1], q.c2 = v[2];
      }
      const Winner win = search_winner<1u>(q, 0u, a, tk, reach, max_d2, offs, keys, hits, xyz, looked);
      int st = -1;
      if (q.cls >= 0) {
        st = point_state(q, win);
        if (st == FMX_PROBE_SOLID) st = add_rows(rows, a, q, win, xyz, inv, acc);
      }
      if constexpr (Rows::kCounters == 6) n_unor += (uint32_t)__popcll(__ballot(st == kAlignUnoriented));
      n_found += (uint32_t)__popcll(__ballot(st == FMX_PROBE_SOLID));
      n_none += (uint32_t)__popcll(__ballot(st == FMX_PROBE_ABSENT));
      n_oor += (uint32_t)__popcll(__ballot(st == FMX_PROBE_OUT_OF_RANGE));
      n_inv += (uint32_t)__popcll(__ballot(st == FMX_PROBE_INVALID));
    }
    const unsigned long long wl = wave_sum(looked);
    if (lane_id() == 0) {
      s_look[w] = wl;
      s_cnt[w][0] = n_found, s_cnt[w][1] = n_none, s_cnt[w][2] = n_oor, s_cnt[w][3] = n_inv, s_cnt[w][4] = n_unor;
    }
    const double bp = block_sums28(acc, sw);
    RefinePart* const rec = part + ((size_t)pose * tiles + tile);
    if (threadIdx.x < NG) {
      rec->S[threadIdx.x] = bp;
    } else if (threadIdx.x >= 32 && threadIdx.x < 32 + 5) {
      const int k = threadIdx.x - 32;
      uint32_t s = s_cnt[0][k];
#pragma unroll
      for (int i = 1; i < kRefineWaves; ++i) s += s_cnt[i][k];
      rec->cnt[k] = s;
    } else if (threadIdx.x == 32 + 5) {
      unsigned long long s = s_look[0];
#pragma unroll
      for (int i = 1; i < kRefineWaves; ++i) s += s_look[i];
      rec->reserved = 0u;
      rec->lookups = s;
    }
    __syncthreads();  // (the next item writes the same words)
  }
}

// One block per pose of the chunk.  Wave w takes the pose's tiles t = w, w + 4, ...; its lane
// e < 28 sums entry e of their partial records in four running sums (over every fourth of
// them) closed as (s0 + s1) + (s2 + s3), lanes 32 .. 36 the counts, lane 37 the lookups; then
// wave 0 adds the four waves' results as (w0 + w1) + (w2 + w3) from LDS and writes the pose's
// record.  Every order is fixed by `tiles` alone; a whole scan's thousand tiles are sixteen
// chains of adds, not one.
__global__ __launch_bounds__(kDenseThreads) void k_refine_finish(const RefinePart* __restrict__ part, uint32_t tiles,
                                                                 uint32_t poses, fmx_refine_system* __restrict__ out) {
  __shared__ double sq[kRefineWaves][28];
  __shared__ unsigned long long sk[kRefineWaves][6];
  static_assert(kRefineWaves == 4, "the finisher closes four waves");
  const uint32_t pose = blockIdx.x;  // (pose < poses: the grid is the poses)
  const uint32_t w = threadIdx.x / kWave, lane = threadIdx.x & 63u;
  const RefinePart* const p = part + (size_t)pose * tiles;
  if (lane < 28u) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t t = w;
    for (; t + 12u < tiles; t += 16u) {
      s[0] += p[t].S[lane];
      s[1] += p[t + 4u].S[lane];
      s[2] += p[t + 8u].S[lane];
      s[3] += p[t + 12u].S[lane];
    }
    for (int i = 0; i < 3; ++i, t += 4u)
      if (t < tiles) s[i] += p[t].S[lane];
    sq[w][lane] = (s[0] + s[1]) + (s[2] + s[3]);
  } else if (lane >= 32u && lane < 37u) {
    unsigned long long s = 0ull;
    for (uint32_t t = w; t < tiles; t += 4u) s += p[t].cnt[lane - 32u];
    sk[w][lane - 32u] = s;
  } else if (lane == 37u) {
    unsigned long long s = 0ull;
    for (uint32_t t = w; t < tiles; t += 4u) s += p[t].lookups;
    sk[w][5] = s;
  }
  __syncthreads();
  if (w != 0u) return;
  fmx_refine_system* const o = out + pose;
  if (lane < 28u) {
    const double s = (sq[0][lane] + sq[1][lane]) + (sq[2][lane] + sq[3][lane]);
    o->S[lane] = s;
    if (lane == 27u) o->S[28] = 0.5 * s;
  } else if (lane >= 32u && lane < 38u) {
    const uint32_t k = lane - 32u;
    const unsigned long long s = (sk[0][k] + sk[1][k]) + (sk[2][k] + sk[3][k]);
    if (k < 5u)  // found .. unoriented
      reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(o) + offsetof(fmx_refine_system, found))[k] = (uint32_t)s;
    else {
      o->reserved = 0u;
      o->lookups = s;
    }
  }
}

// ---- surface normals (DESIGN.md §Dense map, Normals; include/fmx/fmx.h, fmx_normals_build).
// One record per table slot from the table as it stands: read only, one launch per build.
//
// One lane per slot, a grid stride over the slots (the grid is capped like the downloads').  A
// lane whose slot holds a solid voxel walks the whole cube around the voxel's own cell with
// cube_visit (the offset list in its order, FMX_NEAREST_AHEAD key loads in flight, no early
// stop: every cell counts) and adds each admitted neighbour's e = q - q0 into k, S1 and S2 in
// that order: the sums depend on the offset list alone, not on the order lanes run in.  Then the
// covariance, smallest_eigvec's cyclic Jacobi on it in fp64, the sign rule and the class.  Every
// occupied slot's record is written (a filtered voxel's is all zeros: a later search under a
// wider filter may name it); an empty slot's is not, and is never read: while the snapshot is
// current the same slots are empty, and k_align and the download index occupied slots only
// (the writes of a mostly empty table were most of the build's bytes).  The lanes of empty slots, half the table and more,
// idle through the walk: not compacted (the walk's loads, not the lanes, bound the launch; see
// DESIGN.md).  No LDS, no scratch, no dynamically indexed array; the counters get one
// return-less atomic per wave and counter.
struct NormalsArgs {
  uint32_t reach, min_support;
  double max_d2, max_flat;
};
constexpr int kNormalOriented = 0, kNormalFlat = 1, kNormalSparse = 2, kNormalFiltered = 3;

// cnt: {oriented, flat_rejected, sparse, filtered, lookups}, zeroed by the caller
__global__ __launch_bounds__(kDenseThreads) void k_normals_build(const unsigned long long* __restrict__ keys,
                                                                 const uint32_t* __restrict__ hits,
                                                                 const double* __restrict__ xyz, uint64_t slots,
                                                                 DenseTake tk, NormalsArgs na,
                                                                 const uint32_t* __restrict__ offs,
                                                                 float4* __restrict__ nrm, uint32_t* __restrict__ support,
                                                                 unsigned long long* __restrict__ cnt) {
  const uint32_t slot_mask = (uint32_t)(slots - 1);
  const uint32_t side = 2u * na.reach + 1u, cells = side * side * side;
  unsigned long long looked = 0;
  uint32_t n_cls[4] = {0, 0, 0, 0};  // (the same in every lane of the wave)
  for (uint64_t base = (uint64_t)blockIdx.x * kDenseThreads; base < slots; base += (uint64_t)gridDim.x * kDenseThreads) {
    const uint64_t s = base + threadIdx.x;
    const unsigned long long key0 = s < slots ? keys[s] : kDenseEmpty;
    int cls = -1;  // empty, or past the end
    float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t k = 0;
    if (key0 != kDenseEmpty) {
      cls = kNormalFiltered;
      if (dense_take(tk, hits[s], s)) {
        const int c0 = (int)((key0 >> 42) & 0x1FFFFFull) - (int)kDenseBias, c1 = (int)((key0 >> 21) & 0x1FFFFFull) - (int)kDenseBias,
                  c2 = (int)(key0 & 0x1FFFFFull) - (int)kDenseBias;
        const double q0 = xyz[3 * s + 0], q1 = xyz[3 * s + 1], q2 = xyz[3 * s + 2];
        double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
        cube_visit<1u>(0u, cells, 0u, c0, c1, c2, slot_mask, tk, offs, keys, hits, looked,
                       [&](unsigned long long, uint32_t slot) {
                         const double e0 = xyz[3 * (size_t)slot + 0] - q0, e1 = xyz[3 * (size_t)slot + 1] - q1,
                                      e2 = xyz[3 * (size_t)slot + 2] - q2;
                         const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                         if (d2 <= na.max_d2) {
                           ++k;
                           s1x += e0, s1y += e1, s1z += e2;
                           sxx += e0 * e0, sxy += e0 * e1, sxz += e0 * e2;
                           syy += e1 * e1, syz += e1 * e2, szz += e2 * e2;
                         }
                       });
        const double kd = (double)k;  // (k >= 1: the voxel admits itself)
        const double m0 = s1x / kd, m1 = s1y / kd, m2 = s1z / kd;
        double C[3][3];
        C[0][0] = sxx / kd - m0 * m0;
        C[0][1] = C[1][0] = sxy / kd - m0 * m1;
        C[0][2] = C[2][0] = sxz / kd - m0 * m2;
        C[1][1] = syy / kd - m1 * m1;
        C[1][2] = C[2][1] = syz / kd - m1 * m2;
        C[2][2] = szz / kd - m2 * m2;
        double n[3], lam[3];
        smallest_eigvec(C, n, lam);
        // l0 <= l1 <= l2 without an indexed array
        const double lo01 = fmin(lam[0], lam[1]), hi01 = fmax(lam[0], lam[1]);
        const double l0r = fmin(lo01, lam[2]), l1 = fmax(lo01, fmin(hi01, lam[2]));
        const double l0 = l0r < 0.0 ? 0.0 : l0r;
        const double flat = l1 > 0.0 ? l0 / l1 : (double)INFINITY;
        rec.w = (float)flat;
        cls = k < na.min_support ? kNormalSparse : (l1 > 0.0 && l0 <= na.max_flat * l1) ? kNormalOriented : kNormalFlat;
        if (cls == kNormalOriented) {
          // the component of largest magnitude is positive, the lowest axis among equal ones
          const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
          const double lead = (a0 >= a1 && a0 >= a2) ? n[0] : (a1 >= a2 ? n[1] : n[2]);
          const double sg = lead < 0.0 ? -1.0 : 1.0;
          rec.x = (float)(sg * n[0]);
          rec.y = (float)(sg * n[1]);
          rec.z = (float)(sg * n[2]);
        }
      }
    }
    if (cls >= 0) {
      nrm[s] = rec;
      support[s] = k;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) n_cls[j] += (uint32_t)__popcll(__ballot(cls == j));
  }
  const unsigned long long w_looked = wave_sum(looked);
  if ((threadIdx.x & 63) == 0) {  // results unused: return-less
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (n_cls[j]) atomicAdd(&cnt[j], (unsigned long long)n_cls[j]);
    if (w_looked) atomicAdd(&cnt[4], w_looked);
  }
}

// The slots a normals download takes (solid under the build's filter; oriented: with a normal)
// appended to the outputs in no particular order: one returning atomic per wave and step for
// the wave's place (a download is not a hot path; k_dense_compact's two walks are).  cap: the
// room in the outputs, which the build's counts sized.
__global__ __launch_bounds__(kDenseThreads) void k_normals_compact(
    const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ hits,
    const unsigned long long* __restrict__ tags, const double* __restrict__ xyz, const float4* __restrict__ nrm,
    const uint32_t* __restrict__ support, uint64_t slots, DenseTake tk, int oriented, uint32_t cap,
    uint32_t* __restrict__ out_n, double* __restrict__ o_xyz, unsigned long long* __restrict__ o_tag,
    uint32_t* __restrict__ o_hits, uint32_t* __restrict__ o_miss, float* __restrict__ o_normal, float* __restrict__ o_flat,
    uint32_t* __restrict__ o_support) {
  const int lane = threadIdx.x & 63;
  for (uint64_t base = (uint64_t)blockIdx.x * kDenseThreads; base < slots; base += (uint64_t)gridDim.x * kDenseThreads) {
    const uint64_t s = base + threadIdx.x;
    const uint32_t h = s < slots ? hits[s] : 0u;
    bool take = s < slots && keys[s] != kDenseEmpty && dense_take(tk, h, s);
    float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (take) {
      rec = nrm[s];
      if (oriented && rec.x == 0.0f && rec.y == 0.0f && rec.z == 0.0f) take = false;
    }
    const unsigned long long b = __ballot(take);
    if (!b) continue;  // (the whole wave)
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(out_n, (uint32_t)__popcll(b));
    at = (uint32_t)__shfl((int)at, 0, 64);
    if (take) {
      const uint32_t o = at + (uint32_t)__popcll(b & lanemask_lt());
      if (o < cap) {  // (the build's counts sized the outputs: never false)
        o_xyz[3 * (size_t)o + 0] = xyz[3 * s + 0];
        o_xyz[3 * (size_t)o + 1] = xyz[3 * s + 1];
        o_xyz[3 * (size_t)o + 2] = xyz[3 * s + 2];
        o_tag[o] = tags[s];
        o_hits[o] = h;
        if (o_miss) o_miss[o] = dense_misses(tk, s);
        o_normal[3 * (size_t)o + 0] = rec.x;
        o_normal[3 * (size_t)o + 1] = rec.y;
        o_normal[3 * (size_t)o + 2] = rec.z;
        o_flat[o] = rec.w;
        o_support[o] = support[s];
      }
    }
  }
}

// ---- loading voxels back (DESIGN.md §Dense map, Restoring; include/fmx/fmx.h,
// fmx_upload_voxels).  The inverse of the downloads: entries (world point, owner number, index,
// hits, misses), staged by the host, go into the table.  Three launches on one stream, the
// kernel boundary the only ordering, as above.
//
//   claim  one lane per entry: classify it (invalid / out of range; no pose, no gate), compute
//          its key, find or insert the slot word for word as k_dense_claim does, then one
//          return-less atomicMin on the slot's tag with the temporary tag (temp << 32 | i),
//          return-less atomicAdds of its hits and, where given and nonzero, its misses, and
//          the slot (or the dropped marker) into the n-word scratch.  temp is an owner number
//          larger than every resident one: a resident voxel's tag stays, a new voxel's tag
//          ends as its lowest input position.  No in-wave merge: uploaded keys are mostly
//          distinct.
//   fill   one lane per entry: the lane whose temporary tag equals the slot's is the new
//          voxel's representative (exactly one: positions are unique), writes the point as
//          given and marks its own scratch word (bit 31: slots are below 2^30); one atomic
//          per block counts them.  Nothing writes a tag in this launch.
//   tag    one lane per entry: a marked lane stores the final tag (owner << 32 | index) with a
//          plain store.  Nothing reads a tag in this launch, and each tag word has one writer.
//          Its first lane adds the fill's count to the device's voxel total.
//
// The content does not depend on the order the lanes run in: keys are only inserted, the
// temporary tag is a minimum over a fixed set, hits and misses are sums, and point and final
// tag of a slot are written by exactly one lane.  seen is not touched: a resident voxel keeps
// its mark, a new voxel's slot reads 0 (clear and roll leave empty slots at 0).
constexpr uint32_t kUploadWinner = 0x80000000u;

// 0 valid (key set), 1 invalid, 3 out of range; dead: hits given and 0
__device__ __forceinline__ int upload_classify(double x, double y, double z, bool dead, double w,
                                               unsigned long long* key) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z)) || dead) return 1;
  const double cx = floor(x / w), cy = floor(y / w), cz = floor(z / w);
  // in fp64, before the cast (an infinite quotient fails the comparison)
  if (!(fabs(cx) < kDenseLimit && fabs(cy) < kDenseLimit && fabs(cz) < kDenseLimit)) return 3;
  *key = ((unsigned long long)((long long)cx + kDenseBias) << 42) |
         ((unsigned long long)((long long)cy + kDenseBias) << 21) | (unsigned long long)((long long)cz + kDenseBias);
  return 0;
}

// in_hits / in_miss: null (1 / 0 per entry); misses: the table's array (there whenever in_miss
// is); cnt: {invalid, out_of_range, added}
__global__ __launch_bounds__(kDenseThreads) void k_upload_claim(
    const double* __restrict__ in_xyz, const uint32_t* __restrict__ in_hits, const uint32_t* __restrict__ in_miss,
    uint32_t n, double w, uint32_t slot_mask, uint32_t temp, unsigned long long* keys, unsigned long long* tags,
    uint32_t* hits, uint32_t* misses, uint32_t* __restrict__ slot_of, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  int cls = -1;  // past the end
  unsigned long long key = 0;
  uint32_t h_in = 1;
  if (i < n) {
    if (in_hits) h_in = in_hits[i];
    const double* p = in_xyz + 3 * (size_t)i;
    cls = upload_classify(p[0], p[1], p[2], h_in == 0, w, &key);
  }
  uint32_t slot = kDenseDropped;
  if (cls == 0) {
    uint32_t h = (uint32_t)mix64(key) & slot_mask;
    // (bounded by the table: the host's capacity rule leaves half the slots empty)
    for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
      unsigned long long k = keys[h];  // a stale empty is settled by the CAS; keys never change once set
      if (k == kDenseEmpty) k = atomicCAS(&keys[h], kDenseEmpty, key);
      if (k == kDenseEmpty || k == key) {
        slot = h;
        break;
      }
      h = (h + 1) & slot_mask;
    }
    if (slot != kDenseDropped) {
      atomicMin(&tags[slot], ((unsigned long long)temp << 32) | (unsigned long long)i);  // results unused:
      atomicAdd(&hits[slot], h_in);                                                       // return-less
      if (in_miss) {
        const uint32_t m = in_miss[i];
        if (m) atomicAdd(&misses[slot], m);
      }
    }
  }
  if (i < n) slot_of[i] = slot;
  const unsigned long long bi = __ballot(cls == 1), bo = __ballot(cls == 3);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&cnt[0], (uint32_t)__popcll(bi));
    if (bo) atomicAdd(&cnt[1], (uint32_t)__popcll(bo));
  }
}

__global__ __launch_bounds__(kDenseFillThreads) void k_upload_fill(const double* __restrict__ in_xyz, uint32_t n,
                                                                   uint32_t temp,
                                                                   const unsigned long long* __restrict__ tags,
                                                                   uint32_t* __restrict__ slot_of,
                                                                   double* __restrict__ xyz, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseFillThreads + threadIdx.x;
  bool winner = false;
  if (i < n) {
    const uint32_t slot = slot_of[i];
    if (slot != kDenseDropped && tags[slot] == (((unsigned long long)temp << 32) | (unsigned long long)i)) {
      winner = true;
      const double* p = in_xyz + 3 * (size_t)i;
      double* o = xyz + 3 * (size_t)slot;
      o[0] = p[0];
      o[1] = p[1];
      o[2] = p[2];
      slot_of[i] = slot | kUploadWinner;  // (this lane's own word)
    }
  }
  const uint32_t mine = (uint32_t)__syncthreads_count(winner);
  if (threadIdx.x == 0 && mine) atomicAdd(&cnt[2], mine);  // result unused: return-less
}

// in_index: null (0 per entry); up_cnt: the upload's counters, complete (the fill's launch
// has ended); cnt[3]: the device's voxel total (k_dense_fill adds to it)
__global__ __launch_bounds__(kDenseThreads) void k_upload_tag(const uint32_t* __restrict__ slot_of,
                                                              const uint32_t* __restrict__ in_owner,
                                                              const uint32_t* __restrict__ in_index, uint32_t n,
                                                              unsigned long long* __restrict__ tags,
                                                              const uint32_t* __restrict__ up_cnt,
                                                              uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * (uint32_t)kDenseThreads + threadIdx.x;
  if (i == 0) cnt[3] += up_cnt[2];  // (the only lane of the launch that touches the word)
  if (i >= n) return;
  const uint32_t s = slot_of[i];
  if (s == kDenseDropped || !(s & kUploadWinner)) return;
  tags[s & ~kUploadWinner] = ((unsigned long long)in_owner[i] << 32) | (unsigned long long)(in_index ? in_index[i] : 0u);
}

static DenseArgs dense_args(const fmx_ctx* c, const double* pose34) {
  const auto& D = c->dense;
  DenseArgs a{};
  for (int k = 0; k < 12; ++k) a.T.m[k] = pose34[k];
  a.w = D.voxel_w;
  a.min2 = D.min2;
  a.max2 = D.max2;
  a.slot_mask = (uint32_t)(D.slots - 1);
  return a;
}

// The grid of a scan over the table's slots: one lane per slot up to kDenseScanBlocks blocks, a
// grid stride beyond.
static uint32_t scan_blocks(uint64_t slots) {
  return (uint32_t)std::min<uint64_t>(kDenseScanBlocks, (slots + kDenseThreads - 1) / kDenseThreads);
}
// The grid of a search that wants `want` blocks: capped (kNearestBlocks), a grid stride beyond.
static uint32_t capped_blocks(unsigned long long want) {
  return (uint32_t)std::min<unsigned long long>(want, (unsigned long long)kNearestBlocks);
}
// The cube's offsets in shell order on the device, once per context, whichever search or
// normals build comes first (the host copy outlives the transfer).
static const uint32_t* offsets_on_device(fmx_ctx* c, hipStream_t st) {
  auto& N = c->dense.nearest;
  if (!N.have) {
    FMX_HIP(hipMemcpyAsync(N.offs.p, N.h_offs.data(), N.h_offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    N.have = true;
  }
  return N.offs.p;
}

// Claim + fill of the n points at d_pts (n > 0, capacity checked by the caller) at pose34 as
// integration number seq, on stream st.  The counts, the voxel total and the completion word
// (flag_seq at c->dense.h_res[7]) land in c->dense.h_res once the fill's last block is through.
void run_dense_integrate(fmx_ctx* c, const float4* d_pts, size_t n, const double* pose34, uint32_t seq,
                         uint32_t flag_seq, hipStream_t st) {
  auto& D = c->dense;
  const DenseArgs a = dense_args(c, pose34);
  D.slot_of.ensure(n);
  {
    const uint32_t blocks = (uint32_t)((n + kDenseThreads - 1) / kDenseThreads);
    // DESIGN.md §Dense map: the point (16), the key word it finds or claims (8), the tag
    // and hit atomics (8 + 4) and its slot word (4); probes past the home slot not counted
    ProfScope ps(c->prof, PROF_DENSE, (double)n * 40.0, st);
    hipLaunchKernelGGL(k_dense_claim, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, (uint32_t)n, a, seq, D.keys.p,
                       D.tags.p, D.hits.p, D.slot_of.p, D.cnt.p);
    FMX_HIP(hipGetLastError());
  }
  {
    const uint32_t blocks = (uint32_t)((n + kDenseFillThreads - 1) / kDenseFillThreads);
    // the slot word (4) and the slot's tag (8) per point; a representative's point and
    // world point (16 + 24 per new voxel) are not known at launch and not counted
    ProfScope ps(c->prof, PROF_DENSE, (double)n * 12.0, st);
    hipLaunchKernelGGL(k_dense_fill, dim3(blocks), dim3(kDenseFillThreads), 0, st, d_pts, (uint32_t)n, a, seq, D.tags.p,
                       D.slot_of.p, D.xyz.p, D.cnt.p, reinterpret_cast<unsigned long long*>(D.cnt.p + 4), D.h_res.d,
                       D.h_res.d + 7, flag_seq);
    FMX_HIP(hipGetLastError());
  }
}

// Mark (mark != 0: c->dense.slot_of holds the claim of these same n points) + rays of the n > 0
// points at d_pts from pose34's translation, on stream st.  The counts and the completion
// word (flag_seq, the low half of c->dense.carve.h_res[5]) land in c->dense.carve.h_res once
// the last block of the rays is through.
void run_carve(fmx_ctx* c, const float4* d_pts, size_t n, const double* pose34, uint32_t mark, uint32_t flag_seq,
               hipStream_t st) {
  auto& D = c->dense;
  auto& Cv = D.carve;
  const DenseArgs a = dense_args(c, pose34);
  const CarveArgs cv{Cv.cfg.max2, Cv.cfg.margin, Cv.cfg.stride, mark};
  const uint32_t blocks = (uint32_t)((n + kDenseThreads - 1) / kDenseThreads);
  if (mark) {
    // the slot word and the mark (4 + 4 per point)
    ProfScope ps(c->prof, PROF_CARVE, (double)n * 8.0, st);
    hipLaunchKernelGGL(k_carve_mark, dim3(blocks), dim3(kDenseThreads), 0, st, D.slot_of.p, (uint32_t)n, mark, Cv.seen.p);
    FMX_HIP(hipGetLastError());
  }
  {
    // the points on the stride (16 each); the walk's 8 B per step, + 4 + 4 where the voxel
    // is present, are not known at launch and not counted (DESIGN.md has the model, the
    // launch's own counts give the steps)
    ProfScope ps(c->prof, PROF_CARVE, (double)((n + Cv.cfg.stride - 1) / Cv.cfg.stride) * 16.0, st);
    hipLaunchKernelGGL(k_carve_rays, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, (uint32_t)n, a, cv, D.keys.p,
                       Cv.seen.p, Cv.misses.p, Cv.cnt.p, Cv.h_res.d, reinterpret_cast<uint32_t*>(Cv.h_res.d + 5), flag_seq);
    FMX_HIP(hipGetLastError());
  }
}

// A probe's filter; the miss array wherever it exists (read on a key match only: for the
// ratio, and for the misses a point reports).
static DenseTake probe_take_args(const fmx_ctx* c, const ProbeFilter& f) {
  const auto& Cv = c->dense.carve;
  return DenseTake{f.min_hits, f.num, f.den, Cv.have ? Cv.misses.p : nullptr};
}

// what a launch writes per point: the state byte and the arrays asked for
static double probe_out_bytes(const ProbeOut& o) {
  return 1.0 + (o.step ? 4.0 : 0.0) + (o.t ? 8.0 : 0.0) + (o.tag ? 8.0 : 0.0) + (o.hits ? 4.0 : 0.0) +
         (o.misses ? 4.0 : 0.0) + (o.xyz ? 24.0 : 0.0);
}

void run_probe_points(fmx_ctx* c, const float4* d_pts, size_t n, const double* pose34, const ProbeFilter& f,
                      const ProbeOut& o, hipStream_t st) {
  auto& D = c->dense;
  const DenseArgs a = dense_args(c, pose34);
  const uint32_t blocks = (uint32_t)((n + kDenseThreads - 1) / kDenseThreads);
  FMX_HIP(hipMemsetAsync(D.probe.cnt.p, 0, 8 * sizeof(unsigned long long), st));
  // DESIGN.md §Dense map, Probing: the point (16), the home slot's key word (8) and what is
  // written per point; probes past the home slot, and a present voxel's hits, misses, tag and
  // point (4 + 4 + 8 + 24 at the most), are not known at launch and not counted
  ProfScope ps(c->prof, PROF_DENSE, (double)n * (24.0 + probe_out_bytes(o)), st);
  hipLaunchKernelGGL(k_probe_points, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, (uint32_t)n, a,
                     probe_take_args(c, f), D.keys.p, D.tags.p, D.hits.p, D.xyz.p, o, D.probe.cnt.p);
  FMX_HIP(hipGetLastError());
}

void run_probe_rays(fmx_ctx* c, const float4* d_pts, size_t n, const double* pose34, const ProbeFilter& f,
                    uint32_t skip, const ProbeOut& o, hipStream_t st) {
  auto& D = c->dense;
  const DenseArgs a = dense_args(c, pose34);
  const uint32_t blocks = (uint32_t)((n + kDenseThreads - 1) / kDenseThreads);
  FMX_HIP(hipMemsetAsync(D.probe.cnt.p, 0, 8 * sizeof(unsigned long long), st));
  // the point (16) and what is written per ray; the walk's 8 B per examined voxel, + 4 (+ 4
  // under a miss filter) where one is present, are not known at launch and not counted
  // (DESIGN.md has the model, the call's own counts give the steps)
  ProfScope ps(c->prof, PROF_DENSE, (double)n * (16.0 + probe_out_bytes(o)), st);
  hipLaunchKernelGGL(k_probe_rays, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, (uint32_t)n, a,
                     probe_take_args(c, f), skip, D.keys.p, D.tags.p, D.hits.p, D.xyz.p, o, D.probe.cnt.p);
  FMX_HIP(hipGetLastError());
}

void run_nearest(fmx_ctx* c, const float4* d_pts, size_t n, const double* pose34, const ProbeFilter& f, uint32_t reach,
                 double max_dist2, const ProbeOut& o, hipStream_t st) {
  auto& D = c->dense;
  const uint32_t* offs = offsets_on_device(c, st);
  const DenseArgs a = dense_args(c, pose34);
  // one group of lanes per point up to kNearestBlocks blocks (8 waves on every SIMD of 256 CUs), a grid
  // stride beyond: the counters' same-address atomics, one per wave, bound the launch otherwise
  const unsigned long long want = ((unsigned long long)n * FMX_NEAREST_LANES + kDenseThreads - 1) / kDenseThreads;
  const uint32_t blocks = capped_blocks(want);
  FMX_HIP(hipMemsetAsync(D.probe.cnt.p, 0, 8 * sizeof(unsigned long long), st));
  // DESIGN.md §Dense map, Nearest: the point (16), the own cell's key word (8) and what is
  // written per point; the other cells' 8 B per lookup, + 4 (+ 4 under a ratio) per present
  // voxel and + 24 per solid one, are not known at launch and not counted (the call's own
  // `lookups` gives the first)
  ProfScope ps(c->prof, PROF_DENSE, (double)n * (24.0 + probe_out_bytes(o)), st);
  hipLaunchKernelGGL(k_nearest, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, (uint32_t)n, a, probe_take_args(c, f),
                     reach, max_dist2, offs, D.keys.p, D.tags.p, D.hits.p, D.xyz.p, o, D.probe.cnt.p);
  FMX_HIP(hipGetLastError());
}

size_t align_partials() { return (size_t)kNearestBlocks * kAlignLd; }

template <class Rows>
static void launch_align(fmx_ctx* c, const float4* d_pts, size_t n, uint32_t every, const double* pose34,
                         const ProbeFilter& f, uint32_t reach, double max_dist2, double sigma, uint32_t seq, hipStream_t st,
                         Rows rows) {
  auto& D = c->dense;
  auto& A = D.align;
  const uint32_t* offs = offsets_on_device(c, st);
  const DenseArgs a = dense_args(c, pose34);
  const unsigned long long m = ((unsigned long long)n + every - 1) / every;  // the kept points
  // the grid of run_nearest over the kept points: capped, a grid stride beyond
  const unsigned long long want = (m * FMX_ALIGN_LANES + kDenseThreads - 1) / kDenseThreads;
  const uint32_t blocks = capped_blocks(want);
  FMX_HIP(hipMemsetAsync(A.cnt.p, 0, 8 * sizeof(unsigned long long), st));
  // DESIGN.md §Dense map, Aligning: run_nearest's model without the per-point outputs (the
  // point, 16, and the own cell's key word, 8; the other lookups are not known at launch), plus
  // the block partials written and read back (28 doubles each way); the plane form's 16 B per
  // found point are not known at launch
  ProfScope ps(c->prof, PROF_DENSE, (double)m * 24.0 + (double)blocks * 2.0 * 28.0 * sizeof(double), st);
  hipLaunchKernelGGL(k_align<Rows>, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, (uint32_t)m, every, a,
                     probe_take_args(c, f), reach, max_dist2, 1.0 / sigma, offs, D.keys.p, D.hits.p, D.xyz.p, A.cnt.p,
                     A.bpart.p, A.ticket.p, A.h_out.d, c->h_flag.d, seq, rows);
  FMX_HIP(hipGetLastError());
}

void run_align(fmx_ctx* c, const float4* d_pts, size_t n, uint32_t every, const double* pose34, const ProbeFilter& f,
               uint32_t reach, double max_dist2, double sigma, uint32_t seq, hipStream_t st) {
  launch_align(c, d_pts, n, every, pose34, f, reach, max_dist2, sigma, seq, st, PointRows{});
}

void run_plane(fmx_ctx* c, const float4* d_pts, size_t n, uint32_t every, const double* pose34, const ProbeFilter& f,
               uint32_t reach, double max_dist2, double sigma, uint32_t seq, hipStream_t st) {
  launch_align(c, d_pts, n, every, pose34, f, reach, max_dist2, sigma, seq, st, PlaneRows{c->dense.normals.nrm.p});
}

void run_score(fmx_ctx* c, const float4* d_pts, size_t n, uint32_t every, uint32_t poses, const ProbeFilter& f,
               uint32_t reach, double max_dist2, hipStream_t st) {
  auto& D = c->dense;
  auto& S = D.score;
  const uint32_t* offs = offsets_on_device(c, st);
  const DenseArgs a = dense_args(c, kEye34);  // (the kernel puts each item's pose in)
  const ScorePlan plan = score_plan((unsigned long long)n, every, poses);
  const unsigned long long items = (unsigned long long)poses * plan.tiles;  // (at most 2^24: score_plan's chunk)
  {
    const uint32_t blocks = capped_blocks(items);
    // DESIGN.md §Dense map, Scoring: run_align's model per (pose, kept point) (the point, 16, and
    // the own cell's key word, 8; the other lookups are not known at launch), the item's pose
    // (96) and its partial record (32)
    ProfScope ps(c->prof, PROF_DENSE, (double)poses * (double)plan.kept * 24.0 + (double)items * 128.0, st);
    hipLaunchKernelGGL(k_score, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, plan.kept, every, S.poses.p, plan.tiles,
                       (uint32_t)items, a, probe_take_args(c, f), reach, max_dist2, offs, D.keys.p, D.hits.p, D.xyz.p,
                       S.part.p);
    FMX_HIP(hipGetLastError());
  }
  {
    // the partial records read and the poses' records written (32 each)
    ProfScope ps(c->prof, PROF_DENSE, ((double)items + (double)poses) * 32.0, st);
    hipLaunchKernelGGL(k_score_finish, dim3((poses + kScoreWaves - 1) / kScoreWaves), dim3(kDenseThreads), 0, st, S.part.p,
                       plan.tiles, poses, S.out.p);
    FMX_HIP(hipGetLastError());
  }
}

void run_refine(fmx_ctx* c, const float4* d_pts, size_t n, uint32_t every, uint32_t poses, const ProbeFilter& f,
                uint32_t reach, double max_dist2, double sigma, bool plane, hipStream_t st) {
  auto& D = c->dense;
  auto& Rf = D.refine;
  const uint32_t* offs = offsets_on_device(c, st);
  const DenseArgs a = dense_args(c, kEye34);  // (the kernel puts each item's pose in)
  const RefinePlan plan = refine_plan((unsigned long long)n, every, poses);
  const unsigned long long items = (unsigned long long)poses * plan.tiles;  // (at most 2^22: refine_plan's chunk)
  {
    const uint32_t blocks = capped_blocks(items);
    // DESIGN.md §Dense map, Refining: run_align's model per (pose, kept point) (the point, 16, and
    // the own cell's key word, 8; the other lookups, and the plane form's 16 B per found point,
    // are not known at launch), the item's pose (96) and its partial record (256)
    ProfScope ps(c->prof, PROF_DENSE, (double)poses * (double)plan.kept * 24.0 + (double)items * 352.0, st);
    const auto launch = [&](auto rows) {
      hipLaunchKernelGGL(k_refine<decltype(rows)>, dim3(blocks), dim3(kDenseThreads), 0, st, d_pts, plan.kept, every,
                         Rf.poses.p, plan.tiles, (uint32_t)items, a, probe_take_args(c, f), reach, max_dist2, 1.0 / sigma,
                         offs, D.keys.p, D.hits.p, D.xyz.p, Rf.part.p, rows);
    };
    if (plane) launch(PlaneRows{D.normals.nrm.p});
    else launch(PointRows{});
    FMX_HIP(hipGetLastError());
  }
  {
    // the partial records read (256 each) and the poses' records written (264 each)
    ProfScope ps(c->prof, PROF_DENSE, (double)items * 256.0 + (double)poses * 264.0, st);
    hipLaunchKernelGGL(k_refine_finish, dim3(poses), dim3(kDenseThreads), 0, st,
                       Rf.part.p, plan.tiles, poses, Rf.out.p);
    FMX_HIP(hipGetLastError());
  }
}

// The build's filter; the miss array wherever it exists (the download reports misses from it).
static DenseTake normals_take_args(const fmx_ctx* c, const fmx_normals_params& prm) {
  return probe_take_args(c, probe_filter(prm.min_hits, prm.miss_num, prm.miss_den));
}

void run_normals_build(fmx_ctx* c, const fmx_normals_params& prm, hipStream_t st) {
  auto& D = c->dense;
  auto& M = D.normals;
  const uint32_t* offs = offsets_on_device(c, st);
  const NormalsArgs na{prm.reach, normals_min_support(prm), prm.max_dist2, prm.max_flatness};
  FMX_HIP(hipMemsetAsync(M.cnt.p, 0, 8 * sizeof(unsigned long long), st));
  // DESIGN.md §Dense map, Normals: every slot's key word read (8); per voxel its hits and point
  // (4 + 24), the own cell's key word (8) and its record written (20); the other cells' 8 B per
  // lookup, + 4 per present and + 24 per solid neighbour, are not known at launch (the call's
  // own `lookups` gives the first)
  ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * 8.0 + (double)D.voxels * 56.0, st);
  hipLaunchKernelGGL(k_normals_build, dim3(scan_blocks(D.slots)), dim3(kDenseThreads), 0, st, D.keys.p, D.hits.p, D.xyz.p,
                     D.slots, normals_take_args(c, prm), na, offs, M.nrm.p, M.support.p, M.cnt.p);
  FMX_HIP(hipGetLastError());
}

void run_normals_compact(fmx_ctx* c, const fmx_normals_params& prm, bool oriented_only, bool with_misses, uint32_t count,
                         hipStream_t st) {
  auto& D = c->dense;
  auto& M = D.normals;
  D.o_xyz.ensure(3 * (size_t)count);
  D.o_tag.ensure(count);
  D.o_hits.ensure(count);
  M.o_normal.ensure(3 * (size_t)count);
  M.o_flat.ensure(count);
  M.o_support.ensure(count);
  uint32_t* o_miss = with_misses && D.carve.have ? D.carve.o_miss.p : nullptr;
  FMX_HIP(hipMemsetAsync(D.out_n.p, 0, sizeof(uint32_t), st));
  // every slot's key word, hit count and record (8 + 4 + 16; short-circuits not counted) + per
  // voxel taken its tag and point read and written, its hits, normal, flatness and support
  // written (2 * (8 + 24) + 4 + 12 + 4 + 4 + 4 read for the support)
  ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * 28.0 + (double)count * (o_miss ? 96.0 : 92.0), st);
  hipLaunchKernelGGL(k_normals_compact, dim3(scan_blocks(D.slots)), dim3(kDenseThreads), 0, st, D.keys.p, D.hits.p, D.tags.p,
                     D.xyz.p, M.nrm.p, M.support.p, D.slots, normals_take_args(c, prm), oriented_only ? 1 : 0, count,
                     D.out_n.p, D.o_xyz.p, D.o_tag.p, D.o_hits.p, o_miss, M.o_normal.p, M.o_flat.p, M.o_support.p);
  FMX_HIP(hipGetLastError());
}

void run_dense_upload(fmx_ctx* c, uint32_t n, bool have_index, bool have_hits, bool have_misses, uint32_t temp,
                      hipStream_t st) {
  auto& D = c->dense;
  auto& U = D.upload;
  const uint32_t* in_hits = have_hits ? U.hits.p : nullptr;
  const uint32_t* in_miss = have_misses ? U.misses.p : nullptr;
  FMX_HIP(hipMemsetAsync(U.cnt.p, 0, 4 * sizeof(uint32_t), st));
  {
    const uint32_t blocks = (n + kDenseThreads - 1) / kDenseThreads;
    // DESIGN.md §Dense map, Restoring: the entry's point (24) and, where given, its hits and
    // misses (4 + 4), the key word it finds or claims (8), the tag and hit atomics (8 + 4),
    // the miss atomic where given (4) and its slot word (4); probes past the home slot not
    // counted
    ProfScope ps(c->prof, PROF_DENSE, (double)n * (48.0 + (have_hits ? 4.0 : 0.0) + (have_misses ? 8.0 : 0.0)), st);
    hipLaunchKernelGGL(k_upload_claim, dim3(blocks), dim3(kDenseThreads), 0, st, U.xyz.p, in_hits, in_miss, n, D.voxel_w,
                       (uint32_t)(D.slots - 1), temp, D.keys.p, D.tags.p, D.hits.p,
                       D.carve.have ? D.carve.misses.p : nullptr, U.slot.p, U.cnt.p);
    FMX_HIP(hipGetLastError());
  }
  {
    const uint32_t blocks = (n + kDenseFillThreads - 1) / kDenseFillThreads;
    // the slot word (4) and the slot's tag (8) per entry; a representative's point read and
    // written and its slot word marked (24 + 24 + 4 per new voxel) are not known at launch
    // and not counted
    ProfScope ps(c->prof, PROF_DENSE, (double)n * 12.0, st);
    hipLaunchKernelGGL(k_upload_fill, dim3(blocks), dim3(kDenseFillThreads), 0, st, U.xyz.p, n, temp, D.tags.p, U.slot.p,
                       D.xyz.p, U.cnt.p);
    FMX_HIP(hipGetLastError());
  }
  {
    const uint32_t blocks = (n + kDenseThreads - 1) / kDenseThreads;
    // the slot word (4) per entry; a representative's owner, index and tag (4 + 4 + 8 per new
    // voxel) are not known at launch and not counted
    ProfScope ps(c->prof, PROF_DENSE, (double)n * 4.0, st);
    hipLaunchKernelGGL(k_upload_tag, dim3(blocks), dim3(kDenseThreads), 0, st, U.slot.p, U.owner.p,
                       have_index ? U.index.p : nullptr, n, D.tags.p, U.cnt.p, D.cnt.p);
    FMX_HIP(hipGetLastError());
  }
}

// The miss filter of a download; the miss array only where it exists and the filter reads it.
static DenseTake dense_take_args(const fmx_ctx* c, uint32_t min_hits, uint32_t num, uint32_t den, bool with_misses) {
  const auto& Cv = c->dense.carve;
  return DenseTake{min_hits, num, den, Cv.have && (den || with_misses) ? Cv.misses.p : nullptr};
}

// The number of voxels a download takes into c->dense.h_n[0] (one launch; waits).
uint32_t run_dense_count(fmx_ctx* c, uint32_t min_hits, uint32_t miss_num, uint32_t miss_den, hipStream_t st) {
  auto& D = c->dense;
  const DenseTake tk = dense_take_args(c, min_hits, miss_num, miss_den, false);
  FMX_HIP(hipMemsetAsync(D.out_n.p, 0, sizeof(uint32_t), st));
  {
    const uint32_t blocks = scan_blocks(D.slots);
    // every slot's hit count (+ its miss count under a miss filter; short-circuits not counted)
    ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * (tk.misses ? 8.0 : 4.0), st);
    hipLaunchKernelGGL(k_dense_count, dim3(blocks), dim3(kDenseThreads), 0, st, D.hits.p, D.slots, tk, D.out_n.p);
    FMX_HIP(hipGetLastError());
  }
  FMX_HIP(hipMemcpyAsync(D.h_n.p, D.out_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  return D.h_n.p[0];
}

// Those count voxels appended to c->dense.o_xyz / o_tag / o_hits (and carve.o_miss, sized by
// the caller, with with_misses on a map that has the array) (one launch; queued only).
void run_dense_compact(fmx_ctx* c, uint32_t min_hits, uint32_t miss_num, uint32_t miss_den, bool with_misses,
                       uint32_t count, hipStream_t st) {
  auto& D = c->dense;
  D.o_xyz.ensure(3 * (size_t)count);
  D.o_tag.ensure(count);
  D.o_hits.ensure(count);
  const DenseTake tk = dense_take_args(c, min_hits, miss_num, miss_den, with_misses);
  uint32_t* o_miss = with_misses && D.carve.have ? D.carve.o_miss.p : nullptr;
  FMX_HIP(hipMemsetAsync(D.out_n.p, 0, sizeof(uint32_t), st));
  const uint32_t blocks = scan_blocks(D.slots);
  // every slot's hit count, twice (2 * 4) + per voxel taken its tag and point read and
  // written, its hit count written (2 * (8 + 24) + 4); with the miss array in play each
  // slot's miss count twice more (2 * 4) and a taken voxel's written (4)
  ProfScope ps(c->prof, PROF_DENSE,
               (double)D.slots * (tk.misses ? 16.0 : 8.0) + (double)count * (o_miss ? 72.0 : 68.0), st);
  hipLaunchKernelGGL(k_dense_compact, dim3(blocks), dim3(kDenseThreads), 0, st, D.hits.p, D.tags.p, D.xyz.p, D.slots,
                     tk, count, D.out_n.p, D.o_xyz.p, D.o_tag.p, D.o_hits.p, o_miss);
  FMX_HIP(hipGetLastError());
}

// Keys and tags to all-ones, hits and the counters (and, where they exist, misses and seen) to
// 0, on stream st.
void run_dense_clear(fmx_ctx* c, hipStream_t st) {
  auto& D = c->dense;
  FMX_HIP(hipMemsetAsync(D.keys.p, 0xFF, D.slots * sizeof(unsigned long long), st));
  FMX_HIP(hipMemsetAsync(D.tags.p, 0xFF, D.slots * sizeof(unsigned long long), st));
  FMX_HIP(hipMemsetAsync(D.hits.p, 0, D.slots * sizeof(uint32_t), st));
  FMX_HIP(hipMemsetAsync(D.cnt.p, 0, 8 * sizeof(uint32_t), st));
  if (D.carve.have) {
    FMX_HIP(hipMemsetAsync(D.carve.misses.p, 0, D.slots * sizeof(uint32_t), st));
    FMX_HIP(hipMemsetAsync(D.carve.seen.p, 0, D.slots * sizeof(uint32_t), st));
  }
}

static RollBox roll_box(const long long cc[3], const uint32_t half[3]) {
  RollBox b{};
  for (int k = 0; k < 3; ++k) {
    b.cc[k] = cc[k];
    b.half[k] = (long long)half[k];
  }
  return b;
}

// {inside, outside} of the box into out (one launch; waits).
void run_roll_count(fmx_ctx* c, const long long cc[3], const uint32_t half[3], uint32_t out[2], hipStream_t st) {
  auto& D = c->dense;
  D.roll.n.ensure(4);
  D.h_n.ensure(2);
  FMX_HIP(hipMemsetAsync(D.roll.n.p, 0, 4 * sizeof(uint32_t), st));
  {
    const uint32_t blocks = scan_blocks(D.slots);
    ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * 8.0, st);  // every slot's key
    hipLaunchKernelGGL(k_roll_count, dim3(blocks), dim3(kDenseThreads), 0, st, D.keys.p, D.slots, roll_box(cc, half),
                       D.roll.n.p);
    FMX_HIP(hipGetLastError());
  }
  FMX_HIP(hipMemcpyAsync(D.h_n.p, D.roll.n.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  out[0] = D.h_n.p[0];
  out[1] = D.h_n.p[1];
}

// After run_roll_count of the same box (its cursors are still zero; the outputs and the
// staging list hold evicted / kept entries): the evicted voxels appended to c->dense.o_xyz /
// o_tag / o_hits, the kept ones put back, the device's voxel total set (queued only).  On a
// map with the carve arrays the miss counts go along (carve.o_miss / s_miss, sized by the caller).
void run_roll_rebuild(fmx_ctx* c, const long long cc[3], const uint32_t half[3], uint32_t kept, uint32_t evicted,
                      hipStream_t st) {
  auto& D = c->dense;
  auto& Rl = D.roll;
  auto& Cv = D.carve;
  const double mb = Cv.have ? 1.0 : 0.0;  // (the miss word wherever the hit word goes; seen zeroed)
  {
    const uint32_t blocks = scan_blocks(D.slots);
    // every slot's key, twice (2 * 8) + per evicted voxel its tag, hits and point read and
    // written, its slot emptied (2 * 36 + 20) + per kept voxel the same and its key written (+ 8)
    ProfScope ps(c->prof, PROF_DENSE,
                 (double)D.slots * 16.0 + (double)evicted * (92.0 + 16.0 * mb) + (double)kept * (100.0 + 16.0 * mb), st);
    hipLaunchKernelGGL(k_roll_split, dim3(blocks), dim3(kDenseThreads), 0, st, D.keys.p, D.tags.p, D.hits.p, D.xyz.p,
                       D.slots, roll_box(cc, half), evicted, kept, Rl.n.p + 2, D.o_xyz.p, D.o_tag.p, D.o_hits.p, Rl.s_key.p,
                       Rl.s_tag.p, Rl.s_hits.p, Rl.s_xyz.p, Cv.have ? Cv.misses.p : nullptr,
                       Cv.have ? Cv.seen.p : nullptr, Cv.have ? Cv.o_miss.p : nullptr,
                       Cv.have && kept ? Cv.s_miss.p : nullptr);
    FMX_HIP(hipGetLastError());
  }
  if (kept) {
    const uint32_t blocks = (kept + kDenseThreads - 1) / kDenseThreads;
    // the staged voxel read (44) and written: key, tag, hits, point (44); probes past the home slot not counted
    ProfScope ps(c->prof, PROF_DENSE, (double)kept * (88.0 + 8.0 * mb), st);
    hipLaunchKernelGGL(k_roll_reinsert, dim3(blocks), dim3(kDenseThreads), 0, st, Rl.s_key.p, Rl.s_tag.p, Rl.s_hits.p,
                       Rl.s_xyz.p, kept, D.keys.p, D.tags.p, D.hits.p, D.xyz.p, (uint32_t)(D.slots - 1), D.cnt.p,
                       Cv.have ? Cv.s_miss.p : nullptr, Cv.have ? Cv.misses.p : nullptr);
    FMX_HIP(hipGetLastError());
  } else {
    FMX_HIP(hipMemsetAsync(D.cnt.p + 3, 0, sizeof(uint32_t), st));
  }
}

}  // namespace fmx
