// densemap.hip — the opt-in dense voxel map of the registered scans (DESIGN.md §Dense map;
// include/fmx/fmx.h, fmx_dense_integrate).  A fixed-capacity open-addressed hash of world
// voxels, structure-of-arrays, 44 B per slot: keys (u64), tags (u64), hits (u32), xyz
// (3 doubles).  An integration is two launches on one stream, no host round trip between
// them; the kernel boundary is the only ordering (no in-kernel device-scope fence: see
// organize.hip's header for what one per wave costs on gfx950).
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

// Slots with hits >= min_hits: counted (out_n), one atomic per wave.
__global__ __launch_bounds__(kDenseThreads) void k_dense_count(const uint32_t* __restrict__ hits, uint64_t slots,
                                                               uint32_t min_hits, uint32_t* __restrict__ out_n) {
  uint32_t mine = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kDenseThreads; base < slots; base += (uint64_t)gridDim.x * kDenseThreads) {
    const uint64_t s = base + threadIdx.x;
    const bool take = s < slots && hits[s] >= min_hits;
    mine += (uint32_t)__popcll(__ballot(take));  // the same in every lane of the wave
  }
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out_n, mine);
}

// ... appended: (xyz, tag, hits) of each, in no particular order; cap: the room in the outputs.
// Each wave walks its slots twice: once to count what it will take, then ONE atomic for its
// place in the output, then again to copy (an atomic per wave and step, one word for all:
// 4.0 ms for 430k voxels in 2^26 slots at C4, profiles/dense_cost.json has this form's time).
__global__ __launch_bounds__(kDenseThreads) void k_dense_compact(const uint32_t* __restrict__ hits,
                                                                 const unsigned long long* __restrict__ tags,
                                                                 const double* __restrict__ xyz, uint64_t slots,
                                                                 uint32_t min_hits, uint32_t cap,
                                                                 uint32_t* __restrict__ out_n, double* __restrict__ o_xyz,
                                                                 unsigned long long* __restrict__ o_tag,
                                                                 uint32_t* __restrict__ o_hits) {
  const int lane = threadIdx.x & 63;
  const uint64_t first = (uint64_t)blockIdx.x * kDenseThreads, step = (uint64_t)gridDim.x * kDenseThreads;
  uint32_t mine = 0;
  for (uint64_t base = first; base < slots; base += step) {
    const uint64_t s = base + threadIdx.x;
    mine += (uint32_t)__popcll(__ballot(s < slots && hits[s] >= min_hits));  // the same in every lane of the wave
  }
  if (!mine) return;  // (the whole wave)
  uint32_t at = 0;
  if (lane == 0) at = atomicAdd(out_n, mine);
  at = (uint32_t)__shfl((int)at, 0, 64);
  for (uint64_t base = first; base < slots; base += step) {
    const uint64_t s = base + threadIdx.x;
    const uint32_t h = s < slots ? hits[s] : 0u;
    const bool take = s < slots && h >= min_hits;
    const unsigned long long b = __ballot(take);
    if (take) {
      const uint32_t o = at + (uint32_t)__popcll(b & lanemask_lt());
      if (o < cap) {  // (the count pass sized the outputs: never false)
        o_xyz[3 * (size_t)o + 0] = xyz[3 * s + 0];
        o_xyz[3 * (size_t)o + 1] = xyz[3 * s + 1];
        o_xyz[3 * (size_t)o + 2] = xyz[3 * s + 2];
        o_tag[o] = tags[s];
        o_hits[o] = h;
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

// cur: {evicted, kept} cursors; cap_e / cap_k: the room in the outputs (e_*) and the staging list (s_*)
__global__ __launch_bounds__(kDenseThreads) void k_roll_split(
    unsigned long long* keys, unsigned long long* tags, uint32_t* hits, const double* __restrict__ xyz, uint64_t slots,
    RollBox box, uint32_t cap_e, uint32_t cap_k, uint32_t* __restrict__ cur,
    double* __restrict__ e_xyz, unsigned long long* __restrict__ e_tag, uint32_t* __restrict__ e_hits,
    unsigned long long* __restrict__ s_key, unsigned long long* __restrict__ s_tag, uint32_t* __restrict__ s_hits,
    double* __restrict__ s_xyz) {
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
      const double x = xyz[3 * s + 0], y = xyz[3 * s + 1], z = xyz[3 * s + 2];
      if (in) {
        const uint32_t o = at_k + (uint32_t)__popcll(b_k & lanemask_lt());
        if (o < cap_k) {  // (the count pass sized both: never false)
          s_key[o] = k;
          s_tag[o] = t;
          s_hits[o] = h;
          s_xyz[3 * (size_t)o + 0] = x;
          s_xyz[3 * (size_t)o + 1] = y;
          s_xyz[3 * (size_t)o + 2] = z;
        }
      } else {
        const uint32_t o = at_e + (uint32_t)__popcll(b_e & lanemask_lt());
        if (o < cap_e) {
          e_tag[o] = t;
          e_hits[o] = h;
          e_xyz[3 * (size_t)o + 0] = x;
          e_xyz[3 * (size_t)o + 1] = y;
          e_xyz[3 * (size_t)o + 2] = z;
        }
      }
      keys[s] = kDenseEmpty;
      tags[s] = ~0ull;
      hits[s] = 0u;
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
    uint32_t* __restrict__ cnt) {
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
      xyz[3 * (size_t)h + 0] = s_xyz[3 * (size_t)i + 0];
      xyz[3 * (size_t)h + 1] = s_xyz[3 * (size_t)i + 1];
      xyz[3 * (size_t)h + 2] = s_xyz[3 * (size_t)i + 2];
      return;
    }
    h = (h + 1) & slot_mask;
  }
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

// The number of voxels with hits >= min_hits into c->dense.h_n[0] (one launch; waits).
uint32_t run_dense_count(fmx_ctx* c, uint32_t min_hits, hipStream_t st) {
  auto& D = c->dense;
  FMX_HIP(hipMemsetAsync(D.out_n.p, 0, sizeof(uint32_t), st));
  {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kDenseScanBlocks, (D.slots + kDenseThreads - 1) / kDenseThreads);
    ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * 4.0, st);  // every slot's hit count
    hipLaunchKernelGGL(k_dense_count, dim3(blocks), dim3(kDenseThreads), 0, st, D.hits.p, D.slots, min_hits, D.out_n.p);
    FMX_HIP(hipGetLastError());
  }
  FMX_HIP(hipMemcpyAsync(D.h_n.p, D.out_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  return D.h_n.p[0];
}

// Those count voxels appended to c->dense.o_xyz / o_tag / o_hits (one launch; queued only).
void run_dense_compact(fmx_ctx* c, uint32_t min_hits, uint32_t count, hipStream_t st) {
  auto& D = c->dense;
  D.o_xyz.ensure(3 * (size_t)count);
  D.o_tag.ensure(count);
  D.o_hits.ensure(count);
  FMX_HIP(hipMemsetAsync(D.out_n.p, 0, sizeof(uint32_t), st));
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(kDenseScanBlocks, (D.slots + kDenseThreads - 1) / kDenseThreads);
  // every slot's hit count, twice (2 * 4) + per voxel taken its tag and point read and
  // written, its hit count written (2 * (8 + 24) + 4)
  ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * 8.0 + (double)count * 68.0, st);
  hipLaunchKernelGGL(k_dense_compact, dim3(blocks), dim3(kDenseThreads), 0, st, D.hits.p, D.tags.p, D.xyz.p, D.slots,
                     min_hits, count, D.out_n.p, D.o_xyz.p, D.o_tag.p, D.o_hits.p);
  FMX_HIP(hipGetLastError());
}

// Keys and tags to all-ones, hits and the counters to 0, on stream st.
void run_dense_clear(fmx_ctx* c, hipStream_t st) {
  auto& D = c->dense;
  FMX_HIP(hipMemsetAsync(D.keys.p, 0xFF, D.slots * sizeof(unsigned long long), st));
  FMX_HIP(hipMemsetAsync(D.tags.p, 0xFF, D.slots * sizeof(unsigned long long), st));
  FMX_HIP(hipMemsetAsync(D.hits.p, 0, D.slots * sizeof(uint32_t), st));
  FMX_HIP(hipMemsetAsync(D.cnt.p, 0, 8 * sizeof(uint32_t), st));
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
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kDenseScanBlocks, (D.slots + kDenseThreads - 1) / kDenseThreads);
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
// o_tag / o_hits, the kept ones put back, the device's voxel total set (queued only).
void run_roll_rebuild(fmx_ctx* c, const long long cc[3], const uint32_t half[3], uint32_t kept, uint32_t evicted,
                      hipStream_t st) {
  auto& D = c->dense;
  auto& Rl = D.roll;
  {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kDenseScanBlocks, (D.slots + kDenseThreads - 1) / kDenseThreads);
    // every slot's key, twice (2 * 8) + per evicted voxel its tag, hits and point read and
    // written, its slot emptied (2 * 36 + 20) + per kept voxel the same and its key written (+ 8)
    ProfScope ps(c->prof, PROF_DENSE, (double)D.slots * 16.0 + (double)evicted * 92.0 + (double)kept * 100.0, st);
    hipLaunchKernelGGL(k_roll_split, dim3(blocks), dim3(kDenseThreads), 0, st, D.keys.p, D.tags.p, D.hits.p, D.xyz.p,
                       D.slots, roll_box(cc, half), evicted, kept, Rl.n.p + 2, D.o_xyz.p, D.o_tag.p, D.o_hits.p, Rl.s_key.p,
                       Rl.s_tag.p, Rl.s_hits.p, Rl.s_xyz.p);
    FMX_HIP(hipGetLastError());
  }
  if (kept) {
    const uint32_t blocks = (kept + kDenseThreads - 1) / kDenseThreads;
    // the staged voxel read (44) and written: key, tag, hits, point (44); probes past the home slot not counted
    ProfScope ps(c->prof, PROF_DENSE, (double)kept * 88.0, st);
    hipLaunchKernelGGL(k_roll_reinsert, dim3(blocks), dim3(kDenseThreads), 0, st, Rl.s_key.p, Rl.s_tag.p, Rl.s_hits.p,
                       Rl.s_xyz.p, kept, D.keys.p, D.tags.p, D.hits.p, D.xyz.p, (uint32_t)(D.slots - 1), D.cnt.p);
    FMX_HIP(hipGetLastError());
  } else {
    FMX_HIP(hipMemsetAsync(D.cnt.p + 3, 0, sizeof(uint32_t), st));
  }
}

}  // namespace fmx
