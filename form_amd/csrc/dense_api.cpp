// dense_api.cpp — the host layer of the dense voxel map (densemap.hip): every fmx_dense_*,
// fmx_roll_*, fmx_carve_*, fmx_probe_*, fmx_upload_*, fmx_nearest_*, fmx_align_*, fmx_score_*,
// fmx_refine_*, fmx_normals_* and fmx_plane_* entry point of include/fmx/fmx.h, and the four calls
// register_scan (fmx_api.cpp) makes into the map (fmx_api.hpp).  The argument checks that need
// no device live in the *_host.hpp headers.
// Host code only; built like fmx_api.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fmx_api.hpp"

using namespace fmx;

namespace {

// ---- the pieces every feature shares
void need_map(const fmx_ctx* c) {
  if (!c->dense.on) throw StatusError(FMX_E_STATE, "the dense map is not enabled (fmx_dense_configure)");
}
// The normal snapshot is indexed by slot and depends on hits and misses: every path that
// changes, or may change, the table ends it here (one host-side flag: nothing is launched).
void normals_stale(fmx_ctx* c) { c->dense.normals.current = false; }
// A host-only check (the *_host.hpp ones return a status and write a text): its refusal thrown.
template <class F>
void checked(F&& check) {
  const char* why = "";
  const fmx_status st = check(&why);
  if (st != FMX_OK) throw StatusError(st, why);
}
// The capacity rule: n more points or entries (what) must fit beside the voxels there are.
void need_room(const fmx_ctx* c, size_t n, const char* what) {
  const auto& D = c->dense;
  if (D.voxels + n > D.max_voxels)
    throw StatusError(FMX_E_OOM, "dense map: " + std::to_string(D.voxels) + " voxels + " + std::to_string(n) + " " + what +
                                     " exceed max_voxels " + std::to_string(D.max_voxels));
}
bool any_array(const fmx_voxel_arrays& A) { return A.xyz || A.scan || A.index || A.hits || A.misses; }

// Exactly n elements (DBuf::ensure doubles what it is asked for: not for a table of up to
// 2^30 slots); a failed allocation is a capacity error, not a HIP one.
template <class T>
void alloc_exact(DBuf<T>& b, size_t n) {
  b.release();
  T* p = nullptr;
  if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    throw StatusError(FMX_E_OOM, "dense map: device allocation of " + std::to_string(n * sizeof(T)) + " bytes failed");
  }
  b.p = p;
  b.cap = n;
}
// DBuf::ensure with a failed allocation reported as a capacity error, not a HIP one (what:
// whose buffer it is, for the message).
template <class T>
void roll_ensure(DBuf<T>& b, size_t n, const char* what = "dense map roll") {
  try {
    b.ensure(n);
  } catch (const HipError&) {
    (void)hipGetLastError();
    throw StatusError(FMX_E_OOM, std::string(what) + ": device allocation of " + std::to_string(n * sizeof(T)) + " bytes failed");
  }
}
// The device pointer for these n points: the caller's, or dense.in behind a copy queued on the
// context stream.  The caller has sized dense.in (each call reports a failure to in its own way).
const float4* scan_on_device(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev) {
  if (src_on_dev || !n) return reinterpret_cast<const float4*>(xyzw);
  auto& in = c->dense.in;
  FMX_HIP(hipMemcpyAsync(in.p, xyzw, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  return in.p;
}
// The cube's offsets for the nearest-voxel search (nearest_host.hpp), built and sized at first use.
void offsets_ensure(fmx_ctx* c, const char* what) {
  auto& N = c->dense.nearest;
  if (!N.have && N.h_offs.empty()) N.h_offs = nearest_offsets(FMX_NEAREST_MAX_REACH);
  roll_ensure(N.offs, N.h_offs.size(), what);
}

void dense_release(fmx_ctx* c) {
  auto& D = c->dense;
  D.on = false;
  D.keys.release();
  D.tags.release();
  D.hits.release();
  D.xyz.release();
  D.carve.misses.release();  // (the carve arrays belong to the table they were sized for)
  D.carve.seen.release();
  D.carve.have = false;
  D.carve.cfg = CarveCfg{};
  D.carve.last = fmx_carve_counts{};
  D.carve.last_carved = 0;
  D.normals.nrm.release();  // (the snapshot belongs to the table it was built from)
  D.normals.support.release();
  D.normals.built = D.normals.current = false;
  D.normals.voxels = D.normals.oriented = D.normals.solid = 0;
  D.max_voxels = D.slots = D.voxels = 0;
  D.seq_scan.clear();
  D.integrations = 0;
  D.roll.on = D.roll.have_centre = false;  // (a roll configuration belongs to the map it was made for)
}
// Queue the rays of the n > 0 device points at d (the origin's voxel checked by the caller)
// behind what the context stream holds; carve_finish waits for them.
void carve_queue(fmx_ctx* c, const float4* d, size_t n, const double* pose34, uint32_t mark) {
  auto& Cv = c->dense.carve;
  normals_stale(c);
  run_carve(c, d, n, pose34, mark, Cv.flag_seq + 1, c->stream);
  Cv.flag_seq = Cv.pending = Cv.flag_seq + 1;
}
// A queued carve: wait for its completion word (the rays have then read the scan), take the counts.
void carve_finish(fmx_ctx* c, fmx_carve_counts* out) {
  auto& Cv = c->dense.carve;
  if (!Cv.pending) return;
  wait_flag(c, reinterpret_cast<const volatile uint32_t*>(Cv.h_res.p + 5), Cv.pending, c->stream);
  Cv.pending = 0;
  if (out) {
    const unsigned long long* h = Cv.h_res.p;
    *out = fmx_carve_counts{(uint32_t)h[0], h[1], h[2], h[3]};
  }
}
// The first `count` entries of the compacted list (o_xyz / o_tag / o_hits, carve.o_miss: a
// download's or an eviction's) to the caller's arrays, any of them null; waits.  misses reads
// 0 on a map that never enabled carving; the host keeps the owner number -> scan_idx table.
void list_fetch(fmx_ctx* c, uint32_t count, const fmx_voxel_arrays& A) {
  auto& D = c->dense;
  const auto out = [&](void* dst, const void* src, size_t bytes) {
    if (dst) FMX_HIP(hipMemcpyAsync(dst, src, count * bytes, hipMemcpyDeviceToHost, c->stream));
  };
  if (D.carve.have)
    out(A.misses, D.carve.o_miss.p, sizeof(uint32_t));
  else if (A.misses)
    std::memset(A.misses, 0, (size_t)count * sizeof(uint32_t));
  std::vector<unsigned long long> tag;
  if (A.scan || A.index) tag.resize(count);
  out(tag.empty() ? nullptr : tag.data(), D.o_tag.p, sizeof(unsigned long long));
  out(A.xyz, D.o_xyz.p, 3 * sizeof(double));
  out(A.hits, D.o_hits.p, sizeof(uint32_t));
  FMX_HIP(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < tag.size(); ++i) {
    if (A.scan) A.scan[i] = D.seq_scan.at((size_t)(tag[i] >> 32));
    if (A.index) A.index[i] = (uint32_t)tag[i];
  }
}

// ---- rolling (fmx_roll_*)
// The centre voxel, the integration's own expression; false when it is out of the key range.
bool roll_centre_voxel(const fmx_ctx* c, const double centre[3], long long cc[3]) {
  for (int k = 0; k < 3; ++k) {
    const double v = std::floor(centre[k] / c->dense.voxel_w);
    if (!(std::fabs(v) < 1048575.0)) return false;  // 2^20 - 1, in fp64 before the cast
    cc[k] = (long long)v;
  }
  return true;
}
void roll_check_box(const fmx_ctx* c, const double* centre, const uint32_t* half, long long cc[3]) {
  if (!centre || !half) throw StatusError(FMX_E_INVAL, "null roll centre or half-extents");
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(centre[k])) throw StatusError(FMX_E_INVAL, "non-finite roll centre");
    if (half[k] > (1u << 21)) throw StatusError(FMX_E_INVAL, "roll half-extents are at most 2^21 voxels");
  }
  if (!roll_centre_voxel(c, centre, cc)) throw StatusError(FMX_E_INVAL, "the roll centre's voxel is out of range");
}
// After run_roll_count gave {kept, evicted} with evicted > 0: size the buffers (FMX_E_OOM
// with nothing changed), split, reinsert, take the new voxel total.  Queued only.
void roll_rebuild(fmx_ctx* c, const long long cc[3], const uint32_t half[3], uint32_t kept, uint32_t evicted) {
  auto& D = c->dense;
  roll_ensure(D.o_xyz, 3 * (size_t)evicted);
  roll_ensure(D.o_tag, evicted);
  roll_ensure(D.o_hits, evicted);
  if (kept) {
    roll_ensure(D.roll.s_key, kept);
    roll_ensure(D.roll.s_tag, kept);
    roll_ensure(D.roll.s_hits, kept);
    roll_ensure(D.roll.s_xyz, 3 * (size_t)kept);
  }
  if (D.carve.have) {  // the miss counts travel with the voxels
    roll_ensure(D.carve.o_miss, evicted);
    if (kept) roll_ensure(D.carve.s_miss, kept);
  }
  normals_stale(c);
  run_roll_rebuild(c, cc, half, kept, evicted, c->stream);
  D.voxels = kept;
}

// ---- probing and the nearest solid voxel (fmx_probe_points, fmx_probe_rays,
// fmx_nearest_voxels; probe_host.hpp, nearest_host.hpp)
// What the three have in common once the caller has checked its arguments: the per-call
// buffers, the scan staged, one launch, the copies out.  word: "probe" / "nearest", for the
// messages; offsets: the launch reads the cube's offsets; step, t: asked for or null (t holds
// the search's dist2); launch(d, o): queue the kernel over the device points d with outputs
// o; cnt: the launch's five counters.
template <class Launch>
void query_call(fmx_ctx* c, const char* word, bool offsets, const float* xyzw, size_t n, int src_on_dev, uint8_t* state,
                uint32_t* step, double* t, const fmx_voxel_arrays* voxels, unsigned long long cnt[5], Launch&& launch) {
  auto& D = c->dense;
  auto& P = D.probe;
  dense_settle(c);
  for (int k = 0; k < 5; ++k) cnt[k] = 0;
  if (!n) return;
  const fmx_voxel_arrays A = voxels ? *voxels : fmx_voxel_arrays{};
  const bool want_tag = A.scan || A.index;
  // every buffer before anything is launched or written (FMX_E_OOM when one cannot be had)
  const std::string what = std::string("dense map ") + word;
  const auto ensure = [&](auto& b, size_t m) { roll_ensure(b, m, what.c_str()); };
  if (offsets) offsets_ensure(c, what.c_str());
  ensure(P.cnt, 8);
  ensure(P.state, n);
  if (step) ensure(P.step, n);
  if (t) ensure(P.t, n);
  if (want_tag) ensure(P.tag, n);
  if (A.hits) ensure(P.hits, n);
  if (A.misses) ensure(P.misses, n);
  if (A.xyz) ensure(P.xyz, 3 * n);
  if (!src_on_dev) ensure(D.in, n);
  std::vector<uint8_t> own_state;
  std::vector<unsigned long long> tag;
  if (want_tag) {
    tag.resize(n);
    if (!state) own_state.resize(n);
  }
  uint8_t* h_state = state ? state : (want_tag ? own_state.data() : nullptr);
  const float4* d = scan_on_device(c, xyzw, n, src_on_dev);
  launch(d, ProbeOut{P.state.p,
                     step ? P.step.p : nullptr,
                     t ? P.t.p : nullptr,
                     want_tag ? P.tag.p : nullptr,
                     A.hits ? P.hits.p : nullptr,
                     A.misses ? P.misses.p : nullptr,
                     A.xyz ? P.xyz.p : nullptr});
  const auto out = [&](void* dst, const void* src, size_t bytes) {
    if (dst) FMX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  };
  out(cnt, P.cnt.p, 5 * sizeof(unsigned long long));
  out(h_state, P.state.p, n);
  out(step, P.step.p, n * sizeof(uint32_t));
  out(t, P.t.p, n * sizeof(double));
  out(want_tag ? tag.data() : nullptr, P.tag.p, n * sizeof(unsigned long long));
  out(A.hits, P.hits.p, n * sizeof(uint32_t));
  out(A.misses, P.misses.p, n * sizeof(uint32_t));
  out(A.xyz, P.xyz.p, 3 * n * sizeof(double));
  FMX_HIP(hipStreamSynchronize(c->stream));  // the caller owns the points again
  if (want_tag && !probe_resolve(h_state, tag.data(), n, D.seq_scan, A.scan, A.index))
    throw StatusError(FMX_E_STATE, std::string(word) + ": a voxel's tag names an integration the context does not know");
}

// ---- aligning (fmx_align_system, fmx_align_dense; align_host.hpp).  align_begin: the checks,
// the per-call buffers, the scan staged once; align_eval: one system at a pose (one memset,
// one launch, one wait on the completion word).
struct AlignCall {
  const float4* d = nullptr;
  size_t n = 0;
  fmx_align_params prm{};
};
AlignCall align_begin(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double* pose34,
                      const fmx_align_params* prm) {
  auto& D = c->dense;
  auto& A = D.align;
  checked([&](const char** why) { return align_check(xyzw, (unsigned long long)n, pose34, prm, why); });
  dense_settle(c);
  AlignCall call;
  call.n = n;
  call.prm = *prm;
  if (!n) return call;
  // every buffer before anything is launched or written (FMX_E_OOM when one cannot be had)
  const auto ensure = [](auto& b, size_t m) { roll_ensure(b, m, "dense map align"); };
  offsets_ensure(c, "dense map align");
  ensure(A.cnt, 8);
  ensure(A.bpart, align_partials());
  if (!A.ticket.p) {
    ensure(A.ticket, 1);
    FMX_HIP(hipMemsetAsync(A.ticket.p, 0, A.ticket.cap * sizeof(uint32_t), c->stream));
  }
  if (!src_on_dev) ensure(D.in, n);
  A.h_out.ensure(40);
  call.d = scan_on_device(c, xyzw, n, src_on_dev);
  return call;
}
// run: run_align or run_plane.  S and the kernel's counters k (the point rows write five of
// the six), all zero when there are no points.
void align_launch(fmx_ctx* c, const AlignCall& call, const double* pose34, decltype(run_align)* run, double S[29],
                  unsigned long long k[6]) {
  auto& A = c->dense.align;
  for (int i = 0; i < 29; ++i) S[i] = 0.0;
  for (int i = 0; i < 6; ++i) k[i] = 0;
  if (!call.n) return;
  const uint32_t seq = next_flag(c);
  run(c, call.d, call.n, align_stride(call.prm), pose34, probe_filter(call.prm.min_hits, call.prm.miss_num, call.prm.miss_den),
      call.prm.reach, call.prm.max_dist2, call.prm.sigma, seq, c->stream);
  wait_flag(c, c->h_flag.p, seq);
  std::memcpy(S, A.h_out.p, 29 * sizeof(double));
  std::memcpy(k, A.h_out.p + 32, (run == run_plane ? 6 : 5) * sizeof(unsigned long long));
}
void align_eval(fmx_ctx* c, const AlignCall& call, const double* pose34, double S[29], fmx_align_counts* cnt) {
  unsigned long long k[6];
  align_launch(c, call, pose34, run_align, S, k);
  const unsigned long long kept = align_kept((unsigned long long)call.n, align_stride(call.prm));
  if (cnt)
    *cnt = fmx_align_counts{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3],
                            (uint32_t)((unsigned long long)call.n - kept), k[4]};
}
void plane_eval(fmx_ctx* c, const AlignCall& call, const double* pose34, double S[29], fmx_plane_counts* cnt) {
  unsigned long long k[6];
  align_launch(c, call, pose34, run_plane, S, k);
  if (cnt) *cnt = plane_counts(k, (unsigned long long)call.n, align_stride(call.prm));
}
// fmx_plane_*: the map on and the normal snapshot current.
void need_normals(const fmx_ctx* c) {
  need_map(c);
  if (!c->dense.normals.current)
    throw StatusError(FMX_E_STATE, c->dense.normals.built ? "the normal snapshot is stale: the table changed since fmx_normals_build"
                                                          : "no normal snapshot (fmx_normals_build)");
}

// ---- pose batches (fmx_score_poses, fmx_refine_systems, fmx_refine_poses; score_host.hpp,
// refine_host.hpp), the caller having run the checks and settled the queue.  pose_batch_begin:
// the buffers `buf` of the feature `what` for the largest chunk of at most n_poses poses, every
// one before anything is launched or written (FMX_E_OOM when one cannot be had), then the scan
// staged once; nothing without points.  pose_batch_eval: the records of `count` <= n_poses poses
// into host memory, chunk by chunk (the poses staged, run(k) queueing the two launches over
// them, the records' copy out), one wait at the end; all zeros without points.
struct PoseBatchCall {
  const float4* d = nullptr;
  size_t n = 0;
  fmx_align_params prm{};
  bool plane = false;
  uint32_t every = 1, chunk = 1;
  ProbeFilter f{};
};
template <class B>
PoseBatchCall pose_batch_begin(fmx_ctx* c, B& buf, const char* what, const BatchPlan& plan, const float* xyzw, size_t n,
                               int src_on_dev, uint32_t n_poses, const fmx_align_params* prm, bool plane) {
  PoseBatchCall call{nullptr, n, *prm, plane, align_stride(*prm), plan.chunk,
                     probe_filter(prm->min_hits, prm->miss_num, prm->miss_den)};
  if (!n) return call;
  const uint32_t most = std::min(plan.chunk, n_poses);  // the poses of the largest chunk
  const auto ensure = [&](auto& b, size_t m) { roll_ensure(b, m, what); };
  offsets_ensure(c, what);
  ensure(buf.poses, (size_t)most * 12);
  ensure(buf.part, (size_t)most * plan.tiles);
  ensure(buf.out, most);
  if (!src_on_dev) ensure(c->dense.in, n);
  call.d = scan_on_device(c, xyzw, n, src_on_dev);
  return call;
}
template <class B, class Rec, class Run>
void pose_batch_eval(fmx_ctx* c, B& buf, const PoseBatchCall& call, const double* poses34, uint32_t count, Rec* out, Run&& run) {
  if (!call.n) {
    std::memset(out, 0, (size_t)count * sizeof(Rec));
    return;
  }
  for (uint32_t k0 = 0; k0 < count; k0 += call.chunk) {
    const uint32_t k = std::min(call.chunk, count - k0);
    FMX_HIP(hipMemcpyAsync(buf.poses.p, poses34 + (size_t)k0 * 12, (size_t)k * 12 * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
    run(k);
    FMX_HIP(hipMemcpyAsync(out + k0, buf.out.p, (size_t)k * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
  }
  FMX_HIP(hipStreamSynchronize(c->stream));  // the caller owns the points and the poses again
}
// fmx_score_plan's and fmx_refine_plan's body.
fmx_status plan_export(const BatchPlan& p, uint32_t out[6]) {
  const uint32_t v[6] = {p.kept, p.tile, p.tiles, p.chunk, p.chunks, p.cap};
  std::memcpy(out, v, sizeof(v));
  return FMX_OK;
}

PoseBatchCall refine_begin(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, uint32_t n_poses,
                           const fmx_align_params* prm, bool plane) {
  return pose_batch_begin(c, c->dense.refine, "dense map refine", refine_plan((unsigned long long)n, prm->stride, n_poses), xyzw, n,
                          src_on_dev, n_poses, prm, plane);
}
void refine_eval(fmx_ctx* c, const PoseBatchCall& call, const double* poses34, uint32_t count, fmx_refine_system* out) {
  pose_batch_eval(c, c->dense.refine, call, poses34, count, out, [&](uint32_t k) {
    run_refine(c, call.d, call.n, call.every, k, call.f, call.prm.reach, call.prm.max_dist2, call.prm.sigma, call.plane, c->stream);
  });
}

}  // namespace

// ============================================================================ register_scan's four
namespace fmx {

// Queue the integration of the n device points at d (the capacity rule checked by the
// caller) on the context stream; returns the completion word's value to wait for, 0 when
// nothing was launched (n = 0: an integration that counts nothing).
// With carving on and this integration's number a multiple of its `every`, the mark and the
// rays follow on the same stream (none when the origin's voxel is out of range, or n = 0: a
// carve that casts no ray).
uint32_t dense_queue(fmx_ctx* c, const float4* d, size_t n, const double* pose34, uint64_t scan_idx) {
  auto& D = c->dense;
  auto& Cv = D.carve;
  D.used = true;
  uint32_t flag = 0;
  // the tag's owner number; the integration's own number, which `every` counts, is apart
  // from it once an upload has drawn owner numbers too (fmx_upload_voxels)
  const uint32_t seq = (uint32_t)D.seq_scan.size();
  Cv.last = fmx_carve_counts{};
  Cv.last_carved = Cv.have && Cv.cfg.on && D.integrations % Cv.cfg.every == 0 ? 1 : 0;
  if (n) {
    flag = D.flag_seq + 1;
    normals_stale(c);
    run_dense_integrate(c, d, n, pose34, seq, flag, c->stream);
    D.flag_seq = D.pending = flag;
    if (Cv.last_carved && carve_origin_ok(pose34, D.voxel_w)) carve_queue(c, d, n, pose34, seq + 1);
  } else {
    std::memset(D.h_res.p, 0, 5 * sizeof(uint32_t));
  }
  D.seq_scan.push_back(scan_idx);
  D.integrations++;
  return flag;
}
// Wait for it (the fill's last block has then seen every block's ticket: the scan is read),
// take the new voxel total and the counts.
void dense_finish(fmx_ctx* c, uint32_t flag, fmx_dense_counts* out) {
  auto& D = c->dense;
  if (flag) {
    wait_flag(c, D.h_res.p + 7, flag, c->stream);
    D.voxels = D.h_res.p[5];
    D.pending = 0;
  }
  if (out) {
    const uint32_t* h = D.h_res.p;
    *out = fmx_dense_counts{h[0], h[1], h[2], h[3], h[4]};
  }
  carve_finish(c, &D.carve.last);  // the rays behind it: they have read the scan too
}
// An integration whose wait never ran (the call that queued it failed in between): its
// voxel total is taken before anything reads or relies on the host's copy.
void dense_settle(fmx_ctx* c) {
  if (c->dense.pending) dense_finish(c, c->dense.pending, nullptr);
  carve_finish(c, &c->dense.carve.last);
}
// Register path, at the start of scan j >= 1's registration (the previous integration is
// settled): p is scan j - 1's final translation; due: scan j would be integrated by `every`.
// Never fails the registration for a centre out of range or a failed allocation.
void roll_on_register(fmx_ctx* c, uint64_t j, const double p[3], bool due, size_t n) {
  auto& D = c->dense;
  auto& Rl = D.roll;
  if (!Rl.have_centre) {
    std::memcpy(Rl.centre, p, sizeof(Rl.centre));
    Rl.have_centre = true;
    return;
  }
  double far = 0.0;
  for (int k = 0; k < 3; ++k) far = std::max(far, std::fabs(p[k] - Rl.centre[k]));
  if (!(far >= Rl.step) && !(due && D.voxels + n > D.max_voxels)) return;
  long long cc[3];
  if (!roll_centre_voxel(c, p, cc)) return;
  uint32_t io[2];
  run_roll_count(c, cc, Rl.half, io, c->stream);
  const uint32_t kept = io[0], evicted = io[1];
  if (evicted) {
    try {
      if (Rl.spill) Rl.sp.reserve(evicted);
      roll_rebuild(c, cc, Rl.half, kept, evicted);
    } catch (const std::bad_alloc&) {
      return;
    } catch (const StatusError& e) {
      if (e.st == FMX_E_OOM) return;
      throw;
    }
    if (Rl.spill) {
      const size_t at = Rl.sp.grow(evicted);  // within the reserved room: no allocation
      list_fetch(c, evicted,
                 fmx_voxel_arrays{Rl.sp.xyz.data() + 3 * at, Rl.sp.scan.data() + at, Rl.sp.index.data() + at,
                                  Rl.sp.hits.data() + at, Rl.sp.misses.data() + at});
    }
  }
  std::memcpy(Rl.centre, p, sizeof(Rl.centre));
  Rl.rolls++;
  Rl.evicted_total += evicted;
  Rl.last_kept = kept;
  Rl.last_evicted = evicted;
  Rl.last_scan = j;
}

}  // namespace fmx

// ============================================================================ C ABI
extern "C" {

// ---- dense voxel map
fmx_status fmx_dense_configure(fmx_ctx* c, const fmx_dense_params* p) {
  return guard<false>(c, [&] {
    if (!p) throw StatusError(FMX_E_INVAL, "null dense map parameters");
    auto& D = c->dense;
    if (c->est || D.used)
      throw StatusError(FMX_E_STATE, "fmx_dense_configure after the first registration or integration");
    if (!p->enable) {
      sync_all(c);
      dense_release(c);
      return;
    }
    if (!(p->voxel_width > 0.0) || !std::isfinite(p->voxel_width))
      throw StatusError(FMX_E_INVAL, "dense map: the voxel width must be finite and positive");
    if (p->max_voxels == 0 || p->max_voxels > (1ull << 29))
      throw StatusError(FMX_E_INVAL, "dense map: max_voxels must be in [1, 2^29]");
    double min2 = p->min_norm_squared, max2 = p->max_norm_squared;
    if (min2 == 0.0 && max2 == 0.0) {
      min2 = c->P.extraction.min_norm_squared;
      max2 = c->P.extraction.max_norm_squared;
    }
    if (!(min2 >= 0.0) || !(max2 > min2))  // also rejects NaN
      throw StatusError(FMX_E_INVAL, "dense map: the range gate must satisfy 0 <= min_norm_squared < max_norm_squared");
    uint64_t slots = 2;
    while (slots < 2 * p->max_voxels) slots <<= 1;
    sync_all(c);
    dense_release(c);
    try {
      alloc_exact(D.keys, slots);
      alloc_exact(D.tags, slots);
      alloc_exact(D.hits, slots);
      alloc_exact(D.xyz, 3 * slots);
    } catch (...) {
      dense_release(c);
      throw;
    }
    D.voxel_w = p->voxel_width;
    D.min2 = min2;
    D.max2 = max2;
    D.every = p->every ? p->every : 1;
    D.max_voxels = p->max_voxels;
    D.slots = slots;
    D.cnt.ensure(8);
    D.out_n.ensure(1);
    D.h_n.ensure(1);
    D.h_res.ensure(8);
    std::memset(D.h_res.p, 0, 8 * sizeof(uint32_t));
    D.flag_seq = D.pending = 0;
    // every per-scan buffer now: a registration allocates nothing for the map
    const auto& E = c->P.extraction;
    const size_t RC = (size_t)(E.num_rows > 0 ? E.num_rows : 0) * (size_t)(E.num_columns > 0 ? E.num_columns : 0);
    if (RC) {
      D.slot_of.ensure(RC);
      D.keep.ensure(RC);
    }
    run_dense_clear(c, c->stream);  // on the context stream, which the claims are ordered behind
    D.on = true;
  });
}

fmx_status fmx_dense_integrate(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                               uint64_t scan_idx, fmx_dense_counts* counts) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    need_map(c);
    dense_settle(c);
    checked([&](const char** why) {
      return scan_check(xyzw, (unsigned long long)n, pose34, "an integration holds fewer than 2^32 points", why);
    });
    need_room(c, n, "points");
    if (D.seq_scan.size() >= 0xFFFFFFFEull) throw StatusError(FMX_E_STATE, "dense map: owner numbering exhausted");
    if (n && !src_on_dev) D.in.ensure(n);
    const uint32_t flag = dense_queue(c, scan_on_device(c, xyzw, n, src_on_dev), n, pose34, scan_idx);
    dense_finish(c, flag, counts);  // the caller owns the points again
  });
}

fmx_status fmx_dense_last(fmx_ctx* c, fmx_dense_counts* counts, int* integrated) {
  return guard<false>(c, [&] {
    if (counts) *counts = c->dense.last;
    if (integrated) *integrated = c->dense.last_integrated;
  });
}

fmx_status fmx_dense_stats(fmx_ctx* c, uint64_t out[4]) {
  return guard<false>(c, [&] {
    if (!out) throw StatusError(FMX_E_INVAL, "null output");
    dense_settle(c);
    const auto& D = c->dense;
    out[0] = D.voxels;
    out[1] = D.max_voxels;
    out[2] = D.integrations;
    out[3] = D.slots;
  });
}

fmx_status fmx_carve_download(fmx_ctx* c, uint32_t min_hits, uint32_t miss_num, uint32_t miss_den,
                              const fmx_voxel_arrays* arrays, uint32_t* n) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    need_map(c);
    dense_settle(c);
    if (!n) throw StatusError(FMX_E_INVAL, "null count");
    const fmx_voxel_arrays A = arrays ? *arrays : fmx_voxel_arrays{};
    const uint32_t mh = min_hits ? min_hits : 1;
    const uint32_t count = run_dense_count(c, mh, miss_num, miss_den, c->stream);
    if (!any_array(A)) {  // the sizing call
      *n = count;
      return;
    }
    if (*n < count)
      throw StatusError(FMX_E_SIZE, "dense map download: room for " + std::to_string(*n) + " of " +
                                        std::to_string(count) + " voxels");
    if (count) {
      const bool with_misses = A.misses && D.carve.have;
      if (with_misses) D.carve.o_miss.ensure(count);
      run_dense_compact(c, mh, miss_num, miss_den, with_misses, count, c->stream);
      list_fetch(c, count, A);
    }
    *n = count;
  });
}

fmx_status fmx_dense_download(fmx_ctx* c, uint32_t min_hits, double* xyz, uint64_t* scan, uint32_t* index,
                              uint32_t* hits, uint32_t* n) {
  const fmx_voxel_arrays A{xyz, scan, index, hits, nullptr};
  return fmx_carve_download(c, min_hits, 0, 0, &A, n);
}

fmx_status fmx_upload_voxels(fmx_ctx* c, const fmx_voxel_input* in, uint32_t n, fmx_upload_counts* counts) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    auto& U = D.upload;
    checked([&](const char** why) { return upload_check(in, n, D.on, D.carve.have, why); });
    dense_settle(c);
    if (counts) *counts = fmx_upload_counts{};
    if (!n) return;
    need_room(c, n, "entries");
    // the owner numbers, the table's room for them and every buffer before anything is
    // launched or changed (FMX_E_OOM when one cannot be had)
    UploadOwners own;
    if (!upload_owners(in->scan, n, D.seq_scan.size(), &own))
      throw StatusError(FMX_E_STATE, "dense map: owner numbering exhausted");
    D.seq_scan.reserve(D.seq_scan.size() + own.scans.size());
    const auto up_ensure = [](auto& b, size_t m) { roll_ensure(b, m, "dense map upload"); };
    up_ensure(U.cnt, 4);
    up_ensure(U.xyz, 3 * (size_t)n);
    up_ensure(U.owner, n);
    up_ensure(U.slot, n);
    if (in->index) up_ensure(U.index, n);
    if (in->hits) up_ensure(U.hits, n);
    if (in->misses) up_ensure(U.misses, n);
    try {
      U.h_cnt.ensure(4);
    } catch (const HipError&) {
      (void)hipGetLastError();
      throw StatusError(FMX_E_OOM, "dense map upload: pinned host allocation failed");
    }
    const auto put = [&](void* dst, const void* src, size_t bytes) {
      if (src) FMX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    };
    put(U.xyz.p, in->xyz, 3 * (size_t)n * sizeof(double));
    put(U.owner.p, own.owner.data(), (size_t)n * sizeof(uint32_t));
    put(U.index.p, in->index, (size_t)n * sizeof(uint32_t));
    put(U.hits.p, in->hits, (size_t)n * sizeof(uint32_t));
    put(U.misses.p, in->misses, (size_t)n * sizeof(uint32_t));
    // (within the reserved room; before the launches, so that no tag ever names an owner the table lacks)
    D.seq_scan.insert(D.seq_scan.end(), own.scans.begin(), own.scans.end());
    D.used = true;  // the configuration is final, as after an integration
    normals_stale(c);
    run_dense_upload(c, n, in->index != nullptr, in->hits != nullptr, in->misses != nullptr, own.temp, c->stream);
    FMX_HIP(hipMemcpyAsync(U.h_cnt.p, U.cnt.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    FMX_HIP(hipStreamSynchronize(c->stream));  // the caller owns the arrays again (own.owner too)
    const uint32_t invalid = U.h_cnt.p[0], oor = U.h_cnt.p[1], added = U.h_cnt.p[2];
    D.voxels += added;
    if (counts) *counts = fmx_upload_counts{added, n - invalid - oor - added, oor, invalid};
  });
}

fmx_status fmx_dense_clear(fmx_ctx* c) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    need_map(c);
    dense_settle(c);
    normals_stale(c);
    run_dense_clear(c, c->stream);
    D.voxels = 0;
    D.seq_scan.clear();
    D.integrations = 0;
    D.roll.have_centre = false;  // (the spill holds scan_idx values: it stays)
  });
}

// ---- rolling the dense map
fmx_status fmx_roll_configure(fmx_ctx* c, const fmx_roll_params* p) {
  return guard<false>(c, [&] {
    if (!p) throw StatusError(FMX_E_INVAL, "null roll parameters");
    need_map(c);
    for (int k = 0; k < 3; ++k)
      if (p->half[k] > (1u << 21)) throw StatusError(FMX_E_INVAL, "roll half-extents are at most 2^21 voxels");
    if (!(p->step >= 0.0) || !std::isfinite(p->step)) throw StatusError(FMX_E_INVAL, "the roll step must be finite and >= 0");
    auto& Rl = c->dense.roll;
    Rl.on = p->enable != 0;
    for (int k = 0; k < 3; ++k) Rl.half[k] = p->half[k];
    Rl.step = p->step;
    Rl.spill = p->spill != 0;
    Rl.have_centre = false;
  });
}

fmx_status fmx_roll_count(fmx_ctx* c, const double centre[3], const uint32_t half[3], uint64_t out[2]) {
  return guard<false>(c, [&] {
    need_map(c);
    if (!out) throw StatusError(FMX_E_INVAL, "null output");
    long long cc[3];
    roll_check_box(c, centre, half, cc);
    dense_settle(c);
    uint32_t io[2];
    run_roll_count(c, cc, half, io, c->stream);
    out[0] = io[0];
    out[1] = io[1];
  });
}

fmx_status fmx_carve_evict(fmx_ctx* c, const double centre[3], const uint32_t half[3],
                           const fmx_voxel_arrays* arrays, uint32_t* n) {
  return guard<false>(c, [&] {
    need_map(c);
    const fmx_voxel_arrays A = arrays ? *arrays : fmx_voxel_arrays{};
    const bool any = any_array(A);
    if (any && !n) throw StatusError(FMX_E_INVAL, "null count");
    long long cc[3];
    roll_check_box(c, centre, half, cc);
    dense_settle(c);
    uint32_t io[2];
    run_roll_count(c, cc, half, io, c->stream);
    const uint32_t kept = io[0], evicted = io[1];
    if (any && *n < evicted)
      throw StatusError(FMX_E_SIZE, "dense map roll: room for " + std::to_string(*n) + " of " + std::to_string(evicted) +
                                        " evicted voxels");
    if (evicted) {
      roll_rebuild(c, cc, half, kept, evicted);
      if (any) list_fetch(c, evicted, A);
    }
    if (n) *n = evicted;
  });
}

fmx_status fmx_roll_evict(fmx_ctx* c, const double centre[3], const uint32_t half[3], double* xyz, uint64_t* scan,
                          uint32_t* index, uint32_t* hits, uint32_t* n) {
  const fmx_voxel_arrays A{xyz, scan, index, hits, nullptr};
  return fmx_carve_evict(c, centre, half, &A, n);
}

fmx_status fmx_carve_drain(fmx_ctx* c, const fmx_voxel_arrays* arrays, uint32_t* n) {
  return guard<false>(c, [&] {
    need_map(c);
    if (!n) throw StatusError(FMX_E_INVAL, "null count");
    const fmx_voxel_arrays A = arrays ? *arrays : fmx_voxel_arrays{};
    auto& Rl = c->dense.roll;
    if (Rl.sp.size() > 0xFFFFFFFFull) throw StatusError(FMX_E_SIZE, "the spill holds more than 2^32 - 1 voxels");
    const uint32_t count = (uint32_t)Rl.sp.size();
    if (!any_array(A)) {  // the sizing call
      *n = count;
      return;
    }
    if (*n < count)
      throw StatusError(FMX_E_SIZE, "roll drain: room for " + std::to_string(*n) + " of " + std::to_string(count) + " voxels");
    Rl.sp.drain(A.xyz, A.scan, A.index, A.hits, A.misses);
    *n = count;
  });
}

fmx_status fmx_roll_drain(fmx_ctx* c, double* xyz, uint64_t* scan, uint32_t* index, uint32_t* hits, uint32_t* n) {
  const fmx_voxel_arrays A{xyz, scan, index, hits, nullptr};
  return fmx_carve_drain(c, &A, n);
}

fmx_status fmx_roll_stats(fmx_ctx* c, uint64_t out[6]) {
  return guard<false>(c, [&] {
    if (!out) throw StatusError(FMX_E_INVAL, "null output");
    const auto& Rl = c->dense.roll;
    out[0] = Rl.rolls;
    out[1] = Rl.evicted_total;
    out[2] = Rl.sp.size();
    out[3] = Rl.last_kept;
    out[4] = Rl.last_evicted;
    out[5] = Rl.last_scan;
  });
}

// ---- carving the dense map (carve_host.hpp)
fmx_status fmx_carve_configure(fmx_ctx* c, const fmx_carve_params* p) {
  return guard<false>(c, [&] {
    need_map(c);
    auto& D = c->dense;
    auto& Cv = D.carve;
    CarveCfg cfg;
    checked([&](const char** why) { return carve_check(p, D.max2, &cfg, why); });
    dense_settle(c);
    if (cfg.on && !Cv.have) {
      // exactly `slots` entries each, as the table's own arrays; nothing kept on a failure
      DBuf<uint32_t> misses, seen;
      alloc_exact(misses, D.slots);
      alloc_exact(seen, D.slots);
      Cv.cnt.ensure(8);
      Cv.h_res.ensure(8);
      std::memset(Cv.h_res.p, 0, 8 * sizeof(unsigned long long));
      Cv.flag_seq = Cv.pending = 0;
      FMX_HIP(hipMemsetAsync(misses.p, 0, D.slots * sizeof(uint32_t), c->stream));
      FMX_HIP(hipMemsetAsync(seen.p, 0, D.slots * sizeof(uint32_t), c->stream));
      FMX_HIP(hipMemsetAsync(Cv.cnt.p, 0, 8 * sizeof(unsigned long long), c->stream));
      FMX_HIP(hipStreamSynchronize(c->stream));
      Cv.misses = std::move(misses);
      Cv.seen = std::move(seen);
      Cv.have = true;  // (the per-scan scratch it uses, slot_of, is the integration's own)
    }
    Cv.cfg = cfg;
  });
}

fmx_status fmx_carve_rays(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                          fmx_carve_counts* counts) {
  return guard<false>(c, [&] {
    need_map(c);
    auto& D = c->dense;
    if (!D.carve.have) throw StatusError(FMX_E_STATE, "carving has not been enabled on this map (fmx_carve_configure)");
    dense_settle(c);
    checked([&](const char** why) {
      return scan_check(xyzw, (unsigned long long)n, pose34, "a carve holds fewer than 2^32 points", why);
    });
    fmx_carve_counts out{};
    if (n && carve_origin_ok(pose34, D.voxel_w)) {
      if (!src_on_dev) D.in.ensure(n);
      carve_queue(c, scan_on_device(c, xyzw, n, src_on_dev), n, pose34, 0);
      carve_finish(c, &out);  // the caller owns the points again
    }
    if (counts) *counts = out;
  });
}

fmx_status fmx_carve_last(fmx_ctx* c, fmx_carve_counts* counts, int* carved) {
  return guard<false>(c, [&] {
    if (counts) *counts = c->dense.carve.last;
    if (carved) *carved = c->dense.carve.last_carved;
  });
}

// ---- probing the dense map (probe_host.hpp)
fmx_status fmx_probe_points(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                            uint32_t min_hits, uint32_t miss_num, uint32_t miss_den, uint8_t* state,
                            const fmx_voxel_arrays* voxels, fmx_probe_point_counts* counts) {
  return guard<false>(c, [&] {
    need_map(c);
    checked([&](const char** why) { return probe_check(xyzw, (unsigned long long)n, pose34, why); });
    const ProbeFilter f = probe_filter(min_hits, miss_num, miss_den);
    unsigned long long k[5];
    query_call(c, "probe", false, xyzw, n, src_on_dev, state, nullptr, nullptr, voxels, k,
               [&](const float4* d, const ProbeOut& o) { run_probe_points(c, d, n, pose34, f, o, c->stream); });
    if (counts)
      *counts = fmx_probe_point_counts{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3], (uint32_t)k[4]};
  });
}

fmx_status fmx_probe_rays(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                          uint32_t min_hits, uint32_t miss_num, uint32_t miss_den, uint32_t skip, uint8_t* state,
                          uint32_t* step, double* t, const fmx_voxel_arrays* voxels, fmx_probe_ray_counts* counts) {
  return guard<false>(c, [&] {
    need_map(c);
    checked([&](const char** why) { return probe_check(xyzw, (unsigned long long)n, pose34, why); });
    if (!probe_origin_ok(pose34, c->dense.voxel_w))
      throw StatusError(FMX_E_RANGE, "probe: the voxel of the ray origin is out of range");
    const ProbeFilter f = probe_filter(min_hits, miss_num, miss_den);
    unsigned long long k[5];
    query_call(c, "probe", false, xyzw, n, src_on_dev, state, step, t, voxels, k,
               [&](const float4* d, const ProbeOut& o) { run_probe_rays(c, d, n, pose34, f, skip, o, c->stream); });
    if (counts) *counts = fmx_probe_ray_counts{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3], k[4]};
  });
}

// ---- the nearest solid voxel (nearest_host.hpp)
fmx_status fmx_nearest_voxels(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                              uint32_t min_hits, uint32_t miss_num, uint32_t miss_den, uint32_t reach, double max_dist2,
                              uint8_t* state, double* dist2, const fmx_voxel_arrays* voxels, fmx_nearest_counts* counts) {
  return guard<false>(c, [&] {
    need_map(c);
    checked([&](const char** why) { return nearest_check(xyzw, (unsigned long long)n, pose34, reach, max_dist2, why); });
    const ProbeFilter f = probe_filter(min_hits, miss_num, miss_den);
    unsigned long long k[5];
    query_call(c, "nearest", true, xyzw, n, src_on_dev, state, nullptr, dist2, voxels, k,
               [&](const float4* d, const ProbeOut& o) { run_nearest(c, d, n, pose34, f, reach, max_dist2, o, c->stream); });
    if (counts) *counts = fmx_nearest_counts{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3], k[4]};
  });
}

// ---- aligning a scan to the dense map (align_host.hpp)
fmx_status fmx_align_system(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                            const fmx_align_params* prm, double out[29], fmx_align_counts* counts) {
  return guard<false>(c, [&] {
    need_map(c);
    if (!out) throw StatusError(FMX_E_INVAL, "null output");
    const AlignCall call = align_begin(c, xyzw, n, src_on_dev, pose34, prm);
    align_eval(c, call, pose34, out, counts);
  });
}

fmx_status fmx_align_dense(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose_init34[12],
                           const fmx_align_params* prm, uint32_t max_iters, double threshold, double pose_out34[12],
                           fmx_align_result* result) {
  return guard<false>(c, [&] {
    need_map(c);
    checked([&](const char** why) { return align_loop_check(pose_out34, threshold, why); });
    const AlignCall call = align_begin(c, xyzw, n, src_on_dev, pose_init34, prm);
    fmx_align_result R{};
    double T[12];
    const char* why = "";
    const fmx_status st = align_loop(
        pose_init34, max_iters, threshold,
        [&](const double* pose, double* S, fmx_align_counts* k) { align_eval(c, call, pose, S, k); }, T, &R, &why);
    if (!R.iters && n && !src_on_dev) stream_wait(c);  // no system waited for the staged scan: the caller owns it again
    if (st != FMX_OK) throw StatusError(st, why);
    std::memcpy(pose_out34, T, sizeof(T));
    if (result) *result = R;
  });
}

// ---- scoring many candidate poses (score_host.hpp).  The queries' path: the checks, the queue
// settled, then pose_batch_begin and one pose_batch_eval.
fmx_status fmx_score_poses(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double* poses34,
                           uint32_t n_poses, const fmx_align_params* prm, fmx_pose_score* scores) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    need_map(c);
    checked([&](const char** why) {
      return score_check(xyzw, (unsigned long long)n, poses34, (unsigned long long)n_poses, prm, scores, why);
    });
    dense_settle(c);
    if (!n_poses) return;
    const PoseBatchCall call = pose_batch_begin(c, D.score, "dense map score", score_plan((unsigned long long)n, prm->stride, n_poses),
                                                xyzw, n, src_on_dev, n_poses, prm, false);
    pose_batch_eval(c, D.score, call, poses34, n_poses, scores, [&](uint32_t k) {
      run_score(c, call.d, n, call.every, k, call.f, prm->reach, prm->max_dist2, c->stream);
    });
  });
}

fmx_status fmx_score_plan(uint64_t n_points, uint32_t stride, uint32_t n_poses, uint32_t out[6]) {
  if (!out || n_poses > (uint32_t)FMX_SCORE_MAX_POSES || n_points >= (1ull << 32)) return FMX_E_INVAL;
  return plan_export(score_plan(n_points, stride, n_poses), out);
}

// ---- refining many candidate poses (refine_host.hpp).  The scoring's path: the checks, the
// queue settled, pose_batch_begin (refine_begin), then one pose_batch_eval per evaluation
// (refine_eval).
fmx_status fmx_refine_systems(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double* poses34,
                              uint32_t n_poses, const fmx_align_params* prm, int plane, fmx_refine_system* out) {
  return guard<false>(c, [&] {
    if (plane) need_normals(c);
    else need_map(c);
    checked([&](const char** why) {
      return refine_check(xyzw, (unsigned long long)n, poses34, (unsigned long long)n_poses, prm, out, why);
    });
    dense_settle(c);
    if (!n_poses) return;
    const PoseBatchCall call = refine_begin(c, xyzw, n, src_on_dev, n_poses, prm, plane != 0);
    refine_eval(c, call, poses34, n_poses, out);
  });
}

fmx_status fmx_refine_poses(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double* poses_init34,
                            uint32_t n_poses, const fmx_align_params* prm, int plane, uint32_t max_iters, double threshold,
                            double* poses_out34, fmx_refine_result* results) {
  return guard<false>(c, [&] {
    if (plane) need_normals(c);
    else need_map(c);
    checked([&](const char** why) {
      return refine_check(xyzw, (unsigned long long)n, poses_init34, (unsigned long long)n_poses, prm, poses_out34, why);
    });
    checked([&](const char** why) { return refine_loop_check(threshold, why); });
    dense_settle(c);
    if (!n_poses) return;
    PoseBatchCall call;
    if (max_iters) call = refine_begin(c, xyzw, n, src_on_dev, n_poses, prm, plane != 0);
    refine_loop(
        poses_init34, n_poses, max_iters, threshold,
        [&](const double* poses, uint32_t count, fmx_refine_system* rec) { refine_eval(c, call, poses, count, rec); },
        poses_out34, results);
  });
}

fmx_status fmx_refine_plan(uint64_t n_points, uint32_t stride, uint32_t n_poses, uint32_t out[6]) {
  if (!out || n_poses > (uint32_t)FMX_REFINE_MAX_POSES || n_points >= (1ull << 32)) return FMX_E_INVAL;
  return plan_export(refine_plan(n_points, stride, n_poses), out);
}

// ---- surface normals of the dense map (normals_host.hpp)
fmx_status fmx_normals_build(fmx_ctx* c, const fmx_normals_params* prm, fmx_normals_counts* counts) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    auto& M = D.normals;
    need_map(c);
    checked([&](const char** why) { return normals_check(prm, why); });
    dense_settle(c);
    // every buffer before anything is launched or changed (FMX_E_OOM when one cannot be had)
    offsets_ensure(c, "dense map normals");
    roll_ensure(M.cnt, 8, "dense map normals");
    if (!M.nrm.p || !M.support.p) {  // exactly `slots` entries each, as the table's own arrays
      DBuf<float4> nrm;
      DBuf<uint32_t> support;
      alloc_exact(nrm, D.slots);
      alloc_exact(support, D.slots);
      M.nrm = std::move(nrm);
      M.support = std::move(support);
    }
    try {
      M.h_cnt.ensure(8);
    } catch (const HipError&) {
      (void)hipGetLastError();
      throw StatusError(FMX_E_OOM, "dense map normals: pinned host allocation failed");
    }
    fmx_normals_counts out{};
    if (D.voxels) {  // (an empty table: nothing to launch, no record is ever indexed)
      M.current = false;
      run_normals_build(c, *prm, c->stream);
      FMX_HIP(hipMemcpyAsync(M.h_cnt.p, M.cnt.p, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      FMX_HIP(hipStreamSynchronize(c->stream));
      const unsigned long long* k = M.h_cnt.p;
      out = fmx_normals_counts{(uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3], k[4]};
    }
    M.prm = *prm;
    M.voxels = D.voxels;
    M.oriented = out.oriented;
    M.solid = normals_take(out, false);
    M.built = M.current = true;
    if (counts) *counts = out;
  });
}

fmx_status fmx_normals_stats(fmx_ctx* c, uint64_t out[4]) {
  return guard<false>(c, [&] {
    if (!out) throw StatusError(FMX_E_INVAL, "null output");
    const auto& M = c->dense.normals;
    out[0] = M.built ? 1 : 0;
    out[1] = M.current ? 1 : 0;
    out[2] = M.voxels;
    out[3] = M.oriented;
  });
}

fmx_status fmx_normals_download(fmx_ctx* c, int oriented_only, const fmx_voxel_arrays* arrays, float* normal,
                                float* flatness, uint32_t* support, uint32_t* n) {
  return guard<false>(c, [&] {
    auto& D = c->dense;
    auto& M = D.normals;
    need_normals(c);
    dense_settle(c);
    if (!n) throw StatusError(FMX_E_INVAL, "null count");
    const fmx_voxel_arrays A = arrays ? *arrays : fmx_voxel_arrays{};
    const uint32_t count = (uint32_t)(oriented_only ? M.oriented : M.solid);
    if (!any_array(A) && !normal && !flatness && !support) {  // the sizing call
      *n = count;
      return;
    }
    if (*n < count)
      throw StatusError(FMX_E_SIZE, "dense map normals download: room for " + std::to_string(*n) + " of " +
                                        std::to_string(count) + " voxels");
    if (count) {
      const bool with_misses = A.misses && D.carve.have;
      if (with_misses) D.carve.o_miss.ensure(count);
      run_normals_compact(c, M.prm, oriented_only != 0, with_misses, count, c->stream);
      const auto out = [&](void* dst, const void* src, size_t bytes) {
        if (dst) FMX_HIP(hipMemcpyAsync(dst, src, count * bytes, hipMemcpyDeviceToHost, c->stream));
      };
      out(normal, M.o_normal.p, 3 * sizeof(float));
      out(flatness, M.o_flat.p, sizeof(float));
      out(support, M.o_support.p, sizeof(uint32_t));
      list_fetch(c, count, A);  // (waits)
    }
    *n = count;
  });
}

// ---- point-to-plane alignment against the normals (align_host.hpp's checks and loop)
fmx_status fmx_plane_system(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose34[12],
                            const fmx_align_params* prm, double out[29], fmx_plane_counts* counts) {
  return guard<false>(c, [&] {
    need_normals(c);
    if (!out) throw StatusError(FMX_E_INVAL, "null output");
    const AlignCall call = align_begin(c, xyzw, n, src_on_dev, pose34, prm);
    plane_eval(c, call, pose34, out, counts);
  });
}

fmx_status fmx_plane_align(fmx_ctx* c, const float* xyzw, size_t n, int src_on_dev, const double pose_init34[12],
                           const fmx_align_params* prm, uint32_t max_iters, double threshold, double pose_out34[12],
                           fmx_plane_result* result) {
  return guard<false>(c, [&] {
    need_normals(c);
    checked([&](const char** why) { return align_loop_check(pose_out34, threshold, why); });
    const AlignCall call = align_begin(c, xyzw, n, src_on_dev, pose_init34, prm);
    fmx_plane_result R{};
    double T[12];
    const char* why = "";
    const fmx_status st = align_loop_as<fmx_plane_result>(
        pose_init34, max_iters, threshold,
        [&](const double* pose, double* S, fmx_plane_counts* k) { plane_eval(c, call, pose, S, k); }, T, &R, &why);
    if (!R.iters && n && !src_on_dev) stream_wait(c);  // no system waited for the staged scan: the caller owns it again
    if (st != FMX_OK) throw StatusError(st, why);
    std::memcpy(pose_out34, T, sizeof(T));
    if (result) *result = R;
  });
}

}  // extern "C"
