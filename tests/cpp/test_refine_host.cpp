// The host-only parts of refining candidate poses against the dense map
// (form_amd/csrc/refine_host.hpp, no HIP headers): the argument checks of fmx_refine_systems and
// fmx_refine_poses, the plan fmx_refine_plan reports, held against hand-computed plans at the
// tile and chunk edges, and the lockstep loop driven by a brute-force batch callable, each
// pose's result compared byte for byte with align_loop_as run alone on that pose.
// Built by __graft_entry__.build() (tests/cpp/refine_host.mk) with the address and
// undefined-behaviour sanitizers linked in statically; tests/test_refine_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "refine_host.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static fmx_align_params params() {
  fmx_align_params p{};
  p.min_hits = 1;
  p.reach = 1;
  p.max_dist2 = std::numeric_limits<double>::infinity();
  p.sigma = 0.1;
  p.stride = 1;
  return p;
}

static void arguments() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double T[12] = {1, 0, 0, 0.5, 0, 1, 0, -2.0, 0, 0, 1, 3.0};
  std::vector<double> poses;  // exactly 3 poses: a read past the last is the sanitizer's to find
  for (int k = 0; k < 3; ++k) poses.insert(poses.end(), T, T + 12);
  std::vector<float> pts = {1, 2, 3, 0, 4, 5, 6, 0};
  std::vector<fmx_refine_system> out(3);
  const char* why = nullptr;
  fmx_align_params p = params();
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_OK && why == nullptr);
  // nothing to read: no points, no poses
  CHECK(fmx::refine_check(nullptr, 0, poses.data(), 3, &p, out.data(), &why) == FMX_OK && why == nullptr);
  CHECK(fmx::refine_check(pts.data(), 2, nullptr, 0, &p, nullptr, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, nullptr, out.data(), &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::refine_check(pts.data(), 2, nullptr, 3, &p, out.data(), &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, nullptr, &why) == FMX_E_INVAL && why);
  CHECK(std::strcmp(why, "null output") == 0);
  why = nullptr;
  CHECK(fmx::refine_check(nullptr, 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::refine_check(pts.data(), 1ull << 32, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL && why);
  CHECK(fmx::refine_check(pts.data(), (1ull << 32) - 1, poses.data(), 3, &p, out.data(), &why) == FMX_OK);
  // the count is refused before a pose is read, and before the params are
  why = nullptr;
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), FMX_REFINE_MAX_POSES + 1ull, &p, out.data(), &why) == FMX_E_INVAL && why);
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), FMX_REFINE_MAX_POSES + 1ull, nullptr, out.data(), &why) == FMX_E_INVAL);
  for (int k = 0; k < 36; ++k)
    for (double bad : {nan, inf, -inf}) {
      std::vector<double> B = poses;
      B[(size_t)k] = bad;
      why = nullptr;
      CHECK(fmx::refine_check(pts.data(), 2, B.data(), 3, &p, out.data(), &why) == FMX_E_INVAL && why);
    }
  // every align_check case
  p = params();
  p.reach = FMX_NEAREST_MAX_REACH;
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_OK);
  p.reach = FMX_NEAREST_MAX_REACH + 1;
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL);
  p = params();
  for (double bad : {nan, -1.0}) {
    p.max_dist2 = bad;
    CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL);
  }
  p = params();
  p.max_dist2 = 0.0;
  CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_OK);
  for (double bad : {nan, inf, 0.0, -0.1}) {
    p = params();
    p.sigma = bad;
    CHECK(fmx::refine_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL);
  }
  // the loop's threshold: align_loop_check's rule
  why = nullptr;
  CHECK(fmx::refine_loop_check(0.0, &why) == FMX_OK && fmx::refine_loop_check(1e-6, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::refine_loop_check(inf, &why) == FMX_OK);
  CHECK(fmx::refine_loop_check(nan, &why) == FMX_E_INVAL && why);
  CHECK(fmx::refine_loop_check(-1e-300, &why) == FMX_E_INVAL);
}

// The plan from its definition, the tile being the build's: kept = ceil(n / max(stride, 1));
// tiles = ceil(kept / tile); chunk = min(16384, (32 MiB / 256 B) / tiles), at least 1; chunks =
// ceil(poses / chunk), 0 when nothing is kept.  Then plans computed by hand.
static void plan() {
  const unsigned long long tile = fmx::kRefineTile;
  CHECK(tile == fmx::refine_plan(1, 1, 1).tile && tile % 256 == 0);
  const unsigned long long ns[] = {0,        1,        2,         63,         64,         65,         tile - 1,        tile,
                                   tile + 1, 2 * tile, 3 * tile + 5, 8 * tile, 8 * tile + 1, 1ull << 24, 1ull << 28, (1ull << 32) - 1};
  const uint32_t strides[] = {0, 1, 3, 64, 0xFFFFFFFFu};
  const uint32_t poses[] = {0, 1, 7, 16384, 16385, 65536};
  for (unsigned long long n : ns)
    for (uint32_t s : strides)
      for (uint32_t k : poses) {
        const fmx::RefinePlan p = fmx::refine_plan(n, s, k);
        const unsigned long long every = s ? s : 1, kept = (n + every - 1) / every, tiles = (kept + tile - 1) / tile;
        unsigned long long chunk = (1ull << 17) / (tiles ? tiles : 1);  // 32 MiB / 256 B
        chunk = chunk > 16384 ? 16384 : chunk < 1 ? 1 : chunk;
        CHECK(p.kept == kept && p.tile == tile && p.tiles == tiles && p.chunk == chunk && p.cap == 2048);
        CHECK(p.chunks == (kept ? (k + chunk - 1) / chunk : 0));
        // what the call allocates and indexes with 32-bit words
        CHECK((unsigned long long)p.chunk * p.tiles <= (1ull << 24));
        CHECK(p.tiles > (1u << 17) || (unsigned long long)p.chunk * p.tiles * sizeof(fmx::RefinePart) <= (32ull << 20));
      }
  // by hand, in tiles: up to 8 tiles a chunk is the full 16384 poses (8 * 16384 records fill 32 MiB)
  CHECK(fmx::refine_plan(8 * tile, 1, 16385).chunk == 16384 && fmx::refine_plan(8 * tile, 1, 16385).chunks == 2);
  CHECK(fmx::refine_plan(8 * tile, 1, 16384).chunks == 1);
  CHECK(fmx::refine_plan(8 * tile + 1, 1, 100).tiles == 9 && fmx::refine_plan(8 * tile + 1, 1, 100).chunk == 14563);  // 131072 / 9
  CHECK(fmx::refine_plan(128 * tile, 1, 1025).chunk == 1024 && fmx::refine_plan(128 * tile, 1, 1025).chunks == 2);
  CHECK(fmx::refine_plan(tile * 64, 64, 10000).kept == tile && fmx::refine_plan(tile * 64, 64, 10000).tiles == 1);
  CHECK(fmx::refine_plan(tile * 64 + 1, 64, 10000).tiles == 2);
  CHECK(fmx::refine_plan((1ull << 18) * tile, 1, 3).chunk == 1 && fmx::refine_plan((1ull << 18) * tile, 1, 3).chunks == 3);
  CHECK(fmx::refine_plan(0, 1, 9).chunks == 0 && fmx::refine_plan(0, 1, 9).chunk == 16384);
}

// ---- the loop.  A brute-force point-to-point system against fixed targets: scan points p_i
// with targets q_i = p_i (a zero-residual problem whose solution is the identity), rows as
// fmx_align_system's, summed in index order.  A pose with a translation past `far` finds nothing.
struct Problem {
  std::vector<double> p;  // 3 per point
  double far = 50.0;
  int calls = 0;
  std::vector<uint32_t> batch_sizes;
};
static void system_of(const Problem& pr, const double T[12], fmx_refine_system* out) {
  std::memset(out, 0, sizeof(*out));
  const size_t n = pr.p.size() / 3;
  if (std::fabs(T[3]) > pr.far) {
    out->none = (uint32_t)n;
    return;
  }
  const double inv = 1.0 / 0.1;
  for (size_t i = 0; i < n; ++i) {
    const double* p = &pr.p[3 * i];
    for (int a = 0; a < 3; ++a) {
      const double R0 = T[4 * a], R1 = T[4 * a + 1], R2 = T[4 * a + 2];
      const double w = ((R0 * p[0] + R1 * p[1]) + R2 * p[2]) + T[4 * a + 3];
      const double r = w - p[a];
      const double v[7] = {(R2 * p[1] - R1 * p[2]) * inv, (R0 * p[2] - R2 * p[0]) * inv, (R1 * p[0] - R0 * p[1]) * inv,
                           R0 * inv,                      R1 * inv,                      R2 * inv,
                           -r * inv};
      for (int r7 = 0; r7 < 7; ++r7)
        for (int q7 = r7; q7 < 7; ++q7) out->S[r7 * 7 - r7 * (r7 - 1) / 2 + (q7 - r7)] += v[r7] * v[q7];
    }
  }
  out->S[28] = 0.5 * out->S[27];
  out->found = (uint32_t)n;
  out->lookups = 27ull * n;
}

// align_loop_as's Result over the refine record's counts
struct Counts {
  uint32_t found, none, out_of_range, invalid, unoriented;
  uint64_t lookups;
};
struct OneResult {
  uint32_t iters;
  int32_t converged;
  double last_step, error;
  Counts counts;
};

static void loop() {
  Problem pr;
  for (int i = 0; i < 40; ++i) {
    const double x = (i % 4) - 1.5 + 0.07 * i, y = ((i / 4) % 4) - 1.3 - 0.03 * i, z = (i / 16) - 0.9 + 0.011 * i * i;
    pr.p.insert(pr.p.end(), {x, y, z});
  }
  const double xi[6] = {0.02, -0.015, 0.025, 0.06, -0.04, 0.05}, half[6] = {0.01, -0.0075, 0.0125, 0.03, -0.02, 0.025};
  const fmxh::Pose eye = fmxh::identity(), near = fmxh::expmap(xi), mid = fmxh::expmap(half);
  fmxh::Pose lost = near;
  lost.m[3] = 1e3;  // nothing found: singular
  // mixed: converging, already converged, singular (in the middle), converging, singular, converging
  const fmxh::Pose list[6] = {near, eye, lost, mid, lost, near};
  std::vector<double> init;
  for (const fmxh::Pose& T : list) init.insert(init.end(), T.m, T.m + 12);
  const uint32_t K = 6;
  const double threshold = 1e-9;
  for (uint32_t max_iters : {0u, 1u, 2u, 30u}) {
    pr.batch_sizes.clear();
    std::vector<double> out((size_t)K * 12, 7.0);
    std::vector<fmx_refine_result> res(K);
    std::memset(res.data(), 0xA5, K * sizeof(fmx_refine_result));
    fmx::refine_loop(
        init.data(), K, max_iters, threshold,
        [&](const double* poses, uint32_t count, fmx_refine_system* rec) {
          pr.batch_sizes.push_back(count);
          for (uint32_t a = 0; a < count; ++a) system_of(pr, poses + (size_t)a * 12, rec + a);
        },
        out.data(), res.data());
    uint32_t most = 0;
    for (uint32_t k = 0; k < K; ++k) {
      // the one-pose loop the library has, on the same per-pose callable
      double alone[12];
      for (double& v : alone) v = 7.0;
      OneResult R{};
      const char* why = nullptr;
      const fmx_status st = fmx::align_loop_as<OneResult>(
          &init[(size_t)k * 12], max_iters, threshold,
          [&](const double* pose, double* S, Counts* c) {
            fmx_refine_system s;
            system_of(pr, pose, &s);
            std::memcpy(S, s.S, sizeof(s.S));
            *c = Counts{s.found, s.none, s.out_of_range, s.invalid, s.unoriented, s.lookups};
          },
          alone, &R, &why);
      const fmx_refine_result& r = res[k];
      CHECK(r.reserved == 0 && r.reserved2 == 0);
      most = r.iters > most ? r.iters : most;
      if (st == FMX_OK) {
        CHECK(!r.singular);
        CHECK(std::memcmp(&out[(size_t)k * 12], alone, sizeof(alone)) == 0);
        CHECK(r.iters == R.iters && r.converged == R.converged);
        CHECK(std::memcmp(&r.last_step, &R.last_step, 8) == 0 && std::memcmp(&r.error, &R.error, 8) == 0);
        CHECK(r.found == R.counts.found && r.none == R.counts.none && r.out_of_range == R.counts.out_of_range &&
              r.invalid == R.counts.invalid && r.unoriented == R.counts.unoriented && r.lookups == R.counts.lookups);
      } else {  // singular: the one-pose loop refuses, the batch reports it and returns the pose as it came
        CHECK(st == FMX_E_STATE && why && alone[0] == 7.0);
        CHECK(r.singular == 1 && r.converged == 0 && r.iters == 1 && r.last_step == 0.0 && r.error == 0.0);
        CHECK(r.found == 0 && r.none == 40);
        CHECK(std::memcmp(&out[(size_t)k * 12], &init[(size_t)k * 12], 12 * sizeof(double)) == 0);
      }
    }
    // what each kind did
    if (max_iters == 0) {
      CHECK(pr.batch_sizes.empty() && std::memcmp(out.data(), init.data(), out.size() * sizeof(double)) == 0);
      for (uint32_t k = 0; k < K; ++k) CHECK(res[k].iters == 0 && !res[k].converged && !res[k].singular && res[k].last_step == 0.0);
      continue;
    }
    CHECK(res[1].iters == 1 && res[1].converged);            // already converged: one evaluation
    CHECK((res[2].singular && res[4].singular) && (res[2].iters == 1 && res[4].iters == 1));
    CHECK(std::memcmp(&res[0], &res[5], sizeof(fmx_refine_result)) == 0);  // the same pose twice: the same record
    CHECK(std::memcmp(&out[0], &out[5 * 12], 12 * sizeof(double)) == 0);
    if (max_iters <= 2) CHECK(res[0].iters == max_iters && !res[0].converged && res[3].iters == max_iters);  // stopped by max_iters
    if (max_iters == 30) {
      CHECK(res[0].converged && res[3].converged && res[0].iters > 2 && res[0].iters < 30);
      for (int e = 0; e < 12; ++e) CHECK(std::fabs(out[(size_t)e] - eye.m[e]) < 1e-9 && std::fabs(out[36 + (size_t)e] - eye.m[e]) < 1e-9);
    }
    // one batch per round, each of the poses still running: all six, then those neither converged nor singular
    CHECK(pr.batch_sizes.size() == most && pr.batch_sizes[0] == K);
    if (max_iters >= 2) CHECK(pr.batch_sizes[1] == 3);
    for (size_t i = 1; i < pr.batch_sizes.size(); ++i) CHECK(pr.batch_sizes[i] <= pr.batch_sizes[i - 1]);
  }
  // a singular pose in the middle of the list changes no other result: the list without the two
  {
    const uint32_t keep[4] = {0, 1, 3, 5};
    std::vector<double> sub;
    for (uint32_t k : keep) sub.insert(sub.end(), &init[(size_t)k * 12], &init[(size_t)k * 12] + 12);
    const auto at = [&](const double* poses, uint32_t count, fmx_refine_system* rec) {
      for (uint32_t a = 0; a < count; ++a) system_of(pr, poses + (size_t)a * 12, rec + a);
    };
    std::vector<double> all((size_t)K * 12), few(4 * 12);
    std::vector<fmx_refine_result> ra(K), rf(4);
    fmx::refine_loop(init.data(), K, 30, threshold, at, all.data(), ra.data());
    fmx::refine_loop(sub.data(), 4, 30, threshold, at, few.data(), rf.data());
    for (uint32_t j = 0; j < 4; ++j) {
      CHECK(std::memcmp(&few[(size_t)j * 12], &all[(size_t)keep[j] * 12], 12 * sizeof(double)) == 0);
      CHECK(std::memcmp(&rf[j], &ra[keep[j]], sizeof(fmx_refine_result)) == 0);
    }
    // results may be NULL; no poses: nothing is read, written or evaluated
    std::vector<double> again((size_t)K * 12);
    fmx::refine_loop(init.data(), K, 30, threshold, at, again.data(), nullptr);
    CHECK(std::memcmp(again.data(), all.data(), all.size() * sizeof(double)) == 0);
    int called = 0;
    fmx::refine_loop(nullptr, 0, 30, threshold, [&](const double*, uint32_t, fmx_refine_system*) { ++called; }, nullptr, nullptr);
    CHECK(called == 0);
  }
}

int main() {
  arguments();
  plan();
  loop();
  std::printf("refine host ok\n");
  return 0;
}
