// The host-only parts of scoring candidate poses against the dense map
// (form_amd/csrc/score_host.hpp, no HIP headers): the argument checks of fmx_score_poses, the
// plan fmx_score_plan reports, held against its definition restated here, and the ranking rule.
// Built by __graft_entry__.build() (tests/cpp/score_host.mk) with the address and
// undefined-behaviour sanitizers linked in statically; tests/test_score_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "score_host.hpp"

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
  std::vector<fmx_pose_score> out(3);
  const char* why = nullptr;
  fmx_align_params p = params();
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_OK && why == nullptr);
  // nothing to read: no points, no poses
  CHECK(fmx::score_check(nullptr, 0, poses.data(), 3, &p, out.data(), &why) == FMX_OK && why == nullptr);
  CHECK(fmx::score_check(pts.data(), 2, nullptr, 0, &p, nullptr, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, nullptr, out.data(), &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::score_check(pts.data(), 2, nullptr, 3, &p, out.data(), &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, nullptr, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::score_check(nullptr, 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::score_check(pts.data(), 1ull << 32, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL && why);
  CHECK(fmx::score_check(pts.data(), (1ull << 32) - 1, poses.data(), 3, &p, out.data(), &why) == FMX_OK);
  // the count is refused before a pose is read
  why = nullptr;
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), FMX_SCORE_MAX_POSES + 1ull, &p, out.data(), &why) == FMX_E_INVAL && why);
  for (int k = 0; k < 36; ++k)
    for (double bad : {nan, inf, -inf}) {
      std::vector<double> B = poses;
      B[(size_t)k] = bad;
      why = nullptr;
      CHECK(fmx::score_check(pts.data(), 2, B.data(), 3, &p, out.data(), &why) == FMX_E_INVAL && why);
    }
  p = params();
  p.reach = FMX_NEAREST_MAX_REACH;
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_OK);
  p.reach = FMX_NEAREST_MAX_REACH + 1;
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL);
  p = params();
  for (double bad : {nan, -1.0}) {
    p.max_dist2 = bad;
    CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL);
  }
  p = params();
  p.max_dist2 = 0.0;
  CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_OK);
  for (double bad : {nan, inf, 0.0, -0.1}) {  // sigma enters nothing and is validated all the same
    p = params();
    p.sigma = bad;
    CHECK(fmx::score_check(pts.data(), 2, poses.data(), 3, &p, out.data(), &why) == FMX_E_INVAL);
  }
}

// The plan from its definition: kept = ceil(n / max(stride, 1)); tiles = ceil(kept / tile);
// chunk = min(16384, (32 MiB / 32 B) / tiles), at least 1; chunks = ceil(poses / chunk), 0
// when nothing is kept.
static void plan() {
  const unsigned long long ns[] = {0,   1,   2,    63,   64,        65,         255,        256,        257,
                                   511, 512, 1000, 4096, 262144ull, 1ull << 24, 1ull << 28, (1ull << 32) - 1};
  const uint32_t strides[] = {0, 1, 3, 64, 0xFFFFFFFFu};
  const uint32_t poses[] = {0, 1, 7, 16384, 16385, 65536};
  for (unsigned long long n : ns)
    for (uint32_t s : strides)
      for (uint32_t k : poses) {
        const fmx::ScorePlan p = fmx::score_plan(n, s, k);
        const unsigned long long every = s ? s : 1, kept = (n + every - 1) / every, tiles = (kept + 255) / 256;
        unsigned long long chunk = (1ull << 20) / (tiles ? tiles : 1);
        chunk = chunk > 16384 ? 16384 : chunk < 1 ? 1 : chunk;
        CHECK(p.kept == kept && p.tile == 256 && p.tiles == tiles && p.chunk == chunk && p.cap == 2048);
        CHECK(p.chunks == (kept ? (k + chunk - 1) / chunk : 0));
        // what the call allocates and indexes with 32-bit words
        CHECK((unsigned long long)p.chunk * p.tiles <= (1ull << 24));
        CHECK(p.tiles > (1u << 20) || (unsigned long long)p.chunk * p.tiles * sizeof(fmx_pose_score) <= (32ull << 20));
      }
  CHECK(fmx::score_plan(4096 * 64, 64, 10000).chunk == 16384);
  CHECK(fmx::score_plan(1ull << 24, 1, 100).chunk == 16);  // 65536 tiles: 16 poses fill 32 MiB
  CHECK(fmx::score_plan(1ull << 24, 1, 100).chunks == 7);
}

static void ranking() {
  std::vector<fmx_pose_score> s(6);
  const uint32_t found[6] = {3, 5, 5, 5, 0, 5};
  const double d2[6] = {0.5, 2.0, 1.0, 1.0, 0.0, 0.25};
  for (int i = 0; i < 6; ++i) {
    s[(size_t)i] = fmx_pose_score{};
    s[(size_t)i].found = found[i];
    s[(size_t)i].sum_d2 = d2[i];
  }
  std::vector<uint32_t> order(6);
  fmx::score_rank(s.data(), 6, order.data());
  const uint32_t want[6] = {5, 2, 3, 1, 0, 4};  // found first, then sum_d2, the tie 2 / 3 by index
  CHECK(std::memcmp(order.data(), want, sizeof(want)) == 0);
  for (uint32_t a = 0; a < 6; ++a) {
    CHECK(!fmx::score_before(s.data(), a, a));
    for (uint32_t b = 0; b < 6; ++b)
      if (a != b) CHECK(fmx::score_before(s.data(), a, b) != fmx::score_before(s.data(), b, a));  // a total order
  }
  fmx::score_rank(s.data(), 0, order.data());  // nothing to rank: nothing touched
  CHECK(order[0] == 5);
}

int main() {
  arguments();
  plan();
  ranking();
  std::printf("score host ok\n");
  return 0;
}
