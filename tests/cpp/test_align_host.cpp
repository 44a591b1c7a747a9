// The host-only parts of aligning a scan to the dense map (form_amd/csrc/align_host.hpp, no HIP
// headers): the argument checks of fmx_align_system and fmx_align_dense, the packed system
// taken apart, and the Gauss-Newton loop driven by a CPU brute-force system over a few dozen
// points.  Built by __graft_entry__.build() (tests/cpp/align_host.mk) with the address and
// undefined-behaviour sanitizers linked in statically; tests/test_align_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "align_host.hpp"

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
  double T[12] = {1, 0, 0, 0.5, 0, 1, 0, -2.0, 0, 0, 1, 3.0};
  float pts[8] = {1, 2, 3, 0, 4, 5, 6, 0};
  const char* why = nullptr;
  fmx_align_params p = params();
  CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::align_check(nullptr, 0, T, &p, &why) == FMX_OK && why == nullptr);  // no points: nothing to read
  CHECK(fmx::align_check(pts, 2, T, nullptr, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::align_check(pts, 2, nullptr, &p, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::align_check(nullptr, 2, T, &p, &why) == FMX_E_INVAL && why);
  why = nullptr;
  CHECK(fmx::align_check(pts, 1ull << 32, T, &p, &why) == FMX_E_INVAL && why);
  CHECK(fmx::align_check(pts, (1ull << 32) - 1, T, &p, &why) == FMX_OK);
  for (int k = 0; k < 12; ++k)
    for (double bad : {nan, inf, -inf}) {
      double B[12];
      std::memcpy(B, T, sizeof(B));
      B[k] = bad;
      why = nullptr;
      CHECK(fmx::align_check(pts, 2, B, &p, &why) == FMX_E_INVAL && why);
    }
  p = params();
  p.reach = FMX_NEAREST_MAX_REACH;
  CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_OK);
  p.reach = FMX_NEAREST_MAX_REACH + 1;
  why = nullptr;
  CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_E_INVAL && why);
  for (double bad : {nan, -1.0, -inf}) {
    p = params();
    p.max_dist2 = bad;
    why = nullptr;
    CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_E_INVAL && why);
  }
  p = params();
  p.max_dist2 = 0.0;
  CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_OK);
  for (double bad : {nan, 0.0, -0.0, -1.0, inf, -inf}) {
    p = params();
    p.sigma = bad;
    why = nullptr;
    CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_E_INVAL && why);
  }
  p = params();
  p.sigma = std::numeric_limits<double>::denorm_min();
  CHECK(fmx::align_check(pts, 2, T, &p, &why) == FMX_OK);
  // the loop's own
  double out[12];
  why = nullptr;
  CHECK(fmx::align_loop_check(nullptr, 1e-6, &why) == FMX_E_INVAL && why);
  for (double bad : {nan, -1e-300, -inf}) {
    why = nullptr;
    CHECK(fmx::align_loop_check(out, bad, &why) == FMX_E_INVAL && why);
  }
  CHECK(fmx::align_loop_check(out, 0.0, &why) == FMX_OK && fmx::align_loop_check(out, inf, &why) == FMX_OK);
  // the stride
  p = params();
  p.stride = 0;
  CHECK(fmx::align_stride(p) == 1);
  p.stride = 7;
  CHECK(fmx::align_stride(p) == 7);
  CHECK(fmx::align_kept(0, 3) == 0 && fmx::align_kept(1, 3) == 1 && fmx::align_kept(3, 3) == 1 && fmx::align_kept(4, 3) == 2);
  CHECK(fmx::align_kept((1ull << 32) - 1, 1) == (1ull << 32) - 1 && fmx::align_kept(5, 0xFFFFFFFFu) == 1);
}

static void unpack() {
  double S[29], H[6][6], g[6];
  for (int k = 0; k < 29; ++k) S[k] = 100.0 + k;
  fmx::align_unpack(S, H, g);
  int o = 0;
  for (int r = 0; r < 7; ++r)
    for (int q = r; q < 7; ++q, ++o) {
      if (q < 6) CHECK(H[r][q] == 100.0 + o && H[q][r] == 100.0 + o);
      else if (r < 6) CHECK(g[r] == 100.0 + o);
    }
  CHECK(o == 28);
}

// The definition by brute force: every scan point at the pose against its nearest map point.
struct Brute {
  std::vector<double> map, scan;  // xyz triples
  double sigma;
  int calls = 0;
  void operator()(const double* T, double* S, fmx_align_counts* cnt) {
    ++calls;
    for (int k = 0; k < 29; ++k) S[k] = 0.0;
    *cnt = fmx_align_counts{};
    const double inv = 1.0 / sigma;
    for (size_t i = 0; i < scan.size(); i += 3) {
      const double* p = &scan[i];
      double w[3];
      for (int a = 0; a < 3; ++a) w[a] = ((T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2]) + T[4 * a + 3];
      size_t best = 0;
      double bd = std::numeric_limits<double>::infinity();
      for (size_t j = 0; j < map.size(); j += 3) {
        const double e0 = map[j] - w[0], e1 = map[j + 1] - w[1], e2 = map[j + 2] - w[2];
        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
        if (d2 < bd) bd = d2, best = j;
      }
      if (map.empty()) {
        ++cnt->none;
        continue;
      }
      ++cnt->found;
      for (int a = 0; a < 3; ++a) {
        const double R0 = T[4 * a], R1 = T[4 * a + 1], R2 = T[4 * a + 2];
        const double v[7] = {(R2 * p[1] - R1 * p[2]) * inv, (R0 * p[2] - R2 * p[0]) * inv, (R1 * p[0] - R0 * p[1]) * inv,
                             R0 * inv, R1 * inv, R2 * inv, -(w[a] - map[best + a]) * inv};
        int o = 0;
        for (int r = 0; r < 7; ++r)
          for (int q = r; q < 7; ++q) S[o++] += v[r] * v[q];
      }
    }
    S[28] = 0.5 * S[27];
  }
};

static Brute problem(int n) {
  Brute b;
  b.sigma = 0.1;
  unsigned long long s = 12345;
  const auto next = [&] {  // a 48-bit LCG in [-4, 4)
    s = (s * 0x5DEECE66Dull + 0xBull) & ((1ull << 48) - 1);
    return (double)(s >> 16) / (double)(1ull << 32) * 8.0 - 4.0;
  };
  for (int i = 0; i < 3 * n; ++i) b.map.push_back(next());
  b.scan = b.map;  // at the identity the scan is the map: a zero-residual problem
  return b;
}

static void loop() {
  Brute b = problem(48);
  const double xi[6] = {0.01, -0.015, 0.02, 0.03, -0.02, 0.025};
  const fmxh::Pose T0 = fmxh::expmap(xi);
  const char* why = nullptr;
  double out[12];
  fmx_align_result res{};
  CHECK(fmx::align_loop(T0.m, 30, 1e-9, b, out, &res, &why) == FMX_OK && why == nullptr);
  const fmxh::Pose I = fmxh::identity();
  for (int k = 0; k < 12; ++k) CHECK(std::fabs(out[k] - I.m[k]) < 1e-9);
  CHECK(res.converged == 1 && res.iters >= 2 && res.iters < 30 && res.last_step < 1e-9 && res.last_step >= 0.0);
  CHECK(res.counts.found == 48 && res.counts.none == 0 && res.error >= 0.0 && res.error < 1e-12);
  // max_iters cuts it short: not converged, one step taken
  double one[12];
  fmx_align_result r1{};
  CHECK(fmx::align_loop(T0.m, 1, 1e-9, b, one, &r1, &why) == FMX_OK);
  CHECK(r1.iters == 1 && r1.converged == 0 && r1.last_step > 1e-3 && r1.error > 0.0);
  // a threshold of +inf stops after the first step, converged
  fmx_align_result r2{};
  double two[12];
  CHECK(fmx::align_loop(T0.m, 30, std::numeric_limits<double>::infinity(), b, two, &r2, &why) == FMX_OK);
  CHECK(r2.iters == 1 && r2.converged == 1 && std::memcmp(one, two, sizeof(one)) == 0);
  // threshold 0 never converges: all the iterations
  fmx_align_result r3{};
  CHECK(fmx::align_loop(T0.m, 5, 0.0, b, two, &r3, &why) == FMX_OK && r3.iters == 5 && r3.converged == 0);
  // max_iters == 0: the initial pose, nothing evaluated; a NULL result is allowed
  const int before = b.calls;
  double same[12];
  fmx_align_result r0{};
  r0.iters = 99;
  CHECK(fmx::align_loop(T0.m, 0, 1e-9, b, same, &r0, &why) == FMX_OK && b.calls == before);
  CHECK(std::memcmp(same, T0.m, sizeof(same)) == 0 && r0.iters == 0 && r0.converged == 0 && r0.last_step == 0.0 &&
        r0.error == 0.0 && r0.counts.found == 0);
  CHECK(fmx::align_loop(T0.m, 2, 1e-9, b, same, nullptr, &why) == FMX_OK);
  // singular: one point fixes no pose (at the identity, (1, 0, 0) leaves H[0][0] = 0 exactly);
  // pose_out and the result stay as they were
  Brute few = problem(0);
  few.map = few.scan = {1.0, 0.0, 0.0};
  double keep[12];
  for (int k = 0; k < 12; ++k) keep[k] = 7.0 + k;
  fmx_align_result rk{};
  rk.iters = 42;
  why = nullptr;
  CHECK(fmx::align_loop(I.m, 30, 1e-9, few, keep, &rk, &why) == FMX_E_STATE && why && few.calls == 1);
  for (int k = 0; k < 12; ++k) CHECK(keep[k] == 7.0 + k);
  CHECK(rk.iters == 42);
  Brute none = problem(0);
  CHECK(fmx::align_loop(T0.m, 30, 1e-9, none, keep, &rk, &why) == FMX_E_STATE && keep[0] == 7.0);
}

int main() {
  arguments();
  unpack();
  loop();
  std::printf("align host ok\n");
  return 0;
}
