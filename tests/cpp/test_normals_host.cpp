// The host-only parts of the dense map's surface normals and of the point-to-plane alignment
// (form_amd/csrc/normals_host.hpp, no HIP headers): the argument checks of fmx_normals_build,
// the support threshold, what a download takes, the plane system's counts, and the
// Gauss-Newton loop with fmx_plane_result driven by a CPU brute-force point-to-plane system on
// three exact planes.  Built by __graft_entry__.build() (tests/cpp/normals_host.mk) with the
// address and undefined-behaviour sanitizers linked in statically; tests/test_normals_cpu.py
// runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "normals_host.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static fmx_normals_params params() {
  fmx_normals_params p{};
  p.min_hits = 1;
  p.reach = 1;
  p.max_dist2 = std::numeric_limits<double>::infinity();
  p.min_support = 5;
  p.max_flatness = 0.1;
  return p;
}

static void arguments() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const char* why = nullptr;
  fmx_normals_params p = params();
  CHECK(fmx::normals_check(&p, &why) == FMX_OK && why == nullptr);
  CHECK(fmx::normals_check(nullptr, &why) == FMX_E_INVAL && why);
  for (uint32_t bad : {0u, (uint32_t)FMX_NEAREST_MAX_REACH + 1u, 0xFFFFFFFFu}) {
    p = params();
    p.reach = bad;
    why = nullptr;
    CHECK(fmx::normals_check(&p, &why) == FMX_E_INVAL && why);
  }
  p = params();
  p.reach = FMX_NEAREST_MAX_REACH;
  CHECK(fmx::normals_check(&p, &why) == FMX_OK);
  for (double bad : {nan, -1.0, -inf}) {
    p = params();
    p.max_dist2 = bad;
    why = nullptr;
    CHECK(fmx::normals_check(&p, &why) == FMX_E_INVAL && why);
  }
  p = params();
  p.max_dist2 = 0.0;
  CHECK(fmx::normals_check(&p, &why) == FMX_OK);
  for (double bad : {nan, -1e-300, 1.0000000000000002, inf, -inf}) {
    p = params();
    p.max_flatness = bad;
    why = nullptr;
    CHECK(fmx::normals_check(&p, &why) == FMX_E_INVAL && why);
  }
  for (double good : {0.0, 1.0, 0.05}) {
    p = params();
    p.max_flatness = good;
    CHECK(fmx::normals_check(&p, &why) == FMX_OK);
  }
  // the support threshold
  for (uint32_t s = 0; s < 6; ++s) {
    p.min_support = s;
    CHECK(fmx::normals_min_support(p) == (s < 3 ? 3u : s));
  }
  p.min_support = 0xFFFFFFFFu;
  CHECK(fmx::normals_min_support(p) == 0xFFFFFFFFu);
  // a download's size, the plane system's counts
  const fmx_normals_counts k{363, 66, 19, 5, 12096};
  CHECK(fmx::normals_take(k, true) == 363 && fmx::normals_take(k, false) == 448);
  const fmx_normals_counts big{0xFFFFFFFFu, 0xFFFFFFFFu, 1, 0, 0};
  CHECK(fmx::normals_take(big, false) == 2ull * 0xFFFFFFFFull + 1ull);
  const unsigned long long raw[6] = {10, 20, 3, 4, 999, 5};
  const fmx_plane_counts c = fmx::plane_counts(raw, 100, 2);
  CHECK(c.found == 10 && c.none == 20 && c.out_of_range == 3 && c.invalid == 4 && c.unoriented == 5 && c.lookups == 999);
  CHECK(c.skipped == 50);
  CHECK(fmx::plane_counts(raw, 0, 1).skipped == 0 && fmx::plane_counts(raw, 7, 0xFFFFFFFFu).skipped == 6);
}

// The definition by brute force: every scan point at the pose against its nearest map point and
// that point's normal; a map point without a normal (all zeros) makes the point unoriented.
struct Brute {
  std::vector<double> map, normal, scan;  // xyz triples
  double sigma;
  int calls = 0;
  void operator()(const double* T, double* S, fmx_plane_counts* cnt) {
    ++calls;
    for (int k = 0; k < 29; ++k) S[k] = 0.0;
    *cnt = fmx_plane_counts{};
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
      const double* n = &normal[best];
      if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) {
        ++cnt->unoriented;
        continue;
      }
      ++cnt->found;
      const double r = (n[0] * (w[0] - map[best]) + n[1] * (w[1] - map[best + 1])) + n[2] * (w[2] - map[best + 2]);
      double m[3];
      for (int a = 0; a < 3; ++a) m[a] = (T[a] * n[0] + T[4 + a] * n[1]) + T[8 + a] * n[2];
      const double v[7] = {(m[2] * p[1] - m[1] * p[2]) * inv, (m[0] * p[2] - m[2] * p[0]) * inv, (m[1] * p[0] - m[0] * p[1]) * inv,
                           m[0] * inv, m[1] * inv, m[2] * inv, -r * inv};
      int o = 0;
      for (int rr = 0; rr < 7; ++rr)
        for (int q = rr; q < 7; ++q) S[o++] += v[rr] * v[q];
    }
    S[28] = 0.5 * S[27];
  }
};

// planes: how many of the three axis planes x = 0, y = 0, z = 0 carry a 5 x 5 grid of points
// (the scan is the map: a zero-residual problem at the identity); every fourth point of the
// first plane has no normal
static Brute problem(int planes) {
  Brute b;
  b.sigma = 0.1;
  for (int a = 0; a < planes; ++a)
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j) {
        double p[3], n[3] = {0.0, 0.0, 0.0};
        p[a] = 0.0;
        p[(a + 1) % 3] = 1.0 + 0.5 * i + 0.01 * j;
        p[(a + 2) % 3] = 1.0 + 0.5 * j - 0.02 * i;
        if (!(a == 0 && (5 * i + j) % 4 == 0)) n[a] = (i + j) % 2 ? -1.0 : 1.0;  // either sign: the system does not care
        for (int k = 0; k < 3; ++k) b.map.push_back(p[k]), b.normal.push_back(n[k]);
      }
  b.scan = b.map;
  return b;
}

static void loop() {
  Brute b = problem(3);
  const double xi[6] = {0.004, -0.003, 0.005, 0.03, -0.02, 0.025};
  const fmxh::Pose T0 = fmxh::expmap(xi);
  const char* why = nullptr;
  double out[12];
  fmx_plane_result res{};
  CHECK(fmx::align_loop_as<fmx_plane_result>(T0.m, 30, 1e-9, b, out, &res, &why) == FMX_OK && why == nullptr);
  const fmxh::Pose I = fmxh::identity();
  for (int k = 0; k < 12; ++k) CHECK(std::fabs(out[k] - I.m[k]) < 1e-9);
  CHECK(res.converged == 1 && res.iters >= 2 && res.iters < 30 && res.last_step < 1e-9 && res.last_step >= 0.0);
  CHECK(res.counts.found == 75 - 7 && res.counts.unoriented == 7 && res.counts.none == 0 && (int)res.iters == b.calls);
  CHECK(res.error < 1e-12);
  // max_iters cuts it short; max_iters == 0: the initial pose, nothing evaluated; a NULL result is allowed
  double one[12];
  fmx_plane_result r1{};
  CHECK(fmx::align_loop_as<fmx_plane_result>(T0.m, 1, 1e-9, b, one, &r1, &why) == FMX_OK);
  CHECK(r1.iters == 1 && r1.converged == 0 && r1.last_step > 1e-3 && r1.error > 0.0);
  const int before = b.calls;
  fmx_plane_result r0{};
  r0.iters = 99;
  CHECK(fmx::align_loop_as<fmx_plane_result>(T0.m, 0, 1e-9, b, one, &r0, &why) == FMX_OK && b.calls == before);
  CHECK(std::memcmp(one, T0.m, sizeof(one)) == 0 && r0.iters == 0 && r0.counts.unoriented == 0);
  CHECK(fmx::align_loop_as<fmx_plane_result>(T0.m, 2, 1e-9, b, one, (fmx_plane_result*)nullptr, &why) == FMX_OK);
  // singular: one plane fixes no pose (at the identity m = n = e_x: columns 0, 4 and 5 of every
  // row are exactly zero); pose_out and the result stay as they were
  Brute flat = problem(1);
  double keep[12];
  for (int k = 0; k < 12; ++k) keep[k] = 7.0 + k;
  fmx_plane_result rk{};
  rk.iters = 42;
  why = nullptr;
  CHECK(fmx::align_loop_as<fmx_plane_result>(I.m, 30, 1e-9, flat, keep, &rk, &why) == FMX_E_STATE && why && flat.calls == 1);
  for (int k = 0; k < 12; ++k) CHECK(keep[k] == 7.0 + k);
  CHECK(rk.iters == 42);
}

int main() {
  arguments();
  loop();
  std::printf("normals host ok\n");
  return 0;
}
