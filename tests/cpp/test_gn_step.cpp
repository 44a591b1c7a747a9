// gn_step (form_amd/csrc/align_host.hpp), the one Gauss-Newton step under align_loop_as and
// refine_loop (refine_host.hpp), called directly: on a well-conditioned system, field by field
// what one iteration of each of the two loops gives from the same system; on a singular one,
// false with nothing touched, where the two loops then differ as they always did (FMX_E_STATE
// with nothing written, against singular = 1 with the pose put back).
// Built by __graft_entry__.build() (tests/cpp/gn_step.mk) with the address and
// undefined-behaviour sanitizers linked in statically; tests/test_gn_step_cpu.py runs it.
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

// A brute-force point-to-point system against fixed targets (tests/cpp/test_refine_host.cpp's):
// scan points p_i with targets q_i = p_i, rows as fmx_align_system's, summed in index order.  A
// pose with a translation past 50 finds nothing: an all-zero, singular system.
static std::vector<double> points40() {
  std::vector<double> p;
  for (int i = 0; i < 40; ++i) {
    const double x = (i % 4) - 1.5 + 0.07 * i, y = ((i / 4) % 4) - 1.3 - 0.03 * i, z = (i / 16) - 0.9 + 0.011 * i * i;
    p.insert(p.end(), {x, y, z});
  }
  return p;
}
static void system_of(const std::vector<double>& pts, const double T[12], fmx_refine_system* out) {
  std::memset(out, 0, sizeof(*out));
  const size_t n = pts.size() / 3;
  if (std::fabs(T[3]) > 50.0) {
    out->none = (uint32_t)n;
    return;
  }
  const double inv = 1.0 / 0.1;
  for (size_t i = 0; i < n; ++i) {
    const double* p = &pts[3 * i];
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main() {
  const std::vector<double> pts = points40();
  const double xi[6] = {0.02, -0.015, 0.025, 0.06, -0.04, 0.05};
  const fmxh::Pose near = fmxh::expmap(xi);
  fmxh::Pose lost = near;
  lost.m[3] = 1e3;
  const auto batch = [&](const double* poses, uint32_t count, fmx_refine_system* rec) {
    for (uint32_t a = 0; a < count; ++a) system_of(pts, poses + (size_t)a * 12, rec + a);
  };
  const auto single = [&](const double* pose, double* S, fmx_align_counts* c) {
    fmx_refine_system s;
    system_of(pts, pose, &s);
    std::memcpy(S, s.S, sizeof(s.S));
    *c = fmx_align_counts{};
    c->found = s.found, c->none = s.none;
  };
  // well-conditioned: below the threshold and above it
  for (double threshold : {1e-9, std::numeric_limits<double>::infinity()}) {
    fmx_refine_system s;
    system_of(pts, near.m, &s);
    fmxh::Pose T = near;
    double last_step = -1.0;
    int32_t converged = -1;
    CHECK(fmx::gn_step(s.S, T, threshold, &last_step, &converged));
    CHECK(last_step > 1e-3 && converged == (threshold > 1.0 ? 1 : 0) && std::memcmp(T.m, near.m, sizeof(T.m)) != 0);
    double many[12], alone[12];
    fmx_refine_result r{};
    fmx::refine_loop(near.m, 1, 1, threshold, batch, many, &r);
    CHECK(std::memcmp(T.m, many, sizeof(many)) == 0);
    CHECK(r.iters == 1 && !r.singular && r.converged == converged && same_bits(r.last_step, last_step));
    CHECK(same_bits(r.error, s.S[28]) && r.found == 40);
    fmx_align_result R{};
    const char* why = nullptr;
    CHECK(fmx::align_loop(near.m, 1, threshold, single, alone, &R, &why) == FMX_OK && why == nullptr);
    CHECK(std::memcmp(T.m, alone, sizeof(alone)) == 0);
    CHECK(R.iters == 1 && R.converged == converged && same_bits(R.last_step, last_step));
    CHECK(same_bits(R.error, s.S[28]) && R.counts.found == 40);
  }
  // singular
  {
    fmx_refine_system s;
    system_of(pts, lost.m, &s);
    fmxh::Pose T = lost;
    double last_step = -1.0;
    int32_t converged = -1;
    CHECK(!fmx::gn_step(s.S, T, 1e-9, &last_step, &converged));
    CHECK(std::memcmp(T.m, lost.m, sizeof(T.m)) == 0 && last_step == -1.0 && converged == -1);
    double many[12], alone[12];
    for (double& v : alone) v = 7.0;
    fmx_refine_result r{};
    fmx::refine_loop(lost.m, 1, 30, 1e-9, batch, many, &r);
    CHECK(r.singular == 1 && r.converged == 0 && r.iters == 1 && r.last_step == 0.0 && r.none == 40);
    CHECK(std::memcmp(many, lost.m, sizeof(many)) == 0);
    fmx_align_result R{};
    R.iters = 42;
    const char* why = nullptr;
    CHECK(fmx::align_loop(lost.m, 30, 1e-9, single, alone, &R, &why) == FMX_E_STATE && why);
    CHECK(alone[0] == 7.0 && R.iters == 42);
  }
  std::printf("gn step ok\n");
  return 0;
}
