// test_extract_plan.cpp — the host-side kernel choice of one extraction
// (form_amd/csrc/extract_plan.hpp), on the CPU with plain g++:
//   1. the project's own geometries keep the plan they have always had (the benchmark
//      and the default tests cannot move);
//   2. every row of the case table (tests/extract_cases.py) lands on the plan it names;
//   3. over every shape the API accepts, a sector-parallel plan never meets a sector
//      with more possible candidates than the register sort holds, its LDS lists fit,
//      and no plan asks for more dynamic LDS than the kernels were granted.
// `test_extract_plan R C k S P` prints one plan instead (the pytest compares the Python
// table with it).
#include <cstdio>
#include <cstdlib>

#include "extract_plan.hpp"

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      if (++g_fail <= 20) std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                                  \
  } while (0)

struct Row {
  const char* id;
  int R, C, k, S, P;
  bool par, fused;
};

static void check_row(const Row& r) {
  const fmx::ExtractPlan p = fmx::extract_plan(r.R, r.C, r.k, r.S, r.P);
  if (p.sector_parallel != r.par || p.fused_normals != r.fused || p.kc5 != (r.k == 5)) {
    std::fprintf(stderr, "FAIL %s (%dx%d k=%d S=%d P=%d): plan par=%d fused=%d kc5=%d, expected par=%d fused=%d\n", r.id,
                 r.R, r.C, r.k, r.S, r.P, (int)p.sector_parallel, (int)p.fused_normals, (int)p.kc5, (int)r.par,
                 (int)r.fused);
    ++g_fail;
  }
}

// The columns of sector s that can be planar-valid, counted one by one (independent of
// the header's closed form): sector s is [s * pps, (s + 1) * pps), the last one runs to
// C, and a column is valid only inside [k, C - k).
static int valid_columns(int C, int k, int S, int s) {
  const int pps = C / S;
  const int b = s * pps, e = s == S - 1 ? C : (s + 1) * pps;
  int n = 0;
  for (int c = b; c < e; ++c) n += c >= k && c < C - k;
  return n;
}

int main(int argc, char** argv) {
  if (argc == 6) {
    const int R = std::atoi(argv[1]), C = std::atoi(argv[2]), k = std::atoi(argv[3]), S = std::atoi(argv[4]),
              P = std::atoi(argv[5]);
    const fmx::ExtractPlan p = fmx::extract_plan(R, C, k, S, P);
    std::printf("%d %d %d %zu %zu\n", (int)p.sector_parallel, (int)p.kc5, (int)p.fused_normals, p.lds_rows,
                p.lds_normals);
    return 0;
  }
  constexpr bool PAR = true, SEQ = false, FUSED = true, SPLIT = false;

  // 1. the project's geometries (form_amd/synth.py GEOMETRIES), S = 6, P = 50.  "tiny" is
  // sequential: its two kept lists, 2 * 6 * 51 ints, do not fit beside the sorted columns
  // in the 16 * 256 bytes of a staged line.
  const Row geo[] = {{"tiny", 16, 256, 0, 6, 50, SEQ, FUSED},  {"small", 32, 512, 0, 6, 50, PAR, FUSED},
                     {"c2", 64, 1024, 0, 6, 50, PAR, FUSED},   {"c3", 64, 2048, 0, 6, 50, PAR, FUSED},
                     {"c4", 128, 2048, 0, 6, 50, PAR, FUSED},  {"wide", 8, 4096, 0, 6, 50, SEQ, SPLIT}};
  for (Row r : geo)
    for (int k = 3; k <= 5; ++k) {
      r.k = k;
      check_row(r);
    }

  // 2. the case table (tests/extract_cases.py, same order)
  const Row table[] = {
      {"A-1800", 4, 1800, 5, 6, 50, PAR, FUSED},
      {"A-200-S16", 4, 200, 5, 16, 5, PAR, FUSED},
      {"B-2560-k5", 4, 2560, 5, 6, 50, PAR, SPLIT},
      {"B-2560-k3", 4, 2560, 3, 6, 50, PAR, SPLIT},
      {"B-2048-S16-P100", 4, 2048, 3, 16, 100, PAR, SPLIT},
      {"B-1800-k2-P100", 4, 1800, 2, 6, 100, PAR, SPLIT},
      {"C-2048-S3", 4, 2048, 5, 3, 50, SEQ, FUSED},
      {"C-1024-S17", 4, 1024, 4, 17, 20, SEQ, FUSED},
      {"C-100-S16", 4, 100, 5, 16, 5, SEQ, FUSED},
      {"C-512-S8-P70", 4, 512, 5, 8, 70, SEQ, FUSED},
      {"C-1000-S1-k8", 4, 1000, 8, 1, 64, SEQ, FUSED},
      {"D-3590-S7-P120", 3, 3590, 5, 7, 120, SEQ, SPLIT},
      {"D-3077-k2", 3, 3077, 2, 6, 200, SEQ, SPLIT},
      {"D-3077-k4", 3, 3077, 4, 6, 100, SEQ, SPLIT},
      {"D-3077-k5-boundary", 3, 3077, 5, 6, 50, PAR, SPLIT},
      {"E-1x256", 1, 256, 5, 6, 50, SEQ, FUSED},
      {"E-1x2560", 1, 2560, 5, 6, 50, PAR, SPLIT},
      {"E-2x256-nopt", 2, 256, 5, 6, 50, SEQ, FUSED},
      {"E-1000-k1-P63", 4, 1000, 1, 7, 63, PAR, FUSED},
      {"F-512", 4, 512, 5, 6, 50, PAR, FUSED},
  };
  for (const Row& r : table) check_row(r);
  // each clause that refuses the sector-parallel kernel is the only one failing in its
  // group-C row (so the row tests that clause and not another)
  {
    auto clauses = [](int C, int k, int S, int P, bool out[5]) {
      const int pps = C / S;
      out[0] = pps <= 512;
      out[1] = S <= 16;
      out[2] = pps >= 2 * k;
      out[3] = S * (P + 1) + (C + 63) / 64 + 1 <= C;
      out[4] = pps + C % S - k - (S == 1 ? k : 0) <= 512;
    };
    bool c[5];
    clauses(2048, 5, 3, 50, c);
    CHECK(!c[0] && c[1] && c[2] && c[3]);
    clauses(1024, 4, 17, 20, c);
    CHECK(c[0] && !c[1] && c[2] && c[3] && c[4]);
    clauses(100, 5, 16, 5, c);
    CHECK(c[0] && c[1] && !c[2] && c[3] && c[4]);
    clauses(512, 5, 8, 70, c);
    CHECK(c[0] && c[1] && c[2] && !c[3] && c[4]);
    clauses(3590, 5, 7, 120, c);
    CHECK(c[0] && c[1] && c[2] && c[3] && !c[4]);
    clauses(3077, 4, 6, 100, c);
    CHECK(c[0] && c[1] && c[2] && c[3] && !c[4]);
    clauses(3077, 5, 6, 50, c);
    CHECK(c[0] && c[1] && c[2] && c[3] && c[4]);
  }

  // 3. the sweep
  long n_par = 0, n_seq = 0, n_fused = 0, n_edge = 0;
  const int Ps[] = {0, 50, 120, 200};
  for (int C = 12; C <= 4096; ++C)
    for (int S = 1; S <= 32 && S <= C; ++S) {
      for (int k = 1; k <= 8; ++k) {
        if (C < 2 * k + 2) continue;
        int longest = 0;
        for (int s = 0; s < S; ++s) {
          const int n = valid_columns(C, k, S, s);
          if (n > longest) longest = n;
        }
        CHECK(longest == fmx::extract_longest_sector(C, k, S));
        for (int P : Ps) {
          const fmx::ExtractPlan p = fmx::extract_plan(4, C, k, S, P);
          CHECK(p.kc5 == (k == 5));
          CHECK(p.lds_rows <= fmx::kRowLdsMax);
          if (p.fused_normals) {
            CHECK(p.lds_normals <= fmx::kNrmLdsMax);
            CHECK(C <= fmx::kNrmMaxC);  // its work items pack the 64-column block in 6 bits
            ++n_fused;
          }
          if (p.sector_parallel) {
            ++n_par;
            CHECK(longest <= fmx::kSortCapacity);
            n_edge += longest == fmx::kSortCapacity;
            CHECK(S <= fmx::kParMaxSectors);  // a wave per sector
            CHECK(C / S >= 2 * k);            // suppression reaches the next sector only
            // sorted columns + stamps (8C bytes), the bitmap, two kept lists: inside the
            // 16C bytes of the staged points
            const size_t nwd = (size_t)(C + 63) / 64 + 1;
            CHECK(8 * (size_t)C + 8 * nwd + 8 * (size_t)S * (P + 1) <= 16 * (size_t)C);
          } else {
            ++n_seq;
          }
        }
      }
    }
  CHECK(n_par > 0 && n_seq > 0 && n_fused > 0);
  CHECK(n_edge > 0);  // the rule is not so conservative that the full capacity is never used
  // the grants are what one workgroup can have at all (160 KB of LDS per CU)
  CHECK(fmx::kRowLdsMax + 4096 <= 160 * 1024 && fmx::kNrmLdsMax < 160 * 1024);

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("extract plan ok (%ld sector-parallel, %ld sequential, %ld fused shapes swept)\n", n_par, n_seq, n_fused);
  return 0;
}
