// The host-only planning of the keypoint pool and the window store
// (form_amd/csrc/store_plan.hpp) under the address and undefined-behaviour sanitizers.
//
//   test_store_plan          fixed cases, prints "store_plan ok"
//   test_store_plan drive    one command per line on stdin, one answer line per command on
//                            stdout: tests/test_store_cpu.py drives random sequences through
//                            it and checks every answer against tests/store_ref.py
//
// drive commands (all numbers decimal):
//   P limit alloc                pool of `alloc` records taking `limit`
//   a scan n                     ensure room for n, then append n records of scan
//   r scan                       remove the scan
//   W kpc lim_pl lim_pt          window store as win_reserve sets it up (kpc: keypoint_pool_capacity)
//   p j K (scan npl npt) x K     win_persist of segment j
//   e scan                       win_remove
// answers:
//   pool:   <ok|oom|state> <compacted> <ncopies> (src dst n)* | <used> <nranges> (scan off n)*
//   window: ok <compacted> <grow_pl> <grow_pt> <nseg copies> (src dst n)*pl (src dst n)*pt |
//           <cap_pl> <cap_pt> <tail_pl> <tail_pt> <alloc_pl0> <alloc_pl1> <alloc_pt0> <alloc_pt1> <cur>
//           <nsegs> (j pl_off pt_off pl_n pt_n npairs (i pl_off pt_off pl_n pt_n)*)*
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "store_plan.hpp"

using namespace fmx;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

namespace {

struct PoolSim {
  PoolRanges ranges;
  uint64_t used = 0, limit = 0, alloc = 0;
};

// ensure_pool_room + pool_append as fmx_api.cpp runs them
std::string pool_add(PoolSim& P, uint64_t scan, uint32_t n) {
  std::ostringstream o;
  PoolPlan plan;
  bool compacted = false;
  const char* st = "ok";
  if (n) {
    if (!pool_has_room(P.used, n, P.limit)) {
      plan = plan_pool_compact(P.ranges);
      P.used = plan.used;
      compacted = true;
      if (!pool_has_room(P.used, n, P.limit)) st = "oom";
    }
    if (!std::strcmp(st, "ok") && !pool_append(P.ranges, P.used, scan, n)) st = "state";
  }
  o << st << ' ' << (int)compacted << ' ' << plan.copies.size();
  for (auto& c : plan.copies) o << ' ' << c.src << ' ' << c.dst << ' ' << c.n;
  return o.str();
}
std::string pool_state(const PoolSim& P) {
  std::ostringstream o;
  o << " | " << P.used << ' ' << P.ranges.size();
  for (auto& [s, r] : P.ranges) o << ' ' << s << ' ' << r.first << ' ' << r.second;
  return o.str();
}

struct Arena {  // DBuf<double>'s size bookkeeping
  size_t cap = 0;
  void ensure(size_t n) {
    if (n > cap) cap = dbuf_alloc_elems(n);
  }
};
struct WinSim {
  StoreLimits lim;
  uint64_t kpc = 0;
  Arena pl[2], pt[2];
  int cur = 0;
  uint64_t cap_pl = 0, cap_pt = 0, tail_pl = 0, tail_pt = 0;
  bool exact_pl = false, exact_pt = false;
  WinSegs segs;
};

// win_persist + win_reserve as window.hip runs them (allocation sizes only)
std::string win_persist(WinSim& W, uint64_t j, const std::vector<uint64_t>& scans, const std::vector<uint32_t>& cpl,
                        const std::vector<uint32_t>& cpt) {
  uint64_t npl = 0, npt = 0;
  for (size_t k = 0; k < scans.size(); ++k) {
    npl += cpl[k];
    npt += cpt[k];
  }
  if (W.cap_pl == 0) {
    W.exact_pl = W.lim.win_pl != 0;
    W.exact_pt = W.lim.win_pt != 0;
    uint64_t want_pl, want_pt;
    win_initial_caps(W.kpc, W.lim, want_pl, want_pt);
    for (int b = 0; b < 2; ++b) {
      W.pl[b].ensure(9 * want_pl);
      W.pt[b].ensure(6 * want_pt);
    }
    W.cap_pl = win_cap_of(want_pl, W.pl[0].cap, 9, W.exact_pl);
    W.cap_pt = win_cap_of(want_pt, W.pt[0].cap, 6, W.exact_pt);
  }
  const WinPlan plan = plan_win_reserve(W.segs, W.tail_pl, W.tail_pt, W.cap_pl, W.cap_pt, npl, npt);
  bool grow_pl = false, grow_pt = false;
  if (plan.compact) {
    const int nxt = 1 - W.cur;
    grow_pl = plan.want_pl != W.cap_pl;
    grow_pt = plan.want_pt != W.cap_pt;
    if (grow_pl || grow_pt) {
      W.pl[nxt].ensure(9 * plan.want_pl);
      W.pt[nxt].ensure(6 * plan.want_pt);
    }
    const uint64_t ncap_pl = grow_pl ? win_cap_of(plan.want_pl, W.pl[nxt].cap, 9, W.exact_pl) : W.cap_pl;
    const uint64_t ncap_pt = grow_pt ? win_cap_of(plan.want_pt, W.pt[nxt].cap, 6, W.exact_pt) : W.cap_pt;
    W.cur = nxt;
    W.tail_pl = plan.tail_pl;
    W.tail_pt = plan.tail_pt;
    W.pl[1 - nxt].ensure(9 * ncap_pl);
    W.pt[1 - nxt].ensure(6 * ncap_pt);
    W.cap_pl = ncap_pl;
    W.cap_pt = ncap_pt;
  }
  WinSeg s = win_make_seg(j, W.tail_pl, W.tail_pt, scans.data(), cpl.data(), cpt.data(), (uint32_t)scans.size());
  W.tail_pl += npl;
  W.tail_pt += npt;
  W.segs[j] = std::move(s);
  std::ostringstream o;
  o << "ok " << (int)plan.compact << ' ' << (int)grow_pl << ' ' << (int)grow_pt << ' ' << plan.pl.size();
  for (auto& c : plan.pl) o << ' ' << c.src << ' ' << c.dst << ' ' << c.n;
  for (auto& c : plan.pt) o << ' ' << c.src << ' ' << c.dst << ' ' << c.n;
  return o.str();
}
std::string win_state(const WinSim& W) {
  std::ostringstream o;
  o << " | " << W.cap_pl << ' ' << W.cap_pt << ' ' << W.tail_pl << ' ' << W.tail_pt << ' ' << W.pl[0].cap << ' '
    << W.pl[1].cap << ' ' << W.pt[0].cap << ' ' << W.pt[1].cap << ' ' << W.cur << ' ' << W.segs.size();
  for (auto& [j, s] : W.segs) {
    o << ' ' << j << ' ' << s.pl_off << ' ' << s.pt_off << ' ' << s.pl_n << ' ' << s.pt_n << ' ' << s.pairs.size();
    for (auto& p : s.pairs) o << ' ' << p.i << ' ' << p.pl_off << ' ' << p.pt_off << ' ' << p.pl_n << ' ' << p.pt_n;
  }
  return o.str();
}

int drive() {
  PoolSim P;
  WinSim W;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char op = 0;
    in >> op;
    std::string out;
    if (op == 'P') {
      P = PoolSim{};
      in >> P.limit >> P.alloc;
      P.limit = std::min(P.limit ? P.limit : P.alloc, P.alloc);
      out = "ok 0 0" + pool_state(P);
    } else if (op == 'a') {
      uint64_t scan;
      uint32_t n;
      in >> scan >> n;
      out = pool_add(P, scan, n);
      out += pool_state(P);
    } else if (op == 'r') {
      uint64_t scan;
      in >> scan;
      P.ranges.erase(scan);
      out = "ok 0 0" + pool_state(P);
    } else if (op == 'W') {
      W = WinSim{};
      in >> W.kpc >> W.lim.win_pl >> W.lim.win_pt;
      out = "ok 0 0 0 0" + win_state(W);
    } else if (op == 'p') {
      uint64_t j;
      uint32_t K;
      in >> j >> K;
      std::vector<uint64_t> scans(K);
      std::vector<uint32_t> cpl(K), cpt(K);
      for (uint32_t k = 0; k < K; ++k) in >> scans[k] >> cpl[k] >> cpt[k];
      out = win_persist(W, j, scans, cpl, cpt);
      out += win_state(W);
    } else if (op == 'e') {
      uint64_t s;
      in >> s;
      win_erase_scan(W.segs, s);
      out = "ok 0 0 0 0" + win_state(W);
    } else {
      continue;
    }
    if (!in) return 2;
    std::cout << out << std::endl;
  }
  return 0;
}

int fixed() {
  // limits: absent, empty, partial, full
  CHECK(parse_store_limits(nullptr).pool == 0 && parse_store_limits("").win_pl == 0);
  StoreLimits l = parse_store_limits("3000,4096,512");
  CHECK(l.pool == 3000 && l.win_pl == 4096 && l.win_pt == 512);
  l = parse_store_limits("0,0,700");
  CHECK(l.pool == 0 && l.win_pl == 0 && l.win_pt == 700);
  l = parse_store_limits("5");
  CHECK(l.pool == 5 && l.win_pl == 0 && l.win_pt == 0);
  l = parse_store_limits("x");
  CHECK(l.pool == 0 && l.win_pl == 0 && l.win_pt == 0);
  // production sizes are untouched without limits
  uint64_t a, b;
  win_initial_caps(4u << 20, StoreLimits{}, a, b);
  CHECK(a == (4u << 20) && b == (1u << 20));
  win_initial_caps(100, StoreLimits{}, a, b);
  CHECK(a == (1u << 20) && b == (1u << 18));
  CHECK(dbuf_alloc_elems(1) == (1u << 18) && dbuf_alloc_elems(1u << 20) == (2u << 20) + 64);
  CHECK(win_cap_of(100, 1u << 18, 9, false) == (1u << 18) / 9 && win_cap_of(100, 1u << 18, 9, true) == 100);

  // pool: exact fit needs no compaction, one over does; a hole closes; order by offset
  PoolSim P;
  P.limit = 100;
  P.alloc = 1 << 18;
  CHECK(pool_add(P, 7, 40) == "ok 0 0");
  CHECK(pool_add(P, 3, 30) == "ok 0 0");
  CHECK(pool_add(P, 9, 30) == "ok 0 0");  // exact fit
  CHECK(P.used == 100);
  CHECK(pool_add(P, 9, 1) == "oom 1 3 0 0 40 40 40 30 70 70 30");  // nothing to reclaim
  P.ranges.erase(3);
  CHECK(pool_add(P, 9, 30) == "ok 1 2 0 0 40 70 40 30");  // fits only after compaction; scan 9 stays last
  CHECK(P.ranges[7].first == 0 && P.ranges[9].first == 40 && P.ranges[9].second == 60 && P.used == 100);
  CHECK(pool_add(P, 7, 0) == "ok 0 0");
  P.ranges.erase(9);
  CHECK(pool_add(P, 7, 5) == "ok 1 1 0 0 40" && P.used == 45);
  CHECK(pool_add(P, 11, 10) == "ok 0 0");
  CHECK(pool_add(P, 7, 5) == "state 0 0" && P.used == 55);  // scan 7's records would not be contiguous
  CHECK(pool_add(P, 11, 1000).substr(0, 3) == "oom");  // larger than the whole pool

  // window store: growth from empty, compaction without growth, pair offsets rebased
  WinSim W;
  W.lim.win_pl = 64;
  W.lim.win_pt = 16;
  std::vector<uint64_t> sc{0};
  win_persist(W, 1, sc, {100}, {3});  // first segment larger than the plane capacity
  CHECK(W.cap_pl == 256 && W.cap_pt == 16 && W.segs[1].pl_off == 0 && W.tail_pl == 100);
  sc = {0, 1};
  win_persist(W, 2, sc, {20, 30}, {2, 2});
  CHECK(W.segs[2].pairs.size() == 2 && W.segs[2].pairs[1].pl_off == 120 && W.segs[2].pairs[1].pt_off == 5);
  win_erase_scan(W.segs, 1);
  CHECK(W.segs.size() == 1 && W.segs[2].pairs.size() == 1 && W.segs[2].pairs[0].i == 0);
  sc = {0, 5};
  win_persist(W, 3, sc, {35, 35}, {1, 1});
  CHECK(W.tail_pl == 220 && W.tail_pt == 9);
  win_erase_scan(W.segs, 2);
  sc = {0, 3};
  std::string r = win_persist(W, 4, sc, {25, 25}, {1, 1});  // 220 + 50 > 256, 2 * 120 <= 256: compact, no growth
  CHECK(r == "ok 1 0 0 1 150 0 70 7 0 2");
  CHECK(W.cap_pl == 256 && W.segs[3].pl_off == 0 && W.segs[3].pairs[1].pl_off == 35 && W.segs[3].pairs[1].pt_off == 1);
  CHECK(W.segs[4].pl_off == 70 && W.segs[4].pt_off == 2 && W.segs[4].pairs[1].pl_off == 95 && W.cur == 0);
  CHECK(W.tail_pl == 120 && W.tail_pt == 4);
  std::printf("store_plan ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "drive")) return drive();
  return fixed();
}
