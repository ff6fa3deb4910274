// Drives sassy_amd/csrc/pass_planner.h (plain C++, no HIP) with random begin / finish sequences and checks what every
// sequence must keep: see tests/test_pass_planner_cpu.py.  Usage: pass_planner_driver <seed> <sequences>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sassy_amd/csrc/pass_planner.h"

using namespace sassy_hip;

struct Sim {
  bool live = false, groupable = false, has_pass = false, splittable = false;
  int buffer = 0;
  uint64_t seq = 0;
  uint8_t got = 0;
  int max_members = 0;
};
static Sim g_t[PassPlanner::kTickets];

static bool fits(void*, int a, int b) {
  return g_t[a].live && g_t[b].live && g_t[a].groupable && g_t[b].groupable && g_t[a].buffer == g_t[b].buffer &&
         g_t[a].splittable == g_t[b].splittable;
}

static uint64_t g_rng;
static uint32_t rnd(uint32_t n) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_rng >> 33) % n);
}

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      fprintf(stderr, "FAIL %s: ", #cond);    \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
      exit(1);                                \
    }                                         \
  } while (0)

static long g_launches = 0, g_pairs = 0, g_halves = 0;

static void apply(const std::vector<PassLaunch>& out, int mode, uint64_t s) {
  for (const PassLaunch& pl : out) {
    ++g_launches;
    CHECK(pl.range == kPassH0 || pl.range == kPassH1 || pl.range == kPassWhole, "range %d seq %llu", pl.range, (unsigned long long)s);
    CHECK(pl.leader >= 0 && pl.leader < PassPlanner::kTickets && g_t[pl.leader].live, "leader %d", pl.leader);
    CHECK(pl.member >= -1 && pl.member < PassPlanner::kTickets && pl.member != pl.leader, "member %d", pl.member);
    if (pl.range != kPassWhole) ++g_halves;
    if (mode == 0 || mode == 2 || mode == 3) CHECK(pl.range == kPassWhole, "mode %d launches a half", mode);
    if (mode == 0) CHECK(pl.member < 0, "mode 0 shares a launch");
    if (pl.range != kPassWhole) CHECK(g_t[pl.leader].splittable, "half of a grid of one workgroup");
    for (int id : {pl.leader, pl.member}) {  // (both members get the same range: one field)
      if (id < 0) continue;
      CHECK(g_t[id].live && g_t[id].has_pass, "member %d is not open", id);
      CHECK((g_t[id].got & pl.range) == 0, "ticket %d gets range %d twice (has %d)", id, pl.range, g_t[id].got);
      g_t[id].got |= pl.range;
      g_t[id].max_members = pl.member >= 0 ? 2 : (g_t[id].max_members ? g_t[id].max_members : 1);
    }
    if (pl.member >= 0) {
      ++g_pairs;
      CHECK(fits(nullptr, pl.leader, pl.member), "members %d and %d do not fit", pl.leader, pl.member);
      CHECK(g_t[pl.leader].seq < g_t[pl.member].seq, "the leader is not the older ticket");
    }
  }
}

static void sequence(uint64_t s) {
  PassPlanner P;
  for (Sim& t : g_t) t = Sim();
  const int modes[5] = {0, 1, 2, 3, 4};
  const int mode = modes[rnd(5)];
  const int depth = 2 + (int)rnd(3);
  const int order = (int)rnd(3);             // finish oldest / newest / any
  const uint32_t p_plain = rnd(4) ? rnd(40) : 0;  // per cent of tickets that cannot share
  const uint32_t p_other = rnd(3) ? rnd(40) : 0;  // ... on another buffer
  uint64_t seq = 1;
  int in_flight = 0, last = -1;
  std::vector<PassLaunch> out;
  const int steps = 5 + (int)rnd(60);
  for (int step = 0; step < steps || in_flight; ++step) {
    const bool can_begin = step < steps && in_flight < depth;
    if (can_begin && (in_flight == 0 || rnd(3))) {
      int id = -1;
      for (int l = 0; l < depth; ++l)
        if (!g_t[(last + 1 + l) % depth].live) { id = (last + 1 + l) % depth; break; }
      Sim& t = g_t[id];
      t = Sim();
      t.live = true;
      t.has_pass = rnd(20) != 0;
      t.groupable = t.has_pass && rnd(100) >= p_plain && mode != 0 && depth > 1;
      t.splittable = t.groupable && rnd(12) != 0;
      t.buffer = rnd(100) < p_other ? 1 : 0;
      t.seq = seq++;
      last = id;
      ++in_flight;
      out.clear();
      P.begin(id, t.groupable, t.splittable, t.has_pass, rnd(2) != 0, mode, fits, nullptr, out);
      apply(out, mode, s);
      if (!t.groupable) CHECK(t.got == (t.has_pass ? kPassWhole : 0), "a ticket that cannot share is not launched whole at once");
      if (mode == 0) CHECK(!P.any_open(), "mode 0 keeps something back");
    } else if (in_flight) {
      int id = -1;
      for (int i = 0; i < PassPlanner::kTickets; ++i) {
        if (!g_t[i].live) continue;
        if (id < 0 || (order == 0 && g_t[i].seq < g_t[id].seq) || (order == 1 && g_t[i].seq > g_t[id].seq) || (order == 2 && rnd(2))) id = i;
      }
      out.clear();
      P.finish(id, rnd(2) != 0, mode, fits, nullptr, out);
      apply(out, mode, s);
      CHECK(g_t[id].got == (g_t[id].has_pass ? kPassWhole : 0), "finish(%d) returns with range(s) %d unlaunched, mode %d", id, kPassWhole ^ g_t[id].got, mode);
      CHECK(P.need(id) == 0, "planner still holds a need of a finished ticket");
      g_t[id].live = false;
      --in_flight;
    }
    for (int i = 0; i < PassPlanner::kTickets; ++i)  // the planner's book and the launches agree
      if (g_t[i].live) CHECK(P.need(i) == (g_t[i].has_pass ? (kPassWhole ^ g_t[i].got) : 0), "ticket %d: planner needs %d, launched %d", i, P.need(i), g_t[i].got);
  }
  CHECK(!P.any_open(), "something is open after the last finish");
}

// a stream of tickets that all fit, finished oldest first, mode 4: every ticket with a predecessor and a successor shares
// both of its halves, and every begin queues exactly one launch
static void staggered_stream(int depth, int n) {
  PassPlanner P;
  for (Sim& t : g_t) t = Sim();
  std::vector<PassLaunch> out;
  std::vector<int> members_of(n, 0), launches_of(n, 0), lane_of(n, -1);
  uint64_t seq = 1;
  auto note = [&](int mode) {
    apply(out, mode, 0);
    for (const PassLaunch& pl : out)
      for (int id : {pl.leader, pl.member})
        if (id >= 0) {
          const int j = (int)g_t[id].seq - 1;
          launches_of[j] += 1;
          if (pl.member >= 0) members_of[j] += 1;
        }
  };
  for (int j = 0; j < n + depth; ++j) {
    if (j >= depth) {
      const int id = lane_of[j - depth];
      out.clear();
      P.finish(id, true, 4, fits, nullptr, out);
      note(4);
      g_t[id].live = false;
    }
    if (j < n) {
      const int id = j % depth;
      g_t[id] = Sim();
      g_t[id].live = g_t[id].groupable = g_t[id].has_pass = g_t[id].splittable = true;
      g_t[id].seq = seq++;
      lane_of[j] = id;
      out.clear();
      P.begin(id, true, true, true, false, 4, fits, nullptr, out);
      CHECK(out.size() == 1, "begin %d queues %zu launches", j, out.size());
      note(4);
    }
  }
  for (int j = 1; j + 1 < n; ++j) CHECK(launches_of[j] == 2 && members_of[j] == 2, "ticket %d: %d launches, %d shared", j, launches_of[j], members_of[j]);
}

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const long n = argc > 2 ? atol(argv[2]) : 1000;
  g_rng = seed * 0x9E3779B97F4A7C15ull + 1;
  for (long i = 0; i < n; ++i) sequence((uint64_t)i);
  for (int depth = 2; depth <= 4; ++depth)
    for (int len : {3, 4, 7, 10}) staggered_stream(depth, len);
  printf("ok sequences=%ld launches=%ld shared=%ld halves=%ld\n", n, g_launches, g_pairs, g_halves);
  return 0;
}
