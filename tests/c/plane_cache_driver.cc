// Drives sassy_amd/csrc/plane_cache.h together with pass_planner.h (plain C++, no HIP) the way c_abi.hip does -- every
// launch the planner emits asks the cache where its planes come from -- over ALL begin / finish sequences of a given
// depth and length, and checks what every sequence must keep: see tests/test_plane_cache_cpu.py.
// Usage: plane_cache_driver <depth 2..4> <events>
//
// A sequence is a string of events; with t tickets open an event is one of: begin a ticket of key A, begin one of key B
// (another buffer: a foreign ticket), begin one that cannot take planes at all, finish the oldest, finish the newest.  The
// model next to the cache is the truth it is checked against: for every half, under which key it was written since the
// open count was last zero, and by which launch slot.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sassy_amd/csrc/pass_planner.h"
#include "../../sassy_amd/csrc/plane_cache.h"

using namespace sassy_hip;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      fprintf(stderr, "FAIL %s: ", #cond);    \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
      exit(1);                                \
    }                                         \
  } while (0)

constexpr int kSlots = 8;  // (host_internal.h: kPassSlots)

struct Ticket {
  bool live = false;
  int key = 0;        // 0 / 1: buffer A / B; 2: a search that cannot take planes (and cannot share a launch)
  uint64_t seq = 0;
  std::vector<int> slots;
  int plane_launches = 0;
};

struct Model {  // the truth
  int written_key[2] = {-1, -1};   // key the half was written under since the open count was last zero (-1: not)
  int written_slot[2] = {-1, -1};  // ... by this slot, until the host has seen it complete (-1 then)
  int store_key = -1;
};

static Ticket g_t[PassPlanner::kTickets];
static int g_users[kSlots];
static long g_sequences = 0, g_launches = 0, g_reads = 0, g_writes = 0, g_waits = 0, g_foreign_raw = 0, g_forgets = 0, g_stores = 0, g_lone_raw = 0;

static bool fits(void*, int a, int b) {
  return g_t[a].live && g_t[b].live && g_t[a].key < 2 && g_t[a].key == g_t[b].key;
}
static PlaneKey key_of(int k) {
  static const char bufs[2] = {0, 0};
  PlaneKey pk;
  pk.text = &bufs[k];
  pk.text_len = 1u << 22;
  pk.n_blocks = 1u << 16;
  pk.n_chunks = 1024;
  pk.bpl = 64;
  pk.n_iter = 66;
  pk.fgrid = 4;
  return pk;
}

struct Sim {
  PassPlanner planner;
  PlaneCache cache;
  Model model;
  int open = 0;
  uint64_t next_seq = 1;
  int mode = 4;

  void run(const std::vector<PassLaunch>& out) {
    for (const PassLaunch& pl : out) {
      ++g_launches;
      Ticket& a = g_t[pl.leader];
      Ticket* b = pl.member >= 0 ? &g_t[pl.member] : nullptr;
      const bool eligible = a.key < 2 && (!b || b->key < 2);
      int slot = -1;
      for (int i = 0; i < kSlots && slot < 0; ++i)
        if (g_users[i] == 0) slot = i;
      CHECK(slot >= 0, "no free launch slot");
      PlaneUse use;  // (a launch with a member that cannot take planes never asks: the text)
      if (eligible) {
        const PlaneKey k = key_of(a.key);
        // (c_abi.hip: a reader can follow -- a second ticket open, a second member, or a half held back)
        const bool may_write = cache.open_tickets() >= 2 || b != nullptr || pl.range != kPassWhole;
        const bool wants = cache.wants_store(may_write);
        if (wants) CHECK(model.written_key[0] < 0 && model.written_key[1] < 0, "the store is taken while a half is written");
        if (wants) ++g_stores;
        use = cache.launch(k, pl.range, slot, may_write, true);
        if (wants && use.source != kPlaneRaw) model.store_key = a.key;
        // a search with nothing else in flight: no store, no planes, its own launch
        if (open == 1 && !b && pl.range == kPassWhole) {
          CHECK(!wants && use.source != kPlaneWrite, "a lone whole launch asks for the store or writes (source %d)", use.source);
          if (use.source == kPlaneRaw) ++g_lone_raw;
        }
      }
      const bool plain = !b && pl.range == kPassWhole && use.source == kPlaneRaw;  // (the search's plain chain: no slot)
      if (!plain) {
        g_users[slot] = b ? 2 : 1;
        a.slots.push_back(slot);
        if (b) b->slots.push_back(slot);
      }
      CHECK(open > 0, "a launch with no ticket open");
      for (int h = 0; h < 2; ++h) {
        if (!(pl.range & (1 << h))) continue;
        if (use.source == kPlaneRead) {
          // no launch reads a half that was not written under the same key since the open count was last zero
          CHECK(model.written_key[h] == a.key, "half %d read under key %d, written under %d", h, a.key, model.written_key[h]);
          CHECK(model.store_key == a.key, "the store is key %d's, the reader's key is %d", model.store_key, a.key);
          // a reader always names the writer's slot (until the host has seen the writer complete)
          if (model.written_slot[h] >= 0) {
            CHECK(use.wait[0] == model.written_slot[h] || use.wait[1] == model.written_slot[h], "half %d: writer slot %d not named (%d, %d)", h,
                  model.written_slot[h], use.wait[0], use.wait[1]);
            CHECK(g_users[model.written_slot[h]] > 0 || model.written_slot[h] == slot, "the writer's slot %d was given back", model.written_slot[h]);
          }
        } else if (use.source == kPlaneWrite) {
          // a foreign ticket never clobbers: a half is written once per interval, under the store's key
          CHECK(model.written_key[h] < 0, "half %d written again (under %d, now %d)", h, model.written_key[h], a.key);
          CHECK(model.store_key == a.key, "a writer of key %d into the store of key %d", a.key, model.store_key);
          model.written_key[h] = a.key;
          model.written_slot[h] = slot;
        }
      }
      for (int i = 0; i < 2; ++i)
        if (use.wait[i] >= 0) {
          CHECK(use.source == kPlaneRead, "a wait without a read");
          CHECK(use.wait[i] == model.written_slot[0] || use.wait[i] == model.written_slot[1], "waits for slot %d, which wrote nothing", use.wait[i]);
          CHECK(use.wait[i] != slot, "a launch waits for itself");
          ++g_waits;
        }
      if (use.source == kPlaneRead) {
        ++g_reads;
        a.plane_launches += 1;
        if (b) b->plane_launches += 1;
      }
      if (use.source == kPlaneWrite) ++g_writes;
      if (use.source == kPlaneRaw && eligible && (model.written_key[0] >= 0 || model.written_key[1] >= 0) && a.key != model.store_key) ++g_foreign_raw;
    }
  }

  void begin(int key) {
    int id = -1;
    for (int i = 0; i < PassPlanner::kTickets && id < 0; ++i)
      if (!g_t[i].live) id = i;
    CHECK(id >= 0, "no free ticket");
    g_t[id] = Ticket();
    g_t[id].live = true;
    g_t[id].key = key;
    g_t[id].seq = next_seq++;
    cache.ticket_opened();
    ++open;
    std::vector<PassLaunch> out;
    planner.begin(id, key < 2, key < 2, true, false, mode, fits, nullptr, out);
    run(out);
  }

  void finish(bool newest) {
    int id = -1;
    for (int i = 0; i < PassPlanner::kTickets; ++i)
      if (g_t[i].live && (id < 0 || (newest ? g_t[i].seq > g_t[id].seq : g_t[i].seq < g_t[id].seq))) id = i;
    CHECK(id >= 0, "nothing to finish");
    std::vector<PassLaunch> out;
    planner.finish(id, false, mode, fits, nullptr, out);
    run(out);
    for (int s : g_t[id].slots) {
      g_users[s] -= 1;
      cache.slot_done(s);
      for (int h = 0; h < 2; ++h)
        if (model.written_slot[h] == s) model.written_slot[h] = -1;
    }
    g_t[id].live = false;
    cache.ticket_closed();
    --open;
    CHECK(cache.open_tickets() == open, "open count %d, the cache says %d", open, cache.open_tickets());
    if (open == 0) {  // dropping to zero open tickets forgets everything
      CHECK(!cache.anything_written(), "planes outlive the last open ticket");
      model = Model();
      ++g_forgets;
      for (int i = 0; i < kSlots; ++i) CHECK(g_users[i] == 0, "slot %d still held with no ticket open", i);
    }
    for (int h = 0; h < 2; ++h) {
      CHECK((cache.state(h) != 0) == (model.written_key[h] >= 0), "half %d: cache state %d, model key %d", h, cache.state(h), model.written_key[h]);
      if (cache.state(h) == 1) CHECK(cache.writer(h) == model.written_slot[h], "half %d: writer %d, model %d", h, cache.writer(h), model.written_slot[h]);
    }
  }
};

// events: 0 begin A, 1 begin B, 2 begin a search without planes, 3 finish oldest, 4 finish newest
static void replay(const std::vector<int>& ev, int mode) {
  for (Ticket& t : g_t) t = Ticket();
  for (int& u : g_users) u = 0;
  Sim sim;
  sim.mode = mode;
  for (int e : ev) {
    if (e <= 2) sim.begin(e);
    else sim.finish(e == 4);
  }
  while (sim.open > 0) sim.finish(false);
  ++g_sequences;
}

static void enumerate(std::vector<int>& ev, int open, int depth, int left, int mode) {
  if (left == 0) {
    replay(ev, mode);
    return;
  }
  for (int e = 0; e < 5; ++e) {
    if (e <= 2 && open >= depth) continue;
    if (e >= 3 && open == 0) continue;
    if (e == 4 && open == 1) continue;  // (the same as finishing the oldest)
    ev.push_back(e);
    enumerate(ev, e <= 2 ? open + 1 : open - 1, depth, left - 1, mode);
    ev.pop_back();
  }
}

int main(int argc, char** argv) {
  const int depth = argc > 1 ? atoi(argv[1]) : 3;
  const int events = argc > 2 ? atoi(argv[2]) : 8;
  CHECK(depth >= 2 && depth <= PassPlanner::kTickets && events >= 1 && events <= 12, "usage: plane_cache_driver <depth 2..4> <events 1..12>");
  for (int mode : {1, 4, 3, 0}) {
    std::vector<int> ev;
    enumerate(ev, 0, depth, events, mode);
  }
  // serial begin / finish (one ticket at a time), every mode: no store is asked for, nothing is written or read
  for (int mode : {1, 4, 3, 0}) {
    if (mode == 4) continue;  // (4 holds a half back even for a lone ticket: the tests' way to the staggered launches)
    const long stores = g_stores, reads = g_reads, writes = g_writes;
    replay({0, 3, 0, 3, 0, 3, 1, 3}, mode);
    CHECK(g_stores == stores && g_reads == reads && g_writes == writes, "serial searches in mode %d use planes", mode);
  }
  // a launch error drops everything, and nothing is kept again before the open count has been zero
  {
    PlaneCache c;
    c.ticket_opened();
    c.ticket_opened();
    PlaneUse u = c.launch(key_of(0), PlaneCache::kH0, 0, true, true);
    CHECK(u.source == kPlaneWrite, "first launch writes");
    u = c.launch(key_of(0), PlaneCache::kH0, 1, true, true);
    CHECK(u.source == kPlaneRead && u.wait[0] == 0 && u.wait[1] == -1, "second launch reads behind slot 0");
    u = c.launch(key_of(0), PlaneCache::kWhole, 2, true, true);
    CHECK(u.source == kPlaneRaw && c.state(1) == 0, "a whole launch over a written and an unwritten half reads the text");
    c.drop_all();
    CHECK(!c.anything_written(), "drop_all keeps planes");
    u = c.launch(key_of(0), PlaneCache::kH0, 3, true, true);
    CHECK(u.source == kPlaneRaw && !c.wants_store(true), "planes are kept again before the open count was zero");
    c.ticket_closed();
    c.ticket_closed();
    c.ticket_opened();
    CHECK(c.wants_store(true) && !c.wants_store(false), "a fresh stream does not ask for the store");
    u = c.launch(key_of(0), PlaneCache::kH0, 3, true, false);
    CHECK(u.source == kPlaneRaw && !c.anything_written(), "a launch without a store keeps planes");
    u = c.launch(key_of(0), PlaneCache::kWhole, 3, false, true);
    CHECK(u.source == kPlaneRaw && !c.anything_written(), "a launch no reader can follow writes");
    u = c.launch(key_of(0), PlaneCache::kWhole, 3, true, true);
    CHECK(u.source == kPlaneWrite && c.state(0) == 1 && c.state(1) == 1, "a whole launch writes both halves");
    c.slot_done(3);
    u = c.launch(key_of(0), PlaneCache::kWhole, 4, true, true);
    CHECK(u.source == kPlaneRead && u.wait[0] == -1 && u.wait[1] == -1, "valid halves are read without a wait");
    c.ticket_closed();
    CHECK(!c.anything_written() && c.open_tickets() == 0, "the last ticket takes the planes with it");
    u = c.launch(key_of(0), PlaneCache::kWhole, 4, true, true);
    CHECK(u.source == kPlaneRaw, "a launch with no ticket open takes planes");
  }
  printf("ok sequences=%ld launches=%ld reads=%ld writes=%ld waits=%ld foreign_raw=%ld forgets=%ld lone_raw=%ld\n", g_sequences, g_launches, g_reads,
         g_writes, g_waits, g_foreign_raw, g_forgets, g_lone_raw);
  return 0;
}
