// The shared pass's planner (c_abi.hip: searches in flight over one buffer share text passes).  Plain C++, no HIP: tickets
// in, "launch this workgroup range for these members" out, so that the state machine is checked on the CPU
// (tests/test_pass_planner_cpu.py).
//
// The fused filter's workgroups are independent, so a ticket's text pass need not be one launch.  The grid is cut in two
// halves, H0 = workgroups [0, ceil(fgrid / 2)) and H1 = the rest; a ticket needs both, in either order, each from a launch
// with at most two members.  Two policies:
//   grouped   (shared_pass 2, 3): a groupable ticket that is begun while a pass streams waits, whole, for a second one;
//             the two share one whole launch.
//   staggered (shared_pass 1, 4): begin(i) launches { ticket i-1: its second half, ticket i: its first half } over the same
//             half of the grid.  Every begin queues one half launch of two members, a ticket is complete one begin
//             after its own, and the host never waits with nothing queued behind the running half pass.
// Nothing stays unlaunched across finish(): no deadlock.
#pragma once
#include <cstdint>
#include <vector>

namespace sassy_hip {

enum : uint8_t { kPassH0 = 1, kPassH1 = 2, kPassWhole = 3 };  // a range = a set of halves

struct PassLaunch {
  int leader;     // the older ticket: its lane's stream carries the launch
  int member;     // the second member (-1: the leader alone)
  uint8_t range;  // kPassH0 / kPassH1 / kPassWhole, the same for both members
};

class PassPlanner {
 public:
  static constexpr int kTickets = 4;  // one per lane; a ticket is named by its lane
  // may tickets a and b share a launch (ScanJob::group_fits)
  typedef bool (*Fits)(void* ctx, int a, int b);

  // what ticket id still needs (a set of halves; 0: every launch it needs is queued)
  uint8_t need(int id) const { return t_[id].live ? t_[id].need : 0; }
  bool any_open() const {
    for (const T& t : t_)
      if (t.live && t.need) return true;
    return false;
  }

  // Ticket id is begun.  groupable: it can share a launch at all (ScanJob::group_ok and more than one search in flight);
  // splittable: its grid has two halves; has_pass: it needs a launch (not an empty shard); streaming: a pass of this
  // searcher is still running on the device; mode: the switch shared_pass.
  void begin(int id, bool groupable, bool splittable, bool has_pass, bool streaming, int mode, Fits fits, void* ctx,
             std::vector<PassLaunch>& out) {
    T& x = t_[id];
    x = T{true, groupable && mode != 0, (uint8_t)(has_pass ? kPassWhole : 0), next_seq_++};
    if (!has_pass || !x.groupable) {  // order: what waits goes in front of a search that cannot join it
      flush(fits, ctx, out);
      return;
    }
    if (mode == 2 || mode == 3) {  // grouped: wait, whole, for a partner while a pass streams
      const int p = oldest_open(id, kPassWhole, 0);
      if (p >= 0 && !pair_ok(p, id, fits, ctx)) flush_others(id, fits, ctx, out);
      const bool waiting = oldest_open(id, 0, 0) >= 0;
      if (waiting || !streaming) flush(fits, ctx, out);  // the group is full, or nothing streams any more: go
      return;
    }
    // staggered: the oldest ticket that still needs one half and fits gets it together with this one's first half
    if (splittable) {
      const int p = oldest_open(id, kPassH0, kPassH1, fits, ctx);
      if (p >= 0) {
        const uint8_t h = t_[p].need;
        out.push_back(PassLaunch{p, id, h});
        t_[p].need = 0;
        x.need = (uint8_t)(kPassWhole ^ h);
        return;
      }
    }
    const bool flushed = oldest_open(id, 0, 0) >= 0;
    flush_others(id, fits, ctx, out);  // (tickets that fit nobody: their halves go first)
    if (splittable && (streaming || flushed || mode == 4)) {
      out.push_back(PassLaunch{id, -1, kPassH0});  // keep the second half back for the next begin
      x.need = kPassH1;
    } else {
      out.push_back(PassLaunch{id, -1, kPassWhole});
      x.need = 0;
    }
  }

  // Ticket id is about to be waited for (would_wait: its lane still has work queued) and leaves.
  void finish(int id, bool would_wait, int mode, Fits fits, void* ctx, std::vector<PassLaunch>& out) {
    T& x = t_[id];
    if (!x.live) return;
    if (mode == 2 || mode == 3) {
      if (x.need || (mode == 2 && would_wait)) flush(fits, ctx, out);
    } else if (x.need) {
      const uint8_t h = x.need;
      const int p = oldest_open(id, h, h, fits, ctx);  // another ticket that needs the same range shares the launch
      if (p >= 0) {
        const bool p_older = t_[p].seq < x.seq;
        out.push_back(PassLaunch{p_older ? p : id, p_older ? id : p, h});
        t_[p].need = 0;
      } else {
        out.push_back(PassLaunch{id, -1, h});
      }
      x.need = 0;
    }
    x.live = false;
  }

  // ticket id leaves without another launch (its begin failed)
  void drop(int id) { t_[id].live = false; }

  // launches everything open tickets still need, two tickets that need the same range and fit together
  void flush(Fits fits, void* ctx, std::vector<PassLaunch>& out) { flush_others(-1, fits, ctx, out); }

 private:
  struct T {
    bool live;
    bool groupable;
    uint8_t need;
    uint64_t seq;
  };
  T t_[kTickets] = {};
  uint64_t next_seq_ = 1;

  bool pair_ok(int a, int b, Fits fits, void* ctx) const { return t_[a].groupable && t_[b].groupable && fits(ctx, a, b); }
  // the oldest live ticket other than `skip` whose need is a or b (a = b = 0: any need) and, with fits, that fits `skip`
  int oldest_open(int skip, uint8_t a, uint8_t b, Fits fits = nullptr, void* ctx = nullptr) const {
    int best = -1;
    for (int i = 0; i < kTickets; ++i) {
      const T& t = t_[i];
      if (i == skip || !t.live || !t.need) continue;
      if ((a || b) && t.need != a && t.need != b) continue;
      if (fits && !pair_ok(i, skip, fits, ctx)) continue;
      if (best < 0 || t.seq < t_[best].seq) best = i;
    }
    return best;
  }
  void flush_others(int skip, Fits fits, void* ctx, std::vector<PassLaunch>& out) {
    for (;;) {
      const int a = oldest_open(skip, 0, 0);
      if (a < 0) return;
      const uint8_t h = t_[a].need;
      int b = -1;
      for (int i = 0; i < kTickets; ++i) {
        const T& t = t_[i];
        if (i == a || i == skip || !t.live || t.need != h || !pair_ok(a, i, fits, ctx)) continue;
        if (b < 0 || t.seq < t_[b].seq) b = i;
      }
      out.push_back(PassLaunch{a, b, h});
      t_[a].need = 0;
      if (b >= 0) t_[b].need = 0;
    }
  }
};

}  // namespace sassy_hip
