// The kept code planes' validity (c_abi.hip: run_pass_launch; scan_kernel.hip: filter_dna_kernel<.., SRC>).  Plain C++, no
// HIP: launches in, "where do this launch's planes come from, and whose end must it wait for" out, so that the state
// machine is checked on the CPU (tests/test_plane_cache_cpu.py).
//
// The two code planes of a text block depend on the text alone.  In a stream of searches over a resident text every pass
// derives the same 16 bytes per 64-byte block again; the first launch over a half of the grid stores them (kPlaneWrite)
// and the launches behind it load them (kPlaneRead) instead of staging the text and extracting them.  What makes that
// safe is the in-flight contract (include/sassy_hip.h): the text stays unchanged while a ticket is open.  Planes written
// while ticket a was open are the text's planes for ticket c if the open intervals between them overlap into one interval.
// So:
//   - planes exist only while the searcher has at least one open ticket, counted without a break since they were written;
//     when the open count reaches zero every state drops to "not written" (the caller may rewrite the buffer then);
//   - the store has one key -- everything geometric that ScanJob::group_fits compares -- and a launch whose key differs
//     neither reads nor overwrites it while anything of the stored key is written;
//   - a half that launch slot X wrote is read behind X's end (the reader's stream waits for X's event) until the host has
//     seen X complete; then it is valid and read without a wait;
//   - a launch error drops everything, and nothing is kept again before the open count has been zero;
//   - planes are written only where a reader can follow (may_write: the caller sees a second ticket open, a second
//     member in the launch, or a half held back for the next begin).  A search with nothing else in flight takes its own
//     launch, writes nothing and has no store made for it: what it wrote would be forgotten at its finish.
#pragma once
#include <cstdint>

namespace sassy_hip {

enum : int { kPlaneRaw = 0, kPlaneWrite = 1, kPlaneRead = 2 };  // filter_dna_kernel's SRC: where a block's code planes come from

struct PlaneKey {
  const void* text = nullptr;
  uint64_t text_len = 0, n_blocks = 0, first_owned_block = 0, n_chunks = 0;
  uint32_t bpl = 0, n_iter = 0, fgrid = 0;
  // (not geometry: the search's flags.  The planes do not depend on them, but group_fits does: with them in the key the
  // tickets that use a store are exactly those that could share a launch with its writer)
  uint32_t flags = 0;
  bool operator==(const PlaneKey& o) const {
    return text == o.text && text_len == o.text_len && n_blocks == o.n_blocks && first_owned_block == o.first_owned_block &&
           n_chunks == o.n_chunks && bpl == o.bpl && n_iter == o.n_iter && fgrid == o.fgrid && flags == o.flags;
  }
  // [workgroup of the whole grid][wave 0..3][iteration][lane 0..63] x 16 bytes
  uint64_t store_bytes() const { return (uint64_t)fgrid * 4u * n_iter * 1024u; }
};

struct PlaneUse {
  int source = kPlaneRaw;
  int wait[2] = {-1, -1};  // kPlaneRead: the launch slots whose end the reader's stream waits for (-1: none)
};

class PlaneCache {
 public:
  enum : uint8_t { kH0 = 1, kH1 = 2, kWhole = 3 };  // (pass_planner.h: kPassH0 / kPassH1 / kPassWhole)

  int open_tickets() const { return open_; }
  // 0: not written; 1: written by writer(h), not yet seen complete; 2: valid
  int state(int h) const { return half_[h].state; }
  int writer(int h) const { return half_[h].slot; }
  bool anything_written() const { return half_[0].state != kNone || half_[1].state != kNone; }
  const PlaneKey& key() const { return key_; }

  void ticket_opened() { ++open_; }
  void ticket_closed() {
    if (open_ > 0) --open_;
    if (open_ == 0) {
      forget();
      poisoned_ = false;
    }
  }
  // would a launch that may write take the store for itself (nothing is written: the caller makes the store fit its key first)
  bool wants_store(bool may_write) const { return may_write && open_ > 0 && !poisoned_ && !anything_written(); }
  // One launch over `range` (a set of halves) of the grid of key k, carried by launch slot `slot`, of members that can take
  // their planes from a store.  may_write: a reader can follow; store_ok: the store fits k (asked only when wants_store
  // said so).
  PlaneUse launch(const PlaneKey& k, uint8_t range, int slot, bool may_write, bool store_ok) {
    PlaneUse u;
    if (open_ <= 0 || poisoned_ || (range & kWhole) == 0) return u;
    if (!anything_written()) {
      if (!may_write || !store_ok) return u;
      key_ = k;
    } else if (!(k == key_)) {
      return u;  // a foreign ticket among open ones: the text, as ever
    }
    int written = 0, halves = 0;
    for (int h = 0; h < 2; ++h)
      if (range & (1u << h)) {
        ++halves;
        if (half_[h].state != kNone) ++written;
      }
    if (written == halves) {
      u.source = kPlaneRead;
      int n = 0;
      for (int h = 0; h < 2; ++h)
        if ((range & (1u << h)) && half_[h].state == kWritten && (n == 0 || u.wait[0] != half_[h].slot)) u.wait[n++] = half_[h].slot;
    } else if (written == 0 && may_write) {
      u.source = kPlaneWrite;
      for (int h = 0; h < 2; ++h)
        if (range & (1u << h)) half_[h] = Half{kWritten, slot};
    }
    // (a whole launch over one written and one unwritten half reads the text and leaves both as they are)
    return u;
  }
  // the host has seen the launch of `slot` complete (a ticket it served is finished)
  void slot_done(int slot) {
    for (Half& h : half_)
      if (h.state == kWritten && h.slot == slot) h = Half{kValid, -1};
  }
  // a launch failed: nothing is read any more, nothing is written again before every open ticket has left
  void drop_all() {
    forget();
    poisoned_ = open_ > 0;
  }

 private:
  enum : uint8_t { kNone = 0, kWritten = 1, kValid = 2 };
  struct Half {
    uint8_t state;
    int slot;
  };
  Half half_[2] = {{kNone, -1}, {kNone, -1}};
  PlaneKey key_;
  int open_ = 0;
  bool poisoned_ = false;
  void forget() { half_[0] = half_[1] = Half{kNone, -1}; }
};

}  // namespace sassy_hip
