// tests/c/piece_pair_driver.cc -- the block-pair piece test (sassy_amd/csrc/piece_pair_step.h) against a per-column
// comparison of 2-bit codes and against two calls of the single-block form.  A stand-alone program: its own main, no HIP.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o piece_pair_driver piece_pair_driver.cc
//   ./piece_pair_driver <seed>      prints "ok plants=.. reach_prev=.. reach_a=.. random=.. occurrences=.. chance=.." or the first mismatch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sassy_amd/csrc/piece_pair_step.h"

using namespace sassy_hip;

namespace {

constexpr int NS = 8;

struct Rng {
  uint64_t x;
  uint32_t next() {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return (uint32_t)(x >> 16);
  }
};

// the 32 columns in front of a, a and b as one row of columns -32 .. 127 per plane
struct Cols {
  uint32_t w[2][5];  // [plane]{prev high half, a low, a high, b low, b high}
  uint32_t bit(int plane, int col) const { return (w[plane][(col + 32) >> 5] >> ((col + 32) & 31)) & 1u; }
  void set(int plane, int col, uint32_t v) {
    uint32_t& word = w[plane][(col + 32) >> 5];
    word = (word & ~(1u << ((col + 32) & 31))) | (v << ((col + 32) & 31));
  }
  PiecePlanes a() const { return PiecePlanes{w[0][1], w[0][2], w[1][1], w[1][2]}; }
  PiecePlanes b() const { return PiecePlanes{w[0][3], w[0][4], w[1][3], w[1][4]}; }
};

struct Counts {
  long plants = 0, reach_prev = 0, reach_a = 0, random = 0, occurrences = 0, chance = 0;
};

template <int Q>
bool check(const Cols& t, const uint32_t (&p0)[NS], const uint32_t (&p1)[NS], const char* what, int slot, int col, Counts* n, bool planted) {
  uint32_t nb0[NS], nb1[NS];
  for (int s = 0; s < NS; ++s) { nb0[s] = ~p0[s]; nb1[s] = ~p1[s]; }  // (as the kernel: the complement of the whole word)
  alignas(16) uint32_t tab[Q * NS * 2];
  static_assert(piece_row_table_words<Q, NS>() == Q * NS * 2, "table size");
  piece_row_table_fill<Q, NS>(tab, 0u, 1u, [&](uint32_t s, int plane) { return plane ? nb1[s] : nb0[s]; });
  uint32_t al[NS], ah[NS], bl[NS], bh[NS];
  uint32_t prev0 = t.w[0][0], prev1 = t.w[1][0];
  piece_pair_step<Q, NS>(t.a(), t.b(), prev0, prev1, tab, al, ah, bl, bh);
  if (prev0 != t.w[0][4] || prev1 != t.w[1][4]) {
    printf("FAIL %s Q=%d slot=%d col=%d: handed on %08x %08x, b's high halves are %08x %08x\n", what, Q, slot, col, prev0, prev1, t.w[0][4], t.w[1][4]);
    return false;
  }
  // two calls of the single-block form
  uint32_t sal[NS], sah[NS], sbl[NS], sbh[NS];
  uint32_t q0 = t.w[0][0], q1 = t.w[1][0];
  piece_block_step<Q, NS>(t.a(), q0, q1, nb0, nb1, sal, sah);
  piece_block_step<Q, NS>(t.b(), q0, q1, nb0, nb1, sbl, sbh);
  if (q0 != prev0 || q1 != prev1) {
    printf("FAIL %s Q=%d: the single-block form hands on %08x %08x\n", what, Q, q0, q1);
    return false;
  }
  for (int s = 0; s < NS; ++s) {
    // the definition, column by column: every row's 2-bit code against the text's
    uint64_t want[2] = {0, 0};
    for (int c = 0; c < 128; ++c) {
      bool all = true;
      for (int j = 0; j < Q && all; ++j) {
        const int at = c - (Q - 1 - j);
        all = t.bit(0, at) == ((p0[s] >> j) & 1u) && t.bit(1, at) == ((p1[s] >> j) & 1u);
      }
      if (all) want[c >> 6] |= 1ull << (c & 63);
    }
    const uint64_t got_a = ((uint64_t)ah[s] << 32) | al[s], got_b = ((uint64_t)bh[s] << 32) | bl[s];
    const uint64_t one_a = ((uint64_t)sah[s] << 32) | sal[s], one_b = ((uint64_t)sbh[s] << 32) | sbl[s];
    if (got_a != want[0] || got_b != want[1] || one_a != want[0] || one_b != want[1]) {
      printf("FAIL %s Q=%d planted slot=%d col=%d, slot %d: pair %016llx %016llx, single %016llx %016llx, by column %016llx %016llx\n", what, Q, slot,
             col, s, (unsigned long long)got_a, (unsigned long long)got_b, (unsigned long long)one_a, (unsigned long long)one_b,
             (unsigned long long)want[0], (unsigned long long)want[1]);
      return false;
    }
    const long occ = __builtin_popcountll(want[0]) + __builtin_popcountll(want[1]);
    n->occurrences += occ;
    if (planted && s == slot) {
      if (!((want[col >> 6] >> (col & 63)) & 1u)) {
        printf("FAIL %s Q=%d slot=%d col=%d: the planted occurrence is not in the reference mask\n", what, Q, slot, col);
        return false;
      }
      n->chance += occ - 1;
    } else {
      n->chance += occ;
    }
  }
  return true;
}

template <int Q>
bool run(Rng& rng, Counts* n) {
  uint32_t p0[NS], p1[NS];
  for (int s = 0; s < NS; ++s) {
    p0[s] = rng.next() & ((1u << Q) - 1u);
    p1[s] = rng.next() & ((1u << Q) - 1u);
  }
  p1[NS - 2] = p0[NS - 2];  // a piece of two codes and one of plane 0 alone: the random planes below meet them by chance
  p1[NS - 1] = 0u;
  // every end column of every slot, planted into otherwise random planes
  for (int s = 0; s < NS; ++s) {
    for (int c = 0; c < 128; ++c) {
      Cols t;
      for (auto& pl : t.w)
        for (auto& w : pl) w = rng.next();
      for (int j = 0; j < Q; ++j) {
        t.set(0, c - (Q - 1 - j), (p0[s] >> j) & 1u);
        t.set(1, c - (Q - 1 - j), (p1[s] >> j) & 1u);
      }
      const bool reach_prev = c <= Q - 2, reach_a = c >= 64 && c <= 64 + Q - 2;
      const char* what = reach_prev ? "plant reaching back into the previous block" : reach_a ? "plant in b reaching back into a" : "plant";
      if (!check<Q>(t, p0, p1, what, s, c, n, true)) return false;
      ++n->plants;
      n->reach_prev += reach_prev;
      n->reach_a += reach_a;
    }
  }
  // random planes without plants: chance occurrences count too (short alphabets of planes make them frequent)
  for (int r = 0; r < 600; ++r) {
    Cols t;
    const uint32_t kind = r % 3;  // all four codes / two codes / one plane constant: denser chance occurrences
    for (int pl = 0; pl < 2; ++pl)
      for (auto& w : t.w[pl]) w = (kind == 2 && pl == 1) ? 0u : rng.next();
    if (kind == 1)
      for (int i = 0; i < 5; ++i) t.w[1][i] = t.w[0][i];
    if (!check<Q>(t, p0, p1, "random planes", -1, -1, n, false)) return false;
    ++n->random;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  Rng rng{0x9E3779B97F4A7C15ull ^ (argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x2545F4914F6CDD1Dull : 0ull)};
  Counts n;
  for (int rep = 0; rep < 2; ++rep) {
    if (!run<7>(rng, &n) || !run<8>(rng, &n) || !run<9>(rng, &n) || !run<10>(rng, &n) || !run<11>(rng, &n) || !run<12>(rng, &n)) return 1;
  }
  printf("ok plants=%ld reach_prev=%ld reach_a=%ld random=%ld occurrences=%ld chance=%ld\n", n.plants, n.reach_prev, n.reach_a, n.random, n.occurrences,
         n.chance);
  return 0;
}
