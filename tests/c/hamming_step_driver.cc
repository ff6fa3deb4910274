// hamming_step_driver.cc -- drives sassy_amd/csrc/hamming_step.h (the arithmetic of the Hamming search, free of HIP) on the
// host against brute force: the hit mask of a block over random slot masks for every m in 1 .. 200, 256, 257, 1024 and
// every k of the list below (all counter-plane boundaries), the N count through the same counter, the position mask, and
// the per-hit cost / N count / cigar writer.  Built by tests/test_hamming_cpu.py with -fsanitize=address,undefined.
//   hamming_step_driver <seed>   prints "ok cases=<n> hits=<n> emits=<n>", exit status 0; a mismatch: a line on stderr, 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sassy_amd/csrc/hamming_step.h"

using namespace sassy_hip;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

struct Case {
  uint32_t m, k, nslots;
  std::vector<std::vector<uint64_t>> masks;  // [slot][block 0 .. W]
  std::vector<uint32_t> rows;                // packed slots, 4 per word
  std::vector<uint8_t> slot_of;
};

template <int P, bool INVERT>
static uint64_t run(const Case& c, uint32_t k) {
  auto fetch = [&](uint32_t slot, uint32_t q) { return c.masks.at(slot).at(q); };  // (.at: a read outside the halo aborts)
  auto row_word = [&](uint32_t w) { return c.rows.at(w); };
  auto all_over = [](uint64_t over) { return over == ~(uint64_t)0; };
  return ham_hit_mask<P, INVERT>(fetch, row_word, c.m, k, all_over);
}
template <bool INVERT>
static uint64_t run_planes(const Case& c, uint32_t k, int planes) {
  switch (planes) {
    case 2: return run<2, INVERT>(c, k);
    case 4: return run<4, INVERT>(c, k);
    case 8: return run<8, INVERT>(c, k);
    default: return run<11, INVERT>(c, k);
  }
}

static int fail(const std::string& what) {
  fprintf(stderr, "MISMATCH %s\n", what.c_str());
  return 1;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  std::vector<uint32_t> ms;
  for (uint32_t m = 1; m <= 200; ++m) ms.push_back(m);
  ms.push_back(256); ms.push_back(257); ms.push_back(1024);
  uint64_t cases = 0, hits = 0, emits = 0;
  for (uint32_t m : ms) {
    const uint32_t ks[] = {0, 1, 2, 3, 4, 7, 8, 15, 16, 63, 64, 254, 255, 256, m - 1, m, m + 1};
    for (uint32_t k_in : ks) {
      if (k_in == 0xFFFFFFFFu) continue;
      const uint32_t k = k_in < m ? k_in : m;  // (the entry point's clamp: k >= m reports every start)
      Case c;
      c.m = m; c.k = k;
      c.nslots = 1 + (uint32_t)(rnd() % 8);
      const uint32_t W = ham_halo_blocks(m);
      if (W > kHamMaxHalo) return fail("halo of m=" + std::to_string(m));
      // a match density that puts H around k, so that both sides of the threshold occur
      double p = 1.0 - ((double)k + 0.5) / (double)m;
      p = p < 0.02 ? 0.02 : p > 0.98 ? 0.98 : p;
      c.masks.assign(c.nslots, std::vector<uint64_t>(W + 1, 0));
      for (auto& slot : c.masks)
        for (auto& w : slot)
          for (int b = 0; b < 64; ++b) w |= (uint64_t)(unit() < p) << b;
      c.slot_of.resize(m);
      c.rows.assign((m + 3) / 4, 0u);
      for (uint32_t j = 0; j < m; ++j) {
        c.slot_of[j] = (uint8_t)(rnd() % c.nslots);
        c.rows[j >> 2] |= (uint32_t)c.slot_of[j] << (8 * (j & 3));
      }
      uint64_t want = 0, want_n = 0;
      for (uint32_t i = 0; i < 64; ++i) {
        uint32_t h = 0;
        for (uint32_t j = 0; j < m; ++j) {
          const uint32_t at = i + j;
          h += !((c.masks[c.slot_of[j]][at >> 6] >> (at & 63)) & 1);
        }
        if (h <= k) want |= (uint64_t)1 << i;
        if (m - h <= k) want_n |= (uint64_t)1 << i;  // the matches counted instead (the N count's direction)
      }
      const uint64_t got = run_planes<true>(c, k, ham_planes(k));
      if (got != want) return fail("hit mask m=" + std::to_string(m) + " k=" + std::to_string(k));
      // every plane count that can hold k gives the same answer (saturation)
      for (int planes : {2, 4, 8, 11})
        if (k < (1u << planes) && run_planes<true>(c, k, planes) != want)
          return fail("planes=" + std::to_string(planes) + " m=" + std::to_string(m) + " k=" + std::to_string(k));
      if (run<kHamNPlanes, false>(c, k) != want_n) return fail("N count m=" + std::to_string(m) + " k=" + std::to_string(k));
      ++cases;
      hits += (uint64_t)__builtin_popcountll(want);
    }
    // the position mask: starts 64 b + i with 64 b + i + m <= n
    for (int rep = 0; rep < 40; ++rep) {
      const uint64_t block = rnd() % 5, n = rnd() % (5 * 64 + m + 2);
      uint64_t want = 0;
      for (uint32_t i = 0; i < 64; ++i)
        if (block * 64 + i + m <= n) want |= (uint64_t)1 << i;
      if (ham_valid_mask(block, n, m) != want) return fail("valid mask m=" + std::to_string(m) + " n=" + std::to_string(n));
    }
    // one hit: cost, N count, cigar, both directions, every profile
    const uint32_t profiles[] = {0, kHamDna, kHamIupac, kHamAsciiCi};
    for (uint32_t profile : profiles) {
      const char* alpha = profile == 0 ? "abAB" : profile == kHamAsciiCi ? "aAbB[{" : profile == kHamDna ? "ACGTNacgtn" : "ACGTNRYXacgtn";
      const size_t na = strlen(alpha);
      std::vector<uint8_t> pat(m), text(m);
      for (uint32_t j = 0; j < m; ++j) {
        pat[j] = (uint8_t)alpha[rnd() % na];
        text[j] = (rnd() % 3) ? pat[j] : (uint8_t)alpha[rnd() % na];
      }
      for (int minus = 0; minus < 2; ++minus) {
        std::vector<char> cigar(2 * m + 8, 0x7F);
        uint32_t cost = 0, n_count = 0, len = 0;
        ham_emit_hit(profile, pat.data(), m, [&](uint32_t i) { return (uint32_t)text.at(i); }, minus != 0, cigar.data(), &cost, &n_count,
                     &len);
        std::string want;
        uint32_t want_cost = 0, want_n = 0, run_len = 0;
        char op = 0;
        for (uint32_t j = 0; j <= m; ++j) {
          char o = 0;
          if (j < m) {
            const uint32_t i = minus ? m - 1 - j : j;
            bool eq;
            const uint8_t a = pat[i], b = text[i];
            if (profile == kHamDna) eq = ((a >> 1) & 3) == ((b >> 1) & 3);
            else if (profile == kHamIupac) eq = (ham_iupac_nib(a) & ham_iupac_nib(b)) != 0;
            else if (profile == kHamAsciiCi) eq = ((a >= 'A' && a <= 'Z') ? a + 32 : a) == ((b >= 'A' && b <= 'Z') ? b + 32 : b);
            else eq = a == b;
            want_cost += !eq;
            want_n += (b == 'N' || b == 'n');
            o = eq ? '=' : 'X';
          }
          if (o != op) {
            if (run_len) want += std::to_string(run_len) + op;
            op = o;
            run_len = 0;
          }
          ++run_len;
        }
        if (cost != want_cost || n_count != want_n || len != want.size() || std::string(cigar.data()) != want || len > 2 * m)
          return fail("emit m=" + std::to_string(m) + " profile=" + std::to_string(profile) + " minus=" + std::to_string(minus) + ": " +
                      std::string(cigar.data()) + " vs " + want);
        uint32_t c2 = 0, n2 = 0, l2 = 77;
        ham_emit_hit(profile, pat.data(), m, [&](uint32_t i) { return (uint32_t)text.at(i); }, minus != 0, nullptr, &c2, &n2, &l2);
        if (c2 != want_cost || n2 != want_n || l2 != 0) return fail("emit without cigar m=" + std::to_string(m));
        ++emits;
      }
    }
    // the N threshold: the largest count that passes the float rule
    for (float frac : {0.0f, 0.1f, 0.2f, 0.3f, 0.5f, 0.999f, 1.5f, -0.1f}) {
      int64_t want = -1;
      for (uint32_t cnt = 0; cnt <= m; ++cnt)
        if ((float)cnt / (float)m <= frac) want = cnt;
      if (ham_n_max(m, frac) != want) return fail("n_max m=" + std::to_string(m));
    }
  }
  printf("ok cases=%llu hits=%llu emits=%llu\n", (unsigned long long)cases, (unsigned long long)hits, (unsigned long long)emits);
  return 0;
}
