// reads_gate_driver.cc -- sassy_amd/csrc/reads_gate.h alone, on the host: the shared refusals of the read-batch calls in
// their order, for one handle and for two, and the bounded read length against its definition.  A stand-alone program (its
// own main, no HIP); built by tests/test_reads_front_cpu.py with -fsanitize=address,undefined.
//   reads_gate_driver    prints "ok refusals=<n> lengths=<n>", exit status 0; a message and exit status 1 on any difference
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../sassy_amd/csrc/reads_gate.h"

using namespace sassy_hip;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// everything wrong at once: taking the faults away one at a time from the front shows each refusal in its place
static unsigned walk(uint32_t handles) {
  unsigned n = 0;
  ReadsGate g{};
  g.handles = handles;
  g.profile = 0; g.overhang = g.only_best = g.max_n_frac = true;
  g.handle_read = true; g.device_s = 1; g.in_flight = true;
  for (uint32_t h = 0; h < 2; ++h) { g.have_reads[h] = false; g.device_r[h] = 0; g.longest[h] = 513; }
  const auto searcher = [&](ReadsRefusal want) { CHECK(reads_gate_searcher(g) == want); ++n; };
  const auto in_handles = [&](ReadsRefusal want) { CHECK(reads_gate_handles(g) == want); ++n; };
  searcher(kRdsAscii); g.profile = kHamAsciiCi;
  searcher(kRdsAscii); g.profile = kHamIupac;
  searcher(kRdsOverhang); g.overhang = false;
  searcher(kRdsOnlyBest); g.only_best = false;
  searcher(kRdsNFrac); g.max_n_frac = false;
  for (uint32_t h = 0; h < handles; ++h) { searcher(kRdsNullReads); g.have_reads[h] = true; }
  searcher(kRdsOk);  // (a second handle that a one-handle call does not have is not asked for)
  g.profile = kHamDna;
  searcher(kRdsOk);
  // the handles: nothing of them is judged before they are read; then every device before any length
  g.handle_read = false;
  in_handles(kRdsOk);
  g.handle_read = true;
  for (uint32_t h = 0; h < handles; ++h) { in_handles(kRdsDevice); g.device_r[h] = 1; }
  for (uint32_t h = 0; h < handles; ++h) { in_handles(kRdsTooLong); g.longest[h] = 512; }
  in_handles(kRdsOk);
  g.device_s = 0;
  in_handles(kRdsDevice);
  g.device_s = 1;
  // the tickets are a part of their own: neither predicate above looks at them
  CHECK(reads_gate_tickets(g) == kRdsInFlight); ++n;
  g.in_flight = false;
  CHECK(reads_gate_tickets(g) == kRdsOk); ++n;
  return n;
}

static unsigned lengths() {
  unsigned n = 0;
  const uint64_t starts[] = {0, 64, 448, 511, 512, 513, ~0ull - 3, ~0ull};
  const uint64_t lens[] = {0, 1, 63, 64, 65, 511, 512, 513, 1ull << 32, (1ull << 32) + 5, ~0ull};
  const uint64_t sizes[] = {0, 64, 512, 576, 1ull << 33};
  for (uint64_t max_len : {64ull, 512ull})
    for (uint64_t bytes : sizes)
      for (uint64_t start : starts)
        for (uint64_t len : lens) {
          // the definition, without a subtraction that could wrap: the read lies in [0, bytes) and is at most max_len long
          bool fits = len <= max_len && start <= bytes;
          for (uint64_t i = 0; fits && i < len; ++i) fits = start + i < bytes;
          CHECK(reads_fit_len(start, len, bytes, max_len) == (fits ? (uint32_t)len : 0u));
          ++n;
        }
  return n;
}

int main() {
  const unsigned refusals = walk(1) + walk(2);
  printf("ok refusals=%u lengths=%u\n", refusals, lengths());
  return 0;
}
