// Drives sassy_amd/csrc/pass_lds.h (plain C++, no HIP): every (members, source, piece length) of the shared pass's fused
// launches, and what each layout must keep: see tests/test_pass_lds_cpu.py.  Every range is also written and read back in
// a buffer of exactly the bytes per wave (built with -fsanitize=address,undefined: a range outside it is a report).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/pass_lds.h"

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

// the layout is usable in constant expressions (the kernel's static_asserts take it from there)
static_assert(pass_lds_per_wave(2, kPlaneRaw, 192u) == 11296u && pass_lds_per_wave(2, kPlaneWrite, 192u) == 11296u, "today's grouped launch");
static_assert(pass_lds_per_wave(2, kPlaneRead, 192u) == 10016u, "the compact reader");

int main() {
  const uint32_t cap = kPassLdsQueueCap;
  CHECK(cap == 192u, "queue capacity %u", cap);
  long ranges = 0, cases = 0;
  for (int members = 1; members <= 2; ++members)
    for (int src : {(int)kPlaneRaw, (int)kPlaneWrite, (int)kPlaneRead})
      for (int q = 7; q <= 12; ++q) {
        ++cases;
        const uint32_t per_wave = pass_lds_per_wave(members, src, cap);
        struct Named { const char* name; LdsRange r; };
        std::vector<Named> rs = {{"dp", pass_lds_dp(members, src)}, {"state", pass_lds_state(members, src)}};
        for (int g = 0; g < members; ++g) {
          rs.push_back({g ? "queue1" : "queue0", pass_lds_queue(members, src, cap, g)});
          rs.push_back({g ? "count1" : "count0", pass_lds_count(members, src, cap, g)});
        }
        std::vector<uint8_t> wave(per_wave, 0);  // (exactly the launch's bytes per wave)
        for (size_t i = 0; i < rs.size(); ++i) {
          const LdsRange r = rs[i].r;
          ++ranges;
          CHECK(r.begin < r.end, "%s empty (members %d src %d)", rs[i].name, members, src);
          CHECK(r.begin % 16u == 0 && r.end % 16u == 0, "%s [%u, %u) not 16-byte aligned (members %d src %d)", rs[i].name, r.begin, r.end, members, src);
          CHECK(r.end <= per_wave, "%s ends at %u behind the wave's %u bytes (members %d src %d)", rs[i].name, r.end, per_wave, members, src);
          for (size_t j = 0; j < i; ++j)
            CHECK(r.end <= rs[j].r.begin || rs[j].r.end <= r.begin, "%s [%u, %u) overlaps %s [%u, %u) (members %d src %d)", rs[i].name, r.begin,
                  r.end, rs[j].name, rs[j].r.begin, rs[j].r.end, members, src);
          for (uint32_t b = r.begin; b < r.end; ++b) {
            CHECK(wave[b] == 0, "%s: byte %u written twice", rs[i].name, b);
            wave[b] = (uint8_t)(i + 1);
          }
        }
        // what the kernel relies on: sizes of the ranges, their order, the count behind its queue
        // (four masks and four words of carries; the one-member staging launch keeps room for eight of either)
        CHECK(pass_lds_dp(members, src).begin == 0 && pass_lds_dp(members, src).end == (members == 2 || src == kPlaneRead ? 4096u : 6144u), "dp");
        const LdsRange st = pass_lds_state(members, src);
        CHECK(st.end - st.begin == (members == 2 ? 11u : 7u) * 256u, "state rows");
        CHECK(st.begin == pass_lds_dp(members, src).end, "state at the end of the carries");
        for (int g = 0; g < members; ++g) {
          const LdsRange qu = pass_lds_queue(members, src, cap, g), co = pass_lds_count(members, src, cap, g);
          CHECK(qu.end - qu.begin == cap * 8u && co.begin == qu.end && co.end - co.begin == 16u, "queue %d", g);
          CHECK(qu.begin == pass_lds_queues(members, src) + (uint32_t)g * pass_lds_queue_stride(cap), "queue %d at", g);
          CHECK(qu.begin >= st.end, "queue %d in front of the state", g);
        }
        CHECK(pass_lds_count(members, src, cap, members - 1).end == per_wave, "bytes behind the last count");
        const uint32_t group = pass_lds_per_group(members, src, cap, q);
        CHECK(group == 4u * per_wave + (members == 2 ? (uint32_t)q * 64u : 0u), "workgroup bytes");
        if (src != kPlaneRead) {  // text-staging launches: today's layout, bit for bit
          CHECK(pass_lds_queues(members, src) == 8192u, "queues behind the tile");
          CHECK(st.begin == (members == 2 ? 4096u : 6144u) && st.end <= 8192u, "state inside the tile");
          CHECK(per_wave == (members == 2 ? 11296u : 9744u), "per wave %u", per_wave);
          if (members == 2) CHECK(4u * per_wave == 45184u, "per workgroup %u", 4u * per_wave);
        } else {  // the reader: queues at the state's end; four workgroups per CU with the table
          CHECK(pass_lds_queues(members, src) == st.end, "queues behind the state");
          CHECK(per_wave == (members == 2 ? 10016u : 7440u), "per wave %u", per_wave);
          CHECK(group <= 40960u && 4u * group <= kPassLdsCuBytes, "reader workgroup %u bytes at q %d", group, q);
        }
      }
  printf("ok cases=%ld ranges=%ld\n", cases, ranges);
  return 0;
}
