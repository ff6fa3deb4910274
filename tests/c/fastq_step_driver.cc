// fastq_step_driver.cc -- sassy_amd/csrc/fastq_step.h against a byte-wise parse, as a stand-alone host program (its own main,
// no HIP; tests/test_fastq_reads_cpu.py builds it with -fsanitize=address,undefined and runs it).
//
//   lanes      the lane shapes written out -- newlines at bit 0, at bit 63 and at both, len in {0, 1, 63, 64}, "\r\n" inside a
//              lane and across a lane border, a '\r'-only line, a last line without '\n' -- and random lanes over
//              {A, @, +, '\n', '\r'} at every length and both outside bits, each with every carried class 0 .. 3: the byte
//              masks, line starts, stripped bytes, the line and class of every start and of every stripped byte
//   combines   whole inputs cut into lanes, tiles and super-tiles at random sizes: the counts summed level by level (32-bit
//              below, 64-bit on top) put every line start at its line; the lengths from consecutive starts, the verdict and
//              the record fields equal the byte-wise parse
//   layouts    the layout scan with empty reads first, last and in runs; a block of the layout from every source alignment
//              and every kept length against a byte copy
// usage: fastq_step_driver SEED        prints "ok lanes=.. combines=.. layouts=.." and exits 0, or a message and exits 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sassy_amd/csrc/fastq_step.h"

using namespace sassy_hip;

static uint64_t g_state = 1;
static uint64_t rnd() {  // splitmix64
  uint64_t x = (g_state += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      fprintf(stderr, "line %d: ", __LINE__);  \
      fprintf(stderr, __VA_ARGS__);            \
      fprintf(stderr, "\n");                   \
      exit(1);                                 \
    }                                          \
  } while (0)

typedef std::vector<uint8_t> Bytes;

static Bytes random_bytes(size_t n, uint32_t special) {
  Bytes b(n);
  for (size_t i = 0; i < n; ++i) b[i] = below(64) < special ? (uint8_t)"\n\n\r@+"[below(5)] : (uint8_t)'A';
  return b;
}

// ---- the definition, byte by byte
struct Line {
  uint64_t start, len;  // len without the line end
  bool cr;              // it lost a '\r'
  uint64_t cr_at;
};
static std::vector<Line> brute_lines(const Bytes& t) {
  std::vector<Line> out;
  const size_t n = t.size();
  size_t at = 0;
  while (at < n) {
    size_t e = at;
    while (e < n && t[e] != '\n') ++e;
    Line l{at, e - at, false, 0};
    if (l.len && t[e - 1] == '\r') {
      l.cr = true;
      l.cr_at = e - 1;
      --l.len;
    }
    out.push_back(l);
    at = e + 1;
  }
  return out;
}
static FastqVerdict brute_verdict(const Bytes& t, const std::vector<Line>& lines) {
  for (size_t r = 0; 4 * r < lines.size(); ++r) {
    const Line& a = lines[4 * r];
    if (!(a.len && t[a.start] == '@')) return FastqVerdict{r, kFqNoAt};
    if (4 * r + 3 >= lines.size()) return FastqVerdict{r, kFqShort};
    const Line& p = lines[4 * r + 2];
    if (!(p.len && t[p.start] == '+')) return FastqVerdict{r, kFqNoPlus};
  }
  return FastqVerdict{0, kFqOk};
}

static void lane_words(const Bytes& t, size_t base, uint32_t (&w)[16]) {
  uint8_t b[64] = {};
  for (size_t i = 0; i < 64 && base + i < t.size(); ++i) b[i] = t[base + i];
  memcpy(w, b, 64);
}
struct LaneIn {
  uint64_t nl, cr, at, plus;
  uint32_t len;
  bool prev, next;
};
static LaneIn lane_in(const Bytes& t, size_t base) {
  const size_t n = t.size();
  uint32_t w[16];
  lane_words(t, base, w);
  LaneIn L;
  L.len = base >= n ? 0u : (uint32_t)(n - base < 64 ? n - base : 64);
  const uint64_t valid = fq_below(L.len);
  L.nl = fq_eq_bits64(w, '\n') & valid;
  L.cr = fq_eq_bits64(w, '\r') & valid;
  L.at = fq_eq_bits64(w, '@') & valid;
  L.plus = fq_eq_bits64(w, '+') & valid;
  L.prev = base == 0 || t[base - 1] == '\n';
  L.next = base + 64 >= n || t[base + 64] == '\n';
  for (uint32_t i = 0; i < L.len; ++i) {
    const uint8_t c = t[base + i];
    CHECK(((L.nl >> i) & 1) == (c == '\n') && ((L.cr >> i) & 1) == (c == '\r') && ((L.at >> i) & 1) == (c == '@') && ((L.plus >> i) & 1) == (c == '+'),
          "byte masks at %u", i);
  }
  return L;
}

// one lane of t at `base` against the byte-wise lines; every carried class by shifting the line numbers
static void check_lane(const Bytes& t, size_t base) {
  const std::vector<Line> lines = brute_lines(t);
  const LaneIn in = lane_in(t, base);
  const FastqLane L = fq_lane(in.nl, in.cr, in.len, in.prev, in.next);
  uint64_t ls = 0, strip = 0, front = 0;
  for (size_t j = 0; j < lines.size(); ++j) {
    if (lines[j].start < base) ++front;
    else if (lines[j].start < base + 64) ls |= 1ull << (lines[j].start - base);
    if (lines[j].cr && lines[j].cr_at >= base && lines[j].cr_at < base + 64) strip |= 1ull << (lines[j].cr_at - base);
  }
  CHECK(L.ls == ls, "line starts %llx != %llx (base %zu of %zu)", (unsigned long long)L.ls, (unsigned long long)ls, base, t.size());
  CHECK(L.strip == strip, "stripped %llx != %llx (base %zu of %zu)", (unsigned long long)L.strip, (unsigned long long)strip, base, t.size());
  CHECK(fq_count(L) == fq_popc(ls), "count");
  for (uint64_t carried = 0; carried < 4; ++carried) {
    const uint64_t f = front + carried;
    for (size_t j = 0; j < lines.size(); ++j) {
      if (lines[j].start >= base && lines[j].start < base + 64) {
        const uint64_t line = fq_line_of_start(L, f, (uint32_t)(lines[j].start - base));
        CHECK(line == j + carried && fq_class(line) == ((j + carried) & 3), "line of start");
      }
      if (lines[j].cr && lines[j].cr_at >= base && lines[j].cr_at < base + 64)
        CHECK(fq_line_of_byte(L, f, (uint32_t)(lines[j].cr_at - base)) == j + carried, "line of stripped byte");
    }
  }
}

static Bytes bytes_of(const std::string& s) { return Bytes(s.begin(), s.end()); }

static uint64_t run_lanes() {
  uint64_t count = 0;
  // the shapes, each at every length that cuts the input inside or behind the lane under test (lane 1 of three)
  const std::string a63(63, 'A'), a62(62, 'A'), a64(64, 'A');
  const std::vector<std::string> shapes = {
      a64 + "\n" + a62 + "\n" + a64,                      // newlines at bit 0 and bit 63
      a64 + "\n" + a63 + a64,                             // bit 0 only
      a64 + a63 + "\n" + a64,                             // bit 63 only
      a63 + "\n" + a63 + "\n" + "\n" + a63,               // the lane in front ends with '\n', the lane behind begins with one
      a64 + a62 + "\r\n" + a64,                           // "\r\n" at bits 62, 63
      a64 + a63 + "\r" + "\n" + a63,                      // '\r' the lane's last byte, '\n' the next lane's first
      a63 + "\r" + "\n" + a63 + a64,                      // the same one lane earlier: '\n' at bit 0
      a64 + "AA\r\nAA\n\r\n\r\r\nA\rA\n" + a64,           // inside a lane: "\r\n", a '\r'-only line, "\r\r\n", a '\r' that stays
      a64 + a63 + "\r",                                   // the input's last line has no '\n' and ends in '\r' at bit 63
      a64 + "A\r",                                        // ... at bit 1 (len 2)
      a64 + "\r",                                         // len 1, a '\r'-only last line
      a64 + "\n",                                         // len 1
      a64,                                                // len 0
  };
  for (const std::string& s : shapes) {
    const Bytes whole = bytes_of(s);
    for (size_t n : {whole.size(), (size_t)64, (size_t)65, (size_t)127, (size_t)128, (size_t)129}) {
      if (n > whole.size()) continue;
      const Bytes t(whole.begin(), whole.begin() + (long)n);
      for (size_t base = 0; base <= n; base += 64) {  // (base == n: a lane of len 0 behind the input)
        check_lane(t, base);
        ++count;
      }
    }
  }
  // random: three lanes, the middle one under test at every length 0 .. 64
  for (uint32_t special : {1u, 4u, 16u, 40u, 64u})
    for (uint32_t len = 0; len <= 64; ++len)
      for (int rep = 0; rep < 4; ++rep) {
        const Bytes t = random_bytes(64 + len + (len == 64 ? below(3) : 0), special);
        check_lane(t, 64);
        check_lane(t, 0);
        count += 2;
      }
  return count;
}

// a whole input through the passes as the kernels run them, with `tile` lanes per tile and `super` tiles per super-tile
static void pipeline(const Bytes& t, uint32_t tile, uint32_t super) {
  const size_t n = t.size();
  const std::vector<Line> lines = brute_lines(t);
  const size_t n_lanes = (n + 63) / 64, n_tiles = (n_lanes + tile - 1) / tile, n_super = (n_tiles + super - 1) / super;
  std::vector<FastqLane> L(n_lanes);
  std::vector<LaneIn> in(n_lanes);
  for (size_t l = 0; l < n_lanes; ++l) {
    in[l] = lane_in(t, 64 * l);
    L[l] = fq_lane(in[l].nl, in[l].cr, in[l].len, in[l].prev, in[l].next);
  }
  // count: per tile the starts in front of it inside its super-tile, per super-tile its own; scan: 64-bit
  std::vector<uint32_t> tile_pre(n_tiles), super_sum(n_super, 0);
  for (size_t s = 0; s < n_super; ++s) {
    uint32_t run = 0;
    for (size_t tt = s * super; tt < (s + 1) * super && tt < n_tiles; ++tt) {
      tile_pre[tt] = run;
      for (size_t l = tt * tile; l < (tt + 1) * tile && l < n_lanes; ++l) run += fq_count(L[l]);
    }
    super_sum[s] = run;
  }
  std::vector<uint64_t> super_pre(n_super + 1, 0);
  for (size_t s = 0; s < n_super; ++s) super_pre[s + 1] = super_pre[s] + super_sum[s];
  const uint64_t n_lines = super_pre[n_super];
  CHECK(n_lines == lines.size(), "%llu lines, %zu by bytes", (unsigned long long)n_lines, lines.size());
  // lines
  std::vector<uint64_t> line_start(n_lines, ~0ull);
  std::vector<uint8_t> line_cr(n_lines, 0);
  uint64_t bad = ~0ull;
  for (size_t tt = 0; tt < n_tiles; ++tt) {
    uint64_t front = fq_front(super_pre[tt / super], tile_pre[tt]);
    for (size_t l = tt * tile; l < (tt + 1) * tile && l < n_lanes; ++l) {
      for (uint64_t m = L[l].ls; m; m &= m - 1) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        const uint64_t line = fq_line_of_start(L[l], front, i);
        CHECK(line < n_lines && line_start[line] == ~0ull, "line %llu twice or out of range", (unsigned long long)line);
        line_start[line] = 64 * l + i;
        const uint32_t cls = fq_class(line);
        const bool ok = cls == 0 ? ((in[l].at >> i) & 1) != 0 : cls == 2 ? ((in[l].plus >> i) & 1) != 0 : true;
        if (!ok && line < bad) bad = line;
      }
      for (uint64_t m = L[l].strip; m; m &= m - 1) {
        const uint64_t line = fq_line_of_byte(L[l], front, (uint32_t)__builtin_ctzll(m));
        CHECK(line < n_lines && !line_cr[line], "a line strips twice");
        line_cr[line] = 1;
      }
      front += fq_count(L[l]);
    }
  }
  const uint64_t virt = fq_virtual_start(n, n && t[n - 1] == '\n');
  for (size_t j = 0; j < lines.size(); ++j) {
    CHECK(line_start[j] == lines[j].start, "start of line %zu", j);
    // (a marker line that is empty has no byte to test: its start holds the line end, which is no marker)
    const uint64_t len = fq_line_len(line_start[j], j + 1 < lines.size() ? line_start[j + 1] : virt, line_cr[j] != 0);
    CHECK(len == lines[j].len && (line_cr[j] != 0) == lines[j].cr, "line %zu: length %llu, by bytes %llu", j, (unsigned long long)len,
          (unsigned long long)lines[j].len);
  }
  const FastqVerdict want = brute_verdict(t, lines), got = fq_verdict(n_lines, bad);
  CHECK(want.rule == got.rule && (want.rule == kFqOk || want.record == got.record), "verdict %u at %llu, by bytes %u at %llu", got.rule,
        (unsigned long long)got.record, want.rule, (unsigned long long)want.record);
}

static Bytes random_fastq(uint32_t n_rec, bool crlf_some) {
  std::string s;
  for (uint32_t r = 0; r < n_rec; ++r) {
    const uint32_t len = below(8) == 0 ? 0 : below(150);
    const char* eol[4];
    for (auto& e : eol) e = crlf_some && below(3) == 0 ? "\r\n" : "\n";
    s += "@" + std::string(below(12), 'i') + eol[0] + std::string(len, "ACGTN@+\r"[below(8)]) + eol[1] + "+" + (below(2) ? "x" : "") + eol[2] +
         std::string(len, "I@+"[below(3)]) + eol[3];
  }
  return bytes_of(s);
}

static uint64_t run_combines() {
  uint64_t count = 0;
  for (int rep = 0; rep < 60; ++rep) {
    Bytes t = rep % 3 == 0 ? random_bytes(below(3000), 1 + below(40)) : random_fastq(1 + below(40), rep % 2 == 0);
    if (rep % 3 == 1 && t.size() > 4) {  // damage: cut the tail, or change one byte
      if (below(2)) t.resize(t.size() - 1 - below((uint32_t)t.size() / 2));
      else t[below((uint32_t)t.size())] = (uint8_t)"A\n@+"[below(4)];
    }
    if (rep % 3 == 2 && below(2) && !t.empty() && t.back() == '\n') t.pop_back();  // no final newline
    pipeline(t, 1 + below(8), 1 + below(5));
    pipeline(t, 64, 16);
    count += 2;
  }
  pipeline(Bytes(), 64, 16);
  pipeline(bytes_of("@"), 64, 16);
  pipeline(bytes_of("@\n\n+\n\n"), 64, 16);
  pipeline(bytes_of("@a\nAC\n+\nII\n\n"), 64, 16);
  return count + 4;
}

static uint64_t run_layouts() {
  uint64_t count = 0;
  const std::vector<std::vector<uint64_t>> cases = {
      {}, {0}, {0, 0, 0}, {0, 5, 0}, {0, 0, 64, 0, 0, 65, 0}, {1, 63, 64, 65, 0, 0, 0}, {4097, 0, 0, 1, 0}, {0, 0, 0, 128},
  };
  for (const auto& lens : cases) {
    std::vector<uint64_t> starts(lens.size() + 1, 7);
    const uint64_t total = fq_layout(lens.data(), lens.size(), starts.data());
    uint64_t at = 0;
    for (size_t r = 0; r < lens.size(); ++r) {
      CHECK(starts[r] == at && at % 64 == 0, "start of read %zu", r);
      at += (lens[r] + 63) / 64 * 64;
    }
    CHECK(total == at && starts[lens.size()] == 7, "layout bytes");
    ++count;
  }
  for (int rep = 0; rep < 40; ++rep) {
    std::vector<uint64_t> lens(1 + below(50));
    for (auto& l : lens) l = below(3) == 0 ? 0 : below(300);
    std::vector<uint64_t> starts(lens.size());
    const uint64_t total = fq_layout(lens.data(), lens.size(), starts.data());
    for (size_t r = 0; r + 1 < lens.size(); ++r) CHECK(starts[r + 1] == starts[r] + fq_round64(lens[r]), "scan");
    CHECK(total == starts.back() + fq_round64(lens.back()), "total");
    ++count;
  }
  // a block from every source alignment and kept length
  Bytes src(96);
  for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(1 + i * 7 % 251);
  for (uint32_t shift = 0; shift < 16; ++shift)
    for (uint32_t keep = 0; keep <= 64; ++keep) {
      uint32_t w[20], out[16];
      memcpy(w, src.data(), 80);
      fq_shift_block(w, shift, keep, out);
      uint8_t got[64], want[64] = {};
      memcpy(got, out, 64);
      memcpy(want, src.data() + shift, keep);
      CHECK(memcmp(got, want, 64) == 0, "block at shift %u, keep %u", shift, keep);
      ++count;
    }
  return count;
}

int main(int argc, char** argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const uint64_t lanes = run_lanes(), combines = run_combines(), layouts = run_layouts();
  printf("ok lanes=%llu combines=%llu layouts=%llu\n", (unsigned long long)lanes, (unsigned long long)combines, (unsigned long long)layouts);
  return 0;
}
