// relayout_step_driver.cc -- sassy_amd/csrc/relayout_step.h as a stand-alone host program (its own main, no HIP;
// tests/test_reads_relayout_cpu.py builds it with -fsanitize=address,undefined and runs it).
//
//   checks   rl_word_mask for every word and every [lo, hi) of a block, rl_segment against a byte-wise intersection,
//            rl_piece_bytes around `total`, rl_other_letter against the byte-wise acgt_only
//   a case   the destination of one relayout, block by block as the kernel makes it: rl_block per 64-byte block with a
//            16-byte load that refuses any piece outside the source buffer, unaligned, or without a byte of a read; the
//            kernel's stores (a whole 16-byte piece, or the last piece byte by byte) into a buffer of exactly `total` bytes
// usage: relayout_step_driver              prints "ok checks=.." and exits 0
//        relayout_step_driver CASE SRC OUT reads the case (text: "n_src first count total pad", n_src lines "src_start len",
//                                          count destination starts) and the source buffer, writes the destination's `total`
//                                          bytes to OUT, prints "ok blocks=.. loads=.."; a message and exit 1 on any refusal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sassy_amd/csrc/relayout_step.h"

using namespace sassy_hip;

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      fprintf(stderr, "line %d: ", __LINE__);  \
      fprintf(stderr, __VA_ARGS__);            \
      fprintf(stderr, "\n");                   \
      exit(1);                                 \
    }                                          \
  } while (0)

static uint64_t run_checks() {
  uint64_t count = 0;
  for (uint32_t lo = 0; lo <= 64; ++lo)
    for (uint32_t hi = 0; hi <= 64; ++hi)
      for (uint32_t j = 0; j < 16; ++j) {
        uint32_t want = 0;
        for (uint32_t i = 0; i < 4; ++i)
          if (4 * j + i >= lo && 4 * j + i < hi) want |= 0xFFu << (8 * i);
        CHECK(rl_word_mask(j, lo, hi) == want, "word mask %u [%u, %u)", j, lo, hi);
        ++count;
      }
  for (uint64_t pos : {0ull, 64ull, 4096ull})
    for (uint64_t start = 0; start < 4300; start += (start < 200 ? 1 : 97))
      for (uint64_t len : {0ull, 1ull, 15ull, 16ull, 17ull, 63ull, 64ull, 65ull, 200ull}) {
        uint32_t lo = 99, hi = 99;
        int64_t off = 0;
        const bool got = rl_segment(pos, start, len, &lo, &hi, &off);
        uint32_t wlo = 64, whi = 0;
        for (uint32_t i = 0; i < 64; ++i)
          if (pos + i >= start && pos + i < start + len) {
            if (wlo == 64) wlo = i;
            whi = i + 1;
          }
        CHECK(got == (wlo != 64), "segment: pos %llu start %llu len %llu", (unsigned long long)pos, (unsigned long long)start, (unsigned long long)len);
        if (got) CHECK(lo == wlo && hi == whi && off == (int64_t)pos - (int64_t)start, "segment bounds");
        ++count;
      }
  for (uint64_t total : {1ull, 15ull, 16ull, 17ull, 64ull, 100ull})
    for (uint64_t p = 0; p < 128; p += 16) {
      const uint64_t want = p >= total ? 0 : (total - p < 16 ? total - p : 16);
      CHECK(rl_piece_bytes(p, total) == want, "piece bytes");
      ++count;
    }
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t at = 0; at < 4; ++at)
      for (uint32_t keep = 0; keep <= 4; ++keep) {
        const uint32_t w = 0x41414141u ^ ((0x41u ^ c) << (8 * at));  // 'A' everywhere but byte `at`
        const uint32_t u = c & ~0x20u;
        const bool other = !(u == 'A' || u == 'C' || u == 'G' || u == 'T');
        CHECK(rl_other_letter(w, keep) == (other && at < keep), "other letter %u at %u keep %u", c, at, keep);
        ++count;
      }
  return count;
}

static std::vector<uint8_t> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f, "cannot open %s", path);
  std::vector<uint8_t> out;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return out;
}

static int run_case(const char* case_path, const char* src_path, const char* out_path) {
  FILE* f = fopen(case_path, "r");
  CHECK(f, "cannot open %s", case_path);
  unsigned long long n_src, first, count, total, pad;
  CHECK(fscanf(f, "%llu %llu %llu %llu %llu", &n_src, &first, &count, &total, &pad) == 5, "case header");
  std::vector<uint64_t> src_start(n_src), src_len(n_src), dst_start(count);
  for (size_t r = 0; r < n_src; ++r) {
    unsigned long long a, b;
    CHECK(fscanf(f, "%llu %llu", &a, &b) == 2, "source table");
    src_start[r] = a;
    src_len[r] = b;
  }
  for (size_t i = 0; i < count; ++i) {
    unsigned long long a;
    CHECK(fscanf(f, "%llu", &a) == 1, "destination table");
    dst_start[i] = a;
  }
  fclose(f);
  CHECK(first + count <= n_src, "range outside the source");
  const std::vector<uint8_t> src = read_file(src_path);
  CHECK(src.size() % 64 == 0, "the source buffer ends at a multiple of 64");
  uint64_t loads = 0;
  auto load16 = [&](int64_t a, uint32_t* w4) {
    CHECK(a >= 0 && a % 16 == 0 && (uint64_t)a + 16 <= src.size(), "load at %lld outside the source of %zu bytes", (long long)a, src.size());
    bool in_read = false;  // the piece holds a byte of a read of the range
    for (uint64_t r = first; r < first + count && !in_read; ++r)
      in_read = src_start[r] < (uint64_t)a + 16 && src_start[r] + src_len[r] > (uint64_t)a;
    CHECK(in_read, "load at %lld touches no read", (long long)a);
    memcpy(w4, src.data() + a, 16);
    ++loads;
  };
  std::vector<uint8_t> dst(total);  // exactly: a store behind `total` is the sanitizer's
  const uint64_t n_blocks = (total + 63) / 64;
  for (uint64_t b = 0; b < n_blocks; ++b) {
    uint32_t out[16];
    rl_block(load16, [&](uint32_t i) { return dst_start[i]; }, [&](uint32_t i) { return src_len[first + i]; },
             [&](uint32_t i) { return src_start[first + i]; }, (uint32_t)count, b, (uint8_t)pad, out);
    for (int j = 0; j < 4; ++j) {
      const uint64_t p = b * 64 + 16u * j;
      const uint32_t have = rl_piece_bytes(p, total);
      if (have == 16u) memcpy(dst.data() + p, &out[4 * j], 16);
      else
        for (uint32_t q = 0; q < have; ++q) dst[p + q] = (uint8_t)(out[4 * j + (q >> 2)] >> (8u * (q & 3u)));
    }
  }
  FILE* o = fopen(out_path, "wb");
  CHECK(o, "cannot open %s", out_path);
  CHECK(dst.empty() || fwrite(dst.data(), 1, dst.size(), o) == dst.size(), "short write");
  fclose(o);
  printf("ok blocks=%llu loads=%llu\n", (unsigned long long)n_blocks, (unsigned long long)loads);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4) return run_case(argv[1], argv[2], argv[3]);
  printf("ok checks=%llu\n", (unsigned long long)run_checks());
  return 0;
}
