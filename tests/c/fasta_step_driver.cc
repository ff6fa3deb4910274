// fasta_step_driver.cc -- sassy_amd/csrc/fasta_step.h against a byte-by-byte brute force, as a stand-alone host program (its
// own main, no HIP; tests/test_fasta_unwrap_cpu.py builds it with -fsanitize=address,undefined and runs it).
//
//   lanes      random 64-byte lanes over {A, '\n', '\r', '>'} at densities from one special byte per lane to all special, every
//              length 0 .. 64, every carry-in state, the byte in front '\n' or not, the byte behind '\n' / end or not: line
//              starts, header starts, the in-header mask, the kept mask and the summary against the definition
//   combines   a 4 KiB buffer cut at random places: the summaries of the pieces, combined left to right and in a random
//              bracketing, equal the summary of the whole; applied to either carried state they give the brute-force counts
//   pipelines  whole inputs through the passes as the kernels run them -- lane summaries, tile prefixes, the scan, the record
//              table, every kept byte's destination -- against the line-by-line parse
// usage: fasta_step_driver SEED        prints "ok lanes=.. combines=.. pipelines=.." and exits 0, or a message and exits 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sassy_amd/csrc/fasta_step.h"

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

// bytes over the alphabet; `special` of 64 positions on average hold one of '\n' '\r' '>'
static std::vector<uint8_t> random_bytes(size_t n, uint32_t special) {
  std::vector<uint8_t> b(n);
  for (size_t i = 0; i < n; ++i) {
    if (below(64) < special) b[i] = (uint8_t)"\n\r>"[below(3)];
    else b[i] = 'A';
  }
  return b;
}

// ---- the definition, byte by byte, over a stretch [a, b) of an input of n bytes.  `in`: the line open at a is a header (read
// only in front of the stretch's first line start)
struct Brute {
  std::vector<uint8_t> ls, hs, hdr, kept;
};
static Brute brute(const std::vector<uint8_t>& t, size_t a, size_t b, bool in) {
  const size_t n = t.size();
  Brute r;
  bool state = in;
  for (size_t p = a; p < b; ++p) {
    const bool ls = p == 0 || t[p - 1] == '\n';
    const bool hs = ls && t[p] == '>';
    if (ls) state = hs;
    const bool drop = t[p] == '\n' || (t[p] == '\r' && (p + 1 == n || t[p + 1] == '\n'));
    r.ls.push_back(ls);
    r.hs.push_back(hs);
    r.hdr.push_back(state);
    r.kept.push_back(!state && !drop);
  }
  return r;
}

static FastaLane lane_of(const std::vector<uint8_t>& t, size_t base) {
  const size_t n = t.size();
  const uint32_t len = base >= n ? 0u : (uint32_t)(n - base < 64 ? n - base : 64);
  uint64_t nl = 0, gt = 0, cr = 0;
  for (uint32_t i = 0; i < len; ++i) {
    nl |= (uint64_t)(t[base + i] == '\n') << i;
    gt |= (uint64_t)(t[base + i] == '>') << i;
    cr |= (uint64_t)(t[base + i] == '\r') << i;
  }
  const bool prev = base == 0 || (base - 1 < n && t[base - 1] == '\n');
  const bool next = base + 64 >= n || t[base + 64] == '\n';
  return fa_lane(nl, gt, cr, len, prev, next);
}

static FastaSum64 brute_summary(const std::vector<uint8_t>& t, size_t a, size_t b) {
  FastaSum64 s = fa_identity<uint64_t>();
  const Brute r = brute(t, a, b, false);
  bool seen = false;
  for (size_t i = 0; i < b - a; ++i) {
    if (r.ls[i]) { seen = true; s.has_ls = 1; s.last_hdr = r.hs[i]; }
    s.n_hdr += r.hs[i];
    const bool drop = t[a + i] == '\n' || (t[a + i] == '\r' && (a + i + 1 == t.size() || t[a + i + 1] == '\n'));
    if (!seen) s.kept_pre += !drop;
    else s.kept_post += r.kept[i];
  }
  return s;
}
template <typename A, typename B>
static bool same(const FastaSumT<A>& x, const FastaSumT<B>& y) {
  return x.has_ls == y.has_ls && x.last_hdr == y.last_hdr && (uint64_t)x.kept_pre == (uint64_t)y.kept_pre &&
         (uint64_t)x.kept_post == (uint64_t)y.kept_post && (uint64_t)x.n_hdr == (uint64_t)y.n_hdr;
}

static uint64_t test_lanes() {
  uint64_t done = 0;
  for (uint32_t special = 1; special <= 64; special = special < 8 ? special + 1 : special * 2)
    for (int rep = 0; rep < 300; ++rep) {
      // the lane sits at offset 64 of a 3-lane input, or ends the input after `len` bytes
      const uint32_t len = rep % 3 == 0 ? below(65) : 64;
      std::vector<uint8_t> t = random_bytes(64 + len + (len == 64 ? below(2) * (1 + below(64)) : 0), special);
      if (rep % 5 == 0 && t.size() > 63) t[63] = '\n';
      if (rep % 7 == 0 && t.size() > 128) t[128] = '\n';
      if (rep % 11 == 0 && len > 0) t[64 + len - 1] = '\r';
      const FastaLane L = lane_of(t, 64);
      for (int in = 0; in < 2; ++in) {
        const Brute r = brute(t, 64, 64 + len, in != 0);
        const uint64_t hdr = fa_in_header(L.ls, L.hs, in != 0), kept = fa_kept(L, in != 0);
        for (uint32_t i = 0; i < len; ++i) {
          CHECK(((L.ls >> i) & 1) == r.ls[i], "line start %u", i);
          CHECK(((L.hs >> i) & 1) == r.hs[i], "header start %u", i);
          CHECK(((hdr >> i) & 1) == r.hdr[i], "in header %u (in %d)", i, in);
          CHECK(((kept >> i) & 1) == r.kept[i], "kept %u (in %d, len %u)", i, in, len);
        }
        CHECK(len == 64 || (L.ls >> len) == 0, "line start bits behind the input");
        CHECK(len == 64 || (kept >> len) == 0, "kept bits behind the input");
        const FastaSum s = fa_summary(L);
        CHECK(same(s, brute_summary(t, 64, 64 + len)), "summary (special %u rep %d)", special, rep);
        uint64_t k = 0;
        for (uint32_t i = 0; i < len; ++i) k += r.kept[i];
        CHECK(fa_kept_total(s, in != 0) == k, "kept total");
        if (len) CHECK(fa_state_out(s, in != 0) == (r.hdr[len - 1] != 0), "state out");
        ++done;
      }
    }
  return done;
}

static uint64_t test_combines() {
  uint64_t done = 0;
  for (uint32_t special = 1; special <= 64; special *= 2)
    for (int rep = 0; rep < 40; ++rep) {
      std::vector<uint8_t> t = random_bytes(4096, special);
      if (rep % 2) t[0] = '>';
      // lane summaries first (what the kernels combine), then pieces of whole lanes cut at random
      std::vector<FastaSum64> lane(64);
      for (uint32_t l = 0; l < 64; ++l) {
        const FastaSum s = fa_summary(lane_of(t, 64 * l));
        lane[l] = fa_combine(fa_identity<uint64_t>(), s);
        CHECK(same(lane[l], brute_summary(t, 64 * l, 64 * l + 64)), "lane summary %u", l);
      }
      std::vector<uint32_t> cut = {0, 64};
      for (uint32_t c = 1; c < 64; ++c)
        if (below(4) == 0) cut.insert(cut.end() - 1, c);
      std::vector<FastaSum64> piece;
      for (size_t i = 0; i + 1 < cut.size(); ++i) {
        FastaSum64 s = fa_identity<uint64_t>();
        for (uint32_t l = cut[i]; l < cut[i + 1]; ++l) s = fa_combine(s, lane[l]);
        CHECK(same(s, brute_summary(t, 64 * cut[i], 64 * cut[i + 1])), "piece [%u, %u)", cut[i], cut[i + 1]);
        piece.push_back(s);
      }
      // any bracketing: combine random neighbours until one is left
      while (piece.size() > 1) {
        const size_t i = below((uint32_t)piece.size() - 1);
        piece[i] = fa_combine(piece[i], piece[i + 1]);
        piece.erase(piece.begin() + (long)i + 1);
      }
      const FastaSum64 whole = brute_summary(t, 0, 4096);
      CHECK(same(piece[0], whole), "bracketing (special %u rep %d)", special, rep);
      for (int in = 0; in < 2; ++in) {
        // (position 0 is a line start: the carried state is read only where the buffer is taken as a later stretch)
        std::vector<uint8_t> u(1, 'A');
        u.insert(u.end(), t.begin(), t.end());
        const Brute r = brute(u, 1, 4097, in != 0);
        uint64_t k = 0;
        for (uint8_t x : r.kept) k += x;
        const FastaSum64 s = brute_summary(u, 1, 4097);
        CHECK(fa_kept_total(s, in != 0) == k, "kept total under state %d", in);
        CHECK(fa_state_out(s, in != 0) == (r.hdr.back() != 0), "state out under state %d", in);
      }
      ++done;
    }
  return done;
}

// ---- the passes as the kernels run them
struct Rec {
  uint64_t id_start, id_len, seq_start, seq_len;
  std::string seq;
};
static std::vector<Rec> parse(const std::vector<uint8_t>& t) {  // the line-by-line definition
  std::vector<Rec> out;
  size_t p = 0;
  while (p < t.size()) {
    size_t e = p;
    while (e < t.size() && t[e] != '\n') ++e;
    size_t le = e;
    if (le > p && t[le - 1] == '\r') --le;
    if (t[p] == '>') out.push_back(Rec{p + 1, le - p - 1, 0, 0, ""});
    else if (!out.empty()) out.back().seq.append((const char*)&t[p], le - p);
    p = e + 1;
  }
  uint64_t at = 0;
  for (Rec& r : out) {
    r.seq_start = at;
    r.seq_len = r.seq.size();
    at += (r.seq_len + 63) / 64 * 64;
  }
  return out;
}

static void pipeline(const std::vector<uint8_t>& t) {
  const uint64_t n = t.size();
  const std::vector<Rec> want = parse(t);
  const uint64_t n_tiles = (n + kFaTileBytes - 1) / kFaTileBytes;
  // count pass + scan: in front of every tile, resolved from byte 0
  std::vector<FastaSum64> front(n_tiles + 1);
  std::vector<FastaSum> tile_sum(n_tiles);
  FastaSum64 run = fa_identity<uint64_t>();
  for (uint64_t tile = 0; tile < n_tiles; ++tile) {
    FastaSum s = fa_identity<uint32_t>();
    for (uint32_t l = 0; l < 64; ++l) s = fa_combine(s, fa_summary(lane_of(t, tile * kFaTileBytes + 64 * l)));
    tile_sum[tile] = s;
    front[tile] = run;
    run = fa_combine(run, s);
  }
  front[n_tiles] = run;
  const uint64_t n_rec = run.n_hdr, total_kept = fa_kept_total(run, false);
  CHECK(n_rec == want.size(), "record count %llu, want %zu", (unsigned long long)n_rec, want.size());
  std::vector<uint64_t> hs_pos(n_rec, ~0ull), kept_at(n_rec, ~0ull), hdr_end(n_rec, ~0ull);
  std::vector<uint8_t> keep(n, 0);
  std::vector<uint64_t> rank(n, 0), owner(n, 0);
  for (uint64_t tile = 0; tile < n_tiles; ++tile) {
    const bool tile_in = fa_state_out(front[tile], false);
    const uint64_t tile_kept = fa_kept_total(front[tile], false), tile_hdr = front[tile].n_hdr;
    FastaSum excl = fa_identity<uint32_t>();
    for (uint32_t l = 0; l < 64; ++l) {
      const uint64_t base = tile * kFaTileBytes + 64 * l;
      const uint32_t len = base >= n ? 0u : (uint32_t)(n - base < 64 ? n - base : 64);
      const FastaLane L = lane_of(t, base);
      const bool in = fa_state_out(excl, tile_in);
      const uint64_t kept_before = tile_kept + fa_kept_total(excl, tile_in), hdr_before = tile_hdr + excl.n_hdr;
      const uint64_t hdr = fa_in_header(L.ls, L.hs, in), kept = L.cand & ~hdr;
      uint64_t nl = 0;
      for (uint32_t i = 0; i < len; ++i) nl |= (uint64_t)(t[base + i] == '\n') << i;
      for (uint32_t i = 0; i < len; ++i) {
        if ((L.hs >> i) & 1) {
          const uint64_t rec = hdr_before + fa_popc(L.hs & fa_below(i));
          CHECK(rec < n_rec && hs_pos[rec] == ~0ull, "header start written twice");
          hs_pos[rec] = base + i;
          kept_at[rec] = kept_before + fa_popc(kept & fa_below(i));
        }
        if ((nl & hdr) >> i & 1) {
          const uint64_t recs = hdr_before + fa_popc(L.hs & fa_below(i + 1));
          CHECK(recs >= 1 && recs <= n_rec && hdr_end[recs - 1] == ~0ull, "header end written twice");
          hdr_end[recs - 1] = base + i;
        }
        if ((kept >> i) & 1) {
          keep[base + i] = 1;
          rank[base + i] = kept_before + fa_popc(kept & fa_below(i));
          owner[base + i] = hdr_before + fa_popc(L.hs & fa_below(i + 1));
        }
      }
      if (len > 0 && base + len == n && ((hdr >> (len - 1)) & 1) && !((nl >> (len - 1)) & 1)) {
        const uint64_t recs = hdr_before + fa_popc(L.hs);
        CHECK(recs >= 1 && recs <= n_rec && hdr_end[recs - 1] == ~0ull, "last header end written twice");
        hdr_end[recs - 1] = n;
      }
      excl = fa_combine(excl, fa_summary(L));
    }
    CHECK(same(excl, tile_sum[tile]), "tile summary");
  }
  uint64_t at = 0;
  std::vector<uint64_t> seq_start(n_rec);
  for (uint64_t r = 0; r < n_rec; ++r) {
    CHECK(hs_pos[r] != ~0ull && hdr_end[r] != ~0ull, "record %llu not written", (unsigned long long)r);
    const uint64_t len = (r + 1 < n_rec ? kept_at[r + 1] : total_kept) - kept_at[r];
    const uint64_t id_len = hdr_end[r] - hs_pos[r] - 1 - (t[hdr_end[r] - 1] == '\r');
    CHECK(hs_pos[r] + 1 == want[r].id_start && id_len == want[r].id_len, "id of record %llu", (unsigned long long)r);
    CHECK(len == want[r].seq_len && at == want[r].seq_start, "length / start of record %llu", (unsigned long long)r);
    seq_start[r] = at;
    at += (len + 63) / 64 * 64;
  }
  std::vector<uint8_t> text(at + 64, 0);
  for (uint64_t p = 0; p < n; ++p)
    if (keep[p]) {
      CHECK(owner[p] >= 1 && owner[p] <= n_rec, "kept byte without a record");
      const uint64_t r = owner[p] - 1;
      text[seq_start[r] + (rank[p] - kept_at[r])] = t[p];
    }
  for (uint64_t r = 0; r < n_rec; ++r)
    CHECK(memcmp(&text[seq_start[r]], want[r].seq.data(), want[r].seq.size()) == 0, "sequence of record %llu", (unsigned long long)r);
}

static uint64_t test_pipelines() {
  uint64_t done = 0;
  auto bytes = [](const std::string& s) { return std::vector<uint8_t>(s.begin(), s.end()); };
  for (const char* s : {">", ">a\nACGT", ">a\r\nAC\r\nGT\r", ">\n>\n>\n", ">a\n\n\nAC\n\n>b", ">a>b\nAC>GT\n>c\r", ">x\nA\rC\r\r\nG\n"}) {
    pipeline(bytes(s));
    ++done;
  }
  for (uint32_t special = 1; special <= 64; special *= 2)
    for (int rep = 0; rep < 12; ++rep) {
      std::vector<uint8_t> t = random_bytes(1 + below(3 * kFaTileBytes), special);
      t[0] = '>';
      pipeline(t);
      ++done;
    }
  // borders: '>' / '\n' / "\r\n" / the input's end at and next to 63, 64, 4095, 4096
  for (uint32_t at : {63u, 64u, 4095u, 4096u})
    for (int what = 0; what < 6; ++what) {
      std::string s = ">" + std::string(at > 40 ? 20 : 0, 'i') + "\n";
      while (s.size() < at) s += s.size() % 61 == 60 ? '\n' : 'A';
      s.resize(at);
      if (s.size() > 23 && s[s.size() - 1] == '\n') s[s.size() - 1] = 'A';
      if (what == 0) s[at - 1] = '\n', s += ">next\nACGT\n";  // '>' at `at`
      if (what == 1) s += "\nACGT\n";                           // '\n' at `at`
      if (what == 2) s[at - 1] = '\r', s += "\nACGT\n";        // '\r' | '\n' across the border
      if (what == 3) s[at - 1] = '\r';                          // the input ends with '\r' in front of the border
      if (what == 4) s += "A";                                  // ... with a base at the border
      if (what == 5) s[at - 1] = '\n', s += ">hdr";            // ... inside a header line
      pipeline(bytes(s));
      ++done;
    }
  return done;
}

int main(int argc, char** argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const uint64_t lanes = test_lanes(), combines = test_combines(), pipelines = test_pipelines();
  printf("ok lanes=%llu combines=%llu pipelines=%llu\n", (unsigned long long)lanes, (unsigned long long)combines,
         (unsigned long long)pipelines);
  return 0;
}
