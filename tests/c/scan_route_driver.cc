// Drives sassy_amd/csrc/scan_route.h (host only, no HIP call) without a device: see tests/test_scan_route_cpu.py.
//   scan_route_driver rows        one search per stdin line -> "filtered piece_len fused pair" as stats() reports them
//   scan_route_driver invariants  what every route keeps, over profile x m x k x pattern kind x option
//   scan_route_driver packing <seed>   the filter's launch parameters and the two tables against brute force
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>  // (types only: common.h names hipEvent_t and uint4; nothing of the runtime is called or linked)

#include "../../sassy_amd/csrc/scan_route.h"

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

static bool set_sw(Switches& sw, const char* name, long v) {
#define SET_ONE(field, dflt, doc) \
  if (!strcmp(name, #field)) { sw.field = v; return true; }
  SASSY_HIP_SWITCHES(SET_ONE)
#undef SET_ONE
  return false;
}

static uint64_t g_rng = 1;
static uint32_t rnd(uint32_t n) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_rng >> 33) % n);
}

// the lane's side of prepare(): the table key a route leaves behind
struct Lane {
  uint32_t fuse_backoff = 0, table_q = 0, table_r = 0, table_k = 0;
  int table_profile = -1;
  bool table_rc = false;
  std::vector<uint8_t> table_pattern, h_table;
  double table_density = 0;
};

struct Job {
  Profile profile = PROFILE_DNA;
  PatternPlan plan;
  std::vector<uint8_t> pat, rc_pat;
  uint32_t k = 0;
  Switches sw;
  int prefilter = -1;
  bool fuse = true, want_counters = false, overhang = false, do_trace = true;
  bool ext_bitmap = false, ext_desc = false, rc_bitmap = false, reversed = false, texts = false, no_fuse = false;
  uint32_t ext_q = 0;
  uint64_t n_blocks = 1024;
};

// trace_shape(m, k).wave_fits (host_internal.h): a band row fits a wavefront, four slices with their patterns a CU's LDS
static bool wave_fits(uint32_t m, uint32_t k) {
  const uint64_t cell = (k + 1 <= 255) ? 1 : 2;
  const uint64_t band = ((uint64_t)(m + 1) * (2ull * k + 3) * cell + 3) / 4 * 4;
  const uint64_t win = ((uint64_t)m + k + 15 + 15) / 16 * 16, ops = ((uint64_t)m + k + 1 + 3) / 4 * 4;
  const uint64_t str = (2ull * (m + k + 1) + 2 + 15) / 16 * 16, pat_bytes = ((uint64_t)m + 15) / 16 * 16;
  const uint64_t wave_stride = (band + win + ops + str + 128 + 15) / 16 * 16;
  return 2ull * k + 3 <= 64 && 4 * pat_bytes + 4 * wave_stride <= 160 * 1024;
}

static void run_route(const Job& j, Lane& L, Route& R) {
  const RouteInput in{j.profile, j.plan.m, j.plan.nwords, j.plan.nslots, j.plan.bytes, j.plan.classes, j.pat.data(),
                      j.rc_bitmap ? j.rc_pat.data() : nullptr, j.k, j.sw, j.prefilter, j.fuse, j.want_counters, j.overhang, j.do_trace,
                      wave_fits(j.plan.m, j.k), j.ext_bitmap, j.ext_q, j.ext_desc, j.rc_bitmap, j.reversed, j.texts, j.no_fuse, j.n_blocks,
                      L.fuse_backoff, L.table_q, L.table_r, L.table_k, L.table_profile, L.table_rc, L.table_pattern, L.table_density};
  choose_route(in, R, L.h_table);
  if (R.table_dropped) L.table_q = 0;
  if (R.table != kTableNone && !R.table_cached) {
    L.table_q = R.table_q; L.table_r = R.table_r; L.table_k = j.k; L.table_profile = (int)j.profile;
    if (R.table == kTableCount) { L.table_rc = R.rc_marked; L.table_density = R.table_density; }
    L.table_pattern = j.pat;
  }
}

static void set_plan(Job& j, Profile pr, const std::vector<uint8_t>& pat) {
  std::string err;
  j.profile = pr;
  j.pat = pat;
  j.plan = PatternPlan{};
  CHECK(make_plan(pr, pat.data(), pat.size(), j.plan, err), "%s", err.c_str());
}

// ---------------------------------------------------------------- rows
// line: alphabet rc overhang trace prefilter fuse classes m nslots k n_opts [name value]... pattern-hex
// Both strands as search_text() runs them: the last job to finish is the one stats() shows.
static int rows_main() {
  char alphabet[32], hex[4096], name[64];
  int rc, overhang, trace, prefilter, fuse, classes, n_opts;
  unsigned m, nslots, k;
  long n = 0;
  while (scanf("%31s %d %d %d %d %d %d %u %u %u %d", alphabet, &rc, &overhang, &trace, &prefilter, &fuse, &classes, &m, &nslots, &k, &n_opts) == 11) {
    Job j;
    for (int i = 0; i < n_opts; ++i) {
      long v;
      CHECK(scanf("%63s %ld", name, &v) == 2 && set_sw(j.sw, name, v), "switch %s", name);
    }
    CHECK(scanf("%4095s", hex) == 1, "pattern");
    const Profile pr = !strcmp(alphabet, "dna") ? PROFILE_DNA : !strcmp(alphabet, "iupac") ? PROFILE_IUPAC
                       : !strcmp(alphabet, "ascii_ci") ? PROFILE_ASCII_CI : PROFILE_ASCII;
    std::vector<uint8_t> pat;
    if (classes) {  // (the route reads the plan's numbers, never a class pattern's rows)
      j.profile = pr;
      j.pat.assign(m, 0);
      j.plan.classes = true;
      j.plan.m = m; j.plan.nwords = (m + 31) / 32; j.plan.nslots = nslots;
    } else {
      for (size_t i = 0; hex[i] && hex[i + 1]; i += 2) {
        unsigned b;
        sscanf(hex + i, "%2x", &b);
        pat.push_back((uint8_t)b);
      }
      set_plan(j, pr, pat);
    }
    j.k = k; j.prefilter = prefilter; j.fuse = fuse != 0; j.overhang = overhang != 0; j.do_trace = trace != 0;
    Lane lane0, lane1;
    Route R;
    run_route(j, lane0, R);
    uint32_t fkind = R.filtered ? R.fkind : 0, q = R.q, fused = R.fused, pair = R.fused ? R.pair : 0;
    if (rc) {
      Job c = j;  // the Rc strand's job: complement(pattern)
      for (uint8_t& ch : pat) ch = complement_char(pr, ch);
      set_plan(c, pr, pat);
      uint32_t ps = 0, pq = 0;
      const bool pair_strands = j.sw.pair_rc != 0 && j.fuse && j.do_trace && pair_eligible(pr, j.sw, j.prefilter, j.pat.data(), m, k, &ps, &pq);
      const bool can_fuse = j.sw.rc_fused != 0 && !j.overhang && !is_ascii(pr) && !pair_strands;
      Route Rc;
      bool by_bitmap = false;
      if (can_fuse) {  // the forward job's filter marks the Rc strand's blocks where it can
        Job f = j;
        f.rc_bitmap = true;
        f.rc_pat = c.pat;
        lane0 = Lane{};
        run_route(f, lane0, R);
        bool rc_marked = R.rc_marked, second = false;
        if (R.filtered) {
          ScanParams F{};
          pack_filter(F, R, f.plan.row_tab, f.pat.data(), f.rc_pat.data(), m, k, true, &rc_marked, &second);
        }
        by_bitmap = rc_marked;
        if (by_bitmap) {
          c.ext_bitmap = true;
          c.ext_q = R.q;
          c.reversed = true;
          run_route(c, lane1, Rc);
        }
      }
      // else two searches, in flight on two lanes or one behind the other on the first: the Rc strand's finishes last
      if (!by_bitmap) run_route(c, can_fuse || j.overhang || j.sw.strands_in_flight == 0 ? lane0 : lane1, Rc);
      fkind = Rc.filtered ? Rc.fkind : 0; q = Rc.q; fused = Rc.fused; pair = Rc.fused ? Rc.pair : 0;
    }
    printf("%u %u %u %u\n", fkind, q, fused, pair);
    ++n;
  }
  fprintf(stderr, "rows %ld\n", n);
  return 0;
}

// ---------------------------------------------------------------- invariants
static std::vector<uint8_t> make_pattern(int kind, uint32_t m) {
  std::vector<uint8_t> p(m);
  for (uint32_t i = 0; i < m; ++i) p[i] = "ACGT"[rnd(4)];
  if (kind == 1 && m >= 3) { p[m - 3] = 'N'; p[m - 2] = 'G'; p[m - 1] = 'G'; }
  if (kind == 2)
    for (uint32_t i = 1; i < m; i += 3) p[i] = "RYKMSWN"[(i / 3) % 7];
  if (kind == 3)  // Ascii, at most 16 distinct bytes
    for (uint32_t i = 0; i < m; ++i) p[i] = (uint8_t)('a' + rnd(12));
  if (kind == 4)  // more than 16 (once the pattern is long enough)
    for (uint32_t i = 0; i < m; ++i) p[i] = (uint8_t)('A' + (i < 40 ? i : rnd(40)));
  if (kind == 5)  // byte mode from 65 rows on
    for (uint32_t i = 0; i < m; ++i) p[i] = (uint8_t)(33 + (i < 94 ? i : rnd(94)));
  return p;
}

static int invariants_main() {
  struct Case { Profile pr; int kind; bool classes; };
  const Case cases[] = {{PROFILE_DNA, 0, false}, {PROFILE_IUPAC, 0, false}, {PROFILE_IUPAC, 1, false}, {PROFILE_IUPAC, 2, false},
                        {PROFILE_ASCII, 3, false}, {PROFILE_ASCII, 4, false}, {PROFILE_ASCII, 5, false}, {PROFILE_ASCII_CI, 3, false},
                        {PROFILE_ASCII_CI, 4, false}, {PROFILE_ASCII_CI, 5, false}, {PROFILE_ASCII, 3, true}};
  struct Opt { const char* name; long value; };
  // "" the defaults; the searcher's own prefilter / fuse / counters, the job's booleans, then the switches
  const Opt opts[] = {{"", 0}, {"S.prefilter", 0}, {"S.prefilter", 1}, {"S.fuse", 0}, {"S.want_counters", 1}, {"overhang", 1}, {"do_trace", 0},
                      {"rc_bitmap", 1}, {"reversed", 1}, {"texts", 1}, {"no_fuse", 1}, {"fuse_backoff", 3}, {"prefilter", 0}, {"prefilter", 1},
                      {"pair", 0}, {"pair", 2}, {"filter_kind", 1}, {"filter_kind", 2}, {"filter_kind", 3}, {"filter_kind", 4},
                      {"short_pieces", 0}, {"iupac_planes", 0}, {"count_fused", 0}, {"trace_wave", 0}, {"self_rank", 0}};
  long routes = 0, by_kind[5] = {0, 0, 0, 0, 0}, pairs = 0, fused_n = 0, direct = 0;
  for (const Case& c : cases)
    for (uint32_t m = 1; m <= 130; ++m) {
      const std::vector<uint8_t> pat = make_pattern(c.kind, m);
      std::vector<uint8_t> rc_pat(pat);
      if (!is_ascii(c.pr))
        for (uint8_t& ch : rc_pat) ch = complement_char(c.pr, ch);
      Job base;
      set_plan(base, c.pr, pat);
      if (c.classes) { base.plan.classes = true; base.plan.bytes = false; }
      base.rc_pat = rc_pat;
      for (uint32_t k = 0; k <= 16; ++k)
        for (const Opt& o : opts) {
          Job j = base;
          j.k = k;
          if (!strcmp(o.name, "S.prefilter")) j.prefilter = (int)o.value;
          else if (!strcmp(o.name, "S.fuse")) j.fuse = false;
          else if (!strcmp(o.name, "S.want_counters")) j.want_counters = true;
          else if (!strcmp(o.name, "overhang")) j.overhang = true;
          else if (!strcmp(o.name, "do_trace")) j.do_trace = false;
          else if (!strcmp(o.name, "rc_bitmap")) { if (is_ascii(c.pr)) continue; j.rc_bitmap = true; }
          else if (!strcmp(o.name, "reversed")) j.reversed = true;
          else if (!strcmp(o.name, "texts")) j.texts = true;
          else if (!strcmp(o.name, "no_fuse")) j.no_fuse = true;
          else if (o.name[0] && strcmp(o.name, "fuse_backoff")) CHECK(set_sw(j.sw, o.name, o.value), "switch %s", o.name);
          Lane L;
          if (!strcmp(o.name, "fuse_backoff")) L.fuse_backoff = (uint32_t)o.value;
          Route R;
          run_route(j, L, R);
          ++routes;
          by_kind[R.filtered ? R.fkind : 0]++;
          pairs += R.pair != 0; fused_n += R.fused; direct += R.count_direct;
#define INV(cond) CHECK(cond, "profile %u kind %d m %u k %u option %s=%ld: fkind %u q %u pair %u fused %d", (unsigned)c.pr, c.kind, m, k, o.name, o.value, \
                        (unsigned)R.fkind, R.q, R.pair, (int)R.fused)
          INV(!R.filtered || R.q > 0);
          INV(R.filtered || R.q == 0);
          INV(!(j.overhang || j.plan.classes || j.plan.bytes || j.plan.nslots > 16) || !R.filtered);
          INV(prefilter_mode(j.prefilter, j.sw) != 0 || !R.filtered);
          INV(R.pair == 0 || (R.fused && R.fkind == kFilterPlanes));
          // the Iupac bit-plane filter exists as the fused launch only (choose_route asserts it, too)
          INV(!(c.pr == PROFILE_IUPAC && R.filtered && R.fkind == kFilterPlanes) || R.fused);
          INV(!(R.filtered && R.fkind == kFilterCount) || (R.count_t >= 1 && R.count_w <= 64 && R.count_tail < 0.05));
          INV(!(R.filtered && R.fkind == kFilterTable) || (R.q >= 7 && R.q <= 9));
          INV(!(R.filtered && R.fkind == kFilterGeneric) || (uint64_t)(k + 1) * R.q <= 255);
          INV(!R.fused || R.use_wave);
          INV(!R.fused || (R.filtered && R.fkind == kFilterPlanes));
          INV(!R.count_direct || (R.filtered && R.fkind == kFilterCount && !R.rc_marked));
          INV((R.table == kTableCount) == (R.filtered && R.fkind == kFilterCount));
          INV((R.table == kTableQgram) == (R.filtered && R.fkind == kFilterTable));
          INV(R.table == kTableNone || R.table_cached || !L.h_table.empty());
          // the same search again on the same lane: the same route, from the cached table
          if (R.table != kTableNone && (!o.name[0] || j.rc_bitmap)) {
            Route R2;
            run_route(j, L, R2);
            INV(R2.table_cached && R2.table == R.table && R2.q == R.q && R2.fkind == R.fkind && R2.count_r == R.count_r &&
                R2.count_t == R.count_t && R2.count_tail == R.count_tail && R2.fused == R.fused && R2.count_direct == R.count_direct);
          }
#undef INV
        }
    }
  printf("ok routes=%ld none=%ld generic=%ld planes=%ld table=%ld count=%ld pair=%ld fused=%ld direct=%ld\n", routes, by_kind[0], by_kind[1],
         by_kind[2], by_kind[3], by_kind[4], pairs, fused_n, direct);
  return 0;
}

// ---------------------------------------------------------------- packing and tables
static uint32_t base_set(Profile pr, uint8_t c) { return pr == PROFILE_IUPAC ? (iupac_code(c) & 15u) : (1u << ((c >> 1) & 3u)); }
// does the Q-gram `gram` (first row most significant) fit rows p[0 .. Q)?
static bool gram_fits(Profile pr, const uint8_t* p, uint32_t Q, uint32_t gram) {
  for (uint32_t j = 0; j < Q; ++j)
    if (!((base_set(pr, p[j]) >> ((gram >> (2 * (Q - 1 - j))) & 3u)) & 1u)) return false;
  return true;
}

static int packing_main(uint64_t seed) {
  g_rng = seed;
  long packed = 0, tables = 0;
  for (int it = 0; it < 400; ++it) {
    const uint32_t k = rnd(8), np = k + 1;
    uint32_t pair = 0, q = 2 + rnd(11);
    if (it % 4 == 3 && k >= 1) { pair = (k + 2) / 2; q = 5 + rnd(2); }
    const uint32_t n_own = pair ? 2 * pair : np;
    const uint32_t m = n_own * q + rnd(7);
    const bool with_rc = !pair && rnd(2);
    std::vector<uint8_t> pat(m), rc_pat(m);
    for (uint32_t i = 0; i < m; ++i) { pat[i] = "ACGTacgt"[rnd(8)]; rc_pat[i] = complement_char(PROFILE_DNA, pat[i] & 0xDFu); }
    PatternPlan plan;
    std::string err;
    CHECK(make_plan(PROFILE_DNA, pat.data(), m, plan, err), "%s", err.c_str());
    Route R;
    R.q = q; R.pair = pair; R.filtered = true; R.fkind = kFilterPlanes;
    ScanParams F{};
    memset(&F, 0xA5, sizeof(F));  // whatever the launch reads must have been written
    bool rc_marked = false, second = false;
    pack_filter(F, R, plan.row_tab, pat.data(), rc_pat.data(), m, k, with_rc, &rc_marked, &second);
    auto code = [](uint8_t c) { return (uint32_t)(c >> 1) & 3u; };
    auto piece_rows = [&](const ScanParams& X, uint32_t pp, uint32_t j) { return ((X.piece_bits[pp][1] >> j) & 1u) << 1 | ((X.piece_bits[pp][0] >> j) & 1u); };
    CHECK(rc_marked == with_rc && second == (with_rc && np > 4), "rc flags");
    CHECK(F.piece_len == q && F.pair == pair && F.piece_planes == 1 && F.count_rc == 0, "geometry");
    const bool both = with_rc && np <= 4;
    CHECK(F.n_pieces == (both ? 8 : n_own) && F.piece_groups == (F.n_pieces <= 4 ? 1u : 2u), "pieces %u", F.n_pieces);
    CHECK(F.piece_mirror == (both ? 0xF0u : 0u), "mirror %x", F.piece_mirror);
    for (uint32_t pp = 0; pp < 8; ++pp) {
      const bool mirror = both && pp >= 4;
      uint32_t piece = both ? (pp & 3u) : pp;
      if (piece >= (both ? np : n_own)) piece = 0;
      for (uint32_t j = 0; j < q; ++j)
        CHECK(piece_rows(F, pp, j) == (mirror ? code(rc_pat[piece * q + q - 1 - j]) : code(pat[piece * q + j])), "piece_bits pp %u row %u", pp, j);
      CHECK(F.piece_bits[pp][0] >> q == 0 && F.piece_bits[pp][1] >> q == 0, "bits above the piece");
      int32_t rem = (int32_t)(m - (piece + 1) * q);
      if (pair && (piece & 1u) == 0) rem -= (int32_t)(q + 2);
      CHECK((int32_t)F.piece_rem[pp] == rem, "piece_rem pp %u", pp);
    }
    // the slot-mask filter's rows: byte pp of piece_tab[g][j] = 2 * slot of row j of piece 4 g + pp (Dna: slot = code)
    const uint32_t n_tab = pair ? 2 * pair : np;  // (as filled in front of the two-strand layout)
    for (uint32_t g = 0; g < (n_tab <= 4 ? 1u : 2u); ++g)
      for (uint32_t pp = 0; pp < 4; ++pp) {
        uint32_t piece = 4 * g + pp;
        if (piece >= n_tab) piece = 0;
        for (uint32_t j = 0; j + 1 < q; ++j) CHECK(((F.piece_tab[g][j] >> (8 * pp)) & 0xFFu) == 2 * code(pat[piece * q + j]), "piece_tab");
        for (uint32_t j = q - 1; j < 12; ++j) CHECK(F.piece_tab[g][j] == 0, "piece_tab behind the piece");
        CHECK(((F.piece_last[g] >> (8 * pp)) & 0xFFu) == 2 * code(pat[piece * q + q - 1]), "piece_last");
      }
    if (pair)
      for (uint32_t pp = 0; pp < 2 * pair; ++pp)
        for (uint32_t j = 0; j < 8; ++j) {
          const uint32_t y = ((F.pair_y[2 * (pp >> 2) + 1] >> (8 * (pp & 3u) + j)) & 1u) << 1 | ((F.pair_y[2 * (pp >> 2)] >> (8 * (pp & 3u) + j)) & 1u);
          const uint32_t sib = pp ^ 1u;
          CHECK(y == (j < q ? code(pat[sib * q + ((pp & 1u) ? q - 1 - j : j)]) : 0u), "pair_y pp %u row %u", pp, j);
        }
    if (second) {  // the second launch: the same parameters with the Rc strand's pieces, all mirrored
      ScanParams F2 = F, W = F;
      rc_pieces(F2, rc_pat.data(), m, k, q);
      W.piece_mirror = 0;
      for (uint32_t pp = 0; pp < 8; ++pp) set_piece(W, rc_pat.data(), m, q, 0, pp, pp < np ? pp : 0, true);
      CHECK(memcmp(&F2, &W, sizeof(F2)) == 0 && F2.piece_mirror == 0xFFu, "F2");
      for (uint32_t pp = 0; pp < 8; ++pp) {
        const uint32_t piece = pp < np ? pp : 0;
        for (uint32_t j = 0; j < q; ++j) CHECK(piece_rows(F2, pp, j) == code(rc_pat[piece * q + q - 1 - j]), "F2 piece_bits");
        CHECK(F2.piece_rem[pp] == m - (piece + 1) * q, "F2 piece_rem");
      }
    }
    ++packed;
  }
  // the tables against a loop over every gram
  for (int it = 0; it < 24; ++it) {
    const Profile pr = it % 2 ? PROFILE_IUPAC : PROFILE_DNA;
    const uint32_t m = 21 + rnd(40);
    std::vector<uint8_t> pat = make_pattern(0, m), pat2 = make_pattern(0, m);
    if (pr == PROFILE_IUPAC)
      for (uint32_t i = rnd(5); i < m; i += 4 + rnd(5)) pat[i] = "RYKMSWNBDHV"[rnd(11)];
    {
      const uint32_t q = 7, pieces = 1 + rnd(m / q);
      std::vector<uint8_t> tab;
      CHECK(build_qgram_table(pr, pat.data(), q, pieces, tab), "qgram table");
      CHECK(tab.size() == (1u << (2 * q - 3)), "qgram table size");
      for (uint32_t gram = 0; gram < (1u << (2 * q)); ++gram) {
        bool want = false;
        for (uint32_t p = 0; p < pieces && !want; ++p) want = gram_fits(pr, pat.data() + p * q, q, gram);
        const uint32_t low = 2 * q - 3;
        CHECK((((tab[gram & ((1u << low) - 1u)] >> (gram >> low)) & 1u) != 0) == want, "qgram table gram %u", gram);
      }
      ++tables;
    }
    const uint32_t qr[3][2] = {{5, 2}, {6, 2}, {7, 1}};
    for (const auto& v : qr) {
      const uint32_t Q = v[0], Rr = v[1], nq = 1u << (2 * Q);
      const bool two = rnd(2);
      std::vector<uint8_t> tab, H(nq, 0);
      double density = -1;
      CHECK(build_count_table(pr, pat.data(), two ? pat2.data() : nullptr, m, Q, Rr, tab, &density), "count table");
      size_t set_bits = 0;
      for (uint32_t gram = 0; gram < nq; ++gram) {
        for (uint32_t o = 0; o + Q <= m && !H[gram]; ++o)
          H[gram] = gram_fits(pr, pat.data() + o, Q, gram) || (two && gram_fits(pr, pat2.data() + o, Q, gram));
        set_bits += H[gram];
      }
      CHECK(std::fabs(density - (double)set_bits / nq) < 1e-12, "density");
      CHECK(tab.size() == (1u << (2 * (Q + Rr - 1))), "count table size");
      for (uint32_t w = 0; w < tab.size(); ++w) {
        uint32_t c = 0;
        for (uint32_t r = 0; r < Rr; ++r) c += H[(w >> (2 * r)) & (nq - 1)];
        CHECK(tab[w] == c, "count table (%u, %u) entry %u", Q, Rr, w);
      }
      ++tables;
    }
  }
  printf("ok packed=%ld tables=%ld\n", packed, tables);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "rows")) return rows_main();
  if (argc >= 2 && !strcmp(argv[1], "invariants")) return invariants_main();
  if (argc >= 3 && !strcmp(argv[1], "packing")) return packing_main(strtoull(argv[2], nullptr, 10));
  fprintf(stderr, "usage: scan_route_driver rows | invariants | packing <seed>\n");
  return 2;
}
