// scan_route.h -- the route of one scan job, as a pure function of what it depends on, and the filter's launch
// parameters that follow from it.  Host only, no HIP call: ScanJob::prepare() (scan_driver.hip) fills a RouteInput, calls
// choose_route(), uploads the table it hands back and copies the Route into the job; search_text() asks pair_eligible()
// here whether two strands run as two searches.  Driven without a device by tests/c/scan_route_driver.cc
// (tests/test_scan_route_cpu.py).
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <vector>

#include "profiles.h"
#include "switches.h"

namespace sassy_hip {

// The prefilter kernels (scan_kernel.hip, count_filter.hip): which one evaluates the pieces.
enum FilterKind : uint32_t {
  kFilterGeneric = 1,  // filter_kernel: slot masks in LDS, any profile, <= 255 piece rows
  kFilterPlanes = 2,   // filter_dna_kernel: Dna, <= 8 pieces
  kFilterTable = 3,    // filter_table_kernel: q-gram bit table, Dna / Iupac, 7 <= q <= 9
  kFilterCount = 4,    // filter_count_kernel: q-gram lemma (count the pattern's q-grams per window), Dna / Iupac
};

// Prefilter geometry: k+1 disjoint pattern pieces of q rows.  Enabled when the pieces are long
// enough to be selective (expected hit blocks on random DNA: 64*(k+1)/4^q of all blocks).
// mode: the searcher's own setting (sassy_hip_set_prefilter), -1 = the process default (SASSY_HIP_PREFILTER)
inline int prefilter_mode(int prefilter, const Switches& sw) { return prefilter >= 0 ? prefilter : (int)sw.prefilter; }
inline uint32_t filter_piece_len(uint32_t m, uint32_t k, int env) {
  if (env == 0) return 0;
  const uint64_t pieces = (uint64_t)k + 1;
  uint64_t q = m / pieces;
  if (q > 12) q = 12;
  if (q < (env == 1 ? 2u : 7u)) return 0;    // too unselective: stream the full DP instead
  return (uint32_t)q;
}

// The paired filter's geometry for a shape (filter_dna_kernel<.., PAIR>): S = ceil((k+1)/2) super-pieces of two sub-pieces
// of Q = m / (2 S) rows each.  Taken where the k+1 pigeonhole pieces are shorter than 7 rows and Q is 5 or 6 (m = 23, k = 3;
// m = 32, k = 4, 5; m = 12, k = 1; ...).  False: the shape is not one of them.
inline bool pair_geometry(uint32_t m, uint32_t k, uint32_t* s_out, uint32_t* q_out) {
  if (k < 1 || m / (k + 1) >= 7) return false;
  const uint32_t s = (k + 2) / 2;
  if (s > 4) return false;
  const uint32_t q = m / (2 * s);
  if (q != 5 && q != 6) return false;
  *s_out = s;
  *q_out = q;
  return true;
}
// rows of the pattern, from row 0 on, that are plain bases
inline size_t plain_prefix(const uint8_t* pat, size_t m) {
  size_t j = 0;
  for (; j < m; ++j) {
    const uint8_t u = pat[j] & 0xDFu;
    if (u != 'A' && u != 'C' && u != 'G' && u != 'T') break;
  }
  return j;
}
// May a searcher (its profile, switches and prefilter setting) take the paired filter for this pattern and k, and with
// which S and Q?  The part of the answer that choose_route() (one job's route) and search_text() (two strands as two
// searches) share; each adds what only it knows.
// An Iupac searcher: the filter's 2 S Q rows are plain bases -- the rows behind them may hold ambiguity letters, a guide's NGG.
inline bool pair_eligible(Profile profile, const Switches& sw, int prefilter, const uint8_t* pat, uint32_t m, uint32_t k,
                          uint32_t* s_out, uint32_t* q_out) {
  if (sw.pair == 0 || prefilter_mode(prefilter, sw) >= 0 || !pair_geometry(m, k, s_out, q_out)) return false;
  if (profile == PROFILE_DNA) return true;
  return profile == PROFILE_IUPAC && *s_out <= 3 && plain_prefix(pat, m) >= (size_t)2 * *s_out * *q_out;
}


// Bit table of every q-gram (2 bits per char, first piece row most significant; codes A0 C1 T2 G3)
// that some piece accepts; rows with ambiguity letters are expanded.  False if that takes more
// than `limit` q-grams (then the table says nothing useful anyway).
inline bool build_qgram_table(Profile pr, const uint8_t* pat, uint32_t q, uint32_t pieces, std::vector<uint8_t>& tab) {
  const size_t limit = 1u << 16;
  tab.assign((size_t)1 << (2 * q - 3), 0);
  const uint32_t low_bits = 2 * q - 3;
  std::vector<uint32_t> cur, nxt;
  size_t total = 0;
  for (uint32_t p = 0; p < pieces; ++p) {
    cur.assign(1, 0u);
    for (uint32_t j = 0; j < q && !cur.empty(); ++j) {
      const uint8_t c = pat[p * q + j];
      // base set of the row as a nibble whose bit index is the 2-bit text code
      const uint32_t set = pr == PROFILE_IUPAC ? (iupac_code(c) & 15u) : (1u << ((c >> 1) & 3u));
      nxt.clear();
      for (uint32_t code : cur)
        for (uint32_t b = 0; b < 4; ++b)
          if ((set >> b) & 1u) nxt.push_back((code << 2) | b);
      if (nxt.size() + total > limit) return false;
      cur.swap(nxt);
    }
    total += cur.size();
    for (uint32_t code : cur) tab[code & ((1u << low_bits) - 1u)] |= (uint8_t)(1u << (code >> low_bits));
  }
  return true;
}

// The counting filter's table (count_filter.hip): H = every Q-gram some Q consecutive pattern rows
// accept (2 bits per letter, first row most significant, codes A0 C1 T2 G3; ambiguous rows are
// expanded); entry w of the table, w a (Q+R-1)-gram, = how many of the R Q-grams w ends with are
// in H.  density = |H| / 4^Q, the chance that a random position counts.  False if the expansion
// takes more than `limit` Q-grams.
inline bool build_count_table(Profile pr, const uint8_t* pat, const uint8_t* pat2, uint32_t m, uint32_t Q, uint32_t R,
                              std::vector<uint8_t>& tab, double* density) {
  const size_t limit = 1u << 20;
  const uint32_t nq = 1u << (2 * Q);
  std::vector<uint8_t> H(nq, 0);
  std::vector<uint32_t> cur, nxt;
  size_t total = 0;
  // pat2: a second pattern whose q-grams also count (the Rc strand's, in forward orientation)
  for (uint32_t o = 0; o + Q <= (pat2 ? 2 * m : m); ++o) {
    if (o + Q > m && o < m) continue;  // no q-gram across the two patterns
    cur.assign(1, 0u);
    for (uint32_t j = 0; j < Q; ++j) {
      const uint8_t c = o < m ? pat[o + j] : pat2[o - m + j];
      const uint32_t set = pr == PROFILE_IUPAC ? (iupac_code(c) & 15u) : (1u << ((c >> 1) & 3u));
      nxt.clear();
      for (uint32_t code : cur)
        for (uint32_t b = 0; b < 4; ++b)
          if ((set >> b) & 1u) nxt.push_back((code << 2) | b);
      if (nxt.size() + total > limit) return false;
      cur.swap(nxt);
    }
    total += cur.size();
    for (uint32_t code : cur) H[code] = 1;
  }
  size_t set_bits = 0;
  for (uint8_t v : H) set_bits += v;
  *density = (double)set_bits / (double)nq;
  const uint32_t nw = 1u << (2 * (Q + R - 1));
  tab.assign(nw, 0);
  for (uint32_t w = 0; w < nw; ++w) {
    uint32_t c = 0;
    for (uint32_t r = 0; r < R; ++r) c += H[(w >> (2 * r)) & (nq - 1)];
    tab[w] = (uint8_t)c;
  }
  return true;
}

// How often a window of random text reaches the threshold t when it holds lambda q-gram hits on
// average.  Hits come in clumps (a text stretch that equals L >= Q pattern rows gives L - Q + 1 of
// them): clumps arrive Poisson(lambda (1 - r)) with geometric sizes, P(j) = (1 - r) r^(j-1), r = 1/4
// the chance that the next letter extends the stretch.  P(S >= t) by Panjer's recursion.
inline double clumped_tail(double lambda, uint32_t t) {
  if (t == 0) return 1.0;
  if (lambda <= 0) return 0.0;
  if (lambda >= (double)t) return 1.0;  // at or above the mean: no filter
  const double r = 0.25, lc = lambda * (1.0 - r);
  std::vector<double> p(t, 0.0);
  p[0] = std::exp(-lc);
  if (p[0] <= 0) return 1.0;
  double below = p[0];
  for (uint32_t s = 1; s < t; ++s) {
    double acc = 0, g = 1.0 - r;  // g = P(size j)
    for (uint32_t j = 1; j <= s && j <= 48; ++j, g *= r) acc += (double)j * g * p[s - j];
    p[s] = lc / (double)s * acc;
    below += p[s];
  }
  return std::min(1.0, std::max(0.0, 1.0 - below));
}

// Everything the route of a scan job depends on.
struct RouteInput {
  Profile profile;
  uint32_t m, nwords, nslots;  // the pattern's plan
  bool bytes, classes;
  const uint8_t* pat;
  const uint8_t* rc_pat;       // complement(pattern), read when rc_bitmap is set
  uint32_t k;
  const Switches& sw;
  int prefilter;               // the searcher's own setting (-1: the switch decides)
  bool fuse, want_counters;    // ... its set_fused and enable_counters
  bool overhang;
  bool do_trace;
  bool wave_fits;              // trace_shape(m, k).wave_fits: the wave-per-report traceback takes this shape
  // the job: a bitmap or a chunk list made elsewhere, the Rc strand marked in the same pass, the buffer read backwards,
  // several texts in the buffer, already fallen back from the fused launch
  bool ext_bitmap;
  uint32_t ext_q;
  bool ext_desc, rc_bitmap, reversed, texts, no_fuse;
  uint64_t n_blocks;
  // the lane: searches it still runs unfused, and the table it holds from its last search
  uint32_t fuse_backoff;
  uint32_t table_q, table_r, table_k;
  int table_profile;
  bool table_rc;
  const std::vector<uint8_t>& table_pattern;
  double table_density;
};

enum RouteTable : uint32_t { kTableNone = 0, kTableQgram = 1, kTableCount = 2 };

// What the rest of prepare(), the launches and finish_once() consume.
struct Route {
  uint32_t q = 0;               // piece length (counting filter: its Q); 0: no filter
  bool filtered = false;
  FilterKind fkind = kFilterGeneric;
  uint32_t pair = 0;            // paired filter: super-pieces (0: not taken)
  uint32_t count_r = 0, count_w = 0, count_t = 0;  // counting filter: R, window blocks, threshold
  double count_tail = 0;        // ... and the expected fraction of candidate blocks
  bool count_direct = false;    // ... files the chunk descriptors itself
  bool fused = false;           // filter + chunk DP in one launch
  bool use_wave = false;        // the wave-per-report traceback is this job's
  bool rc_marked = false;       // the counting filter marks the Rc strand's blocks too (the bit-plane filter: pack_filter)
  // the filter's table: kind, (q, r), whether the lane's cached one serves.  Not cached: choose_route() left its bytes in
  // `table` and the caller uploads them and records the key.  table_dropped: the lane's cached table is no longer valid.
  RouteTable table = kTableNone;
  uint32_t table_q = 0, table_r = 0;
  bool table_cached = false, table_dropped = false;
  double table_density = 0;     // counting table
};

// The route of one job.  table: the lane's host copy of its table; rebuilt in place when the route needs another one.
inline void choose_route(const RouteInput& in, Route& R, std::vector<uint8_t>& table) {
  R = Route{};
  const Profile profile = in.profile;
  const Switches& sw = in.sw;
  const uint32_t k = in.k, m = in.m;
  const uint8_t* pat = in.pat;
  const bool overhang = in.overhang, ext_bitmap = in.ext_bitmap, ext_desc = in.ext_desc;
  uint32_t lane_q = in.table_q;   // 0 once a build failed: the lane's table is gone
  double density = in.table_density;
  const bool table_pattern_same = in.table_pattern.size() == m && memcmp(in.table_pattern.data(), pat, m) == 0;
  uint32_t q = filter_piece_len(m, k, prefilter_mode(in.prefilter, sw));
  // a match that hangs over an end of the text contains only part of the pattern: the pigeonhole
  // argument of the prefilter does not cover it, so overhang searches stream the full DP
  if (overhang) q = 0;
  // Ascii patterns with more than 16 distinct bytes: only the DP kernels carry that many slot masks (or, byte mode,
  // compare bytes instead of looking slots up); class patterns exist on the streaming DP only
  if (in.nslots > 16 || in.bytes || in.classes) q = 0;
  if (ext_bitmap) q = in.ext_q;
  if (ext_desc) q = 1;  // list mode without a filter
  // which prefilter kernel (SASSY_HIP_FILTER_KIND=1|2|3|4 forces one where it applies)
  const int env_kind = (int)sw.filter_kind;
  const int env_pre = prefilter_mode(in.prefilter, sw);
  FilterKind fkind = kFilterGeneric;
  if (ext_bitmap || ext_desc) fkind = kFilterPlanes;  // (ext_bitmap: marked like filter_dna_kernel does)
  const uint32_t pieces = k + 1;
  // The fused launch (filter + chunk DP in one kernel) takes one strand of one text whose reports the
  // traceback waves rank themselves: the wave-per-report traceback must be this job's (use_wave).
  const bool use_wave = in.do_trace && sw.trace_wave != 0 && in.wave_fits;
  const bool fuse_ok = !ext_bitmap && !ext_desc && !in.rc_bitmap && !in.reversed && in.fuse && !in.no_fuse &&
                       in.fuse_backoff == 0 && sw.self_rank != 0 && use_wave &&
                       !in.texts && in.nwords <= 8 && in.n_blocks < 0x7FFFFFFFull && !in.want_counters;
  // Iupac searcher, pattern of plain A C G T, <= 4 pieces: the Dna bit-plane filter with a check of the text
  // (filter_dna_kernel, CHECK) -- as the fused launch only.  Where the text holds other letters (N runs, ambiguity codes,
  // anything) the lane that owns the block queues the columns a match touching them can end in, like a piece
  // occurrence, and the chunk DP of such a launch builds the Iupac profile's masks: exact on any text.
  const int env_iupac_planes = (int)sw.iupac_planes;
  bool plain_pattern = profile == PROFILE_IUPAC && env_iupac_planes != 0 && !overhang;
  for (uint32_t j = 0; plain_pattern && j < m; ++j) {
    const uint8_t u = pat[j] & 0xDFu;
    plain_pattern = u == 'A' || u == 'C' || u == 'G' || u == 'T';
  }
  bool iupac_planes = plain_pattern && fuse_ok && q >= 6 && q <= 12 && pieces <= 4 && in.nslots <= 4;
  bool can_planes = q > 0 && pieces <= 8 && (profile == PROFILE_DNA || iupac_planes);
  // Pieces of 6 rows, at most four of them, where the q-gram counting filter below finds nothing selective (m = 24, k = 3;
  // m = 18, k = 2; m = 12, k = 1): a window chunk in every sixteenth block is still less work for the fused launch than
  // the streaming DP over every block -- 0.85 against 1.03 ms per 3 GB (Iupac searcher: 0.94 against 1.29), m = 12, k = 1 with
  // its 13 764 matches 0.99 against 1.21.  Where the counting filter applies it stays (a 20-mer with k = 2: 0.76 against 0.79;
  // m = 27, k = 3: 0.72 against 0.87); five pieces, or pieces of 5 rows, lose against the streaming DP
  // (tools/probe_short_pieces.py).  SASSY_HIP_SHORT_PIECES=0: never.
  const bool env_short = sw.short_pieces != 0;
  const bool short_ok = q == 0 && env_pre < 0 && env_short && fuse_ok && !overhang && !ext_bitmap && !ext_desc && in.nslots <= 16 &&
                        !in.bytes && (profile == PROFILE_DNA || plain_pattern) && pieces <= 4 && m / pieces == 6;
  // (5-row pieces lose everywhere: m = 11, k = 1 takes 2.6 ms against 1.7 on the streaming DP, m = 15, k = 2 2.2 against 1.2)
  // The paired filter (filter_dna_kernel<.., PAIR>): S = ceil((k+1)/2) super-pieces of 2 Q rows, each with at most one of
  // the k edits -- one half exact, the other half with <= 1 edit right next to it, tested on the bit planes the lane
  // holds.  For the shapes whose k+1 pigeonhole pieces are 5 or 6 rows (m = 23, k = 3; m = 32, k = 4, 5; ...): the fused
  // launch, and only it (what it cannot finish goes to the paths below, as before).  SASSY_HIP_PAIR=0: never; 2: the
  // q-gram counting filter keeps the shapes it is selective for.
  const int env_pair = (int)sw.pair;
  uint32_t pair_s = 0, pair_q = 0;
  // (what only a job's route adds to pair_eligible(): an Iupac searcher's launch is the bit-plane launch with the text
  // check (switch iupac_planes), and its chunk DP builds up to eight slot masks for the rows behind the plain prefix)
  const bool pair_iupac_dp_ok = profile != PROFILE_IUPAC ||
                                (env_iupac_planes != 0 && (in.nslots <= 4 || (in.nslots <= 8 && in.nwords <= 4)));
  const bool pair_ok = pair_eligible(profile, sw, in.prefilter, pat, m, k, &pair_s, &pair_q) && pair_iupac_dp_ok && q == 0 && fuse_ok &&
                       !overhang && !ext_bitmap && !ext_desc && !in.bytes && (env_kind == 0 || env_kind == kFilterPlanes);
  // q-gram counting (count_filter.hip): per (Q, R) variant the threshold t = m + 1 - (k+1) Q, the
  // window W, and how often a window of random text reaches t by chance (the pattern's q-grams,
  // ambiguity letters expanded, against 4^Q; Poisson tail).  Taken when that beats the expected
  // hit blocks of the k+1 pieces, except where the cheaper bit-plane kernel applies (one strand: both
  // strands in one pass cost the bit-plane kernel 8 pieces, 0.85 ms per 3 GB, the counting kernel nothing extra).
  if (!overhang && !ext_bitmap && !ext_desc && !is_ascii(profile) && env_pre != 0 &&
      (env_kind == 0 || env_kind == kFilterCount) && !(can_planes && env_kind == 0 && !in.rc_bitmap) &&
      !(pair_ok && env_pair != 2)) {
    // two positions per lookup first (half the LDS traffic of (7,1)); the 7-gram variant only where
    // the shorter q-grams are not selective enough
    static const uint32_t variants[][2] = {{6, 2}, {5, 2}, {7, 1}};
    double best = 1.0;
    uint32_t bq = 0, br = 0;
    // the same pattern as in the last call on this lane: the decision and the table are still there
    const bool with_rc = in.rc_bitmap;
    std::vector<uint8_t> rc_fwd;  // the Rc strand's pattern as it reads on the forward text: reversed
    if (with_rc) rc_fwd.assign(std::reverse_iterator<const uint8_t*>(in.rc_pat + m), std::reverse_iterator<const uint8_t*>(in.rc_pat));
    const bool same_as_last = in.table_r != 0 && in.table_k == k && in.table_profile == (int)profile && in.table_rc == with_rc &&
                              table_pattern_same;
    if (same_as_last) { bq = lane_q; br = in.table_r; best = 0.0; }
    for (const auto& v : variants) {
      if (same_as_last) break;
      const uint32_t Q = v[0];
      if (v[1] == 1 && best < 1e-3) break;
      if ((uint64_t)pieces * Q > m) continue;  // t >= 1
      const uint32_t t = m + 1 - pieces * Q;
      const uint32_t W = (m + k - Q + 63) / 64 + 1;
      if (W > 64) continue;
      double grams = 0;  // expected size of H: the product of the rows' base-set sizes, per q-gram
      for (uint32_t o = 0; o + Q <= m; ++o) {
        double e = 1;
        for (uint32_t j = 0; j < Q; ++j)
          e *= profile == PROFILE_IUPAC ? (double)__builtin_popcount(iupac_code(pat[o + j]) & 15u) : 1.0;
        grams += e;
      }
      const double dens = std::min(1.0, (with_rc ? 2.0 : 1.0) * grams / std::pow(4.0, (double)Q));
      const double tail = clumped_tail(64.0 * W * dens, t);
      if (tail < (v[1] == 1 ? 0.1 * best : best)) { best = tail; bq = Q; br = v[1]; }
    }
    // (the piece-table kernel this competes with is the slower kernel -- 1.0 against 0.64 ms per 3 GB -- so a
    // modest candidate rate is enough; beyond ~5 % of the blocks the chunk DP behind it would dominate)
    if (bq && best < 0.05) {
      const bool cached = lane_q == bq && in.table_r == br && in.table_k == k && in.table_profile == (int)profile &&
                          in.table_rc == with_rc && table_pattern_same;
      bool ok = true;
      if (!cached) {
        ok = build_count_table(profile, pat, with_rc ? rc_fwd.data() : nullptr, m, bq, br, table, &density);
        if (!ok) { lane_q = 0; R.table_dropped = true; }
      }
      if (ok) {
        fkind = kFilterCount;
        R.table = kTableCount;
        R.table_q = bq; R.table_r = br;
        R.table_cached = cached;
        R.table_density = density;
        R.rc_marked = with_rc;
        q = bq;
        R.count_r = br;
        R.count_w = (m + k - bq + 63) / 64 + 1;
        R.count_t = m + 1 - pieces * bq;
        R.count_tail = clumped_tail(64.0 * R.count_w * density, R.count_t);
      }
    }
  }
  if (pair_ok && fkind != kFilterCount) {
    R.pair = pair_s;
    q = pair_q;
    iupac_planes = profile == PROFILE_IUPAC;
    can_planes = true;
  } else if (short_ok && fkind != kFilterCount) {
    q = m / pieces;
    iupac_planes = plain_pattern && in.nslots <= 4;
    can_planes = profile == PROFILE_DNA || iupac_planes;
  }
  bool filtered = q > 0;
  if (filtered && !ext_bitmap && !ext_desc && fkind != kFilterCount) {
    const bool can_table = !is_ascii(profile) && q >= 7;
    const bool can_generic = (uint64_t)pieces * q <= 255;   // its term table holds 256 piece rows
    if (can_planes && (env_kind == 0 || env_kind == kFilterPlanes)) fkind = kFilterPlanes;
    else if (can_table && (env_kind == 0 || env_kind == kFilterTable || !can_generic)) fkind = kFilterTable;
    else if (!can_generic) { q = 0; filtered = false; }  // too many piece rows for any filter: stream the full DP
    if (fkind == kFilterTable) {
      const uint32_t tq = std::min<uint32_t>(q, 9);
      const bool cached = lane_q == tq && in.table_r == 0 && in.table_k == k && in.table_profile == (int)profile && table_pattern_same;
      if (!cached && !build_qgram_table(profile, pat, tq, pieces, table)) {
        R.table_dropped = true;
        fkind = kFilterGeneric;
        if (!can_generic) { q = 0; filtered = false; }
      }
      if (fkind == kFilterTable) {
        q = tq;
        R.table = kTableQgram;
        R.table_q = tq; R.table_r = 0;
        R.table_cached = cached;
      }
    }
  }
  R.q = q;
  R.filtered = filtered;
  R.fkind = fkind;
  R.use_wave = use_wave;
  // The counting filter of ONE strand files its chunk descriptors itself (count_filter.hip, DIRECT): no hit bitmap (and no
  // 6 MB memset per 3 GB), no chunk-list launch.  Switch count_fused = 0: bitmap + build_chunks_kernel as before.
  R.count_direct = filtered && fkind == kFilterCount && !R.rc_marked && !ext_bitmap && !ext_desc && sw.count_fused != 0 &&
                   in.n_blocks < 0xFFFFFFFFull && !in.no_fuse && in.fuse_backoff == 0;
  // one launch for filter + chunk DP?  (bit-plane filter, one strand, one text, reports ranked by the
  // traceback waves themselves; the chunk DP's masks and carries must fit the filter's 8 KiB tile)
  R.fused = filtered && fkind == kFilterPlanes && fuse_ok;
  // the Iupac bit-plane filter exists as the fused launch only
  assert(!(profile == PROFILE_IUPAC && fkind == kFilterPlanes && !R.fused && !ext_bitmap && !ext_desc));
}

// ---- the filter's launch parameters, from the route ----

// piece_bits / piece_rem / piece_mirror of slot pp: piece `piece` of the forward pattern `src`, or (mirror) of the Rc
// strand's pattern with its string reversed: rows q-1 .. 0 of complement(pattern)'s piece, as they read on the forward text
inline void set_piece(ScanParams& X, const uint8_t* src, uint32_t m, uint32_t q, uint32_t pair, uint32_t pp, uint32_t piece, bool mirror) {
  uint32_t b0 = 0, b1 = 0;
  for (uint32_t j = 0; j < q; ++j) {
    const uint8_t ch = mirror ? src[piece * q + (q - 1 - j)] : src[piece * q + j];
    const uint32_t code = (ch >> 1) & 3u;  // src/profiles/dna.rs:19-40
    b0 |= (code & 1u) << j;
    b1 |= (code >> 1) << j;
  }
  X.piece_bits[pp][0] = b0;
  X.piece_bits[pp][1] = b1;
  X.piece_rem[pp] = m - (piece + 1) * q;
  // (paired filter: an A-type sub-piece is detected q + 2 columns behind its end)
  if (pair && (piece & 1u) == 0) X.piece_rem[pp] = (uint32_t)((int32_t)X.piece_rem[pp] - (int32_t)(q + 2));
  if (mirror) X.piece_mirror |= 1u << pp;
}

// What the route and the pattern decide of the filter launch F: piece geometry, the slot-mask filter's piece rows
// (piece_tab / piece_last), the counting filter's numbers, the bit-plane filter's pieces (piece_bits / piece_rem /
// piece_mirror, pair_y).  with_rc: the launch also marks the Rc strand's blocks -- in the same launch with up to four pieces
// per strand (*rc_marked), else in a second launch (*rc_marked and *rc_second_pass; rc_pieces() fills it).
inline void pack_filter(ScanParams& F, const Route& R, const std::vector<uint32_t>& row_tab, const uint8_t* pat, const uint8_t* rc_pat,
                        uint32_t m, uint32_t k, bool with_rc, bool* rc_marked, bool* rc_second_pass) {
  const uint32_t q = R.q, pair = R.pair;
  F.n_pieces = pair ? 2 * pair : k + 1;
  F.pair = pair;
  F.piece_len = q;
  F.piece_groups = F.n_pieces <= 4 ? 1u : F.n_pieces <= 8 ? 2u : 0u;
  if (F.piece_groups) {
    auto row_byte = [&](uint32_t r) { return (row_tab[r >> 2] >> (8 * (r & 3))) & 0xFFu; };
    for (uint32_t g = 0; g < F.piece_groups; ++g) {
      for (uint32_t j = 0; j < 12; ++j) F.piece_tab[g][j] = 0;
      F.piece_last[g] = 0;
      for (uint32_t pp = 0; pp < 4; ++pp) {
        uint32_t piece = 4 * g + pp;
        if (piece >= F.n_pieces) piece = 0;  // a repeated piece changes nothing
        for (uint32_t j = 0; j + 1 < q; ++j) F.piece_tab[g][j] |= row_byte(piece * q + j) << (8 * pp);
        F.piece_last[g] |= row_byte(piece * q + q - 1) << (8 * pp);
      }
    }
  }
  // Dna with <= 8 pieces: the filter works on the two code bit planes (filter_dna_kernel)
  F.piece_planes = R.fkind == kFilterPlanes ? 1u : 0u;
  F.count_r = R.count_r;
  F.count_window = R.count_w;
  F.count_thresh = R.count_t;
  F.piece_mirror = 0;
  F.count_rc = R.fkind == kFilterCount && R.rc_marked ? 1u : 0u;
  if (!F.piece_planes) return;
  if (pair) {
    for (uint32_t w = 0; w < 4; ++w) F.pair_y[w] = 0;
    for (uint32_t pp = 0; pp < 2 * pair; ++pp) {
      const uint32_t sib = pp ^ 1u;
      for (uint32_t j = 0; j < q; ++j) {
        // piece pp even (A): its B read forwards; odd (B): its A read backwards
        const uint32_t code = (pat[sib * q + ((pp & 1u) ? q - 1 - j : j)] >> 1) & 3u;
        F.pair_y[2 * (pp >> 2)] |= (code & 1u) << (8 * (pp & 3u) + j);
        F.pair_y[2 * (pp >> 2) + 1] |= (code >> 1) << (8 * (pp & 3u) + j);
      }
    }
  }
  const uint32_t np = k + 1;
  if (with_rc && np <= 4) {  // both strands' pieces in one launch (a repeated piece changes nothing)
    for (uint32_t pp = 0; pp < 4; ++pp) set_piece(F, pat, m, q, pair, pp, pp < np ? pp : 0, false);
    for (uint32_t pp = 0; pp < 4; ++pp) set_piece(F, rc_pat, m, q, pair, 4 + pp, pp < np ? pp : 0, true);
    F.n_pieces = 8;
    F.piece_groups = 2;
    *rc_marked = true;
  } else {
    for (uint32_t pp = 0; pp < 8; ++pp) set_piece(F, pat, m, q, pair, pp, pp < F.n_pieces ? pp : 0, false);
    if (with_rc) *rc_marked = *rc_second_pass = true;  // 5 .. 8 pieces per strand: a second launch for the Rc strand's pieces
  }
}

// The second launch's pieces: the Rc strand's (all mirrored) instead of the forward ones.
inline void rc_pieces(ScanParams& F2, const uint8_t* rc_pat, uint32_t m, uint32_t k, uint32_t q) {
  F2.piece_mirror = 0;
  for (uint32_t pp = 0; pp < 8; ++pp) set_piece(F2, rc_pat, m, q, 0, pp, pp < k + 1 ? pp : 0, true);
}

}  // namespace sassy_hip
