// all_alignments.hip -- Searcher::search_all_alignments on the device: every alignment of cost <= k at every end
// position of search_all (reference: src/search.rs:702-760 on top of src/alignment_iterator.rs:44-370).
//
// The end positions come from the library's own search (search_text with ALL_MINIMA | WITHOUT_TRACE: the searcher's
// strands, only_best_match and N-fraction endpoint filter apply as they do there).  Then two launches of
// enumerate_kernel over those ends, one lane per end:
//   count pass: alignments and cigar bytes (string + NUL) per end;
//   the host turns the counts into offsets and cuts the ends into batches whose output fits a fixed device buffer;
//   emit pass (per batch): the same DFS again, now writing sassy_hip_Match-layout rows and cigar text at the offsets.
// Writing to fixed per-end offsets keeps the output order deterministic without a sort.
//
// Per lane (DESIGN.md "search_all_alignments"):
//   * the (m+1) x (2k+3) cost band of trace_kernel.hip (window text[e-(m+k) .. e), top row 0, left column j, values
//     saturated at k+1).  Every cell of a <= k path, and every neighbour the edge test reads, lies within k diagonals
//     of the end's diagonal; there the band values are exact whenever they can decide an edge.
//   * for every band cell two bits of diagonal knowledge, so that both diagonal rules are O(1):
//       up(j, b):  pattern[0 .. j) equals the text on the cell's diagonal up to row 0 (the "may not leave" rule);
//       down(j, b): the row at which the exact-match run from the cell down its diagonal ends (the "may not enter" rule:
//                   entering is refused iff that row reaches the last row visited on the diagonal).  The run reads up
//                   to k+1 bytes past the end position, clipped to the text.
//   * the DFS stack (one frame per depth <= m+k: surviving edges in order, next edge, the saved last-row-on-diagonal
//     entry, net indels since the last '=') and the 2k+3 last-row-on-diagonal entries.
// Everything lives in a global scratch slice per lane, interleaved by lane (element x of lane l at x*64 + l) so that the
// fill passes, which every lane runs in step, load and store whole lines.
// The Rc strand runs on the reversed text without a copy of its own: byte x of the reversed text is fwd[n-1-x].
#include <hip/hip_runtime.h>

#include <cmath>

#include "host_internal.h"

namespace sassy_hip {

namespace {

__constant__ uint8_t kAaIupac[32] = {
    255, 1, 14, 2, 13, 255, 255, 8, 7, 255, 255, 12, 255, 3, 15, 255,
    255, 255, 9, 10, 4, 4, 11, 5, 0, 6, 255, 255, 255, 255, 255, 255};

// scan equality (the cost band) and Profile::is_match ('=' / 'X' and the diagonal rules), as profiles.h on the host
__device__ __forceinline__ bool aa_scan_eq(uint32_t pr, uint32_t p, uint32_t t) {
  if (pr == PROFILE_DNA) return ((p >> 1) & 3u) == ((t >> 1) & 3u);
  if (pr == PROFILE_IUPAC) return ((kAaIupac[p & 31u] & kAaIupac[t & 31u]) & 15u) != 0u;
  if (pr == PROFILE_ASCII_CI) return fold_ascii(p) == fold_ascii(t);
  return p == t;
}
__device__ __forceinline__ bool aa_is_match(uint32_t pr, uint32_t p, uint32_t t) {
  if (pr == PROFILE_DNA) return (p | 0x20u) == (t | 0x20u);
  if (pr == PROFILE_IUPAC) return (kAaIupac[p & 31u] & kAaIupac[t & 31u]) != 0u;
  if (pr == PROFILE_ASCII_CI) return fold_ascii(p) == fold_ascii(t);
  return p == t;
}

constexpr uint64_t kRcBit = 1ull << 63;
constexpr uint32_t kUpBit = 1u << 31;
enum : uint32_t { OP_EQ = 0, OP_X = 1, OP_D = 2, OP_I = 3 };

struct AaParams {
  const uint8_t* text;       // forward text (device)
  uint64_t n;
  const uint8_t* pat;        // pattern, then complement(pattern) (device, 2m bytes)
  uint32_t m, k, profile;
  uint32_t n_frac_on;
  float max_n_frac;
  const uint64_t* ends;      // end position in its strand's coordinates | kRcBit for the Rc strand
  uint32_t first, count;     // this launch: ends [first, first + count)
  // per-lane scratch: offsets (in elements * 64) of the arrays inside a wave's slice
  unsigned char* scratch;
  uint64_t wave_bytes;
  uint64_t off_cost, off_run, off_win, off_frame, off_saved, off_net, off_ops, off_last;
  // count pass (emit == 0)
  uint64_t* out_count;
  uint64_t* out_bytes;
  // emit pass
  int emit;
  const uint64_t* aln_off;   // global offsets of every end's first row / first cigar byte
  const uint64_t* byte_off;
  uint64_t aln_base, byte_base;  // this batch's first row / byte
  MatchOut* rows;
  char* pool;
};

template <typename T>
__device__ __forceinline__ T* lane_arr(const AaParams& P, unsigned char* wave, uint64_t off) {
  return reinterpret_cast<T*>(wave + off) + (threadIdx.x & 63u);
}

__global__ __launch_bounds__(64) void enumerate_kernel(const AaParams P) {
  const uint32_t lane = threadIdx.x & 63u;
  unsigned char* wave = P.scratch + (uint64_t)blockIdx.x * P.wave_bytes;
  uint16_t* cost = lane_arr<uint16_t>(P, wave, P.off_cost);
  uint32_t* run = lane_arr<uint32_t>(P, wave, P.off_run);
  uint8_t* win = lane_arr<uint8_t>(P, wave, P.off_win);
  uint16_t* frame = lane_arr<uint16_t>(P, wave, P.off_frame);
  uint32_t* saved = lane_arr<uint32_t>(P, wave, P.off_saved);
  int32_t* netv = lane_arr<int32_t>(P, wave, P.off_net);
  uint8_t* ops = lane_arr<uint8_t>(P, wave, P.off_ops);
  uint32_t* lastrow = lane_arr<uint32_t>(P, wave, P.off_last);
#define AA(a, x) (a)[(uint64_t)(x) * 64u]

  const int m = (int)P.m, k = (int)P.k;
  const int bw = 2 * k + 3, inf = k + 1;
  const uint64_t n = P.n;
  for (uint32_t u = blockIdx.x * 64u + lane; u < P.count; u += gridDim.x * 64u) {
    const uint32_t idx = P.first + u;
    const uint64_t ee = P.ends[idx];
    const bool rc = (ee & kRcBit) != 0;
    const uint64_t e = ee & ~kRcBit;                          // end position on the strand's text
    const uint8_t* pat = P.pat + (rc ? P.m : 0u);
    // window [o, e) of the band (trace_kernel.hip: report_window) and the bytes behind it the rules read
    const uint64_t fill = (uint64_t)m + (uint64_t)k;
    const uint64_t o = e > fill ? e - fill : 0;
    const int wl = (int)(e - o);
    const uint64_t wend = e + (uint64_t)k + 1 < n ? e + (uint64_t)k + 1 : n;
    const int wn = (int)(wend - o);
    for (int x = 0; x < wn; ++x) {
      const uint64_t g = o + (uint64_t)x;
      AA(win, x) = rc ? P.text[n - 1 - g] : P.text[g];
    }
    const int dlo = wl - m - k - 1;  // band column b of row j holds window column i = j + dlo + b
    // ---- cost band and the up-bits, rows 0 .. m ----
    for (int b = 0; b < bw; ++b) {
      const int i = dlo + b;
      AA(cost, b) = (uint16_t)((i < 0 || i > wl) ? inf : 0);
      AA(run, b) = kUpBit;  // row 0: the empty prefix matches
    }
    for (int j = 1; j <= m; ++j) {
      const uint32_t pc = pat[j - 1];
      int left = inf;
      for (int b = 0; b < bw; ++b) {
        const int i = j + dlo + b;
        const uint64_t c = (uint64_t)j * bw + b, cp = (uint64_t)(j - 1) * bw + b;
        int v;
        uint32_t up = 0;
        if (i < 0 || i > wl) v = inf;
        else if (i == 0) v = j < inf ? j : inf;
        else {
          const uint32_t tc = AA(win, i - 1);
          v = (int)AA(cost, cp) + (aa_scan_eq(P.profile, pc, tc) ? 0 : 1);
          const int l = left + 1;
          const int uu = (b + 1 < bw ? (int)AA(cost, cp + 1) : inf) + 1;
          v = v < l ? v : l;
          v = v < uu ? v : uu;
          v = v < inf ? v : inf;
          if (aa_is_match(P.profile, pc, tc)) up = AA(run, cp) & kUpBit;
        }
        AA(cost, c) = (uint16_t)v;
        AA(run, c) = up;
        left = v;
      }
    }
    // ---- down runs, rows m .. 0: the row at which the exact run from (j, i) down the diagonal ends ----
    for (int j = m; j >= 0; --j) {
      for (int b = 0; b < bw; ++b) {
        const uint64_t c = (uint64_t)j * bw + b;
        const int i = j + dlo + b;  // the run's first compare: pattern[j] against window byte i
        uint32_t r = (uint32_t)j;
        if (j < m && i >= 0 && i < wn && aa_is_match(P.profile, pat[j], AA(win, i)))
          r = AA(run, c + bw) & ~kUpBit;
        AA(run, c) = (AA(run, c) & kUpBit) | r;
      }
    }
    // ---- DFS from (m, wl) ----
    for (int b = 0; b < bw; ++b) AA(lastrow, b) = (uint32_t)m;
    uint64_t n_aln = 0, n_bytes = 0;
    uint64_t row_at = 0, byte_at = 0;
    if (P.emit) {
      row_at = P.aln_off[idx] - P.aln_base;
      byte_at = P.byte_off[idx] - P.byte_base;
    }
    int i = wl, j = m, c = 0, d = 0, net = 0;
    bool alive = (int)AA(cost, (uint64_t)m * bw + (k + 1)) <= k;
    bool enter = true;
    while (alive) {
      if (enter) {
        enter = false;
        if (j == 0) {
          // a complete alignment: [o + i, e) on this strand, ops[0 .. d) from the end back to the start
          bool keep = true;
          if (P.n_frac_on) {
            const int len = wl - i;
            if (len > 0 && o + (uint64_t)i < n) {
              int nn = 0;
              for (int x = i; x < wl; ++x) nn += ((AA(win, x) | 0x20u) == (uint32_t)'n') ? 1 : 0;
              keep = (float)nn / (float)len <= P.max_n_frac;
            }
          }
          if (keep) {
            // run-length encoded cigar, start -> end
            uint32_t w = 0;
            int x = d - 1;
            while (x >= 0) {
              const uint32_t op = AA(ops, x);
              int r = 1;
              while (x - r >= 0 && AA(ops, x - r) == op) ++r;
              x -= r;
              uint32_t p10 = 1;
              while (p10 * 10u <= (uint32_t)r) p10 *= 10u;
              if (P.emit) {
                uint32_t rr = (uint32_t)r;
                char* s = P.pool + byte_at + w;
                uint32_t q = 0;
                while (p10) { s[q++] = (char)('0' + rr / p10); rr %= p10; p10 /= 10u; }
                s[q++] = "=XDI"[op];
                w += q;
              } else {
                while (p10) { ++w; p10 /= 10u; }
                ++w;
              }
            }
            if (P.emit) {
              P.pool[byte_at + w] = 0;
              MatchOut rec;
              const uint64_t s0 = o + (uint64_t)i;
              rec.pattern_idx = 0;
              rec.text_idx = 0;
              rec.text_start = rc ? n - e : s0;
              rec.text_end = rc ? n - s0 : e;
              rec.pattern_start = 0;
              rec.pattern_end = P.m;
              rec.cost = c;
              rec.strand = rc ? 1 : 0;
              rec.pad_[0] = rec.pad_[1] = rec.pad_[2] = 0;
              rec.cigar_off = (uint32_t)(P.byte_base + byte_at);
              rec.cigar_len = w;
              P.rows[row_at] = rec;
              ++row_at;
              byte_at += w + 1;
            }
            ++n_aln;
            n_bytes += w + 1;
          }
          // nothing leaves row 0 (no 'D' there, src/alignment_iterator.rs:263-268): back up
          goto backtrack;
        }
        {
          // the surviving edges of (j, i), stably sorted by total cost; ties keep the order diagonal, D, I
          const int b = i - j - dlo;
          const uint64_t cc = (uint64_t)j * bw + b;
          const bool stay_up = (AA(run, cc) & kUpBit) != 0;  // the diagonal matches exactly up to row 0
          uint32_t eop[3];
          int etot[3];
          int ne = 0;
          auto push = [&](uint32_t op, int tot) {
            int q = ne++;
            while (q > 0 && etot[q - 1] > tot) { eop[q] = eop[q - 1]; etot[q] = etot[q - 1]; --q; }
            eop[q] = op;
            etot[q] = tot;
          };
          if (i >= 1) {
            const bool eq = aa_is_match(P.profile, pat[j - 1], AA(win, i - 1));
            const int tot = c + (eq ? 0 : 1) + (int)AA(cost, cc - bw);
            if (tot <= k) push(eq ? OP_EQ : OP_X, tot);
          }
          if (j != m && i >= 1 && b >= 1 && net <= 0 && !stay_up) {
            const int tot = c + 1 + (int)AA(cost, cc - 1);
            // entering diagonal b-1 at (j, i-1): refused if it runs exactly down to the last row visited on it
            if (tot <= k && (AA(run, cc - 1) & ~kUpBit) < AA(lastrow, b - 1)) push(OP_D, tot);
          }
          if (b + 1 < bw && net >= 0 && !stay_up) {
            const int tot = c + 1 + (int)AA(cost, cc - bw + 1);
            if (tot <= k && (AA(run, cc - bw + 1) & ~kUpBit) < AA(lastrow, b + 1)) push(OP_I, tot);
          }
          uint32_t f = (uint32_t)ne << 8;
          for (int q = 0; q < ne; ++q) f |= eop[q] << (2 * q);
          AA(frame, d) = (uint16_t)f;  // edges | count << 8 | next << 10
          AA(netv, d) = net;
        }
      }
      {  // take the next edge of frame d
        const uint32_t f = AA(frame, d);
        const uint32_t ne = (f >> 8) & 3u, nx = (f >> 10) & 3u;
        if (nx == ne) goto backtrack;
        AA(frame, d) = (uint16_t)((f & 0x3FFu) | ((nx + 1u) << 10));
        const uint32_t op = (f >> (2 * nx)) & 3u;
        int ni = i, nj = j;
        if (op != OP_I) --ni;
        if (op != OP_D) --nj;
        const int nb = ni - nj - dlo;
        AA(saved, d) = AA(lastrow, nb);
        AA(lastrow, nb) = (uint32_t)nj;
        AA(ops, d) = (uint8_t)op;
        c += op == OP_EQ ? 0 : 1;
        net = op == OP_EQ ? 0 : op == OP_I ? net + 1 : op == OP_D ? net - 1 : net;
        i = ni;
        j = nj;
        ++d;
        enter = true;
        continue;
      }
    backtrack:
      if (d == 0) break;
      {
        --d;
        const uint32_t op = AA(ops, d);
        const int b = i - j - dlo;
        AA(lastrow, b) = AA(saved, d);
        if (op != OP_I) ++i;
        if (op != OP_D) ++j;
        c -= op == OP_EQ ? 0 : 1;
        net = AA(netv, d);
      }
    }
    if (!P.emit) {
      P.out_count[idx] = n_aln;
      P.out_bytes[idx] = n_bytes;
    }
  }
#undef AA
}

}  // namespace

}  // namespace sassy_hip

// ------------------------------------------------------------------ host side

namespace {

// bytes of one lane's scratch arrays, rounded to 16 so that every array of the interleaved slice stays aligned
struct AaLayout {
  uint64_t cost, run, win, frame, saved, net, ops, last, lane_bytes;
};
AaLayout aa_layout(uint64_t m, uint64_t k) {
  auto r16 = [](uint64_t x) { return (x + 15u) & ~(uint64_t)15u; };
  const uint64_t cells = (m + 1) * (2 * k + 3), depth = m + k + 2;
  AaLayout L{};
  uint64_t at = 0;
  L.cost = at; at += r16(cells * 2);
  L.run = at; at += r16(cells * 4);
  L.win = at; at += r16(m + 2 * k + 2);
  L.frame = at; at += r16(depth * 2);
  L.saved = at; at += r16(depth * 4);
  L.net = at; at += r16(depth * 4);
  L.ops = at; at += r16(depth);
  L.last = at; at += r16((2 * k + 3) * 4);
  L.lane_bytes = at;
  return L;
}

constexpr uint64_t kAaScratchBytes = (uint64_t)128 << 20;  // DFS scratch of all waves of one launch
constexpr uint64_t kAaBatchRows = (uint64_t)1 << 19;       // default batch: 32 MiB of rows ...
constexpr uint64_t kAaBatchBytes = (uint64_t)32 << 20;     // ... and 32 MiB of cigar text

}  // namespace

int sassy_hip_search_all_alignments(sassy_SearcherType* s, const uint8_t* pattern, size_t pattern_len,
                                    const uint8_t* text, size_t text_len, size_t k, uint32_t flags,
                                    sassy_hip_Result** out) {
  if (!s || !pattern || (!text && text_len) || !out)
    return fail(SASSY_HIP_EINVAL, "Pointers in search_all_alignments() must not be null");
  SASSY_NO_LINE_SPANS(flags);
  if (flags & ~(uint32_t)(SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_TEXT_UNCHANGED))
    return fail(SASSY_HIP_EINVAL, "search_all_alignments takes SASSY_HIP_TEXT_ON_DEVICE / SASSY_HIP_TEXT_UNCHANGED only");
  SASSY_NO_TICKETS(s);
  if (!std::isnan(s->alpha))  // the reference asserts (src/alignment_iterator.rs:61-64)
    return fail(SASSY_HIP_EUNSUPPORTED, "search_all_alignments: tracing all alignments with overhang is not implemented");
  if (k > 0xFFF0u) return fail(SASSY_HIP_EINVAL, "search_all_alignments: k too large");
  DeviceGuard on_device(s);
  const double t0 = now_ms();
  reset_stats(s);
  // 1. the end positions: the library's own search_all without trace, under the searcher's settings
  std::unique_ptr<sassy_hip_Result> ends_res(new sassy_hip_Result());
  if (int rc = search_text(s, pattern, pattern_len, text, text_len, k,
                           flags | SASSY_HIP_ALL_MINIMA | SASSY_HIP_WITHOUT_TRACE, 0, true, s->rc, ends_res.get()))
    return rc;
  const sassy_hip_Stats search_stats = s->stats;
  std::unique_ptr<sassy_hip_Result> R(new sassy_hip_Result());
  const size_t n_found = ends_res->size();
  const uint64_t n = text_len;
  if (n_found == 0 || n == 0) {
    R->pool.push_back('\0');
    s->stats = search_stats;
    s->stats.trace_ms = 0;
    s->stats.total_ms = now_ms() - t0;
    *out = R.release();
    return 0;
  }
  // Fwd ends ascending, then Rc ends ascending on the reversed text (= descending text_start): the contract's order
  std::vector<uint64_t> fwd, rev;
  const sassy_hip_Match* fm = ends_res->data();
  for (size_t x = 0; x < n_found; ++x) {
    if (fm[x].strand) rev.push_back(n - fm[x].text_start);
    else fwd.push_back(fm[x].text_end);
  }
  std::stable_sort(fwd.begin(), fwd.end());
  std::stable_sort(rev.begin(), rev.end());
  std::vector<uint64_t> ends(fwd);
  for (uint64_t e : rev) ends.push_back(e | kRcBit);
  const uint32_t n_ends = (uint32_t)ends.size();

  const uint8_t* d_fwd = (flags & SASSY_HIP_TEXT_ON_DEVICE) ? text : s->d_text.p;  // what the search read
  hipStream_t st = s->stream;
  const uint64_t m = pattern_len;
  std::vector<uint8_t> pats(2 * m);
  for (size_t x = 0; x < m; ++x) {
    pats[x] = pattern[x];
    pats[m + x] = complement_char(s->profile, pattern[x]);
  }
  // device buffers of this call (freed when it returns)
  struct Dev {
    void* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
  } d_pat, d_ends, d_cnt, d_off, d_scr, d_rows, d_pool;
  HIP_TRY(hipMalloc(&d_pat.p, 2 * m + 16));
  HIP_TRY(hipMalloc(&d_ends.p, (size_t)n_ends * 8));
  HIP_TRY(hipMalloc(&d_cnt.p, (size_t)n_ends * 16));
  HIP_TRY(hipMalloc(&d_off.p, (size_t)n_ends * 16));
  HIP_TRY(hipMemcpyAsync(d_pat.p, pats.data(), 2 * m, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_ends.p, ends.data(), (size_t)n_ends * 8, hipMemcpyHostToDevice, st));

  const AaLayout lay = aa_layout(m, k);
  const uint64_t wave_bytes = lay.lane_bytes * 64u;
  const uint64_t need_waves = ((uint64_t)n_ends + 63u) / 64u;
  uint64_t waves = std::max<uint64_t>(1, kAaScratchBytes / wave_bytes);
  waves = std::min<uint64_t>(std::min<uint64_t>(waves, 2048), need_waves);
  HIP_TRY(hipMalloc(&d_scr.p, waves * wave_bytes));

  AaParams P{};
  P.text = d_fwd;
  P.n = n;
  P.pat = static_cast<const uint8_t*>(d_pat.p);
  P.m = (uint32_t)m;
  P.k = (uint32_t)k;
  P.profile = (uint32_t)s->profile;
  P.n_frac_on = std::isnan(s->max_n_frac) ? 0u : 1u;
  P.max_n_frac = s->max_n_frac;
  P.ends = static_cast<const uint64_t*>(d_ends.p);
  P.scratch = static_cast<unsigned char*>(d_scr.p);
  P.wave_bytes = wave_bytes;
  P.off_cost = lay.cost * 64u; P.off_run = lay.run * 64u; P.off_win = lay.win * 64u; P.off_frame = lay.frame * 64u;
  P.off_saved = lay.saved * 64u; P.off_net = lay.net * 64u; P.off_ops = lay.ops * 64u; P.off_last = lay.last * 64u;
  P.out_count = static_cast<uint64_t*>(d_cnt.p);
  P.out_bytes = P.out_count + n_ends;

  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  HIP_TRY(hipEventCreate(&ev0));
  struct EvGuard {
    hipEvent_t& a; hipEvent_t& b;
    ~EvGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  } evg{ev0, ev1};
  HIP_TRY(hipEventCreate(&ev1));
  float enum_ms = 0;

  // 2. count pass over all ends
  auto launch = [&](uint32_t first, uint32_t count) -> int {
    P.first = first;
    P.count = count;
    const uint64_t g = std::min<uint64_t>(waves, ((uint64_t)count + 63u) / 64u);
    hipLaunchKernelGGL(enumerate_kernel, dim3((uint32_t)g), dim3(64), 0, st, P);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  HIP_TRY(hipEventRecord(ev0, st));
  if (int rc = launch(0, n_ends)) return rc;
  HIP_TRY(hipEventRecord(ev1, st));
  std::vector<uint64_t> cnt(2 * (size_t)n_ends);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.p, cnt.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    enum_ms += ms;
  }
  // 3. offsets (exclusive prefix sums) and the host result
  std::vector<uint64_t> off(2 * (size_t)n_ends);
  uint64_t total = 0, total_bytes = 0;
  for (uint32_t x = 0; x < n_ends; ++x) {
    off[x] = total;
    off[n_ends + x] = total_bytes;
    total += cnt[x];
    total_bytes += cnt[n_ends + x];
  }
  if (total_bytes >= 0xFFFFFFFFull)
    return fail(SASSY_HIP_ENOMEM, "search_all_alignments: " + std::to_string(total) + " alignments with " +
                                      std::to_string(total_bytes) + " bytes of cigar text exceed the 4 GiB cigar pool");
  try {
    R->matches.resize(total);
    R->pool.resize(total_bytes ? total_bytes : 1, '\0');
  } catch (const std::bad_alloc&) {
    return fail(SASSY_HIP_ENOMEM, "search_all_alignments: out of host memory for " + std::to_string(total) + " alignments (" +
                                      std::to_string(total_bytes) + " bytes of cigar text)");
  }
  if (total) {
    HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
    // 4. batches: consecutive ends whose rows and cigar text fit the device buffers (an end larger than a batch on
    // its own is a batch of one, for which the buffers grow)
    uint64_t cap_rows = kAaBatchRows, cap_bytes = kAaBatchBytes;
    if (s->sw.aa_batch > 0) {
      cap_rows = (uint64_t)s->sw.aa_batch;
      cap_bytes = cap_rows * 16u;
    }
    struct Batch { uint32_t b0, b1; };
    std::vector<Batch> batches;
    uint64_t max_rows = 0, max_bytes = 0;
    for (uint32_t b0 = 0; b0 < n_ends;) {
      uint32_t b1 = b0;
      uint64_t r = 0, y = 0;
      while (b1 < n_ends && (b1 == b0 || (r + cnt[b1] <= cap_rows && y + cnt[n_ends + b1] <= cap_bytes))) {
        r += cnt[b1];
        y += cnt[n_ends + b1];
        ++b1;
      }
      if (r) batches.push_back(Batch{b0, b1});
      max_rows = std::max(max_rows, r);
      max_bytes = std::max(max_bytes, y);
      b0 = b1;
    }
    HIP_TRY(hipMalloc(&d_rows.p, max_rows * sizeof(MatchOut)));
    HIP_TRY(hipMalloc(&d_pool.p, max_bytes + 16));
    P.emit = 1;
    P.aln_off = static_cast<const uint64_t*>(d_off.p);
    P.byte_off = P.aln_off + n_ends;
    P.rows = static_cast<MatchOut*>(d_rows.p);
    P.pool = static_cast<char*>(d_pool.p);
    for (const Batch& bt : batches) {
      P.aln_base = off[bt.b0];
      P.byte_base = off[n_ends + bt.b0];
      const uint64_t r_end = bt.b1 < n_ends ? off[bt.b1] : total;
      const uint64_t y_end = bt.b1 < n_ends ? off[n_ends + bt.b1] : total_bytes;
      HIP_TRY(hipEventRecord(ev0, st));
      if (int rc = launch(bt.b0, bt.b1 - bt.b0)) return rc;
      HIP_TRY(hipEventRecord(ev1, st));
      HIP_TRY(hipMemcpyAsync(R->matches.data() + P.aln_base, d_rows.p, (r_end - P.aln_base) * sizeof(MatchOut),
                             hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(&R->pool[P.byte_base], d_pool.p, y_end - P.byte_base, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
      enum_ms += ms;
    }
  }
  s->stats = search_stats;
  s->stats.trace_ms = enum_ms;
  s->stats.candidates = n_ends;
  s->stats.total_ms = now_ms() - t0;
  *out = R.release();
  return 0;
}
