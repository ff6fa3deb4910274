// amplicons.hip -- sassy_hip_hamming_amplicons: which products a primer pair makes, joined on the device (DESIGN.md 5.10,
// "Amplicons").
//
// The Hamming scan (hamming.hip: ham_scan_range) leaves the hits of every scanned pattern of a launch group in one range of
// tiles as items (pattern, block, 64-bit hit mask) sorted by (pattern, block).  A group scans, per pair, the LEFT patterns
// F (strand 0) and -- an rc searcher -- R (strand 1) in front of all PARTNER patterns rc(R) and rc(F), so the left hits are
// the first hits of the sorted list, in the contract's order (pair, strand, start).  Two kernels join them:
//   amp_count_kernel  a lane per left hit: its item and bit through the popcount prefix, the partner pattern's run of items
//                     from a small table, the partner window's first and last item by binary search, the count from a
//                     partial first and last mask and the prefix in between (amplicon_step.h).  A left hit that the range
//                     does not own counts 0.
//   amp_emit_kernel   a lane per record: a binary search in the scanned counts gives the left hit and j, amp_select the j-th
//                     partner, the two windows' text bytes both costs; one 24-byte record, in the contract's order.
// The counts are scanned on the host (4 bytes per left hit come back, 8 go out); the total is known there.
#include "host_internal.h"
#include "hamming_step.h"
#include "amplicon_step.h"

namespace sassy_hip {
namespace {

static_assert(kAmpTileBytes == (uint64_t)kHamTileBlocks * 64, "a tile of the scan");
static_assert(sizeof(sassy_hip_Amplicon) == 24, "the record is 24 bytes");

// per scanned pattern of a group, kAmpTabWords words: rows, offset of its bytes in `pats`, its partner's run of items [lo, hi),
// pair index of the call, strand, the partner's rows, offset of the partner's bytes
constexpr uint32_t kAmpTabWords = 8;

struct AmpParams {
  const uint8_t* text;
  const HamItem* items;    // sorted
  const uint32_t* prefix;  // n_items + 1: prefix[i] = hits of the items in front of item i
  uint32_t n_left_items;   // the items of the left patterns come first
  uint32_t n_left;         // their hits
  const uint32_t* tab;
  const uint8_t* pats;     // the patterns as scanned
  uint32_t profile;
  uint64_t min_len, max_len;
  uint64_t own_from, t1;   // the range's ownership (amp_owns)
  uint32_t last;
  uint32_t* counts;        // n_left
  const uint64_t* offs;    // n_left + 1: the exclusive scan of counts
  uint64_t first;          // emit: records [first, first + count) of the range
  uint32_t count;
  sassy_hip_Amplicon* out;
};

// left hit h of the range: its item and start
__device__ __forceinline__ uint64_t amp_left_hit(const AmpParams& A, uint32_t h, uint32_t* pattern) {
  uint32_t lo = 0, hi = A.n_left_items;  // the last item whose prefix is <= h
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (A.prefix[mid] <= h) lo = mid;
    else hi = mid;
  }
  const HamItem it = A.items[lo];
  uint64_t mask = it.mask;
  for (uint32_t skip = h - A.prefix[lo]; skip; --skip) mask &= mask - 1;
  *pattern = (uint32_t)(it.key >> 32);
  return (it.key & 0xFFFFFFFFull) * 64 + (uint32_t)__builtin_ctzll(mask);
}

__global__ __launch_bounds__(256) void amp_count_kernel(const AmpParams A) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= A.n_left) return;
  uint32_t p;
  const uint64_t s = amp_left_hit(A, h, &p);
  const uint32_t* row = A.tab + kAmpTabWords * p;
  uint64_t lo, hi, c = 0;
  if (amp_owns(s, A.own_from, A.t1, A.last != 0, A.max_len) && amp_window(s, A.min_len, A.max_len, row[0], row[6], row[6], &lo, &hi))
    c = amp_count([&](uint32_t i) { return A.items[i].key & 0xFFFFFFFFull; }, [&](uint32_t i) { return A.items[i].mask; },
                  [&](uint32_t i) { return A.prefix[i]; }, row[2], row[3], lo, hi);
  A.counts[h] = (uint32_t)c;  // (at most max_len <= 2^24 partners)
}

__global__ __launch_bounds__(256) void amp_emit_kernel(const AmpParams A) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= A.count) return;
  const uint64_t r = A.first + t;
  uint32_t a = 0, b = A.n_left;  // the last left hit whose offset is <= r: it has a record r
  while (b - a > 1) {
    const uint32_t mid = a + (b - a) / 2;
    if (A.offs[mid] <= r) a = mid;
    else b = mid;
  }
  uint32_t p;
  const uint64_t s = amp_left_hit(A, a, &p);
  const uint32_t* row = A.tab + kAmpTabWords * p;
  const uint32_t m = row[0], mq = row[6], strand = row[5];
  uint64_t lo = 0, hi = 0, q = 0;
  sassy_hip_Amplicon o{};
  const bool ok = amp_window(s, A.min_len, A.max_len, m, mq, mq, &lo, &hi) &&
                  amp_select([&](uint32_t i) { return A.items[i].key & 0xFFFFFFFFull; }, [&](uint32_t i) { return A.items[i].mask; },
                             [&](uint32_t i) { return A.prefix[i]; }, row[2], row[3], lo, hi, r - A.offs[a], &q);
  if (!ok) {  // (never: the count said there is one; the host refuses the call)
    o.pad_ = 1;
    A.out[t] = o;
    return;
  }
  uint32_t left_cost, right_cost, n_count, cigar_len;
  const uint8_t* lw = A.text + s;
  const uint8_t* rw = A.text + q;
  ham_emit_hit(A.profile, A.pats + row[1], m, [&](uint32_t i) { return (uint32_t)lw[i]; }, false, nullptr, &left_cost, &n_count, &cigar_len);
  ham_emit_hit(A.profile, A.pats + row[7], mq, [&](uint32_t i) { return (uint32_t)rw[i]; }, false, nullptr, &right_cost, &n_count, &cigar_len);
  o.start = s;
  o.end = q + mq;
  o.pair_idx = row[4];
  o.strand = (uint8_t)strand;
  o.fwd_cost = (uint8_t)(strand ? right_cost : left_cost);
  o.rev_cost = (uint8_t)(strand ? left_cost : right_cost);
  A.out[t] = o;
}

struct AmpPair {
  uint32_t idx;
  uint32_t nmax_f, nmax_r;
};

// The join proper: refusals are the caller's; d_text is readable up to the next multiple of 64 bytes.
int amplicons_on_device(sassy_SearcherType* S, const uint8_t* const* fwd, const size_t* fwd_lens, const uint8_t* const* rev,
                        const size_t* rev_lens, size_t n_pairs, const uint8_t* d_text, uint64_t n, uint32_t k, uint64_t min_len,
                        uint64_t max_len, std::vector<sassy_hip_Amplicon>& out) {
  const Profile pr = S->profile;
  hipStream_t st = S->stream;
  ScanLane& L = S->lanes[0];
  const uint64_t n_blocks = (n + 63) / 64, n_tiles = (n_blocks + kHamTileBlocks - 1) / kHamTileBlocks;
  if (n_blocks + kHamMaxHalo > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "text too long for the Hamming search (2^32 blocks)");
  S->stats.filtered = 7;
  S->stats.blocks_per_chunk = kHamTileBlocks;
  S->stats.chunks = n_tiles;

  // the pairs that can have a record at all
  std::vector<AmpPair> pairs;
  for (size_t i = 0; i < n_pairs; ++i) {
    const uint64_t a = fwd_lens[i], b = rev_lens[i];
    if (n < a || n < b || std::max(a, b) > max_len || std::max(std::max(a, b), min_len) > n) continue;
    uint32_t nmax[2] = {kHamNoFilter, kHamNoFilter};
    bool none = false;
    if (!std::isnan(S->max_n_frac))
      for (int e = 0; e < 2; ++e) {
        const uint32_t m = (uint32_t)(e ? b : a);
        const int64_t c = ham_n_max(m, S->max_n_frac);
        if (c < 0) none = true;  // not even a site without N passes
        else if (c < (int64_t)m) nmax[e] = (uint32_t)c;
      }
    if (!none) pairs.push_back(AmpPair{(uint32_t)i, nmax[0], nmax[1]});
  }
  auto revcomp = [&](const uint8_t* p, size_t m) {
    std::vector<uint8_t> r;
    for (size_t j = m; j-- > 0;) r.push_back(complement_char(pr, p[j]));
    return r;
  };
  const uint32_t sides = S->rc ? 2u : 1u;  // left patterns per pair, and partner patterns
  const long batch_sw = S->sw.hamming_batch, records_sw = S->sw.hamming_records;
  const size_t max_batch = batch_sw > 0 ? (size_t)batch_sw : 512;
  const size_t group_pairs = std::max<size_t>(1, max_batch / (2 * sides));  // a pair's patterns never straddle two groups
  const uint64_t rec_cap = records_sw > 0 ? (uint64_t)records_sw : (1u << 20);
  const uint64_t min_span = amp_min_span(max_len);
  uint64_t total = 0;  // records of the call; past 2^32 - 1 the ranges are only counted
  bool counting_only = false;

  for (size_t g0 = 0; g0 < pairs.size(); g0 += group_pairs) {
    const size_t gp = std::min(group_pairs, pairs.size() - g0);
    const uint32_t nl = (uint32_t)gp * sides, np = 2 * nl;
    std::vector<HamPattern> all(np);
    for (size_t q = 0; q < gp; ++q) {
      const AmpPair& P = pairs[g0 + q];
      const uint8_t *F = fwd[P.idx], *R = rev[P.idx];
      const size_t a = fwd_lens[P.idx], b = rev_lens[P.idx];
      all[q * sides] = HamPattern{P.idx, 0, std::vector<uint8_t>(F, F + a), P.nmax_f};
      all[nl + q * sides] = HamPattern{P.idx, 0, revcomp(R, b), P.nmax_r};
      if (S->rc) {
        all[q * sides + 1] = HamPattern{P.idx, 1, std::vector<uint8_t>(R, R + b), P.nmax_r};
        all[nl + q * sides + 1] = HamPattern{P.idx, 1, revcomp(F, a), P.nmax_f};
      }
    }
    HamRange G;
    ham_slots_init(pr, G);
    G.SP.nslots = G.ns;
    G.SP.profile = (uint32_t)pr;
    G.pats = all.data(); G.np = np;
    G.d_text = d_text; G.n = n; G.k = k;
    G.min_span = min_span;
    const size_t first_row = out.size();
    uint32_t ranges = 0;
    uint64_t tile0 = 0, own_from = 0;
    for (;;) {
      G.tile0 = tile0;
      G.span = n_tiles - tile0;  // everything that is left (ham_scan_range keeps it within what the counter takes)
      if (int rc = ham_scan_range(S, G)) return rc;
      const uint64_t t1 = tile0 + G.span;
      const bool last = t1 >= n_tiles;
      if (G.overflow || (!last && G.span < min_span))
        return fail(SASSY_HIP_ENOMEM, "hamming_amplicons: a range of " + std::to_string(min_span) + " tiles (max_len = " + std::to_string(max_len) +
                                          ") does not fit the item list of " + std::to_string(G.item_cap) + " items (" + std::to_string(G.count) +
                                          " items; option hamming_items)");
      ++ranges;
      const uint32_t count = G.count;
      const std::vector<HamItem>& items = G.items;
      // every pattern's run of items, the popcount prefix
      std::vector<uint32_t> run(np + 1, count), prefix((size_t)count + 1);
      uint64_t hits = 0;
      for (uint32_t i = count; i-- > 0;) run[(uint32_t)(items[i].key >> 32)] = i;
      for (uint32_t p = np; p-- > 0;) run[p] = std::min(run[p], run[p + 1]);  // (a pattern without items: an empty run)
      for (uint32_t i = 0; i < count; ++i) {
        prefix[i] = (uint32_t)hits;
        hits += (uint64_t)__builtin_popcountll(items[i].mask);
      }
      if (hits > 0xFFFFFFFFull) return fail(SASSY_HIP_ENOMEM, "hamming_amplicons: more than 2^32 primer sites in one range (" + std::to_string(hits) + ")");
      prefix[count] = (uint32_t)hits;
      const uint32_t n_left_items = run[nl], n_left = prefix[n_left_items];
      if (n_left != 0 && n_left_items != count) {
        std::vector<uint32_t> tab((size_t)np * kAmpTabWords, 0u);
        for (uint32_t p = 0; p < nl; ++p) {
          uint32_t* row = &tab[(size_t)p * kAmpTabWords];
          const uint32_t q = nl + p;  // its partner
          row[0] = G.tab[(size_t)p * kHamTabWords]; row[1] = G.tab[(size_t)p * kHamTabWords + 2];
          row[2] = run[q]; row[3] = run[q + 1];
          row[4] = all[p].idx; row[5] = all[p].strand;
          row[6] = G.tab[(size_t)q * kHamTabWords]; row[7] = G.tab[(size_t)q * kHamTabWords + 2];
        }
        if (int rc = S->d_amp_tab.reserve(tab.size())) return rc;
        if (int rc = S->d_ham_prefix.reserve((size_t)count + 1)) return rc;
        if (int rc = S->d_amp_counts.reserve(n_left)) return rc;
        HIP_TRY(hipMemcpyAsync(S->d_amp_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(S->d_ham_prefix.p, prefix.data(), ((size_t)count + 1) * 4, hipMemcpyHostToDevice, st));
        AmpParams A{};
        A.text = d_text; A.items = reinterpret_cast<const HamItem*>(S->d_ham_sorted.p); A.prefix = S->d_ham_prefix.p;
        A.n_left_items = n_left_items; A.n_left = n_left; A.tab = S->d_amp_tab.p; A.pats = G.d_pats; A.profile = (uint32_t)pr;
        A.min_len = min_len; A.max_len = max_len; A.own_from = own_from; A.t1 = t1; A.last = last ? 1u : 0u;
        A.counts = S->d_amp_counts.p;
        hipLaunchKernelGGL(amp_count_kernel, dim3((n_left + 255) / 256), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> counts(n_left);
        if (int rc = L.download(counts.data(), S->d_amp_counts.p, (size_t)n_left * 4)) return rc;
        HIP_TRY(hipStreamSynchronize(st));  // (the pageable uploads above are read by now)
        std::vector<uint64_t> offs((size_t)n_left + 1);
        uint64_t recs = 0;
        for (uint32_t h = 0; h < n_left; ++h) {
          offs[h] = recs;
          recs += counts[h];
        }
        offs[n_left] = recs;
        total += recs;
        if (total > 0xFFFFFFFFull && !counting_only) {
          counting_only = true;
          std::vector<sassy_hip_Amplicon>().swap(out);
        }
        if (recs && !counting_only) {
          if (int rc = S->d_amp_offs.reserve((size_t)n_left + 1)) return rc;
          HIP_TRY(hipMemcpyAsync(S->d_amp_offs.p, offs.data(), ((size_t)n_left + 1) * 8, hipMemcpyHostToDevice, st));
          const uint64_t batch = std::min<uint64_t>(recs, rec_cap);
          if (int rc = S->d_amp_out.reserve(batch)) return rc;
          A.offs = S->d_amp_offs.p;
          A.out = S->d_amp_out.p;
          for (uint64_t r0 = 0; r0 < recs; r0 += batch) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, recs - r0);
            A.first = r0; A.count = cnt;
            hipLaunchKernelGGL(amp_emit_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, A);
            HIP_TRY(hipGetLastError());
            const size_t at = out.size();
            out.resize(at + cnt);
            if (int rc = L.download(out.data() + at, S->d_amp_out.p, (size_t)cnt * sizeof(sassy_hip_Amplicon))) return rc;
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t i = at; i < out.size(); ++i)
              if (out[i].pad_ != 0) return fail(SASSY_HIP_EINVAL, "hamming_amplicons: internal error: a counted partner was not found");
          }
        }
        S->stats.candidates += recs;
      }
      if (last) break;
      own_from = amp_next_from(own_from, t1, max_len);
      tile0 = own_from / kAmpTileBytes;  // (beyond this range's first tile: it spans min_span tiles or more)
    }
    // several ranges: each came sorted by (pair, strand, start, end); the owned starts ascend from range to range, so a stable
    // sort restores the order
    if (ranges > 1 && !counting_only)
      std::stable_sort(out.begin() + (long)first_row, out.end(), [](const sassy_hip_Amplicon& a, const sassy_hip_Amplicon& b) {
        return a.pair_idx != b.pair_idx ? a.pair_idx < b.pair_idx : a.strand < b.strand;
      });
    S->stats.text_bytes += n;
  }
  if (counting_only) return fail(SASSY_HIP_ENOMEM, "hamming_amplicons: more than 2^32 - 1 records (" + std::to_string(total) + ")");
  return 0;
}

}  // namespace
}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_hamming_amplicons(sassy_SearcherType* s, const uint8_t* const* fwd, const size_t* fwd_lens, const uint8_t* const* rev,
                                const size_t* rev_lens, size_t n_pairs, const void* text, size_t text_len, size_t k, uint64_t min_len,
                                uint64_t max_len, uint32_t flags, sassy_hip_Amplicon** out, size_t* n_out) {
  if (!s || !out || !n_out || (n_pairs && (!fwd || !fwd_lens || !rev || !rev_lens)) || (!text && text_len))
    return fail(SASSY_HIP_EINVAL, "Pointers in hamming_amplicons() must not be null");
  *out = nullptr;
  *n_out = 0;
  if (flags & ~(uint32_t)(SASSY_HIP_TEXT_ON_DEVICE | SASSY_HIP_TEXT_UNCHANGED))
    return fail(SASSY_HIP_EINVAL, "hamming_amplicons takes SASSY_HIP_TEXT_ON_DEVICE and _TEXT_UNCHANGED only");
  if (is_ascii(s->profile))
    return fail(SASSY_HIP_EUNSUPPORTED, "hamming_amplicons takes dna and iupac searchers only: reverse complement is not defined for the ascii alphabet");
  if (k > 254) return fail(SASSY_HIP_EINVAL, "hamming_amplicons: k must be <= 254 (the Hamming family's costs are bytes)");
  if (min_len == 0) return fail(SASSY_HIP_EINVAL, "hamming_amplicons: min_len must be at least 1");
  if (min_len > max_len)
    return fail(SASSY_HIP_EINVAL, "hamming_amplicons: min_len (" + std::to_string(min_len) + ") is larger than max_len (" + std::to_string(max_len) + ")");
  if (max_len > SASSY_HIP_AMPLICON_MAX_LEN)
    return fail(SASSY_HIP_EINVAL, "hamming_amplicons: max_len (" + std::to_string(max_len) + ") is larger than SASSY_HIP_AMPLICON_MAX_LEN (" +
                                      std::to_string(SASSY_HIP_AMPLICON_MAX_LEN) + ")");
  // all 2 n_pairs primers through the family's one function: F_0, R_0, F_1, R_1, ...
  std::vector<const uint8_t*> pats(2 * n_pairs);
  std::vector<size_t> lens(2 * n_pairs);
  for (size_t i = 0; i < n_pairs; ++i) {
    pats[2 * i] = fwd[i]; lens[2 * i] = fwd_lens[i];
    pats[2 * i + 1] = rev[i]; lens[2 * i + 1] = rev_lens[i];
  }
  if (int rc = hamming_family_refusals(s, pats.data(), lens.data(), pats.size(), k, "hamming_amplicons")) return rc;
  DeviceGuard on_device(s);
  const double t0 = now_ms();
  reset_stats(s);
  if (int rc = s->ensure_device()) return rc;
  const uint8_t* d_text = static_cast<const uint8_t*>(text);
  if (flags & SASSY_HIP_TEXT_ON_DEVICE) {
    if (((uintptr_t)text & 15) != 0) return fail(SASSY_HIP_EINVAL, "device text pointer must be 16-byte aligned");
  } else if (text_len) {
    if (int rc = s->d_text.reserve(text_len + 64)) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_text.p, text, text_len, hipMemcpyHostToDevice, s->stream));
    d_text = s->d_text.p;
  }
  size_t longest = 0;
  for (size_t m : lens) longest = std::max(longest, m);
  const uint32_t kk = (uint32_t)std::min<size_t>(k, longest);  // k >= m: every start is a site
  std::vector<sassy_hip_Amplicon> recs;
  if (int rc = amplicons_on_device(s, fwd, fwd_lens, rev, rev_lens, n_pairs, d_text, text_len, kk, min_len, max_len, recs)) {
    (void)hipStreamSynchronize(s->stream);
    return rc;
  }
  if (!recs.empty()) {
    sassy_hip_Amplicon* p = static_cast<sassy_hip_Amplicon*>(malloc(recs.size() * sizeof(sassy_hip_Amplicon)));
    if (!p) return fail(SASSY_HIP_ENOMEM, "out of host memory (amplicon records)");
    memcpy(p, recs.data(), recs.size() * sizeof(sassy_hip_Amplicon));
    *out = p;
    *n_out = recs.size();
  }
  s->stats.total_ms = now_ms() - t0;
  return 0;
}

void sassy_hip_amplicons_free(sassy_hip_Amplicon* p) { free(p); }

}  // extern "C"
