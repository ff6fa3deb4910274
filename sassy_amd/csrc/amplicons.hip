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

// The join proper: refusals are the caller's.
int amplicons_on_device(sassy_SearcherType* S, const uint8_t* const* fwd, const size_t* fwd_lens, const uint8_t* const* rev,
                        const size_t* rev_lens, size_t n_pairs, const HamText& text, uint32_t k, uint64_t min_len, uint64_t max_len,
                        std::vector<sassy_hip_Amplicon>& out) {
  const Profile pr = S->profile;
  hipStream_t st = S->stream;
  ScanLane& L = S->lanes[0];
  const uint64_t n = text.n, n_tiles = text.n_tiles();
  if (text.n_blocks() + kHamMaxHalo > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "text too long for the Hamming search (2^32 blocks)");
  S->stats.filtered = 7;
  S->stats.blocks_per_chunk = kHamTileBlocks;
  S->stats.chunks = n_tiles;

  // the pairs that can have a record at all, four scanned patterns each: F, rc(F), R, rc(R)
  std::vector<HamPattern> primers;
  auto complement = [pr](uint8_t c) { return complement_char(pr, c); };
  for (size_t i = 0; i < n_pairs; ++i) {
    const uint64_t a = fwd_lens[i], b = rev_lens[i];
    if (n < a || n < b || std::max(a, b) > max_len || std::max(std::max(a, b), min_len) > n) continue;
    const size_t at = primers.size();
    if (!ham_add_scanned((uint32_t)i, fwd[i], a, true, S->max_n_frac, n, complement, primers) ||
        !ham_add_scanned((uint32_t)i, rev[i], b, true, S->max_n_frac, n, complement, primers))
      primers.resize(at);  // not even a site without N passes
  }
  const uint32_t sides = S->rc ? 2u : 1u;  // left patterns per pair, and partner patterns
  const size_t group_pairs = ham_group_pairs(ham_batch_patterns(S->sw.hamming_batch), sides), kept = primers.size() / 4;
  const uint64_t min_span = amp_min_span(max_len);
  uint64_t total = 0;  // records of the call; past 2^32 - 1 the ranges are only counted
  bool counting_only = false;

  for (size_t g0 = 0; g0 < kept; g0 += group_pairs) {
    const size_t gp = std::min(group_pairs, kept - g0);
    const uint32_t nl = (uint32_t)gp * sides, np = 2 * nl;
    std::vector<HamPattern> all(np);  // the left patterns F and -- rc -- R, then their partners rc(R) and rc(F)
    for (size_t q = 0; q < gp; ++q) {
      const HamPattern* P4 = &primers[4 * (g0 + q)];
      all[q * sides] = P4[0];
      all[nl + q * sides] = P4[3];
      all[nl + q * sides].strand = 0;
      if (S->rc) {
        all[q * sides + 1] = P4[2];
        all[q * sides + 1].strand = 1;
        all[nl + q * sides + 1] = P4[1];
      }
    }
    HamJob J;
    J.group = ham_next_group((uint32_t)pr, all, 0, np);  // (Dna and Iupac: every pattern shares the slots)
    J.pats = all.data(); J.np = np;
    J.text = text; J.k = k; J.min_span = min_span;
    HamPrepared P;
    if (int rc = ham_prepare(S, J, P)) return rc;
    const size_t first_row = out.size();
    uint64_t own_from = 0;
    auto per_range = [&](const HamRangeOut& range, uint64_t t1, bool last, uint64_t* next) {
      if (range.overflow || (!last && range.span < min_span))
        return fail(SASSY_HIP_ENOMEM, "hamming_amplicons: a range of " + std::to_string(min_span) + " tiles (max_len = " + std::to_string(max_len) +
                                          ") does not fit the item list of " + std::to_string(P.item_cap) + " items (" + std::to_string(range.count) +
                                          " items; option hamming_items)");
      const uint32_t count = range.count;
      // every pattern's run of items, the popcount prefix
      std::vector<uint32_t> run(np + 1, count), prefix;
      uint64_t hits = 0;
      for (uint32_t i = count; i-- > 0;) run[(uint32_t)(range.items[i].key >> 32)] = i;
      for (uint32_t p = np; p-- > 0;) run[p] = std::min(run[p], run[p + 1]);  // (a pattern without items: an empty run)
      if (!ham_prefix(range.items, 0, prefix, &hits))
        return fail(SASSY_HIP_ENOMEM, "hamming_amplicons: more than 2^32 primer sites in one range (" + std::to_string(hits) + ")");
      const uint32_t n_left_items = run[nl], n_left = prefix[n_left_items];
      if (n_left != 0 && n_left_items != count) {
        std::vector<uint32_t> tab((size_t)np * kAmpTabWords, 0u);
        for (uint32_t p = 0; p < nl; ++p) {
          uint32_t* row = &tab[(size_t)p * kAmpTabWords];
          const uint32_t q = nl + p;  // its partner
          row[0] = P.t.tab[(size_t)p * kHamTabWords]; row[1] = P.t.tab[(size_t)p * kHamTabWords + 2];
          row[2] = run[q]; row[3] = run[q + 1];
          row[4] = all[p].idx; row[5] = all[p].strand;
          row[6] = P.t.tab[(size_t)q * kHamTabWords]; row[7] = P.t.tab[(size_t)q * kHamTabWords + 2];
        }
        if (int rc = S->d_amp_tab.reserve(tab.size())) return rc;
        if (int rc = S->d_amp_counts.reserve(n_left)) return rc;
        HIP_TRY(hipMemcpyAsync(S->d_amp_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        if (int rc = S->d_ham_prefix.reserve(prefix.size())) return rc;
        HIP_TRY(hipMemcpyAsync(S->d_ham_prefix.p, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, st));
        AmpParams A{};
        A.text = text.d_text; A.items = reinterpret_cast<const HamItem*>(S->d_ham_sorted.p); A.prefix = S->d_ham_prefix.p;
        A.n_left_items = n_left_items; A.n_left = n_left; A.tab = S->d_amp_tab.p; A.pats = P.d_pats; A.profile = (uint32_t)pr;
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
          auto reserve = [&](uint64_t batch) { return S->d_amp_out.reserve(batch); };
          auto emit = [&](uint64_t r0, uint32_t cnt) {
            A.offs = S->d_amp_offs.p; A.out = S->d_amp_out.p;
            A.first = r0; A.count = cnt;
            hipLaunchKernelGGL(amp_emit_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, A);
            HIP_TRY(hipGetLastError());
            const size_t at = out.size();
            out.resize(at + cnt);
            if (int rc = L.download(out.data() + at, S->d_amp_out.p, (size_t)cnt * sizeof(sassy_hip_Amplicon))) return rc;
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t i = at; i < out.size(); ++i)
              if (out[i].pad_ != 0) return fail(SASSY_HIP_EINVAL, "hamming_amplicons: internal error: a counted partner was not found");
            return 0;
          };
          if (int rc = ham_emit_batches(S, recs, reserve, emit)) return rc;
        }
        S->stats.candidates += recs;
      }
      if (!last) {
        own_from = amp_next_from(own_from, t1, max_len);
        *next = own_from / kAmpTileBytes;  // (beyond this range's first tile: it spans min_span tiles or more)
      }
      return 0;
    };
    // several ranges: each came sorted by (pair, strand, start, end); the owned starts ascend from range to range, so a stable
    // sort restores the order
    auto reorder = [&] {
      if (!counting_only)
        std::stable_sort(out.begin() + (long)first_row, out.end(), [](const sassy_hip_Amplicon& a, const sassy_hip_Amplicon& b) {
          return a.pair_idx != b.pair_idx ? a.pair_idx < b.pair_idx : a.strand < b.strand;
        });
    };
    if (int rc = ham_walk_ranges(S, J, P, per_range, reorder)) return rc;
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
  if (int rc = hamming_refusals(s, pats.data(), lens.data(), pats.size(), k, "hamming_amplicons")) return rc;
  return hamming_call(s, lens.data(), lens.size(), k, [&](uint32_t kk) {  // (k >= m: every start is a site)
    HamText one;
    if (int rc = ham_one_text(s, text, text_len, flags, &one)) return rc;
    std::vector<sassy_hip_Amplicon> recs;
    if (int rc = amplicons_on_device(s, fwd, fwd_lens, rev, rev_lens, n_pairs, one, kk, min_len, max_len, recs)) return rc;
    if (!recs.empty()) {
      sassy_hip_Amplicon* p = static_cast<sassy_hip_Amplicon*>(malloc(recs.size() * sizeof(sassy_hip_Amplicon)));
      if (!p) return fail(SASSY_HIP_ENOMEM, "out of host memory (amplicon records)");
      memcpy(p, recs.data(), recs.size() * sizeof(sassy_hip_Amplicon));
      *out = p;
      *n_out = recs.size();
    }
    return 0;
  });
}

void sassy_hip_amplicons_free(sassy_hip_Amplicon* p) { free(p); }

}  // extern "C"
