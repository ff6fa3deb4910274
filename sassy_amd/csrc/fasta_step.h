// fasta_step.h -- the arithmetic of the FASTA unwrap (fasta_unwrap.hip), free of HIP: plain C++17 that the device kernels and
// the host test driver (tests/c/fasta_step_driver.cc) compile alike.
//
// The definition is the line-by-line parse: split at '\n' (a final empty piece is no line), strip one trailing '\r' from each
// line, a line that begins with '>' opens a record, every other line is appended to the open record's sequence.  Per byte p of
// an input of n bytes:
//   line start    p == 0 or byte p - 1 is '\n'
//   header start  a line start whose byte is '>'
//   in header     the last line start at or in front of p is a header start (a header's own '\n' is a header byte)
//   kept          not in a header, not '\n', and not a '\r' whose next byte is '\n' or that is the input's last byte
// A lane works on 64 consecutive bytes as bit masks (bit b = byte b).  What it needs from outside is one bit from either
// side -- "the byte in front is '\n' (or this is position 0)", "the byte behind is '\n' (or the input ends there)" -- and the
// carried state "the line that is open where the lane begins is a header".  That state and the counts in front of a lane come
// from an ordered scan of lane summaries (FastaSum), which combine associatively.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SASSY_FA_HD __host__ __device__ __forceinline__
#else
#define SASSY_FA_HD inline
#endif

namespace sassy_hip {

constexpr uint32_t kFaLaneBytes = 64;
constexpr uint32_t kFaTileBytes = 4096;  // a wavefront's tile: 64 lanes x 64 bytes

SASSY_FA_HD uint32_t fa_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}
// the bits below bit i, 0 <= i <= 64
SASSY_FA_HD uint64_t fa_below(uint32_t i) { return i >= 64 ? ~0ull : (1ull << i) - 1ull; }

// The masks of one lane.  nl, gt, cr: byte b is '\n', '>', '\r'; len: how many of the 64 bytes lie inside the input (the
// masks hold no bit at len or above); prev_nl: the byte in front of the lane is '\n', or the lane begins the input; next_end:
// the byte behind the lane's 64 is '\n' or lies behind the input (read only when len == 64).
struct FastaLane {
  uint64_t ls;    // line starts
  uint64_t hs;    // header starts
  uint64_t cand;  // bytes that are kept unless they lie in a header
};
SASSY_FA_HD FastaLane fa_lane(uint64_t nl, uint64_t gt, uint64_t cr, uint32_t len, bool prev_nl, bool next_end) {
  const uint64_t valid = fa_below(len);
  FastaLane L;
  L.ls = ((nl << 1) | (prev_nl ? 1ull : 0ull)) & valid;
  L.hs = L.ls & gt;
  // bit b: byte b + 1 is '\n' or the input ends behind byte b
  uint64_t after = nl >> 1;
  if (len == 64) after |= next_end ? 1ull << 63 : 0ull;
  else if (len > 0) after |= 1ull << (len - 1);
  L.cand = valid & ~nl & ~(cr & after);
  return L;
}

// The in-header mask, given `in` = the line that is open at the lane's first byte is a header: bit b = HS[the last line start
// at or in front of b], `in` where there is none.  This is the carry chain of an adder that generates at header starts,
// propagates where no line starts and kills at the other line starts: A = hs | ~ls, B = hs, carry-in `in`; the carry INTO bit b
// is (A + B + in) ^ A ^ B, and the carry out of it is generate | propagate & carry-in.
SASSY_FA_HD uint64_t fa_in_header(uint64_t ls, uint64_t hs, bool in) {
  const uint64_t a = hs | ~ls, b = hs;
  const uint64_t into = (a + b + (in ? 1ull : 0ull)) ^ a ^ b;
  return hs | (~ls & into);
}
SASSY_FA_HD uint64_t fa_kept(const FastaLane& L, bool in) { return L.cand & ~fa_in_header(L.ls, L.hs, in); }

// What a stretch of bytes says to the stretches around it.  Count is uint32_t inside a tile or a super-tile, uint64_t above.
template <typename Count>
struct FastaSumT {
  uint32_t has_ls;    // the stretch holds a line start
  uint32_t last_hdr;  // its last line start is a header start (0 without one)
  Count kept_pre;     // kept candidates in front of its first line start: they count only if the carried state is "sequence"
  Count kept_post;    // kept bytes from its first line start on
  Count n_hdr;        // header starts
};
using FastaSum = FastaSumT<uint32_t>;
using FastaSum64 = FastaSumT<uint64_t>;

template <typename Count>
SASSY_FA_HD FastaSumT<Count> fa_identity() {
  return FastaSumT<Count>{0u, 0u, 0, 0, 0};
}

SASSY_FA_HD FastaSum fa_summary(const FastaLane& L) {
  FastaSum s;
  s.has_ls = L.ls != 0;
  const uint64_t pre = L.ls ? (L.ls & (0 - L.ls)) - 1ull : ~0ull;  // the bytes in front of the first line start
  const uint64_t hdr = fa_in_header(L.ls, L.hs, false);             // (exact from the first line start on)
  s.last_hdr = L.ls ? (uint32_t)(hdr >> 63) & 1u : 0u;              // bit 63 carries the last line start's value
  s.kept_pre = fa_popc(L.cand & pre);
  s.kept_post = fa_popc(L.cand & ~pre & ~hdr);
  s.n_hdr = fa_popc(L.hs);
  return s;
}

// a in front of b
template <typename CA, typename CB>
SASSY_FA_HD FastaSumT<CA> fa_combine(const FastaSumT<CA>& a, const FastaSumT<CB>& b) {
  FastaSumT<CA> r;
  r.has_ls = a.has_ls | b.has_ls;
  r.last_hdr = b.has_ls ? b.last_hdr : a.last_hdr;
  r.kept_pre = a.kept_pre + (a.has_ls ? (CA)0 : (CA)b.kept_pre);
  r.kept_post = a.kept_post + (CA)b.kept_post + ((a.has_ls && !a.last_hdr) ? (CA)b.kept_pre : (CA)0);
  r.n_hdr = a.n_hdr + (CA)b.n_hdr;
  return r;
}

// A summary applied to the state carried into its stretch.
template <typename Count>
SASSY_FA_HD bool fa_state_out(const FastaSumT<Count>& s, bool in) { return s.has_ls ? s.last_hdr != 0 : in; }
template <typename Count>
SASSY_FA_HD Count fa_kept_total(const FastaSumT<Count>& s, bool in) { return s.kept_post + (in ? (Count)0 : s.kept_pre); }

}  // namespace sassy_hip
