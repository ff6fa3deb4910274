// profiles.h -- host side of the alphabet profiles (the reference's Profile trait for this path).
//
// Mirrors, per profile, exactly what the reference's Profile implementations expose to the search
// driver: pattern validation + encoding into profile slots, the scan equality, the traceback
// equality (is_match), complement / reverse complement.
//   Dna   : reference src/profiles/dna.rs:14-138
//   Iupac : reference src/profiles/iupac.rs:13-344
//   Ascii : reference src/profiles/ascii.rs:13-73 (case sensitive, what src/c.rs:64 instantiates)
//   Ascii, case-insensitive (PROFILE_ASCII_CI): Ascii<false>::is_match, ascii.rs:44-51, for the scan and the traceback
//           alike -- not the reference's own case-insensitive scan profile, which cannot match '_', '@', '[' or '\n'
//           with themselves
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"

namespace sassy_hip {

// IUPAC letter (5 low bits) -> base set, A=1 C=2 T=4 G=8; 255 = not a letter; X = empty set
// (reference: src/profiles/iupac.rs:281-317).
inline uint8_t iupac_code(uint8_t c) {
  static const uint8_t tab[32] = {
      /* 0 @ */ 255, /* A */ 1,   /* B */ 14,  /* C */ 2,   /* D */ 13,  /* E */ 255, /* F */ 255,
      /* G */ 8,     /* H */ 7,   /* I */ 255, /* J */ 255, /* K */ 12,  /* L */ 255, /* M */ 3,
      /* N */ 15,    /* O */ 255, /* P */ 255, /* Q */ 255, /* R */ 9,   /* S */ 10,  /* T */ 4,
      /* U */ 4,     /* V */ 11,  /* W */ 5,   /* X */ 0,   /* Y */ 6,   /* Z */ 255, 255,
      255,           255,         255,         255};
  return tab[c & 31];
}

// Scan equality = what the bit-parallel profile encodes.
inline bool scan_eq(Profile pr, uint8_t p, uint8_t t) {
  switch (pr) {
    case PROFILE_DNA: return ((p >> 1) & 3) == ((t >> 1) & 3);
    case PROFILE_IUPAC: return ((iupac_code(p) & iupac_code(t)) & 0x0F) != 0;
    case PROFILE_ASCII_CI: return fold_ascii(p) == fold_ascii(t);
    default: return p == t;
  }
}
// Traceback equality = Profile::is_match (dna.rs:48-50, iupac.rs:136-138, ascii.rs:44-51).
inline bool trace_is_match(Profile pr, uint8_t p, uint8_t t) {
  switch (pr) {
    case PROFILE_DNA: return (p | 0x20) == (t | 0x20);
    case PROFILE_IUPAC: return (iupac_code(p) & iupac_code(t)) > 0;
    case PROFILE_ASCII_CI: return fold_ascii(p) == fold_ascii(t);
    default: return p == t;
  }
}

// Iupac::valid_seq (iupac.rs:156-204).  Dna / Ascii patterns are never rejected by the reference.
inline bool valid_pattern(Profile pr, const uint8_t* p, size_t m) {
  if (pr != PROFILE_IUPAC) return true;
  for (size_t i = 0; i < m; ++i) {
    const uint8_t c = p[i] & (uint8_t)~0x20;
    if (c <= '@' || c >= 'Z' || iupac_code(c) == 255) return false;
  }
  return true;
}

inline uint8_t complement_char(Profile pr, uint8_t c) {
  if (pr == PROFILE_DNA) {  // dna.rs:121-133: upper-case ACGT only
    switch (c) {
      case 'A': return 'T';
      case 'C': return 'G';
      case 'T': return 'A';
      case 'G': return 'C';
      default: return c;
    }
  }
  // iupac.rs:235-278: IUPAC letters, both cases
  static const char from[] = "ACTGRYSWKMBDHVNX";
  static const char to[] = "TGACYRSWMKVHDBNX";
  for (int i = 0; from[i]; ++i) {
    if (c == (uint8_t)from[i]) return (uint8_t)to[i];
    if (c == (uint8_t)(from[i] | 0x20)) return (uint8_t)(to[i] | 0x20);
  }
  return c;
}

// The encoded pattern: which profile slot every row compares against, and what each slot tests.
struct PatternPlan {
  uint32_t m = 0;
  uint32_t nslots = 0;
  uint32_t nwords = 0;               // ceil(m / 32)
  uint8_t slot_val[kMaxSlots] = {};  // Dna: 2-bit code; Iupac: base-set nibble; Ascii: byte (PROFILE_ASCII_CI: folded)
  std::vector<uint32_t> row_tab;     // one byte per row = 2 * its profile slot, 4 rows per word,
                                     // 8 words per 32 rows (padded with slot 0)
  bool bytes = false;                // Ascii with more than kMaxSlots distinct (folded) bytes (PROFILE_ASCII_BYTES): nslots = 8
                                     // (the bit planes), the row table holds the pattern bytes themselves
  // class patterns (make_class_plan; PROFILE_CLASSES): a slot is a set of byte values
  bool classes = false;
  std::vector<uint32_t> class_tab;   // kClassTabWords words: slot headers, then the cubes (common.h)
  std::vector<uint8_t> class_bits;   // 32 bytes per slot: the set itself, for the traceback
};

// Profile::encode_pattern (dna.rs:19-23, iupac.rs:18-36, ascii.rs:18-29).
// Returns false with `err` set for what the reference would panic on.
inline bool make_plan(Profile pr, const uint8_t* pat, size_t m, PatternPlan& plan, std::string& err) {
  if (m == 0) { err = "empty pattern"; return false; }
  if (m > (1u << 20)) { err = "pattern longer than 2^20 is not supported"; return false; }
  plan.m = (uint32_t)m;
  plan.nwords = (uint32_t)((m + 31) / 32);
  plan.row_tab.assign((size_t)plan.nwords * 8, 0u);
  auto set_row = [&](size_t j, uint32_t slot) { plan.row_tab[j >> 2] |= (2u * slot) << (8 * (j & 3)); };
  std::vector<uint8_t> letters;
  if (pr == PROFILE_DNA) {
    plan.nslots = 4;
    for (int s = 0; s < 4; ++s) plan.slot_val[s] = (uint8_t)s;
    for (size_t j = 0; j < m; ++j) set_row(j, (uint32_t)((pat[j] >> 1) & 3));
    return true;
  }
  if (pr == PROFILE_IUPAC) {
    if (!valid_pattern(pr, pat, m)) {
      err = "Pattern is not valid IUPAC";  // iupac.rs:19-24 panics with this message
      return false;
    }
    letters = {'A', 'C', 'T', 'G'};
  }
  for (size_t j = 0; j < m; ++j) {
    // (PROFILE_ASCII_CI: one slot per folded byte -- 'l' and 'L' share it)
    const uint8_t c = pr == PROFILE_IUPAC ? (uint8_t)(pat[j] & ~0x20) : pr == PROFILE_ASCII_CI ? (uint8_t)fold_ascii(pat[j]) : pat[j];
    size_t s = 0;
    while (s < letters.size() && letters[s] != c) ++s;
    if (s == letters.size()) letters.push_back(c);
    if (s < (size_t)kMaxSlots) set_row(j, (uint32_t)s);
  }
  // Iupac: the reference's profile holds 16 masks and asserts (iupac.rs:69).  Ascii: 256 slots in the
  // reference (ascii.rs:13-29); here every distinct pattern byte takes one LDS mask slot per lane, up to
  // 64 of them; patterns with more distinct bytes run in byte mode (below).
  if (pr == PROFILE_IUPAC && letters.size() > 16) {
    err = "pattern uses more than 16 distinct letters";
    return false;
  }
  if (letters.size() > (size_t)kMaxSlots) {
    // Ascii, more distinct bytes than mask slots (the reference's profile has 256, ascii.rs:13-29): byte mode
    plan.bytes = true;
    plan.nslots = 8;
    plan.row_tab.assign((size_t)plan.nwords * 8, 0u);
    for (size_t j = 0; j < m; ++j)
      plan.row_tab[j >> 2] |= (pr == PROFILE_ASCII_CI ? fold_ascii(pat[j]) : (uint32_t)pat[j]) << (8 * (j & 3));
    return true;
  }
  plan.nslots = (uint32_t)letters.size();
  for (size_t s = 0; s < letters.size(); ++s)
    plan.slot_val[s] = pr == PROFILE_IUPAC ? (uint8_t)(iupac_code(letters[s]) & 0x0F) : letters[s];
  return true;
}

// ---- character classes: a pattern position is a set of byte values (256 bits: byte c at bit c & 7 of set[c >> 3]) ----
inline bool class_has(const uint8_t* set, uint32_t c) { return (set[c >> 3] >> (c & 7)) & 1u; }

// The runs of consecutive members of `set` (inverted: of its complement), each split into aligned power-of-two cubes --
// at most 14 per run (7 growing, 7 shrinking).  Cube i = (value[i], care[i]): byte c is in it iff ((c ^ value) & care) == 0.
// Writes the first `cap` cubes (value == nullptr: none) and returns how many there are.
inline size_t class_run_cubes(const uint8_t* set, bool inverted, uint8_t* value, uint8_t* care, size_t cap) {
  size_t n = 0;
  uint32_t c = 0;
  while (c < 256) {
    if (class_has(set, c) == inverted) { ++c; continue; }
    uint32_t hi = c;
    while (hi + 1 < 256 && class_has(set, hi + 1) != inverted) ++hi;
    uint32_t a = c;
    while (a <= hi) {
      uint32_t size = 1;
      while (2 * size <= 256 && (a & (2 * size - 1)) == 0 && a + 2 * size - 1 <= hi) size *= 2;
      if (value && n < cap) { value[n] = (uint8_t)a; care[n] = (uint8_t)(~(size - 1) & 0xFFu); }
      ++n;
      a += size;
    }
    c = hi + 1;
  }
  return n;
}
// The cover of one set: its own runs, or -- where that takes fewer cubes -- the runs of its complement (*complemented = 1:
// a byte is a member iff NO cube holds it).  Never more than 128 cubes: a set of n bytes takes at most n, its complement
// at most 256 - n.
inline size_t class_cover(const uint8_t* set, uint8_t* value, uint8_t* care, size_t cap, int* complemented) {
  const size_t plain = class_run_cubes(set, false, nullptr, nullptr, 0);
  const size_t inv = class_run_cubes(set, true, nullptr, nullptr, 0);
  const bool use_inv = inv < plain;
  if (complemented) *complemented = use_inv ? 1 : 0;
  return class_run_cubes(set, use_inv, value, care, cap);
}

// The plan of a class pattern: `sets` holds m sets of 32 bytes.  Distinct sets become slots (PROFILE_ASCII_CI: after
// closing every set under the A-Z / a-z twin); `rows` receives the slot of every row -- the "pattern" the traceback sees.
inline bool make_class_plan(Profile pr, const uint8_t* sets, size_t m, PatternPlan& plan, std::vector<uint8_t>& rows, std::string& err) {
  if (m == 0) { err = "empty pattern"; return false; }
  if (m > (1u << 20)) { err = "pattern longer than 2^20 is not supported"; return false; }
  plan = PatternPlan{};
  plan.classes = true;
  plan.m = (uint32_t)m;
  plan.nwords = (uint32_t)((m + 31) / 32);
  plan.row_tab.assign((size_t)plan.nwords * 8, 0u);
  rows.assign(m, 0);
  std::vector<uint8_t> slots;  // 32 bytes each
  for (size_t j = 0; j < m; ++j) {
    uint8_t set[32];
    memcpy(set, sets + 32 * j, 32);
    if (pr == PROFILE_ASCII_CI)
      for (uint32_t c = 'A'; c <= 'Z'; ++c)
        if (class_has(set, c) || class_has(set, c | 0x20u)) {
          set[c >> 3] |= (uint8_t)(1u << (c & 7));
          set[(c | 0x20u) >> 3] |= (uint8_t)(1u << ((c | 0x20u) & 7));
        }
    size_t s = 0;
    const size_t ns = slots.size() / 32;
    while (s < ns && memcmp(slots.data() + 32 * s, set, 32) != 0) ++s;
    if (s == ns) {
      if (ns == (size_t)kMaxSlots) {
        err = "class pattern uses more than " + std::to_string(kMaxSlots) + " distinct sets";
        return false;
      }
      slots.insert(slots.end(), set, set + 32);
    }
    rows[j] = (uint8_t)s;
    plan.row_tab[j >> 2] |= (2u * (uint32_t)s) << (8 * (j & 3));
  }
  plan.nslots = (uint32_t)(slots.size() / 32);
  plan.class_bits = slots;
  plan.class_tab.assign(kClassTabWords, 0u);
  uint32_t total = 0;
  for (uint32_t s = 0; s < plan.nslots; ++s) {
    uint8_t value[128], care[128];
    int inv = 0;
    const uint32_t n = (uint32_t)class_cover(slots.data() + 32 * s, value, care, 128, &inv);
    if (total + n > kMaxClassCubes) {
      err = "class pattern needs more than " + std::to_string(kMaxClassCubes) + " cubes (SASSY_HIP_CLASS_MAX_CUBES)";
      return false;
    }
    plan.class_tab[s] = total | (n << 16) | (inv ? 0x80000000u : 0u);
    for (uint32_t i = 0; i < n; ++i) plan.class_tab[kMaxSlots + total + i] = (uint32_t)value[i] | ((uint32_t)care[i] << 8);
    total += n;
  }
  return true;
}

}  // namespace sassy_hip
