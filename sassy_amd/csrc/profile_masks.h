// profile_masks.h -- the alphabet profiles on the device: the bit planes of a lane's 64 text bytes and the slot masks
// (one 64-bit match mask per profile slot) every scanning unit builds from them.  Device code only; the host side of
// the profiles is profiles.h.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace sassy_hip {

// v_bitop3_b32 with an explicit truth table: result bit = TT[(a << 2) | (b << 1) | c].
template <int TT>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
__device__ __forceinline__ uint32_t mux(uint32_t s, uint32_t x0, uint32_t x1) {  // s ? x1 : x0
  return bitop3<0xAC>(s, x0, x1);
}

// ------------------------------------------------------------------ the profile, lane-parallel
// Bit-plane BIT of the lane's 64 text bytes: bit c of the result = bit BIT of byte c.
// Per dword: v_and isolates the bit of its 4 bytes, v_dot4_u32_u8 with weights 1,2,4,8 (even
// dword of a pair) / 16,32,64,128 (odd dword) gathers them; 8 chars land in bits BIT..BIT+7.
template <int BIT>
__device__ __forceinline__ uint2 bit_plane(const uint32_t (&x)[16]) {
  constexpr uint32_t kSel = 0x01010101u << BIT;
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t a = __builtin_amdgcn_udot4(x[2 * i] & kSel, 0x08040201u, 0u, false);
    v[i] = __builtin_amdgcn_udot4(x[2 * i + 1] & kSel, 0x80402010u, a, false);
  }
  uint2 r;
  r.x = (v[0] >> BIT) | (v[1] << (8 - BIT)) | (v[2] << (16 - BIT)) | (v[3] << (24 - BIT));
  r.y = (v[4] >> BIT) | (v[5] << (8 - BIT)) | (v[6] << (16 - BIT)) | (v[7] << (24 - BIT));
  return r;
}

// IUPAC letter (c & 31) -> low nibble of its base set; non-letters act as N (15), X = 0
// (reference: src/profiles/iupac.rs:281-330).  A=1 C=2 T=4 G=8.
__host__ __device__ constexpr int iupac_nib(int i) {
  return i == 1 ? 1 : i == 3 ? 2 : i == 20 ? 4 : i == 21 ? 4 : i == 7 ? 8 : i == 14 ? 15
       : i == 18 ? 9 : i == 25 ? 6 : i == 19 ? 10 : i == 23 ? 5 : i == 11 ? 12 : i == 13 ? 3
       : i == 2 ? 14 : i == 4 ? 13 : i == 8 ? 7 : i == 22 ? 11 : i == 24 ? 0 : 15;
}
// Truth table (index = b2*4 + b1*2 + b0) of output bit O of the nibble table for letters
// 8*HI .. 8*HI+7.
template <int O, int HI>
struct IupacTT {
  static constexpr int value() {
    int tt = 0;
    for (int i = 0; i < 8; ++i) tt |= ((iupac_nib(HI * 8 + i) >> O) & 1) << i;
    return tt;
  }
};
// Bit-sliced table lookup: base-set bit O of all 32 text chars of a half word, from the five
// letter-index planes b0..b4: Shannon expansion on b4, b3 over four 3-input functions.
template <int O>
__device__ __forceinline__ uint32_t iupac_base_plane(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3,
                                                     uint32_t b4) {
  const uint32_t g0 = bitop3<IupacTT<O, 0>::value()>(b2, b1, b0);
  const uint32_t g1 = bitop3<IupacTT<O, 1>::value()>(b2, b1, b0);
  const uint32_t g2 = bitop3<IupacTT<O, 2>::value()>(b2, b1, b0);
  const uint32_t g3 = bitop3<IupacTT<O, 3>::value()>(b2, b1, b0);
  return mux(b4, mux(b3, g0, g1), mux(b3, g2, g3));
}

// Byte mode (common.h: PROFILE_ASCII_BYTES), case-sensitive or folded.
__host__ __device__ constexpr bool bytes_profile(int profile) {
  return profile == (int)PROFILE_ASCII_BYTES || profile == (int)PROFILE_ASCII_CI_BYTES;
}
// PROFILE_ASCII_CI: plane 5 of the block's text with the upper-case letters folded onto the lower-case ones (the host
// folds the pattern the same way, profiles.h: make_plan).  A byte is an upper-case letter iff planes 7..5 read 010 and
// its low five bits are 1 .. 26: not 0 and not 27 .. 31 (11011, 111xx).  20 VALU per block, whatever the slot count.
__device__ __forceinline__ uint2 folded_plane5(const uint2 (&pl)[8]) {
  auto upper = [](uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t p4, uint32_t p5, uint32_t p6, uint32_t p7) {
    const uint32_t any = p0 | p1 | p2 | p3 | p4;
    const uint32_t high = p4 & p3 & (p2 | (p1 & p0));
    return p6 & ~(p7 | p5) & any & ~high;
  };
  return make_uint2(pl[5].x | upper(pl[0].x, pl[1].x, pl[2].x, pl[3].x, pl[4].x, pl[5].x, pl[6].x, pl[7].x),
                    pl[5].y | upper(pl[0].y, pl[1].y, pl[2].y, pl[3].y, pl[4].y, pl[5].y, pl[6].y, pl[7].y));
}

// Slot masks of one block from the lane's 64 text bytes.  m[s] = mask of slot s (lo, hi).
template <int PROFILE, int NS>
__device__ __forceinline__ void build_masks(const uint32_t (&x)[16], const ScanParams& P, uint2 (&m)[NS]) {
  if constexpr (PROFILE == PROFILE_DNA) {
    // code = (c >> 1) & 3: A=0 C=1 T=2 G=3 (reference: src/profiles/dna.rs:19-40)
    const uint2 p1 = bit_plane<1>(x), p2 = bit_plane<2>(x);
    m[0] = make_uint2(~(p1.x | p2.x), ~(p1.y | p2.y));
    m[1] = make_uint2(p1.x & ~p2.x, p1.y & ~p2.y);
    m[2] = make_uint2(~p1.x & p2.x, ~p1.y & p2.y);
    m[3] = make_uint2(p1.x & p2.x, p1.y & p2.y);
  } else if constexpr (PROFILE == PROFILE_IUPAC) {
    // mask[slot] = (base set of the text letter) intersects (base set of the slot's pattern
    // letter) (reference: src/profiles/iupac.rs:68-128)
    const uint2 b0 = bit_plane<0>(x), b1 = bit_plane<1>(x), b2 = bit_plane<2>(x), b3 = bit_plane<3>(x),
                b4 = bit_plane<4>(x);
    uint2 base[4];
    base[0] = make_uint2(iupac_base_plane<0>(b0.x, b1.x, b2.x, b3.x, b4.x), iupac_base_plane<0>(b0.y, b1.y, b2.y, b3.y, b4.y));
    base[1] = make_uint2(iupac_base_plane<1>(b0.x, b1.x, b2.x, b3.x, b4.x), iupac_base_plane<1>(b0.y, b1.y, b2.y, b3.y, b4.y));
    base[2] = make_uint2(iupac_base_plane<2>(b0.x, b1.x, b2.x, b3.x, b4.x), iupac_base_plane<2>(b0.y, b1.y, b2.y, b3.y, b4.y));
    base[3] = make_uint2(iupac_base_plane<3>(b0.x, b1.x, b2.x, b3.x, b4.x), iupac_base_plane<3>(b0.y, b1.y, b2.y, b3.y, b4.y));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const uint32_t sv = P.slot_val[s];  // wave-uniform; unused slots hold 0 -> empty mask
      uint2 r = make_uint2(0u, 0u);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const uint32_t sel = ((sv >> o) & 1u) ? 0xFFFFFFFFu : 0u;
        r.x |= base[o].x & sel;
        r.y |= base[o].y & sel;
      }
      m[s] = r;
    }
  } else if constexpr (bytes_profile(PROFILE)) {
    // byte mode: the eight bit planes themselves (dp_word compares them with the row's pattern byte)
    static_assert(NS == 8, "byte mode keeps eight planes");
    m[0] = bit_plane<0>(x); m[1] = bit_plane<1>(x); m[2] = bit_plane<2>(x); m[3] = bit_plane<3>(x);
    m[4] = bit_plane<4>(x); m[5] = bit_plane<5>(x); m[6] = bit_plane<6>(x); m[7] = bit_plane<7>(x);
    if constexpr (PROFILE == (int)PROFILE_ASCII_CI_BYTES) m[5] = folded_plane5(m);
  } else {
    // Ascii: byte equality with the slot's pattern byte (reference: src/profiles/ascii.rs:75-90)
    uint2 pl[8];
    pl[0] = bit_plane<0>(x); pl[1] = bit_plane<1>(x); pl[2] = bit_plane<2>(x); pl[3] = bit_plane<3>(x);
    pl[4] = bit_plane<4>(x); pl[5] = bit_plane<5>(x); pl[6] = bit_plane<6>(x); pl[7] = bit_plane<7>(x);
    if constexpr (PROFILE == (int)PROFILE_ASCII_CI) pl[5] = folded_plane5(pl);  // (the slots hold folded bytes)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const uint32_t sv = P.slot_val[s];
      uint2 r = (s < (int)P.nslots) ? make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu) : make_uint2(0u, 0u);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const uint32_t inv = ((sv >> b) & 1u) ? 0u : 0xFFFFFFFFu;  // XNOR with the slot's bit
        r.x &= pl[b].x ^ inv;
        r.y &= pl[b].y ^ inv;
      }
      m[s] = r;
    }
  }
}

}  // namespace sassy_hip
