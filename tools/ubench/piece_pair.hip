// Microbenchmark for the piece test of the grouped text pass (filter_dna_kernel<.., G = 2>; profiles/r12_piece_pair.txt).
//   1. explicit-register rows: v_bitop3_b32 with a scalar third source against three vector sources, a scalar constant's
//      way into a vector register (v_mov_b32, v_bfe_i32), and s_bfe_i32 read by the very next vector instruction;
//   2. the kernel's block in its own shape, three waves per SIMD (45 184 B of LDS per workgroup and at most 168 VGPRs,
//      as the kernel has them): today's per-block form against the block-pair form with its constants in vector registers;
//   3. the LDS-table body at three waves per SIMD and 45 184 + Q x 64 B of LDS per workgroup against four waves and
//      40 064 + Q x 64 B (the plane reader's own layout, csrc/pass_lds.h; profiles/r13_reader_occupancy.txt): each alone and
//      as two launches side by side on two streams, the rows alternating three times.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -o piece_pair piece_pair.hip
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define R4(x) x x x x
#define R16(x) R4(R4(x))
#define VCLOB "v100","v101","v102","v103","v104","v105","v106","v107","v108","v109","v110","v111","v112","v113","v114","v115","v116","v117","v118","v119","v120","v121","v122","v123"
#define SCLOB "s20","s21","s22","s23","s24","s25","s26","s27","s28","s29","scc"
// each BODY string is one unit of eight vector instructions on v100..v123 (scalar ones come on top); s20..s27 hold 0 / ~0
// words, s28 and s29 piece words
#define DEFK(NAME, BODY)                                                               \
  __global__ __launch_bounds__(256) void NAME(unsigned* out, int iters) {                \
    asm volatile("v_mov_b32 v100, 1\n v_mov_b32 v101, 2\n v_mov_b32 v102, 3\n v_mov_b32 v103, 4\n" \
                 "v_mov_b32 v104, 5\n v_mov_b32 v105, 6\n v_mov_b32 v106, 7\n v_mov_b32 v107, 8\n" \
                 "v_mov_b32 v108, 9\n v_mov_b32 v109, 10\n v_mov_b32 v110, 11\n v_mov_b32 v111, 12\n" \
                 "v_mov_b32 v112, 13\n v_mov_b32 v113, 14\n v_mov_b32 v114, 15\n v_mov_b32 v115, 16\n" \
                 "v_mov_b32 v116, 9\n v_mov_b32 v117, 10\n v_mov_b32 v118, 11\n v_mov_b32 v119, 12\n" \
                 "v_mov_b32 v120, 13\n v_mov_b32 v121, 14\n v_mov_b32 v122, 15\n v_mov_b32 v123, 16\n" \
                 "s_mov_b32 s20, 0\n s_mov_b32 s21, -1\n s_mov_b32 s22, 0\n s_mov_b32 s23, -1\n"  \
                 "s_mov_b32 s24, -1\n s_mov_b32 s25, 0\n s_mov_b32 s26, -1\n s_mov_b32 s27, 0\n" \
                 "s_mov_b32 s28, 0x5a\n s_mov_b32 s29, 0xc3\n" ::: VCLOB, SCLOB);        \
    for (int it = 0; it < iters; ++it) {                                                 \
      asm volatile(R16(BODY) ::: VCLOB, SCLOB, "vcc");                                   \
    }                                                                                    \
    unsigned r;                                                                          \
    asm volatile("v_xor_b32 %0, v100, v104" : "=v"(r));                                  \
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;                                      \
  }
// eight independent bitop3 (a & (b ^ c)), every source a VGPR of its own bank
DEFK(k_b3_vvv, "v_bitop3_b32 v100, v101, v102, v103 bitop3:0x60\n v_bitop3_b32 v104, v105, v106, v107 bitop3:0x60\n v_bitop3_b32 v108, v109, v110, v111 bitop3:0x60\n v_bitop3_b32 v112, v113, v114, v115 bitop3:0x60\n"
               "v_bitop3_b32 v116, v117, v118, v119 bitop3:0x60\n v_bitop3_b32 v120, v121, v122, v123 bitop3:0x60\n v_bitop3_b32 v100, v105, v110, v115 bitop3:0x60\n v_bitop3_b32 v104, v109, v114, v119 bitop3:0x60\n")
// the same eight, the third source an SGPR
DEFK(k_b3_vvs, "v_bitop3_b32 v100, v101, v102, s20 bitop3:0x60\n v_bitop3_b32 v104, v105, v106, s21 bitop3:0x60\n v_bitop3_b32 v108, v109, v110, s22 bitop3:0x60\n v_bitop3_b32 v112, v113, v114, s23 bitop3:0x60\n"
               "v_bitop3_b32 v116, v117, v118, s24 bitop3:0x60\n v_bitop3_b32 v120, v121, v122, s25 bitop3:0x60\n v_bitop3_b32 v100, v105, v110, s26 bitop3:0x60\n v_bitop3_b32 v104, v109, v114, s27 bitop3:0x60\n")
// accumulator chains as the kernel has them (dst = first source), VGPR constants: every accumulator is read again four
// instructions later (the pair form) ...
DEFK(k_b3_acc4_v, "v_bitop3_b32 v100, v100, v101, v120 bitop3:0x60\n v_bitop3_b32 v104, v104, v105, v120 bitop3:0x60\n v_bitop3_b32 v108, v108, v109, v120 bitop3:0x60\n v_bitop3_b32 v112, v112, v113, v120 bitop3:0x60\n"
                  "v_bitop3_b32 v100, v100, v102, v121 bitop3:0x60\n v_bitop3_b32 v104, v104, v106, v121 bitop3:0x60\n v_bitop3_b32 v108, v108, v110, v121 bitop3:0x60\n v_bitop3_b32 v112, v112, v114, v121 bitop3:0x60\n")
// ... and two instructions later with SGPR constants (today's block)
DEFK(k_b3_acc2_s, "v_bitop3_b32 v100, v100, v101, s20 bitop3:0x60\n v_bitop3_b32 v104, v104, v105, s20 bitop3:0x60\n v_bitop3_b32 v100, v100, v102, s21 bitop3:0x60\n v_bitop3_b32 v104, v104, v106, s21 bitop3:0x60\n"
                  "v_bitop3_b32 v108, v108, v109, s22 bitop3:0x60\n v_bitop3_b32 v112, v112, v113, s22 bitop3:0x60\n v_bitop3_b32 v108, v108, v110, s23 bitop3:0x60\n v_bitop3_b32 v112, v112, v114, s23 bitop3:0x60\n")
// two instructions later, VGPR constants (the dependency alone)
DEFK(k_b3_acc2_v, "v_bitop3_b32 v100, v100, v101, v120 bitop3:0x60\n v_bitop3_b32 v104, v104, v105, v120 bitop3:0x60\n v_bitop3_b32 v100, v100, v102, v121 bitop3:0x60\n v_bitop3_b32 v104, v104, v106, v121 bitop3:0x60\n"
                  "v_bitop3_b32 v108, v108, v109, v122 bitop3:0x60\n v_bitop3_b32 v112, v112, v113, v122 bitop3:0x60\n v_bitop3_b32 v108, v108, v110, v123 bitop3:0x60\n v_bitop3_b32 v112, v112, v114, v123 bitop3:0x60\n")
DEFK(k_mov_s, "v_mov_b32 v100, s20\n v_mov_b32 v104, s21\n v_mov_b32 v108, s22\n v_mov_b32 v112, s23\n"
              "v_mov_b32 v116, s24\n v_mov_b32 v120, s25\n v_mov_b32 v101, s26\n v_mov_b32 v105, s27\n")
DEFK(k_mov_v, "v_mov_b32 v100, v101\n v_mov_b32 v104, v105\n v_mov_b32 v108, v109\n v_mov_b32 v112, v113\n"
              "v_mov_b32 v116, v117\n v_mov_b32 v120, v121\n v_mov_b32 v101, v102\n v_mov_b32 v105, v106\n")
DEFK(k_vbfe_s, "v_bfe_i32 v100, s28, 0, 1\n v_bfe_i32 v104, s29, 1, 1\n v_bfe_i32 v108, s28, 2, 1\n v_bfe_i32 v112, s29, 3, 1\n"
               "v_bfe_i32 v116, s28, 4, 1\n v_bfe_i32 v120, s29, 5, 1\n v_bfe_i32 v101, s28, 6, 1\n v_bfe_i32 v105, s29, 7, 1\n")
// s_bfe_i32 and, at once, a vector reader of its result (eight pairs: 8 SALU + 8 VALU)
DEFK(k_sbfe_mov, "s_bfe_i32 s20, s28, 0x10000\n v_mov_b32 v100, s20\n s_bfe_i32 s21, s29, 0x10001\n v_mov_b32 v104, s21\n s_bfe_i32 s22, s28, 0x10002\n v_mov_b32 v108, s22\n s_bfe_i32 s23, s29, 0x10003\n v_mov_b32 v112, s23\n"
                 "s_bfe_i32 s24, s28, 0x10004\n v_mov_b32 v116, s24\n s_bfe_i32 s25, s29, 0x10005\n v_mov_b32 v120, s25\n s_bfe_i32 s26, s28, 0x10006\n v_mov_b32 v101, s26\n s_bfe_i32 s27, s29, 0x10007\n v_mov_b32 v105, s27\n")
// today's unit: s_bfe_i32, then the two dependent-paired bitop3 that read it (4 SALU + 8 VALU)
DEFK(k_sbfe_b3x2, "s_bfe_i32 s20, s28, 0x10000\n s_bfe_i32 s21, s29, 0x10000\n v_bitop3_b32 v100, v100, v101, s20 bitop3:0x60\n v_bitop3_b32 v104, v104, v105, s20 bitop3:0x60\n v_bitop3_b32 v100, v100, v102, s21 bitop3:0x60\n v_bitop3_b32 v104, v104, v106, s21 bitop3:0x60\n"
                  "s_bfe_i32 s22, s28, 0x10001\n s_bfe_i32 s23, s29, 0x10001\n v_bitop3_b32 v108, v108, v109, s22 bitop3:0x60\n v_bitop3_b32 v112, v112, v113, s22 bitop3:0x60\n v_bitop3_b32 v108, v108, v110, s23 bitop3:0x60\n v_bitop3_b32 v112, v112, v114, s23 bitop3:0x60\n")
// the pair unit: two v_bfe_i32 from the piece words, then eight bitop3 on VGPRs (10 VALU, counted as 8 + 2)
DEFK(k_vbfe_b3x8, "v_bfe_i32 v120, s28, 0, 1\n v_bfe_i32 v121, s29, 0, 1\n v_bitop3_b32 v100, v100, v101, v120 bitop3:0x60\n v_bitop3_b32 v104, v104, v105, v120 bitop3:0x60\n v_bitop3_b32 v108, v108, v109, v120 bitop3:0x60\n v_bitop3_b32 v112, v112, v113, v120 bitop3:0x60\n"
                  "v_bitop3_b32 v100, v100, v102, v121 bitop3:0x60\n v_bitop3_b32 v104, v104, v106, v121 bitop3:0x60\n v_bitop3_b32 v108, v108, v110, v121 bitop3:0x60\n v_bitop3_b32 v112, v112, v114, v121 bitop3:0x60\n")

template <typename K> void run(const char* name, K kern, unsigned* d, int waves_per_simd, double valu_per_unit) {
  const int iters = 2048, grid = 256 * waves_per_simd;  // blocks of 256 = 4 waves = 1 per SIMD
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, d, 8);
  hipEventRecord(a);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, d, iters);
  hipEventRecord(b); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b);
  const double units = (double)waves_per_simd * iters * 16.0;  // units of one SIMD
  const double ns = ms * 1e6 / units;
  printf("%-44s w/SIMD=%d %8.3f ms  %7.2f ns per unit and SIMD = %5.2f cyc @2.4GHz per VALU instr (%g per unit)\n", name, waves_per_simd, ms, ns,
         ns * 2.4 / valu_per_unit, valu_per_unit);
  hipEventDestroy(a); hipEventDestroy(b);
}

// ---- the kernel's block ----
template <int TT> __device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, TT); }
__device__ __forceinline__ uint4 stream_load16(const uint8_t* p) {
  typedef uint32_t u32x4_nt __attribute__((ext_vector_type(4)));
  const u32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

enum Form { kBlockSgpr = 0, kPairMov = 1, kPairVbfe = 2, kPairLds = 3 };
constexpr int kSlotsN = 8;
constexpr uint32_t kBodyLds = 45184;  // per workgroup, as the grouped launch: three workgroups per CU
constexpr uint32_t kStoreIters = 256; // the plane store every wave reads, over and over: 256 KiB, L2-resident

// What the hot block of filter_dna_kernel<Q, 2, true, false, false, 4, 2, kPlaneRead> does per iteration, nothing else: the
// lane's 16 plane bytes (asked for four iterations ahead), the piece test of eight slots, the OR of the masks and a rare
// branch.  FORM: today's block with scalar constants, or the block pair with the constants in vector registers -- moved
// there from s_bfe_i32's result, made by v_bfe_i32 from the scalar piece word, or read from an LDS table by broadcast.
template <int Q, int FORM, int W = 3>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(W, W))) void piece_body(const uint8_t* planes, const uint32_t* piece_bits, uint32_t* out, uint32_t n_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kAhead = 4;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t nb0[kSlotsN], nb1[kSlotsN];
#pragma unroll
  for (int pp = 0; pp < kSlotsN; ++pp) {
    nb0[pp] = __builtin_amdgcn_readfirstlane(~piece_bits[2 * pp]);
    nb1[pp] = __builtin_amdgcn_readfirstlane(~piece_bits[2 * pp + 1]);
  }
  if constexpr (FORM == kPairLds) {  // [row][slot]{n0, n1}: one ds_read_b128 = a row's constants of two slots
    uint32_t* tab = reinterpret_cast<uint32_t*>(smem);
    if (threadIdx.x < kSlotsN * Q) {
      const uint32_t pp = threadIdx.x % kSlotsN, j = threadIdx.x / kSlotsN;
      tab[(j * kSlotsN + pp) * 2] = (uint32_t)(-(int32_t)((~piece_bits[2 * pp] >> j) & 1u));
      tab[(j * kSlotsN + pp) * 2 + 1] = (uint32_t)(-(int32_t)((~piece_bits[2 * pp + 1] >> j) & 1u));
    }
    __syncthreads();
  }
  const uint8_t* base = planes + lane * 16u;
  uint4 pln[kAhead + 2];
#pragma unroll
  for (int j = 0; j < kAhead + 2; ++j) {
    pln[j] = make_uint4(0u, 0u, 0u, 0u);
    if (j >= 2 && (uint32_t)(j - 2) < n_iter) pln[j] = stream_load16(base + (uint64_t)((uint32_t)(j - 2) % kStoreIters) * 1024u);
  }
  uint32_t prev0 = 0, prev1 = 0, found = 0;
  for (uint32_t it = 0; it < n_iter; it += (FORM == kBlockSgpr ? 1u : 2u)) {
    if ((it & 1u) == 0) {
#pragma unroll
      for (int j = 0; j < kAhead; ++j) pln[j] = pln[j + 2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (it + (uint32_t)(kAhead + j) < n_iter) pln[kAhead + j] = stream_load16(base + (uint64_t)((it + (uint32_t)(kAhead + j)) % kStoreIters) * 1024u);
    }
    uint32_t b0[kSlotsN], b1[kSlotsN];
#pragma unroll
    for (int pp = 0; pp < kSlotsN; ++pp) {
      b0[pp] = nb0[pp];
      b1[pp] = nb1[pp];
      asm volatile("" : "+s"(b0[pp]), "+s"(b1[pp]));
    }
    if constexpr (FORM == kBlockSgpr) {
      const uint4 pv = (it & 1u) ? pln[1] : pln[0];
      const uint2 t0 = make_uint2(pv.x, pv.y), t1 = make_uint2(pv.z, pv.w);
      uint32_t al[kSlotsN], ah[kSlotsN];
#pragma unroll
      for (int pp = 0; pp < kSlotsN; ++pp) { al[pp] = 0xFFFFFFFFu; ah[pp] = 0xFFFFFFFFu; }
#pragma unroll
      for (int d = 0; d < Q; ++d) {
        uint32_t s0l, s0h, s1l, s1h;
        if (d == 0) {
          s0l = t0.x; s0h = t0.y; s1l = t1.x; s1h = t1.y;
        } else {
          s0l = __builtin_amdgcn_alignbit(t0.x, prev0, 32 - d);
          s0h = __builtin_amdgcn_alignbit(t0.y, t0.x, 32 - d);
          s1l = __builtin_amdgcn_alignbit(t1.x, prev1, 32 - d);
          s1h = __builtin_amdgcn_alignbit(t1.y, t1.x, 32 - d);
        }
#pragma unroll
        for (int pp = 0; pp < kSlotsN; ++pp) {
          const int j = Q - 1 - d;
          const uint32_t n0 = (uint32_t)__builtin_amdgcn_sbfe((int)b0[pp], j, 1);
          const uint32_t n1 = (uint32_t)__builtin_amdgcn_sbfe((int)b1[pp], j, 1);
          al[pp] = bitop3<0x60>(al[pp], s0l, n0);
          ah[pp] = bitop3<0x60>(ah[pp], s0h, n0);
          al[pp] = bitop3<0x60>(al[pp], s1l, n1);
          ah[pp] = bitop3<0x60>(ah[pp], s1h, n1);
        }
      }
      prev0 = t0.y;
      prev1 = t1.y;
      uint32_t hit = 0;
#pragma unroll
      for (int pp = 0; pp < kSlotsN; ++pp) hit |= al[pp] | ah[pp];
      if (hit != 0) found += __popc(hit) + it;
    } else {
      const uint2 a0 = make_uint2(pln[0].x, pln[0].y), a1 = make_uint2(pln[0].z, pln[0].w);
      const uint2 c0 = make_uint2(pln[1].x, pln[1].y), c1 = make_uint2(pln[1].z, pln[1].w);
      uint32_t al[kSlotsN], ah[kSlotsN], bl[kSlotsN], bh[kSlotsN];
#pragma unroll
      for (int pp = 0; pp < kSlotsN; ++pp) { al[pp] = ah[pp] = bl[pp] = bh[pp] = 0xFFFFFFFFu; }
#pragma unroll
      for (int d = 0; d < Q; ++d) {
        uint32_t s[8];
        if (d == 0) {
          s[0] = a0.x; s[1] = a0.y; s[2] = c0.x; s[3] = c0.y; s[4] = a1.x; s[5] = a1.y; s[6] = c1.x; s[7] = c1.y;
        } else {
          s[0] = __builtin_amdgcn_alignbit(a0.x, prev0, 32 - d);
          s[1] = __builtin_amdgcn_alignbit(a0.y, a0.x, 32 - d);
          s[2] = __builtin_amdgcn_alignbit(c0.x, a0.y, 32 - d);
          s[3] = __builtin_amdgcn_alignbit(c0.y, c0.x, 32 - d);
          s[4] = __builtin_amdgcn_alignbit(a1.x, prev1, 32 - d);
          s[5] = __builtin_amdgcn_alignbit(a1.y, a1.x, 32 - d);
          s[6] = __builtin_amdgcn_alignbit(c1.x, a1.y, 32 - d);
          s[7] = __builtin_amdgcn_alignbit(c1.y, c1.x, 32 - d);
        }
        const int j = Q - 1 - d;
        uint4 two = make_uint4(0u, 0u, 0u, 0u);
        uint32_t tab_off = 0;  // (opaque: the table is read in the loop, not held in registers across it)
        if constexpr (FORM == kPairLds) asm volatile("" : "+v"(tab_off));
#pragma unroll
        for (int pp = 0; pp < kSlotsN; ++pp) {
          uint32_t n0, n1;
          if constexpr (FORM == kPairMov) {
            const uint32_t n0s = (uint32_t)__builtin_amdgcn_sbfe((int)b0[pp], j, 1);
            const uint32_t n1s = (uint32_t)__builtin_amdgcn_sbfe((int)b1[pp], j, 1);
            asm("v_mov_b32 %0, %1" : "=v"(n0) : "s"(n0s));
            asm("v_mov_b32 %0, %1" : "=v"(n1) : "s"(n1s));
          } else if constexpr (FORM == kPairVbfe) {
            asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(n0) : "s"(b0[pp]), "n"(j));
            asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(n1) : "s"(b1[pp]), "n"(j));
          } else {
            // slots pp and pp + 1 arrive together
            if ((pp & 1) == 0) two = *reinterpret_cast<const uint4*>(smem + tab_off + ((j * kSlotsN + pp) * 8));
            n0 = (pp & 1) ? two.z : two.x;
            n1 = (pp & 1) ? two.w : two.y;
          }
          al[pp] = bitop3<0x60>(al[pp], s[0], n0);
          ah[pp] = bitop3<0x60>(ah[pp], s[1], n0);
          bl[pp] = bitop3<0x60>(bl[pp], s[2], n0);
          bh[pp] = bitop3<0x60>(bh[pp], s[3], n0);
          al[pp] = bitop3<0x60>(al[pp], s[4], n1);
          ah[pp] = bitop3<0x60>(ah[pp], s[5], n1);
          bl[pp] = bitop3<0x60>(bl[pp], s[6], n1);
          bh[pp] = bitop3<0x60>(bh[pp], s[7], n1);
        }
      }
      prev0 = c0.y;
      prev1 = c1.y;
      uint32_t hit = 0;
#pragma unroll
      for (int pp = 0; pp < kSlotsN; ++pp) hit |= al[pp] | ah[pp];
      if (hit != 0) found += __popc(hit) + it;
      hit = 0;
#pragma unroll
      for (int pp = 0; pp < kSlotsN; ++pp) hit |= bl[pp] | bh[pp];
      if (hit != 0) found += __popc(hit) + it + 1u;
    }
  }
  out[blockIdx.x * 256u + threadIdx.x] = found;
}

template <int Q, int FORM> float run_body(const char* name, const uint8_t* planes, const uint32_t* pieces, uint32_t* out, std::vector<uint32_t>* sums) {
  // the half launch of the bench: 509 workgroups, 182 iterations (370 552 wave-iterations); timed: ten in a row
  const uint32_t grid = 509, n_iter = 182;
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  hipLaunchKernelGGL((piece_body<Q, FORM>), dim3(grid), dim3(256), kBodyLds, 0, planes, pieces, out, n_iter);
  hipEventRecord(a);
  for (int r = 0; r < 10; ++r) hipLaunchKernelGGL((piece_body<Q, FORM>), dim3(grid), dim3(256), kBodyLds, 0, planes, pieces, out, n_iter);
  hipEventRecord(b); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b);
  ms /= 10.f;
  std::vector<uint32_t> h(grid * 256u);
  hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost);
  uint32_t sum = 0;
  for (uint32_t v : h) sum += v;
  sums->push_back(sum);
  const double per = ms * 1e6 / ((double)grid * 4 * n_iter / 1024.0);  // ns per block of one SIMD's waves
  printf("body Q=%-2d %-34s %7.4f ms per launch  %7.1f ns per wave-block and SIMD (%6.0f cyc @2.4GHz)  checksum %08x\n", Q, name, ms, per, per * 2.4, sum);
  hipEventDestroy(a); hipEventDestroy(b);
  return ms;
}

template <int Q> void bodies(const uint8_t* planes, const uint32_t* pieces, uint32_t* out) {
  std::vector<uint32_t> sums;
  const float t_a = run_body<Q, kBlockSgpr>("(a) block, scalar constants", planes, pieces, out, &sums);
  const float t_m = run_body<Q, kPairMov>("(b) pair, s_bfe + v_mov", planes, pieces, out, &sums);
  const float t_v = run_body<Q, kPairVbfe>("(b) pair, v_bfe_i32 from the SGPR", planes, pieces, out, &sums);
  const float t_l = run_body<Q, kPairLds>("(b) pair, LDS table ds_read_b128", planes, pieces, out, &sums);
  const float t_a2 = run_body<Q, kBlockSgpr>("(a) again", planes, pieces, out, &sums);
  bool same = true;
  for (uint32_t s : sums) same = same && s == sums[0];
  printf("body Q=%-2d per block against (a): mov %.3f  v_bfe %.3f  lds %.3f  ((a) again %.3f)  checksums %s\n\n", Q, t_m / t_a, t_v / t_a, t_l / t_a,
         t_a2 / t_a, same ? "equal" : "DIFFER");
}

// ---- section 3: the LDS-table body at three and at four waves per SIMD ----
// W = 3: 45 184 B + the table (three workgroups per CU); W = 4: 40 064 B + the table (four).  `streams` launches of 509
// workgroups side by side, ten in a row on each stream; returns ms per launch.
template <int Q, int W> float run_occ(int streams, const uint8_t* planes, const uint32_t* pieces, uint32_t* out, hipStream_t* st, uint32_t* checksum) {
  const uint32_t grid = 509, n_iter = 182, lds = (W == 4 ? 40064u : kBodyLds) + (uint32_t)Q * 64u;
  hipEvent_t a, b, j; hipEventCreate(&a); hipEventCreate(&b); hipEventCreate(&j);
  for (int s = 0; s < streams; ++s) hipLaunchKernelGGL((piece_body<Q, kPairLds, W>), dim3(grid), dim3(256), lds, st[s], planes, pieces, out + s * grid * 256u, n_iter);
  hipDeviceSynchronize();
  hipEventRecord(a, st[0]);
  if (streams == 2) hipStreamWaitEvent(st[1], a, 0);
  for (int r = 0; r < 10; ++r)
    for (int s = 0; s < streams; ++s) hipLaunchKernelGGL((piece_body<Q, kPairLds, W>), dim3(grid), dim3(256), lds, st[s], planes, pieces, out + s * grid * 256u, n_iter);
  if (streams == 2) { hipEventRecord(j, st[1]); hipStreamWaitEvent(st[0], j, 0); }
  hipEventRecord(b, st[0]); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b);
  ms /= 10.f * (float)streams;
  std::vector<uint32_t> h(grid * 256u);
  hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost);
  uint32_t sum = 0;
  for (uint32_t v : h) sum += v;
  *checksum = sum;
  const double per = ms * 1e6 / ((double)grid * 4 * n_iter / 1024.0);
  printf("occ  Q=%-2d %d waves/SIMD %6u B LDS  %s  %7.4f ms per launch  %7.1f ns per wave-block and SIMD (%6.0f cyc @2.4GHz)  checksum %08x\n", Q, W, lds,
         streams == 2 ? "two side by side" : "alone           ", ms, per, per * 2.4, sum);
  hipEventDestroy(a); hipEventDestroy(b); hipEventDestroy(j);
  return ms;
}
template <int Q> bool occupancy_rows(const uint8_t* planes, const uint32_t* pieces, uint32_t* out, hipStream_t* st) {
  bool gate = true, same = true;
  uint32_t first = 0, sum = 0;
  for (int streams = 1; streams <= 2; ++streams) {
    float worst4 = 0.f, best3 = 1e9f;
    for (int rep = 0; rep < 3; ++rep) {  // the rows alternate: a drift of the box hits both
      const float t3 = run_occ<Q, 3>(streams, planes, pieces, out, st, &sum);
      if (streams == 1 && rep == 0) first = sum;
      same = same && sum == first;
      const float t4 = run_occ<Q, 4>(streams, planes, pieces, out, st, &sum);
      same = same && sum == first;
      best3 = t3 < best3 ? t3 : best3;
      worst4 = t4 > worst4 ? t4 : worst4;
    }
    printf("occ  Q=%-2d %s: slowest four-wave run %.4f ms, fastest three-wave run %.4f ms: %.3f\n", Q, streams == 2 ? "two side by side" : "alone", worst4, best3,
           worst4 / best3);
    gate = gate && worst4 < best3;
  }
  printf("occ  Q=%-2d gate (every four-wave run faster than every three-wave run) %s; checksums %s\n\n", Q, gate ? "passed" : "FAILED", same ? "equal" : "DIFFER");
  return gate && same;
}

int main() {
  unsigned* d; hipMalloc(&d, 256 * 8 * 256 * 4);
  for (int w : {1, 2, 3, 4}) {
    run("v_bitop3 0x60 (3 VGPR)", k_b3_vvv, d, w, 8);
    run("v_bitop3 0x60 (2 VGPR + SGPR)", k_b3_vvs, d, w, 8);
    run("v_bitop3 chains, reread after 4, VGPR const", k_b3_acc4_v, d, w, 8);
    run("v_bitop3 chains, reread after 2, VGPR const", k_b3_acc2_v, d, w, 8);
    run("v_bitop3 chains, reread after 2, SGPR const", k_b3_acc2_s, d, w, 8);
    run("v_mov_b32 from an SGPR", k_mov_s, d, w, 8);
    run("v_mov_b32 from a VGPR", k_mov_v, d, w, 8);
    run("v_bfe_i32 from an SGPR", k_vbfe_s, d, w, 8);
    run("s_bfe_i32 -> v_mov_b32 at once (8 + 8)", k_sbfe_mov, d, w, 8);
    run("2 s_bfe_i32 -> 4 bitop3 SGPR (today, x2)", k_sbfe_b3x2, d, w, 8);
    run("2 v_bfe_i32 -> 8 bitop3 VGPR (pair)", k_vbfe_b3x8, d, w, 10);
    printf("\n");
  }
  // random planes and pieces: chance occurrences take the rare branch as in the kernel (Q = 8: 0.8 % of the blocks)
  std::vector<uint32_t> hp(kStoreIters * 64u * 4u), pc(16);
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 16); };
  for (auto& v : hp) v = rnd();
  for (auto& v : pc) v = rnd() & 0xFFFu;
  uint8_t* planes; uint32_t* pieces; uint32_t* out;
  hipMalloc(&planes, hp.size() * 4); hipMalloc(&pieces, 64); hipMalloc(&out, 509 * 256 * 4);
  hipMemcpy(planes, hp.data(), hp.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(pieces, pc.data(), 64, hipMemcpyHostToDevice);
  bodies<8>(planes, pieces, out);
  bodies<7>(planes, pieces, out);
  bodies<12>(planes, pieces, out);
  uint32_t* out2; hipMalloc(&out2, 2 * 509 * 256 * 4);
  hipStream_t st[2]; hipStreamCreate(&st[0]); hipStreamCreate(&st[1]);
  bool gate = occupancy_rows<7>(planes, pieces, out2, st);
  gate = occupancy_rows<8>(planes, pieces, out2, st) && gate;
  gate = occupancy_rows<12>(planes, pieces, out2, st) && gate;
  printf("occ  gate over Q = 7, 8, 12: %s\n", gate ? "passed" : "FAILED");
  return 0;
}
