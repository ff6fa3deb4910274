// reads_relayout.hip -- a resident read batch (fastq_reads.hip) into the two batch layouts the one-pass paths of search_many
// scan (many_patterns.hip: search_many_batched's separator layout, search_many_pertext's whole blocks per read), on the
// device: what layout_and_upload does for host texts, without the host layout and the upload.  The arithmetic is in
// relayout_step.h.  Geometry as fastq_copy_kernel: a lane per 64-byte block of the DESTINATION, its first read by binary
// search in the destination's start table, 16-byte loads from the (in general unaligned) source, 16-byte stores; the
// destination's last piece, where it is shorter than 16 bytes, byte by byte.  Bytes behind `total` are not written, as
// layout_and_upload leaves them.  Also here: acgt_only over the handle's sequences, and the handle as a text source.
#include "host_internal.h"
#include "relayout_step.h"

namespace sassy_hip {

namespace {

// src: the handle's text; src_start / src_len: its tables from read `first` on; dst_start: `count` starts (device).
__global__ __launch_bounds__(256) void reads_relayout_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_start,
                                                             const uint64_t* __restrict__ src_len, const uint64_t* __restrict__ dst_start,
                                                             uint32_t count, uint64_t total, uint64_t n_blocks, uint32_t pad,
                                                             uint8_t* __restrict__ dst) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  uint32_t out[16];
  rl_block(
      [&](int64_t a, uint32_t* w4) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + a);
        w4[0] = v.x; w4[1] = v.y; w4[2] = v.z; w4[3] = v.w;
      },
      [&](uint32_t i) { return dst_start[i]; }, [&](uint32_t i) { return src_len[i]; }, [&](uint32_t i) { return src_start[i]; }, count, b,
      (uint8_t)pad, out);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t p = b * 64 + 16u * j;
    const uint32_t have = rl_piece_bytes(p, total);
    if (have == 16u) {
      *reinterpret_cast<uint4*>(dst + p) = make_uint4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
    } else {
      for (uint32_t q = 0; q < have; ++q) dst[p + q] = (uint8_t)(out[4 * j + (q >> 2)] >> (8u * (q & 3u)));
    }
  }
}

// A lane per 64-byte block of the handle's text: the block's bytes that belong to its read (rem[]) must be A, C, G, T in
// either case.  The zeros between the reads do not count; a zero inside a read does.
__global__ __launch_bounds__(256) void reads_plain_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ rem, uint64_t n_blocks,
                                                          uint32_t* __restrict__ flag) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const uint32_t keep = min(rem[b], 64u);
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (keep <= 16u * j) break;
    const uint4 v = *reinterpret_cast<const uint4*>(text + b * 64 + 16u * j);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t at = 16u * j + 4u * d;
      bad = bad || rl_other_letter(w[d], keep > at ? keep - at : 0u);
    }
  }
  if (bad) *flag = 1u;
}

constexpr uint64_t kMaxGridBlocks = 0x7FFFFFFFull * 256ull;  // 64-byte blocks one launch of 256 lanes per workgroup takes

}  // namespace

int reads_relayout(const sassy_hip_Reads* reads, uint64_t first, uint64_t count, const uint64_t* d_dst_start, uint64_t total, uint8_t pad,
                   uint8_t* d_dst, hipStream_t stream) {
  const uint64_t n_blocks = (total + 63) / 64;
  if (n_blocks == 0) return 0;
  if (n_blocks > kMaxGridBlocks || count > 0xFFFFFFFFull) return fail(SASSY_HIP_EUNSUPPORTED, "reads_relayout: the layout is too long for a grid");
  hipLaunchKernelGGL(reads_relayout_kernel, dim3((uint32_t)((n_blocks + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)reads->d_text,
                     (const uint64_t*)reads->d_table + first, (const uint64_t*)reads->d_table + reads->n_records + first, d_dst_start,
                     (uint32_t)count, total, n_blocks, (uint32_t)pad, d_dst);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return hip_fail(le, "reads relayout launch");
  return 0;
}

int reads_plain(sassy_SearcherType* s, TextSource& src, bool* plain) {
  *plain = false;
  if (src.plain < 0) {
    const sassy_hip_Reads* r = src.reads;
    const uint64_t n_blocks = (r->text_bytes - 64) / 64;
    uint32_t bad = 0;
    if (n_blocks) {
      if (n_blocks > kMaxGridBlocks) return fail(SASSY_HIP_EUNSUPPORTED, "reads: the text is too long for a grid");
      if (int rc = s->d_ncount.reserve(4)) return rc;
      HIP_TRY(hipMemsetAsync(s->d_ncount.p, 0, 4, s->stream));
      hipLaunchKernelGGL(reads_plain_kernel, dim3((uint32_t)((n_blocks + 255) / 256)), dim3(256), 0, s->stream, (const uint8_t*)r->d_text,
                         (const uint32_t*)r->d_rem, n_blocks, s->d_ncount.p);
      const hipError_t le = hipGetLastError();
      if (le != hipSuccess) return hip_fail(le, "reads letter check launch");
      bad = 1;
      HIP_TRY(hipMemcpyAsync(&bad, s->d_ncount.p, 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    src.plain = bad ? 0 : 1;
  }
  *plain = src.plain == 1;
  return 0;
}

int reads_as_source(sassy_SearcherType* s, const sassy_hip_Reads* reads, uint32_t flags, const char* who, ReadsTexts* out) {
  if (!s || !reads) return fail(SASSY_HIP_EINVAL, std::string("Pointers in ") + who + "() must not be null");
  if (flags & SASSY_HIP_TEXT_ON_DEVICE)
    return fail(SASSY_HIP_EINVAL, std::string(who) + ": SASSY_HIP_TEXT_ON_DEVICE has no meaning for a read batch, which is on the device");
  SASSY_NO_TICKETS(s);
  {
    DeviceGuard on_device(s);  // (first use binds the searcher to the thread's device)
    if (s->device != reads->device)
      return fail(SASSY_HIP_EINVAL, std::string(who) + ": the reads were made on device " + std::to_string(reads->device) +
                                        ", the searcher is on device " + std::to_string(s->device));
  }
  const size_t n = (size_t)reads->n_records;
  out->ptr.resize(n);
  out->len.resize(n);
  for (size_t r = 0; r < n; ++r) {
    out->ptr[r] = reads->d_text + reads->records[r].seq_start;
    out->len[r] = (size_t)reads->records[r].seq_len;
  }
  out->src = TextSource{out->ptr.data(), out->len.data(), n, reads, -1};
  return 0;
}

}  // namespace sassy_hip

using namespace sassy_hip;

extern "C" {

int sassy_hip_reads_relayout(const sassy_hip_Reads* reads, uint64_t first, uint64_t count, const uint64_t* dst_starts, uint64_t total,
                             uint8_t pad, void* d_dst, void* hip_stream) {
  if (!reads || !d_dst || (count && !dst_starts)) return fail(SASSY_HIP_EINVAL, "reads_relayout: null argument");
  if (first > reads->n_records || count > reads->n_records - first)
    return fail(SASSY_HIP_EINVAL, "reads_relayout: reads " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(count) +
                                      " lie outside the handle's " + std::to_string(reads->n_records));
  if (((uintptr_t)d_dst & 15) != 0) return fail(SASSY_HIP_EINVAL, "reads_relayout: the destination must be 16-byte aligned");
  // the destination's table: ascending, no read over the next one's start or over the end
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t len = reads->records[first + i].seq_len, next = i + 1 < count ? dst_starts[i + 1] : total;
    if (dst_starts[i] > next || len > next - dst_starts[i])
      return fail(SASSY_HIP_EINVAL, "reads_relayout: read " + std::to_string(first + i) + " does not fit between its start and the next one");
  }
  if (total == 0) return 0;
  int prev = -1;
  HIP_TRY(hipGetDevice(&prev));
  if (prev != reads->device) HIP_TRY(hipSetDevice(reads->device));
  struct Back {
    int prev, cur;
    ~Back() { if (prev != cur) (void)hipSetDevice(prev); }
  } back{prev, reads->device};
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  uint64_t* d_tab = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d_tab), std::max<uint64_t>(count, 1) * 8) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SASSY_HIP_ENOMEM, "reads_relayout: out of device memory (" + std::to_string(count * 8) + " bytes of starts)");
  }
  int rc = 0;
  hipError_t e = count ? hipMemcpyAsync(d_tab, dst_starts, count * 8, hipMemcpyHostToDevice, st) : hipSuccess;
  if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (relayout starts)");
  if (!rc) rc = reads_relayout(reads, first, count, d_tab, total, pad, static_cast<uint8_t*>(d_dst), st);
  e = hipStreamSynchronize(st);  // (the table goes; the caller finds the buffer written)
  if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize (relayout)");
  (void)hipFree(d_tab);
  return rc;
}

}  // extern "C"
