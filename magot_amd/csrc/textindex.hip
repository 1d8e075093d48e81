// The byte index of a resident text (textindex.h): the first step of
// besthits_from_psl, heterozygosity_from_vcf, exclude_from_fasta / fasta2tab
// and replace_names.
//
//   count_kernel    per text block of kTextBlock bytes, one 16-byte load per
//                   lane: the occurrences of the indexed byte and, where asked,
//                   of a second byte.  Block n_blocks is a sentinel that counts
//                   nothing, so one rocprim exclusive scan per byte gives each
//                   block the occurrences before it, and the total.
//   fill_kernel     from the same load, a lane owns the occurrences in its 16
//                   bytes: a wave scan and the wave totals number them, and
//                   occurrence j at byte p gives pos[j] = p (plain mode) or
//                   pos[j + 1] = p + 1 (line mode: the start of the line behind an
//                   LF).  Line mode with the stray-CR check also looks at the
//                   load's CRs; a CR in a lane's last byte reads the one byte
//                   after it.
// The bytes between the text's end and the next multiple of 16 are loaded and
// masked out: they are anything.
//
// LDS: the wave totals.  No spin-wait, no compare-and-swap; nothing is float.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kIxThreads = 256;
constexpr int kIxLane = 16;
constexpr int kIxWaves = kIxThreads / 64;
static_assert(kTextBlock == kIxThreads * kIxLane, "one 16-byte load per lane");

// bit j of *m, and with kTwo of *m2: byte i + j of the text is `byte`, is `byte2`
// (i the lane's first byte).  A lane behind the text loads nothing; the load and
// the mask arithmetic stay inside that branch.
template <bool kTwo>
__device__ __forceinline__ void text_lane_masks(const uint8_t* __restrict__ text, uint64_t i,
                                                uint64_t n, uint32_t byte, uint32_t byte2,
                                                uint32_t* m, uint32_t* m2) {
  *m = *m2 = 0;
  if (i >= n) return;
  const uint4 v = *reinterpret_cast<const uint4*>(text + i);  // readable to the next 16
  const uint32_t keep = n - i < kIxLane ? (1u << (n - i)) - 1 : 0xffffu;  // behind the text: anything
  *m = byte_eq_mask16(v, byte * 0x01010101u) & keep;
  if constexpr (kTwo) *m2 = byte_eq_mask16(v, byte2 * 0x01010101u) & keep;
}

template <bool kSecond>
__global__ __launch_bounds__(kIxThreads) void text_count_kernel(TextIndexArgs a) {
  __shared__ uint32_t wave_count[kSecond ? 2 : 1][kIxWaves];
  const int t = threadIdx.x;
  uint32_t c = 0, c2 = 0;
  if (blockIdx.x < a.n_blocks) {  // block n_blocks is the sentinel: its prefix is the total
    uint32_t m, m2;
    text_lane_masks<kSecond>(a.text, (uint64_t)blockIdx.x * kTextBlock + kIxLane * t, a.n, a.byte,
                             a.byte2, &m, &m2);
    c = __popc(m);
    c2 = __popc(m2);
  }
  for (int d = 32; d; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    if constexpr (kSecond) c2 += __shfl_xor(c2, d, 64);
  }
  if ((t & 63) == 0) {
    wave_count[0][t >> 6] = c;
    if constexpr (kSecond) wave_count[1][t >> 6] = c2;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0, sum2 = 0;
    for (int w = 0; w < kIxWaves; ++w) {
      sum += wave_count[0][w];
      if constexpr (kSecond) sum2 += wave_count[1][w];
    }
    a.blk[blockIdx.x] = sum;
    if constexpr (kSecond) a.blk2[blockIdx.x] = sum2;
  }
}

template <TextFill kMode>
__global__ __launch_bounds__(kIxThreads) void text_fill_kernel(TextIndexArgs a) {
  constexpr bool kLines = kMode != kTextFillPlain;
  __shared__ uint32_t wave_count[kIxWaves];
  const int t = threadIdx.x;
  const uint32_t lane = t & 63, wave = t >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * kTextBlock + kIxLane * t;
  uint32_t hit, cr;  // cr stays 0 without the stray-CR check
  text_lane_masks<kMode == kTextFillLinesCr>(a.text, p0, a.n, a.byte, '\r', &hit, &cr);
  const uint32_t c = __popc(hit);
  const uint32_t inc = wave_scan(c);
  if (lane == 63) wave_count[wave] = inc;
  __syncthreads();
  if (hit | cr) {  // p0 < n
    // the occurrences before this lane's bytes: below the text's, which are at most n_lines
    uint64_t j = a.pre[blockIdx.x] + (inc - c);
    for (uint32_t w = 0; w < wave; ++w) j += wave_count[w];
    if (cr) {
      uint32_t ok = hit >> 1;                                  // the next byte is LF
      if (a.n - p0 <= kIxLane) ok |= 1u << (a.n - 1 - p0);     // the text's last byte
      else if ((cr >> 15) && a.text[p0 + kIxLane] == '\n') ok |= 1u << 15;  // p0 + 16 < n
      const uint32_t stray = cr & ~ok;
      if (stray) {  // the lane's first one is on its lowest line
        const uint64_t line = j + __popc(hit & ((1u << (__ffs(stray) - 1)) - 1));
        atomicMin(a.stray_status, (unsigned long long)(line << 8 | a.stray_reason));
      }
    }
    // __ffs counts from 1: the byte behind the occurrence
    for (uint32_t m = hit; m; m &= m - 1, ++j)
      a.pos[kLines ? j + 1 : j] = p0 + __ffs(m) - (kLines ? 0 : 1);
  }
  if (kLines && blockIdx.x == 0 && t == 0) {
    a.pos[0] = 0;
    a.pos[a.n_lines] = a.n;  // a last line without LF ends with the text
  }
}

template <class T>
hipError_t sum_scan(void* tmp, size_t& tmp_bytes, const T* in, T* out, uint64_t n, hipStream_t s) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), s);
}

}  // namespace

hipError_t exclusive_sum(void* tmp, size_t& tmp_bytes, const uint64_t* in, uint64_t* out,
                         uint64_t n, hipStream_t s) {
  return sum_scan(tmp, tmp_bytes, in, out, n, s);
}

hipError_t exclusive_sum(void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out,
                         uint64_t n, hipStream_t s) {
  return sum_scan(tmp, tmp_bytes, in, out, n, s);
}

hipError_t launch_text_count(const TextIndexArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  const unsigned grid = (unsigned)a.n_blocks + 1;
  const bool second = a.byte2 != kTextNoByte;
  if (second) text_count_kernel<true><<<grid, kIxThreads, 0, s>>>(a);
  else text_count_kernel<false><<<grid, kIxThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  if (second)
    if (hipError_t e = exclusive_sum(tmp, tmp_bytes, a.blk2, a.pre2, a.n_blocks + 1, s)) return e;
  return exclusive_sum(tmp, tmp_bytes, a.blk, a.pre, a.n_blocks + 1, s);
}

hipError_t launch_text_fill(const TextIndexArgs& a, TextFill mode, hipStream_t s) {
  if (!a.n_blocks) return hipSuccess;
  const unsigned grid = (unsigned)a.n_blocks;
  switch (mode) {
    case kTextFillPlain: text_fill_kernel<kTextFillPlain><<<grid, kIxThreads, 0, s>>>(a); break;
    case kTextFillLines: text_fill_kernel<kTextFillLines><<<grid, kIxThreads, 0, s>>>(a); break;
    default: text_fill_kernel<kTextFillLinesCr><<<grid, kIxThreads, 0, s>>>(a);
  }
  return hipGetLastError();
}

}  // namespace magot
