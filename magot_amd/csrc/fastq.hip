// fqstats on the device (genome_tools.py:85-124): the lengths of a FASTQ's
// sequence lines -- line k (from 0) with k % 4 == 1, whatever it holds -- as a
// histogram, and the tool's nine figures from it.
//
// The length of a line is the distance between two LFs, so no kernel looks at
// anything but LFs and a line of 3 MB costs what one of 100 bytes costs.
//
// Per chunk of text (cut anywhere, a line may span any number of chunks):
//   block_kernel    per text block of kTextBlock bytes, one 16-byte load per
//                   lane: the LFs, and the file offset of the last one (-1:
//                   none).  One rocprim exclusive scan under (sum, max) gives
//                   each block the LFs before it in the chunk and the last LF
//                   before it; the carry holds the same over the chunks before.
//   length_kernel   a lane owns the LFs of its 16 bytes.  Line index = carry +
//                   block prefix + the lanes' prefix + the LFs below in the
//                   lane; for an index = 1 (mod 4) the length is the LF's offset
//                   minus the offset of the LF before it minus 1, that LF being
//                   the lane's own, or the running max over the lanes before,
//                   the blocks before and the carry.  A workgroup walks many
//                   text blocks and counts lengths below kFqLocal in LDS, one
//                   global atomic per non-empty bin per workgroup at the end; a
//                   longer line ends at most once per kFqLocal bytes of text and
//                   goes to its global bin, or at kFqDense and above to the list.
// After the last chunk:
//   tail_kernel     a last line without LF, from the final carry.
//   the list sorted descending (rocprim), then one inclusive scan of (count,
//   count * length) over the list followed by the bins from the top down, and
//   find_kernel: the item at which a running total first passes each of the six
//   marks.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kFqThreads = 256;
constexpr int kLaneBytes = 16;
constexpr int kFqWaves = kFqThreads / 64;
constexpr uint32_t kFqLocal = 4096;  // bins a workgroup counts in LDS
static_assert(kTextBlock == kFqThreads * kLaneBytes, "one 16-byte load per lane");
static_assert(kFqLocal % kFqThreads == 0 && kFqLocal <= kFqDense, "the flush's stride");

// bit j: byte i + j of the chunk is LF (i the lane's first byte)
__device__ __forceinline__ uint32_t lane_lfs(const uint8_t* __restrict__ text, int64_t i,
                                             int64_t n) {
  if (i >= n) return 0;
  if (i + kLaneBytes <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + i);
    return byte_eq_mask16(v, 0x0A0A0A0Au);
  }
  uint32_t m = 0;
  for (int j = 0; j < kLaneBytes && i + j < n; ++j)
    if (text[i + j] == '\n') m |= 1u << j;
  return m;
}

struct FqBlockOp {
  __host__ __device__ FqBlock operator()(const FqBlock& a, const FqBlock& b) const {
    FqBlock r;
    r.lines = a.lines + b.lines;
    r.last_lf = a.last_lf > b.last_lf ? a.last_lf : b.last_lf;
    return r;
  }
};

__global__ __launch_bounds__(kFqThreads) void block_kernel(const uint8_t* __restrict__ text,
                                                           int64_t n, int64_t file_off,
                                                           uint32_t n_blocks,
                                                           FqBlock* __restrict__ blk) {
  __shared__ uint32_t wave_count[kFqWaves];
  __shared__ int64_t wave_last[kFqWaves];
  const int t = threadIdx.x;
  uint32_t c = 0;
  int64_t last = -1;
  if (blockIdx.x < n_blocks) {  // block n_blocks is the sentinel: its prefix is the total
    const int64_t i = (int64_t)blockIdx.x * kTextBlock + kLaneBytes * t;
    const uint32_t lf = lane_lfs(text, i, n);
    c = __popc(lf);
    if (lf) last = file_off + i + (31 - __clz(lf));
  }
  for (int d = 32; d; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    const int64_t o = __shfl_xor(last, d, 64);
    last = o > last ? o : last;
  }
  if ((t & 63) == 0) {
    wave_count[t >> 6] = c;
    wave_last[t >> 6] = last;
  }
  __syncthreads();
  if (t == 0) {
    FqBlock b;
    b.lines = 0;
    b.last_lf = -1;
    for (int w = 0; w < kFqWaves; ++w) {
      b.lines += wave_count[w];
      b.last_lf = wave_last[w] > b.last_lf ? wave_last[w] : b.last_lf;
    }
    blk[blockIdx.x] = b;
  }
}

__device__ __forceinline__ void fq_record(const FqChunkArgs& a, uint32_t* local, int64_t len) {
  if (len < (int64_t)kFqLocal) {
    atomicAdd(&local[len], 1u);
  } else if (len < (int64_t)kFqDense) {
    atomicAdd(&a.hist[len], 1ull);
  } else {
    const unsigned long long slot = atomicAdd(a.n_longs, 1ull);
    if (slot < a.longs_cap) a.longs[slot] = len;
  }
}

__global__ __launch_bounds__(kFqThreads) void length_kernel(FqChunkArgs a, uint32_t n_blocks) {
  __shared__ uint32_t local[kFqLocal];
  __shared__ uint32_t wave_count[kFqWaves];
  __shared__ int64_t wave_last[kFqWaves];
  const int t = threadIdx.x;
  const uint32_t lane = t & 63, wave = t >> 6;
  for (uint32_t q = t; q < kFqLocal; q += kFqThreads) local[q] = 0;
  const FqCarry in = *a.in;
  __syncthreads();
  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t p0 = (int64_t)b * kTextBlock + kLaneBytes * t;
    const uint32_t lf = lane_lfs(a.text, p0, a.n);
    const uint32_t c = __popc(lf);
    // inclusive prefixes over the wave: the LFs, and the last LF's offset
    uint32_t inc = c;
    int64_t far = lf ? a.file_off + p0 + (31 - __clz(lf)) : -1;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(inc, d, 64);
      const int64_t upf = __shfl_up(far, d, 64);
      if ((int)lane >= d) {
        inc += up;
        far = upf > far ? upf : far;
      }
    }
    if (lane == 63) {
      wave_count[wave] = inc;
      wave_last[wave] = far;
    }
    int64_t prev = __shfl_up(far, 1, 64);  // the last LF of the lanes before
    if (lane == 0) prev = -1;
    __syncthreads();
    if (lf) {
      const FqBlock pre = a.pre[b];
      uint64_t line = in.lines + pre.lines + (inc - c);
      prev = prev > pre.last_lf ? prev : pre.last_lf;
      prev = prev > in.last_lf ? prev : in.last_lf;
      for (uint32_t w = 0; w < wave; ++w) {
        line += wave_count[w];
        prev = wave_last[w] > prev ? wave_last[w] : prev;
      }
      for (uint32_t m = lf; m; m &= m - 1, ++line) {
        const int64_t at = a.file_off + p0 + (__ffs(m) - 1);
        if ((line & 3) == 1) fq_record(a, local, at - prev - 1);
        prev = at;
      }
    }
    __syncthreads();  // the wave totals are written again in the next round
  }
  for (uint32_t q = t; q < kFqLocal; q += kFqThreads) {
    const uint32_t k = local[q];
    if (k) atomicAdd(&a.hist[q], (unsigned long long)k);
  }
  if (blockIdx.x == 0 && t == 0) {
    const FqBlock total = a.pre[n_blocks];
    FqCarry out;
    out.lines = in.lines + total.lines;
    out.last_lf = total.last_lf > in.last_lf ? total.last_lf : in.last_lf;
    *a.out = out;
  }
}

// a last line without its LF: `in` is the carry after the last chunk
__global__ void tail_kernel(FqChunkArgs a, int64_t file_bytes) {
  const FqCarry in = *a.in;
  const int64_t bytes = file_bytes - in.last_lf - 1;  // of the unterminated line
  if (bytes <= 0 || (in.lines & 3) != 1) return;
  const int64_t len = bytes - 1;
  if (len < (int64_t)kFqDense) {
    atomicAdd(&a.hist[len], 1ull);
  } else {
    const unsigned long long slot = atomicAdd(a.n_longs, 1ull);
    if (slot < a.longs_cap) a.longs[slot] = len;
  }
}

// item i of the descending walk: the list, then the bins from the top
struct FqItemAt {
  const unsigned long long* hist;
  const int64_t* longs;
  uint64_t n_longs;
  __host__ __device__ int64_t length(uint64_t i) const {
    return i < n_longs ? longs[i] : (int64_t)(kFqDense - 1 - (i - n_longs));
  }
  __host__ __device__ FqItem operator()(uint64_t i) const {
    FqItem r;
    const int64_t len = length(i);
    r.count = i < n_longs ? 1 : hist[len];
    r.bases = r.count * (uint64_t)len;
    return r;
  }
};

struct FqItemOp {
  __host__ __device__ FqItem operator()(const FqItem& a, const FqItem& b) const {
    FqItem r;
    r.count = a.count + b.count;
    r.bases = a.bases + b.bases;
    return r;
  }
};

__global__ __launch_bounds__(kFqThreads) void find_kernel(FqReduceArgs a, uint64_t n_items) {
  const uint64_t i = (uint64_t)blockIdx.x * kFqThreads + threadIdx.x;
  if (i >= n_items) return;
  const FqItem total = a.cum[n_items - 1];
  if (i == 0) {
    a.out[0] = total.count;
    a.out[1] = total.bases;
  }
  if (!total.count) return;
  const FqItem cur = a.cum[i];
  FqItem below;
  below.count = below.bases = 0;
  if (i) below = a.cum[i - 1];
  if (cur.count == below.count) return;  // an empty bin
  FqItemAt at;
  at.hist = a.hist;
  at.longs = a.longs;
  at.n_longs = a.n_longs;
  const uint64_t len = (uint64_t)at.length(i);
  const uint64_t n = total.count, bp = total.bases;
  // desc[r]: the item whose running count first passes r
  const uint64_t rank[3] = {n / 2, n / 4, n * 3 / 4};
  for (int k = 0; k < 3; ++k)
    if (below.count <= rank[k] && rank[k] < cur.count) a.out[2 + k] = len;
  // the first length at which the running sum is above the mark
  const uint64_t mark[3] = {bp / 4, bp / 2, bp * 3 / 4};
  for (int k = 0; k < 3; ++k)
    if (below.bases <= mark[k] && mark[k] < cur.bases) {
      a.out[5 + k] = len;
      atomicOr((unsigned long long*)&a.out[8], 1ull << k);
    }
}

auto fq_items(const FqItemAt& at) {
  return rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), at);
}

FqBlock fq_block_zero() {
  FqBlock z;
  z.lines = 0;
  z.last_lf = -1;
  return z;
}

}  // namespace

size_t fq_scan_bytes(uint64_t n_blocks, uint64_t n_items) {
  size_t a = 0, b = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (const FqBlock*)nullptr, (FqBlock*)nullptr,
                                fq_block_zero(), (size_t)n_blocks, FqBlockOp(), hipStream_t(0));
  FqItemAt at{};
  (void)rocprim::inclusive_scan(nullptr, b, fq_items(at), (FqItem*)nullptr, (size_t)n_items,
                                FqItemOp(), hipStream_t(0));
  return a > b ? a : b;
}

size_t fq_sort_bytes(uint64_t n) {
  size_t a = 0;
  (void)rocprim::radix_sort_keys_desc(nullptr, a, (const int64_t*)nullptr, (int64_t*)nullptr,
                                      (size_t)n, 0, 64, hipStream_t(0));
  return a;
}

// workgroups of the length pass over n bytes: a few per compute unit, each
// walking many text blocks, so a bin's count reaches memory once per workgroup
unsigned fq_grid(uint64_t n, int n_cu) {
  const uint64_t blocks = depth_text_blocks(n);
  const uint64_t most = (uint64_t)(n_cu > 0 ? n_cu : 256) * 4;
  return (unsigned)(blocks < most ? (blocks ? blocks : 1) : most);
}

hipError_t launch_fq_line_index(const FqChunkArgs& a, void* scan_tmp, size_t scan_bytes,
                                hipStream_t s) {
  const uint32_t n_blocks = (uint32_t)depth_text_blocks((uint64_t)a.n);
  block_kernel<<<n_blocks + 1, kFqThreads, 0, s>>>(a.text, a.n, a.file_off, n_blocks, a.blk);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::exclusive_scan(scan_tmp, scan_bytes, (const FqBlock*)a.blk, a.pre,
                                 fq_block_zero(), (size_t)n_blocks + 1, FqBlockOp(), s);
}

hipError_t launch_fq_lengths(const FqChunkArgs& a, unsigned grid, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const uint32_t n_blocks = (uint32_t)depth_text_blocks((uint64_t)a.n);
  length_kernel<<<grid < n_blocks ? grid : n_blocks, kFqThreads, 0, s>>>(a, n_blocks);
  return hipGetLastError();
}

hipError_t launch_fq_tail(const FqChunkArgs& a, uint64_t file_bytes, hipStream_t s) {
  tail_kernel<<<1, 1, 0, s>>>(a, (int64_t)file_bytes);
  return hipGetLastError();
}

hipError_t launch_fq_sort(const int64_t* in, int64_t* out, uint64_t n, void* tmp, size_t bytes,
                          hipStream_t s) {
  if (!n) return hipSuccess;
  return rocprim::radix_sort_keys_desc(tmp, bytes, in, out, (size_t)n, 0, 64, s);
}

hipError_t launch_fq_reduce(const FqReduceArgs& a, void* scan_tmp, size_t scan_bytes,
                            hipStream_t s) {
  const uint64_t n_items = a.n_longs + kFqDense;
  FqItemAt at;
  at.hist = a.hist;
  at.longs = a.longs;
  at.n_longs = a.n_longs;
  if (hipError_t e = rocprim::inclusive_scan(scan_tmp, scan_bytes, fq_items(at), a.cum,
                                             (size_t)n_items, FqItemOp(), s))
    return e;
  find_kernel<<<(unsigned)((n_items + kFqThreads - 1) / kFqThreads), kFqThreads, 0, s>>>(a, n_items);
  return hipGetLastError();
}

}  // namespace magot
