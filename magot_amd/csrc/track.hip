// position_dic on the device (genome.py:981-1100): a bit track over the
// forward coordinates [0, span) of a packed genome, one bit per base (bit
// g & 31 of word g >> 5), every bit outside [kOrigin, extent) zero.
//
// Producers
//   class_kernel      one lane per word: 32 nibbles (one 16-byte load) ->
//                     the A/T or C/G class bits, the pad bases cleared,
//                     OR-ed into the track or replacing it.
//   (paint)           mask_paint_kernel of maskgen.hip sets interval pieces,
//                     straight into the track (value 1) or into a scratch
//                     plane that andnot_kernel then clears from it (value 0).
//   bytes_set_kernel  one lane per word of one contig: 32 staged bytes (two
//                     16-byte loads), non-zero -> bit; the bits of the
//                     neighbouring contigs in the edge words are kept.
// Consumers
//   bytes_get_kernel  the reverse: one word -> 32 bytes of 0 / 1.
//   rank directory    block_count_kernel (ones per kRankWords-word block) and
//                     rocprim's exclusive scan; rank(x) = ones below
//                     coordinate x = one directory entry + the block's words
//                     below x, at most kRankWords / 4 16-byte loads.
//   window_kernel     one lane per window of any contig: the difference of
//                     two ranks.  A wave finds the contig of its 64 windows
//                     once, on wave-uniform values.
//   flip_count_kernel / flip_write_kernel   the windows whose threshold test
//                     differs from the previous window's of the same contig:
//                     count per 64 windows (a wave's ballot), scan, write.
//   count_kernel      one lane per interval: the ones under it.
//
// Every pass streams HBM; none uses LDS or a workgroup barrier (the scans
// are rocprim's).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kTrackThreads = 256;

inline unsigned blocks_for(uint64_t n) {
  return (unsigned)((n + kTrackThreads - 1) / kTrackThreads);
}

// bit 4k of m (k = 0..7) -> bit k
__device__ __forceinline__ uint32_t gather_nibble_bits(uint32_t m) {
  m = (m | (m >> 3)) & 0x03030303u;
  m = (m | (m >> 6)) & 0x000F000Fu;
  return (m | (m >> 12)) & 0xFFu;
}

// the class bits of the 8 bases of one nibble word: code A=0 C=1 G=2 T=3, so
// A/T have equal code bits and C/G differing ones; exceptions (bit 3) are in
// neither class, the soft-mask bit (2) does not matter
__device__ __forceinline__ uint32_t class8(uint32_t x, bool gc) {
  const uint32_t differ = (x ^ (x >> 1)) & 0x11111111u;
  const uint32_t exc = (x >> 3) & 0x11111111u;
  return gather_nibble_bits((gc ? differ : differ ^ 0x11111111u) & ~exc);
}

// ones for the coordinates of word w that lie in [lo, hi)
__device__ __forceinline__ uint32_t word_range_mask(uint64_t w, uint64_t lo, uint64_t hi) {
  const uint64_t b = w << 5;
  if (b + 32 <= lo || b >= hi) return 0;
  uint32_t m = ~0u;
  if (lo > b) m &= ~0u << (lo - b);
  if (hi < b + 32) m &= ~0u >> (b + 32 - hi);
  return m;
}

__global__ __launch_bounds__(kTrackThreads) void class_kernel(
    const uint32_t* __restrict__ nib, uint64_t n_words, uint64_t lo, uint64_t hi, int gc,
    int replace, uint32_t* __restrict__ track) {
  const uint64_t w = (uint64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (w >= n_words) return;
  const uint4 v = reinterpret_cast<const uint4*>(nib)[w];
  uint32_t bits = class8(v.x, gc) | class8(v.y, gc) << 8 | class8(v.z, gc) << 16 |
                  class8(v.w, gc) << 24;
  bits &= word_range_mask(w, lo, hi);  // pad bases are code 0 ('A')
  track[w] = replace ? bits : (track[w] | bits);
}

__global__ __launch_bounds__(kTrackThreads) void andnot_kernel(uint32_t* __restrict__ track,
                                                               const uint32_t* __restrict__ clear,
                                                               uint64_t n_words) {
  const uint64_t q = (uint64_t)blockIdx.x * kTrackThreads + threadIdx.x;  // four words
  if (q * 4 >= n_words) return;
  // the planes are allocated in whole 16-byte groups
  uint4 t = reinterpret_cast<uint4*>(track)[q];
  const uint4 c = reinterpret_cast<const uint4*>(clear)[q];
  t.x &= ~c.x;
  t.y &= ~c.y;
  t.z &= ~c.z;
  t.w &= ~c.w;
  reinterpret_cast<uint4*>(track)[q] = t;
}

// 0x01 in every non-zero byte's lowest bit, gathered to 4 bits
__device__ __forceinline__ uint32_t nonzero4(uint32_t x) {
  // bit 7 of each byte: byte != 0 (no carry crosses a byte)
  const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
  return ((nz >> 7) * 0x10204080u) >> 28;  // bits 0, 8, 16, 24 -> 28..31 -> 0..3
}

__device__ __forceinline__ uint32_t nonzero16(uint4 v) {
  return nonzero4(v.x) | nonzero4(v.y) << 4 | nonzero4(v.z) << 8 | nonzero4(v.w) << 12;
}

// stage holds the contig's bytes at stage[(lo & 31) + i]: coordinate g is
// byte g - 32 * w0, so every word's 32 bytes are two aligned 16-byte loads
__global__ __launch_bounds__(kTrackThreads) void bytes_set_kernel(
    const uint8_t* __restrict__ stage, uint64_t w0, uint64_t n, uint64_t lo, uint64_t hi,
    uint32_t* __restrict__ track) {
  const uint64_t k = (uint64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (k >= n) return;
  const uint4* p = reinterpret_cast<const uint4*>(stage + 32 * k);
  const uint32_t bits = nonzero16(p[0]) | nonzero16(p[1]) << 16;
  const uint32_t m = word_range_mask(w0 + k, lo, hi);
  track[w0 + k] = (track[w0 + k] & ~m) | (bits & m);
}

// bits 0..3 of n -> 0x01 / 0x00 in bytes 0..3
__device__ __forceinline__ uint32_t spread_ones4(uint32_t n) {
  return ((n & 15u) * 0x00204081u) & 0x01010101u;
}

__device__ __forceinline__ uint4 spread_ones16(uint32_t n) {
  uint4 o;
  o.x = spread_ones4(n);
  o.y = spread_ones4(n >> 4);
  o.z = spread_ones4(n >> 8);
  o.w = spread_ones4(n >> 12);
  return o;
}

__global__ __launch_bounds__(kTrackThreads) void bytes_get_kernel(
    const uint32_t* __restrict__ track, uint64_t w0, uint64_t n, uint8_t* __restrict__ stage) {
  const uint64_t k = (uint64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (k >= n) return;
  const uint32_t bits = track[w0 + k];
  uint4* p = reinterpret_cast<uint4*>(stage + 32 * k);
  p[0] = spread_ones16(bits);
  p[1] = spread_ones16(bits >> 16);
}

__device__ __forceinline__ uint32_t popc4(uint4 v) {
  return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
}

__global__ __launch_bounds__(kTrackThreads) void block_count_kernel(
    const uint32_t* __restrict__ track, uint64_t n_blocks, uint32_t* __restrict__ count) {
  const uint64_t b = (uint64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (b > n_blocks) return;
  uint32_t c = 0;
  if (b < n_blocks) {  // entry n_blocks is the sentinel: its prefix is the total
    const uint4* p = reinterpret_cast<const uint4*>(track + b * kRankWords);
#pragma unroll
    for (int q = 0; q < kRankWords / 4; ++q) c += popc4(p[q]);
  }
  count[b] = c;
}

// ones at coordinates below x (x <= span): the plane is allocated in whole
// blocks, and no quarter of a block is loaded unless a coordinate below x
// lies in it
__device__ __forceinline__ uint32_t rank_of(const uint32_t* __restrict__ track,
                                            const uint32_t* __restrict__ rank, uint64_t x) {
  const uint64_t b = x / (32 * kRankWords);
  const uint32_t rem = (uint32_t)(x % (32 * kRankWords));
  uint32_t r = rank[b];
  const uint4* p = reinterpret_cast<const uint4*>(track + b * kRankWords);
#pragma unroll
  for (int q = 0; q < kRankWords / 4; ++q) {
    const uint32_t base = 128u * q;
    if (rem <= base) break;
    uint4 v = p[q];
    const uint32_t left = rem - base;  // bits of this quarter below x
    if (left < 128) {
      const uint32_t full = left >> 5, part = left & 31;
      const uint32_t pm = part ? ~0u >> (32 - part) : 0u;
      v.x &= full > 0 ? ~0u : pm;
      v.y &= full > 1 ? ~0u : (full == 1 ? pm : 0u);
      v.z &= full > 2 ? ~0u : (full == 2 ? pm : 0u);
      v.w &= full == 3 ? pm : 0u;
    }
    r += popc4(v);
  }
  return r;
}

// largest c in [lo, hi] with first[c] <= x
__device__ __forceinline__ uint64_t contig_of(const uint64_t* __restrict__ first, uint64_t lo,
                                              uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (first[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kTrackThreads) void window_kernel(TrackWindowArgs a) {
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t i0 = ((uint64_t)blockIdx.x * (kTrackThreads / 64) + wv) * 64;
  if (i0 >= a.n_windows) return;
  // the contigs of the wave's 64 windows: one search pair on wave-uniform
  // values; nearly every wave lies inside one contig
  const uint64_t last = min(i0 + 63, a.n_windows - 1);
  const uint64_t c_lo = contig_of(a.first, 0, a.n_contigs - 1, i0);
  const uint64_t c_hi = contig_of(a.first, c_lo, a.n_contigs - 1, last);
  const uint64_t i = i0 + (threadIdx.x & 63);
  if (i >= a.n_windows) return;
  const uint64_t c = c_lo == c_hi ? c_lo : contig_of(a.first, c_lo, c_hi, i);
  const uint64_t g = a.contig_base[c] + (i - a.first[c]) * a.jump;
  a.sums[i] = rank_of(a.track, a.rank, g + a.W) - rank_of(a.track, a.rank, g);
}

// does window i pass the test and its predecessor in the same contig not, or
// the reverse (nothing passes before a contig's window 0); false past the last
// window.  i0 is the wave's first window: the contig search is window_kernel's.
__device__ __forceinline__ bool flips_at(const TrackWindowArgs& a, uint32_t s_min, uint64_t i0,
                                         uint64_t i) {
  const uint64_t last = min(i0 + 63, a.n_windows - 1);
  const uint64_t c_lo = contig_of(a.first, 0, a.n_contigs - 1, i0);
  const uint64_t c_hi = contig_of(a.first, c_lo, a.n_contigs - 1, last);
  if (i >= a.n_windows) return false;
  const uint64_t c = c_lo == c_hi ? c_lo : contig_of(a.first, c_lo, c_hi, i);
  const bool p = a.sums[i] >= s_min;
  const bool prev = i > a.first[c] && a.sums[i - 1] >= s_min;
  return p != prev;
}

// one wave per group of 64 windows, one lane per window: the group's count is
// a ballot's popcount, a flip's place in the list its rank among the lanes
__global__ __launch_bounds__(kTrackThreads) void flip_count_kernel(TrackWindowArgs a,
                                                                   uint32_t s_min,
                                                                   uint64_t n_groups) {
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g = (uint64_t)blockIdx.x * (kTrackThreads / 64) + wv;
  const uint32_t lane = threadIdx.x & 63;
  if (g > n_groups) return;
  if (g == n_groups) {  // sentinel: its prefix is the total
    if (lane == 0) a.flip_count[g] = 0;
    return;
  }
  const uint64_t mask = __ballot(flips_at(a, s_min, g * 64, g * 64 + lane));
  if (lane == 0) a.flip_count[g] = (uint32_t)__popcll(mask);
}

__global__ __launch_bounds__(kTrackThreads) void flip_write_kernel(TrackWindowArgs a,
                                                                   uint32_t s_min,
                                                                   uint64_t n_groups,
                                                                   uint64_t cap) {
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g = (uint64_t)blockIdx.x * (kTrackThreads / 64) + wv;
  const uint32_t lane = threadIdx.x & 63;
  if (g >= n_groups || !a.flip_count[g]) return;
  const bool flip = flips_at(a, s_min, g * 64, g * 64 + lane);
  const uint64_t mask = __ballot(flip);
  const uint64_t at = a.flip_slot[g] + __popcll(mask & ((1ull << lane) - 1));
  if (flip && at < cap) a.flip_index[at] = g * 64 + lane;
}

__global__ __launch_bounds__(kTrackThreads) void count_kernel(
    const magot_mask_interval* __restrict__ rows, uint64_t n_rows,
    const uint64_t* __restrict__ contig_base, const uint32_t* __restrict__ track,
    const uint32_t* __restrict__ rank, uint64_t span, uint32_t* __restrict__ ones) {
  const uint64_t i = (uint64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i >= n_rows) return;
  const magot_mask_interval iv = rows[i];
  const uint64_t b = contig_base[iv.contig] + iv.start;
  const uint64_t e = b + iv.len;
  // the host checked every row: never taken
  ones[i] = e > span ? 0u : rank_of(track, rank, e) - rank_of(track, rank, b);
}

}  // namespace

size_t track_scan_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                uint32_t(0), (size_t)n, rocprim::plus<uint32_t>(), hipStream_t(0));
  (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint64_t*)nullptr,
                                uint64_t(0), (size_t)n, rocprim::plus<uint64_t>(), hipStream_t(0));
  return a > b ? a : b;
}

hipError_t launch_track_class(const uint32_t* nib, uint64_t n_words, uint64_t lo, uint64_t hi,
                              bool gc, bool replace, uint32_t* track, hipStream_t s) {
  if (!n_words) return hipSuccess;
  class_kernel<<<blocks_for(n_words), kTrackThreads, 0, s>>>(nib, n_words, lo, hi, gc, replace,
                                                             track);
  return hipGetLastError();
}

hipError_t launch_track_andnot(uint32_t* track, const uint32_t* clear, uint64_t n_words,
                               hipStream_t s) {
  if (!n_words) return hipSuccess;
  andnot_kernel<<<blocks_for((n_words + 3) / 4), kTrackThreads, 0, s>>>(track, clear, n_words);
  return hipGetLastError();
}

hipError_t launch_track_bytes_set(const uint8_t* stage, uint64_t lo, uint64_t hi, uint32_t* track,
                                  hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  const uint64_t w0 = lo >> 5, n = ((hi + 31) >> 5) - w0;
  bytes_set_kernel<<<blocks_for(n), kTrackThreads, 0, s>>>(stage, w0, n, lo, hi, track);
  return hipGetLastError();
}

hipError_t launch_track_bytes_get(const uint32_t* track, uint64_t lo, uint64_t hi, uint8_t* stage,
                                  hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  const uint64_t w0 = lo >> 5, n = ((hi + 31) >> 5) - w0;
  bytes_get_kernel<<<blocks_for(n), kTrackThreads, 0, s>>>(track, w0, n, stage);
  return hipGetLastError();
}

hipError_t launch_track_rank(const uint32_t* track, uint64_t n_blocks, uint32_t* count,
                             uint32_t* rank, void* scan_tmp, size_t scan_bytes, hipStream_t s) {
  block_count_kernel<<<blocks_for(n_blocks + 1), kTrackThreads, 0, s>>>(track, n_blocks, count);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::exclusive_scan(scan_tmp, scan_bytes, count, rank, uint32_t(0),
                                 (size_t)(n_blocks + 1), rocprim::plus<uint32_t>(), s);
}

hipError_t launch_track_windows(const TrackWindowArgs& a, hipStream_t s) {
  if (!a.n_windows) return hipSuccess;
  window_kernel<<<blocks_for(a.n_windows), kTrackThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_track_flip_count(const TrackWindowArgs& a, uint32_t s_min, void* scan_tmp,
                                   size_t scan_bytes, hipStream_t s) {
  const uint64_t groups = track_flip_groups(a.n_windows);
  flip_count_kernel<<<blocks_for((groups + 1) * 64), kTrackThreads, 0, s>>>(a, s_min, groups);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::exclusive_scan(scan_tmp, scan_bytes, a.flip_count, a.flip_slot, uint64_t(0),
                                 (size_t)(groups + 1), rocprim::plus<uint64_t>(), s);
}

hipError_t launch_track_flip_write(const TrackWindowArgs& a, uint32_t s_min, uint64_t cap,
                                   hipStream_t s) {
  const uint64_t groups = track_flip_groups(a.n_windows);
  if (!groups || !cap) return hipSuccess;
  flip_write_kernel<<<blocks_for(groups * 64), kTrackThreads, 0, s>>>(a, s_min, groups, cap);
  return hipGetLastError();
}

hipError_t launch_track_count(const magot_mask_interval* rows, uint64_t n_rows,
                              const uint64_t* contig_base, const uint32_t* track,
                              const uint32_t* rank, uint64_t span, uint32_t* ones, hipStream_t s) {
  if (!n_rows) return hipSuccess;
  count_kernel<<<blocks_for(n_rows), kTrackThreads, 0, s>>>(rows, n_rows, contig_base, track,
                                                            rank, span, ones);
  return hipGetLastError();
}

}  // namespace magot
