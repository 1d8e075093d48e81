// besthits_from_psl on the device (genome_tools.py:572-592): for every query
// name of a PSL the line with the highest matches - misMatches, as a reduction
// keyed by a string.  The whole text is resident: the verification reads the
// key bytes of any two lines.
//
//   count_kernel    per text block of kTextBlock bytes, one 16-byte load per
//                   lane: the LFs.  One rocprim exclusive scan gives each block
//                   the LFs before it, and the total: n_lines on the host.
//   fill_kernel     a lane owns the LFs of its 16 bytes: LF number j (from 0)
//                   at byte p gives line_start[j + 1] = p + 1.
//   parse_kernel    one lane per line, 16 aligned bytes per load, every loop
//                   bounded by the line's end.  The first byte says pass-through
//                   or data; a data line gives field 0 and field 1, the key span
//                   after the 9th tab and CPython 2.7's string hash of it, and
//                   rank = psl_rank(score, line).  The walk stops at the 10th
//                   tab, so the long lists at a PSL line's end are not read.  A
//                   line outside the grammar atomic-mins (line, reason) into the
//                   status word and stops nothing.
//   scatter_kernel  after an exclusive scan of the data flags: the data lines'
//                   (masked hash, rank) compacted in line order, the
//                   pass-through lines' (offset, length) in file order.
//   a stable rocprim radix sort of the pairs by the masked hash: within a key
//                   the ranks stay in line order.
//   verify_kernel   one lane per sorted element whose masked hash equals its
//                   predecessor's: the two lines' keys compared, length then
//                   bytes; a difference is atomic-minned as a hash collision.
//                   Equality of neighbours is transitive, so a clean pass means
//                   every run of equal masked hashes is one key.
//   rocprim reduce_by_key over the masked hashes: per key the maximum rank (the
//                   best line) and the maximum of the ranks' line bits (the
//                   first line).
//   seg_kernel, a radix sort of the keys by first line, gather_kernel: the
//                   rows of magot_psl_groups in first-seen order.
//
// No LDS beyond the wave totals of the two index kernels, no spin-wait, no
// compare-and-swap loop; nothing is float.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kPslThreads = 256;
constexpr int kPslLane = 16;
constexpr int kPslWaves = kPslThreads / 64;
static_assert(kTextBlock == kPslThreads * kPslLane, "one 16-byte load per lane");

inline unsigned psl_blocks_for(uint64_t n) { return (unsigned)((n + kPslThreads - 1) / kPslThreads); }

// bit k: byte k of x is LF (fastq.hip, depth.hip)
__device__ __forceinline__ uint32_t psl_lf_mask4(uint32_t x) {
  x ^= 0x0A0A0A0Au;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;  // bit 7: low seven bits non-zero
  const uint32_t z = ~(t | x | 0x7f7f7f7fu) >> 7;      // bits 0, 8, 16, 24
  return (z * 0x00204081u) >> 21 & 0xFu;
}

// bit j: byte i + j of the text is LF (i the lane's first byte)
__device__ __forceinline__ uint32_t psl_lane_lfs(const uint8_t* __restrict__ text, uint64_t i,
                                                 uint64_t n) {
  if (i >= n) return 0;
  const uint4 v = *reinterpret_cast<const uint4*>(text + i);  // readable to the next 16
  uint32_t m = psl_lf_mask4(v.x) | psl_lf_mask4(v.y) << 4 | psl_lf_mask4(v.z) << 8 |
               psl_lf_mask4(v.w) << 12;
  if (n - i < kPslLane) m &= (1u << (n - i)) - 1;  // the bytes behind the text are anything
  return m;
}

__global__ __launch_bounds__(kPslThreads) void psl_count_kernel(PslArgs a) {
  __shared__ uint32_t wave_count[kPslWaves];
  const int t = threadIdx.x;
  uint32_t c = 0;
  if (blockIdx.x < a.n_blocks)  // block n_blocks is the sentinel: its prefix is the total
    c = __popc(psl_lane_lfs(a.text, (uint64_t)blockIdx.x * kTextBlock + kPslLane * t, a.n));
  for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
  if ((t & 63) == 0) wave_count[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0;
    for (int w = 0; w < kPslWaves; ++w) sum += wave_count[w];
    a.blk[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(kPslThreads) void psl_fill_kernel(PslArgs a) {
  __shared__ uint32_t wave_count[kPslWaves];
  const int t = threadIdx.x;
  const uint32_t lane = t & 63, wave = t >> 6;
  const uint64_t p0 = (uint64_t)blockIdx.x * kTextBlock + kPslLane * t;
  const uint32_t lf = psl_lane_lfs(a.text, p0, a.n);
  const uint32_t c = __popc(lf);
  uint32_t inc = c;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += up;
  }
  if (lane == 63) wave_count[wave] = inc;
  __syncthreads();
  if (lf) {
    // LF number j is below the text's LFs, and those are at most n_lines
    uint64_t j = a.pre[blockIdx.x] + (inc - c);
    for (uint32_t w = 0; w < wave; ++w) j += wave_count[w];
    for (uint32_t m = lf; m; m &= m - 1, ++j) a.line_start[j + 1] = p0 + __ffs(m);
  }
  if (blockIdx.x == 0 && t == 0) {
    a.line_start[0] = 0;
    a.line_start[a.n_lines] = a.n;  // a last line without LF ends with the text
  }
}

__device__ __forceinline__ bool psl_pass_byte(uint32_t c) {
  return c == 'p' || c == '\n' || c == 'm' || c == '-' || c == '\t' || c == ' ';
}

__global__ __launch_bounds__(kPslThreads) void psl_parse_kernel(PslArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (k > a.n_lines) return;
  if (k == a.n_lines) {  // the scan's last entry: the data lines of the text
    a.kind[k] = 0;
    return;
  }
  const uint64_t start = a.line_start[k], end = a.line_start[k + 1];  // start < end <= n
  uint32_t tabs = 0, nd0 = 0, nd1 = 0, key_len = 0;
  uint64_t v0 = 0, v1 = 0, h = 0, key_off = end;
  bool bad0 = false, bad1 = false, data = true, done = false;
  for (uint64_t base = start & ~15ull; base < end && !done; base += kPslLane) {
    const uint4 q = *reinterpret_cast<const uint4*>(a.text + base);
    const uint32_t lo = base < start ? (uint32_t)(start - base) : 0;
    const uint32_t hi = end - base < kPslLane ? (uint32_t)(end - base) : kPslLane;
#pragma unroll
    for (uint32_t b = 0; b < kPslLane; ++b) {
      if (b < lo || b >= hi || done) continue;
      const uint32_t word = b < 4 ? q.x : b < 8 ? q.y : b < 12 ? q.z : q.w;
      const uint32_t c = word >> ((b & 3) * 8) & 0xffu;
      if (base + b == start && psl_pass_byte(c)) {
        data = false;
        done = true;
      } else if (tabs == 9) {
        if (c == '\t') {
          done = true;  // the key ends at the 10th tab
        } else {
          if (!key_len) h = (uint64_t)c << 7;
          h = (h * 1000003ull) ^ c;
          ++key_len;
        }
      } else if (c == '\t') {
        if (++tabs == 9) key_off = base + b + 1;
      } else if (tabs == 0) {
        if (c >= '0' && c <= '9') {
          if (++nd0 <= 10) v0 = v0 * 10 + (c - '0');
        } else {
          bad0 = true;
        }
      } else if (tabs == 1) {
        if (c >= '0' && c <= '9') {
          if (++nd1 <= 10) v1 = v1 * 10 + (c - '0');
        } else {
          bad1 = true;
        }
      }
    }
  }
  a.kind[k] = data ? 1u : 0u;
  if (!data) return;
  uint32_t reason = 0;
  if (tabs < 9) reason = MAGOT_PSL_FEW_FIELDS;
  else if (bad0 || !nd0) reason = MAGOT_PSL_INTEGER_FORM;
  else if (nd0 > 10 || v0 > 0x7fffffffull) reason = MAGOT_PSL_NUMBER_RANGE;
  else if (bad1 || !nd1) reason = MAGOT_PSL_INTEGER_FORM;
  else if (nd1 > 10 || v1 > 0x7fffffffull) reason = MAGOT_PSL_NUMBER_RANGE;
  if (reason) {
    atomicMin(a.status, (unsigned long long)(k << 8 | reason));
    v0 = v1 = 0;
  }
  if (key_len) {
    h ^= key_len;
    if (h == ~0ull) h = ~0ull - 1;
  }
  a.hash[k] = h;
  a.key_off[k] = key_off;
  a.key_len[k] = key_len;
  a.rank[k] = psl_rank((int64_t)v0 - (int64_t)v1, k);
}

__global__ __launch_bounds__(kPslThreads) void psl_scatter_kernel(PslArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (k >= a.n_lines) return;
  const uint64_t d = a.dpos[k];  // below n_data when this is a data line, else k - d below the rest
  if (a.kind[k]) {
    const uint64_t mask = a.hash_bits >= 64 ? ~0ull : (1ull << a.hash_bits) - 1;
    a.skey[d] = a.hash[k] & mask;
    a.sval[d] = a.rank[k];
  } else {
    const uint64_t start = a.line_start[k];
    a.pass_off[k - d] = start;
    a.pass_len[k - d] = a.line_start[k + 1] - start;
  }
}

__global__ __launch_bounds__(kPslThreads) void psl_verify_kernel(PslArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (i == 0 || i >= a.n_data) return;
  if (a.skey_sorted[i] != a.skey_sorted[i - 1]) return;
  const uint64_t la = psl_rank_line(a.sval_sorted[i]);      // ranks hold lines below n_lines
  const uint64_t lb = psl_rank_line(a.sval_sorted[i - 1]);
  const uint32_t len = a.key_len[la];
  bool same = len == a.key_len[lb];
  if (same) {
    const uint8_t* x = a.text + a.key_off[la];  // key_off + key_len is at most the line's end
    const uint8_t* y = a.text + a.key_off[lb];
    for (uint32_t j = 0; j < len && same; ++j) same = x[j] == y[j];
  }
  if (!same) atomicMin(a.status, (unsigned long long)(la << 8 | MAGOT_PSL_HASH_COLLISION));
}

struct PslToAgg {
  __host__ __device__ PslAgg operator()(uint64_t rank) const {
    PslAgg r;
    r.best = rank;
    r.first = rank & kPslLineMask;
    return r;
  }
};

struct PslAggMax {
  __host__ __device__ PslAgg operator()(const PslAgg& x, const PslAgg& y) const {
    PslAgg r;
    r.best = x.best > y.best ? x.best : y.best;
    r.first = x.first > y.first ? x.first : y.first;
    return r;
  }
};

auto psl_aggs(const uint64_t* ranks) {
  return rocprim::make_transform_iterator(ranks, PslToAgg());
}

__global__ __launch_bounds__(kPslThreads) void psl_seg_kernel(PslArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (g >= a.n_groups) return;
  a.seg_first[g] = (uint32_t)(kPslLineMask - a.agg[g].first);
  a.seg_id[g] = (uint32_t)g;
}

__global__ __launch_bounds__(kPslThreads) void psl_gather_kernel(PslArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (r >= a.n_groups) return;
  const uint32_t first = a.seg_first_sorted[r];      // lines, below n_lines
  const uint64_t best = a.agg[a.seg_id_sorted[r]].best;
  const uint64_t line = psl_rank_line(best);
  const uint64_t off = a.line_start[line];
  a.g_hash[r] = a.hash[first];
  a.g_first[r] = first;
  a.g_best[r] = (uint32_t)line;
  a.g_score[r] = psl_rank_score(best);
  a.g_off[r] = off;
  a.g_len[r] = a.line_start[line + 1] - off;
}

}  // namespace

size_t psl_count_tmp_bytes(uint64_t n_blocks) {
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                uint64_t(0), (size_t)n_blocks + 1, rocprim::plus<uint64_t>(),
                                hipStream_t(0));
  return b;
}

size_t psl_tmp_bytes(uint64_t n_lines) {
  size_t a = 0, b = 0, c = 0, d = 0;
  const size_t n = (size_t)n_lines;
  (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                uint32_t(0), n + 1, rocprim::plus<uint32_t>(), hipStream_t(0));
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                  (const uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 64,
                                  hipStream_t(0));
  (void)rocprim::reduce_by_key(nullptr, c, (const uint64_t*)nullptr,
                               psl_aggs((const uint64_t*)nullptr), n, (uint64_t*)nullptr,
                               (PslAgg*)nullptr, (unsigned long long*)nullptr, PslAggMax(),
                               rocprim::equal_to<uint64_t>(), hipStream_t(0));
  (void)rocprim::radix_sort_pairs(nullptr, d, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32,
                                  hipStream_t(0));
  return std::max(std::max(a, b), std::max(c, d));
}

hipError_t launch_psl_count(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  psl_count_kernel<<<(unsigned)a.n_blocks + 1, kPslThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::exclusive_scan(tmp, tmp_bytes, (const uint64_t*)a.blk, a.pre, uint64_t(0),
                                 (size_t)a.n_blocks + 1, rocprim::plus<uint64_t>(), s);
}

hipError_t launch_psl_fill(const PslArgs& a, hipStream_t s) {
  if (!a.n_blocks) return hipSuccess;
  psl_fill_kernel<<<(unsigned)a.n_blocks, kPslThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_psl_parse(const PslArgs& a, hipStream_t s) {
  psl_parse_kernel<<<psl_blocks_for(a.n_lines + 1), kPslThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_psl_compact(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, (const uint32_t*)a.kind, a.dpos, uint32_t(0),
                                 (size_t)a.n_lines + 1, rocprim::plus<uint32_t>(), s);
}

hipError_t launch_psl_scatter(const PslArgs& a, hipStream_t s) {
  if (!a.n_lines) return hipSuccess;
  psl_scatter_kernel<<<psl_blocks_for(a.n_lines), kPslThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_psl_sort(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (!a.n_data) return hipSuccess;
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint64_t*)a.skey, a.skey_sorted,
                                   (const uint64_t*)a.sval, a.sval_sorted, (size_t)a.n_data, 0,
                                   a.hash_bits, s);
}

hipError_t launch_psl_verify(const PslArgs& a, hipStream_t s) {
  if (a.n_data < 2) return hipSuccess;
  psl_verify_kernel<<<psl_blocks_for(a.n_data), kPslThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_psl_reduce(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (!a.n_data) return hipMemsetAsync(a.n_uniq, 0, sizeof *a.n_uniq, s);
  return rocprim::reduce_by_key(tmp, tmp_bytes, (const uint64_t*)a.skey_sorted,
                                psl_aggs(a.sval_sorted), (size_t)a.n_data, a.uniq, a.agg, a.n_uniq,
                                PslAggMax(), rocprim::equal_to<uint64_t>(), s);
}

hipError_t launch_psl_order(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (!a.n_groups) return hipSuccess;
  psl_seg_kernel<<<psl_blocks_for(a.n_groups), kPslThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint32_t*)a.seg_first,
                                               a.seg_first_sorted, (const uint32_t*)a.seg_id,
                                               a.seg_id_sorted, (size_t)a.n_groups, 0, 32, s))
    return e;
  psl_gather_kernel<<<psl_blocks_for(a.n_groups), kPslThreads, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace magot
