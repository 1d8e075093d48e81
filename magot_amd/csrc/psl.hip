// besthits_from_psl on the device (genome_tools.py:572-592): for every query
// name of a PSL the line with the highest matches - misMatches, as a reduction
// keyed by a string.  The whole text is resident: the verification reads the
// key bytes of any two lines.
//
//   the line index  textindex.hip's count and fill over the LFs, line mode: the
//                   total gives n_lines on the host, ix.pos[k] is where line k
//                   starts.
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
// No LDS, no spin-wait, no compare-and-swap loop; nothing is float.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kPslThreads = 256;
constexpr int kPslLane = 16;

inline unsigned psl_blocks_for(uint64_t n) { return (unsigned)((n + kPslThreads - 1) / kPslThreads); }

__device__ __forceinline__ bool psl_pass_byte(uint32_t c) {
  return c == 'p' || c == '\n' || c == 'm' || c == '-' || c == '\t' || c == ' ';
}

__global__ __launch_bounds__(kPslThreads) void psl_parse_kernel(PslArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (k > a.ix.n_lines) return;
  if (k == a.ix.n_lines) {  // the scan's last entry: the data lines of the text
    a.kind[k] = 0;
    return;
  }
  const uint64_t start = a.ix.pos[k], end = a.ix.pos[k + 1];  // start < end <= n
  uint32_t tabs = 0, nd0 = 0, nd1 = 0, key_len = 0;
  uint64_t v0 = 0, v1 = 0, h = 0, key_off = end;
  bool bad0 = false, bad1 = false, data = true, done = false;
  for (uint64_t base = start & ~15ull; base < end && !done; base += kPslLane) {
    const uint4 q = *reinterpret_cast<const uint4*>(a.ix.text + base);
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
          h = py27_hash_step(h, key_len++, c);
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
  a.hash[k] = py27_hash_end(h, key_len);
  a.key_off[k] = key_off;
  a.key_len[k] = key_len;
  a.rank[k] = psl_rank((int64_t)v0 - (int64_t)v1, k);
}

__global__ __launch_bounds__(kPslThreads) void psl_scatter_kernel(PslArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kPslThreads + threadIdx.x;
  if (k >= a.ix.n_lines) return;
  const uint64_t d = a.dpos[k];  // below n_data when this is a data line, else k - d below the rest
  if (a.kind[k]) {
    const uint64_t mask = a.hash_bits >= 64 ? ~0ull : (1ull << a.hash_bits) - 1;
    a.skey[d] = a.hash[k] & mask;
    a.sval[d] = a.rank[k];
  } else {
    const uint64_t start = a.ix.pos[k];
    a.pass_off[k - d] = start;
    a.pass_len[k - d] = a.ix.pos[k + 1] - start;
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
    const uint8_t* x = a.ix.text + a.key_off[la];  // key_off + key_len is at most the line's end
    const uint8_t* y = a.ix.text + a.key_off[lb];
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
  const uint64_t off = a.ix.pos[line];
  a.g_hash[r] = a.hash[first];
  a.g_first[r] = first;
  a.g_best[r] = (uint32_t)line;
  a.g_score[r] = psl_rank_score(best);
  a.g_off[r] = off;
  a.g_len[r] = a.ix.pos[line + 1] - off;
}

}  // namespace

size_t psl_tmp_bytes(uint64_t n_lines) {
  size_t b = 0, c = 0, d = 0;
  const size_t n = (size_t)n_lines;
  const size_t a = exclusive_sum_bytes<uint32_t>(n + 1);
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

hipError_t launch_psl_parse(const PslArgs& a, hipStream_t s) {
  psl_parse_kernel<<<psl_blocks_for(a.ix.n_lines + 1), kPslThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_psl_compact(const PslArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  return exclusive_sum(tmp, tmp_bytes, a.kind, a.dpos, a.ix.n_lines + 1, s);
}

hipError_t launch_psl_scatter(const PslArgs& a, hipStream_t s) {
  if (!a.ix.n_lines) return hipSuccess;
  psl_scatter_kernel<<<psl_blocks_for(a.ix.n_lines), kPslThreads, 0, s>>>(a);
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
