// Interval joins on the device: purge_overlaps (genome_tools.py:548-568) and
// annotation_overlap (annotation_funcs.py:13-30), the reference's two loops
// over every pair, as a sort and a few binary searches per query.
//
// Index build (once per interval set of n intervals (seqid, p0, p1)):
//   keys_kernel      per interval its composite keys ov_key(seqid, p0) and
//                    ov_key(seqid, p1) for each of three tables; an interval a
//                    table leaves out gets the all-ones key there:
//                      in   p0 <  p1   starts, ends
//                      all  every      starts
//                      cl   p0 <= p1   starts carrying p1, ends
//   five rocprim radix sorts (four of keys, one of pairs); the left-out keys
//                    end up behind the last segment.
//   segment_kernel   one lane per (table, seqid): the first key of the seqid,
//                    by binary search.  A query searches [seg[s], seg[s + 1])
//                    only, so no search leaves its seqid and each takes
//                    log2(segment) steps, not log2(n).
//
// Queries, one lane each, in the caller's order (GFF lines arrive sorted by
// position almost always: neighbouring lanes then walk the same search path
// and share its cache lines; nothing depends on it but speed):
//   purge_kernel     all comparisons strict; (c0, c1) unordered.
//                      p0 < x < p1 for x = c0, then c1: among p0 < p1 every
//                        p1 <= x has p0 < x, so #{p0 < x} - #{p1 <= x} counts
//                        them: lower_bound(in_s, x) > upper_bound(in_e, x);
//                      c0 < p0 < c1 over all starts:
//                        lower_bound(all_s, c1) > upper_bound(all_s, c0).
//   overlap_kernel   closed comparisons; lo = min(q), hi = max(q); only
//                    p0 <= p1 can match.  Count = S + R,
//                      S = #{p0 <= lo <= p1} = upper_bound(cl_s, lo) -
//                          lower_bound(cl_e, lo),
//                      R = #{lo < p0 <= hi, p1 >= hi}: the slice
//                          [upper_bound(cl_s, lo), upper_bound(cl_s, hi)) of
//                          the start-sorted table, each end beside its start.
//                    A slice of at most kOvLaneScan intervals is scanned by the
//                    lane itself; a longer one is appended to a list.
//   long_kernel      one wave per listed query, lanes strided over the slice,
//                    one ballot + popcount per 64 intervals; a fixed grid
//                    walks the list, whose length stays on the device.
//
// No LDS, no barrier; every table index is below a segment bound, every
// segment bound at most n.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kOvThreads = 256;
constexpr int kOvWave = 64;
constexpr uint64_t kOvLeftOut = ~0ull;

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kOvThreads - 1) / kOvThreads); }

// first index in [lo, hi) whose key is >= k (hi when none)
__device__ inline uint64_t lower_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t k) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// first index in [lo, hi) whose key is > k (hi when none)
__device__ inline uint64_t upper_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t k) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] <= k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kOvThreads) void ov_keys_kernel(OvBuildArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kOvThreads + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t s = a.seq[i];
  const int64_t p0 = a.p0[i], p1 = a.p1[i];
  const uint64_t ks = ov_key(s, p0), ke = ov_key(s, p1);
  a.raw[i] = p0 < p1 ? ks : kOvLeftOut;
  a.raw[a.n + i] = p0 < p1 ? ke : kOvLeftOut;
  a.raw[2 * a.n + i] = ks;
  a.raw[3 * a.n + i] = p0 <= p1 ? ks : kOvLeftOut;
  a.raw[4 * a.n + i] = p0 <= p1 ? ke : kOvLeftOut;
  a.raw_v[i] = p1;
}

__global__ __launch_bounds__(kOvThreads) void ov_segment_kernel(OvBuildArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * kOvThreads + threadIdx.x;
  const uint64_t per = (uint64_t)a.n_seq + 1;
  if (t >= 3 * per) return;
  const uint32_t table = (uint32_t)(t / per);
  const uint64_t s = t % per;
  const uint64_t* keys = table == 0 ? a.in_s : table == 1 ? a.all_s : a.cl_s;
  uint64_t* seg = table == 0 ? a.seg_in : table == 1 ? a.seg_all : a.seg_cl;
  // s == n_seq <= kOvMaxSeq: the key is at most the left-out key
  seg[s] = lower_bound(keys, 0, a.n, s << kOvCoordBits);
}

__global__ __launch_bounds__(kOvThreads) void ov_purge_kernel(OvIndex ix, OvQuery q, uint8_t* drop) {
  const uint64_t i = (uint64_t)blockIdx.x * kOvThreads + threadIdx.x;
  if (i >= q.n) return;
  const uint32_t s = q.seq[i];
  bool hit = false;
  if (s < ix.n_seq) {
    const int64_t c0 = q.c0[i], c1 = q.c1[i];
    const uint64_t k0 = ov_key(s, c0), k1 = ov_key(s, c1);
    uint64_t a = ix.seg_in[s], b = ix.seg_in[s + 1];
    if (a < b) {
      hit = lower_bound(ix.in_s, a, b, k0) > upper_bound(ix.in_e, a, b, k0);
      if (!hit) hit = lower_bound(ix.in_s, a, b, k1) > upper_bound(ix.in_e, a, b, k1);
    }
    if (!hit && c0 < c1) {
      a = ix.seg_all[s];
      b = ix.seg_all[s + 1];
      if (a < b) hit = lower_bound(ix.all_s, a, b, k1) > upper_bound(ix.all_s, a, b, k0);
    }
  }
  drop[i] = hit ? 1 : 0;
}

// the slice of cl_s whose starts lie in (lo, hi]; false: the seqid has no interval
struct OvSlice {
  uint64_t a, b, from, to;
  int64_t lo, hi;
};
__device__ inline bool ov_slice(const OvIndex& ix, const OvQuery& q, uint64_t i, OvSlice* out) {
  const uint32_t s = q.seq[i];
  if (s >= ix.n_seq) return false;
  out->a = ix.seg_cl[s];
  out->b = ix.seg_cl[s + 1];
  if (out->a >= out->b) return false;
  const int64_t c0 = q.c0[i], c1 = q.c1[i];
  out->lo = c0 < c1 ? c0 : c1;
  out->hi = c0 < c1 ? c1 : c0;
  out->from = upper_bound(ix.cl_s, out->a, out->b, ov_key(s, out->lo));
  out->to = out->lo == out->hi ? out->from
                               : upper_bound(ix.cl_s, out->from, out->b, ov_key(s, out->hi));
  return true;
}

__global__ __launch_bounds__(kOvThreads) void ov_overlap_kernel(OvIndex ix, OvQuery q,
                                                                int64_t* counts,
                                                                uint32_t* long_list,
                                                                unsigned long long* n_long) {
  const uint64_t i = (uint64_t)blockIdx.x * kOvThreads + threadIdx.x;
  if (i >= q.n) return;
  int64_t count = 0;
  OvSlice sl;
  if (ov_slice(ix, q, i, &sl)) {
    const uint64_t ended = lower_bound(ix.cl_e, sl.a, sl.b, ov_key(q.seq[i], sl.lo));
    count = (int64_t)(sl.from - sl.a) - (int64_t)(ended - sl.a);
    if (sl.to - sl.from <= kOvLaneScan) {
      for (uint64_t j = sl.from; j < sl.to; ++j) count += ix.cl_v[j] >= sl.hi;
    } else {
      long_list[atomicAdd(n_long, 1ull)] = (uint32_t)i;  // each query at most once: below q.n
    }
  }
  counts[i] = count;
}

__global__ __launch_bounds__(kOvThreads) void ov_long_kernel(OvIndex ix, OvQuery q, int64_t* counts,
                                                             const uint32_t* long_list,
                                                             const unsigned long long* n_long) {
  const uint64_t waves = (uint64_t)gridDim.x * (kOvThreads / kOvWave);
  const uint32_t lane = threadIdx.x & (kOvWave - 1);
  const uint64_t listed = *n_long;
  for (uint64_t k = (uint64_t)blockIdx.x * (kOvThreads / kOvWave) + threadIdx.x / kOvWave; k < listed;
       k += waves) {
    const uint64_t i = long_list[k];
    OvSlice sl;
    if (!ov_slice(ix, q, i, &sl)) continue;  // the same in every lane
    int64_t r = 0;
    for (uint64_t base = sl.from; base < sl.to; base += kOvWave) {
      const uint64_t j = base + lane;
      const bool in = j < sl.to && ix.cl_v[j] >= sl.hi;
      r += __popcll(__ballot(in));
    }
    if (lane == 0) counts[i] += r;
  }
}

}  // namespace

size_t ov_sort_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_keys(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                 (size_t)n, 0, 64, hipStream_t(0));
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                  (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n, 0, 64,
                                  hipStream_t(0));
  return a > b ? a : b;
}

hipError_t launch_ov_keys(const OvBuildArgs& a, hipStream_t s) {
  if (!a.n) return hipSuccess;
  ov_keys_kernel<<<blocks_for(a.n), kOvThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_ov_sort(const OvBuildArgs& a, void* tmp, size_t bytes, hipStream_t s) {
  if (!a.n) return hipSuccess;
  uint64_t* const out[5] = {a.in_s, a.in_e, a.all_s, a.cl_s, a.cl_e};
  for (int t = 0; t < 5; ++t) {
    const uint64_t* in = a.raw + (uint64_t)t * a.n;
    const hipError_t e =
        t == 3 ? rocprim::radix_sort_pairs(tmp, bytes, in, out[t], (const int64_t*)a.raw_v, a.cl_v,
                                           (size_t)a.n, 0, 64, s)
               : rocprim::radix_sort_keys(tmp, bytes, in, out[t], (size_t)a.n, 0, 64, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ov_segments(const OvBuildArgs& a, hipStream_t s) {
  ov_segment_kernel<<<blocks_for(3 * ((uint64_t)a.n_seq + 1)), kOvThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_ov_purge(const OvIndex& ix, const OvQuery& q, uint8_t* drop, hipStream_t s) {
  if (!q.n) return hipSuccess;
  ov_purge_kernel<<<blocks_for(q.n), kOvThreads, 0, s>>>(ix, q, drop);
  return hipGetLastError();
}

hipError_t launch_ov_overlap(const OvIndex& ix, const OvQuery& q, int64_t* counts,
                             uint32_t* long_list, unsigned long long* n_long, int n_cu,
                             hipStream_t s) {
  if (!q.n) return hipSuccess;
  if (hipError_t e = hipMemsetAsync(n_long, 0, sizeof *n_long, s)) return e;
  ov_overlap_kernel<<<blocks_for(q.n), kOvThreads, 0, s>>>(ix, q, counts, long_list, n_long);
  if (hipError_t e = hipGetLastError()) return e;
  // every wave of the machine takes listed queries in turn
  const uint64_t want = (q.n + (kOvThreads / kOvWave) - 1) / (kOvThreads / kOvWave);
  const uint64_t grid = std::min<uint64_t>(want, (uint64_t)(n_cu > 0 ? n_cu : 256) * 4);
  ov_long_kernel<<<(unsigned)grid, kOvThreads, 0, s>>>(ix, q, counts, long_list, n_long);
  return hipGetLastError();
}

}  // namespace magot
