// The longest six-frame ORF of every record, fused (get_CDS_peptides,
// genome_tools.py:283-321, through Sequence.get_orfs(longest=True),
// genome.py:824-851).  The records are the nucleotide output of an executed
// extraction plan, where it lies in HBM: what get_seq() returns, '-' records
// already reverse-complemented, case and non-ACGT letters kept, each record at
// any byte phase.  No stream, ORF table or losing ORF is written to memory: a
// record's bases are translated in registers, and one row per record comes
// out.
//
// Streams.  Stream j of a record of L bases has frame f = j >> 1 and strand
// '+' when j is odd (the reference's loop order, 0-, 0+, 1-, 1+, 2-, 2+).  It
// has c = (L - 2f) / 3 codons when L >= 2f + 3, else none; codon i covers
// bases [2f + 3i, 2f + 3i + 3) of the record ('+') or of its reverse
// complement ('-'): the definition above magot_orf6_sizes.  A residue is
// lut[codon], 'X' when a base is not one of ACGTacgt.  A frame-0 stream whose
// residue 0 is 'X' loses it (trimX), and residue indices count from the
// trimmed start.  A None or empty stream has no run and is passed over, as
// get_orfs passes it over.
//
// The winner.  Among the maximal runs of residues other than '*', the first in
// order (j, then start k) whose length is the maximum; a record whose maximum
// is 0 is flagged kOrfFlagNoLongest (the reference's IndexError).
//
// Calling pass: one wave per record, striding over the records.  Per stream,
// steps of kLongOrfStep codons, a lane per codon.  The stops of a step are a
// ballot mask; a stop lane gets the run that ends at it from the mask below
// it, or, without a stop below it, from the run carried into the step.
// Carried across steps (wave-uniform): the open run's first codon and its
// length so far.  Carried across streams: the best (length, j, k) so far.
// Streams and steps are visited in ascending (j, k), so only a strictly longer
// run replaces the best, and inside a step the lowest lane of the longest run
// is taken: "first seen wins" is the reference's tie rule.
//
// Writing pass, behind a scan of the winners' lengths: one wave per record
// translates the winner again, a lane per residue, into the concatenated
// payload or into the tool's text '>' name '\n' residues '\n'.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr uint32_t kWavesPerBlock = 4;
static_assert(kLongOrfStep == 64, "one codon per lane, the stops as one ballot mask");

// A/a 0, C/c 1, G/g 2, T/t 3, anything else 4
__device__ __forceinline__ uint32_t base_code(uint32_t b) {
  const uint32_t l = b | 0x20u;
  return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}

// residue i of stream j of the L bases at rec (i inside the stream: the three
// bases lie inside the record)
__device__ __forceinline__ uint32_t residue(const uint8_t* __restrict__ rec, uint32_t L, uint32_t j,
                                            uint32_t i, const uint8_t* lut) {
  const uint32_t q = 2u * (j >> 1) + 3u * i;
  uint32_t c0, c1, c2;
  if (j & 1u) {
    c0 = base_code(rec[q]);
    c1 = base_code(rec[q + 1]);
    c2 = base_code(rec[q + 2]);
    if ((c0 | c1 | c2) & 4u) return 'X';
  } else {
    const uint32_t e = L - 1u - q;
    c0 = base_code(rec[e]);
    c1 = base_code(rec[e - 1]);
    c2 = base_code(rec[e - 2]);
    if ((c0 | c1 | c2) & 4u) return 'X';
    c0 = 3u - c0, c1 = 3u - c1, c2 = 3u - c2;
  }
  return lut[c0 | c1 << 2 | c2 << 4];
}

__device__ __forceinline__ uint32_t stream_codons(uint32_t L, uint32_t j) {
  const uint32_t f = j >> 1;
  return L >= 2u * f + 3u ? (L - 2u * f) / 3u : 0u;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ void stage_lut(const LongOrfArgs& a, uint8_t* lut) {
  if (threadIdx.x < 64) lut[threadIdx.x] = a.lut[threadIdx.x];
  __syncthreads();
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void longorf_call_kernel(LongOrfArgs a) {
  __shared__ uint8_t lut[64];
  stage_lut(a, lut);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock +
                        (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  for (uint64_t r = wave; r < a.n; r += a.waves) {
    const uint32_t L = (uint32_t)(a.noff[r + 1] - a.noff[r]);
    const uint8_t* const rec = a.nuc + a.start[r];
    uint32_t best_len = 0, best_j = 0, best_k = 0, best_ku = 0;  // wave-uniform
    for (uint32_t j = 0; j < 6; ++j) {
      const uint32_t c = stream_codons(L, j);
      uint32_t trim = 0, run_start = 0, run_len = 0;  // the open run: its first codon, its length
      for (uint32_t i0 = 0; i0 < c; i0 += kLongOrfStep) {
        const uint32_t i = i0 + lane;
        bool valid = i < c;
        const uint32_t res = valid ? residue(rec, L, j, i, lut) : 0u;
        if (i0 == 0 && j < 2) {  // trimX: a frame-0 stream loses a leading 'X'
          trim = (uint32_t)(__ballot(valid && lane == 0 && res == 'X') & 1ull);
          if (trim && lane == 0) valid = false;
          run_start = trim;
        }
        const uint32_t lo = i0 == 0 ? trim : 0u;  // the valid lanes are [lo, lo + nv)
        const uint32_t nv = (uint32_t)__popcll(__ballot(valid));
        const bool stop = valid && res == '*';
        const uint64_t sm = __ballot(stop);
        if (sm == 0) {
          run_len += nv;
          continue;
        }
        uint32_t st = 0, len = 0;  // the run that ends at this stop lane
        if (stop) {
          const uint64_t below = sm & ((1ull << lane) - 1ull);
          if (below) {
            const uint32_t p = 63u - (uint32_t)__clzll((long long)below);
            st = i0 + p + 1u;
            len = lane - p - 1u;
          } else {
            st = run_start;
            len = run_len + (lane - lo);
          }
        }
        if (__ballot(len > best_len)) {
          const uint32_t m = wave_max(len);
          const uint32_t first = (uint32_t)__ffsll((long long)__ballot(stop && len == m)) - 1u;
          best_len = m;
          best_j = j;
          best_ku = (uint32_t)__builtin_amdgcn_readlane((int)st, (int)first);
          best_k = best_ku - trim;
        }
        const uint32_t last = 63u - (uint32_t)__clzll((long long)sm);
        run_start = i0 + last + 1u;
        run_len = lo + nv - 1u - last;
      }
      if (run_len > best_len) {  // the run the stream's end closes
        best_len = run_len;
        best_j = j;
        best_ku = run_start;
        best_k = run_start - trim;
      }
    }
    if (lane == 0) {
      a.j[r] = (uint8_t)best_j;
      a.k[r] = best_k;
      a.ku[r] = best_ku;
      a.len[r] = best_len;
      a.flags[r] = best_len ? 0 : kOrfFlagNoLongest;
    }
  }
}

__global__ void longorf_tlen_kernel(LongOrfArgs a, LongOrfTextArgs t) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= t.n_print) return;
  t.tlen[r] = (uint32_t)(t.name_off[r + 1] - t.name_off[r]) + a.len[r] + 3u;
}

// TEXT: '>' name '\n' residues '\n' of records [0, n_print); else the payload
template <bool TEXT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void longorf_write_kernel(LongOrfArgs a,
                                                                          LongOrfTextArgs t) {
  __shared__ uint8_t lut[64];
  stage_lut(a, lut);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock +
                        (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint64_t n = TEXT ? t.n_print : a.n;
  for (uint64_t r = wave; r < n; r += a.waves) {
    const uint32_t L = (uint32_t)(a.noff[r + 1] - a.noff[r]);
    const uint8_t* const rec = a.nuc + a.start[r];
    const uint32_t len = a.len[r], j = a.j[r], ku = a.ku[r];
    uint8_t* dst;
    if (TEXT) {
      const uint64_t n0 = t.name_off[r];
      const uint32_t nl = (uint32_t)(t.name_off[r + 1] - n0);
      uint8_t* const e = t.out + t.tstart[r];
      for (uint32_t x = lane; x < nl; x += 64) e[1 + x] = t.names[n0 + x];
      dst = e + nl + 2;
      if (lane == 0) {
        e[0] = '>';
        e[1 + nl] = '\n';
        dst[len] = '\n';
      }
    } else {
      dst = a.payload + a.poff[r];
    }
    for (uint32_t x = lane; x < len; x += 64) dst[x] = (uint8_t)residue(rec, L, j, ku + x, lut);
  }
}

hipError_t scan_u32(void* tmp, size_t bytes, const uint32_t* in, uint64_t* out, uint64_t n,
                    hipStream_t s) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, uint64_t(0), (size_t)n,
                                 rocprim::plus<uint64_t>(), s);
}

}  // namespace

size_t longorf_scan_bytes(uint64_t n) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t*)nullptr, (uint64_t*)nullptr,
                                uint64_t(0), (size_t)n, rocprim::plus<uint64_t>(),
                                hipStream_t(0));
  return bytes;
}

hipError_t launch_longorf_call(const LongOrfArgs& a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.len + a.n, 0, 4, s)) return e;
  if (a.n) longorf_call_kernel<<<a.waves / kWavesPerBlock, 64 * kWavesPerBlock, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return scan_u32(a.scan_tmp, a.scan_bytes, a.len, a.poff, a.n + 1, s);
}

hipError_t launch_longorf_write(const LongOrfArgs& a, hipStream_t s) {
  if (a.n)
    longorf_write_kernel<false>
        <<<a.waves / kWavesPerBlock, 64 * kWavesPerBlock, 0, s>>>(a, LongOrfTextArgs{});
  return hipGetLastError();
}

hipError_t launch_longorf_text_sizes(const LongOrfArgs& a, const LongOrfTextArgs& t,
                                     hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(t.tlen + t.n_print, 0, 4, s)) return e;
  if (t.n_print)
    longorf_tlen_kernel<<<(unsigned)((t.n_print + 255) / 256), 256, 0, s>>>(a, t);
  if (hipError_t e = hipGetLastError()) return e;
  return scan_u32(t.scan_tmp, t.scan_bytes, t.tlen, t.tstart, t.n_print + 1, s);
}

hipError_t launch_longorf_text_write(const LongOrfArgs& a, const LongOrfTextArgs& t,
                                     hipStream_t s) {
  if (t.n_print)
    longorf_write_kernel<true><<<a.waves / kWavesPerBlock, 64 * kWavesPerBlock, 0, s>>>(a, t);
  return hipGetLastError();
}

}  // namespace magot
