// mask_from_gff on the device (genome_tools.py:394-428): two HBM-bound passes
// over the bytes of a whole-contig extraction (every contig gathered whole by
// extract_kernel, which reproduces every input byte).
//
//   mask_paint_kernel  one lane per interval piece (at most kMaskPiece bases,
//                      maskplan.cpp) sets the piece's bits in a coverage plane
//                      of one bit per source byte, zeroed before the launch.
//   mask_text_kernel   one lane per 16-byte chunk of the final text: the
//                      chunks inside a contig's body load their 16 source
//                      bytes (a funnel-shifted pair of aligned loads: the
//                      headers shift the body, so source and text are at
//                      different 16-byte phases), fetch their 16 coverage
//                      bits, change case or write 'N' with 32-bit SWAR
//                      arithmetic and store once; the chunks that hold a
//                      header, a contig's closing '\n' or a body's first or
//                      last bytes go byte by byte.  The chunks partition the
//                      text, so every byte is written exactly once.  A wave
//                      finds the records of its 4 KB range and reads their
//                      places once, on wave-uniform (scalar) values: with a
//                      lookup per lane the pass took 1.6x as long (C3).
//
// Neither kernel needs a workgroup barrier or LDS.
#include <hip/hip_runtime.h>

#include "common.h"
#include "wavecopy.h"

namespace magot {
namespace {

constexpr int kMaskThreads = 256;
constexpr int kMaskUnroll = 4;  // text chunks per lane, their loads in flight together

// The intervals come unsorted and may overlap, nest or repeat.  A piece's
// first and last words are partial and are set with atomicOr; its interior
// words are covered whole and get plain 32-bit stores of all-ones.  The two
// may meet on one word (an interior word of one piece is an edge word of
// another), in either order, without any ordering between them: the store
// writes all-ones, the atomicOr can only add bits, so the word ends as
// all-ones whichever lands last -- and all-ones is right, since the piece that
// stored it covers the whole word.  Two plain stores write the same value.
// A 32-bit store is a single access, so there is no torn word to see.
__global__ __launch_bounds__(kMaskThreads) void mask_paint_kernel(
    const magot_mask_interval* __restrict__ rows, uint64_t n_rows,
    const uint64_t* __restrict__ contig_src, uint32_t* __restrict__ cov, uint64_t n_bits) {
  const uint64_t i = (uint64_t)blockIdx.x * kMaskThreads + threadIdx.x;
  if (i >= n_rows) return;
  const magot_mask_interval iv = rows[i];
  if (!iv.len) return;
  const uint64_t b = contig_src[iv.contig] + iv.start;
  const uint64_t e = b + iv.len - 1;  // last bit
  if (e >= n_bits) return;             // the host checked every piece: never taken
  const uint64_t fw = b >> 5, lw = e >> 5;
  const uint32_t head = ~0u << (b & 31), tail = ~0u >> (31 - (e & 31));
  if (fw == lw) {
    atomicOr(cov + fw, head & tail);
    return;
  }
  atomicOr(cov + fw, head);
  for (uint64_t w = fw + 1; w < lw; ++w) cov[w] = ~0u;
  atomicOr(cov + lw, tail);
}

// number of records whose text starts at or before x, minus one: the record
// that holds text byte x (x < tstart[n]); searched in [lo, hi]
__device__ __forceinline__ uint64_t record_of(const uint64_t* __restrict__ tstart, uint64_t lo,
                                              uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (tstart[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// 0x80 in every byte of x that lies in [lo, hi] (ASCII bounds), 0 elsewhere;
// no carry crosses a byte: the low 7 bits are compared, the top bit excluded
__device__ __forceinline__ uint32_t swar_in_range(uint32_t x, uint32_t lo, uint32_t hi) {
  const uint32_t l7 = x & 0x7f7f7f7fu;
  const uint32_t ge = l7 + (0x80u - lo) * 0x01010101u;        // bit 7: byte >= lo
  const uint32_t gt = l7 + (0x80u - (hi + 1)) * 0x01010101u;  // bit 7: byte > hi
  return ge & ~gt & ~x & 0x80808080u;
}

// the reference's order: upper() of the whole line first (unless the case is
// kept), then the feature's lower() or 'N' on the covered bytes; m has 0xff
// in every covered byte
__device__ __forceinline__ uint32_t mask_word(uint32_t x, uint32_t m, uint32_t flags) {
  if (!(flags & MAGOT_MASK_KEEP_CASE)) x ^= swar_in_range(x, 'a', 'z') >> 2;
  if (flags & MAGOT_MASK_HARD) return (x & ~m) | (0x4e4e4e4eu & m);
  return x ^ ((swar_in_range(x, 'A', 'Z') & m) >> 2);
}

// bits 0..3 of n spread to 0xff / 0x00 in bytes 0..3
__device__ __forceinline__ uint32_t spread4(uint32_t n) {
  return (((n & 15u) * 0x00204081u) & 0x01010101u) * 0xffu;
}

__device__ __forceinline__ uint8_t mask_byte(uint8_t c, bool covered, uint32_t flags) {
  if (!(flags & MAGOT_MASK_KEEP_CASE) && c >= 'a' && c <= 'z') c -= 32;
  if (!covered) return c;
  if (flags & MAGOT_MASK_HARD) return 'N';
  return c >= 'A' && c <= 'Z' ? c + 32 : c;
}

__global__ __launch_bounds__(kMaskThreads) void mask_text_kernel(MaskArgs a) {
  const uint64_t n_chunks = (a.text_bytes + 15) >> 4;
  // the wave's kMaskUnroll * 64 consecutive chunks
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t wave = (uint64_t)blockIdx.x * (kMaskThreads / 64) + wv;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t c0 = wave * (64 * kMaskUnroll);
  if (c0 >= n_chunks) return;
  // the records the wave's range touches: one search pair per wave, on
  // wave-uniform values (scalar loads)
  const uint64_t last_byte = min((c0 + 64 * kMaskUnroll) << 4, a.text_bytes) - 1;
  const uint64_t r_lo = record_of(a.tstart, 0, a.n_rec - 1, c0 << 4);
  const uint64_t r_hi = record_of(a.tstart, r_lo, a.n_rec - 1, last_byte);
  // nearly every wave lies inside one record: its places are read once
  const bool one = r_lo == r_hi;
  const uint64_t u_body = a.tstart[r_lo] + a.hlen[r_lo];
  const uint64_t u_end = a.tstart[r_lo + 1] - 1;
  const uint64_t u_src = a.rsrc[r_lo];

  uint4 lo[kMaskUnroll], hi[kMaskUnroll];
  uint32_t w0[kMaskUnroll], w1[kMaskUnroll], sh[kMaskUnroll];
  uint64_t S[kMaskUnroll], rec[kMaskUnroll];
  bool fast[kMaskUnroll];
#pragma unroll
  for (int j = 0; j < kMaskUnroll; ++j) {
    const uint64_t C = (c0 + lane + 64ull * j) << 4;
    fast[j] = false;
    rec[j] = r_lo;
    if (C >= a.text_bytes) continue;
    // the body's first text byte, its closing '\n', its first source byte
    uint64_t body = u_body, body_end = u_end, rs = u_src;
    if (!one) {
      const uint64_t r = record_of(a.tstart, r_lo, r_hi, C);
      rec[j] = r;
      body = a.tstart[r] + a.hlen[r];
      body_end = a.tstart[r + 1] - 1;
      rs = a.rsrc[r];
    }
    if (C >= body && C + 16 <= body_end) {
      fast[j] = true;
      S[j] = rs + (C - body);
      sh[j] = (uint32_t)(S[j] & 15);
      const uint8_t* sb = a.src + (S[j] & ~15ull);
      lo[j] = *reinterpret_cast<const uint4*>(sb);
      hi[j] = sh[j] ? *reinterpret_cast<const uint4*>(sb + 16) : lo[j];
      w0[j] = a.cov[S[j] >> 5];
      w1[j] = a.cov[(S[j] >> 5) + 1];  // the plane has one word of slack
    }
  }
#pragma unroll
  for (int j = 0; j < kMaskUnroll; ++j) {
    const uint64_t C = (c0 + lane + 64ull * j) << 4;
    if (C >= a.text_bytes) continue;
    if (fast[j]) {
      const uint4 v = funnel16_lane(lo[j], hi[j], sh[j]);
      const uint32_t bits = (uint32_t)((((uint64_t)w1[j] << 32) | w0[j]) >> (S[j] & 31));
      uint4 o;
      o.x = mask_word(v.x, spread4(bits), a.flags);
      o.y = mask_word(v.y, spread4(bits >> 4), a.flags);
      o.z = mask_word(v.z, spread4(bits >> 8), a.flags);
      o.w = mask_word(v.w, spread4(bits >> 12), a.flags);
      *reinterpret_cast<uint4*>(a.out + C) = o;
      continue;
    }
    // a chunk with header bytes, a closing '\n' or a body's edge: byte by byte
    uint64_t r = rec[j];
    const uint64_t end = min(C + 16, a.text_bytes);
    for (uint64_t x = C; x < end; ++x) {
      while (a.tstart[r + 1] <= x) ++r;
      const uint64_t o = x - a.tstart[r], hl = a.hlen[r];
      uint8_t c;
      if (o < hl) {
        c = a.hdr[a.hoff[r] + o];
      } else if (x + 1 == a.tstart[r + 1]) {
        c = '\n';
      } else {
        const uint64_t s = a.rsrc[r] + (o - hl);
        c = mask_byte(a.src[s], (a.cov[s >> 5] >> (s & 31)) & 1u, a.flags);
      }
      a.out[x] = c;
    }
  }
}

}  // namespace

hipError_t launch_mask_paint_rows(const magot_mask_interval* rows, uint64_t n_rows,
                                  const uint64_t* contig_src, uint32_t* cov, uint64_t n_bits,
                                  hipStream_t s) {
  if (!n_rows) return hipSuccess;
  const uint64_t blocks = (n_rows + kMaskThreads - 1) / kMaskThreads;
  mask_paint_kernel<<<(unsigned)blocks, kMaskThreads, 0, s>>>(rows, n_rows, contig_src, cov,
                                                               n_bits);
  return hipGetLastError();
}

hipError_t launch_mask_paint(const MaskArgs& a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.cov, 0, (a.cov_words + 1) * 4, s)) return e;
  return launch_mask_paint_rows(a.rows, a.n_rows, a.contig_src, a.cov, a.src_bytes, s);
}

hipError_t launch_mask_text(const MaskArgs& a, hipStream_t s) {
  if (!a.text_bytes || !a.n_rec) return hipSuccess;
  const uint64_t n_chunks = (a.text_bytes + 15) >> 4;
  const uint64_t per_block = (uint64_t)kMaskThreads * kMaskUnroll;
  const uint64_t blocks = (n_chunks + per_block - 1) / per_block;
  mask_text_kernel<<<(unsigned)blocks, kMaskThreads, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace magot
