// Column cuts of a resident text on the device: tab2fasta
// (magot_smallfuncs.py:12-18) and repeatmasker2augustushints
// (genome_tools.py:449-454).  For every line a few leading fields are taken by
// their TAB positions and written out with literals between them (common.h:
// TcArgs); a line with too few TABs is skipped or reported.
//
//   the indexes     textindex.hip's count over the LFs with the TABs counted
//                   beside them; its fill in line mode gives the line starts,
//                   its fill in plain mode over the TABs' own block counts the
//                   offset of every TAB.
//   rows_kernel     one lane per line.  A lower bound of the line's start in
//                   the TAB offsets (searched among the TABs of the start's text
//                   block, which the block scan brackets) names its first TAB;
//                   the next `need`
//                   entries, and one more for field `need`, are the line's while
//                   they lie below its end.  The lane writes the verdict, the
//                   bytes the line prints and its pieces of kTcPiece bytes; a
//                   short line of error mode atomic-mins (line << 8 | reason).
//                   It reads the line's last two bytes and nothing else of the
//                   text: O(log n_tabs + items) per line, whatever its length
//                   and however many TABs it has.
//   the layout      two scans: the lines' output offsets and piece numbers.
//   pieces_kernel   one lane per piece, so a field of 40 Mb is 10,000 lanes'
//                   work and not one's.  A search in the piece scan names the
//                   line, a walk over the items the item and the offset in it:
//                   source (a literal lies behind the text, so it is an offset
//                   from `text` too), destination, length.
//   the copy        wavecopy.h's launch_piece_copy, as the renamed text's.
//
// LDS: the copy's piece table.  No spin-wait, no compare-and-swap; the atomics
// are the status word's minimum and the kept lines' count.
#include <hip/hip_runtime.h>

#include "common.h"
#include "wavecopy.h"

namespace magot {
namespace {

constexpr int kTcThreads = 256;

inline unsigned tc_blocks_for(uint64_t n) { return (unsigned)((n + kTcThreads - 1) / kTcThreads); }

// What the items of a kept line are cut from.
struct TcLine {
  uint64_t start;  // the line's first byte
  uint64_t end;    // its end less the LF and less one CR before it
  uint64_t t0;     // its first TAB in tx.pos
  bool extra;      // it has a TAB behind its first `need`
};

// the first j in [0, n) with v[j] >= x, n where there is none (v increasing)
__device__ __forceinline__ uint64_t tc_lower_bound(const uint64_t* __restrict__ v, uint64_t n,
                                                   uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Line k (below n_lines) from its two ends and the TAB at t0; false when it has
// fewer than `need` TABs.
__device__ __forceinline__ bool tc_line(const TcArgs& a, uint64_t k, uint64_t t0, TcLine* L) {
  const uint64_t s = a.ix.pos[k], e = a.ix.pos[k + 1];  // s < e <= n
  uint64_t end = e;
  if (end > s && a.ix.text[end - 1] == '\n') --end;
  if (end > s && a.ix.text[end - 1] == '\r') --end;
  L->start = s;
  L->end = end;
  L->t0 = t0;
  // TAB t0 + i is the line's while it exists and lies below e; the TABs before it do then too
  const uint64_t last = t0 + a.need;  // the TAB behind the first `need`
  L->extra = last < a.n_tabs && a.tx.pos[last] < e;
  return !a.need || (last - 1 < a.n_tabs && a.tx.pos[last - 1] < e);
}

// an item's source (from `text`) and length on a kept line
__device__ __forceinline__ void tc_span(const TcArgs& a, const TcLine& L, const TcItem& it,
                                        uint64_t* src, uint64_t* len) {
  if (it.kind == kTcLiteral) {
    *src = a.lit_base + it.a;
    *len = it.b;
    return;
  }
  // the host checked a <= b <= need: every index below is one of the line's TABs
  const uint64_t from = it.a ? a.tx.pos[L.t0 + it.a - 1] + 1 : L.start;
  const uint64_t to = it.b < a.need ? a.tx.pos[L.t0 + it.b]
                      : L.extra     ? a.tx.pos[L.t0 + a.need]
                                    : L.end;  // at or behind the line's last TAB + 1
  *src = from;
  *len = to - from;
}

__device__ __forceinline__ uint64_t tc_pieces_of(uint64_t len) {
  return (len + kTcPiece - 1) / kTcPiece;
}

__global__ __launch_bounds__(kTcThreads) void tc_rows_kernel(TcArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kTcThreads + threadIdx.x;
  if (k > a.ix.n_lines) return;
  uint64_t olen = 0, pcnt = 0, t0 = a.n_tabs;
  uint32_t verdict = kTcSkipped;
  if (k < a.ix.n_lines) {
    // the TABs before the text block of the line's start lie before it, those behind the
    // block behind it: the bound is searched among the block's own (tx.pre: n_blocks + 1)
    const uint64_t s = a.ix.pos[k], blk = s / kTextBlock;  // s < n: blk < n_blocks
    const uint64_t lo = a.tx.pre[blk], hi = a.tx.pre[blk + 1];
    t0 = lo + tc_lower_bound(a.tx.pos + lo, hi - lo, s);
    TcLine L;
    if (tc_line(a, k, t0, &L)) {
      verdict = kTcKept;
#pragma unroll
      for (uint32_t i = 0; i < kTcMaxItems; ++i)
        if (i < a.n_items) {
          uint64_t src, len;
          tc_span(a, L, a.items[i], &src, &len);
          olen += len;
          pcnt += tc_pieces_of(len);
        }
      atomicAdd(a.n_kept, 1ull);
    } else if (a.short_mode == kTcShortError) {
      verdict = kTcShort;
      atomicMin(a.status + 1, (unsigned long long)(k << 8 | kTcShortLine));
    }
  }
  a.verdict[k] = (uint8_t)verdict;
  a.tab0[k] = t0;
  a.olen[k] = olen;
  a.pcnt[k] = pcnt;
}

// the last i in [lo, hi) with v[i] <= x (v non-decreasing, v[lo] <= x)
__device__ __forceinline__ uint64_t tc_last_le(const uint64_t* __restrict__ v, uint64_t lo,
                                               uint64_t hi, uint64_t x) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kTcThreads) void tc_pieces_kernel(TcArgs a, TcRenderArgs o) {
  const uint64_t t = (uint64_t)blockIdx.x * kTcThreads + threadIdx.x;
  if (t >= o.n_pieces) return;
  // pbase[0] = 0 <= t < pbase[n_lines]; a line without a piece shares its successor's entry,
  // so k is a kept line with pbase[k] <= t < pbase[k + 1]
  const uint64_t k = tc_last_le(a.pbase, 0, a.ix.n_lines, t);
  uint64_t q = t - a.pbase[k];
  TcLine L;
  (void)tc_line(a, k, a.tab0[k], &L);
  uint64_t dst = a.obase[k];
  uint64_t p_src = 0, p_dst = 0;
  uint32_t p_len = 0;
  bool found = false;
#pragma unroll
  for (uint32_t i = 0; i < kTcMaxItems; ++i)
    if (i < a.n_items && !found) {
      uint64_t src, len;
      tc_span(a, L, a.items[i], &src, &len);
      const uint64_t np = tc_pieces_of(len);
      if (q < np) {
        const uint64_t at = q * kTcPiece, left = len - at;
        p_src = src + at;
        p_dst = dst + at;
        p_len = (uint32_t)(left < kTcPiece ? left : kTcPiece);
        found = true;
      } else {
        q -= np;
        dst += len;
      }
    }
  // found: q was below the line's pieces.  A piece of no bytes copies nothing.
  o.p_src[t] = p_src;
  o.p_dst[t] = p_dst;
  o.p_len[t] = p_len;
}

}  // namespace

hipError_t launch_tc_rows(const TcArgs& a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.status + 1, 0xff, sizeof(unsigned long long), s)) return e;
  if (hipError_t e = hipMemsetAsync(a.n_kept, 0, sizeof(unsigned long long), s)) return e;
  tc_rows_kernel<<<tc_blocks_for(a.ix.n_lines + 1), kTcThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_tc_layout(const TcArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (hipError_t e = exclusive_sum(tmp, tmp_bytes, a.olen, a.obase, a.ix.n_lines + 1, s)) return e;
  return exclusive_sum(tmp, tmp_bytes, a.pcnt, a.pbase, a.ix.n_lines + 1, s);
}

hipError_t launch_tc_pieces(const TcArgs& a, const TcRenderArgs& r, hipStream_t s) {
  if (!r.n_pieces) return hipSuccess;
  tc_pieces_kernel<<<tc_blocks_for(r.n_pieces), kTcThreads, 0, s>>>(a, r);
  return hipGetLastError();
}

hipError_t launch_tc_copy(const TcArgs& a, const TcRenderArgs& r, hipStream_t s) {
  if (!r.n_pieces) return hipSuccess;
  return launch_piece_copy<kTcGroup>(r.p_src, r.p_dst, r.p_len, r.n_pieces, a.ix.text, r.out, s);
}

}  // namespace magot
