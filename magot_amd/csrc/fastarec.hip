// exclude_from_fasta and fasta2tab on the device (genome_tools.py:377-391,
// magot_smallfuncs.py:21-29; genome.py:854-877 for the records): the records of
// a resident FASTA text, a dict of them keyed by name, an anti-join against a
// list of names, and the text reflowed into one line per record.  A header line
// is short; a sequence line may be a whole chromosome, so no pass walks one.
//
//   the line index  textindex.hip's count and fill over the LFs, line mode with the
//                   stray-CR check: the total gives n_lines on the host, ix.pos[k]
//                   is where line k starts, and a CR that is neither before an LF
//                   nor the text's last byte atomic-mins (line, stray_cr) into the
//                   status word.
//   lines_kernel    one lane per line, O(1) bytes: the first byte (header or not),
//                   the byte before the LF (a CR or not).  payload = the line less
//                   its LF and that CR, 0 for a header; pieces = ceil(payload /
//                   kFaPiece).  Three exclusive scans: the headers before a line
//                   (its record), the payload before it, the pieces before it.
//   heads_kernel    the line of each header, compacted by the first scan.
//   names_kernel    one lane per header: the name span, CPython 2.7's string hash
//                   of it, the first word's span and hash (Python 2's str.split
//                   whitespace), a flag where there is no word, the record's
//                   sequence length as a difference of the payload scan.  The loop
//                   is bounded by kFaMaxName; a longer name atomic-mins (line,
//                   long_name).  Then a scan of "sequence not empty".
//   scatter_kernel  the records with a sequence, in file order: (masked hash,
//                   record).  A stable rocprim radix sort by the masked hash.
//   runs_kernel     one lane per sorted element: a run head keeps its position;
//                   any other is verified against its predecessor, length then
//                   bytes, as psl.hip's verify_kernel: a difference atomic-mins
//                   (line, hash_collision).  A running maximum gives every element
//                   its run's head.
//   ends_kernel     one lane per run end: the run's first record (stable sort: the
//                   first in the file) is marked, with the run's last record.  A
//                   scan of the marks numbers the keys in first-seen order;
//   rows_kernel     writes one row per key there: hash, first and last record.
//   Membership (magot_fastarec_exclude): list_kernel hashes the names of the list,
//                   one lane each, bounded by kFaMaxName (a longer one equals no
//                   key); a radix sort by the masked hash; member_kernel, one lane
//                   per key: a lower bound, then length and bytes against every
//                   entry of the run of equal masked hashes.
//   Reflow (magot_fastarec_render): size_kernel gives each printed record its
//                   bytes and its pieces (1 for the name, then the difference of
//                   the piece scan), two scans place them; piece_kernel, one lane
//                   per piece: two binary searches name its record and its line,
//                   the payload scan its destination; the lane of a name piece
//                   also stores the record's literal bytes ('>', TAB, LF).
//                   wavecopy.h's launch_piece_copy: one wave per kFaGroup pieces,
//                   its lanes dealt over the group's whole 16-byte chunks (a
//                   funnel-shifted pair of aligned loads, one vector store) and
//                   then over its remaining bytes.  Every output byte is written
//                   exactly once.
//
// No LDS beyond the copy's piece table, no spin-wait, no compare-and-swap loop;
// nothing is float.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "common.h"
#include "wavecopy.h"

namespace magot {
namespace {

constexpr int kFaThreads = 256;

inline unsigned fa_blocks_for(uint64_t n) { return (unsigned)((n + kFaThreads - 1) / kFaThreads); }

// the end of line k's bytes, its LF and a CR before it left out (start < end)
__device__ __forceinline__ uint64_t fa_line_end(const uint8_t* __restrict__ text, uint64_t start,
                                                uint64_t end) {
  uint64_t e = end - (text[end - 1] == '\n' ? 1 : 0);
  if (e > start && text[e - 1] == '\r') --e;
  return e;
}

__global__ __launch_bounds__(kFaThreads) void fa_lines_kernel(FaArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (k > a.ix.n_lines) return;
  uint64_t hdr = 0, pay = 0;
  if (k < a.ix.n_lines) {
    const uint64_t start = a.ix.pos[k], end = a.ix.pos[k + 1];  // start < end <= n
    hdr = a.ix.text[start] == '>' ? 1 : 0;
    if (!hdr) pay = fa_line_end(a.ix.text, start, end) - start;
  }
  a.hdr[k] = hdr;
  a.pay[k] = pay;
  a.pcs[k] = (pay + kFaPiece - 1) / kFaPiece;
}

__global__ __launch_bounds__(kFaThreads) void fa_heads_kernel(FaArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (k > a.ix.n_lines) return;
  if (k == a.ix.n_lines) a.hdr_line[a.n_rec] = (uint32_t)k;
  else if (a.hdr[k]) a.hdr_line[a.rec_of[k]] = (uint32_t)k;  // rec_of[k] < n_rec: a header's own
}

__device__ __forceinline__ bool fa_py2_space(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }

__global__ __launch_bounds__(kFaThreads) void fa_names_kernel(FaArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (r > a.n_rec) return;
  if (r == a.n_rec) {  // the scan's last entry: the records with a sequence
    a.ne[r] = 0;
    return;
  }
  const uint64_t k = a.hdr_line[r];  // below n_lines
  const uint64_t start = a.ix.pos[k];
  const uint64_t off = start + 1;    // behind the '>'
  const uint64_t full = fa_line_end(a.ix.text, start, a.ix.pos[k + 1]) - off;
  if (full > kFaMaxName)
    atomicMin(a.status, (unsigned long long)(k << 8 | MAGOT_FASTAREC_LONG_NAME));
  const uint32_t len = (uint32_t)(full > kFaMaxName ? kFaMaxName : full);
  uint64_t h = 0, wh = 0, woff = off;
  uint32_t wlen = 0, state = 0;  // 0: before the first word, 1: in it, 2: behind it
  for (uint32_t i = 0; i < len; ++i) {
    const uint32_t c = a.ix.text[off + i];
    h = py27_hash_step(h, i, c);
    const bool ws = fa_py2_space(c);
    if (state == 0 && !ws) {
      state = 1;
      woff = off + i;
    }
    if (state == 1) {
      if (ws) state = 2;
      else wh = py27_hash_step(wh, wlen++, c);
    }
  }
  const uint64_t seq = a.pay_pre[a.hdr_line[r + 1]] - a.pay_pre[k];
  a.name_off[r] = off;
  a.name_len[r] = len;
  a.hash[r] = py27_hash_end(h, len);
  a.word_off[r] = woff;
  a.word_len[r] = wlen;
  a.word_hash[r] = py27_hash_end(wh, wlen);
  a.no_word[r] = state == 0 ? 1u : 0u;
  a.seq_len[r] = seq;
  a.ne[r] = seq ? 1 : 0;
}

__device__ __forceinline__ uint64_t fa_mask(uint32_t bits) {
  return bits >= 64 ? ~0ull : (1ull << bits) - 1;
}

__global__ __launch_bounds__(kFaThreads) void fa_scatter_kernel(FaArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (r >= a.n_rec || !a.ne[r]) return;
  const uint64_t d = a.ne_pos[r];  // below n_ne
  a.skey[d] = a.hash[r] & fa_mask(a.hash_bits);
  a.sval[d] = (uint32_t)r;
}

__device__ __forceinline__ bool fa_same(const uint8_t* __restrict__ x, uint64_t xl,
                                        const uint8_t* __restrict__ y, uint64_t yl) {
  bool same = xl == yl;
  for (uint64_t j = 0; j < xl && same; ++j) same = x[j] == y[j];
  return same;
}

__global__ __launch_bounds__(kFaThreads) void fa_runs_kernel(FaArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (i >= a.n_ne) return;
  const bool head = i == 0 || a.skey_sorted[i] != a.skey_sorted[i - 1];
  a.head[i] = head ? i : 0;
  if (head) return;
  const uint32_t ra = a.sval_sorted[i], rb = a.sval_sorted[i - 1];  // records, below n_rec
  // a name's span ends inside its line, and its length is at most kFaMaxName
  if (!fa_same(a.ix.text + a.name_off[ra], a.name_len[ra], a.ix.text + a.name_off[rb], a.name_len[rb]))
    atomicMin(a.status,
              (unsigned long long)((uint64_t)a.hdr_line[ra] << 8 | MAGOT_FASTAREC_HASH_COLLISION));
}

__global__ __launch_bounds__(kFaThreads) void fa_ends_kernel(FaArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (i >= a.n_ne) return;
  if (i + 1 < a.n_ne && a.skey_sorted[i + 1] == a.skey_sorted[i]) return;
  const uint32_t first = a.sval_sorted[a.head_pos[i]];  // head_pos[i] <= i
  a.is_first[first] = 1;
  a.last_of[first] = a.sval_sorted[i];
}

__global__ __launch_bounds__(kFaThreads) void fa_rows_kernel(FaArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (r >= a.n_rec || !a.is_first[r]) return;
  const uint64_t q = a.kpos[r];  // below n_keys
  a.k_hash[q] = a.hash[r];
  a.k_first[q] = (uint32_t)r;
  a.k_last[q] = a.last_of[r];
  a.k_no_word[q] = a.no_word[r];
}

__global__ __launch_bounds__(kFaThreads) void fa_list_kernel(FaArgs a, FaMemberArgs m) {
  const uint64_t j = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (j >= m.m) return;
  const uint64_t s = m.off[j], full = m.off[j + 1] - s;  // the host checked the offsets
  const uint32_t len = (uint32_t)(full > kFaMaxName ? kFaMaxName : full);
  uint64_t h = 0;
  for (uint32_t i = 0; i < len; ++i) h = py27_hash_step(h, i, m.blob[s + i]);
  m.lkey[j] = py27_hash_end(h, len) & fa_mask(a.hash_bits);
  m.lidx[j] = (uint32_t)j;
}

__global__ __launch_bounds__(kFaThreads) void fa_member_kernel(FaArgs a, FaMemberArgs m) {
  const uint64_t q = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (q >= a.n_keys) return;
  const uint32_t r = a.k_first[q];
  const uint64_t off = m.first_word ? a.word_off[r] : a.name_off[r];
  const uint64_t len = m.first_word ? a.word_len[r] : a.name_len[r];
  const uint64_t key = (m.first_word ? a.word_hash[r] : a.hash[r]) & fa_mask(a.hash_bits);
  uint64_t lo = 0, hi = m.m;  // the first entry not below the key
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (m.lkey_sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  bool found = false;
  // an equal hash with other bytes is no match: the run is walked to its end
  for (uint64_t i = lo; i < m.m && m.lkey_sorted[i] == key && !found; ++i) {
    const uint64_t s = m.off[m.lidx_sorted[i]];
    found = fa_same(a.ix.text + off, len, m.blob + s, m.off[m.lidx_sorted[i] + 1] - s);
  }
  m.keep[q] = found ? 0 : 1;
}

__global__ __launch_bounds__(kFaThreads) void fa_size_kernel(FaArgs a, FaRenderArgs o) {
  const uint64_t j = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (j > o.n_out) return;
  uint64_t bytes = 0, pieces = 0;
  if (j < o.n_out) {
    const uint32_t r = o.recs[j];  // the host checked: below n_rec
    const uint64_t k0 = a.hdr_line[r], k1 = a.hdr_line[r + 1];
    // '>' name LF seq LF, or name TAB seq LF
    bytes = (o.style == kFaStyleFasta ? 1 : 0) + (uint64_t)a.name_len[r] + 1 + a.seq_len[r] + 1;
    pieces = 1 + a.pcs_pre[k1] - a.pcs_pre[k0];
  }
  o.olen[j] = bytes;
  o.pcnt[j] = pieces;
}

// the last i in [lo, hi) with v[i] <= x (v non-decreasing, v[lo] <= x)
__device__ __forceinline__ uint64_t fa_last_le(const uint64_t* __restrict__ v, uint64_t lo,
                                               uint64_t hi, uint64_t x) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kFaThreads) void fa_piece_kernel(FaArgs a, FaRenderArgs o) {
  const uint64_t t = (uint64_t)blockIdx.x * kFaThreads + threadIdx.x;
  if (t >= o.n_pieces) return;
  const uint64_t j = fa_last_le(o.pbase, 0, o.n_out, t);  // pbase[0] = 0 <= t < pbase[n_out]
  const uint64_t q = t - o.pbase[j];
  const uint32_t r = o.recs[j];
  const uint64_t k0 = a.hdr_line[r];
  const uint64_t lead = o.style == kFaStyleFasta ? 1 : 0;
  const uint64_t at = o.obase[j], name_len = a.name_len[r];
  if (q == 0) {  // the name, and the record's literal bytes
    if (lead) o.out[at] = '>';
    o.out[at + lead + name_len] = o.style == kFaStyleFasta ? '\n' : '\t';
    o.out[o.obase[j + 1] - 1] = '\n';
    o.p_src[t] = a.name_off[r];
    o.p_dst[t] = at + lead;
    o.p_len[t] = (uint32_t)name_len;
    return;
  }
  // piece g of the text's sequence pieces lies on the last line whose scan entry
  // is at most g: lines without a piece share their successor's entry
  const uint64_t g = a.pcs_pre[k0] + q - 1;  // below pcs_pre[hdr_line[r + 1]]
  const uint64_t k = fa_last_le(a.pcs_pre, k0, a.hdr_line[r + 1], g);
  const uint64_t in_line = (g - a.pcs_pre[k]) * kFaPiece;  // below pay[k]
  const uint64_t left = a.pay[k] - in_line;
  o.p_src[t] = a.ix.pos[k] + in_line;
  o.p_dst[t] = at + lead + name_len + 1 + (a.pay_pre[k] - a.pay_pre[k0]) + in_line;
  o.p_len[t] = (uint32_t)(left < kFaPiece ? left : kFaPiece);
}

hipError_t fa_pair_sort(void* tmp, size_t& tmp_bytes, const uint64_t* k, uint64_t* k2,
                        const uint32_t* v, uint32_t* v2, uint64_t n, uint32_t bits,
                        hipStream_t s) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, k, k2, v, v2, (size_t)n, 0, bits, s);
}

}  // namespace

size_t fa_tmp_bytes(uint64_t n) {
  size_t b = 0, c = 0;
  const size_t a = exclusive_sum_bytes<uint64_t>(n + 1);
  (void)fa_pair_sort(nullptr, b, nullptr, nullptr, nullptr, nullptr, n, 64, hipStream_t(0));
  (void)rocprim::inclusive_scan(nullptr, c, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                (size_t)n, rocprim::maximum<uint64_t>(), hipStream_t(0));
  return std::max(a, std::max(b, c));
}

hipError_t launch_fa_lines(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  fa_lines_kernel<<<fa_blocks_for(a.ix.n_lines + 1), kFaThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = exclusive_sum(tmp, tmp_bytes, a.hdr, a.rec_of, a.ix.n_lines + 1, s)) return e;
  if (hipError_t e = exclusive_sum(tmp, tmp_bytes, a.pay, a.pay_pre, a.ix.n_lines + 1, s)) return e;
  return exclusive_sum(tmp, tmp_bytes, a.pcs, a.pcs_pre, a.ix.n_lines + 1, s);
}

hipError_t launch_fa_names(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  fa_heads_kernel<<<fa_blocks_for(a.ix.n_lines + 1), kFaThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  fa_names_kernel<<<fa_blocks_for(a.n_rec + 1), kFaThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return exclusive_sum(tmp, tmp_bytes, a.ne, a.ne_pos, a.n_rec + 1, s);
}

hipError_t launch_fa_sort(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (!a.n_ne) return hipSuccess;
  fa_scatter_kernel<<<fa_blocks_for(a.n_rec), kFaThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return fa_pair_sort(tmp, tmp_bytes, a.skey, a.skey_sorted, a.sval, a.sval_sorted, a.n_ne,
                      a.hash_bits, s);
}

hipError_t launch_fa_keys(const FaArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.is_first, 0, (a.n_rec + 1) * sizeof(uint64_t), s)) return e;
  if (a.n_ne) {
    fa_runs_kernel<<<fa_blocks_for(a.n_ne), kFaThreads, 0, s>>>(a);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = rocprim::inclusive_scan(tmp, tmp_bytes, (const uint64_t*)a.head, a.head_pos,
                                               (size_t)a.n_ne, rocprim::maximum<uint64_t>(), s))
      return e;
    fa_ends_kernel<<<fa_blocks_for(a.n_ne), kFaThreads, 0, s>>>(a);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return exclusive_sum(tmp, tmp_bytes, a.is_first, a.kpos, a.n_rec + 1, s);
}

hipError_t launch_fa_rows(const FaArgs& a, hipStream_t s) {
  if (!a.n_keys) return hipSuccess;
  fa_rows_kernel<<<fa_blocks_for(a.n_rec), kFaThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_fa_member(const FaArgs& a, const FaMemberArgs& m, void* tmp, size_t tmp_bytes,
                            hipStream_t s) {
  if (!a.n_keys) return hipSuccess;
  if (m.m) {
    fa_list_kernel<<<fa_blocks_for(m.m), kFaThreads, 0, s>>>(a, m);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = fa_pair_sort(tmp, tmp_bytes, m.lkey, m.lkey_sorted, m.lidx, m.lidx_sorted,
                                    m.m, a.hash_bits, s))
      return e;
  }
  fa_member_kernel<<<fa_blocks_for(a.n_keys), kFaThreads, 0, s>>>(a, m);
  return hipGetLastError();
}

hipError_t launch_fa_render_sizes(const FaArgs& a, const FaRenderArgs& r, void* tmp,
                                  size_t tmp_bytes, hipStream_t s) {
  fa_size_kernel<<<fa_blocks_for(r.n_out + 1), kFaThreads, 0, s>>>(a, r);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = exclusive_sum(tmp, tmp_bytes, r.olen, r.obase, r.n_out + 1, s)) return e;
  return exclusive_sum(tmp, tmp_bytes, r.pcnt, r.pbase, r.n_out + 1, s);
}

hipError_t launch_fa_render(const FaArgs& a, const FaRenderArgs& r, hipStream_t s) {
  if (!r.n_pieces) return hipSuccess;
  fa_piece_kernel<<<fa_blocks_for(r.n_pieces), kFaThreads, 0, s>>>(a, r);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_piece_copy<kFaGroup>(r.p_src, r.p_dst, r.p_len, r.n_pieces, a.ix.text, r.out, s);
}

}  // namespace magot
