// heterozygosity_from_vcf on the device (magot_variants.py:16-139): the het
// calls of every sample column of a VCF, counted per locus.  The whole text is
// resident; its line index is textindex.hip's (the LFs, line mode).
//
//   classify_kernel  one lane per line, its first two bytes: blank, "##", the
//                    '#' line, or data.  One rocprim scan of the two flags packed
//                    in 64 bits places the data lines and the "##" lines.
//   cr_kernel        16 bytes a lane over the whole text: a CR anywhere declines
//                    it (read_vcf drops every CR before it splits the text).
//   parse_kernel     one wave (a workgroup of 64) per data line, every byte read
//                    once from memory: 16 bytes a lane, the tabs by byte compare,
//                    the field starts into LDS by a wave scan of the tab counts;
//                    the line's first 4 KB stay in LDS for the byte walks below.
//                    A ballot against the first bytes of the data line before
//                    says whether CHROM differs from it.  Lane 0 walks CHROM,
//                    POS and FORMAT (tens of bytes): the CPython 2.7 hash of
//                    CHROM<:>POS, POS as int32, the index of GT.  Then
//                    all 9 + S fields go into an open-addressed LDS table keyed by
//                    their bytes (a 32-bit hash picks the slot, bytes decide)
//                    that keeps the least field index per byte string: read_vcf's
//                    fields.index.  A lane per sample column looks its own bytes
//                    up, finds its GT subfield and votes; lane 0 stores the
//                    ballot's words.
//   runs             an exclusive scan of the run heads; the heads' CHROM spans
//                    for the host, which names each run's contig.
//   keys + a stable rocprim radix sort of (contig << 32 | POS, data line).
//   flags_kernel     per sorted row: the last of its key (kept: last wins), the
//                    first of its key (the dict's insertion order).
//   ranges_kernel    per locus two binary searches: its rows [b, e) of the
//                    sorted keys, and its pieces of kVcfSplit rows.
//   count_kernel     a wave per piece, lanes over the samples: the kept rows'
//                    bits added up, then one integer atomic per sample.
//
// No spin-wait; the only compare-and-swap claims an empty LDS slot and is not
// retried on the same slot; nothing is float.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdlib>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kVcfThreads = 256;
constexpr uint32_t kVcfEmpty = 0xffffffffu;
constexpr uint32_t kVcfFixed = 9;  // CHROM .. FORMAT

inline unsigned vcf_blocks_for(uint64_t n) { return (unsigned)((n + kVcfThreads - 1) / kVcfThreads); }

// read_vcf drops every CR of the text before it splits it: a text with one is
// the host path's
__global__ __launch_bounds__(kVcfThreads) void vcf_cr_kernel(VcfArgs a) {
  const uint64_t p = ((uint64_t)blockIdx.x * kVcfThreads + threadIdx.x) * 16;
  if (p >= a.n) return;
  uint32_t m = byte_eq_mask16(*reinterpret_cast<const uint4*>(a.text + p), 0x0D0D0D0Du);
  if (a.n - p < 16) m &= (1u << (a.n - p)) - 1;
  if (m) atomicMax(a.status + 4, 1ull);
}

// the line's bytes without its LF: [start, start + len)
__device__ __forceinline__ uint64_t vcf_content_len(const VcfArgs& a, uint64_t line, uint64_t* start) {
  const uint64_t s = a.line_start[line], e = a.line_start[line + 1];  // s < e <= n
  *start = s;
  // every line ends in its LF but a last line without one: no byte is read for it
  return e - s - (line + 1 < a.n_lines || a.final_lf ? 1 : 0);
}

__global__ __launch_bounds__(kVcfThreads) void vcf_classify_kernel(VcfArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (k > a.n_lines) return;
  if (k == a.n_lines) {
    a.kind[k] = 0;
    return;
  }
  uint64_t start;
  const uint64_t len = vcf_content_len(a, k, &start);
  uint64_t kind = 0;
  if (len) {
    if (a.text[start] != '#') {
      kind = 1;
    } else if (len >= 2 && a.text[start + 1] == '#') {
      kind = 1ull << 32;
    } else {
      atomicAdd(a.status + 1, 1ull);
      atomicMin(a.status + 2, (unsigned long long)k);
    }
  }
  a.kind[k] = kind;
  // the first data line: the wave's lowest lane with one speaks for it, and
  // only while the word is above its line (the word only falls: a stale read
  // sends one atomic too many, never one too few)
  const unsigned long long data = __ballot(kind == 1);
  if (kind == 1 && !(data & ((1ull << (threadIdx.x & 63)) - 1)) &&
      k < *(volatile unsigned long long*)(a.status + 3))
    atomicMin(a.status + 3, (unsigned long long)k);
}

__global__ __launch_bounds__(kVcfThreads) void vcf_compact_kernel(VcfArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (k >= a.n_lines) return;
  const uint64_t kind = a.kind[k], at = a.kpos[k];
  if (kind & 1) a.data_line[at & 0xffffffffull] = (uint32_t)k;  // below n_data
  if (kind >> 32) {  // at >> 32 is below n_hdr
    uint64_t start;
    a.hdr_len[at >> 32] = vcf_content_len(a, k, &start);
    a.hdr_off[at >> 32] = start;
  }
}

constexpr uint32_t kVcfStage = 4096;  // bytes of a line kept in LDS: four rounds of the tab pass

// the table's slots for F fields: a power of two, at least 2 F, at most kVcfTable
__host__ __device__ inline uint32_t vcf_slots(uint32_t fields) {
  uint32_t slots = 16;
  while (slots < 2 * fields) slots <<= 1;
  return slots;
}

inline size_t vcf_parse_lds(uint32_t n_samples) {
  const uint32_t fields = kVcfFixed + n_samples;
  return kVcfStage + (fields + 2 + vcf_slots(fields) + 2) * sizeof(uint32_t);
}

__device__ __forceinline__ void vcf_fail(const VcfArgs& a, uint64_t line, uint32_t reason) {
  atomicMin(a.status, (unsigned long long)(line << 8 | reason));
}

__global__ __launch_bounds__(64) void vcf_parse_kernel(VcfArgs a) {
  // col[f]: where field f starts, from the line's start; col[F] = len + 1, so
  // field f is [col[f], col[f + 1] - 1)
  // Dynamic LDS (vcf_parse_lds): the line's first kVcfStage bytes from its
  // aligned base, as the tab pass loaded them -- what lane 0 and the column
  // lanes read byte by byte comes from here, and from memory behind it --, then
  // col (F + 2), the table (slots) and lane 0's two words: the index of GT in
  // FORMAT, a reason.
  extern __shared__ uint4 vcf_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t S = a.n_samples, F = kVcfFixed + S, W = a.words;
  const uint32_t slots = vcf_slots(F);
  uint4* stage = vcf_lds;
  const uint8_t* stage8 = reinterpret_cast<const uint8_t*>(vcf_lds);
  uint32_t* col = reinterpret_cast<uint32_t*>(vcf_lds + kVcfStage / 16);
  uint32_t* table = col + F + 2;
  int32_t* lane0 = reinterpret_cast<int32_t*>(table + slots);
  for (uint64_t d = blockIdx.x; d < a.n_data; d += gridDim.x) {
    const uint64_t line = a.data_line[d];
    uint64_t start;
    const uint64_t len64 = vcf_content_len(a, line, &start);
    const uint8_t* t = a.text + start;
    if (len64 >= (1ull << 31)) {
      if (lane == 0) vcf_fail(a, line, MAGOT_VCF_LINE_TOO_LONG);
      continue;
    }
    const uint32_t len = (uint32_t)len64;
    const uint32_t skew = (uint32_t)(start & 15);
    // the first 64 bytes of the data line before, a lane each, asked for now
    // and used behind the tab pass; 0x100: no such byte
    uint32_t before = 0x100;
    uint64_t ps = 0, pl = 0;
    if (d > 0) {
      pl = vcf_content_len(a, a.data_line[d - 1], &ps);
      if (lane < pl) before = a.text[ps + lane];
    }
    // byte i of the line, i below len
    auto at = [&](uint32_t i) -> uint32_t {
      const uint32_t o = skew + i;
      return o < kVcfStage ? stage8[o] : t[i];
    };
    auto same = [&](uint32_t x, uint32_t y, uint32_t n) -> bool {
      for (uint32_t j = 0; j < n; ++j)
        if (at(x + j) != at(y + j)) return false;
      return true;
    };
    // ---- the tabs: 16 aligned bytes a lane, 1024 a round
    const uint64_t abase = start & ~15ull;
    const uint64_t end = start + len;
    uint32_t tabs = 0;  // before this round, the same in every lane
    for (uint64_t base = abase; base < end; base += 1024) {
      const uint64_t p = base + 16 * lane;
      uint32_t m = 0;
      if (p < end) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.text + p);
        m = byte_eq_mask16(v, 0x09090909u);  // TAB
        if (base - abase < kVcfStage) stage[(base - abase) / 16 + lane] = v;
        if (p < start) m &= ~((1u << (start - p)) - 1);      // start - p is below 16
        if (end - p < 16) m &= (1u << (end - p)) - 1;
      }
      const uint32_t c = __popc(m);
      uint32_t inc = c;
      for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(inc, s, 64);
        if ((int)lane >= s) inc += up;
      }
      uint32_t f = tabs + (inc - c) + 1;  // the field that starts behind this lane's first tab
      for (uint32_t mm = m; mm; mm &= mm - 1, ++f)
        if (f < F) col[f] = (uint32_t)(p + __ffs(mm) - start);
      tabs += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      col[0] = 0;
      col[F] = len + 1;
    }
    __syncthreads();
    if (tabs + 1 != F) {  // the same in every lane
      if (lane == 0) vcf_fail(a, line, MAGOT_VCF_FIELD_COUNT);
      __syncthreads();
      continue;
    }
    // ---- a run head: CHROM is not the data line before's, whose byte behind
    // it must be a tab
    const uint32_t chrom = col[1] - 1;
    uint32_t run_head = 1;
    if (d > 0 && chrom < 64) {
      const bool differs = lane < chrom ? before != at(lane) : lane == chrom && before != '\t';
      run_head = __ballot(differs) != 0;
    } else if (d > 0 && pl > chrom && a.text[ps + chrom] == '\t') {
      run_head = 0;
      for (uint32_t j = 0; j < chrom && !run_head; ++j) run_head = a.text[ps + j] != at(j);
    }
    // ---- lane 0: CHROM, POS, FORMAT
    if (lane == 0) {
      uint32_t reason = 0;
      const uint32_t clen = col[1] - 1;
      const uint32_t p0 = col[1], plen = col[2] - 1 - col[1];
      const uint32_t klen = clen + 3 + plen;
      uint64_t h = 0;
      uint32_t k = 0;
      auto feed = [&](uint32_t c) { h = py27_hash_step(h, k++, c); };
      for (uint32_t j = 0; j < clen; ++j) {
        feed(at(j));
        if (j + 2 < clen && at(j) == '<' && at(j + 1) == ':' && at(j + 2) == '>')
          reason = MAGOT_VCF_CHROM_FORM;  // the key would split elsewhere
      }
      feed('<');
      feed(':');
      feed('>');
      uint64_t v = 0;
      bool digits = plen >= 1;
      for (uint32_t j = 0; j < plen; ++j) {
        const uint32_t c = at(p0 + j);
        feed(c);
        if (c < '0' || c > '9') digits = false;
        else if (j < 10) v = v * 10 + (c - '0');
      }
      h = py27_hash_end(h, klen);  // klen >= 3
      if (!reason) {
        if (!digits || (plen > 1 && at(p0) == '0')) reason = MAGOT_VCF_POS_FORM;
        else if (plen > 10 || v > 0x7fffffffull) reason = MAGOT_VCF_POS_RANGE;
      }
      // FORMAT: the first subfield that is "GT"
      int32_t gi = -1, idx = 0;
      const uint32_t f0 = col[8], f1 = col[9] - 1;
      for (uint32_t b = f0; b <= f1 && gi < 0;) {
        uint32_t e = b;
        while (e < f1 && at(e) != ':') ++e;
        if (e - b == 2 && at(b) == 'G' && at(b + 1) == 'T') gi = idx;
        ++idx;
        b = e + 1;
      }
      if (!reason && gi < 0) reason = MAGOT_VCF_NO_GT;
      a.pos[d] = reason ? 0 : (int32_t)v;
      a.hash[d] = h;
      a.chrom_len[d] = clen;
      a.head[d] = run_head;
      lane0[0] = gi;
      lane0[1] = (int32_t)reason;
    }
    for (uint32_t i = lane; i < slots; i += 64) table[i] = kVcfEmpty;
    __syncthreads();
    const int32_t gi = lane0[0];
    if (lane0[1]) {
      if (lane == 0) vcf_fail(a, line, (uint32_t)lane0[1]);
      __syncthreads();
      continue;
    }
    // ---- every field into the table: the least index per byte string
    for (uint32_t f = lane; f < F; f += 64) {
      const uint32_t b = col[f], n = col[f + 1] - 1 - b;
      uint32_t h = 2166136261u;
      for (uint32_t j = 0; j < n; ++j) h = (h ^ at(b + j)) * 16777619u;
      uint32_t slot = h & (slots - 1);
      for (uint32_t tries = 0; tries < slots; ++tries, slot = (slot + 1) & (slots - 1)) {
        const uint32_t old = atomicCAS(&table[slot], kVcfEmpty, f);
        if (old == kVcfEmpty) break;  // claimed
        // old is a field below F whose string owns the slot for good
        const uint32_t ob = col[old], on = col[old + 1] - 1 - ob;
        if (on == n && same(ob, b, n)) {
          atomicMin(&table[slot], f);
          break;
        }
      }
    }
    __syncthreads();
    // ---- a lane per sample column
    for (uint32_t g = 0; g < S; g += 64) {
      const uint32_t s = g + lane;
      bool het = false;
      if (s < S) {
        const uint32_t f = kVcfFixed + s;
        const uint32_t b = col[f], n = col[f + 1] - 1 - b;
        uint32_t h = 2166136261u;
        for (uint32_t j = 0; j < n; ++j) h = (h ^ at(b + j)) * 16777619u;
        uint32_t slot = h & (slots - 1), least = f;
        for (uint32_t tries = 0; tries < slots; ++tries, slot = (slot + 1) & (slots - 1)) {
          const uint32_t m = table[slot];
          if (m == kVcfEmpty) break;  // not reached: f itself is in the table
          const uint32_t ob = col[m], on = col[m + 1] - 1 - ob;
          if (m == f || (on == n && same(ob, b, n))) {
            least = m;
            break;
          }
        }
        // the GT subfield: behind gi colons
        uint32_t x = b;
        const uint32_t e = b + n;
        int32_t colons = 0;
        while (x < e && colons < gi) colons += at(x++) == ':';
        uint32_t y = x;
        while (y < e && at(y) != ':') ++y;
        if (least < kVcfFixed) vcf_fail(a, line, MAGOT_VCF_EQUALS_FIXED);
        else if (colons < gi || y == x) vcf_fail(a, line, MAGOT_VCF_EMPTY_GT);
        else het = least == f && at(x) != at(y - 1);
      }
      const unsigned long long vote = __ballot(het);
      if (lane == 0) {
        const uint32_t w = g >> 5;
        a.bits[d * W + w] = (uint32_t)vote;
        if (w + 1 < W) a.bits[d * W + w + 1] = (uint32_t)(vote >> 32);
      }
    }
    __syncthreads();  // the table and col are rewritten for the next line
  }
}

__global__ __launch_bounds__(kVcfThreads) void vcf_runs_kernel(VcfArgs a) {
  const uint64_t d = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (d >= a.n_data || !a.head[d]) return;
  const uint32_t r = a.run[d];  // below n_runs
  a.run_off[r] = a.line_start[a.data_line[d]];
  a.run_len[r] = a.chrom_len[d];
}

__global__ __launch_bounds__(kVcfThreads) void vcf_keys_kernel(VcfArgs a) {
  const uint64_t d = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (d >= a.n_data) return;
  const uint32_t r = a.run[d] + a.head[d] - 1;  // head[0] is 1: never below 0
  a.key[d] = (uint64_t)a.contig_of_run[r] << 32 | (uint32_t)a.pos[d];
  a.val[d] = (uint32_t)d;
}

__global__ __launch_bounds__(kVcfThreads) void vcf_flags_kernel(VcfArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (i >= a.n_data) return;
  const uint64_t k = a.key_sorted[i];
  const uint8_t first = i == 0 || a.key_sorted[i - 1] != k;
  const uint8_t last = i + 1 == a.n_data || a.key_sorted[i + 1] != k;
  const uint32_t d = a.val_sorted[i];  // below n_data
  a.kept_sorted[i] = last;
  a.kept[d] = last;
  a.first[d] = first;
}

__global__ __launch_bounds__(kVcfThreads) void vcf_last_of_kernel(VcfArgs a, uint64_t d,
                                                                  uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (i >= a.n_data) return;
  if (a.kept_sorted[i] && a.key_sorted[i] == a.key[d]) *out = a.data_line[a.val_sorted[i]];
}

// the first row in [0, n) whose key is not below k
__device__ __forceinline__ uint64_t vcf_lower(const uint64_t* keys, uint64_t n, uint64_t k) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kVcfThreads) void vcf_ranges_kernel(VcfArgs a, VcfCountArgs c) {
  const uint64_t l = (uint64_t)blockIdx.x * kVcfThreads + threadIdx.x;
  if (l > c.n_loci) return;
  if (l == c.n_loci) {
    c.pieces[l] = 0;
    return;
  }
  uint64_t b = 0, e = 0;
  if (c.lo[l] <= c.hi[l]) {
    const uint64_t top = (uint64_t)c.contig[l] << 32;
    b = vcf_lower(a.key_sorted, a.n_data, top | c.lo[l]);
    // hi + 1 may carry into the contig: the first key of the next one
    e = vcf_lower(a.key_sorted, a.n_data, (top | c.hi[l]) + 1);
    if ((top | c.hi[l]) == ~0ull) e = a.n_data;
  }
  c.rng_b[l] = b;
  c.rng_e[l] = e;
  c.pieces[l] = (e - b + kVcfSplit - 1) / kVcfSplit;
}

__global__ __launch_bounds__(64) void vcf_count_kernel(VcfArgs a, VcfCountArgs c) {
  const uint64_t p = blockIdx.x;  // below n_pieces
  // the locus whose pieces hold p: the last l with piece_off[l] <= p
  uint64_t lo = 0, hi = c.n_loci;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (c.piece_off[mid] <= p) lo = mid;
    else hi = mid;
  }
  const uint64_t l = lo;
  const uint64_t r0 = c.rng_b[l] + (p - c.piece_off[l]) * kVcfSplit;
  const uint64_t r1 = r0 + kVcfSplit < c.rng_e[l] ? r0 + kVcfSplit : c.rng_e[l];
  const uint32_t S = a.n_samples, W = a.words;
  bool foreign = false;
  for (uint32_t s = threadIdx.x; s < ((S + 63) & ~63u); s += 64) {
    const uint32_t w = s >> 5;
    const uint32_t ok = w < W ? c.allowed[w] : 0;
    uint32_t cnt = 0;
    if (w < W)
      for (uint64_t i = r0; i < r1; ++i) {  // rows below n_data
        if (!a.kept_sorted[i]) continue;
        const uint32_t word = a.bits[(uint64_t)a.val_sorted[i] * W + w];
        cnt += word >> (s & 31) & 1;
        foreign |= (word & ~ok) != 0;
      }
    if (s < S && cnt) atomicAdd(&c.counts[l * S + s], cnt);
  }
  if (foreign) atomicMax(c.foreign, 1u);
}

}  // namespace

size_t vcf_tmp_bytes(uint64_t n_lines) {
  size_t z = 0;
  const size_t n = (size_t)n_lines;
  const size_t x = exclusive_sum_bytes<uint64_t>(n + 1), y = exclusive_sum_bytes<uint32_t>(n + 1);
  (void)rocprim::radix_sort_pairs(nullptr, z, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 64,
                                  hipStream_t(0));
  return std::max(x, std::max(y, z));
}

size_t vcf_count_tmp_bytes(uint64_t n_loci) { return exclusive_sum_bytes<uint64_t>(n_loci + 1); }

hipError_t launch_vcf_classify(const VcfArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  // status: nothing declined, no '#' line, no first '#' line, no first data line, no CR
  static const unsigned long long kClean[5] = {~0ull, 0, ~0ull, ~0ull, 0};
  if (hipError_t e = hipMemcpyAsync(a.status, kClean, sizeof kClean, hipMemcpyHostToDevice, s))
    return e;
  vcf_cr_kernel<<<vcf_blocks_for((a.n + 15) / 16), kVcfThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  vcf_classify_kernel<<<vcf_blocks_for(a.n_lines + 1), kVcfThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return exclusive_sum(tmp, tmp_bytes, a.kind, a.kpos, a.n_lines + 1, s);
}

hipError_t launch_vcf_compact(const VcfArgs& a, hipStream_t s) {
  if (!a.n_lines) return hipSuccess;
  vcf_compact_kernel<<<vcf_blocks_for(a.n_lines), kVcfThreads, 0, s>>>(a);
  return hipGetLastError();
}

// the most workgroups of the parse pass: 2^20, above which its workgroups stride
// over the data lines.  MAGOT_VCF_PARSE_GRID = 1 .. 2^20 lowers it (test hook:
// force the stride); read on every call, anything else is 2^20.
static uint64_t vcf_parse_grid_cap() {
  constexpr uint64_t kCap = 1u << 20;
  const char* e = std::getenv("MAGOT_VCF_PARSE_GRID");
  if (!e || !*e) return kCap;
  char* end = nullptr;
  errno = 0;
  const unsigned long long v = std::strtoull(e, &end, 10);
  if (errno || *end || *e < '0' || *e > '9' || v < 1 || v > kCap) return kCap;
  return v;
}

hipError_t launch_vcf_parse(const VcfArgs& a, hipStream_t s) {
  if (!a.n_data) return hipSuccess;
  // what a line outside the grammar leaves unwritten is zero, and head[n_data] ends the scan
  if (hipError_t e = hipMemsetAsync(a.head, 0, (a.n_data + 1) * sizeof(uint32_t), s)) return e;
  if (hipError_t e = hipMemsetAsync(a.bits, 0, a.n_data * a.words * sizeof(uint32_t), s)) return e;
  // a workgroup per line (a grid of 8192 that strides over the lines measured 22 % slower)
  const unsigned grid = (unsigned)std::min<uint64_t>(a.n_data, vcf_parse_grid_cap());
  vcf_parse_kernel<<<grid, 64, vcf_parse_lds(a.n_samples), s>>>(a);
  return hipGetLastError();
}

hipError_t launch_vcf_runs_scan(const VcfArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  return exclusive_sum(tmp, tmp_bytes, a.head, a.run, a.n_data + 1, s);
}

hipError_t launch_vcf_runs(const VcfArgs& a, hipStream_t s) {
  if (!a.n_data) return hipSuccess;
  vcf_runs_kernel<<<vcf_blocks_for(a.n_data), kVcfThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_vcf_sort(const VcfArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (!a.n_data) return hipSuccess;
  vcf_keys_kernel<<<vcf_blocks_for(a.n_data), kVcfThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint64_t*)a.key, a.key_sorted,
                                   (const uint32_t*)a.val, a.val_sorted, (size_t)a.n_data, 0,
                                   a.key_bits, s);
}

hipError_t launch_vcf_flags(const VcfArgs& a, hipStream_t s) {
  if (!a.n_data) return hipSuccess;
  vcf_flags_kernel<<<vcf_blocks_for(a.n_data), kVcfThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_vcf_last_of(const VcfArgs& a, uint64_t d, uint32_t* out, hipStream_t s) {
  vcf_last_of_kernel<<<vcf_blocks_for(a.n_data), kVcfThreads, 0, s>>>(a, d, out);
  return hipGetLastError();
}

hipError_t launch_vcf_ranges(const VcfArgs& a, const VcfCountArgs& c, void* tmp, size_t tmp_bytes,
                             hipStream_t s) {
  vcf_ranges_kernel<<<vcf_blocks_for(c.n_loci + 1), kVcfThreads, 0, s>>>(a, c);
  if (hipError_t e = hipGetLastError()) return e;
  return exclusive_sum(tmp, tmp_bytes, c.pieces, c.piece_off, c.n_loci + 1, s);
}

hipError_t launch_vcf_count(const VcfArgs& a, const VcfCountArgs& c, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(c.counts, 0, c.n_loci * a.n_samples * sizeof(uint32_t), s))
    return e;
  if (hipError_t e = hipMemsetAsync(c.foreign, 0, sizeof(uint32_t), s)) return e;
  if (!c.n_pieces) return hipSuccess;
  vcf_count_kernel<<<(unsigned)c.n_pieces, 64, 0, s>>>(a, c);
  return hipGetLastError();
}

}  // namespace magot
