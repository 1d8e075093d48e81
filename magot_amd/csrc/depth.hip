// depth_from_gff on the device (genome_tools.py:598-652): a `samtools depth`
// table (name, position, depth; one line per base) parsed into an int32 per
// line, and interval sums over it.
//
// A table whose contigs each form one run of lines with positions 1, 2, ..
// needs no scatter: the depth of (contig, pos) is the depth column at line
// run_start + pos - 1.  The track is that column in line order ("arena"), the
// contig table the list of run heads.
//
// Per chunk of text (the host cuts the file after an LF):
//   lf_count_kernel   LFs per text block of kTextBlock bytes, one 16-byte load
//                     per lane; rocprim's exclusive scan gives each block's
//                     first line within the chunk, the carry's running total
//                     its place in the file.
//   parse_kernel      the block's text (and a halo for lines that run past it)
//                     staged in LDS; a lane owns the lines that start in its
//                     16 bytes: tokenise, validate, compare name and position
//                     with the line before (the carry's for a chunk's first
//                     line), store the depth at arena[line], append a run head
//                     through one atomic counter, and atomic-min the first
//                     offending line and its reason into the status word.
// After the last chunk:
//   block_sum_kernel  one wave per kDepthBlock depths -> int64, then the scan:
//                     the directory.
//   sums_kernel       one lane per (start, length) row: two directory entries
//                     and two partial block edges.
//   group_kernel      one lane per CSR group of rows.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace magot {
namespace {

constexpr int kDepthThreads = 256;
constexpr int kLaneBytes = 16;
constexpr int kHalo = 512;  // a line of the grammar's usual length ends inside it
static_assert(kTextBlock == kDepthThreads * kLaneBytes, "one 16-byte load per lane");
static_assert(kDepthBlock == 64 * 4, "one 16-byte load per lane of a wave");

inline unsigned blocks_for(uint64_t n) {
  return (unsigned)((n + kDepthThreads - 1) / kDepthThreads);
}

__device__ __forceinline__ bool is_blank(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool is_graph(uint32_t c) { return c >= 0x21 && c <= 0x7E; }
__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }

// bytes of x equal to LF
__device__ __forceinline__ uint32_t lf_count4(uint32_t x) {
  x ^= 0x0A0A0A0Au;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;  // bit 7: low seven bits non-zero
  return __popc(~(t | x | 0x7f7f7f7fu));
}

__global__ __launch_bounds__(kDepthThreads) void lf_count_kernel(const uint8_t* __restrict__ text,
                                                                 int64_t n, uint32_t n_blocks,
                                                                 uint32_t* __restrict__ count) {
  __shared__ uint32_t total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  uint32_t c = 0;
  if (blockIdx.x < n_blocks) {  // block n_blocks is the sentinel: its prefix is the total
    const int64_t i = (int64_t)blockIdx.x * kTextBlock + kLaneBytes * threadIdx.x;
    if (i + kLaneBytes <= n) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + i);
      c = lf_count4(v.x) + lf_count4(v.y) + lf_count4(v.z) + lf_count4(v.w);
    } else {
      for (int j = 0; j < kLaneBytes; ++j)
        if (i + j < n && text[i + j] == '\n') ++c;
    }
  }
  if (c) atomicAdd(&total, c);
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = total;
}

// The chunk's bytes [0, n): the block's text and its halo from LDS, anything
// else (a predecessor before the block, a line longer than the halo) from
// memory; every index at or past n reads as LF, so no loop leaves the chunk.
struct TextView {
  const uint8_t* text;
  const uint8_t* lds;
  int64_t lo, hi, n;
  __device__ __forceinline__ uint32_t at(int64_t i) const {
    if (i >= n) return '\n';
    if (i >= lo && i < hi) return lds[i - lo];
    return text[i];
  }
  // an LF, or a CR directly before one
  __device__ __forceinline__ bool ends(int64_t i) const {
    const uint32_t c = at(i);
    return c == '\n' || (c == '\r' && at(i + 1) == '\n');
  }
};

// 1 to 10 digits, value <= 2^31 - 1, followed by a blank or the line's end
__device__ __forceinline__ uint32_t parse_number(const TextView& v, int64_t& i, uint32_t& out) {
  uint32_t c = v.at(i);
  if (c == '+' || c == '-') return MAGOT_DEPTH_SIGN;
  if (!is_digit(c)) return is_graph(c) ? MAGOT_DEPTH_NOT_NUMBER : MAGOT_DEPTH_BAD_BYTE;
  uint64_t val = 0;
  int digits = 0;
  while (is_digit(c)) {
    if (++digits > 10) return MAGOT_DEPTH_NUMBER_RANGE;
    val = val * 10 + (c - '0');
    c = v.at(++i);
  }
  if (val > 0x7fffffffull) return MAGOT_DEPTH_NUMBER_RANGE;
  if (!is_blank(c) && !v.ends(i)) return is_graph(c) ? MAGOT_DEPTH_NOT_NUMBER : MAGOT_DEPTH_BAD_BYTE;
  out = (uint32_t)val;
  return 0;
}

__device__ __forceinline__ void skip_blanks(const TextView& v, int64_t& i) {
  while (is_blank(v.at(i))) ++i;
}

struct LineFields {
  uint32_t name_len, pos, depth;
};

// the grammar of one line starting at p; 0, or the reason it is outside it
__device__ uint32_t parse_line(const TextView& v, int64_t p, LineFields& f) {
  int64_t i = p;
  uint32_t c = v.at(i);
  if (v.ends(i)) return MAGOT_DEPTH_EMPTY_LINE;
  if (is_blank(c)) return MAGOT_DEPTH_LEADING_BLANK;
  uint32_t len = 0;
  while (is_graph(c)) {
    if (++len > 255) return MAGOT_DEPTH_NAME_LONG;
    c = v.at(++i);
  }
  if (len == 0) return MAGOT_DEPTH_BAD_BYTE;
  if (v.ends(i)) return MAGOT_DEPTH_FEW_FIELDS;
  if (!is_blank(c)) return MAGOT_DEPTH_BAD_BYTE;
  f.name_len = len;
  skip_blanks(v, i);
  if (v.ends(i)) return MAGOT_DEPTH_FEW_FIELDS;
  if (uint32_t code = parse_number(v, i, f.pos)) return code;
  skip_blanks(v, i);
  if (v.ends(i)) return MAGOT_DEPTH_FEW_FIELDS;
  if (uint32_t code = parse_number(v, i, f.depth)) return code;
  for (;;) {  // further columns are ignored, their bytes are not
    skip_blanks(v, i);
    if (v.ends(i)) break;
    c = v.at(i);
    if (!is_graph(c)) return MAGOT_DEPTH_BAD_BYTE;
    while (is_graph(c)) c = v.at(++i);
  }
  return 0;
}

__device__ void depth_line(const DepthParseArgs& a, const TextView& v, int64_t p, uint64_t line,
                           bool last) {
  LineFields f;
  f.name_len = f.pos = f.depth = 0;
  const uint32_t code = parse_line(v, p, f);
  if (code) {
    atomicMin(a.status, (unsigned long long)(line << 8 | code));
    return;
  }
  if (line < a.arena_cap) a.arena[line] = (int32_t)f.depth;
  // the line before: the carry's for a chunk's first line
  bool have_prev, same = false;
  uint32_t prev_pos = 0;
  if (p == 0) {
    have_prev = a.in->has_prev != 0;
    if (have_prev) {
      prev_pos = a.in->pos;
      same = a.in->name_len == f.name_len;
      for (uint32_t k = 0; same && k < f.name_len; ++k) same = a.in->name[k] == v.at(p + k);
    }
  } else {
    have_prev = true;
    int64_t q = p - 1;  // the predecessor's LF
    while (q > 0 && v.at(q - 1) != '\n') --q;
    // its name and position; when it is outside the grammar its own lane
    // reports it, with the smaller line index
    uint32_t plen = 0;
    while (plen < 256 && is_graph(v.at(q + plen))) ++plen;
    int64_t i = q + plen;
    skip_blanks(v, i);
    uint64_t val = 0;
    for (int d = 0; d < 10 && is_digit(v.at(i)); ++d, ++i) val = val * 10 + (v.at(i) - '0');
    prev_pos = (uint32_t)val;
    same = plen == f.name_len;
    for (uint32_t k = 0; same && k < plen; ++k) same = v.at(q + k) == v.at(p + k);
  }
  const bool head = !have_prev || !same;
  if (f.pos != (head ? 1u : prev_pos + 1u))
    atomicMin(a.status, (unsigned long long)(line << 8 | MAGOT_DEPTH_POS_SEQUENCE));
  if (head) {
    const uint32_t slot = atomicAdd(a.n_heads, 1u);
    if (slot < a.heads_cap) {
      DepthHead h;
      h.line = line;
      h.offset = a.file_off + (uint64_t)p;
      h.name_len = f.name_len;
      h.pad = 0;
      a.heads[slot] = h;
    }
  }
  if (last) {  // the chunk's last line: what the next chunk's first compares with
    a.out->has_prev = 1;
    a.out->name_len = f.name_len;
    a.out->pos = f.pos;
    for (uint32_t k = 0; k < f.name_len; ++k) a.out->name[k] = (uint8_t)v.at(p + k);
  }
}

__global__ __launch_bounds__(kDepthThreads) void parse_kernel(DepthParseArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kTextBlock + kHalo];
  __shared__ uint32_t wave_sum[kDepthThreads / 64];
  const int t = threadIdx.x;
  const int64_t blk0 = (int64_t)blockIdx.x * kTextBlock;
  for (int q = t; q < (kTextBlock + kHalo) / kLaneBytes; q += kDepthThreads) {
    const int64_t i = blk0 + kLaneBytes * q;
    if (i + kLaneBytes <= a.n) {
      *reinterpret_cast<uint4*>(stage + kLaneBytes * q) =
          *reinterpret_cast<const uint4*>(a.text + i);
    } else {
      for (int j = 0; j < kLaneBytes; ++j)
        if (i + j < a.n) stage[kLaneBytes * q + j] = a.text[i + j];
    }
  }
  __syncthreads();
  TextView v;
  v.text = a.text;
  v.lds = stage;
  v.lo = blk0;
  v.hi = min(blk0 + (int64_t)(kTextBlock + kHalo), a.n);
  v.n = a.n;

  // the LFs of this lane's 16 bytes, and the line starts: the byte after an
  // LF, and the chunk's first byte
  const int64_t p0 = blk0 + kLaneBytes * t;
  uint32_t lf = 0, valid = 0;
  for (int j = 0; j < kLaneBytes; ++j)
    if (p0 + j < a.n) {
      valid |= 1u << j;
      if (stage[kLaneBytes * t + j] == '\n') lf |= 1u << j;
    }
  bool before;  // the byte before p0 is an LF
  if (t > 0) before = stage[kLaneBytes * t - 1] == '\n';
  else before = blk0 == 0 || a.text[blk0 - 1] == '\n';
  const uint32_t starts = ((lf << 1) | (before ? 1u : 0u)) & valid;

  // exclusive prefix of the lanes' LF counts over the block
  const uint32_t c = __popc(lf);
  const uint32_t lane = t & 63, wave = t >> 6;
  uint32_t inc = c;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += up;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t below = inc - c;
  for (uint32_t w = 0; w < wave; ++w) below += wave_sum[w];

  const uint64_t first = a.in->lines + a.blk_first[blockIdx.x];
  // the lines of the file up to the chunk's end; a last line may lack its LF
  const uint64_t lines = a.in->lines + a.blk_first[gridDim.x] + (a.text[a.n - 1] != '\n' ? 1 : 0);
  for (uint32_t m = starts; m; m &= m - 1) {
    const int j = __ffs(m) - 1;
    const uint64_t line = first + below + __popc(lf & ((1u << j) - 1));
    depth_line(a, v, p0 + j, line, line + 1 == lines);
  }
  if (blockIdx.x == 0 && t == 0) a.out->lines = lines;
}

__global__ __launch_bounds__(kDepthThreads) void block_sum_kernel(
    const int32_t* __restrict__ arena, uint64_t n_lines, uint64_t n_blocks,
    int64_t* __restrict__ sum) {
  const uint64_t b = (uint64_t)blockIdx.x * (kDepthThreads / 64) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (b > n_blocks) return;
  int64_t s = 0;
  if (b < n_blocks) {  // entry n_blocks is the sentinel: its prefix is the total
    // the arena is allocated in whole blocks; what lies past n_lines is not summed
    const uint64_t i = b * kDepthBlock + 4 * lane;
    const int4 v = *reinterpret_cast<const int4*>(arena + i);
    if (i < n_lines) s += v.x;
    if (i + 1 < n_lines) s += v.y;
    if (i + 2 < n_lines) s += v.z;
    if (i + 3 < n_lines) s += v.w;
  }
  for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) sum[b] = s;
}

// the sum of the depths of the lines below x (x <= n_lines)
__device__ __forceinline__ int64_t depth_prefix(const int32_t* __restrict__ arena,
                                                const int64_t* __restrict__ dir, uint64_t x) {
  const uint64_t b = x / kDepthBlock;
  const uint32_t rem = (uint32_t)(x % kDepthBlock);
  int64_t r = dir[b];
  const int4* p = reinterpret_cast<const int4*>(arena + b * kDepthBlock);
  for (uint32_t q = 0; 4 * q < rem; ++q) {
    const int4 v = p[q];
    const uint32_t left = rem - 4 * q;
    r += v.x;
    if (left > 1) r += v.y;
    if (left > 2) r += v.z;
    if (left > 3) r += v.w;
  }
  return r;
}

__global__ __launch_bounds__(kDepthThreads) void sums_kernel(
    const int32_t* __restrict__ arena, const int64_t* __restrict__ dir, uint64_t n_lines,
    const int64_t* __restrict__ start, const int64_t* __restrict__ length, uint64_t n_rows,
    int64_t* __restrict__ sums) {
  const uint64_t i = (uint64_t)blockIdx.x * kDepthThreads + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t s = start[i], len = length[i];
  int64_t r = 0;
  // the host checked every row: the range test is never what decides
  if (len > 0 && s >= 0 && (uint64_t)s <= n_lines && (uint64_t)len <= n_lines - (uint64_t)s)
    r = depth_prefix(arena, dir, (uint64_t)(s + len)) - depth_prefix(arena, dir, (uint64_t)s);
  sums[i] = r;
}

__global__ __launch_bounds__(kDepthThreads) void group_kernel(
    const int64_t* __restrict__ sums, const uint64_t* __restrict__ offsets, uint64_t n_groups,
    int64_t* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * kDepthThreads + threadIdx.x;
  if (g >= n_groups) return;
  int64_t r = 0;
  for (uint64_t k = offsets[g]; k < offsets[g + 1]; ++k) r += sums[k];
  out[g] = r;
}

}  // namespace

size_t depth_scan_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                uint32_t(0), (size_t)n, rocprim::plus<uint32_t>(), hipStream_t(0));
  (void)rocprim::exclusive_scan(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr,
                                int64_t(0), (size_t)n, rocprim::plus<int64_t>(), hipStream_t(0));
  return a > b ? a : b;
}

hipError_t launch_depth_line_index(const uint8_t* text, uint64_t n, uint32_t* count,
                                   uint32_t* first, void* scan_tmp, size_t scan_bytes,
                                   hipStream_t s) {
  const uint32_t n_blocks = (uint32_t)depth_text_blocks(n);
  lf_count_kernel<<<n_blocks + 1, kDepthThreads, 0, s>>>(text, (int64_t)n, n_blocks, count);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::exclusive_scan(scan_tmp, scan_bytes, count, first, uint32_t(0),
                                 (size_t)n_blocks + 1, rocprim::plus<uint32_t>(), s);
}

hipError_t launch_depth_parse(const DepthParseArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  parse_kernel<<<(unsigned)depth_text_blocks((uint64_t)a.n), kDepthThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_depth_directory(const int32_t* arena, uint64_t n_lines, int64_t* block_sum,
                                  int64_t* dir, void* scan_tmp, size_t scan_bytes,
                                  hipStream_t s) {
  const uint64_t n_blocks = depth_blocks(n_lines);
  block_sum_kernel<<<blocks_for((n_blocks + 1) * 64), kDepthThreads, 0, s>>>(arena, n_lines,
                                                                             n_blocks, block_sum);
  if (hipError_t e = hipGetLastError()) return e;
  return rocprim::exclusive_scan(scan_tmp, scan_bytes, block_sum, dir, int64_t(0),
                                 (size_t)(n_blocks + 1), rocprim::plus<int64_t>(), s);
}

hipError_t launch_depth_sums(const int32_t* arena, const int64_t* dir, uint64_t n_lines,
                             const int64_t* start, const int64_t* length, uint64_t n_rows,
                             int64_t* sums, hipStream_t s) {
  if (!n_rows) return hipSuccess;
  sums_kernel<<<blocks_for(n_rows), kDepthThreads, 0, s>>>(arena, dir, n_lines, start, length,
                                                           n_rows, sums);
  return hipGetLastError();
}

hipError_t launch_depth_groups(const int64_t* sums, const uint64_t* offsets, uint64_t n_groups,
                               int64_t* out, hipStream_t s) {
  if (!n_groups) return hipSuccess;
  group_kernel<<<blocks_for(n_groups), kDepthThreads, 0, s>>>(sums, offsets, n_groups, out);
  return hipGetLastError();
}

}  // namespace magot
