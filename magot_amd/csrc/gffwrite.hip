// write_gff's text on the device (genome.py:228-238, 616-645, 733-778): the
// host planner (gffplan.cpp: magot_gff_lower_write) says what every output line
// is made of, one magot_gffrow per line in output order; these kernels make the
// bytes.
//
//   size_kernel    one lane per row.  It walks its source line to the eighth
//                  tab (at most kGwMaxHead bytes, never past an LF or the text's
//                  end), classifies the score and the phase and adds the line's
//                  length up, the decimal widths of lo and hi included.  The
//                  tabs and the score's digit runs stay in a GwAux for the
//                  render.  A line without its eight tabs, or a score outside
//                  the two classes of magot.h, atomic-mins (row << 8 | reason)
//                  into the status word; the host declines the table.
//   the scan       textindex.hip's exclusive_sum over the lengths (64-bit).
//   render_kernel  one wave per kGwGroup consecutive rows, four waves a
//                  workgroup.  One lane per row stages the row in LDS as ten
//                  segments: runs of the text or the blob (a column with its
//                  tab, a referenced name), or bytes made up in the row's LDS
//                  scratch (the integers, the normalised score, the phase and
//                  the literals).  The group's output range is contiguous, so
//                  after the barrier the lanes are dealt over its 16-byte
//                  chunks: a lane finds its chunk's first row by a binary
//                  search over the staged offsets, its segment by a walk over
//                  at most ten ends, and from there takes byte after byte.
//                  A chunk that lies whole inside the group's range is one
//                  16-byte store; the range's first and last chunk, where
//                  shared with a neighbouring group, are stored byte by byte
//                  within the range.  Every output byte is written exactly once.
//
// Score rule (Python 2's str(float(s)) = '%.12g' and '.0' on a bare integer):
// a double carries more than 15 significant decimal digits, so a literal of at
// most 12 significant digits prints as its own digits as long as '%.12g' stays
// in fixed notation, that is for a decimal exponent of -5 < x < 12: at most 12
// integer digits and, below 1, at most 3 zeros behind the point.
//
// Where the headroom is: the staging uses 32 of a wave's 64 lanes (one lane a
// row, kGwGroup rows), each walking its own row serially, and the copy takes
// every output byte by a byte load of its own behind a segment lookup in LDS.
// Measured at 5.4 to 6.4 times a device copy of as many bytes (EXPERIMENTS).
//
// LDS: 8200 bytes a wave.  No spin-wait, no atomics but the status word's min.
#include "common.h"

namespace magot {
namespace {

constexpr int kGwSegs = 10;
constexpr int kGwScratch = 128;
constexpr uint64_t kGwLds = 1ull << 63;  // a segment source in the row's scratch
constexpr int kGwWaves = kGwThreads / 64;

struct GwStage {
  uint64_t rowoff[kGwGroup + 1];
  uint64_t src[kGwGroup][kGwSegs];
  uint32_t end[kGwGroup][kGwSegs];
  uint8_t scratch[kGwGroup][kGwScratch];
};

__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }
__device__ __forceinline__ bool is_letter(uint32_t c) { return (c | 32u) - 'a' < 26u; }

__device__ __forceinline__ uint32_t dec_width(int64_t v) {
  uint64_t m = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  uint32_t w = v < 0 ? 2 : 1;
  while (m >= 10) {
    m /= 10;
    ++w;
  }
  return w;
}

// v in decimal at p; returns its width
__device__ __forceinline__ uint32_t dec_put(uint8_t* p, int64_t v) {
  const uint32_t w = dec_width(v);
  uint64_t m = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  for (uint32_t i = w; i-- > (v < 0 ? 1u : 0u);) {
    p[i] = (uint8_t)('0' + m % 10);
    m /= 10;
  }
  if (v < 0) p[0] = '-';
  return w;
}

__device__ __forceinline__ void offend(const GwArgs& a, uint64_t r, uint32_t why) {
  atomicMin(a.status, (unsigned long long)(r << 8 | why));
}

__device__ __forceinline__ uint32_t prefix_len(uint32_t kind) {
  return kind == MAGOT_GFFROW_GTF ? 14u : kind == MAGOT_GFFROW_EXON_TWIN ? 9u : 3u;
}

__global__ __launch_bounds__(256) void size_kernel(GwArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > a.n_rows) return;
  if (r == a.n_rows) {
    a.len[r] = 0;
    return;
  }
  const magot_gffrow row = a.rows[r];
  const uint32_t kind = row.kind & 0xffu;
  const bool has_parent = (row.kind & MAGOT_GFFROW_HAS_PARENT) != 0;
  GwAux x{};
  const uint64_t p0 = row.line_off;
  const uint64_t limit = a.n - p0 < kGwMaxHead ? a.n : p0 + kGwMaxHead;  // p0 <= n (the host checked)
  uint32_t tabs = 0;
  for (uint64_t i = p0; i < limit && tabs < 8; ++i) {
    const uint32_t c = a.text[i];
    if (c == '\n') break;
    if (c == '\t') x.tab[tabs++] = (uint32_t)(i - p0);
  }
  if (tabs < 8) {
    offend(a, r, MAGOT_GFFWRITE_COLUMNS);
    a.len[r] = 0;
    a.aux[r] = x;
    return;
  }
  const uint8_t* line = a.text + p0;
  const bool made = kind == MAGOT_GFFROW_MADE_PARENT;
  uint32_t score_len = 1;
  if (!made) {
    const uint32_t b0 = x.tab[4] + 1, b1 = x.tab[5];
    bool alnum = false;
    for (uint32_t i = b0; i < b1; ++i) alnum |= is_digit(line[i]) || is_letter(line[i]);
    if (alnum) {
      uint32_t i = b0;
      const bool neg = line[i] == '-';
      i += neg;
      uint32_t i0 = i;
      while (i < b1 && is_digit(line[i])) ++i;
      const uint32_t i1 = i;
      const bool dot = i < b1 && line[i] == '.';
      i += dot;
      const uint32_t f0 = i;
      while (i < b1 && is_digit(line[i])) ++i;
      uint32_t f1 = i;
      bool ok = i == b1 && (i1 > i0 || (dot && f1 > f0));
      while (i0 < i1 && line[i0] == '0') ++i0;
      uint32_t lead = 0;
      while (f0 + lead < f1 && line[f0 + lead] == '0') ++lead;
      while (f1 > f0 && line[f1 - 1] == '0') --f1;
      const uint32_t il = i1 - i0, fl = f1 - f0;
      const uint32_t span = il ? il + fl : (fl ? fl - lead : 0);
      ok = ok && il <= 12 && span <= 12 && (il || !fl || lead <= 3);
      if (!ok) {
        offend(a, r, MAGOT_GFFWRITE_SCORE);
        a.len[r] = 0;
        a.aux[r] = x;
        return;
      }
      x.flags |= kGwScoreNum | (neg ? kGwScoreNeg : 0u);
      x.int_off = i0;
      x.int_len = il;
      x.frac_off = f0;
      x.frac_len = fl;
      score_len = (neg ? 1u : 0u) + (il ? il : 1u) + 1u + (fl ? fl : 1u);
    }
    if (x.tab[7] - x.tab[6] == 2 && line[x.tab[6] + 1] - '0' < 3u) x.flags |= kGwPhase;
  }
  uint64_t n = x.tab[0] + 1;                                       // c1 and its tab
  n += made ? 2 : x.tab[1] - x.tab[0];                             // c2
  n += made ? row.type_len + 1
            : kind == MAGOT_GFFROW_EXON_TWIN ? 5 : x.tab[2] - x.tab[1];  // c3
  n += dec_width(row.lo) + 1 + dec_width(row.hi) + 1 + score_len + 1;
  n += x.tab[6] - x.tab[5];                                        // c7
  n += 2 + prefix_len(kind) + row.id_len;
  if (has_parent) n += (kind == MAGOT_GFFROW_GTF ? 9 : 8) + row.parent_len;
  n += 1;
  a.len[r] = n;
  a.aux[r] = x;
}

__device__ __forceinline__ uint32_t put(uint8_t* p, const char* s, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) p[i] = (uint8_t)s[i];
  return n;
}

// One row's segments into the wave's stage.
__device__ __forceinline__ void stage_row(const GwArgs& a, uint64_t r, GwStage& S, uint32_t k) {
  const magot_gffrow row = a.rows[r];
  const GwAux x = a.aux[r];
  const uint32_t kind = row.kind & 0xffu;
  const bool has_parent = (row.kind & MAGOT_GFFROW_HAS_PARENT) != 0;
  const bool made = kind == MAGOT_GFFROW_MADE_PARENT;
  const uint8_t* line = a.text + row.line_off;
  uint8_t* sc = S.scratch[k];
  uint64_t* src = S.src[k];
  uint32_t len[kGwSegs];
  // 0: c1 with its tab
  src[0] = row.line_off;
  len[0] = x.tab[0] + 1;
  // 1: c2 with its tab, or "."
  if (made) {
    src[1] = kGwLds | 0;
    len[1] = put(sc, ".\t", 2);
  } else {
    src[1] = row.line_off + x.tab[0] + 1;
    len[1] = x.tab[1] - x.tab[0];
  }
  // 2: c3 with its tab, "exon", or the made parent's type (its tab leads segment 3)
  if (made) {
    src[2] = row.type_off;
    len[2] = row.type_len;
  } else if (kind == MAGOT_GFFROW_EXON_TWIN) {
    src[2] = kGwLds | 0;
    len[2] = put(sc, "exon\t", 5);
  } else {
    src[2] = row.line_off + x.tab[1] + 1;
    len[2] = x.tab[2] - x.tab[1];
  }
  // 3: lo, hi and the score, a tab behind each
  {
    uint8_t* p = sc + 8;
    uint32_t n = 0;
    if (made) p[n++] = '\t';
    n += dec_put(p + n, row.lo);
    p[n++] = '\t';
    n += dec_put(p + n, row.hi);
    p[n++] = '\t';
    if (x.flags & kGwScoreNum) {
      if (x.flags & kGwScoreNeg) p[n++] = '-';
      if (x.int_len)
        for (uint32_t i = 0; i < x.int_len; ++i) p[n++] = line[x.int_off + i];
      else
        p[n++] = '0';
      p[n++] = '.';
      if (x.frac_len)
        for (uint32_t i = 0; i < x.frac_len; ++i) p[n++] = line[x.frac_off + i];
      else
        p[n++] = '0';
    } else {
      p[n++] = '.';
    }
    p[n++] = '\t';
    src[3] = kGwLds | 8;
    len[3] = n;
  }
  // 4: c7 with its tab
  src[4] = row.line_off + x.tab[5] + 1;
  len[4] = x.tab[6] - x.tab[5];
  // 5: the phase, its tab, and what leads the ID
  {
    uint8_t* p = sc + 88;
    uint32_t n = 0;
    p[n++] = (x.flags & kGwPhase) ? line[x.tab[6] + 1] : (uint8_t)'.';
    p[n++] = '\t';
    n += kind == MAGOT_GFFROW_GTF         ? put(p + n, "transcript_id ", 14)
         : kind == MAGOT_GFFROW_EXON_TWIN ? put(p + n, "ID=ExonOf", 9)
                                          : put(p + n, "ID=", 3);
    src[5] = kGwLds | 88;
    len[5] = n;
  }
  src[6] = row.id_off;
  len[6] = row.id_len;
  src[7] = kGwLds | 104;
  len[7] = !has_parent                  ? 0
           : kind == MAGOT_GFFROW_GTF ? put(sc + 104, ";gene_id ", 9)
                                      : put(sc + 104, ";Parent=", 8);
  src[8] = row.parent_off;
  len[8] = has_parent ? row.parent_len : 0;
  sc[116] = '\n';
  src[9] = kGwLds | 116;
  len[9] = 1;
  uint32_t e = 0;
  for (int s = 0; s < kGwSegs; ++s) {
    e += len[s];
    S.end[k][s] = e;
  }
}

__global__ __launch_bounds__(kGwThreads) void render_kernel(GwArgs a, uint8_t* __restrict__ out) {
  __shared__ GwStage stage[kGwWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  GwStage& S = stage[wave];
  const uint64_t g0 = ((uint64_t)blockIdx.x * kGwWaves + wave) * kGwGroup;
  const uint32_t m = g0 >= a.n_rows ? 0u
                                    : (uint32_t)(a.n_rows - g0 < kGwGroup ? a.n_rows - g0 : kGwGroup);
  if (lane <= m && m) S.rowoff[lane] = a.off[g0 + lane];
  if (lane < m) stage_row(a, g0 + lane, S, lane);
  __syncthreads();
  if (!m) return;
  const uint64_t A = S.rowoff[0], B = S.rowoff[m];
  const uint64_t a0 = A & ~15ull;
  const uint64_t n_chunks = (B - a0 + 15) >> 4;
  for (uint64_t c = lane; c < n_chunks; c += 64) {
    const uint64_t x0 = a0 + 16 * c;
    const uint64_t lo = x0 < A ? A : x0, hi = x0 + 16 > B ? B : x0 + 16;
    if (lo >= hi) continue;
    // the row that holds byte lo: the last k with rowoff[k] <= lo
    uint32_t k = 0;
    for (uint32_t step = kGwGroup / 2; step; step >>= 1)
      if (k + step < m && S.rowoff[k + step] <= lo) k += step;
    uint32_t pos = (uint32_t)(lo - S.rowoff[k]);  // within the row
    uint32_t s = 0;
    while (s < kGwSegs - 1 && S.end[k][s] <= pos) ++s;  // pos < end[k][9]: the row holds the byte
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint64_t x = lo; x < hi; ++x) {
      const uint32_t begin = s ? S.end[k][s - 1] : 0u;
      const uint64_t from = S.src[k][s];
      const uint64_t at = (from & ~kGwLds) + (pos - begin);
      // the host checked every reference: the bounds below never bite
      const uint32_t byte = (from & kGwLds)         ? S.scratch[k][at & (kGwScratch - 1)]
                            : at < a.n              ? a.text[at]
                            : at - a.n < a.blob_len ? a.blob[at - a.n]
                                                    : 0u;
      const uint32_t j = (uint32_t)(x - x0);
      w[j >> 2] |= byte << (8 * (j & 3));
      ++pos;
      while (s < kGwSegs && S.end[k][s] <= pos) ++s;
      if (s == kGwSegs) {  // the row is through
        ++k;
        pos = 0;
        s = 0;
        if (k < m)
          while (s < kGwSegs - 1 && S.end[k][s] == 0) ++s;
      }
    }
    if (hi - lo == 16) {
      *reinterpret_cast<uint4*>(out + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (uint64_t x = lo; x < hi; ++x) {
        const uint32_t j = (uint32_t)(x - x0);
        out[x] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
      }
    }
  }
}

}  // namespace

hipError_t launch_gw_size(const GwArgs& a, hipStream_t s) {
  const uint64_t blocks = (a.n_rows + 1 + 255) / 256;
  size_kernel<<<(unsigned)blocks, 256, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_gw_render(const GwArgs& a, uint8_t* out, hipStream_t s) {
  if (!a.n_rows) return hipSuccess;
  const uint64_t groups = (a.n_rows + kGwGroup - 1) / kGwGroup;
  render_kernel<<<(unsigned)((groups + kGwWaves - 1) / kGwWaves), kGwThreads, 0, s>>>(a, out);
  return hipGetLastError();
}

}  // namespace magot
