// ORF calling on device (dna2orfs, genome_tools.py:145-180): the six-frame
// streams an executed magot_orf6 left in HBM are split at their stops into an
// ORF table, a concatenated payload and, on request, the tool's FASTA text.
// The residues never visit the host.
//
// Order.  ORFs are numbered in the reference's loop order: record, then
// stream j = 2*frame + (strand == '+') (0-, 0+, 1-, 1+, 2-, 2+), then position
// in the stream.  That is the index order of the stream_off table, not the
// order of the streams in memory (strand-major blocks, in the six-frame
// kernel's own walk order): every stream is found through its offset, so the
// tables come out in the plan's record order whatever the layout.
//
// Tiles.  A non-None stream is cut into tiles of kOrfCallTile residues (one
// 16-byte chunk per lane of a wave; an empty stream has one empty tile), a
// None stream (len <= 2 + frame) has none and flags its record.  A frame-0
// stream loses one leading 'X' (trimX, genome.py:819-821): lane 0 of its first
// tile masks that byte off, and residue indices count from the trimmed start.
// An ORF belongs to the tile that holds the stop before it (ORF 0 of a stream
// to the stream's first tile), so a tile owns stops + [first tile] ORFs and no
// tile needs to know where an ORF ends: its length is the distance to the next
// ORF's payload offset.
//
// State carried across tiles.  An ORF may span any number of tiles.  The
// default output drops the stops and keeps everything else, so a tile's output
// size is its own.  from_atg ('M' + what follows the ORF's first M, further Ms
// removed; 'M' alone without one) needs one bit at a tile's start: has the
// ORF running into it already had its M?  The count pass sizes a tile both
// ways and leaves two flags (a stop in the tile; an M after its last stop);
// the resolve pass walks back over the stream's earlier tiles to the nearest
// one with either flag and picks the size.  Every stop emits the 'M' of the
// ORF that follows it, and a stream's first tile one more in front.
//
// Passes (all on the context stream):
//   stream_tiles  per stream: tile count, None flag          -> scan
//   fill_tiles    per stream: its tiles' stream index
//   count         per tile (one wave): ORFs, output bytes    \  scans give each
//   resolve       per tile: from_atg carry (walk back)       /  tile's bases
//   write         per tile: table rows; the output compacted in LDS at the
//                 destination's 16-byte phase, stored as 16-byte chunks
//   lens          per ORF: payload_off[i + 1] - payload_off[i]
//   longest       per record (one block): arg-max on (length, earliest index),
//                 then a compaction of the chosen rows and their payload
//   text          per ORF: sizes incl. the decimal position -> scan; then the
//                 grouped span copy of wavecopy.h over two pieces per ORF
//                 (header | digits + payload)
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "wavecopy.h"

namespace magot {
namespace {

constexpr uint32_t kT = kOrfCallTile;
static_assert(kT == 64 * 16, "one 16-byte chunk per lane");
constexpr int kStageVecs = (16 + kT + 1 + 15) / 16 + 1;  // phase + tile + leading 'M'

struct TileCtx {
  uint32_t g, r, j, ti, k0, c, trim;
  uint64_t soff;
};

// residues of stream j of a record of L bases (magot_orf6_sizes); None: ~0u
__device__ __forceinline__ uint32_t stream_residues(uint64_t L, uint32_t j) {
  const uint32_t f = j >> 1;
  if (L <= 2 + f) return ~0u;
  return L >= 2 * f + 3 ? (uint32_t)((L - 2 * f) / 3) : 0u;
}

__device__ __forceinline__ TileCtx tile_ctx(const OrfCallArgs& a, uint64_t t) {
  TileCtx x;
  x.g = a.tile_stream[t];
  x.r = x.g / 6;
  x.j = x.g - 6 * x.r;
  x.c = stream_residues(a.noff[x.r + 1] - a.noff[x.r], x.j);
  x.ti = (uint32_t)(t - a.tile_first[x.g]);
  x.k0 = x.ti * kT;
  x.soff = a.soff[x.g];
  x.trim = (x.j < 2 && x.c > 0 && a.res[x.soff] == 'X') ? 1u : 0u;
  return x;
}

// this lane's 16 residues of the tile: the chunk, and bit masks of its valid
// bytes, its stops and its Ms (valid bytes only)
__device__ __forceinline__ void lane_chunk(const OrfCallArgs& a, const TileCtx& x, uint32_t lane,
                                           uint32_t w[4], uint32_t* vm, uint32_t* stop,
                                           uint32_t* mm) {
  const uint32_t pos = x.k0 + 16 * lane;
  const uint32_t nv = pos < x.c ? (x.c - pos < 16 ? x.c - pos : 16u) : 0u;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (nv) v = *reinterpret_cast<const uint4*>(a.res + x.soff + pos);  // inside pad16(c)
  w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  uint32_t valid = nv == 16 ? 0xFFFFu : (1u << nv) - 1u;
  if (x.trim && pos == 0) valid &= ~1u;
  uint32_t s = 0, m = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 255u;
    s |= (c == '*' ? 1u : 0u) << i;
    m |= (c == 'M' ? 1u : 0u) << i;
  }
  *vm = valid;
  *stop = s & valid;
  *mm = m & valid;
}

// bytes this lane emits: default, every valid residue but the stops; from_atg,
// an 'M' per stop and the other residues while the running ORF has had its M
template <bool ATG>
__device__ __forceinline__ uint32_t emit_count(uint32_t vm, uint32_t stop, uint32_t mm, bool seen) {
  if (!ATG) return (uint32_t)__popc(vm & ~stop);
  uint32_t n = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t bit = 1u << i;
    if (!(vm & bit)) continue;
    if (stop & bit) {
      ++n;
      seen = false;
    } else if (mm & bit) {
      seen = true;
    } else if (seen) {
      ++n;
    }
  }
  return n;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan(v), 63);
}

// inclusive running maximum over the lanes of a wave
__device__ __forceinline__ int wave_max_scan(int v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if ((int)lane >= d) v = o > v ? o : v;
  }
  return v;
}

// positions (in the tile) of the last stop and the last M before this lane's
// chunk (-1: none), and of the tile's last ones
__device__ __forceinline__ void last_marks(uint32_t stop, uint32_t mm, uint32_t lane, int* in_s,
                                           int* in_m, int* all_s, int* all_m) {
  const int ls = stop ? (int)(16 * lane + 31 - __clz((int)stop)) : -1;
  const int lm = mm ? (int)(16 * lane + 31 - __clz((int)mm)) : -1;
  const int is = wave_max_scan(ls, lane), im = wave_max_scan(lm, lane);
  const int ps = __shfl_up(is, 1), pm = __shfl_up(im, 1);
  *in_s = lane ? ps : -1;
  *in_m = lane ? pm : -1;
  *all_s = __shfl(is, 63);
  *all_m = __shfl(im, 63);
}

constexpr uint8_t kTileStop = 1;    // the tile holds a stop
constexpr uint8_t kTileMAfter = 2;  // an M after its last stop (anywhere, without a stop)

__global__ void stream_tiles_kernel(OrfCallArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 6 * a.n_rec) return;
  const uint64_t r = g / 6;
  const uint32_t c = stream_residues(a.noff[r + 1] - a.noff[r], (uint32_t)(g - 6 * r));
  if (c == ~0u) {
    a.scnt[g] = 0;
    a.flags[r] = kOrfFlagNone;  // the same byte from every None stream of the record
  } else {
    a.scnt[g] = c ? (c + kT - 1) / kT : 1u;
  }
}

__global__ void fill_tiles_kernel(OrfCallArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 6 * a.n_rec) return;
  const uint64_t t0 = a.tile_first[g], t1 = a.tile_first[g + 1];
  for (uint64_t t = t0; t < t1; ++t) a.tile_stream[t] = (uint32_t)g;
}

template <bool ATG>
__global__ __launch_bounds__(256) void orf_count_kernel(OrfCallArgs a) {
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t t = (uint64_t)blockIdx.x * 4 + wv;
  if (t >= a.n_tiles) return;
  const TileCtx x = tile_ctx(a, t);
  uint32_t w[4], vm, stop, mm;
  lane_chunk(a, x, lane, w, &vm, &stop, &mm);
  const uint32_t first = x.ti == 0 ? 1u : 0u;
  const uint32_t ns = wave_sum((uint32_t)__popc(stop));
  if (!ATG) {
    const uint32_t kept = wave_sum(emit_count<false>(vm, stop, mm, false));
    if (lane == 0) {
      a.orfs[t] = ns + first;
      a.kept[t] = kept;
    }
    return;
  }
  int in_s, in_m, all_s, all_m;
  last_marks(stop, mm, lane, &in_s, &in_m, &all_s, &all_m);
  // sized twice: the ORF running into the tile without its M yet, and with it
  const bool seen_u = in_m > in_s;
  const bool seen_s = in_s < 0 ? true : seen_u;
  const uint32_t ku = wave_sum(emit_count<true>(vm, stop, mm, seen_u));
  const uint32_t ks = wave_sum(emit_count<true>(vm, stop, mm, seen_s));
  if (lane == 0) {
    a.orfs[t] = ns + first;
    a.kept[t] = ku + first;  // a stream's first tile opens ORF 0 with its 'M'
    a.extra[t] = ks - ku;
    a.tflags[t] = (uint8_t)((all_s >= 0 ? kTileStop : 0) | (all_m > all_s ? kTileMAfter : 0));
  }
}

// from_atg: has the ORF running into tile t had its M?  Walk back over the
// stream's earlier tiles to the nearest with a stop or an M.
__global__ void orf_resolve_kernel(OrfCallArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_tiles) return;
  const uint64_t t0 = a.tile_first[a.tile_stream[t]];
  bool seen = false;
  for (uint64_t q = t; q > t0;) {
    const uint8_t f = a.tflags[--q];
    if (f & kTileMAfter) seen = true;
    if (f) break;
  }
  a.tseen[t] = seen ? 1 : 0;
  if (seen) a.kept[t] += a.extra[t];
}

template <bool ATG>
__global__ __launch_bounds__(256) void orf_write_kernel(OrfCallArgs a) {
  __shared__ uint4 stage[4][kStageVecs];
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t t = (uint64_t)blockIdx.x * 4 + wv;
  if (t >= a.n_tiles) return;
  const TileCtx x = tile_ctx(a, t);
  uint32_t w[4], vm, stop, mm;
  lane_chunk(a, x, lane, w, &vm, &stop, &mm);
  const uint64_t pb = a.kbase[t], ob = a.obase[t];
  const uint32_t K = (uint32_t)(a.kbase[t + 1] - pb);
  const uint32_t first = x.ti == 0 ? 1u : 0u;
  bool seen = false;
  if (ATG) {
    int in_s, in_m, all_s, all_m;
    last_marks(stop, mm, lane, &in_s, &in_m, &all_s, &all_m);
    seen = in_s < 0 ? (a.tseen[t] != 0 || in_m >= 0) : in_m > in_s;
  }
  const uint32_t e = emit_count<ATG>(vm, stop, mm, seen);
  const uint32_t ns = (uint32_t)__popc(stop);
  const uint32_t packed = e | (ns << 16);  // both sums <= kT
  const uint32_t sc = wave_scan(packed) - packed;
  // the tile's output, at its destination's phase inside a 16-byte chunk
  uint8_t* const S = reinterpret_cast<uint8_t*>(stage[wv]) + (pb & 15);
  uint32_t eo = (sc & 0xFFFFu) + (ATG ? first : 0u);
  uint64_t oi = ob + first + (sc >> 16);
  if (first && lane == 0) {  // ORF 0 of the stream
    if (ATG) S[0] = 'M';
    a.rec[ob] = x.r;
    a.j[ob] = (uint8_t)x.j;
    a.k[ob] = 0;
    a.poff[ob] = pb;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t bit = 1u << i;
    if (!(vm & bit)) continue;
    const uint8_t c = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
    if (stop & bit) {  // the ORF after this stop
      a.rec[oi] = x.r;
      a.j[oi] = (uint8_t)x.j;
      a.k[oi] = x.k0 + 16 * lane + i - x.trim + 1;
      a.poff[oi] = pb + eo;
      ++oi;
      if (ATG) {
        S[eo++] = 'M';
        seen = false;
      }
    } else if (ATG) {
      if (mm & bit) seen = true;
      else if (seen) S[eo++] = c;
    } else {
      S[eo++] = c;
    }
  }
  __builtin_amdgcn_wave_barrier();
  // [pb, pb + K): head bytes up to the first 16-byte boundary, whole chunks,
  // tail bytes; every byte is this tile's alone
  const uint64_t end = pb + K, base16 = pb & ~15ull;
  const uint64_t a16 = (pb + 15) & ~15ull;
  const uint8_t* const S0 = reinterpret_cast<const uint8_t*>(stage[wv]);  // global byte base16
  if (a16 >= end) {
    if (lane < K) a.payload[pb + lane] = S0[pb - base16 + lane];
    return;
  }
  const uint32_t head = (uint32_t)(a16 - pb);
  const uint32_t nw = (uint32_t)((end - a16) >> 4);
  const uint64_t g = a16 + 16ull * nw;
  if (lane < head) a.payload[pb + lane] = S0[pb - base16 + lane];
  for (uint32_t q = lane; q < nw; q += 64)
    *reinterpret_cast<uint4*>(a.payload + a16 + 16ull * q) =
        *reinterpret_cast<const uint4*>(S0 + (a16 - base16) + 16ull * q);
  if (lane < (uint32_t)(end - g)) a.payload[g + lane] = S0[g - base16 + lane];
}

__global__ void orf_lens_kernel(OrfCallArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_orfs) return;
  const uint64_t e = i + 1 < a.n_orfs ? a.poff[i + 1] : a.kbase[a.n_tiles];
  a.len[i] = (uint32_t)(e - a.poff[i]);
}

// per record: the first ORF in loop order with the greatest output length > 0
__global__ __launch_bounds__(256) void orf_longest_kernel(OrfCallArgs a) {
  __shared__ uint32_t sl[4];
  __shared__ uint64_t si[4];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x / 64;
  for (uint64_t r = blockIdx.x; r < a.n_rec; r += gridDim.x) {
    const uint64_t b = a.obase[a.tile_first[6 * r]], e = a.obase[a.tile_first[6 * r + 6]];
    uint32_t bl = 0;
    uint64_t bi = ~0ull;
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) {
      const uint32_t l = a.len[i];
      if (l > bl) bl = l, bi = i;  // ascending i: a tie keeps the earlier one
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      const uint32_t ol = __shfl_down(bl, d);
      const uint64_t oi = __shfl_down(bi, d);
      if (ol > bl || (ol == bl && oi < bi)) bl = ol, bi = oi;
    }
    if (lane == 0) sl[wv] = bl, si[wv] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < 4; ++q)
        if (sl[q] > bl || (sl[q] == bl && si[q] < bi)) bl = sl[q], bi = si[q];
      uint8_t f = a.flags[r];
      if (!(f & kOrfFlagNone) && bl == 0) a.flags[r] = (f |= kOrfFlagNoLongest);
      const bool ok = f == 0;
      a.sel[r] = bi;
      a.valid[r] = ok ? 1u : 0u;
      a.sellen[r] = ok ? bl : 0u;
    }
    __syncthreads();
  }
}

__global__ void orf_compact_kernel(OrfCallArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_rec) return;
  if (r == 0) a.dst_off[a.slot[a.n_rec]] = a.cpoff[a.n_rec];
  if (!a.valid[r]) return;
  const uint64_t e = a.slot[r], s = a.sel[r];
  a.c_rec[e] = (uint32_t)r;
  a.c_j[e] = a.j[s];
  a.c_k[e] = a.k[s];
  a.c_len[e] = a.len[s];
  a.c_poff[e] = a.cpoff[r];
  a.src_off[e] = a.poff[s];
  a.dst_off[e] = a.cpoff[r];
}

// --- text ------------------------------------------------------------------

// the reference's orf_start: frame on '+', len - frame on '-', plus 3 per residue
__device__ __forceinline__ uint64_t orf_position(const OrfTextArgs& a, uint64_t i) {
  const uint32_t r = a.rec[i], j = a.j[i], f = j >> 1;
  const uint64_t L = a.noff[r + 1] - a.noff[r];
  return ((j & 1) ? (uint64_t)f : L - f) + 3ull * a.k[i];
}

__device__ __forceinline__ uint32_t decimal_width(uint64_t v) {
  uint32_t n = 1;
  while (v >= 10) v /= 10, ++n;
  return n;
}

// header text of record r is stored as '\n' + header: an entry's header piece
// carries the newline that ends the entry before it
__global__ void orftext_len_kernel(OrfTextArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t r = a.rec[i];
  uint32_t n = (uint32_t)(a.hoff[r + 1] - a.hoff[r] - 1) + a.len[i] + 1;
  if (!a.longest) {
    uint64_t v = orf_position(a, i);
    const uint32_t nd = decimal_width(v);
    uint8_t* d = a.text + a.dig_off + kOrfDigits * i;
    for (uint32_t q = nd; q--; v /= 10) d[q] = (uint8_t)('0' + v % 10);
    d[nd] = '\n';
    n += nd + 1;
  }
  a.tlen[i] = n;
}

__global__ __launch_bounds__(256) void orftext_copy_kernel(OrfTextArgs a) {
  __shared__ SpanGroup lds[256 / 64];
  constexpr uint32_t kPer = kSpanGroup / 2;  // entries per wave, two pieces each
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i0 = ((uint64_t)blockIdx.x * 4 + wv) * kPer;
  if (i0 >= a.n) return;
  const uint32_t ne = (uint32_t)(a.n - i0 < kPer ? a.n - i0 : kPer);
  const uint32_t m = 2 * ne;
  SpanGroup& L = lds[wv];
  if (lane < m) {
    const uint64_t i = i0 + lane / 2;
    const uint32_t r = a.rec[i];
    const uint64_t ts = a.tstart[i];
    const uint64_t hl = a.hoff[r + 1] - a.hoff[r] - 1;
    if (!(lane & 1)) {  // the newline of the entry before, and the header
      const uint64_t nl = i ? 1 : 0;
      L.o[lane] = ts - nl;
      L.te[lane] = ts + hl;
      L.toff[lane] = a.hoff[r] + 1 - nl;
      L.src[lane] = 0;
    } else {  // the digits and their newline, then the payload
      const uint64_t dl = a.longest ? 0 : decimal_width(orf_position(a, i)) + 1;
      L.o[lane] = ts + hl;
      L.te[lane] = ts + hl + dl;
      L.toff[lane] = a.dig_off + kOrfDigits * i;
      L.src[lane] = a.poff[i];
      if (lane == m - 1) L.o[m] = a.tstart[i + 1] - 1;
    }
  }
  __builtin_amdgcn_wave_barrier();
  span_group_copy(L, m, a.text, a.payload, a.out, lane);
  if (i0 + ne == a.n && lane == 0) a.out[a.tstart[a.n] - 1] = '\n';  // the last entry's
}

inline unsigned blocks_of(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }

hipError_t scan_u32(void* tmp, size_t bytes, const uint32_t* in, uint64_t* out, uint64_t n,
                    hipStream_t s) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, uint64_t(0), (size_t)n,
                                 rocprim::plus<uint64_t>(), s);
}

}  // namespace

size_t orfcall_scan_bytes(uint64_t n) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t*)nullptr, (uint64_t*)nullptr,
                                uint64_t(0), (size_t)n, rocprim::plus<uint64_t>(),
                                hipStream_t(0));
  return bytes;
}

// tile counts per stream and their prefix (6n + 1: the last one the total)
hipError_t launch_orfcall_streams(const OrfCallArgs& a, hipStream_t s) {
  const uint64_t ns = 6 * a.n_rec;
  if (hipError_t e = hipMemsetAsync(a.flags, 0, a.n_rec ? a.n_rec : 1, s)) return e;
  if (hipError_t e = hipMemsetAsync(a.scnt + ns, 0, 4, s)) return e;
  if (ns) stream_tiles_kernel<<<blocks_of(ns, 256), 256, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return scan_u32(a.scan_tmp, a.scan_bytes, a.scnt, a.tile_first, ns + 1, s);
}

// per tile: ORFs and output bytes, and their prefixes (n_tiles + 1)
hipError_t launch_orfcall_count(const OrfCallArgs& a, hipStream_t s) {
  const bool atg = a.mode & MAGOT_ORF_FROM_ATG;
  if (hipError_t e = hipMemsetAsync(a.orfs + a.n_tiles, 0, 4, s)) return e;
  if (hipError_t e = hipMemsetAsync(a.kept + a.n_tiles, 0, 4, s)) return e;
  if (a.n_tiles) {
    fill_tiles_kernel<<<blocks_of(6 * a.n_rec, 256), 256, 0, s>>>(a);
    if (atg) {
      orf_count_kernel<true><<<blocks_of(a.n_tiles, 4), 256, 0, s>>>(a);
      orf_resolve_kernel<<<blocks_of(a.n_tiles, 256), 256, 0, s>>>(a);
    } else {
      orf_count_kernel<false><<<blocks_of(a.n_tiles, 4), 256, 0, s>>>(a);
    }
  }
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = scan_u32(a.scan_tmp, a.scan_bytes, a.orfs, a.obase, a.n_tiles + 1, s))
    return e;
  return scan_u32(a.scan_tmp, a.scan_bytes, a.kept, a.kbase, a.n_tiles + 1, s);
}

hipError_t launch_orfcall_write(const OrfCallArgs& a, hipStream_t s) {
  if (!a.n_tiles) return hipSuccess;
  if (a.mode & MAGOT_ORF_FROM_ATG)
    orf_write_kernel<true><<<blocks_of(a.n_tiles, 4), 256, 0, s>>>(a);
  else
    orf_write_kernel<false><<<blocks_of(a.n_tiles, 4), 256, 0, s>>>(a);
  if (a.n_orfs) orf_lens_kernel<<<blocks_of(a.n_orfs, 256), 256, 0, s>>>(a);
  return hipGetLastError();
}

// longest: each record's choice, and the prefixes of the chosen rows / bytes
hipError_t launch_orfcall_longest(const OrfCallArgs& a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.valid + a.n_rec, 0, 4, s)) return e;
  if (hipError_t e = hipMemsetAsync(a.sellen + a.n_rec, 0, 4, s)) return e;
  if (a.n_rec) {
    const uint64_t grid = a.n_rec < (1u << 20) ? a.n_rec : (1u << 20);
    orf_longest_kernel<<<(unsigned)grid, 256, 0, s>>>(a);
  }
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = scan_u32(a.scan_tmp, a.scan_bytes, a.valid, a.slot, a.n_rec + 1, s)) return e;
  return scan_u32(a.scan_tmp, a.scan_bytes, a.sellen, a.cpoff, a.n_rec + 1, s);
}

hipError_t launch_orfcall_compact(const OrfCallArgs& a, hipStream_t s) {
  if (!a.n_rec) return hipSuccess;
  orf_compact_kernel<<<blocks_of(a.n_rec, 256), 256, 0, s>>>(a);
  launch_segments_copy(a.payload, a.src_off, a.dst_off, a.n_sel, a.c_payload, s);
  return hipGetLastError();
}

// per entry text sizes (and the digits), and their prefix (n + 1)
hipError_t launch_orftext_sizes(const OrfTextArgs& a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.tlen + a.n, 0, 4, s)) return e;
  if (a.n) orftext_len_kernel<<<blocks_of(a.n, 256), 256, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return scan_u32(a.scan_tmp, a.scan_bytes, a.tlen, a.tstart, a.n + 1, s);
}

hipError_t launch_orftext_copy(const OrfTextArgs& a, hipStream_t s) {
  if (!a.n) return hipSuccess;
  const uint64_t groups = (a.n + kSpanGroup / 2 - 1) / (kSpanGroup / 2);
  orftext_copy_kernel<<<blocks_of(groups, 4), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace magot
