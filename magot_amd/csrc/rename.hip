// replace_names on the device (genome_tools.py:431-446): every word of a
// resident text that a table names, and that ends at the one-byte delimiter d,
// replaced by the table's value.  The reference tries every key on every line;
// here a line is its fields (what lies between two ds), and under the host's
// conditions (no d inside a name or a value, no chain between two keys: see
// genome_tools.replace_names) a field is rewritten at most once, by the key of
// lowest rank whose name is a suffix of it.
//
//   hash_kernel     one lane per name: a multiplicative hash from the name's
//                   last byte to its first, so that a lane walking left from a d
//                   extends it by one byte at a time; masked to hash_bits.
//   insert_kernel   one lane per name claims a slot of an open-addressing table
//                   (linear probing, one compare-and-swap per probe; the loop is
//                   bounded by the table's size).  A claimed slot whose key has
//                   the same masked hash ends the insertion with
//                   MAGOT_RENAME_HASH_COLLISION: the matcher relies on one name
//                   per masked hash.
//   slots_kernel    one lane per slot: (hash, key, length) in 16 bytes.
//   the d index     textindex.hip's count over the ds, the LFs counted beside
//                   them, and its fill in plain mode: d number j at byte p gives
//                   ix.pos[j] = p.
//   match_kernel    one lane per d.  It walks left over at most max_len bytes
//                   and stops at the previous d, at an LF and at offset 0, so
//                   its cost does not depend on the field's or the line's
//                   length.  At every length some name has, it probes the table;
//                   a slot with its hash is the only candidate: length, then
//                   bytes.  A false hit is no hit.  The lowest rank wins.  Then
//                   a scan of the hit flags.
//   compact_kernel  the hits in text order: the d's offset and the key.
//   items_kernel    one lane per hit and one for the text's end: the unchanged
//                   run in front of it cut into pieces of kRnPiece bytes, one
//                   piece for the value, value less name in bytes.  Two scans
//                   give the output offsets (64-bit) and the pieces' numbers.
//   piece_kernel    one lane per piece: a binary search names its hit; source,
//                   destination, length.  The values lie behind the text in one
//                   allocation, so a piece's source is an offset from `text`.
//   the copy        wavecopy.h's launch_piece_copy, as the FASTA reflow's.
// The last output byte is the LF `print` adds after taking the line's last byte.
//
// LDS: the copy's piece table.  No spin-wait; the only compare-and-swap is
// insert_kernel's bounded probe.
#include <hip/hip_runtime.h>

#include "common.h"
#include "wavecopy.h"

namespace magot {
namespace {

constexpr int kRnThreads = 256;
constexpr int kRnGroup = kSpanGroup;  // pieces per wave of the copy

constexpr uint64_t kRnSeed = 0xcbf29ce484222325ull, kRnPrime = 0x100000001b3ull;
constexpr uint64_t kRnSpread = 0x9E3779B97F4A7C15ull;

inline unsigned rn_blocks_for(uint64_t n) { return (unsigned)((n + kRnThreads - 1) / kRnThreads); }

__device__ __forceinline__ uint64_t rn_mask(uint32_t bits) {
  return bits >= 64 ? ~0ull : (1ull << bits) - 1;
}
__device__ __forceinline__ uint64_t rn_hash_byte(uint64_t h, uint32_t c) {
  return (h ^ c) * kRnPrime;
}
__device__ __forceinline__ uint64_t rn_home(const RnArgs& a, uint64_t masked) {
  return (masked * kRnSpread) >> a.slot_shift;  // below cap
}

__global__ __launch_bounds__(kRnThreads) void rn_hash_kernel(RnArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (k >= a.n_keys) return;
  const uint64_t off = a.name_off[k];
  const uint32_t len = (uint32_t)(a.name_off[k + 1] - off);  // the host checked: 1..kRnMaxName
  uint64_t h = kRnSeed;
  for (uint32_t i = len; i; --i) h = rn_hash_byte(h, a.names[off + i - 1]);
  a.key_hash[k] = h & rn_mask(a.hash_bits);
}

__global__ __launch_bounds__(kRnThreads) void rn_insert_kernel(RnArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (k >= a.n_keys) return;
  const uint64_t h = a.key_hash[k];
  uint64_t s = rn_home(a, h);
  for (uint64_t tries = 0; tries < a.cap; ++tries, s = (s + 1) & (a.cap - 1)) {
    const uint32_t prev = atomicCAS(&a.claim[s], kRnNoKey, (uint32_t)k);
    if (prev == kRnNoKey) return;
    if (a.key_hash[prev] == h) {  // prev is a key, below n_keys
      atomicMin(a.status, (unsigned long long)MAGOT_RENAME_HASH_COLLISION);
      return;
    }
  }
}

__global__ __launch_bounds__(kRnThreads) void rn_slots_kernel(RnArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (s >= a.cap) return;
  const uint32_t k = a.claim[s];
  RnSlot slot{0, kRnNoKey, 0};
  if (k != kRnNoKey) {
    slot.hash = a.key_hash[k];
    slot.key = k;
    slot.len = (uint32_t)(a.name_off[k + 1] - a.name_off[k]);
  }
  a.slots[s] = slot;
}

__device__ __forceinline__ bool rn_len_present(const RnArgs& a, uint32_t len) {
  const uint32_t b = len - 1;
  uint64_t w = a.len_mask[0];
#pragma unroll
  for (uint32_t q = 1; q < kRnMaxName / 64; ++q) w = (b >> 6) == q ? a.len_mask[q] : w;
  return (w >> (b & 63)) & 1;
}

__global__ __launch_bounds__(kRnThreads) void rn_match_kernel(RnArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (j > a.n_fields) return;
  if (j == a.n_fields) {  // the scan's last entry: the hits
    a.f_hit[j] = 0;
    return;
  }
  const uint64_t p = a.ix.pos[j];  // below n
  const uint32_t lim = (uint32_t)(p < a.max_len ? p : a.max_len);
  const uint64_t mask = rn_mask(a.hash_bits);
  uint64_t h = kRnSeed;
  uint32_t best = kRnNoKey, best_rank = 0xffffffffu;
  uint32_t next = lim ? a.ix.text[p - 1] : 0;
  for (uint32_t i = 1; i <= lim; ++i) {
    const uint32_t c = next;
    if (c == a.ix.byte || c == '\n') break;
    if (i < lim) next = a.ix.text[p - i - 1];  // in flight while this length is probed
    h = rn_hash_byte(h, c);
    if (!rn_len_present(a, i)) continue;
    const uint64_t hm = h & mask;
    uint64_t s = rn_home(a, hm);
    // at most a quarter of the slots is taken, so an empty one ends the probe
    for (uint64_t tries = 0; tries < a.cap; ++tries, s = (s + 1) & (a.cap - 1)) {
      const RnSlot slot = a.slots[s];
      if (slot.key == kRnNoKey) break;
      if (slot.hash != hm) continue;
      // the one name with this masked hash
      bool same = slot.len == i;
      const uint8_t* name = a.names + a.name_off[slot.key];
      for (uint32_t q = 0; q < i && same; ++q) same = name[q] == a.ix.text[p - i + q];
      if (same) {
        const uint32_t r = a.rank[slot.key];
        if (r < best_rank) {
          best_rank = r;
          best = slot.key;
        }
      }
      break;
    }
  }
  a.f_key[j] = best;
  a.f_hit[j] = best != kRnNoKey ? 1 : 0;
}

__global__ __launch_bounds__(kRnThreads) void rn_compact_kernel(RnArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (j >= a.n_fields || !a.f_hit[j]) return;
  const uint64_t k = a.f_hpos[j];  // below n_hits
  a.h_end[k] = a.ix.pos[j];
  a.h_key[k] = a.f_key[j];
}

// hit k's unchanged run [*from, *from + *run): from the d of the hit before it
// (the text's start) to its name; for k = n_hits to the text's end
__device__ __forceinline__ void rn_run(const RnArgs& a, uint64_t k, uint64_t* from, uint64_t* run,
                                       uint64_t* name_len, uint64_t* val_len) {
  *from = k ? a.h_end[k - 1] : 0;
  *name_len = *val_len = 0;
  uint64_t to = a.ix.n;
  if (k < a.n_hits) {
    const uint32_t key = a.h_key[k];
    *name_len = a.name_off[key + 1] - a.name_off[key];
    *val_len = a.val_off[key + 1] - a.val_off[key];
    to = a.h_end[k] - *name_len;  // the name lies behind the d before it: to >= *from
  }
  *run = to - *from;
}

__global__ __launch_bounds__(kRnThreads) void rn_items_kernel(RnArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (k > a.n_hits + 1) return;
  if (k == a.n_hits + 1) {
    a.h_pcnt[k] = 0;
    return;
  }
  uint64_t from, run, name_len, val_len;
  rn_run(a, k, &from, &run, &name_len, &val_len);
  a.h_delta[k] = val_len - name_len;
  a.h_pcnt[k] = (run + kRnPiece - 1) / kRnPiece + (k < a.n_hits ? 1 : 0);
}

// the last i in [lo, hi) with v[i] <= x (v non-decreasing, v[lo] <= x)
__device__ __forceinline__ uint64_t rn_last_le(const uint64_t* __restrict__ v, uint64_t lo,
                                               uint64_t hi, uint64_t x) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kRnThreads) void rn_piece_kernel(RnArgs a, RnRenderArgs o) {
  const uint64_t t = (uint64_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (t >= o.n_pieces) return;
  // h_pbase[0] = 0 <= t < h_pbase[n_hits + 1]; an item without a piece shares its successor's entry
  const uint64_t k = rn_last_le(a.h_pbase, 0, a.n_hits + 1, t);
  const uint64_t q = t - a.h_pbase[k];
  uint64_t from, run, name_len, val_len;
  rn_run(a, k, &from, &run, &name_len, &val_len);
  const uint64_t run_pieces = (run + kRnPiece - 1) / kRnPiece;
  const uint64_t shift = a.h_dsum[k];  // mod 2^64, as every destination
  if (q < run_pieces) {
    const uint64_t at = from + q * kRnPiece, left = run - q * kRnPiece;
    o.p_src[t] = at;
    o.p_dst[t] = at + shift;
    o.p_len[t] = (uint32_t)(left < kRnPiece ? left : kRnPiece);
  } else {  // the value, in the name's place (k < n_hits)
    o.p_src[t] = a.val_base + a.val_off[a.h_key[k]];
    o.p_dst[t] = from + run + shift;
    o.p_len[t] = (uint32_t)val_len;
  }
}

}  // namespace

hipError_t launch_rn_table(const RnArgs& a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.claim, 0xff, a.cap * sizeof(uint32_t), s)) return e;
  if (a.n_keys) {
    rn_hash_kernel<<<rn_blocks_for(a.n_keys), kRnThreads, 0, s>>>(a);
    if (hipError_t e = hipGetLastError()) return e;
    rn_insert_kernel<<<rn_blocks_for(a.n_keys), kRnThreads, 0, s>>>(a);
    if (hipError_t e = hipGetLastError()) return e;
  }
  rn_slots_kernel<<<rn_blocks_for(a.cap), kRnThreads, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_rn_match(const RnArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  rn_match_kernel<<<rn_blocks_for(a.n_fields + 1), kRnThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  return exclusive_sum(tmp, tmp_bytes, a.f_hit, a.f_hpos, a.n_fields + 1, s);
}

hipError_t launch_rn_layout(const RnArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s) {
  if (a.n_hits) {
    rn_compact_kernel<<<rn_blocks_for(a.n_fields), kRnThreads, 0, s>>>(a);
    if (hipError_t e = hipGetLastError()) return e;
  }
  rn_items_kernel<<<rn_blocks_for(a.n_hits + 2), kRnThreads, 0, s>>>(a);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = exclusive_sum(tmp, tmp_bytes, a.h_delta, a.h_dsum, a.n_hits + 1, s)) return e;
  return exclusive_sum(tmp, tmp_bytes, a.h_pcnt, a.h_pbase, a.n_hits + 2, s);
}

hipError_t launch_rn_render(const RnArgs& a, const RnRenderArgs& r, hipStream_t s) {
  if (!r.n_pieces) return hipSuccess;
  rn_piece_kernel<<<rn_blocks_for(r.n_pieces), kRnThreads, 0, s>>>(a, r);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = launch_piece_copy<kRnGroup>(r.p_src, r.p_dst, r.p_len, r.n_pieces, a.ix.text,
                                                 r.out, s))
    return e;
  return hipMemsetAsync(r.out + r.out_bytes - 1, '\n', 1, s);  // n > 0 gives out_bytes > 0
}

}  // namespace magot
