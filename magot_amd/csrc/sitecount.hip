// composition_by_site's counting pass (genome_tools.py:488-503): for every
// site of an alignment, the rows that hold a, t, c or g there.  The rows are
// records of the forward nibble plane, so a cell is a nibble: bit 3 clear means
// ACGTacgt, bits 0-1 the code (A C G T = 0..3); the case bit is not looked at.
// The plane is walked across records: a lane keeps its kSiteLane sites and
// goes down the rows.
//
// Loads.  Site s of a row that starts at base b is base b + s.  A lane's sites
// start at a multiple of 8, so its eight nibbles are the word (b >> 3) + s / 8
// and the next one, shifted right by 4 (b & 7) bits: two aligned 4-byte loads
// and one v_alignbit.  b is the same for the whole wave, so is the shift.
// Lanes of a wave read consecutive words; a lane's second word is its
// neighbour's first and comes from the same cache line.
//
// Bounds.  A lane with a site below n_sites reads bases up to b + s + 15 with
// b + s inside a contig, hence below extent + 15, inside the 64 bases of padding
// every plane ends with (pack.cpp: span = extent + 64 rounded up to 32).  A
// lane with no site reads word 0 and 1.  Nibbles at sites >= n_sites belong to
// the row's tail or to the next record: `keep` clears them from every mask.
//
// Output.  counts[site][a, t, c, g] as one uint4 per site: the tool's column
// order, so the host reads rows as they are printed, and a site's four numbers
// -- always wanted together, the total being their sum -- share 16 bytes.  A
// lane's 32 numbers go through LDS so that every store or atomic instruction
// of a wave covers 256 contiguous bytes.
#include "common.h"

namespace magot {
namespace {

constexpr uint32_t kOnes = 0x11111111u;
constexpr uint32_t kLowNibbles = 0x0f0f0f0fu;
constexpr uint32_t kLdsPitch = 4 * kSiteLane + 1;  // odd: lanes on distinct banks

// the row's cells at the lane's sites into the four 4-bit counter words:
// n (counted at all), c, g, t
__device__ __forceinline__ void site_row(const uint32_t* __restrict__ nib, uint64_t start,
                                         uint64_t lane_word, bool live, uint32_t keep,
                                         uint32_t (&acc)[4]) {
  const uint64_t w = live ? (start >> 3) + lane_word : 0;
  const uint32_t lo = nib[w], hi = nib[w + 1];
  const uint32_t x = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(start & 7) * 4);
  const uint32_t n = ~(x >> 3) & keep;
  const uint32_t p0 = x & n, p1 = (x >> 1) & n;
  const uint32_t t = p0 & p1;
  acc[0] += n;
  acc[1] += p0 ^ t;
  acc[2] += p1 ^ t;
  acc[3] += t;
}

__global__ __launch_bounds__(kSiteBlock) void site_count_kernel(SiteArgs a) {
  __shared__ uint32_t lds[kSiteBlock * kLdsPitch];
  const uint32_t tile = blockIdx.x % a.n_tiles, strip = blockIdx.x / a.n_tiles;
  const uint32_t tid = threadIdx.x;
  const uint64_t site0 = (uint64_t)tile * kSiteTile + (uint64_t)tid * kSiteLane;
  const uint32_t valid =
      site0 < a.n_sites ? (uint32_t)(a.n_sites - site0 < kSiteLane ? a.n_sites - site0 : kSiteLane) : 0;
  const uint32_t keep = valid == kSiteLane ? kOnes : kOnes & ((1u << (4 * valid)) - 1);
  const bool live = valid != 0;
  const uint64_t lane_word = site0 >> 3;
  const uint64_t* __restrict__ row_start = a.row_start;
  const uint32_t* __restrict__ nib = a.nib;

  uint32_t cnt[kSiteLane][4];
#pragma unroll
  for (uint32_t i = 0; i < kSiteLane; ++i)
    cnt[i][0] = cnt[i][1] = cnt[i][2] = cnt[i][3] = 0;

  uint64_t r = (uint64_t)strip * kSiteStrip;
  const uint64_t r_end = a.n_rows - r < kSiteStrip ? a.n_rows : r + kSiteStrip;
  while (r < r_end) {
    const uint64_t end8 = r_end - r < kSiteWiden8 ? r_end : r + kSiteWiden8;
    uint32_t acc8[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};  // bytes: even sites, odd sites
    while (r < end8) {
      uint32_t acc4[4] = {0, 0, 0, 0};
      if (end8 - r >= kSiteWiden4) {
#pragma unroll
        for (uint32_t k = 0; k < kSiteWiden4; ++k)
          site_row(nib, row_start[r + k], lane_word, live, keep, acc4);
        r += kSiteWiden4;
      } else {
        for (; r < end8; ++r) site_row(nib, row_start[r], lane_word, live, keep, acc4);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc8[c][0] += acc4[c] & kLowNibbles;
        acc8[c][1] += (acc4[c] >> 4) & kLowNibbles;
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < kSiteLane; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) cnt[i][c] += (acc8[c][i & 1] >> (8 * (i >> 1))) & 0xffu;
  }

  // a, t, c, g of the lane's sites, then the tile's numbers in memory order
#pragma unroll
  for (uint32_t i = 0; i < kSiteLane; ++i) {
    uint32_t* at = lds + tid * kLdsPitch + 4 * i;
    at[0] = cnt[i][0] - cnt[i][1] - cnt[i][2] - cnt[i][3];
    at[1] = cnt[i][3];
    at[2] = cnt[i][1];
    at[3] = cnt[i][2];
  }
  __syncthreads();
  const uint64_t tile_first = (uint64_t)tile * kSiteTile * 4;
  const uint64_t n_numbers = a.n_sites * 4;
#pragma unroll 4
  for (uint32_t k = 0; k < 4 * kSiteLane; ++k) {
    const uint32_t e = k * kSiteBlock + tid;
    const uint32_t v = lds[(e / (4 * kSiteLane)) * kLdsPitch + e % (4 * kSiteLane)];
    const uint64_t g = tile_first + e;
    if (g >= n_numbers) continue;
    if (a.n_strips == 1)
      a.counts[g] = v;
    else if (v)
      atomicAdd(a.counts + g, v);
  }
}

}  // namespace

hipError_t launch_site_count(const SiteArgs& a, hipStream_t s) {
  if (a.n_strips > 1)
    if (hipError_t e = hipMemsetAsync(a.counts, 0, a.n_sites * 4 * sizeof(uint32_t), s)) return e;
  hipLaunchKernelGGL(site_count_kernel, dim3(a.n_tiles * a.n_strips), dim3(kSiteBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace magot
