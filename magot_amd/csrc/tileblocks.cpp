// Packed tile descriptor blocks (host only): what extract_kernel stages for a
// tile, computed once per plan from the planner's u64 tables (layout and row
// format: common.h).  The arithmetic is the per-launch staging arithmetic the
// kernel used to do: the unified anchor U, the clamped tile-relative end, the
// first-chunk index.
#include <algorithm>
#include <cstring>

#include "common.h"

namespace magot {

TileGeometry tile_geometry(const TileRec* tiles, uint64_t n_tiles, uint32_t force_ex,
                           uint32_t force_tx) {
  // histograms of interval rows (m) and record rows (nt + 1, or none)
  uint64_t hm[kExonCap + 1] = {0}, hr[kTxCap + 2] = {0};
  uint32_t max_m = 0, max_r = 0;
  for (uint64_t t = 0; t < n_tiles; ++t) {
    const uint32_t m = std::min<uint32_t>(tiles[t].e2 - tiles[t].e1, kExonCap);
    const uint32_t nt = std::min<uint32_t>(tiles[t].j2 - tiles[t].j1, kTxCap);
    const uint32_t r = nt ? nt + 1 : 0u;
    ++hm[m];
    ++hr[r];
    max_m = std::max(max_m, m);
    max_r = std::max(max_r, r);
  }
  auto pct98 = [&](const uint64_t* h, uint32_t top) -> uint32_t {
    uint64_t acc = 0;
    for (uint32_t v = 0; v <= top; ++v) {
      acc += h[v];
      if (acc * 50 >= n_tiles * 49) return v;
    }
    return top;
  };
  uint32_t ex = force_ex ? force_ex : pct98(hm, kExonCap);
  uint32_t tx = force_tx ? force_tx : pct98(hr, kTxCap + 1);
  // at most 64 overflow rows of either kind (one per lane)
  ex = std::min((std::max({ex, 1u, max_m > 64u ? max_m - 64u : 0u}) + 1u) & ~1u, kBlkExMax);  // even
  tx = std::min(std::max({tx, 1u, max_r > 64u ? max_r - 64u : 0u}), kBlkTxMax);
  return TileGeometry{ex, tx, tile_block_stride(ex, tx)};
}

void pack_tile_block(const TileTables& tb, const TileGeometry& g, const TileRec& r, uint32_t oe,
                     uint32_t ot, uint8_t* b, uint64_t* ovf_ex, TxRow* ovf_tx) {
  const uint32_t m = r.e2 - r.e1, nt = r.j2 - r.j1;
  // record rows 0 .. nt (row nt: the sentinel); none for a tile without residues
  const uint32_t rows = nt ? nt + 1 : 0u;
  TileHead h;
  h.T0 = r.T0;
  h.Q0 = r.Q0;
  h.span_res = (uint32_t)(r.T1 - r.T0) | (uint32_t)(r.Q1 - r.Q0) << 16;
  h.counts = m | nt << 8;
  h.ovf_ex = m > g.ex_rows ? oe : 0u;
  h.ovf_tx = rows > g.tx_rows ? ot : 0u;
  std::memcpy(b, &h, sizeof h);
  uint64_t* const ex = reinterpret_cast<uint64_t*>(b + sizeof(TileHead));
  TxRow* const tx = reinterpret_cast<TxRow*>(b + sizeof(TileHead) + 8 * (size_t)g.ex_rows);
  const int64_t end_cap = tile_bytes((int)tb.lane_chunks) + 4 * kHalo;
  for (uint32_t j = 0; j < m; ++j) {
    const uint64_t gw = tb.ex_g[r.e1 + j];
    const uint64_t o0 = tb.ex_out[r.e1 + j], o1 = tb.ex_out[r.e1 + j + 1];
    const uint64_t gs = gw & ~kExFlagBits;
    const uint64_t s = o0 - r.T0;  // wraps below 0 for the interval holding T0
    // U mod 2^64; the kernel keeps 33 bits (tile byte p reads unified base U + p)
    const uint64_t U = (gw & kRcBit) ? 2 * tb.span - gs - (o1 - o0) - s : gs - s;
    const uint64_t end = (uint64_t)std::min<int64_t>((int64_t)(o1 - r.T0), end_cap);
    // rows past the first start inside the tile (s > 0)
    const uint64_t cj = j == 0 ? kBlkNoChunk
                               : std::min<uint64_t>((s + kChunk - 1) / kChunk, kBlkNoChunk);
    const uint64_t fl = ((gw & kRcBit) ? kFlagRc : 0u) | ((gw & kExcBit) ? kFlagExc : 0u) |
                        ((gw & kSlowLitBit) ? kFlagSlowLit : 0u);
    const uint64_t hi = ((U >> 32) & 1u) | end << 1 | fl << 14 | cj << 17;
    const uint64_t row = (U & 0xFFFFFFFFull) | hi << 32;
    if (j < g.ex_rows) ex[j] = row;
    else ovf_ex[oe + (j - g.ex_rows)] = row;
  }
  for (uint32_t j = m; j < g.ex_rows; ++j) ex[j] = 0;
  for (uint32_t k = 0; k < rows; ++k) {
    const TxRow x{(int64_t)(tb.tx_nuc[r.j1 + k] - r.T0), (int64_t)(tb.tx_pep[r.j1 + k] - r.Q0)};
    if (k < g.tx_rows) tx[k] = x;
    else ovf_tx[ot + (k - g.tx_rows)] = x;
  }
  for (uint32_t k = rows; k < g.tx_rows; ++k) tx[k] = TxRow{0, 0};
  // the stride's padding to 16 bytes
  const size_t used = sizeof(TileHead) + 8 * (size_t)g.ex_rows + 16 * (size_t)g.tx_rows;
  std::memset(b + used, 0, g.stride - used);
}

}  // namespace magot

using namespace magot;

extern "C" int magot_debug_tile_blocks(const uint64_t* ex_g, const uint64_t* ex_out,
                                       const uint64_t* tx_nuc, const uint64_t* tx_pep,
                                       uint64_t span, uint32_t lane_chunks, const void* tiles,
                                       uint64_t n_tiles, uint32_t* geometry, void* blocks,
                                       uint64_t* ovf_ex, uint64_t ovf_ex_cap, int64_t* ovf_tx,
                                       uint64_t ovf_tx_cap, uint64_t* n_ovf) {
  if (!ex_g || !ex_out || !tx_nuc || !tx_pep || !n_ovf || !geometry || (n_tiles && !tiles) ||
      geometry[0] > kBlkExMax || geometry[1] > kBlkTxMax ||
      (lane_chunks != (uint32_t)kLaneChunksLarge && lane_chunks != (uint32_t)kLaneChunksSmall)) {
    set_error("magot_debug_tile_blocks: bad argument");
    return MAGOT_ERR_ARG;
  }
  const TileRec* tr = static_cast<const TileRec*>(tiles);
  for (uint64_t t = 0; t < n_tiles; ++t) {
    const uint64_t m = (uint64_t)tr[t].e2 - tr[t].e1, nt = (uint64_t)tr[t].j2 - tr[t].j1;
    if (tr[t].e2 < tr[t].e1 || tr[t].j2 < tr[t].j1 || m > (uint64_t)kExonCap ||
        nt > (uint64_t)kTxCap || tr[t].T1 - tr[t].T0 > 0xFFFFull ||
        tr[t].Q1 - tr[t].Q0 > 0xFFFFull) {
      set_error("magot_debug_tile_blocks: tile " + std::to_string(t) + " out of range");
      return MAGOT_ERR_RANGE;
    }
  }
  const TileGeometry g = tile_geometry(tr, n_tiles, geometry[0], geometry[1]);
  geometry[0] = g.ex_rows;
  geometry[1] = g.tx_rows;
  geometry[2] = g.stride;
  uint64_t ne = 0, nx = 0;
  for (uint64_t t = 0; t < n_tiles; ++t) {
    ne += tile_ovf_ex(g, tr[t]);
    nx += tile_ovf_tx(g, tr[t]);
  }
  n_ovf[0] = ne;
  n_ovf[1] = nx;
  if (!blocks) return MAGOT_OK;  // geometry and sizes only
  if (ne > ovf_ex_cap || nx > ovf_tx_cap || (ne && !ovf_ex) || (nx && !ovf_tx) ||
      ne > 0xFFFFFFFFull || nx > 0xFFFFFFFFull) {
    set_error("magot_debug_tile_blocks: overflow arrays too small");
    return MAGOT_ERR_ARG;
  }
  const TileTables tb{ex_g, ex_out, tx_nuc, tx_pep, span, lane_chunks};
  uint64_t oe = 0, ot = 0;
  for (uint64_t t = 0; t < n_tiles; ++t) {
    pack_tile_block(tb, g, tr[t], (uint32_t)oe, (uint32_t)ot,
                    static_cast<uint8_t*>(blocks) + t * g.stride, ovf_ex,
                    reinterpret_cast<TxRow*>(ovf_tx));
    oe += tile_ovf_ex(g, tr[t]);
    ot += tile_ovf_tx(g, tr[t]);
  }
  return MAGOT_OK;
}
