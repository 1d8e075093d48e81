// Stand-alone check of the tile block packer (magot_amd/csrc/tileblocks.cpp)
// for a sanitizer build (tests/sanitize/run_tile_blocks.py): packs a small
// synthetic plan -- multi-exon records on both strands, short single-exon
// records, one tile per geometry corner -- under forced and chosen block
// geometries, decodes every row back and compares it with the u64 tables.
// Exit status 0 = every row round-trips.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../magot_amd/csrc/common.h"

namespace magot {
void set_error(const std::string&) {}
}  // namespace magot

extern "C" int magot_debug_tile_blocks(const uint64_t*, const uint64_t*, const uint64_t*,
                                       const uint64_t*, uint64_t, uint32_t, const void*, uint64_t,
                                       uint32_t*, void*, uint64_t*, uint64_t, int64_t*, uint64_t,
                                       uint64_t*);

using namespace magot;

static int fail(const char* what, size_t t, size_t j) {
  fprintf(stderr, "tile_blocks_check: %s (tile %zu row %zu)\n", what, t, j);
  return 1;
}

static int run(uint32_t lane_chunks, uint32_t force_ex, uint32_t force_tx) {
  std::mt19937_64 rng(12345 + lane_chunks);
  const uint64_t span = 1ull << 30;
  // records: 40 of 30 exons of 20..219 bases, then 300 single exons of 3..11 bases
  std::vector<uint64_t> ex_g, ex_out{0}, tn, tp;
  uint64_t q = 0;
  auto record = [&](int n_ex, int lo, int hi) {
    uint64_t len = 0;
    const uint64_t o0 = ex_out.back();
    for (int i = 0; i < n_ex; ++i) {
      const uint64_t n = lo + rng() % (hi - lo);
      uint64_t gw = 64 + rng() % (span - 1024);
      if (rng() & 1) gw |= kRcBit;
      if (rng() % 4 == 0) gw |= kExcBit;
      ex_g.push_back(gw);
      ex_out.push_back(ex_out.back() + n);
      len += n;
    }
    if (len >= 3) {
      tn.push_back(o0);
      tp.push_back(q);
    }
    q += len / 3;
  };
  for (int r = 0; r < 40; ++r) record(30, 20, 220);
  for (int r = 0; r < 300; ++r) record(1, 3, 12);
  const uint64_t B = ex_out.back(), P = q, Ec = ex_g.size(), Tc = tn.size();
  ex_g.push_back(0);
  tn.push_back(B);
  tp.push_back(P);
  // tiles of at most 2048 bytes and 48 residue-bearing records (not the
  // planner's cut: any consistent tiling exercises the packer)
  std::vector<TileRec> tiles;
  uint64_t T0 = 0, e1 = 0, j1 = 0;
  while (T0 < B) {
    while (ex_out[e1 + 1] <= T0) ++e1;
    while (j1 + 1 < Tc && tn[j1 + 1] <= T0) ++j1;
    uint64_t T1 = std::min(T0 + 2048, B);
    if (e1 + 100 < Ec) T1 = std::min(T1, ex_out[e1 + 100]);
    if (j1 + 48 < Tc) T1 = std::min(T1, std::max(tn[j1 + 48], T0 + 16));
    uint64_t e2 = e1, j2 = j1;
    while (e2 < Ec && ex_out[e2] < T1) ++e2;
    while (j2 < Tc && tn[j2] < T1) ++j2;
    const uint64_t Q0 = tp[j1], Q1 = tp[j2];
    tiles.push_back(TileRec{T0, T1, Q0, Q1, (uint32_t)e1, (uint32_t)e2, (uint32_t)(Q1 > Q0 ? j1 : 0),
                            (uint32_t)(Q1 > Q0 ? j2 : 0)});
    T0 = T1;
  }
  uint32_t geo[3] = {force_ex, force_tx, 0};
  uint64_t n_ovf[2] = {0, 0};
  if (magot_debug_tile_blocks(ex_g.data(), ex_out.data(), tn.data(), tp.data(), span, lane_chunks,
                              tiles.data(), tiles.size(), geo, nullptr, nullptr, 0, nullptr, 0,
                              n_ovf))
    return fail("sizes call failed", 0, 0);
  // exact-size buffers: a write past any of them is the sanitizer's to find
  std::vector<uint8_t> blocks(tiles.size() * geo[2], 0xA5);
  std::vector<uint64_t> oex(n_ovf[0]);
  std::vector<int64_t> otx(2 * n_ovf[1]);
  if (magot_debug_tile_blocks(ex_g.data(), ex_out.data(), tn.data(), tp.data(), span, lane_chunks,
                              tiles.data(), tiles.size(), geo, blocks.data(), oex.data(),
                              oex.size(), otx.data(), n_ovf[1], n_ovf))
    return fail("pack call failed", 0, 0);
  const uint32_t E = geo[0], X = geo[1];
  uint64_t at_e = 0, at_x = 0;
  const uint64_t m33 = (1ull << 33) - 1;
  for (size_t t = 0; t < tiles.size(); ++t) {
    const TileRec& r = tiles[t];
    const uint8_t* b = blocks.data() + t * geo[2];
    TileHead h;
    std::memcpy(&h, b, sizeof h);
    const uint32_t m = r.e2 - r.e1, nt = r.j2 - r.j1, rows = nt ? nt + 1 : 0;
    if (h.T0 != r.T0 || h.Q0 != r.Q0 || h.counts != (m | nt << 8)) return fail("header", t, 0);
    for (uint32_t j = 0; j < m; ++j) {
      uint64_t row;
      if (j < E) std::memcpy(&row, b + sizeof h + 8 * j, 8);
      else row = oex[at_e + j - E];
      const uint64_t gw = ex_g[r.e1 + j], o0 = ex_out[r.e1 + j], o1 = ex_out[r.e1 + j + 1];
      const uint64_t gs = gw & ~kExFlagBits, s = o0 - r.T0;
      const uint64_t U = (gw & kRcBit) ? 2 * span - gs - (o1 - o0) - s : gs - s;
      const uint64_t hi = row >> 32;
      if (((row & 0xFFFFFFFFull) | (hi & 1) << 32) != (U & m33)) return fail("anchor", t, j);
      if (((hi >> 14) & 1) != (gw >> 63)) return fail("strand flag", t, j);
    }
    for (uint32_t k = 0; k < rows; ++k) {
      TxRow x;
      if (k < X) std::memcpy(&x, b + sizeof h + 8 * (size_t)E + 16 * k, 16);
      else x = TxRow{otx[2 * (at_x + k - X)], otx[2 * (at_x + k - X) + 1]};
      if (x.tn != (int64_t)(tn[r.j1 + k] - r.T0) || x.tp != (int64_t)(tp[r.j1 + k] - r.Q0))
        return fail("record row", t, k);
    }
    at_e += m > E ? m - E : 0;
    at_x += rows > X ? rows - X : 0;
  }
  if (at_e != n_ovf[0] || at_x != n_ovf[1]) return fail("overflow counts", 0, 0);
  printf("lane_chunks %u rows %u + %u (stride %u): %zu tiles, overflow %llu + %llu ok\n",
         lane_chunks, E, X, geo[2], tiles.size(), (unsigned long long)n_ovf[0],
         (unsigned long long)n_ovf[1]);
  return 0;
}

int main() {
  for (uint32_t lc : {3u, 6u})
    for (auto f : {std::pair<uint32_t, uint32_t>{0, 0}, {64, 14}, {2, 1}})
      if (run(lc, f.first, f.second)) return 1;
  return 0;
}
