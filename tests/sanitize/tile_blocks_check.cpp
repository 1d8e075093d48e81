// Stand-alone check of the extraction planner and the tile block packer
// (magot_amd/csrc/tileplan.cpp, tileblocks.cpp) for a sanitizer build
// (tests/sanitize/run_tile_blocks.py): plans a small synthetic workload --
// multi-exon records on both strands over a genome with exception runs, short
// single-exon records -- in record order and in genome order, and a plan of
// 2^15 + 1000 short records (the threaded sweeps), packs the planner's tiles
// under forced and chosen block geometries, decodes every row back and
// compares it with the u64 tables.  Exit status 0 = every row round-trips.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../magot_amd/csrc/common.h"

namespace magot {
void set_error(const std::string& msg) { fprintf(stderr, "tile_blocks_check: %s\n", msg.c_str()); }
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

struct Workload {
  std::vector<uint8_t> genome;  // one contig
  std::vector<magot_exon> exons;
  std::vector<magot_tx> txs;
};

// n_rec records of n_ex exons of lo .. hi - 1 bases, at random places and strands
static void add_records(Workload* w, std::mt19937_64& rng, int n_rec, int n_ex, int lo, int hi) {
  for (int r = 0; r < n_rec; ++r) {
    w->txs.push_back(magot_tx{w->exons.size(), (uint32_t)n_ex, 0});
    const uint64_t rc = (rng() & 1) ? kRcBit : 0;
    for (int i = 0; i < n_ex; ++i) {
      const uint32_t n = (uint32_t)(lo + rng() % (hi - lo));
      w->exons.push_back(magot_exon{rng() % (w->genome.size() - n) | rc, 0, n});
    }
  }
}

static Workload make_workload(uint64_t seed, uint64_t bases, int n_long, int n_short) {
  std::mt19937_64 rng(seed);
  Workload w;
  w.genome.resize(bases);
  for (uint8_t& b : w.genome) b = "ACGTacgt"[rng() % 8];
  for (int k = 0; k < 200; ++k) {  // exception runs, some without a literal class
    const uint64_t at = rng() % (bases - 40), n = 1 + rng() % 30;
    std::memset(&w.genome[at], "NnSR"[k % 4], n);
  }
  add_records(&w, rng, n_long, 30, 20, 220);
  w.txs.push_back(magot_tx{w.exons.size(), 0, 0});  // a record without intervals
  add_records(&w, rng, n_short, 1, 0, 12);          // some of them empty
  return w;
}

// Stages 1 and 2 over w, then every block of the planner's tiles packed and read back.
static int run(const Workload& w, uint32_t outputs, int lane_chunks, uint32_t force_ex,
               uint32_t force_tx) {
  const ContigSource src{w.genome.data(), w.genome.size(), 0, 0};
  HostPacked hp;
  pack_genome(&src, 1, &hp);
  PlanOptions opt = plan_options(outputs);
  opt.lane_chunks = lane_chunks;
  opt.block_ex = force_ex;
  opt.block_tx = force_tx;
  const PlanInput in{GenomeView{hp.contig_base.data(), hp.contig_len.data(), 1, hp.span,
                                hp.runs.data(), hp.dir.data()},
                     w.exons.data(), w.exons.size(), w.txs.data(), w.txs.size(), opt};
  Lap lap("MAGOT_PLAN_TIMING", "plan");
  PlanCount cnt;
  if (plan_count(in, &cnt)) return fail("stage 1 failed", 0, 0);
  const unsigned nth = cnt.nth;
  TilePlan p;
  if (plan_build(in, std::move(cnt), lap, &p)) return fail("stage 2 failed", 0, 0);
  const std::vector<TileRec>& tiles = p.tiles;
  const uint64_t* ex_g = p.ex_g.data();
  const uint64_t* ex_out = p.ex_out.data();
  const std::vector<uint64_t>&tn = p.tn, &tp = p.tp;
  const uint64_t span = hp.span;
  uint32_t geo[3] = {force_ex, force_tx, 0};
  uint64_t n_ovf[2] = {0, 0};
  if (magot_debug_tile_blocks(ex_g, ex_out, tn.data(), tp.data(), span, p.lane_chunks,
                              tiles.data(), tiles.size(), geo, nullptr, nullptr, 0, nullptr, 0,
                              n_ovf))
    return fail("sizes call failed", 0, 0);
  if (geo[0] != p.geo.ex_rows || geo[1] != p.geo.tx_rows || geo[2] != p.geo.stride ||
      n_ovf[0] != p.n_ovf_ex || n_ovf[1] != p.n_ovf_tx)
    return fail("the planner's geometry differs from the packer's", 0, 0);
  // exact-size buffers: a write past any of them is the sanitizer's to find
  std::vector<uint8_t> blocks(tiles.size() * geo[2], 0xA5);
  std::vector<uint64_t> oex(n_ovf[0]);
  std::vector<int64_t> otx(2 * n_ovf[1]);
  if (magot_debug_tile_blocks(ex_g, ex_out, tn.data(), tp.data(), span, p.lane_chunks,
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
    if (at_e != p.ovf_at[2 * t] || at_x != p.ovf_at[2 * t + 1]) return fail("overflow place", t, 0);
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
  printf("%zu records (%u threads), outputs %u, lane_chunks %u rows %u + %u (stride %u): %zu "
         "tiles, overflow %llu + %llu ok\n",
         w.txs.size(), nth, outputs, p.lane_chunks, E, X, geo[2], tiles.size(),
         (unsigned long long)n_ovf[0], (unsigned long long)n_ovf[1]);
  return 0;
}

int main() {
  const uint32_t both = MAGOT_OUT_NUC | MAGOT_OUT_PEP;
  const Workload small = make_workload(12345, 1u << 20, 40, 300);
  for (uint32_t outputs : {both, both | MAGOT_OUT_GENOME_ORDER})
    for (int lc : {3, 6})
      for (auto f : {std::pair<uint32_t, uint32_t>{0, 0}, {64, 14}, {2, 1}})
        if (run(small, outputs, lc, f.first, f.second)) return 1;
  // enough records for the planner's sweeps to run on several threads
  const Workload wide = make_workload(777, 1u << 22, 100, (1 << 15) + 1000);
  for (uint32_t outputs : {both, MAGOT_OUT_NUC | MAGOT_OUT_GENOME_ORDER})
    if (run(wide, outputs, 0, 0, 0)) return 1;
  return 0;
}
