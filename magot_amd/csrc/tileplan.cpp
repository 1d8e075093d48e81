// The extraction planner (host only): from the caller's interval and record
// tables to the tiles a launch runs, in launch order, and the geometry of
// their descriptor blocks (tileblocks.cpp packs them; declarations and the
// table formats: common.h).  magot_plan_create allocates and uploads what
// this file plans; the magot_debug_* entries at the end run it without a device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.h"

namespace magot {

int plan_check_tables(const magot_exon* exons, uint64_t n_exons, const magot_tx* txs,
                      uint64_t n_tx, uint32_t outputs) {
  if ((n_exons && !exons) || (n_tx && !txs)) {
    set_error("magot_plan_create: null argument");
    return MAGOT_ERR_ARG;
  }
  if (outputs & ~(MAGOT_OUT_NUC | MAGOT_OUT_PEP | MAGOT_OUT_GENOME_ORDER)) {
    set_error("magot_plan_create: unknown output flags");
    return MAGOT_ERR_ARG;
  }
  if (n_tx >= 0xFFFFFFFFull || n_exons >= 0xFFFFFFFFull) {
    set_error("magot_plan_create: table too large for one plan (split it)");
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

PlanOptions plan_options(uint32_t outputs) {
  PlanOptions o{outputs & ~MAGOT_OUT_GENOME_ORDER, (outputs & MAGOT_OUT_GENOME_ORDER) != 0, 0, 0, 0};
  // MAGOT_EXTRACT_LANE_CHUNKS=3|6 forces a tile size, MAGOT_TILE_BLOCK_ROWS=ex,tx
  // the blocks' inline capacities (tests and A/Bs)
  if (const char* e = std::getenv("MAGOT_EXTRACT_LANE_CHUNKS")) o.lane_chunks = std::atoi(e);
  if (const char* e = std::getenv("MAGOT_TILE_BLOCK_ROWS")) {
    unsigned fe = 0, fx = 0;
    if (sscanf(e, "%u,%u", &fe, &fx) == 2) {
      o.block_ex = std::min(fe, kBlkExMax);
      o.block_tx = std::min(fx, kBlkTxMax);
    }
  }
  return o;
}

namespace {

// --- stage 1 ----------------------------------------------------------------

// Records tile the interval table in order.
int check_records(const PlanInput& in) {
  uint64_t expect = 0;
  for (uint64_t t = 0; t < in.T; ++t) {
    if (in.txs[t].exon_begin != expect) {
      set_error("magot_plan_create: record " + std::to_string(t) +
                " does not start where the previous one ended");
      return MAGOT_ERR_ARG;
    }
    expect += in.txs[t].n_exons;
    if (expect > in.E) {
      set_error("magot_plan_create: records reference more exons than given");
      return MAGOT_ERR_ARG;
    }
  }
  if (expect != in.E) {
    set_error("magot_plan_create: exons not covered by records");
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

// Every record's length (rec_len) and count of non-empty intervals (rec_ex),
// record ranges in parallel.  Returns the first interval outside its contig, or ~0.
uint64_t count_sweep(const PlanInput& in, PlanCount* c) {
  const GenomeView& g = in.g;
  std::vector<uint64_t> first_bad(c->nth, ~0ull);
  parallel_ranges(in.T, c->nth, [&](uint64_t t0, uint64_t t1, unsigned part) {
    for (uint64_t t = t0; t < t1; ++t) {
      uint64_t len = 0, nz = 0;
      const uint64_t e0 = in.txs[t].exon_begin, e1 = e0 + in.txs[t].n_exons;
      for (uint64_t e = e0; e < e1; ++e) {
        const magot_exon& x = in.exons[e];
        const uint64_t st = x.start_rc & ~kRcBit;
        if (x.contig >= g.n_contigs || st > g.contig_len[x.contig] ||
            st + x.len > g.contig_len[x.contig]) {
          first_bad[part] = e;
          return;
        }
        len += x.len;
        nz += x.len != 0;
      }
      c->rec_len[t] = len;
      c->rec_ex[t] = nz;
    }
  });
  for (uint64_t e : first_bad)  // ranges ascend: the first bad range holds the first bad interval
    if (e != ~0ull) return e;
  return ~0ull;
}

// --- stage 2 ----------------------------------------------------------------

// Record order: every non-empty interval's word (global start | strand |
// exception flags) at its compacted place, and its length.
void word_sweep(const PlanInput& in, const PlanCount& c, uint64_t* w_g, uint32_t* w_len) {
  const GenomeView& g = in.g;
  parallel_ranges(in.T, c.nth, [&](uint64_t t0, uint64_t t1, unsigned) {
    for (uint64_t t = t0; t < t1; ++t) {
      uint64_t k = c.rec_ex[t];
      const uint64_t e0 = in.txs[t].exon_begin, e1 = e0 + in.txs[t].n_exons;
      for (uint64_t e = e0; e < e1; ++e) {
        const magot_exon& x = in.exons[e];
        if (x.len == 0) continue;
        const uint64_t gs = g.contig_base[x.contig] + (x.start_rc & ~kRcBit);
        // does [gs, gs+len) touch an exception run?  (dir: first run ending past the block)
        uint64_t d = g.dir[gs >> kDirShift] & ~kDirClean;
        while (g.runs[d].start + g.runs[d].len <= gs) ++d;
        uint64_t exc = g.runs[d].start < gs + x.len ? kExcBit : 0;
        if (exc && !(x.start_rc & kRcBit)) {
          // forward strand: a byte without a literal class needs the run list
          for (uint64_t r = d; g.runs[r].start < gs + x.len; ++r)
            if (lit_class(g.runs[r].byte) == 7u) {
              exc |= kSlowLitBit;
              break;
            }
        }
        w_g[k] = gs | (x.start_rc & kRcBit) | exc;
        w_len[k] = x.len;
        ++k;
      }
    }
  });
}

// Layout order of the records: record order (empty), or (MAGOT_OUT_GENOME_ORDER) by
// the genome position of each record's first non-empty interval (records
// without output last), so that records sharing genome lines run in
// neighbouring tiles (C3: fills 0.89 -> 0.54 GB per launch); the places come
// back through magot_plan_layout, and fetch / copy_outputs restore record order.
std::vector<uint32_t> layout_order(const PlanInput& in, const PlanCount& c, const uint64_t* w_g) {
  std::vector<uint32_t> order;
  if (in.opt.by_genome) {
    std::vector<uint64_t> key(in.T);
    for (uint64_t t = 0; t < in.T; ++t)
      key[t] = c.rec_ex[t] < c.rec_ex[t + 1] ? w_g[c.rec_ex[t]] & ~kExFlagBits : in.g.span;
    radix_order(key, &order);
  }
  return order;
}

// Each record's place (lay_*, indexed by record) from one sweep in layout
// order, then the interval table in layout order with its output offsets,
// record ranges in parallel (each record's rows are one block).  The
// record-order rows themselves when the layout is record order.
void lay_out(const PlanInput& in, const PlanCount& c, const std::vector<uint32_t>& order,
             HostBuf<uint64_t>&& w_g, const uint32_t* w_len, TilePlan* p) {
  const uint64_t T = in.T, Ec = c.Ec;
  const bool by_genome = in.opt.by_genome;
  p->lay_nuc.resize(T);
  p->lay_pep.resize(T);
  uint64_t* const lay_nuc = p->lay_nuc.data();
  uint64_t* const lay_pep = p->lay_pep.data();
  HostBuf<uint64_t> lay_ex(T);
  uint64_t acc = 0, q = 0, ek = 0;
  for (uint64_t k = 0; k < T; ++k) {
    const uint64_t t = by_genome ? order[k] : k;
    lay_nuc[t] = acc;
    lay_pep[t] = q;
    lay_ex[t] = ek;
    acc += c.rec_len[t];
    q += c.rec_len[t] / 3;
    ek += c.rec_ex[t + 1] - c.rec_ex[t];
  }
  p->ex_g = by_genome ? HostBuf<uint64_t>(Ec + 1) : std::move(w_g);
  p->ex_out = HostBuf<uint64_t>(Ec + 2);
  uint64_t* const ex_g = p->ex_g.data();
  uint64_t* const ex_out = p->ex_out.data();
  parallel_ranges(T, c.nth, [&](uint64_t t0, uint64_t t1, unsigned) {
    for (uint64_t t = t0; t < t1; ++t) {
      uint64_t k = lay_ex[t], o = lay_nuc[t];
      for (uint64_t i = c.rec_ex[t]; i < c.rec_ex[t + 1]; ++i, ++k) {
        if (by_genome) ex_g[k] = w_g[i];
        ex_out[k] = o;
        o += w_len[i];
      }
    }
  });
  ex_g[Ec] = 0;
  ex_out[Ec] = c.B;
  ex_out[Ec + 1] = c.B;
}

// The compacted record table in layout order (records with at least one
// codon; sentinel B, P) and the record-order prefix offsets (what fetch returns).
void record_tables(const PlanInput& in, const PlanCount& c, const std::vector<uint32_t>& order,
                   TilePlan* p) {
  const uint64_t T = in.T;
  std::vector<uint64_t> tn, tp;
  tn.reserve(T + 3);
  tp.reserve(T + 3);
  for (uint64_t k = 0; k < T; ++k) {
    const uint64_t t = in.opt.by_genome ? order[k] : k;
    if (c.rec_len[t] >= 3) {
      tn.push_back(p->lay_nuc[t]);
      tp.push_back(p->lay_pep[t]);
    }
  }
  std::vector<uint64_t> nuc_off(T + 1), pep_off(T + 1);
  nuc_off[0] = pep_off[0] = 0;
  for (uint64_t t = 0; t < T; ++t) {
    nuc_off[t + 1] = nuc_off[t] + c.rec_len[t];
    pep_off[t + 1] = pep_off[t] + c.rec_len[t] / 3;
  }
  p->Tc = tn.size();
  tn.push_back(c.B);
  tp.push_back(c.P);
  p->tn = std::move(tn);
  p->tp = std::move(tp);
  p->nuc_off = std::move(nuc_off);
  p->pep_off = std::move(pep_off);
}

struct Cursor {  // upper_bound over a non-decreasing table, for non-decreasing queries
  const uint64_t* v;
  uint64_t n, j;
  uint64_t operator()(uint64_t x) {
    while (j < n && v[j] <= x) ++j;
    return j;
  }
};

}  // namespace

// A tile owns nucleotide bytes [T0, T1) and residues [R0, R1).  Residue
// ownership is rounded up to 16-residue (16-byte) store chunks, so nearly
// every peptide store is a full aligned chunk; the residues a tile owns past
// its last codon start are decoded from its kHalo bytes of look-ahead.
// Every query below is monotone over the cut (tile ends, decode ends and
// residue bounds only grow), so the searches are cursors that move forward:
// O(records + tiles) per cut instead of a binary search per query.
int cut_tiles(const uint64_t* ex_out, uint64_t Ec, const uint64_t* tn, const uint64_t* tp,
              uint64_t Tc, uint64_t tile, std::vector<TileRec>* tiles) {
  const uint64_t B = ex_out[Ec], P = tp[Tc];
  auto pcount = [&](Cursor& c, uint64_t T) -> uint64_t {  // residues whose codon starts before T
    const uint64_t j = c(T);
    if (j == 0) return 0;
    const uint64_t into = T - tn[j - 1];
    return tp[j - 1] + std::min((into + 2) / 3, tp[j] - tp[j - 1]);
  };
  auto rec_of = [&](Cursor& c, uint64_t q) -> uint64_t {  // compacted record holding residue q < P
    return c(q) - 1;
  };
  Cursor c_end{tn, Tc, 0}, c_dec{tn, Tc, 0};  // pcount(T1), pcount(dec_end - 2)
  Cursor c_r0{tp, Tc, 0}, c_r1{tp, Tc, 0};    // rec_of(R0), rec_of(R1 - 1)
  uint64_t e1 = 0, e2 = 0;
  uint64_t T0 = 0, R0 = 0;
  while (T0 < B) {
    while (e1 < Ec && ex_out[e1 + 1] <= T0) ++e1;           // interval containing T0
    const uint64_t j1 = R0 < P ? rec_of(c_r0, R0) : Tc;      // record holding residue R0
    uint64_t T1 = std::min<uint64_t>(T0 + tile, B);
    if (e1 + kExonCap < Ec) T1 = std::min<uint64_t>(T1, ex_out[e1 + kExonCap] - kHalo);
    if (j1 + kTxCap - kChunk < Tc) T1 = std::min<uint64_t>(T1, tn[j1 + kTxCap - kChunk]);
    // cut on a 128-byte line boundary where the tile keeps one (no
    // nucleotide line is then written by two tiles), else on a chunk
    if (T1 < B) T1 = (T1 & ~(uint64_t)(kTileAlign - 1)) > T0 ? T1 & ~(uint64_t)(kTileAlign - 1)
                                                           : T1 & ~(uint64_t)(kChunk - 1);
    if (T1 < T0 + kChunk) T1 = std::min<uint64_t>(T0 + kChunk, B);
    const uint64_t dec_end = std::min<uint64_t>(T1 + kHalo, B);
    // residues owned: every codon starting before T1, rounded up to a chunk,
    // but only codons that end inside the decoded range and at most kPepSlots chunks
    uint64_t R1 = P;
    if (T1 < B) {
      R1 = std::min<uint64_t>((pcount(c_end, T1) + kChunk - 1) & ~(uint64_t)(kChunk - 1), P);
      R1 = std::min<uint64_t>(R1, pcount(c_dec, dec_end - 2));
      R1 = std::min<uint64_t>(R1, (R0 & ~(uint64_t)(kChunk - 1)) + kPepSlots * kChunk);
    }
    if (R1 < R0) R1 = R0;
    if (e2 < e1) e2 = e1;
    while (e2 < Ec && ex_out[e2] < dec_end) ++e2;           // intervals touching the decode range
    const uint64_t jl = R1 > R0 ? rec_of(c_r1, R1 - 1) : 0;  // record holding the last residue
    const uint64_t j2 = R1 > R0 ? jl + 1 : j1;               // records holding residues [R0, R1)
    if (e2 - e1 > (uint64_t)kExonCap || (R1 > R0 && j2 - j1 > (uint64_t)kTxCap) ||
        (R1 > R0 && tn[jl] + 3 * (R1 - 1 - tp[jl]) + 3 > dec_end)) {
      set_error("magot_plan_create: internal tiling error");
      return MAGOT_ERR_STATE;
    }
    tiles->push_back(TileRec{T0, T1, R0, R1, (uint32_t)e1, (uint32_t)e2,
                             (uint32_t)(R1 > R0 ? j1 : 0), (uint32_t)(R1 > R0 ? j2 : 0)});
    T0 = T1;
    R0 = R1;
  }
  if (R0 != P) {
    set_error("magot_plan_create: internal tiling error (residues)");
    return MAGOT_ERR_STATE;
  }
  return MAGOT_OK;
}

namespace {

// The large tile, or the small one for translating plans too small to fill
// the chip several times over (MAGOT_EXTRACT_LANE_CHUNKS=3|6 forces one, for
// A/Bs); nucleotide-only plans keep the large tile (C2: 0.0164 vs 0.0172 ms).
int choose_tiles(const PlanOptions& opt, TilePlan* p) {
  auto cut = [&](int lane_chunks) {
    p->lane_chunks = (uint32_t)lane_chunks;
    p->tiles.clear();
    return cut_tiles(p->ex_out.data(), p->Ec, p->tn.data(), p->tp.data(), p->Tc,
                     tile_bytes(lane_chunks), &p->tiles);
  };
  if (int rc = cut(kLaneChunksLarge)) return rc;
  if (opt.lane_chunks == kLaneChunksSmall ||
      (opt.lane_chunks != kLaneChunksLarge && (opt.outputs & MAGOT_OUT_PEP) &&
       p->tiles.size() < kSmallTilePlan))
    return cut(kLaneChunksSmall);
  return MAGOT_OK;
}

// Launch order: tiles that may take the run-list path first -- a staged
// interval over a byte without a literal class (kSlowLitBit), or one short
// enough that a chunk can span three intervals.  Their chains of dependent
// run-list loads then overlap the rest of the launch; at the end of the grid
// they set its tail (C2: 0.0174 ms with the 23 such tiles where they fall,
// 0.0151 ms with none).  Every other tile keeps output order.
void launch_order(TilePlan* p) {
  const uint64_t n = p->tiles.size();
  const uint64_t* ex_g = p->ex_g.data();
  const uint64_t* ex_out = p->ex_out.data();
  const std::vector<TileRec> cut = std::move(p->tiles);
  std::vector<uint8_t> slow_tile(n);
  parallel_ranges(n, n >= (1u << 14) ? p->nth : 1u, [&](uint64_t t0, uint64_t t1, unsigned) {
    for (uint64_t t = t0; t < t1; ++t) {
      bool slow = false;
      for (uint32_t e = cut[t].e1; e < cut[t].e2 && !slow; ++e)
        slow = (ex_g[e] & kSlowLitBit) || ex_out[e + 1] - ex_out[e] < (uint64_t)kChunk;
      slow_tile[t] = slow;
    }
  });
  p->tiles.assign(n, TileRec{});
  const uint64_t n_first = std::count(slow_tile.begin(), slow_tile.end(), 1);
  uint64_t at[2] = {n_first, 0};  // next place of a tile that is not / is slow
  for (uint64_t t = 0; t < n; ++t) p->tiles[at[slow_tile[t]]++] = cut[t];
}

// The blocks' inline capacities, from what this plan's tiles stage, and each
// tile's place in the overflow arrays (rows past a block's inline part).
int place_overflow(const PlanOptions& opt, TilePlan* p) {
  const uint64_t n = p->tiles.size();
  p->geo = tile_geometry(p->tiles.data(), n, opt.block_ex, opt.block_tx);
  p->ovf_at.resize(2 * n);
  for (uint64_t t = 0; t < n; ++t) {
    const TileRec& r = p->tiles[t];
    if (r.T1 - r.T0 > 0xFFFFull || r.Q1 - r.Q0 > 0xFFFFull) {
      set_error("magot_plan_create: internal tiling error (tile block fields)");
      return MAGOT_ERR_STATE;
    }
    p->ovf_at[2 * t] = (uint32_t)p->n_ovf_ex;
    p->ovf_at[2 * t + 1] = (uint32_t)p->n_ovf_tx;
    p->n_ovf_ex += tile_ovf_ex(p->geo, r);
    p->n_ovf_tx += tile_ovf_tx(p->geo, r);
  }
  if (p->n_ovf_ex >= 0xFFFFFFFFull || p->n_ovf_tx >= 0xFFFFFFFFull) {
    set_error("magot_plan_create: table too large for one plan (split it)");
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

}  // namespace

// Stage 1.  Host threads over record ranges for the per-interval passes (a
// large plan: C3's 4M intervals); small plans stay on the calling thread.
int plan_count(const PlanInput& in, PlanCount* c) {
  if (int rc = check_records(in)) return rc;
  c->nth = in.T >= (1u << 15) ? host_threads() : 1u;
  c->rec_ex.resize(in.T + 1);
  c->rec_len.resize(in.T);
  const uint64_t bad = count_sweep(in, c);
  if (bad != ~0ull) {
    set_error("magot_plan_create: exon " + std::to_string(bad) + " outside its contig");
    return MAGOT_ERR_RANGE;
  }
  for (uint64_t t = 0; t < in.T; ++t) {  // counts -> each record's first compacted interval
    const uint64_t n = c->rec_ex[t];
    c->rec_ex[t] = c->Ec;
    c->Ec += n;
    c->B += c->rec_len[t];
    c->P += c->rec_len[t] / 3;
  }
  c->rec_ex[in.T] = c->Ec;
  return MAGOT_OK;
}

// Stage 2.  The laps are EXPERIMENTS.md's breakdown of plan time.
int plan_build(const PlanInput& in, PlanCount&& c, Lap& lap, TilePlan* p) {
  p->Ec = c.Ec;
  p->nth = c.nth;
  HostBuf<uint64_t> w_g(c.Ec + 1);
  HostBuf<uint32_t> w_len(c.Ec);
  word_sweep(in, c, w_g.data(), w_len.data());
  lap("pass1");
  const std::vector<uint32_t> order = layout_order(in, c, w_g.data());
  lap("order");
  lay_out(in, c, order, std::move(w_g), w_len.data(), p);
  record_tables(in, c, order, p);
  lap("pass2");
  if (p->Ec >= 0xFFFFFFFFull || p->Tc >= 0xFFFFFFFFull) {
    set_error("magot_plan_create: table too large for one plan (split it)");
    return MAGOT_ERR_ARG;
  }
  if (int rc = choose_tiles(in.opt, p)) return rc;
  lap("tiles");
  if (p->tiles.size() >= 0x7FFFFFFFull) {
    set_error("magot_plan_create: output too large for one launch");
    return MAGOT_ERR_ARG;
  }
  launch_order(p);
  if (int rc = place_overflow(in.opt, p)) return rc;
  lap("launch_ord");
  return MAGOT_OK;
}

}  // namespace magot

using namespace magot;

extern "C" int magot_debug_tile_cut(const uint64_t* ex_out, uint64_t n_ex, const uint64_t* tx_nuc,
                                    const uint64_t* tx_pep, uint64_t n_rec, uint32_t lane_chunks,
                                    void* tiles, uint64_t tiles_cap, uint64_t* n_tiles) {
  if (!ex_out || !tx_nuc || !tx_pep || !n_tiles ||
      (lane_chunks != (uint32_t)kLaneChunksLarge && lane_chunks != (uint32_t)kLaneChunksSmall)) {
    set_error("magot_debug_tile_cut: bad argument");
    return MAGOT_ERR_ARG;
  }
  std::vector<TileRec> cut;
  if (int rc = cut_tiles(ex_out, n_ex, tx_nuc, tx_pep, n_rec, tile_bytes((int)lane_chunks), &cut))
    return rc;
  *n_tiles = cut.size();
  if (!tiles) return MAGOT_OK;  // the count only
  if (cut.size() > tiles_cap) {
    set_error("magot_debug_tile_cut: tile array too small");
    return MAGOT_ERR_ARG;
  }
  if (!cut.empty()) std::memcpy(tiles, cut.data(), cut.size() * sizeof(TileRec));
  return MAGOT_OK;
}

extern "C" int magot_debug_plan(const uint8_t* const* seqs, const uint64_t* lens,
                                uint32_t n_contigs, const magot_exon* exons, uint64_t n_exons,
                                const magot_tx* txs, uint64_t n_tx, uint32_t outputs,
                                uint64_t* info, uint64_t* ex_g, uint64_t* ex_out, uint64_t* tx_nuc,
                                uint64_t* tx_pep, uint64_t* lay_nuc, uint64_t* lay_pep,
                                void* tiles) {
  if (!info || (n_contigs && (!seqs || !lens))) {
    set_error("magot_debug_plan: null argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = plan_check_tables(exons, n_exons, txs, n_tx, outputs)) return rc;
  std::vector<ContigSource> src(n_contigs);
  for (uint32_t i = 0; i < n_contigs; ++i) src[i] = ContigSource{seqs[i], lens[i], 0, 0};
  HostPacked hp;
  pack_genome(src.data(), n_contigs, &hp);
  if (hp.runs.size() >= (size_t)kDirClean) {
    set_error("magot_debug_plan: too many exception runs");
    return MAGOT_ERR_ARG;
  }
  const PlanInput in{GenomeView{hp.contig_base.data(), hp.contig_len.data(), n_contigs, hp.span,
                                hp.runs.data(), hp.dir.data()},
                     exons, n_exons, txs, n_tx, plan_options(outputs)};
  Lap lap("MAGOT_PLAN_TIMING", "plan");
  PlanCount cnt;
  if (int rc = plan_count(in, &cnt)) return rc;
  const uint64_t B = cnt.B, P = cnt.P;
  TilePlan p;
  if (int rc = plan_build(in, std::move(cnt), lap, &p)) return rc;
  const uint64_t sizes[9] = {B, P, p.Ec, p.Tc, p.tiles.size(), p.lane_chunks, p.geo.ex_rows,
                             p.geo.tx_rows, p.geo.stride};
  if (!tiles) {  // sizes only
    std::memcpy(info, sizes, sizeof sizes);
    return MAGOT_OK;
  }
  if (!ex_g || !ex_out || !tx_nuc || !tx_pep || !lay_nuc || !lay_pep ||
      std::memcmp(info, sizes, sizeof sizes) != 0) {
    set_error("magot_debug_plan: tables need the sizes of a first call in info");
    return MAGOT_ERR_ARG;
  }
  std::memcpy(ex_g, p.ex_g.data(), (p.Ec + 1) * 8);
  std::memcpy(ex_out, p.ex_out.data(), (p.Ec + 1) * 8);
  std::memcpy(tx_nuc, p.tn.data(), (p.Tc + 1) * 8);
  std::memcpy(tx_pep, p.tp.data(), (p.Tc + 1) * 8);
  if (n_tx) std::memcpy(lay_nuc, p.lay_nuc.data(), n_tx * 8);
  if (n_tx) std::memcpy(lay_pep, p.lay_pep.data(), n_tx * 8);
  if (!p.tiles.empty()) std::memcpy(tiles, p.tiles.data(), p.tiles.size() * sizeof(TileRec));
  return MAGOT_OK;
}
