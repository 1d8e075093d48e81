// C ABI: extraction plans (tileplan.cpp, extract.hip) and the FASTA text
// assembled from a plan's output (render.hip).
#include <cstdio>
#include <cstdlib>

#include "abi_internal.h"

using namespace magot;

namespace {

// Host rows bound for one device allocation (dev_off into it).
struct HostPiece {
  uint64_t dev_off;
  const void* src;
  uint64_t bytes;
};

// Upload host rows through the context's two pinned staging buffers: host
// threads copy one 64 MiB piece in while the DMA engine drains the other (a
// pageable hipMemcpy stages through the runtime's own small buffers at a
// fraction of the link rate).  Synchronous: the rows are on the device when
// it returns.
int upload_pieces(magot_ctx* ctx, char* dev, const std::vector<HostPiece>& pieces) {
  std::lock_guard<std::mutex> lock(ctx->pin_mu);
  if (int rc = ensure_pin_ring(ctx)) return rc;
  const unsigned nt = host_threads();
  uint64_t k = 0;
  for (const HostPiece& pc : pieces)
    for (uint64_t q0 = 0; q0 < pc.bytes; q0 += kPinRing, ++k) {
      const int b = (int)(k & 1);
      const uint64_t q1 = std::min(pc.bytes, q0 + kPinRing);
      MAGOT_HIP_TRY(hipEventSynchronize(ctx->pin_ev[b]));
      const char* src = static_cast<const char*>(pc.src) + q0;
      uint8_t* ring = ctx->pin[b];
      parallel_ranges(q1 - q0, q1 - q0 >= (4ull << 20) ? nt : 1u,
                      [&](uint64_t lo, uint64_t hi, unsigned) { memcpy(ring + lo, src + lo, hi - lo); });
      MAGOT_HIP_TRY(hipMemcpyAsync(dev + pc.dev_off + q0, ring, q1 - q0, hipMemcpyHostToDevice,
                                   ctx->stream));
      MAGOT_HIP_TRY(hipEventRecord(ctx->pin_ev[b], ctx->stream));
    }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

// As upload_pieces for rows that are generated, not copied: fill(lo, hi, dst)
// writes items [lo, hi) of `item` bytes each to dst, from several host threads
// straight into the pinned buffer that is uploaded next (no pageable copy of
// the table and no second pass over it).
template <class F>
int upload_generated(magot_ctx* ctx, char* dev, uint64_t n, uint64_t item, unsigned threads, F fill) {
  std::lock_guard<std::mutex> lock(ctx->pin_mu);
  if (int rc = ensure_pin_ring(ctx)) return rc;
  const uint64_t per = kPinRing / item;
  for (uint64_t i0 = 0, k = 0; i0 < n; i0 += per, ++k) {
    const int b = (int)(k & 1);
    const uint64_t i1 = std::min(n, i0 + per);
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->pin_ev[b]));
    uint8_t* ring = ctx->pin[b];
    parallel_ranges(i1 - i0, (i1 - i0) * item >= (1ull << 20) ? threads : 1u,
                    [&](uint64_t lo, uint64_t hi, unsigned) { fill(i0 + lo, i0 + hi, ring + lo * item); });
    MAGOT_HIP_TRY(hipMemcpyAsync(dev + i0 * item, ring, (i1 - i0) * item, hipMemcpyHostToDevice,
                                 ctx->stream));
    MAGOT_HIP_TRY(hipEventRecord(ctx->pin_ev[b], ctx->stream));
  }
  return MAGOT_OK;  // in flight: the caller's next upload_pieces (or a stream sync) completes it
}

// A genome-ordered plan's output (nucleotides, or residues) put back into
// record order at dst (16-byte aligned device memory): one segment copy per
// record from its layout place to its record-order offset, on the context stream.
int plan_reassemble(magot_ctx* ctx, const magot_plan* p, bool residues, void* dst) {
  if (!p->n_tx) return MAGOT_OK;
  launch_segments_copy(residues ? p->args.pep : p->args.nuc,
                       residues ? p->d_lay_pep : p->d_lay_nuc,
                       residues ? p->d_pep_off : p->d_nuc_off, p->n_tx,
                       static_cast<uint8_t*>(dst), ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  return MAGOT_OK;
}

// A genome-ordered plan's output copied down in record order through a
// bounded device scratch: consecutive records in batches of at most
// kFetchBatchBytes (or one longer record) are put back into record order on
// the device (one segment-copy launch per batch), then copied to the host.
// The scratch is 16-byte aligned and the batch's first record keeps its
// offset mod 16, so the copy kernel's aligned stores stay aligned.
constexpr uint64_t kFetchBatchBytes = 256ull << 20;

uint64_t fetch_batch_bytes() {  // MAGOT_FETCH_BATCH_BYTES: test hook (small batches)
  const char* e = std::getenv("MAGOT_FETCH_BATCH_BYTES");
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? v : kFetchBatchBytes;
}

int plan_fetch_reordered(magot_ctx* ctx, const magot_plan* p, bool residues, uint8_t* host) {
  const std::vector<uint64_t>& off = residues ? p->pep_off : p->nuc_off;
  const uint64_t T = p->n_tx;
  if (!T || off[T] == 0) return MAGOT_OK;
  uint64_t longest = 0;
  for (uint64_t t = 0; t < T; ++t) longest = std::max(longest, off[t + 1] - off[t]);
  const uint64_t cap = std::max(std::min(off[T], fetch_batch_bytes()), longest);
  DevBuf scratch;
  MAGOT_HIP_TRY(hipMalloc(&scratch.p, cap + 16));
  uint8_t* S = static_cast<uint8_t*>(scratch.p);
  const uint8_t* src = residues ? p->args.pep : p->args.nuc;
  const uint64_t* lay = residues ? p->d_lay_pep : p->d_lay_nuc;
  const uint64_t* doff = residues ? p->d_pep_off : p->d_nuc_off;
  for (uint64_t r0 = 0; r0 < T;) {
    uint64_t r1 = r0 + 1;
    while (r1 < T && off[r1 + 1] - off[r0] <= cap) ++r1;
    const uint64_t base = off[r0], bytes = off[r1] - base;
    if (bytes) {
      // record-order offset x lands at S + (x - (base & ~15))
      launch_segments_copy(src, lay + r0, doff + r0, r1 - r0, S - (base & ~15ull), ctx->stream);
      MAGOT_HIP_TRY(hipGetLastError());
      MAGOT_HIP_TRY(hipMemcpyAsync(host + base, S + (base & 15), bytes, hipMemcpyDeviceToHost,
                                   ctx->stream));
    }
    r0 = r1;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

}  // namespace

extern "C" {

// The planning is tileplan.cpp's (host only); here: the device side of a plan.
int magot_plan_create(magot_ctx* ctx, const magot_genome* g, const magot_exon* exons,
                      uint64_t n_exons, const magot_tx* txs, uint64_t n_tx, uint32_t outputs,
                      magot_plan** out, uint64_t* nuc_bytes, uint64_t* pep_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!g || !out) {
    set_error("magot_plan_create: null argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = plan_check_tables(exons, n_exons, txs, n_tx, outputs)) return rc;
  *out = nullptr;
  Lap lap("MAGOT_PLAN_TIMING", "plan");
  const PlanInput in{GenomeView{g->contig_base.data(), g->contig_len.data(), g->contig_base.size(),
                                g->span, g->host_runs.data(), g->host_dir.data()},
                     exons, n_exons, txs, n_tx, plan_options(outputs)};
  const bool by_genome = in.opt.by_genome;
  PlanCount cnt;
  if (int rc = plan_count(in, &cnt)) return rc;
  const uint64_t T = n_tx, B = cnt.B, P = cnt.P;
  // The output buffers' size is known now: allocate them on another thread
  // while this one plans.
  const uint64_t out_nuc = (in.opt.outputs & MAGOT_OUT_NUC) ? B + 64 : 64;
  const uint64_t out_pep = (in.opt.outputs & MAGOT_OUT_PEP) ? P + 64 : 64;
  const uint64_t out_bytes = ((out_nuc + 255) & ~255ull) + out_pep;
  AsyncAlloc out_alloc(ctx->device, out_bytes);
  TilePlan pl;
  if (int rc = plan_build(in, std::move(cnt), lap, &pl)) return rc;
  const uint32_t n_tiles = (uint32_t)pl.tiles.size();
  const TileGeometry geo = pl.geo;

  // --- device arena -----------------------------------------------------------
  std::unique_ptr<magot_plan> p(new magot_plan());
  p->ctx = ctx;
  p->g = g;
  Carve cv;
  // The device holds the tiles' packed blocks and their overflow rows, not
  // the u64 tables they are packed from.
  const uint64_t o_blocks = cv.take(&p->args.blocks, (uint64_t)n_tiles * geo.stride);
  const uint64_t o_ovf_ex = cv.take(&p->args.ovf_ex, pl.n_ovf_ex + 1);
  const uint64_t o_ovf_tx = cv.take(&p->args.ovf_tx, pl.n_ovf_tx + 1);
  // genome order: {layout place, record-order offsets} per output, for the
  // reassembly copies (magot_plan_fetch / copy_outputs)
  const uint64_t lay_rows = by_genome ? T : 0;
  const uint64_t o_lay_nuc = cv.take<uint64_t>(lay_rows);
  const uint64_t o_rec_nuc = cv.take<uint64_t>(by_genome ? T + 1 : 0);
  const uint64_t o_lay_pep = cv.take<uint64_t>(lay_rows);
  const uint64_t o_rec_pep = cv.take<uint64_t>(by_genome ? T + 1 : 0);
  MAGOT_HIP_TRY(hipMalloc(&p->arena, cv.used));
  cv.place(p->arena);
  p->arena_bytes = cv.used;
  const hipError_t out_err = out_alloc.take(&p->out_arena);
  MAGOT_HIP_TRY(out_err);
  p->out_bytes = out_bytes;
  lap("malloc");
  char* base = static_cast<char*>(p->arena);
  // Blocks are packed by the host threads straight into the upload's pinned
  // buffers, tile ranges in parallel; a tile's overflow rows go to its place
  // in the (small) overflow arrays, uploaded after.
  HostBuf<uint64_t> ovf_ex(pl.n_ovf_ex + 1);
  HostBuf<TxRow> ovf_tx(pl.n_ovf_tx + 1);
  ovf_ex[pl.n_ovf_ex] = 0;
  ovf_tx[pl.n_ovf_tx] = TxRow{0, 0};
  const TileTables tb{pl.ex_g.data(), pl.ex_out.data(), pl.tn.data(), pl.tp.data(), g->span,
                      pl.lane_chunks};
  if (int rc = upload_generated(
          ctx, base + o_blocks, n_tiles, geo.stride, n_tiles >= (1u << 12) ? pl.nth : 1u,
          [&](uint64_t t0, uint64_t t1, uint8_t* dst) {
            for (uint64_t t = t0; t < t1; ++t)
              pack_tile_block(tb, geo, pl.tiles[t], pl.ovf_at[2 * t], pl.ovf_at[2 * t + 1],
                              dst + (t - t0) * geo.stride, ovf_ex.data(), ovf_tx.data());
          }))
    return rc;
  lap("blocks");
  std::vector<HostPiece> pieces = {{o_ovf_ex, ovf_ex.data(), (pl.n_ovf_ex + 1) * 8},
                                   {o_ovf_tx, ovf_tx.data(), (pl.n_ovf_tx + 1) * sizeof(TxRow)}};
  if (by_genome) {
    pieces.push_back({o_lay_nuc, pl.lay_nuc.data(), T * 8});
    pieces.push_back({o_rec_nuc, pl.nuc_off.data(), (T + 1) * 8});
    pieces.push_back({o_lay_pep, pl.lay_pep.data(), T * 8});
    pieces.push_back({o_rec_pep, pl.pep_off.data(), (T + 1) * 8});
  }
  if (int rc = upload_pieces(ctx, base, pieces)) return rc;
  if (by_genome) {
    p->genome_order = true;
    p->d_lay_nuc = reinterpret_cast<const uint64_t*>(base + o_lay_nuc);
    p->d_nuc_off = reinterpret_cast<const uint64_t*>(base + o_rec_nuc);
    p->d_lay_pep = reinterpret_cast<const uint64_t*>(base + o_lay_pep);
    p->d_pep_off = reinterpret_cast<const uint64_t*>(base + o_rec_pep);
  }
  lap("upload");
  if (lap.on) {  // everything in the arena is uploaded once, here
    uint64_t up = (uint64_t)n_tiles * geo.stride;
    for (const HostPiece& pc : pieces) up += pc.bytes;
    fprintf(stderr,
            "[plan] tiles %u, block rows %u + %u (%u bytes), overflow rows %llu + %llu, arena %llu "
            "bytes, uploaded %llu\n",
            n_tiles, geo.ex_rows, geo.tx_rows, geo.stride, (unsigned long long)pl.n_ovf_ex,
            (unsigned long long)pl.n_ovf_tx, (unsigned long long)cv.used, (unsigned long long)up);
  }

  ExtractArgs& a = p->args;
  a.nib = g->nib;
  a.span = g->span;
  a.runs = g->runs;
  a.dir = g->dir;
  a.blk = geo;
  a.nuc = static_cast<uint8_t*>(p->out_arena);
  a.pep = static_cast<uint8_t*>(p->out_arena) + ((out_nuc + 255) & ~255ull);
  a.total_nuc = B;
  a.total_pep = P;
  a.n_tiles = n_tiles;
  a.outputs = in.opt.outputs;
  a.lane_chunks = pl.lane_chunks;
  if (const char* dbg = std::getenv("MAGOT_DEBUG_PATHS")) {
    const int v = std::atoi(dbg);
    if (v & 1) a.outputs |= kDebugSlowNuc;
    if (v & 2) a.outputs |= kDebugSlowPep;
  }
  uint8_t lut[64];
  standard_lut(lut);
  std::memcpy(a.lut, lut, 64);

  p->nuc_off = std::move(pl.nuc_off);
  p->pep_off = std::move(pl.pep_off);
  p->lay_nuc = std::move(pl.lay_nuc);
  p->lay_pep = std::move(pl.lay_pep);
  p->n_exons = n_exons;
  p->n_ex_c = pl.Ec;
  p->n_tx = T;
  if (!by_genome) {  // magot_plan_orf6's rows (it refuses a genome-order plan)
    p->host_ex_g = std::move(pl.ex_g.p);
    p->host_ex_out = std::move(pl.ex_out.p);
  }
  if (nuc_bytes) *nuc_bytes = B;
  if (pep_bytes) *pep_bytes = P;
  *out = p.release();
  return MAGOT_OK;
}

void magot_plan_destroy(magot_plan* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->arena) (void)hipFree(p->arena);
  if (p->out_arena) (void)hipFree(p->out_arena);
  delete p;
}

int magot_plan_execute(magot_ctx* ctx, magot_plan* p) {
  if (int rc = bind(ctx)) return rc;
  if (!p) {
    set_error("magot_plan_execute: null plan");
    return MAGOT_ERR_ARG;
  }
  launch_extract(p->args, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  p->executed = true;
  return MAGOT_OK;
}

int magot_plan_fetch(magot_ctx* ctx, magot_plan* p, uint8_t* nuc_out, uint64_t* nuc_off,
                     uint8_t* pep_out, uint64_t* pep_off) {
  if (int rc = bind(ctx)) return rc;
  if (!p) {
    set_error("magot_plan_fetch: null plan");
    return MAGOT_ERR_ARG;
  }
  if (!p->executed) {
    set_error("magot_plan_fetch: plan not executed");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if ((nuc_out && p->args.total_nuc && !(p->args.outputs & MAGOT_OUT_NUC)) ||
      (pep_out && p->args.total_pep && !(p->args.outputs & MAGOT_OUT_PEP))) {
    set_error(std::string("magot_plan_fetch: plan built without ") +
              (nuc_out && !(p->args.outputs & MAGOT_OUT_NUC) ? "MAGOT_OUT_NUC" : "MAGOT_OUT_PEP"));
    return MAGOT_ERR_STATE;
  }
  const bool want_nuc = nuc_out && p->args.total_nuc, want_pep = pep_out && p->args.total_pep;
  if (want_nuc) {
    if (p->genome_order) {
      if (int rc = plan_fetch_reordered(ctx, p, false, nuc_out)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(nuc_out, p->args.nuc, p->args.total_nuc,
                                   hipMemcpyDeviceToHost, ctx->stream));
      MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  }
  if (want_pep) {
    if (p->genome_order) {
      if (int rc = plan_fetch_reordered(ctx, p, true, pep_out)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(pep_out, p->args.pep, p->args.total_pep,
                                   hipMemcpyDeviceToHost, ctx->stream));
      MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  }
  if (nuc_off) std::memcpy(nuc_off, p->nuc_off.data(), p->nuc_off.size() * 8);
  if (pep_off) std::memcpy(pep_off, p->pep_off.data(), p->pep_off.size() * 8);
  return MAGOT_OK;
}

int magot_run(magot_ctx* ctx, magot_plan* p, uint8_t* nuc_out, uint64_t* nuc_off, uint8_t* pep_out,
              uint64_t* pep_off) {
  if (int rc = magot_plan_execute(ctx, p)) return rc;
  return magot_plan_fetch(ctx, p, nuc_out, nuc_off, pep_out, pep_off);
}

int magot_plan_time(magot_ctx* ctx, magot_plan* p, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!p || iters <= 0 || !avg_ms) {
    set_error("magot_plan_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = time_passes(ctx, iters, 1, avg_ms, [&](int) {
        launch_extract(p->args, ctx->stream);
        return hipGetLastError();
      }))
    return rc;
  p->executed = true;
  return MAGOT_OK;
}

int magot_plan_time_b2b(magot_ctx* ctx, magot_plan* p, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!p || iters <= 0 || !avg_ms) {
    set_error("magot_plan_time_b2b: bad argument");
    return MAGOT_ERR_ARG;
  }
  // one event pair around `iters` back-to-back launches: the per-launch time
  // of a step loop (no host round trip between launches)
  double ms = 0.0;
  if (int rc = time_pass(ctx, &ms, [&] {
        for (int i = 0; i < iters; ++i) launch_extract(p->args, ctx->stream);
        return hipGetLastError();
      }))
    return rc;
  p->executed = true;
  *avg_ms = ms / iters;
  return MAGOT_OK;
}

int magot_plan_copy_outputs(magot_ctx* ctx, magot_plan* p, void* nuc_dst_dev, void* pep_dst_dev) {
  if (int rc = bind(ctx)) return rc;
  if (!p) {
    set_error("magot_plan_copy_outputs: null plan");
    return MAGOT_ERR_ARG;
  }
  if (p->genome_order && ((nuc_dst_dev && (reinterpret_cast<uintptr_t>(nuc_dst_dev) & 15)) ||
                          (pep_dst_dev && (reinterpret_cast<uintptr_t>(pep_dst_dev) & 15)))) {
    set_error("magot_plan_copy_outputs: a genome-ordered plan needs 16-byte aligned destinations");
    return MAGOT_ERR_ARG;
  }
  if (nuc_dst_dev && p->args.total_nuc && (p->args.outputs & MAGOT_OUT_NUC)) {
    if (p->genome_order) {
      if (int rc = plan_reassemble(ctx, p, false, nuc_dst_dev)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(nuc_dst_dev, p->args.nuc, p->args.total_nuc,
                                   hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  if (pep_dst_dev && p->args.total_pep && (p->args.outputs & MAGOT_OUT_PEP)) {
    if (p->genome_order) {
      if (int rc = plan_reassemble(ctx, p, true, pep_dst_dev)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(pep_dst_dev, p->args.pep, p->args.total_pep,
                                   hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

int magot_plan_layout(const magot_plan* p, uint64_t* nuc_start, uint64_t* pep_start) {
  if (!p) {
    set_error("magot_plan_layout: null plan");
    return MAGOT_ERR_ARG;
  }
  const uint64_t T = p->n_tx;
  if (nuc_start) {
    if (p->genome_order) std::memcpy(nuc_start, p->lay_nuc.data(), T * 8);
    else std::memcpy(nuc_start, p->nuc_off.data(), T * 8);
  }
  if (pep_start) {
    if (p->genome_order) std::memcpy(pep_start, p->lay_pep.data(), T * 8);
    else std::memcpy(pep_start, p->pep_off.data(), T * 8);
  }
  return MAGOT_OK;
}

int magot_plan_device_outputs(magot_plan* p, void** nuc_dev, void** pep_dev) {
  if (!p) {
    set_error("magot_plan_device_outputs: null plan");
    return MAGOT_ERR_ARG;
  }
  if (nuc_dev) *nuc_dev = p->args.nuc;
  if (pep_dev) *pep_dev = p->args.pep;
  return MAGOT_OK;
}

uint64_t magot_plan_algorithmic_bytes(const magot_plan* p) {
  if (!p) return 0;
  const uint64_t B = p->args.total_nuc, P = p->args.total_pep;
  uint64_t bytes = (B + 3) / 4 + 16 * p->n_exons + 32 * p->n_tx;
  if (p->args.outputs & MAGOT_OUT_NUC) bytes += B;
  if (p->args.outputs & MAGOT_OUT_PEP) bytes += P;
  return bytes;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// FASTA text assembly on device (render.hip)
// ---------------------------------------------------------------------------

struct magot_fasta_text {
  magot_ctx* ctx = nullptr;
  const magot_plan* plan = nullptr;
  void* arena = nullptr;
  const TextUnit* units = nullptr;
  const uint64_t* roff = nullptr;
  const uint8_t* text = nullptr;
  uint64_t* len = nullptr;
  uint64_t* psrc = nullptr;  // each unit's payload start in the plan's buffer
  uint64_t* end = nullptr;
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  uint8_t* out = nullptr;
  uint64_t n_units = 0, cap = 0;
  int protein = 0;
  void launch(hipStream_t s) const {
    launch_text_assembly(units, n_units, roff, protein ? plan->args.pep : plan->args.nuc,
                         protein, text, len, psrc, end, scan_tmp, scan_bytes, out, s);
  }
};

extern "C" {

int magot_fasta_text_create(magot_ctx* ctx, const magot_gffplan* gp, const magot_plan* p,
                            magot_fasta_text** out, uint64_t* max_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!gp || !p || !out) {
    set_error("magot_fasta_text_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  const std::string* text = nullptr;
  std::vector<TextUnit> units;
  bool protein = false;
  uint64_t n_rec = 0;
  if (!gffplan_units(gp, &text, &units, &protein, &n_rec)) {
    set_error("magot_fasta_text_create: too many records, or longest=True protein choices "
              "(magot_gffplan_selections; render those on the host)");
    return MAGOT_ERR_ARG;
  }
  if (n_rec != p->n_tx || !(p->args.outputs & (protein ? MAGOT_OUT_PEP : MAGOT_OUT_NUC))) {
    set_error("magot_fasta_text_create: the plan was not built from this skeleton's tables");
    return MAGOT_ERR_ARG;
  }
  std::unique_ptr<magot_fasta_text> o(new magot_fasta_text());
  o->ctx = ctx;
  o->plan = p;
  o->protein = protein;
  o->n_units = units.size();
  // each record's {start, end} in the plan's device buffer (its layout order)
  const std::vector<uint64_t>& roff = protein ? p->pep_off : p->nuc_off;
  const std::vector<uint64_t>& lay = p->genome_order ? (protein ? p->lay_pep : p->lay_nuc) : roff;
  std::vector<uint64_t> span(2 * n_rec);
  for (uint64_t r = 0; r < n_rec; ++r) {
    span[2 * r] = lay[r];
    span[2 * r + 1] = lay[r] + (roff[r + 1] - roff[r]);
  }
  o->cap = text->size() + (roff.empty() ? 0 : roff.back());
  o->scan_bytes = text_scan_bytes(o->n_units);
  Carve cv;
  // the uploads go to the arena + offset: the kernels' fields are const
  const uint64_t o_units = cv.take(&o->units, o->n_units);
  const uint64_t o_roff = cv.take(&o->roff, span.size());
  const uint64_t o_text = cv.take(&o->text, text->size());
  cv.take(&o->len, o->n_units);
  cv.take(&o->psrc, o->n_units);
  cv.take(&o->end, o->n_units);
  cv.take(&o->scan_tmp, o->scan_bytes);
  cv.take(&o->out, o->cap);
  MAGOT_HIP_TRY(hipMalloc(&o->arena, cv.used));
  cv.place(o->arena);
  char* base = static_cast<char*>(o->arena);
  if (!units.empty())
    MAGOT_HIP_TRY(hipMemcpy(base + o_units, units.data(), units.size() * sizeof(TextUnit),
                            hipMemcpyHostToDevice));
  if (!span.empty())
    MAGOT_HIP_TRY(hipMemcpy(base + o_roff, span.data(), span.size() * 8, hipMemcpyHostToDevice));
  if (!text->empty())
    MAGOT_HIP_TRY(hipMemcpy(base + o_text, text->data(), text->size(), hipMemcpyHostToDevice));
  if (max_bytes) *max_bytes = o->cap;
  *out = o.release();
  return MAGOT_OK;
}

int magot_fasta_text_execute(magot_ctx* ctx, magot_fasta_text* o) {
  if (int rc = bind(ctx)) return rc;
  if (!o) {
    set_error("magot_fasta_text_execute: null handle");
    return MAGOT_ERR_ARG;
  }
  if (!o->plan->executed) {
    set_error("magot_fasta_text_execute: execute the extraction plan first");
    return MAGOT_ERR_ARG;
  }
  o->launch(ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  return MAGOT_OK;
}

int magot_fasta_text_fetch(magot_ctx* ctx, magot_fasta_text* o, uint8_t* out, uint64_t cap,
                           uint64_t* out_len) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !out_len) {
    set_error("magot_fasta_text_fetch: null argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  uint64_t n = 0;
  if (o->n_units)
    MAGOT_HIP_TRY(hipMemcpy(&n, o->end + o->n_units - 1, 8, hipMemcpyDeviceToHost));
  *out_len = n;
  if (!out) return MAGOT_OK;
  if (cap < n) {
    set_error("magot_fasta_text_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  if (n) MAGOT_HIP_TRY(hipMemcpy(out, o->out, n, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_fasta_text_time(magot_ctx* ctx, magot_fasta_text* o, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !avg_ms || iters <= 0) {
    set_error("magot_fasta_text_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  return time_passes(ctx, iters, 1, avg_ms,
                     [&](int) { return o->launch(ctx->stream), hipSuccess; });
}

void magot_fasta_text_destroy(magot_fasta_text* o) {
  if (!o) return;
  if (o->ctx) (void)hipSetDevice(o->ctx->device);
  if (o->arena) (void)hipFree(o->arena);
  delete o;
}

}  // extern "C"
