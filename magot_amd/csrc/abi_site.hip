// C ABI: composition_by_site's counting pass over a resident genome
// (sitecount.hip; genome_tools.py:488-503).  The renderer from counts to the
// tool's text is host only: sitehost.cpp.
#include "abi_internal.h"

using namespace magot;

struct magot_site {
  magot_ctx* ctx = nullptr;
  const magot_genome* g = nullptr;
  void* mem = nullptr;  // the row starts, then the counts
  SiteArgs a{};
  bool executed = false;
};

extern "C" {

void magot_site_params(uint32_t* sites_per_lane, uint32_t* sites_per_tile, uint32_t* rows_per_strip,
                       uint32_t* widen4_rows, uint32_t* widen8_rows) {
  if (sites_per_lane) *sites_per_lane = kSiteLane;
  if (sites_per_tile) *sites_per_tile = kSiteTile;
  if (rows_per_strip) *rows_per_strip = kSiteStrip;
  if (widen4_rows) *widen4_rows = kSiteWiden4;
  if (widen8_rows) *widen8_rows = kSiteWiden8;
}

void magot_site_destroy(magot_site* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->mem) (void)hipFree(p->mem);
  delete p;
}

int magot_site_create(magot_ctx* ctx, const magot_genome* g, const uint32_t* contig,
                      const uint64_t* offset, uint64_t n_rows, uint64_t n_sites, magot_site** out) {
  if (int rc = handle_of(ctx, g, "magot_site_create", "genome")) return rc;
  if (!out) {
    set_error("magot_site_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (!n_sites || !n_rows) {
    set_error("magot_site_create: no sites, or no rows");
    return MAGOT_ERR_ARG;
  }
  if (!contig || !offset) {
    set_error("magot_site_create: null argument");
    return MAGOT_ERR_ARG;
  }
  if (n_rows >= (1ull << 32)) {  // a site's count is 32 bits wide
    set_error("magot_site_create: 2^32 rows or more");
    return MAGOT_ERR_ARG;
  }
  std::vector<uint64_t> start(n_rows);
  for (uint64_t r = 0; r < n_rows; ++r) {
    const uint64_t c = contig[r];
    if (c >= g->contig_len.size() || offset[r] > g->contig_len[c] ||
        n_sites > g->contig_len[c] - offset[r]) {
      set_error("magot_site_create: row " + std::to_string(r) +
                " names no contig, or runs past its contig's end");
      return MAGOT_ERR_RANGE;
    }
    start[r] = g->contig_base[c] + offset[r];
  }
  const uint64_t n_tiles = (n_sites + kSiteTile - 1) / kSiteTile;
  const uint64_t n_strips = (n_rows + kSiteStrip - 1) / kSiteStrip;
  if (n_tiles * n_strips > 0x7fffffffull) {
    set_error("magot_site_create: more workgroups than a grid holds");
    return MAGOT_ERR_ARG;
  }
  Building<magot_site, magot_site_destroy> guard{new magot_site()};
  magot_site* p = guard.p;
  p->ctx = ctx;
  p->g = g;
  SiteArgs& a = p->a;
  Carve cv;
  uint64_t* d_start;  // uploaded into; the kernel reads it as const
  cv.take(&d_start, n_rows);
  cv.take(&a.counts, n_sites * 4);
  MAGOT_HIP_TRY(hipMalloc(&p->mem, cv.used + 256));
  cv.place(p->mem);
  MAGOT_HIP_TRY(hipMemcpyAsync(d_start, start.data(), n_rows * sizeof(uint64_t),
                               hipMemcpyHostToDevice, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));  // `start` goes out of scope
  a.nib = g->nib;
  a.row_start = d_start;
  a.n_rows = n_rows;
  a.n_sites = n_sites;
  a.n_tiles = (uint32_t)n_tiles;
  a.n_strips = (uint32_t)n_strips;
  *out = guard.release();
  return MAGOT_OK;
}

int magot_site_execute(magot_ctx* ctx, magot_site* p) {
  if (int rc = handle_of(ctx, p, "magot_site_execute", "handle")) return rc;
  MAGOT_HIP_TRY(launch_site_count(p->a, ctx->stream));
  p->executed = true;
  return MAGOT_OK;
}

int magot_site_counts(magot_ctx* ctx, magot_site* p, uint32_t* counts) {
  if (int rc = handle_of(ctx, p, "magot_site_counts", "handle")) return rc;
  if (!counts) {
    set_error("magot_site_counts: null buffer");
    return MAGOT_ERR_ARG;
  }
  if (!p->executed) {
    set_error("magot_site_counts: before magot_site_execute");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(hipMemcpyAsync(counts, p->a.counts, p->a.n_sites * 4 * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

int magot_site_time(magot_ctx* ctx, magot_site* p, int iters, double* ms) {
  if (int rc = handle_of(ctx, p, "magot_site_time", "handle")) return rc;
  if (iters <= 0 || !ms) {
    set_error("magot_site_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = time_passes(ctx, iters, 1, ms,
                           [&](int) { return launch_site_count(p->a, ctx->stream); }))
    return rc;
  p->executed = true;  // every run writes the same counts
  return MAGOT_OK;
}

}  // extern "C"
