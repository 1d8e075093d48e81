// C ABI: mask_from_gff on the device, over a plan's output (maskplan.cpp,
// maskgen.hip; genome_tools.py:394-428).
#include "abi_internal.h"

using namespace magot;

struct magot_mask {
  magot_ctx* ctx = nullptr;
  const magot_plan* plan = nullptr;
  void* arena = nullptr;
  MaskArgs a{};
};

extern "C" {

void magot_mask_destroy(magot_mask* m) {
  if (!m) return;
  if (m->ctx) (void)hipSetDevice(m->ctx->device);
  if (m->arena) (void)hipFree(m->arena);
  delete m;
}

int magot_mask_create(magot_ctx* ctx, const magot_plan* p, const magot_maskplan* mp,
                      const uint32_t* rec_contig, const uint64_t* name_off, const uint8_t* names,
                      magot_mask** out, uint64_t* text_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!p || !mp || !out || (p->n_tx && (!rec_contig || !name_off))) {
    set_error("magot_mask_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  const uint64_t n = p->n_tx, nc = mp->contig_lens.size();
  if (!(p->args.outputs & MAGOT_OUT_NUC) || n != nc || n >= (1ull << 32)) {
    set_error("magot_mask_create: the plan must be a nucleotide plan with one record per contig");
    return MAGOT_ERR_ARG;
  }
  // each record's place in the plan's buffer; each contig's through its record
  const std::vector<uint64_t>& lay = p->genome_order ? p->lay_nuc : p->nuc_off;
  const uint64_t kNone = ~0ull;
  std::vector<uint64_t> contig_src(nc, kNone), tstart(n + 1), rsrc(n), hoff(n);
  std::vector<uint32_t> hlen(n);
  std::string hdr;
  uint64_t at = 0;
  for (uint64_t r = 0; r < n; ++r) {
    const uint32_t c = rec_contig[r];
    const uint64_t len = p->nuc_off[r + 1] - p->nuc_off[r];
    if (c >= nc || contig_src[c] != kNone || len != mp->contig_lens[c]) {
      set_error("magot_mask_create: record " + std::to_string(r) +
                " is not one whole contig of the mask plan, or its contig has a record already");
      return MAGOT_ERR_ARG;
    }
    if (name_off[r + 1] < name_off[r] || (name_off[r + 1] > name_off[r] && !names) ||
        name_off[r + 1] - name_off[r] >= (1ull << 31)) {
      set_error("magot_mask_create: bad name table");
      return MAGOT_ERR_ARG;
    }
    contig_src[c] = rsrc[r] = lay[r];
    hoff[r] = hdr.size();
    hdr += '>';
    if (name_off[r + 1] > name_off[r])
      hdr.append(reinterpret_cast<const char*>(names) + name_off[r], name_off[r + 1] - name_off[r]);
    hdr += '\n';
    hlen[r] = (uint32_t)(hdr.size() - hoff[r]);
    tstart[r] = at;
    at += hlen[r] + len + 1;  // '>' name '\n' sequence '\n'
  }
  tstart[n] = at;
  const uint64_t src_bytes = p->args.total_nuc;
  for (const magot_mask_interval& iv : mp->rows)
    if (iv.contig >= nc || (uint64_t)iv.start + iv.len > mp->contig_lens[iv.contig] ||
        contig_src[iv.contig] + iv.start + iv.len > src_bytes) {
      set_error("magot_mask_create: an interval outside its contig");
      return MAGOT_ERR_RANGE;
    }
  Building<magot_mask, magot_mask_destroy> guard{new magot_mask()};
  magot_mask* m = guard.p;
  m->ctx = ctx;
  m->plan = p;
  MaskArgs& a = m->a;
  a.flags = mp->flags;
  a.src = p->args.nuc;
  a.src_bytes = src_bytes;
  a.n_rows = mp->rows.size();
  a.cov_words = (src_bytes + 31) / 32;
  a.n_rec = n;
  a.text_bytes = at;
  Carve cv;  // the uploads go to the arena + offset: the kernels' fields are const
  const uint64_t o_rows = cv.take(&a.rows, a.n_rows);
  const uint64_t o_csrc = cv.take(&a.contig_src, nc);
  const uint64_t o_tstart = cv.take(&a.tstart, n + 1);
  const uint64_t o_rsrc = cv.take(&a.rsrc, n);
  const uint64_t o_hlen = cv.take(&a.hlen, n);
  const uint64_t o_hoff = cv.take(&a.hoff, n);
  const uint64_t o_hdr = cv.take(&a.hdr, hdr.size());
  cv.take(&a.cov, a.cov_words + 1);
  cv.take(&a.out, a.text_bytes);
  MAGOT_HIP_TRY(hipMalloc(&m->arena, cv.used + 256));
  cv.place(m->arena);
  char* base = static_cast<char*>(m->arena);
  auto up = [&](uint64_t off, const void* src, uint64_t bytes) {
    return bytes ? hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  MAGOT_HIP_TRY(up(o_rows, mp->rows.data(), a.n_rows * sizeof(magot_mask_interval)));
  MAGOT_HIP_TRY(up(o_csrc, contig_src.data(), nc * 8));
  MAGOT_HIP_TRY(up(o_tstart, tstart.data(), (n + 1) * 8));
  MAGOT_HIP_TRY(up(o_rsrc, rsrc.data(), n * 8));
  MAGOT_HIP_TRY(up(o_hlen, hlen.data(), n * 4));
  MAGOT_HIP_TRY(up(o_hoff, hoff.data(), n * 8));
  MAGOT_HIP_TRY(up(o_hdr, hdr.data(), hdr.size()));
  if (text_bytes) *text_bytes = a.text_bytes;
  *out = guard.release();
  return MAGOT_OK;
}

int magot_mask_execute(magot_ctx* ctx, magot_mask* m) {
  if (int rc = bind(ctx)) return rc;
  if (!m) {
    set_error("magot_mask_execute: null handle");
    return MAGOT_ERR_ARG;
  }
  if (!m->plan->executed) {
    set_error("magot_mask_execute: execute the extraction plan first");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(launch_mask_paint(m->a, ctx->stream));
  MAGOT_HIP_TRY(launch_mask_text(m->a, ctx->stream));
  return MAGOT_OK;
}

int magot_mask_fetch(magot_ctx* ctx, magot_mask* m, uint8_t* out, uint64_t cap) {
  if (int rc = bind(ctx)) return rc;
  if (!m || cap < m->a.text_bytes || (m->a.text_bytes && !out)) {
    set_error("magot_mask_fetch: null handle, or output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (m->a.text_bytes)
    MAGOT_HIP_TRY(hipMemcpy(out, m->a.out, m->a.text_bytes, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_mask_coverage_fetch(magot_ctx* ctx, magot_mask* m, uint32_t* words, uint64_t cap_words,
                              uint64_t* n_words) {
  if (int rc = bind(ctx)) return rc;
  if (!m) {
    set_error("magot_mask_coverage_fetch: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_words) *n_words = m->a.cov_words;
  if (!words) return MAGOT_OK;
  if (cap_words < m->a.cov_words) {
    set_error("magot_mask_coverage_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (m->a.cov_words)
    MAGOT_HIP_TRY(hipMemcpy(words, m->a.cov, m->a.cov_words * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_mask_time(magot_ctx* ctx, magot_mask* m, int iters, double* paint_ms, double* text_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!m || iters <= 0) {
    set_error("magot_mask_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (!m->plan->executed) {
    set_error("magot_mask_time: execute the extraction plan first");
    return MAGOT_ERR_STATE;
  }
  double ms[2];
  if (int rc = time_passes(ctx, iters, 2, ms, [&](int k) {
        return k ? launch_mask_text(m->a, ctx->stream) : launch_mask_paint(m->a, ctx->stream);
      }))
    return rc;
  if (paint_ms) *paint_ms = ms[0];
  if (text_ms) *text_ms = ms[1];
  return MAGOT_OK;
}

}  // extern "C"
