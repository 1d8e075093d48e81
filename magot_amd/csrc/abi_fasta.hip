// C ABI: the records of a resident FASTA text, their dict, its anti-join with a
// list of names and the reflow into one line per record (fastarec.hip;
// genome_tools.py:377-391, magot_smallfuncs.py:21-29).
#include "abi_internal.h"

using namespace magot;

struct magot_fastarec {
  magot_ctx* ctx = nullptr;
  ResidentText rt;           // the text and its line index; the status word
  void* line_mem = nullptr;  // everything sized by the lines
  void* rec_mem = nullptr;   // everything sized by the records
  void* out_mem = nullptr;   // the last rendered text and its tables
  void* copy_mem = nullptr;  // magot_fastarec_time's copy target
  FaArgs a{};
  FaRenderArgs r{};
  uint64_t out_bytes = 0;
  bool rendered = false;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

namespace {

constexpr int kFaPasses = 7;

constexpr char kOutside[] =
    "magot_fastarec_parse: input outside the device path; use the host loop";

// The plan of a render: the records on the device, every printed record's
// place and pieces, the output buffer.  Replaces the handle's last one.
int fa_plan_render(magot_fastarec* p, const uint32_t* rec, uint64_t n, uint32_t style) {
  hipStream_t s = p->ctx->stream;
  const FaArgs& a = p->a;
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (p->out_mem) MAGOT_HIP_TRY(hipFree(p->out_mem));
  p->out_mem = nullptr;
  p->rendered = false;
  p->out_bytes = 0;
  FaRenderArgs r{};
  r.n_out = n;
  r.style = style;
  if (!n) {
    p->r = r;
    return MAGOT_OK;
  }
  DevBuf plan;
  Carve cv;
  uint32_t* d_recs;  // uploaded into; the kernels read it as const
  void* tmp;
  cv.take(&d_recs, n);
  cv.take(&r.olen, n + 1);
  cv.take(&r.obase, n + 1);
  cv.take(&r.pcnt, n + 1);
  cv.take(&r.pbase, n + 1);
  size_t tmp_bytes = fa_tmp_bytes(n);
  cv.take(&tmp, tmp_bytes);
  MAGOT_HIP_TRY(hipMalloc(&plan.p, cv.used + 256));
  cv.place(plan.p);
  MAGOT_HIP_TRY(hipMemcpyAsync(d_recs, rec, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  r.recs = d_recs;
  MAGOT_HIP_TRY(launch_fa_render_sizes(a, r, tmp, tmp_bytes, s));
  uint64_t total = 0, pieces = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(&total, r.obase + n, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&pieces, r.pbase + n, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  // the tables the kernels keep reading, and the text, in one allocation
  Carve co;
  uint64_t *q_obase, *q_pbase;  // recs, obase and pbase move over from the plan
  co.take(&r.out, total + 16);
  co.take(&d_recs, n);
  co.take(&q_obase, n + 1);
  co.take(&q_pbase, n + 1);
  co.take(&r.p_src, pieces);
  co.take(&r.p_dst, pieces);
  co.take(&r.p_len, pieces);
  MAGOT_HIP_TRY(hipMalloc(&p->out_mem, co.used + 256));
  co.place(p->out_mem);
  MAGOT_HIP_TRY(hipMemcpyAsync(d_recs, r.recs, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(q_obase, r.obase, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(q_pbase, r.pbase, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));  // the plan's scratch goes
  r.recs = d_recs;
  r.olen = r.pcnt = nullptr;
  r.obase = q_obase;
  r.pbase = q_pbase;
  r.n_pieces = pieces;
  p->r = r;
  p->out_bytes = total;
  return MAGOT_OK;
}

// pass k of magot_fastarec_time on the handle's own buffers
hipError_t fa_pass(const magot_fastarec* p, int k, hipStream_t s) {
  const FaArgs& a = p->a;
  switch (k) {
    case 0: return text_index_pass(a.ix, p->rt, kTextFillLinesCr, s);
    case 1: return launch_fa_lines(a, p->tmp, p->tmp_bytes, s);
    case 2: return launch_fa_names(a, p->tmp, p->tmp_bytes, s);
    case 3: return launch_fa_sort(a, p->tmp, p->tmp_bytes, s);
    case 4:
      if (hipError_t e = launch_fa_keys(a, p->tmp, p->tmp_bytes, s)) return e;
      return launch_fa_rows(a, s);
    case 5: return launch_fa_render(a, p->r, s);
    default: return hipMemcpyAsync(p->copy_mem, a.ix.text, a.ix.n, hipMemcpyDeviceToDevice, s);
  }
}

}  // namespace

extern "C" {

void magot_fastarec_destroy(magot_fastarec* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->copy_mem) (void)hipFree(p->copy_mem);
  if (p->out_mem) (void)hipFree(p->out_mem);
  if (p->rec_mem) (void)hipFree(p->rec_mem);
  if (p->line_mem) (void)hipFree(p->line_mem);
  if (p->rt.mem) (void)hipFree(p->rt.mem);
  delete p;
}

void magot_fastarec_params(uint32_t* max_name, uint32_t* piece, uint32_t* text_block) {
  if (max_name) *max_name = kFaMaxName;
  if (piece) *piece = kFaPiece;
  if (text_block) *text_block = kTextBlock;
}

int magot_fastarec_parse(magot_ctx* ctx, const char* text, uint64_t len, uint32_t hash_bits,
                         uint64_t max_bytes, magot_fastarec** out, uint32_t* reason,
                         uint64_t* line) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text)) {
    set_error("magot_fastarec_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  if (line) *line = 0;
  if (hash_bits < 1 || hash_bits > 64) {
    set_error("magot_fastarec_parse: hash_bits outside 1..64");
    return MAGOT_ERR_ARG;
  }
  if (int rc = resident_text_budget(&max_bytes)) return rc;
  if (len > max_bytes) return decline(kOutside, reason, line, MAGOT_FASTAREC_TOO_LARGE, 0);
  if (len && text[0] != '>')
    return decline(kOutside, reason, line, MAGOT_FASTAREC_LEADING_TEXT, 1);

  Building<magot_fastarec, magot_fastarec_destroy> guard{new magot_fastarec()};
  magot_fastarec* p = guard.p;
  p->ctx = ctx;
  FaArgs& a = p->a;
  a.hash_bits = hash_bits;
  hipStream_t s = ctx->stream;
  if (len) {
    Carve cv;  // the caller's slice: the status word
    cv.take(&a.status, 1);
    if (int rc = resident_text_open(ctx, text, len, '\n', kTextNoByte, cv.used, &p->rt, &a.ix))
      return rc;
    cv.place(p->rt.extra);
    a.ix.stray_status = a.status;
    a.ix.stray_reason = MAGOT_FASTAREC_STRAY_CR;
    MAGOT_HIP_TRY(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), s));
    a.ix.n_lines = p->rt.n_lines;
    if (a.ix.n_lines > kFaMaxLines)
      return decline(kOutside, reason, line, MAGOT_FASTAREC_TOO_MANY_LINES, 0);
  }
  if (a.ix.n_lines) {
    const uint64_t L = a.ix.n_lines;
    p->tmp_bytes = fa_tmp_bytes(L);  // records and keys are at most the lines
    {
      Carve cv;
      for (uint64_t** f : {&a.ix.pos, &a.hdr, &a.pay, &a.pcs, &a.rec_of, &a.pay_pre, &a.pcs_pre})
        cv.take(f, L + 1);
      cv.take(&p->tmp, p->tmp_bytes);
      MAGOT_HIP_TRY(hipMalloc(&p->line_mem, cv.used + 256));
      cv.place(p->line_mem);
    }
    MAGOT_HIP_TRY(launch_text_fill(a.ix, kTextFillLinesCr, s));
    MAGOT_HIP_TRY(launch_fa_lines(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&a.n_rec, a.rec_of + L, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (a.n_rec > L) {
      set_error("magot_fastarec_parse: more records than lines");
      return MAGOT_ERR_STATE;
    }
    const uint64_t N = a.n_rec;
    {
      Carve cv;
      for (uint64_t** f : {&a.name_off, &a.word_off, &a.hash, &a.word_hash, &a.seq_len, &a.ne,
                           &a.ne_pos, &a.skey, &a.skey_sorted, &a.head, &a.head_pos, &a.is_first,
                           &a.kpos, &a.k_hash})
        cv.take(f, N + 1);
      for (uint32_t** f : {&a.hdr_line, &a.name_len, &a.word_len, &a.no_word, &a.sval,
                           &a.sval_sorted, &a.last_of, &a.k_first, &a.k_last, &a.k_no_word})
        cv.take(f, N + 1);
      MAGOT_HIP_TRY(hipMalloc(&p->rec_mem, cv.used + 256));
      cv.place(p->rec_mem);
    }
    MAGOT_HIP_TRY(launch_fa_names(a, p->tmp, p->tmp_bytes, s));
    unsigned long long status = 0;
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&a.n_ne, a.ne_pos + N, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (int rc = decline_if_offended(kOutside, reason, line, status)) return rc;
    if (a.n_ne > N) {
      set_error("magot_fastarec_parse: more records with a sequence than records");
      return MAGOT_ERR_STATE;
    }
    MAGOT_HIP_TRY(launch_fa_sort(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(launch_fa_keys(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&a.n_keys, a.kpos + N, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (int rc = decline_if_offended(kOutside, reason, line, status)) return rc;
    if (a.n_keys > a.n_ne) {
      set_error("magot_fastarec_parse: more keys than records with a sequence");
      return MAGOT_ERR_STATE;
    }
    MAGOT_HIP_TRY(launch_fa_rows(a, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
  }
  *out = guard.release();
  return MAGOT_OK;
}

int magot_fastarec_sizes(const magot_fastarec* p, uint64_t* n_lines, uint64_t* n_records,
                         uint64_t* n_with_sequence, uint64_t* n_keys) {
  if (!p) {
    set_error("magot_fastarec_sizes: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_lines) *n_lines = p->a.ix.n_lines;
  if (n_records) *n_records = p->a.n_rec;
  if (n_with_sequence) *n_with_sequence = p->a.n_ne;
  if (n_keys) *n_keys = p->a.n_keys;
  return MAGOT_OK;
}

double magot_fastarec_upload_ms(const magot_fastarec* p) { return p ? (double)p->rt.upload_ms : 0.0; }

int magot_fastarec_records(magot_ctx* ctx, magot_fastarec* p, uint32_t* line, uint64_t* name_off,
                           uint32_t* name_len, uint64_t* seq_len, uint64_t* hash,
                           uint64_t* word_off, uint32_t* word_len, uint64_t* word_hash,
                           uint32_t* no_word) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_records", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const FaArgs& a = p->a;
  const uint64_t n = a.n_rec;
  if (int rc = fetch_rows(line, a.hdr_line, n)) return rc;
  if (int rc = fetch_rows(name_off, a.name_off, n)) return rc;
  if (int rc = fetch_rows(name_len, a.name_len, n)) return rc;
  if (int rc = fetch_rows(seq_len, a.seq_len, n)) return rc;
  if (int rc = fetch_rows(hash, a.hash, n)) return rc;
  if (int rc = fetch_rows(word_off, a.word_off, n)) return rc;
  if (int rc = fetch_rows(word_len, a.word_len, n)) return rc;
  if (int rc = fetch_rows(word_hash, a.word_hash, n)) return rc;
  return fetch_rows(no_word, a.no_word, n);
}

int magot_fastarec_keys(magot_ctx* ctx, magot_fastarec* p, uint64_t* hash, uint32_t* first_record,
                        uint32_t* last_record, uint32_t* no_word) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_keys", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const FaArgs& a = p->a;
  const uint64_t n = a.n_keys;
  if (int rc = fetch_rows(hash, a.k_hash, n)) return rc;
  if (int rc = fetch_rows(first_record, a.k_first, n)) return rc;
  if (int rc = fetch_rows(last_record, a.k_last, n)) return rc;
  return fetch_rows(no_word, a.k_no_word, n);
}

int magot_fastarec_exclude(magot_ctx* ctx, magot_fastarec* p, const uint8_t* blob,
                           uint64_t blob_len, const uint64_t* off, uint64_t m, int first_word,
                           uint8_t* keep) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_exclude", "handle")) return rc;
  const FaArgs& a = p->a;
  if ((m && !off) || (blob_len && !blob) || (a.n_keys && !keep)) {
    set_error("magot_fastarec_exclude: null argument");
    return MAGOT_ERR_ARG;
  }
  if (m > 0xffffffffull) {
    set_error("magot_fastarec_exclude: 2^32 names or more");
    return MAGOT_ERR_RANGE;
  }
  for (uint64_t j = 0; j < m; ++j)
    if (off[j] > off[j + 1] || off[j + 1] > blob_len) {
      set_error("magot_fastarec_exclude: an offset decreases or leaves the blob");
      return MAGOT_ERR_RANGE;
    }
  if (!a.n_keys) return MAGOT_OK;
  hipStream_t s = ctx->stream;
  DevBuf buf;
  FaMemberArgs g{};
  g.m = m;
  g.first_word = first_word ? 1u : 0u;
  Carve cv;
  uint8_t* d_blob;  // uploaded into; the kernels read them as const
  uint64_t* d_off;
  void* tmp;
  cv.take(&d_blob, blob_len + 16);
  cv.take(&d_off, m + 1);
  cv.take(&g.lkey, m);
  cv.take(&g.lkey_sorted, m);
  cv.take(&g.lidx, m);
  cv.take(&g.lidx_sorted, m);
  cv.take(&g.keep, a.n_keys);
  const size_t tmp_bytes = fa_tmp_bytes(m);
  cv.take(&tmp, tmp_bytes);
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  cv.place(buf.p);
  g.blob = d_blob;
  g.off = d_off;
  if (blob_len) MAGOT_HIP_TRY(hipMemcpyAsync(d_blob, blob, blob_len, hipMemcpyHostToDevice, s));
  if (m) MAGOT_HIP_TRY(hipMemcpyAsync(d_off, off, (m + 1) * 8, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(launch_fa_member(a, g, tmp, tmp_bytes, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(keep, g.keep, a.n_keys, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  return MAGOT_OK;
}

int magot_fastarec_render(magot_ctx* ctx, magot_fastarec* p, const uint32_t* rec, uint64_t n,
                          uint32_t style, uint64_t* bytes) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_render", "handle")) return rc;
  if ((n && !rec) || !bytes || style > MAGOT_FASTAREC_STYLE_TAB) {
    set_error("magot_fastarec_render: bad argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t j = 0; j < n; ++j)
    if (rec[j] >= p->a.n_rec) {
      set_error("magot_fastarec_render: a record beyond the text's");
      return MAGOT_ERR_RANGE;
    }
  if (int rc = fa_plan_render(p, rec, n, style)) return rc;
  MAGOT_HIP_TRY(launch_fa_render(p->a, p->r, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  p->rendered = true;
  *bytes = n ? p->out_bytes : (style == MAGOT_FASTAREC_STYLE_TAB ? 1 : 0);
  return MAGOT_OK;
}

int magot_fastarec_render_fetch(magot_ctx* ctx, magot_fastarec* p, uint8_t* out, uint64_t cap) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_render_fetch", "handle")) return rc;
  if (!p->rendered) {
    set_error("magot_fastarec_render_fetch: nothing rendered");
    return MAGOT_ERR_STATE;
  }
  const uint64_t need = p->r.n_out ? p->out_bytes : (p->r.style == kFaStyleTab ? 1 : 0);
  if (cap < need || (need && !out)) {
    set_error("magot_fastarec_render_fetch: buffer too small");
    return MAGOT_ERR_ARG;
  }
  if (!p->r.n_out) {
    if (need) out[0] = '\n';  // `print ''`
    return MAGOT_OK;
  }
  MAGOT_HIP_TRY(hipMemcpy(out, p->r.out, need, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_fastarec_time(magot_ctx* ctx, magot_fastarec* p, int iters, double* ms7,
                        uint64_t* text_bytes, uint64_t* reflow_bytes) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_time", "handle")) return rc;
  if (iters <= 0 || !ms7) {
    set_error("magot_fastarec_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text_bytes) *text_bytes = p->a.ix.n;
  if (reflow_bytes) *reflow_bytes = 0;
  for (int k = 0; k < kFaPasses; ++k) ms7[k] = 0;
  if (!p->a.ix.n_lines) return MAGOT_OK;  // an empty text: nothing was launched
  if (!p->copy_mem) MAGOT_HIP_TRY(hipMalloc(&p->copy_mem, p->a.ix.n + 256));
  {  // the reflow that is timed: fasta2tab's
    std::vector<uint32_t> all(p->a.n_rec);
    for (uint64_t r = 0; r < p->a.n_rec; ++r) all[r] = (uint32_t)r;
    if (int rc = fa_plan_render(p, all.data(), all.size(), kFaStyleTab)) return rc;
    if (reflow_bytes) *reflow_bytes = p->out_bytes;
  }
  // every pass writes what it wrote in magot_fastarec_parse: the answers stand
  return time_passes(ctx, iters, kFaPasses, ms7,
                     [&](int k) { return fa_pass(p, k, ctx->stream); });
}

}  // extern "C"
