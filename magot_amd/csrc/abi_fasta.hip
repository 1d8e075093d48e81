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

int fa_decline(uint32_t* reason, uint64_t* line, uint32_t why, uint64_t at) {
  if (reason) *reason = why;
  if (line) *line = at;
  set_error("magot_fastarec_parse: input outside the device path; use the host loop");
  return MAGOT_ERR_UNSUPPORTED;
}

template <class T>
int fa_fetch(T* dst, const T* src, uint64_t n) {
  if (dst && n) MAGOT_HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

template <class T>
T* at(char* base, uint64_t off) {
  return reinterpret_cast<T*>(base + off);
}

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
  const uint64_t o_recs = cv.take<uint32_t>(n);
  const uint64_t o_olen = cv.take<uint64_t>(n + 1), o_obase = cv.take<uint64_t>(n + 1);
  const uint64_t o_pcnt = cv.take<uint64_t>(n + 1), o_pbase = cv.take<uint64_t>(n + 1);
  size_t tmp_bytes = fa_tmp_bytes(n);
  const uint64_t o_tmp = cv.take<uint8_t>(tmp_bytes);
  MAGOT_HIP_TRY(hipMalloc(&plan.p, cv.used + 256));
  char* base = static_cast<char*>(plan.p);
  MAGOT_HIP_TRY(hipMemcpyAsync(base + o_recs, rec, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  r.recs = at<uint32_t>(base, o_recs);
  r.olen = at<uint64_t>(base, o_olen);
  r.obase = at<uint64_t>(base, o_obase);
  r.pcnt = at<uint64_t>(base, o_pcnt);
  r.pbase = at<uint64_t>(base, o_pbase);
  MAGOT_HIP_TRY(launch_fa_render_sizes(a, r, base + o_tmp, tmp_bytes, s));
  uint64_t total = 0, pieces = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(&total, r.obase + n, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&pieces, r.pbase + n, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  // the tables the kernels keep reading, and the text, in one allocation
  Carve co;
  const uint64_t q_out = co.take<uint8_t>(total + 16);
  const uint64_t q_recs = co.take<uint32_t>(n);
  const uint64_t q_obase = co.take<uint64_t>(n + 1), q_pbase = co.take<uint64_t>(n + 1);
  const uint64_t q_src = co.take<uint64_t>(pieces), q_dst = co.take<uint64_t>(pieces);
  const uint64_t q_len = co.take<uint32_t>(pieces);
  MAGOT_HIP_TRY(hipMalloc(&p->out_mem, co.used + 256));
  char* ob = static_cast<char*>(p->out_mem);
  MAGOT_HIP_TRY(hipMemcpyAsync(ob + q_recs, r.recs, n * sizeof(uint32_t),
                               hipMemcpyDeviceToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(ob + q_obase, r.obase, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(ob + q_pbase, r.pbase, (n + 1) * 8, hipMemcpyDeviceToDevice, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));  // the plan's scratch goes
  r.recs = at<uint32_t>(ob, q_recs);
  r.olen = r.pcnt = nullptr;
  r.obase = at<uint64_t>(ob, q_obase);
  r.pbase = at<uint64_t>(ob, q_pbase);
  r.n_pieces = pieces;
  r.p_src = at<uint64_t>(ob, q_src);
  r.p_dst = at<uint64_t>(ob, q_dst);
  r.p_len = at<uint32_t>(ob, q_len);
  r.out = at<uint8_t>(ob, q_out);
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
  if (len > max_bytes) return fa_decline(reason, line, MAGOT_FASTAREC_TOO_LARGE, 0);
  if (len && text[0] != '>') return fa_decline(reason, line, MAGOT_FASTAREC_LEADING_TEXT, 1);

  struct Guard {
    magot_fastarec* p;
    ~Guard() { magot_fastarec_destroy(p); }
  } guard{new magot_fastarec()};
  magot_fastarec* p = guard.p;
  p->ctx = ctx;
  FaArgs& a = p->a;
  a.hash_bits = hash_bits;
  hipStream_t s = ctx->stream;
  if (len) {
    if (int rc = resident_text_open(ctx, text, len, '\n', kTextNoByte, sizeof(unsigned long long),
                                    &p->rt, &a.ix))
      return rc;
    a.status = a.ix.stray_status = reinterpret_cast<unsigned long long*>(p->rt.extra);
    a.ix.stray_reason = MAGOT_FASTAREC_STRAY_CR;
    MAGOT_HIP_TRY(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), s));
    a.ix.n_lines = p->rt.n_lines;
    if (a.ix.n_lines > kFaMaxLines) return fa_decline(reason, line, MAGOT_FASTAREC_TOO_MANY_LINES, 0);
  }
  if (a.ix.n_lines) {
    const uint64_t L = a.ix.n_lines;
    p->tmp_bytes = fa_tmp_bytes(L);  // records and keys are at most the lines
    {
      Carve cv;
      uint64_t o[7];
      for (uint64_t& x : o) x = cv.take<uint64_t>(L + 1);
      const uint64_t o_tmp = cv.take<uint8_t>(p->tmp_bytes);
      MAGOT_HIP_TRY(hipMalloc(&p->line_mem, cv.used + 256));
      char* base = static_cast<char*>(p->line_mem);
      a.ix.pos = at<uint64_t>(base, o[0]);
      a.hdr = at<uint64_t>(base, o[1]);
      a.pay = at<uint64_t>(base, o[2]);
      a.pcs = at<uint64_t>(base, o[3]);
      a.rec_of = at<uint64_t>(base, o[4]);
      a.pay_pre = at<uint64_t>(base, o[5]);
      a.pcs_pre = at<uint64_t>(base, o[6]);
      p->tmp = base + o_tmp;
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
      uint64_t o64[14], o32[10];
      for (uint64_t& x : o64) x = cv.take<uint64_t>(N + 1);
      for (uint64_t& x : o32) x = cv.take<uint32_t>(N + 1);
      MAGOT_HIP_TRY(hipMalloc(&p->rec_mem, cv.used + 256));
      char* base = static_cast<char*>(p->rec_mem);
      a.name_off = at<uint64_t>(base, o64[0]);
      a.word_off = at<uint64_t>(base, o64[1]);
      a.hash = at<uint64_t>(base, o64[2]);
      a.word_hash = at<uint64_t>(base, o64[3]);
      a.seq_len = at<uint64_t>(base, o64[4]);
      a.ne = at<uint64_t>(base, o64[5]);
      a.ne_pos = at<uint64_t>(base, o64[6]);
      a.skey = at<uint64_t>(base, o64[7]);
      a.skey_sorted = at<uint64_t>(base, o64[8]);
      a.head = at<uint64_t>(base, o64[9]);
      a.head_pos = at<uint64_t>(base, o64[10]);
      a.is_first = at<uint64_t>(base, o64[11]);
      a.kpos = at<uint64_t>(base, o64[12]);
      a.k_hash = at<uint64_t>(base, o64[13]);
      a.hdr_line = at<uint32_t>(base, o32[0]);
      a.name_len = at<uint32_t>(base, o32[1]);
      a.word_len = at<uint32_t>(base, o32[2]);
      a.no_word = at<uint32_t>(base, o32[3]);
      a.sval = at<uint32_t>(base, o32[4]);
      a.sval_sorted = at<uint32_t>(base, o32[5]);
      a.last_of = at<uint32_t>(base, o32[6]);
      a.k_first = at<uint32_t>(base, o32[7]);
      a.k_last = at<uint32_t>(base, o32[8]);
      a.k_no_word = at<uint32_t>(base, o32[9]);
    }
    MAGOT_HIP_TRY(launch_fa_names(a, p->tmp, p->tmp_bytes, s));
    unsigned long long status = 0;
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&a.n_ne, a.ne_pos + N, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (status != ~0ull)
      return fa_decline(reason, line, (uint32_t)(status & 0xff), (status >> 8) + 1);
    if (a.n_ne > N) {
      set_error("magot_fastarec_parse: more records with a sequence than records");
      return MAGOT_ERR_STATE;
    }
    MAGOT_HIP_TRY(launch_fa_sort(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(launch_fa_keys(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&a.n_keys, a.kpos + N, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (status != ~0ull)
      return fa_decline(reason, line, (uint32_t)(status & 0xff), (status >> 8) + 1);
    if (a.n_keys > a.n_ne) {
      set_error("magot_fastarec_parse: more keys than records with a sequence");
      return MAGOT_ERR_STATE;
    }
    MAGOT_HIP_TRY(launch_fa_rows(a, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
  }
  guard.p = nullptr;
  *out = p;
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
  if (int rc = fa_fetch(line, a.hdr_line, n)) return rc;
  if (int rc = fa_fetch(name_off, a.name_off, n)) return rc;
  if (int rc = fa_fetch(name_len, a.name_len, n)) return rc;
  if (int rc = fa_fetch(seq_len, a.seq_len, n)) return rc;
  if (int rc = fa_fetch(hash, a.hash, n)) return rc;
  if (int rc = fa_fetch(word_off, a.word_off, n)) return rc;
  if (int rc = fa_fetch(word_len, a.word_len, n)) return rc;
  if (int rc = fa_fetch(word_hash, a.word_hash, n)) return rc;
  return fa_fetch(no_word, a.no_word, n);
}

int magot_fastarec_keys(magot_ctx* ctx, magot_fastarec* p, uint64_t* hash, uint32_t* first_record,
                        uint32_t* last_record, uint32_t* no_word) {
  if (int rc = handle_of(ctx, p, "magot_fastarec_keys", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const FaArgs& a = p->a;
  const uint64_t n = a.n_keys;
  if (int rc = fa_fetch(hash, a.k_hash, n)) return rc;
  if (int rc = fa_fetch(first_record, a.k_first, n)) return rc;
  if (int rc = fa_fetch(last_record, a.k_last, n)) return rc;
  return fa_fetch(no_word, a.k_no_word, n);
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
  Carve cv;
  const uint64_t o_blob = cv.take<uint8_t>(blob_len + 16), o_off = cv.take<uint64_t>(m + 1);
  const uint64_t o_k = cv.take<uint64_t>(m), o_k2 = cv.take<uint64_t>(m);
  const uint64_t o_i = cv.take<uint32_t>(m), o_i2 = cv.take<uint32_t>(m);
  const uint64_t o_keep = cv.take<uint8_t>(a.n_keys);
  const size_t tmp_bytes = fa_tmp_bytes(m);
  const uint64_t o_tmp = cv.take<uint8_t>(tmp_bytes);
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  char* base = static_cast<char*>(buf.p);
  FaMemberArgs g{};
  g.m = m;
  g.blob = at<const uint8_t>(base, o_blob);
  g.off = at<const uint64_t>(base, o_off);
  g.lkey = at<uint64_t>(base, o_k);
  g.lkey_sorted = at<uint64_t>(base, o_k2);
  g.lidx = at<uint32_t>(base, o_i);
  g.lidx_sorted = at<uint32_t>(base, o_i2);
  g.first_word = first_word ? 1u : 0u;
  g.keep = at<uint8_t>(base, o_keep);
  if (blob_len)
    MAGOT_HIP_TRY(hipMemcpyAsync(base + o_blob, blob, blob_len, hipMemcpyHostToDevice, s));
  if (m)
    MAGOT_HIP_TRY(hipMemcpyAsync(base + o_off, off, (m + 1) * 8, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(launch_fa_member(a, g, base + o_tmp, tmp_bytes, s));
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
  double total[kFaPasses] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < kFaPasses; ++k)
      if (int rc = time_pass(ctx, &total[k],
                             [&]() -> hipError_t { return fa_pass(p, k, ctx->stream); }))
        return rc;
  for (int k = 0; k < kFaPasses; ++k) ms7[k] = total[k] / iters;
  return MAGOT_OK;
}

}  // extern "C"
