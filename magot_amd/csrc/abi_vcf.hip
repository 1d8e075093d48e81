// C ABI: heterozygosity_from_vcf's parse, sort and counting on the device
// (vcf.hip; magot_variants.py:16-139).  The text is made resident and its lines
// indexed by resident_text_open and textindex.hip.  The renderer is in
// vcfhost.cpp.
#include "abi_internal.h"

using namespace magot;

struct magot_vcf {
  magot_ctx* ctx = nullptr;
  ResidentText rt;           // the text and its line index; the status words and last_line
  void* mem = nullptr;       // everything sized by the lines
  void* data_mem = nullptr;  // everything sized by the data lines
  void* loci_mem = nullptr;  // the last magot_vcf_count's tables
  void* copy_mem = nullptr;  // magot_vcf_time's copy target
  TextIndexArgs ix{};        // the line index
  VcfArgs a{};
  VcfCountArgs c{};
  void *tmp = nullptr, *ctmp = nullptr;
  size_t tmp_bytes = 0, ctmp_bytes = 0;
  uint32_t* last_line = nullptr;
  uint64_t head_off = 0, head_len = 0;
  bool resolved = false;
};

namespace {

constexpr int kVcfPasses = 8;

constexpr char kOutside[] =
    "magot_vcf_parse: input outside the device path; use the host functions";

// the span of 0-based line k without its LF
int vcf_line_span(const magot_vcf* p, const char* host_text, uint64_t k, uint64_t* off,
                  uint64_t* len) {
  uint64_t se[2] = {0, 0};
  MAGOT_HIP_TRY(hipMemcpy(se, p->a.line_start + k, sizeof se, hipMemcpyDeviceToHost));
  uint8_t last = 0;
  if (host_text) last = (uint8_t)host_text[se[1] - 1];
  else MAGOT_HIP_TRY(hipMemcpy(&last, p->a.text + se[1] - 1, 1, hipMemcpyDeviceToHost));
  *off = se[0];
  *len = se[1] - se[0] - (last == '\n' ? 1 : 0);
  return MAGOT_OK;
}

hipError_t vcf_pass(const magot_vcf* p, int k, hipStream_t s) {
  const VcfArgs& a = p->a;
  switch (k) {
    case 0: return text_index_pass(p->ix, p->rt, kTextFillLines, s);
    case 1:
      if (hipError_t e = launch_vcf_classify(a, p->tmp, p->tmp_bytes, s)) return e;
      return launch_vcf_compact(a, s);
    case 2: return launch_vcf_parse(a, s);
    case 3:
      if (hipError_t e = launch_vcf_runs_scan(a, p->tmp, p->tmp_bytes, s)) return e;
      return launch_vcf_runs(a, s);
    case 4: return p->resolved ? launch_vcf_sort(a, p->tmp, p->tmp_bytes, s) : hipSuccess;
    case 5: return p->resolved ? launch_vcf_flags(a, s) : hipSuccess;
    case 6:
      if (!p->loci_mem) return hipSuccess;
      if (hipError_t e = launch_vcf_ranges(a, p->c, p->ctmp, p->ctmp_bytes, s)) return e;
      return launch_vcf_count(a, p->c, s);
    default: return hipMemcpyAsync(p->copy_mem, a.text, a.n, hipMemcpyDeviceToDevice, s);
  }
}

}  // namespace

extern "C" {

void magot_vcf_destroy(magot_vcf* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  for (void* m : {p->copy_mem, p->loci_mem, p->data_mem, p->mem, p->rt.mem})
    if (m) (void)hipFree(m);
  delete p;
}

void magot_vcf_params(uint32_t* split_rows, uint32_t* max_samples, uint32_t* max_runs,
                      uint64_t* max_counts) {
  if (split_rows) *split_rows = kVcfSplit;
  if (max_samples) *max_samples = kVcfMaxSamples;
  if (max_runs) *max_runs = kVcfMaxRuns;
  if (max_counts) *max_counts = kVcfMaxCounts;
}

int magot_vcf_parse(magot_ctx* ctx, const char* text, uint64_t len, uint64_t max_bytes,
                    uint32_t max_samples, uint32_t max_runs, magot_vcf** out, uint32_t* reason,
                    uint64_t* line) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text)) {
    set_error("magot_vcf_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  if (line) *line = 0;
  if (!max_samples || max_samples > kVcfMaxSamples) max_samples = kVcfMaxSamples;
  if (!max_runs || max_runs > kVcfMaxRuns) max_runs = kVcfMaxRuns;
  if (int rc = resident_text_budget(&max_bytes)) return rc;
  if (len > max_bytes) return decline(kOutside, reason, line, MAGOT_VCF_TOO_LARGE, 0);
  if (!len) return decline(kOutside, reason, line, MAGOT_VCF_NO_HEADER, 0);

  Building<magot_vcf, magot_vcf_destroy> guard{new magot_vcf()};
  magot_vcf* p = guard.p;
  p->ctx = ctx;
  TextIndexArgs& ix = p->ix;
  VcfArgs& a = p->a;
  hipStream_t s = ctx->stream;
  {
    Carve cv;  // the caller's slices: eight status words and last_line
    cv.take(&a.status, 8);
    cv.take(&p->last_line, 1);
    if (int rc = resident_text_open(ctx, text, len, '\n', kTextNoByte, cv.used, &p->rt, &ix))
      return rc;
    cv.place(p->rt.extra);
    a.text = ix.text;
    a.n = len;
    ix.n_lines = p->rt.n_lines;
    if (ix.n_lines > kPslLineMask)
      return decline(kOutside, reason, line, MAGOT_VCF_TOO_MANY_LINES, 0);
  }
  const uint64_t L = a.n_lines = ix.n_lines;  // at least 1
  a.final_lf = text[len - 1] == '\n' ? 1 : 0;
  {
    p->tmp_bytes = vcf_tmp_bytes(L);
    Carve cv;
    cv.take(&ix.pos, L + 1);
    cv.take(&a.kind, L + 1);
    cv.take(&a.kpos, L + 1);
    cv.take(&p->tmp, p->tmp_bytes);
    MAGOT_HIP_TRY(hipMalloc(&p->mem, cv.used + 256));
    cv.place(p->mem);
    a.line_start = ix.pos;
  }
  MAGOT_HIP_TRY(launch_text_fill(ix, kTextFillLines, s));
  MAGOT_HIP_TRY(launch_vcf_classify(a, p->tmp, p->tmp_bytes, s));
  unsigned long long st[5] = {0, 0, 0, 0, 0};
  uint64_t totals = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&totals, a.kpos + L, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  a.n_data = totals & 0xffffffffull;
  a.n_hdr = totals >> 32;
  if (st[4]) return decline(kOutside, reason, line, MAGOT_VCF_CARRIAGE_RETURN, 0);
  if (st[1] == 0) return decline(kOutside, reason, line, MAGOT_VCF_NO_HEADER, 0);
  if (st[1] > 1) return decline(kOutside, reason, line, MAGOT_VCF_MANY_HEADERS, 0);
  if (!a.n_data) return decline(kOutside, reason, line, MAGOT_VCF_NO_DATA, 0);
  if (st[3] < st[2])
    return decline(kOutside, reason, line, MAGOT_VCF_HEADER_AFTER_DATA, st[3] + 1);
  // S from the '#' line: the fields of the text behind '#', less nine
  if (int rc = vcf_line_span(p, text, st[2], &p->head_off, &p->head_len)) return rc;
  uint64_t fields = 1;
  for (uint64_t i = 1; i < p->head_len; ++i) fields += text[p->head_off + i] == '\t';
  if (fields < 10) return decline(kOutside, reason, line, MAGOT_VCF_NO_SAMPLES, st[2] + 1);
  if (fields - 9 > max_samples)
    return decline(kOutside, reason, line, MAGOT_VCF_TOO_MANY_SAMPLES, st[2] + 1);
  a.n_samples = (uint32_t)(fields - 9);
  a.words = (a.n_samples + 31) / 32;
  {
    const uint64_t D = a.n_data;
    Carve cv;
    cv.take(&a.data_line, D);
    cv.take(&a.hdr_off, a.n_hdr + 1);
    cv.take(&a.hdr_len, a.n_hdr + 1);
    cv.take(&a.pos, D);
    cv.take(&a.hash, D);
    cv.take(&a.chrom_len, D);
    cv.take(&a.head, D + 1);
    cv.take(&a.run, D + 1);
    cv.take(&a.bits, D * a.words);
    cv.take(&a.run_off, max_runs);
    cv.take(&a.run_len, max_runs);
    cv.take(&a.contig_of_run, max_runs);
    cv.take(&a.key, D);
    cv.take(&a.key_sorted, D);
    cv.take(&a.val, D);
    cv.take(&a.val_sorted, D);
    cv.take(&a.kept_sorted, D);
    cv.take(&a.kept, D);
    cv.take(&a.first, D);
    MAGOT_HIP_TRY(hipMalloc(&p->data_mem, cv.used + 256));
    cv.place(p->data_mem);
    MAGOT_HIP_TRY(hipMemsetAsync(a.kept, 0, D, s));
    MAGOT_HIP_TRY(hipMemsetAsync(a.first, 0, D, s));
  }
  MAGOT_HIP_TRY(launch_vcf_compact(a, s));
  MAGOT_HIP_TRY(launch_vcf_parse(a, s));
  MAGOT_HIP_TRY(launch_vcf_runs_scan(a, p->tmp, p->tmp_bytes, s));
  uint32_t n_runs = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(st, a.status, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&n_runs, a.run + a.n_data, 4, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (int rc = decline_if_offended(kOutside, reason, line, st[0])) return rc;
  if (n_runs > max_runs) return decline(kOutside, reason, line, MAGOT_VCF_TOO_MANY_RUNS, 0);
  a.n_runs = n_runs;  // the run tables hold max_runs
  MAGOT_HIP_TRY(launch_vcf_runs(a, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  *out = guard.release();
  return MAGOT_OK;
}

int magot_vcf_sizes(const magot_vcf* p, uint64_t* n_lines, uint64_t* n_data, uint64_t* n_hdr,
                    uint32_t* n_samples, uint32_t* words, uint64_t* n_runs, uint64_t* head_off,
                    uint64_t* head_len) {
  if (!p) {
    set_error("magot_vcf_sizes: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_lines) *n_lines = p->a.n_lines;
  if (n_data) *n_data = p->a.n_data;
  if (n_hdr) *n_hdr = p->a.n_hdr;
  if (n_samples) *n_samples = p->a.n_samples;
  if (words) *words = p->a.words;
  if (n_runs) *n_runs = p->a.n_runs;
  if (head_off) *head_off = p->head_off;
  if (head_len) *head_len = p->head_len;
  return MAGOT_OK;
}

double magot_vcf_upload_ms(const magot_vcf* p) { return p ? (double)p->rt.upload_ms : 0.0; }

int magot_vcf_header_lines(magot_ctx* ctx, magot_vcf* p, uint64_t* off, uint64_t* len) {
  if (int rc = handle_of(ctx, p, "magot_vcf_header_lines", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (int rc = fetch_rows(off, p->a.hdr_off, p->a.n_hdr)) return rc;
  return fetch_rows(len, p->a.hdr_len, p->a.n_hdr);
}

int magot_vcf_runs(magot_ctx* ctx, magot_vcf* p, uint64_t* off, uint64_t* len) {
  if (int rc = handle_of(ctx, p, "magot_vcf_runs", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (int rc = fetch_rows(off, p->a.run_off, p->a.n_runs)) return rc;
  return fetch_rows(len, p->a.run_len, p->a.n_runs);
}

int magot_vcf_resolve(magot_ctx* ctx, magot_vcf* p, const uint32_t* contig, uint64_t n_runs) {
  if (int rc = handle_of(ctx, p, "magot_vcf_resolve", "handle")) return rc;
  VcfArgs& a = p->a;
  if (!contig || n_runs != a.n_runs) {
    set_error("magot_vcf_resolve: one contig per run");
    return MAGOT_ERR_ARG;
  }
  uint32_t top = 0;
  for (uint64_t r = 0; r < n_runs; ++r) top = std::max(top, contig[r]);
  a.key_bits = 32;
  while (a.key_bits < 64 && (top >> (a.key_bits - 32))) ++a.key_bits;
  hipStream_t s = ctx->stream;
  MAGOT_HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(a.contig_of_run), contig,
                               n_runs * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));  // the caller's array is read
  p->resolved = true;
  MAGOT_HIP_TRY(launch_vcf_sort(a, p->tmp, p->tmp_bytes, s));
  MAGOT_HIP_TRY(launch_vcf_flags(a, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  return MAGOT_OK;
}

int magot_vcf_tables(magot_ctx* ctx, magot_vcf* p, uint32_t* line, int32_t* pos, uint64_t* hash,
                     uint8_t* kept, uint8_t* first, uint32_t* bits) {
  if (int rc = handle_of(ctx, p, "magot_vcf_tables", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const VcfArgs& a = p->a;
  const uint64_t n = a.n_data;
  if (int rc = fetch_rows(line, a.data_line, n)) return rc;
  if (int rc = fetch_rows(pos, a.pos, n)) return rc;
  if (int rc = fetch_rows(hash, a.hash, n)) return rc;
  if (int rc = fetch_rows(kept, a.kept, n)) return rc;
  if (int rc = fetch_rows(first, a.first, n)) return rc;
  return fetch_rows(bits, a.bits, n * a.words);
}

int magot_vcf_last_of(magot_ctx* ctx, magot_vcf* p, uint64_t d, uint64_t* line, uint64_t* off,
                      uint64_t* len) {
  if (int rc = handle_of(ctx, p, "magot_vcf_last_of", "handle")) return rc;
  if (!p->resolved || d >= p->a.n_data || !line || !off || !len) {
    set_error("magot_vcf_last_of: before magot_vcf_resolve, no such data line, or null argument");
    return p->resolved ? MAGOT_ERR_ARG : MAGOT_ERR_STATE;
  }
  hipStream_t s = ctx->stream;
  MAGOT_HIP_TRY(launch_vcf_last_of(p->a, d, p->last_line, s));
  uint32_t ln = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(&ln, p->last_line, 4, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  *line = ln;
  return vcf_line_span(p, nullptr, ln, off, len);
}

int magot_vcf_count(magot_ctx* ctx, magot_vcf* p, const uint32_t* contig, const uint32_t* lo,
                    const uint32_t* hi, uint64_t n_loci, const uint32_t* allowed, uint32_t* counts,
                    uint32_t* foreign, uint32_t* reason) {
  if (int rc = handle_of(ctx, p, "magot_vcf_count", "handle")) return rc;
  if (reason) *reason = 0;
  if (!p->resolved) {
    set_error("magot_vcf_count: before magot_vcf_resolve");
    return MAGOT_ERR_STATE;
  }
  const VcfArgs& a = p->a;
  if (n_loci > kVcfMaxCounts || n_loci * a.n_samples > kVcfMaxCounts) {  // before any table is read
    if (reason) *reason = MAGOT_VCF_TOO_MANY_COUNTS;
    set_error("magot_vcf_count: more counters than the device path takes");
    return MAGOT_ERR_UNSUPPORTED;
  }
  if (!allowed || !foreign || (n_loci && (!contig || !lo || !hi || !counts))) {
    set_error("magot_vcf_count: null argument");
    return MAGOT_ERR_ARG;
  }
  *foreign = 0;
  if (!n_loci) return MAGOT_OK;
  if (p->loci_mem) {
    MAGOT_HIP_TRY(hipFree(p->loci_mem));
    p->loci_mem = nullptr;
  }
  VcfCountArgs& c = p->c;
  c = VcfCountArgs{};
  c.n_loci = n_loci;
  p->ctmp_bytes = vcf_count_tmp_bytes(n_loci);
  Carve cv;
  uint32_t *d_c, *d_lo, *d_hi, *d_al;  // uploaded into; the kernels read them as const
  cv.take(&d_c, n_loci);
  cv.take(&d_lo, n_loci);
  cv.take(&d_hi, n_loci);
  cv.take(&c.rng_b, n_loci);
  cv.take(&c.rng_e, n_loci);
  cv.take(&c.pieces, n_loci + 1);
  cv.take(&c.piece_off, n_loci + 1);
  cv.take(&d_al, a.words);
  cv.take(&c.foreign, 1);
  cv.take(&c.counts, n_loci * a.n_samples);
  cv.take(&p->ctmp, p->ctmp_bytes);
  MAGOT_HIP_TRY(hipMalloc(&p->loci_mem, cv.used + 256));
  cv.place(p->loci_mem);
  c.contig = d_c;
  c.lo = d_lo;
  c.hi = d_hi;
  c.allowed = d_al;
  hipStream_t s = ctx->stream;
  MAGOT_HIP_TRY(hipMemcpyAsync(d_c, contig, n_loci * 4, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(d_lo, lo, n_loci * 4, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(d_hi, hi, n_loci * 4, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(d_al, allowed, a.words * 4, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(launch_vcf_ranges(a, c, p->ctmp, p->ctmp_bytes, s));
  uint64_t n_pieces = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(&n_pieces, c.piece_off + n_loci, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (n_pieces > 0x7fffffffull) {
    set_error("magot_vcf_count: more pieces than one launch holds");
    return MAGOT_ERR_RANGE;
  }
  c.n_pieces = n_pieces;
  MAGOT_HIP_TRY(launch_vcf_count(a, c, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(counts, c.counts, n_loci * a.n_samples * 4, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(foreign, c.foreign, 4, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  return MAGOT_OK;
}

int magot_vcf_time(magot_ctx* ctx, magot_vcf* p, int iters, double* ms8, uint64_t* text_bytes) {
  if (int rc = handle_of(ctx, p, "magot_vcf_time", "handle")) return rc;
  if (iters <= 0 || !ms8) {
    set_error("magot_vcf_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text_bytes) *text_bytes = p->a.n;
  if (!p->copy_mem) MAGOT_HIP_TRY(hipMalloc(&p->copy_mem, p->a.n + 256));
  // every pass writes what it wrote before: the answers stand
  return time_passes(ctx, iters, kVcfPasses, ms8,
                     [&](int k) { return vcf_pass(p, k, ctx->stream); });
}

}  // extern "C"
