// C ABI: besthits_from_psl's keyed reduction on the device (psl.hip;
// genome_tools.py:572-592).  The host-only entry points (the dict order, the
// line renderer) are in pslhost.cpp.
#include "abi_internal.h"

using namespace magot;

struct magot_psl {
  magot_ctx* ctx = nullptr;
  ResidentText rt;           // the text and its line index; the status words
  void* mem = nullptr;       // everything sized by the lines
  void* copy_mem = nullptr;  // magot_psl_time's copy target
  PslArgs a{};
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

namespace {

constexpr int kPslPasses = 8;

// pass k of magot_psl_time on the handle's own buffers
hipError_t psl_pass(const magot_psl* p, int k, hipStream_t s) {
  const PslArgs& a = p->a;
  switch (k) {
    case 0: return text_index_pass(a.ix, p->rt, kTextFillLines, s);
    case 1: return launch_psl_parse(a, s);
    case 2:
      if (hipError_t e = launch_psl_compact(a, p->tmp, p->tmp_bytes, s)) return e;
      return launch_psl_scatter(a, s);
    case 3: return launch_psl_sort(a, p->tmp, p->tmp_bytes, s);
    case 4: return launch_psl_verify(a, s);
    case 5: return launch_psl_reduce(a, p->tmp, p->tmp_bytes, s);
    case 6: return launch_psl_order(a, p->tmp, p->tmp_bytes, s);
    default:
      if (!a.ix.n) return hipSuccess;
      return hipMemcpyAsync(p->copy_mem, a.ix.text, a.ix.n, hipMemcpyDeviceToDevice, s);
  }
}

constexpr char kOutside[] = "magot_psl_parse: input outside the device path; use the line loop";

}  // namespace

extern "C" {

void magot_psl_destroy(magot_psl* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->copy_mem) (void)hipFree(p->copy_mem);
  if (p->mem) (void)hipFree(p->mem);
  if (p->rt.mem) (void)hipFree(p->rt.mem);
  delete p;
}

int magot_psl_parse(magot_ctx* ctx, const char* text, uint64_t len, uint32_t hash_bits,
                    uint64_t max_bytes, magot_psl** out, uint32_t* reason, uint64_t* line) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text)) {
    set_error("magot_psl_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  if (line) *line = 0;
  if (hash_bits < 1 || hash_bits > 64) {
    set_error("magot_psl_parse: hash_bits outside 1..64");
    return MAGOT_ERR_ARG;
  }
  if (int rc = resident_text_budget(&max_bytes)) return rc;
  if (len > max_bytes) return decline(kOutside, reason, line, MAGOT_PSL_TOO_LARGE, 0);

  Building<magot_psl, magot_psl_destroy> guard{new magot_psl()};
  magot_psl* p = guard.p;
  p->ctx = ctx;
  PslArgs& a = p->a;
  a.hash_bits = hash_bits;
  hipStream_t s = ctx->stream;
  if (len) {
    Carve cv;  // the caller's slice: the status word, then the count of keys
    cv.take(&a.status, 2);
    if (int rc = resident_text_open(ctx, text, len, '\n', kTextNoByte, cv.used, &p->rt, &a.ix))
      return rc;
    cv.place(p->rt.extra);
    a.n_uniq = a.status + 1;
    MAGOT_HIP_TRY(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), s));
    a.ix.n_lines = p->rt.n_lines;
    if (a.ix.n_lines > kPslLineMask)
      return decline(kOutside, reason, line, MAGOT_PSL_TOO_MANY_LINES, 0);
  }
  if (a.ix.n_lines) {
    const uint64_t L = a.ix.n_lines;
    p->tmp_bytes = psl_tmp_bytes(L);
    Carve cv;
    cv.take(&a.ix.pos, L + 1);
    cv.take(&a.hash, L);
    cv.take(&a.key_off, L);
    cv.take(&a.key_len, L);
    cv.take(&a.rank, L);
    cv.take(&a.kind, L + 1);
    cv.take(&a.dpos, L + 1);
    cv.take(&a.skey, L);
    cv.take(&a.sval, L);
    cv.take(&a.skey_sorted, L);
    cv.take(&a.sval_sorted, L);
    cv.take(&a.pass_off, L);
    cv.take(&a.pass_len, L);
    cv.take(&a.uniq, L);
    cv.take(&a.agg, L);
    cv.take(&a.seg_first, 4 * L);  // and seg_id and their sorted copies
    cv.take(&a.g_hash, 4 * L);     // and g_off, g_len, g_score
    cv.take(&a.g_first, 2 * L);    // and g_best
    cv.take(&p->tmp, p->tmp_bytes);
    MAGOT_HIP_TRY(hipMalloc(&p->mem, cv.used + 256));
    cv.place(p->mem);
    a.seg_id = a.seg_first + L;
    a.seg_first_sorted = a.seg_first + 2 * L;
    a.seg_id_sorted = a.seg_first + 3 * L;
    a.g_off = a.g_hash + L;
    a.g_len = a.g_hash + 2 * L;
    a.g_score = reinterpret_cast<int64_t*>(a.g_hash + 3 * L);
    a.g_best = a.g_first + L;

    MAGOT_HIP_TRY(launch_text_fill(a.ix, kTextFillLines, s));
    MAGOT_HIP_TRY(launch_psl_parse(a, s));
    MAGOT_HIP_TRY(launch_psl_compact(a, p->tmp, p->tmp_bytes, s));
    unsigned long long status = 0;
    uint32_t n_data = 0;
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&n_data, a.dpos + L, 4, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (int rc = decline_if_offended(kOutside, reason, line, status)) return rc;
    a.n_data = n_data;
    MAGOT_HIP_TRY(launch_psl_scatter(a, s));
    MAGOT_HIP_TRY(launch_psl_sort(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(launch_psl_verify(a, s));
    MAGOT_HIP_TRY(launch_psl_reduce(a, p->tmp, p->tmp_bytes, s));
    unsigned long long n_uniq = 0;
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&n_uniq, a.n_uniq, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (int rc = decline_if_offended(kOutside, reason, line, status)) return rc;
    if (n_uniq > a.n_data) {
      set_error("magot_psl_parse: more keys than data lines");
      return MAGOT_ERR_STATE;
    }
    a.n_groups = n_uniq;
    MAGOT_HIP_TRY(launch_psl_order(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
  }
  *out = guard.release();
  return MAGOT_OK;
}

int magot_psl_sizes(const magot_psl* p, uint64_t* n_lines, uint64_t* n_pass, uint64_t* n_data,
                    uint64_t* n_groups) {
  if (!p) {
    set_error("magot_psl_sizes: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_lines) *n_lines = p->a.ix.n_lines;
  if (n_pass) *n_pass = p->a.ix.n_lines - p->a.n_data;
  if (n_data) *n_data = p->a.n_data;
  if (n_groups) *n_groups = p->a.n_groups;
  return MAGOT_OK;
}

double magot_psl_upload_ms(const magot_psl* p) { return p ? (double)p->rt.upload_ms : 0.0; }

int magot_psl_pass_lines(magot_ctx* ctx, magot_psl* p, uint64_t* off, uint64_t* len) {
  if (int rc = handle_of(ctx, p, "magot_psl_pass_lines", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t n = p->a.ix.n_lines - p->a.n_data;
  if (int rc = fetch_rows(off, p->a.pass_off, n)) return rc;
  return fetch_rows(len, p->a.pass_len, n);
}

int magot_psl_groups(magot_ctx* ctx, magot_psl* p, uint64_t* hash, uint32_t* first_line,
                     uint32_t* best_line, int64_t* score, uint64_t* off, uint64_t* len) {
  if (int rc = handle_of(ctx, p, "magot_psl_groups", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const PslArgs& a = p->a;
  const uint64_t n = a.n_groups;
  if (int rc = fetch_rows(hash, a.g_hash, n)) return rc;
  if (int rc = fetch_rows(first_line, a.g_first, n)) return rc;
  if (int rc = fetch_rows(best_line, a.g_best, n)) return rc;
  if (int rc = fetch_rows(score, a.g_score, n)) return rc;
  if (int rc = fetch_rows(off, a.g_off, n)) return rc;
  return fetch_rows(len, a.g_len, n);
}

int magot_psl_time(magot_ctx* ctx, magot_psl* p, int iters, double* ms8, uint64_t* text_bytes) {
  if (int rc = handle_of(ctx, p, "magot_psl_time", "handle")) return rc;
  if (iters <= 0 || !ms8) {
    set_error("magot_psl_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text_bytes) *text_bytes = p->a.ix.n;
  for (int k = 0; k < kPslPasses; ++k) ms8[k] = 0;
  if (!p->a.ix.n_lines) return MAGOT_OK;  // an empty text: nothing was launched
  if (!p->copy_mem) MAGOT_HIP_TRY(hipMalloc(&p->copy_mem, p->a.ix.n + 256));
  // every pass writes what it wrote in magot_psl_parse: the answers stand
  return time_passes(ctx, iters, kPslPasses, ms8,
                     [&](int k) { return psl_pass(p, k, ctx->stream); });
}

}  // extern "C"
