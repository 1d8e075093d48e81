// C ABI: write_gff's text from a table of rows (gffwrite.hip; genome.py:228-238,
// 616-645, 733-778): the GFF text made resident with the blob of made-up names
// and the rows, every row sized, the output laid out and rendered.
#include "abi_internal.h"

using namespace magot;

static_assert(sizeof(magot_gffrow) == 64, "a row is 64 bytes");
static_assert(sizeof(GwAux) == 64, "a row's pass-1 record is 64 bytes");

struct magot_gffwrite {
  magot_ctx* ctx = nullptr;
  ResidentText rt;           // the text; the blob, the rows and everything sized by them
  void* out_mem = nullptr;   // the rendered text
  void* copy_mem = nullptr;  // magot_gffwrite_time's copy source and target
  GwArgs a{};
  uint8_t* out = nullptr;
  uint64_t out_bytes = 0;
  bool rendered = false;
  void* tmp = nullptr;  // the scan's scratch
  size_t tmp_bytes = 0;
};

namespace {

constexpr int kGwPasses = 4;

constexpr char kOutside[] =
    "magot_gffwrite_open: input outside the device path; use the object path";

int gw_plan_render(magot_gffwrite* p) {
  p->rendered = false;
  if (p->out_mem || !p->out_bytes) return MAGOT_OK;
  MAGOT_HIP_TRY(hipMalloc(&p->out_mem, p->out_bytes + 256));
  p->out = static_cast<uint8_t*>(p->out_mem);
  return MAGOT_OK;
}

hipError_t gw_scan(const magot_gffwrite* p, hipStream_t s) {
  size_t b = p->tmp_bytes;
  return exclusive_sum(p->tmp, b, p->a.len, p->a.off, p->a.n_rows + 1, s);
}

hipError_t gw_pass(const magot_gffwrite* p, int k, hipStream_t s) {
  switch (k) {
    case 0: return launch_gw_size(p->a, s);
    case 1: return gw_scan(p, s);
    case 2: return launch_gw_render(p->a, p->out, s);
    default:
      return hipMemcpyAsync(p->copy_mem, static_cast<char*>(p->copy_mem) + p->out_bytes + 256,
                            p->out_bytes, hipMemcpyDeviceToDevice, s);
  }
}

// offset + length inside the text and the blob behind it
bool ref_ok(uint64_t off, uint32_t len, uint64_t whole) { return off <= whole && len <= whole - off; }

}  // namespace

extern "C" {

void magot_gffwrite_destroy(magot_gffwrite* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->copy_mem) (void)hipFree(p->copy_mem);
  if (p->out_mem) (void)hipFree(p->out_mem);
  if (p->rt.mem) (void)hipFree(p->rt.mem);
  delete p;
}

void magot_gffwrite_params(uint32_t* rows_per_group, uint32_t* threads, uint32_t* max_head) {
  if (rows_per_group) *rows_per_group = kGwGroup;
  if (threads) *threads = kGwThreads;
  if (max_head) *max_head = kGwMaxHead;
}

int magot_gffwrite_open(magot_ctx* ctx, const char* text, uint64_t len, const uint8_t* blob,
                        uint64_t blob_len, const magot_gffrow* rows, uint64_t n_rows,
                        uint64_t max_bytes, magot_gffwrite** out, uint32_t* reason, uint64_t* row) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text) || (blob_len && !blob) || (n_rows && !rows)) {
    set_error("magot_gffwrite_open: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  if (row) *row = 0;
  if (blob_len > ~0ull - len) {
    set_error("magot_gffwrite_open: text and blob beyond 2^64 bytes");
    return MAGOT_ERR_ARG;
  }
  const uint64_t whole = len + blob_len;
  for (uint64_t r = 0; r < n_rows; ++r) {
    const magot_gffrow& R = rows[r];
    const uint32_t kind = R.kind & 0xffu;
    const bool has_parent = (R.kind & MAGOT_GFFROW_HAS_PARENT) != 0;
    const bool made = kind == MAGOT_GFFROW_MADE_PARENT;
    if (kind > MAGOT_GFFROW_MADE_PARENT || (R.kind & ~(0xffu | MAGOT_GFFROW_HAS_PARENT))) {
      set_error("magot_gffwrite_open: a row of no known kind");
      return MAGOT_ERR_RANGE;
    }
    if (R.line_off > len || !ref_ok(R.id_off, R.id_len, whole) ||
        (has_parent && !ref_ok(R.parent_off, R.parent_len, whole)) ||
        (made && !ref_ok(R.type_off, R.type_len, whole))) {
      set_error("magot_gffwrite_open: a row's line or reference leaves the text and the blob");
      return MAGOT_ERR_RANGE;
    }
    if (R.id_len >= kGwMaxRef || (has_parent && R.parent_len >= kGwMaxRef) ||
        (made && R.type_len >= kGwMaxRef)) {
      set_error("magot_gffwrite_open: a reference of 2^28 bytes or more");
      return MAGOT_ERR_ARG;
    }
  }
  if (int rc = resident_text_budget(&max_bytes)) return rc;
  if (len > max_bytes || blob_len > max_bytes || n_rows > max_bytes / 160)
    return decline(kOutside, reason, row, MAGOT_GFFWRITE_TOO_LARGE, 0);

  Building<magot_gffwrite, magot_gffwrite_destroy> guard{new magot_gffwrite()};
  magot_gffwrite* p = guard.p;
  p->ctx = ctx;
  GwArgs& a = p->a;
  a.n = len;
  a.blob_len = blob_len;
  a.n_rows = n_rows;
  hipStream_t s = ctx->stream;
  p->tmp_bytes = exclusive_sum_bytes<uint64_t>(n_rows + 1);
  Carve cv;
  const uint64_t o_blob = cv.take(&a.blob, blob_len + 1);
  const uint64_t o_rows = cv.take(&a.rows, n_rows + 1);
  cv.take(&a.aux, n_rows + 1);
  cv.take(&a.len, n_rows + 1);
  cv.take(&a.off, n_rows + 1);
  cv.take(&a.status, 1);
  cv.take(&p->tmp, p->tmp_bytes);
  unsigned long long status = 0;
  uint64_t total = 0;
  TextIndexArgs ix{};
  auto passes = [&](char* base) -> int {
    cv.place(base);
    a.text = ix.text;
    if (blob_len)
      MAGOT_HIP_TRY(hipMemcpyAsync(base + o_blob, blob, blob_len, hipMemcpyHostToDevice, s));
    if (n_rows)
      MAGOT_HIP_TRY(hipMemcpyAsync(base + o_rows, rows, n_rows * sizeof(magot_gffrow),
                                   hipMemcpyHostToDevice, s));
    MAGOT_HIP_TRY(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), s));
    MAGOT_HIP_TRY(launch_gw_size(a, s));
    MAGOT_HIP_TRY(gw_scan(p, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&total, a.off + n_rows, 8, hipMemcpyDeviceToHost, s));
    return MAGOT_OK;
  };
  if (int rc = resident_text_open(ctx, text, len, '\n', kTextNoByte, cv.used, passes, &p->rt, &ix))
    return rc;
  if (int rc = decline_if_offended(kOutside, reason, row, status)) return rc;
  p->out_bytes = total;
  *out = guard.release();
  return MAGOT_OK;
}

int magot_gffwrite_sizes(const magot_gffwrite* p, uint64_t* n_rows, uint64_t* out_bytes) {
  if (!p) {
    set_error("magot_gffwrite_sizes: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_rows) *n_rows = p->a.n_rows;
  if (out_bytes) *out_bytes = p->out_bytes;
  return MAGOT_OK;
}

double magot_gffwrite_upload_ms(const magot_gffwrite* p) {
  return p ? (double)p->rt.upload_ms : 0.0;
}

int magot_gffwrite_render(magot_ctx* ctx, magot_gffwrite* p, uint64_t* bytes) {
  if (int rc = handle_of(ctx, p, "magot_gffwrite_render", "handle")) return rc;
  if (!bytes) {
    set_error("magot_gffwrite_render: null argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (int rc = gw_plan_render(p)) return rc;
  MAGOT_HIP_TRY(launch_gw_render(p->a, p->out, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  p->rendered = true;
  *bytes = p->out_bytes;
  return MAGOT_OK;
}

int magot_gffwrite_render_fetch(magot_ctx* ctx, magot_gffwrite* p, uint8_t* out, uint64_t cap) {
  if (int rc = handle_of(ctx, p, "magot_gffwrite_render_fetch", "handle")) return rc;
  if (!p->rendered) {
    set_error("magot_gffwrite_render_fetch: nothing rendered");
    return MAGOT_ERR_STATE;
  }
  const uint64_t need = p->out_bytes;
  if (cap < need || (need && !out)) {
    set_error("magot_gffwrite_render_fetch: buffer too small");
    return MAGOT_ERR_ARG;
  }
  if (need) MAGOT_HIP_TRY(hipMemcpy(out, p->out, need, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_gffwrite_time(magot_ctx* ctx, magot_gffwrite* p, int iters, double* ms4,
                        uint64_t* text_bytes, uint64_t* out_bytes) {
  if (int rc = handle_of(ctx, p, "magot_gffwrite_time", "handle")) return rc;
  if (iters <= 0 || !ms4) {
    set_error("magot_gffwrite_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text_bytes) *text_bytes = p->a.n;
  if (out_bytes) *out_bytes = p->out_bytes;
  for (int k = 0; k < kGwPasses; ++k) ms4[k] = 0;
  if (!p->out_bytes) return MAGOT_OK;  // no row: nothing to time
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!p->copy_mem) {
    MAGOT_HIP_TRY(hipMalloc(&p->copy_mem, 2 * (p->out_bytes + 256)));
    MAGOT_HIP_TRY(hipMemset(p->copy_mem, 0, 2 * (p->out_bytes + 256)));
  }
  if (int rc = gw_plan_render(p)) return rc;
  // every pass writes what it wrote in magot_gffwrite_open: the answers stand
  return time_passes(ctx, iters, kGwPasses, ms4,
                     [&](int k) { return gw_pass(p, k, ctx->stream); });
}

}  // extern "C"
