// C ABI: the longest ORF of every record of an executed extraction plan's
// nucleotide output (longorf.hip; get_CDS_peptides, genome_tools.py:283-321).
#include "abi_internal.h"

using namespace magot;

struct magot_longorf {
  magot_ctx* ctx = nullptr;
  magot_plan* plan = nullptr;
  void* arena = nullptr;    // the tables: one row per record
  void* payload = nullptr;  // the winners, concatenated
  uint64_t payload_cap = 0, payload_bytes = 0;
  void* tmem = nullptr;     // the tables of the last magot_longorf_text
  void* tout = nullptr;     // its text
  LongOrfArgs a{};
  LongOrfTextArgs t{};
  uint64_t text_bytes = 0;
  bool executed = false, has_text = false;
};

namespace {

// waves that keep every CU full (8 per SIMD), as whole workgroups of 4
uint32_t longorf_max_waves(const magot_ctx* ctx) {
  return 32u * (uint32_t)std::max(ctx->n_cu, 1);
}

void free_text(magot_longorf* h) {
  if (h->tmem) (void)hipFree(h->tmem);
  if (h->tout) (void)hipFree(h->tout);
  h->tmem = h->tout = nullptr;
  h->has_text = false;
}

hipError_t read_u64(const uint64_t* dev, uint64_t* host, hipStream_t s) {
  if (hipError_t e = hipMemcpyAsync(host, dev, 8, hipMemcpyDeviceToHost, s)) return e;
  return hipStreamSynchronize(s);
}

}  // namespace

extern "C" {

void magot_longorf_destroy(magot_longorf* h) {
  if (!h) return;
  if (h->ctx) (void)hipSetDevice(h->ctx->device);
  free_text(h);
  if (h->payload) (void)hipFree(h->payload);
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

int magot_longorf_create(magot_ctx* ctx, magot_plan* p, const uint8_t* lut64, magot_longorf** out) {
  if (int rc = bind(ctx)) return rc;
  if (!p || !out || p->ctx != ctx) {
    set_error("magot_longorf_create: null argument, or a plan of another context");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (!(p->args.outputs & MAGOT_OUT_NUC)) {
    set_error("magot_longorf_create: the plan has no nucleotide output (MAGOT_OUT_NUC)");
    return MAGOT_ERR_ARG;
  }
  if (!p->executed) {
    set_error("magot_longorf_create: execute the extraction plan first");
    return MAGOT_ERR_STATE;
  }
  const uint64_t n = p->n_tx;
  for (uint64_t r = 0; r < n; ++r)
    if (p->nuc_off[r + 1] - p->nuc_off[r] >= (1ull << 32)) {
      set_error("magot_longorf_create: a record of 2^32 bases or more");
      return MAGOT_ERR_RANGE;
    }
  Building<magot_longorf, magot_longorf_destroy> guard{new magot_longorf()};
  magot_longorf* h = guard.p;
  h->ctx = ctx;
  h->plan = p;
  LongOrfArgs& a = h->a;
  a.n = n;
  a.nuc = p->args.nuc;
  const uint64_t blocks = std::min<uint64_t>((n + 3) / 4, longorf_max_waves(ctx) / 4);
  a.waves = (uint32_t)(4 * std::max<uint64_t>(blocks, 1));
  a.scan_bytes = longorf_scan_bytes(n + 1);
  Carve cv;  // the uploads go to the arena + offset: the kernel's fields are const
  const uint64_t o_start = cv.take(&a.start, n + 1);
  const uint64_t o_noff = cv.take(&a.noff, n + 1);
  const uint64_t o_lut = cv.take(&a.lut, 64);
  cv.take(&a.j, n + 1);
  cv.take(&a.k, n + 1);
  cv.take(&a.ku, n + 1);
  cv.take(&a.len, n + 1);
  cv.take(&a.flags, n + 1);
  cv.take(&a.poff, n + 1);
  cv.take(&a.scan_tmp, a.scan_bytes);
  MAGOT_HIP_TRY(hipMalloc(&h->arena, cv.used));
  cv.place(h->arena);
  char* const base = static_cast<char*>(h->arena);
  uint8_t lut[64];
  if (lut64) std::memcpy(lut, lut64, 64);
  else standard_lut(lut);
  const std::vector<uint64_t>& lay = p->genome_order ? p->lay_nuc : p->nuc_off;
  if (n) MAGOT_HIP_TRY(hipMemcpy(base + o_start, lay.data(), n * 8, hipMemcpyHostToDevice));
  MAGOT_HIP_TRY(hipMemcpy(base + o_noff, p->nuc_off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
  MAGOT_HIP_TRY(hipMemcpy(base + o_lut, lut, 64, hipMemcpyHostToDevice));
  *out = guard.release();
  return MAGOT_OK;
}

int magot_longorf_execute(magot_ctx* ctx, magot_longorf* h, uint64_t* payload_bytes) {
  if (int rc = handle_of(ctx, h, "magot_longorf_execute", "handle")) return rc;
  hipStream_t s = ctx->stream;
  h->executed = false;
  MAGOT_HIP_TRY(launch_longorf_call(h->a, s));
  MAGOT_HIP_TRY(read_u64(h->a.poff + h->a.n, &h->payload_bytes, s));
  if (h->payload_bytes > h->payload_cap || !h->payload) {
    if (h->payload) MAGOT_HIP_TRY(hipFree(h->payload));
    h->payload = nullptr;
    MAGOT_HIP_TRY(hipMalloc(&h->payload, h->payload_bytes + 64));
    h->payload_cap = h->payload_bytes;
    h->a.payload = static_cast<uint8_t*>(h->payload);
  }
  MAGOT_HIP_TRY(launch_longorf_write(h->a, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  h->executed = true;
  if (payload_bytes) *payload_bytes = h->payload_bytes;
  return MAGOT_OK;
}

int magot_longorf_fetch(magot_ctx* ctx, magot_longorf* h, uint8_t* stream, uint32_t* start,
                        uint32_t* length, uint64_t* payload_off, uint8_t* payload,
                        uint8_t* record_flags) {
  if (int rc = handle_of(ctx, h, "magot_longorf_fetch", "handle")) return rc;
  if (!h->executed) {
    set_error("magot_longorf_fetch: call magot_longorf_execute first");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const LongOrfArgs& a = h->a;
  if (int rc = fetch_rows(stream, a.j, a.n)) return rc;
  if (int rc = fetch_rows(start, a.k, a.n)) return rc;
  if (int rc = fetch_rows(length, a.len, a.n)) return rc;
  if (int rc = fetch_rows(payload_off, a.poff, a.n)) return rc;
  if (int rc = fetch_rows(payload, a.payload, h->payload_bytes)) return rc;
  return fetch_rows(record_flags, a.flags, a.n);
}

int magot_longorf_text(magot_ctx* ctx, magot_longorf* h, const uint64_t* name_off,
                       const uint8_t* names, uint64_t n_print, uint64_t* out_len) {
  if (int rc = handle_of(ctx, h, "magot_longorf_text", "handle")) return rc;
  if (!name_off || !out_len || n_print > h->a.n) {
    set_error("magot_longorf_text: null argument, or more entries than records");
    return MAGOT_ERR_ARG;
  }
  if (!h->executed) {
    set_error("magot_longorf_text: call magot_longorf_execute first");
    return MAGOT_ERR_STATE;
  }
  for (uint64_t r = 0; r < n_print; ++r)
    if (name_off[r + 1] < name_off[r] || (name_off[r + 1] > name_off[r] && !names) ||
        name_off[r + 1] - name_off[r] >= (1ull << 31)) {
      set_error("magot_longorf_text: bad name table");
      return MAGOT_ERR_ARG;
    }
  free_text(h);
  struct Undo {  // a call that fails half way leaves no text and none of its tables
    magot_longorf* h;
    ~Undo() {
      if (h) free_text(h);
    }
  } undo{h};
  hipStream_t s = ctx->stream;
  LongOrfTextArgs& t = h->t;
  t = LongOrfTextArgs{};
  t.n_print = n_print;
  const uint64_t name_bytes = name_off[n_print] - name_off[0];
  t.scan_bytes = longorf_scan_bytes(n_print + 1);
  Carve cv;
  const uint64_t o_noff = cv.take(&t.name_off, n_print + 1);
  const uint64_t o_names = cv.take(&t.names, name_bytes + 1);
  cv.take(&t.tlen, n_print + 1);
  cv.take(&t.tstart, n_print + 1);
  cv.take(&t.scan_tmp, t.scan_bytes);
  MAGOT_HIP_TRY(hipMalloc(&h->tmem, cv.used));
  cv.place(h->tmem);
  char* const base = static_cast<char*>(h->tmem);
  // the blob from its first used byte: the offsets are uploaded relative to it
  std::vector<uint64_t> rel(n_print + 1);
  for (uint64_t r = 0; r <= n_print; ++r) rel[r] = name_off[r] - name_off[0];
  MAGOT_HIP_TRY(hipMemcpy(base + o_noff, rel.data(), (n_print + 1) * 8, hipMemcpyHostToDevice));
  if (name_bytes)
    MAGOT_HIP_TRY(hipMemcpy(base + o_names, names + name_off[0], name_bytes, hipMemcpyHostToDevice));
  MAGOT_HIP_TRY(launch_longorf_text_sizes(h->a, t, s));
  MAGOT_HIP_TRY(read_u64(t.tstart + n_print, &h->text_bytes, s));
  MAGOT_HIP_TRY(hipMalloc(&h->tout, h->text_bytes + 64));
  t.out = static_cast<uint8_t*>(h->tout);
  MAGOT_HIP_TRY(launch_longorf_text_write(h->a, t, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  undo.h = nullptr;
  h->has_text = true;
  *out_len = h->text_bytes;
  return MAGOT_OK;
}

int magot_longorf_text_fetch(magot_ctx* ctx, magot_longorf* h, uint8_t* out, uint64_t cap) {
  if (int rc = handle_of(ctx, h, "magot_longorf_text_fetch", "handle")) return rc;
  if (!h->has_text) {
    set_error("magot_longorf_text_fetch: call magot_longorf_text first");
    return MAGOT_ERR_STATE;
  }
  if (cap < h->text_bytes || (h->text_bytes && !out)) {
    set_error("magot_longorf_text_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return fetch_rows(out, h->t.out, h->text_bytes);
}

int magot_longorf_time(magot_ctx* ctx, magot_longorf* h, int text, int iters, double* avg_ms) {
  if (int rc = handle_of(ctx, h, "magot_longorf_time", "handle")) return rc;
  if (!avg_ms || iters <= 0) {
    set_error("magot_longorf_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (!h->executed || (text && !h->has_text)) {
    set_error(text ? "magot_longorf_time: call magot_longorf_text first"
                   : "magot_longorf_time: call magot_longorf_execute first");
    return MAGOT_ERR_STATE;
  }
  // the same input gives the same sizes: the buffers at hand fit
  return time_passes(ctx, iters, 1, avg_ms, [&](int) {
    if (!text) {
      if (hipError_t e = launch_longorf_call(h->a, ctx->stream)) return e;
      return launch_longorf_write(h->a, ctx->stream);
    }
    if (hipError_t e = launch_longorf_text_sizes(h->a, h->t, ctx->stream)) return e;
    return launch_longorf_text_write(h->a, h->t, ctx->stream);
  });
}

int magot_longorf_params(magot_ctx* ctx, const magot_longorf* h, uint32_t* step, uint64_t* waves) {
  if (int rc = bind(ctx)) return rc;
  if (h && h->ctx != ctx) {
    set_error("magot_longorf_params: a handle of another context");
    return MAGOT_ERR_ARG;
  }
  if (step) *step = kLongOrfStep;
  if (waves) *waves = h ? h->a.waves : longorf_max_waves(ctx);
  return MAGOT_OK;
}

}  // extern "C"
