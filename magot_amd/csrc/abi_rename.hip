// C ABI: replace_names over a resident text (rename.hip; genome_tools.py:431-446):
// the text and the table made resident, the table's lookup structure, the field
// ends and their matches, the layout and the renamed text.
#include "abi_internal.h"

using namespace magot;

struct magot_rename {
  magot_ctx* ctx = nullptr;
  ResidentText rt;            // the text and the index of its ds; the values, the table, the status
  void* field_mem = nullptr;  // everything sized by the fields
  void* hit_mem = nullptr;    // everything sized by the hits
  void* out_mem = nullptr;    // the rendered text and its pieces
  void* copy_mem = nullptr;   // magot_rename_time's copy target
  RnArgs a{};
  RnRenderArgs r{};
  bool rendered = false;
  void* tmp = nullptr;   // the field and hit scans' scratch
  size_t tmp_bytes = 0;
};

namespace {

constexpr int kRnPasses = 6;

constexpr char kOutside[] =
    "magot_rename_parse: input outside the device path; use the host loop";

// The buffers of a render: the output and one row per piece.  Replaces the
// handle's last ones.
int rn_plan_render(magot_rename* p) {
  if (p->out_mem) MAGOT_HIP_TRY(hipFree(p->out_mem));
  p->out_mem = nullptr;
  p->rendered = false;
  RnRenderArgs& r = p->r;
  if (!r.n_pieces) return MAGOT_OK;
  Carve co;
  co.take(&r.out, r.out_bytes + 16);
  co.take(&r.p_src, r.n_pieces);
  co.take(&r.p_dst, r.n_pieces);
  co.take(&r.p_len, r.n_pieces);
  MAGOT_HIP_TRY(hipMalloc(&p->out_mem, co.used + 256));
  co.place(p->out_mem);
  return MAGOT_OK;
}

// pass k of magot_rename_time on the handle's own buffers
hipError_t rn_pass(const magot_rename* p, int k, hipStream_t s) {
  const RnArgs& a = p->a;
  switch (k) {
    case 0: return launch_rn_table(a, s);
    case 1: return text_index_pass(a.ix, p->rt, kTextFillPlain, s);
    case 2: return launch_rn_match(a, p->tmp, p->tmp_bytes, s);
    case 3: return launch_rn_layout(a, p->tmp, p->tmp_bytes, s);
    case 4: return launch_rn_render(a, p->r, s);
    default: return hipMemcpyAsync(p->copy_mem, a.ix.text, a.ix.n, hipMemcpyDeviceToDevice, s);
  }
}

}  // namespace

extern "C" {

void magot_rename_destroy(magot_rename* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->copy_mem) (void)hipFree(p->copy_mem);
  if (p->out_mem) (void)hipFree(p->out_mem);
  if (p->hit_mem) (void)hipFree(p->hit_mem);
  if (p->field_mem) (void)hipFree(p->field_mem);
  if (p->rt.mem) (void)hipFree(p->rt.mem);
  delete p;
}

void magot_rename_params(uint32_t* max_name, uint32_t* text_block, uint32_t* piece) {
  if (max_name) *max_name = kRnMaxName;
  if (text_block) *text_block = kTextBlock;
  if (piece) *piece = kRnPiece;
}

int magot_rename_parse(magot_ctx* ctx, const char* text, uint64_t len, const uint8_t* names,
                       const uint64_t* name_off, const uint8_t* values, const uint64_t* val_off,
                       const uint32_t* rank, uint64_t n_keys, uint32_t delim, uint32_t hash_bits,
                       uint64_t max_bytes, magot_rename** out, uint32_t* reason) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text) || (n_keys && (!names || !name_off || !val_off || !rank))) {
    set_error("magot_rename_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  if (hash_bits < 1 || hash_bits > 64) {
    set_error("magot_rename_parse: hash_bits outside 1..64");
    return MAGOT_ERR_ARG;
  }
  if (delim > 255 || delim == '\n') {
    set_error("magot_rename_parse: the delimiter is one byte other than LF");
    return MAGOT_ERR_ARG;
  }
  if (n_keys >= kRnMaxKeys)
    return decline(kOutside, reason, nullptr, MAGOT_RENAME_TABLE_TOO_LARGE, 0);
  const uint64_t names_len = n_keys ? name_off[n_keys] : 0, vals_len = n_keys ? val_off[n_keys] : 0;
  if (names_len >= kRnMaxBlob || vals_len >= kRnMaxBlob)
    return decline(kOutside, reason, nullptr, MAGOT_RENAME_TABLE_TOO_LARGE, 0);
  if (vals_len && !values) {
    set_error("magot_rename_parse: null argument");
    return MAGOT_ERR_ARG;
  }

  Building<magot_rename, magot_rename_destroy> guard{new magot_rename()};
  magot_rename* p = guard.p;
  p->ctx = ctx;
  RnArgs& a = p->a;
  if (n_keys && (name_off[0] || val_off[0])) {
    set_error("magot_rename_parse: the offsets begin at 0");
    return MAGOT_ERR_RANGE;
  }
  for (uint64_t k = 0; k < n_keys; ++k) {
    // monotone below a checked total: every span lies inside its blob
    if (name_off[k + 1] > names_len || name_off[k] >= name_off[k + 1] ||
        name_off[k + 1] - name_off[k] > kRnMaxName) {
      set_error("magot_rename_parse: a name is empty, longer than max_name or leaves the blob");
      return MAGOT_ERR_RANGE;
    }
    if (val_off[k + 1] > vals_len || val_off[k] > val_off[k + 1]) {
      set_error("magot_rename_parse: a value's offsets decrease or leave the blob");
      return MAGOT_ERR_RANGE;
    }
    if (rank[k] >= n_keys) {
      set_error("magot_rename_parse: a rank beyond the table");
      return MAGOT_ERR_RANGE;
    }
    const uint32_t l = (uint32_t)(name_off[k + 1] - name_off[k]);
    a.len_mask[(l - 1) >> 6] |= 1ull << ((l - 1) & 63);
    a.max_len = std::max(a.max_len, l);
  }
  if (int rc = resident_text_budget(&max_bytes)) return rc;
  if (len > max_bytes) return decline(kOutside, reason, nullptr, MAGOT_RENAME_TOO_LARGE, 0);

  a.hash_bits = hash_bits;
  a.n_keys = n_keys;
  a.cap = 2;
  a.slot_shift = 63;
  while (a.cap < 4 * n_keys) {
    a.cap <<= 1;
    --a.slot_shift;
  }
  hipStream_t s = ctx->stream;
  {
    Carve cv;  // the caller's slices: the values (pieces are copied from them), the table, the status
    // the uploads go to base + offset: the kernels' fields are const
    const uint64_t o_vals = cv.take<uint8_t>(vals_len + kTextPad);
    const uint64_t o_names = cv.take(&a.names, names_len + 1);
    const uint64_t o_noff = cv.take(&a.name_off, n_keys + 1);
    const uint64_t o_voff = cv.take(&a.val_off, n_keys + 1);
    const uint64_t o_rank = cv.take(&a.rank, n_keys + 1);
    cv.take(&a.key_hash, n_keys + 1);
    cv.take(&a.claim, a.cap);
    cv.take(&a.slots, a.cap);
    cv.take(&a.status, 1);
    // between the text's upload and the count: the table's upload, its lookup structure and
    // the status word's way back, which resident_text_open's synchronisation completes.
    // a.ix.text is set by then: the values' offset is counted from it.
    unsigned long long status = 0;
    auto table = [&](char* base) -> int {
      cv.place(base);
      a.val_base = (uint64_t)(base + o_vals - reinterpret_cast<const char*>(a.ix.text));
      if (n_keys) {
        MAGOT_HIP_TRY(hipMemcpyAsync(base + o_names, names, names_len, hipMemcpyHostToDevice, s));
        if (vals_len)
          MAGOT_HIP_TRY(hipMemcpyAsync(base + o_vals, values, vals_len, hipMemcpyHostToDevice, s));
        MAGOT_HIP_TRY(hipMemcpyAsync(base + o_noff, name_off, (n_keys + 1) * 8,
                                     hipMemcpyHostToDevice, s));
        MAGOT_HIP_TRY(hipMemcpyAsync(base + o_voff, val_off, (n_keys + 1) * 8,
                                     hipMemcpyHostToDevice, s));
        MAGOT_HIP_TRY(hipMemcpyAsync(base + o_rank, rank, n_keys * 4, hipMemcpyHostToDevice, s));
      }
      MAGOT_HIP_TRY(hipMemsetAsync(a.status, 0xff, sizeof(unsigned long long), s));
      MAGOT_HIP_TRY(launch_rn_table(a, s));
      MAGOT_HIP_TRY(hipMemcpyAsync(&status, a.status, 8, hipMemcpyDeviceToHost, s));
      return MAGOT_OK;
    };
    if (int rc = resident_text_open(ctx, text, len, delim, '\n', cv.used, table, &p->rt, &a.ix))
      return rc;
    if (status != ~0ull) return decline(kOutside, reason, nullptr, (uint32_t)status, 0);
    a.n_fields = p->rt.total;
    if (a.n_fields > len) {
      set_error("magot_rename_parse: more delimiters than bytes");
      return MAGOT_ERR_STATE;
    }
  }
  {
    const uint64_t F = a.n_fields;
    p->tmp_bytes = exclusive_sum_bytes<uint64_t>(F + 2);  // the hits are at most the fields
    Carve cv;
    cv.take(&a.ix.pos, F + 1);
    cv.take(&a.f_hit, F + 1);
    cv.take(&a.f_hpos, F + 1);
    cv.take(&a.f_key, F + 1);
    cv.take(&p->tmp, p->tmp_bytes);
    size_t free_b = 0, total_b = 0;
    MAGOT_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (cv.used > free_b / 2)
      return decline(kOutside, reason, nullptr, MAGOT_RENAME_TOO_LARGE, 0);
    MAGOT_HIP_TRY(hipMalloc(&p->field_mem, cv.used + 256));
    cv.place(p->field_mem);
    MAGOT_HIP_TRY(launch_text_fill(a.ix, kTextFillPlain, s));
    MAGOT_HIP_TRY(launch_rn_match(a, p->tmp, p->tmp_bytes, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&a.n_hits, a.f_hpos + F, 8, hipMemcpyDeviceToHost, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
    if (a.n_hits > F) {
      set_error("magot_rename_parse: more hits than fields");
      return MAGOT_ERR_STATE;
    }
  }
  {
    const uint64_t H = a.n_hits;
    Carve cv;
    cv.take(&a.h_end, H + 1);
    cv.take(&a.h_delta, H + 1);
    cv.take(&a.h_dsum, H + 1);
    cv.take(&a.h_pcnt, H + 2);
    cv.take(&a.h_pbase, H + 2);
    cv.take(&a.h_key, H + 1);
    MAGOT_HIP_TRY(hipMalloc(&p->hit_mem, cv.used + 256));
    cv.place(p->hit_mem);
    uint64_t shift = 0;
    if (len) {  // an empty text has no run and no piece
      MAGOT_HIP_TRY(launch_rn_layout(a, p->tmp, p->tmp_bytes, s));
      MAGOT_HIP_TRY(hipMemcpyAsync(&shift, a.h_dsum + H, 8, hipMemcpyDeviceToHost, s));
      MAGOT_HIP_TRY(hipMemcpyAsync(&p->r.n_pieces, a.h_pbase + H + 1, 8, hipMemcpyDeviceToHost, s));
      MAGOT_HIP_TRY(hipStreamSynchronize(s));
    }
    p->r.out_bytes = len + shift;  // mod 2^64: the shift may be negative
    // every hit keeps its d, and a text without one keeps all its bytes
    if (len && !p->r.out_bytes) {
      set_error("magot_rename_parse: a text with an empty output");
      return MAGOT_ERR_STATE;
    }
  }
  *out = guard.release();
  return MAGOT_OK;
}

int magot_rename_sizes(const magot_rename* p, uint64_t* n_lines, uint64_t* n_fields,
                       uint64_t* n_hits, uint64_t* out_bytes) {
  if (!p) {
    set_error("magot_rename_sizes: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_lines) *n_lines = p->rt.n_lines;
  if (n_fields) *n_fields = p->a.n_fields;
  if (n_hits) *n_hits = p->a.n_hits;
  if (out_bytes) *out_bytes = p->r.out_bytes;
  return MAGOT_OK;
}

double magot_rename_upload_ms(const magot_rename* p) { return p ? (double)p->rt.upload_ms : 0.0; }

int magot_rename_hits(magot_ctx* ctx, magot_rename* p, uint64_t* end, uint32_t* key) {
  if (int rc = handle_of(ctx, p, "magot_rename_hits", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t n = p->a.n_hits;
  if (end && n) MAGOT_HIP_TRY(hipMemcpy(end, p->a.h_end, n * 8, hipMemcpyDeviceToHost));
  if (key && n) MAGOT_HIP_TRY(hipMemcpy(key, p->a.h_key, n * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_rename_render(magot_ctx* ctx, magot_rename* p, uint64_t* bytes) {
  if (int rc = handle_of(ctx, p, "magot_rename_render", "handle")) return rc;
  if (!bytes) {
    set_error("magot_rename_render: null argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (int rc = rn_plan_render(p)) return rc;
  MAGOT_HIP_TRY(launch_rn_render(p->a, p->r, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  p->rendered = true;
  *bytes = p->r.out_bytes;
  return MAGOT_OK;
}

int magot_rename_render_fetch(magot_ctx* ctx, magot_rename* p, uint8_t* out, uint64_t cap) {
  if (int rc = handle_of(ctx, p, "magot_rename_render_fetch", "handle")) return rc;
  if (!p->rendered) {
    set_error("magot_rename_render_fetch: nothing rendered");
    return MAGOT_ERR_STATE;
  }
  const uint64_t need = p->r.out_bytes;
  if (cap < need || (need && !out)) {
    set_error("magot_rename_render_fetch: buffer too small");
    return MAGOT_ERR_ARG;
  }
  if (need) MAGOT_HIP_TRY(hipMemcpy(out, p->r.out, need, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_rename_time(magot_ctx* ctx, magot_rename* p, int iters, double* ms6,
                      uint64_t* text_bytes, uint64_t* out_bytes) {
  if (int rc = handle_of(ctx, p, "magot_rename_time", "handle")) return rc;
  if (iters <= 0 || !ms6) {
    set_error("magot_rename_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text_bytes) *text_bytes = p->a.ix.n;
  if (out_bytes) *out_bytes = p->r.out_bytes;
  for (int k = 0; k < kRnPasses; ++k) ms6[k] = 0;
  if (!p->a.ix.n) return MAGOT_OK;  // an empty text: nothing to time
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!p->copy_mem) MAGOT_HIP_TRY(hipMalloc(&p->copy_mem, p->a.ix.n + 256));
  if (int rc = rn_plan_render(p)) return rc;
  // every pass writes what it wrote in magot_rename_parse: the answers stand
  return time_passes(ctx, iters, kRnPasses, ms6,
                     [&](int k) { return rn_pass(p, k, ctx->stream); });
}

}  // extern "C"
