// C ABI: column cuts of a resident text (tabcut.hip; magot_smallfuncs.py:12-18,
// genome_tools.py:449-454): the text and the literals made resident, the line
// and TAB indexes, every line's verdict and place, and the cut text.
#include "abi_internal.h"

using namespace magot;

struct magot_tabcut {
  magot_ctx* ctx = nullptr;
  ResidentText rt;           // the text and the block counts of its LFs and TABs; the literals, the status
  void* line_mem = nullptr;  // everything sized by the lines and the TABs
  void* out_mem = nullptr;   // the rendered text and its pieces
  void* copy_mem = nullptr;  // magot_tabcut_time's copy target
  TcArgs a{};
  TcRenderArgs r{};
  TextFill line_mode = kTextFillLines;
  uint64_t n_kept = 0;
  uint64_t short_line = ~0ull;  // the lowest short line of error mode, 0-based
  bool rendered = false;
  void* tmp = nullptr;  // the layout scans' scratch
  size_t tmp_bytes = 0;
};

namespace {

constexpr int kTcPasses = 6;

constexpr char kOutside[] =
    "magot_tabcut_parse: input outside the device path; use the host loop";

// The buffers of a render: the output and one row per piece.  Replaces the
// handle's last ones.
int tc_plan_render(magot_tabcut* p) {
  if (p->out_mem) MAGOT_HIP_TRY(hipFree(p->out_mem));
  p->out_mem = nullptr;
  p->rendered = false;
  TcRenderArgs& r = p->r;
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

// pass k of magot_tabcut_time on the handle's own buffers
hipError_t tc_pass(const magot_tabcut* p, int k, hipStream_t s) {
  const TcArgs& a = p->a;
  switch (k) {
    case 0:
      if (hipError_t e = text_index_pass(a.ix, p->rt, p->line_mode, s)) return e;
      return launch_text_fill(a.tx, kTextFillPlain, s);
    case 1: return launch_tc_rows(a, s);
    case 2: return launch_tc_layout(a, p->tmp, p->tmp_bytes, s);
    case 3: return launch_tc_pieces(a, p->r, s);
    case 4: return launch_tc_copy(a, p->r, s);
    default: return hipMemcpyAsync(p->copy_mem, a.ix.text, a.ix.n, hipMemcpyDeviceToDevice, s);
  }
}

}  // namespace

extern "C" {

void magot_tabcut_destroy(magot_tabcut* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->copy_mem) (void)hipFree(p->copy_mem);
  if (p->out_mem) (void)hipFree(p->out_mem);
  if (p->line_mem) (void)hipFree(p->line_mem);
  if (p->rt.mem) (void)hipFree(p->rt.mem);
  delete p;
}

void magot_tabcut_params(uint32_t* piece, uint32_t* text_block, uint32_t* max_items) {
  if (piece) *piece = kTcPiece;
  if (text_block) *text_block = kTextBlock;
  if (max_items) *max_items = kTcMaxItems;
}

int magot_tabcut_parse(magot_ctx* ctx, const char* text, uint64_t len,
                       const magot_tabcut_item* items, uint32_t n_items, const uint8_t* literals,
                       uint64_t literals_len, uint32_t need, uint32_t short_mode,
                       uint32_t cr_check, uint64_t max_bytes, magot_tabcut** out,
                       uint32_t* reason) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text) || (n_items && !items) || (literals_len && !literals)) {
    set_error("magot_tabcut_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  if (n_items > kTcMaxItems) {
    set_error("magot_tabcut_parse: more items than a program holds");
    return MAGOT_ERR_ARG;
  }
  if (short_mode > MAGOT_TABCUT_SHORT_ERROR || need > kTcMaxLines) {
    set_error("magot_tabcut_parse: bad short_mode or need");
    return MAGOT_ERR_ARG;
  }
  if (literals_len > 0xffffffffull) {
    set_error("magot_tabcut_parse: 4 GiB of literals or more");
    return MAGOT_ERR_ARG;
  }
  for (uint32_t i = 0; i < n_items; ++i) {
    const magot_tabcut_item& it = items[i];
    if (it.kind == MAGOT_TABCUT_ITEM_LITERAL) {
      if (it.a > literals_len || it.b > literals_len - it.a) {
        set_error("magot_tabcut_parse: a literal outside the blob");
        return MAGOT_ERR_ARG;
      }
    } else if (it.kind == MAGOT_TABCUT_ITEM_FIELDS) {
      if (it.a > it.b || it.b > need) {
        set_error("magot_tabcut_parse: a field range that decreases or names a field above need");
        return MAGOT_ERR_ARG;
      }
    } else {
      set_error("magot_tabcut_parse: an item that is neither a literal nor a field range");
      return MAGOT_ERR_ARG;
    }
  }
  if (int rc = resident_text_budget(&max_bytes)) return rc;
  if (len > max_bytes) return decline(kOutside, reason, nullptr, MAGOT_TABCUT_TOO_LARGE, 0);

  Building<magot_tabcut, magot_tabcut_destroy> guard{new magot_tabcut()};
  magot_tabcut* p = guard.p;
  p->ctx = ctx;
  p->line_mode = cr_check ? kTextFillLinesCr : kTextFillLines;
  TcArgs& a = p->a;
  a.need = need;
  a.short_mode = short_mode;
  a.n_items = n_items;
  for (uint32_t i = 0; i < n_items; ++i) a.items[i] = TcItem{items[i].kind, items[i].a, items[i].b};
  if (!len) {  // an empty text: no line, nothing launched
    *out = guard.release();
    return MAGOT_OK;
  }
  hipStream_t s = ctx->stream;
  {
    Carve cv;  // the caller's slices: the literals (pieces are copied from them), the status words
    const uint64_t o_lit = cv.take<uint8_t>(literals_len + kTextPad);
    cv.take(&a.status, 2);
    cv.take(&a.n_kept, 1);
    auto blob = [&](char* base) -> int {
      cv.place(base);
      a.lit_base = (uint64_t)(base + o_lit - reinterpret_cast<const char*>(a.ix.text));
      if (literals_len)
        MAGOT_HIP_TRY(hipMemcpyAsync(base + o_lit, literals, literals_len, hipMemcpyHostToDevice, s));
      MAGOT_HIP_TRY(hipMemsetAsync(a.status, 0xff, 2 * sizeof(unsigned long long), s));
      return MAGOT_OK;
    };
    if (int rc = resident_text_open(ctx, text, len, '\n', '\t', cv.used, blob, &p->rt, &a.ix))
      return rc;
  }
  a.ix.stray_status = a.status;
  a.ix.stray_reason = MAGOT_TABCUT_STRAY_CR;
  a.ix.n_lines = p->rt.n_lines;
  a.n_tabs = p->rt.total2;
  if (a.ix.n_lines > kTcMaxLines)
    return decline(kOutside, reason, nullptr, MAGOT_TABCUT_TOO_MANY_LINES, 0);
  if (a.n_tabs > len || a.ix.n_lines > len) {
    set_error("magot_tabcut_parse: more TABs or lines than bytes");
    return MAGOT_ERR_STATE;
  }
  a.tx = a.ix;  // the TABs' index over their own block counts
  a.tx.byte = '\t';
  a.tx.byte2 = kTextNoByte;
  a.tx.blk = a.ix.blk2;
  a.tx.pre = a.ix.pre2;
  a.tx.blk2 = a.tx.pre2 = nullptr;
  a.tx.stray_status = nullptr;
  const uint64_t L = a.ix.n_lines, T = a.n_tabs;
  {
    p->tmp_bytes = exclusive_sum_bytes<uint64_t>(L + 1);
    Carve cv;
    cv.take(&a.ix.pos, L + 1);
    cv.take(&a.tx.pos, T + 1);
    cv.take(&a.verdict, L + 1);
    for (uint64_t** f : {&a.tab0, &a.olen, &a.obase, &a.pcnt, &a.pbase}) cv.take(f, L + 1);
    cv.take(&p->tmp, p->tmp_bytes);
    size_t free_b = 0, total_b = 0;
    MAGOT_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (cv.used > free_b / 2) return decline(kOutside, reason, nullptr, MAGOT_TABCUT_TOO_LARGE, 0);
    MAGOT_HIP_TRY(hipMalloc(&p->line_mem, cv.used + 256));
    cv.place(p->line_mem);
  }
  MAGOT_HIP_TRY(launch_text_fill(a.ix, p->line_mode, s));
  MAGOT_HIP_TRY(launch_text_fill(a.tx, kTextFillPlain, s));
  MAGOT_HIP_TRY(launch_tc_rows(a, s));
  MAGOT_HIP_TRY(launch_tc_layout(a, p->tmp, p->tmp_bytes, s));
  unsigned long long status[2] = {0, 0}, kept = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(status, a.status, sizeof status, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&kept, a.n_kept, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&p->r.out_bytes, a.obase + L, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&p->r.n_pieces, a.pbase + L, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (status[0] != ~0ull) return decline(kOutside, reason, nullptr, (uint32_t)(status[0] & 0xff), 0);
  if (kept > L) {
    set_error("magot_tabcut_parse: more kept lines than lines");
    return MAGOT_ERR_STATE;
  }
  p->n_kept = kept;
  uint32_t why = 0;
  uint64_t line0 = 0;
  if (first_offence(status[1], &why, &line0)) p->short_line = line0;
  *out = guard.release();
  return MAGOT_OK;
}

int magot_tabcut_sizes(const magot_tabcut* p, uint64_t* n_lines, uint64_t* n_tabs,
                       uint64_t* n_kept, uint64_t* n_pieces, uint64_t* out_bytes,
                       uint64_t* short_line) {
  if (!p) {
    set_error("magot_tabcut_sizes: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_lines) *n_lines = p->a.ix.n_lines;
  if (n_tabs) *n_tabs = p->a.n_tabs;
  if (n_kept) *n_kept = p->n_kept;
  if (n_pieces) *n_pieces = p->r.n_pieces;
  if (out_bytes) *out_bytes = p->r.out_bytes;
  if (short_line) *short_line = p->short_line;
  return MAGOT_OK;
}

double magot_tabcut_upload_ms(const magot_tabcut* p) { return p ? (double)p->rt.upload_ms : 0.0; }

int magot_tabcut_rows(magot_ctx* ctx, magot_tabcut* p, uint8_t* verdict, uint64_t* offset) {
  if (int rc = handle_of(ctx, p, "magot_tabcut_rows", "handle")) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t n = p->a.ix.n_lines;
  if (int rc = fetch_rows(verdict, p->a.verdict, n)) return rc;
  return fetch_rows(offset, p->a.obase, n);
}

int magot_tabcut_render(magot_ctx* ctx, magot_tabcut* p, uint64_t* bytes) {
  if (int rc = handle_of(ctx, p, "magot_tabcut_render", "handle")) return rc;
  if (!bytes) {
    set_error("magot_tabcut_render: null argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (int rc = tc_plan_render(p)) return rc;
  MAGOT_HIP_TRY(launch_tc_pieces(p->a, p->r, ctx->stream));
  MAGOT_HIP_TRY(launch_tc_copy(p->a, p->r, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  p->rendered = true;
  *bytes = p->r.out_bytes;
  return MAGOT_OK;
}

int magot_tabcut_render_fetch(magot_ctx* ctx, magot_tabcut* p, uint8_t* out, uint64_t cap) {
  if (int rc = handle_of(ctx, p, "magot_tabcut_render_fetch", "handle")) return rc;
  if (!p->rendered) {
    set_error("magot_tabcut_render_fetch: nothing rendered");
    return MAGOT_ERR_STATE;
  }
  const uint64_t need = p->r.out_bytes;
  if (cap < need || (need && !out)) {
    set_error("magot_tabcut_render_fetch: buffer too small");
    return MAGOT_ERR_ARG;
  }
  if (need) MAGOT_HIP_TRY(hipMemcpy(out, p->r.out, need, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_tabcut_time(magot_ctx* ctx, magot_tabcut* p, int iters, double* ms6,
                      uint64_t* text_bytes, uint64_t* out_bytes) {
  if (int rc = handle_of(ctx, p, "magot_tabcut_time", "handle")) return rc;
  if (iters <= 0 || !ms6) {
    set_error("magot_tabcut_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text_bytes) *text_bytes = p->a.ix.n;
  if (out_bytes) *out_bytes = p->r.out_bytes;
  for (int k = 0; k < kTcPasses; ++k) ms6[k] = 0;
  if (!p->a.ix.n) return MAGOT_OK;  // an empty text: nothing to time
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!p->copy_mem) MAGOT_HIP_TRY(hipMalloc(&p->copy_mem, p->a.ix.n + 256));
  if (int rc = tc_plan_render(p)) return rc;
  // every pass writes what it wrote in magot_tabcut_parse: the answers stand
  return time_passes(ctx, iters, kTcPasses, ms6,
                     [&](int k) { return tc_pass(p, k, ctx->stream); });
}

}  // extern "C"
