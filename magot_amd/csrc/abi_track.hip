// C ABI: position_dic's bit track and its sliding windows (track.hip;
// genome.py:981-1100).
#include "abi_internal.h"

using namespace magot;

struct magot_track {
  magot_ctx* ctx = nullptr;
  const magot_genome* g = nullptr;
  void* arena = nullptr;
  uint32_t* words = nullptr;    // the track: track_plane_words(span) words
  uint32_t* scratch = nullptr;  // a second plane (paint with 0, the timed class pass)
  uint64_t* contig_base = nullptr;
  uint32_t* blk_count = nullptr;  // n_blocks + 1
  uint32_t* blk_rank = nullptr;   // n_blocks + 1
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  uint64_t n_words = 0, n_blocks = 0, plane_words = 0;
  bool dirty = true;  // the rank directory is older than the track
  void* stage = nullptr;  // one contig's bytes (magot_track_set_bytes / _get_bytes)
  uint64_t stage_bytes = 0;
};

struct magot_track_windows {
  magot_ctx* ctx = nullptr;
  magot_track* t = nullptr;
  void* arena = nullptr;
  TrackWindowArgs a{};
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  void* flips = nullptr;
  uint64_t n_flips = 0;
  bool have_flips = false;
};

namespace {

int track_rank_ready(magot_ctx* ctx, magot_track* t) {
  if (!t->dirty) return MAGOT_OK;
  MAGOT_HIP_TRY(launch_track_rank(t->words, t->n_blocks, t->blk_count, t->blk_rank, t->scan_tmp,
                                  t->scan_bytes, ctx->stream));
  t->dirty = false;
  return MAGOT_OK;
}

// rows inside their contigs; `piece` > 0: no row longer than it
int track_check_rows(const magot_track* t, const magot_mask_interval* rows, uint64_t n_rows,
                     uint32_t piece, const char* who) {
  if (n_rows && !rows) {
    set_error(std::string(who) + ": null row table");
    return MAGOT_ERR_ARG;
  }
  const uint64_t nc = t->g->contig_len.size();
  for (uint64_t i = 0; i < n_rows; ++i) {
    const magot_mask_interval& iv = rows[i];
    if (iv.contig >= nc || (uint64_t)iv.start + iv.len > t->g->contig_len[iv.contig]) {
      set_error(std::string(who) + ": row " + std::to_string(i) + " is outside its contig");
      return MAGOT_ERR_RANGE;
    }
    if (piece && iv.len > piece) {
      set_error(std::string(who) + ": row " + std::to_string(i) + " is longer than one piece");
      return MAGOT_ERR_ARG;
    }
  }
  return MAGOT_OK;
}

int track_stage(magot_track* t, uint64_t bytes) {
  if (bytes <= t->stage_bytes) return MAGOT_OK;
  if (t->stage) (void)hipFree(t->stage);
  t->stage = nullptr;
  t->stage_bytes = 0;
  MAGOT_HIP_TRY(hipMalloc(&t->stage, bytes));
  t->stage_bytes = bytes;
  return MAGOT_OK;
}

}  // namespace

extern "C" {

void magot_track_destroy(magot_track* t) {
  if (!t) return;
  if (t->ctx) (void)hipSetDevice(t->ctx->device);
  if (t->stage) (void)hipFree(t->stage);
  if (t->arena) (void)hipFree(t->arena);
  delete t;
}

void magot_track_windows_destroy(magot_track_windows* w) {
  if (!w) return;
  if (w->ctx) (void)hipSetDevice(w->ctx->device);
  if (w->flips) (void)hipFree(w->flips);
  if (w->arena) (void)hipFree(w->arena);
  delete w;
}

uint32_t magot_track_rank_block(void) { return 32u * kRankWords; }

int magot_track_create(magot_ctx* ctx, const magot_genome* g, magot_track** out,
                       uint64_t* n_words) {
  if (int rc = bind(ctx)) return rc;
  if (!g || !out || g->ctx != ctx) {
    set_error("magot_track_create: null argument, or a genome of another context");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  Building<magot_track, magot_track_destroy> guard{new magot_track()};
  magot_track* t = guard.p;
  t->ctx = ctx;
  t->g = g;
  t->n_words = g->span / 32;
  t->n_blocks = track_blocks(g->span);
  t->plane_words = track_plane_words(g->span);
  t->scan_bytes = track_scan_bytes(t->n_blocks + 1);
  const uint64_t nc = g->contig_base.size();
  Carve cv;
  cv.take(&t->words, t->plane_words);
  cv.take(&t->scratch, t->plane_words);
  cv.take(&t->contig_base, nc + 1);
  cv.take(&t->blk_count, t->n_blocks + 1);
  cv.take(&t->blk_rank, t->n_blocks + 1);
  cv.take(&t->scan_tmp, t->scan_bytes);
  MAGOT_HIP_TRY(hipMalloc(&t->arena, cv.used + 256));
  cv.place(t->arena);
  // both planes zeroed whole: no pass writes a word at or past n_words
  MAGOT_HIP_TRY(hipMemsetAsync(t->words, 0, 2 * ((t->plane_words * 4 + 255) & ~255ull),
                               ctx->stream));
  if (nc)
    MAGOT_HIP_TRY(hipMemcpy(t->contig_base, g->contig_base.data(), nc * 8, hipMemcpyHostToDevice));
  if (n_words) *n_words = t->n_words;
  *out = guard.release();
  return MAGOT_OK;
}

int magot_track_base_class(magot_ctx* ctx, magot_track* t, const magot_genome* g, uint32_t flags) {
  if (int rc = handle_of(ctx, t, "magot_track_base_class", "track")) return rc;
  if (g != t->g) {
    set_error("magot_track_base_class: the track was created over another genome");
    return MAGOT_ERR_ARG;
  }
  if (flags & ~(uint32_t)(MAGOT_TRACK_GC | MAGOT_TRACK_REPLACE)) {
    set_error("magot_track_base_class: unknown flag");
    return MAGOT_ERR_ARG;
  }
  t->dirty = true;
  MAGOT_HIP_TRY(launch_track_class(g->nib, t->n_words, kOrigin, g->extent, flags & MAGOT_TRACK_GC,
                                   flags & MAGOT_TRACK_REPLACE, t->words, ctx->stream));
  return MAGOT_OK;
}

int magot_track_paint(magot_ctx* ctx, magot_track* t, const magot_mask_interval* rows,
                      uint64_t n_rows, int value) {
  if (int rc = handle_of(ctx, t, "magot_track_paint", "track")) return rc;
  if (value != 0 && value != 1) {
    set_error("magot_track_paint: value must be 0 or 1");
    return MAGOT_ERR_ARG;
  }
  if (int rc = track_check_rows(t, rows, n_rows, kMaskPiece, "magot_track_paint")) return rc;
  if (!n_rows) return MAGOT_OK;
  DevBuf d;
  MAGOT_HIP_TRY(hipMalloc(&d.p, n_rows * sizeof(magot_mask_interval)));
  MAGOT_HIP_TRY(hipMemcpy(d.p, rows, n_rows * sizeof(magot_mask_interval), hipMemcpyHostToDevice));
  const auto* d_rows = static_cast<const magot_mask_interval*>(d.p);
  t->dirty = true;
  if (value) {
    MAGOT_HIP_TRY(launch_mask_paint_rows(d_rows, n_rows, t->contig_base, t->words, t->g->span,
                                         ctx->stream));
  } else {
    MAGOT_HIP_TRY(hipMemsetAsync(t->scratch, 0, t->plane_words * 4, ctx->stream));
    MAGOT_HIP_TRY(launch_mask_paint_rows(d_rows, n_rows, t->contig_base, t->scratch, t->g->span,
                                         ctx->stream));
    MAGOT_HIP_TRY(launch_track_andnot(t->words, t->scratch, t->n_words, ctx->stream));
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));  // the rows are freed on return
  return MAGOT_OK;
}

int magot_track_set_bytes(magot_ctx* ctx, magot_track* t, uint32_t contig, const uint8_t* bytes,
                          uint64_t len) {
  if (int rc = handle_of(ctx, t, "magot_track_set_bytes", "track")) return rc;
  if (contig >= t->g->contig_len.size() || len != t->g->contig_len[contig] || (len && !bytes)) {
    set_error("magot_track_set_bytes: no such contig, or not one byte per base of it");
    return MAGOT_ERR_ARG;
  }
  if (!len) return MAGOT_OK;
  const uint64_t lo = t->g->contig_base[contig], hi = lo + len;
  const uint64_t n = ((hi + 31) >> 5) - (lo >> 5);
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));  // an earlier pass may read the staging
  if (int rc = track_stage(t, 32 * n)) return rc;
  // the bytes before the first base and after the last are never used: the
  // kernel keeps the track's own bits there
  MAGOT_HIP_TRY(hipMemcpy(static_cast<uint8_t*>(t->stage) + (lo & 31), bytes, len,
                          hipMemcpyHostToDevice));
  t->dirty = true;
  MAGOT_HIP_TRY(launch_track_bytes_set(static_cast<const uint8_t*>(t->stage), lo, hi, t->words,
                                       ctx->stream));
  return MAGOT_OK;
}

int magot_track_get_bytes(magot_ctx* ctx, magot_track* t, uint32_t contig, uint8_t* bytes,
                          uint64_t len) {
  if (int rc = handle_of(ctx, t, "magot_track_get_bytes", "track")) return rc;
  if (contig >= t->g->contig_len.size() || len != t->g->contig_len[contig] || (len && !bytes)) {
    set_error("magot_track_get_bytes: no such contig, or not one byte per base of it");
    return MAGOT_ERR_ARG;
  }
  if (!len) return MAGOT_OK;
  const uint64_t lo = t->g->contig_base[contig], hi = lo + len;
  const uint64_t n = ((hi + 31) >> 5) - (lo >> 5);
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (int rc = track_stage(t, 32 * n)) return rc;
  MAGOT_HIP_TRY(launch_track_bytes_get(t->words, lo, hi, static_cast<uint8_t*>(t->stage),
                                       ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(bytes, static_cast<const uint8_t*>(t->stage) + (lo & 31), len,
                          hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_track_fetch(magot_ctx* ctx, magot_track* t, uint32_t* words, uint64_t cap_words,
                      uint64_t* n_words) {
  if (int rc = handle_of(ctx, t, "magot_track_fetch", "track")) return rc;
  if (n_words) *n_words = t->n_words;
  if (!words) return MAGOT_OK;
  if (cap_words < t->n_words) {
    set_error("magot_track_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (t->n_words)
    MAGOT_HIP_TRY(hipMemcpy(words, t->words, t->n_words * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_track_windows_create(magot_ctx* ctx, magot_track* t, uint64_t window, uint64_t jump,
                               const uint8_t* skip, magot_track_windows** out,
                               uint64_t* n_windows, uint64_t* first) {
  if (int rc = handle_of(ctx, t, "magot_track_windows_create", "track")) return rc;
  if (!out) {
    set_error("magot_track_windows_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (window < 1 || jump < 1) {
    set_error("magot_track_windows_create: the window and the jump must be at least 1");
    return MAGOT_ERR_ARG;
  }
  // genome.py:1043, 1048: a contig longer than the window has
  // (len - window) / jump windows (integer division), any other none
  const uint64_t nc = t->g->contig_len.size();
  std::vector<uint64_t> tab(nc + 1);
  uint64_t total = 0;
  for (uint64_t c = 0; c < nc; ++c) {
    tab[c] = total;
    const uint64_t len = t->g->contig_len[c];
    if (len > window && !(skip && skip[c])) total += (len - window) / jump;
  }
  tab[nc] = total;
  Building<magot_track_windows, magot_track_windows_destroy> guard{new magot_track_windows()};
  magot_track_windows* w = guard.p;
  w->ctx = ctx;
  w->t = t;
  const uint64_t groups = track_flip_groups(total);
  w->scan_bytes = track_scan_bytes(groups + 1);
  TrackWindowArgs& a = w->a;
  Carve cv;
  uint64_t* d_first;  // uploaded into; the kernels read it as const
  cv.take(&d_first, nc + 1);
  cv.take(&a.sums, total);
  cv.take(&a.flip_count, groups + 1);
  cv.take(&a.flip_slot, groups + 1);
  cv.take(&w->scan_tmp, w->scan_bytes);
  MAGOT_HIP_TRY(hipMalloc(&w->arena, cv.used + 256));
  cv.place(w->arena);
  MAGOT_HIP_TRY(hipMemcpy(d_first, tab.data(), (nc + 1) * 8, hipMemcpyHostToDevice));
  a.track = t->words;
  a.rank = t->blk_rank;
  a.contig_base = t->contig_base;
  a.first = d_first;
  a.n_contigs = nc;
  a.n_windows = total;
  a.W = window;
  a.jump = jump;
  if (int rc = track_rank_ready(ctx, t)) return rc;
  MAGOT_HIP_TRY(launch_track_windows(a, ctx->stream));
  if (n_windows) *n_windows = total;
  if (first) memcpy(first, tab.data(), (nc + 1) * 8);
  *out = guard.release();
  return MAGOT_OK;
}

int magot_track_windows_fetch(magot_ctx* ctx, magot_track_windows* w, uint32_t* sums,
                              uint64_t cap) {
  if (int rc = bind(ctx)) return rc;
  if (!w || w->ctx != ctx || cap < w->a.n_windows || (w->a.n_windows && !sums)) {
    set_error("magot_track_windows_fetch: null handle, or output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (w->a.n_windows)
    MAGOT_HIP_TRY(hipMemcpy(sums, w->a.sums, w->a.n_windows * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_track_transitions(magot_ctx* ctx, magot_track_windows* w, uint32_t s_min,
                            uint64_t* n) {
  if (int rc = bind(ctx)) return rc;
  if (!w || w->ctx != ctx || !n) {
    set_error("magot_track_transitions: null argument");
    return MAGOT_ERR_ARG;
  }
  w->have_flips = false;
  if (w->flips) MAGOT_HIP_TRY(hipFree(w->flips));
  w->flips = nullptr;
  w->a.flip_index = nullptr;
  w->n_flips = 0;
  MAGOT_HIP_TRY(launch_track_flip_count(w->a, s_min, w->scan_tmp, w->scan_bytes, ctx->stream));
  const uint64_t groups = track_flip_groups(w->a.n_windows);
  uint64_t total = 0;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(&total, w->a.flip_slot + groups, 8, hipMemcpyDeviceToHost));
  if (total > w->a.n_windows) {
    set_error("magot_track_transitions: inconsistent count");
    return MAGOT_ERR_HIP;
  }
  if (total) {
    MAGOT_HIP_TRY(hipMalloc(&w->flips, total * 8));
    w->a.flip_index = static_cast<uint64_t*>(w->flips);
    MAGOT_HIP_TRY(launch_track_flip_write(w->a, s_min, total, ctx->stream));
  }
  w->n_flips = total;
  w->have_flips = true;
  *n = total;
  return MAGOT_OK;
}

int magot_track_transitions_fetch(magot_ctx* ctx, magot_track_windows* w, uint64_t* index,
                                  uint64_t cap) {
  if (int rc = bind(ctx)) return rc;
  if (!w || w->ctx != ctx) {
    set_error("magot_track_transitions_fetch: null handle");
    return MAGOT_ERR_ARG;
  }
  if (!w->have_flips) {
    set_error("magot_track_transitions_fetch: call magot_track_transitions first");
    return MAGOT_ERR_STATE;
  }
  if (cap < w->n_flips || (w->n_flips && !index)) {
    set_error("magot_track_transitions_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (w->n_flips)
    MAGOT_HIP_TRY(hipMemcpy(index, w->flips, w->n_flips * 8, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_track_count(magot_ctx* ctx, magot_track* t, const magot_mask_interval* rows,
                      uint64_t n_rows, uint32_t* ones) {
  if (int rc = handle_of(ctx, t, "magot_track_count", "track")) return rc;
  if (n_rows && !ones) {
    set_error("magot_track_count: null output");
    return MAGOT_ERR_ARG;
  }
  if (int rc = track_check_rows(t, rows, n_rows, 0, "magot_track_count")) return rc;
  if (!n_rows) return MAGOT_OK;
  DevBuf d, o;
  MAGOT_HIP_TRY(hipMalloc(&d.p, n_rows * sizeof(magot_mask_interval)));
  MAGOT_HIP_TRY(hipMalloc(&o.p, n_rows * 4));
  MAGOT_HIP_TRY(hipMemcpy(d.p, rows, n_rows * sizeof(magot_mask_interval), hipMemcpyHostToDevice));
  if (int rc = track_rank_ready(ctx, t)) return rc;
  MAGOT_HIP_TRY(launch_track_count(static_cast<const magot_mask_interval*>(d.p), n_rows,
                                   t->contig_base, t->words, t->blk_rank, t->g->span,
                                   static_cast<uint32_t*>(o.p), ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(ones, o.p, n_rows * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_track_time(magot_ctx* ctx, magot_track* t, magot_track_windows* w, uint32_t s_min,
                     int iters, double* ms5) {
  if (int rc = handle_of(ctx, t, "magot_track_time", "track")) return rc;
  if (iters <= 0 || !ms5 || (w && (w->t != t || w->ctx != ctx))) {
    set_error("magot_track_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  // one whole-contig row per contig for the count pass
  const uint64_t nc = t->g->contig_len.size();
  std::vector<magot_mask_interval> rows;
  for (uint64_t c = 0; c < nc; ++c)
    if (t->g->contig_len[c] < (1ull << 32))
      rows.push_back({(uint32_t)c, 0u, (uint32_t)t->g->contig_len[c]});
  DevBuf d, o;
  if (!rows.empty()) {
    MAGOT_HIP_TRY(hipMalloc(&d.p, rows.size() * sizeof(magot_mask_interval)));
    MAGOT_HIP_TRY(hipMalloc(&o.p, rows.size() * 4));
    MAGOT_HIP_TRY(hipMemcpy(d.p, rows.data(), rows.size() * sizeof(magot_mask_interval),
                            hipMemcpyHostToDevice));
  }
  if (int rc = track_rank_ready(ctx, t)) return rc;
  uint64_t cap = 0;
  if (w) {  // sizes the index list for this s_min
    if (int rc = magot_track_transitions(ctx, w, s_min, &cap)) return rc;
  }
  return time_passes(
      ctx, iters, 5, ms5,
      [&](int k) {
        switch (k) {
          case 0:  // into the scratch plane: the track keeps its bits
            return launch_track_class(t->g->nib, t->n_words, kOrigin, t->g->extent, false, true,
                                      t->scratch, ctx->stream);
          case 1:
            return launch_track_rank(t->words, t->n_blocks, t->blk_count, t->blk_rank,
                                     t->scan_tmp, t->scan_bytes, ctx->stream);
          case 2:
            return launch_track_windows(w->a, ctx->stream);
          case 3:
            if (hipError_t e = launch_track_flip_count(w->a, s_min, w->scan_tmp, w->scan_bytes,
                                                       ctx->stream))
              return e;
            return launch_track_flip_write(w->a, s_min, cap, ctx->stream);
          default:
            return launch_track_count(static_cast<const magot_mask_interval*>(d.p), rows.size(),
                                      t->contig_base, t->words, t->blk_rank, t->g->span,
                                      static_cast<uint32_t*>(o.p), ctx->stream);
        }
      },
      [&](int k) { return k >= 2 && k <= 3 && !w; });  // no window set was given
}

}  // extern "C"
