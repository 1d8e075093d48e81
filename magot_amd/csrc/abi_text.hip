// C ABI: tables parsed from text streamed to the device in chunks, the depth
// table (depth.hip) and the FASTQ read lengths (fastq.hip).
#include <unordered_set>

#include "abi_internal.h"

using namespace magot;

// ---------------------------------------------------------------------------
// depth_from_gff's integer track (depth.hip; genome_tools.py:598-652)
// ---------------------------------------------------------------------------

struct magot_depth {
  magot_ctx* ctx = nullptr;
  void* arena_mem = nullptr;  // everything but the text buffers
  int32_t* arena = nullptr;
  uint64_t arena_cap = 0, n_lines = 0;
  int64_t* block_sum = nullptr;
  int64_t* dir = nullptr;
  uint32_t* blk_count = nullptr;
  uint32_t* blk_first = nullptr;
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  DepthCarry* carry = nullptr;          // two that alternate, and a scratch one for the timed pass
  unsigned long long* status = nullptr;  // [1]: scratch
  uint32_t* n_heads = nullptr;           // [1]: scratch
  DepthHead* heads = nullptr;
  uint32_t heads_cap = 0;
  TextStream ts;                // its last chunk stays on the device (magot_depth_time)
  std::vector<DepthHead> runs;  // in file order
};

namespace {

constexpr uint64_t kDepthMaxLines = 0x7fffffffull;

DepthParseArgs depth_args(const magot_depth* t, int slot, uint64_t n, uint64_t off, int in,
                          int out, bool scratch) {
  DepthParseArgs a{};
  a.text = t->ts.dev[slot];
  a.n = (int64_t)n;
  a.file_off = off;
  a.blk_first = t->blk_first;
  a.in = t->carry + in;
  a.out = t->carry + out;
  a.arena = t->arena;
  a.arena_cap = t->arena_cap;
  a.heads = t->heads;
  a.n_heads = t->n_heads + (scratch ? 1 : 0);
  a.heads_cap = scratch ? 0u : t->heads_cap;
  a.status = t->status + (scratch ? 1 : 0);
  return a;
}

}  // namespace

extern "C" {

void magot_depth_destroy(magot_depth* t) {
  if (!t) return;
  if (t->ctx) (void)hipSetDevice(t->ctx->device);
  t->ts.close();
  if (t->arena_mem) (void)hipFree(t->arena_mem);
  delete t;
}

uint32_t magot_depth_block(void) { return (uint32_t)kDepthBlock; }

int magot_depth_parse(magot_ctx* ctx, const char* text, uint64_t len, uint64_t chunk_bytes,
                      uint32_t max_runs, magot_depth** out, uint64_t* n_lines, uint64_t* n_runs,
                      uint32_t* reason, uint64_t* line) {
  if (int rc = bind(ctx)) return rc;
  if (!out || !reason || !line || (len && !text)) {
    set_error("magot_depth_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  *reason = 0;
  *line = 0;
  if (n_lines) *n_lines = 0;
  if (n_runs) *n_runs = 0;
  Building<magot_depth, magot_depth_destroy> guard{new magot_depth()};
  magot_depth* t = guard.p;
  t->ctx = ctx;
  const uint64_t chunk = text_chunk_bytes(chunk_bytes, len);
  // a line of the grammar has at least 6 bytes ("a 1 0" and its LF)
  t->arena_cap = (depth_blocks(len / 6 + 2) + 1) * kDepthBlock;
  t->heads_cap = max_runs ? max_runs : (1u << 20);
  const uint64_t text_blocks = depth_text_blocks(chunk);
  t->scan_bytes = depth_scan_bytes(std::max(text_blocks, depth_blocks(t->arena_cap)) + 1);
  Carve cv;
  uint8_t* small;  // three carries, two status words, two head counters
  cv.take(&t->arena, t->arena_cap);
  cv.take(&t->block_sum, depth_blocks(t->arena_cap) + 1);
  cv.take(&t->dir, depth_blocks(t->arena_cap) + 1);
  cv.take(&t->blk_count, text_blocks + 1);
  cv.take(&t->blk_first, text_blocks + 1);
  cv.take(&t->scan_tmp, t->scan_bytes);
  cv.take(&t->heads, t->heads_cap);
  cv.take(&small, 3 * sizeof(DepthCarry) + 64);
  MAGOT_HIP_TRY(hipMalloc(&t->arena_mem, cv.used + 256));
  cv.place(t->arena_mem);
  t->carry = reinterpret_cast<DepthCarry*>(small);
  t->status = reinterpret_cast<unsigned long long*>(small + 3 * sizeof(DepthCarry));
  t->n_heads = reinterpret_cast<uint32_t*>(t->status + 2);
  // the carries and the head counters zero, the status words all ones
  MAGOT_HIP_TRY(hipMemsetAsync(t->carry, 0, 3 * sizeof(DepthCarry) + 64, ctx->stream));
  MAGOT_HIP_TRY(hipMemsetAsync(t->status, 0xff, 16, ctx->stream));
  if (int rc = t->ts.open(chunk, len > chunk ? 2 : 1)) return rc;
  // the zeroing above is on the context stream; the first upload is not
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));

  uint64_t off = 0, k = 0;
  bool line_long = false;
  while (off < len) {
    uint64_t end = std::min(off + chunk, len);
    if (end < len) {  // cut after the window's last LF
      const void* lf = memrchr(text + off, '\n', end - off);
      if (!lf) {
        line_long = true;
        break;
      }
      end = (uint64_t)(static_cast<const char*>(lf) - text) + 1;
    }
    const int s = (int)(k & 1);
    const uint64_t n = end - off;
    if (int rc = t->ts.push(ctx, text + off, n, off, k)) return rc;
    MAGOT_HIP_TRY(launch_depth_line_index(t->ts.dev[s], n, t->blk_count, t->blk_first,
                                          t->scan_tmp, t->scan_bytes, ctx->stream));
    MAGOT_HIP_TRY(launch_depth_parse(depth_args(t, s, n, off, (int)(k & 1), (int)((k + 1) & 1),
                                                false), ctx->stream));
    if (int rc = t->ts.passed(ctx, s)) return rc;
    off = end;
    ++k;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(t->ts.copy));
  t->ts.release_pinned();

  unsigned long long status = 0;
  uint32_t heads = 0;
  DepthCarry last;
  MAGOT_HIP_TRY(hipMemcpy(&status, t->status, 8, hipMemcpyDeviceToHost));
  MAGOT_HIP_TRY(hipMemcpy(&heads, t->n_heads, 4, hipMemcpyDeviceToHost));
  MAGOT_HIP_TRY(hipMemcpy(&last, t->carry + (k & 1), sizeof(last), hipMemcpyDeviceToHost));
  // the first offending line, whichever check finds it
  uint64_t bad_line = ~0ull;
  uint32_t bad = 0;
  first_offence(status, &bad, &bad_line);
  if (line_long && last.lines < bad_line) {
    bad_line = last.lines;
    bad = MAGOT_DEPTH_LINE_LONG;
  }
  if (heads <= t->heads_cap) {
    t->runs.resize(heads);
    if (heads)
      MAGOT_HIP_TRY(hipMemcpy(t->runs.data(), t->heads, heads * sizeof(DepthHead),
                              hipMemcpyDeviceToHost));
    std::sort(t->runs.begin(), t->runs.end(),
              [](const DepthHead& a, const DepthHead& b) { return a.line < b.line; });
    std::unordered_set<std::string> seen;
    for (const DepthHead& h : t->runs) {
      if (h.line >= bad_line) break;
      if (h.offset + h.name_len > len) {
        set_error("magot_depth_parse: a run head outside the text");
        return MAGOT_ERR_STATE;
      }
      if (!seen.emplace(text + h.offset, h.name_len).second) {
        bad_line = h.line;
        bad = MAGOT_DEPTH_REPEATED_CONTIG;
        break;
      }
    }
  }
  if (bad) {
    *reason = bad;
    *line = bad_line + 1;
    return MAGOT_OK;
  }
  if (last.lines > kDepthMaxLines || heads > t->heads_cap) {
    *reason = last.lines > kDepthMaxLines ? MAGOT_DEPTH_TOO_MANY_LINES : MAGOT_DEPTH_TOO_MANY_RUNS;
    return MAGOT_OK;
  }
  t->n_lines = last.lines;
  if (t->n_lines > t->arena_cap) {
    set_error("magot_depth_parse: more lines than the arena holds");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(launch_depth_directory(t->arena, t->n_lines, t->block_sum, t->dir, t->scan_tmp,
                                       t->scan_bytes, ctx->stream));
  if (n_lines) *n_lines = t->n_lines;
  if (n_runs) *n_runs = t->runs.size();
  *out = guard.release();
  return MAGOT_OK;
}

int magot_depth_runs(const magot_depth* t, uint64_t* first, uint64_t* offset, uint32_t* name_len,
                     uint64_t cap) {
  if (!t || cap < t->runs.size() || (t->runs.size() && (!first || !offset || !name_len))) {
    set_error("magot_depth_runs: null argument, or output buffers too small");
    return MAGOT_ERR_ARG;
  }
  for (size_t i = 0; i < t->runs.size(); ++i) {
    first[i] = t->runs[i].line;
    offset[i] = t->runs[i].offset;
    name_len[i] = t->runs[i].name_len;
  }
  return MAGOT_OK;
}

int magot_depth_values(magot_ctx* ctx, magot_depth* t, uint64_t start, uint64_t n, int32_t* out) {
  if (int rc = handle_of(ctx, t, "magot_depth_values", "track")) return rc;
  if (start > t->n_lines || n > t->n_lines - start || (n && !out)) {
    set_error("magot_depth_values: lines outside the table, or null output");
    return MAGOT_ERR_RANGE;
  }
  if (!n) return MAGOT_OK;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(out, t->arena + start, n * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_depth_sums(magot_ctx* ctx, magot_depth* t, const int64_t* start, const int64_t* length,
                     uint64_t n_rows, const uint64_t* group_offsets, uint64_t n_groups,
                     int64_t* sums, int64_t* group_sums) {
  if (int rc = handle_of(ctx, t, "magot_depth_sums", "track")) return rc;
  if (n_rows && (!start || !length)) {
    set_error("magot_depth_sums: null row table");
    return MAGOT_ERR_ARG;
  }
  if (!group_offsets) n_groups = 0;
  if (n_groups && !group_sums) {
    set_error("magot_depth_sums: null group output");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t i = 0; i < n_rows; ++i)
    if (length[i] > 0 && (start[i] < 0 || (uint64_t)start[i] > t->n_lines ||
                          (uint64_t)length[i] > t->n_lines - (uint64_t)start[i])) {
      set_error("magot_depth_sums: row " + std::to_string(i) + " is outside the table");
      return MAGOT_ERR_RANGE;
    }
  for (uint64_t g = 0; g < n_groups; ++g)
    if (group_offsets[g] > group_offsets[g + 1] || group_offsets[g + 1] > n_rows) {
      set_error("magot_depth_sums: group " + std::to_string(g) + " is not a range of rows");
      return MAGOT_ERR_ARG;
    }
  if (!n_rows && !n_groups) return MAGOT_OK;
  Carve cv;
  int64_t *d_start, *d_len, *d_sums, *d_group;
  uint64_t* d_off;
  cv.take(&d_start, n_rows);
  cv.take(&d_len, n_rows);
  cv.take(&d_sums, n_rows);
  cv.take(&d_off, n_groups + 1);
  cv.take(&d_group, n_groups);
  DevBuf d;
  MAGOT_HIP_TRY(hipMalloc(&d.p, cv.used + 256));
  cv.place(d.p);
  if (n_rows) {
    MAGOT_HIP_TRY(hipMemcpyAsync(d_start, start, n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
    MAGOT_HIP_TRY(hipMemcpyAsync(d_len, length, n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (n_groups)
    MAGOT_HIP_TRY(hipMemcpyAsync(d_off, group_offsets, (n_groups + 1) * 8, hipMemcpyHostToDevice,
                                 ctx->stream));
  MAGOT_HIP_TRY(launch_depth_sums(t->arena, t->dir, t->n_lines, d_start, d_len, n_rows, d_sums,
                                  ctx->stream));
  MAGOT_HIP_TRY(launch_depth_groups(d_sums, d_off, n_groups, d_group, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (n_rows && sums) MAGOT_HIP_TRY(hipMemcpy(sums, d_sums, n_rows * 8, hipMemcpyDeviceToHost));
  if (n_groups) MAGOT_HIP_TRY(hipMemcpy(group_sums, d_group, n_groups * 8, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_depth_time(magot_ctx* ctx, magot_depth* t, int iters, double* ms4,
                     uint64_t* chunk_len) {
  if (int rc = handle_of(ctx, t, "magot_depth_time", "track")) return rc;
  if (iters <= 0 || !ms4) {
    set_error("magot_depth_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  const TextStream& ts = t->ts;
  if (chunk_len) *chunk_len = ts.last_len;
  // one whole-run row per run for the sum pass
  const uint64_t nr = t->runs.size();
  std::vector<int64_t> rows(2 * nr);
  for (uint64_t i = 0; i < nr; ++i) {
    rows[i] = (int64_t)t->runs[i].line;
    rows[nr + i] = (int64_t)((i + 1 < nr ? t->runs[i + 1].line : t->n_lines) - t->runs[i].line);
  }
  DevBuf d;
  if (nr) {
    MAGOT_HIP_TRY(hipMalloc(&d.p, 3 * nr * 8));
    MAGOT_HIP_TRY(hipMemcpy(d.p, rows.data(), 2 * nr * 8, hipMemcpyHostToDevice));
  }
  int64_t* dr = static_cast<int64_t*>(d.p);
  return time_passes(
      ctx, iters, 4, ms4,
      [&](int k) {
        switch (k) {
          case 0:
            return launch_depth_line_index(ts.dev[ts.last_slot], ts.last_len, t->blk_count,
                                           t->blk_first, t->scan_tmp, t->scan_bytes, ctx->stream);
          case 1:  // the same depths into the same lines; heads, status and carry into scratch
            return launch_depth_parse(depth_args(t, ts.last_slot, ts.last_len, ts.last_off,
                                                 ts.last_in, 2, true), ctx->stream);
          case 2:
            return launch_depth_directory(t->arena, t->n_lines, t->block_sum, t->dir,
                                          t->scan_tmp, t->scan_bytes, ctx->stream);
          default:
            return launch_depth_sums(t->arena, t->dir, t->n_lines, dr, dr + nr, nr, dr + 2 * nr,
                                     ctx->stream);
        }
      },
      [&](int k) { return k < 2 && !ts.last_len; });  // an empty text left no chunk
}

}  // extern "C"

// ---------------------------------------------------------------------------
// fqstats' read-length histogram (fastq.hip; genome_tools.py:85-124)
// ---------------------------------------------------------------------------

struct magot_fq {
  magot_ctx* ctx = nullptr;
  void* mem = nullptr;  // everything but the text buffers
  unsigned long long* hist = nullptr;
  int64_t* longs = nullptr;    // as appended; sorted descending behind them
  uint64_t longs_cap = 0, n_longs = 0;
  FqBlock* blk = nullptr;
  FqBlock* pre = nullptr;
  FqItem* cum = nullptr;
  void* scan_tmp = nullptr;
  void* sort_tmp = nullptr;
  size_t scan_bytes = 0, sort_bytes = 0;
  FqCarry* carry = nullptr;               // two that alternate, and a scratch one for the timed pass
  unsigned long long* cursor = nullptr;   // the list's
  uint64_t* out = nullptr;                // launch_fq_reduce's nine words; [9..17]: scratch
  TextStream ts;  // its last chunk stays on the device (magot_fq_time)
  uint64_t file_bytes = 0;
  uint64_t stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool fetched = false;  // the histogram below
  std::vector<int64_t> lengths;
  std::vector<uint64_t> counts;
};

namespace {

FqChunkArgs fq_args(const magot_fq* t, int slot, uint64_t n, uint64_t off, int in, int out) {
  FqChunkArgs a{};
  a.text = t->ts.dev[slot];
  a.n = (int64_t)n;
  a.file_off = (int64_t)off;
  a.blk = t->blk;
  a.pre = t->pre;
  a.in = t->carry + in;
  a.out = t->carry + out;
  a.hist = t->hist;
  a.longs = t->longs;
  a.n_longs = t->cursor;
  a.longs_cap = t->longs_cap;
  return a;
}

}  // namespace

extern "C" {

void magot_fq_destroy(magot_fq* t) {
  if (!t) return;
  if (t->ctx) (void)hipSetDevice(t->ctx->device);
  t->ts.close();
  if (t->mem) (void)hipFree(t->mem);
  delete t;
}

uint64_t magot_fq_dense(void) { return kFqDense; }

int magot_fq_parse(magot_ctx* ctx, const char* text, uint64_t len, uint64_t chunk_bytes,
                   magot_fq** out) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text)) {
    set_error("magot_fq_parse: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  Building<magot_fq, magot_fq_destroy> guard{new magot_fq()};
  magot_fq* t = guard.p;
  t->ctx = ctx;
  t->file_bytes = len;
  const uint64_t chunk = text_chunk_bytes(chunk_bytes, len);
  t->longs_cap = fq_long_cap(len);
  const uint64_t text_blocks = depth_text_blocks(chunk);
  t->scan_bytes = fq_scan_bytes(text_blocks + 1, t->longs_cap + kFqDense);
  t->sort_bytes = fq_sort_bytes(t->longs_cap);
  Carve cv;
  uint8_t* small_block;
  cv.take(&t->hist, kFqDense);
  cv.take(&t->longs, 2 * t->longs_cap);
  cv.take(&t->blk, text_blocks + 1);
  cv.take(&t->pre, text_blocks + 1);
  cv.take(&t->cum, t->longs_cap + kFqDense);
  cv.take(&t->scan_tmp, t->scan_bytes);
  cv.take(&t->sort_tmp, t->sort_bytes);
  cv.take(&small_block, 256);
  MAGOT_HIP_TRY(hipMalloc(&t->mem, cv.used + 256));
  cv.place(t->mem);
  // 256 bytes: three carries, the list's cursor, the nine result words twice
  static_assert(3 * sizeof(FqCarry) + 8 + 18 * 8 <= 256, "the small block");
  t->carry = reinterpret_cast<FqCarry*>(small_block);
  t->cursor = reinterpret_cast<unsigned long long*>(small_block + 3 * sizeof(FqCarry));
  t->out = reinterpret_cast<uint64_t*>(t->cursor + 1);
  struct {
    FqCarry carry[3];
    uint64_t words[19];
  } small{};
  for (FqCarry& c : small.carry) c.last_lf = -1;  // no LF yet
  MAGOT_HIP_TRY(hipMemsetAsync(t->hist, 0, kFqDense * 8, ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(t->carry, &small, sizeof(small), hipMemcpyHostToDevice));
  if (int rc = t->ts.open(chunk, len > chunk ? 2 : 1)) return rc;
  // the zeroing above is on the context stream; the first upload is not
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));

  uint64_t off = 0, k = 0;
  while (off < len) {  // cut wherever the chunk ends
    const uint64_t n = std::min(chunk, len - off);
    const int s = (int)(k & 1);
    if (int rc = t->ts.push(ctx, text + off, n, off, k)) return rc;
    const FqChunkArgs a = fq_args(t, s, n, off, (int)(k & 1), (int)((k + 1) & 1));
    MAGOT_HIP_TRY(launch_fq_line_index(a, t->scan_tmp, t->scan_bytes, ctx->stream));
    MAGOT_HIP_TRY(launch_fq_lengths(a, fq_grid(n, ctx->n_cu), ctx->stream));
    if (int rc = t->ts.passed(ctx, s)) return rc;
    off += n;
    ++k;
  }
  // a last line without its LF, from the carry the last chunk left
  MAGOT_HIP_TRY(launch_fq_tail(fq_args(t, 0, 0, len, (int)(k & 1), 2), len, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(t->ts.copy));
  t->ts.release_pinned();

  unsigned long long n_longs = 0;
  MAGOT_HIP_TRY(hipMemcpy(&n_longs, t->cursor, 8, hipMemcpyDeviceToHost));
  if (n_longs > t->longs_cap) {
    set_error("magot_fq_parse: more long lines than the text has room for");
    return MAGOT_ERR_STATE;
  }
  t->n_longs = n_longs;
  FqReduceArgs r{};
  r.hist = t->hist;
  r.longs = t->longs + t->longs_cap;
  r.n_longs = t->n_longs;
  r.cum = t->cum;
  r.out = t->out;
  MAGOT_HIP_TRY(launch_fq_sort(t->longs, t->longs + t->longs_cap, t->n_longs, t->sort_tmp,
                               t->sort_bytes, ctx->stream));
  MAGOT_HIP_TRY(launch_fq_reduce(r, t->scan_tmp, t->scan_bytes, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(t->stats, t->out, sizeof(t->stats), hipMemcpyDeviceToHost));
  *out = guard.release();
  return MAGOT_OK;
}

int magot_fq_stats(const magot_fq* t, uint64_t* out8, uint32_t* flags) {
  if (!t || !out8 || !flags) {
    set_error("magot_fq_stats: null argument");
    return MAGOT_ERR_ARG;
  }
  for (int k = 0; k < 8; ++k) out8[k] = t->stats[k];
  *flags = (uint32_t)t->stats[8];
  return MAGOT_OK;
}

int magot_fq_histogram(magot_ctx* ctx, magot_fq* t, int64_t* lengths, uint64_t* counts,
                       uint64_t cap, uint64_t* n) {
  if (int rc = handle_of(ctx, t, "magot_fq_histogram", "handle")) return rc;
  if (!n) {
    set_error("magot_fq_histogram: null argument");
    return MAGOT_ERR_ARG;
  }
  if (!t->fetched) {
    std::vector<unsigned long long> hist(kFqDense);
    std::vector<int64_t> longs(t->n_longs);
    MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
    MAGOT_HIP_TRY(hipMemcpy(hist.data(), t->hist, kFqDense * 8, hipMemcpyDeviceToHost));
    if (t->n_longs)
      MAGOT_HIP_TRY(hipMemcpy(longs.data(), t->longs + t->longs_cap, t->n_longs * 8,
                              hipMemcpyDeviceToHost));
    for (uint64_t b = 0; b < kFqDense; ++b)
      if (hist[b]) {
        t->lengths.push_back((int64_t)b);
        t->counts.push_back(hist[b]);
      }
    for (uint64_t i = t->n_longs; i-- > 0;) {  // descending on the device
      if (!t->lengths.empty() && t->lengths.back() == longs[i]) {
        ++t->counts.back();
      } else {
        t->lengths.push_back(longs[i]);
        t->counts.push_back(1);
      }
    }
    t->fetched = true;
  }
  *n = t->lengths.size();
  if (!lengths && !counts) return MAGOT_OK;  // the size alone
  if (!lengths || !counts || cap < t->lengths.size()) {
    set_error("magot_fq_histogram: null output, or output buffers too small");
    return MAGOT_ERR_ARG;
  }
  std::copy(t->lengths.begin(), t->lengths.end(), lengths);
  std::copy(t->counts.begin(), t->counts.end(), counts);
  return MAGOT_OK;
}

int magot_fq_time(magot_ctx* ctx, magot_fq* t, int iters, double* ms4, uint64_t* chunk_len) {
  if (int rc = handle_of(ctx, t, "magot_fq_time", "handle")) return rc;
  if (iters <= 0 || !ms4) {
    set_error("magot_fq_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  const TextStream& ts = t->ts;
  if (chunk_len) *chunk_len = ts.last_len;
  // a histogram, a list and a cursor of their own for the timed length pass,
  // and the copy's target
  FqChunkArgs a = fq_args(t, ts.last_slot, ts.last_len, ts.last_off, ts.last_in, 2);
  Carve cv;
  uint8_t* copy;
  cv.take(&a.hist, kFqDense);
  cv.take(&a.longs, t->longs_cap);
  cv.take(&a.n_longs, 1);
  const uint64_t o_copy = cv.take(&copy, ts.last_len);
  DevBuf d;
  MAGOT_HIP_TRY(hipMalloc(&d.p, cv.used + 256));
  cv.place(d.p);
  MAGOT_HIP_TRY(hipMemsetAsync(d.p, 0, o_copy, ctx->stream));  // all but the copy's target
  FqReduceArgs r{};
  r.hist = t->hist;
  r.longs = t->longs + t->longs_cap;
  r.n_longs = t->n_longs;
  r.cum = t->cum;
  r.out = t->out + 9;
  double total[4] = {0, 0, 0, 0};
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < 4; ++k) {
      if (k != 2 && !ts.last_len) continue;
      if (k == 2) MAGOT_HIP_TRY(hipMemsetAsync(r.out, 0, 9 * 8, ctx->stream));
      if (int rc = time_pass(ctx, &total[k], [&] {
            switch (k) {
              case 0:
                return launch_fq_line_index(a, t->scan_tmp, t->scan_bytes, ctx->stream);
              case 1:
                return launch_fq_lengths(a, fq_grid(ts.last_len, ctx->n_cu), ctx->stream);
              case 2:
                if (hipError_t e = launch_fq_sort(t->longs, t->longs + t->longs_cap, t->n_longs,
                                                  t->sort_tmp, t->sort_bytes, ctx->stream))
                  return e;
                return launch_fq_reduce(r, t->scan_tmp, t->scan_bytes, ctx->stream);
              default:
                return hipMemcpyAsync(copy, ts.dev[ts.last_slot], ts.last_len,
                                      hipMemcpyDeviceToDevice, ctx->stream);
            }
          }))
        return rc;
    }
  for (int k = 0; k < 4; ++k) ms4[k] = total[k] / iters;
  return MAGOT_OK;
}

}  // extern "C"
