// C ABI of libmagot.so (declarations and contracts: include/magot.h): errors,
// devices and contexts, and the debug entries of the routines the text tools
// share (textindex.hip, wavecopy.h).  The features are in the abi_*.hip units.
#include "abi_internal.h"
#include "wavecopy.h"

namespace magot {

namespace {
thread_local std::string g_last_error;

// the debug copies: the grouped copies count a group's chunks and bytes in 32
// bits (wavecopy.h)
constexpr uint64_t kDebugCopyMax = 1ull << 28;
// [at, at + len) lies in a buffer of `size` bytes
inline bool span_inside(uint64_t at, uint64_t len, uint64_t size) {
  return at <= size && len <= size - at;
}
// n bytes (or none) to and from the device on s
inline hipError_t to_device(void* dev, const void* host, uint64_t n, hipStream_t s) {
  return n ? hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, s) : hipSuccess;
}
inline hipError_t to_host(void* host, const void* dev, uint64_t n, hipStream_t s) {
  return n ? hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, s) : hipSuccess;
}
}

void set_error(const std::string& msg) { g_last_error = msg; }

void standard_lut(uint8_t out[64]) {
  // genome.py:795-802, walked in TCAG order (first, second, third base).
  static const char kAA[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
  static const int kTcagToCode[4] = {3, 1, 0, 2};  // T C A G -> A=0 C=1 G=2 T=3
  int n = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b)
      for (int c = 0; c < 4; ++c) {
        int x = kTcagToCode[a] + 4 * kTcagToCode[b] + 16 * kTcagToCode[c];
        out[x] = (uint8_t)kAA[n++];
      }
}

}  // namespace magot

using namespace magot;

extern "C" {

int magot_abi_version(void) { return MAGOT_ABI_VERSION; }

const char* magot_last_error(void) { return g_last_error.c_str(); }

int magot_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int magot_ctx_create(int device, magot_ctx** out) {
  if (!out) {
    set_error("magot_ctx_create: null out");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  int n = 0;
  MAGOT_HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) {
    set_error("magot_ctx_create: device " + std::to_string(device) + " out of range (" +
              std::to_string(n) + " visible)");
    return MAGOT_ERR_ARG;
  }
  std::unique_ptr<magot_ctx> c(new magot_ctx());
  c->device = device;
  MAGOT_HIP_TRY(hipSetDevice(device));
  MAGOT_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  MAGOT_HIP_TRY(hipEventCreate(&c->ev0));
  MAGOT_HIP_TRY(hipEventCreate(&c->ev1));
  MAGOT_HIP_TRY(hipEventCreate(&c->mark0));
  MAGOT_HIP_TRY(hipEventCreate(&c->mark1));
  MAGOT_HIP_TRY(hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
  c->blocks_per_cu = extract_blocks_per_cu();
  *out = c.release();
  return MAGOT_OK;
}

void magot_ctx_destroy(magot_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->mark0) (void)hipEventDestroy(ctx->mark0);
  if (ctx->mark1) (void)hipEventDestroy(ctx->mark1);
  for (int k = 0; k < 2; ++k) {
    if (ctx->pin_ev[k]) (void)hipEventDestroy(ctx->pin_ev[k]);
    if (ctx->pin[k]) (void)hipHostFree(ctx->pin[k]);
  }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int magot_ctx_info(const magot_ctx* ctx, int* n_cu, int* extract_blocks_per_cu) {
  if (!ctx) {
    set_error("magot_ctx_info: null context");
    return MAGOT_ERR_ARG;
  }
  if (n_cu) *n_cu = ctx->n_cu;
  if (extract_blocks_per_cu) *extract_blocks_per_cu = ctx->blocks_per_cu;
  return MAGOT_OK;
}

int magot_ctx_sync(magot_ctx* ctx) {
  if (int rc = bind(ctx)) return rc;
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

int magot_ctx_mark(magot_ctx* ctx, int which) {
  if (int rc = bind(ctx)) return rc;
  if (which != 0 && which != 1) {
    set_error("magot_ctx_mark: which must be 0 or 1");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipEventRecord(which ? ctx->mark1 : ctx->mark0, ctx->stream));
  return MAGOT_OK;
}

int magot_ctx_elapsed(magot_ctx* ctx, double* ms) {
  if (int rc = bind(ctx)) return rc;
  if (!ms) {
    set_error("magot_ctx_elapsed: null argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipEventSynchronize(ctx->mark1));
  float f = 0.f;
  MAGOT_HIP_TRY(hipEventElapsedTime(&f, ctx->mark0, ctx->mark1));
  *ms = f;
  return MAGOT_OK;
}

// The byte index of the resident-text tools on its own (textindex.hip, plain
// mode): the tests' direct view of its tail mask and block sums.
int magot_debug_text_index(magot_ctx* ctx, const uint8_t* text, uint64_t len, uint64_t index_len,
                           uint32_t byte, int32_t second_byte, uint64_t* pos_out, uint64_t* n_out,
                           uint64_t* second_count_out) {
  if (int rc = bind(ctx)) return rc;
  if (!n_out || (len && !text) || index_len > len || byte > 255 || second_byte < -1 ||
      second_byte > 255) {
    set_error("magot_debug_text_index: bad argument");
    return MAGOT_ERR_ARG;
  }
  hipStream_t s = ctx->stream;
  const bool second = second_byte >= 0;
  TextIndexArgs ix{};
  ix.n = index_len;
  ix.n_blocks = depth_text_blocks(index_len);
  ix.byte = byte;
  ix.byte2 = second ? (uint32_t)second_byte : kTextNoByte;
  const size_t tmp_bytes = exclusive_sum_bytes<uint64_t>(ix.n_blocks + 1);
  Carve cv;
  uint8_t* d_text;  // uploaded into; the index reads it as const
  void* tmp;
  cv.take(&d_text, len + kTextPad);
  for (uint64_t** f : {&ix.blk, &ix.pre, &ix.blk2, &ix.pre2}) cv.take(f, ix.n_blocks + 1);
  cv.take(&tmp, tmp_bytes);
  // at most one occurrence per byte; room for every byte a lane loads, so that an
  // index that counted behind the text's end would be a wrong answer, not a wild store
  cv.take(&ix.pos, len + kTextPad);
  DevBuf buf;
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  cv.place(buf.p);
  ix.text = d_text;
  if (len) MAGOT_HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(launch_text_count(ix, tmp, tmp_bytes, s));
  MAGOT_HIP_TRY(launch_text_fill(ix, kTextFillPlain, s));
  uint64_t total = 0, total2 = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(&total, ix.pre + ix.n_blocks, 8, hipMemcpyDeviceToHost, s));
  if (second)
    MAGOT_HIP_TRY(hipMemcpyAsync(&total2, ix.pre2 + ix.n_blocks, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (total > index_len) {
    set_error("magot_debug_text_index: more occurrences than bytes");
    return MAGOT_ERR_STATE;
  }
  if (pos_out && total)
    MAGOT_HIP_TRY(hipMemcpy(pos_out, ix.pos, total * 8, hipMemcpyDeviceToHost));
  *n_out = total;
  if (second_count_out) *second_count_out = total2;
  return MAGOT_OK;
}

// The same index in line mode, the way resident_text_open and the four tools
// run it: the LF count, n_lines from it and the text's last byte, the status
// word preset to all ones, then the fill (with the stray-CR check or without).
int magot_debug_text_lines(magot_ctx* ctx, const uint8_t* text, uint64_t len, uint64_t index_len,
                           int check_cr, uint32_t stray_reason, uint64_t* pos_out,
                           uint64_t* n_lines_out, uint64_t* stray_out) {
  if (int rc = bind(ctx)) return rc;
  if (!n_lines_out || (len && !text) || index_len > len || stray_reason > 255) {
    set_error("magot_debug_text_lines: bad argument");
    return MAGOT_ERR_ARG;
  }
  hipStream_t s = ctx->stream;
  TextIndexArgs ix{};
  ix.n = index_len;
  ix.n_blocks = depth_text_blocks(index_len);
  ix.byte = '\n';
  ix.byte2 = kTextNoByte;
  ix.stray_reason = stray_reason;
  const size_t tmp_bytes = exclusive_sum_bytes<uint64_t>(ix.n_blocks + 1);
  Carve cv;
  uint8_t* d_text;  // uploaded into; the index reads it as const
  void* tmp;
  cv.take(&d_text, len + kTextPad);
  cv.take(&ix.blk, ix.n_blocks + 1);
  cv.take(&ix.pre, ix.n_blocks + 1);
  cv.take(&tmp, tmp_bytes);
  cv.take(&ix.stray_status, 1);
  // a line start per byte and the two end entries; room for every byte a lane loads
  cv.take(&ix.pos, len + kTextPad + 2);
  DevBuf buf;
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  cv.place(buf.p);
  ix.text = d_text;
  if (len) MAGOT_HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(hipMemsetAsync(ix.stray_status, 0xff, sizeof(unsigned long long), s));
  MAGOT_HIP_TRY(launch_text_count(ix, tmp, tmp_bytes, s));
  uint64_t total = 0;
  MAGOT_HIP_TRY(hipMemcpyAsync(&total, ix.pre + ix.n_blocks, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (total > index_len) {
    set_error("magot_debug_text_lines: more line feeds than bytes");
    return MAGOT_ERR_STATE;
  }
  ix.n_lines = total + (index_len && text[index_len - 1] != '\n' ? 1 : 0);
  unsigned long long status = ~0ull;
  if (ix.n_lines) {
    MAGOT_HIP_TRY(launch_text_fill(ix, check_cr ? kTextFillLinesCr : kTextFillLines, s));
    MAGOT_HIP_TRY(hipMemcpyAsync(&status, ix.stray_status, 8, hipMemcpyDeviceToHost, s));
    if (pos_out) MAGOT_HIP_TRY(to_host(pos_out, ix.pos, (ix.n_lines + 1) * 8, s));
    MAGOT_HIP_TRY(hipStreamSynchronize(s));
  }
  *n_lines_out = ix.n_lines;
  if (stray_out) *stray_out = status;
  return MAGOT_OK;
}

// wavecopy.h's grouped piece copy on its own, as fastarec.hip and rename.hip
// launch it (kFaGroup = kRnGroup = 16).
int magot_debug_piece_copy(magot_ctx* ctx, const uint8_t* base, uint64_t base_len,
                           const uint64_t* src, const uint64_t* dst, const uint32_t* len,
                           uint64_t n, uint8_t* out, uint64_t out_len) {
  if (int rc = bind(ctx)) return rc;
  if ((n && (!src || !dst || !len)) || (base_len && !base) || (out_len && !out) ||
      base_len >= kDebugCopyMax || out_len >= kDebugCopyMax) {
    set_error("magot_debug_piece_copy: bad argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (!span_inside(src[i], len[i], base_len) || !span_inside(dst[i], len[i], out_len)) {
      set_error("magot_debug_piece_copy: piece " + std::to_string(i) +
                " lies outside its buffer");
      return MAGOT_ERR_RANGE;
    }
  hipStream_t s = ctx->stream;
  Carve cv;
  uint8_t *d_base, *d_out;
  uint64_t *d_src, *d_dst;
  uint32_t* d_len;
  cv.take(&d_base, ((base_len + 15) & ~15ull) + kTextPad);
  cv.take(&d_out, out_len);
  cv.take(&d_src, n);
  cv.take(&d_dst, n);
  cv.take(&d_len, n);
  DevBuf buf;
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  cv.place(buf.p);
  MAGOT_HIP_TRY(to_device(d_base, base, base_len, s));
  MAGOT_HIP_TRY(to_device(d_out, out, out_len, s));
  MAGOT_HIP_TRY(to_device(d_src, src, n * 8, s));
  MAGOT_HIP_TRY(to_device(d_dst, dst, n * 8, s));
  MAGOT_HIP_TRY(to_device(d_len, len, n * 4, s));
  if (n) MAGOT_HIP_TRY(launch_piece_copy<16>(d_src, d_dst, d_len, n, d_base, d_out, s));
  MAGOT_HIP_TRY(to_host(out, d_out, out_len, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  return MAGOT_OK;
}

// render.hip's text assembly on its own, as magot_fasta_text_execute launches
// it: the unit lengths, their scan, the grouped span copy with text parts.
int magot_debug_text_assembly(magot_ctx* ctx, const magot_text_unit* units, uint64_t n,
                              const uint8_t* text, uint64_t text_len, const uint64_t* rspan,
                              uint64_t n_rec, const uint8_t* pay, uint64_t pay_len, int protein,
                              uint8_t* out, uint64_t out_len, uint64_t* written) {
  static_assert(sizeof(magot_text_unit) == sizeof(TextUnit) && MAGOT_NO_RECORD == kNoRecord,
                "magot_text_unit is TextUnit");
  if (int rc = bind(ctx)) return rc;
  if (!written || (n && !units) || (text_len && !text) || (n_rec && !rspan) ||
      (pay_len && !pay) || (out_len && !out) || n_rec >= kNoRecord ||
      text_len >= kDebugCopyMax || pay_len >= kDebugCopyMax || out_len >= kDebugCopyMax) {
    set_error("magot_debug_text_assembly: bad argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t r = 0; r < n_rec; ++r)
    if (rspan[2 * r] > rspan[2 * r + 1] || rspan[2 * r + 1] > pay_len) {
      set_error("magot_debug_text_assembly: record " + std::to_string(r) + " lies outside pay");
      return MAGOT_ERR_RANGE;
    }
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const magot_text_unit& u = units[i];
    if (!span_inside(u.text_off, u.text_len, text_len) ||
        (u.rec != MAGOT_NO_RECORD && u.rec >= n_rec)) {
      set_error("magot_debug_text_assembly: unit " + std::to_string(i) +
                " lies outside text, or names no record");
      return MAGOT_ERR_RANGE;
    }
    total += u.text_len;
    if (u.rec != MAGOT_NO_RECORD) {
      uint64_t a = rspan[2 * (uint64_t)u.rec];
      const uint64_t e = rspan[2 * (uint64_t)u.rec + 1];
      if (protein && e > a && pay[a] == 'X') ++a;  // unit_payload's rule (render.hip)
      total += e - a;
    }
    if (total > out_len) {
      set_error("magot_debug_text_assembly: the text is longer than out_len");
      return MAGOT_ERR_RANGE;
    }
  }
  hipStream_t s = ctx->stream;
  const size_t scan_bytes = text_scan_bytes(n);
  Carve cv;
  TextUnit* d_units;
  uint64_t *d_rspan, *d_len, *d_psrc, *d_end;
  uint8_t *d_text, *d_pay, *d_out;
  void* tmp;
  cv.take(&d_units, n);
  cv.take(&d_rspan, 2 * n_rec);
  cv.take(&d_text, ((text_len + 15) & ~15ull) + kTextPad);
  cv.take(&d_pay, ((pay_len + 15) & ~15ull) + kTextPad);
  cv.take(&d_len, n);
  cv.take(&d_psrc, n);
  cv.take(&d_end, n);
  cv.take(&tmp, scan_bytes);
  cv.take(&d_out, out_len);
  DevBuf buf;
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  cv.place(buf.p);
  MAGOT_HIP_TRY(to_device(d_units, units, n * sizeof(TextUnit), s));
  MAGOT_HIP_TRY(to_device(d_rspan, rspan, 2 * n_rec * 8, s));
  MAGOT_HIP_TRY(to_device(d_text, text, text_len, s));
  MAGOT_HIP_TRY(to_device(d_pay, pay, pay_len, s));
  MAGOT_HIP_TRY(to_device(d_out, out, out_len, s));
  launch_text_assembly(d_units, n, d_rspan, d_pay, protein, d_text, d_len, d_psrc, d_end, tmp,
                       scan_bytes, d_out, s);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(to_host(out, d_out, out_len, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  *written = total;
  return MAGOT_OK;
}

}  // extern "C"
