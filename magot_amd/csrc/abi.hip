// C ABI of libmagot.so (declarations and contracts: include/magot.h): errors,
// devices and contexts.  The features are in the abi_*.hip units.
#include "abi_internal.h"

namespace magot {

namespace {
thread_local std::string g_last_error;
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
  const uint64_t o_text = cv.take<uint8_t>(len + kTextPad);
  uint64_t o_blk[4];  // blk, pre, blk2, pre2
  for (uint64_t& o : o_blk) o = cv.take<uint64_t>(ix.n_blocks + 1);
  const uint64_t o_tmp = cv.take<uint8_t>(tmp_bytes);
  // at most one occurrence per byte; room for every byte a lane loads, so that an
  // index that counted behind the text's end would be a wrong answer, not a wild store
  const uint64_t o_pos = cv.take<uint64_t>(len + kTextPad);
  DevBuf buf;
  MAGOT_HIP_TRY(hipMalloc(&buf.p, cv.used + 256));
  char* base = static_cast<char*>(buf.p);
  ix.text = reinterpret_cast<const uint8_t*>(base + o_text);
  ix.blk = reinterpret_cast<uint64_t*>(base + o_blk[0]);
  ix.pre = reinterpret_cast<uint64_t*>(base + o_blk[1]);
  ix.blk2 = reinterpret_cast<uint64_t*>(base + o_blk[2]);
  ix.pre2 = reinterpret_cast<uint64_t*>(base + o_blk[3]);
  ix.pos = reinterpret_cast<uint64_t*>(base + o_pos);
  if (len) MAGOT_HIP_TRY(hipMemcpyAsync(base + o_text, text, len, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(launch_text_count(ix, base + o_tmp, tmp_bytes, s));
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

}  // extern "C"
