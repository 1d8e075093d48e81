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

}  // extern "C"
