// C ABI: interval joins on the device (overlap.hip; genome_tools.py:548-568,
// annotation_funcs.py:13-30).  The planner's entry points are in
// overlapplan.cpp.
#include "abi_internal.h"

using namespace magot;

struct magot_overlap {
  magot_ctx* ctx = nullptr;
  void* arena = nullptr;
  OvBuildArgs b{};
  OvIndex ix{};
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0;
  // the last query set, kept for magot_overlap_time
  void* qmem = nullptr;
  uint64_t qcap = 0;
  OvQuery q{};
  uint8_t* drop = nullptr;
  int64_t* counts = nullptr;
  uint32_t* long_list = nullptr;
  unsigned long long* n_long = nullptr;
};

namespace {

bool coords_in_range(const int64_t* a, const int64_t* b, uint64_t n) {
  bool ok = true;
  for (uint64_t i = 0; i < n; ++i)
    ok &= a[i] >= kOvCoordMin && a[i] <= kOvCoordMax && b[i] >= kOvCoordMin && b[i] <= kOvCoordMax;
  return ok;
}

hipError_t build(const magot_overlap* h, hipStream_t s) {
  if (hipError_t e = launch_ov_keys(h->b, s)) return e;
  if (hipError_t e = launch_ov_sort(h->b, h->sort_tmp, h->sort_bytes, s)) return e;
  return launch_ov_segments(h->b, s);
}

// The query set on the device, in the handle's slot (grown when too small).
int upload_query(magot_ctx* ctx, magot_overlap* h, const char* who, const uint32_t* seq,
                 const int64_t* c0, const int64_t* c1, uint64_t n) {
  if (n && (!seq || !c0 || !c1)) {
    set_error(std::string(who) + ": null argument");
    return MAGOT_ERR_ARG;
  }
  if (n >= (1ull << 32)) {
    set_error(std::string(who) + ": 2^32 queries or more in one call");
    return MAGOT_ERR_ARG;
  }
  if (!coords_in_range(c0, c1, n)) {
    set_error(std::string(who) + ": a coordinate outside [-2^39, 2^39)");
    return MAGOT_ERR_RANGE;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (n > h->qcap || !h->qmem) {
    if (h->qmem) MAGOT_HIP_TRY(hipFree(h->qmem));
    h->qmem = nullptr;
    h->qcap = 0;
    h->q = OvQuery{};
    const uint64_t cap = std::max<uint64_t>(n, 1);
    Carve cv;
    cv.take(&h->q.seq, cap);
    cv.take(&h->q.c0, cap);
    cv.take(&h->q.c1, cap);
    cv.take(&h->drop, cap);
    cv.take(&h->counts, cap);
    cv.take(&h->long_list, cap);
    cv.take(&h->n_long, 1);
    MAGOT_HIP_TRY(hipMalloc(&h->qmem, cv.used));
    cv.place(h->qmem);
    h->qcap = cap;
  }
  h->q.n = n;
  if (n) {
    MAGOT_HIP_TRY(hipMemcpy(const_cast<uint32_t*>(h->q.seq), seq, n * 4, hipMemcpyHostToDevice));
    MAGOT_HIP_TRY(hipMemcpy(const_cast<int64_t*>(h->q.c0), c0, n * 8, hipMemcpyHostToDevice));
    MAGOT_HIP_TRY(hipMemcpy(const_cast<int64_t*>(h->q.c1), c1, n * 8, hipMemcpyHostToDevice));
  }
  return MAGOT_OK;
}

}  // namespace

extern "C" {

uint32_t magot_overlap_lane_scan(void) { return kOvLaneScan; }

void magot_overlap_coord_range(int64_t* lo, int64_t* hi) {
  if (lo) *lo = kOvCoordMin;
  if (hi) *hi = kOvCoordMax;
}

void magot_overlap_destroy(magot_overlap* h) {
  if (!h) return;
  if (h->ctx) (void)hipSetDevice(h->ctx->device);
  if (h->qmem) (void)hipFree(h->qmem);
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

int magot_overlap_create(magot_ctx* ctx, const uint32_t* seq, const int64_t* p0, const int64_t* p1,
                         uint64_t n, uint32_t n_seq, magot_overlap** out) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (n && (!seq || !p0 || !p1))) {
    set_error("magot_overlap_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (n_seq > kOvMaxSeq || n >= (1ull << 40)) {
    set_error("magot_overlap_create: more seqids or intervals than the index holds");
    return MAGOT_ERR_ARG;
  }
  bool known = true;
  for (uint64_t i = 0; i < n; ++i) known &= seq[i] < n_seq;
  if (!known) {
    set_error("magot_overlap_create: a seqid not below n_seq");
    return MAGOT_ERR_ARG;
  }
  if (!coords_in_range(p0, p1, n)) {
    set_error("magot_overlap_create: a coordinate outside [-2^39, 2^39)");
    return MAGOT_ERR_RANGE;
  }
  Building<magot_overlap, magot_overlap_destroy> guard{new magot_overlap()};
  magot_overlap* h = guard.p;
  h->ctx = ctx;
  h->sort_bytes = ov_sort_bytes(n);
  const uint64_t segs = (uint64_t)n_seq + 1;
  OvBuildArgs& b = h->b;
  b.n = n;
  b.n_seq = n_seq;
  Carve cv;
  uint32_t* d_seq;  // uploaded into; the kernels read them as const
  int64_t *d_p0, *d_p1;
  cv.take(&d_seq, n);
  cv.take(&d_p0, n);
  cv.take(&d_p1, n);
  cv.take(&b.raw, 5 * n);
  cv.take(&b.raw_v, n);
  cv.take(&b.in_s, 5 * n);  // and in_e, all_s, cl_s, cl_e
  cv.take(&b.cl_v, n);
  cv.take(&b.seg_in, 3 * segs);  // and seg_all, seg_cl
  cv.take(&h->sort_tmp, h->sort_bytes);
  MAGOT_HIP_TRY(hipMalloc(&h->arena, cv.used + 256));
  cv.place(h->arena);
  if (n) {
    MAGOT_HIP_TRY(hipMemcpy(d_seq, seq, n * 4, hipMemcpyHostToDevice));
    MAGOT_HIP_TRY(hipMemcpy(d_p0, p0, n * 8, hipMemcpyHostToDevice));
    MAGOT_HIP_TRY(hipMemcpy(d_p1, p1, n * 8, hipMemcpyHostToDevice));
  }
  b.seq = d_seq;
  b.p0 = d_p0;
  b.p1 = d_p1;
  b.in_e = b.in_s + n;
  b.all_s = b.in_s + 2 * n;
  b.cl_s = b.in_s + 3 * n;
  b.cl_e = b.in_s + 4 * n;
  b.seg_all = b.seg_in + segs;
  b.seg_cl = b.seg_in + 2 * segs;
  h->ix = OvIndex{n, n_seq, b.in_s, b.in_e, b.all_s, b.cl_s, b.cl_e, b.cl_v,
                  b.seg_in, b.seg_all, b.seg_cl};
  MAGOT_HIP_TRY(build(h, ctx->stream));
  *out = guard.release();
  return MAGOT_OK;
}

int magot_overlap_purge(magot_ctx* ctx, magot_overlap* h, const uint32_t* seq, const int64_t* c0,
                        const int64_t* c1, uint64_t n, uint8_t* drop) {
  if (int rc = handle_of(ctx, h, "magot_overlap_purge", "index")) return rc;
  if (n && !drop) {
    set_error("magot_overlap_purge: null output");
    return MAGOT_ERR_ARG;
  }
  if (int rc = upload_query(ctx, h, "magot_overlap_purge", seq, c0, c1, n)) return rc;
  MAGOT_HIP_TRY(launch_ov_purge(h->ix, h->q, h->drop, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (n) MAGOT_HIP_TRY(hipMemcpy(drop, h->drop, n, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_overlap_counts(magot_ctx* ctx, magot_overlap* h, const uint32_t* seq, const int64_t* q0,
                         const int64_t* q1, uint64_t n, int64_t* counts) {
  if (int rc = handle_of(ctx, h, "magot_overlap_counts", "index")) return rc;
  if (n && !counts) {
    set_error("magot_overlap_counts: null output");
    return MAGOT_ERR_ARG;
  }
  if (int rc = upload_query(ctx, h, "magot_overlap_counts", seq, q0, q1, n)) return rc;
  MAGOT_HIP_TRY(launch_ov_overlap(h->ix, h->q, h->counts, h->long_list, h->n_long, ctx->n_cu,
                                  ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (n) MAGOT_HIP_TRY(hipMemcpy(counts, h->counts, n * 8, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_overlap_time(magot_ctx* ctx, magot_overlap* h, int iters, double* ms,
                       uint64_t* copy_bytes) {
  if (int rc = handle_of(ctx, h, "magot_overlap_time", "index")) return rc;
  if (iters <= 0 || !ms) {
    set_error("magot_overlap_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  // the yardstick: the six sorted tables copied once, device to device, over
  // the unsorted keys (the keys pass writes them again)
  const uint64_t bytes = h->b.n * 8 * 5;
  if (copy_bytes) *copy_bytes = bytes + h->b.n * 8;
  hipStream_t s = ctx->stream;
  return time_passes(
      ctx, iters, 6, ms,
      [&](int k) -> hipError_t {
        switch (k) {
          case 0: return launch_ov_keys(h->b, s);
          case 1: return launch_ov_sort(h->b, h->sort_tmp, h->sort_bytes, s);
          case 2: return launch_ov_segments(h->b, s);
          case 3: return launch_ov_purge(h->ix, h->q, h->drop, s);
          case 4:
            return launch_ov_overlap(h->ix, h->q, h->counts, h->long_list, h->n_long, ctx->n_cu,
                                     s);
          default:
            if (!bytes) return hipSuccess;
            if (hipError_t e = hipMemcpyAsync(h->b.raw, h->b.in_s, bytes, hipMemcpyDeviceToDevice, s))
              return e;
            return hipMemcpyAsync(h->b.raw_v, h->b.cl_v, h->b.n * 8, hipMemcpyDeviceToDevice, s);
        }
      },
      [&](int k) { return k >= 3 && k <= 4 && !h->q.n; });  // no query set was given yet
}

}  // extern "C"
