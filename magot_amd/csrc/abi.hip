// C ABI of libmagot.so (declarations and contracts: include/magot.h).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_set>

#include "common.h"

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

struct magot_ctx {
  int device = 0;
  int n_cu = 0;
  int blocks_per_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t mark0 = nullptr, mark1 = nullptr;  // magot_ctx_mark
  // pinned staging ring for genome uploads (allocated on first use); loads on
  // one context from several host threads take turns on it
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  std::mutex pin_mu;
};

struct magot_genome {
  magot_ctx* ctx = nullptr;
  void* arena = nullptr;
  uint64_t arena_bytes = 0;
  bool owns_arena = true;  // false: caller memory (magot_genome_attach)
  uint32_t* nib = nullptr;  // forward then reverse-strand nibble plane (ExtractArgs::span)
  uint64_t span = 0;
  ExcRun* runs = nullptr;
  uint32_t* dir = nullptr;
  std::vector<uint64_t> contig_base, contig_len;
  std::vector<std::string> names;  // contig names (magot_genome_load_fasta)
  std::vector<ExcRun> host_runs;   // host copies for per-interval exception flags
  std::vector<uint32_t> host_dir;
  uint64_t extent = 0, total_bases = 0, n_runs = 0;
};

struct magot_plan {
  magot_ctx* ctx = nullptr;
  const magot_genome* g = nullptr;
  void* arena = nullptr;       // tables (intervals, records, tiles, layout)
  uint64_t arena_bytes = 0;
  void* out_arena = nullptr;   // output buffers (nucleotides, residues)
  uint64_t out_bytes = 0;
  ExtractArgs args{};
  std::vector<uint64_t> nuc_off, pep_off;  // host copies, n_tx+1 (record order)
  // MAGOT_OUT_GENOME_ORDER: records laid out in genome order; each record's
  // place in the output buffers (record order; device copies for reassembly)
  bool genome_order = false;
  std::vector<uint64_t> lay_nuc, lay_pep;
  const uint64_t* d_lay_nuc = nullptr;  // T
  const uint64_t* d_lay_pep = nullptr;  // T
  const uint64_t* d_nuc_off = nullptr;  // T+1
  const uint64_t* d_pep_off = nullptr;  // T+1
  uint64_t n_exons = 0, n_tx = 0;
  uint64_t n_ex_c = 0;  // compacted (non-empty) intervals
  // the interval table of a record-order plan (n_ex_c starts with flag bits,
  // n_ex_c + 1 output offsets), for magot_plan_orf6: the device holds only
  // the packed tile blocks
  std::unique_ptr<uint64_t[]> host_ex_g, host_ex_out;
  bool executed = false;
};

namespace {

// Sub-allocate 256-byte aligned slices of one device allocation.
struct Carve {
  uint64_t used = 0;
  template <class T>
  uint64_t take(uint64_t count) {
    uint64_t at = used;
    used += (count * sizeof(T) + 255) & ~255ull;
    return at;
  }
};

int bind(magot_ctx* ctx) {
  if (!ctx) {
    set_error("null context");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipSetDevice(ctx->device));
  return MAGOT_OK;
}

}  // namespace

// Host meta blob of a packed genome (magot_genome_export / _attach).
namespace {

struct MetaWriter {
  std::vector<uint8_t> buf;
  template <class T>
  void put(const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    buf.insert(buf.end(), p, p + sizeof(T));
  }
  template <class T>
  void put_vec(const std::vector<T>& v) {
    put<uint64_t>(v.size());
    const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
    buf.insert(buf.end(), p, p + v.size() * sizeof(T));
  }
};

struct MetaReader {
  const uint8_t* p;
  const uint8_t* end;
  template <class T>
  bool get(T* v) {
    if ((uint64_t)(end - p) < sizeof(T)) return false;
    memcpy(v, p, sizeof(T));
    p += sizeof(T);
    return true;
  }
  template <class T>
  bool get_vec(std::vector<T>* v) {
    uint64_t n;
    if (!get(&n) || n > (uint64_t)(end - p) / sizeof(T)) return false;
    v->resize(n);
    memcpy(v->data(), p, n * sizeof(T));
    p += n * sizeof(T);
    return true;
  }
};

constexpr uint64_t kMetaMagic = 0x4d41474f54474e31ull;  // "MAGOTGN1"

std::vector<uint8_t> genome_meta(const magot_genome* g) {
  MetaWriter w;
  w.put(kMetaMagic);
  w.put(g->arena_bytes);
  w.put<uint64_t>((const char*)g->nib - (const char*)g->arena);
  w.put<uint64_t>((const char*)g->runs - (const char*)g->arena);
  w.put<uint64_t>((const char*)g->dir - (const char*)g->arena);
  w.put(g->span);
  w.put(g->extent);
  w.put(g->total_bases);
  w.put(g->n_runs);
  w.put_vec(g->contig_base);
  w.put_vec(g->contig_len);
  w.put_vec(g->host_runs);
  w.put_vec(g->host_dir);
  return w.buf;
}

// Parse a meta blob into g's host fields; the piece offsets into *o.
bool parse_genome_meta(const uint8_t* meta, uint64_t meta_len, magot_genome* g, uint64_t o[3]) {
  MetaReader r{meta, meta + meta_len};
  uint64_t magic = 0;
  bool ok = r.get(&magic) && magic == kMetaMagic && r.get(&g->arena_bytes) && r.get(&o[0]) &&
            r.get(&o[1]) && r.get(&o[2]) && r.get(&g->span) && r.get(&g->extent) &&
            r.get(&g->total_bases) && r.get(&g->n_runs) && r.get_vec(&g->contig_base) &&
            r.get_vec(&g->contig_len) && r.get_vec(&g->host_runs) && r.get_vec(&g->host_dir);
  return ok && o[0] < g->arena_bytes && o[1] < g->arena_bytes && o[2] < g->arena_bytes &&
         g->host_runs.size() == g->n_runs + 1 && g->span % 32 == 0 &&
         o[0] + (2 * (g->span / 8) + 4) * 4 <= o[1] && o[1] <= o[2];
}

// Pack the contigs and place the planes in HBM (magot_genome_load*): on the
// device by default, on the host (pack.cpp) with MAGOT_PACK_HOST.
int load_packed(magot_ctx* ctx, const ContigSource* src, uint32_t n_contigs, uint32_t flags,
                magot_genome** out);

}  // namespace

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

int magot_genome_load_ex(magot_ctx* ctx, const uint8_t* const* seqs, const uint64_t* lens,
                         uint32_t n_contigs, uint32_t flags, magot_genome** out) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (n_contigs && (!seqs || !lens))) {
    set_error("magot_genome_load: null argument");
    return MAGOT_ERR_ARG;
  }
  if (flags & ~MAGOT_PACK_HOST) {
    set_error("magot_genome_load_ex: unknown flags");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  for (uint32_t i = 0; i < n_contigs; ++i)
    if (lens[i] && !seqs[i]) {
      set_error("magot_genome_load: null contig pointer");
      return MAGOT_ERR_ARG;
    }
  std::vector<ContigSource> src(n_contigs);
  for (uint32_t i = 0; i < n_contigs; ++i) src[i] = ContigSource{seqs[i], lens[i], 0, 0};
  return load_packed(ctx, src.data(), n_contigs, flags, out);
}

int magot_genome_load(magot_ctx* ctx, const uint8_t* const* seqs, const uint64_t* lens,
                      uint32_t n_contigs, magot_genome** out) {
  return magot_genome_load_ex(ctx, seqs, lens, n_contigs, 0u, out);
}

}  // extern "C"

namespace {

// Host rows bound for one device allocation (dev_off into it).
struct HostPiece {
  uint64_t dev_off;
  const void* src;
  uint64_t bytes;
};

constexpr uint64_t kPinRing = 64ull << 20;  // each of the context's two pinned staging buffers

int ensure_pin_ring(magot_ctx* ctx) {  // callers hold ctx->pin_mu
  for (int k = 0; k < 2; ++k)
    if (!ctx->pin[k]) {
      MAGOT_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->pin[k]), kPinRing,
                                  hipHostMallocDefault));
      MAGOT_HIP_TRY(hipEventCreateWithFlags(&ctx->pin_ev[k], hipEventDisableTiming));
    }
  return MAGOT_OK;
}

// Upload host rows through the context's two pinned staging buffers: host
// threads copy one 64 MiB piece in while the DMA engine drains the other (a
// pageable hipMemcpy stages through the runtime's own small buffers at a
// fraction of the link rate).  Synchronous: the rows are on the device when
// it returns.
int upload_pieces(magot_ctx* ctx, char* dev, const std::vector<HostPiece>& pieces) {
  std::lock_guard<std::mutex> lock(ctx->pin_mu);
  if (int rc = ensure_pin_ring(ctx)) return rc;
  const unsigned nt = host_threads();
  uint64_t k = 0;
  for (const HostPiece& pc : pieces)
    for (uint64_t q0 = 0; q0 < pc.bytes; q0 += kPinRing, ++k) {
      const int b = (int)(k & 1);
      const uint64_t q1 = std::min(pc.bytes, q0 + kPinRing);
      MAGOT_HIP_TRY(hipEventSynchronize(ctx->pin_ev[b]));
      const char* src = static_cast<const char*>(pc.src) + q0;
      uint8_t* ring = ctx->pin[b];
      parallel_ranges(q1 - q0, q1 - q0 >= (4ull << 20) ? nt : 1u,
                      [&](uint64_t lo, uint64_t hi, unsigned) { memcpy(ring + lo, src + lo, hi - lo); });
      MAGOT_HIP_TRY(hipMemcpyAsync(dev + pc.dev_off + q0, ring, q1 - q0, hipMemcpyHostToDevice,
                                   ctx->stream));
      MAGOT_HIP_TRY(hipEventRecord(ctx->pin_ev[b], ctx->stream));
    }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

// As upload_pieces for rows that are generated, not copied: fill(lo, hi, dst)
// writes items [lo, hi) of `item` bytes each to dst, from several host threads
// straight into the pinned buffer that is uploaded next (no pageable copy of
// the table and no second pass over it).
template <class F>
int upload_generated(magot_ctx* ctx, char* dev, uint64_t n, uint64_t item, unsigned threads, F fill) {
  std::lock_guard<std::mutex> lock(ctx->pin_mu);
  if (int rc = ensure_pin_ring(ctx)) return rc;
  const uint64_t per = kPinRing / item;
  for (uint64_t i0 = 0, k = 0; i0 < n; i0 += per, ++k) {
    const int b = (int)(k & 1);
    const uint64_t i1 = std::min(n, i0 + per);
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->pin_ev[b]));
    uint8_t* ring = ctx->pin[b];
    parallel_ranges(i1 - i0, (i1 - i0) * item >= (1ull << 20) ? threads : 1u,
                    [&](uint64_t lo, uint64_t hi, unsigned) { fill(i0 + lo, i0 + hi, ring + lo * item); });
    MAGOT_HIP_TRY(hipMemcpyAsync(dev + i0 * item, ring, (i1 - i0) * item, hipMemcpyHostToDevice,
                                 ctx->stream));
    MAGOT_HIP_TRY(hipEventRecord(ctx->pin_ev[b], ctx->stream));
  }
  return MAGOT_OK;  // in flight: the caller's next upload_pieces (or a stream sync) completes it
}

// Stream the contigs' bytes (FASTA line layout removed) into dev[0, total),
// total = extent - kOrigin, through two pinned 64 MiB host buffers: host
// threads fill one while the DMA engine uploads the other.
int upload_raw(magot_ctx* ctx, const ContigSource* src, const HostPacked& lay, uint8_t* dev) {
  const uint64_t total = lay.extent - kOrigin;
  if (!total) return MAGOT_OK;
  constexpr uint64_t kRing = kPinRing;
  std::lock_guard<std::mutex> lock(ctx->pin_mu);
  if (int rc = ensure_pin_ring(ctx)) return rc;
  const unsigned nt = host_threads();
  const auto& base = lay.contig_base;
  auto fill = [&](uint8_t* dst, uint64_t x0, uint64_t x1) {  // raw [x0, x1) -> dst
    size_t c = std::upper_bound(base.begin(), base.end(), x0 + kOrigin) - base.begin();
    c = c ? c - 1 : 0;
    for (; c < base.size() && x0 < x1; ++c) {
      const uint64_t cb = base[c] - kOrigin, ce = cb + lay.contig_len[c];
      if (ce <= x0) continue;
      const uint64_t hi = std::min(ce, x1);
      copy_bases(src[c], x0 - cb, hi - x0, dst);
      dst += hi - x0;
      x0 = hi;
    }
  };
  for (uint64_t q0 = 0, k = 0; q0 < total; q0 += kRing, ++k) {
    const int b = (int)(k & 1);
    const uint64_t q1 = std::min(total, q0 + kRing);
    // the buffer's previous DMA (of this load, or of an earlier one whose
    // last copies may still be in flight) has drained
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->pin_ev[b]));
    const uint64_t step = ((q1 - q0) + nt - 1) / nt;
    std::vector<std::thread> pool;
    for (unsigned i = 1; i < nt && q0 + i * step < q1; ++i) {
      const uint64_t x0 = q0 + i * step, x1 = std::min(q1, x0 + step);
      pool.emplace_back([&, x0, x1] { fill(ctx->pin[b] + (x0 - q0), x0, x1); });
    }
    fill(ctx->pin[b], q0, std::min(q1, q0 + step));
    for (auto& t : pool) t.join();
    MAGOT_HIP_TRY(hipMemcpyAsync(dev + q0, ctx->pin[b], q1 - q0, hipMemcpyHostToDevice,
                                 ctx->stream));
    MAGOT_HIP_TRY(hipEventRecord(ctx->pin_ev[b], ctx->stream));
  }
  return MAGOT_OK;
}

// RAII device scratch
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// A device allocation made on another thread while the caller goes on
// (hipMalloc of C3's 0.8 GB of outputs takes ~10 ms).  It is joined, and
// freed unless taken, when it goes out of scope.
struct AsyncAlloc {
  void* mem = nullptr;
  hipError_t err = hipSuccess;
  std::thread th;
  AsyncAlloc(int device, uint64_t bytes)
      : th([this, device, bytes]() {
          err = hipSetDevice(device);
          if (err == hipSuccess) err = hipMalloc(&mem, bytes);
        }) {}
  hipError_t take(void** out) {  // the caller owns *out now
    th.join();
    *out = mem;
    mem = nullptr;
    return err;
  }
  ~AsyncAlloc() {
    if (th.joinable()) th.join();
    if (mem) (void)hipFree(mem);
  }
};

// A genome-ordered plan's output (nucleotides, or residues) put back into
// record order at dst (16-byte aligned device memory): one segment copy per
// record from its layout place to its record-order offset, on the context stream.
int plan_reassemble(magot_ctx* ctx, const magot_plan* p, bool residues, void* dst) {
  if (!p->n_tx) return MAGOT_OK;
  launch_segments_copy(residues ? p->args.pep : p->args.nuc,
                       residues ? p->d_lay_pep : p->d_lay_nuc,
                       residues ? p->d_pep_off : p->d_nuc_off, p->n_tx,
                       static_cast<uint8_t*>(dst), ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  return MAGOT_OK;
}

// A genome-ordered plan's output copied down in record order through a
// bounded device scratch: consecutive records in batches of at most
// kFetchBatchBytes (or one longer record) are put back into record order on
// the device (one segment-copy launch per batch), then copied to the host.
// The scratch is 16-byte aligned and the batch's first record keeps its
// offset mod 16, so the copy kernel's aligned stores stay aligned.
constexpr uint64_t kFetchBatchBytes = 256ull << 20;

uint64_t fetch_batch_bytes() {  // MAGOT_FETCH_BATCH_BYTES: test hook (small batches)
  const char* e = std::getenv("MAGOT_FETCH_BATCH_BYTES");
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v ? v : kFetchBatchBytes;
}

int plan_fetch_reordered(magot_ctx* ctx, const magot_plan* p, bool residues, uint8_t* host) {
  const std::vector<uint64_t>& off = residues ? p->pep_off : p->nuc_off;
  const uint64_t T = p->n_tx;
  if (!T || off[T] == 0) return MAGOT_OK;
  uint64_t longest = 0;
  for (uint64_t t = 0; t < T; ++t) longest = std::max(longest, off[t + 1] - off[t]);
  const uint64_t cap = std::max(std::min(off[T], fetch_batch_bytes()), longest);
  DevBuf scratch;
  MAGOT_HIP_TRY(hipMalloc(&scratch.p, cap + 16));
  uint8_t* S = static_cast<uint8_t*>(scratch.p);
  const uint8_t* src = residues ? p->args.pep : p->args.nuc;
  const uint64_t* lay = residues ? p->d_lay_pep : p->d_lay_nuc;
  const uint64_t* doff = residues ? p->d_pep_off : p->d_nuc_off;
  for (uint64_t r0 = 0; r0 < T;) {
    uint64_t r1 = r0 + 1;
    while (r1 < T && off[r1 + 1] - off[r0] <= cap) ++r1;
    const uint64_t base = off[r0], bytes = off[r1] - base;
    if (bytes) {
      // record-order offset x lands at S + (x - (base & ~15))
      launch_segments_copy(src, lay + r0, doff + r0, r1 - r0, S - (base & ~15ull), ctx->stream);
      MAGOT_HIP_TRY(hipGetLastError());
      MAGOT_HIP_TRY(hipMemcpyAsync(host + base, S + (base & 15), bytes, hipMemcpyDeviceToHost,
                                   ctx->stream));
    }
    r0 = r1;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

// Device packing: raw bytes streamed to HBM once, runs counted and written by
// kernels (devpack.hip), the nibble plane packed and mirrored on the device;
// only the run list (and its directory, built from it) passes through the host.
int load_device_packed(magot_ctx* ctx, const ContigSource* src, uint32_t n_contigs,
                       magot_genome** out) {
  Lap lap;
  HostPacked hp;
  pack_layout(src, n_contigs, &hp);
  const uint64_t n = hp.extent - kOrigin;
  const uint64_t groups = (n + 31) / 32;
  const size_t scan_bytes = devpack_scan_bytes(groups);
  Carve sc;
  const uint64_t o_raw = sc.take<uint8_t>(32 * groups + 64);
  const uint64_t o_cnt = sc.take<uint32_t>(groups + 1);
  const uint64_t o_slot = sc.take<uint64_t>(groups + 1);
  const uint64_t o_tmp = sc.take<uint8_t>(scan_bytes + 1);
  DevBuf scratch;
  MAGOT_HIP_TRY(hipMalloc(&scratch.p, sc.used));
  char* sbase = static_cast<char*>(scratch.p);
  uint8_t* raw = reinterpret_cast<uint8_t*>(sbase + o_raw);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(sbase + o_cnt);
  uint64_t* slot = reinterpret_cast<uint64_t*>(sbase + o_slot);
  // the padding past n is read by the 32-byte loads (and masked)
  MAGOT_HIP_TRY(hipMemsetAsync(raw + n, 0, 32 * groups + 64 - n, ctx->stream));
  if (int rc = upload_raw(ctx, src, hp, raw)) return rc;
  lap("upload");
  MAGOT_HIP_TRY(launch_run_count(raw, n, cnt, slot, sbase + o_tmp, scan_bytes, ctx->stream));
  uint64_t n_runs = 0;
  if (groups) {
    uint64_t last_slot = 0;
    uint32_t last_cnt = 0;
    MAGOT_HIP_TRY(hipMemcpyAsync(&last_slot, slot + groups - 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    MAGOT_HIP_TRY(hipMemcpyAsync(&last_cnt, cnt + groups - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
    n_runs = last_slot + last_cnt;
  }
  if (n_runs + 1 >= (uint64_t)kDirClean) {
    set_error("magot_genome_load: too many exception runs");
    return MAGOT_ERR_ARG;
  }
  DevBuf runs_tmp;
  std::vector<uint64_t> rs(n_runs), re(n_runs);
  std::vector<uint8_t> rb(n_runs);
  if (n_runs) {
    MAGOT_HIP_TRY(hipMalloc(&runs_tmp.p, n_runs * 17 + 16));
    uint64_t* d_rs = static_cast<uint64_t*>(runs_tmp.p);
    uint64_t* d_re = d_rs + n_runs;
    uint8_t* d_rb = reinterpret_cast<uint8_t*>(d_re + n_runs);
    launch_run_write(raw, n, slot, d_rs, d_re, d_rb, ctx->stream);
    MAGOT_HIP_TRY(hipGetLastError());
    MAGOT_HIP_TRY(hipMemcpyAsync(rs.data(), d_rs, n_runs * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAGOT_HIP_TRY(hipMemcpyAsync(re.data(), d_re, n_runs * 8, hipMemcpyDeviceToHost, ctx->stream));
    MAGOT_HIP_TRY(hipMemcpyAsync(rb.data(), d_rb, n_runs, hipMemcpyDeviceToHost, ctx->stream));
    MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  // ExcRun list: runs longer than the 31-bit length field are split (as the
  // host packer does), then the sentinel and the directory
  hp.runs.clear();
  hp.runs.reserve(n_runs + 1);
  for (uint64_t k = 0; k < n_runs; ++k) {
    for (uint64_t a = rs[k]; a < re[k];) {
      const uint64_t len = std::min<uint64_t>(re[k] - a, 0x7fffffffull);
      hp.runs.push_back(ExcRun{a, (uint32_t)len, rb[k]});
      a += len;
    }
  }
  hp.runs.push_back(ExcRun{~0ull, 0, 0});
  if (hp.runs.size() >= (size_t)kDirClean) {
    set_error("magot_genome_load: too many exception runs");
    return MAGOT_ERR_ARG;
  }
  exc_runs_directory(&hp);
  lap("runs");
  std::unique_ptr<magot_genome> g(new magot_genome());
  g->ctx = ctx;
  Carve cv;
  const uint64_t o_nib = cv.take<uint32_t>(2 * hp.nib_words + 4);
  const uint64_t o_runs = cv.take<ExcRun>(hp.runs.size());
  const uint64_t o_dir = cv.take<uint32_t>(hp.dir.size());
  MAGOT_HIP_TRY(hipMalloc(&g->arena, cv.used));
  g->arena_bytes = cv.used;
  char* base = static_cast<char*>(g->arena);
  g->nib = reinterpret_cast<uint32_t*>(base + o_nib);
  g->runs = reinterpret_cast<ExcRun*>(base + o_runs);
  g->dir = reinterpret_cast<uint32_t*>(base + o_dir);
  launch_nib_pack(raw, n, g->nib, hp.nib_words, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipMemsetAsync(g->nib + 2 * hp.nib_words, 0, 16, ctx->stream));
  launch_mirror_planes(g->nib, hp.span, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipMemcpyAsync(g->runs, hp.runs.data(), hp.runs.size() * sizeof(ExcRun),
                               hipMemcpyHostToDevice, ctx->stream));
  MAGOT_HIP_TRY(hipMemcpyAsync(g->dir, hp.dir.data(), hp.dir.size() * 4, hipMemcpyHostToDevice,
                               ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  g->span = hp.span;
  g->contig_base = std::move(hp.contig_base);
  g->contig_len = std::move(hp.contig_len);
  g->n_runs = hp.runs.size() - 1;
  g->host_runs = std::move(hp.runs);
  g->host_dir = std::move(hp.dir);
  g->extent = hp.extent;
  g->total_bases = hp.extent - kOrigin;
  lap("pack");
  *out = g.release();
  return MAGOT_OK;
}

int load_packed(magot_ctx* ctx, const ContigSource* src, uint32_t n_contigs, uint32_t flags,
                magot_genome** out) {
  {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_contigs; ++i) total += src[i].len;
    // the packed span (kOrigin + bases + padding, pack_genome) must stay below
    // 4 Gi nibble bytes: 32-bit window offsets in extract_kernel
    if (total + kOrigin + 256 > 0xFFFFFFF0ull) {
      set_error("magot_genome_load: genomes above 4 Gbases take several device planes "
                "(engine.PartitionedGenome)");
      return MAGOT_ERR_UNSUPPORTED;
    }
  }
  if (!(flags & MAGOT_PACK_HOST)) return load_device_packed(ctx, src, n_contigs, out);
  Lap lap;
  HostPacked hp;
  pack_genome(src, n_contigs, &hp);
  lap("pack");
  if (hp.runs.size() >= (size_t)kDirClean) {
    set_error("magot_genome_load: too many exception runs");
    return MAGOT_ERR_ARG;
  }
  if (2 * hp.nib_words * 4 + 16 > 0xFFFFFFFFull) {  // 32-bit buffer offsets (extract.hip)
    set_error("magot_genome_load: genomes above 4 Gbases take several device planes");
    return MAGOT_ERR_UNSUPPORTED;
  }
  std::unique_ptr<magot_genome> g(new magot_genome());
  g->ctx = ctx;
  Carve cv;
  // forward + reverse-strand planes, 4 words of slack for window over-reads
  uint64_t o_nib = cv.take<uint32_t>(2 * hp.nib_words + 4);
  uint64_t o_runs = cv.take<ExcRun>(hp.runs.size());
  uint64_t o_dir = cv.take<uint32_t>(hp.dir.size());
  MAGOT_HIP_TRY(hipMalloc(&g->arena, cv.used));
  g->arena_bytes = cv.used;
  char* base = static_cast<char*>(g->arena);
  g->nib = reinterpret_cast<uint32_t*>(base + o_nib);
  g->runs = reinterpret_cast<ExcRun*>(base + o_runs);
  g->dir = reinterpret_cast<uint32_t*>(base + o_dir);
  MAGOT_HIP_TRY(hipMemcpy(g->nib, hp.nib.get(), hp.nib_words * 4, hipMemcpyHostToDevice));
  MAGOT_HIP_TRY(hipMemset(g->nib + 2 * hp.nib_words, 0, 16));
  launch_mirror_planes(g->nib, hp.span, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  g->span = hp.span;
  MAGOT_HIP_TRY(hipMemcpy(g->runs, hp.runs.data(), hp.runs.size() * sizeof(ExcRun),
                          hipMemcpyHostToDevice));
  MAGOT_HIP_TRY(hipMemcpy(g->dir, hp.dir.data(), hp.dir.size() * 4, hipMemcpyHostToDevice));
  g->contig_base = std::move(hp.contig_base);
  g->contig_len = std::move(hp.contig_len);
  g->n_runs = hp.runs.size() - 1;
  g->host_runs = std::move(hp.runs);
  g->host_dir = std::move(hp.dir);
  g->extent = hp.extent;
  g->total_bases = hp.extent - kOrigin;
  lap("upload");
  *out = g.release();
  return MAGOT_OK;
}

}  // namespace

extern "C" {

int magot_genome_load_fasta(magot_ctx* ctx, const char* text, uint64_t len, int truncate_names,
                            magot_genome** out) {
  if (int rc = bind(ctx)) return rc;
  if (!out || (len && !text)) {
    set_error("magot_genome_load_fasta: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  FastaContigs fc;
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = scan_fasta(text, len, truncate_names != 0, &fc)) {
    set_error("magot_genome_load_fasta: header needs the Python reader");
    return rc;
  }
  if (std::getenv("MAGOT_GENOME_TIMING"))
    fprintf(stderr, "[genome] scan     %.3f s\n",
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  magot_genome* g = nullptr;
  if (int rc = load_packed(ctx, fc.src.data(), (uint32_t)fc.src.size(), 0u, &g)) return rc;
  g->names = std::move(fc.names);
  *out = g;
  return MAGOT_OK;
}

int magot_genome_contigs(const magot_genome* g, uint32_t* n, uint64_t* lens, char* names,
                         uint64_t names_cap, uint64_t* names_len) {
  if (!g || !n) {
    set_error("magot_genome_contigs: null argument");
    return MAGOT_ERR_ARG;
  }
  *n = (uint32_t)g->contig_len.size();
  if (lens) std::memcpy(lens, g->contig_len.data(), g->contig_len.size() * 8);
  uint64_t need = 0;
  for (const auto& s : g->names) need += s.size() + 1;
  if (names_len) *names_len = need;
  if (names) {
    if (names_cap < need) {
      set_error("magot_genome_contigs: names buffer too small");
      return MAGOT_ERR_ARG;
    }
    for (const auto& s : g->names) {
      std::memcpy(names, s.data(), s.size());
      names += s.size();
      *names++ = '\0';
    }
  }
  return MAGOT_OK;
}

int magot_genome_stats(const magot_genome* g, uint64_t* total_bases, uint64_t* n_exc_runs,
                       uint64_t* device_bytes) {
  if (!g) {
    set_error("magot_genome_stats: null genome");
    return MAGOT_ERR_ARG;
  }
  if (total_bases) *total_bases = g->total_bases;
  if (n_exc_runs) *n_exc_runs = g->n_runs;
  if (device_bytes) *device_bytes = g->arena_bytes;
  return MAGOT_OK;
}

void magot_genome_destroy(magot_genome* g) {
  if (!g) return;
  if (g->ctx) (void)hipSetDevice(g->ctx->device);
  if (g->arena && g->owns_arena) (void)hipFree(g->arena);
  delete g;
}

// --- replication (one packed genome broadcast to every rank) ---------------

int magot_genome_export(const magot_genome* g, uint8_t* meta, uint64_t cap, uint64_t* meta_len,
                        uint64_t* arena_bytes) {
  if (!g || !meta_len) {
    set_error("magot_genome_export: null argument");
    return MAGOT_ERR_ARG;
  }
  const std::vector<uint8_t> m = genome_meta(g);
  *meta_len = m.size();
  if (arena_bytes) *arena_bytes = g->arena_bytes;
  if (!meta) return MAGOT_OK;
  if (cap < m.size()) {
    set_error("magot_genome_export: meta buffer too small");
    return MAGOT_ERR_ARG;
  }
  memcpy(meta, m.data(), m.size());
  return MAGOT_OK;
}

int magot_genome_copy_arena(const magot_genome* g, void* dst_dev) {
  if (!g || !dst_dev) {
    set_error("magot_genome_copy_arena: null argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = bind(g->ctx)) return rc;
  MAGOT_HIP_TRY(hipMemcpyAsync(dst_dev, g->arena, g->arena_bytes, hipMemcpyDeviceToDevice,
                               g->ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(g->ctx->stream));
  return MAGOT_OK;
}

int magot_genome_attach(magot_ctx* ctx, const uint8_t* meta, uint64_t meta_len, void* arena_dev,
                        magot_genome** out) {
  if (int rc = bind(ctx)) return rc;
  if (!meta || !arena_dev || !out) {
    set_error("magot_genome_attach: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  std::unique_ptr<magot_genome> g(new magot_genome());
  uint64_t o[3];
  if (!parse_genome_meta(meta, meta_len, g.get(), o)) {
    set_error("magot_genome_attach: malformed genome meta");
    return MAGOT_ERR_ARG;
  }
  g->ctx = ctx;
  g->arena = arena_dev;
  g->owns_arena = false;
  char* base = static_cast<char*>(arena_dev);
  g->nib = reinterpret_cast<uint32_t*>(base + o[0]);
  g->runs = reinterpret_cast<ExcRun*>(base + o[1]);
  g->dir = reinterpret_cast<uint32_t*>(base + o[2]);
  *out = g.release();
  return MAGOT_OK;
}

int magot_genome_wire_ranges(const magot_genome* g, uint64_t* off, uint64_t* len, uint32_t* n) {
  if (!g || !off || !len || !n) {
    set_error("magot_genome_wire_ranges: null argument");
    return MAGOT_ERR_ARG;
  }
  // [forward nibble plane] and [exception runs .. directory end]: the mirror
  // plane between them (and its 16 bytes of slack) is derived on attach
  const char* a = static_cast<const char*>(g->arena);
  off[0] = (uint64_t)((const char*)g->nib - a);
  len[0] = g->span / 2;  // span bases, 8 per 4-byte word
  off[1] = (uint64_t)((const char*)g->runs - a);
  len[1] = g->arena_bytes - off[1];
  *n = 2;
  return MAGOT_OK;
}

int magot_genome_attach_wire(magot_ctx* ctx, const uint8_t* meta, uint64_t meta_len,
                             void* arena_dev, magot_genome** out) {
  if (int rc = magot_genome_attach(ctx, meta, meta_len, arena_dev, out)) return rc;
  magot_genome* g = *out;
  const uint64_t nw = g->span / 8;
  if ((uint64_t)((char*)g->runs - (char*)g->arena) < (2 * nw + 4) * 4) {
    magot_genome_destroy(g);
    *out = nullptr;
    set_error("magot_genome_attach_wire: malformed genome meta");
    return MAGOT_ERR_ARG;
  }
  hipError_t e = hipMemsetAsync(g->nib + 2 * nw, 0, 16, ctx->stream);
  if (e == hipSuccess) {
    launch_mirror_planes(g->nib, g->span, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    magot_genome_destroy(g);
    *out = nullptr;
    set_error(std::string("magot_genome_attach_wire: ") + hipGetErrorString(e));
    return MAGOT_ERR_HIP;
  }
  return MAGOT_OK;
}

// --- the compact replica image (wire.hip) ---------------------------------

namespace {

uint64_t fnv1a(const uint8_t* p, uint64_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

// The image layout of a genome (span bases, arena_bytes with the exception
// runs at runs_off, meta blob hash) with n_mask soft-mask runs.
WireHeader wire_layout(uint64_t span, uint64_t arena_bytes, uint64_t runs_off, uint64_t n_mask,
                       uint64_t meta_hash) {
  WireHeader h{};
  h.magic = kWireMagic;
  h.meta_hash = meta_hash;
  h.span = span;
  h.n_mask = n_mask;
  h.n_mdir = (span >> kDirShift) + 2;
  Carve cv;
  cv.take<WireHeader>(1);
  h.o_code2 = cv.take<uint32_t>(span / 16);
  h.o_mask = cv.take<uint32_t>(2 * (n_mask + 1));
  h.o_mdir = cv.take<uint32_t>(h.n_mdir);
  h.exc_bytes = arena_bytes - runs_off;
  h.o_exc = cv.take<uint8_t>(h.exc_bytes);
  h.total = cv.used;
  return h;
}

}  // namespace

int magot_genome_wire_export(const magot_genome* g, void* wire_dev, uint64_t cap,
                             uint64_t* wire_bytes) {
  if (!g || !wire_bytes) {
    set_error("magot_genome_wire_export: null argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = bind(g->ctx)) return rc;
  hipStream_t st = g->ctx->stream;
  const uint64_t groups = g->span / 32;
  const size_t scan_bytes = wire_scan_bytes(groups);
  Carve sc;
  const uint64_t o_cnt = sc.take<uint32_t>(groups + 1);
  const uint64_t o_slot = sc.take<uint64_t>(groups + 1);
  const uint64_t o_tmp = sc.take<uint8_t>(scan_bytes + 1);
  DevBuf scratch;
  MAGOT_HIP_TRY(hipMalloc(&scratch.p, sc.used));
  char* sb = static_cast<char*>(scratch.p);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(sb + o_cnt);
  uint64_t* slot = reinterpret_cast<uint64_t*>(sb + o_slot);
  MAGOT_HIP_TRY(launch_wire_count(g->nib, g->span, cnt, slot, sb + o_tmp, scan_bytes, st));
  uint64_t n_mask = 0;
  if (groups) {
    uint64_t last_slot = 0;
    uint32_t last_cnt = 0;
    MAGOT_HIP_TRY(hipMemcpyAsync(&last_slot, slot + groups - 1, 8, hipMemcpyDeviceToHost, st));
    MAGOT_HIP_TRY(hipMemcpyAsync(&last_cnt, cnt + groups - 1, 4, hipMemcpyDeviceToHost, st));
    MAGOT_HIP_TRY(hipStreamSynchronize(st));
    n_mask = last_slot + last_cnt;
  }
  const std::vector<uint8_t> meta = genome_meta(g);
  const WireHeader h = wire_layout(g->span, g->arena_bytes,
                                   (uint64_t)((const char*)g->runs - (const char*)g->arena), n_mask,
                                   fnv1a(meta.data(), meta.size()));
  *wire_bytes = h.total;
  if (!wire_dev) return MAGOT_OK;
  if (cap < h.total) {
    set_error("magot_genome_wire_export: image buffer too small");
    return MAGOT_ERR_ARG;
  }
  char* wb = static_cast<char*>(wire_dev);
  uint32_t* runs = reinterpret_cast<uint32_t*>(wb + h.o_mask);
  launch_code2(g->nib, g->span / 8, reinterpret_cast<uint32_t*>(wb + h.o_code2), st);
  MAGOT_HIP_TRY(hipGetLastError());
  launch_wire_runs(g->nib, g->span, slot, runs, st);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipMemsetAsync(runs + 2 * n_mask, 0xFF, 8, st));  // sentinel {~0, ~0}
  launch_wire_mdir(runs, n_mask, h.n_mdir, reinterpret_cast<uint32_t*>(wb + h.o_mdir), st);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipMemcpyAsync(wb + h.o_exc, g->runs, h.exc_bytes, hipMemcpyDeviceToDevice, st));
  MAGOT_HIP_TRY(hipMemcpyAsync(wb, &h, sizeof(h), hipMemcpyHostToDevice, st));
  MAGOT_HIP_TRY(hipStreamSynchronize(st));
  return MAGOT_OK;
}

int magot_genome_wire_import(magot_ctx* ctx, const uint8_t* meta, uint64_t meta_len,
                             const void* wire_dev, uint64_t wire_bytes, magot_genome** out) {
  if (int rc = bind(ctx)) return rc;
  if (!meta || !wire_dev || !out) {
    set_error("magot_genome_wire_import: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  std::unique_ptr<magot_genome> g(new magot_genome());
  uint64_t o[3];
  if (!parse_genome_meta(meta, meta_len, g.get(), o)) {
    set_error("magot_genome_wire_import: malformed genome meta");
    return MAGOT_ERR_ARG;
  }
  if (wire_bytes < sizeof(WireHeader)) {
    set_error("magot_genome_wire_import: image too small");
    return MAGOT_ERR_ARG;
  }
  WireHeader h{};
  MAGOT_HIP_TRY(hipMemcpyAsync(&h, wire_dev, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  g->ctx = ctx;
  // the image must have been cut from the genome the meta describes
  const WireHeader want = wire_layout(g->span, g->arena_bytes, o[1], h.n_mask,
                                      fnv1a(meta, meta_len));
  if (h.magic != kWireMagic || h.total > wire_bytes || h.n_mask >= (1ull << 32) ||
      std::memcmp(&h, &want, sizeof(h)) != 0) {
    set_error("magot_genome_wire_import: image does not match the genome meta");
    return MAGOT_ERR_ARG;
  }
  DevBuf arena;  // owned by the genome once everything below succeeded
  MAGOT_HIP_TRY(hipMalloc(&arena.p, g->arena_bytes));
  g->arena = arena.p;
  g->owns_arena = true;
  char* base = static_cast<char*>(g->arena);
  g->nib = reinterpret_cast<uint32_t*>(base + o[0]);
  g->runs = reinterpret_cast<ExcRun*>(base + o[1]);
  g->dir = reinterpret_cast<uint32_t*>(base + o[2]);
  const char* wb = static_cast<const char*>(wire_dev);
  const ExcRun* w_exc = reinterpret_cast<const ExcRun*>(wb + h.o_exc);
  const uint32_t* w_edir = reinterpret_cast<const uint32_t*>(wb + h.o_exc + (o[2] - o[1]));
  const uint64_t nw = g->span / 8;
  hipStream_t st = ctx->stream;
  launch_wire_unpack(reinterpret_cast<const uint32_t*>(wb + h.o_code2),
                     reinterpret_cast<const uint32_t*>(wb + h.o_mask), h.n_mask,
                     reinterpret_cast<const uint32_t*>(wb + h.o_mdir), h.n_mdir, w_exc, g->n_runs,
                     w_edir, g->host_dir.size(), g->span, g->nib, st);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipMemsetAsync(g->nib + 2 * nw, 0, 16, st));
  launch_mirror_planes(g->nib, g->span, st);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipMemcpyAsync(g->runs, w_exc, h.exc_bytes, hipMemcpyDeviceToDevice, st));
  MAGOT_HIP_TRY(hipStreamSynchronize(st));
  arena.p = nullptr;
  *out = g.release();
  return MAGOT_OK;
}

int magot_copy_segments(magot_ctx* ctx, const void* src_dev, uint64_t src_bytes, void* dst_dev,
                        const uint64_t* src_off, const uint64_t* dst_off, uint64_t n) {
  if (int rc = bind(ctx)) return rc;
  if (!src_off || !dst_off) {
    set_error("magot_copy_segments: null argument");
    return MAGOT_ERR_ARG;
  }
  if (!n || dst_off[n] == dst_off[0]) return MAGOT_OK;
  if (!src_dev || !dst_dev) {
    set_error("magot_copy_segments: null buffer");
    return MAGOT_ERR_ARG;
  }
  // the kernel reads whole 16-byte blocks of src (each holds a byte of its
  // segment, so an aligned block never leaves the allocation's pages) and
  // stores 16-byte chunks at 16-aligned dst offsets
  if ((reinterpret_cast<uintptr_t>(src_dev) | reinterpret_cast<uintptr_t>(dst_dev)) & 15u) {
    set_error("magot_copy_segments: src and dst must be 16-byte aligned");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t i = 0; i < n; ++i) {
    if (dst_off[i + 1] < dst_off[i]) {
      set_error("magot_copy_segments: dst_off must be non-decreasing");
      return MAGOT_ERR_ARG;
    }
    const uint64_t len = dst_off[i + 1] - dst_off[i];
    if (len && (src_off[i] > src_bytes || len > src_bytes - src_off[i])) {
      set_error("magot_copy_segments: segment " + std::to_string(i) + " reads past src_bytes");
      return MAGOT_ERR_RANGE;
    }
    // the grouped copy counts a group's 16-byte chunks in 32 bits (wavecopy.h):
    // below 4 GiB per segment, a group of kSpanGroup stays below 2^32 chunks
    if (len >> 32) {
      set_error("magot_copy_segments: segment " + std::to_string(i) +
                " is 4 GiB or longer (split it)");
      return MAGOT_ERR_ARG;
    }
  }
  DevBuf tables;
  MAGOT_HIP_TRY(hipMalloc(&tables.p, (2 * n + 1) * 8));
  uint64_t* d_src = static_cast<uint64_t*>(tables.p);
  uint64_t* d_dst = d_src + n;
  MAGOT_HIP_TRY(hipMemcpyAsync(d_src, src_off, n * 8, hipMemcpyHostToDevice, ctx->stream));
  MAGOT_HIP_TRY(hipMemcpyAsync(d_dst, dst_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  launch_segments_copy(static_cast<const uint8_t*>(src_dev), d_src, d_dst, n,
                       static_cast<uint8_t*>(dst_dev), ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

// The planning is tileplan.cpp's (host only); here: the device side of a plan.
int magot_plan_create(magot_ctx* ctx, const magot_genome* g, const magot_exon* exons,
                      uint64_t n_exons, const magot_tx* txs, uint64_t n_tx, uint32_t outputs,
                      magot_plan** out, uint64_t* nuc_bytes, uint64_t* pep_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!g || !out) {
    set_error("magot_plan_create: null argument");
    return MAGOT_ERR_ARG;
  }
  if (int rc = plan_check_tables(exons, n_exons, txs, n_tx, outputs)) return rc;
  *out = nullptr;
  Lap lap("MAGOT_PLAN_TIMING", "plan");
  const PlanInput in{GenomeView{g->contig_base.data(), g->contig_len.data(), g->contig_base.size(),
                                g->span, g->host_runs.data(), g->host_dir.data()},
                     exons, n_exons, txs, n_tx, plan_options(outputs)};
  const bool by_genome = in.opt.by_genome;
  PlanCount cnt;
  if (int rc = plan_count(in, &cnt)) return rc;
  const uint64_t T = n_tx, B = cnt.B, P = cnt.P;
  // The output buffers' size is known now: allocate them on another thread
  // while this one plans.
  const uint64_t out_nuc = (in.opt.outputs & MAGOT_OUT_NUC) ? B + 64 : 64;
  const uint64_t out_pep = (in.opt.outputs & MAGOT_OUT_PEP) ? P + 64 : 64;
  const uint64_t out_bytes = ((out_nuc + 255) & ~255ull) + out_pep;
  AsyncAlloc out_alloc(ctx->device, out_bytes);
  TilePlan pl;
  if (int rc = plan_build(in, std::move(cnt), lap, &pl)) return rc;
  const uint32_t n_tiles = (uint32_t)pl.tiles.size();
  const TileGeometry geo = pl.geo;

  // --- device arena -----------------------------------------------------------
  std::unique_ptr<magot_plan> p(new magot_plan());
  p->ctx = ctx;
  p->g = g;
  Carve cv;
  // The device holds the tiles' packed blocks and their overflow rows, not
  // the u64 tables they are packed from.
  const uint64_t o_blocks = cv.take<uint8_t>((uint64_t)n_tiles * geo.stride);
  const uint64_t o_ovf_ex = cv.take<uint64_t>(pl.n_ovf_ex + 1);
  const uint64_t o_ovf_tx = cv.take<TxRow>(pl.n_ovf_tx + 1);
  // genome order: {layout place, record-order offsets} per output, for the
  // reassembly copies (magot_plan_fetch / copy_outputs)
  const uint64_t lay_rows = by_genome ? T : 0;
  const uint64_t o_lay_nuc = cv.take<uint64_t>(lay_rows);
  const uint64_t o_rec_nuc = cv.take<uint64_t>(by_genome ? T + 1 : 0);
  const uint64_t o_lay_pep = cv.take<uint64_t>(lay_rows);
  const uint64_t o_rec_pep = cv.take<uint64_t>(by_genome ? T + 1 : 0);
  MAGOT_HIP_TRY(hipMalloc(&p->arena, cv.used));
  p->arena_bytes = cv.used;
  const hipError_t out_err = out_alloc.take(&p->out_arena);
  MAGOT_HIP_TRY(out_err);
  p->out_bytes = out_bytes;
  lap("malloc");
  char* base = static_cast<char*>(p->arena);
  // Blocks are packed by the host threads straight into the upload's pinned
  // buffers, tile ranges in parallel; a tile's overflow rows go to its place
  // in the (small) overflow arrays, uploaded after.
  HostBuf<uint64_t> ovf_ex(pl.n_ovf_ex + 1);
  HostBuf<TxRow> ovf_tx(pl.n_ovf_tx + 1);
  ovf_ex[pl.n_ovf_ex] = 0;
  ovf_tx[pl.n_ovf_tx] = TxRow{0, 0};
  const TileTables tb{pl.ex_g.data(), pl.ex_out.data(), pl.tn.data(), pl.tp.data(), g->span,
                      pl.lane_chunks};
  if (int rc = upload_generated(
          ctx, base + o_blocks, n_tiles, geo.stride, n_tiles >= (1u << 12) ? pl.nth : 1u,
          [&](uint64_t t0, uint64_t t1, uint8_t* dst) {
            for (uint64_t t = t0; t < t1; ++t)
              pack_tile_block(tb, geo, pl.tiles[t], pl.ovf_at[2 * t], pl.ovf_at[2 * t + 1],
                              dst + (t - t0) * geo.stride, ovf_ex.data(), ovf_tx.data());
          }))
    return rc;
  lap("blocks");
  std::vector<HostPiece> pieces = {{o_ovf_ex, ovf_ex.data(), (pl.n_ovf_ex + 1) * 8},
                                   {o_ovf_tx, ovf_tx.data(), (pl.n_ovf_tx + 1) * sizeof(TxRow)}};
  if (by_genome) {
    pieces.push_back({o_lay_nuc, pl.lay_nuc.data(), T * 8});
    pieces.push_back({o_rec_nuc, pl.nuc_off.data(), (T + 1) * 8});
    pieces.push_back({o_lay_pep, pl.lay_pep.data(), T * 8});
    pieces.push_back({o_rec_pep, pl.pep_off.data(), (T + 1) * 8});
  }
  if (int rc = upload_pieces(ctx, base, pieces)) return rc;
  if (by_genome) {
    p->genome_order = true;
    p->d_lay_nuc = reinterpret_cast<const uint64_t*>(base + o_lay_nuc);
    p->d_nuc_off = reinterpret_cast<const uint64_t*>(base + o_rec_nuc);
    p->d_lay_pep = reinterpret_cast<const uint64_t*>(base + o_lay_pep);
    p->d_pep_off = reinterpret_cast<const uint64_t*>(base + o_rec_pep);
  }
  lap("upload");
  if (lap.on) {  // everything in the arena is uploaded once, here
    uint64_t up = (uint64_t)n_tiles * geo.stride;
    for (const HostPiece& pc : pieces) up += pc.bytes;
    fprintf(stderr,
            "[plan] tiles %u, block rows %u + %u (%u bytes), overflow rows %llu + %llu, arena %llu "
            "bytes, uploaded %llu\n",
            n_tiles, geo.ex_rows, geo.tx_rows, geo.stride, (unsigned long long)pl.n_ovf_ex,
            (unsigned long long)pl.n_ovf_tx, (unsigned long long)cv.used, (unsigned long long)up);
  }

  ExtractArgs& a = p->args;
  a.nib = g->nib;
  a.span = g->span;
  a.runs = g->runs;
  a.dir = g->dir;
  a.blocks = reinterpret_cast<const uint8_t*>(base + o_blocks);
  a.blk = geo;
  a.ovf_ex = reinterpret_cast<const uint64_t*>(base + o_ovf_ex);
  a.ovf_tx = reinterpret_cast<const TxRow*>(base + o_ovf_tx);
  a.nuc = static_cast<uint8_t*>(p->out_arena);
  a.pep = static_cast<uint8_t*>(p->out_arena) + ((out_nuc + 255) & ~255ull);
  a.total_nuc = B;
  a.total_pep = P;
  a.n_tiles = n_tiles;
  a.outputs = in.opt.outputs;
  a.lane_chunks = pl.lane_chunks;
  if (const char* dbg = std::getenv("MAGOT_DEBUG_PATHS")) {
    const int v = std::atoi(dbg);
    if (v & 1) a.outputs |= kDebugSlowNuc;
    if (v & 2) a.outputs |= kDebugSlowPep;
  }
  uint8_t lut[64];
  standard_lut(lut);
  std::memcpy(a.lut, lut, 64);

  p->nuc_off = std::move(pl.nuc_off);
  p->pep_off = std::move(pl.pep_off);
  p->lay_nuc = std::move(pl.lay_nuc);
  p->lay_pep = std::move(pl.lay_pep);
  p->n_exons = n_exons;
  p->n_ex_c = pl.Ec;
  p->n_tx = T;
  if (!by_genome) {  // magot_plan_orf6's rows (it refuses a genome-order plan)
    p->host_ex_g = std::move(pl.ex_g.p);
    p->host_ex_out = std::move(pl.ex_out.p);
  }
  if (nuc_bytes) *nuc_bytes = B;
  if (pep_bytes) *pep_bytes = P;
  *out = p.release();
  return MAGOT_OK;
}

void magot_plan_destroy(magot_plan* p) {
  if (!p) return;
  if (p->ctx) (void)hipSetDevice(p->ctx->device);
  if (p->arena) (void)hipFree(p->arena);
  if (p->out_arena) (void)hipFree(p->out_arena);
  delete p;
}

int magot_plan_execute(magot_ctx* ctx, magot_plan* p) {
  if (int rc = bind(ctx)) return rc;
  if (!p) {
    set_error("magot_plan_execute: null plan");
    return MAGOT_ERR_ARG;
  }
  launch_extract(p->args, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  p->executed = true;
  return MAGOT_OK;
}

int magot_plan_fetch(magot_ctx* ctx, magot_plan* p, uint8_t* nuc_out, uint64_t* nuc_off,
                     uint8_t* pep_out, uint64_t* pep_off) {
  if (int rc = bind(ctx)) return rc;
  if (!p) {
    set_error("magot_plan_fetch: null plan");
    return MAGOT_ERR_ARG;
  }
  if (!p->executed) {
    set_error("magot_plan_fetch: plan not executed");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if ((nuc_out && p->args.total_nuc && !(p->args.outputs & MAGOT_OUT_NUC)) ||
      (pep_out && p->args.total_pep && !(p->args.outputs & MAGOT_OUT_PEP))) {
    set_error(std::string("magot_plan_fetch: plan built without ") +
              (nuc_out && !(p->args.outputs & MAGOT_OUT_NUC) ? "MAGOT_OUT_NUC" : "MAGOT_OUT_PEP"));
    return MAGOT_ERR_STATE;
  }
  const bool want_nuc = nuc_out && p->args.total_nuc, want_pep = pep_out && p->args.total_pep;
  if (want_nuc) {
    if (p->genome_order) {
      if (int rc = plan_fetch_reordered(ctx, p, false, nuc_out)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(nuc_out, p->args.nuc, p->args.total_nuc,
                                   hipMemcpyDeviceToHost, ctx->stream));
      MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  }
  if (want_pep) {
    if (p->genome_order) {
      if (int rc = plan_fetch_reordered(ctx, p, true, pep_out)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(pep_out, p->args.pep, p->args.total_pep,
                                   hipMemcpyDeviceToHost, ctx->stream));
      MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  }
  if (nuc_off) std::memcpy(nuc_off, p->nuc_off.data(), p->nuc_off.size() * 8);
  if (pep_off) std::memcpy(pep_off, p->pep_off.data(), p->pep_off.size() * 8);
  return MAGOT_OK;
}

int magot_run(magot_ctx* ctx, magot_plan* p, uint8_t* nuc_out, uint64_t* nuc_off, uint8_t* pep_out,
              uint64_t* pep_off) {
  if (int rc = magot_plan_execute(ctx, p)) return rc;
  return magot_plan_fetch(ctx, p, nuc_out, nuc_off, pep_out, pep_off);
}

int magot_plan_time(magot_ctx* ctx, magot_plan* p, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!p || iters <= 0 || !avg_ms) {
    set_error("magot_plan_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  double total = 0.0;
  for (int i = 0; i < iters; ++i) {
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    launch_extract(p->args, ctx->stream);
    MAGOT_HIP_TRY(hipGetLastError());
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total += ms;
  }
  p->executed = true;
  *avg_ms = total / iters;
  return MAGOT_OK;
}

int magot_plan_time_b2b(magot_ctx* ctx, magot_plan* p, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!p || iters <= 0 || !avg_ms) {
    set_error("magot_plan_time_b2b: bad argument");
    return MAGOT_ERR_ARG;
  }
  // one event pair around `iters` back-to-back launches: the per-launch time
  // of a step loop (no host round trip between launches)
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int i = 0; i < iters; ++i) launch_extract(p->args, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  p->executed = true;
  *avg_ms = (double)ms / iters;
  return MAGOT_OK;
}

int magot_plan_copy_outputs(magot_ctx* ctx, magot_plan* p, void* nuc_dst_dev, void* pep_dst_dev) {
  if (int rc = bind(ctx)) return rc;
  if (!p) {
    set_error("magot_plan_copy_outputs: null plan");
    return MAGOT_ERR_ARG;
  }
  if (p->genome_order && ((nuc_dst_dev && (reinterpret_cast<uintptr_t>(nuc_dst_dev) & 15)) ||
                          (pep_dst_dev && (reinterpret_cast<uintptr_t>(pep_dst_dev) & 15)))) {
    set_error("magot_plan_copy_outputs: a genome-ordered plan needs 16-byte aligned destinations");
    return MAGOT_ERR_ARG;
  }
  if (nuc_dst_dev && p->args.total_nuc && (p->args.outputs & MAGOT_OUT_NUC)) {
    if (p->genome_order) {
      if (int rc = plan_reassemble(ctx, p, false, nuc_dst_dev)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(nuc_dst_dev, p->args.nuc, p->args.total_nuc,
                                   hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  if (pep_dst_dev && p->args.total_pep && (p->args.outputs & MAGOT_OUT_PEP)) {
    if (p->genome_order) {
      if (int rc = plan_reassemble(ctx, p, true, pep_dst_dev)) return rc;
    } else {
      MAGOT_HIP_TRY(hipMemcpyAsync(pep_dst_dev, p->args.pep, p->args.total_pep,
                                   hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

int magot_plan_layout(const magot_plan* p, uint64_t* nuc_start, uint64_t* pep_start) {
  if (!p) {
    set_error("magot_plan_layout: null plan");
    return MAGOT_ERR_ARG;
  }
  const uint64_t T = p->n_tx;
  if (nuc_start) {
    if (p->genome_order) std::memcpy(nuc_start, p->lay_nuc.data(), T * 8);
    else std::memcpy(nuc_start, p->nuc_off.data(), T * 8);
  }
  if (pep_start) {
    if (p->genome_order) std::memcpy(pep_start, p->lay_pep.data(), T * 8);
    else std::memcpy(pep_start, p->pep_off.data(), T * 8);
  }
  return MAGOT_OK;
}

int magot_plan_device_outputs(magot_plan* p, void** nuc_dev, void** pep_dev) {
  if (!p) {
    set_error("magot_plan_device_outputs: null plan");
    return MAGOT_ERR_ARG;
  }
  if (nuc_dev) *nuc_dev = p->args.nuc;
  if (pep_dev) *pep_dev = p->args.pep;
  return MAGOT_OK;
}

uint64_t magot_plan_algorithmic_bytes(const magot_plan* p) {
  if (!p) return 0;
  const uint64_t B = p->args.total_nuc, P = p->args.total_pep;
  uint64_t bytes = (B + 3) / 4 + 16 * p->n_exons + 32 * p->n_tx;
  if (p->args.outputs & MAGOT_OUT_NUC) bytes += B;
  if (p->args.outputs & MAGOT_OUT_PEP) bytes += P;
  return bytes;
}

int magot_revcomp_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                        uint8_t* out) {
  if (int rc = bind(ctx)) return rc;
  if (!seq_off) {
    set_error("magot_revcomp_batch: null argument");
    return MAGOT_ERR_ARG;
  }
  const uint64_t total = n ? seq_off[n] : 0;
  if (total == 0) return MAGOT_OK;  // empty strings only: nothing to read or write
  if (!seqs || !out) {
    set_error("magot_revcomp_batch: null argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (seq_off[i + 1] < seq_off[i]) {
      set_error("magot_revcomp_batch: offsets not monotone");
      return MAGOT_ERR_ARG;
    }
  void* d = nullptr;
  const uint64_t off_bytes = (n + 1) * 8, pad = 64;
  MAGOT_HIP_TRY(hipMalloc(&d, 2 * (total + pad) + off_bytes));
  uint8_t* d_in = static_cast<uint8_t*>(d);
  uint8_t* d_out = d_in + total + pad;
  uint64_t* d_off = reinterpret_cast<uint64_t*>(d_out + total + pad);
  int rc = MAGOT_OK;
  hipError_t e = hipMemcpyAsync(d_in, seqs, total, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_off, seq_off, off_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_revcomp(d_in, d_off, n, total, d_out, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    set_error(std::string("magot_revcomp_batch: ") + hipGetErrorString(e));
    rc = MAGOT_ERR_HIP;
  }
  (void)hipFree(d);
  return rc;
}

int magot_translate_sizes(const uint64_t* seq_off, uint64_t n, const int32_t* frames,
                          uint64_t* pep_off, int64_t* codons_out) {
  if (!seq_off || !pep_off || (n && !frames)) {
    set_error("magot_translate_sizes: null argument");
    return MAGOT_ERR_ARG;
  }
  uint64_t acc = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const int64_t f = frames[i];
    if (f < 0) {
      set_error("magot_translate_sizes: negative frame");
      return MAGOT_ERR_ARG;
    }
    const int64_t L = (int64_t)(seq_off[i + 1] - seq_off[i]);
    int64_t c = -1;
    if (L > 2 + f) {
      const int64_t pe = f + ((2 - 2 * f) % 3 + 3) % 3;
      c = 1 + (L - 1 - pe) / 3;
    }
    pep_off[i] = acc;
    if (codons_out) codons_out[i] = c;
    if (c > 0) acc += (uint64_t)c;
  }
  pep_off[n] = acc;
  return MAGOT_OK;
}

int magot_translate_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                          const int32_t* frames, const uint8_t* strands, const uint8_t* lut64,
                          const uint64_t* pep_off, uint8_t* out) {
  if (int rc = bind(ctx)) return rc;
  if (!seq_off || !pep_off || (n && (!frames || !strands))) {
    set_error("magot_translate_batch: null argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (strands[i] != '+' && strands[i] != '-') {
      set_error("magot_translate_batch: strand must be '+' or '-'");
      return MAGOT_ERR_ARG;
    }
  const uint64_t total = n ? seq_off[n] : 0, total_pep = n ? pep_off[n] : 0;
  if (total_pep == 0) return MAGOT_OK;
  if (!seqs || !out) {
    set_error("magot_translate_batch: null buffer");
    return MAGOT_ERR_ARG;
  }
  uint8_t lut[64];
  if (lut64) std::memcpy(lut, lut64, 64);
  else standard_lut(lut);
  uint32_t lut16[16];
  std::memcpy(lut16, lut, 64);
  const uint64_t pad = 64, ob = (n + 1) * 8;
  const uint64_t bytes = (total + pad) + (total_pep + pad) + 2 * ob + n * 4 + n + pad;
  void* d = nullptr;
  MAGOT_HIP_TRY(hipMalloc(&d, bytes));
  uint8_t* d_in = static_cast<uint8_t*>(d);
  uint8_t* d_out = d_in + total + pad;
  uint64_t* d_off = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(d_out + total_pep + pad) + 7) & ~7ull);
  uint64_t* d_poff = d_off + (n + 1);
  int32_t* d_fr = reinterpret_cast<int32_t*>(d_poff + (n + 1));
  uint8_t* d_st = reinterpret_cast<uint8_t*>(d_fr + n);
  hipError_t e = hipSuccess;
  if (total) e = hipMemcpyAsync(d_in, seqs, total, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off, seq_off, ob, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_poff, pep_off, ob, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_fr, frames, n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_st, strands, n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_translate(d_in, d_off, n, d_fr, d_st, d_poff, total_pep, lut16, d_out, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, total_pep, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  int rc = MAGOT_OK;
  if (e != hipSuccess) {
    set_error(std::string("magot_translate_batch: ") + hipGetErrorString(e));
    rc = MAGOT_ERR_HIP;
  }
  (void)hipFree(d);
  return rc;
}

int magot_codon_symbols(magot_ctx* ctx, const uint8_t* seq, uint64_t n_codons,
                        const uint8_t* class256, uint32_t n_classes, const uint8_t* lut,
                        uint8_t* out) {
  if (int rc = bind(ctx)) return rc;
  const uint64_t nl = (uint64_t)n_classes * n_classes * n_classes;
  if (!class256 || !lut || n_classes == 0 || nl > kMaxSymbolLut || (n_codons && (!seq || !out))) {
    set_error("magot_codon_symbols: bad argument");
    return MAGOT_ERR_ARG;
  }
  for (int b = 0; b < 256; ++b)
    if (class256[b] >= n_classes) {
      set_error("magot_codon_symbols: class out of range");
      return MAGOT_ERR_ARG;
    }
  if (n_codons == 0) return MAGOT_OK;
  const uint64_t in_bytes = 3 * n_codons;
  void* d = nullptr;
  MAGOT_HIP_TRY(hipMalloc(&d, in_bytes + n_codons + 256 + nl + 64));
  uint8_t* d_in = static_cast<uint8_t*>(d);
  uint8_t* d_out = d_in + in_bytes;
  uint8_t* d_cls = d_out + n_codons;
  uint8_t* d_lut = d_cls + 256;
  hipError_t e = hipMemcpyAsync(d_in, seq, in_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cls, class256, 256, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_lut, lut, nl, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_codon_symbols(d_in, n_codons, d_cls, n_classes, d_lut, d_out, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n_codons, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error(std::string("magot_codon_symbols: ") + hipGetErrorString(e));
    return MAGOT_ERR_HIP;
  }
  return MAGOT_OK;
}

// --- single sequences (SURVEY 8(b) sketch) ---------------------------------

int magot_revcomp(magot_ctx* ctx, const uint8_t* seq, uint64_t len, uint8_t* out) {
  const uint64_t off[2] = {0, len};
  return magot_revcomp_batch(ctx, seq, off, 1, out);
}

int magot_translate(magot_ctx* ctx, const uint8_t* seq, uint64_t len, int frame, int strand,
                    int trimX, uint8_t* out, int64_t* out_len) {
  if (!out_len || (len && !seq)) {
    set_error("magot_translate: null argument");
    return MAGOT_ERR_ARG;
  }
  if (strand != '+' && strand != '-') {
    set_error("magot_translate: strand must be '+' or '-'");
    return MAGOT_ERR_ARG;
  }
  if (frame < 0) {
    set_error("magot_translate: negative frame (the Python layer lays those out itself)");
    return MAGOT_ERR_UNSUPPORTED;
  }
  const uint64_t off[2] = {0, len};
  const int32_t fr = frame;
  uint64_t poff[2];
  int64_t codons = 0;
  if (int rc = magot_translate_sizes(off, 1, &fr, poff, &codons)) return rc;
  if (codons < 0) {  // translate() returns None (len <= 2 + frame)
    *out_len = -1;
    return MAGOT_OK;
  }
  if (codons && !out) {
    set_error("magot_translate: null output");
    return MAGOT_ERR_ARG;
  }
  const uint8_t st = (uint8_t)strand;
  // translated into a private buffer, so exactly *out_len bytes reach `out`
  std::vector<uint8_t> tmp((size_t)codons + 1);
  if (int rc = magot_translate_batch(ctx, seq, off, 1, &fr, &st, nullptr, poff, tmp.data()))
    return rc;
  int64_t n = codons;
  const uint8_t* res = tmp.data();
  if (trimX && n > 0 && res[0] == 'X') {  // genome.py:819-821
    ++res;
    --n;
  }
  if (n) std::memcpy(out, res, (size_t)n);
  *out_len = n;
  return MAGOT_OK;
}

// --- six-frame translation (Sequence.get_orfs, genome.py:824-851) ----------

int magot_orf6_sizes(const uint64_t* seq_off, uint64_t n, uint64_t* stream_off,
                     uint64_t* stream_len, uint8_t* none_mask) {
  if (!seq_off || !stream_off) {
    set_error("magot_orf6_sizes: null argument");
    return MAGOT_ERR_ARG;
  }
  // A record's streams are placed strand-major: its three '-' streams, then
  // its three '+' streams.  orf6_kernel writes every '-' chunk of a record
  // batch before its '+' chunks (strand-uniform chunk passes), so each pass
  // then stores one contiguous run per record instead of three runs with
  // gaps the other pass fills later (whose shared 128-B lines leave L2 half
  // written).
  uint64_t acc = 0;
  for (uint64_t r = 0; r < n; ++r) {
    const uint64_t L = seq_off[r + 1] - seq_off[r];
    for (int st = 0; st < 2; ++st) {
      for (uint32_t f = 0; f < 3; ++f) {
        // real codons start at 2f, 2f+3, ... (frames 1/2 emit a junk codon first)
        const bool none = L <= 2 + f;
        const uint64_t c = (!none && L >= 2 * f + 3) ? (L - 2 * f) / 3 : 0;
        const uint64_t j = 6 * r + 2 * f + st;
        stream_off[j] = acc;  // streams start on 16-byte boundaries
        if (stream_len) stream_len[j] = c;
        if (none_mask) none_mask[j] = none ? 1 : 0;
        acc += (c + 15) & ~15ull;
      }
    }
  }
  stream_off[6 * n] = acc;
  return MAGOT_OK;
}

int magot_orf6_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                     const uint8_t* lut64, const uint64_t* stream_off, uint8_t* out) {
  if (int rc = bind(ctx)) return rc;
  if (!seq_off || !stream_off) {
    set_error("magot_orf6_batch: null argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t r = 0; r < n; ++r)
    if (seq_off[r + 1] < seq_off[r]) {
      set_error("magot_orf6_batch: seq_off must be non-decreasing");
      return MAGOT_ERR_ARG;
    }
  {
    // the kernel places each stream from its record's block start and length
    // (magot_orf6_sizes' layout); a different table would send its stores
    // past the caller's buffer, so it is refused
    std::vector<uint64_t> want(6 * n + 1);
    magot_orf6_sizes(seq_off, n, want.data(), nullptr, nullptr);
    if (std::memcmp(want.data(), stream_off, want.size() * 8) != 0) {
      set_error("magot_orf6_batch: stream_off is not magot_orf6_sizes' table for seq_off");
      return MAGOT_ERR_ARG;
    }
  }
  const uint64_t total = n ? seq_off[n] : 0, total_res = n ? stream_off[6 * n] : 0;
  if (total_res == 0) return MAGOT_OK;
  if (!seqs || !out) {
    set_error("magot_orf6_batch: null buffer");
    return MAGOT_ERR_ARG;
  }
  uint8_t lut[64], tables[256];
  if (lut64) std::memcpy(lut, lut64, 64);
  else standard_lut(lut);
  orf6_tables(lut, tables);
  Orf6Tiles tiles;
  orf6_plan_tiles(seq_off, n, nullptr, 0, &tiles);
  const uint64_t n_tiles = tiles.r0.size();
  Carve cv;
  const uint64_t o_in = cv.take<uint8_t>(total + 64);
  const uint64_t o_out = cv.take<uint8_t>(total_res + 64);
  const uint64_t o_off = cv.take<uint64_t>(n + 1);
  const uint64_t o_boff = cv.take<uint64_t>(n + 1);
  const uint64_t o_t0 = cv.take<uint64_t>(n_tiles + 1);
  const uint64_t o_r0 = cv.take<uint32_t>(n_tiles);
  const uint64_t o_lut = cv.take<uint8_t>(256);
  void* d = nullptr;
  MAGOT_HIP_TRY(hipMalloc(&d, cv.used));
  char* base = static_cast<char*>(d);
  hipError_t e = hipMemcpyAsync(base + o_in, seqs, total, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(base + o_lut, tables, 256, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(base + o_off, seq_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
  // the kernel takes each record's block start (its streams' places follow
  // from the record length, magot_orf6_sizes' layout)
  std::vector<uint64_t> boff(n + 1);
  for (uint64_t r = 0; r <= n; ++r) boff[r] = stream_off[6 * r];
  if (e == hipSuccess)
    e = hipMemcpyAsync(base + o_boff, boff.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(base + o_t0, tiles.t0.data(), (n_tiles + 1) * 8, hipMemcpyHostToDevice,
                       ctx->stream);
  if (e == hipSuccess && n_tiles)
    e = hipMemcpyAsync(base + o_r0, tiles.r0.data(), n_tiles * 4, hipMemcpyHostToDevice,
                       ctx->stream);
  if (e == hipSuccess) {
    Orf6Args a{};
    a.nuc = reinterpret_cast<const uint8_t*>(base + o_in);
    a.noff = reinterpret_cast<const uint64_t*>(base + o_off);
    a.n_rec = n;
    a.total = total;
    a.boff = reinterpret_cast<const uint64_t*>(base + o_boff);
    a.tile_t0 = reinterpret_cast<const uint64_t*>(base + o_t0);
    a.tile_r0 = reinterpret_cast<const uint32_t*>(base + o_r0);
    a.n_tiles = n_tiles;
    a.tables = reinterpret_cast<const uint8_t*>(base + o_lut);
    a.out = reinterpret_cast<uint8_t*>(base + o_out);
    launch_orf6(a, false, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, base + o_out, total_res, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  int rc = MAGOT_OK;
  if (e != hipSuccess) {
    set_error(std::string("magot_orf6_batch: ") + hipGetErrorString(e));
    rc = MAGOT_ERR_HIP;
  }
  (void)hipFree(d);
  return rc;
}

// Six frames over an extraction plan: the records are gathered from the
// genome plane through the plan's intervals inside the kernel (fused; the
// plan's nucleotide output is not read).
struct magot_orf6 {
  magot_ctx* ctx = nullptr;
  magot_plan* plan = nullptr;
  void* arena = nullptr;
  Orf6Args args{};
  uint8_t* out = nullptr;
  uint64_t n_rec = 0, total = 0;
  std::vector<uint64_t> host_soff;
  bool executed = false;  // the streams are in HBM (magot_orfcall_create asks)
  void launch(hipStream_t s) const { launch_orf6(args, true, s); }
};

int magot_plan_orf6(magot_ctx* ctx, magot_plan* p, const uint8_t* lut64, magot_orf6** out,
                    uint64_t* total_res) {
  if (int rc = bind(ctx)) return rc;
  if (!p || !out) {
    set_error("magot_plan_orf6: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (p->genome_order) {
    // the six-frame plan walks the plan's intervals against record-order
    // offsets (and lays its own walk out in genome order anyway)
    set_error("magot_plan_orf6: plan built with MAGOT_OUT_GENOME_ORDER (build it without)");
    return MAGOT_ERR_ARG;
  }
  std::unique_ptr<magot_orf6> o(new magot_orf6());
  o->ctx = ctx;
  o->plan = p;
  o->n_rec = p->n_tx;
  o->host_soff.resize(6 * o->n_rec + 1);
  if (int rc = magot_orf6_sizes(p->nuc_off.data(), o->n_rec, o->host_soff.data(), nullptr, nullptr))
    return rc;
  o->total = o->host_soff.back();
  const uint64_t total_nuc = p->nuc_off.back();
  // interval rows {unified anchor, start} from the plan's compacted table
  // (a '-' interval reads the mirror plane forward; staging every interval
  // from the forward planes instead, '-' read backwards and reverse-
  // complemented in registers, measured 5 % slower: DESIGN.md 4, round 4)
  const uint64_t ne = p->n_ex_c;
  const uint64_t* const ex_g = p->host_ex_g.get();
  const uint64_t* const ex_out = p->host_ex_out.get();
  std::vector<uint64_t> rows(2 * (ne + 1));
  const uint64_t span = p->args.span;
  std::vector<uint64_t> starts(ne + 1);
  for (uint64_t i = 0; i < ne; ++i) {
    const uint64_t gw = ex_g[i], o0 = ex_out[i], len = ex_out[i + 1] - o0;
    const uint64_t gs = gw & ~kExFlagBits;
    rows[2 * i] = (gw & kRcBit) ? 2 * span - gs - len - o0 : gs - o0;
    rows[2 * i + 1] = o0 | ((gw & kExcBit) ? kOrf6ExcRow : 0ull);  // the exact path's flag
    starts[i] = o0;
  }
  rows[2 * ne] = 0;
  rows[2 * ne + 1] = total_nuc;
  starts[ne] = total_nuc;
  // Processing order.  The kernel walks a concatenation of the records; every
  // stream is found through its offset, so the walk may follow the genome
  // instead: records sorted by the plane position of their first interval
  // put neighbouring loci into concurrently running tiles (one XCD sweeps one
  // contiguous range), whose plane reads then share L2 lines.  The records'
  // six-stream blocks are laid out in the same walk order, so each XCD's
  // stores advance through one contiguous stretch of the output (record
  // order would scatter them in ~2 KB runs); magot_orf6_fetch returns every
  // stream's offset.  MAGOT_ORF6_ORDER=record keeps record order (walk and
  // layout).
  std::vector<uint64_t> noff_k, soff_k;
  uint64_t ne_k = ne;
  {
    const char* env = getenv("MAGOT_ORF6_ORDER");
    const bool genome_order = !(env && std::strcmp(env, "record") == 0);
    const uint64_t n = o->n_rec;
    const uint64_t* noff = p->nuc_off.data();
    if (genome_order && ne && n > 1) {
      std::vector<uint64_t> ie(n + 1), key(n), perm(n);
      uint64_t i = 0;
      for (uint64_t r = 0; r < n; ++r) {  // record r's intervals: [ie[r], ie[r+1])
        while (i < ne && starts[i] < noff[r]) ++i;
        ie[r] = i;
      }
      ie[n] = ne;
      for (uint64_t r = 0; r < n; ++r)
        key[r] = noff[r + 1] > noff[r] && ie[r] < ie[r + 1] ? rows[2 * ie[r]] + starts[ie[r]]
                                                             : ~0ull;
      for (uint64_t r = 0; r < n; ++r) perm[r] = r;
      std::stable_sort(perm.begin(), perm.end(),
                       [&](uint64_t x, uint64_t y) { return key[x] < key[y]; });
      noff_k.resize(n + 1);
      soff_k.resize(6 * n + 1);
      std::vector<uint64_t> rows_k(2 * (ne + 1)), starts_k(ne + 1);
      uint64_t j = 0;
      noff_k[0] = 0;
      for (uint64_t k = 0; k < n; ++k) {
        const uint64_t r = perm[k];
        noff_k[k + 1] = noff_k[k] + (noff[r + 1] - noff[r]);
        for (uint64_t e = ie[r]; e < ie[r + 1]; ++e) {
          const uint64_t st = starts[e];
          if (starts[e + 1] == st || st >= noff[r + 1]) continue;  // empty
          // the remap assumes no compacted interval crosses a record end
          // (compaction only drops empty intervals, magot_plan_create)
          if (starts[e + 1] > noff[r + 1]) {
            set_error("magot_plan_orf6: an interval crosses the end of its record");
            return MAGOT_ERR_STATE;
          }
          const uint64_t st_k = noff_k[k] + (st - noff[r]);
          rows_k[2 * j] = rows[2 * e] + st - st_k;  // the same unified anchor
          rows_k[2 * j + 1] = st_k | (rows[2 * e + 1] & kOrf6ExcRow);
          starts_k[j] = st_k;
          ++j;
        }
      }
      // the blocks in walk order; the fetch table maps record r's streams there
      if (int rc = magot_orf6_sizes(noff_k.data(), n, soff_k.data(), nullptr, nullptr)) return rc;
      for (uint64_t k = 0; k < n; ++k)
        for (int s = 0; s < 6; ++s) o->host_soff[6 * perm[k] + s] = soff_k[6 * k + s];
      o->host_soff[6 * n] = soff_k[6 * n];
      rows_k[2 * j] = 0;
      rows_k[2 * j + 1] = total_nuc;
      starts_k[j] = total_nuc;
      rows_k.resize(2 * (j + 1));
      starts_k.resize(j + 1);
      rows.swap(rows_k);
      starts.swap(starts_k);
      ne_k = j;
    } else {
      noff_k.assign(noff, noff + n + 1);
      soff_k = o->host_soff;
    }
  }
  Orf6Tiles tiles;
  orf6_plan_tiles(noff_k.data(), o->n_rec, starts.data(), ne_k, &tiles);
  const uint64_t n_tiles = tiles.r0.size();
  uint8_t lut[64], tables[256];
  if (lut64) std::memcpy(lut, lut64, 64);
  else standard_lut(lut);
  orf6_tables(lut, tables);
  Carve cv;
  const uint64_t o_off = cv.take<uint64_t>(o->n_rec + 1);
  const uint64_t o_boff = cv.take<uint64_t>(o->n_rec + 1);
  const uint64_t o_out = cv.take<uint8_t>(o->total + 64);
  const uint64_t o_rows = cv.take<uint64_t>(2 * (ne_k + 1));
  const uint64_t o_t0 = cv.take<uint64_t>(n_tiles + 1);
  const uint64_t o_r0 = cv.take<uint32_t>(n_tiles);
  const uint64_t o_e0 = cv.take<uint32_t>(n_tiles);
  const uint64_t o_m = cv.take<uint32_t>(n_tiles);
  const uint64_t o_lut = cv.take<uint8_t>(256);
  const uint64_t nib_words = p->args.span / 4;  // forward + reverse planes, 8 bases per word
  const uint64_t code2_words = nib_words / 2;
  const uint64_t o_code2 = cv.take<uint32_t>(code2_words + 4);
  const uint64_t exc1_words = nib_words / 4;
  const uint64_t o_exc1 = cv.take<uint32_t>(exc1_words + 4);
  MAGOT_HIP_TRY(hipMalloc(&o->arena, cv.used));
  char* base = static_cast<char*>(o->arena);
  auto up = [&](uint64_t off, const void* src, uint64_t bytes) {
    return bytes ? hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  uint32_t* code2 = reinterpret_cast<uint32_t*>(base + o_code2);
  uint32_t* exc1 = reinterpret_cast<uint32_t*>(base + o_exc1);
  launch_code2(p->args.nib, nib_words, code2, ctx->stream);
  launch_exc1(p->args.nib, nib_words, exc1, ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(up(o_off, noff_k.data(), (o->n_rec + 1) * 8));
  std::vector<uint64_t> boff_k(o->n_rec + 1);  // block starts in walk order
  for (uint64_t k = 0; k <= o->n_rec; ++k) boff_k[k] = soff_k[6 * k];
  MAGOT_HIP_TRY(up(o_boff, boff_k.data(), (o->n_rec + 1) * 8));
  MAGOT_HIP_TRY(up(o_rows, rows.data(), rows.size() * 8));
  MAGOT_HIP_TRY(up(o_t0, tiles.t0.data(), (n_tiles + 1) * 8));
  MAGOT_HIP_TRY(up(o_r0, tiles.r0.data(), n_tiles * 4));
  MAGOT_HIP_TRY(up(o_e0, tiles.e0.data(), n_tiles * 4));
  MAGOT_HIP_TRY(up(o_m, tiles.m.data(), n_tiles * 4));
  MAGOT_HIP_TRY(up(o_lut, tables, 256));
  o->out = reinterpret_cast<uint8_t*>(base + o_out);
  Orf6Args& a = o->args;
  a.nib = p->args.nib;
  a.nib_words = nib_words;
  a.code2 = code2;
  a.code2_words = code2_words;
  a.exc1 = exc1;
  a.exc1_words = exc1_words;
  a.rows = reinterpret_cast<const uint64_t*>(base + o_rows);
  a.n_rows = ne_k;
  a.noff = reinterpret_cast<const uint64_t*>(base + o_off);
  a.n_rec = o->n_rec;
  a.total = total_nuc;
  a.boff = reinterpret_cast<const uint64_t*>(base + o_boff);
  a.tile_t0 = reinterpret_cast<const uint64_t*>(base + o_t0);
  a.tile_r0 = reinterpret_cast<const uint32_t*>(base + o_r0);
  a.tile_e0 = reinterpret_cast<const uint32_t*>(base + o_e0);
  a.tile_m = reinterpret_cast<const uint32_t*>(base + o_m);
  a.n_tiles = n_tiles;
  a.tables = reinterpret_cast<const uint8_t*>(base + o_lut);
  a.out = o->out;
  if (total_res) *total_res = o->total;
  *out = o.release();
  return MAGOT_OK;
}

int magot_orf6_execute(magot_ctx* ctx, magot_orf6* o) {
  if (int rc = bind(ctx)) return rc;
  if (!o) {
    set_error("magot_orf6_execute: null handle");
    return MAGOT_ERR_ARG;
  }
  o->launch(ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  o->executed = true;
  return MAGOT_OK;
}

int magot_orf6_fetch(magot_ctx* ctx, magot_orf6* o, uint8_t* out, uint64_t* stream_off,
                     uint64_t* stream_len) {
  if (int rc = bind(ctx)) return rc;
  if (!o) {
    set_error("magot_orf6_fetch: null handle");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (out && o->total) MAGOT_HIP_TRY(hipMemcpy(out, o->out, o->total, hipMemcpyDeviceToHost));
  if (stream_off)
    std::memcpy(stream_off, o->host_soff.data(), o->host_soff.size() * sizeof(uint64_t));
  if (stream_len) {
    std::vector<uint64_t> tmp(6 * o->n_rec + 1);
    return magot_orf6_sizes(o->plan->nuc_off.data(), o->n_rec, tmp.data(), stream_len, nullptr);
  }
  return MAGOT_OK;
}

int magot_orf6_copy_outputs(magot_ctx* ctx, magot_orf6* o, void* dst_dev) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !dst_dev) {
    set_error("magot_orf6_copy_outputs: null argument");
    return MAGOT_ERR_ARG;
  }
  if (o->total)
    MAGOT_HIP_TRY(hipMemcpyAsync(dst_dev, o->out, o->total, hipMemcpyDeviceToDevice, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MAGOT_OK;
}

int magot_orf6_time(magot_ctx* ctx, magot_orf6* o, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !avg_ms || iters <= 0) {
    set_error("magot_orf6_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  double total = 0;
  for (int i = 0; i < iters; ++i) {
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    o->launch(ctx->stream);
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0;
    MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total += ms;
  }
  o->executed = true;
  *avg_ms = total / iters;
  return MAGOT_OK;
}

int magot_orf6_time_b2b(magot_ctx* ctx, magot_orf6* o, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !avg_ms || iters <= 0) {
    set_error("magot_orf6_time_b2b: bad argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int i = 0; i < iters; ++i) o->launch(ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
  float ms = 0;
  MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  o->executed = true;
  *avg_ms = (double)ms / iters;
  return MAGOT_OK;
}

void magot_orf6_destroy(magot_orf6* o) {
  if (!o) return;
  if (o->ctx) (void)hipSetDevice(o->ctx->device);
  if (o->arena) (void)hipFree(o->arena);
  delete o;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// ORF calling over the six-frame streams (orfcall.hip; dna2orfs,
// genome_tools.py:145-180)
// ---------------------------------------------------------------------------

struct magot_orfcall {
  magot_ctx* ctx = nullptr;
  magot_orf6* o6 = nullptr;
  std::vector<void*> mem;   // device allocations of the calling passes
  std::vector<void*> tmem;  // of the last magot_orfcall_text
  OrfCallArgs a{};
  OrfTextArgs t{};
  uint64_t payload_bytes = 0, sel_bytes = 0, text_bytes = 0;
  bool has_text = false;
  bool longest() const { return (a.mode & MAGOT_ORF_LONGEST) != 0; }
  uint64_t rows() const { return longest() ? a.n_sel : a.n_orfs; }
};

namespace {

template <class T>
hipError_t orf_alloc(std::vector<void*>* mem, T** p, uint64_t count) {
  void* d = nullptr;
  // 64 bytes of slack: the span copies read whole 16-byte chunks around a payload
  if (hipError_t e = hipMalloc(&d, count * sizeof(T) + 64)) return e;
  mem->push_back(d);
  *p = static_cast<T*>(d);
  return hipSuccess;
}

// scan scratch for `count` elements (kept when the one at hand is large enough)
hipError_t orf_scan_tmp(std::vector<void*>* mem, void** tmp, size_t* bytes, uint64_t count) {
  const size_t need = orfcall_scan_bytes(count);
  if (*tmp && need <= *bytes) return hipSuccess;
  uint8_t* d = nullptr;
  if (hipError_t e = orf_alloc(mem, &d, need)) return e;
  *tmp = d;
  *bytes = need;
  return hipSuccess;
}

hipError_t orf_read_u64(const uint64_t* dev, uint64_t* host, hipStream_t s) {
  if (hipError_t e = hipMemcpyAsync(host, dev, 8, hipMemcpyDeviceToHost, s)) return e;
  return hipStreamSynchronize(s);
}

// every calling pass again, over the buffers magot_orfcall_create sized
hipError_t orf_run(const magot_orfcall* c, hipStream_t s) {
  if (hipError_t e = launch_orfcall_streams(c->a, s)) return e;
  if (hipError_t e = launch_orfcall_count(c->a, s)) return e;
  if (hipError_t e = launch_orfcall_write(c->a, s)) return e;
  if (!c->longest()) return hipSuccess;
  if (hipError_t e = launch_orfcall_longest(c->a, s)) return e;
  return launch_orfcall_compact(c->a, s);
}

void orf_free(std::vector<void*>* mem) {
  for (void* d : *mem) (void)hipFree(d);
  mem->clear();
}

}  // namespace

extern "C" {

uint32_t magot_orfcall_tile(void) { return kOrfCallTile; }

void magot_orfcall_destroy(magot_orfcall* c) {
  if (!c) return;
  if (c->ctx) (void)hipSetDevice(c->ctx->device);
  orf_free(&c->tmem);
  orf_free(&c->mem);
  delete c;
}

int magot_orfcall_create(magot_ctx* ctx, magot_orf6* o, uint32_t flags, magot_orfcall** out,
                         uint64_t* n_orfs, uint64_t* payload_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !out || (flags & ~(MAGOT_ORF_FROM_ATG | MAGOT_ORF_LONGEST))) {
    set_error("magot_orfcall_create: null argument or unknown flag");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (!o->executed) {
    set_error("magot_orfcall_create: execute the six-frame plan first");
    return MAGOT_ERR_STATE;
  }
  const uint64_t n = o->n_rec;
  if (6 * n + 1 >= (1ull << 32)) {
    set_error("magot_orfcall_create: too many records (stream indices are 32-bit)");
    return MAGOT_ERR_ARG;
  }
  struct Guard {
    magot_orfcall* c;
    ~Guard() { magot_orfcall_destroy(c); }
  } guard{new magot_orfcall()};
  magot_orfcall* c = guard.c;
  c->ctx = ctx;
  c->o6 = o;
  OrfCallArgs& a = c->a;
  hipStream_t s = ctx->stream;
  a.mode = flags;
  a.res = o->out;
  a.n_rec = n;
  uint64_t *soff = nullptr, *noff = nullptr;
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &soff, 6 * n + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &noff, n + 1));
  MAGOT_HIP_TRY(hipMemcpyAsync(soff, o->host_soff.data(), (6 * n + 1) * 8, hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(noff, o->plan->nuc_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  a.soff = soff;
  a.noff = noff;
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.scnt, 6 * n + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.tile_first, 6 * n + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.flags, n + 1));
  MAGOT_HIP_TRY(orf_scan_tmp(&c->mem, &a.scan_tmp, &a.scan_bytes, 6 * n + 1));
  MAGOT_HIP_TRY(launch_orfcall_streams(a, s));
  MAGOT_HIP_TRY(orf_read_u64(a.tile_first + 6 * n, &a.n_tiles, s));
  const uint64_t nt = a.n_tiles;
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.tile_stream, nt));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.orfs, nt + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.kept, nt + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.extra, nt));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.tflags, nt));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.tseen, nt));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.obase, nt + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.kbase, nt + 1));
  MAGOT_HIP_TRY(orf_scan_tmp(&c->mem, &a.scan_tmp, &a.scan_bytes, nt + 1));
  MAGOT_HIP_TRY(launch_orfcall_count(a, s));
  MAGOT_HIP_TRY(orf_read_u64(a.obase + nt, &a.n_orfs, s));
  MAGOT_HIP_TRY(orf_read_u64(a.kbase + nt, &c->payload_bytes, s));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.rec, a.n_orfs));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.j, a.n_orfs));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.k, a.n_orfs));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.len, a.n_orfs));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.poff, a.n_orfs));
  MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.payload, c->payload_bytes));
  MAGOT_HIP_TRY(launch_orfcall_write(a, s));
  if (c->longest()) {
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.sel, n));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.valid, n + 1));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.sellen, n + 1));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.slot, n + 1));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.cpoff, n + 1));
    MAGOT_HIP_TRY(launch_orfcall_longest(a, s));
    MAGOT_HIP_TRY(orf_read_u64(a.slot + n, &a.n_sel, s));
    MAGOT_HIP_TRY(orf_read_u64(a.cpoff + n, &c->sel_bytes, s));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.c_rec, a.n_sel));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.c_j, a.n_sel));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.c_k, a.n_sel));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.c_len, a.n_sel));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.c_poff, a.n_sel));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.c_payload, c->sel_bytes));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.src_off, a.n_sel));
    MAGOT_HIP_TRY(orf_alloc(&c->mem, &a.dst_off, a.n_sel + 1));
    MAGOT_HIP_TRY(launch_orfcall_compact(a, s));
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  if (n_orfs) *n_orfs = c->rows();
  if (payload_bytes) *payload_bytes = c->longest() ? c->sel_bytes : c->payload_bytes;
  guard.c = nullptr;
  *out = c;
  return MAGOT_OK;
}

int magot_orfcall_fetch(magot_ctx* ctx, magot_orfcall* c, uint32_t* record, uint8_t* stream,
                        uint32_t* start, uint32_t* length, uint64_t* payload_off,
                        uint8_t* payload, uint8_t* record_flags) {
  if (int rc = bind(ctx)) return rc;
  if (!c) {
    set_error("magot_orfcall_fetch: null handle");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const OrfCallArgs& a = c->a;
  const bool lg = c->longest();
  const uint64_t n = c->rows(), pb = lg ? c->sel_bytes : c->payload_bytes;
  auto down = [](void* dst, const void* src, uint64_t bytes) {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  MAGOT_HIP_TRY(down(record, lg ? a.c_rec : a.rec, n * 4));
  MAGOT_HIP_TRY(down(stream, lg ? a.c_j : a.j, n));
  MAGOT_HIP_TRY(down(start, lg ? a.c_k : a.k, n * 4));
  MAGOT_HIP_TRY(down(length, lg ? a.c_len : a.len, n * 4));
  MAGOT_HIP_TRY(down(payload_off, lg ? a.c_poff : a.poff, n * 8));
  MAGOT_HIP_TRY(down(payload, lg ? a.c_payload : a.payload, pb));
  MAGOT_HIP_TRY(down(record_flags, a.flags, a.n_rec));
  return MAGOT_OK;
}

int magot_orfcall_text(magot_ctx* ctx, magot_orfcall* c, const uint64_t* name_off,
                       const uint8_t* names, uint64_t* out_len) {
  if (int rc = bind(ctx)) return rc;
  if (!c || !name_off || !out_len) {
    set_error("magot_orfcall_text: null argument");
    return MAGOT_ERR_ARG;
  }
  const OrfCallArgs& a = c->a;
  const uint64_t n = a.n_rec, ne = c->rows();
  const bool lg = c->longest();
  // each record's header, behind the newline that ends the entry before it
  static const char kPos[] = "-pos:", kLongest[] = "_longestORF\n";
  const char* const tail = lg ? kLongest : kPos;
  const size_t tail_len = std::strlen(tail);
  std::string hdr;
  std::vector<uint64_t> hoff(n + 1);
  for (uint64_t r = 0; r < n; ++r) {
    if (name_off[r + 1] < name_off[r] || (name_off[r + 1] > name_off[r] && !names) ||
        name_off[r + 1] - name_off[r] >= (1ull << 31)) {
      set_error("magot_orfcall_text: bad name table");
      return MAGOT_ERR_ARG;
    }
    hoff[r] = hdr.size();
    hdr += "\n>";
    if (name_off[r + 1] > name_off[r])
      hdr.append(reinterpret_cast<const char*>(names) + name_off[r], name_off[r + 1] - name_off[r]);
    hdr.append(tail, tail_len);
  }
  hoff[n] = hdr.size();
  c->has_text = false;
  orf_free(&c->tmem);
  OrfTextArgs& t = c->t;
  t = OrfTextArgs{};
  hipStream_t s = ctx->stream;
  t.longest = lg;
  t.n = ne;
  t.rec = lg ? a.c_rec : a.rec;
  t.j = lg ? a.c_j : a.j;
  t.k = lg ? a.c_k : a.k;
  t.len = lg ? a.c_len : a.len;
  t.poff = lg ? a.c_poff : a.poff;
  t.payload = lg ? a.c_payload : a.payload;
  t.noff = a.noff;
  uint64_t* d_hoff = nullptr;
  MAGOT_HIP_TRY(orf_alloc(&c->tmem, &d_hoff, n + 1));
  MAGOT_HIP_TRY(hipMemcpyAsync(d_hoff, hoff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  t.hoff = d_hoff;
  t.dig_off = (hdr.size() + 15) & ~15ull;
  MAGOT_HIP_TRY(orf_alloc(&c->tmem, &t.text, t.dig_off + (lg ? 0 : kOrfDigits * ne)));
  if (!hdr.empty())
    MAGOT_HIP_TRY(hipMemcpyAsync(t.text, hdr.data(), hdr.size(), hipMemcpyHostToDevice, s));
  MAGOT_HIP_TRY(orf_alloc(&c->tmem, &t.tlen, ne + 1));
  MAGOT_HIP_TRY(orf_alloc(&c->tmem, &t.tstart, ne + 1));
  MAGOT_HIP_TRY(orf_scan_tmp(&c->tmem, &t.scan_tmp, &t.scan_bytes, ne + 1));
  MAGOT_HIP_TRY(launch_orftext_sizes(t, s));
  MAGOT_HIP_TRY(orf_read_u64(t.tstart + ne, &c->text_bytes, s));  // also: hdr is uploaded
  MAGOT_HIP_TRY(orf_alloc(&c->tmem, &t.out, c->text_bytes));
  MAGOT_HIP_TRY(launch_orftext_copy(t, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  c->has_text = true;
  *out_len = c->text_bytes;
  return MAGOT_OK;
}

int magot_orfcall_text_fetch(magot_ctx* ctx, magot_orfcall* c, uint8_t* out, uint64_t cap) {
  if (int rc = bind(ctx)) return rc;
  if (!c || !c->has_text) {
    set_error("magot_orfcall_text_fetch: call magot_orfcall_text first");
    return c ? MAGOT_ERR_STATE : MAGOT_ERR_ARG;
  }
  if (cap < c->text_bytes || (c->text_bytes && !out)) {
    set_error("magot_orfcall_text_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (c->text_bytes) MAGOT_HIP_TRY(hipMemcpy(out, c->t.out, c->text_bytes, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_orfcall_time(magot_ctx* ctx, magot_orfcall* c, int text, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!c || !avg_ms || iters <= 0) {
    set_error("magot_orfcall_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (text && !c->has_text) {
    set_error("magot_orfcall_time: call magot_orfcall_text first");
    return MAGOT_ERR_STATE;
  }
  double total = 0;
  for (int i = 0; i < iters; ++i) {
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (text) {
      MAGOT_HIP_TRY(launch_orftext_sizes(c->t, ctx->stream));
      MAGOT_HIP_TRY(launch_orftext_copy(c->t, ctx->stream));
    } else {
      MAGOT_HIP_TRY(orf_run(c, ctx->stream));
    }
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0;
    MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total += ms;
  }
  *avg_ms = total / iters;
  return MAGOT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// FASTA text assembly on device (render.hip)
// ---------------------------------------------------------------------------

struct magot_fasta_text {
  magot_ctx* ctx = nullptr;
  const magot_plan* plan = nullptr;
  void* arena = nullptr;
  const TextUnit* units = nullptr;
  const uint64_t* roff = nullptr;
  const uint8_t* text = nullptr;
  uint64_t* len = nullptr;
  uint64_t* psrc = nullptr;  // each unit's payload start in the plan's buffer
  uint64_t* end = nullptr;
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  uint8_t* out = nullptr;
  uint64_t n_units = 0, cap = 0;
  int protein = 0;
  void launch(hipStream_t s) const {
    launch_text_assembly(units, n_units, roff, protein ? plan->args.pep : plan->args.nuc,
                         protein, text, len, psrc, end, scan_tmp, scan_bytes, out, s);
  }
};

extern "C" {

int magot_fasta_text_create(magot_ctx* ctx, const magot_gffplan* gp, const magot_plan* p,
                            magot_fasta_text** out, uint64_t* max_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!gp || !p || !out) {
    set_error("magot_fasta_text_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  const std::string* text = nullptr;
  std::vector<TextUnit> units;
  bool protein = false;
  uint64_t n_rec = 0;
  if (!gffplan_units(gp, &text, &units, &protein, &n_rec)) {
    set_error("magot_fasta_text_create: too many records, or longest=True protein choices "
              "(magot_gffplan_selections; render those on the host)");
    return MAGOT_ERR_ARG;
  }
  if (n_rec != p->n_tx || !(p->args.outputs & (protein ? MAGOT_OUT_PEP : MAGOT_OUT_NUC))) {
    set_error("magot_fasta_text_create: the plan was not built from this skeleton's tables");
    return MAGOT_ERR_ARG;
  }
  std::unique_ptr<magot_fasta_text> o(new magot_fasta_text());
  o->ctx = ctx;
  o->plan = p;
  o->protein = protein;
  o->n_units = units.size();
  // each record's {start, end} in the plan's device buffer (its layout order)
  const std::vector<uint64_t>& roff = protein ? p->pep_off : p->nuc_off;
  const std::vector<uint64_t>& lay = p->genome_order ? (protein ? p->lay_pep : p->lay_nuc) : roff;
  std::vector<uint64_t> span(2 * n_rec);
  for (uint64_t r = 0; r < n_rec; ++r) {
    span[2 * r] = lay[r];
    span[2 * r + 1] = lay[r] + (roff[r + 1] - roff[r]);
  }
  o->cap = text->size() + (roff.empty() ? 0 : roff.back());
  o->scan_bytes = text_scan_bytes(o->n_units);
  Carve cv;
  const uint64_t o_units = cv.take<TextUnit>(o->n_units);
  const uint64_t o_roff = cv.take<uint64_t>(span.size());
  const uint64_t o_text = cv.take<uint8_t>(text->size());
  const uint64_t o_len = cv.take<uint64_t>(o->n_units);
  const uint64_t o_psrc = cv.take<uint64_t>(o->n_units);
  const uint64_t o_end = cv.take<uint64_t>(o->n_units);
  const uint64_t o_tmp = cv.take<uint8_t>(o->scan_bytes);
  const uint64_t o_out = cv.take<uint8_t>(o->cap);
  MAGOT_HIP_TRY(hipMalloc(&o->arena, cv.used));
  char* base = static_cast<char*>(o->arena);
  o->units = reinterpret_cast<const TextUnit*>(base + o_units);
  o->roff = reinterpret_cast<const uint64_t*>(base + o_roff);
  o->text = reinterpret_cast<const uint8_t*>(base + o_text);
  o->len = reinterpret_cast<uint64_t*>(base + o_len);
  o->psrc = reinterpret_cast<uint64_t*>(base + o_psrc);
  o->end = reinterpret_cast<uint64_t*>(base + o_end);
  o->scan_tmp = base + o_tmp;
  o->out = reinterpret_cast<uint8_t*>(base + o_out);
  if (!units.empty())
    MAGOT_HIP_TRY(hipMemcpy(base + o_units, units.data(), units.size() * sizeof(TextUnit),
                            hipMemcpyHostToDevice));
  if (!span.empty())
    MAGOT_HIP_TRY(hipMemcpy(base + o_roff, span.data(), span.size() * 8, hipMemcpyHostToDevice));
  if (!text->empty())
    MAGOT_HIP_TRY(hipMemcpy(base + o_text, text->data(), text->size(), hipMemcpyHostToDevice));
  if (max_bytes) *max_bytes = o->cap;
  *out = o.release();
  return MAGOT_OK;
}

int magot_fasta_text_execute(magot_ctx* ctx, magot_fasta_text* o) {
  if (int rc = bind(ctx)) return rc;
  if (!o) {
    set_error("magot_fasta_text_execute: null handle");
    return MAGOT_ERR_ARG;
  }
  if (!o->plan->executed) {
    set_error("magot_fasta_text_execute: execute the extraction plan first");
    return MAGOT_ERR_ARG;
  }
  o->launch(ctx->stream);
  MAGOT_HIP_TRY(hipGetLastError());
  return MAGOT_OK;
}

int magot_fasta_text_fetch(magot_ctx* ctx, magot_fasta_text* o, uint8_t* out, uint64_t cap,
                           uint64_t* out_len) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !out_len) {
    set_error("magot_fasta_text_fetch: null argument");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  uint64_t n = 0;
  if (o->n_units)
    MAGOT_HIP_TRY(hipMemcpy(&n, o->end + o->n_units - 1, 8, hipMemcpyDeviceToHost));
  *out_len = n;
  if (!out) return MAGOT_OK;
  if (cap < n) {
    set_error("magot_fasta_text_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  if (n) MAGOT_HIP_TRY(hipMemcpy(out, o->out, n, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_fasta_text_time(magot_ctx* ctx, magot_fasta_text* o, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !avg_ms || iters <= 0) {
    set_error("magot_fasta_text_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  double total = 0;
  for (int i = 0; i < iters; ++i) {
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    o->launch(ctx->stream);
    MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0;
    MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total += ms;
  }
  *avg_ms = total / iters;
  return MAGOT_OK;
}

void magot_fasta_text_destroy(magot_fasta_text* o) {
  if (!o) return;
  if (o->ctx) (void)hipSetDevice(o->ctx->device);
  if (o->arena) (void)hipFree(o->arena);
  delete o;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// mask_from_gff on the device (maskgen.hip; genome_tools.py:394-428)
// ---------------------------------------------------------------------------

struct magot_mask {
  magot_ctx* ctx = nullptr;
  const magot_plan* plan = nullptr;
  void* arena = nullptr;
  MaskArgs a{};
};

extern "C" {

void magot_mask_destroy(magot_mask* m) {
  if (!m) return;
  if (m->ctx) (void)hipSetDevice(m->ctx->device);
  if (m->arena) (void)hipFree(m->arena);
  delete m;
}

int magot_mask_create(magot_ctx* ctx, const magot_plan* p, const magot_maskplan* mp,
                      const uint32_t* rec_contig, const uint64_t* name_off, const uint8_t* names,
                      magot_mask** out, uint64_t* text_bytes) {
  if (int rc = bind(ctx)) return rc;
  if (!p || !mp || !out || (p->n_tx && (!rec_contig || !name_off))) {
    set_error("magot_mask_create: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  const uint64_t n = p->n_tx, nc = mp->contig_lens.size();
  if (!(p->args.outputs & MAGOT_OUT_NUC) || n != nc || n >= (1ull << 32)) {
    set_error("magot_mask_create: the plan must be a nucleotide plan with one record per contig");
    return MAGOT_ERR_ARG;
  }
  // each record's place in the plan's buffer; each contig's through its record
  const std::vector<uint64_t>& lay = p->genome_order ? p->lay_nuc : p->nuc_off;
  const uint64_t kNone = ~0ull;
  std::vector<uint64_t> contig_src(nc, kNone), tstart(n + 1), rsrc(n), hoff(n);
  std::vector<uint32_t> hlen(n);
  std::string hdr;
  uint64_t at = 0;
  for (uint64_t r = 0; r < n; ++r) {
    const uint32_t c = rec_contig[r];
    const uint64_t len = p->nuc_off[r + 1] - p->nuc_off[r];
    if (c >= nc || contig_src[c] != kNone || len != mp->contig_lens[c]) {
      set_error("magot_mask_create: record " + std::to_string(r) +
                " is not one whole contig of the mask plan, or its contig has a record already");
      return MAGOT_ERR_ARG;
    }
    if (name_off[r + 1] < name_off[r] || (name_off[r + 1] > name_off[r] && !names) ||
        name_off[r + 1] - name_off[r] >= (1ull << 31)) {
      set_error("magot_mask_create: bad name table");
      return MAGOT_ERR_ARG;
    }
    contig_src[c] = rsrc[r] = lay[r];
    hoff[r] = hdr.size();
    hdr += '>';
    if (name_off[r + 1] > name_off[r])
      hdr.append(reinterpret_cast<const char*>(names) + name_off[r], name_off[r + 1] - name_off[r]);
    hdr += '\n';
    hlen[r] = (uint32_t)(hdr.size() - hoff[r]);
    tstart[r] = at;
    at += hlen[r] + len + 1;  // '>' name '\n' sequence '\n'
  }
  tstart[n] = at;
  const uint64_t src_bytes = p->args.total_nuc;
  for (const magot_mask_interval& iv : mp->rows)
    if (iv.contig >= nc || (uint64_t)iv.start + iv.len > mp->contig_lens[iv.contig] ||
        contig_src[iv.contig] + iv.start + iv.len > src_bytes) {
      set_error("magot_mask_create: an interval outside its contig");
      return MAGOT_ERR_RANGE;
    }
  struct Guard {
    magot_mask* m;
    ~Guard() { magot_mask_destroy(m); }
  } guard{new magot_mask()};
  magot_mask* m = guard.m;
  m->ctx = ctx;
  m->plan = p;
  MaskArgs& a = m->a;
  a.flags = mp->flags;
  a.src = p->args.nuc;
  a.src_bytes = src_bytes;
  a.n_rows = mp->rows.size();
  a.cov_words = (src_bytes + 31) / 32;
  a.n_rec = n;
  a.text_bytes = at;
  Carve cv;
  const uint64_t o_rows = cv.take<magot_mask_interval>(a.n_rows);
  const uint64_t o_csrc = cv.take<uint64_t>(nc);
  const uint64_t o_tstart = cv.take<uint64_t>(n + 1);
  const uint64_t o_rsrc = cv.take<uint64_t>(n);
  const uint64_t o_hlen = cv.take<uint32_t>(n);
  const uint64_t o_hoff = cv.take<uint64_t>(n);
  const uint64_t o_hdr = cv.take<uint8_t>(hdr.size());
  const uint64_t o_cov = cv.take<uint32_t>(a.cov_words + 1);
  const uint64_t o_out = cv.take<uint8_t>(a.text_bytes);
  MAGOT_HIP_TRY(hipMalloc(&m->arena, cv.used + 256));
  char* base = static_cast<char*>(m->arena);
  auto up = [&](uint64_t off, const void* src, uint64_t bytes) {
    return bytes ? hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  MAGOT_HIP_TRY(up(o_rows, mp->rows.data(), a.n_rows * sizeof(magot_mask_interval)));
  MAGOT_HIP_TRY(up(o_csrc, contig_src.data(), nc * 8));
  MAGOT_HIP_TRY(up(o_tstart, tstart.data(), (n + 1) * 8));
  MAGOT_HIP_TRY(up(o_rsrc, rsrc.data(), n * 8));
  MAGOT_HIP_TRY(up(o_hlen, hlen.data(), n * 4));
  MAGOT_HIP_TRY(up(o_hoff, hoff.data(), n * 8));
  MAGOT_HIP_TRY(up(o_hdr, hdr.data(), hdr.size()));
  a.rows = reinterpret_cast<const magot_mask_interval*>(base + o_rows);
  a.contig_src = reinterpret_cast<const uint64_t*>(base + o_csrc);
  a.tstart = reinterpret_cast<const uint64_t*>(base + o_tstart);
  a.rsrc = reinterpret_cast<const uint64_t*>(base + o_rsrc);
  a.hlen = reinterpret_cast<const uint32_t*>(base + o_hlen);
  a.hoff = reinterpret_cast<const uint64_t*>(base + o_hoff);
  a.hdr = reinterpret_cast<const uint8_t*>(base + o_hdr);
  a.cov = reinterpret_cast<uint32_t*>(base + o_cov);
  a.out = reinterpret_cast<uint8_t*>(base + o_out);
  if (text_bytes) *text_bytes = a.text_bytes;
  guard.m = nullptr;
  *out = m;
  return MAGOT_OK;
}

int magot_mask_execute(magot_ctx* ctx, magot_mask* m) {
  if (int rc = bind(ctx)) return rc;
  if (!m) {
    set_error("magot_mask_execute: null handle");
    return MAGOT_ERR_ARG;
  }
  if (!m->plan->executed) {
    set_error("magot_mask_execute: execute the extraction plan first");
    return MAGOT_ERR_STATE;
  }
  MAGOT_HIP_TRY(launch_mask_paint(m->a, ctx->stream));
  MAGOT_HIP_TRY(launch_mask_text(m->a, ctx->stream));
  return MAGOT_OK;
}

int magot_mask_fetch(magot_ctx* ctx, magot_mask* m, uint8_t* out, uint64_t cap) {
  if (int rc = bind(ctx)) return rc;
  if (!m || cap < m->a.text_bytes || (m->a.text_bytes && !out)) {
    set_error("magot_mask_fetch: null handle, or output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (m->a.text_bytes)
    MAGOT_HIP_TRY(hipMemcpy(out, m->a.out, m->a.text_bytes, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_mask_coverage_fetch(magot_ctx* ctx, magot_mask* m, uint32_t* words, uint64_t cap_words,
                              uint64_t* n_words) {
  if (int rc = bind(ctx)) return rc;
  if (!m) {
    set_error("magot_mask_coverage_fetch: null handle");
    return MAGOT_ERR_ARG;
  }
  if (n_words) *n_words = m->a.cov_words;
  if (!words) return MAGOT_OK;
  if (cap_words < m->a.cov_words) {
    set_error("magot_mask_coverage_fetch: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (m->a.cov_words)
    MAGOT_HIP_TRY(hipMemcpy(words, m->a.cov, m->a.cov_words * 4, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_mask_time(magot_ctx* ctx, magot_mask* m, int iters, double* paint_ms, double* text_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!m || iters <= 0) {
    set_error("magot_mask_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (!m->plan->executed) {
    set_error("magot_mask_time: execute the extraction plan first");
    return MAGOT_ERR_STATE;
  }
  double total[2] = {0, 0};
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < 2; ++k) {
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
      MAGOT_HIP_TRY(k ? launch_mask_text(m->a, ctx->stream) : launch_mask_paint(m->a, ctx->stream));
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
      MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
      float ms = 0;
      MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      total[k] += ms;
    }
  if (paint_ms) *paint_ms = total[0] / iters;
  if (text_ms) *text_ms = total[1] / iters;
  return MAGOT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// position_dic's bit track (track.hip; genome.py:981-1100)
// ---------------------------------------------------------------------------

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

int track_handle(magot_ctx* ctx, const magot_track* t, const char* who) {
  if (int rc = bind(ctx)) return rc;
  if (!t || t->ctx != ctx) {
    set_error(std::string(who) + ": null track, or a track of another context");
    return MAGOT_ERR_ARG;
  }
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
  struct Guard {
    magot_track* t;
    ~Guard() { magot_track_destroy(t); }
  } guard{new magot_track()};
  magot_track* t = guard.t;
  t->ctx = ctx;
  t->g = g;
  t->n_words = g->span / 32;
  t->n_blocks = track_blocks(g->span);
  t->plane_words = track_plane_words(g->span);
  t->scan_bytes = track_scan_bytes(t->n_blocks + 1);
  const uint64_t nc = g->contig_base.size();
  Carve cv;
  const uint64_t o_words = cv.take<uint32_t>(t->plane_words);
  const uint64_t o_scratch = cv.take<uint32_t>(t->plane_words);
  const uint64_t o_base = cv.take<uint64_t>(nc + 1);
  const uint64_t o_count = cv.take<uint32_t>(t->n_blocks + 1);
  const uint64_t o_rank = cv.take<uint32_t>(t->n_blocks + 1);
  const uint64_t o_tmp = cv.take<uint8_t>(t->scan_bytes);
  MAGOT_HIP_TRY(hipMalloc(&t->arena, cv.used + 256));
  char* base = static_cast<char*>(t->arena);
  t->words = reinterpret_cast<uint32_t*>(base + o_words);
  t->scratch = reinterpret_cast<uint32_t*>(base + o_scratch);
  t->contig_base = reinterpret_cast<uint64_t*>(base + o_base);
  t->blk_count = reinterpret_cast<uint32_t*>(base + o_count);
  t->blk_rank = reinterpret_cast<uint32_t*>(base + o_rank);
  t->scan_tmp = base + o_tmp;
  // both planes zeroed whole: no pass writes a word at or past n_words
  MAGOT_HIP_TRY(hipMemsetAsync(t->words, 0, 2 * ((t->plane_words * 4 + 255) & ~255ull),
                               ctx->stream));
  if (nc)
    MAGOT_HIP_TRY(hipMemcpy(t->contig_base, g->contig_base.data(), nc * 8, hipMemcpyHostToDevice));
  if (n_words) *n_words = t->n_words;
  guard.t = nullptr;
  *out = t;
  return MAGOT_OK;
}

int magot_track_base_class(magot_ctx* ctx, magot_track* t, const magot_genome* g, uint32_t flags) {
  if (int rc = track_handle(ctx, t, "magot_track_base_class")) return rc;
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
  if (int rc = track_handle(ctx, t, "magot_track_paint")) return rc;
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
  if (int rc = track_handle(ctx, t, "magot_track_set_bytes")) return rc;
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
  if (int rc = track_handle(ctx, t, "magot_track_get_bytes")) return rc;
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
  if (int rc = track_handle(ctx, t, "magot_track_fetch")) return rc;
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
  if (int rc = track_handle(ctx, t, "magot_track_windows_create")) return rc;
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
  struct Guard {
    magot_track_windows* w;
    ~Guard() { magot_track_windows_destroy(w); }
  } guard{new magot_track_windows()};
  magot_track_windows* w = guard.w;
  w->ctx = ctx;
  w->t = t;
  const uint64_t groups = track_flip_groups(total);
  w->scan_bytes = track_scan_bytes(groups + 1);
  Carve cv;
  const uint64_t o_first = cv.take<uint64_t>(nc + 1);
  const uint64_t o_sums = cv.take<uint32_t>(total);
  const uint64_t o_fc = cv.take<uint32_t>(groups + 1);
  const uint64_t o_fs = cv.take<uint64_t>(groups + 1);
  const uint64_t o_tmp = cv.take<uint8_t>(w->scan_bytes);
  MAGOT_HIP_TRY(hipMalloc(&w->arena, cv.used + 256));
  char* base = static_cast<char*>(w->arena);
  MAGOT_HIP_TRY(hipMemcpy(base + o_first, tab.data(), (nc + 1) * 8, hipMemcpyHostToDevice));
  TrackWindowArgs& a = w->a;
  a.track = t->words;
  a.rank = t->blk_rank;
  a.contig_base = t->contig_base;
  a.first = reinterpret_cast<const uint64_t*>(base + o_first);
  a.n_contigs = nc;
  a.n_windows = total;
  a.W = window;
  a.jump = jump;
  a.sums = reinterpret_cast<uint32_t*>(base + o_sums);
  a.flip_count = reinterpret_cast<uint32_t*>(base + o_fc);
  a.flip_slot = reinterpret_cast<uint64_t*>(base + o_fs);
  w->scan_tmp = base + o_tmp;
  if (int rc = track_rank_ready(ctx, t)) return rc;
  MAGOT_HIP_TRY(launch_track_windows(a, ctx->stream));
  if (n_windows) *n_windows = total;
  if (first) memcpy(first, tab.data(), (nc + 1) * 8);
  guard.w = nullptr;
  *out = w;
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
  if (int rc = track_handle(ctx, t, "magot_track_count")) return rc;
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
  if (int rc = track_handle(ctx, t, "magot_track_time")) return rc;
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
  double total[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < 5; ++k) {
      if (k >= 2 && k <= 3 && !w) continue;
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
      switch (k) {
        case 0:  // into the scratch plane: the track keeps its bits
          MAGOT_HIP_TRY(launch_track_class(t->g->nib, t->n_words, kOrigin, t->g->extent, false,
                                           true, t->scratch, ctx->stream));
          break;
        case 1:
          MAGOT_HIP_TRY(launch_track_rank(t->words, t->n_blocks, t->blk_count, t->blk_rank,
                                          t->scan_tmp, t->scan_bytes, ctx->stream));
          break;
        case 2:
          MAGOT_HIP_TRY(launch_track_windows(w->a, ctx->stream));
          break;
        case 3:
          MAGOT_HIP_TRY(launch_track_flip_count(w->a, s_min, w->scan_tmp, w->scan_bytes,
                                                ctx->stream));
          MAGOT_HIP_TRY(launch_track_flip_write(w->a, s_min, cap, ctx->stream));
          break;
        default:
          MAGOT_HIP_TRY(launch_track_count(static_cast<const magot_mask_interval*>(d.p),
                                           rows.size(), t->contig_base, t->words, t->blk_rank,
                                           t->g->span, static_cast<uint32_t*>(o.p), ctx->stream));
      }
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
      MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
      float ms = 0;
      MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      total[k] += ms;
    }
  for (int k = 0; k < 5; ++k) ms5[k] = total[k] / iters;
  return MAGOT_OK;
}

}  // extern "C"

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
  // text staging: chunk k goes through slot k & 1
  uint8_t* dev[2] = {nullptr, nullptr};
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t up_done[2] = {nullptr, nullptr}, parse_done[2] = {nullptr, nullptr};
  hipStream_t copy = nullptr;
  // the last chunk, still in dev[last_slot] (magot_depth_time)
  int last_slot = 0, last_in = 0;
  uint64_t last_len = 0, last_off = 0;
  std::vector<DepthHead> runs;  // in file order
};

namespace {

constexpr uint64_t kDepthChunkDefault = 64ull << 20;
constexpr uint64_t kDepthChunkMin = 1024, kDepthChunkMax = 1ull << 30;
constexpr uint64_t kDepthMaxLines = 0x7fffffffull;

void depth_free_staging(magot_depth* t, bool text_too) {
  for (int s = 0; s < 2; ++s) {
    if (t->pin[s]) (void)hipHostFree(t->pin[s]);
    t->pin[s] = nullptr;
    if (text_too && t->dev[s]) {
      (void)hipFree(t->dev[s]);
      t->dev[s] = nullptr;
    }
  }
}

int depth_handle(magot_ctx* ctx, const magot_depth* t, const char* who) {
  if (int rc = bind(ctx)) return rc;
  if (!t || t->ctx != ctx) {
    set_error(std::string(who) + ": null track, or a track of another context");
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

DepthParseArgs depth_args(const magot_depth* t, int slot, uint64_t n, uint64_t off, int in,
                          int out, bool scratch) {
  DepthParseArgs a{};
  a.text = t->dev[slot];
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
  depth_free_staging(t, true);
  for (int s = 0; s < 2; ++s) {
    if (t->up_done[s]) (void)hipEventDestroy(t->up_done[s]);
    if (t->parse_done[s]) (void)hipEventDestroy(t->parse_done[s]);
  }
  if (t->copy) (void)hipStreamDestroy(t->copy);
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
  struct Guard {
    magot_depth* t;
    ~Guard() { magot_depth_destroy(t); }
  } guard{new magot_depth()};
  magot_depth* t = guard.t;
  t->ctx = ctx;
  uint64_t chunk = chunk_bytes ? chunk_bytes : kDepthChunkDefault;
  chunk = std::min(std::max(chunk, kDepthChunkMin), kDepthChunkMax);
  chunk = std::min(chunk, std::max<uint64_t>(len, 1));
  const int n_slots = len > chunk ? 2 : 1;
  // a line of the grammar has at least 6 bytes ("a 1 0" and its LF)
  t->arena_cap = (depth_blocks(len / 6 + 2) + 1) * kDepthBlock;
  t->heads_cap = max_runs ? max_runs : (1u << 20);
  const uint64_t text_blocks = depth_text_blocks(chunk);
  t->scan_bytes = depth_scan_bytes(std::max(text_blocks, depth_blocks(t->arena_cap)) + 1);
  Carve cv;
  const uint64_t o_arena = cv.take<int32_t>(t->arena_cap);
  const uint64_t o_sum = cv.take<int64_t>(depth_blocks(t->arena_cap) + 1);
  const uint64_t o_dir = cv.take<int64_t>(depth_blocks(t->arena_cap) + 1);
  const uint64_t o_count = cv.take<uint32_t>(text_blocks + 1);
  const uint64_t o_first = cv.take<uint32_t>(text_blocks + 1);
  const uint64_t o_tmp = cv.take<uint8_t>(t->scan_bytes);
  const uint64_t o_heads = cv.take<DepthHead>(t->heads_cap);
  const uint64_t o_small = cv.take<uint8_t>(3 * sizeof(DepthCarry) + 64);
  MAGOT_HIP_TRY(hipMalloc(&t->arena_mem, cv.used + 256));
  char* base = static_cast<char*>(t->arena_mem);
  t->arena = reinterpret_cast<int32_t*>(base + o_arena);
  t->block_sum = reinterpret_cast<int64_t*>(base + o_sum);
  t->dir = reinterpret_cast<int64_t*>(base + o_dir);
  t->blk_count = reinterpret_cast<uint32_t*>(base + o_count);
  t->blk_first = reinterpret_cast<uint32_t*>(base + o_first);
  t->scan_tmp = base + o_tmp;
  t->heads = reinterpret_cast<DepthHead*>(base + o_heads);
  t->carry = reinterpret_cast<DepthCarry*>(base + o_small);
  t->status = reinterpret_cast<unsigned long long*>(base + o_small + 3 * sizeof(DepthCarry));
  t->n_heads = reinterpret_cast<uint32_t*>(t->status + 2);
  // the carries and the head counters zero, the status words all ones
  MAGOT_HIP_TRY(hipMemsetAsync(t->carry, 0, 3 * sizeof(DepthCarry) + 64, ctx->stream));
  MAGOT_HIP_TRY(hipMemsetAsync(t->status, 0xff, 16, ctx->stream));
  MAGOT_HIP_TRY(hipStreamCreateWithFlags(&t->copy, hipStreamNonBlocking));
  for (int s = 0; s < n_slots; ++s) {
    MAGOT_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->dev[s]), chunk + 256));
    MAGOT_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->pin[s]), chunk, hipHostMallocDefault));
    MAGOT_HIP_TRY(hipEventCreateWithFlags(&t->up_done[s], hipEventDisableTiming));
    MAGOT_HIP_TRY(hipEventCreateWithFlags(&t->parse_done[s], hipEventDisableTiming));
  }
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
    if (k >= 2) MAGOT_HIP_TRY(hipEventSynchronize(t->up_done[s]));  // pin[s] was read
    std::memcpy(t->pin[s], text + off, n);
    if (k >= 2) MAGOT_HIP_TRY(hipStreamWaitEvent(t->copy, t->parse_done[s], 0));
    MAGOT_HIP_TRY(hipMemcpyAsync(t->dev[s], t->pin[s], n, hipMemcpyHostToDevice, t->copy));
    MAGOT_HIP_TRY(hipEventRecord(t->up_done[s], t->copy));
    MAGOT_HIP_TRY(hipStreamWaitEvent(ctx->stream, t->up_done[s], 0));
    MAGOT_HIP_TRY(launch_depth_line_index(t->dev[s], n, t->blk_count, t->blk_first, t->scan_tmp,
                                          t->scan_bytes, ctx->stream));
    MAGOT_HIP_TRY(launch_depth_parse(depth_args(t, s, n, off, (int)(k & 1), (int)((k + 1) & 1),
                                                false), ctx->stream));
    MAGOT_HIP_TRY(hipEventRecord(t->parse_done[s], ctx->stream));
    t->last_slot = s;
    t->last_in = (int)(k & 1);
    t->last_len = n;
    t->last_off = off;
    off = end;
    ++k;
  }
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(t->copy));
  depth_free_staging(t, false);

  unsigned long long status = 0;
  uint32_t heads = 0;
  DepthCarry last;
  MAGOT_HIP_TRY(hipMemcpy(&status, t->status, 8, hipMemcpyDeviceToHost));
  MAGOT_HIP_TRY(hipMemcpy(&heads, t->n_heads, 4, hipMemcpyDeviceToHost));
  MAGOT_HIP_TRY(hipMemcpy(&last, t->carry + (k & 1), sizeof(last), hipMemcpyDeviceToHost));
  // the first offending line, whichever check finds it
  uint64_t bad_line = ~0ull;
  uint32_t bad = 0;
  if (status != ~0ull) {
    bad_line = (uint64_t)(status >> 8);
    bad = (uint32_t)(status & 0xff);
  }
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
  guard.t = nullptr;
  *out = t;
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
  if (int rc = depth_handle(ctx, t, "magot_depth_values")) return rc;
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
  if (int rc = depth_handle(ctx, t, "magot_depth_sums")) return rc;
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
  const uint64_t o_start = cv.take<int64_t>(n_rows);
  const uint64_t o_len = cv.take<int64_t>(n_rows);
  const uint64_t o_sums = cv.take<int64_t>(n_rows);
  const uint64_t o_off = cv.take<uint64_t>(n_groups + 1);
  const uint64_t o_group = cv.take<int64_t>(n_groups);
  DevBuf d;
  MAGOT_HIP_TRY(hipMalloc(&d.p, cv.used + 256));
  char* base = static_cast<char*>(d.p);
  int64_t* d_sums = reinterpret_cast<int64_t*>(base + o_sums);
  if (n_rows) {
    MAGOT_HIP_TRY(hipMemcpyAsync(base + o_start, start, n_rows * 8, hipMemcpyHostToDevice,
                                 ctx->stream));
    MAGOT_HIP_TRY(hipMemcpyAsync(base + o_len, length, n_rows * 8, hipMemcpyHostToDevice,
                                 ctx->stream));
  }
  if (n_groups)
    MAGOT_HIP_TRY(hipMemcpyAsync(base + o_off, group_offsets, (n_groups + 1) * 8,
                                 hipMemcpyHostToDevice, ctx->stream));
  MAGOT_HIP_TRY(launch_depth_sums(t->arena, t->dir, t->n_lines,
                                  reinterpret_cast<const int64_t*>(base + o_start),
                                  reinterpret_cast<const int64_t*>(base + o_len), n_rows, d_sums,
                                  ctx->stream));
  MAGOT_HIP_TRY(launch_depth_groups(d_sums, reinterpret_cast<const uint64_t*>(base + o_off),
                                    n_groups, reinterpret_cast<int64_t*>(base + o_group),
                                    ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (n_rows && sums) MAGOT_HIP_TRY(hipMemcpy(sums, d_sums, n_rows * 8, hipMemcpyDeviceToHost));
  if (n_groups)
    MAGOT_HIP_TRY(hipMemcpy(group_sums, base + o_group, n_groups * 8, hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

int magot_depth_time(magot_ctx* ctx, magot_depth* t, int iters, double* ms4,
                     uint64_t* chunk_len) {
  if (int rc = depth_handle(ctx, t, "magot_depth_time")) return rc;
  if (iters <= 0 || !ms4) {
    set_error("magot_depth_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (chunk_len) *chunk_len = t->last_len;
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
  double total[4] = {0, 0, 0, 0};
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < 4; ++k) {
      if (k < 2 && !t->last_len) continue;
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
      switch (k) {
        case 0:
          MAGOT_HIP_TRY(launch_depth_line_index(t->dev[t->last_slot], t->last_len, t->blk_count,
                                                t->blk_first, t->scan_tmp, t->scan_bytes,
                                                ctx->stream));
          break;
        case 1:  // the same depths into the same lines; heads, status and carry into scratch
          MAGOT_HIP_TRY(launch_depth_parse(depth_args(t, t->last_slot, t->last_len, t->last_off,
                                                      t->last_in, 2, true), ctx->stream));
          break;
        case 2:
          MAGOT_HIP_TRY(launch_depth_directory(t->arena, t->n_lines, t->block_sum, t->dir,
                                               t->scan_tmp, t->scan_bytes, ctx->stream));
          break;
        default:
          MAGOT_HIP_TRY(launch_depth_sums(t->arena, t->dir, t->n_lines, dr, dr + nr, nr,
                                          dr + 2 * nr, ctx->stream));
      }
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
      MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
      float ms = 0;
      MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      total[k] += ms;
    }
  for (int k = 0; k < 4; ++k) ms4[k] = total[k] / iters;
  return MAGOT_OK;
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
  // text staging: chunk k goes through slot k & 1
  uint8_t* dev[2] = {nullptr, nullptr};
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t up_done[2] = {nullptr, nullptr}, pass_done[2] = {nullptr, nullptr};
  hipStream_t copy = nullptr;
  // the last chunk, still in dev[last_slot] (magot_fq_time)
  int last_slot = 0, last_in = 0;
  uint64_t last_len = 0, last_off = 0, file_bytes = 0;
  uint64_t stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool fetched = false;  // the histogram below
  std::vector<int64_t> lengths;
  std::vector<uint64_t> counts;
};

namespace {

void fq_free_staging(magot_fq* t, bool text_too) {
  for (int s = 0; s < 2; ++s) {
    if (t->pin[s]) (void)hipHostFree(t->pin[s]);
    t->pin[s] = nullptr;
    if (text_too && t->dev[s]) {
      (void)hipFree(t->dev[s]);
      t->dev[s] = nullptr;
    }
  }
}

int fq_handle(magot_ctx* ctx, const magot_fq* t, const char* who) {
  if (int rc = bind(ctx)) return rc;
  if (!t || t->ctx != ctx) {
    set_error(std::string(who) + ": null handle, or a handle of another context");
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

FqChunkArgs fq_args(const magot_fq* t, int slot, uint64_t n, uint64_t off, int in, int out) {
  FqChunkArgs a{};
  a.text = t->dev[slot];
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
  fq_free_staging(t, true);
  for (int s = 0; s < 2; ++s) {
    if (t->up_done[s]) (void)hipEventDestroy(t->up_done[s]);
    if (t->pass_done[s]) (void)hipEventDestroy(t->pass_done[s]);
  }
  if (t->copy) (void)hipStreamDestroy(t->copy);
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
  struct Guard {
    magot_fq* t;
    ~Guard() { magot_fq_destroy(t); }
  } guard{new magot_fq()};
  magot_fq* t = guard.t;
  t->ctx = ctx;
  t->file_bytes = len;
  uint64_t chunk = chunk_bytes ? chunk_bytes : kDepthChunkDefault;
  chunk = std::min(std::max(chunk, kDepthChunkMin), kDepthChunkMax);
  chunk = std::min(chunk, std::max<uint64_t>(len, 1));
  const int n_slots = len > chunk ? 2 : 1;
  t->longs_cap = fq_long_cap(len);
  const uint64_t text_blocks = depth_text_blocks(chunk);
  t->scan_bytes = fq_scan_bytes(text_blocks + 1, t->longs_cap + kFqDense);
  t->sort_bytes = fq_sort_bytes(t->longs_cap);
  Carve cv;
  const uint64_t o_hist = cv.take<unsigned long long>(kFqDense);
  const uint64_t o_longs = cv.take<int64_t>(2 * t->longs_cap);
  const uint64_t o_blk = cv.take<FqBlock>(text_blocks + 1);
  const uint64_t o_pre = cv.take<FqBlock>(text_blocks + 1);
  const uint64_t o_cum = cv.take<FqItem>(t->longs_cap + kFqDense);
  const uint64_t o_scan = cv.take<uint8_t>(t->scan_bytes);
  const uint64_t o_sort = cv.take<uint8_t>(t->sort_bytes);
  const uint64_t o_small = cv.take<uint8_t>(256);
  MAGOT_HIP_TRY(hipMalloc(&t->mem, cv.used + 256));
  char* base = static_cast<char*>(t->mem);
  t->hist = reinterpret_cast<unsigned long long*>(base + o_hist);
  t->longs = reinterpret_cast<int64_t*>(base + o_longs);
  t->blk = reinterpret_cast<FqBlock*>(base + o_blk);
  t->pre = reinterpret_cast<FqBlock*>(base + o_pre);
  t->cum = reinterpret_cast<FqItem*>(base + o_cum);
  t->scan_tmp = base + o_scan;
  t->sort_tmp = base + o_sort;
  // 256 bytes: three carries, the list's cursor, the nine result words twice
  static_assert(3 * sizeof(FqCarry) + 8 + 18 * 8 <= 256, "the small block");
  t->carry = reinterpret_cast<FqCarry*>(base + o_small);
  t->cursor = reinterpret_cast<unsigned long long*>(base + o_small + 3 * sizeof(FqCarry));
  t->out = reinterpret_cast<uint64_t*>(t->cursor + 1);
  struct {
    FqCarry carry[3];
    uint64_t words[19];
  } small{};
  for (FqCarry& c : small.carry) c.last_lf = -1;  // no LF yet
  MAGOT_HIP_TRY(hipMemsetAsync(t->hist, 0, kFqDense * 8, ctx->stream));
  MAGOT_HIP_TRY(hipMemcpy(t->carry, &small, sizeof(small), hipMemcpyHostToDevice));
  MAGOT_HIP_TRY(hipStreamCreateWithFlags(&t->copy, hipStreamNonBlocking));
  for (int s = 0; s < n_slots; ++s) {
    MAGOT_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->dev[s]), chunk + 256));
    MAGOT_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&t->pin[s]), chunk, hipHostMallocDefault));
    MAGOT_HIP_TRY(hipEventCreateWithFlags(&t->up_done[s], hipEventDisableTiming));
    MAGOT_HIP_TRY(hipEventCreateWithFlags(&t->pass_done[s], hipEventDisableTiming));
  }
  // the zeroing above is on the context stream; the first upload is not
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));

  uint64_t off = 0, k = 0;
  while (off < len) {  // cut wherever the chunk ends
    const uint64_t n = std::min(chunk, len - off);
    const int s = (int)(k & 1);
    if (k >= 2) MAGOT_HIP_TRY(hipEventSynchronize(t->up_done[s]));  // pin[s] was read
    std::memcpy(t->pin[s], text + off, n);
    if (k >= 2) MAGOT_HIP_TRY(hipStreamWaitEvent(t->copy, t->pass_done[s], 0));
    MAGOT_HIP_TRY(hipMemcpyAsync(t->dev[s], t->pin[s], n, hipMemcpyHostToDevice, t->copy));
    MAGOT_HIP_TRY(hipEventRecord(t->up_done[s], t->copy));
    MAGOT_HIP_TRY(hipStreamWaitEvent(ctx->stream, t->up_done[s], 0));
    const FqChunkArgs a = fq_args(t, s, n, off, (int)(k & 1), (int)((k + 1) & 1));
    MAGOT_HIP_TRY(launch_fq_line_index(a, t->scan_tmp, t->scan_bytes, ctx->stream));
    MAGOT_HIP_TRY(launch_fq_lengths(a, fq_grid(n, ctx->n_cu), ctx->stream));
    MAGOT_HIP_TRY(hipEventRecord(t->pass_done[s], ctx->stream));
    t->last_slot = s;
    t->last_in = (int)(k & 1);
    t->last_len = n;
    t->last_off = off;
    off += n;
    ++k;
  }
  // a last line without its LF, from the carry the last chunk left
  MAGOT_HIP_TRY(launch_fq_tail(fq_args(t, 0, 0, len, (int)(k & 1), 2), len, ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(ctx->stream));
  MAGOT_HIP_TRY(hipStreamSynchronize(t->copy));
  fq_free_staging(t, false);

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
  guard.t = nullptr;
  *out = t;
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
  if (int rc = fq_handle(ctx, t, "magot_fq_histogram")) return rc;
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
  if (int rc = fq_handle(ctx, t, "magot_fq_time")) return rc;
  if (iters <= 0 || !ms4) {
    set_error("magot_fq_time: bad argument");
    return MAGOT_ERR_ARG;
  }
  if (chunk_len) *chunk_len = t->last_len;
  // a histogram, a list and a cursor of their own for the timed length pass,
  // and the copy's target
  Carve cv;
  const uint64_t o_hist = cv.take<unsigned long long>(kFqDense);
  const uint64_t o_longs = cv.take<int64_t>(t->longs_cap);
  const uint64_t o_cursor = cv.take<unsigned long long>(1);
  const uint64_t o_copy = cv.take<uint8_t>(t->last_len);
  DevBuf d;
  MAGOT_HIP_TRY(hipMalloc(&d.p, cv.used + 256));
  char* base = static_cast<char*>(d.p);
  MAGOT_HIP_TRY(hipMemsetAsync(base, 0, o_copy, ctx->stream));
  FqChunkArgs a = fq_args(t, t->last_slot, t->last_len, t->last_off, t->last_in, 2);
  a.hist = reinterpret_cast<unsigned long long*>(base + o_hist);
  a.longs = reinterpret_cast<int64_t*>(base + o_longs);
  a.n_longs = reinterpret_cast<unsigned long long*>(base + o_cursor);
  FqReduceArgs r{};
  r.hist = t->hist;
  r.longs = t->longs + t->longs_cap;
  r.n_longs = t->n_longs;
  r.cum = t->cum;
  r.out = t->out + 9;
  double total[4] = {0, 0, 0, 0};
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < 4; ++k) {
      if (k != 2 && !t->last_len) continue;
      if (k == 2) MAGOT_HIP_TRY(hipMemsetAsync(r.out, 0, 9 * 8, ctx->stream));
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
      switch (k) {
        case 0:
          MAGOT_HIP_TRY(launch_fq_line_index(a, t->scan_tmp, t->scan_bytes, ctx->stream));
          break;
        case 1:
          MAGOT_HIP_TRY(launch_fq_lengths(a, fq_grid(t->last_len, ctx->n_cu), ctx->stream));
          break;
        case 2:
          MAGOT_HIP_TRY(launch_fq_sort(t->longs, t->longs + t->longs_cap, t->n_longs,
                                       t->sort_tmp, t->sort_bytes, ctx->stream));
          MAGOT_HIP_TRY(launch_fq_reduce(r, t->scan_tmp, t->scan_bytes, ctx->stream));
          break;
        default:
          MAGOT_HIP_TRY(hipMemcpyAsync(base + o_copy, t->dev[t->last_slot], t->last_len,
                                       hipMemcpyDeviceToDevice, ctx->stream));
      }
      MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
      MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
      float ms = 0;
      MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      total[k] += ms;
    }
  for (int k = 0; k < 4; ++k) ms4[k] = total[k] / iters;
  return MAGOT_OK;
}

}  // extern "C"
