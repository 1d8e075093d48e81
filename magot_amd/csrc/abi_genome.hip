// C ABI: genome load, replication and the wire image (pack.cpp, devpack.hip,
// wire.hip).
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "abi_internal.h"

using namespace magot;

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
  uint8_t* raw;
  uint32_t* cnt;
  uint64_t* slot;
  void* tmp;
  sc.take(&raw, 32 * groups + 64);
  sc.take(&cnt, groups + 1);
  sc.take(&slot, groups + 1);
  sc.take(&tmp, scan_bytes + 1);
  DevBuf scratch;
  MAGOT_HIP_TRY(hipMalloc(&scratch.p, sc.used));
  sc.place(scratch.p);
  // the padding past n is read by the 32-byte loads (and masked)
  MAGOT_HIP_TRY(hipMemsetAsync(raw + n, 0, 32 * groups + 64 - n, ctx->stream));
  if (int rc = upload_raw(ctx, src, hp, raw)) return rc;
  lap("upload");
  MAGOT_HIP_TRY(launch_run_count(raw, n, cnt, slot, tmp, scan_bytes, ctx->stream));
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
  cv.take(&g->nib, 2 * hp.nib_words + 4);
  cv.take(&g->runs, hp.runs.size());
  cv.take(&g->dir, hp.dir.size());
  MAGOT_HIP_TRY(hipMalloc(&g->arena, cv.used));
  cv.place(g->arena);
  g->arena_bytes = cv.used;
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
  cv.take(&g->nib, 2 * hp.nib_words + 4);
  cv.take(&g->runs, hp.runs.size());
  cv.take(&g->dir, hp.dir.size());
  MAGOT_HIP_TRY(hipMalloc(&g->arena, cv.used));
  cv.place(g->arena);
  g->arena_bytes = cv.used;
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
  uint32_t* cnt;
  uint64_t* slot;
  void* tmp;
  sc.take(&cnt, groups + 1);
  sc.take(&slot, groups + 1);
  sc.take(&tmp, scan_bytes + 1);
  DevBuf scratch;
  MAGOT_HIP_TRY(hipMalloc(&scratch.p, sc.used));
  sc.place(scratch.p);
  MAGOT_HIP_TRY(launch_wire_count(g->nib, g->span, cnt, slot, tmp, scan_bytes, st));
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

}  // extern "C"
