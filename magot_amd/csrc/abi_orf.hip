// C ABI: six frames over an extraction plan (seqops.hip) and ORF calling over
// their streams (orfcall.hip).
#include <cstdlib>

#include "abi_internal.h"

using namespace magot;

extern "C" {

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
  Orf6Args& a = o->args;
  Carve cv;  // the uploads go to the arena + offset: the kernel's fields are const
  const uint64_t o_off = cv.take(&a.noff, o->n_rec + 1);
  const uint64_t o_boff = cv.take(&a.boff, o->n_rec + 1);
  cv.take(&o->out, o->total + 64);
  const uint64_t o_rows = cv.take(&a.rows, 2 * (ne_k + 1));
  const uint64_t o_t0 = cv.take(&a.tile_t0, n_tiles + 1);
  const uint64_t o_r0 = cv.take(&a.tile_r0, n_tiles);
  const uint64_t o_e0 = cv.take(&a.tile_e0, n_tiles);
  const uint64_t o_m = cv.take(&a.tile_m, n_tiles);
  const uint64_t o_lut = cv.take(&a.tables, 256);
  const uint64_t nib_words = p->args.span / 4;  // forward + reverse planes, 8 bases per word
  const uint64_t code2_words = nib_words / 2;
  uint32_t *code2, *exc1;  // written here; the kernel reads them as const
  cv.take(&code2, code2_words + 4);
  const uint64_t exc1_words = nib_words / 4;
  cv.take(&exc1, exc1_words + 4);
  MAGOT_HIP_TRY(hipMalloc(&o->arena, cv.used));
  cv.place(o->arena);
  char* base = static_cast<char*>(o->arena);
  auto up = [&](uint64_t off, const void* src, uint64_t bytes) {
    return bytes ? hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
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
  a.nib = p->args.nib;
  a.nib_words = nib_words;
  a.code2 = code2;
  a.code2_words = code2_words;
  a.exc1 = exc1;
  a.exc1_words = exc1_words;
  a.n_rows = ne_k;
  a.n_rec = o->n_rec;
  a.total = total_nuc;
  a.n_tiles = n_tiles;
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

int magot_orf6_poison(magot_ctx* ctx, magot_orf6* o, uint8_t byte) {
  if (int rc = bind(ctx)) return rc;
  if (!o) {
    set_error("magot_orf6_poison: null handle");
    return MAGOT_ERR_ARG;
  }
  if (o->total) MAGOT_HIP_TRY(hipMemsetAsync(o->out, byte, o->total, ctx->stream));
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
  if (int rc = time_passes(ctx, iters, 1, avg_ms,
                           [&](int) { return o->launch(ctx->stream), hipSuccess; }))
    return rc;
  o->executed = true;
  return MAGOT_OK;
}

int magot_orf6_time_b2b(magot_ctx* ctx, magot_orf6* o, int iters, double* avg_ms) {
  if (int rc = bind(ctx)) return rc;
  if (!o || !avg_ms || iters <= 0) {
    set_error("magot_orf6_time_b2b: bad argument");
    return MAGOT_ERR_ARG;
  }
  double ms = 0;
  if (int rc = time_pass(ctx, &ms, [&] {
        for (int i = 0; i < iters; ++i) o->launch(ctx->stream);
        return hipGetLastError();
      }))
    return rc;
  o->executed = true;
  *avg_ms = ms / iters;
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
  Building<magot_orfcall, magot_orfcall_destroy> guard{new magot_orfcall()};
  magot_orfcall* c = guard.p;
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
  *out = guard.release();
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
  return time_passes(ctx, iters, 1, avg_ms, [&](int) {
    if (!text) return orf_run(c, ctx->stream);
    if (hipError_t e = launch_orftext_sizes(c->t, ctx->stream)) return e;
    return launch_orftext_copy(c->t, ctx->stream);
  });
}

}  // extern "C"
