// C ABI: the batch sequence operations (seqops.hip).
#include "abi_internal.h"

using namespace magot;

extern "C" {

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
  // the tables are checked on the host before the device is touched
  if (!seq_off || !pep_off || (n && (!frames || !strands))) {
    set_error("magot_translate_batch: null argument");
    return MAGOT_ERR_ARG;
  }
  for (uint64_t i = 0; i < n; ++i) {
    if (seq_off[i + 1] < seq_off[i]) {
      set_error("magot_translate_batch: seq_off must be non-decreasing");
      return MAGOT_ERR_ARG;
    }
    if (frames[i] < 0) {
      set_error("magot_translate_batch: negative frame");
      return MAGOT_ERR_ARG;
    }
    if (strands[i] != '+' && strands[i] != '-') {
      set_error("magot_translate_batch: strand must be '+' or '-'");
      return MAGOT_ERR_ARG;
    }
  }
  {
    // the kernel finds a residue's record in pep_off and reads its codon at
    // the place the record's length and frame give (magot_translate_sizes'
    // counts); a different table would send its loads past the record and
    // past the input, so it is refused
    std::vector<uint64_t> want(n + 1);
    if (int rc = magot_translate_sizes(seq_off, n, frames, want.data(), nullptr)) return rc;
    if (std::memcmp(want.data(), pep_off, want.size() * 8) != 0) {
      set_error(
          "magot_translate_batch: pep_off is not magot_translate_sizes' table for seq_off, frames");
      return MAGOT_ERR_ARG;
    }
  }
  if (int rc = bind(ctx)) return rc;
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

int magot_debug_orf6_tiles(const uint64_t* noff, uint64_t n_rec, const uint64_t* row_start,
                           uint64_t n_rows, uint64_t* t0, uint32_t* r0, uint32_t* e0, uint32_t* m,
                           uint64_t tiles_cap, uint64_t* n_tiles) {
  if (!noff || !n_tiles || (t0 && !r0) || (t0 && row_start && (!e0 || !m))) {
    set_error("magot_debug_orf6_tiles: null argument");
    return MAGOT_ERR_ARG;
  }
  Orf6Tiles tiles;
  orf6_plan_tiles(noff, n_rec, row_start, n_rows, &tiles);
  *n_tiles = tiles.r0.size();
  if (!t0) return MAGOT_OK;
  if (*n_tiles > tiles_cap) {
    set_error("magot_debug_orf6_tiles: tile arrays too small");
    return MAGOT_ERR_ARG;
  }
  std::memcpy(t0, tiles.t0.data(), tiles.t0.size() * 8);
  std::memcpy(r0, tiles.r0.data(), tiles.r0.size() * 4);
  if (row_start) {
    std::memcpy(e0, tiles.e0.data(), tiles.e0.size() * 4);
    std::memcpy(m, tiles.m.data(), tiles.m.size() * 4);
  }
  return MAGOT_OK;
}

int magot_orf6_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                     const uint8_t* lut64, const uint64_t* stream_off, uint8_t* out) {
  return magot_debug_orf6_batch(ctx, seqs, seq_off, n, lut64, stream_off, out, -1);
}

int magot_debug_orf6_batch(magot_ctx* ctx, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n,
                           const uint8_t* lut64, const uint64_t* stream_off, uint8_t* out,
                           int32_t poison) {
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
  Orf6Args a{};
  Carve cv;  // the uploads go to base + offset: the kernel's fields are const
  const uint64_t o_in = cv.take(&a.nuc, total + 64);
  cv.take(&a.out, total_res + 64);
  const uint64_t o_off = cv.take(&a.noff, n + 1);
  const uint64_t o_boff = cv.take(&a.boff, n + 1);
  const uint64_t o_t0 = cv.take(&a.tile_t0, n_tiles + 1);
  const uint64_t o_r0 = cv.take(&a.tile_r0, n_tiles);
  const uint64_t o_lut = cv.take(&a.tables, 256);
  void* d = nullptr;
  MAGOT_HIP_TRY(hipMalloc(&d, cv.used));
  cv.place(d);
  char* base = static_cast<char*>(d);
  hipError_t e = hipMemcpyAsync(base + o_in, seqs, total, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && poison >= 0)
    e = hipMemsetAsync(a.out, poison & 0xFF, total_res, ctx->stream);
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
    a.n_rec = n;
    a.total = total;
    a.n_tiles = n_tiles;
    launch_orf6(a, false, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, a.out, total_res, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  int rc = MAGOT_OK;
  if (e != hipSuccess) {
    set_error(std::string("magot_orf6_batch: ") + hipGetErrorString(e));
    rc = MAGOT_ERR_HIP;
  }
  (void)hipFree(d);
  return rc;
}

}  // extern "C"
