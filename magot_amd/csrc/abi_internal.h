// What more than one unit of the C ABI (abi*.hip) needs, each defined once: the
// handles whose insides another unit reads, and the host helpers the units
// share.  Header only, as hostutil.h; included by the ABI units alone.
#pragma once

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

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
  magot::ExcRun* runs = nullptr;
  uint32_t* dir = nullptr;
  std::vector<uint64_t> contig_base, contig_len;
  std::vector<std::string> names;  // contig names (magot_genome_load_fasta)
  std::vector<magot::ExcRun> host_runs;   // host copies for per-interval exception flags
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
  magot::ExtractArgs args{};
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

// Six frames over an extraction plan: the records are gathered from the
// genome plane through the plan's intervals inside the kernel (fused; the
// plan's nucleotide output is not read).
struct magot_orf6 {
  magot_ctx* ctx = nullptr;
  magot_plan* plan = nullptr;
  void* arena = nullptr;
  magot::Orf6Args args{};
  uint8_t* out = nullptr;
  uint64_t n_rec = 0, total = 0;
  std::vector<uint64_t> host_soff;
  bool executed = false;  // the streams are in HBM (magot_orfcall_create asks)
  void launch(hipStream_t s) const { magot::launch_orf6(args, true, s); }
};

// internal to the library: what is not inlined stays out of its exported symbols
#pragma GCC visibility push(hidden)

namespace magot {

inline int bind(magot_ctx* ctx) {
  if (!ctx) {
    set_error("null context");
    return MAGOT_ERR_ARG;
  }
  MAGOT_HIP_TRY(hipSetDevice(ctx->device));
  return MAGOT_OK;
}

constexpr uint64_t kPinRing = 64ull << 20;  // each of the context's two pinned staging buffers

inline int ensure_pin_ring(magot_ctx* ctx) {  // callers hold ctx->pin_mu
  for (int k = 0; k < 2; ++k)
    if (!ctx->pin[k]) {
      MAGOT_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->pin[k]), kPinRing,
                                  hipHostMallocDefault));
      MAGOT_HIP_TRY(hipEventCreateWithFlags(&ctx->pin_ev[k], hipEventDisableTiming));
    }
  return MAGOT_OK;
}

// A text into its device buffer through the context's two pinned buffers
// (resident_text_open).
inline int upload_text(magot_ctx* ctx, const char* text, uint64_t len, uint8_t* dev) {
  std::lock_guard<std::mutex> lock(ctx->pin_mu);
  if (int rc = ensure_pin_ring(ctx)) return rc;
  int b = 0;
  for (uint64_t q0 = 0; q0 < len; q0 += kPinRing, b ^= 1) {
    const uint64_t n = std::min(kPinRing, len - q0);
    MAGOT_HIP_TRY(hipEventSynchronize(ctx->pin_ev[b]));  // the buffer's previous copy has drained
    std::memcpy(ctx->pin[b], text + q0, n);
    MAGOT_HIP_TRY(hipMemcpyAsync(dev + q0, ctx->pin[b], n, hipMemcpyHostToDevice, ctx->stream));
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

// A whole text resident in HBM with the byte index of textindex.hip counted
// (magot_psl_parse, magot_vcf_parse, magot_fastarec_parse, magot_rename_parse).
// One allocation holds the text, the block counts, their scan's scratch and
// the caller's own slices; the owner frees `mem`.
constexpr uint64_t kTextPad = 32;  // 16-byte loads at and behind the text's last byte
struct ResidentText {
  void* mem = nullptr;
  char* extra = nullptr;  // the caller's slices, 256-byte aligned
  void* tmp = nullptr;    // the block scan's scratch
  size_t tmp_bytes = 0;
  uint64_t total = 0, total2 = 0;  // occurrences of the indexed byte, of the second
  uint64_t n_lines = 0;            // from the LF count, when one of the two bytes is LF
  float upload_ms = 0.f;  // first enqueue to last byte on the device, the staging copies included
};

// *max_bytes == 0: a quarter of the free memory (the tables take about as much
// again as the text)
inline int resident_text_budget(uint64_t* max_bytes) {
  if (*max_bytes) return MAGOT_OK;
  size_t free_b = 0, total_b = 0;
  MAGOT_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  *max_bytes = free_b / 4;
  return MAGOT_OK;
}

// Allocates, uploads the text between the context's event pair, runs
// before_count(rt->extra) -- what the caller enqueues between the upload and
// the count --, counts `byte` (and byte2 unless kTextNoByte) per text block and
// reads the totals back.  Inside before_count ix->text, n, n_blocks, blk and
// pre are already set (replace_names counts its values' offset from ix->text),
// and a device-to-host copy it enqueues on the context stream has arrived on
// return: the stream is idle then.  ix->pos and ix->n_lines are the caller's
// to set before the fill.
template <class F>
int resident_text_open(magot_ctx* ctx, const char* text, uint64_t len, uint32_t byte,
                       uint32_t byte2, uint64_t extra_bytes, F before_count, ResidentText* rt,
                       TextIndexArgs* ix) {
  hipStream_t s = ctx->stream;
  const bool second = byte2 != kTextNoByte;
  ix->n = len;
  ix->n_blocks = depth_text_blocks(len);
  ix->byte = byte;
  ix->byte2 = byte2;
  rt->tmp_bytes = exclusive_sum_bytes<uint64_t>(ix->n_blocks + 1);
  Carve cv;
  uint8_t* d_text;  // uploaded into; the index reads it as const
  cv.take(&d_text, len + kTextPad);
  uint64_t** const blk[4] = {&ix->blk, &ix->pre, &ix->blk2, &ix->pre2};
  ix->blk2 = ix->pre2 = nullptr;
  for (int k = 0; k < (second ? 4 : 2); ++k) cv.take(blk[k], ix->n_blocks + 1);
  cv.take(&rt->tmp, rt->tmp_bytes);
  cv.take(&rt->extra, extra_bytes);
  MAGOT_HIP_TRY(hipMalloc(&rt->mem, cv.used + 256));
  cv.place(rt->mem);
  ix->text = d_text;
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, s));
  if (len)
    if (int rc = upload_text(ctx, text, len, d_text)) return rc;
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, s));
  if (int rc = before_count(rt->extra)) return rc;
  MAGOT_HIP_TRY(launch_text_count(*ix, rt->tmp, rt->tmp_bytes, s));
  MAGOT_HIP_TRY(hipMemcpyAsync(&rt->total, ix->pre + ix->n_blocks, 8, hipMemcpyDeviceToHost, s));
  if (second)
    MAGOT_HIP_TRY(hipMemcpyAsync(&rt->total2, ix->pre2 + ix->n_blocks, 8, hipMemcpyDeviceToHost, s));
  MAGOT_HIP_TRY(hipStreamSynchronize(s));
  MAGOT_HIP_TRY(hipEventElapsedTime(&rt->upload_ms, ctx->ev0, ctx->ev1));
  const uint64_t lfs = byte == '\n' ? rt->total : byte2 == '\n' ? rt->total2 : 0;
  rt->n_lines = lfs + (len && text[len - 1] != '\n' ? 1 : 0);
  return MAGOT_OK;
}

inline int resident_text_open(magot_ctx* ctx, const char* text, uint64_t len, uint32_t byte,
                              uint32_t byte2, uint64_t extra_bytes, ResidentText* rt,
                              TextIndexArgs* ix) {
  return resident_text_open(
      ctx, text, len, byte, byte2, extra_bytes, [](char*) { return MAGOT_OK; }, rt, ix);
}

// The index pass of the *_time entry points: the count, then the fill.
inline hipError_t text_index_pass(const TextIndexArgs& ix, const ResidentText& rt, TextFill mode,
                                  hipStream_t s) {
  if (hipError_t e = launch_text_count(ix, rt.tmp, rt.tmp_bytes, s)) return e;
  return launch_text_fill(ix, mode, s);
}

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

// The context bound and h a handle made on it; `noun` is what the message
// calls the handle.
template <class H>
int handle_of(magot_ctx* ctx, const H* h, const char* who, const char* noun) {
  if (int rc = bind(ctx)) return rc;
  if (!h || h->ctx != ctx) {
    set_error(std::string(who) + ": null " + noun + ", or a " + noun + " of another context");
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

// launch() (it returns a hipError_t) timed on the context stream between the
// context's event pair; its milliseconds are added to *total_ms.
template <class F>
int time_pass(magot_ctx* ctx, double* total_ms, F launch) {
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  MAGOT_HIP_TRY(launch());
  MAGOT_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  MAGOT_HIP_TRY(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  MAGOT_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *total_ms += ms;
  return MAGOT_OK;
}

// The loop of the *_time entry points: `iters` rounds of the passes 0..n-1,
// pass(k) (it returns a hipError_t) timed by time_pass; ms[k] is pass k's mean.
// A pass that skip(k) names is not launched and reports exactly 0.
template <class F, class S>
int time_passes(magot_ctx* ctx, int iters, int n, double* ms, F pass, S skip) {
  for (int k = 0; k < n; ++k) ms[k] = 0;
  for (int i = 0; i < iters; ++i)
    for (int k = 0; k < n; ++k)
      if (!skip(k))
        if (int rc = time_pass(ctx, &ms[k], [&]() -> hipError_t { return pass(k); })) return rc;
  for (int k = 0; k < n; ++k) ms[k] /= iters;
  return MAGOT_OK;
}

template <class F>
int time_passes(magot_ctx* ctx, int iters, int n, double* ms, F pass) {
  return time_passes(ctx, iters, n, ms, pass, [](int) { return false; });
}

// A handle under construction: destroyed unless released.
template <class H, void (*Destroy)(H*)>
struct Building {
  H* p;
  ~Building() { Destroy(p); }
  H* release() {
    H* done = p;
    p = nullptr;
    return done;
  }
};

// n rows of a device table to the host; a null dst or no rows: nothing.
template <class T>
int fetch_rows(T* dst, const T* src, uint64_t n) {
  if (dst && n) MAGOT_HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
  return MAGOT_OK;
}

// An input the device path does not take: `who` is the entry point's whole
// message, *reason and *line (1-based, 0: none; either may be null) say why.
inline int decline(const char* who, uint32_t* reason, uint64_t* line, uint32_t why, uint64_t at) {
  if (reason) *reason = why;
  if (line) *line = at;
  set_error(who);
  return MAGOT_ERR_UNSUPPORTED;
}

// The kernels' status word of the first offending line: all ones while none
// offends, else its 0-based line << 8 | the reason.
inline bool first_offence(unsigned long long status, uint32_t* why, uint64_t* line0) {
  if (status == ~0ull) return false;
  *why = (uint32_t)(status & 0xff);
  *line0 = status >> 8;
  return true;
}

// MAGOT_OK, or the decline that a status word names.
inline int decline_if_offended(const char* who, uint32_t* reason, uint64_t* line,
                               unsigned long long status) {
  uint32_t why = 0;
  uint64_t line0 = 0;
  if (!first_offence(status, &why, &line0)) return MAGOT_OK;
  return decline(who, reason, line, why, line0 + 1);
}

// Text parsed on the device in chunks (abi_text.hip): chunk k is staged in
// pinned slot k & 1 and copied to device slot k & 1 on a stream of its own,
// while the context stream still parses the chunk before it.  Where to cut
// the text is the caller's.
constexpr uint64_t kTextChunkDefault = 64ull << 20;
constexpr uint64_t kTextChunkMin = 1024, kTextChunkMax = 1ull << 30;

inline uint64_t text_chunk_bytes(uint64_t asked, uint64_t len) {
  const uint64_t chunk = std::min(std::max(asked ? asked : kTextChunkDefault, kTextChunkMin),
                                  kTextChunkMax);
  return std::min(chunk, std::max<uint64_t>(len, 1));
}

struct TextStream {
  uint8_t* dev[2] = {nullptr, nullptr};
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t up_done[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  hipStream_t copy = nullptr;
  // the last chunk, still in dev[last_slot] (the timed passes)
  int last_slot = 0, last_in = 0;
  uint64_t last_len = 0, last_off = 0;

  int open(uint64_t chunk, int n_slots) {
    MAGOT_HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
    for (int s = 0; s < n_slots; ++s) {
      MAGOT_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev[s]), chunk + 256));
      MAGOT_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pin[s]), chunk, hipHostMallocDefault));
      MAGOT_HIP_TRY(hipEventCreateWithFlags(&up_done[s], hipEventDisableTiming));
      MAGOT_HIP_TRY(hipEventCreateWithFlags(&done[s], hipEventDisableTiming));
    }
    return MAGOT_OK;
  }
  // Chunk k, the n bytes at src that start at byte `off` of the text, to its
  // slot; the context stream waits for it.
  int push(magot_ctx* ctx, const char* src, uint64_t n, uint64_t off, uint64_t k) {
    const int s = (int)(k & 1);
    if (k >= 2) MAGOT_HIP_TRY(hipEventSynchronize(up_done[s]));  // pin[s] was read
    std::memcpy(pin[s], src, n);
    if (k >= 2) MAGOT_HIP_TRY(hipStreamWaitEvent(copy, done[s], 0));  // dev[s] was parsed
    MAGOT_HIP_TRY(hipMemcpyAsync(dev[s], pin[s], n, hipMemcpyHostToDevice, copy));
    MAGOT_HIP_TRY(hipEventRecord(up_done[s], copy));
    MAGOT_HIP_TRY(hipStreamWaitEvent(ctx->stream, up_done[s], 0));
    last_slot = s;
    last_in = (int)(k & 1);
    last_len = n;
    last_off = off;
    return MAGOT_OK;
  }
  int passed(magot_ctx* ctx, int s) {  // the passes over slot s are on the context stream
    MAGOT_HIP_TRY(hipEventRecord(done[s], ctx->stream));
    return MAGOT_OK;
  }
  void release_pinned() {
    for (int s = 0; s < 2; ++s) {
      if (pin[s]) (void)hipHostFree(pin[s]);
      pin[s] = nullptr;
    }
  }
  void close() {  // the owner's device is current
    for (int s = 0; s < 2; ++s) {
      if (pin[s]) (void)hipHostFree(pin[s]);
      if (dev[s]) (void)hipFree(dev[s]);
      pin[s] = dev[s] = nullptr;
    }
    for (int s = 0; s < 2; ++s) {
      if (up_done[s]) (void)hipEventDestroy(up_done[s]);
      if (done[s]) (void)hipEventDestroy(done[s]);
    }
    if (copy) (void)hipStreamDestroy(copy);
  }
};

}  // namespace magot

#pragma GCC visibility pop
