// The byte index of a resident text (textindex.hip): where one byte value
// occurs in a text that lies whole in HBM.  besthits_from_psl,
// heterozygosity_from_vcf and the FASTA record tools index the LFs (the line
// starts), replace_names its delimiter.  Included by common.h, whose structs
// hold a TextIndexArgs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace magot {

// Text bytes per workgroup of every text index and text parse (here, depth.hip,
// fastq.hip): 256 lanes, one 16-byte load each.
constexpr int kTextBlock = 4096;
constexpr uint64_t depth_text_blocks(uint64_t n) { return (n + kTextBlock - 1) / kTextBlock; }

constexpr uint32_t kTextNoByte = 0xffffffffu;

struct TextIndexArgs {
  const uint8_t* text;  // n bytes, 16-byte aligned, readable to the next multiple of 16
                        // (and one byte more for the stray-CR check)
  uint64_t n;
  uint64_t n_blocks;    // depth_text_blocks(n)
  uint32_t byte;        // the indexed byte
  uint32_t byte2;       // a second byte counted in the same pass, or kTextNoByte
  uint64_t* blk;        // n_blocks + 1: the byte's occurrences per text block, the last entry 0
  uint64_t* pre;        // their exclusive scan; pre[n_blocks]: the occurrences of the text
  uint64_t *blk2, *pre2;  // the same of byte2
  // plain mode: the offset of every occurrence, in text order.  Line mode:
  // n_lines + 1 line starts, pos[0] = 0, one behind every occurrence, pos[n_lines] = n
  uint64_t* pos;
  uint64_t n_lines;     // line mode: the occurrences, and one more when the text does not end in one
  // line mode's stray-CR check: min of (line << 8 | stray_reason)
  unsigned long long* stray_status;
  uint32_t stray_reason;
};

enum TextFill {
  kTextFillPlain,   // pos[j] = p for occurrence j at byte p
  kTextFillLines,   // pos[j + 1] = p + 1, and the two end entries
  kTextFillLinesCr  // the same; a CR that is neither before an LF nor the text's last byte
                    // atomic-mins its line into stray_status (the indexed byte is LF)
};

// tmp: the scan's scratch, exclusive_sum_bytes<uint64_t>(n_blocks + 1)
hipError_t launch_text_count(const TextIndexArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_text_fill(const TextIndexArgs& a, TextFill mode, hipStream_t s);

// out[i] = in[0] + ... + in[i - 1] over n entries (rocprim); tmp == nullptr
// asks for the scratch size in tmp_bytes
hipError_t exclusive_sum(void* tmp, size_t& tmp_bytes, const uint64_t* in, uint64_t* out,
                         uint64_t n, hipStream_t s);
hipError_t exclusive_sum(void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out,
                         uint64_t n, hipStream_t s);
template <class T>
size_t exclusive_sum_bytes(uint64_t n) {
  size_t b = 0;
  (void)exclusive_sum(nullptr, b, (const T*)nullptr, (T*)nullptr, n, hipStream_t(0));
  return b;
}

// CPython 2.7's string hash, a byte at a time: byte `index` (from 0) into h,
// then the length.  The empty string hashes to 0, and no string to -1.
__host__ __device__ inline uint64_t py27_hash_step(uint64_t h, uint32_t index, uint32_t byte) {
  if (!index) h = (uint64_t)byte << 7;
  return (h * 1000003ull) ^ byte;
}
__host__ __device__ inline uint64_t py27_hash_end(uint64_t h, uint32_t len) {
  if (!len) return 0;
  h ^= len;
  return h == ~0ull ? ~0ull - 1 : h;
}

}  // namespace magot
