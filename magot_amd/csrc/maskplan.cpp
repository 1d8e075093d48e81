// Host planner of mask_from_gff (genome_tools.py:394-428): the GFF pass
// lowered to an interval table for the device painter (maskgen.hip), and the
// check that the native FASTA reader's contigs are the ones the reference's
// own read loop builds.  Host only; no sequence byte is touched here.
//
// The reference replays the features one after another on Python lists.
// In-range features are idempotent and commute (a base ends up covered or
// not), which is what the device path relies on.  Every line whose effect
// depends on the replay declines with MAGOT_ERR_UNSUPPORTED, and the caller's
// line loop reproduces it:
//   int() failing (ValueError), an unknown fields[0] (KeyError);
//   a negative slice index (start < 1, stop < 0) unless the slice is empty
//     and nothing is inserted;
//   a hard mask that changes the list's length (stop > len with
//     start <= stop): every later feature of the contig is then shifted.
// Lines that change nothing (start > stop, start > len in soft mode,
// stop == 0) are dropped.
//
// Piece size.  An interval longer than kMaskPiece bases is cut into pieces of
// at most that many, so one device lane never writes more than
// kMaskPiece / 32 = 64 interior coverage words (256 bytes, two cache lines)
// however long a feature is: a hard-masked 100 Mb repeat becomes ~49 K pieces
// spread over the grid instead of one lane's 12 MB loop.  CDS intervals (a few
// hundred bases) stay one piece, and the table costs 12 bytes per piece, 6 MB
// for a fully masked 1 Gb genome.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace magot {
namespace {

using sv = std::string_view;

struct Declined {};

inline bool py_space(char c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f';
}

// int() of a coordinate column, as magot_flank_plan reads it: optional
// surrounding whitespace and sign, at most 18 decimal digits; anything else
// (ValueError in the reference, or beyond int64) declines.
int64_t coordinate(sv s) {
  size_t i = 0, n = s.size();
  while (i < n && py_space(s[i])) ++i;
  while (n > i && py_space(s[n - 1])) --n;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
  if (i >= n || n - i > 18) throw Declined();
  int64_t v = 0;
  for (; i < n; ++i) {
    if (s[i] < '0' || s[i] > '9') throw Declined();
    v = v * 10 + (s[i] - '0');
  }
  return neg ? -v : v;
}

// slice.indices() of one bound for a list of L items (step 1)
inline int64_t slice_bound(int64_t x, int64_t L) {
  return x < 0 ? (x + L < 0 ? 0 : x + L) : (x < L ? x : L);
}

}  // namespace
}  // namespace magot

using magot::sv;

extern "C" {

uint32_t magot_mask_piece(void) { return magot::kMaskPiece; }

int magot_mask_fasta_check(const char* text, uint64_t len, uint32_t n_contigs) {
  if (len && !text) {
    magot::set_error("magot_mask_fasta_check: null argument");
    return MAGOT_ERR_ARG;
  }
  auto decline = [](const char* why) {
    magot::set_error(std::string("magot_mask_fasta_check: ") + why);
    return MAGOT_ERR_UNSUPPORTED;
  };
  // a line before the first header is appended to genome_dict[""]: KeyError
  if (len && text[0] != '>') return decline("sequence before the first header");
  uint64_t headers = 0;
  for (uint64_t pos = 0; pos < len;) {
    if (text[pos] == '>') {
      // the name is line.split()[0][1:]: whitespace right after '>' (or the
      // line's end) makes it "", not the first word the native reader takes
      if (pos + 1 >= len || magot::py_space(text[pos + 1]))
        return decline("whitespace directly after '>'");
      ++headers;
    }
    const char* nl = static_cast<const char*>(memchr(text + pos, '\n', len - pos));
    if (!nl) break;
    pos = (uint64_t)(nl - text) + 1;
  }
  // the native reader drops empty contigs and folds repeated names into one;
  // the reference keeps (and prints) the former and resets the latter
  if (headers != n_contigs) return decline("an empty contig or a repeated name");
  return MAGOT_OK;
}

int magot_mask_plan(const char* gff, uint64_t gff_len, const char* const* seqids,
                    const uint64_t* contig_lens, uint32_t n_contigs, const char* feature_type,
                    uint32_t flags, magot_maskplan** out, uint64_t* n_intervals) {
  if (!out || (gff_len && !gff) || (n_contigs && (!seqids || !contig_lens)) || !feature_type ||
      (flags & ~(MAGOT_MASK_HARD | MAGOT_MASK_KEEP_CASE))) {
    magot::set_error("magot_mask_plan: null argument or unknown flag");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  std::unique_ptr<magot_maskplan> P(new magot_maskplan());
  P->flags = flags;
  P->contig_lens.assign(contig_lens, contig_lens + n_contigs);
  const bool hard = (flags & MAGOT_MASK_HARD) != 0;
  const sv ftype(feature_type);
  try {
    std::unordered_map<sv, uint32_t> contig_of;
    for (uint32_t i = 0; i < n_contigs; ++i) {
      if (!seqids[i] || contig_lens[i] >= (1ull << 32)) {
        magot::set_error("magot_mask_plan: null name, or a contig of 4 Gbases or more");
        return MAGOT_ERR_ARG;
      }
      contig_of[sv(seqids[i])] = i;
    }
    for (uint64_t pos = 0; pos < gff_len;) {
      // `for line in gff_file`: lines end after '\n', which they keep
      const char* nl = static_cast<const char*>(memchr(gff + pos, '\n', gff_len - pos));
      const uint64_t end = nl ? (uint64_t)(nl - gff) + 1 : gff_len;
      const sv line(gff + pos, end - pos);
      pos = end;
      // line.count('\t') > 5, with no '#' test; fields = line.split('\t')
      size_t tab[6];
      int tabs = 0;
      for (size_t i = 0; i < line.size() && tabs < 6; ++i)
        if (line[i] == '\t') tab[tabs++] = i;
      if (tabs < 6) continue;
      auto field = [&](int k) {  // k <= 4
        const size_t b = k ? tab[k - 1] + 1 : 0;
        return line.substr(b, tab[k] - b);
      };
      if (field(2) != ftype) continue;
      const int64_t start = magot::coordinate(field(3));
      const int64_t stop = magot::coordinate(field(4));
      const auto ci = contig_of.find(field(0));
      if (ci == contig_of.end()) throw magot::Declined();  // KeyError
      const int64_t L = (int64_t)contig_lens[ci->second];
      // lst[start - 1:stop]
      const int64_t a = magot::slice_bound(start - 1, L);
      const int64_t b = std::max(a, magot::slice_bound(stop, L));
      const bool negative = start < 1 || stop < 0;
      if (hard) {
        // ... = ['N'] * (1 + stop - start): range() of a negative count is empty
        const int64_t n = std::max<int64_t>(0, 1 + stop - start);
        if (n == 0 && b == a) continue;
        if (negative || n != b - a) throw magot::Declined();  // the list changes length
      } else {
        if (b == a) continue;
        if (negative) throw magot::Declined();  // e.g. start = 0: the last base
      }
      for (int64_t at = a; at < b; at += magot::kMaskPiece)
        P->rows.push_back(magot_mask_interval{
            ci->second, (uint32_t)at, (uint32_t)std::min<int64_t>(magot::kMaskPiece, b - at)});
    }
  } catch (const magot::Declined&) {
    magot::set_error("magot_mask_plan: input needs the sequential replay; use the line loop");
    return MAGOT_ERR_UNSUPPORTED;
  } catch (const std::exception& e) {
    magot::set_error(std::string("magot_mask_plan: ") + e.what());
    return MAGOT_ERR_ARG;
  }
  if (n_intervals) *n_intervals = P->rows.size();
  *out = P.release();
  return MAGOT_OK;
}

int magot_maskplan_table(const magot_maskplan* p, const magot_mask_interval** rows,
                         uint64_t* n_intervals, uint32_t* flags) {
  if (!p) {
    magot::set_error("magot_maskplan_table: null plan");
    return MAGOT_ERR_ARG;
  }
  if (rows) *rows = p->rows.empty() ? nullptr : p->rows.data();
  if (n_intervals) *n_intervals = p->rows.size();
  if (flags) *flags = p->flags;
  return MAGOT_OK;
}

void magot_maskplan_destroy(magot_maskplan* p) { delete p; }

}  // extern "C"
