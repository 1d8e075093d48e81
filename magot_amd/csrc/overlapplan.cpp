// Host planner of purge_overlaps (genome_tools.py:548-568): both GFF texts
// lowered to one table each, a row per line, for the interval index
// (overlap.hip) and for the output pass, which copies the kept lines.  Host
// only.
//
// The reference reads `for line in open(...)`: a line ends after '\n' only and
// keeps it.  A line with more than 6 tabs is split at its tabs; x[0] names the
// seqid, int(x[3]) and int(x[4]) are its coordinates, taken as they come
// (reversed and negative ones included).  There is no '#' test.  The first
// file fills a dictionary seqid -> intervals; a line of the second file whose
// seqid the dictionary lacks is printed without its integers being read.  A
// line with 6 tabs or fewer is skipped in both files: the second file's is not
// printed either, the print being inside the test for tabs.
//
// What depends on the reference's sequential run declines with
// MAGOT_ERR_UNSUPPORTED and a reason, and the caller's line loop reproduces it:
//   MAGOT_OVERLAP_BAD_INT_FIRST   int() fails in the first file: ValueError
//                                 before anything is printed;
//   MAGOT_OVERLAP_BAD_INT_SECOND  int() fails in the second file on a line
//                                 whose seqid is known: everything before it is
//                                 printed, then ValueError;
//   MAGOT_OVERLAP_COORD_RANGE     a coordinate outside the composite key;
//   MAGOT_OVERLAP_SEQIDS          more seqids than the composite key holds.
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

struct OvDeclined {
  uint32_t reason;
};

inline bool ov_space(char c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f';
}

// Python 2's int() of a column, as coordinate() of maskplan.cpp reads it:
// optional surrounding whitespace and sign, at most 18 decimal digits.
// A longer run of digits is an integer to Python and out of range here.
int64_t ov_int(sv s, bool first) {
  size_t i = 0, n = s.size();
  while (i < n && ov_space(s[i])) ++i;
  while (n > i && ov_space(s[n - 1])) --n;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
  const size_t digits = n - i;
  int64_t v = 0;
  for (size_t k = i; k < n; ++k) {
    if (s[k] < '0' || s[k] > '9') break;
    if (digits <= 18) v = v * 10 + (s[k] - '0');
    ++i;
  }
  if (i < n || !digits)
    throw OvDeclined{first ? MAGOT_OVERLAP_BAD_INT_FIRST : MAGOT_OVERLAP_BAD_INT_SECOND};
  if (neg) v = -v;
  if (digits > 18 || v < kOvCoordMin || v > kOvCoordMax) throw OvDeclined{MAGOT_OVERLAP_COORD_RANGE};
  return v;
}

// One file's table.  `dict` maps the first file's seqids to dense numbers: the
// first file adds to it, the second looks up in it.
void ov_scan(const char* text, uint64_t len, bool first,
             std::unordered_map<sv, uint32_t>& dict, magot_ovtable& t) {
  for (uint64_t pos = 0; pos < len;) {
    const char* nl = static_cast<const char*>(memchr(text + pos, '\n', len - pos));
    const uint64_t end = nl ? (uint64_t)(nl - text) + 1 : len;
    const sv line(text + pos, end - pos);
    size_t tab[7];
    int tabs = 0;
    for (size_t i = 0; i < line.size() && tabs < 7; ++i)
      if (line[i] == '\t') tab[tabs++] = i;
    uint32_t seq = kOvNoSeq;
    int64_t c0 = 0, c1 = 0;
    if (tabs == 7) {
      const sv name = line.substr(0, tab[0]);
      const auto it = dict.find(name);
      if (it != dict.end()) seq = it->second;
      if (first || seq != kOvNoSeq) {
        // int(x[3]) then int(x[4]): either failure is the same ValueError
        c0 = ov_int(line.substr(tab[2] + 1, tab[3] - tab[2] - 1), first);
        c1 = ov_int(line.substr(tab[3] + 1, tab[4] - tab[3] - 1), first);
        if (seq == kOvNoSeq) {
          if (dict.size() >= kOvMaxSeq) throw OvDeclined{MAGOT_OVERLAP_SEQIDS};
          seq = (uint32_t)dict.size();
          dict.emplace(name, seq);
        }
      }
    }
    t.flag.push_back(tabs == 7);
    t.seq.push_back(seq);
    t.c0.push_back(c0);
    t.c1.push_back(c1);
    t.off.push_back(pos);
    t.len.push_back(end - pos);
    pos = end;
  }
}

}  // namespace
}  // namespace magot

extern "C" {

int magot_overlap_plan(const char* gff1, uint64_t len1, const char* gff2, uint64_t len2,
                       magot_ovplan** out, uint32_t* reason) {
  if (!out || (len1 && !gff1) || (len2 && !gff2)) {
    magot::set_error("magot_overlap_plan: null argument");
    return MAGOT_ERR_ARG;
  }
  *out = nullptr;
  if (reason) *reason = 0;
  std::unique_ptr<magot_ovplan> P(new magot_ovplan());
  try {
    std::unordered_map<magot::sv, uint32_t> dict;
    magot::ov_scan(gff1, len1, true, dict, P->t[0]);
    magot::ov_scan(gff2, len2, false, dict, P->t[1]);
    P->n_seq = (uint32_t)dict.size();
  } catch (const magot::OvDeclined& d) {
    if (reason) *reason = d.reason;
    magot::set_error("magot_overlap_plan: input needs the sequential run; use the line loop");
    return MAGOT_ERR_UNSUPPORTED;
  } catch (const std::exception& e) {
    magot::set_error(std::string("magot_overlap_plan: ") + e.what());
    return MAGOT_ERR_ARG;
  }
  *out = P.release();
  return MAGOT_OK;
}

int magot_ovplan_table(const magot_ovplan* p, int which, uint64_t* n_lines, uint32_t* n_seq,
                       const uint8_t** flag, const uint32_t** seq, const int64_t** c0,
                       const int64_t** c1, const uint64_t** off, const uint64_t** len) {
  if (!p || which < 0 || which > 1) {
    magot::set_error("magot_ovplan_table: null plan, or a file other than 0 and 1");
    return MAGOT_ERR_ARG;
  }
  const magot_ovtable& t = p->t[which];
  if (n_lines) *n_lines = t.flag.size();
  if (n_seq) *n_seq = p->n_seq;
  if (flag) *flag = t.flag.data();
  if (seq) *seq = t.seq.data();
  if (c0) *c0 = t.c0.data();
  if (c1) *c1 = t.c1.data();
  if (off) *off = t.off.data();
  if (len) *len = t.len.data();
  return MAGOT_OK;
}

int magot_ovplan_render(const magot_ovplan* p, const char* gff2, uint64_t len2,
                        const uint8_t* drop, uint8_t* out, uint64_t cap, uint64_t* bytes) {
  if (!p || !bytes || (len2 && !gff2)) {
    magot::set_error("magot_ovplan_render: null argument");
    return MAGOT_ERR_ARG;
  }
  const magot_ovtable& t = p->t[1];
  const uint64_t n = t.flag.size();
  if (n && (!drop || t.off[n - 1] + t.len[n - 1] != len2)) {
    magot::set_error("magot_ovplan_render: no flags, or not the text the plan was made from");
    return MAGOT_ERR_ARG;
  }
  // `print line[:-1]`: the line without its last byte (its LF, or the last
  // byte of a final line that has none), then '\n'
  uint64_t need = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (!drop[i]) need += t.len[i];
  *bytes = need;
  if (!out) return MAGOT_OK;
  if (cap < need) {
    magot::set_error("magot_ovplan_render: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (drop[i]) continue;
    memcpy(out + at, gff2 + t.off[i], t.len[i] - 1);
    at += t.len[i];
    out[at - 1] = '\n';
  }
  return MAGOT_OK;
}

void magot_ovplan_destroy(magot_ovplan* p) { delete p; }

}  // extern "C"
