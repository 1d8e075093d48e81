// Stand-alone driver for the write_gff lowering (magot_amd/csrc/gffplan.cpp:
// magot_gff_read with MAGOT_GFF_FOR_WRITE, magot_gff_lower_write), built host-only
// with AddressSanitizer + UBSan by run_gffwrite.py.  Its one argument is a list
// file, one case per line:
//     <gff file> TAB <format 0|1|2> TAB <py2 0|1> TAB <expected file, or "-">
// The expected file holds the bytes write_gff gives followed by one LF; "-" says
// the planner has to decline.  The rows are rendered here by a plain restatement
// of magot.h's row rules, walked with every reference checked against the text
// and the blob, so a row that points outside them is a failure, not a fault.
//
// Two more modes, both about the score rule (score_text below, the rule of
// magot.h restated, as gffwrite.hip's size pass and tests/gffwrite_expect.py
// restate it):
//     gffwrite_check --rule <file>   one column per line in, the rule's answer
//                                    per line out ("None" where it declines):
//                                    the tests compare this with the expect
//                                    module's rule
//     gffwrite_check --scores        the rule against Python 2's str(float(s)),
//                                    that is '%.12g' of strtod with ".0" behind a
//                                    bare integer, over EVERY literal of the three
//                                    forms -?D+, -?D+.D*, -?.D+ with up to 4
//                                    integer and 4 fraction digits (11111 integer
//                                    strings, the empty one included, times 11111
//                                    fraction strings, times dot or none, times the
//                                    sign: 2.5e8 literals, on up to 16 threads)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <atomic>
#include <thread>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/magot.h"

namespace magot {
void set_error(const std::string&) {}
}  // namespace magot

namespace {

int failures = 0;

void fail(const std::string& what) {
  std::fprintf(stderr, "FAIL: %s\n", what.c_str());
  ++failures;
}

bool slurp(const std::string& path, std::string* out) {
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  std::ostringstream ss;
  ss << in.rdbuf();
  *out = ss.str();
  return true;
}

bool is_digit(char c) { return c >= '0' && c <= '9'; }
bool is_letter(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

// the printed score, or false where the device path declines
bool score_text(const std::string& f, std::string* out) {
  bool alnum = false;
  for (char c : f) alnum |= is_digit(c) || is_letter(c);
  if (!alnum) {
    *out = ".";
    return true;
  }
  size_t i = 0;
  const bool neg = f[0] == '-';
  i += neg;
  size_t i0 = i;
  while (i < f.size() && is_digit(f[i])) ++i;
  const size_t i1 = i;
  const bool dot = i < f.size() && f[i] == '.';
  i += dot;
  const size_t f0 = i;
  while (i < f.size() && is_digit(f[i])) ++i;
  size_t f1 = i;
  if (i != f.size() || !(i1 > i0 || (dot && f1 > f0))) return false;
  while (i0 < i1 && f[i0] == '0') ++i0;
  size_t lead = 0;
  while (f0 + lead < f1 && f[f0 + lead] == '0') ++lead;
  while (f1 > f0 && f[f1 - 1] == '0') --f1;
  const size_t il = i1 - i0, fl = f1 - f0;
  const size_t span = il ? il + fl : (fl ? fl - lead : 0);
  if (il > 12 || span > 12 || (!il && fl && lead > 3)) return false;
  *out = (neg ? "-" : "") + (il ? f.substr(i0, il) : std::string("0")) + "." +
         (fl ? f.substr(f0, fl) : std::string("0"));
  return true;
}

bool ref(const std::string& text, const std::string& blob, uint64_t off, uint32_t len,
         std::string* out) {
  const uint64_t whole = text.size() + blob.size();
  if (off > whole || len > whole - off) return false;
  out->clear();
  for (uint64_t k = off; k < off + len; ++k)
    out->push_back(k < text.size() ? text[k] : blob[k - text.size()]);
  return true;
}

// 0: rendered; 1: a score outside the device path; 2: a broken row
int render(const std::string& text, const std::string& blob, const magot_gffrow* rows, uint64_t n,
           std::string* out) {
  for (uint64_t r = 0; r < n; ++r) {
    const magot_gffrow& R = rows[r];
    if (R.line_off > text.size()) return 2;
    size_t end = text.find('\n', R.line_off);
    if (end == std::string::npos) end = text.size();
    const std::string line = text.substr(R.line_off, end - R.line_off);
    std::vector<std::string> cols;
    size_t b = 0;
    for (size_t e; cols.size() < 8 && (e = line.find('\t', b)) != std::string::npos; b = e + 1)
      cols.push_back(line.substr(b, e - b));
    if (cols.size() < 8) return 2;
    const uint32_t kind = R.kind & 0xffu;
    const bool has_parent = (R.kind & MAGOT_GFFROW_HAS_PARENT) != 0;
    if (kind > MAGOT_GFFROW_MADE_PARENT) return 2;
    std::string id, parent, type, score = ".", phase = ".";
    if (!ref(text, blob, R.id_off, R.id_len, &id)) return 2;
    if (has_parent && !ref(text, blob, R.parent_off, R.parent_len, &parent)) return 2;
    if (kind == MAGOT_GFFROW_MADE_PARENT) {
      if (!ref(text, blob, R.type_off, R.type_len, &type)) return 2;
    } else {
      if (!score_text(cols[5], &score)) return 1;
      if (cols[7] == "0" || cols[7] == "1" || cols[7] == "2") phase = cols[7];
    }
    const std::string c2 = kind == MAGOT_GFFROW_MADE_PARENT ? "." : cols[1];
    const std::string c3 = kind == MAGOT_GFFROW_MADE_PARENT  ? type
                           : kind == MAGOT_GFFROW_EXON_TWIN ? "exon"
                                                            : cols[2];
    *out += cols[0] + "\t" + c2 + "\t" + c3 + "\t" + std::to_string(R.lo) + "\t" +
            std::to_string(R.hi) + "\t" + score + "\t" + cols[6] + "\t" + phase + "\t";
    if (kind == MAGOT_GFFROW_GTF) {
      *out += "transcript_id " + id + ";gene_id " + parent;
    } else {
      *out += (kind == MAGOT_GFFROW_EXON_TWIN ? "ID=ExonOf" : "ID=") + id;
      if (has_parent) *out += ";Parent=" + parent;
    }
    *out += "\n";
  }
  return 0;
}

void run_case(const std::string& gff_path, uint32_t format, bool py2, const std::string& want_path) {
  const std::string what = gff_path + " format " + std::to_string(format) + (py2 ? " py2" : "");
  std::string text, want;
  if (!slurp(gff_path, &text)) return fail(what + ": cannot read the input");
  const bool expect_decline = want_path == "-";
  if (!expect_decline && !slurp(want_path, &want)) return fail(what + ": cannot read " + want_path);
  // the planner reads exactly len bytes: a heap copy without a terminator
  std::vector<char> exact(text.begin(), text.end());
  magot_gffplan* plan = nullptr;
  int rc = magot_gff_read(exact.data(), exact.size(), MAGOT_GFF_FOR_WRITE, &plan);
  if (rc == MAGOT_OK) {
    uint64_t n_rows = 0, blob_len = 0;
    rc = magot_gff_lower_write(plan, format, py2 ? MAGOT_GFF_ORDER_PY2 : 0, &n_rows, &blob_len);
    if (rc == MAGOT_OK) {
      const magot_gffrow* rows = nullptr;
      const uint8_t* blob = nullptr;
      magot_gffplan_write_views(plan, &rows, &n_rows, &blob, &blob_len);
      std::string got;
      const int how = render(text, std::string(reinterpret_cast<const char*>(blob), blob_len),
                             rows, n_rows, &got);
      if (how == 2) fail(what + ": a row leaves the text and the blob");
      else if (how == 1) rc = MAGOT_ERR_UNSUPPORTED;  // the device hands it back
      else {
        if (!got.empty()) got.pop_back();  // the lines are joined
        got += "\n";
        if (expect_decline) fail(what + ": lowered, expected a decline");
        else if (got != want) fail(what + ": bytes differ from the expected ones");
      }
      // a second lowering replaces the first
      if (magot_gff_lower_write(plan, format, 0, nullptr, nullptr) != MAGOT_OK)
        fail(what + ": the second lowering failed");
    }
  }
  if (rc == MAGOT_ERR_UNSUPPORTED) {
    if (!expect_decline) fail(what + ": declined, expected bytes");
  } else if (rc != MAGOT_OK) {
    fail(what + ": status " + std::to_string(rc));
  }
  magot_gffplan_destroy(plan);
}

// Python 2's str(float(s)) for a literal float() accepts
std::string py2_str_float(const std::string& lit) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%.12g", std::strtod(lit.c_str(), nullptr));
  std::string out(buf);
  if (out.find_first_of(".en") == std::string::npos) out += ".0";
  return out;
}

// every digit string of 0 to 4 digits
std::vector<std::string> digit_strings() {
  std::vector<std::string> out{""};
  for (int width = 1, n = 10; width <= 4; ++width, n *= 10)
    for (int v = 0; v < n; ++v) {
      char buf[8];
      std::snprintf(buf, sizeof buf, "%0*d", width, v);
      out.push_back(buf);
    }
  return out;
}

int all_scores() {
  const std::vector<std::string> digits = digit_strings();
  std::atomic<size_t> next{0};
  std::atomic<unsigned long long> checked{0}, wrong{0};
  auto work = [&]() {
    std::string lit, got;
    unsigned long long n = 0, bad = 0;
    for (size_t w; (w = next.fetch_add(1)) < digits.size();) {
      for (int sign = 0; sign < 2; ++sign) {
        const std::string head = (sign ? "-" : "") + digits[w];
        if (!digits[w].empty()) {  // -?D+
          ++n;
          if (!score_text(head, &got) || got != py2_str_float(head)) ++bad;
        }
        for (const std::string& f : digits) {  // -?D+.D* and -?.D+
          if (digits[w].empty() && f.empty()) continue;
          lit = head;
          lit += '.';
          lit += f;
          ++n;
          if (!score_text(lit, &got) || got != py2_str_float(lit)) {
            if (!bad) std::fprintf(stderr, "FAIL: score %s\n", lit.c_str());
            ++bad;
          }
        }
      }
    }
    checked += n;
    wrong += bad;
  };
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < hw; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  std::printf("gffwrite_check: %llu score literal(s), %llu check failure(s)\n",
              checked.load(), wrong.load());
  return wrong.load() ? 1 : 0;
}

int dump_rule(const char* path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) return 2;
  std::string line, got;
  while (std::getline(in, line)) std::printf("%s\n", score_text(line, &got) ? got.c_str() : "None");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--scores") return all_scores();
  if (argc == 3 && std::string(argv[1]) == "--rule") return dump_rule(argv[2]);
  if (argc != 2) {
    std::fprintf(stderr, "usage: gffwrite_check <list file>\n");
    return 2;
  }
  std::ifstream list(argv[1]);
  std::string line;
  int n = 0;
  while (std::getline(list, line)) {
    std::vector<std::string> f;
    std::stringstream ss(line);
    for (std::string part; std::getline(ss, part, '\t');) f.push_back(part);
    if (f.size() != 4) continue;
    run_case(f[0], (uint32_t)std::atoi(f[1].c_str()), f[2] == "1", f[3]);
    ++n;
  }
  std::printf("gffwrite_check: %d case(s), %d check failure(s)\n", n, failures);
  return failures ? 1 : 0;
}
