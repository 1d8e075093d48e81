// Stand-alone check of the purge_overlaps planner
// (magot_amd/csrc/overlapplan.cpp) for a sanitizer build
// (tests/sanitize/run_overlap_plan.py): fixed pairs of GFF texts with every
// accept and decline rule, every prefix of a valid GFF as either file (no final
// newline, fields at the buffer's end), and seeded random mutations.  Every
// accepted table is checked row by row -- the lines tile their buffer, a seqid
// is below n_seq or absent -- and rendered with none, all and every other line
// dropped.  Exit status 0 = every expectation held (and the sanitizers found
// nothing).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../magot_amd/csrc/common.h"

namespace magot {
void set_error(const std::string&) {}
}  // namespace magot

static int g_failures = 0;

static void expect(bool ok, const char* what, const std::string& input) {
  if (ok) return;
  ++g_failures;
  fprintf(stderr, "overlap_plan_check: %s\n  input: %s\n", what, input.c_str());
}

// status of magot_overlap_plan; *reason its reason; *kept the lines of the
// second file with more than 6 tabs when accepted
static int plan(const std::string& first, const std::string& second, uint32_t* reason,
                uint64_t* kept) {
  // exact-size heap copies: a read past either text is a sanitizer finding
  std::vector<char> a(first.begin(), first.end()), b(second.begin(), second.end());
  const std::string both = first + "\n----\n" + second;
  magot_ovplan* p = nullptr;
  uint32_t why = 99;
  const int rc = magot_overlap_plan(a.data(), a.size(), b.data(), b.size(), &p, &why);
  if (reason) *reason = why;
  if (rc != MAGOT_OK) {
    expect(p == nullptr, "a failed plan returned a handle", both);
    expect(rc != MAGOT_ERR_UNSUPPORTED || (why >= 1 && why <= 4), "a decline without a reason",
           both);
    return rc;
  }
  expect(why == 0, "an accepted plan with a reason", both);
  uint64_t flagged = 0;
  for (int which = 0; which < 2; ++which) {
    const std::vector<char>& text = which ? b : a;
    uint64_t n = 0;
    uint32_t n_seq = 0;
    const uint8_t* flag = nullptr;
    const uint32_t* seq = nullptr;
    const int64_t *c0 = nullptr, *c1 = nullptr;
    const uint64_t *off = nullptr, *len = nullptr;
    expect(magot_ovplan_table(p, which, &n, &n_seq, &flag, &seq, &c0, &c1, &off, &len) == MAGOT_OK,
           "magot_ovplan_table failed", both);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
      expect(off[i] == at && len[i] > 0, "the lines do not tile the text", both);
      at += len[i];
      expect(at <= text.size() && (text[at - 1] == '\n' || at == text.size()),
             "a line that does not end at an LF or at the text's end", both);
      expect(seq[i] == MAGOT_OVERLAP_NO_SEQ || (flag[i] && seq[i] < n_seq),
             "a seqid without a flag, or not below n_seq", both);
      expect(which == 1 || !flag[i] || seq[i] != MAGOT_OVERLAP_NO_SEQ,
             "a first-file line without its seqid", both);
      expect(c0[i] >= magot::kOvCoordMin && c0[i] <= magot::kOvCoordMax &&
                 c1[i] >= magot::kOvCoordMin && c1[i] <= magot::kOvCoordMax,
             "a coordinate outside the key", both);
      if (which == 1) flagged += flag[i];
    }
    expect(at == text.size(), "the lines do not cover the text", both);
    if (which == 1) {
      for (int mode = 0; mode < 3; ++mode) {
        std::vector<uint8_t> drop(n);
        uint64_t want = 0;
        for (uint64_t i = 0; i < n; ++i) {
          drop[i] = mode == 0 ? 0 : mode == 1 ? 1 : (uint8_t)(i & 1);
          if (!drop[i]) want += len[i];
        }
        uint64_t bytes = ~0ull;
        expect(magot_ovplan_render(p, b.data(), b.size(), drop.data(), nullptr, 0, &bytes) ==
                       MAGOT_OK && bytes == want,
               "render: size", both);
        std::vector<uint8_t> out(want);  // exact size: a write past it is a finding
        expect(magot_ovplan_render(p, b.data(), b.size(), drop.data(), out.data(), want, &bytes) ==
                   MAGOT_OK,
               "render: text", both);
        expect(want == 0 || out[want - 1] == '\n', "render: the last byte is not an LF", both);
        if (want)
          expect(magot_ovplan_render(p, b.data(), b.size(), drop.data(), out.data(), want - 1,
                                     &bytes) == MAGOT_ERR_ARG,
                 "render: a short buffer was accepted", both);
      }
    }
  }
  if (kept) *kept = flagged;
  magot_ovplan_destroy(p);
  return rc;
}

static std::string line(const char* seqid, const char* a, const char* b) {
  return std::string(seqid) + "\tsrc\tgene\t" + a + "\t" + b + "\t.\t+\t.\tID=x\n";
}

int main() {
  struct Case {
    std::string first, second;
    int status;
    uint32_t reason;
    uint64_t flagged;  // lines of the second file with more than 6 tabs
  };
  const int U = MAGOT_ERR_UNSUPPORTED;
  const std::vector<Case> cases = {
      {"", "", 0, 0, 0},
      {line("a", "100", "200"), line("a", "150", "160") + line("b", "x", "y"), 0, 0, 2},
      {line("a", "200", "100") + line("a", "-5", "+5"), line("a", " 1 ", "\v2\f"), 0, 0, 1},
      {"a\ts\tt\t1\t2\t.\t+\n", "a\ts\tt\tx\ty\t.\t+\n", 0, 0, 0},      // six tabs: not read
      {"a\ts\tt\t1\t2\t.\t+\t", "a\ts\tt\t1\t2\t.\t+\t", 0, 0, 1},      // seven, no newline
      {"#a\ts\tt\t1\t2\t.\t+\t.\n", "#a\ts\tt\t1\t2\t.\t+\t.\n", 0, 0, 1},
      {"\t\t\t1\t2\t\t\t", "\t\t\t3\t4\t\t\t\n\n\n", 0, 0, 1},
      {"\t\t\t\t\t\t\t", "", U, MAGOT_OVERLAP_BAD_INT_FIRST, 0},
      {line("a", "1e3", "5"), "", U, MAGOT_OVERLAP_BAD_INT_FIRST, 0},
      {line("a", "5", ""), "", U, MAGOT_OVERLAP_BAD_INT_FIRST, 0},
      {line("a", "-", "5"), "", U, MAGOT_OVERLAP_BAD_INT_FIRST, 0},
      {line("a", "1", "5"), line("a", "1", "5 5"), U, MAGOT_OVERLAP_BAD_INT_SECOND, 0},
      {line("a", "1", "5"), line("b", "1", "5 5"), 0, 0, 1},
      {line("a", "549755813887", "-549755813888"), line("a", "549755813887", "0"), 0, 0, 1},
      {line("a", "549755813888", "5"), "", U, MAGOT_OVERLAP_COORD_RANGE, 0},
      {line("a", "1", "5"), line("a", "-549755813889", "5"), U, MAGOT_OVERLAP_COORD_RANGE, 0},
      {line("a", "1", "1000000000000000000000"), "", U, MAGOT_OVERLAP_COORD_RANGE, 0},
      {line("a", "1", "1000000000000000000000x"), "", U, MAGOT_OVERLAP_BAD_INT_FIRST, 0},
  };
  for (const Case& c : cases) {
    uint32_t why = 0;
    uint64_t flagged = 0;
    const int rc = plan(c.first, c.second, &why, &flagged);
    expect(rc == c.status && why == c.reason && (rc || flagged == c.flagged),
           "status, reason or flagged lines", c.first + "\n----\n" + c.second);
  }
  // every prefix of a valid text, as the first file and as the second: fields
  // and lines that end at the buffer's end
  const std::string valid = line("c1", "3", "12") + "#c3\ts\tCDS\t1\t7\t.\t-\t0\tz\r\n" +
                            line("c2", "-1", "5000") + "# comment\n\n" + "c2\ts\tt\t7\t9\t.\t+\n" +
                            line("c1", "7", "9");
  for (size_t n = 0; n <= valid.size(); ++n) {
    int rc = plan(valid.substr(0, n), valid, nullptr, nullptr);
    expect(rc == MAGOT_OK || rc == U, "a prefix gave another status", valid.substr(0, n));
    rc = plan(valid, valid.substr(0, n), nullptr, nullptr);
    expect(rc == MAGOT_OK || rc == U, "a prefix gave another status", valid.substr(0, n));
  }
  // seeded mutations: a byte replaced, removed or doubled, in either file
  std::mt19937_64 rng(20261020);
  const char alphabet[] = "\t\n\r 0123456789-+#c12x";
  for (int it = 0; it < 4000; ++it) {
    std::string s = valid;
    for (int k = 0; k < 1 + (int)(rng() % 3); ++k) {
      const size_t at = rng() % s.size();
      switch (rng() % 3) {
        case 0: s[at] = alphabet[rng() % (sizeof alphabet - 1)]; break;
        case 1: s.erase(at, 1); break;
        default: s.insert(at, 1, s[at]); break;
      }
    }
    const int rc = it & 1 ? plan(s, valid, nullptr, nullptr) : plan(valid, s, nullptr, nullptr);
    expect(rc == MAGOT_OK || rc == U, "a mutation gave another status", s);
  }
  // bad arguments
  magot_ovplan* p = nullptr;
  expect(magot_overlap_plan(nullptr, 3, "", 0, &p, nullptr) == MAGOT_ERR_ARG,
         "a null text was accepted", "");
  expect(magot_overlap_plan("", 0, "", 0, nullptr, nullptr) == MAGOT_ERR_ARG,
         "a null result was accepted", "");
  expect(magot_ovplan_table(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr) == MAGOT_ERR_ARG,
         "a null plan was accepted", "");
  expect(magot_overlap_plan("", 0, "x\n", 2, &p, nullptr) == MAGOT_OK && p, "a plain plan", "");
  uint64_t bytes = 0;
  const uint8_t keep[1] = {0};
  expect(magot_ovplan_table(p, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr) == MAGOT_ERR_ARG,
         "a third file was accepted", "");
  expect(magot_ovplan_render(p, "x\n", 1, keep, nullptr, 0, &bytes) == MAGOT_ERR_ARG,
         "render took another text", "");
  expect(magot_ovplan_render(p, "x\n", 2, nullptr, nullptr, 0, &bytes) == MAGOT_ERR_ARG,
         "render took no flags", "");
  magot_ovplan_destroy(p);
  magot_ovplan_destroy(nullptr);

  printf("overlap_plan_check: %d check failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
