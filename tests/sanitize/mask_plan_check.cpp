// Stand-alone check of the mask_from_gff planner (magot_amd/csrc/maskplan.cpp)
// for a sanitizer build (tests/sanitize/run_mask_plan.py): fixed GFF texts
// with every accept / drop / decline rule, lines cut at every byte (no final
// newline, fields at the buffer's end), seeded random mutations of a valid
// GFF, and FASTA texts through magot_mask_fasta_check.  Every accepted table
// is checked row by row: inside its contig, at most magot_mask_piece() bases.
// Exit status 0 = every expectation held (and the sanitizers found nothing).
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
  fprintf(stderr, "mask_plan_check: %s\n  input: %s\n", what, input.c_str());
}

static const char* kNames[] = {"c1", "c2", "#c3"};
static const uint64_t kLens[] = {100, 5000, 7};

// status of magot_mask_plan; *bases = bases covered (pieces summed) when accepted
static int plan(const std::string& gff, uint32_t flags, uint64_t* rows_out, uint64_t* bases) {
  // an exact-size heap copy: a read past the text is a sanitizer finding
  std::vector<char> text(gff.begin(), gff.end());
  magot_maskplan* p = nullptr;
  uint64_t n = 0;
  const int rc = magot_mask_plan(text.data(), text.size(), kNames, kLens, 3, "CDS", flags, &p, &n);
  if (rc != MAGOT_OK) {
    expect(p == nullptr, "a failed plan returned a handle", gff);
    return rc;
  }
  const magot_mask_interval* rows = nullptr;
  uint64_t n2 = 0;
  uint32_t f = ~0u;
  expect(magot_maskplan_table(p, &rows, &n2, &f) == MAGOT_OK && n2 == n && f == flags,
         "table view disagrees with the plan", gff);
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n; ++i) {
    expect(rows[i].contig < 3 && rows[i].len > 0 && rows[i].len <= magot_mask_piece() &&
               (uint64_t)rows[i].start + rows[i].len <= kLens[rows[i].contig],
           "a row outside its contig or longer than a piece", gff);
    sum += rows[i].len;
  }
  if (rows_out) *rows_out = n;
  if (bases) *bases = sum;
  magot_maskplan_destroy(p);
  return rc;
}

static std::string line(const char* seqid, const char* type, const char* a, const char* b) {
  return std::string(seqid) + "\tsrc\t" + type + "\t" + a + "\t" + b + "\t.\t+\t.\tID=x\n";
}

int main() {
  struct Case {
    std::string gff;
    int soft, hard;             // expected status
    uint64_t soft_b, hard_b;    // expected covered bases (pieces summed)
  };
  const int U = MAGOT_ERR_UNSUPPORTED;
  const std::vector<Case> cases = {
      {"", 0, 0, 0, 0},
      {line("c1", "CDS", "1", "100"), 0, 0, 100, 100},
      {line("c1", "CDS", "3", "12") + line("c1", "gene", "1", "50") + line("c1", "CDS", "3", "12"),
       0, 0, 20, 20},
      {line("c2", "CDS", "10", "4500"), 0, 0, 4491, 4491},
      {line("c1", "CDS", "90", "120"), 0, U, 11, 0},
      {line("c1", "CDS", "150", "160"), 0, U, 0, 0},
      {line("c1", "CDS", "30", "10") + line("c1", "CDS", "500", "400") + line("c1", "CDS", "1", "0"),
       0, 0, 0, 0},
      {line("c1", "CDS", "0", "-1"), 0, 0, 0, 0},
      {line("c1", "CDS", "0", "200"), U, U, 0, 0},
      {line("c1", "CDS", "1", "-1"), U, U, 0, 0},
      {line("c1", "CDS", "-5", "10"), 0, U, 0, 0},
      {line("nope", "CDS", "9", "2"), U, U, 0, 0},
      {line("c1", "CDS", "12a", "20"), U, U, 0, 0},
      {line("c1", "CDS", "", "20"), U, U, 0, 0},
      {line("c1", "CDS", "1", "1000000000000000000000"), U, U, 0, 0},
      {line("#c3", "CDS", " +2 ", "5"), 0, 0, 4, 4},
      {"c1\tsrc\tCDS\t1\t5\t.\n", 0, 0, 0, 0},           // five tabs: not considered
      {"c1\tsrc\tCDS\t1\t5\t.\t", 0, 0, 5, 5},            // six tabs, no newline
      {"\t\t\t\t\t\t", 0, 0, 0, 0},
      {"\t\tCDS\t\t\t\t", U, U, 0, 0},
  };
  for (const Case& c : cases) {
    uint64_t rows = 0, bases = 0;
    int rc = plan(c.gff, 0, &rows, &bases);
    expect(rc == c.soft && (rc || bases == c.soft_b), "soft: status or covered bases", c.gff);
    rc = plan(c.gff, MAGOT_MASK_HARD | MAGOT_MASK_KEEP_CASE, &rows, &bases);
    expect(rc == c.hard && (rc || bases == c.hard_b), "hard: status or covered bases", c.gff);
  }
  // every prefix of a valid text: fields and lines that end at the buffer's end
  const std::string valid = line("c1", "CDS", "3", "12") + "#c3\ts\tCDS\t1\t7\t.\t-\t0\tz\r\n" +
                            line("c2", "CDS", "1", "5000") + "# comment\n\n" +
                            line("c2", "exon", "7", "9");
  for (size_t n = 0; n <= valid.size(); ++n) {
    const int rc = plan(valid.substr(0, n), n & 1 ? MAGOT_MASK_HARD : 0, nullptr, nullptr);
    expect(rc == MAGOT_OK || rc == U, "a prefix gave another status", valid.substr(0, n));
  }
  // seeded mutations: a byte replaced, removed or doubled
  std::mt19937_64 rng(20261019);
  const char alphabet[] = "\t\n\r 0123456789-+#cCDSx";
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
    const int rc = plan(s, it & 1 ? MAGOT_MASK_HARD : 0, nullptr, nullptr);
    expect(rc == MAGOT_OK || rc == U, "a mutation gave another status", s);
  }
  // bad arguments
  magot_maskplan* p = nullptr;
  expect(magot_mask_plan("", 0, kNames, kLens, 3, "CDS", 4u, &p, nullptr) == MAGOT_ERR_ARG,
         "an unknown flag was accepted", "");
  expect(magot_mask_plan("", 0, kNames, kLens, 3, nullptr, 0, &p, nullptr) == MAGOT_ERR_ARG,
         "a null feature type was accepted", "");
  const uint64_t big[] = {1ull << 32};
  expect(magot_mask_plan("", 0, kNames, big, 1, "CDS", 0, &p, nullptr) == MAGOT_ERR_ARG,
         "a contig of 4 Gbases was accepted", "");
  magot_maskplan_destroy(nullptr);

  struct Fasta {
    std::string text;
    uint32_t n;
    int want;
  };
  const std::vector<Fasta> fastas = {
      {"", 0, 0},
      {">a\nACGT\n>b x\nGG", 2, 0},
      {">a\nACGT\n>b x\nGG", 1, U},
      {"> a\nACGT\n", 1, U},
      {">\nACGT\n", 1, U},
      {">", 1, U},
      {">a\r\nAC\r\n", 1, 0},
      {"ACGT\n>a\nGG\n", 2, U},
      {"\n>a\nGG\n", 1, U},
      {">a\nAC>GT\n", 1, 0},
      {">a\n>b\nGG\n", 1, U},
  };
  for (const Fasta& f : fastas) {
    std::vector<char> text(f.text.begin(), f.text.end());
    expect(magot_mask_fasta_check(text.data(), text.size(), f.n) == f.want,
           "magot_mask_fasta_check: status", f.text);
  }
  printf("mask_plan_check: %d check failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
