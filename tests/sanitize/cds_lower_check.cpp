// Stand-alone driver of the get_CDS_peptides lowering (magot_gff_read +
// magot_gff_lower_cds, magot_amd/csrc/gffplan.cpp) for a host-only build under
// AddressSanitizer + UBSan (tests/sanitize/run_cds_lower.py).  Its argument is
// a listing, one case per line, tab separated:
//   gff file, contigs file (name TAB length per line), py2 order (0/1),
//   names_from (0..2), length filter ("-": none), filters (joined by \x01, may
//   be empty), expected file ("-": the lowering, or the read before it, has to
//   decline)
// The expected file holds, per record in output order, name TAB bases TAB
// transcript group; the driver prints its own table the same way and compares
// the bytes.  Every view the lowering hands out is read to its last element.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/magot.h"

namespace magot {
void set_error(const std::string&) {}
}  // namespace magot

namespace {

int failures = 0;

void fail(const std::string& what) {
  ++failures;
  printf("FAIL: %s\n", what.c_str());
}

std::string slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  std::ostringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  size_t b = 0;
  for (;;) {
    const size_t e = s.find(sep, b);
    out.push_back(s.substr(b, e == std::string::npos ? std::string::npos : e - b));
    if (e == std::string::npos) return out;
    b = e + 1;
  }
}

void run_case(const std::vector<std::string>& f) {
  const std::string gff = slurp(f[0]);
  std::vector<std::string> names;
  std::vector<uint64_t> lens;
  for (const std::string& line : split(slurp(f[1]), '\n')) {
    if (line.empty()) continue;
    const std::vector<std::string> c = split(line, '\t');
    names.push_back(c[0]);
    lens.push_back(strtoull(c[1].c_str(), nullptr, 10));
  }
  std::vector<const char*> name_ptr;
  for (const std::string& s : names) name_ptr.push_back(s.c_str());
  std::vector<std::string> filters;
  if (!f[5].empty()) filters = split(f[5], '\x01');
  std::vector<const char*> filter_ptr;
  for (const std::string& s : filters) filter_ptr.push_back(s.c_str());
  const int64_t len_filter = f[4] == "-" ? 0 : strtoll(f[4].c_str(), nullptr, 10);
  magot_gffplan* p = nullptr;
  const int read_rc = magot_gff_read(gff.data(), gff.size(), 0, &p);
  if (read_rc != MAGOT_OK) {
    // read_gff returns None: no annotations, so nothing to lower (a decline)
    if (read_rc != MAGOT_ERR_UNSUPPORTED || f[6] != "-") fail(f[0] + ": magot_gff_read");
    magot_gffplan_destroy(p);
    return;
  }
  uint64_t n_rec = 0, n_groups = 0;
  const int rc = magot_gff_lower_cds(
      p, name_ptr.data(), lens.data(), (uint32_t)names.size(), filter_ptr.data(),
      (uint32_t)filters.size(), f[4] == "-" ? nullptr : &len_filter, (uint32_t)atoi(f[3].c_str()),
      atoi(f[2].c_str()) ? MAGOT_GFF_ORDER_PY2 : 0u, &n_rec, &n_groups);
  if (f[6] == "-") {
    if (rc != MAGOT_ERR_UNSUPPORTED) fail(f[0] + ": not declined");
  } else if (rc != MAGOT_OK) {
    fail(f[0] + ": declined or failed");
  } else {
    const magot_exon* ex = nullptr;
    const magot_tx* tx = nullptr;
    const uint64_t *noff = nullptr, *goff = nullptr;
    const uint8_t* blob = nullptr;
    if (magot_gffplan_table_views(p, &ex, &tx) != MAGOT_OK ||
        magot_gffplan_cds_views(p, &noff, &blob, &goff) != MAGOT_OK) {
      fail(f[0] + ": views");
    } else {
      std::string got;
      uint64_t g = 0;
      for (uint64_t r = 0; r < n_rec; ++r) {
        while (g + 1 < n_groups && goff[g + 1] <= r) ++g;
        if (tx[r].n_exons != 1 || tx[r].exon_begin != r) fail(f[0] + ": record shape");
        got.append(reinterpret_cast<const char*>(blob) + noff[r], noff[r + 1] - noff[r]);
        got += '\t' + std::to_string(ex[r].len) + '\t' + std::to_string(g) + '\n';
      }
      if (goff[0] != 0 || goff[n_groups] != n_rec) fail(f[0] + ": group bounds");
      if (got != slurp(f[6])) fail(f[0] + " -> " + f[6] + ": table differs");
    }
    if (magot_gff_lower_cds(p, name_ptr.data(), lens.data(), (uint32_t)names.size(), nullptr, 0,
                            nullptr, 0, 0, nullptr, nullptr) != MAGOT_ERR_STATE)
      fail(f[0] + ": lowered twice");
  }
  magot_gffplan_destroy(p);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  int n = 0;
  for (const std::string& line : split(slurp(argv[1]), '\n')) {
    if (line.empty()) continue;
    const std::vector<std::string> f = split(line, '\t');
    if (f.size() != 7) {
      fail("listing line");
      continue;
    }
    run_case(f);
    ++n;
  }
  printf("cds_lower_check: %d case(s), %d check failure(s)\n", n, failures);
  return failures ? 1 : 0;
}
