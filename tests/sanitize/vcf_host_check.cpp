// Stand-alone check of heterozygosity_from_vcf's host renderer
// (magot_amd/csrc/vcfhost.cpp) for a sanitizer build
// (tests/sanitize/run_vcf_host.py).  magot_vcf_render: fixed counts with the
// text known digit for digit (thirds, the exponent form, 0.0, a rate above
// 100), loci of length 0 and below left out, seeded counts on 1, 3 and 16
// threads against a plain restatement, no locus, no column, every locus left
// out, a column beyond the samples refused.  Every table lives in a heap buffer
// of exactly its size.  Exit status 0 = every expectation held (and the
// sanitizers found nothing).
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

extern "C" void magot_site_text_free(uint8_t* text) { free(text); }  // sitehost.cpp's, not linked

static int g_failures = 0;

static void expect(bool ok, const char* what) {
  if (ok) return;
  ++g_failures;
  fprintf(stderr, "vcf_host_check: %s\n", what);
}

struct World {
  std::vector<std::string> loci;
  std::vector<int64_t> seqlen;
  std::vector<uint32_t> counts;  // loci x samples
  uint32_t samples = 0;
  std::vector<uint32_t> cols;
};

static std::string model(const World& w) {
  std::string out;
  bool any = false;
  for (size_t l = 0; l < w.loci.size(); ++l) {
    if (w.seqlen[l] < 1) continue;
    if (any) out += '\n';
    any = true;
    out += w.loci[l];
    for (uint32_t c : w.cols) {
      char buf[64];
      snprintf(buf, sizeof buf, "%.12g", 100.0 * w.counts[l * w.samples + c] / (double)w.seqlen[l]);
      std::string f = buf;
      if (f.find('.') == std::string::npos && f.find('e') == std::string::npos) f += ".0";
      out += ',';
      out += f;
    }
  }
  return out;
}

static void check_render(const World& w, uint32_t threads, const std::string& want,
                         const char* what) {
  std::string blob;
  std::vector<uint64_t> off(w.loci.size() + 1, 0);  // exact sizes throughout
  for (size_t l = 0; l < w.loci.size(); ++l) {
    blob += w.loci[l];
    off[l + 1] = blob.size();
  }
  std::vector<char> text_in(blob.begin(), blob.end());
  std::vector<int64_t> seqlen(w.seqlen);
  std::vector<uint32_t> counts(w.counts), cols(w.cols);
  uint8_t* text = nullptr;
  uint64_t bytes = 77;
  const uint64_t n = w.loci.size();
  const int rc = magot_vcf_render(n ? text_in.data() : nullptr, off.data(),
                                  n ? seqlen.data() : nullptr,
                                  counts.empty() ? nullptr : counts.data(), n, w.samples,
                                  cols.empty() ? nullptr : cols.data(), (uint32_t)cols.size(),
                                  threads, &text, &bytes);
  expect(rc == MAGOT_OK && text, what);
  if (text) {
    expect(std::string(text, text + bytes) == want, what);
    magot_site_text_free(text);
  }
}

int main() {
  {
    World w;
    w.loci = {"c1,1,3", "c1,4,3", "c2,30000", "c1,5,5", "c3,-2", "c1,1,7"};
    w.seqlen = {3, 0, 30000, 1, -2, 7};
    w.samples = 3;
    w.counts = {1, 2, 0, 9, 9, 9, 1, 29999, 0, 2, 0, 1, 5, 5, 5, 1, 3, 7};
    w.cols = {1, 0, 2};
    check_render(w, 0,
                 "c1,1,3,66.6666666667,33.3333333333,0.0\n"
                 "c2,30000,99.9966666667,0.00333333333333,0.0\n"
                 "c1,5,5,0.0,200.0,100.0\n"
                 "c1,1,7,42.8571428571,14.2857142857,100.0",
                 "fixed counts");
    expect(model(w).find("0.00333333333333") != std::string::npos, "the model's own floats");
    World none = w;
    none.seqlen = {0, 0, -1, 0, -2, 0};
    check_render(none, 0, "", "every locus left out");
    World bare = w;
    bare.cols.clear();
    check_render(bare, 1, "c1,1,3\nc2,30000\nc1,5,5\nc1,1,7", "no column");
  }
  {
    World w;
    w.samples = 4;
    w.cols = {0, 3};
    check_render(w, 0, "", "no locus");
  }
  std::mt19937_64 rng(20261020);
  World w;
  w.samples = 5;
  w.cols = {4, 0, 2, 2};
  const int64_t lens[6] = {1, 3, 7, 10000, 1000000000, 1ll << 40};
  for (int l = 0; l < 20000; ++l) {
    w.loci.push_back("ctg" + std::to_string(l % 17) + "," + std::to_string(l));
    w.seqlen.push_back(l % 11 == 0 ? (int64_t)(rng() % 5) - 3 : lens[rng() % 6]);
    for (uint32_t s = 0; s < w.samples; ++s)
      w.counts.push_back(l % 7 == 0 ? 0 : (uint32_t)(rng() % (l % 5 == 0 ? 1ull << 32 : 40)));
  }
  const std::string want = model(w);
  expect(want.find("e-0") != std::string::npos && want.find(",0.0") != std::string::npos,
         "the seeded counts lack a form");
  for (uint32_t threads : {1u, 3u, 16u}) check_render(w, threads, want, "seeded counts");
  {
    std::vector<uint64_t> off = {0, 2};
    std::vector<int64_t> seqlen = {5};
    std::vector<uint32_t> counts = {1, 2}, cols = {2};
    const char loci[2] = {'c', '1'};
    uint8_t* text = nullptr;
    uint64_t bytes = 0;
    expect(magot_vcf_render(loci, off.data(), seqlen.data(), counts.data(), 1, 2, cols.data(), 1, 0,
                            &text, &bytes) == MAGOT_ERR_RANGE && !text,
           "a column beyond the samples accepted");
    expect(magot_vcf_render(nullptr, off.data(), seqlen.data(), counts.data(), 1, 2, cols.data(), 1,
                            0, &text, &bytes) == MAGOT_ERR_ARG,
           "null loci accepted");
    expect(magot_vcf_render(loci, off.data(), seqlen.data(), counts.data(), 1, 2, cols.data(), 1, 0,
                            nullptr, &bytes) == MAGOT_ERR_ARG,
           "null text accepted");
    expect(magot_vcf_render(loci, off.data(), seqlen.data(), counts.data(), 1, 2, cols.data(), 1, 0,
                            &text, nullptr) == MAGOT_ERR_ARG,
           "null size accepted");
    off = {2, 0};
    expect(magot_vcf_render(loci, off.data(), seqlen.data(), counts.data(), 1, 2, cols.data(), 0, 0,
                            &text, &bytes) == MAGOT_ERR_RANGE,
           "falling offsets accepted");
  }
  printf("vcf_host_check: %d check failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
