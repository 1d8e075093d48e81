// Stand-alone check of composition_by_site's host renderer
// (magot_amd/csrc/sitehost.cpp) for a sanitizer build
// (tests/sanitize/run_site_host.py).  magot_site_render: fixed counts with the
// text known digit for digit (thirds both ways, the exponent form, 1.0 and
// 0.0), seeded counts over every path of the renderer (short-cuts, the table
// of small totals, snprintf) on 1, 3 and 16 threads against a plain
// restatement, totals above 2^32, no site at all, and an empty site first,
// last and in the middle: reported, nothing allocated.  The counts live in
// heap buffers of exactly their size.  Exit status 0 = every expectation held
// (and the sanitizers found nothing).
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

static void expect(bool ok, const char* what) {
  if (ok) return;
  ++g_failures;
  fprintf(stderr, "site_host_check: %s\n", what);
}

static std::string model(const std::vector<uint32_t>& counts) {
  std::string out = "a\tt\tc\tg\n";
  for (size_t s = 0; s < counts.size() / 4; ++s) {
    const uint32_t* c = &counts[4 * s];
    const double total = (double)((uint64_t)c[0] + c[1] + c[2] + c[3]);
    for (int k = 0; k < 4; ++k) {
      char buf[64];
      snprintf(buf, sizeof buf, "%.12g", c[k] * 1.0 / total);
      std::string f = buf;
      if (f.find('.') == std::string::npos && f.find('e') == std::string::npos) f += ".0";
      out += f;
      out += k == 3 ? '\n' : '\t';
    }
  }
  return out;
}

static void check_render(const std::vector<uint32_t>& counts, uint32_t threads,
                         const std::string& want, const char* what) {
  std::vector<uint32_t> c(counts);  // exact size
  uint8_t* text = nullptr;
  uint64_t bytes = 77, empty = 77;
  const uint64_t n = c.size() / 4;
  const int rc = magot_site_render(n ? c.data() : nullptr, n, threads, &text, &bytes, &empty);
  expect(rc == MAGOT_OK && text && empty == n, what);
  if (text) {
    expect(std::string(text, text + bytes) == want, what);
    magot_site_text_free(text);
  }
}

static void check_empty(std::vector<uint32_t> counts, uint64_t site, const char* what) {
  for (int k = 0; k < 4; ++k) counts[4 * site + k] = 0;
  uint8_t* text = reinterpret_cast<uint8_t*>(&counts);
  uint64_t bytes = 77, empty = 77;
  const int rc = magot_site_render(counts.data(), counts.size() / 4, 0, &text, &bytes, &empty);
  expect(rc == MAGOT_ERR_RANGE && !text && !bytes && empty == site, what);
}

int main() {
  check_render({1, 2, 0, 0, 3, 0, 0, 0, 1, 29999, 0, 0, 0, 0, 5, 5},
               0,
               "a\tt\tc\tg\n0.333333333333\t0.666666666667\t0.0\t0.0\n1.0\t0.0\t0.0\t0.0\n"
               "3.33333333333e-05\t0.999966666667\t0.0\t0.0\n0.0\t0.0\t0.5\t0.5\n",
               "fixed counts");
  check_render({}, 0, "a\tt\tc\tg\n", "no site");
  check_render({4294967295u, 4294967295u, 4294967295u, 1}, 1, model({4294967295u, 4294967295u,
                                                                   4294967295u, 1}),
               "a total above 2^32");

  std::mt19937_64 rng(20261020);
  std::vector<uint32_t> counts;
  const uint64_t tops[4] = {4, 70, 40000, 1ull << 32};
  for (uint64_t top : tops)
    for (int s = 0; s < 6000; ++s) {
      uint32_t c[4];
      do
        for (auto& x : c) x = (uint32_t)(rng() % top);
      while (!(c[0] | c[1] | c[2] | c[3]));
      counts.insert(counts.end(), c, c + 4);
    }
  for (uint32_t total : {63u, 64u, 65u, 30000u, 1000000u, 100000000u, 4000000000u}) {
    const uint32_t edge[12] = {total, 0, 0, 0, 1, total - 1, 0, 0, 0, 3, 0, total - 3};
    counts.insert(counts.end(), edge, edge + 12);
  }
  const std::string want = model(counts);
  expect(want.find("e-05") != std::string::npos && want.find("e-10") != std::string::npos,
         "the seeded counts lack an exponent form");
  for (uint32_t threads : {1u, 3u, 16u}) check_render(counts, threads, want, "seeded counts");

  const uint64_t n = counts.size() / 4;
  check_empty(counts, 0, "an empty first site");
  check_empty(counts, n / 2, "an empty site in the middle");
  check_empty(counts, n - 1, "an empty last site");
  {
    std::vector<uint32_t> two(counts.begin(), counts.begin() + 8);
    uint8_t* text = nullptr;
    uint64_t bytes = 0, empty = 0;
    expect(magot_site_render(nullptr, 2, 0, &text, &bytes, &empty) == MAGOT_ERR_ARG,
           "null counts accepted");
    expect(magot_site_render(two.data(), 2, 0, nullptr, &bytes, &empty) == MAGOT_ERR_ARG,
           "null text accepted");
    expect(magot_site_render(two.data(), 2, 0, &text, nullptr, &empty) == MAGOT_ERR_ARG,
           "null size accepted");
    expect(magot_site_render(two.data(), 2, 0, &text, &bytes, nullptr) == MAGOT_ERR_ARG,
           "null site accepted");
    magot_site_text_free(nullptr);
  }
  printf("site_host_check: %d check failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
