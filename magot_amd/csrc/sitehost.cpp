// Host side of composition_by_site (genome_tools.py:488-503): from the counts
// of a, t, c, g per site to the text the tool prints -- "a\tt\tc\tg\n", then
// per site str(count * 1.0 / total) of the four, total being their sum.  Host
// only.
//
// str(float) is Python 2's: '%.12g', and ".0" appended when the result has
// neither '.' nor 'e' (nor is inf or nan, which a ratio never is).  glibc's
// printf rounds the exact binary value correctly, as Python's own conversion
// does, and the quotient is taken in double as the tool takes it.
//
// Every total is checked before a byte is written: a site without a counted
// base is the tool's ZeroDivisionError, raised before it prints anything.
// Sites are rendered in parallel over ranges; count == 0 and count == total
// are short-cut, and the ratios of totals below kSmallTotal -- all there is in
// an alignment of a few dozen rows -- are kept per thread once formatted.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

namespace magot {
namespace {

constexpr uint32_t kSmallTotal = 64;
constexpr int kMaxField = kPy2FloatMax;

struct Field {
  uint8_t len = 0;
  char text[kMaxField];
};

int site_ratio(uint32_t count, uint64_t total, char* out) {
  return py2_float_str(count * 1.0 / (double)total, out);
}

// sites [s0, s1) into `out`
void site_render_range(const uint32_t* counts, uint64_t s0, uint64_t s1, std::string* out) {
  std::vector<Field> small(kSmallTotal * kSmallTotal);
  out->reserve((s1 - s0) * 20);
  char buf[kMaxField];
  for (uint64_t s = s0; s < s1; ++s) {
    const uint32_t* c = counts + 4 * s;
    const uint64_t total = (uint64_t)c[0] + c[1] + c[2] + c[3];
    for (int k = 0; k < 4; ++k) {
      if (c[k] == 0) {
        out->append("0.0", 3);
      } else if (c[k] == total) {
        out->append("1.0", 3);
      } else if (total < kSmallTotal) {
        Field& f = small[total * kSmallTotal + c[k]];
        if (!f.len) f.len = (uint8_t)site_ratio(c[k], total, f.text);
        out->append(f.text, f.len);
      } else {
        out->append(buf, site_ratio(c[k], total, buf));
      }
      out->push_back(k == 3 ? '\n' : '\t');
    }
  }
}

}  // namespace
}  // namespace magot

extern "C" {

void magot_site_text_free(uint8_t* text) { free(text); }

int magot_site_render(const uint32_t* counts, uint64_t n_sites, uint32_t n_threads, uint8_t** text,
                      uint64_t* bytes, uint64_t* empty_site) {
  if (!text || !bytes || !empty_site || (n_sites && !counts)) {
    magot::set_error("magot_site_render: null argument");
    return MAGOT_ERR_ARG;
  }
  *text = nullptr;
  *bytes = 0;
  *empty_site = n_sites;
  for (uint64_t s = 0; s < n_sites; ++s) {
    const uint32_t* c = counts + 4 * s;
    if (!(c[0] | c[1] | c[2] | c[3])) {
      *empty_site = s;
      magot::set_error("magot_site_render: site " + std::to_string(s) + " has no counted base");
      return MAGOT_ERR_RANGE;
    }
  }
  try {
    if (!n_threads) n_threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    const uint64_t n_parts = std::max<uint64_t>(1, std::min<uint64_t>(n_threads, n_sites / 4096));
    std::vector<std::string> part(n_parts);
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> failed(n_parts);
    auto work = [&](uint64_t k) {
      try {
        magot::site_render_range(counts, n_sites * k / n_parts, n_sites * (k + 1) / n_parts,
                                 &part[k]);
      } catch (...) {
        failed[k] = std::current_exception();
      }
    };
    for (uint64_t k = 1; k < n_parts; ++k) pool.emplace_back(work, k);
    work(0);
    for (auto& th : pool) th.join();
    for (auto& e : failed)
      if (e) std::rethrow_exception(e);
    static const char kHead[] = "a\tt\tc\tg\n";
    uint64_t need = sizeof(kHead) - 1;
    for (const auto& p : part) need += p.size();
    uint8_t* out = static_cast<uint8_t*>(malloc(need));
    if (!out) throw std::bad_alloc();
    memcpy(out, kHead, sizeof(kHead) - 1);
    uint64_t at = sizeof(kHead) - 1;
    for (const auto& p : part) {
      memcpy(out + at, p.data(), p.size());
      at += p.size();
    }
    *text = out;
    *bytes = need;
  } catch (const std::exception& e) {
    magot::set_error(std::string("magot_site_render: ") + e.what());
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

}  // extern "C"
