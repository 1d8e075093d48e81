// Host side of heterozygosity_from_vcf (magot_variants.py:72-88): from the het
// counts per locus and sample to the string the function returns -- per locus
// of positive length "locus,rate,rate,...", the rows joined by LF with none at
// the end.  Host only.
//
// A rate is str(100.0 * count / seqlen): the product and the quotient in
// double, as the function takes them, printed as Python 2 prints a float
// (hostutil.h's py2_float_str, which sitehost.cpp uses too).  Loci are rendered
// in parallel over ranges.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

namespace magot {
namespace {

void vcf_render_range(const char* loci, const uint64_t* loci_off, const int64_t* seqlen,
                      const uint32_t* counts, uint32_t n_samples, const uint32_t* cols,
                      uint32_t n_cols, uint64_t l0, uint64_t l1, std::string* out) {
  char buf[kPy2FloatMax];
  for (uint64_t l = l0; l < l1; ++l) {
    if (seqlen[l] < 1) continue;
    out->append(loci + loci_off[l], loci_off[l + 1] - loci_off[l]);
    const uint32_t* row = counts + l * n_samples;
    const double len = (double)seqlen[l];
    for (uint32_t c = 0; c < n_cols; ++c) {
      out->push_back(',');
      const uint32_t v = row[cols[c]];
      if (!v) out->append("0.0", 3);
      else out->append(buf, py2_float_str(100.0 * v / len, buf));
    }
    out->push_back('\n');
  }
}

}  // namespace
}  // namespace magot

extern "C" {

int magot_vcf_render(const char* loci, const uint64_t* loci_off, const int64_t* seqlen,
                     const uint32_t* counts, uint64_t n_loci, uint32_t n_samples,
                     const uint32_t* cols, uint32_t n_cols, uint32_t n_threads, uint8_t** text,
                     uint64_t* bytes) {
  if (!text || !bytes || (n_loci && (!loci || !loci_off || !seqlen || (n_cols && !counts))) ||
      (n_cols && !cols)) {
    magot::set_error("magot_vcf_render: null argument");
    return MAGOT_ERR_ARG;
  }
  *text = nullptr;
  *bytes = 0;
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= n_samples) {
      magot::set_error("magot_vcf_render: a column beyond the samples");
      return MAGOT_ERR_RANGE;
    }
  for (uint64_t l = 0; l < n_loci; ++l)
    if (loci_off[l + 1] < loci_off[l]) {
      magot::set_error("magot_vcf_render: locus offsets that fall");
      return MAGOT_ERR_RANGE;
    }
  try {
    if (!n_threads) n_threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    const uint64_t n_parts = std::max<uint64_t>(1, std::min<uint64_t>(n_threads, n_loci / 1024));
    std::vector<std::string> part(n_parts);
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> failed(n_parts);
    auto work = [&](uint64_t k) {
      try {
        magot::vcf_render_range(loci, loci_off, seqlen, counts, n_samples, cols, n_cols,
                                n_loci * k / n_parts, n_loci * (k + 1) / n_parts, &part[k]);
      } catch (...) {
        failed[k] = std::current_exception();
      }
    };
    for (uint64_t k = 1; k < n_parts; ++k) pool.emplace_back(work, k);
    work(0);
    for (auto& th : pool) th.join();
    for (auto& e : failed)
      if (e) std::rethrow_exception(e);
    uint64_t need = 0;
    for (const auto& p : part) need += p.size();
    if (need) --need;  // the rows are joined: no LF behind the last
    uint8_t* out = static_cast<uint8_t*>(malloc(need ? need : 1));
    if (!out) throw std::bad_alloc();
    uint64_t at = 0;
    for (const auto& p : part) {
      const uint64_t n = std::min<uint64_t>(p.size(), need - at);
      memcpy(out + at, p.data(), n);
      at += n;
    }
    *text = out;
    *bytes = need;
  } catch (const std::exception& e) {
    magot::set_error(std::string("magot_vcf_render: ") + e.what());
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

}  // extern "C"
