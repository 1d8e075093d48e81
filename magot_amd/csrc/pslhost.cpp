// Host side of besthits_from_psl (genome_tools.py:572-592): the order in which
// a CPython 2.7 dict iterates the winners' keys, from the hashes the device
// computed, and the copy of the printed lines.  Host only.
//
// The dict model is that of magot_amd/py2order.py, with
// equality as identity: the n keys are distinct, so a probe never finds its
// own key and every insertion is a new one.
//   * lookdict: i = h & mask, then i = 5 i + perturb + 1, perturb >>= 5;
//   * after an insertion with fill * 3 >= size * 2 the table is rebuilt at the
//     smallest power of two above (used > 50000 ? 2 : 4) * used, the entries
//     re-inserted in slot order.
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "common.h"

namespace magot {
namespace {

void psl_place(std::vector<int64_t>& tab, const uint64_t* hash, int64_t k) {
  const uint64_t mask = tab.size() - 1, h = hash[k];
  uint64_t i = h & mask, perturb = h;
  while (tab[i & mask] >= 0) {  // the table is never full: it ends
    i = i * 5 + perturb + 1;
    perturb >>= 5;
  }
  tab[i & mask] = k;
}

}  // namespace
}  // namespace magot

extern "C" {

int magot_psl_order(const uint64_t* hash, uint64_t n, uint64_t* perm) {
  if (n && (!hash || !perm)) {
    magot::set_error("magot_psl_order: null argument");
    return MAGOT_ERR_ARG;
  }
  try {
    std::vector<int64_t> slots(8, -1);
    uint64_t used = 0;
    for (uint64_t k = 0; k < n; ++k) {
      magot::psl_place(slots, hash, (int64_t)k);
      ++used;
      if (used * 3 >= slots.size() * 2) {
        const uint64_t want = (used > 50000 ? 2 : 4) * used;
        uint64_t size = 8;
        while (size <= want) size <<= 1;
        std::vector<int64_t> fresh(size, -1);
        for (int64_t k2 : slots)
          if (k2 >= 0) magot::psl_place(fresh, hash, k2);
        slots.swap(fresh);
      }
    }
    uint64_t at = 0;
    for (int64_t k : slots)
      if (k >= 0) perm[at++] = (uint64_t)k;
  } catch (const std::exception& e) {
    magot::set_error(std::string("magot_psl_order: ") + e.what());
    return MAGOT_ERR_ARG;
  }
  return MAGOT_OK;
}

int magot_psl_render(const char* text, uint64_t len, const uint64_t* off, const uint64_t* row_len,
                     uint64_t n, int whole, uint8_t* out, uint64_t cap, uint64_t* bytes) {
  if (!bytes || (len && !text) || (n && (!off || !row_len))) {
    magot::set_error("magot_psl_render: null argument");
    return MAGOT_ERR_ARG;
  }
  uint64_t need = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (off[i] > len || row_len[i] > len - off[i] || (!whole && !row_len[i])) {
      magot::set_error("magot_psl_render: a row outside the text, or an empty one");
      return MAGOT_ERR_RANGE;
    }
    // `print line[:-1]`: the line without its last byte (its LF, or the last
    // byte of a final line that has none), then '\n'; `print line`: all of it
    need += row_len[i] + (whole ? 1 : 0);
  }
  *bytes = need;
  if (!out) return MAGOT_OK;
  if (cap < need) {
    magot::set_error("magot_psl_render: output buffer too small");
    return MAGOT_ERR_ARG;
  }
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t body = row_len[i] - (whole ? 0 : 1);
    if (body) memcpy(out + at, text + off[i], body);
    at += body;
    out[at++] = '\n';
  }
  return MAGOT_OK;
}

}  // extern "C"
