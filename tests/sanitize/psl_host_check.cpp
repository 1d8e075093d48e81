// Stand-alone check of besthits_from_psl's two host functions
// (magot_amd/csrc/pslhost.cpp) for a sanitizer build
// (tests/sanitize/run_psl_host.py).  magot_psl_order: fixed hash arrays, sizes
// around every resize, seeded arrays whose low bits repeat, each result checked
// to be a permutation and against a plain restatement of the dict model.
// magot_psl_render: fixed rows, a last row without LF, zero rows, both modes,
// every output written into a heap buffer of exactly the size asked for, and
// rows outside the text refused.  Exit status 0 = every expectation held (and
// the sanitizers found nothing).
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
  fprintf(stderr, "psl_host_check: %s\n", what);
}

// the model of magot_amd/py2order.py over indices, one key at a time
static std::vector<uint64_t> model_order(const std::vector<uint64_t>& hash) {
  std::vector<long long> slots(8, -1);
  auto place = [&](std::vector<long long>& tab, long long k) {
    const uint64_t mask = tab.size() - 1;
    uint64_t i = hash[k] & mask, perturb = hash[k];
    while (tab[i & mask] >= 0) {
      i = i * 5 + perturb + 1;
      perturb >>= 5;
    }
    tab[i & mask] = k;
  };
  uint64_t used = 0;
  for (size_t k = 0; k < hash.size(); ++k) {
    place(slots, (long long)k);
    ++used;
    if (used * 3 >= slots.size() * 2) {
      uint64_t size = 8;
      while (size <= (used > 50000 ? 2 : 4) * used) size <<= 1;
      std::vector<long long> fresh(size, -1);
      for (long long k2 : slots)
        if (k2 >= 0) place(fresh, k2);
      slots.swap(fresh);
    }
  }
  std::vector<uint64_t> out;
  for (long long k : slots)
    if (k >= 0) out.push_back((uint64_t)k);
  return out;
}

static void check_order(const std::vector<uint64_t>& hash, const char* what) {
  // exact-size heap buffers: a write past perm is a sanitizer finding
  std::vector<uint64_t> h(hash), perm(hash.size(), ~0ull);
  const int rc = magot_psl_order(h.empty() ? nullptr : h.data(), h.size(),
                                 perm.empty() ? nullptr : perm.data());
  expect(rc == MAGOT_OK, what);
  std::vector<char> seen(hash.size(), 0);
  for (uint64_t k : perm) {
    expect(k < hash.size() && !seen[k], "not a permutation");
    if (k < hash.size()) seen[k] = 1;
  }
  expect(perm == model_order(hash), what);
}

static void check_render(const std::string& text, const std::vector<uint64_t>& off,
                         const std::vector<uint64_t>& len, int whole, const std::string& want) {
  std::vector<char> t(text.begin(), text.end());
  uint64_t need = 77;
  const uint64_t n = off.size();
  int rc = magot_psl_render(t.data(), t.size(), n ? off.data() : nullptr, n ? len.data() : nullptr,
                            n, whole, nullptr, 0, &need);
  expect(rc == MAGOT_OK && need == want.size(), "render: size");
  std::vector<uint8_t> out(need);
  rc = magot_psl_render(t.data(), t.size(), n ? off.data() : nullptr, n ? len.data() : nullptr, n,
                        whole, out.data(), out.size(), &need);
  expect(rc == MAGOT_OK, "render: status");
  expect(std::string(out.begin(), out.end()) == want, "render: bytes");
  if (need) {
    std::vector<uint8_t> small(need);  // not null even when one byte is asked for
    rc = magot_psl_render(t.data(), t.size(), off.data(), len.data(), n, whole, small.data(),
                          need - 1, &need);
    expect(rc == MAGOT_ERR_ARG, "render: a buffer too small was accepted");
  }
}

int main() {
  check_order({}, "no keys");
  check_order({0}, "one key");
  check_order({5, 13, 21, 29, 37}, "five keys in one slot");
  check_order({5, 13, 21, 29, 37, 45}, "the first resize");
  check_order({~0ull - 1, 0, 1ull << 63, 7, 7 + 8, 7 + 16, 7 + 32}, "large hashes");
  std::mt19937_64 rng(20261020);
  for (uint64_t n : {2u, 7u, 21u, 22u, 85u, 86u, 341u, 342u, 1000u, 5462u, 60000u}) {
    std::vector<uint64_t> h(n);
    for (auto& x : h) x = rng();
    check_order(h, "random hashes");
    // the low bits repeat: long probe chains, perturb doing the work
    for (auto& x : h) x = (x << 12) | (rng() % 3);
    check_order(h, "hashes with few low bits");
  }
  {
    std::vector<uint64_t> h(3000);
    for (size_t k = 0; k < h.size(); ++k) h[k] = (uint64_t)k << 40;  // equal in the low 40 bits
    check_order(h, "hashes equal in the low 40 bits");
  }

  const std::string text = "first line\n\nabc\r\nlast without lf";
  check_render(text, {0, 11, 12, 17, 0}, {11, 1, 5, 15, 11}, 0,
               "first line\n\nabc\r\nlast without l\nfirst line\n");
  check_render(text, {0, 11, 17}, {11, 1, 15}, 1, "first line\n\n\n\nlast without lf\n");
  check_render(text, {}, {}, 0, "");
  check_render("", {}, {}, 1, "");
  check_render("", {0}, {0}, 1, "\n");
  check_render("x", {0}, {1}, 0, "\n");
  {
    uint64_t need = 0;
    const uint64_t off[4] = {33, 30, 0, 1ull << 63}, len[4] = {1, 3, 0, 1ull << 63};
    for (int k = 0; k < 4; ++k)
      expect(magot_psl_render(text.data(), text.size(), off + k, len + k, 1, 0, nullptr, 0,
                              &need) == MAGOT_ERR_RANGE,
             "render: a row outside the text was accepted");
    expect(magot_psl_render(text.data(), text.size(), off, len, 1, 0, nullptr, 0, nullptr) ==
               MAGOT_ERR_ARG,
           "render: null size accepted");
    expect(magot_psl_order(nullptr, 3, nullptr) == MAGOT_ERR_ARG, "order: null accepted");
  }
  printf("psl_host_check: %d check failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
