// Stand-alone check of the slice carve of the C ABI units
// (magot_amd/csrc/hostutil.h: Carve) for a sanitizer build
// (tests/sanitize/run_carve.py).  A mixed list of slices -- elements of 1, 4, 8
// and 16 bytes, a const field, an untyped scratch field, a zero count, counts
// of exactly 32, 64 and 256 elements and their neighbours -- is taken once by
// type alone and once through the fields: both give the same offsets and the
// same `used`.  place() on a heap buffer of exactly `used` bytes sets every
// field to base + its offset; every slice is then written from its first to
// its last element through the field's own type, which a sanitizer would report
// if a slice were a byte short; a second place() sets nothing.  Exit status 0 =
// every expectation held (and the sanitizers found nothing).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../magot_amd/csrc/hostutil.h"

using magot::Carve;

static int g_failures = 0;

static void expect(bool ok, const char* what) {
  if (ok) return;
  ++g_failures;
  fprintf(stderr, "carve_check: %s\n", what);
}

struct Wide {  // a 16-byte element, as PslAgg and RnSlot are
  uint64_t a, b;
};
static_assert(sizeof(Wide) == 16, "a 16-byte element");

// the fields of a handle: they stay where they are between take and place
struct Fields {
  uint8_t* bytes = nullptr;
  const uint8_t* text = nullptr;
  uint32_t* words = nullptr;
  uint32_t* words64 = nullptr;
  uint64_t* longs = nullptr;
  uint64_t* longs33 = nullptr;
  Wide* wide = nullptr;
  Wide* wide256 = nullptr;
  uint32_t* none = nullptr;
  void* scratch = nullptr;
  const uint64_t* last = nullptr;
};

static const uint64_t kCounts[11] = {256, 7, 31, 64, 32, 33, 1, 256, 0, 100, 256};

// every element from the first to the last, written through the field's type
template <class T>
static void fill(T* p, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) std::memset(&p[i], 0x5a, sizeof(T));
}

int main() {
  const uint64_t* c = kCounts;
  Carve by_type;
  const uint64_t want[11] = {
      by_type.take<uint8_t>(c[0]),  by_type.take<uint8_t>(c[1]),  by_type.take<uint32_t>(c[2]),
      by_type.take<uint32_t>(c[3]), by_type.take<uint64_t>(c[4]), by_type.take<uint64_t>(c[5]),
      by_type.take<Wide>(c[6]),     by_type.take<Wide>(c[7]),     by_type.take<uint32_t>(c[8]),
      by_type.take<uint8_t>(c[9]),  by_type.take<uint64_t>(c[10])};

  auto f = std::make_unique<Fields>();
  Carve cv;
  const uint64_t got[11] = {
      cv.take(&f->bytes, c[0]),   cv.take(&f->text, c[1]),  cv.take(&f->words, c[2]),
      cv.take(&f->words64, c[3]), cv.take(&f->longs, c[4]), cv.take(&f->longs33, c[5]),
      cv.take(&f->wide, c[6]),    cv.take(&f->wide256, c[7]), cv.take(&f->none, c[8]),
      cv.take(&f->scratch, c[9]), cv.take(&f->last, c[10])};
  expect(cv.used == by_type.used, "take(&field, n) and take<T>(n) disagree on `used`");
  for (int k = 0; k < 11; ++k) {
    expect(got[k] == want[k], "take(&field, n) and take<T>(n) disagree on an offset");
    expect(got[k] % 256 == 0, "an offset is not 256-byte aligned");
  }
  // 256 bytes exactly fill a slice: the next begins right behind it
  expect(want[1] == 256 && want[4] - want[3] == 256 && want[5] - want[4] == 256 &&
             want[8] - want[7] == 4096 && want[9] == want[8],
         "an exact multiple of 256 bytes, or a zero count, moved `used` wrongly");
  expect(f->bytes == nullptr && f->last == nullptr, "take() wrote a field before place()");

  // a buffer of exactly `used` bytes: ASan guards both ends
  std::unique_ptr<char[]> mem(new char[cv.used]);
  char* base = mem.get();
  cv.place(base);
  static_assert(std::is_same<decltype(f->text), const uint8_t*>::value, "the const field");
  const void* at[11] = {f->bytes,   f->text,    f->words, f->words64, f->longs, f->longs33,
                        f->wide,    f->wide256, f->none,  f->scratch, f->last};
  for (int k = 0; k < 11; ++k)
    expect(at[k] == base + want[k], "place() set a field to another address than base + offset");

  fill(f->bytes, c[0]);
  fill(const_cast<uint8_t*>(f->text), c[1]);
  fill(f->words, c[2]);
  fill(f->words64, c[3]);
  fill(f->longs, c[4]);
  fill(f->longs33, c[5]);
  fill(f->wide, c[6]);
  fill(f->wide256, c[7]);
  fill(f->none, c[8]);
  fill(static_cast<uint8_t*>(f->scratch), c[9]);
  fill(const_cast<uint64_t*>(f->last), c[10]);
  expect(f->wide256[255].b == 0x5a5a5a5a5a5a5a5aull && f->last[255] == 0x5a5a5a5a5a5a5a5aull,
         "the last element of a slice does not hold what was written");
  expect(static_cast<const void*>(&f->last[255] + 1) == base + cv.used,
         "the last slice does not end where the buffer ends");

  // the fields are forgotten: another place() moves nothing
  std::unique_ptr<char[]> other(new char[cv.used]);
  cv.place(other.get());
  const void* again[11] = {f->bytes,   f->text,    f->words, f->words64, f->longs, f->longs33,
                           f->wide,    f->wide256, f->none,  f->scratch, f->last};
  for (int k = 0; k < 11; ++k) expect(again[k] == at[k], "a second place() set a field");

  // a carve goes on after place(): offsets continue, only the new field is set
  uint32_t* more = nullptr;
  const uint64_t used = cv.used;
  expect(cv.take(&more, 64) == used && cv.used == used + 256, "a take after place()");
  std::unique_ptr<char[]> grown(new char[cv.used]);
  cv.place(grown.get());
  expect(static_cast<const void*>(more) == grown.get() + used && f->bytes == at[0],
         "place() after a later take");
  fill(more, 64);

  printf("carve_check: %d check failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
