// Host-side helpers shared by the translation units that plan on the CPU
// (the abi*.hip units, tileplan.cpp): lap timing, the thread count,
// range-parallel loops, the slice carve and uninitialised arrays.  No HIP here.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

namespace magot {

// Wall-clock laps on stderr while the environment variable `env` is set.
struct Lap {
  const char* tag;
  const bool on;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit Lap(const char* env = "MAGOT_GENOME_TIMING", const char* tag_ = "genome")
      : tag(tag_), on(std::getenv(env) != nullptr) {}
  void operator()(const char* what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[%s] %-10s %.4f s\n", tag, what,
            std::chrono::duration<double>(t1 - t0).count());
    t0 = t1;
  }
};

// Host threads for staging copies and planning: the GPU's share of the host
// (OMP_NUM_THREADS on the pool's boxes), at most 16.
inline unsigned host_threads() {
  unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  if (const char* e = std::getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0) hw = (unsigned)v;
  }
  return std::min(hw, 16u);
}

// fn(lo, hi, part) over `parts` contiguous ranges of [0, n), part 0 on the
// calling thread; fn must not throw.
template <class F>
void parallel_ranges(uint64_t n, unsigned parts, F fn) {
  if (parts <= 1 || n < 2) {
    fn(0, n, 0u);
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve(parts - 1);
  for (unsigned k = 1; k < parts; ++k)
    pool.emplace_back([&fn, n, parts, k]() { fn(n * k / parts, n * (k + 1) / parts, k); });
  fn(0, n / parts, 0u);
  for (std::thread& th : pool) th.join();
}

// str(float) of Python 2 into out[kPy2FloatMax]; the bytes written.  '%.12g',
// and ".0" appended when the result has neither '.' nor 'e' (nor is inf or
// nan, which the callers' ratios never are).  glibc's printf rounds the exact
// binary value correctly, as Python's own conversion does.
constexpr int kPy2FloatMax = 24;  // "3.33333333333e-05" is 17 bytes
inline int py2_float_str(double v, char* out) {
  int n = snprintf(out, kPy2FloatMax, "%.12g", v);
  if (!memchr(out, '.', n) && !memchr(out, 'e', n)) {
    out[n++] = '.';
    out[n++] = '0';
  }
  return n;
}

// Sub-allocate 256-byte aligned slices of one allocation.  take<T>(count) gives
// a slice's offset, for the sites whose offsets are themselves the product;
// take(&field, count) sizes the slice from the field's own type and records the
// field, and place(base) sets every recorded field to base + its offset and
// forgets them.  A recorded field must not move between the two.
struct Carve {
  uint64_t used = 0;
  template <class T>
  uint64_t take(uint64_t count) {
    uint64_t at = used;
    used += (count * sizeof(T) + 255) & ~255ull;
    return at;
  }
  template <class T>
  uint64_t take(T** field, uint64_t count) {
    const uint64_t at = take<T>(count);
    slots.push_back({field, at, [](void* f, char* p) { *static_cast<T**>(f) = reinterpret_cast<T*>(p); }});
    return at;
  }
  uint64_t take(void** field, uint64_t bytes) {  // untyped scratch: a slice of bytes
    const uint64_t at = take<uint8_t>(bytes);
    slots.push_back({field, at, [](void* f, char* p) { *static_cast<void**>(f) = p; }});
    return at;
  }
  void place(void* base) {
    for (const Slot& s : slots) s.set(s.field, static_cast<char*>(base) + s.at);
    slots.clear();
  }

 private:
  struct Slot {
    void* field;
    uint64_t at;
    void (*set)(void*, char*);  // writes the field through its own type
  };
  std::vector<Slot> slots;
};

// A host array left uninitialised (POD rows the planner writes itself, in
// parallel: no sequential zero fill, and its pages fault in on the writing threads).
template <class T>
struct HostBuf {
  std::unique_ptr<T[]> p;
  uint64_t n = 0;
  explicit HostBuf(uint64_t count = 0) : p(count ? new T[count] : nullptr), n(count) {}
  T& operator[](uint64_t i) { return p[i]; }
  const T& operator[](uint64_t i) const { return p[i]; }
  T* data() { return p.get(); }
  const T* data() const { return p.get(); }
};

}  // namespace magot
