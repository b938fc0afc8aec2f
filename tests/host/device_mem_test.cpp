// Buffer and Array of csrc/device_mem.hpp on a malloc-backed policy that logs what it is asked: the growth rule, the order of
// release and request, what a refusal leaves behind, moves, and the borrowed-or-owned array.  Built with
// -fsanitize=address,undefined and run by tests/test_device_mem_host.py; exit status 0 = every check held, nothing leaked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../neuralbarkcalculator_amd/csrc/device_mem.hpp"

namespace {

struct Entry {
  char what;      // 'a' allocate, 'r' release, 'x' refused allocate, 'c' copy, 'f' forget_error
  void* p;
  size_t bytes;
};

struct TestMem {
  using Error = int;
  static constexpr Error ok() { return 0; }
  static constexpr Error kRefused = 2, kCopyFailed = 3;
  static std::vector<Entry> log;
  static int live;
  static size_t limit;          // an allocate above this many bytes is refused
  static bool fail_copy;

  static Error allocate(void** p, size_t bytes) {
    if (bytes > limit) { log.push_back({'x', nullptr, bytes}); return kRefused; }
    *p = std::malloc(bytes);
    ++live;
    log.push_back({'a', *p, bytes});
    return ok();
  }
  static void release(void* p) {
    std::free(p);
    --live;
    log.push_back({'r', p, 0});
  }
  static void forget_error() { log.push_back({'f', nullptr, 0}); }
  static Error copy_in(void* dst, const void* host, size_t bytes) {
    if (fail_copy) return kCopyFailed;
    std::memcpy(dst, host, bytes);
    log.push_back({'c', dst, bytes});
    return ok();
  }
  static void fresh(size_t new_limit = ~size_t(0)) { log.clear(); limit = new_limit; fail_copy = false; }
  static std::string ops() {      // the log's letters in order
    std::string s;
    for (const Entry& e : log) s += e.what;
    return s;
  }
};
std::vector<Entry> TestMem::log;
int TestMem::live = 0;
size_t TestMem::limit = ~size_t(0);
bool TestMem::fail_copy = false;

using Buf = nbc::Buffer<TestMem>;
using Arr = nbc::Array<float, TestMem>;
using nbc::Grow;

int failures = 0;
#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

void reserve_that_fits_allocates_nothing() {
  TestMem::fresh();
  Buf b;
  CHECK(!b && b.capacity() == 0);
  CHECK(b.reserve(0) == 0 && TestMem::ops().empty() && !b);
  CHECK(b.reserve(100) == 0 && b && b.capacity() == 100);
  void* p = b.get();
  std::memset(p, 0xab, 100);                   // the block is really that large (the sanitizer watches)
  TestMem::log.clear();
  CHECK(b.reserve(100) == 0 && b.reserve(1, Grow::kMargin) == 0 && b.reserve(0) == 0);
  CHECK(TestMem::ops().empty() && b.get() == p && b.capacity() == 100);
}

void margin_growth_releases_before_it_requests() {
  TestMem::fresh();
  Buf b;
  CHECK(b.reserve(100, Grow::kMargin) == 0 && b.capacity() == 100);      // nothing to grow from: the exact size
  void* old = b.get();
  CHECK(b.reserve(101, Grow::kMargin) == 0);
  CHECK(b.capacity() >= 150);
  std::memset(b.get(), 1, b.capacity());
  CHECK(TestMem::ops() == "ara");
  CHECK(TestMem::log[1].p == old && TestMem::log[2].bytes == b.capacity());
  CHECK(b.reserve(1000, Grow::kMargin) == 0 && b.capacity() == 1000);    // max(need, cap + cap / 2)
  CHECK(TestMem::live == 1);
  // the exact policy asks for `need` and nothing else
  Buf e;
  CHECK(e.reserve(100) == 0 && e.reserve(101) == 0 && e.capacity() == 101);
}

void margin_refused_falls_back_to_exact() {
  TestMem::fresh();
  Buf b;
  CHECK(b.reserve(100, Grow::kMargin) == 0);
  TestMem::log.clear();
  TestMem::limit = 101;
  CHECK(b.reserve(101, Grow::kMargin) == 0);
  CHECK(b && b.capacity() == 101);
  CHECK(TestMem::ops() == "rxfa");             // release, the margin refused, the error forgotten, exactly `need`
  CHECK(TestMem::log[1].bytes == 150 && TestMem::log[3].bytes == 101);
  std::memset(b.get(), 2, 101);
}

void refused_reserve_leaves_the_buffer_empty() {
  for (Grow g : {Grow::kExact, Grow::kMargin}) {
    TestMem::fresh();
    Buf b;
    CHECK(b.reserve(100, g) == 0);
    TestMem::limit = 100;
    TestMem::log.clear();
    CHECK(b.reserve(101, g) == TestMem::kRefused);
    CHECK(!b && b.get() == nullptr && b.capacity() == 0 && TestMem::live == 0);
    CHECK(TestMem::ops() == (g == Grow::kMargin ? "rxfx" : "rx"));
    TestMem::limit = 1000;
    CHECK(b.reserve(101, g) == 0 && b && b.capacity() == 101);
    std::memset(b.get(), 3, 101);
  }
}

void moves_leave_the_source_empty() {
  TestMem::fresh();
  {
    Buf a;
    CHECK(a.reserve(64) == 0);
    void* p = a.get();
    Buf b(std::move(a));
    CHECK(!a && a.capacity() == 0 && b.get() == p && b.capacity() == 64);
    Buf c;
    CHECK(c.reserve(32) == 0);
    void* pc = c.get();
    TestMem::log.clear();
    c = std::move(b);                          // releases what it held, takes the other
    CHECK(!b && c.get() == p && c.capacity() == 64);
    CHECK(TestMem::ops() == "r" && TestMem::log[0].p == pc);
    Buf& same = c;
    c = std::move(same);                       // onto itself: nothing
    CHECK(c.get() == p && TestMem::live == 1);
    CHECK(a.reserve(16) == 0 && a.capacity() == 16);   // a moved-from buffer is an empty one
    std::vector<Buf> v(3);
    CHECK(v[1].reserve(8) == 0);
    v.resize(64);                              // reallocates: moves
    CHECK(v[1].capacity() == 8 && TestMem::live == 3);
  }
  CHECK(TestMem::live == 0);                   // moved-from and moved-to both destructed, each block released once
}

void array_attach_and_upload() {
  TestMem::fresh();
  const float host[4] = {1.f, 2.f, 3.f, 4.f}, host2[2] = {5.f, 6.f};
  float borrowed[3] = {7.f, 8.f, 9.f};
  {
    Arr a;
    CHECK(a.data() == nullptr && a.count() == 0);
    a.attach(borrowed, 3);                     // nothing owned: nothing released
    CHECK(a.data() == borrowed && a.count() == 3 && TestMem::ops().empty());
    CHECK(a.upload(host, 4) == 0);
    CHECK(a.count() == 4 && std::memcmp(a.data(), host, sizeof(host)) == 0 && TestMem::ops() == "ac" && TestMem::live == 1);
    const float* own = a.data();
    TestMem::log.clear();
    a.attach(own, 4);                          // the owned block itself: stays owned
    CHECK(TestMem::ops().empty() && a.data() == own && TestMem::live == 1);
    a.attach(borrowed, 3);                     // the caller's memory: the owned block goes, once
    CHECK(TestMem::ops() == "r" && TestMem::log[0].p == own && a.data() == borrowed && a.count() == 3 && TestMem::live == 0);
    a.attach(borrowed, 3);
    CHECK(TestMem::ops() == "r");
    // upload over upload: the first block is released only after the second is in place
    CHECK(a.upload(host, 4) == 0);
    const float* first = a.data();
    TestMem::log.clear();
    CHECK(a.upload(host2, 2) == 0);
    CHECK(TestMem::ops() == "acr" && TestMem::log[2].p == first && TestMem::log[0].p == a.data());
    CHECK(a.count() == 2 && a.data()[1] == 6.f && TestMem::live == 1);
    // a refused allocation, then a refused copy: pointer, count and owned block stay
    const float* kept = a.data();
    TestMem::log.clear();
    TestMem::limit = 4;
    CHECK(a.upload(host, 4) == TestMem::kRefused);
    CHECK(a.data() == kept && a.count() == 2 && kept[0] == 5.f && TestMem::ops() == "x" && TestMem::live == 1);
    TestMem::fresh();
    TestMem::fail_copy = true;
    CHECK(a.upload(host, 4) == TestMem::kCopyFailed);
    CHECK(a.data() == kept && a.count() == 2 && kept[1] == 6.f && TestMem::ops() == "ar" && TestMem::live == 1);
    CHECK(TestMem::log[0].p == TestMem::log[1].p && TestMem::log[0].p != kept);   // the new block went, not the owned one
    // the same on a borrowed array
    Arr b;
    b.attach(borrowed, 3);
    CHECK(b.upload(host, 4) == TestMem::kCopyFailed && b.data() == borrowed && b.count() == 3);
    TestMem::fresh();
    // adopt: a block filled elsewhere becomes the owned one; moves carry the ownership along
    nbc::Buffer<TestMem> block;
    CHECK(block.reserve(sizeof(host)) == 0);
    std::memcpy(block.get(), host, sizeof(host));
    void* pb = block.get();
    a.adopt(std::move(block), 4);
    CHECK(!block && a.data() == pb && a.count() == 4 && TestMem::ops() == "ar" && TestMem::log[1].p == kept);
    Arr m(std::move(a));
    CHECK(a.data() == nullptr && a.count() == 0 && m.data() == pb && TestMem::live == 1);
    b = std::move(m);
    CHECK(m.data() == nullptr && b.data() == pb && b.count() == 4 && b.data()[3] == 4.f && TestMem::live == 1);
  }
  CHECK(TestMem::live == 0);
}

}  // namespace

int main() {
  reserve_that_fits_allocates_nothing();
  margin_growth_releases_before_it_requests();
  margin_refused_falls_back_to_exact();
  refused_reserve_leaves_the_buffer_empty();
  moves_leave_the_source_empty();
  array_attach_and_upload();
  CHECK(TestMem::live == 0);
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("device_mem host test OK\n");
  return 0;
}
