// c_device_table.cpp -- glfer::DeviceTable<T> (glfer_amd/csrc/device_table.hpp) walked without a GPU and without the HIP runtime:
// this program defines the three functions the header calls -- hipMalloc, hipMemcpy, hipFree -- as fakes over malloc / free that
// log every allocation and every free and can be told to fail, and checks the owner's rules one by one.  Built by
// tests/test_device_table_host.py, plain and under the address and undefined-behaviour sanitizers.
#include "device_table.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace {
std::vector<void *> g_made, g_freed;   // in order; a freed block is kept until main ends, so that no address comes twice
std::vector<void *> g_live;
int g_fail_malloc = 0;   // the next so many hipMalloc calls fail
int g_fail_copy = 0;     // the next so many hipMemcpy calls fail
int g_copies = 0;
int g_failures = 0;

void check(bool ok, const char *what, int line) {
  if (ok) return;
  fprintf(stderr, "line %d: %s\n", line, what);
  g_failures++;
}
#define CHECK(x) check((x), #x, __LINE__)

size_t frees_of(void *p) {
  size_t n = 0;
  for (void *q : g_freed) n += q == p;
  return n;
}
}  // namespace

extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
  if (g_fail_malloc > 0) {
    g_fail_malloc--;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  g_made.push_back(*p);
  g_live.push_back(*p);
  return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  g_copies++;
  if (g_fail_copy > 0) {
    g_fail_copy--;
    return hipErrorInvalidValue;
  }
  check(kind == hipMemcpyHostToDevice, "upload copies host to device", __LINE__);
  memcpy(dst, src, bytes);
  return hipSuccess;
}
extern "C" hipError_t hipFree(void *p) {
  if (!p) return hipSuccess;
  g_freed.push_back(p);
  bool was_live = false;
  for (size_t i = 0; i < g_live.size(); i++)
    if (g_live[i] == p) {
      g_live.erase(g_live.begin() + (long)i);
      was_live = true;
      break;
    }
  check(was_live, "a table freed that is not out", __LINE__);
  return hipSuccess;
}

using glfer::DeviceTable;

// what a plan is to its tables: several owners of several types, destroyed together
struct Holder {
  DeviceTable<float> a, b;
  DeviceTable<uint16_t> c;
  DeviceTable<double> never;   // (a table this plan does not have)
};

int main() {
  {  // upload: the elements arrive; the destructor frees once
    void *p = nullptr;
    {
      DeviceTable<double> t;
      CHECK(!t && t.get() == nullptr);
      CHECK(t.upload(std::vector<double>{1.0, 2.0, 3.0, 4.0, 5.0}) == hipSuccess);
      CHECK(t && t.get()[0] == 1.0 && t.get()[4] == 5.0);      // (5 doubles, not 5 bytes: the sanitizer sees the size)
      CHECK(t.as<unsigned char>() == reinterpret_cast<unsigned char *>(t.get()));
      p = t.get();
      CHECK(g_freed.empty());
    }
    CHECK(frees_of(p) == 1 && g_live.empty());
  }
  {  // every table of a holder is freed exactly once; an empty one frees nothing
    const size_t made = g_made.size(), freed = g_freed.size();
    void *pa, *pb, *pc;
    {
      Holder h;
      CHECK(h.a.upload(std::vector<float>(7, 1.0f)) == hipSuccess && h.b.upload(std::vector<float>(2, 2.0f)) == hipSuccess);
      CHECK(h.c.upload(std::vector<uint16_t>(9, 3)) == hipSuccess);
      pa = h.a.get(), pb = h.b.get(), pc = h.c.get();
      CHECK(h.c.get()[8] == 3 && !h.never);
    }
    CHECK(g_made.size() == made + 3 && g_freed.size() == freed + 3);
    CHECK(frees_of(pa) == 1 && frees_of(pb) == 1 && frees_of(pc) == 1 && g_live.empty());
  }
  {  // a failed allocation: empty, no copy tried, nothing freed
    const size_t freed = g_freed.size();
    const int copies = g_copies;
    {
      DeviceTable<int> t;
      g_fail_malloc = 1;
      CHECK(t.upload(std::vector<int>(3, 1)) == hipErrorOutOfMemory);
      CHECK(!t && t.get() == nullptr && g_copies == copies);
    }
    CHECK(g_freed.size() == freed);
  }
  {  // a failed copy leaves the owner empty and frees the block at once, once
    const size_t made = g_made.size();
    {
      DeviceTable<int> t;
      g_fail_copy = 1;
      CHECK(t.upload(std::vector<int>(3, 1)) == hipErrorInvalidValue);
      CHECK(!t && t.get() == nullptr);
      CHECK(g_made.size() == made + 1 && frees_of(g_made.back()) == 1 && g_live.empty());
    }
    CHECK(frees_of(g_made.back()) == 1);
  }
  {  // a second upload frees the first table first; a failed second upload leaves the owner empty
    DeviceTable<float> t;
    CHECK(t.upload(std::vector<float>(4, 1.0f)) == hipSuccess);
    void *first = t.get();
    CHECK(t.upload(std::vector<float>(6, 2.0f)) == hipSuccess);
    CHECK(frees_of(first) == 1 && t.get() != first && t.get()[5] == 2.0f);
    void *second = t.get();
    g_fail_malloc = 1;
    CHECK(t.upload(std::vector<float>(6, 2.0f)) == hipErrorOutOfMemory && !t && frees_of(second) == 1);
  }
  {  // a move leaves the source empty; the table is freed once, by its new owner
    void *p = nullptr, *old = nullptr;
    {
      DeviceTable<float> a;
      CHECK(a.upload(std::vector<float>(4, 1.0f)) == hipSuccess);
      p = a.get();
      DeviceTable<float> b(std::move(a));
      CHECK(!a && a.get() == nullptr && b.get() == p);
      DeviceTable<float> c;
      CHECK(c.upload(std::vector<float>(2, 1.0f)) == hipSuccess);
      old = c.get();
      c = std::move(b);                         // (the table c held is freed before it takes b's)
      CHECK(frees_of(old) == 1 && !b && c.get() == p && frees_of(p) == 0);
      c = std::move(a);                         // (an empty source: c frees its table and is empty)
      CHECK(frees_of(p) == 1 && !c);
    }
    CHECK(frees_of(p) == 1 && frees_of(old) == 1);
  }
  static_assert(!std::is_copy_constructible<DeviceTable<float>>::value && !std::is_copy_assignable<DeviceTable<float>>::value, "move-only");
  static_assert(std::is_nothrow_move_constructible<DeviceTable<float>>::value, "a holder of tables can be moved");
  CHECK(g_live.empty());                        // nothing is out at exit (and the leak check of the sanitizer build agrees)
  CHECK(g_made.size() == g_freed.size());
  for (void *p : g_made) CHECK(frees_of(p) == 1);
  for (void *p : g_freed) free(p);
  printf("tables %zu failures %d\n", g_made.size(), g_failures);
  return g_failures ? 1 : 0;
}
