// c_scratch_guard.cpp -- glfer::Scratch<T> (glfer_amd/csrc/scratch.hpp) walked without a GPU and without the HIP runtime: this
// program defines the three functions the header calls -- glfer::scratch_malloc, glfer::scratch_free, hipMemcpyAsync -- as fakes
// over malloc / free that log every allocation and every give-back (pointer, stream, order), and checks the owner's rules one by
// one.  Built by tests/test_scratch_guard_host.py, plain and under the address and undefined-behaviour sanitizers.
#include "scratch.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace {
struct Event {
  void *p;
  hipStream_t st;
  bool freed;          // false: handed out
};
std::vector<Event> g_log;
std::vector<void *> g_live;
std::vector<void *> g_dead;   // given back; freed when main ends, so that no address comes twice and the log can be read by pointer
int g_fail_malloc = 0;   // the next so many scratch_malloc calls fail
int g_fail_copy = 0;     // the next so many hipMemcpyAsync calls fail
int g_copies = 0;
int g_failures = 0;

void check(bool ok, const char *what, int line) {
  if (ok) return;
  fprintf(stderr, "line %d: %s\n", line, what);
  g_failures++;
}
#define CHECK(x) check((x), #x, __LINE__)

hipStream_t stream(int k) { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(0x1000 + 16 * k)); }
size_t frees() {
  size_t n = 0;
  for (const Event &e : g_log) n += e.freed;
  return n;
}
// the give-backs of `p`: how many, and (by reference) the stream of the last one
size_t frees_of(void *p, hipStream_t *st = nullptr) {
  size_t n = 0;
  for (const Event &e : g_log)
    if (e.freed && e.p == p) {
      n++;
      if (st) *st = e.st;
    }
  return n;
}
}  // namespace

namespace glfer {
hipError_t scratch_malloc(void **p, size_t bytes, hipStream_t st) {
  if (g_fail_malloc > 0) {
    g_fail_malloc--;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  g_log.push_back(Event{*p, st, false});
  g_live.push_back(*p);
  return hipSuccess;
}
void scratch_free(void *p, hipStream_t st) {
  if (!p) return;
  g_log.push_back(Event{p, st, true});
  bool was_live = false;
  for (size_t i = 0; i < g_live.size(); i++)
    if (g_live[i] == p) {
      g_live.erase(g_live.begin() + (long)i);
      was_live = true;
      break;
    }
  check(was_live, "a buffer given back that is not out", __LINE__);
  if (was_live) g_dead.push_back(p);
}
}  // namespace glfer

extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  g_copies++;
  if (g_fail_copy > 0) {
    g_fail_copy--;
    return hipErrorInvalidValue;
  }
  check(kind == hipMemcpyHostToDevice, "upload copies host to device", __LINE__);
  memcpy(dst, src, bytes);
  return hipSuccess;
}

using glfer::Scratch;

// an early return between two takes: the first buffer goes back, the second is never taken
static int early_return(void **first) {
  Scratch<float> a(stream(1)), b(stream(2));
  if (a.take(8) != hipSuccess) return -1;
  *first = a.get();
  if (*first) return 1;
  (void)b.take(8);
  return 0;
}

int main() {
  {  // normal scope exit: once, on the guard's stream
    void *p = nullptr;
    {
      Scratch<double> g(stream(3));
      CHECK(!g && g.get() == nullptr);
      CHECK(g.take(5) == hipSuccess);
      CHECK(g && g.get() != nullptr);
      p = g.get();
      g.get()[4] = 1.0;                        // (5 doubles, not 5 bytes: the sanitizer sees the size)
      CHECK(frees() == 0);
    }
    hipStream_t st = nullptr;
    CHECK(frees_of(p, &st) == 1 && st == stream(3));
    CHECK(g_live.empty());
  }
  {  // early return between two takes
    const size_t before = g_log.size();
    void *p = nullptr;
    CHECK(early_return(&p) == 1);
    CHECK(g_log.size() == before + 2);         // one taken, one given back: the second guard never held anything
    CHECK(g_log.back().freed && g_log.back().p == p && g_log.back().st == stream(1));
    CHECK(g_live.empty());
  }
  {  // a failed take: empty, nothing freed
    const size_t before = g_log.size();
    {
      Scratch<int> g(stream(4));
      g_fail_malloc = 1;
      CHECK(g.take(3) == hipErrorOutOfMemory);
      CHECK(!g && g.get() == nullptr);
    }
    CHECK(g_log.size() == before);
  }
  {  // upload: the elements arrive; a failed copy gives the buffer back at once and leaves the guard empty
    const int host[3] = {7, 8, 9};
    const size_t before = g_log.size();
    Scratch<int> g(stream(5));
    CHECK(g.upload(host, 3) == hipSuccess);
    CHECK(g && g.get()[0] == 7 && g.get()[2] == 9);
    void *first = g.get();
    g_fail_copy = 1;
    CHECK(g.upload(host, 3) == hipErrorInvalidValue);
    CHECK(!g && g.get() == nullptr);
    // taken, (second upload:) first given back, taken, given back at once
    CHECK(g_log.size() == before + 4);
    CHECK(g_log[before + 1].freed && g_log[before + 1].p == first);
    CHECK(g_log[before + 3].freed && g_log[before + 3].p == g_log[before + 2].p && g_log[before + 3].st == stream(5));
    CHECK(g_live.empty());
    g_fail_malloc = 1;                          // a failed take inside upload: no copy is tried
    const int copies = g_copies;
    CHECK(g.upload(host, 3) == hipErrorOutOfMemory && !g && g_copies == copies);
  }
  {  // release() twice frees once; the destructor then frees nothing
    void *p = nullptr;
    {
      Scratch<char> g(stream(6));
      CHECK(g.take(100) == hipSuccess);
      p = g.get();
      g.release();
      CHECK(!g);
      g.release();
    }
    CHECK(frees_of(p) == 1);
  }
  {  // a second take gives the first buffer back first
    Scratch<float> g(stream(7));
    CHECK(g.take(4) == hipSuccess);
    void *first = g.get();
    const size_t before = g_log.size();
    CHECK(g.take(6) == hipSuccess);
    CHECK(g_log.size() == before + 2 && g_log[before].freed && g_log[before].p == first && !g_log[before + 1].freed);
    CHECK(frees_of(first) == 1);
  }
  {  // a moved-from guard frees nothing; the buffer goes back once, from its new owner, on its stream
    void *p = nullptr;
    {
      Scratch<float> a(stream(8));
      CHECK(a.take(4) == hipSuccess);
      p = a.get();
      Scratch<float> b(std::move(a));
      CHECK(!a && b.get() == p);
      Scratch<float> c(stream(9));
      CHECK(c.take(2) == hipSuccess);
      void *old = c.get();
      c = std::move(b);                         // (the buffer c held goes back on c's stream before it takes b's)
      hipStream_t st = nullptr;
      CHECK(frees_of(old, &st) == 1 && st == stream(9));
      CHECK(!b && c.get() == p && frees_of(p) == 0);
    }
    hipStream_t st = nullptr;
    CHECK(frees_of(p, &st) == 1 && st == stream(8));
  }
  {  // two guards in one scope go back in reverse order of declaration
    void *pa = nullptr, *pb = nullptr;
    const size_t before = g_log.size();
    {
      Scratch<float> a(stream(10));
      Scratch<double> b(stream(11));
      CHECK(a.take(1) == hipSuccess && b.take(1) == hipSuccess);
      pa = a.get();
      pb = b.get();
    }
    CHECK(g_log.size() == before + 4);
    CHECK(g_log[before + 2].freed && g_log[before + 2].p == pb && g_log[before + 2].st == stream(11));
    CHECK(g_log[before + 3].freed && g_log[before + 3].p == pa && g_log[before + 3].st == stream(10));
  }
  static_assert(!std::is_copy_constructible<Scratch<float>>::value && !std::is_copy_assignable<Scratch<float>>::value, "move-only");
  CHECK(g_live.empty());                        // nothing is out at exit (and the leak check of the sanitizer build agrees)
  size_t out = 0, back = 0;
  for (const Event &e : g_log) (e.freed ? back : out)++;
  CHECK(out == back);
  for (void *p : g_dead) free(p);
  printf("events %zu failures %d\n", g_log.size(), g_failures);
  return g_failures ? 1 : 0;
}
