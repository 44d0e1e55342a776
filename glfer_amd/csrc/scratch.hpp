// scratch.hpp -- per-call device scratch: the allocator's interface (scratch.cpp) and the owner of one buffer.
// Only the HIP runtime's API header and standard headers: a plain host compile can use it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace glfer {

// Stream-ordered scratch on the current device: small requests from a pool of their own, middle ones
// from the default pool (release threshold raised), 16 MiB and more from blocks the library keeps
// (scratch.cpp: the stream-ordered pool costs milliseconds, and now and then seconds, per GB-sized
// request).  Always given back through scratch_free on the stream that used it -- by a Scratch<T>.
hipError_t scratch_malloc(void **p, size_t bytes, hipStream_t st);
void scratch_free(void *p, hipStream_t st);
// idle kept blocks of `dev` given back until at most keep_bytes stay / bytes kept now / the per-device cap
size_t scratch_trim(int dev, size_t keep_bytes);
size_t scratch_held(int dev);
void scratch_set_cap(size_t bytes);
bool scratch_keeping();                        // false with GLFER_SCRATCH_CACHE=0: the library keeps nothing between calls
size_t scratch_cap();                          // glfer_hip_scratch_limit / GLFER_SCRATCH_CAP_MB

// One scratch buffer of T and the stream it goes back on: when the owner leaves its scope, or at release().
template <class T>
class Scratch {
 public:
  explicit Scratch(hipStream_t st) : st_(st) {}
  Scratch(Scratch &&o) noexcept : p_(std::exchange(o.p_, nullptr)), st_(o.st_) {}
  Scratch &operator=(Scratch &&o) noexcept {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      st_ = o.st_;
    }
    return *this;
  }
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() { release(); }

  // `count` elements (a buffer held so far goes back first); null after a failure
  hipError_t take(size_t count) {
    release();
    const hipError_t e = scratch_malloc((void **)&p_, count * sizeof(T), st_);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  // take(count), then the host's elements copied in on the stream.  (pageable source: the runtime stages it before the call
  // returns, so `host` may be a local vector)  A failed copy keeps nothing.
  hipError_t upload(const T *host, size_t count) {
    hipError_t e = take(count);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(p_, host, count * sizeof(T), hipMemcpyHostToDevice, st_);
    if (e != hipSuccess) release();
    return e;
  }
  T *get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void release() {
    if (p_) scratch_free(p_, st_);
    p_ = nullptr;
  }

 private:
  T *p_ = nullptr;
  hipStream_t st_;
};

}  // namespace glfer
