// device_table.hpp -- the owner of a table that lives as long as its plan: made once by a synchronous hipMalloc + hipMemcpy on
// the current device (not from the scratch pool: glfer_hip_scratch_held does not count it), freed by the destructor.
// Only the HIP runtime's API header and standard headers: a plain host compile can use it (tests/c_device_table.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace glfer {

template <class T>
class DeviceTable {
 public:
  DeviceTable() = default;
  DeviceTable(DeviceTable &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DeviceTable &operator=(DeviceTable &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  DeviceTable(const DeviceTable &) = delete;
  DeviceTable &operator=(const DeviceTable &) = delete;
  ~DeviceTable() { reset(); }

  // the host's elements on the device (a table held so far is freed first); empty after a failure
  hipError_t upload(const std::vector<T> &host) {
    reset();
    const size_t bytes = host.size() * sizeof(T);
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return e;
    }
    p_ = static_cast<T *>(d);
    return hipSuccess;
  }
  T *get() const { return p_; }
  template <class U>
  U *as() const { return reinterpret_cast<U *>(p_); }   // the table read as its kernel does (float pairs as float2)
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  T *p_ = nullptr;
};

}  // namespace glfer
