// gmg_mem.hpp -- the owners of what the library gets from the HIP runtime: device memory, pinned host memory, events.
// Host code only.  Each is move-only and frees what it holds in its destructor; kernel argument structs take .get().
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

namespace gmg {

template <class H, hipError_t (*Free)(H)>
class Owner {
 public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h_(o.release()) {}
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) { reset(); h_ = o.release(); }
    return *this;
  }
  Owner(const Owner &) = delete;
  Owner &operator=(const Owner &) = delete;
  ~Owner() { reset(); }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  void reset() {
    if (h_) (void)Free(h_);
    h_ = nullptr;
  }
  H release() { H h = h_; h_ = nullptr; return h; }

 protected:
  H h_ = nullptr;
};

template <class T> hipError_t dev_free_as(T *p) { return hipFree((void *)p); }
template <class T> hipError_t host_free_as(T *p) { return hipHostFree((void *)p); }

// one hipMalloc allocation; alloc() frees what was held first (n elements, alloc_bytes() where the size is not a count of T)
template <class T>
struct DevPtr : Owner<T *, dev_free_as<T>> {
  hipError_t alloc_bytes(size_t bytes) { this->reset(); return hipMalloc((void **)&this->h_, bytes); }
  hipError_t alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
};

// one hipHostMalloc allocation (pinned, device-visible)
template <class T>
struct HostPtr : Owner<T *, host_free_as<T>> {
  hipError_t alloc(size_t n) { this->reset(); return hipHostMalloc((void **)&this->h_, n * sizeof(T), hipHostMallocDefault); }
};

struct Event : Owner<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&h_, flags); }
};

// allocate max(n, min_n) elements and copy n of them from the host on `stream` (no copy when n == 0)
template <class T>
hipError_t upload(DevPtr<T> &d, const T *src, size_t n, hipStream_t stream, size_t min_n = 1) {
  hipError_t e = d.alloc(std::max(n, min_n));
  if (e == hipSuccess && n) e = hipMemcpyAsync(d.get(), src, sizeof(T) * n, hipMemcpyHostToDevice, stream);
  return e;
}
template <class T>
hipError_t upload(DevPtr<T> &d, const std::vector<T> &v, hipStream_t stream, size_t min_n = 1) {
  return upload(d, v.data(), v.size(), stream, min_n);
}

}  // namespace gmg
