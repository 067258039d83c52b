// Owning buffers of the host code: DevBuf<T> holds one hipMalloc allocation, PinBuf<T> one of pinned host memory
// (hipHostMalloc).  Move-only; the destructor frees.  No pools, no stream-ordered allocation, no reference counts:
// a caller that may have a launch in flight on the old allocation synchronises before it lets the buffer grow.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

namespace bartrt {

struct HipError {
  hipError_t e;
  const char *what;
};
#define HIPCHK(x)                                  \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) throw HipError{_e, #x};  \
  } while (0)

struct DevMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t release(void *p) { return hipFree(p); }
};
struct PinMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t release(void *p) { return hipHostFree(p); }
};

template <class T, class Mem>
class OwnedBuf {
  T *p_ = nullptr;
  size_t n_ = 0;   // elements allocated (at least one once there is an allocation)

 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  OwnedBuf &operator=(OwnedBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }  // (o frees the old one)
  ~OwnedBuf() { if (p_) (void)Mem::release(p_); }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t count() const { return n_; }
  void reset() { n_ = 0; if (T *p = std::exchange(p_, nullptr)) HIPCHK(Mem::release(p)); }
  // room for n elements (at least one); a buffer that has to grow is freed first: its contents are not kept
  void reserve(size_t n) {
    if (p_ && n <= n_) return;
    reset();
    n = std::max<size_t>(n, 1);
    HIPCHK(Mem::alloc(reinterpret_cast<void **>(&p_), n * sizeof(T)));
    n_ = n;
  }
  void upload(const T *h, size_t n) {   // device buffers only (pinned memory is written in place)
    static_assert(std::is_same<Mem, DevMem>::value, "upload: a device buffer");
    reserve(n);
    if (n) HIPCHK(hipMemcpy(p_, h, n * sizeof(T), hipMemcpyHostToDevice));
  }
  void upload(const std::vector<T> &v) { upload(v.data(), v.size()); }
};

template <class T> using DevBuf = OwnedBuf<T, DevMem>;
template <class T> using PinBuf = OwnedBuf<T, PinMem>;

}  // namespace bartrt
