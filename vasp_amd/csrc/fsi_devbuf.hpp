// A device buffer that owns its memory (the context's arrays and those of the types it holds).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdlib>
#include <type_traits>

namespace fsi {

template <class T>
struct DevBuf {      // owns its device memory: freed with the buffer, never copied
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e != hipSuccess) return e;
    // Fresh device memory is whatever the previous owner left (another context of the same process included): every buffer
    // starts from zeros, so that no result can depend on it.  FSI_DEBUG_POISON=1 fills the floating-point buffers with NaN
    // bit patterns instead - a read before the first write then shows up in the first norm that is taken.
    static const bool poison = getenv("FSI_DEBUG_POISON") != nullptr;
    return hipMemset(p, (poison && std::is_floating_point<T>::value) ? 0xFF : 0, count * sizeof(T));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void swap(DevBuf& o) { T* op = o.p; const size_t on = o.n; o.p = p; o.n = n; p = op; n = on; }
};

}  // namespace fsi
