// pt_device_buffer.h -- the owner of one device allocation, shared by the C boundary (pt_capi_internal.h) and the wavefront pipeline's host
// side (pt_wavefront.h). Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace hrt {

// Owns one device allocation: move-only, freed on reset() and on destruction (hipFree waits for work in flight). Converts to the plain
// pointer, so kernels and copies take it as they took the raw field.
template <class T> class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~DeviceBuffer() { reset(); }
    void reset() { if (p_) { (void)hipFree(p_); p_ = nullptr; } }
    hipError_t alloc(size_t bytes)               // the old allocation goes first; empty after a failure
    {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
private:
    T* p_ = nullptr;
};

} // namespace hrt
