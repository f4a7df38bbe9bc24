// pt_device_buffer.h -- the owner of one device allocation, shared by the C boundary (pt_capi_internal.h) and the wavefront pipeline's host
// side (pt_wavefront.h). Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace hrt {

// Owns one device allocation and knows its size: move-only, freed on reset() and on destruction (hipFree waits for work in flight). Converts
// to the plain pointer, so kernels and copies take it as they took the raw field.
template <class T> class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
    ~DeviceBuffer() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; bytes_ = 0; }
    hipError_t alloc(size_t bytes)               // the old allocation goes first; empty after a failure
    {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), bytes);
        if (e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
        return e;
    }
    hipError_t reserve(size_t bytes) { return bytes <= bytes_ ? hipSuccess : alloc(bytes); }     // room for at least `bytes`; what it held is not kept
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t bytes() const { return bytes_; }      // of the allocation held; 0 when empty
private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

} // namespace hrt
